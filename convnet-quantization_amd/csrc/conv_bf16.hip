// bf16 3x3 convolution (stride 1, padding 1) on v_mfma_f32_16x16x32_bf16 with
// fp32 accumulation: the body of the dynamic models with body="bf16" (DESIGN
// §28).  Input and output are fp32 or bf16 in HBM; nothing is calibrated and
// no range is recorded.
//
// Numerics (include/qconvnet.h states the same contract):
//   xb  = bf16_rne(x)                    identity when x is bf16 already
//   acc = sum over taps and ci of xb * wb   fp32 from +0, padding contributes +0
//   t = acc + bias[c]; t = fmaf(t, alpha[c], beta[c]); t = max(t, 0);
//   max over the 2x2 window              (each step optional), all in fp32
//   y   = t, or bf16_rne(t) when y is bf16
// A product of two bf16 values is exact in fp32; the sums run in one order
// fixed here: Cin chunks ascending, inside a chunk 32 K values per MFMA step
// in the unit order below, one accumulator chain per output.  The image index
// enters base pointers only, so an image's bits cannot depend on its batch.
// Rounding to bf16 is monotone, so it commutes with ReLU and the pool: a bf16
// y is bf16_rne of the fp32 y, and the next layer, which rounds what it stages,
// computes the same bits from either.
//
// Shape of the work: conv_dyn.hip's.  Implicit GEMM per image, A = pixels,
// B = output channels.  A pixel tile is 16 pixels = 4 pool windows side by
// side (2 rows x 8 columns), A row 4 q + e is window q, position (e >> 1,
// e & 1); accumulator lane (n = l % 16, g = l / 16) holds window g of column
// n in its four registers, so the pool is a register max.  A wave owns 4 pixel
// tiles stacked down (8 x 8 pixels) x 4 column tiles: 64 fp32 accumulators, 16
// MFMAs per K step for 4 ds_read_b128 and 4 16-byte weight loads.  The 4 waves
// of a workgroup are WPX pixel groups across x WCH channel groups.
//
// Columns.  Column n of tile ct is output channel 32 (ct / 2) + 2 n + ct % 2:
// a lane's tiles 2 j and 2 j + 1 are the adjacent channels 32 j + 2 n and
// 32 j + 2 n + 1, which one v_cvt_pk_bf16_f32 packs into one 4-byte store.
//
// K.  The unit is 8 channels of one tap (one 16-byte fragment); MFMA step s
// takes units 4 s .. 4 s + 3, lane group g unit 4 s + g.  Units run tap-major,
// channel-group-minor inside a chunk of G 8-channel groups, G = 8, 16, 32 for
// cout <= 64, <= 128, more (cb_chunk_groups): the widest block a layer of that
// cout can get is 32, 16, 8 pixels across, so every band stays near 54 KB.
// Units past the chunk's 9 * ngc have zero weights.
//
// LDS: the block's band with a one-pixel halo, [row][column][channel] bf16,
// converted (or, from a bf16 x, copied as 16-byte pieces) while it is staged;
// pixels outside the image and channels past Cin are +0.  In 16-byte units the
// band is conv_dyn.hip's, so the strides are cd_pixel_stride / cd_row_stride:
// chunks of 8, 16 and 32 groups (Cin 64, 128, 256) read conflict-free in the
// model of tools/lds_banks.py (tools/lds_banks_dyn.py with ncg = groups).
#include <string.h>

#include "common.hpp"
#include "conv_dyn.hpp"
#include "qconvnet_abi.hpp"

typedef __bf16 v8bf __attribute__((ext_vector_type(8)));
typedef __bf16 v2bf __attribute__((ext_vector_type(2)));
typedef float v4f __attribute__((ext_vector_type(4)));

namespace qcn {

// 8-channel groups per LDS chunk and MFMA steps of all chunks of a layer
__host__ __device__ constexpr int cb_chunk_groups(int cout) { return cout <= 64 ? 8 : cout <= 128 ? 16 : 32; }
__host__ __device__ constexpr long cb_steps(int cin, int cout) {
  const long ng = (cin + 7L) / 8, G = cb_chunk_groups(cout);
  return (ng / G) * (9 * G / 4) + (9 * (ng % G) + 3) / 4;
}

struct ConvBf16Args {
  const void* x;
  const v8bf* wp;
  const float* bias;
  const float* alpha;
  const float* beta;
  void* y;
  int h, w, cin, cout;
  int x_fmt, x_vec, relu, pool, y_fmt, y_vec;
  int nbx, nby, nbc;   // blocks across, down, channel blocks (per image)
  int ng, G;           // 8-channel groups: of the layer, of a full chunk
  int n64;             // 64-channel groups: ceil(cout / 64)
  int steps;           // cb_steps(cin, cout)
  int ps, rs;          // LDS strides (bytes)
};

// two fp32 -> two bf16 (RNE), the first in the low half
QCN_DEV uint32_t pack_bf16(float lo, float hi) {
  return __builtin_bit_cast(uint32_t, __builtin_convertvector((v2f){lo, hi}, v2bf));
}

template <int WPX, int WCH>
__global__ __launch_bounds__(256) void conv3x3_bf16_kernel(const ConvBf16Args a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t band[];
  constexpr int LROWS = CD_ROWS + 2, LCOLS = 8 * WPX + 2;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c16 = lane & 15, g = lane >> 4;
  const int wpx = wave % WPX, wch = wave / WPX;

  // block -> (image, channel block, band row, band column); the image index
  // is used for the two base offsets below and nowhere else
  int b = blockIdx.x;
  const int bx = b % a.nbx; b /= a.nbx;
  const int by = b % a.nby; b /= a.nby;
  const int bc = b % a.nbc;
  const int img = b / a.nbc;
  const int row0 = by * CD_ROWS, col0 = bx * 8 * WPX;
  const size_t xoff = (size_t)img * a.h * a.w * a.cin;
  const size_t yoff = (size_t)img * (a.pool ? (a.h / 2) * (a.w / 2) : a.h * a.w) * a.cout;
  const float* xf = static_cast<const float*>(a.x) + xoff;
  const uint16_t* xh = static_cast<const uint16_t*>(a.x) + xoff;

  // this lane's A pixel (LDS byte offset of tap (0, 0)) in pixel tile 0; tile
  // pt is 2 pt rows further down
  const int q = c16 >> 2, e = c16 & 3;
  const int abase = (e >> 1) * a.rs + (8 * wpx + 2 * q + (e & 1)) * a.ps;
  // weight streams of the wave's four column tiles (clamped: a wave past the
  // packed tiles recomputes the last group and stores nothing)
  const int g64 = bc * WCH + wch;
  const int g64c = g64 < a.n64 ? g64 : a.n64 - 1;
  const v8bf* wq = a.wp + (size_t)g64c * 4 * a.steps * 64 + lane;
  const size_t wtile = (size_t)a.steps * 64;

  v4f acc[4][4];
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[p][c] = (v4f){0.0f, 0.0f, 0.0f, 0.0f};

  int gs = 0;
  v8bf bn[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) bn[c] = wq[c * wtile];
  const int nchunk = (a.ng + a.G - 1) / a.G;
  for (int ch = 0; ch < nchunk; ++ch) {
    const int ngc = a.ng - a.G * ch < a.G ? a.ng - a.G * ch : a.G;   // channel groups of this chunk
    const int cbase = ch * a.G * 8;
    __syncthreads();   // the previous chunk's reads are done
    if (a.x_fmt == QCN_FMT_BF16_NHWC && a.x_vec) {
      // cin % 8 == 0, 16-byte aligned: one group is one 16-byte piece
      int pix = tid / ngc, u = tid - pix * ngc;
      const int dpix = 256 / ngc, du = 256 - dpix * ngc;
      while (pix < LROWS * LCOLS) {
        const int pr = pix / LCOLS, pc = pix - pr * LCOLS;
        const int gr = row0 - 1 + pr, gcol = col0 - 1 + pc;
        uint4 v = {0u, 0u, 0u, 0u};
        if (gr >= 0 && gr < a.h && gcol >= 0 && gcol < a.w)
          v = *reinterpret_cast<const uint4*>(xh + ((size_t)gr * a.w + gcol) * a.cin + cbase + 8 * u);
        *reinterpret_cast<uint4*>(band + pr * a.rs + pc * a.ps + 16 * u) = v;
        u += du; pix += dpix;
        if (u >= ngc) { u -= ngc; ++pix; }
      }
    } else {
      // one item is 4 channels of a pixel: 8 bytes of LDS
      const int quads = 2 * ngc;
      int pix = tid / quads, u = tid - pix * quads;
      const int dpix = 256 / quads, du = 256 - dpix * quads;
      while (pix < LROWS * LCOLS) {
        const int pr = pix / LCOLS, pc = pix - pr * LCOLS;
        const int gr = row0 - 1 + pr, gcol = col0 - 1 + pc;
        const int c0 = cbase + 4 * u;
        uint2 code = {0u, 0u};
        if (gr >= 0 && gr < a.h && gcol >= 0 && gcol < a.w && c0 < a.cin) {
          const int nv = a.cin - c0 < 4 ? a.cin - c0 : 4;
          const size_t pixel = (size_t)gr * a.w + gcol;
          if (a.x_fmt == QCN_FMT_BF16_NHWC) {
            uint32_t hv[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int k = 0; k < 4; ++k)
              if (k < nv) hv[k] = xh[pixel * a.cin + c0 + k];
            code.x = hv[0] | (hv[1] << 16);
            code.y = hv[2] | (hv[3] << 16);
          } else {
            float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (a.x_vec) {        // NHWC, cin % 4 == 0, 16-byte aligned
              const float4 f = *reinterpret_cast<const float4*>(xf + pixel * a.cin + c0);
              v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
            } else {
#pragma unroll
              for (int k = 0; k < 4; ++k)
                if (k < nv)
                  v[k] = a.x_fmt == QCN_FMT_F32_NCHW ? xf[((size_t)(c0 + k) * a.h + gr) * a.w + gcol]
                                                     : xf[pixel * a.cin + c0 + k];
            }
            code.x = pack_bf16(v[0], v[1]);
            code.y = pack_bf16(v[2], v[3]);
          }
        }
        *reinterpret_cast<uint2*>(band + pr * a.rs + pc * a.ps + 8 * u) = code;
        u += du; pix += dpix;
        if (u >= quads) { u -= quads; ++pix; }
      }
    }
    __syncthreads();

    // lane group g walks units g, g + 4, ...: (tap, cg) of unit u is
    // (u / ngc, u % ngc); a unit past the chunk reads unit 0 (zero weights)
    const int steps = (9 * ngc + 3) / 4;
    int tap = 0, cg = g;
#pragma unroll
    for (int k = 0; k < 3; ++k)
      if (cg >= ngc) { cg -= ngc; ++tap; }
    v8bf an[4];
    {
      const int off = abase + (tap / 3) * a.rs + (tap % 3) * a.ps + 16 * cg;
#pragma unroll
      for (int p = 0; p < 4; ++p) an[p] = *reinterpret_cast<const v8bf*>(band + off + 2 * p * a.rs);
    }
    for (int t = 0; t < steps; ++t) {
      v8bf av[4], bv[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) { av[k] = an[k]; bv[k] = bn[k]; }
      ++gs;
      if (gs < a.steps) {   // next step's weights (runs on across chunk boundaries)
#pragma unroll
        for (int c = 0; c < 4; ++c) bn[c] = wq[c * wtile + (size_t)gs * 64];
      }
      if (t + 1 < steps) {
        cg += 4;
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (cg >= ngc) { cg -= ngc; ++tap; }
        const int off = abase + (tap < 9 ? (tap / 3) * a.rs + (tap % 3) * a.ps + 16 * cg : 0);
#pragma unroll
        for (int p = 0; p < 4; ++p) an[p] = *reinterpret_cast<const v8bf*>(band + off + 2 * p * a.rs);
      }
#pragma unroll
      for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int c = 0; c < 4; ++c)
          acc[p][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[p], bv[c], acc[p][c], 0, 0, 0);
    }
  }

  // epilogue: register r of tile c is window g, position r, of channel
  // 64 g64 + 32 (c / 2) + 2 c16 + c % 2; a lane stores channel pairs
  const int oh = a.pool ? a.h / 2 : a.h, ow = a.pool ? a.w / 2 : a.w;
  float* yf = static_cast<float*>(a.y) + yoff;
  uint16_t* yh = static_cast<uint16_t*>(a.y) + yoff;
  const int cc = col0 + 8 * wpx + 2 * g;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int co = 64 * g64 + 32 * j + 2 * c16;
    if (co >= a.cout) continue;
    const bool two = co + 1 < a.cout;
    float bi[2], al[2], be[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int ck = two ? co + k : co;
      bi[k] = a.bias ? a.bias[ck] : 0.0f;
      al[k] = a.alpha ? a.alpha[ck] : 1.0f;
      be[k] = a.alpha ? a.beta[ck] : 0.0f;
    }
    auto store = [&](int orow, int ocol, float v0, float v1) {
      if (a.y_fmt == QCN_FMT_BF16_NHWC) {
        const size_t o = ((size_t)orow * ow + ocol) * a.cout + co;
        const uint32_t pk = pack_bf16(v0, v1);
        if (a.y_vec) {
          *reinterpret_cast<uint32_t*>(yh + o) = pk;
        } else {
          yh[o] = (uint16_t)pk;
          if (two) yh[o + 1] = (uint16_t)(pk >> 16);
        }
      } else if (a.y_fmt == QCN_FMT_F32_NCHW) {
        const size_t o = ((size_t)co * oh + orow) * ow + ocol;
        yf[o] = v0;
        if (two) yf[o + (size_t)oh * ow] = v1;
      } else {
        const size_t o = ((size_t)orow * ow + ocol) * a.cout + co;
        if (a.y_vec) {
          *reinterpret_cast<float2*>(yf + o) = make_float2(v0, v1);
        } else {
          yf[o] = v0;
          if (two) yf[o + 1] = v1;
        }
      }
    };
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int r = row0 + 2 * p;
      float v[2][4];
#pragma unroll
      for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float tv = acc[p][2 * j + k][i];
          if (a.bias) tv = tv + bi[k];
          if (a.alpha) tv = __builtin_fmaf(tv, al[k], be[k]);
          if (a.relu) tv = fmaxf(tv, 0.0f);
          v[k][i] = tv;
        }
      if (a.pool) {
        if (r < a.h && cc < a.w)
          store(r >> 1, cc >> 1, fmaxf(fmaxf(v[0][0], v[0][1]), fmaxf(v[0][2], v[0][3])),
                fmaxf(fmaxf(v[1][0], v[1][1]), fmaxf(v[1][2], v[1][3])));
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int orow = r + (i >> 1), ocol = cc + (i & 1);
          if (orow < a.h && ocol < a.w) store(orow, ocol, v[0][i], v[1][i]);
        }
      }
    }
  }
}

// (waves across, channel groups) of a layer: a function of (w, cout) only
static void cb_config(int w, int cout, int* wpx, int* wch) {
  *wpx = cout <= 64 ? 4 : cout <= 128 ? 2 : 1;
  if (w <= 8) *wpx = 1;
  else if (w <= 16 && *wpx > 2) *wpx = 2;
  *wch = 4 / *wpx;
}

template <int WPX, int WCH>
static int launch_conv_bf16(ConvBf16Args a, int nimg, hipStream_t stream) {
  a.nbx = (a.w + 8 * WPX - 1) / (8 * WPX);
  a.nby = (a.h + CD_ROWS - 1) / CD_ROWS;
  a.nbc = (a.n64 + WCH - 1) / WCH;
  const long blocks = (long)nimg * a.nbc * a.nby * a.nbx;
  if (blocks > 0x7fffffffL) return QCN_ERR_UNSUPPORTED;
  const int ng0 = a.ng < a.G ? a.ng : a.G;
  a.ps = cd_pixel_stride(ng0);
  a.rs = cd_row_stride(ng0, 8 * WPX + 2);
  // WPX pixel groups only go with cout <= 256 / WPX, i.e. chunks of G <= 32 / WPX groups
  constexpr int max_lds = (CD_ROWS + 2) * cd_row_stride(32 / WPX, 8 * WPX + 2);
  const int lds = (CD_ROWS + 2) * a.rs;
  if (lds > max_lds) return QCN_ERR_UNSUPPORTED;
  static bool lds_set[QCN_MAX_DEV] = {};
  auto kernel = conv3x3_bf16_kernel<WPX, WCH>;
  if (!qcn_set_lds_once(reinterpret_cast<const void*>(kernel), max_lds, lds_set)) return QCN_ERR_HIP;
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), lds, stream, a);
  return hipGetLastError() == hipSuccess ? QCN_OK : QCN_ERR_HIP;
}

// fp32 -> bf16 bits, round to nearest even (finite values)
static uint16_t bf16_rne(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

}  // namespace qcn

extern "C" {

int qcn_conv3x3_bf16_packed_size(int cin, int cout) {
  if (cin < 1 || cout < 1) return QCN_ERR_ARG;
  const long n = 4L * ((cout + 63L) / 64) * qcn::cb_steps(cin, cout) * 1024;
  return n > 0x7fffffffL ? QCN_ERR_UNSUPPORTED : (int)n;
}

// out[((ct * steps + step) * 64 + lane) * 8 + b] = bf16_rne(w[co][ci][tap]) with
// co = 32 (ct / 2) + 2 (lane % 16) + ct % 2; chunk = step / (9 G / 4), unit
// u = 4 (step - chunk * 9 G / 4) + lane / 16, ngc the chunk's channel groups,
// tap = u / ngc, ci = 8 G chunk + 8 (u % ngc) + b; +0 for a unit past 9 ngc, a
// channel past cin or a column past cout.
int qcn_pack_conv3x3_weight_bf16(const float* w_oihw, int cout, int cin, uint16_t* out) {
  if (!w_oihw || !out) return QCN_ERR_ARG;
  const int size = qcn_conv3x3_bf16_packed_size(cin, cout);
  if (size < 0) return size;
  const int ng = (cin + 7) / 8, G = qcn::cb_chunk_groups(cout), full = 9 * G / 4;
  const int steps = (int)qcn::cb_steps(cin, cout), nct = 4 * ((cout + 63) / 64);
  for (int ct = 0; ct < nct; ++ct)
    for (int step = 0; step < steps; ++step) {
      const int chunk = step / full;
      const int ngc = ng - G * chunk < G ? ng - G * chunk : G;
      uint16_t* o = out + ((long)ct * steps + step) * 512;
      for (int lane = 0; lane < 64; ++lane) {
        const int u = 4 * (step - full * chunk) + lane / 16;
        const int tap = u / ngc, co = 32 * (ct / 2) + 2 * (lane % 16) + ct % 2;
        for (int b = 0; b < 8; ++b) {
          const int ci = 8 * G * chunk + 8 * (u % ngc) + b;
          o[lane * 8 + b] = (tap < 9 && ci < cin && co < cout)
                                ? qcn::bf16_rne(w_oihw[((long)co * cin + ci) * 9 + tap]) : 0;
        }
      }
    }
  return QCN_OK;
}

int qcn_conv3x3_bf16(const void* x, int nimg, int h, int w, int cin, int x_fmt, const uint16_t* w_packed,
                     int cout, const float* bias, const float* alpha, const float* beta, int relu, int pool,
                     int y_fmt, void* y, void* stream) {
  using namespace qcn;
  if (!x || !w_packed || !y || nimg < 1 || h < 1 || w < 1 || cin < 1 || cout < 1) return QCN_ERR_ARG;
  if (x_fmt < QCN_FMT_F32_NHWC || x_fmt > QCN_FMT_BF16_NHWC || y_fmt < QCN_FMT_F32_NHWC ||
      y_fmt > QCN_FMT_BF16_NHWC)
    return QCN_ERR_ARG;
  if ((alpha == nullptr) != (beta == nullptr)) return QCN_ERR_ARG;
  if (pool && ((h | w) & 1)) return QCN_ERR_ARG;
  // a bf16 tensor is read in 16-byte and written in 4-byte pieces where its
  // channel count allows (cin % 8 == 0, cout % 2 == 0)
  const uintptr_t xmask = x_fmt != QCN_FMT_BF16_NHWC ? 3 : cin % 8 == 0 ? 15 : 1;
  const uintptr_t ymask = y_fmt != QCN_FMT_BF16_NHWC || cout % 2 == 0 ? 3 : 1;
  if (((uintptr_t)w_packed & 15) || ((uintptr_t)x & xmask) || ((uintptr_t)y & ymask)) return QCN_ERR_ARG;
  if (qcn_conv3x3_bf16_packed_size(cin, cout) < 0) return QCN_ERR_UNSUPPORTED;
  const long px = (long)nimg * h * w;
  if (px * cin > 0x7fffffffL || px * cout > 0x7fffffffL) return QCN_ERR_UNSUPPORTED;

  ConvBf16Args a = {};
  a.x = x; a.wp = reinterpret_cast<const v8bf*>(w_packed);
  a.bias = bias; a.alpha = alpha; a.beta = beta; a.y = y;
  a.h = h; a.w = w; a.cin = cin; a.cout = cout;
  a.x_fmt = x_fmt; a.y_fmt = y_fmt;
  a.x_vec = x_fmt == QCN_FMT_BF16_NHWC ? cin % 8 == 0
                                       : x_fmt == QCN_FMT_F32_NHWC && cin % 4 == 0 && ((uintptr_t)x & 15) == 0;
  a.y_vec = cout % 2 == 0 && (y_fmt == QCN_FMT_BF16_NHWC ||
                              (y_fmt == QCN_FMT_F32_NHWC && ((uintptr_t)y & 7) == 0));
  a.relu = relu != 0; a.pool = pool != 0;
  a.ng = (cin + 7) / 8;
  a.G = cb_chunk_groups(cout);
  a.n64 = (cout + 63) / 64;
  a.steps = (int)cb_steps(cin, cout);
  hipStream_t s = static_cast<hipStream_t>(stream);
  int wpx, wch;
  cb_config(w, cout, &wpx, &wch);
  if (wpx == 4) return launch_conv_bf16<4, 1>(a, nimg, s);
  if (wpx == 2) return launch_conv_bf16<2, 2>(a, nimg, s);
  return launch_conv_bf16<1, 4>(a, nimg, s);
}

}  // extern "C"
