// Dynamically quantized int8 3x3 convolution (stride 1, padding 1) on
// v_mfma_i32_16x16x64_i8: the body of the dynamic models with body="int8"
// (DESIGN §24).  Input and output are fp32 in HBM; every image is quantized
// with the qparams of its own min/max while its band is staged into LDS, the
// products and sums are exact int32, nothing is calibrated.
//
// Numerics, per image n (include/qconvnet.h states the same contract):
//   (s_x, z_x) = choose_qparams(min x_n, max x_n, reduce_range)     (dynq.hpp)
//   q          = quantize_legacy(x, 1 / s_x, z_x)                    u8
//   acc[p][c]  = sum_{tap, ci} (q - z_x) * wq[c][ci][tap]            int32, padding = 0
//   t = fmaf((float)acc, s_x * s_w[c], bias[c]); t = fmaf(t, alpha[c], beta[c]);
//   t = max(t, 0); max over the 2x2 window              (each step after the first optional)
// The MFMA multiplies signed bytes, so LDS holds q ^ 0x80 = q - 128 and the
// epilogue subtracts (z_x - 128) * wsum[c]; positions outside the image and
// channels past Cin are staged as the code z_x and so contribute exactly 0.
// Integer sums are exact in any order: an image's bits cannot depend on its
// batch.  The image index enters base pointers and the stats row only.
//
// Shape of the work.  Implicit GEMM per image: A = pixels (MFMA rows), B =
// output channels (MFMA columns).  A pixel tile is 16 pixels = 4 pool windows
// side by side, 2 rows x 8 columns: A row 4 q + e is window q, position
// (e >> 1, e & 1).  In the 16x16 accumulator lane (c = l % 16, g = l / 16)
// holds rows 4 g + r of column c: its four registers are the 2x2 window g of
// channel c, so the pool is a register max.  A wave owns 4 pixel tiles stacked
// down (8 x 8 pixels) x 4 channel tiles (64 channels): 64 int32 accumulators,
// 16 MFMAs per K step for 4 LDS and 4 weight fragments.  The 4 waves of a
// workgroup are WPX pixel groups across x WCH channel groups; a block covers
// 8 rows x 8 WPX columns x 64 WCH channels.
//
// K.  The K unit is 16 channels of one tap (one 16-byte fragment).  Units run
// tap-major, channel-group-minor inside a chunk of up to 256 channels; MFMA
// step s takes units 4 s .. 4 s + 3, lane group g unit 4 s + g, so every Cin
// that is a multiple of 16 wastes at most 3 units per chunk (conv1: 9 units
// of 3 real channels each).  Units past the chunk's 9 * ncg have zero weights.
//
// LDS: the block's band with a one-pixel halo, [row][column][channel] bytes,
// every channel of the chunk resident (10 x 34 x 64 B for conv2).  Pixel
// stride PS and row stride RS come from cd_pixel_stride / cd_row_stride: for
// Cin chunks of 64 / 128 / 192 / 256 channels every ds_read_b128 of the loop is
// conflict-free in the model of tools/lds_banks.py (tools/lds_banks_dyn.py
// prints the cycles of every chunk size; the others are 2 to 4 times that).
//
// Range hand-off: every block reduces min / max of the outputs it stores
// (registers, wave shuffles, LDS) and writes them to its own slot
// y_stats[n][slot]; the next layer's blocks reduce the image's slots at their
// start.  No atomics, no zeroing launch; every slot is written by every call.
#include "common.hpp"
#include "conv_dyn.hpp"
#include "dynq.hpp"
#include "qconvnet_abi.hpp"

namespace qcn {

struct ConvDynArgs {
  const float* x;
  const float* x_stats;   // [nimg][x_slots][2]
  const v4i* wp;
  const int* wsum;
  const float* w_scale;
  const float* bias;
  const float* alpha;
  const float* beta;
  float* y;
  float* y_stats;         // [nimg][nbc * nby * nbx][2] or null
  float* x_qparams;       // [nimg][2] (scale, zero point bits) or null
  int h, w, cin, cout;
  int x_slots, reduce_range, per_channel;
  int x_nchw, x_vec, relu, pool, y_nchw;
  int nbx, nby, nbc;      // blocks across, down, channel blocks (per image)
  int ncg;                // 16-channel groups: ceil(cin / 16)
  int n64;                // 64-channel groups: ceil(cout / 64)
  int steps;              // cd_steps(cin)
  int ps, rs;             // LDS strides (bytes)
};

template <int WPX, int WCH>
__global__ __launch_bounds__(256) void conv3x3_dyn_kernel(const ConvDynArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t band[];
  __shared__ float red[2][4];
  constexpr int LROWS = CD_ROWS + 2, LCOLS = 8 * WPX + 2;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c16 = lane & 15, g = lane >> 4;
  const int wpx = wave % WPX, wch = wave / WPX;

  // block -> (image, channel block, band row, band column); the image index
  // is used for the base pointers and stats rows below and nowhere else
  int b = blockIdx.x;
  const int bx = b % a.nbx; b /= a.nbx;
  const int by = b % a.nby; b /= a.nby;
  const int bc = b % a.nbc;
  const int img = b / a.nbc;
  const int slots = a.nbc * a.nby * a.nbx, slot = (bc * a.nby + by) * a.nbx + bx;
  const int row0 = by * CD_ROWS, col0 = bx * 8 * WPX;
  const float* ximg = a.x + (size_t)img * a.h * a.w * a.cin;
  float* yimg = a.y + (size_t)img * (a.pool ? (a.h / 2) * (a.w / 2) : a.h * a.w) * a.cout;

  // the image's qparams from its producer's range slots (block-uniform)
  float xlo = __builtin_inff(), xhi = -__builtin_inff();
  {
    const float* st = a.x_stats + (size_t)img * a.x_slots * 2;
    for (int s = 0; s < a.x_slots; ++s) {
      xlo = fminf(xlo, st[2 * s]);
      xhi = fmaxf(xhi, st[2 * s + 1]);
    }
  }
  const float4 qp = choose_qparams(xlo, xhi, a.reduce_range);
  const float s_x = qp.x, inv = qp.y, zpf = qp.z;
  const int z_x = __float_as_int(qp.w);
  if (a.x_qparams && slot == 0 && tid == 0) {
    a.x_qparams[2 * (size_t)img] = s_x;
    a.x_qparams[2 * (size_t)img + 1] = qp.w;
  }
  const uint32_t zcode = splat_u8(z_x) ^ 0x80808080u;

  // this lane's A pixel (LDS byte offset of tap (0, 0)) in pixel tile 0; tile
  // pt is 2 pt rows further down
  const int q = c16 >> 2, e = c16 & 3;
  const int abase = (e >> 1) * a.rs + (8 * wpx + 2 * q + (e & 1)) * a.ps;
  // weight streams of the wave's four 16-channel tiles (clamped: a wave past
  // the packed tiles recomputes the last group and stores nothing)
  const int g64 = bc * WCH + wch;
  const int g64c = g64 < a.n64 ? g64 : a.n64 - 1;
  const v4i* wq = a.wp + (size_t)g64c * 4 * a.steps * 64 + lane;
  const size_t wtile = (size_t)a.steps * 64;

  v4i acc[4][4];
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[p][c] = (v4i){0, 0, 0, 0};

  int gs = 0;
  v4i bn[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) bn[c] = wq[c * wtile];
  const int nchunk = (a.ncg + 15) / 16;
  for (int ch = 0; ch < nchunk; ++ch) {
    const int ncgc = a.ncg - 16 * ch < 16 ? a.ncg - 16 * ch : 16;   // channel groups of this chunk
    const int units = 4 * ncgc;                                     // dwords per pixel
    __syncthreads();   // the previous chunk's reads are done
    for (int idx = tid; idx < LROWS * LCOLS * units; idx += 256) {
      const int pix = idx / units, u = idx - pix * units;
      const int pr = pix / LCOLS, pc = pix - pr * LCOLS;
      const int gr = row0 - 1 + pr, gcol = col0 - 1 + pc;
      const int c0 = ch * CD_CK + 4 * u;
      uint32_t code = zcode;
      if (gr >= 0 && gr < a.h && gcol >= 0 && gcol < a.w && c0 < a.cin) {
        float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        const int nv = a.cin - c0 < 4 ? a.cin - c0 : 4;
        if (a.x_vec) {          // NHWC, cin % 4 == 0, 16-byte aligned
          const float4 f = *reinterpret_cast<const float4*>(ximg + ((size_t)gr * a.w + gcol) * a.cin + c0);
          v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (k < nv)
              v[k] = a.x_nchw ? ximg[((size_t)(c0 + k) * a.h + gr) * a.w + gcol]
                              : ximg[((size_t)gr * a.w + gcol) * a.cin + c0 + k];
        }
        uint32_t qv = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k)
          qv |= (k < nv ? quantize_legacy(v[k], inv, zpf) : (uint32_t)z_x) << (8 * k);
        code = qv ^ 0x80808080u;
      }
      *reinterpret_cast<uint32_t*>(band + pr * a.rs + pc * a.ps + 4 * u) = code;
    }
    __syncthreads();

    // lane group g walks units g, g + 4, ...: (tap, cg) of unit u is
    // (u / ncgc, u % ncgc); a unit past the chunk reads unit 0 (zero weights)
    const int steps = (9 * ncgc + 3) / 4;
    int tap = 0, cg = g;
#pragma unroll
    for (int k = 0; k < 3; ++k)
      if (cg >= ncgc) { cg -= ncgc; ++tap; }
    v4i an[4];
    {
      const int off = abase + (tap / 3) * a.rs + (tap % 3) * a.ps + 16 * cg;
#pragma unroll
      for (int p = 0; p < 4; ++p) an[p] = *reinterpret_cast<const v4i*>(band + off + 2 * p * a.rs);
    }
    for (int t = 0; t < steps; ++t) {
      v4i av[4], bv[4];
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
          if (cg >= ncgc) { cg -= ncgc; ++tap; }
        const int off = abase + (tap < 9 ? (tap / 3) * a.rs + (tap % 3) * a.ps + 16 * cg : 0);
#pragma unroll
        for (int p = 0; p < 4; ++p) an[p] = *reinterpret_cast<const v4i*>(band + off + 2 * p * a.rs);
      }
#pragma unroll
      for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int c = 0; c < 4; ++c)
          acc[p][c] = __builtin_amdgcn_mfma_i32_16x16x64_i8(av[p], bv[c], acc[p][c], 0, 0, 0);
    }
  }

  // epilogue: register r of this lane is window g, position r, of channel c16
  const int oh = a.pool ? a.h / 2 : a.h, ow = a.pool ? a.w / 2 : a.w;
  const int zc = z_x - 128;
  float ylo = __builtin_inff(), yhi = -__builtin_inff();
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int co = (g64 * 4 + c) * 16 + c16;
    if (co >= a.cout) continue;
    const int corr = zc * a.wsum[co];
    const float sc = s_x * (a.per_channel ? a.w_scale[co] : a.w_scale[0]);
    const float bi = a.bias ? a.bias[co] : 0.0f;
    const float al = a.alpha ? a.alpha[co] : 1.0f;
    const float be = a.alpha ? a.beta[co] : 0.0f;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int r = row0 + 2 * p, cc = col0 + 8 * wpx + 2 * g;
      float v[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float tv = __builtin_fmaf((float)(acc[p][c][k] - corr), sc, bi);
        if (a.alpha) tv = __builtin_fmaf(tv, al, be);
        if (a.relu) tv = fmaxf(tv, 0.0f);
        v[k] = tv;
      }
      if (a.pool) {
        if (r < a.h && cc < a.w) {
          const float m = fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3]));
          const int orow = r >> 1, ocol = cc >> 1;
          const size_t o = a.y_nchw ? ((size_t)co * oh + orow) * ow + ocol
                                    : ((size_t)orow * ow + ocol) * a.cout + co;
          yimg[o] = m;
          ylo = fminf(ylo, m);
          yhi = fmaxf(yhi, m);
        }
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int orow = r + (k >> 1), ocol = cc + (k & 1);
          if (orow < a.h && ocol < a.w) {
            const size_t o = a.y_nchw ? ((size_t)co * oh + orow) * ow + ocol
                                      : ((size_t)orow * ow + ocol) * a.cout + co;
            yimg[o] = v[k];
            ylo = fminf(ylo, v[k]);
            yhi = fmaxf(yhi, v[k]);
          }
        }
      }
    }
  }

  // the block's output range -> its own slot (masked lanes hold +-inf)
  if (a.y_stats) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      ylo = fminf(ylo, __shfl_xor(ylo, d));
      yhi = fmaxf(yhi, __shfl_xor(yhi, d));
    }
    if (lane == 0) { red[0][wave] = ylo; red[1][wave] = yhi; }
    __syncthreads();
    if (tid == 0) {
      float* st = a.y_stats + ((size_t)img * slots + slot) * 2;
      st[0] = fminf(fminf(red[0][0], red[0][1]), fminf(red[0][2], red[0][3]));
      st[1] = fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3]));
    }
  }
}

// min / max of each image's count contiguous floats -> stats[n][0] (one slot)
template <bool VEC>
__global__ __launch_bounds__(256) void image_minmax_kernel(const float* __restrict__ x, int count,
                                                           float* __restrict__ stats) {
  __shared__ float red[2][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* xi = x + (size_t)blockIdx.x * count;
  float lo = __builtin_inff(), hi = -__builtin_inff();
  if constexpr (VEC) {
    const float4* x4 = reinterpret_cast<const float4*>(xi);
    for (int i = tid; i < count / 4; i += 256) {
      const float4 v = x4[i];
      lo = fminf(lo, fminf(fminf(v.x, v.y), fminf(v.z, v.w)));
      hi = fmaxf(hi, fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)));
    }
  } else {
    for (int i = tid; i < count; i += 256) {
      lo = fminf(lo, xi[i]);
      hi = fmaxf(hi, xi[i]);
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, d));
    hi = fmaxf(hi, __shfl_xor(hi, d));
  }
  if (lane == 0) { red[0][wave] = lo; red[1][wave] = hi; }
  __syncthreads();
  if (tid == 0) {
    stats[2 * (size_t)blockIdx.x] = fminf(fminf(red[0][0], red[0][1]), fminf(red[0][2], red[0][3]));
    stats[2 * (size_t)blockIdx.x + 1] = fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3]));
  }
}

// (waves across, channel groups) of a layer: a function of (w, cout) only
static void cd_config(int w, int cout, int* wpx, int* wch) {
  *wpx = cout <= 64 ? 4 : cout <= 128 ? 2 : 1;
  if (w <= 8) *wpx = 1;
  else if (w <= 16 && *wpx > 2) *wpx = 2;
  *wch = 4 / *wpx;
}

template <int WPX, int WCH>
static int launch_conv_dyn(ConvDynArgs a, int nimg, hipStream_t stream) {
  a.nbx = (a.w + 8 * WPX - 1) / (8 * WPX);
  a.nby = (a.h + CD_ROWS - 1) / CD_ROWS;
  a.nbc = (a.n64 + WCH - 1) / WCH;
  const long blocks = (long)nimg * a.nbc * a.nby * a.nbx;
  if (blocks > 0x7fffffffL) return QCN_ERR_UNSUPPORTED;
  const int ncg0 = a.ncg < 16 ? a.ncg : 16;
  a.ps = cd_pixel_stride(ncg0);
  a.rs = cd_row_stride(ncg0, 8 * WPX + 2);
  constexpr int max_lds = (CD_ROWS + 2) * cd_row_stride(16, 8 * WPX + 2);
  static bool lds_set[QCN_MAX_DEV] = {};
  auto kernel = conv3x3_dyn_kernel<WPX, WCH>;
  if (!qcn_set_lds_once(reinterpret_cast<const void*>(kernel), max_lds, lds_set)) return QCN_ERR_HIP;
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), (CD_ROWS + 2) * a.rs, stream, a);
  return hipGetLastError() == hipSuccess ? QCN_OK : QCN_ERR_HIP;
}

}  // namespace qcn

extern "C" {

int qcn_conv3x3_dyn_packed_size(int cin, int cout) {
  if (cin < 1 || cout < 1) return QCN_ERR_ARG;
  if (cin > qcn::CD_MAX_CIN) return QCN_ERR_UNSUPPORTED;
  const long n = 4L * ((cout + 63L) / 64) * qcn::cd_steps(cin) * 1024;
  return n > 0x7fffffffL ? QCN_ERR_UNSUPPORTED : (int)n;
}

// out[((ct * steps + step) * 64 + lane) * 16 + b] = w[16 ct + lane % 16][ci][tap] with
// unit u = 4 * (step - 36 * chunk) + lane / 16 of chunk = step / 36, ncgc the
// chunk's channel groups, tap = u / ncgc, ci = 256 chunk + 16 (u % ncgc) + b;
// 0 for a unit past 9 ncgc, a channel past cin or a column past cout.
int qcn_pack_conv3x3_weight_dyn(const int8_t* w_oihw, int cout, int cin, int8_t* out, int32_t* wsum) {
  if (!w_oihw || !out || !wsum) return QCN_ERR_ARG;
  const int size = qcn_conv3x3_dyn_packed_size(cin, cout);
  if (size < 0) return size;
  const int ncg = (cin + 15) / 16, steps = qcn::cd_steps(cin), nct = 4 * ((cout + 63) / 64);
  for (int ct = 0; ct < nct; ++ct)
    for (int step = 0; step < steps; ++step) {
      const int chunk = step / 36;
      const int ncgc = ncg - 16 * chunk < 16 ? ncg - 16 * chunk : 16;
      int8_t* o = out + ((long)ct * steps + step) * 1024;
      for (int lane = 0; lane < 64; ++lane) {
        const int u = 4 * (step - 36 * chunk) + lane / 16;
        const int tap = u / ncgc, co = 16 * ct + lane % 16;
        for (int b = 0; b < 16; ++b) {
          const int ci = 256 * chunk + 16 * (u % ncgc) + b;
          o[lane * 16 + b] = (tap < 9 && ci < cin && co < cout) ? w_oihw[((long)co * cin + ci) * 9 + tap] : 0;
        }
      }
    }
  for (int co = 0; co < cout; ++co) {
    int s = 0;
    for (long i = 0; i < 9L * cin; ++i) s += w_oihw[(long)co * cin * 9 + i];
    wsum[co] = s;
  }
  return QCN_OK;
}

int qcn_conv3x3_dyn_stats_slots(int h, int w, int cout) {
  if (h < 1 || w < 1 || cout < 1) return QCN_ERR_ARG;
  int wpx, wch;
  qcn::cd_config(w, cout, &wpx, &wch);
  const long n = (long)((cout + 63) / 64 + wch - 1) / wch * ((h + qcn::CD_ROWS - 1) / qcn::CD_ROWS) *
                 ((w + 8 * wpx - 1) / (8 * wpx));
  return n > 0x7fffffffL ? QCN_ERR_UNSUPPORTED : (int)n;
}

int qcn_image_minmax_f32(const float* x, int nimg, long long count, float* stats, void* stream) {
  if (!x || !stats || nimg < 1 || count < 1) return QCN_ERR_ARG;
  if (((uintptr_t)x & 3) || ((uintptr_t)stats & 3)) return QCN_ERR_ARG;
  if (count > 0x7fffffffLL) return QCN_ERR_UNSUPPORTED;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (count % 4 == 0 && ((uintptr_t)x & 15) == 0)
    hipLaunchKernelGGL(qcn::image_minmax_kernel<true>, dim3(nimg), dim3(256), 0, s, x, (int)count, stats);
  else
    hipLaunchKernelGGL(qcn::image_minmax_kernel<false>, dim3(nimg), dim3(256), 0, s, x, (int)count, stats);
  return hipGetLastError() == hipSuccess ? QCN_OK : QCN_ERR_HIP;
}

int qcn_conv3x3_dyn(const float* x, int nimg, int h, int w, int cin, int x_nchw, const float* x_stats,
                    int x_slots, int reduce_range, const int8_t* w_packed, const int32_t* wsum,
                    const float* w_scale, int per_channel, int cout, const float* bias,
                    const float* alpha, const float* beta, int relu, int pool, int y_nchw, float* y,
                    float* y_stats, float* x_qparams, void* stream) {
  using namespace qcn;
  if (!x || !x_stats || !w_packed || !wsum || !w_scale || !y) return QCN_ERR_ARG;
  if (nimg < 1 || h < 1 || w < 1 || cin < 1 || cout < 1 || x_slots < 1) return QCN_ERR_ARG;
  if ((alpha == nullptr) != (beta == nullptr)) return QCN_ERR_ARG;
  if (pool && ((h | w) & 1)) return QCN_ERR_ARG;
  if (((uintptr_t)w_packed & 15) || (((uintptr_t)x | (uintptr_t)y | (uintptr_t)x_stats | (uintptr_t)y_stats |
                                      (uintptr_t)x_qparams | (uintptr_t)wsum | (uintptr_t)w_scale) & 3))
    return QCN_ERR_ARG;
  if (qcn_conv3x3_dyn_packed_size(cin, cout) < 0) return QCN_ERR_UNSUPPORTED;
  const long px = (long)nimg * h * w;
  if (px * cin > 0x7fffffffL || px * cout > 0x7fffffffL) return QCN_ERR_UNSUPPORTED;

  ConvDynArgs a = {};
  a.x = x; a.x_stats = x_stats; a.wp = reinterpret_cast<const v4i*>(w_packed); a.wsum = wsum;
  a.w_scale = w_scale; a.bias = bias; a.alpha = alpha; a.beta = beta;
  a.y = y; a.y_stats = y_stats; a.x_qparams = x_qparams;
  a.h = h; a.w = w; a.cin = cin; a.cout = cout;
  a.x_slots = x_slots; a.reduce_range = reduce_range != 0; a.per_channel = per_channel != 0;
  a.x_nchw = x_nchw != 0;
  a.x_vec = !x_nchw && cin % 4 == 0 && ((uintptr_t)x & 15) == 0;
  a.relu = relu != 0; a.pool = pool != 0; a.y_nchw = y_nchw != 0;
  a.ncg = (cin + 15) / 16;
  a.n64 = (cout + 63) / 64;
  a.steps = cd_steps(cin);
  hipStream_t s = static_cast<hipStream_t>(stream);
  int wpx, wch;
  cd_config(w, cout, &wpx, &wch);
  if (wpx == 4) return launch_conv_dyn<4, 1>(a, nimg, s);
  if (wpx == 2) return launch_conv_dyn<2, 2>(a, nimg, s);
  return launch_conv_dyn<1, 4>(a, nimg, s);
}

}  // extern "C"
