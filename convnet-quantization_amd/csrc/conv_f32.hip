// Deterministic fp32 3x3 convolution (stride 1, padding 1) on the fp32 matrix
// instruction v_mfma_f32_32x32x2_f32: the body of the dynamic models with
// body="hip" (DESIGN §23).  Products and sums are true fp32; there is no
// narrowing, no split-K, no atomics and no cross-wave reduction.
//
// Contract (what makes an image's result independent of its batch):
//  * the image index appears in the block index and in addresses only; tile
//    shape, K order and the instantiation depend on (h, w, cin, cout) alone;
//  * every output element is one accumulator chain that starts at +0 and runs
//    over K in one fixed order: Cin chunks of 64 channels ascending, inside a
//    chunk tap-major (ky, kx), channel-minor, two channels per instruction;
//  * the epilogue, in fp32 and in this order: t = acc + bias[c];
//    t = fmaf(t, alpha[c], beta[c]); t = max(t, 0); max over the 2x2 window
//    (each step optional).  The file is built with -ffp-contract=off.
// NaN, inf and denormal inputs are outside the contract (max() and the zero
// padding of K are only order-free on finite normal values).
//
// Shape of the work.  Implicit GEMM per image: A = pixels (MFMA rows), B =
// output channels (MFMA columns), K = 9 * Cin.  A pixel tile is 32 pixels = 8
// pool windows: lane pixel i = 4 q + e is window q, position (e >> 1, e & 1),
// and the windows lie WQ across: 2 rows x 16 columns (WQ = 8) or 4 rows x 8
// columns (WQ = 4, images up to 8 wide).  In the accumulator, register
// 4 g + e of lane (hi, c) is pixel 8 g + 4 hi + e of channel c: the four
// registers e = 0..3 are one 2x2 window, so the pool is a register max.
// A wave owns 2 pixel tiles x 2 channel tiles (64 x 64 outputs, 64 fp32
// accumulators per lane); the 4 waves of a workgroup are WPX pixel groups x
// WCH channel groups.
//
// LDS: the block's input band with a one-pixel halo, one Cin chunk at a time,
// [row][column][channel] with a pixel stride of PS = 68 dwords and a row
// stride RS = 32 (mod 64) dwords.  Inside each group of 8 channels the order
// is 0 2 4 6 1 3 5 7, so lane half `hi` reads the A values of four consecutive
// K steps (channels hi, 2 + hi, 4 + hi, 6 + hi) with one ds_read_b128.
// Out-of-image pixels and channels past Cin are staged as +0: the K loop has
// no bounds test.
//
// Weights: packed on the host (qcn_pack_conv3x3_weight_f32) into the lane
// order of the B operand, in the kernel's K order, so a wave's weight stream
// is one sequential run of 16-byte loads, fetched one 4-instruction step
// (16 MFMAs) ahead of use.
#include "common.hpp"
#include "qconvnet_abi.hpp"

typedef float v16f __attribute__((ext_vector_type(16)));

namespace qcn {

constexpr int CF_CK = 64;   // channels per LDS chunk
constexpr int CF_PS = 68;   // LDS dwords per pixel (64 + 4: consecutive pixels shift 4 banks)

// LDS row stride in dwords: the row of pixels, padded to 32 (mod 64)
__host__ __device__ constexpr int cf_row_stride(int lcols) {
  const int rs = lcols * CF_PS;
  return rs + ((32 - rs % 64) + 64) % 64;
}

struct ConvF32Args {
  const float* x;
  const float4* wp;
  const float* bias;
  const float* alpha;
  const float* beta;
  float* y;
  int h, w, cin, cout;
  int x_nchw, x_vec, relu, pool, y_nchw;
  int tcols;          // pixel tiles across a block (1 or 2)
  int nbx, nby, nbc;  // blocks across, down, channel blocks (per image)
  int ng;             // K groups of 8 channels: ceil(cin / 8)
  int nct;            // packed 32-channel tiles: 2 * ceil(cout / 64)
};

template <int WPX, int WCH, int WQ>
__global__ __launch_bounds__(256) void conv3x3_f32_kernel(const ConvF32Args a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int TH = 16 / WQ, TW = 2 * WQ;   // pixel tile: TH rows x TW columns
  constexpr int NT = 2 * WPX;                // pixel tiles of the block
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l32 = lane & 31, hi = lane >> 5;
  const int wpx = wave % WPX, wch = wave / WPX;

  // block -> (image, channel block, band row, band column); the image index is
  // used for the two base pointers below and nowhere else
  int b = blockIdx.x;
  const int bx = b % a.nbx; b /= a.nbx;
  const int by = b % a.nby; b /= a.nby;
  const int bc = b % a.nbc;
  const int img = b / a.nbc;
  const int tcols = a.tcols, trows = NT / tcols;
  const int row0 = by * trows * TH, col0 = bx * tcols * TW;
  const int lrows = trows * TH + 2, lcols = tcols * TW + 2;
  const int RS = cf_row_stride(lcols);
  const float* ximg = a.x + (size_t)img * a.h * a.w * a.cin;
  float* yimg = a.y + (size_t)img * (a.pool ? (a.h / 2) * (a.w / 2) : a.h * a.w) * a.cout;

  // this lane's A pixel in each of the wave's two tiles (LDS dword offset of
  // tap (0, 0), i.e. of the pixel one up and one left)
  const int q = l32 >> 2, e = l32 & 3;
  const int prow = 2 * (q / WQ) + (e >> 1), pcol = 2 * (q % WQ) + (e & 1);
  int aoff[2];
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int t = 2 * wpx + p;
    aoff[p] = ((t / tcols) * TH + prow) * RS + ((t % tcols) * TW + pcol) * CF_PS + 4 * hi;
  }
  // weight streams of the wave's two 32-channel tiles (clamped: a wave past
  // the packed tiles recomputes the last one and stores nothing)
  const int ct0 = (bc * WCH + wch) * 2;
  const float4* wq[2];
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int ct = ct0 + c < a.nct ? ct0 + c : a.nct - 1;
    wq[c] = a.wp + (size_t)ct * 9 * a.ng * 64 + lane;
  }

  v16f acc[2][2];
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[p][c][r] = 0.0f;

  const int total = 9 * a.ng;   // steps of 4 instructions (8 channels of one tap)
  int gs = 0;
  float4 bn[2] = {wq[0][0], wq[1][0]};
  const int nchunk = (a.ng + 7) / 8;
  for (int ch = 0; ch < nchunk; ++ch) {
    const int gc = a.ng - 8 * ch < 8 ? a.ng - 8 * ch : 8;   // channel groups of this chunk
    const int units = 2 * gc;                              // 4-channel units per pixel
    __syncthreads();   // the previous chunk's reads are done
    for (int pr = 0; pr < lrows; ++pr) {
      const int gr = row0 - 1 + pr;
      const bool row_ok = gr >= 0 && gr < a.h;
      for (int idx = tid; idx < lcols * units; idx += 256) {
        const int pc = idx / units, u = idx - pc * units;
        const int gcol = col0 - 1 + pc;
        const int c0 = ch * CF_CK + 4 * u;
        float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (row_ok && gcol >= 0 && gcol < a.w) {
          if (a.x_vec) {        // NHWC, cin % 4 == 0, 16-byte aligned: c0 + 3 < cin
            if (c0 < a.cin) {
              const float4 f = *reinterpret_cast<const float4*>(
                  ximg + ((size_t)gr * a.w + gcol) * a.cin + c0);
              v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
            }
          } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
              if (c0 + k < a.cin)
                v[k] = a.x_nchw ? ximg[((size_t)(c0 + k) * a.h + gr) * a.w + gcol]
                                : ximg[((size_t)gr * a.w + gcol) * a.cin + c0 + k];
          }
        }
        // channel 8 G + j -> slot 8 G + 4 (j & 1) + (j >> 1)
        float* dst = lds + pr * RS + pc * CF_PS + 8 * (u >> 1) + 2 * (u & 1);
        dst[0] = v[0]; dst[4] = v[1]; dst[1] = v[2]; dst[5] = v[3];
      }
    }
    __syncthreads();

    const int steps = 9 * gc;
    int tap = 0, g = 0;
    float4 an[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) an[p] = *reinterpret_cast<const float4*>(lds + aoff[p]);
    for (int t = 0; t < steps; ++t) {
      const float4 av[2] = {an[0], an[1]};
      const float4 bv[2] = {bn[0], bn[1]};
      ++gs;
      if (gs < total) {   // next step's weights (runs on across chunk boundaries)
        bn[0] = wq[0][(size_t)gs * 64];
        bn[1] = wq[1][(size_t)gs * 64];
      }
      if (t + 1 < steps) {
        if (++g == gc) { g = 0; ++tap; }
        const int toff = (tap / 3) * RS + (tap % 3) * CF_PS + 8 * g;
#pragma unroll
        for (int p = 0; p < 2; ++p) an[p] = *reinterpret_cast<const float4*>(lds + aoff[p] + toff);
      }
      const float as[2][4] = {{av[0].x, av[0].y, av[0].z, av[0].w}, {av[1].x, av[1].y, av[1].z, av[1].w}};
      const float bs[2][4] = {{bv[0].x, bv[0].y, bv[0].z, bv[0].w}, {bv[1].x, bv[1].y, bv[1].z, bv[1].w}};
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
          for (int c = 0; c < 2; ++c)
            acc[p][c] = __builtin_amdgcn_mfma_f32_32x32x2f32(as[p][s], bs[c][s], acc[p][c], 0, 0, 0);
    }
  }

  // epilogue: register 4 g + e of this lane is window 2 g + hi, position e
  const int oh = a.pool ? a.h / 2 : a.h, ow = a.pool ? a.w / 2 : a.w;
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int co = (ct0 + c) * 32 + l32;
    if (co >= a.cout) continue;
    const float bi = a.bias ? a.bias[co] : 0.0f;
    const float al = a.alpha ? a.alpha[co] : 1.0f;
    const float be = a.alpha ? a.beta[co] : 0.0f;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int t = 2 * wpx + p;
      const int tr0 = row0 + (t / tcols) * TH, tc0 = col0 + (t % tcols) * TW;
#pragma unroll
      for (int gq = 0; gq < 4; ++gq) {
        const int win = 2 * gq + hi;
        const int r = tr0 + 2 * (win / WQ), cc = tc0 + 2 * (win % WQ);
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          float tv = acc[p][c][4 * gq + k];
          if (a.bias) tv = tv + bi;
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
          }
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const int orow = r + (k >> 1), ocol = cc + (k & 1);
            if (orow < a.h && ocol < a.w) {
              const size_t o = a.y_nchw ? ((size_t)co * oh + orow) * ow + ocol
                                        : ((size_t)orow * ow + ocol) * a.cout + co;
              yimg[o] = v[k];
            }
          }
        }
      }
    }
  }
}

// LDS bytes of a block: (band rows + 2) x row stride
template <int WPX, int WQ>
constexpr int cf_lds_bytes(int tcols) {
  return ((2 * WPX / tcols) * (16 / WQ) + 2) * cf_row_stride(tcols * 2 * WQ + 2) * 4;
}

template <int WPX, int WCH, int WQ>
static int launch_conv_f32(ConvF32Args a, int nimg, hipStream_t stream) {
  constexpr int TH = 16 / WQ, TW = 2 * WQ, NT = 2 * WPX;
  a.tcols = a.w > TW ? 2 : 1;
  const int bh = (NT / a.tcols) * TH, bw = a.tcols * TW;
  a.nbx = (a.w + bw - 1) / bw;
  a.nby = (a.h + bh - 1) / bh;
  a.nbc = (a.cout + 64 * WCH - 1) / (64 * WCH);
  const long blocks = (long)nimg * a.nbc * a.nby * a.nbx;
  if (blocks > 0x7fffffffL) return QCN_ERR_UNSUPPORTED;
  constexpr int max_lds = cf_lds_bytes<WPX, WQ>(1) > cf_lds_bytes<WPX, WQ>(2) ? cf_lds_bytes<WPX, WQ>(1)
                                                                              : cf_lds_bytes<WPX, WQ>(2);
  static bool lds_set[QCN_MAX_DEV] = {};
  auto kernel = conv3x3_f32_kernel<WPX, WCH, WQ>;
  if (!qcn_set_lds_once(reinterpret_cast<const void*>(kernel), max_lds, lds_set)) return QCN_ERR_HIP;
  const int lds = a.tcols == 1 ? cf_lds_bytes<WPX, WQ>(1) : cf_lds_bytes<WPX, WQ>(2);
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), lds, stream, a);
  return hipGetLastError() == hipSuccess ? QCN_OK : QCN_ERR_HIP;
}

}  // namespace qcn

extern "C" {

int qcn_conv3x3_f32_packed_size(int cin, int cout) {
  if (cin < 1 || cout < 1) return QCN_ERR_ARG;
  const long n = 2L * ((cout + 63L) / 64) * 9 * ((cin + 7L) / 8) * 256;
  return n > 0x7fffffffL / 4 ? QCN_ERR_UNSUPPORTED : (int)n;
}

// out[(((ct * 9 * ng) + step) * 64 + lane) * 4 + s] = w[32 ct + lane % 32][8 G + 2 s + lane / 32][tap]
// with step = 72 * chunk + tap * gc + g, G = 8 * chunk + g, gc the chunk's
// channel groups (8, the last chunk ng - 8 * chunk); +0 past cin and past cout.
int qcn_pack_conv3x3_weight_f32(const float* w_oihw, int cout, int cin, float* out) {
  if (!w_oihw || !out) return QCN_ERR_ARG;
  const int size = qcn_conv3x3_f32_packed_size(cin, cout);
  if (size < 0) return size;
  const int ng = (cin + 7) / 8, nct = 2 * ((cout + 63) / 64);
  for (int ct = 0; ct < nct; ++ct)
    for (int G = 0; G < ng; ++G) {
      const int chunk = G / 8, g = G % 8;
      const int gc = ng - 8 * chunk < 8 ? ng - 8 * chunk : 8;
      for (int tap = 0; tap < 9; ++tap) {
        const long step = 72L * chunk + (long)tap * gc + g;
        float* o = out + (((long)ct * 9 * ng + step) * 64) * 4;
        for (int lane = 0; lane < 64; ++lane)
          for (int s = 0; s < 4; ++s) {
            const int co = 32 * ct + lane % 32, ci = 8 * G + 2 * s + lane / 32;
            o[lane * 4 + s] = (co < cout && ci < cin) ? w_oihw[((long)co * cin + ci) * 9 + tap] : 0.0f;
          }
      }
    }
  return QCN_OK;
}

int qcn_conv3x3_f32(const float* x, int nimg, int h, int w, int cin, int x_nchw, const float* w_packed,
                    int cout, const float* bias, const float* alpha, const float* beta, int relu,
                    int pool, int y_nchw, float* y, void* stream) {
  using namespace qcn;
  if (!x || !w_packed || !y || nimg < 1 || h < 1 || w < 1 || cin < 1 || cout < 1) return QCN_ERR_ARG;
  if ((alpha == nullptr) != (beta == nullptr)) return QCN_ERR_ARG;
  if (pool && ((h | w) & 1)) return QCN_ERR_ARG;
  if (((uintptr_t)w_packed & 15) || ((uintptr_t)x & 3) || ((uintptr_t)y & 3)) return QCN_ERR_ARG;
  if (qcn_conv3x3_f32_packed_size(cin, cout) < 0) return QCN_ERR_UNSUPPORTED;
  const long px = (long)nimg * h * w;
  if (px * cin > 0x7fffffffL || px * cout > 0x7fffffffL) return QCN_ERR_UNSUPPORTED;

  ConvF32Args a = {};
  a.x = x; a.wp = reinterpret_cast<const float4*>(w_packed);
  a.bias = bias; a.alpha = alpha; a.beta = beta; a.y = y;
  a.h = h; a.w = w; a.cin = cin; a.cout = cout;
  a.x_nchw = x_nchw != 0;
  a.x_vec = !x_nchw && cin % 4 == 0 && ((uintptr_t)x & 15) == 0;
  a.relu = relu != 0; a.pool = pool != 0; a.y_nchw = y_nchw != 0;
  a.ng = (cin + 7) / 8;
  a.nct = 2 * ((cout + 63) / 64);
  hipStream_t s = static_cast<hipStream_t>(stream);
  // the instantiation is a function of (w, cout) only: narrow images take the
  // 4 x 8 pixel tile, wide layers spend their waves on channels
  const bool narrow = w <= 8;
  if (cout <= 64) return narrow ? launch_conv_f32<4, 1, 4>(a, nimg, s) : launch_conv_f32<4, 1, 8>(a, nimg, s);
  if (cout <= 128) return narrow ? launch_conv_f32<2, 2, 4>(a, nimg, s) : launch_conv_f32<2, 2, 8>(a, nimg, s);
  return narrow ? launch_conv_f32<1, 4, 4>(a, nimg, s) : launch_conv_f32<1, 4, 8>(a, nimg, s);
}

}  // extern "C"
