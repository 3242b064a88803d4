// Two dynamically quantized int8 3x3 convolutions in one launch for maps up to
// 32 x 32 with up to 64 channels everywhere (conv1 + conv2): layer
// A (no pool) and layer B of conv_dyn.hip's contract, A's output handed to B as
// u8 codes in LDS.  conv_dyn_pair.hip gives every wave one 8 x 8 x 64 piece of
// the intermediate activation, so its 512 threads end at 16 x 16 x 128.  A
// 32 x 32 x 64 image is 16 such pieces: here every wave takes two, runs layer A
// for one after the other and keeps both results, 128 fp32 values per lane,
// in registers until the image's range is known.  Then the workgroup chooses
// the qparams, quantizes its registers into B's band and runs B from there.
// The intermediate never exists in HBM and never as fp32 outside registers.
//
// The bits are those of qcn_conv3x3_dyn (A, range recorded) followed by
// qcn_conv3x3_dyn (B): the same fp32 values meet the same choose_qparams and
// quantize_legacy.  min / max are order-independent but for the sign of a zero,
// which choose_qparams cannot tell apart.  The values that are
// quantized are the registers whose range was taken, so nothing is computed
// twice.  (The form that re-runs A's K loop for the hand-off instead of keeping
// its results was built, is bit-equal too and measured slower: DESIGN §26.)
//
// Work split.  One workgroup per image, 512 threads.  A wave's unit of work is
// conv_dyn.hip's 8 x 8 pixel group (4 pixel tiles of 2 x 8) x 64 channels, 64
// int32 accumulators.  The map is up to 4 x 4 pixel groups; wave (pgy, pgx),
// pgy < 2, pgx < 4, owns (pgy, pgx) and (pgy + 2, pgx) and runs them one after
// the other in every phase.  A group wholly past (h, w) is skipped: the skip is
// wave-uniform, a function of (h, w) only, and no barrier lies inside it.
//
// Phases of a block (barriers between them):
//   1  stage x (quantize on stage, whole image + halo) into the band
//   2  layer A per owned group: the K loop from the band, the epilogue into
//      registers (fp32), min / max of the valid (position, channel) values; B's
//      first weight fragments are requested after the last K loop
//   3  the image's range: xor shuffles, one LDS slot per wave; every thread
//      computes (s_m, z_m)
//   4  the mid band (it aliases the x band, which every wave has finished
//      reading) filled with the code z_m; then every lane quantizes its values,
//      transposes 4 x 4 bytes inside its lane quad (DPP quad_perm) and writes
//      dwords
//   5  B's K loop from the mid band (one chunk) per owned group, B's epilogue
//      (affine, ReLU, 2x2 register-max pool, NHWC / NCHW) and the image's
//      output range into its one y_stats slot
//
// Both bands are [row][column][channel] bytes in exactly the 34-column layout
// that conv3x3_dyn_kernel<4, 1> reads (cd_pixel_stride, cd_row_stride).
#include "common.hpp"
#include "conv_dyn.hpp"
#include "conv_dyn_pair.hpp"
#include "dynq.hpp"
#include "qconvnet_abi.hpp"

namespace qcn {

constexpr int P32_HW = 32, P32_CH = 64;      // largest map side and channel count served
constexpr int P32_NW = 8, P32_NT = 64 * P32_NW;
constexpr int P32_LCOLS = P32_HW + 2;        // band columns (and rows, at most)

// Layer A of the 8 x 8 pixel group at (row0, col0) from the staged band: the K
// loop, the epilogue into mid and the min / max of the valid values.  Register
// k of mid[c][p] is window g, position k, of channel c16 of channel tile c,
// pixel tile p.  bn holds A's step-0 weight fragments on entry and those of
// wnext's step 0 on exit.
QCN_DEV void pair32_layer_a(const ConvDynPairArgs& a, const uint8_t* band, int row0, int col0, int lane, int z_x,
                            float s_x, const v4i* wqa, size_t wtile_a, const v4i* wnext, size_t wtile_next,
                            v4i (&bn)[4], float (&mid)[4][4][4], float& mlo, float& mhi) {
  const int c16 = lane & 15, g = lane >> 4, q = c16 >> 2, e = c16 & 3;
  v4i acc[4][4];
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[p][c] = (v4i){0, 0, 0, 0};
  int gs = 0;
  cdp_chunk(band, (row0 + (e >> 1)) * a.rs + (col0 + 2 * q + (e & 1)) * a.ps, a.rs, a.ps, a.ncg, g, wqa, wtile_a,
            a.la.steps, gs, bn, acc);
  // the next K loop's first fragments: their latency lies under this epilogue
#pragma unroll
  for (int c = 0; c < 4; ++c) bn[c] = wnext[c * wtile_next];

  const int zc = z_x - 128;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int co = c * 16 + c16;
    const bool cok = co < a.la.ch;
    const int cc = cok ? co : 0;
    const int corr = zc * a.la.wsum[cc];
    const float sc = s_x * (a.la.per_channel ? a.la.w_scale[cc] : a.la.w_scale[0]);
    const float bi = a.la.bias ? a.la.bias[cc] : 0.0f;
    const float al = a.la.alpha ? a.la.alpha[cc] : 1.0f;
    const float be = a.la.alpha ? a.la.beta[cc] : 0.0f;
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float tv = cdp_epi(acc[p][c][k], corr, sc, bi, a.la.alpha != nullptr, al, be, a.la.relu);
        mid[c][p][k] = tv;
        if (cok && row0 + 2 * p + (k >> 1) < a.h && col0 + 2 * g + (k & 1) < a.w) {
          mlo = fminf(mlo, tv);
          mhi = fmaxf(mhi, tv);
        }
      }
  }
}

// The hand-off of one pixel group: mid quantized with (invm, zpfm, z_m) and
// written over the filled mid band (conv_dyn_pair.hip's quad transpose)
QCN_DEV void pair32_handoff(const ConvDynPairArgs& a, uint8_t* band, int row0, int col0, int lane, float invm,
                            float zpfm, int z_m, const float (&mid)[4][4][4]) {
  const int c16 = lane & 15, g = lane >> 4, q = c16 >> 2, e = c16 & 3;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const bool cok = c * 16 + c16 < a.la.ch;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      uint32_t d = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        d |= (cok ? quantize_legacy(mid[c][p][k], invm, zpfm) : (uint32_t)z_m) << (8 * k);
      d ^= 0x80808080u;
      // lane e of the quad takes position e of the quad's four channels
      uint32_t o = 0;
      o |= ((uint32_t)__builtin_amdgcn_update_dpp(0, (int)d, 0x00, 0xf, 0xf, false) >> (8 * e) & 0xffu);
      o |= ((uint32_t)__builtin_amdgcn_update_dpp(0, (int)d, 0x55, 0xf, 0xf, false) >> (8 * e) & 0xffu) << 8;
      o |= ((uint32_t)__builtin_amdgcn_update_dpp(0, (int)d, 0xaa, 0xf, 0xf, false) >> (8 * e) & 0xffu) << 16;
      o |= ((uint32_t)__builtin_amdgcn_update_dpp(0, (int)d, 0xff, 0xf, 0xf, false) >> (8 * e) & 0xffu) << 24;
      const int r = row0 + 2 * p + (e >> 1), col = col0 + 2 * g + (e & 1);
      if (c < a.mcg && r < a.h && col < a.w)
        *reinterpret_cast<uint32_t*>(band + (r + 1) * a.mrs + (col + 1) * a.mps + 16 * c + 4 * q) = o;
    }
  }
}

__global__ __launch_bounds__(P32_NT) void conv3x3_dyn_pair32_kernel(const ConvDynPairArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t band[];
  __shared__ float red[2][P32_NW];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c16 = lane & 15, g = lane >> 4;
  // pixel groups down and across that hold a position of the map, and the band
  // they read: rows and columns 0 .. 8 ng + 1
  const int ngy = (a.h + 7) >> 3, ngx = (a.w + 7) >> 3;
  const int lrows = 8 * ngy + 2, lcols = 8 * ngx + 2;
  // this wave's pixel groups (pgy, pgx) and (pgy + 2, pgx): group j starts at
  // row rowa + 16 j; the second is past the map whenever the first is
  const int col0 = 8 * (wave & 3), rowa = 8 * (wave >> 2);
  const int nown = col0 < a.w ? (rowa + 16 < a.h ? 2 : rowa < a.h ? 1 : 0) : 0;

  // the image index is used for the base pointers and stats rows and nowhere else
  const int img = blockIdx.x;
  const float* ximg = a.x + (size_t)img * a.h * a.w * a.cin;
  float* yimg = a.y + (size_t)img * (a.pool ? (a.h / 2) * (a.w / 2) : a.h * a.w) * a.lb.ch;

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
  if (a.x_qparams && tid == 0) {
    a.x_qparams[2 * (size_t)img] = s_x;
    a.x_qparams[2 * (size_t)img + 1] = qp.w;
  }

  const size_t wtile_a = (size_t)a.la.steps * 64, wtile_b = (size_t)a.lb.steps * 64;
  const v4i* wqa = a.la.wp + lane;
  const v4i* wqb = a.lb.wp + lane;
  v4i bn[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) bn[c] = wqa[c * wtile_a];

  // ---- phase 1: stage the image (conv_dyn.hip's loop, one chunk: cin <= 64)
  {
    const uint32_t zcode = splat_u8(z_x) ^ 0x80808080u;
    const int units = 4 * a.ncg;                                      // dwords per pixel
    for (int idx = tid; idx < lrows * lcols * units; idx += P32_NT) {
      const int pix = idx / units, u = idx - pix * units;
      const int pr = pix / lcols, pc = pix - pr * lcols;
      const int gr = pr - 1, gcol = pc - 1;
      const int c0 = 4 * u;
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
  }
  __syncthreads();

  // ---- phase 2: layer A of the wave's groups, results in registers; B's first
  // fragments are requested after the last K loop
  float mid0[4][4][4], mid1[4][4][4];
  float mlo = __builtin_inff(), mhi = -__builtin_inff();
  if (nown > 0)
    pair32_layer_a(a, band, rowa, col0, lane, z_x, s_x, wqa, wtile_a, nown > 1 ? wqa : wqb,
                   nown > 1 ? wtile_a : wtile_b, bn, mid0, mlo, mhi);
  if (nown > 1)
    pair32_layer_a(a, band, rowa + 16, col0, lane, z_x, s_x, wqa, wtile_a, wqb, wtile_b, bn, mid1, mlo, mhi);

  // ---- phase 3: the image's range and the mid qparams (block-uniform)
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    mlo = fminf(mlo, __shfl_xor(mlo, d));
    mhi = fmaxf(mhi, __shfl_xor(mhi, d));
  }
  if (lane == 0) { red[0][wave] = mlo; red[1][wave] = mhi; }
  __syncthreads();   // and every wave has finished reading the x band
#pragma unroll
  for (int i = 0; i < P32_NW; ++i) {
    mlo = fminf(mlo, red[0][i]);
    mhi = fmaxf(mhi, red[1][i]);
  }
  const float4 qm = choose_qparams(mlo, mhi, a.reduce_range);
  const float s_m = qm.x, invm = qm.y, zpfm = qm.z;
  const int z_m = __float_as_int(qm.w);
  if (a.mid_qparams && tid == 0) {
    a.mid_qparams[2 * (size_t)img] = s_m;
    a.mid_qparams[2 * (size_t)img + 1] = qm.w;
  }

  // ---- phase 4: the hand-off.  Every byte of the mid band's rows is the code
  // z_m (halo, positions past (h, w), channels past cmid: exactly 0 in B), then
  // the valid (position, channel) values are written over it.
  {
    const uint32_t mcode = splat_u8(z_m) ^ 0x80808080u;
    const uint4 fill = make_uint4(mcode, mcode, mcode, mcode);
    for (int idx = tid; idx < lrows * a.mrs / 16; idx += P32_NT) reinterpret_cast<uint4*>(band)[idx] = fill;
  }
  __syncthreads();
  if (nown > 0) pair32_handoff(a, band, rowa, col0, lane, invm, zpfm, z_m, mid0);
  if (nown > 1) pair32_handoff(a, band, rowa + 16, col0, lane, invm, zpfm, z_m, mid1);
  __syncthreads();

  // ---- phase 5: layer B from the mid band
  const int q = c16 >> 2, e = c16 & 3;
  const int oh = a.pool ? a.h / 2 : a.h, ow = a.pool ? a.w / 2 : a.w;
  const int cout = a.lb.ch, zc = z_m - 128;
  float ylo = __builtin_inff(), yhi = -__builtin_inff();
#pragma nounroll
  for (int j = 0; j < nown; ++j) {
    const int row0 = rowa + 16 * j;
    v4i acc[4][4];
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[p][c] = (v4i){0, 0, 0, 0};
    int gs = 0;
    cdp_chunk(band, (row0 + (e >> 1)) * a.mrs + (col0 + 2 * q + (e & 1)) * a.mps, a.mrs, a.mps, a.mcg, g, wqb,
              wtile_b, a.lb.steps, gs, bn, acc);
    if (j + 1 < nown) {
#pragma unroll
      for (int c = 0; c < 4; ++c) bn[c] = wqb[c * wtile_b];
    }

    // B's epilogue: register k of this lane is window g, position k, of channel c16
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int co = c * 16 + c16;
      if (co >= cout) continue;
      const int corr = zc * a.lb.wsum[co];
      const float sc = s_m * (a.lb.per_channel ? a.lb.w_scale[co] : a.lb.w_scale[0]);
      const float bi = a.lb.bias ? a.lb.bias[co] : 0.0f;
      const float al = a.lb.alpha ? a.lb.alpha[co] : 1.0f;
      const float be = a.lb.alpha ? a.lb.beta[co] : 0.0f;
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const int r = row0 + 2 * p, cc = col0 + 2 * g;
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
          v[k] = cdp_epi(acc[p][c][k], corr, sc, bi, a.lb.alpha != nullptr, al, be, a.lb.relu);
        if (a.pool) {
          if (r < a.h && cc < a.w) {
            const float m = fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3]));
            const int orow = r >> 1, ocol = cc >> 1;
            const size_t o = a.y_nchw ? ((size_t)co * oh + orow) * ow + ocol
                                      : ((size_t)orow * ow + ocol) * cout + co;
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
                                        : ((size_t)orow * ow + ocol) * cout + co;
              yimg[o] = v[k];
              ylo = fminf(ylo, v[k]);
              yhi = fmaxf(yhi, v[k]);
            }
          }
        }
      }
    }
  }

  // the image's output range -> its one slot (masked lanes hold +-inf)
  if (a.y_stats) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      ylo = fminf(ylo, __shfl_xor(ylo, d));
      yhi = fmaxf(yhi, __shfl_xor(yhi, d));
    }
    if (lane == 0) { red[0][wave] = ylo; red[1][wave] = yhi; }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
      for (int i = 1; i < P32_NW; ++i) {
        ylo = fminf(ylo, red[0][i]);
        yhi = fmaxf(yhi, red[1][i]);
      }
      a.y_stats[2 * (size_t)img] = ylo;
      a.y_stats[2 * (size_t)img + 1] = yhi;
    }
  }
}

static int launch_conv_dyn_pair32(ConvDynPairArgs a, int nimg, hipStream_t stream) {
  a.ps = cd_pixel_stride(a.ncg);
  a.rs = cd_row_stride(a.ncg, P32_LCOLS);
  a.mps = cd_pixel_stride(a.mcg);
  a.mrs = cd_row_stride(a.mcg, P32_LCOLS);
  // the mid band aliases the x band: the larger of the two, at most 34 rows of 64 channels
  constexpr int max_lds = P32_LCOLS * cd_row_stride(P32_CH / 16, P32_LCOLS);
  static_assert(max_lds + 2 * 4 * P32_NW <= 160 * 1024, "past the LDS of a workgroup");
  const int lds = P32_LCOLS * (a.rs > a.mrs ? a.rs : a.mrs);
  static bool lds_set[QCN_MAX_DEV] = {};
  auto kernel = conv3x3_dyn_pair32_kernel;
  if (!qcn_set_lds_once(reinterpret_cast<const void*>(kernel), max_lds, lds_set)) return QCN_ERR_HIP;
  hipLaunchKernelGGL(kernel, dim3((unsigned)nimg), dim3(P32_NT), lds, stream, a);
  return hipGetLastError() == hipSuccess ? QCN_OK : QCN_ERR_HIP;
}

}  // namespace qcn

extern "C" {

int qcn_conv3x3_dyn_pair32_supported(int h, int w, int cin, int cmid, int cout) {
  using namespace qcn;
  if (h < 1 || w < 1 || cin < 1 || cmid < 1 || cout < 1) return 0;
  return h <= P32_HW && w <= P32_HW && cin <= P32_CH && cmid <= P32_CH && cout <= P32_CH;
}

int qcn_conv3x3_dyn_pair32(const float* x, int nimg, int h, int w, int cin, int x_nchw, const float* x_stats,
                           int x_slots, int reduce_range, const qcn_dyn_layer_t* la, const qcn_dyn_layer_t* lb,
                           int pool, int y_nchw, float* y, float* y_stats, float* x_qparams, float* mid_qparams,
                           void* stream) {
  using namespace qcn;
  const int rc = cdp_check(x, nimg, h, w, cin, x_stats, x_slots, la, lb, pool, y, y_stats, x_qparams, mid_qparams,
                           qcn_conv3x3_dyn_pair32_supported);
  if (rc != QCN_OK) return rc;
  return launch_conv_dyn_pair32(cdp_args(x, h, w, cin, x_nchw, x_stats, x_slots, reduce_range, la, lb, pool, y_nchw,
                                         y, y_stats, x_qparams, mid_qparams),
                                nimg, static_cast<hipStream_t>(stream));
}

}  // extern "C"
