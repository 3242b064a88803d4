// Two dynamically quantized int8 3x3 convolutions in one launch:
// layer A (no pool) and layer B of conv_dyn.hip's contract, with A's output
// handed to B as u8 codes in LDS.  One workgroup holds a whole image of the
// intermediate activation in its accumulator registers, so it knows the
// image's range before anything is stored: it reduces min / max, chooses the
// qparams, quantizes its own registers into B's band and runs B from there.
// The intermediate never exists in HBM and never as fp32 outside registers.
//
// The bits are those of qcn_conv3x3_dyn (A, range recorded) followed by
// qcn_conv3x3_dyn (B): the same fp32 values meet the same choose_qparams and
// quantize_legacy.  min / max are order-independent but for the sign of a zero,
// which choose_qparams cannot tell apart.
//
// Work split.  A wave owns one 8 x 8 pixel group (4 pixel tiles of 2 x 8) x 64
// channels, conv_dyn.hip's 64-accumulator shape, in both layers.  The
// workgroup is PGY x PGX pixel groups x CG channel groups of waves and covers
// an (8 PGY) x (8 PGX) map with up to 64 CG channels in cmid and cout:
//   <1,1,4>  256 threads   h, w <= 8    cmid, cout <= 256     (conv5 + conv6)
//   <2,2,2>  512 threads   h, w <= 16   cmid, cout <= 128     (conv3 + conv4)
//
// Phases of a block (barriers between them):
//   1  stage x (quantize on stage, whole image + halo) and run A's K loop,
//      per 256-channel chunk of cin, as conv_dyn.hip
//   2  A's epilogue into registers (fp32); B's first weight fragments requested
//   3  image range of the valid (position, channel) values: xor shuffles, then
//      across waves through LDS; every thread computes (s_m, z_m)
//   4  the mid band [row][column][channel] bytes (strides of cmid's channel
//      groups, may alias A's band): filled with the code z_m (halo, positions
//      past (h, w), channels past cmid), then every lane quantizes its 64
//      values, transposes 4 x 4 bytes inside its lane quad (DPP quad_perm) so
//      that it holds 4 neighbouring channels of one position, and writes dwords
//   5  B's K loop from the mid band (one chunk: cmid <= 256), B's epilogue
//      (affine, ReLU, 2x2 register-max pool, NHWC / NCHW) and the image's
//      output range into its one y_stats slot
#include "common.hpp"
#include "conv_dyn.hpp"
#include "conv_dyn_pair.hpp"
#include "dynq.hpp"
#include "qconvnet_abi.hpp"

namespace qcn {

template <int PGY, int PGX, int CG>
__global__ __launch_bounds__(64 * PGY * PGX * CG) void conv3x3_dyn_pair_kernel(const ConvDynPairArgs a) {
  constexpr int NW = PGY * PGX * CG, NT = 64 * NW;
  constexpr int LROWS = 8 * PGY + 2, LCOLS = 8 * PGX + 2;
  extern __shared__ __attribute__((aligned(16))) uint8_t band[];
  __shared__ float red[2][NW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c16 = lane & 15, g = lane >> 4;
  const int pgx = wave % PGX, pgy = (wave / PGX) % PGY, cgw = wave / (PGX * PGY);
  const int row0 = 8 * pgy, col0 = 8 * pgx;

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
  const uint32_t zcode = splat_u8(z_x) ^ 0x80808080u;

  // this lane's A-operand pixel of pixel tile 0 (tile pt is 2 pt rows further
  // down), in pixels; the byte offset takes the strides of the band it reads
  const int q = c16 >> 2, e = c16 & 3;
  const int prow = row0 + (e >> 1), pcol = col0 + 2 * q + (e & 1);
  // weight streams (clamped: a wave past the packed tiles recomputes the last
  // group; its channels are past cmid / cout and are masked everywhere below)
  const int ga = cgw < a.la.n64 ? cgw : a.la.n64 - 1;
  const int gb = cgw < a.lb.n64 ? cgw : a.lb.n64 - 1;
  const size_t wtile_a = (size_t)a.la.steps * 64, wtile_b = (size_t)a.lb.steps * 64;
  const v4i* wqa = a.la.wp + (size_t)ga * 4 * wtile_a + lane;
  const v4i* wqb = a.lb.wp + (size_t)gb * 4 * wtile_b + lane;

  v4i acc[4][4];
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[p][c] = (v4i){0, 0, 0, 0};

  // ---- phase 1: stage the image, layer A
  int gs = 0;
  v4i bn[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) bn[c] = wqa[c * wtile_a];
  const int nchunk = (a.ncg + 15) / 16;
  for (int ch = 0; ch < nchunk; ++ch) {
    const int ncgc = a.ncg - 16 * ch < 16 ? a.ncg - 16 * ch : 16;
    const int units = 4 * ncgc;                                     // dwords per pixel
    __syncthreads();   // the previous chunk's reads are done
    for (int idx = tid; idx < LROWS * LCOLS * units; idx += NT) {
      const int pix = idx / units, u = idx - pix * units;
      const int pr = pix / LCOLS, pc = pix - pr * LCOLS;
      const int gr = pr - 1, gcol = pc - 1;
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
    cdp_chunk(band, prow * a.rs + pcol * a.ps, a.rs, a.ps, ncgc, g, wqa, wtile_a, a.la.steps, gs, bn, acc);
  }
  // B's first weight fragments: their latency hides under phases 2 to 4
#pragma unroll
  for (int c = 0; c < 4; ++c) bn[c] = wqb[c * wtile_b];

  // ---- phase 2: A's epilogue in registers.  Register k of mid[c][p] is
  // window g, position k, of channel c16 of channel tile c, pixel tile p.
  float mid[4][4][4];
  float mlo = __builtin_inff(), mhi = -__builtin_inff();
  {
    const int zc = z_x - 128;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int co = (cgw * 4 + c) * 16 + c16;
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

  // ---- phase 3: the image's range and the mid qparams (block-uniform)
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    mlo = fminf(mlo, __shfl_xor(mlo, d));
    mhi = fmaxf(mhi, __shfl_xor(mhi, d));
  }
  if (lane == 0) { red[0][wave] = mlo; red[1][wave] = mhi; }
  __syncthreads();   // and every wave has finished reading A's band
#pragma unroll
  for (int i = 0; i < NW; ++i) {
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

  // ---- phase 4: the hand-off.  Every byte of the mid band is the code z_m,
  // then the valid (position, channel) values are written over it.
  {
    const uint32_t mcode = splat_u8(z_m) ^ 0x80808080u;
    const uint4 fill = make_uint4(mcode, mcode, mcode, mcode);
    for (int idx = tid; idx < LROWS * a.mrs / 16; idx += NT) reinterpret_cast<uint4*>(band)[idx] = fill;
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int tile = cgw * 4 + c;                       // 16-channel group of the mid band
    const bool cok = tile * 16 + c16 < a.la.ch;
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
      const int r = row0 + 2 * p + (e >> 1), cc = col0 + 2 * g + (e & 1);
      if (tile < a.mcg && r < a.h && cc < a.w)
        *reinterpret_cast<uint32_t*>(band + (r + 1) * a.mrs + (cc + 1) * a.mps + 16 * tile + 4 * q) = o;
    }
  }
  __syncthreads();

  // ---- phase 5: layer B from the mid band
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[p][c] = (v4i){0, 0, 0, 0};
  gs = 0;
  cdp_chunk(band, prow * a.mrs + pcol * a.mps, a.mrs, a.mps, a.mcg, g, wqb, wtile_b, a.lb.steps, gs, bn, acc);

  // B's epilogue: register k of this lane is window g, position k, of channel c16
  const int oh = a.pool ? a.h / 2 : a.h, ow = a.pool ? a.w / 2 : a.w;
  const int cout = a.lb.ch, zc = z_m - 128;
  float ylo = __builtin_inff(), yhi = -__builtin_inff();
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int co = (cgw * 4 + c) * 16 + c16;
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
      for (int i = 1; i < NW; ++i) {
        ylo = fminf(ylo, red[0][i]);
        yhi = fmaxf(yhi, red[1][i]);
      }
      a.y_stats[2 * (size_t)img] = ylo;
      a.y_stats[2 * (size_t)img + 1] = yhi;
    }
  }
}

// 1: <1,1,4>, 2: <2,2,2>, 0: no pair kernel; a function of (h, w, cmid, cout) only
static int cdp_class(int h, int w, int cmid, int cout) {
  if (h <= 8 && w <= 8 && cmid <= 256 && cout <= 256) return 1;
  if (h <= 16 && w <= 16 && cmid <= 128 && cout <= 128) return 2;
  return 0;
}

template <int PGY, int PGX, int CG>
static int launch_conv_dyn_pair(ConvDynPairArgs a, int nimg, hipStream_t stream) {
  constexpr int LROWS = 8 * PGY + 2, LCOLS = 8 * PGX + 2;
  const int ncg0 = a.ncg < 16 ? a.ncg : 16;
  a.ps = cd_pixel_stride(ncg0);
  a.rs = cd_row_stride(ncg0, LCOLS);
  a.mps = cd_pixel_stride(a.mcg);
  a.mrs = cd_row_stride(a.mcg, LCOLS);
  // the mid band aliases A's band: the larger of the two, at most a full chunk's
  constexpr int max_lds = LROWS * cd_row_stride(16, LCOLS);
  static_assert(max_lds + 2 * 4 * PGY * PGX * CG <= 160 * 1024, "past the LDS of a workgroup");
  const int lds = LROWS * (a.rs > a.mrs ? a.rs : a.mrs);
  static bool lds_set[QCN_MAX_DEV] = {};
  auto kernel = conv3x3_dyn_pair_kernel<PGY, PGX, CG>;
  if (!qcn_set_lds_once(reinterpret_cast<const void*>(kernel), max_lds, lds_set)) return QCN_ERR_HIP;
  hipLaunchKernelGGL(kernel, dim3((unsigned)nimg), dim3(64 * PGY * PGX * CG), lds, stream, a);
  return hipGetLastError() == hipSuccess ? QCN_OK : QCN_ERR_HIP;
}

}  // namespace qcn

extern "C" {

int qcn_conv3x3_dyn_pair_supported(int h, int w, int cin, int cmid, int cout) {
  if (h < 1 || w < 1 || cin < 1 || cmid < 1 || cout < 1 || cin > qcn::CD_MAX_CIN) return 0;
  return qcn::cdp_class(h, w, cmid, cout) != 0;
}

int qcn_conv3x3_dyn_pair(const float* x, int nimg, int h, int w, int cin, int x_nchw, const float* x_stats,
                         int x_slots, int reduce_range, const qcn_dyn_layer_t* la, const qcn_dyn_layer_t* lb,
                         int pool, int y_nchw, float* y, float* y_stats, float* x_qparams, float* mid_qparams,
                         void* stream) {
  using namespace qcn;
  const int rc = cdp_check(x, nimg, h, w, cin, x_stats, x_slots, la, lb, pool, y, y_stats, x_qparams, mid_qparams,
                           qcn_conv3x3_dyn_pair_supported);
  if (rc != QCN_OK) return rc;
  const ConvDynPairArgs a = cdp_args(x, h, w, cin, x_nchw, x_stats, x_slots, reduce_range, la, lb, pool, y_nchw, y,
                                     y_stats, x_qparams, mid_qparams);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (cdp_class(h, w, la->channels, lb->channels) == 1) return launch_conv_dyn_pair<1, 1, 4>(a, nimg, s);
  return launch_conv_dyn_pair<2, 2, 2>(a, nimg, s);
}

}  // extern "C"
