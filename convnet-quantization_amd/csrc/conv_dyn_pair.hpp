// Shared by the dynamic int8 conv pair kernels (conv_dyn_pair.hip, DESIGN §25;
// conv_dyn_pair32.hip): a layer's arguments, the K loop of one
// resident chunk, the epilogue value and the argument checks of the entries.
#pragma once
#include "common.hpp"
#include "conv_dyn.hpp"
#include "qconvnet_abi.hpp"

namespace qcn {

struct ConvDynLayer {
  const v4i* wp;
  const int* wsum;
  const float* w_scale;
  const float* bias;
  const float* alpha;
  const float* beta;
  int ch;                 // output channels
  int per_channel, relu;
  int n64;                // 64-channel groups: ceil(ch / 64)
  int steps;              // cd_steps(input channels)
};

struct ConvDynPairArgs {
  const float* x;
  const float* x_stats;   // [nimg][x_slots][2]
  ConvDynLayer la, lb;
  float* y;
  float* y_stats;         // [nimg][1][2] or null
  float* x_qparams;       // [nimg][2] (scale, zero point bits) or null
  float* mid_qparams;     // [nimg][2] or null
  int h, w, cin;
  int x_slots, reduce_range;
  int x_nchw, x_vec, pool, y_nchw;
  int ncg, ps, rs;        // A: 16-channel groups of cin, band strides of its (first) chunk
  int mcg, mps, mrs;      // mid band: 16-channel groups of cmid, strides
};

// K loop of one chunk of ncgc channel groups resident in `band` (conv_dyn.hip's
// loop): lane group g walks units g, g + 4, ...; (tap, cg) of unit u is
// (u / ncgc, u % ncgc), a unit past the chunk reads unit 0 (zero weights).
// bn holds the weight fragments of step gs on entry and of the step after the
// chunk on exit (none past `total`).
QCN_DEV void cdp_chunk(const uint8_t* band, int abase, int rs, int ps, int ncgc, int g, const v4i* wq,
                       size_t wtile, int total, int& gs, v4i (&bn)[4], v4i (&acc)[4][4]) {
  const int steps = (9 * ncgc + 3) / 4;
  int tap = 0, cg = g;
#pragma unroll
  for (int k = 0; k < 3; ++k)
    if (cg >= ncgc) { cg -= ncgc; ++tap; }
  v4i an[4];
  {
    const int off = abase + (tap / 3) * rs + (tap % 3) * ps + 16 * cg;
#pragma unroll
    for (int p = 0; p < 4; ++p) an[p] = *reinterpret_cast<const v4i*>(band + off + 2 * p * rs);
  }
  for (int t = 0; t < steps; ++t) {
    v4i av[4], bv[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) { av[k] = an[k]; bv[k] = bn[k]; }
    ++gs;
    if (gs < total) {
#pragma unroll
      for (int c = 0; c < 4; ++c) bn[c] = wq[c * wtile + (size_t)gs * 64];
    }
    if (t + 1 < steps) {
      cg += 4;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (cg >= ncgc) { cg -= ncgc; ++tap; }
      const int off = abase + (tap < 9 ? (tap / 3) * rs + (tap % 3) * ps + 16 * cg : 0);
#pragma unroll
      for (int p = 0; p < 4; ++p) an[p] = *reinterpret_cast<const v4i*>(band + off + 2 * p * rs);
    }
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
      for (int c = 0; c < 4; ++c)
        acc[p][c] = __builtin_amdgcn_mfma_i32_16x16x64_i8(av[p], bv[c], acc[p][c], 0, 0, 0);
  }
}

// fmaf(acc - corr, s_x * s_w, bias), the optional affine, the optional ReLU
QCN_DEV float cdp_epi(int acc, int corr, float sc, float bi, bool affine, float al, float be, bool relu) {
  float tv = __builtin_fmaf((float)(acc - corr), sc, bi);
  if (affine) tv = __builtin_fmaf(tv, al, be);
  if (relu) tv = fmaxf(tv, 0.0f);
  return tv;
}

static ConvDynLayer cdp_layer(const qcn_dyn_layer_t& l, int cin) {
  ConvDynLayer d = {};
  d.wp = reinterpret_cast<const v4i*>(l.w_packed); d.wsum = l.wsum; d.w_scale = l.w_scale;
  d.bias = l.bias; d.alpha = l.alpha; d.beta = l.beta;
  d.ch = l.channels; d.per_channel = l.per_channel != 0; d.relu = l.relu != 0;
  d.n64 = (l.channels + 63) / 64;
  d.steps = cd_steps(cin);
  return d;
}

// The argument checks of a pair entry, all before any HIP call: QCN_ERR_ARG for
// bad pointers, sizes, alignment and a pool with odd h or w, then
// QCN_ERR_UNSUPPORTED where `supported` refuses the shape or x or y has more
// than 2^31 - 1 elements.
static int cdp_check(const float* x, int nimg, int h, int w, int cin, const float* x_stats, int x_slots,
                     const qcn_dyn_layer_t* la, const qcn_dyn_layer_t* lb, int pool, const float* y,
                     const float* y_stats, const float* x_qparams, const float* mid_qparams,
                     int (*supported)(int, int, int, int, int)) {
  if (!x || !x_stats || !la || !lb || !y) return QCN_ERR_ARG;
  uintptr_t low = (uintptr_t)x | (uintptr_t)y | (uintptr_t)x_stats | (uintptr_t)y_stats | (uintptr_t)x_qparams |
                  (uintptr_t)mid_qparams;
  for (const qcn_dyn_layer_t* l : {la, lb}) {
    if (!l->w_packed || !l->wsum || !l->w_scale || l->channels < 1) return QCN_ERR_ARG;
    if ((l->alpha == nullptr) != (l->beta == nullptr)) return QCN_ERR_ARG;
    if ((uintptr_t)l->w_packed & 15) return QCN_ERR_ARG;
    low |= (uintptr_t)l->wsum | (uintptr_t)l->w_scale;
  }
  if (nimg < 1 || h < 1 || w < 1 || cin < 1 || x_slots < 1) return QCN_ERR_ARG;
  if (pool && ((h | w) & 1)) return QCN_ERR_ARG;
  if (low & 3) return QCN_ERR_ARG;
  if (!supported(h, w, cin, la->channels, lb->channels)) return QCN_ERR_UNSUPPORTED;
  const long px = (long)nimg * h * w;
  if (px * cin > 0x7fffffffL || px * lb->channels > 0x7fffffffL) return QCN_ERR_UNSUPPORTED;
  return QCN_OK;
}

// The launch arguments of a checked call (band strides are the launcher's)
static ConvDynPairArgs cdp_args(const float* x, int h, int w, int cin, int x_nchw, const float* x_stats,
                                int x_slots, int reduce_range, const qcn_dyn_layer_t* la,
                                const qcn_dyn_layer_t* lb, int pool, int y_nchw, float* y, float* y_stats,
                                float* x_qparams, float* mid_qparams) {
  ConvDynPairArgs a = {};
  a.x = x; a.x_stats = x_stats; a.la = cdp_layer(*la, cin); a.lb = cdp_layer(*lb, la->channels);
  a.y = y; a.y_stats = y_stats; a.x_qparams = x_qparams; a.mid_qparams = mid_qparams;
  a.h = h; a.w = w; a.cin = cin;
  a.x_slots = x_slots; a.reduce_range = reduce_range != 0;
  a.x_nchw = x_nchw != 0;
  a.x_vec = !x_nchw && cin % 4 == 0 && ((uintptr_t)x & 15) == 0;
  a.pool = pool != 0; a.y_nchw = y_nchw != 0;
  a.ncg = (cin + 15) / 16;
  a.mcg = (la->channels + 15) / 16;
  return a;
}

}  // namespace qcn
