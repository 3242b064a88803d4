// Host-side helpers of the 3x3-conv entry points (conv3x3.hip, conv3x3_u8.hip,
// convs36.hip and the diagnostic tools/clock library): how a ConvEpi is
// filled, how a kernel with dynamic LDS is launched and how an array of
// qcn_conv_layer_t is validated are each written here once.  No device code.
#pragma once
#include "conv_epi.hpp"

namespace qcn {

// The epilogue of one conv: requant constants, output zero point, the lower
// clamp of a fused ReLU, the optional QDQ hand-off (set_qdq picks its form)
// and conv6's chunk-major output layout.  Everything else stays zero.
inline ConvEpi make_epi(const float* u, const float* v, const float* mult, const int32_t* corr, int zp_y,
                        bool relu, const qcn_qdq_t* qdq = nullptr, bool kmajor = false) {
  ConvEpi ep{};
  ep.u = u;
  ep.v = v;
  ep.mult = mult;
  ep.corr = corr;
  ep.zp_y = zp_y;
  ep.lo = relu ? zp_y : 0;
  ep.kmajor = kmajor ? 1 : 0;
  if (qdq) set_qdq(ep, qdq);
  return ep;
}
inline ConvEpi make_epi(const qcn_conv_layer_t& l, bool kmajor = false) {
  return make_epi(l.u, l.v, l.mult, l.corr, l.y_zp, l.relu != 0, l.qdq, kmajor);
}

inline bool zp_ok(int zp) { return zp >= 0 && zp <= 255; }

// every pointer of the layer set, both zero points in the u8 range
inline bool layer_ok(const qcn_conv_layer_t& l) {
  return l.w && l.u && l.v && l.mult && l.corr && zp_ok(l.x_zp) && zp_ok(l.y_zp);
}

// conv6's chunk-major stores (and the a2 / a4 write-through stores) take
// 32-bit byte offsets: 4096 B per image
inline bool offsets_fit(int nimg) { return (long)nimg * 4096 <= 0x7fffffffL; }

// k chained conv layers into ep[0 .. k): QCN_ERR_ARG unless every layer is
// layer_ok and conv i reads conv i-1's output (its input zero point is that
// layer's output zero point, or the z2 of that layer's QDQ hand-off).  The
// last layer writes chunk-major when kmajor.  Otherwise returns the epilogue
// form layers [first, k) share: 1 all on the FBGEMM fast path, 2 all on the
// one-fma QDQ form, 0 mixed.
inline int conv_layers_epi(const qcn_conv_layer_t* layers, int k, int first, bool kmajor, ConvEpi* ep) {
  if (!layers) return QCN_ERR_ARG;
  bool all1 = true, all2 = true;
  for (int i = 0; i < k; ++i) {
    const qcn_conv_layer_t& l = layers[i];
    if (!layer_ok(l)) return QCN_ERR_ARG;
    if (i > 0 && l.x_zp != (layers[i - 1].qdq ? layers[i - 1].qdq->z2 : layers[i - 1].y_zp)) return QCN_ERR_ARG;
    ep[i] = make_epi(l, kmajor && i == k - 1);
    if (i >= first) {
      all1 = all1 && epi_mode(ep[i]) == 1;
      all2 = all2 && epi_mode(ep[i]) == 2;
    }
  }
  return all1 ? 1 : (all2 ? 2 : 0);
}

// Launch kernel K with lds bytes of dynamic LDS on the current device; the
// LDS limit of K is raised once per device (the flags are per K: one
// instance of this function each).
template <auto K, class... A>
int launch_lds(dim3 grid, dim3 block, int lds, hipStream_t st, const A&... args) {
  static bool done[QCN_MAX_DEV] = {};
  if (!qcn_set_lds_once((const void*)K, lds, done)) return QCN_ERR_HIP;
  hipLaunchKernelGGL(K, grid, block, lds, st, args...);
  return hipGetLastError() == hipSuccess ? QCN_OK : QCN_ERR_HIP;
}

}  // namespace qcn
