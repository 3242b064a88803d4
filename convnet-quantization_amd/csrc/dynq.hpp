// Dynamic activation quantization, shared by the dynamic Linear (linear.hip)
// and the dynamic int8 conv (conv_dyn.hip): qparams from a [lo, hi] range and
// the LEGACY quantize.  oracle/qref.py restates both on the host
// (choose_qparams_dynamic, quantize_legacy_fma).
#pragma once
#include "common.hpp"

namespace qcn {

// ATen ChooseQuantizationParams (torch/include/ATen/native/quantized/cpu/
// QuantUtils.h:70-185), preserve_sparsity = false, force_scale_power_of_two =
// false, from a [lo, hi] range.  Returns [scale, inv, zp_f, zp_i(bits)].
__device__ __forceinline__ float4 choose_qparams(float lo, float hi, int reduce_range) {
  int qmin = 0, qmax = 255;
  if (reduce_range) { qmin = qmin / 2; qmax = qmax / 2; }
  float mn = fminf(lo, 0.f), mx = fmaxf(hi, 0.f);
  double scale = ((double)mx - (double)mn) / (double)(qmax - qmin);
  if ((float)scale == 0.0f || __builtin_isinf(1.0f / (float)scale)) scale = 0.1;
  const float kSmall = 6.1e-5f;
  if (scale < (double)kSmall) {
    const float org = (float)scale;
    scale = (double)kSmall;
    if (mn == 0.0f) mx = kSmall * (float)(qmax - qmin);
    else if (mx == 0.0f) mn = -kSmall * (float)(qmax - qmin);
    else {
      const float amp = kSmall / org;
      mn *= amp;
      mx *= amp;
    }
  }
  const double zfm = (double)qmin - (double)mn / scale;
  const double zfx = (double)qmax - (double)mx / scale;
  const double efm = fabs((double)qmin) - fabs((double)mn / scale);
  const double efx = fabs((double)qmax) - fabs((double)mx / scale);
  const double z0 = efm < efx ? zfm : zfx;
  int zp;
  if (z0 < qmin) zp = qmin;
  else if (z0 > qmax) zp = qmax;
  else zp = (int)rint(z0);
  const float sf = (float)scale;
  return make_float4(sf, 1.0f / sf, (float)zp, __int_as_float(zp));
}

// fbgemm::QuantizeAvx2<uint8_t, LEGACY=true>: q = clamp(rne(min(fmaf(x, inv, zp), 255)), 0, 255).
__device__ __forceinline__ uint32_t quantize_legacy(float x, float inv, float zpf) {
  float t = __builtin_fmaf(x, inv, zpf);
  t = fminf(t, 255.0f);
  t = __builtin_rintf(t);
  t = fmaxf(t, 0.0f);
  return (uint32_t)(int)t;
}

}  // namespace qcn
