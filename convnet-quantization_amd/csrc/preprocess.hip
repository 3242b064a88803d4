// Raw image input: u8 NHWC [n,h,w,3] -> normalised fp32 NCHW [n,3,h,w].
//
// ToTensor -> Normalize(mean, std) maps byte p of channel c to
// (fp32(p) / 255 - mean_c) / std_c, a function of (c, p): the host builds the
// 3 x 256 fp32 table once with torch's own ops (qconvnet/quant.py
// normalize_table) and this kernel only looks values up, so the result equals
// the host transform bit for bit.  It feeds every path without a u8 input
// stage of its own (the stand-alone conv1, GPU calibration, the fp32 and
// dynamic models, the ResNet executors); the conv1+conv2 phase reads the bytes
// itself (conv3x3_u8.hip).
//
// Memory-bound: 3 B in, 12 B out per pixel.  Persistent grid sized from the CU
// count.  Quad form (h*w a multiple of 4, x 16-B aligned): a lane owns four
// consecutive pixels of one image — 12 contiguous input bytes (any alignment;
// the loads of all kQuadUnroll quads are issued before the first lookup) and
// one float4 per plane, so a wave reads 768 contiguous bytes and writes 1 KB
// contiguous per plane.  Pixel form (any other shape): a lane owns one pixel.
// The table sits in LDS (3 KB per workgroup).  Pixel counts are 64-bit; the
// image index comes from a 32-bit division while the count allows it.
#include "common.hpp"
#include "qconvnet_abi.hpp"

namespace qcn {

constexpr int kNormThreads = 256;
constexpr int kNormBlocksPerCu = 8;
constexpr int kQuadUnroll = 4;

// pixel index P of the flat [n][hw] stream -> offset of (image, channel 0, pixel) in x
QCN_DEV long long nchw_offset(long long P, int hw, bool small) {
  long long im, p;
  if (small) {   // workgroup-uniform: every pixel index fits 32 bits
    const uint32_t q = (uint32_t)P / (uint32_t)hw;
    im = q;
    p = (uint32_t)P - q * (uint32_t)hw;
  } else {
    im = P / hw;
    p = P - im * hw;
  }
  return im * 3 * hw + p;
}

QCN_DEV void load_ntab(float* tab, const float* __restrict__ ntab) {
  for (int i = threadIdx.x; i < 3 * 256; i += kNormThreads) tab[i] = ntab[i];
  __syncthreads();
}

__global__ __launch_bounds__(kNormThreads) void u8img_normalize_quad_kernel(
    const uint8_t* __restrict__ img, long long nquad, int hw, const float* __restrict__ ntab,
    float* __restrict__ x) {
  __shared__ float tab[3 * 256];
  load_ntab(tab, ntab);
  const bool small = nquad <= 0x3fffffffLL;
  const long long stride = (long long)gridDim.x * kNormThreads;
  for (long long base = (long long)blockIdx.x * kNormThreads; base < nquad;
       base += stride * kQuadUnroll) {
    uint32_t w[kQuadUnroll][3];
    bool ok[kQuadUnroll];
#pragma unroll
    for (int u = 0; u < kQuadUnroll; ++u) {
      const long long q = base + u * stride + threadIdx.x;
      ok[u] = q < nquad;
      if (ok[u]) __builtin_memcpy(w[u], img + q * 12, 12);
    }
#pragma unroll
    for (int u = 0; u < kQuadUnroll; ++u) {
      if (!ok[u]) continue;
      const long long q = base + u * stride + threadIdx.x;
      float* o = x + nchw_offset(q * 4, hw, small);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int k = 3 * e + c;   // byte k of the 12: pixel e, channel c
          v[e] = tab[c * 256 + ((w[u][k >> 2] >> (8 * (k & 3))) & 0xffu)];
        }
        *reinterpret_cast<float4*>(o + (long long)c * hw) = make_float4(v[0], v[1], v[2], v[3]);
      }
    }
  }
}

__global__ __launch_bounds__(kNormThreads) void u8img_normalize_pixel_kernel(
    const uint8_t* __restrict__ img, long long npix, int hw, const float* __restrict__ ntab,
    float* __restrict__ x) {
  __shared__ float tab[3 * 256];
  load_ntab(tab, ntab);
  const bool small = npix <= 0xffffffffLL;
  const long long stride = (long long)gridDim.x * kNormThreads;
  for (long long P = (long long)blockIdx.x * kNormThreads + threadIdx.x; P < npix; P += stride) {
    const uint8_t* s = img + P * 3;
    float* o = x + nchw_offset(P, hw, small);
#pragma unroll
    for (int c = 0; c < 3; ++c) o[(long long)c * hw] = tab[c * 256 + s[c]];
  }
}

}  // namespace qcn

extern "C" int qcn_u8img_normalize_f32_nchw(const uint8_t* img, int n, int h, int w, const float* ntab,
                                            float* x, void* stream) {
  if (!img || !ntab || !x || n <= 0 || h <= 0 || w <= 0) return QCN_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(ntab) & 3) || (reinterpret_cast<uintptr_t>(x) & 3)) return QCN_ERR_ARG;
  if ((long long)h * w > 0x7fffffffLL / 3) return QCN_ERR_UNSUPPORTED;   // 3 * h * w as an int
  const int hw = h * w;
  const long long npix = (long long)n * hw;
  const int ncu = qcn_cu_count();
  if (ncu <= 0) return QCN_ERR_HIP;
  const long long cap = (long long)ncu * qcn::kNormBlocksPerCu;
  const bool quad = hw % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0;
  const long long items = quad ? npix / 4 : npix;
  long long grid = (items + qcn::kNormThreads - 1) / qcn::kNormThreads;
  grid = grid > cap ? cap : grid;
  if (quad)
    hipLaunchKernelGGL(qcn::u8img_normalize_quad_kernel, dim3((unsigned)grid), dim3(qcn::kNormThreads), 0,
                       (hipStream_t)stream, img, items, hw, ntab, x);
  else
    hipLaunchKernelGGL(qcn::u8img_normalize_pixel_kernel, dim3((unsigned)grid), dim3(qcn::kNormThreads), 0,
                       (hipStream_t)stream, img, items, hw, ntab, x);
  return hipGetLastError() == hipSuccess ? QCN_OK : QCN_ERR_HIP;
}
