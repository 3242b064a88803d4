// Raw image input: u8 NHWC [n,h,w,3] -> normalised fp32 NCHW [n,3,h,w].
//
// ToTensor -> Normalize(mean, std) maps byte p of channel c to
// (fp32(p) / 255 - mean_c) / std_c, a function of (c, p): the host builds the
// 3 x 256 fp32 table once with torch's own ops (qconvnet/quant.py
// normalize_table) and this kernel only looks values up, so the result equals
// the host transform bit for bit.  It feeds every path without a u8 input
// stage of its own (the stand-alone conv1, GPU calibration, the fp32 and
// dynamic models); the conv1+conv2 phase (conv3x3_u8.hip) and the ResNet stems
// (resnet_stem.hip, stem_pack_u8_kernel below) read the bytes themselves.
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

// stem_pack_kernel (convgen.hip) on raw images: the QuantStub + row im2col of
// the 7x7/2 pad-3 stem, out[n][iy][ox][32] byte 3*s + ch =
// qlut[ch][img[n][iy][2*ox - 3 + s][ch]], the zero point outside the image and
// in bytes 21..31.  The 7 columns of an entry are 21 contiguous image bytes
// (byte loads: any w and any alignment of img); the u8 table sits in LDS.
__global__ __launch_bounds__(kNormThreads) void stem_pack_u8_kernel(
    const uint8_t* __restrict__ img, int n, int h, int w, int ow, const uint8_t* __restrict__ qlut,
    int zp, uint8_t* __restrict__ y) {
  __shared__ uint8_t tab[3 * 256];
  for (int i = threadIdx.x; i < 3 * 256; i += kNormThreads) tab[i] = qlut[i];
  __syncthreads();
  const long long e = (long long)blockIdx.x * kNormThreads + threadIdx.x;
  if (e >= (long long)n * h * ow) return;
  const int ox = (int)(e % ow);
  const long long row = e / ow;   // n * h + iy
  uint32_t wd[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) wd[i] = splat_u8(zp);
#pragma unroll
  for (int s = 0; s < 7; ++s) {
    const int ix = 2 * ox - 3 + s;
    if (ix < 0 || ix >= w) continue;
    const uint8_t* px = img + (row * w + ix) * 3;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const uint32_t q = tab[ch * 256 + px[ch]];
      const int b = 3 * s + ch;
      wd[b >> 2] = (wd[b >> 2] & ~(0xffu << (8 * (b & 3)))) | (q << (8 * (b & 3)));
    }
  }
  uint4* o = reinterpret_cast<uint4*>(y + e * 32);
  o[0] = make_uint4(wd[0], wd[1], wd[2], wd[3]);
  o[1] = make_uint4(wd[4], wd[5], wd[6], wd[7]);
}

}  // namespace qcn

extern "C" int qcn_stem_pack_u8_nhwc(const uint8_t* img, int nimg, int h, int w, const uint8_t* qlut,
                                     int zp, uint8_t* y, void* stream) {
  if (!img || !qlut || !y || nimg <= 0 || h <= 0 || w <= 0 || zp < 0 || zp > 255) return QCN_ERR_ARG;
  if (reinterpret_cast<uintptr_t>(y) & 15) return QCN_ERR_ARG;   // 16-byte stores
  const int ow = (w - 1) / 2 + 1;
  const long long total = (long long)nimg * h * ow;
  const long long grid = (total + qcn::kNormThreads - 1) / qcn::kNormThreads;
  if (grid > 0x7fffffffLL) return QCN_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(qcn::stem_pack_u8_kernel, dim3((unsigned)grid), dim3(qcn::kNormThreads), 0,
                     (hipStream_t)stream, img, nimg, h, w, ow, qlut, zp, y);
  return hipGetLastError() == hipSuccess ? QCN_OK : QCN_ERR_HIP;
}

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
