// Resize(R) -> CenterCrop(C) of raw u8 HWC images of mixed sizes on the
// device, byte for byte Pillow's bilinear Image.resize followed by a crop
// (the arithmetic is restated in tests/resizeref.py and in
// include/qconvnet.h).
//
// Three launches on the caller's stream, nothing allocated, no sync:
//   1. resize_taps_kernel: one lane per needed output column / row of every
//      image computes its window start and its 22-bit fixed-point taps in
//      double, by Pillow's recipe, and writes the record [xmin, n, k[0..n)]
//      to the workspace.  Nothing about an (in, out) pair is computed on the
//      host, so a batch of mixed sizes costs the host one pass over the
//      descriptors (the argument check) and no tables.
//   2. resize_h_kernel: the horizontal pass, over the source rows the crop
//      window's vertical taps reach and the window's columns only; writes the
//      u8 intermediate image to the workspace.
//   3. resize_v_kernel: the vertical pass over that intermediate into y.
// The intermediate goes through memory, not LDS: it is [rows][cw][3] bytes
// per image (about 220 KB at 500x375 -> 224x224), written and read once, a
// small share of the source bytes the first pass has to read anyway, and both
// passes stay plain maps of one lane per output pixel with no tile whose
// source-row reach depends on the image's scale.
//
// Work is laid out the same way in passes 2 and 3: a workgroup takes a unit
// of 256 / cw whole rows of one image (one row, walked in steps of 256
// columns, when cw >= 256); units are numbered image-major in 64 bits and
// walked with a grid-stride loop, so the grid does not grow with nimg.  Every
// image has the same number of units (the batch's largest row count, from
// the host's bound below); lanes past an image's own rows skip.
//
// Sizes: the tap record stride S and the intermediate's per-image stride are
// host arithmetic on the descriptors (resize_check), the same in
// qcn_resize_crop_workspace_size and in the launch.  The rows an image needs
// are bounded without the taps: xmax(last) - xmin(first) <=
// (ch - 1) * scale + 2 * support + 1, taken with one row of slack, so the
// bound holds whatever the last bit of a device double is.
#include <math.h>

#include "common.hpp"
#include "qconvnet_abi.hpp"

namespace qcn {

constexpr int kResizeThreads = 256;
constexpr int kResizeBlocksPerCu = 16;
constexpr double kResizeMaxScale = 32.0;   // ceil(in / out) above this: unsupported
constexpr int kResizePrecisionBits = 22;

// Pillow's precompute_coeffs + normalize_coeffs_8bpc for one output sample.
// rec: [xmin, n, k[0 .. n)], room for kmax taps.
QCN_DEV void resize_taps(int in, int out, int xx, int kmax, int32_t* __restrict__ rec) {
  const double scale = (double)in / (double)out;
  const double fs = scale > 1.0 ? scale : 1.0;
  const double support = 1.0 * fs;
  const double ss = 1.0 / fs;
  const double center = ((double)xx + 0.5) * scale;
  int xmin = (int)(center - support + 0.5);
  xmin = xmin < 0 ? 0 : xmin;
  int xmax = (int)(center + support + 0.5);
  xmax = xmax > in ? in : xmax;
  int n = xmax - xmin;
  n = n < 0 ? 0 : (n > kmax ? kmax : n);   // never taken: (int)ceil(support) * 2 + 1 <= kmax
  double ww = 0.0;
  for (int i = 0; i < n; ++i) {
    const double w = 1.0 - fabs(((double)(i + xmin) - center + 0.5) * ss);
    ww += w > 0.0 ? w : 0.0;
  }
  for (int i = 0; i < n; ++i) {
    double w = 1.0 - fabs(((double)(i + xmin) - center + 0.5) * ss);
    w = w > 0.0 ? w : 0.0;
    rec[2 + i] = (int)(0.5 + (w / ww) * 4194304.0);
  }
  rec[0] = xmin;
  rec[1] = n;
}

__global__ __launch_bounds__(kResizeThreads) void resize_taps_kernel(
    const qcn_resize_img_t* __restrict__ desc, long long nimg, int ch, int cw, int stride,
    int32_t* __restrict__ tab) {
  const int per = cw + ch;
  const long long total = nimg * per;
  for (long long e = (long long)blockIdx.x * kResizeThreads + threadIdx.x; e < total;
       e += (long long)gridDim.x * kResizeThreads) {
    const long long img = e / per;
    const int j = (int)(e - img * per);
    const qcn_resize_img_t d = desc[img];
    if (j < cw)
      resize_taps(d.w, d.ow, d.left + j, stride - 2, tab + e * stride);
    else
      resize_taps(d.h, d.oh, d.top + (j - cw), stride - 2, tab + e * stride);
  }
}

QCN_DEV uint8_t resize_clip8(int acc) {
  const int v = acc >> kResizePrecisionBits;
  return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// The rows of one image per workgroup step and this lane's place in them.
struct ResizeLane {
  int rpb;      // whole rows per unit
  int rr, c0;   // this lane's row in the unit, its first column
  bool active;
  QCN_DEV ResizeLane(int cw) {
    const int tid = threadIdx.x;
    rpb = cw < kResizeThreads ? kResizeThreads / cw : 1;
    rr = cw < kResizeThreads ? tid / cw : 0;
    c0 = tid - rr * cw;
    active = rr < rpb;
  }
};

// Horizontal pass: mid[img][r][c][0..3) for r < rows(img), the source rows
// yfirst + r that the window's vertical taps reach.
__global__ __launch_bounds__(kResizeThreads) void resize_h_kernel(
    const uint8_t* __restrict__ src, const qcn_resize_img_t* __restrict__ desc, long long nimg, int ch,
    int cw, int stride, const int32_t* __restrict__ tab, uint8_t* __restrict__ mid, long long mid_stride,
    int maxrows) {
  const ResizeLane ln(cw);
  const long long upi = (maxrows + ln.rpb - 1) / ln.rpb, units = nimg * upi;
  for (long long u = blockIdx.x; u < units; u += gridDim.x) {
    const long long img = u / upi;
    const int r = (int)(u - img * upi) * ln.rpb + ln.rr;
    const int32_t* vt = tab + (img * (cw + ch) + cw) * stride;
    const int32_t* vl = vt + (long long)(ch - 1) * stride;
    const int yfirst = vt[0];
    int rows = vl[0] + vl[1] - yfirst;
    rows = rows > maxrows ? maxrows : rows;
    if (!ln.active || r >= rows) continue;
    const qcn_resize_img_t d = desc[img];
    const uint8_t* row = src + d.offset + (long long)(yfirst + r) * d.w * 3;
    uint8_t* out = mid + img * mid_stride + (long long)r * cw * 3;
    for (int c = ln.c0; c < cw; c += kResizeThreads) {
      const int32_t* ht = tab + (img * (cw + ch) + c) * stride;
      const int n = ht[1];
      const uint8_t* p = row + (long long)ht[0] * 3;
      int a0 = 1 << (kResizePrecisionBits - 1), a1 = a0, a2 = a0;
      for (int i = 0; i < n; ++i) {
        const int k = ht[2 + i];
        a0 += (int)p[3 * i] * k;
        a1 += (int)p[3 * i + 1] * k;
        a2 += (int)p[3 * i + 2] * k;
      }
      out[3 * c] = resize_clip8(a0);
      out[3 * c + 1] = resize_clip8(a1);
      out[3 * c + 2] = resize_clip8(a2);
    }
  }
}

// Vertical pass: y[img][oy][c][0..3) from the intermediate's rows
// ymin - yfirst + i.
__global__ __launch_bounds__(kResizeThreads) void resize_v_kernel(
    const uint8_t* __restrict__ mid, long long mid_stride, long long nimg, int ch, int cw, int stride,
    const int32_t* __restrict__ tab, uint8_t* __restrict__ y, int maxrows) {
  const ResizeLane ln(cw);
  const long long upi = (ch + ln.rpb - 1) / ln.rpb, units = nimg * upi;
  const long long pitch = (long long)cw * 3;
  for (long long u = blockIdx.x; u < units; u += gridDim.x) {
    const long long img = u / upi;
    const int oy = (int)(u - img * upi) * ln.rpb + ln.rr;
    if (!ln.active || oy >= ch) continue;
    const int32_t* vt = tab + (img * (cw + ch) + cw) * stride;
    const int32_t* rec = vt + (long long)oy * stride;
    const int r0 = rec[0] - vt[0];
    int n = rec[1];
    n = r0 + n > maxrows ? maxrows - r0 : n;   // never taken (the host's row bound)
    const uint8_t* base = mid + img * mid_stride + (long long)r0 * pitch;
    uint8_t* out = y + (img * ch + oy) * pitch;
    for (int c = ln.c0; c < cw; c += kResizeThreads) {
      const uint8_t* p = base + 3 * c;
      int a0 = 1 << (kResizePrecisionBits - 1), a1 = a0, a2 = a0;
      for (int i = 0; i < n; ++i) {
        const int k = rec[2 + i];
        a0 += (int)p[i * pitch] * k;
        a1 += (int)p[i * pitch + 1] * k;
        a2 += (int)p[i * pitch + 2] * k;
      }
      out[3 * c] = resize_clip8(a0);
      out[3 * c + 1] = resize_clip8(a1);
      out[3 * c + 2] = resize_clip8(a2);
    }
  }
}

struct ResizePlan {
  int stride;            // int32 words per tap record: 2 + the most taps, rounded up to 4
  int maxrows;           // intermediate rows per image (the batch's largest)
  long long tab_bytes;   // the tables, 16-byte aligned
  long long mid_stride;  // intermediate bytes per image, rounded up to 16
  long long total;
};

// (int)ceil(support) * 2 + 1 taps at most on an axis (Pillow's ksize).
static int resize_axis(int in, int out, int* ksize, double* scale_out) {
  const double scale = (double)in / (double)out;
  if (ceil(scale) > kResizeMaxScale) return QCN_ERR_UNSUPPORTED;
  const double support = scale > 1.0 ? scale : 1.0;
  *ksize = (int)ceil(support) * 2 + 1;
  *scale_out = scale;
  return QCN_OK;
}

// Host only: validates the descriptors and sizes the workspace.
// src_bytes < 0: no source to check against.
static int resize_check(const qcn_resize_img_t* d, int nimg, int ch, int cw, long long src_bytes,
                        ResizePlan* p) {
  if (!d || nimg < 0 || ch < 1 || cw < 1) return QCN_ERR_ARG;
  int kmax = 1;
  long long maxrows = 1;
  for (int i = 0; i < nimg; ++i) {
    const qcn_resize_img_t& e = d[i];
    if (e.h < 1 || e.w < 1 || e.oh < 1 || e.ow < 1 || e.offset < 0) return QCN_ERR_ARG;
    if (e.top < 0 || e.left < 0 || (long long)e.top + ch > e.oh || (long long)e.left + cw > e.ow)
      return QCN_ERR_ARG;
    const long long bytes = (long long)e.h * e.w * 3;
    if (src_bytes >= 0 && (e.offset > src_bytes || bytes > src_bytes - e.offset)) return QCN_ERR_ARG;
    int kh = 0, kv = 0;
    double sh = 0.0, sv = 0.0;
    if (resize_axis(e.w, e.ow, &kh, &sh) != QCN_OK || resize_axis(e.h, e.oh, &kv, &sv) != QCN_OK)
      return QCN_ERR_UNSUPPORTED;
    kmax = kh > kmax ? kh : kmax;
    kmax = kv > kmax ? kv : kmax;
    const double support = sv > 1.0 ? sv : 1.0;
    long long rows = (long long)floor((double)(ch - 1) * sv + 2.0 * support) + 2;
    rows = rows > e.h ? e.h : rows;
    maxrows = rows > maxrows ? rows : maxrows;
  }
  p->stride = (2 + kmax + 3) & ~3;
  p->maxrows = (int)maxrows;
  p->tab_bytes = (long long)nimg * ((long long)cw + ch) * p->stride * 4;
  p->mid_stride = (maxrows * cw * 3 + 15) & ~15ll;
  p->total = p->tab_bytes + (long long)nimg * p->mid_stride;
  return QCN_OK;
}

static unsigned resize_grid(long long work, int ncu) {
  const long long cap = (long long)ncu * kResizeBlocksPerCu;
  return (unsigned)(work < cap ? (work < 1 ? 1 : work) : cap);
}

}  // namespace qcn

extern "C" long long qcn_resize_crop_workspace_size(const qcn_resize_img_t* desc_host, int nimg, int ch,
                                                    int cw) {
  qcn::ResizePlan p;
  const int rc = qcn::resize_check(desc_host, nimg, ch, cw, -1, &p);
  return rc != QCN_OK ? (long long)rc : p.total;
}

extern "C" int qcn_resize_crop_tap_stride(const qcn_resize_img_t* desc_host, int nimg, int ch, int cw) {
  qcn::ResizePlan p;
  const int rc = qcn::resize_check(desc_host, nimg, ch, cw, -1, &p);
  return rc != QCN_OK ? rc : p.stride;
}

extern "C" int qcn_resize_crop_u8_hwc(const uint8_t* src, long long src_bytes,
                                      const qcn_resize_img_t* desc_host,
                                      const qcn_resize_img_t* desc_dev, int nimg, int ch, int cw,
                                      uint8_t* y, void* workspace, void* stream) {
  using namespace qcn;
  if (!src || !desc_host || !desc_dev || !y || !workspace || src_bytes < 0) return QCN_ERR_ARG;
  ResizePlan p;
  const int rc = resize_check(desc_host, nimg, ch, cw, src_bytes, &p);
  if (rc != QCN_OK) return rc;
  if ((reinterpret_cast<uintptr_t>(workspace) & 15) || (reinterpret_cast<uintptr_t>(desc_dev) & 7))
    return QCN_ERR_ARG;
  if (nimg == 0) return QCN_OK;
  const int ncu = qcn_cu_count();
  if (ncu <= 0) return QCN_ERR_HIP;
  hipStream_t s = (hipStream_t)stream;
  int32_t* tab = reinterpret_cast<int32_t*>(workspace);
  uint8_t* mid = reinterpret_cast<uint8_t*>(workspace) + p.tab_bytes;
  const long long n = nimg;
  const int rpb = cw < kResizeThreads ? kResizeThreads / cw : 1;

  const long long recs = n * ((long long)cw + ch);
  hipLaunchKernelGGL(resize_taps_kernel, dim3(resize_grid((recs + kResizeThreads - 1) / kResizeThreads, ncu)),
                     dim3(kResizeThreads), 0, s, desc_dev, n, ch, cw, p.stride, tab);
  hipLaunchKernelGGL(resize_h_kernel, dim3(resize_grid(n * ((p.maxrows + rpb - 1) / rpb), ncu)),
                     dim3(kResizeThreads), 0, s, src, desc_dev, n, ch, cw, p.stride, tab, mid, p.mid_stride,
                     p.maxrows);
  hipLaunchKernelGGL(resize_v_kernel, dim3(resize_grid(n * ((ch + rpb - 1) / rpb), ncu)),
                     dim3(kResizeThreads), 0, s, mid, p.mid_stride, n, ch, cw, p.stride, tab, y, p.maxrows);
  return hipGetLastError() == hipSuccess ? QCN_OK : QCN_ERR_HIP;
}
