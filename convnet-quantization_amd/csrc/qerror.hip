// The quantization-error report's device half: per-channel signal, error and
// clipping statistics of a u8 activation q (qparams scale, zp) against its
// fp32 reference x, both read once.
//
// Per element (IEEE fp32 unless it says double; nothing is contracted):
//   d    = scale * float(int(q) - zp)                       (A7, dequantize)
//   lo   = scale * float(0 - zp),  hi = scale * float(255 - zp)
//   qref = clamp(zp + rne(x * inv), 0, 255), inv = 1.0f / scale   (A1, quantize)
//   e    = double(x) - double(d)
// Per channel: counts[5] = { elements, #(x < lo), #(x > hi), #(qref != q),
// bits of max fabsf(x - d) }, sums[3] = { sum double(x)^2, sum e^2, sum |e| }.
//
// Shape.  x is NCHW, so with P = n * h * w pixels it is, image by image, a
// [c][hw] matrix; an NHWC q is one [P][c] matrix.  Work is cut into units:
// (a group of TC channels) x (a slice of the pixel range), one workgroup per
// unit, TC = 64, 16 or 4 by the channel count.  A unit walks its slice in
// tiles of TC channels x TP = 4096 / TC pixels:
//   tile kernel (h*w > 1 and c > 1): x is loaded with lanes along the pixels
//   (float4 where hw % 4 == 0 and x is 16-B aligned) and written to LDS as
//   [channel][pixel]; an NHWC q tile is copied to LDS as it lies in memory
//   (uint4 where aligned), an NCHW q tile goes the way x goes.  Then thread
//   (channel = tid % TC, slot = tid / TC) reads its channel's pixels slot,
//   slot + 256 / TC, ... : the x column read has a row stride that is odd in
//   units of the lanes per channel, the q bytes of neighbouring lanes share
//   dwords, so neither read has bank conflicts at TC = 64 or 16.
//   direct kernel (h*w == 1, or c == 1): x and q have the same [P][c] layout,
//   the same thread mapping reads both straight from memory, lanes along the
//   channels (along the pixels at c == 1); no LDS tile, no transpose.
// A thread keeps one channel for the whole unit, so its three double sums and
// four integers stay in registers until the unit ends; the 256 / TC slots of a
// channel are then added in slot order through LDS and the unit's record goes
// to the workspace: [slice][field][channel], doubles first, uint32 after.
//
// Determinism: no floating-point atomics.  The finishing kernel adds a
// channel's slice records in a fixed tree (64 strided runs in slice order,
// the 64 runs in run order) and adds the total into sums with a plain
// read-modify-write; the integer fields go into counts with 64-bit atomicAdd
// / atomicMax.  Slices, tiles and the tree depend on the shape alone, so the
// same calls on one stream give the same bits.
#include "common.hpp"
#include "qconvnet_abi.hpp"

#include <math.h>

namespace qcn {

constexpr int kQerrThreads = 256;
constexpr int kQerrTile = 4096;       // elements per tile: TC channels x TP pixels
constexpr int kQerrSlices = 512;      // pixel slices (workgroups per channel group) at most
constexpr int kQerrMaxC = 65536;
constexpr int kQerrRecBytes = 3 * 8 + 4 * 4;   // a (slice, channel) record
constexpr int kQerrFinCh = 4, kQerrFinWays = 64;
constexpr int kQerrXsMax = 64 * 65;   // floats of the x tile at its widest (TC = 64)
constexpr int kQerrQsMax = kQerrTile + 4 * 64;

struct QerrParams {
  const float* x;
  const uint8_t* q;
  int c, hw, ptot;       // channels, h * w, n * h * w
  int slices, tiles;     // pixel slices, pixel tiles of TP
  int cpad;              // channel groups * TC
  int nhwc, vecx, vecq;
  float scale, inv, lo, hi;
  int zp;
  double* wd;            // [slices][3][cpad]
  uint32_t* wi;          // [slices][4][cpad]
};

static inline int qerr_tc(int c) { return c == 1 ? 1 : (c <= 4 ? 4 : (c <= 16 ? 16 : 64)); }

struct QerrShape {
  int tc, cg, cpad, tiles, slices;
};
static inline QerrShape qerr_shape(int c, long long ptot) {
  QerrShape s;
  s.tc = qerr_tc(c);
  s.cg = (c + s.tc - 1) / s.tc;
  s.cpad = s.cg * s.tc;
  const int tp = kQerrTile / s.tc;
  s.tiles = (int)((ptot + tp - 1) / tp);
  s.slices = s.tiles < kQerrSlices ? s.tiles : kQerrSlices;
  return s;
}

struct QerrAcc {
  double x2, e2, ae;
  uint32_t below, above, differ, maxb;
  QCN_DEV void clear() {
    x2 = e2 = ae = 0.0;
    below = above = differ = maxb = 0u;
  }
  QCN_DEV void add(float xv, int qv, const QerrParams& a) {
    const float d = a.scale * (float)(qv - a.zp);
    below += (uint32_t)(xv < a.lo);
    above += (uint32_t)(xv > a.hi);
    float t = xv * a.inv;
    t = fminf(fmaxf(t, -1.0e9f), 1.0e9f);   // keeps the int conversion defined
    int qr = (int)__builtin_rintf(t) + a.zp;
    qr = qr < 0 ? 0 : (qr > 255 ? 255 : qr);
    differ += (uint32_t)(qr != qv);
    const uint32_t eb = __float_as_uint(fabsf(xv - d));
    maxb = eb > maxb ? eb : maxb;
    const double xd = (double)xv, e = xd - (double)d;
    x2 += xd * xd;
    e2 += e * e;
    ae += fabs(e);
  }
};

// Add the slots of every channel in slot order and write the unit's record.
// `red` holds at least kQerrThreads * kQerrRecBytes bytes and is free.
template <int TC>
QCN_DEV void qerr_flush(const QerrAcc& acc, void* red, int tid, int slice, int ch0,
                        const QerrParams& a) {
  double* rd = reinterpret_cast<double*>(red);                      // [3][256]
  uint32_t* ri = reinterpret_cast<uint32_t*>(rd + 3 * kQerrThreads);   // [4][256]
  rd[tid] = acc.x2;
  rd[kQerrThreads + tid] = acc.e2;
  rd[2 * kQerrThreads + tid] = acc.ae;
  ri[tid] = acc.below;
  ri[kQerrThreads + tid] = acc.above;
  ri[2 * kQerrThreads + tid] = acc.differ;
  ri[3 * kQerrThreads + tid] = acc.maxb;
  __syncthreads();
  if (tid < TC) {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    uint32_t b = 0, ab = 0, df = 0, mx = 0;
    for (int t = tid; t < kQerrThreads; t += TC) {   // slot order
      s0 += rd[t];
      s1 += rd[kQerrThreads + t];
      s2 += rd[2 * kQerrThreads + t];
      b += ri[t];
      ab += ri[kQerrThreads + t];
      df += ri[2 * kQerrThreads + t];
      const uint32_t m = ri[3 * kQerrThreads + t];
      mx = m > mx ? m : mx;
    }
    const size_t ch = (size_t)ch0 + tid, cp = (size_t)a.cpad;   // ch < cpad
    double* wd = a.wd + (size_t)slice * 3 * cp + ch;
    wd[0] = s0;
    wd[cp] = s1;
    wd[2 * cp] = s2;
    uint32_t* wi = a.wi + (size_t)slice * 4 * cp + ch;
    wi[0] = b;
    wi[cp] = ab;
    wi[2 * cp] = df;
    wi[3 * cp] = mx;
  }
}

// h * w > 1 and c > 1.  blockIdx.x = channel group * slices + slice.
template <int TC>
__global__ __launch_bounds__(kQerrThreads) void qerror_tile_kernel(QerrParams a) {
  constexpr int TP = kQerrTile / TC, NSLOT = kQerrThreads / TC;
  constexpr int XS = TP + (TC >= 32 ? 1 : 32 / TC);   // x tile row stride (floats)
  constexpr int QS = TP + 4;                          // NCHW q tile row stride (bytes)
  static_assert(TC * XS <= kQerrXsMax && TC * QS <= kQerrQsMax, "LDS tiles");
  static_assert(kQerrXsMax * 4 >= kQerrThreads * kQerrRecBytes, "the flush reuses the x tile");
  __shared__ __attribute__((aligned(16))) float sx[kQerrXsMax];
  __shared__ __attribute__((aligned(16))) uint8_t sq[kQerrQsMax];
  const int tid = threadIdx.x;
  const int slice = (int)(blockIdx.x % (unsigned)a.slices);
  const int ch0 = (int)(blockIdx.x / (unsigned)a.slices) * TC;
  const int nch = a.c - ch0 < TC ? a.c - ch0 : TC;
  const int t0 = (int)((long long)slice * a.tiles / a.slices);
  const int t1 = (int)((long long)(slice + 1) * a.tiles / a.slices);
  const bool whole_rows = a.c <= TC;   // one channel group: an NHWC q tile is one byte range
  const int qstride = whole_rows ? a.c : TC;
  const int chl = tid % TC, slot = tid / TC;
  const unsigned hw = (unsigned)a.hw;
  QerrAcc acc;
  acc.clear();

  for (int t = t0; t < t1; ++t) {
    const int p0 = t * TP;   // < ptot < 2^31
    const int npix = a.ptot - p0 < TP ? a.ptot - p0 : TP;
    // ---- x: lanes along the pixels, LDS [channel][pixel]
    if (a.vecx) {   // hw % 4 == 0: four pixels of a lane stay in one image
      constexpr int J = TP / 4, ITEMS = TC * J / kQerrThreads;
      float4 v[ITEMS];
#pragma unroll
      for (int u = 0; u < ITEMS; ++u) {
        const int i = u * kQerrThreads + tid, r = i / J, j = i % J;
        const unsigned p = (unsigned)p0 + 4u * j;
        v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < nch && 4 * j < npix) {
          const unsigned img = p / hw, off = p - img * hw;
          v[u] = *reinterpret_cast<const float4*>(
              a.x + ((size_t)img * a.c + (ch0 + r)) * hw + off);
        }
      }
#pragma unroll
      for (int u = 0; u < ITEMS; ++u) {
        const int i = u * kQerrThreads + tid, r = i / J, j = i % J;
        float* dst = sx + r * XS + 4 * j;
        dst[0] = v[u].x;
        dst[1] = v[u].y;
        dst[2] = v[u].z;
        dst[3] = v[u].w;
      }
    } else {
      constexpr int U = 4;
      for (int b = 0; b < kQerrTile; b += U * kQerrThreads) {
        float v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int i = b + u * kQerrThreads + tid, r = i / TP, j = i % TP;
          const unsigned p = (unsigned)p0 + j;
          v[u] = 0.f;
          if (r < nch && j < npix) {
            const unsigned img = p / hw, off = p - img * hw;
            v[u] = a.x[((size_t)img * a.c + (ch0 + r)) * hw + off];
          }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int i = b + u * kQerrThreads + tid;
          sx[(i / TP) * XS + i % TP] = v[u];
        }
      }
    }
    // ---- q
    if (a.nhwc) {
      // rows of `rowlen` bytes, `gstride` apart in memory and `qstride` in LDS
      const int nrows = whole_rows ? 1 : npix;
      const int rowlen = whole_rows ? npix * a.c : nch;
      const uint8_t* src = a.q + (size_t)p0 * a.c + (whole_rows ? 0 : ch0);
      const int n16 = a.vecq ? rowlen / 16 : 0;
      for (int i = tid; i < nrows * n16; i += kQerrThreads) {
        const int r = i / n16, j = i % n16;
        *reinterpret_cast<uint4*>(sq + r * qstride + 16 * j) =
            *reinterpret_cast<const uint4*>(src + (size_t)r * a.c + 16 * j);
      }
      const int rest = rowlen - 16 * n16;
      for (int i = tid; i < nrows * rest; i += kQerrThreads) {
        const int r = i / rest, j = 16 * n16 + i % rest;
        sq[r * qstride + j] = src[(size_t)r * a.c + j];
      }
    } else if (a.vecq) {   // NCHW q, hw % 16 == 0: sixteen pixels of a lane stay in one image
      constexpr int J = TP / 16;
      for (int i = tid; i < TC * J; i += kQerrThreads) {
        const int r = i / J, j = i % J;
        const unsigned p = (unsigned)p0 + 16u * j;
        if (r < nch && 16 * j < npix) {
          const unsigned img = p / hw, off = p - img * hw;
          const uint4 v = *reinterpret_cast<const uint4*>(
              a.q + ((size_t)img * a.c + (ch0 + r)) * hw + off);
          uint32_t* dst = reinterpret_cast<uint32_t*>(sq + r * QS + 16 * j);
          dst[0] = v.x;
          dst[1] = v.y;
          dst[2] = v.z;
          dst[3] = v.w;
        }
      }
    } else {
      for (int i = tid; i < kQerrTile; i += kQerrThreads) {
        const int r = i / TP, j = i % TP;
        const unsigned p = (unsigned)p0 + j;
        if (r < nch && j < npix) {
          const unsigned img = p / hw, off = p - img * hw;
          sq[r * QS + j] = a.q[((size_t)img * a.c + (ch0 + r)) * hw + off];
        }
      }
    }
    __syncthreads();
    // ---- score: a thread keeps its channel
    if (chl < nch) {
      const float* xr = sx + chl * XS;
      const uint8_t* qr = a.nhwc ? sq + chl : sq + chl * QS;
      const int qstep = a.nhwc ? qstride : 1;
#pragma unroll 4
      for (int pix = slot; pix < npix; pix += NSLOT) acc.add(xr[pix], (int)qr[pix * qstep], a);
    }
    __syncthreads();
  }
  qerr_flush<TC>(acc, sx, tid, slice, ch0, a);
}

// h * w == 1 or c == 1: x and q are both [ptot][c]; no tile, no transpose.
template <int TC>
__global__ __launch_bounds__(kQerrThreads) void qerror_direct_kernel(QerrParams a) {
  constexpr int TP = kQerrTile / TC, NSLOT = kQerrThreads / TC, U = 4;
  __shared__ __attribute__((aligned(16))) uint8_t red[kQerrThreads * kQerrRecBytes];
  const int tid = threadIdx.x;
  const int slice = (int)(blockIdx.x % (unsigned)a.slices);
  const int ch0 = (int)(blockIdx.x / (unsigned)a.slices) * TC;
  const int t0 = (int)((long long)slice * a.tiles / a.slices);
  const int t1 = (int)((long long)(slice + 1) * a.tiles / a.slices);
  const int chl = tid % TC, slot = tid / TC, ch = ch0 + chl;
  QerrAcc acc;
  acc.clear();
  if (ch < a.c) {
    const long long pa = (long long)t0 * TP;
    long long pb = (long long)t1 * TP;
    pb = pb < a.ptot ? pb : a.ptot;
    const float* xc = a.x + ch;
    const uint8_t* qc = a.q + ch;
    for (long long p = pa + slot; p < pb; p += (long long)U * NSLOT) {
      float xv[U];
      int qv[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const long long pu = p + (long long)u * NSLOT;
        const bool ok = pu < pb;
        xv[u] = ok ? xc[(size_t)pu * a.c] : 0.f;
        qv[u] = ok ? (int)qc[(size_t)pu * a.c] : 0;
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (p + (long long)u * NSLOT < pb) acc.add(xv[u], qv[u], a);
    }
  }
  qerr_flush<TC>(acc, red, tid, slice, ch0, a);
}

// One workgroup per kQerrFinCh channels: thread (channel, way) adds the slice
// records way, way + 64, ... in that order, then way 0's thread adds the 64
// ways in way order.  The tree is a function of `slices` alone.  Many ways and
// few channels per workgroup: a way's records are dependent-latency loads, and
// 512 slices are 8 of them per thread instead of 32.
__global__ __launch_bounds__(kQerrFinCh* kQerrFinWays) void qerror_finish_kernel(
    const double* __restrict__ wd, const uint32_t* __restrict__ wi, int slices, int c, int cpad,
    long long per_channel, unsigned long long* __restrict__ counts, double* __restrict__ sums) {
  __shared__ double sd[3][kQerrFinWays][kQerrFinCh];
  __shared__ unsigned long long si[3][kQerrFinWays][kQerrFinCh];
  __shared__ uint32_t sm[kQerrFinWays][kQerrFinCh];
  const int chl = threadIdx.x % kQerrFinCh, way = threadIdx.x / kQerrFinCh;
  const int ch = blockIdx.x * kQerrFinCh + chl;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  unsigned long long b = 0, ab = 0, df = 0;
  uint32_t mx = 0;
  if (ch < c) {
    const size_t cp = (size_t)cpad;
#pragma unroll 4   // four records' loads in flight; the adds keep their order
    for (int s = way; s < slices; s += kQerrFinWays) {
      const double* d = wd + (size_t)s * 3 * cp + ch;
      const uint32_t* u = wi + (size_t)s * 4 * cp + ch;
      s0 += d[0];
      s1 += d[cp];
      s2 += d[2 * cp];
      b += u[0];
      ab += u[cp];
      df += u[2 * cp];
      const uint32_t m = u[3 * cp];
      mx = m > mx ? m : mx;
    }
  }
  sd[0][way][chl] = s0;
  sd[1][way][chl] = s1;
  sd[2][way][chl] = s2;
  si[0][way][chl] = b;
  si[1][way][chl] = ab;
  si[2][way][chl] = df;
  sm[way][chl] = mx;
  __syncthreads();
  if (way == 0 && ch < c) {
    s0 = s1 = s2 = 0.0;
    b = ab = df = 0;
    mx = 0;
    for (int w = 0; w < kQerrFinWays; ++w) {
      s0 += sd[0][w][chl];
      s1 += sd[1][w][chl];
      s2 += sd[2][w][chl];
      b += si[0][w][chl];
      ab += si[1][w][chl];
      df += si[2][w][chl];
      mx = sm[w][chl] > mx ? sm[w][chl] : mx;
    }
    double* so = sums + (size_t)ch * 3;
    so[0] += s0;
    so[1] += s1;
    so[2] += s2;
    unsigned long long* co = counts + (size_t)ch * 5;
    atomicAdd(&co[0], (unsigned long long)per_channel);
    if (b) atomicAdd(&co[1], b);
    if (ab) atomicAdd(&co[2], ab);
    if (df) atomicAdd(&co[3], df);
    if (mx) atomicMax(&co[4], (unsigned long long)mx);
  }
}

template <int TC>
static void qerr_launch(const QerrParams& a, bool direct, unsigned grid, hipStream_t st) {
  if constexpr (TC == 1) {   // c == 1 is always direct
    hipLaunchKernelGGL(qerror_direct_kernel<1>, dim3(grid), dim3(kQerrThreads), 0, st, a);
  } else {
    if (direct)
      hipLaunchKernelGGL(qerror_direct_kernel<TC>, dim3(grid), dim3(kQerrThreads), 0, st, a);
    else
      hipLaunchKernelGGL(qerror_tile_kernel<TC>, dim3(grid), dim3(kQerrThreads), 0, st, a);
  }
}

static int qerr_check_shape(int n, int c, int h, int w) {
  if (n < 0 || c < 1 || h < 1 || w < 1) return QCN_ERR_ARG;
  if (c > kQerrMaxC || (long long)h * w >= (1LL << 31) || (long long)n * h * w >= (1LL << 31))
    return QCN_ERR_UNSUPPORTED;
  return QCN_OK;
}

// ---------------------------------------------------------------------------
// fp32 against fp32 (qcn_qerror_f32_f32): the same units, slices, tiles and
// finishing tree as above; a (slice, channel) record is four doubles (sum x^2,
// e^2, |e|, e) and two uint32 (#(x != y), bits of max fabsf(x - y)) — the same
// kQerrRecBytes, so the workspace size is the same function of the shape.
//   tile kernel: x goes through the LDS transpose as above.  An NCHW y goes the
//   same way into a second tile.  An NHWC y is read straight from memory by the
//   scoring thread mapping (lanes along the channels: a wave's 4-byte loads are
//   TC * 4-byte runs, one 256-byte run at TC = 64), all 4096 / 256 = 16 values
//   of a thread issued before x is staged so they land behind the barrier.
//   direct kernel: x and y are both [P][c].
struct QerrFParams {
  const float* x;
  const float* y;
  int c, hw, ptot;
  int slices, tiles;
  int cpad;
  int nhwc, vecx, vecy;
  double* wd;            // [slices][4][cpad]
  uint32_t* wi;          // [slices][2][cpad]
};

struct QerrFAcc {
  double x2, e2, ae, se;
  uint32_t differ, maxb;
  QCN_DEV void clear() {
    x2 = e2 = ae = se = 0.0;
    differ = maxb = 0u;
  }
  QCN_DEV void add(float xv, float yv) {
    differ += (uint32_t)(xv != yv);
    const uint32_t eb = __float_as_uint(fabsf(xv - yv));
    maxb = eb > maxb ? eb : maxb;
    const double xd = (double)xv, e = xd - (double)yv;
    x2 += xd * xd;
    e2 += e * e;
    ae += fabs(e);
    se += e;
  }
};

static_assert(4 * 8 + 2 * 4 == kQerrRecBytes, "both record forms share the workspace size");

// As qerr_flush, for the fp32 record.
template <int TC>
QCN_DEV void qerrf_flush(const QerrFAcc& acc, void* red, int tid, int slice, int ch0,
                         const QerrFParams& a) {
  double* rd = reinterpret_cast<double*>(red);                         // [4][256]
  uint32_t* ri = reinterpret_cast<uint32_t*>(rd + 4 * kQerrThreads);   // [2][256]
  rd[tid] = acc.x2;
  rd[kQerrThreads + tid] = acc.e2;
  rd[2 * kQerrThreads + tid] = acc.ae;
  rd[3 * kQerrThreads + tid] = acc.se;
  ri[tid] = acc.differ;
  ri[kQerrThreads + tid] = acc.maxb;
  __syncthreads();
  if (tid < TC) {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    uint32_t df = 0, mx = 0;
    for (int t = tid; t < kQerrThreads; t += TC) {   // slot order
      s0 += rd[t];
      s1 += rd[kQerrThreads + t];
      s2 += rd[2 * kQerrThreads + t];
      s3 += rd[3 * kQerrThreads + t];
      df += ri[t];
      const uint32_t m = ri[kQerrThreads + t];
      mx = m > mx ? m : mx;
    }
    const size_t ch = (size_t)ch0 + tid, cp = (size_t)a.cpad;   // ch < cpad
    double* wd = a.wd + (size_t)slice * 4 * cp + ch;
    wd[0] = s0;
    wd[cp] = s1;
    wd[2 * cp] = s2;
    wd[3 * cp] = s3;
    uint32_t* wi = a.wi + (size_t)slice * 2 * cp + ch;
    wi[0] = df;
    wi[cp] = mx;
  }
}

// One tile of an NCHW fp32 tensor into LDS as [channel][pixel] (row stride XS),
// lanes along the pixels; rows past nch and pixels past npix are zero.
template <int TC, int XS>
QCN_DEV void qerrf_stage(const float* __restrict__ src, float* s, bool vec, int c, unsigned hw,
                         int ch0, int nch, int p0, int npix, int tid) {
  constexpr int TP = kQerrTile / TC;
  if (vec) {   // hw % 4 == 0: four pixels of a lane stay in one image
    constexpr int J = TP / 4, ITEMS = TC * J / kQerrThreads;
    float4 v[ITEMS];
#pragma unroll
    for (int u = 0; u < ITEMS; ++u) {
      const int i = u * kQerrThreads + tid, r = i / J, j = i % J;
      const unsigned p = (unsigned)p0 + 4u * j;
      v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (r < nch && 4 * j < npix) {
        const unsigned img = p / hw, off = p - img * hw;
        v[u] = *reinterpret_cast<const float4*>(src + ((size_t)img * c + (ch0 + r)) * hw + off);
      }
    }
#pragma unroll
    for (int u = 0; u < ITEMS; ++u) {
      const int i = u * kQerrThreads + tid, r = i / J, j = i % J;
      float* dst = s + r * XS + 4 * j;
      dst[0] = v[u].x;
      dst[1] = v[u].y;
      dst[2] = v[u].z;
      dst[3] = v[u].w;
    }
  } else {
    constexpr int U = 4;
    for (int b = 0; b < kQerrTile; b += U * kQerrThreads) {
      float v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int i = b + u * kQerrThreads + tid, r = i / TP, j = i % TP;
        const unsigned p = (unsigned)p0 + j;
        v[u] = 0.f;
        if (r < nch && j < npix) {
          const unsigned img = p / hw, off = p - img * hw;
          v[u] = src[((size_t)img * c + (ch0 + r)) * hw + off];
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int i = b + u * kQerrThreads + tid;
        s[(i / TP) * XS + i % TP] = v[u];
      }
    }
  }
}

// h * w > 1 and c > 1.  blockIdx.x = channel group * slices + slice.
template <int TC, bool NHWC>
__global__ __launch_bounds__(kQerrThreads) void qerrorf_tile_kernel(QerrFParams a) {
  constexpr int TP = kQerrTile / TC, NSLOT = kQerrThreads / TC, PER = TP / NSLOT;
  constexpr int XS = TP + (TC >= 32 ? 1 : 32 / TC);
  static_assert(TC * XS <= kQerrXsMax, "LDS tiles");
  static_assert(kQerrXsMax * 4 >= kQerrThreads * kQerrRecBytes, "the flush reuses the x tile");
  __shared__ __attribute__((aligned(16))) float sx[kQerrXsMax];
  __shared__ __attribute__((aligned(16))) float sy[NHWC ? 4 : kQerrXsMax];
  const int tid = threadIdx.x;
  const int slice = (int)(blockIdx.x % (unsigned)a.slices);
  const int ch0 = (int)(blockIdx.x / (unsigned)a.slices) * TC;
  const int nch = a.c - ch0 < TC ? a.c - ch0 : TC;
  const int t0 = (int)((long long)slice * a.tiles / a.slices);
  const int t1 = (int)((long long)(slice + 1) * a.tiles / a.slices);
  const int chl = tid % TC, slot = tid / TC;
  const unsigned hw = (unsigned)a.hw;
  QerrFAcc acc;
  acc.clear();

  for (int t = t0; t < t1; ++t) {
    const int p0 = t * TP;   // < ptot < 2^31
    const int npix = a.ptot - p0 < TP ? a.ptot - p0 : TP;
    float yv[PER];
    if constexpr (NHWC) {   // issued first: in flight while x is staged
      const float* yc = a.y + (size_t)p0 * a.c + (ch0 + chl);
#pragma unroll
      for (int k = 0; k < PER; ++k) {
        const int pix = slot + k * NSLOT;
        yv[k] = (chl < nch && pix < npix) ? yc[(size_t)pix * a.c] : 0.f;
      }
    } else {
      qerrf_stage<TC, XS>(a.y, sy, a.vecy, a.c, hw, ch0, nch, p0, npix, tid);
    }
    qerrf_stage<TC, XS>(a.x, sx, a.vecx, a.c, hw, ch0, nch, p0, npix, tid);
    __syncthreads();
    // ---- score: a thread keeps its channel
    if (chl < nch) {
      const float* xr = sx + chl * XS;
#pragma unroll
      for (int k = 0; k < PER; ++k) {
        const int pix = slot + k * NSLOT;
        if (pix < npix) acc.add(xr[pix], NHWC ? yv[k] : sy[chl * XS + pix]);
      }
    }
    __syncthreads();
  }
  qerrf_flush<TC>(acc, sx, tid, slice, ch0, a);
}

// h * w == 1 or c == 1: x and y are both [ptot][c]; no tile, no transpose.
template <int TC>
__global__ __launch_bounds__(kQerrThreads) void qerrorf_direct_kernel(QerrFParams a) {
  constexpr int TP = kQerrTile / TC, NSLOT = kQerrThreads / TC, U = 4;
  __shared__ __attribute__((aligned(16))) uint8_t red[kQerrThreads * kQerrRecBytes];
  const int tid = threadIdx.x;
  const int slice = (int)(blockIdx.x % (unsigned)a.slices);
  const int ch0 = (int)(blockIdx.x / (unsigned)a.slices) * TC;
  const int t0 = (int)((long long)slice * a.tiles / a.slices);
  const int t1 = (int)((long long)(slice + 1) * a.tiles / a.slices);
  const int chl = tid % TC, slot = tid / TC, ch = ch0 + chl;
  QerrFAcc acc;
  acc.clear();
  if (ch < a.c) {
    const long long pa = (long long)t0 * TP;
    long long pb = (long long)t1 * TP;
    pb = pb < a.ptot ? pb : a.ptot;
    const float* xc = a.x + ch;
    const float* yc = a.y + ch;
    for (long long p = pa + slot; p < pb; p += (long long)U * NSLOT) {
      float xv[U], yv[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const long long pu = p + (long long)u * NSLOT;
        const bool ok = pu < pb;
        xv[u] = ok ? xc[(size_t)pu * a.c] : 0.f;
        yv[u] = ok ? yc[(size_t)pu * a.c] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (p + (long long)u * NSLOT < pb) acc.add(xv[u], yv[u]);
    }
  }
  qerrf_flush<TC>(acc, red, tid, slice, ch0, a);
}

// The tree of qerror_finish_kernel over the fp32 record.
__global__ __launch_bounds__(kQerrFinCh* kQerrFinWays) void qerrorf_finish_kernel(
    const double* __restrict__ wd, const uint32_t* __restrict__ wi, int slices, int c, int cpad,
    long long per_channel, unsigned long long* __restrict__ counts, double* __restrict__ sums) {
  __shared__ double sd[4][kQerrFinWays][kQerrFinCh];
  __shared__ unsigned long long si[kQerrFinWays][kQerrFinCh];
  __shared__ uint32_t sm[kQerrFinWays][kQerrFinCh];
  const int chl = threadIdx.x % kQerrFinCh, way = threadIdx.x / kQerrFinCh;
  const int ch = blockIdx.x * kQerrFinCh + chl;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  unsigned long long df = 0;
  uint32_t mx = 0;
  if (ch < c) {
    const size_t cp = (size_t)cpad;
#pragma unroll 4   // four records' loads in flight; the adds keep their order
    for (int s = way; s < slices; s += kQerrFinWays) {
      const double* d = wd + (size_t)s * 4 * cp + ch;
      const uint32_t* u = wi + (size_t)s * 2 * cp + ch;
      s0 += d[0];
      s1 += d[cp];
      s2 += d[2 * cp];
      s3 += d[3 * cp];
      df += u[0];
      const uint32_t m = u[cp];
      mx = m > mx ? m : mx;
    }
  }
  sd[0][way][chl] = s0;
  sd[1][way][chl] = s1;
  sd[2][way][chl] = s2;
  sd[3][way][chl] = s3;
  si[way][chl] = df;
  sm[way][chl] = mx;
  __syncthreads();
  if (way == 0 && ch < c) {
    s0 = s1 = s2 = s3 = 0.0;
    df = 0;
    mx = 0;
    for (int w = 0; w < kQerrFinWays; ++w) {
      s0 += sd[0][w][chl];
      s1 += sd[1][w][chl];
      s2 += sd[2][w][chl];
      s3 += sd[3][w][chl];
      df += si[w][chl];
      mx = sm[w][chl] > mx ? sm[w][chl] : mx;
    }
    double* so = sums + (size_t)ch * 4;
    so[0] += s0;
    so[1] += s1;
    so[2] += s2;
    so[3] += s3;
    unsigned long long* co = counts + (size_t)ch * 3;
    atomicAdd(&co[0], (unsigned long long)per_channel);
    if (df) atomicAdd(&co[1], df);
    if (mx) atomicMax(&co[2], (unsigned long long)mx);
  }
}

template <int TC>
static void qerrf_launch(const QerrFParams& a, bool direct, unsigned grid, hipStream_t st) {
  if constexpr (TC == 1) {   // c == 1 is always direct
    hipLaunchKernelGGL(qerrorf_direct_kernel<1>, dim3(grid), dim3(kQerrThreads), 0, st, a);
  } else {
    if (direct)
      hipLaunchKernelGGL(qerrorf_direct_kernel<TC>, dim3(grid), dim3(kQerrThreads), 0, st, a);
    else if (a.nhwc)
      hipLaunchKernelGGL((qerrorf_tile_kernel<TC, true>), dim3(grid), dim3(kQerrThreads), 0, st, a);
    else
      hipLaunchKernelGGL((qerrorf_tile_kernel<TC, false>), dim3(grid), dim3(kQerrThreads), 0, st, a);
  }
}

}  // namespace qcn

extern "C" long long qcn_qerror_f32_workspace_size(int n, int c, int h, int w) {
  return qcn_qerror_workspace_size(n, c, h, w);   // the records have the same size
}

extern "C" int qcn_qerror_f32_f32(const float* x, const float* y, int n, int c, int h, int w,
                                  int nhwc_y, long long* counts, double* sums, void* workspace,
                                  void* stream) {
  if (!x || !y || !counts || !sums || !workspace) return QCN_ERR_ARG;
  if (((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 3) ||
      ((reinterpret_cast<uintptr_t>(counts) | reinterpret_cast<uintptr_t>(sums) |
        reinterpret_cast<uintptr_t>(workspace)) & 7))
    return QCN_ERR_ARG;
  const int rc = qcn::qerr_check_shape(n, c, h, w);
  if (rc != QCN_OK) return rc;
  if (n == 0) return QCN_OK;
  const int hw = h * w;
  const long long ptot = (long long)n * hw;
  const qcn::QerrShape s = qcn::qerr_shape(c, ptot);
  const bool direct = hw == 1 || c == 1;
  qcn::QerrFParams a;
  a.x = x;
  a.y = y;
  a.c = c;
  a.hw = direct ? 1 : hw;
  a.ptot = (int)ptot;
  a.slices = s.slices;
  a.tiles = s.tiles;
  a.cpad = s.cpad;
  a.nhwc = nhwc_y != 0;
  a.vecx = (reinterpret_cast<uintptr_t>(x) & 15) == 0 && hw % 4 == 0;
  a.vecy = (reinterpret_cast<uintptr_t>(y) & 15) == 0 && hw % 4 == 0;   // NCHW y only
  a.wd = reinterpret_cast<double*>(workspace);
  a.wi = reinterpret_cast<uint32_t*>(a.wd + (size_t)s.slices * 4 * s.cpad);
  hipStream_t st = (hipStream_t)stream;
  const unsigned grid = (unsigned)s.cg * (unsigned)s.slices;
  switch (s.tc) {
    case 1: qcn::qerrf_launch<1>(a, true, grid, st); break;
    case 4: qcn::qerrf_launch<4>(a, direct, grid, st); break;
    case 16: qcn::qerrf_launch<16>(a, direct, grid, st); break;
    default: qcn::qerrf_launch<64>(a, direct, grid, st); break;
  }
  if (hipGetLastError() != hipSuccess) return QCN_ERR_HIP;
  hipLaunchKernelGGL(qcn::qerrorf_finish_kernel,
                     dim3((unsigned)((c + qcn::kQerrFinCh - 1) / qcn::kQerrFinCh)),
                     dim3(qcn::kQerrFinCh * qcn::kQerrFinWays), 0, st, a.wd, a.wi, s.slices, c, s.cpad,
                     ptot, reinterpret_cast<unsigned long long*>(counts), sums);
  return hipGetLastError() == hipSuccess ? QCN_OK : QCN_ERR_HIP;
}

extern "C" long long qcn_qerror_workspace_size(int n, int c, int h, int w) {
  const int rc = qcn::qerr_check_shape(n, c, h, w);
  if (rc != QCN_OK) return rc;
  const qcn::QerrShape s = qcn::qerr_shape(c, (long long)n * h * w);
  return (long long)s.slices * s.cpad * qcn::kQerrRecBytes;
}

extern "C" int qcn_qerror_u8_f32(const float* x, const uint8_t* q, int n, int c, int h, int w,
                                 int nhwc_q, float scale, int zero_point, long long* counts,
                                 double* sums, void* workspace, void* stream) {
  if (!x || !q || !counts || !sums || !workspace) return QCN_ERR_ARG;
  if (zero_point < 0 || zero_point > 255 || !(scale > 0.f) || __builtin_isinf(scale)) return QCN_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(x) & 3) ||
      ((reinterpret_cast<uintptr_t>(counts) | reinterpret_cast<uintptr_t>(sums) |
        reinterpret_cast<uintptr_t>(workspace)) & 7))
    return QCN_ERR_ARG;
  const int rc = qcn::qerr_check_shape(n, c, h, w);
  if (rc != QCN_OK) return rc;
  if (n == 0) return QCN_OK;
  const int hw = h * w;
  const long long ptot = (long long)n * hw;
  const qcn::QerrShape s = qcn::qerr_shape(c, ptot);
  const bool direct = hw == 1 || c == 1;
  const bool x16 = (reinterpret_cast<uintptr_t>(x) & 15) == 0;
  const bool q16 = (reinterpret_cast<uintptr_t>(q) & 15) == 0;
  qcn::QerrParams a;
  a.x = x;
  a.q = q;
  a.c = c;
  a.hw = direct ? 1 : hw;
  a.ptot = (int)ptot;
  a.slices = s.slices;
  a.tiles = s.tiles;
  a.cpad = s.cpad;
  a.nhwc = nhwc_q != 0;
  a.vecx = x16 && hw % 4 == 0;
  // NHWC: a tile of whole rows is one byte range starting at a multiple of 16;
  // otherwise its 64-byte row pieces need c % 16 == 0.  NCHW: 16 pixels of one image
  a.vecq = q16 && (a.nhwc ? (c <= s.tc || c % 16 == 0) : hw % 16 == 0);
  a.scale = scale;
  a.inv = 1.0f / scale;
  a.lo = scale * (float)(0 - zero_point);
  a.hi = scale * (float)(255 - zero_point);
  a.zp = zero_point;
  a.wd = reinterpret_cast<double*>(workspace);
  a.wi = reinterpret_cast<uint32_t*>(a.wd + (size_t)s.slices * 3 * s.cpad);
  hipStream_t st = (hipStream_t)stream;
  const unsigned grid = (unsigned)s.cg * (unsigned)s.slices;
  switch (s.tc) {
    case 1: qcn::qerr_launch<1>(a, true, grid, st); break;
    case 4: qcn::qerr_launch<4>(a, direct, grid, st); break;
    case 16: qcn::qerr_launch<16>(a, direct, grid, st); break;
    default: qcn::qerr_launch<64>(a, direct, grid, st); break;
  }
  if (hipGetLastError() != hipSuccess) return QCN_ERR_HIP;
  hipLaunchKernelGGL(qcn::qerror_finish_kernel, dim3((unsigned)((c + qcn::kQerrFinCh - 1) / qcn::kQerrFinCh)),
                     dim3(qcn::kQerrFinCh * qcn::kQerrFinWays), 0, st, a.wd, a.wi, s.slices, c, s.cpad,
                     ptot, reinterpret_cast<unsigned long long*>(counts), sums);
  return hipGetLastError() == hipSuccess ? QCN_OK : QCN_ERR_HIP;
}
