// HistogramObserver's device half: torch.histc of an fp32 activation over the
// running [min, max] that qcn_minmax_f32 has just left in device memory.
//
// Bin of an element v with lo <= v <= hi (ATen's CPU histc, every op IEEE fp32,
// the division correctly rounded — keep the plain '/', no reciprocal):
//   bin = min(int(((v - lo) / (hi - lo)) * bins), bins - 1)
// lo == hi widens the range to [lo - 1, hi + 1]; elements outside the range
// (and NaN) are skipped, so the reset state [+inf, -inf] counts nothing.
// bins is a power of two: the multiply is exact.
//
// Counts are exact uint32 integers.  torch.histc counts in fp32 per thread, so
// a bin above 2^24 saturates there and depends on its thread count; the two
// agree while every bin stays below 2^24 (the tests keep it so).
//
// Shape: a persistent grid sized from the CU count; each lane loads 16 B;
// every wave owns a private uint32[bins] copy in LDS (no cross-wave traffic
// until the flush); one flush per workgroup adds the non-zero bins to global
// memory with integer atomics, so the result does not depend on the order.
//
// Hot bin: post-ReLU tensors put about half of all elements on exactly lo,
// i.e. bin 0, and a per-lane LDS atomic would serialise on that one address.
// A lane whose left neighbour (within its row of 16) holds the same bin marks
// a repeated bin; while such a lane exists, the lanes that share its bin are
// balloted out and their popcount is added once.  A bin held by many lanes
// has an adjacent pair almost surely; spread-out data has none and pays one
// DPP move and one ballot before the plain per-lane atomics.
#include "common.hpp"
#include "qconvnet_abi.hpp"

namespace qcn {

constexpr int kHistThreads = 256;
constexpr int kHistWaves = kHistThreads / 64;
constexpr int kHistUnroll = 4;        // float4 loads in flight per lane
constexpr int kHistBlocksPerCu = 4;   // 4 x 32 KB of LDS at bins = 2048

QCN_DEV int histc_bin(float v, float lo, float hi, float range, float fbins, int last) {
  if (!(v >= lo && v <= hi)) return -1;
  const int b = (int)(((v - lo) / range) * fbins);
  return b < 0 ? 0 : (b < last ? b : last);   // < 0 only if the range overflowed fp32
}

// One wave-wide step: every lane brings one bin (-1: nothing to count).
QCN_DEV void hist_add(uint32_t* h, int bin, int lane) {
  // bin of lane - 1 within the row of 16; the row's first lane keeps -2
  const int left = __builtin_amdgcn_update_dpp(-2, bin, 0x111 /* row_shr:1 */, 0xf, 0xf, false);
  unsigned long long live = __ballot(bin >= 0);
  unsigned long long rep = __ballot(bin >= 0 && bin == left);
  while (rep) {
    const int leader = __builtin_ctzll(rep);
    const int b = __builtin_amdgcn_readlane(bin, leader);
    const unsigned long long same = __ballot(bin == b);
    if (lane == leader) atomicAdd(&h[b], (uint32_t)__builtin_popcountll(same));
    live &= ~same;
    rep &= ~same;
  }
  if ((live >> lane) & 1) atomicAdd(&h[bin], 1u);
}

// xa: x advanced past `head` scalar elements to a 16-B boundary; n4 float4s
// follow, then `tail` scalars.  head, tail <= 3.
__global__ __launch_bounds__(kHistThreads) void histc_kernel(
    const float* __restrict__ x, int head, long long n4, int tail,
    const float* __restrict__ minmax, int bins, uint32_t* __restrict__ hist) {
  extern __shared__ uint32_t s_hist[];   // [kHistWaves][bins]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < kHistWaves * bins; i += kHistThreads) s_hist[i] = 0;
  __syncthreads();

  float lo = minmax[0], hi = minmax[1];
  if (lo == hi) {
    lo = lo - 1.0f;
    hi = hi + 1.0f;
  }
  const float range = hi - lo, fbins = (float)bins;
  const int last = bins - 1;
  uint32_t* h = s_hist + wave * bins;

  const float4* x4 = reinterpret_cast<const float4*>(x + head);
  const long long stride = (long long)gridDim.x * kHistThreads;
  // `base` is uniform over the workgroup, so every lane of a wave reaches the
  // ballots in hist_add together; lanes past the end bring bin -1
  for (long long base = (long long)blockIdx.x * kHistThreads; base < n4;
       base += stride * kHistUnroll) {
    float4 v[kHistUnroll];
    bool ok[kHistUnroll];
#pragma unroll
    for (int u = 0; u < kHistUnroll; ++u) {
      const long long i = base + u * stride + tid;
      ok[u] = i < n4;
      v[u] = ok[u] ? x4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int u = 0; u < kHistUnroll; ++u) {
      if (base + u * stride >= n4) break;   // uniform
      hist_add(h, ok[u] ? histc_bin(v[u].x, lo, hi, range, fbins, last) : -1, lane);
      hist_add(h, ok[u] ? histc_bin(v[u].y, lo, hi, range, fbins, last) : -1, lane);
      hist_add(h, ok[u] ? histc_bin(v[u].z, lo, hi, range, fbins, last) : -1, lane);
      hist_add(h, ok[u] ? histc_bin(v[u].w, lo, hi, range, fbins, last) : -1, lane);
    }
  }
  // the scalar head and tail (at most 3 + 3 elements): one step of one wave
  if (blockIdx.x == 0 && wave == 0 && head + tail > 0) {
    int bin = -1;
    if (lane < head + tail) {
      const long long i = lane < head ? lane : head + n4 * 4 + (lane - head);
      bin = histc_bin(x[i], lo, hi, range, fbins, last);
    }
    hist_add(h, bin, lane);
  }
  __syncthreads();
  for (int b = tid; b < bins; b += kHistThreads) {
    uint32_t c = 0;
#pragma unroll
    for (int w = 0; w < kHistWaves; ++w) c += s_hist[w * bins + b];
    if (c) atomicAdd(&hist[b], c);
  }
}

}  // namespace qcn

extern "C" int qcn_histc_f32(const float* x, long long count, const float* minmax, int bins,
                             uint32_t* hist, void* stream) {
  if (!x || !minmax || !hist || count < 0 || count >= (1LL << 32)) return QCN_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(x) & 3) || (reinterpret_cast<uintptr_t>(minmax) & 3) ||
      (reinterpret_cast<uintptr_t>(hist) & 3))
    return QCN_ERR_ARG;
  if (bins < 16 || bins > 4096 || (bins & (bins - 1))) return QCN_ERR_UNSUPPORTED;
  if (count == 0) return QCN_OK;
  long long head = ((16 - (long long)(reinterpret_cast<uintptr_t>(x) & 15)) & 15) / 4;
  if (head > count) head = count;
  const long long n4 = (count - head) / 4;
  const int tail = (int)(count - head - n4 * 4);
  const int ncu = qcn_cu_count();
  if (ncu <= 0) return QCN_ERR_HIP;
  long long grid = (n4 + qcn::kHistThreads - 1) / qcn::kHistThreads;
  const long long cap = (long long)ncu * qcn::kHistBlocksPerCu;
  grid = grid < 1 ? 1 : (grid > cap ? cap : grid);
  const size_t lds = (size_t)qcn::kHistWaves * bins * sizeof(uint32_t);   // <= 64 KB
  hipLaunchKernelGGL(qcn::histc_kernel, dim3((unsigned)grid), dim3(qcn::kHistThreads), lds,
                     (hipStream_t)stream, x, (int)head, n4, tail, minmax, bins, hist);
  return hipGetLastError() == hipSuccess ? QCN_OK : QCN_ERR_HIP;
}
