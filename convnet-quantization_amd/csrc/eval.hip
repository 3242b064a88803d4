// The evaluator's device half: top-1 / top-k hits, per-class totals and
// correct counts, the confusion matrix and the predictions of a batch of fp32
// logits, counted where the logits are.
//
// Order (torch's for max / argmax / topk): NaN above everything and all NaNs
// equal, -0.0 == +0.0, otherwise the usual order with +-inf as values.
// order_key() maps a float to a uint32 whose unsigned order is that preorder.
// For a row x[0..C) with label l:
//   rank = #{ j : x[j] > x[l]  or  (x[j] == x[l] and j < l) }
//   top-k hit iff rank < k, top-1 hit iff rank == 0;
//   pred = the lowest j whose value is maximal.
// A label outside [0, C) makes the row a miss counted in rows and bad_labels
// only.  Every sum is an integer, so the result does not depend on the order
// in which rows, waves or streams arrive.
//
// Shape: a lane group of G = 16, 32 or 64 lanes owns a row (C <= 16, C <= 32,
// above), so a wave scores 4, 2 or 1 rows at once.
//   G < 64: a lane holds one column.  The label and the column are loaded side
//   by side (neither address needs the other), t = x[l] then comes from the
//   label's lane by a shuffle, not from memory.  kEvalUnroll such row sets are
//   loaded before the first is scored, so a workgroup has 4 x its rows in
//   flight and there are 4 x fewer workgroups to flush counters.
//   G = 64: t = x[l] is loaded once, then each lane walks its columns one
//   time — a scalar head up to the first 16-B boundary, float4s, a scalar tail
//   (rows of 1003 floats start off alignment).
// Every lane counts the columns that beat t and keeps its own arg-max; one
// __shfl_xor butterfly inside the group sums the counts and reduces the
// arg-max.
//
// Counting follows observer.hip: rows / top-1 / top-k / bad labels are summed
// per wave by ballot + popcount in registers over the grid-stride loop and
// meet in LDS once; per-class bins live in LDS up to kEvalLdsCols classes and
// are flushed with one global atomic per non-zero bin per workgroup; above
// that, and for the confusion cells (one add per row), the adds go straight
// to global memory.  The flush of every workgroup lands on the same few
// words, so the grid is kept small: see eval_launch.
#include "common.hpp"
#include "qconvnet_abi.hpp"

namespace qcn {

constexpr int kEvalThreads = 256;
constexpr int kEvalWaves = kEvalThreads / 64;
constexpr int kEvalUnroll = 4;        // row sets in flight per step at G < 64
constexpr int kEvalBlocksPerCu = 2;
// LDS class bins up to here.  A workgroup zeroes and flushes 2 * cols bins
// whatever it scored, so the bins pay only while that pass (2 LDS words per
// lane at 256) is small beside the rows a workgroup sees; a wide row (one per
// wave and step) brings at most two class adds, sent to global memory as is.
constexpr int kEvalLdsCols = 256;

QCN_DEV uint32_t order_key(float v) {
  uint32_t b = __float_as_uint(v);
  if ((b & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;   // NaN: the one top key
  if (b == 0x80000000u) b = 0;                               // -0.0 == +0.0
  return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}

struct EvalLane {
  uint32_t kt;   // key of the label's value
  int l;         // the label (-1: none)
  int cnt;       // columns that beat the label's
  uint32_t bk;   // best key so far; 0 is below every real key
  int bi;        // its column
  QCN_DEV void visit(float v, int j) {
    const uint32_t kj = order_key(v);
    cnt += (int)((kj > kt) | ((kj == kt) & (j < l)));
    if (kj > bk || (kj == bk && j < bi)) {
      bk = kj;
      bi = j;
    }
  }
};

struct EvalOut {
  int cols, k;
  bool lds_bins;
  uint32_t* s_bins;
  unsigned long long* counters;
  unsigned long long* confusion;
  long long* pred;
  uint32_t n_rows, n_top1, n_topk, n_bad;   // wave-uniform
};

// Reduce the lanes of each group and count the group's row.  Reached by all
// 64 lanes together (shuffles, ballots); `valid` / `inr`: the lane's row
// exists / has a label in range.
template <int G>
QCN_DEV void eval_finish(EvalLane s, bool valid, bool inr, long long row, int sub, EvalOut& o) {
#pragma unroll
  for (int off = G / 2; off > 0; off >>= 1) {
    s.cnt += __shfl_xor(s.cnt, off);
    const uint32_t ok = (uint32_t)__shfl_xor((int)s.bk, off);
    const int oi = __shfl_xor(s.bi, off);
    if (ok > s.bk || (ok == s.bk && oi < s.bi)) {
      s.bk = ok;
      s.bi = oi;
    }
  }
  const bool lead = valid && sub == 0;
  const bool top1 = inr && s.cnt == 0, topk = inr && s.cnt < o.k;
  o.n_rows += (uint32_t)__builtin_popcountll(__ballot(lead));
  o.n_top1 += (uint32_t)__builtin_popcountll(__ballot(lead && top1));
  o.n_topk += (uint32_t)__builtin_popcountll(__ballot(lead && topk));
  o.n_bad += (uint32_t)__builtin_popcountll(__ballot(lead && !inr));
  if (lead) {
    if (o.pred) o.pred[row] = s.bi;
    if (inr) {
      if (o.lds_bins) {
        atomicAdd(&o.s_bins[s.l], 1u);
        if (top1) atomicAdd(&o.s_bins[o.cols + s.l], 1u);
      } else {
        atomicAdd(&o.counters[4 + s.l], 1ull);
        if (top1) atomicAdd(&o.counters[4 + o.cols + s.l], 1ull);
      }
      if (o.confusion) atomicAdd(&o.confusion[(long long)s.l * o.cols + s.bi], 1ull);
    }
  }
}

// G < 64 requires cols <= G (the launcher's choice of G).
template <int G>
__global__ __launch_bounds__(kEvalThreads) void eval_topk_kernel(
    const float* __restrict__ x, int rows, int cols, const long long* __restrict__ labels, int k,
    unsigned long long* __restrict__ counters, unsigned long long* __restrict__ confusion,
    long long* __restrict__ pred) {
  __shared__ uint32_t s_bins[2 * kEvalLdsCols];   // [total cols][correct cols]
  __shared__ uint32_t s_tot[4];
  constexpr int kUnroll = G == 64 ? 1 : kEvalUnroll;
  constexpr int kRowsPerWave = 64 / G, kRowsPerSet = kRowsPerWave * kEvalWaves;
  constexpr int kRowsPerStep = kRowsPerSet * kUnroll;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, sub = lane & (G - 1);
  EvalOut o;
  o.cols = cols;
  o.k = k;
  o.lds_bins = cols <= kEvalLdsCols;
  o.s_bins = s_bins;
  o.counters = counters;
  o.confusion = confusion;
  o.pred = pred;
  o.n_rows = o.n_top1 = o.n_topk = o.n_bad = 0;
  if (o.lds_bins)
    for (int i = tid; i < 2 * cols; i += kEvalThreads) s_bins[i] = 0;
  if (tid < 4) s_tot[tid] = 0;
  __syncthreads();

  // `base` is uniform over the workgroup: every lane reaches the shuffles and
  // ballots together, lanes of rows past the end bring nothing
  for (long long base = (long long)blockIdx.x * kRowsPerStep; base < rows;
       base += (long long)gridDim.x * kRowsPerStep) {
    if constexpr (G == 64) {   // the row is the wave's: head / float4 body / tail are uniform
      const long long row = base + wave;
      const bool valid = row < rows;
      const long long lab = valid ? labels[row] : -1;
      const bool inr = valid && (unsigned long long)lab < (unsigned long long)cols;
      const float* r = x + (valid ? row : 0) * cols;
      EvalLane s;
      s.l = inr ? (int)lab : -1;
      s.kt = inr ? order_key(r[s.l]) : 0u;
      s.cnt = 0;
      s.bk = 0u;
      s.bi = 0x7fffffff;
      if (valid) {
        int head = (int)((4 - ((reinterpret_cast<uintptr_t>(r) >> 2) & 3)) & 3);
        head = head < cols ? head : cols;
        const int n4 = (cols - head) >> 2, tail = cols - head - 4 * n4;
        if (lane < head) s.visit(r[lane], lane);
        const float4* r4 = reinterpret_cast<const float4*>(r + head);
        for (int i = lane; i < n4; i += 64) {
          const float4 v = r4[i];
          const int j = head + 4 * i;
          s.visit(v.x, j);
          s.visit(v.y, j + 1);
          s.visit(v.z, j + 2);
          s.visit(v.w, j + 3);
        }
        if (lane < tail) s.visit(r[head + 4 * n4 + lane], head + 4 * n4 + lane);
      }
      eval_finish<G>(s, valid, inr, row, sub, o);
    } else {
      long long row[kUnroll], lab[kUnroll];
      float v[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        row[u] = base + u * kRowsPerSet + wave * kRowsPerWave + lane / G;
        const bool valid = row[u] < rows;
        lab[u] = valid ? labels[row[u]] : -1;
        v[u] = (valid && sub < cols) ? x[row[u] * cols + sub] : 0.0f;
      }
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        if (base + u * kRowsPerSet >= rows) break;   // uniform
        const bool valid = row[u] < rows;
        const bool inr = valid && (unsigned long long)lab[u] < (unsigned long long)cols;
        EvalLane s;
        s.l = inr ? (int)lab[u] : -1;
        // the label's value sits in lane l of this group (l < cols <= G)
        s.kt = order_key(__shfl(v[u], (lane & ~(G - 1)) + (inr ? s.l : 0)));
        s.cnt = 0;
        s.bk = 0u;
        s.bi = 0x7fffffff;
        if (valid && sub < cols) s.visit(v[u], sub);
        eval_finish<G>(s, valid, inr, row[u], sub, o);
      }
    }
  }

  if (lane == 0) {
    if (o.n_rows) atomicAdd(&s_tot[0], o.n_rows);
    if (o.n_top1) atomicAdd(&s_tot[1], o.n_top1);
    if (o.n_topk) atomicAdd(&s_tot[2], o.n_topk);
    if (o.n_bad) atomicAdd(&s_tot[3], o.n_bad);
  }
  __syncthreads();
  if (tid < 4 && s_tot[tid]) atomicAdd(&counters[tid], (unsigned long long)s_tot[tid]);
  if (o.lds_bins)
    for (int b = tid; b < 2 * cols; b += kEvalThreads) {
      const uint32_t c = s_bins[b];
      if (c) atomicAdd(&counters[4 + b], (unsigned long long)c);
    }
}

// Grid: one workgroup per step's worth of rows, capped at kEvalBlocksPerCu
// per CU with a grid-stride loop behind the cap.  Every workgroup ends with up
// to 4 + 2 * cols atomics on the same words, which the L2 takes one after the
// other, so a small grid with more rows per workgroup beats a wide one
// (measured at 1, 2, 4 and 8 per CU: [65536,10] 20 / 21 / 32 / 32 us,
// [8192,1000] 34 / 22 / 21 / 31 us).
template <int G>
static int eval_launch(const float* logits, int rows, int cols, const long long* labels, int k,
                       long long* counters, long long* confusion, long long* pred, int ncu,
                       hipStream_t stream) {
  constexpr int kRowsPerStep = (64 / G) * kEvalWaves * (G == 64 ? 1 : kEvalUnroll);
  long long grid = ((long long)rows + kRowsPerStep - 1) / kRowsPerStep;
  const long long cap = (long long)ncu * kEvalBlocksPerCu;
  grid = grid > cap ? cap : grid;
  hipLaunchKernelGGL(eval_topk_kernel<G>, dim3((unsigned)grid), dim3(kEvalThreads), 0, stream, logits,
                     rows, cols, labels, k, reinterpret_cast<unsigned long long*>(counters),
                     reinterpret_cast<unsigned long long*>(confusion), pred);
  return hipGetLastError() == hipSuccess ? QCN_OK : QCN_ERR_HIP;
}

}  // namespace qcn

extern "C" long long qcn_eval_counters_len(int cols) {
  return cols < 1 ? (long long)QCN_ERR_ARG : 4 + 2 * (long long)cols;
}

extern "C" int qcn_eval_topk_f32(const float* logits, int rows, int cols, const long long* labels,
                                 int k, long long* counters, long long* confusion, long long* pred,
                                 void* stream) {
  if (!logits || !labels || !counters || rows < 0 || cols < 1 || k < 1) return QCN_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(logits) & 3) ||
      ((reinterpret_cast<uintptr_t>(labels) | reinterpret_cast<uintptr_t>(counters) |
        reinterpret_cast<uintptr_t>(confusion) | reinterpret_cast<uintptr_t>(pred)) & 7))
    return QCN_ERR_ARG;
  if (rows == 0) return QCN_OK;
  const int ncu = qcn_cu_count();
  if (ncu <= 0) return QCN_ERR_HIP;
  const auto launch = cols <= 16 ? qcn::eval_launch<16>
                      : cols <= 32 ? qcn::eval_launch<32> : qcn::eval_launch<64>;
  return launch(logits, rows, cols, labels, k, counters, confusion, pred, ncu, (hipStream_t)stream);
}
