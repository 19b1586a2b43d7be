// jamun_msm.hip — the reductions over frames behind k-means and the Markov state model of a projected trajectory (jamun_amd/msm.py):
// nearest centre of every frame, sums of the frames of every cluster, transition counts at a lag, occupancy counts over segments.
//
//   k_assign          y [n_frames][row_stride] (fp64, d values read per row: what k_project writes) and centres [k][d] (fp64) -> labels
//                     [n_frames] (int32), optionally the squared distance to the chosen centre and the number of labels that differ
//                     from prev_labels.
//   k_cluster_partial / k_cluster_reduce    y, labels -> counts [k] (int64) and sums [k][d] (fp64): the rows of every cluster added up.
//   k_transitions     labels, a lag, optionally a map microstate -> state: counts [n_states][n_states] (int64) += the pairs
//                     (state(t), state(t + lag)), t < n_frames - lag.
//   k_label_counts    labels, map, bounds [n_seg + 1]: counts [n_seg][n_states] (int64) += the frames of segment s in every state.
//
// BIT FOR BIT.  The distance of a row to a centre is acc = 0; for j ascending: diff = y[j] - c[j], sq = diff * diff, acc = acc + sq,
// every operation rounded on its own (__dsub_rn, __dmul_rn, __dadd_rn: no contraction whatever the compiler flags say): exactly the
// numpy loop of msm.assign_centers_host, so the label (smallest acc, the lowest index on a tie: a strict comparison in ascending
// centre order) is the specification's integer for integer.  A fused multiply-add would round once where numpy rounds twice and can
// turn a near tie around (tests/_msm_cases.py holds such frames).  The cluster sums are additions only, in the order of
// msm.cluster_sums_host: frames cut into slices of JAMUN_TICA_SLICE, a cluster's rows of a slice added in ascending frame order onto
// +0.0 (one lane per output (cluster, column), partials in the caller's workspace [slice][k d + k]), the slices added in ascending
// order onto +0.0.  No floating-point atomics anywhere; the counts are integer atomics and exact in any order of arrival.
//
// ASSIGNMENT.  One lane per frame, 256 frames per workgroup.  The centres go through LDS in tiles of at most MSM_CENTER_TILE doubles
// (32 KB: whole centres, floor(4096 / d) of them at a time); every lane of a wave reads the same centre value (a broadcast).  A row of
// at most MSM_ROW_REGS values is held in registers; a longer one is read again for every centre (from the caches: a projection rarely
// has more than ten columns).  A row with a non-finite value gets label -1 and a NaN distance; no other row reads it.
//
// COUNTS.  k_transitions and k_label_counts count in LDS (uint32; a workgroup sees at most MSM_COUNT_SLICE frames, no overflow) where
// the table has at most MSM_LDS_COUNTERS entries, and add the non-zero entries to the global int64 table; larger tables are counted
// in global memory directly.  bounds is device-resident and not checked by the host: the segment of a frame is found by bisection,
// whose result is clamped to the table whatever bounds holds; frames outside [bounds[0], bounds[n_seg]) count nowhere.
//
// No MFMA, no inline assembly, no allocation: every buffer is the caller's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "jamun_internal.h"

#pragma clang fp contract(off)

namespace {

constexpr int MSM_THREADS = 256;
constexpr int SLICE = JAMUN_TICA_SLICE;
constexpr int MSM_CENTER_TILE = 4096;    // doubles of centres in LDS at a time (>= JAMUN_MSM_MAX_D: a tile holds at least 32 centres)
constexpr int MSM_ROW_REGS = 16;         // columns of a row a lane keeps in registers
constexpr int MSM_COUNT_SLICE = 4096;    // frames a workgroup of the counting kernels sees
constexpr int MSM_LDS_COUNTERS = 8192;   // entries of a count table kept in LDS (32 KB)

static_assert(MSM_CENTER_TILE >= JAMUN_MSM_MAX_D, "a tile holds at least one centre");
static_assert(SLICE == 1024, "one workgroup stages the labels of a slice in 4 KB");

template <bool IN_REGS>
__global__ void __launch_bounds__(MSM_THREADS)
k_assign(const double* __restrict__ y, long long row_stride, int n_frames, int d, const double* __restrict__ centers, int k, int* labels,
         double* __restrict__ sqdist, const int* prev, unsigned long long* __restrict__ n_changed) {
  __shared__ double s_c[MSM_CENTER_TILE];
  __shared__ unsigned s_changed;
  const long long t = (long long)blockIdx.x * MSM_THREADS + threadIdx.x;
  const bool live = t < n_frames;
  const double* const row = y + (live ? t : 0) * row_stride;
  double r[MSM_ROW_REGS];
  bool finite = true;
  if (IN_REGS) {
#pragma unroll
    for (int j = 0; j < MSM_ROW_REGS; ++j) {
      r[j] = (live && j < d) ? row[j] : 0.0;
      finite = finite && isfinite(r[j]);
    }
  } else if (live) {
    for (int j = 0; j < d; ++j) finite = finite && isfinite(row[j]);
  }
  if (threadIdx.x == 0) s_changed = 0u;
  double best = 0.0;
  int best_c = -1;
  const int per_tile = MSM_CENTER_TILE / d;  // whole centres per tile (>= 32)
  for (int c0 = 0; c0 < k; c0 += per_tile) {
    const int nc = min(per_tile, k - c0);
    __syncthreads();  // (the previous tile is read out; s_changed is zero)
    for (int e = threadIdx.x; e < nc * d; e += MSM_THREADS) s_c[e] = centers[(long long)c0 * d + e];
    __syncthreads();
    if (live && finite) {
      for (int c = 0; c < nc; ++c) {
        const double* const cc = s_c + c * d;
        double acc = 0.0;
        if (IN_REGS) {
#pragma unroll
          for (int j = 0; j < MSM_ROW_REGS; ++j)
            if (j < d) {
              const double diff = __dsub_rn(r[j], cc[j]);
              acc = __dadd_rn(acc, __dmul_rn(diff, diff));
            }
        } else {
          for (int j = 0; j < d; ++j) {
            const double diff = __dsub_rn(row[j], cc[j]);
            acc = __dadd_rn(acc, __dmul_rn(diff, diff));
          }
        }
        if (best_c < 0 || acc < best) {  // (strict: the lowest index keeps a tie)
          best = acc;
          best_c = c0 + c;
        }
      }
    }
  }
  if (live) {
    if (prev && prev[t] != best_c) atomicAdd(&s_changed, 1u);  // (prev may be labels itself: read before the store below, by the same lane)
    labels[t] = best_c;
    if (sqdist) sqdist[t] = finite ? best : __builtin_nan("");
  }
  if (n_changed) {
    __syncthreads();
    if (threadIdx.x == 0 && s_changed) atomicAdd(n_changed, (unsigned long long)s_changed);
  }
}

// work [slice][k d + k]: entry e < k d is the sum of column e % d over the rows of the slice labelled e / d, in ascending frame order;
// entry k d + c the number of such rows (a double: at most 1024, exact).
__global__ void __launch_bounds__(MSM_THREADS)
k_cluster_partial(const double* __restrict__ y, long long row_stride, int n_frames, int d, const int* __restrict__ labels, int k,
                  double* __restrict__ work) {
  __shared__ int s_lab[SLICE];
  const int slice = blockIdx.x;
  const long long t0 = (long long)slice * SLICE;  // (< n_frames)
  const int nf = (int)min((long long)SLICE, n_frames - t0);
  for (int f = threadIdx.x; f < nf; f += MSM_THREADS) s_lab[f] = labels[t0 + f];
  __syncthreads();
  const int kd = k * d, e = blockIdx.y * MSM_THREADS + threadIdx.x;
  if (e >= kd + k) return;
  double acc = 0.0;
  if (e < kd) {
    const int c = e / d, j = e - c * d;
    const double* const col = y + t0 * row_stride + j;
    for (int f = 0; f < nf; ++f)
      if (s_lab[f] == c) acc = __dadd_rn(acc, col[f * row_stride]);
  } else {
    const int c = e - kd;
    for (int f = 0; f < nf; ++f)
      if (s_lab[f] == c) acc += 1.0;
  }
  work[(long long)slice * (kd + k) + e] = acc;
}

__global__ void __launch_bounds__(MSM_THREADS)
k_cluster_reduce(const double* __restrict__ work, int kd, int k, int n_slices, double* __restrict__ sums, long long* __restrict__ counts) {
  const int e = blockIdx.x * MSM_THREADS + threadIdx.x;
  if (e >= kd + k) return;
  double acc = 0.0;
  for (int s = 0; s < n_slices; ++s) acc = __dadd_rn(acc, work[(long long)s * (kd + k) + e]);
  if (e < kd)
    sums[e] = acc;
  else
    counts[e - kd] = (long long)acc;  // (whole numbers below 2^31: exact)
}

// the state of a label: -1 for none
__device__ __forceinline__ int state_of(int label, const int* __restrict__ map, int n_in, int n_states) {
  if (label < 0 || label >= n_in) return -1;
  const int s = map ? map[label] : label;
  return (s < 0 || s >= n_states) ? -1 : s;
}

__global__ void __launch_bounds__(MSM_THREADS)
k_transitions(const int* __restrict__ labels, int n_pairs, int lag, const int* __restrict__ map, int n_in, int n_states,
              unsigned long long* __restrict__ counts, int use_lds) {
  extern __shared__ unsigned s_cnt[];
  const int n2 = n_states * n_states;
  if (use_lds) {
    for (int i = threadIdx.x; i < n2; i += MSM_THREADS) s_cnt[i] = 0u;
    __syncthreads();
  }
  const long long t0 = (long long)blockIdx.x * MSM_COUNT_SLICE;
  const int t1 = (int)min((long long)n_pairs, t0 + MSM_COUNT_SLICE);
  for (long long t = t0 + threadIdx.x; t < t1; t += MSM_THREADS) {
    const int a = state_of(labels[t], map, n_in, n_states), b = state_of(labels[t + lag], map, n_in, n_states);
    if (a < 0 || b < 0) continue;
    if (use_lds)
      atomicAdd(&s_cnt[a * n_states + b], 1u);
    else
      atomicAdd(&counts[(long long)a * n_states + b], 1ull);
  }
  if (use_lds) {
    __syncthreads();
    for (int i = threadIdx.x; i < n2; i += MSM_THREADS) {
      const unsigned v = s_cnt[i];
      if (v) atomicAdd(&counts[i], (unsigned long long)v);
    }
  }
}

__global__ void __launch_bounds__(MSM_THREADS)
k_label_counts(const int* __restrict__ labels, int n_frames, const int* __restrict__ map, int n_in, int n_states,
               const int* __restrict__ bounds, int n_seg, unsigned long long* __restrict__ counts, int use_lds) {
  extern __shared__ unsigned s_cnt[];
  const int n_out = n_seg * n_states;
  if (use_lds) {
    for (int i = threadIdx.x; i < n_out; i += MSM_THREADS) s_cnt[i] = 0u;
    __syncthreads();
  }
  const long long t0 = (long long)blockIdx.x * MSM_COUNT_SLICE;
  const int t1 = (int)min((long long)n_frames, t0 + MSM_COUNT_SLICE);
  for (long long t = t0 + threadIdx.x; t < t1; t += MSM_THREADS) {
    const int a = state_of(labels[t], map, n_in, n_states);
    if (a < 0) continue;
    // the number of bounds[0 .. n_seg] that are <= t (upper bound by bisection), less one: the segment with bounds[s] <= t < bounds[s + 1]
    int lo = 0, hi = n_seg + 1;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (bounds[mid] <= t) lo = mid + 1; else hi = mid;
    }
    const int s = lo - 1;
    if (s < 0 || s >= n_seg) continue;  // (before the first bound or behind the last)
    if (use_lds)
      atomicAdd(&s_cnt[s * n_states + a], 1u);
    else
      atomicAdd(&counts[(long long)s * n_states + a], 1ull);
  }
  if (use_lds) {
    __syncthreads();
    for (int i = threadIdx.x; i < n_out; i += MSM_THREADS) {
      const unsigned v = s_cnt[i];
      if (v) atomicAdd(&counts[i], (unsigned long long)v);
    }
  }
}

}  // namespace

static int msm_blocks(int n, int per) { return (int)(((long long)n + per - 1) / per); }  // (n >= 1)

long long cluster_work_doubles(int n_frames, int d, int k) { return (long long)msm_blocks(n_frames, SLICE) * ((long long)k * d + k); }

void launch_assign_centers(const double* y, long long row_stride, int n_frames, int d, const double* centers, int k, int* labels, double* sqdist,
                           const int* prev, long long* n_changed, hipStream_t st) {
  const dim3 grid(msm_blocks(n_frames, MSM_THREADS));
  if (d <= MSM_ROW_REGS)
    hipLaunchKernelGGL(k_assign<true>, grid, dim3(MSM_THREADS), 0, st, y, row_stride, n_frames, d, centers, k, labels, sqdist, prev,
                       (unsigned long long*)n_changed);
  else
    hipLaunchKernelGGL(k_assign<false>, grid, dim3(MSM_THREADS), 0, st, y, row_stride, n_frames, d, centers, k, labels, sqdist, prev,
                       (unsigned long long*)n_changed);
}

void launch_cluster_sums(const double* y, long long row_stride, int n_frames, int d, const int* labels, int k, long long* counts, double* sums,
                         double* work, hipStream_t st) {
  const int slices = msm_blocks(n_frames, SLICE), per_slice = k * d + k, blocks = (per_slice + MSM_THREADS - 1) / MSM_THREADS;
  hipLaunchKernelGGL(k_cluster_partial, dim3(slices, blocks), dim3(MSM_THREADS), 0, st, y, row_stride, n_frames, d, labels, k, work);
  hipLaunchKernelGGL(k_cluster_reduce, dim3(blocks), dim3(MSM_THREADS), 0, st, work, k * d, k, slices, sums, counts);
}

void launch_transition_counts(const int* labels, int n_frames, int lag, const int* map, int n_in, int n_states, long long* counts, hipStream_t st) {
  const int n_pairs = n_frames - lag;  // (>= 1)
  const int use_lds = n_states * n_states <= MSM_LDS_COUNTERS;
  hipLaunchKernelGGL(k_transitions, dim3(msm_blocks(n_pairs, MSM_COUNT_SLICE)), dim3(MSM_THREADS),
                     use_lds ? (size_t)n_states * n_states * sizeof(unsigned) : 0, st, labels, n_pairs, lag, map, n_in, n_states,
                     (unsigned long long*)counts, use_lds);
}

void launch_label_counts(const int* labels, int n_frames, const int* map, int n_in, int n_states, const int* bounds, int n_seg, long long* counts,
                         hipStream_t st) {
  const int use_lds = (long long)n_seg * n_states <= MSM_LDS_COUNTERS;
  hipLaunchKernelGGL(k_label_counts, dim3(msm_blocks(n_frames, MSM_COUNT_SLICE)), dim3(MSM_THREADS),
                     use_lds ? (size_t)n_seg * n_states * sizeof(unsigned) : 0, st, labels, n_frames, map, n_in, n_states, bounds, n_seg,
                     (unsigned long long*)counts, use_lds);
}
