// jamun_hist.hip — two-dimensional histograms of pairs of angle columns, and the Jensen-Shannon divergence of such histograms.
//
//   k_hist2d_pairs    angles [n_frames][row_stride] (fp32; the [T, W] array k_internal_coords writes, or any view of it with a row stride
//                     in floats), pairs [P][2] (int32 columns: x then y), edges [bins + 1] (fp64: numpy's linspace(-pi, pi, bins + 1)
//                     uploaded by the caller, so the bin of a value is numpy's by construction) and up to 64 ascending cuts ->
//                     counts [C][P][bins * bins] and skipped [C][P] (uint32).  SEGMENT c holds the frames cuts[c-1] <= t < cuts[c]
//                     (cuts[-1] := 0); the histogram of the first cuts[c] frames is the sum of the segments 0..c, which k_js_divergence
//                     forms on the fly.  A frame whose x or y is not finite counts in skipped and in no bin.
//   k_js_divergence   counts [C][P][B] and reference counts [P_ref][B] (P_ref = P or 1) -> pooled [C] and per_pair [C][P] (fp64, nats):
//                     JSD of the normalised PREFIX sums against the normalised reference, pooled = all pairs summed into one histogram first.
//
// THE BIN of a value a (fp32 promoted to fp64, clipped to [edges[0], edges[bins]] = [-pi, pi]: float32(pi) > pi, and a dihedral of
// exactly 180 degrees must not fall off the table) is the largest b <= bins - 1 with edges[b] <= a: numpy's searchsorted(edges, a,
// "right") - 1 with the last edge inclusive.  An fp64 guess floor((a - edges[0]) * bins / (edges[bins] - edges[0])) clamped to
// [0, bins - 1] is walked down while a < edges[b] and up while a >= edges[b + 1]; both walks stop at the ends of the table, and the
// result does not depend on how good the guess was (it is off by one at most).  Comparisons only: no contraction can change them.
//
// ONE LANE PER FRAME, consecutive lanes on consecutive frames of a column.  A workgroup owns one (slice of a segment, segment, pair):
// the launcher cuts a segment into slices of JAMUN_HIST_SLICE frames.  Counting is integer atomicAdd, so the result is exact and does
// not depend on the order of arrival.  The workgroup zeroes bins * bins counters in LDS (at most 128 * 128 * 4 B = 64 KB), counts there
// and adds the non-zero ones to the global array.  One global atomicAdd per frame instead (no LDS) was measured beside it on an MI355X
// at 100 bins: 4.1 times slower on one segment of 1e6 frames (0.197 against 0.048 ms), 14 % slower on a chain's nine segments of 100
// to 7200 frames, and inside the noise on 64 segments of 100 frames (0.028 against 0.030 ms, ranges overlapping), where it had most to
// gain: it never won, so there is one code path.
//
// A column of `pairs` outside [0, width) (a device-resident table is not checked by the host) makes its pair count nothing, skipped
// included; nothing is read for it.  The cuts travel in the kernel arguments: no upload, no allocation.
//
// k_js_divergence: one workgroup per (cut, pair) and one per (cut, pooled).  n_i = sum of the segments 0..cut of bin i (uint64), N their
// total, r_i, R the reference's; p = n_i / N, q = r_i / R, m = (p + q) / 2, JSD = (sum p log(p / m) + sum q log(q / m)) / 2 in fp64
// with zero terms skipped: scipy.spatial.distance.jensenshannon(p, q) ** 2.  Every lane sums its bins (i = lane, lane + 256, ...) in
// ascending order and the 256 partial sums are folded by a fixed tree: the value is a function of the inputs alone.  N = 0 or R = 0 is NaN.
//
// No MFMA, no inline assembly, no allocation: every buffer is the caller's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "jamun_internal.h"

namespace {

constexpr int HIST_THREADS = 256;
constexpr int HIST_SLICE = JAMUN_HIST_SLICE;
constexpr int JS_THREADS = 256;

__device__ __forceinline__ int bin_of(double a, const double* __restrict__ edges, int bins, double lo, double hi, double scale) {
  a = a < lo ? lo : a > hi ? hi : a;
  int b = (int)floor((a - lo) * scale);
  b = b < 0 ? 0 : b > bins - 1 ? bins - 1 : b;
  while (b > 0 && a < edges[b]) --b;
  while (b < bins - 1 && a >= edges[b + 1]) ++b;
  return b;
}

__global__ void __launch_bounds__(HIST_THREADS)
k_hist2d_pairs(const float* __restrict__ angles, long long row_stride, int width, const int* __restrict__ pairs, int n_pairs,
               const double* __restrict__ edges, int bins, JamunHistCuts cuts, unsigned* __restrict__ counts, unsigned* __restrict__ skipped) {
  extern __shared__ unsigned s_cnt[];  // bins * bins counters
  const int c = blockIdx.y, p = blockIdx.z;
  const int seg0 = c > 0 ? cuts.cut[c - 1] : 0, seg1 = cuts.cut[c];
  const long long t0 = (long long)seg0 + (long long)blockIdx.x * HIST_SLICE;
  if (t0 >= seg1) return;  // (a short segment has fewer slices than the grid is wide; uniform over the workgroup)
  const int t1 = (int)min((long long)seg1, t0 + HIST_SLICE);
  const int cx = pairs[2 * p], cy = pairs[2 * p + 1];  // (wave-uniform: scalar loads)
  if (cx < 0 || cx >= width || cy < 0 || cy >= width) return;
  const int nb2 = bins * bins;
  unsigned* const g_cnt = counts + ((long long)c * n_pairs + p) * nb2;
  for (int i = threadIdx.x; i < nb2; i += HIST_THREADS) s_cnt[i] = 0u;
  __syncthreads();
  const double lo = edges[0], hi = edges[bins];
  const double scale = (double)bins / (hi - lo);
  unsigned skipped_here = 0u;
  for (long long t = t0 + threadIdx.x; t < t1; t += HIST_THREADS) {
    const float* const row = angles + t * row_stride;
    const float x = row[cx], y = row[cy];
    if (!(isfinite(x) && isfinite(y))) {
      ++skipped_here;
      continue;
    }
    const int b = bin_of((double)x, edges, bins, lo, hi, scale) * bins + bin_of((double)y, edges, bins, lo, hi, scale);
    atomicAdd(&s_cnt[b], 1u);
  }
  if (skipped_here) atomicAdd(&skipped[c * n_pairs + p], skipped_here);  // (rare: straight to the global counter)
  __syncthreads();
  for (int i = threadIdx.x; i < nb2; i += HIST_THREADS) {
    const unsigned v = s_cnt[i];
    if (v) atomicAdd(&g_cnt[i], v);
  }
}

// The sum of 256 doubles, one per lane, in a fixed order; the result in every lane.
__device__ __forceinline__ double block_sum(double v, double* s) {
  __syncthreads();  // (s may still be read from the previous sum)
  s[threadIdx.x] = v;
  __syncthreads();
  for (int w = JS_THREADS / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) s[threadIdx.x] += s[threadIdx.x + w];
    __syncthreads();
  }
  return s[0];
}

__global__ void __launch_bounds__(JS_THREADS)
k_js_divergence(const unsigned* __restrict__ counts, int n_pairs, int nb2, const unsigned* __restrict__ ref, int n_ref_pairs,
                double* __restrict__ pooled, double* __restrict__ per_pair) {
  __shared__ double s_sum[JS_THREADS];
  const int c = blockIdx.y;
  const bool pool = (int)blockIdx.x == n_pairs;
  const int p0 = pool ? 0 : (int)blockIdx.x, p1 = pool ? n_pairs : p0 + 1;                        // the pairs summed into the histogram
  const int r0 = n_ref_pairs == 1 ? 0 : p0, r1 = n_ref_pairs == 1 ? 1 : p1;                       // ... and into the reference
  const long long seg_stride = (long long)n_pairs * nb2;

  auto n_of = [&](int i) {
    unsigned long long n = 0ull;
    for (int s = 0; s <= c; ++s)
      for (int p = p0; p < p1; ++p) n += counts[s * seg_stride + (long long)p * nb2 + i];
    return n;
  };
  auto r_of = [&](int i) {
    unsigned long long r = 0ull;
    for (int p = r0; p < r1; ++p) r += ref[(long long)p * nb2 + i];
    return r;
  };

  // totals: exact in fp64 below 2^53 counts
  unsigned long long n_part = 0ull, r_part = 0ull;
  for (int i = threadIdx.x; i < nb2; i += JS_THREADS) {
    n_part += n_of(i);
    r_part += r_of(i);
  }
  const double N = block_sum((double)n_part, s_sum), R = block_sum((double)r_part, s_sum);

  double acc = 0.0;
  if (N > 0.0 && R > 0.0) {
    for (int i = threadIdx.x; i < nb2; i += JS_THREADS) {
      const double pi = (double)n_of(i) / N, qi = (double)r_of(i) / R;
      const double m = 0.5 * (pi + qi);
      double term = 0.0;
      if (pi > 0.0) term += pi * log(pi / m);
      if (qi > 0.0) term += qi * log(qi / m);
      acc += term;
    }
  }
  const double total = block_sum(acc, s_sum);
  if (threadIdx.x == 0) {
    const double js = (N > 0.0 && R > 0.0) ? 0.5 * total : __builtin_nan("");
    if (pool)
      pooled[c] = js;
    else
      per_pair[c * n_pairs + p0] = js;
  }
}

}  // namespace

void launch_hist2d_pairs(const float* angles, long long row_stride, int width, const int* pairs, int n_pairs, const double* edges, int bins,
                         const JamunHistCuts& cuts, unsigned* counts, unsigned* skipped, hipStream_t st) {
  int longest = 0;
  for (int c = 0; c < cuts.n; ++c) {
    const int len = cuts.cut[c] - (c > 0 ? cuts.cut[c - 1] : 0);
    longest = len > longest ? len : longest;
  }
  const int slices = (longest - 1) / HIST_SLICE + 1;  // (cuts ascend strictly: longest >= 1)
  const size_t lds = (size_t)bins * bins * sizeof(unsigned);  // (bins <= 128: at most 64 KB)
  hipLaunchKernelGGL(k_hist2d_pairs, dim3(slices, cuts.n, n_pairs), dim3(HIST_THREADS), lds, st, angles, row_stride, width, pairs, n_pairs, edges,
                     bins, cuts, counts, skipped);
}

void launch_js_divergence(const unsigned* counts, int n_cuts, int n_pairs, int bins, const unsigned* ref, int n_ref_pairs, double* pooled,
                          double* per_pair, hipStream_t st) {
  hipLaunchKernelGGL(k_js_divergence, dim3(n_pairs + 1, n_cuts), dim3(JS_THREADS), 0, st, counts, n_pairs, bins * bins, ref, n_ref_pairs,
                     pooled, per_pair);
}
