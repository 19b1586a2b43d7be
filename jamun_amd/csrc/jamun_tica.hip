// jamun_tica.hip — the three reductions over frames behind time-lagged independent component analysis (jamun_amd/tica.py): the lagged
// second moments of a feature trajectory, its projection on fitted components, and the autocovariance sums of one projected column.
//
//   k_moments_partial / k_slices_reduce    x [n_frames][row_stride] (fp32, `width` columns read per row) and a lag -> sums [2][W] and
//                     moments [3][W][W] (fp64) over the N = n_frames - lag pairs (x_t, x_{t+lag}):  G = sum x_t x_t^T,
//                     H = sum x_{t+lag} x_{t+lag}^T, K = sum x_t x_{t+lag}^T (row = the earlier frame).
//   k_project         x, mean [W], v [W][d] (fp64) -> out [n_frames][d] (fp64):  out[t][k] = sum_j (x[t][j] - mean[j]) v[j][k].
//   k_autocov_partial / k_slices_reduce    y [n_frames] (fp64, `stride` doubles apart) -> out [max_lag + 1]:  out[k] = sum_{t < n - k} y_t y_{t+k}.
//
// FIXED ORDER.  Both reductions are two passes.  The frames (pairs for the moments, first factors t for the autocovariance) are cut into
// SLICES of JAMUN_TICA_SLICE; a workgroup of the first pass owns one slice and one tile of outputs, every lane adds the terms of its
// own outputs in ascending t and writes the partial sums into the caller's workspace [slice][output]; the second pass adds the slices
// of one output in slice order, one lane per output.  No floating-point atomics, no order of arrival: the same inputs give the same
// bits.  Every partial of the workspace that the second pass reads is written by the first (a zero where a slice has no term), so the
// workspace needs no clearing.
//
// MOMENTS.  Every value is promoted to fp64 before it is multiplied: the product of two fp32 values is exact in fp64 (48 bits), the
// only rounding is in the additions.  A workgroup of 256 lanes owns a 32 x 32 tile of the three matrices, lane (ti, tj) the 2 x 2
// entries rows 2 ti.., columns 2 tj..: 12 accumulators.  Frames are staged 32 pairs at a time in LDS as fp32 (the tile's row columns and
// its column columns, of x_t and of x_{t+lag}: 16 KB); columns past `width` are staged as zeros and their outputs never written, and
// nothing is read past `width` in a row (the padding of a strided view may hold anything, the last row may end the allocation).  Per
// staged pair a lane reads four float2 (broadcasts within the rows / columns of the tile), converts 8 values and issues 12 v_fmac_f64.
// G[i][j] and G[j][i] add the same exact products in the same order, so G and H are symmetric bit for bit without a mirror pass.
// The workgroups of the first tile row also sum x_t and x_{t+lag} of their columns (lanes ti == 0).
// Why no v_mfma_f64_16x16x4_f64 form: DESIGN.md (TICA).  Nothing here has been timed.
//
// PROJECTION.  One lane per output (t, k), k fastest: j ascending, the difference formed in fp64, one accumulator.  A non-finite x[t][j]
// makes (x - mean) non-finite and with it every output of row t (NaN * 0 = NaN); no other row reads it.
//
// AUTOCOVARIANCE.  A workgroup owns a slice of t and 256 consecutive lags, lane = lag.  It stages y of the slice and of the slice shifted
// by its lags (SLICE + 256 values) in LDS; a lane adds y_t y_{t+k} for the t of the slice with t + k < n.  Values behind the end of y are
// never multiplied (a staged zero would turn an infinite y_t into NaN), the loop bound of the lane excludes them.
//
// No MFMA, no inline assembly, no allocation: every buffer is the caller's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "jamun_internal.h"

namespace {

constexpr int TICA_THREADS = 256;
constexpr int SLICE = JAMUN_TICA_SLICE;
constexpr int TILE = JAMUN_TICA_TILE;  // 32: 16 x 16 lanes of 2 x 2 entries
constexpr int STAGE = 32;              // pairs staged at a time

static_assert(TILE == 32 && TICA_THREADS == 256, "lane (ti, tj) = (tid >> 4, tid & 15) owns 2 x 2 entries of a 32 x 32 tile");
static_assert(SLICE % STAGE == 0, "a slice is a whole number of stages");

// the workspace of the moments: [slice][2 W + 3 W W]: sums of x_t, sums of x_{t+lag}, G, H, K
__device__ __forceinline__ long long moments_per_slice(int W) { return 2ll * W + 3ll * W * W; }

__global__ void __launch_bounds__(TICA_THREADS)
k_moments_partial(const float* __restrict__ x, long long row_stride, int n_pairs, int W, int lag, double* __restrict__ work) {
  __shared__ float s_ai[STAGE][TILE], s_aj[STAGE][TILE], s_bi[STAGE][TILE], s_bj[STAGE][TILE];
  const int slice = blockIdx.x;
  const int tiles = (W + TILE - 1) / TILE;
  const int bi = blockIdx.y / tiles, bj = blockIdx.y % tiles;
  const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;
  const long long t0 = (long long)slice * SLICE;
  const int t1 = (int)min((long long)n_pairs, t0 + SLICE);  // (t0 < n_pairs: the grid has ceil(n_pairs / SLICE) slices)
  const bool do_sums = bi == 0;                               // (uniform over the workgroup)

  double g00 = 0.0, g01 = 0.0, g10 = 0.0, g11 = 0.0;
  double h00 = 0.0, h01 = 0.0, h10 = 0.0, h11 = 0.0;
  double k00 = 0.0, k01 = 0.0, k10 = 0.0, k11 = 0.0;
  double sa0 = 0.0, sa1 = 0.0, sb0 = 0.0, sb1 = 0.0;

  for (long long c0 = t0; c0 < t1; c0 += STAGE) {
    const int nf = (int)min((long long)STAGE, t1 - c0);
    __syncthreads();  // (the previous stage is read out)
    // 4 arrays x STAGE x TILE floats, 16 per lane; element e: array (e >> 10), frame (e >> 5) & 31, column e & 31
    for (int e = tid; e < 4 * STAGE * TILE; e += TICA_THREADS) {
      const int arr = e >> 10, f = (e >> 5) & (STAGE - 1), c = e & (TILE - 1);
      const int col = ((arr & 1) ? bj : bi) * TILE + c;
      float v = 0.0f;
      if (f < nf && col < W) v = x[(c0 + f + ((arr & 2) ? lag : 0)) * row_stride + col];
      float* const dst = arr == 0 ? &s_ai[0][0] : arr == 1 ? &s_aj[0][0] : arr == 2 ? &s_bi[0][0] : &s_bj[0][0];
      dst[f * TILE + c] = v;
    }
    __syncthreads();
    for (int f = 0; f < nf; ++f) {
      const double ai0 = (double)s_ai[f][2 * ti], ai1 = (double)s_ai[f][2 * ti + 1];
      const double aj0 = (double)s_aj[f][2 * tj], aj1 = (double)s_aj[f][2 * tj + 1];
      const double bi0 = (double)s_bi[f][2 * ti], bi1 = (double)s_bi[f][2 * ti + 1];
      const double bj0 = (double)s_bj[f][2 * tj], bj1 = (double)s_bj[f][2 * tj + 1];
      // (fma: the product is exact either way, so the bits are those of a multiply and an add, in half the instructions)
      g00 = fma(ai0, aj0, g00); g01 = fma(ai0, aj1, g01); g10 = fma(ai1, aj0, g10); g11 = fma(ai1, aj1, g11);
      h00 = fma(bi0, bj0, h00); h01 = fma(bi0, bj1, h01); h10 = fma(bi1, bj0, h10); h11 = fma(bi1, bj1, h11);
      k00 = fma(ai0, bj0, k00); k01 = fma(ai0, bj1, k01); k10 = fma(ai1, bj0, k10); k11 = fma(ai1, bj1, k11);
      if (do_sums) {
        sa0 += aj0; sa1 += aj1; sb0 += bj0; sb1 += bj1;
      }
    }
  }

  double* const w = work + (long long)slice * moments_per_slice(W);
  const int i0 = bi * TILE + 2 * ti, j0 = bj * TILE + 2 * tj;
  const long long WW = (long long)W * W;
  double* const G = w + 2ll * W;
  auto put = [&](int i, int j, double g, double h, double k) {
    if (i < W && j < W) {
      const long long at = (long long)i * W + j;
      G[at] = g;
      G[WW + at] = h;
      G[2 * WW + at] = k;
    }
  };
  put(i0, j0, g00, h00, k00);
  put(i0, j0 + 1, g01, h01, k01);
  put(i0 + 1, j0, g10, h10, k10);
  put(i0 + 1, j0 + 1, g11, h11, k11);
  if (do_sums && ti == 0) {
    if (j0 < W) { w[j0] = sa0; w[W + j0] = sb0; }
    if (j0 + 1 < W) { w[j0 + 1] = sa1; w[W + j0 + 1] = sb1; }
  }
}

// out[e] = sum over the slices, in slice order, of work[slice][e]: one lane per output.  The moments' outputs are two arrays (sums
// [2 W], then moments [3 W W]) laid out in the workspace one behind the other.
__global__ void __launch_bounds__(TICA_THREADS)
k_slices_reduce(const double* __restrict__ work, long long per_slice, int n_slices, double* __restrict__ out_a, long long n_a,
                double* __restrict__ out_b) {
  const long long e = (long long)blockIdx.x * TICA_THREADS + threadIdx.x;
  if (e >= per_slice) return;
  double acc = 0.0;
  for (int s = 0; s < n_slices; ++s) acc += work[(long long)s * per_slice + e];
  if (e < n_a)
    out_a[e] = acc;
  else
    out_b[e - n_a] = acc;
}

__global__ void __launch_bounds__(TICA_THREADS)
k_project(const float* __restrict__ x, long long row_stride, long long n_out, int W, const double* __restrict__ mean,
          const double* __restrict__ v, int d, double* __restrict__ out) {
  const long long o = (long long)blockIdx.x * TICA_THREADS + threadIdx.x;
  if (o >= n_out) return;
  const long long t = o / d;
  const int k = (int)(o - t * d);
  const float* const row = x + t * row_stride;
  double acc = 0.0;
  for (int j = 0; j < W; ++j) acc += ((double)row[j] - mean[j]) * v[(long long)j * d + k];
  out[o] = acc;
}

__global__ void __launch_bounds__(TICA_THREADS)
k_autocov_partial(const double* __restrict__ y, long long stride, int n, int max_lag, double* __restrict__ work) {
  __shared__ double s_y[SLICE], s_l[SLICE + TICA_THREADS];
  const int slice = blockIdx.x;
  const int k0 = blockIdx.y * TICA_THREADS, k = k0 + threadIdx.x;
  const long long t0 = (long long)slice * SLICE;  // (< n)
  const int nt = (int)min((long long)SLICE, n - t0);
  for (int e = threadIdx.x; e < SLICE + TICA_THREADS; e += TICA_THREADS) {
    const long long t = t0 + k0 + e;
    s_l[e] = t < n ? y[t * stride] : 0.0;  // (never multiplied behind the end: the loop bound below)
    if (e < SLICE) s_y[e] = e < nt ? y[(t0 + e) * stride] : 0.0;
  }
  __syncthreads();
  if (k > max_lag) return;
  // t in [t0, t0 + nt) with t + k < n
  const long long last = (long long)n - k - t0;  // exclusive bound of t - t0
  const int m = last < 0 ? 0 : (int)min((long long)nt, last);
  double acc = 0.0;
  for (int f = 0; f < m; ++f) acc += s_y[f] * s_l[f + threadIdx.x];
  work[(long long)slice * (max_lag + 1) + k] = acc;
}

}  // namespace

int tica_slices(int n) { return (n + SLICE - 1) / SLICE; }  // (n >= 1; below 2^31 / SLICE)

long long moments_work_doubles(int n_frames, int W, int lag) { return (long long)tica_slices(n_frames - lag) * (2ll * W + 3ll * W * W); }

long long autocov_work_doubles(int n_frames, int max_lag) { return (long long)tica_slices(n_frames) * (max_lag + 1ll); }

void launch_lagged_moments(const float* x, long long row_stride, int n_frames, int W, int lag, double* sums, double* moments, double* work,
                           hipStream_t st) {
  const int n_pairs = n_frames - lag, slices = tica_slices(n_pairs), tiles = (W + TILE - 1) / TILE;
  hipLaunchKernelGGL(k_moments_partial, dim3(slices, tiles * tiles), dim3(TICA_THREADS), 0, st, x, row_stride, n_pairs, W, lag, work);
  const long long per_slice = 2ll * W + 3ll * W * W;
  hipLaunchKernelGGL(k_slices_reduce, dim3((unsigned)((per_slice + TICA_THREADS - 1) / TICA_THREADS)), dim3(TICA_THREADS), 0, st, work, per_slice,
                     slices, sums, 2ll * W, moments);
}

void launch_project_frames(const float* x, long long row_stride, int n_frames, int W, const double* mean, const double* v, int d, double* out,
                           hipStream_t st) {
  const long long n_out = (long long)n_frames * d;  // (< 2^38: the grid below fits 31 bits)
  hipLaunchKernelGGL(k_project, dim3((unsigned)((n_out + TICA_THREADS - 1) / TICA_THREADS)), dim3(TICA_THREADS), 0, st, x, row_stride, n_out, W,
                     mean, v, d, out);
}

void launch_autocov_sums(const double* y, long long stride, int n_frames, int max_lag, double* out, double* work, hipStream_t st) {
  const int slices = tica_slices(n_frames), lag_blocks = max_lag / TICA_THREADS + 1;
  hipLaunchKernelGGL(k_autocov_partial, dim3(slices, lag_blocks), dim3(TICA_THREADS), 0, st, y, stride, n_frames, max_lag, work);
  const long long per_slice = max_lag + 1ll;
  hipLaunchKernelGGL(k_slices_reduce, dim3((unsigned)((per_slice + TICA_THREADS - 1) / TICA_THREADS)), dim3(TICA_THREADS), 0, st, work, per_slice,
                     slices, out, per_slice, (double*)nullptr);
}
