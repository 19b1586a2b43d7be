// jamun_swd.hip — the sliced Wasserstein distance of two clouds of descriptors (jamun_amd/swd.py): projection on L directions, a sort of
// every projected column over segments of frames, merges of sorted columns, and the quantile integral of two sorted columns.
//
//   k_swd_project   x [n_frames][row_stride] (fp32, `width` values read per row) and proj [width][L] (fp32) -> keys [L][n_frames] (fp32).
//   k_swd_tile_sort keys [L][n_frames] -> every tile of JAMUN_SWD_TILE keys of every segment sorted (bitonic network in LDS).
//   k_swd_merge_pass  runs of `run` sorted keys of every segment merged two and two into runs of 2 `run` (merge path, global memory).
//   k_swd_merge     a [L][n], b [L][m] (sorted) -> out [L][n + m] (sorted): the device function of the pass above on two caller's rows.
//   k_swd_w2sq_partial / k_swd_w2sq_reduce   sorted u [L][n], v [L][m] -> out [L] (fp64): the integral of (F^-1 - G^-1)^2 over [0, 1].
//
// BIT FOR BIT.  A key is acc = +0.0; for j ascending: acc = acc + double(x[t][j]) * double(proj[j][l]), rounded once to fp32 at the end.
// The product of two promoted fp32 values has at most 48 significant bits: it is EXACT in fp64, so a fused and an unfused accumulate
// round the same sum and give the same bits, whatever the compiler contracts.  That is what makes the keys equal swd.project_host bit
// for bit (written here with a separate multiply and add all the same).
//
// THE ORDER is that of swd.order_image, a map fp32 -> uint32 that preserves the order of the reals: all bits of a negative flipped, the
// sign bit of a non-negative set, every NaN sent to 0xFFFFFFFF.  So -0.0 < +0.0, NaN sorts last, and a sorted column is unique AS BITS
// (every NaN is written back as the quiet NaN 0x7FC00000): tile size, pass structure and merge partition cannot show in the result.
// Keys travel through global memory as fp32 and are mapped on load; nothing but the order depends on the image.
//
// SORT.  Out of place, in three kinds of step, all queued on the caller's stream.  Segment c holds the frames cuts[c-1] <= t < cuts[c]
// and is cut into tiles of JAMUN_SWD_TILE keys from its first frame.  A workgroup sorts one tile of one column in LDS (16 KB; the
// network is sized to the next power of two of the tile's keys, the padding is 0xFFFFFFFF and never written back).  Then ceil(log2(longest
// segment / tile)) passes merge neighbouring runs, ping-pong between `out` and the caller's workspace, arranged so that the last step
// writes `out`: a workgroup owns SWD_CHUNK consecutive outputs of one pair of runs, every lane finds the merge-path split of its
// SWD_ITEMS outputs by bisection on the diagonal and merges them one by one.  A run without a partner is copied.  Frames from the last
// cut on belong to no segment and are copied as they are.  `out` may be `keys` itself: a tile is read whole before it is written.
//
// W2SQ.  On the grid of n m cells u's cell i is [i m, (i + 1) m) and v's cell j is [j n, (j + 1) n).  One lane per cell of the LONGER
// side walks the cells of the shorter side it overlaps (at most ceil(short / long) + 1 = 2), forming per overlap  d = double(u_i) -
// double(v_j); sq = d * d; term = sq * double(w)  (w the overlap's integer length, int64 arithmetic), each rounded once, and adds its terms
// in ascending order.  The lanes of a workgroup are added by a tree in LDS (a fixed order), the workgroups of a column in ascending order
// by one lane, and the sum is divided by double(n m).  No floating-point atomics: two runs give the same bits.
//
// No MFMA, no inline assembly, no allocation: every buffer is the caller's.  Every index is formed in 64 bits and checked against the
// lengths the host passed; the host refuses whatever would not fit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "jamun_internal.h"

#pragma clang fp contract(off)

namespace {

constexpr int SWD_THREADS = 256;
constexpr int SWD_TILE = JAMUN_SWD_TILE;
constexpr int SWD_ITEMS = 8;                          // outputs a lane of a merge writes
constexpr int SWD_CHUNK = SWD_THREADS * SWD_ITEMS;    // outputs a workgroup of a merge writes
constexpr int SWD_PROJ_FRAMES = 32;                   // frames a workgroup of k_swd_project stages
constexpr uint32_t SWD_NAN_IMAGE = 0xFFFFFFFFu;

static_assert(SWD_TILE % SWD_CHUNK == 0, "a chunk of a merge pass lies inside one pair of runs");
static_assert((SWD_TILE & (SWD_TILE - 1)) == 0 && SWD_TILE * 4 <= 65536, "the bitonic network of a tile fits the LDS of a workgroup");
static_assert((SWD_PROJ_FRAMES * (JAMUN_SWD_MAX_WIDTH + 1) + JAMUN_SWD_MAX_WIDTH * JAMUN_SWD_MAX_PROJ) * 4 <= 65536, "k_swd_project: LDS");

__device__ __forceinline__ uint32_t image_of(float f) {
  const uint32_t b = __float_as_uint(f);
  if ((b & 0x7FFFFFFFu) > 0x7F800000u) return SWD_NAN_IMAGE;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ float key_of(uint32_t image) {
  if (image == SWD_NAN_IMAGE) return __uint_as_float(0x7FC00000u);
  return __uint_as_float((image & 0x80000000u) ? (image ^ 0x80000000u) : ~image);
}

// The unit-th block of `unit` frames among the segments, counted segment by segment: first frame of the segment, its length, the block's
// index inside it.  False behind the last block.
__device__ __forceinline__ bool find_block(const JamunHistCuts& cuts, int unit, int q, int* first, int* len, int* local) {
  int start = 0;
  for (int c = 0; c < cuts.n; ++c) {
    const int l = cuts.cut[c] - start, nb = (l + unit - 1) / unit;
    if (q < nb) {
      *first = start;
      *len = l;
      *local = q;
      return true;
    }
    q -= nb;
    start = cuts.cut[c];
  }
  return false;
}

__global__ void __launch_bounds__(SWD_THREADS)
k_swd_project(const float* __restrict__ x, long long row_stride, int n_frames, int width, const float* __restrict__ proj, int n_proj,
              float* __restrict__ out) {
  __shared__ float s_x[SWD_PROJ_FRAMES][JAMUN_SWD_MAX_WIDTH + 1];
  __shared__ float s_p[JAMUN_SWD_MAX_WIDTH * JAMUN_SWD_MAX_PROJ];
  const long long t0 = (long long)blockIdx.x * SWD_PROJ_FRAMES;
  const int nf = (int)min((long long)SWD_PROJ_FRAMES, n_frames - t0);
  for (int e = threadIdx.x; e < width * n_proj; e += SWD_THREADS) s_p[e] = proj[e];
  for (int e = threadIdx.x; e < nf * width; e += SWD_THREADS) {
    const int f = e / width, j = e - f * width;
    s_x[f][j] = x[(t0 + f) * row_stride + j];
  }
  __syncthreads();
  const int f = threadIdx.x % SWD_PROJ_FRAMES;
  if (f >= nf) return;
  for (int l = threadIdx.x / SWD_PROJ_FRAMES; l < n_proj; l += SWD_THREADS / SWD_PROJ_FRAMES) {
    double acc = 0.0;
    for (int j = 0; j < width; ++j) acc = __dadd_rn(acc, __dmul_rn((double)s_x[f][j], (double)s_p[j * n_proj + l]));
    out[(long long)l * n_frames + t0 + f] = (float)acc;
  }
}

__global__ void __launch_bounds__(SWD_THREADS)
k_swd_tile_sort(const float* keys, int n_frames, JamunHistCuts cuts, float* out) {
  __shared__ uint32_t s_k[SWD_TILE];
  int first, len, tile;
  if (!find_block(cuts, SWD_TILE, blockIdx.x, &first, &len, &tile)) return;
  const int n = min(SWD_TILE, len - tile * SWD_TILE);  // (>= 1)
  const long long base = (long long)blockIdx.y * n_frames + first + (long long)tile * SWD_TILE;
  int p2 = 2;
  while (p2 < n) p2 <<= 1;
  for (int i = threadIdx.x; i < p2; i += SWD_THREADS) s_k[i] = i < n ? image_of(keys[base + i]) : SWD_NAN_IMAGE;
  for (int k = 2; k <= p2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      __syncthreads();
      for (int i = threadIdx.x; i < p2; i += SWD_THREADS) {
        const int o = i ^ j;
        if (o > i) {
          const uint32_t a = s_k[i], b = s_k[o];
          if (((i & k) == 0) ? (a > b) : (a < b)) {
            s_k[i] = b;
            s_k[o] = a;
          }
        }
      }
    }
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += SWD_THREADS) out[base + i] = key_of(s_k[i]);
}

// Outputs [d0, d0 + count) of the merge of the sorted a [na] and b [nb] (d0 + count <= na + nb): on a tie a goes first.
__device__ __forceinline__ void merge_range(const float* __restrict__ a, int na, const float* __restrict__ b, int nb, float* __restrict__ out,
                                            long long d0, int count) {
  long long lo = d0 > nb ? d0 - nb : 0, hi = d0 < na ? d0 : na;  // the entries of a among the first d0 outputs
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;  // (mid < na and 0 <= d0 - 1 - mid < nb inside [lo, hi))
    if (image_of(a[mid]) <= image_of(b[d0 - 1 - mid])) lo = mid + 1; else hi = mid;
  }
  long long i = lo, j = d0 - lo;
  uint32_t ka = i < na ? image_of(a[i]) : 0u, kb = j < nb ? image_of(b[j]) : 0u;
  for (int e = 0; e < count; ++e) {
    const bool take_a = j >= nb || (i < na && ka <= kb);
    out[d0 + e] = key_of(take_a ? ka : kb);
    if (take_a) {
      ++i;
      if (i < na) ka = image_of(a[i]);
    } else {
      ++j;
      if (j < nb) kb = image_of(b[j]);
    }
  }
}

__global__ void __launch_bounds__(SWD_THREADS)
k_swd_merge_pass(const float* __restrict__ src, int n_frames, JamunHistCuts cuts, int run, float* __restrict__ dst) {
  int first, len, chunk;
  if (!find_block(cuts, SWD_CHUNK, blockIdx.x, &first, &len, &chunk)) return;
  const long long o0 = (long long)chunk * SWD_CHUNK;       // first output of this workgroup, from the segment's first frame
  const long long pair0 = o0 / (2ll * run) * (2ll * run);  // first frame of the pair of runs it lies in (a chunk never spans two)
  const int na = (int)min((long long)run, len - pair0), nb = (int)min((long long)run, len - pair0 - na);
  const long long d0 = o0 - pair0 + (long long)threadIdx.x * SWD_ITEMS;
  if (d0 >= (long long)na + nb) return;
  const int count = (int)min((long long)SWD_ITEMS, (long long)na + nb - d0);
  const long long base = (long long)blockIdx.y * n_frames + first + pair0;
  merge_range(src + base, na, src + base + na, nb, dst + base, d0, count);
}

__global__ void __launch_bounds__(SWD_THREADS)
k_swd_merge(const float* __restrict__ a, long long a_stride, int n, const float* __restrict__ b, long long b_stride, int m, float* __restrict__ out) {
  const long long total = (long long)n + m, d0 = ((long long)blockIdx.x * SWD_THREADS + threadIdx.x) * SWD_ITEMS;
  if (d0 >= total) return;
  const int count = (int)min((long long)SWD_ITEMS, total - d0);
  const long long l = blockIdx.y;
  merge_range(a + l * a_stride, n, b + l * b_stride, m, out + l * total, d0, count);
}

// work [L][blocks]: the terms of the cells of the longer side a workgroup owns, added lane by lane and then by a tree
__global__ void __launch_bounds__(SWD_THREADS)
k_swd_w2sq_partial(const float* __restrict__ u, long long u_stride, int n, const float* __restrict__ v, long long v_stride, int m,
                   double* __restrict__ work) {
  __shared__ double s_sum[SWD_THREADS];
  const bool u_long = n >= m;
  const long long n_long = u_long ? n : m, n_short = u_long ? m : n;  // (a cell of the longer side is n_short wide, one of the shorter n_long)
  const float* const p_long = (u_long ? u + blockIdx.y * u_stride : v + blockIdx.y * v_stride);
  const float* const p_short = (u_long ? v + blockIdx.y * v_stride : u + blockIdx.y * u_stride);
  const long long k = (long long)blockIdx.x * SWD_THREADS + threadIdx.x;
  double acc = 0.0;
  if (k < n_long) {
    const long long lo = k * n_short, hi = lo + n_short;
    const double mine = (double)p_long[k];
    for (long long c = lo / n_long; c < n_short && c * n_long < hi; ++c) {
      const long long w = min(hi, (c + 1) * n_long) - max(lo, c * n_long);
      const double other = (double)p_short[c];
      const double d = u_long ? __dsub_rn(mine, other) : __dsub_rn(other, mine);  // (u - v)
      acc = __dadd_rn(acc, __dmul_rn(__dmul_rn(d, d), (double)w));
    }
  }
  s_sum[threadIdx.x] = acc;
  for (int s = SWD_THREADS / 2; s > 0; s >>= 1) {
    __syncthreads();
    if (threadIdx.x < s) s_sum[threadIdx.x] = __dadd_rn(s_sum[threadIdx.x], s_sum[threadIdx.x + s]);
  }
  if (threadIdx.x == 0) work[(long long)blockIdx.y * gridDim.x + blockIdx.x] = s_sum[0];
}

__global__ void __launch_bounds__(64)
k_swd_w2sq_reduce(const double* __restrict__ work, int n_blocks, int n_proj, double cells, double* __restrict__ out) {
  const int l = blockIdx.x * 64 + threadIdx.x;
  if (l >= n_proj) return;
  double acc = 0.0;
  for (int b = 0; b < n_blocks; ++b) acc = __dadd_rn(acc, work[(long long)l * n_blocks + b]);
  out[l] = __ddiv_rn(acc, cells);
}

}  // namespace

static int swd_blocks(long long n, int per) { return (int)((n + per - 1) / per); }  // (n >= 1)

static int swd_units(const JamunHistCuts& cuts, int unit) {
  int total = 0, start = 0;
  for (int c = 0; c < cuts.n; ++c) {
    total += swd_blocks(cuts.cut[c] - start, unit);
    start = cuts.cut[c];
  }
  return total;
}

static int swd_passes(const JamunHistCuts& cuts) {
  int longest = 0, start = 0, passes = 0;
  for (int c = 0; c < cuts.n; ++c) {
    longest = cuts.cut[c] - start > longest ? cuts.cut[c] - start : longest;
    start = cuts.cut[c];
  }
  for (long long run = SWD_TILE; run < longest; run *= 2) ++passes;
  return passes;
}

long long swd_sort_work_floats(int n_frames, int n_proj, const JamunHistCuts& cuts) {
  return swd_passes(cuts) > 0 ? (long long)n_frames * n_proj : 0;
}

long long swd_w2sq_work_doubles(int n, int m, int n_proj) { return (long long)swd_blocks(n > m ? n : m, SWD_THREADS) * n_proj; }

void launch_swd_project(const float* x, long long row_stride, int n_frames, int width, const float* proj, int n_proj, float* out, hipStream_t st) {
  hipLaunchKernelGGL(k_swd_project, dim3(swd_blocks(n_frames, SWD_PROJ_FRAMES)), dim3(SWD_THREADS), 0, st, x, row_stride, n_frames, width, proj,
                     n_proj, out);
}

hipError_t launch_swd_sort_segments(const float* keys, int n_frames, int n_proj, const JamunHistCuts& cuts, float* out, float* work, hipStream_t st) {
  const int passes = swd_passes(cuts), last = cuts.cut[cuts.n - 1];
  if (last < n_frames && keys != out) {  // the frames of no segment
    const hipError_t e = hipMemcpy2DAsync(out + last, (size_t)n_frames * sizeof(float), keys + last, (size_t)n_frames * sizeof(float),
                                          (size_t)(n_frames - last) * sizeof(float), (size_t)n_proj, hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess) return e;
  }
  float* bufs[2] = {out, work};  // step s of passes + 1 writes bufs[(passes - s) & 1]: the last one writes out
  hipLaunchKernelGGL(k_swd_tile_sort, dim3(swd_units(cuts, SWD_TILE), n_proj), dim3(SWD_THREADS), 0, st, keys, n_frames, cuts, bufs[passes & 1]);
  int run = SWD_TILE;
  for (int s = 1; s <= passes; ++s, run *= 2)
    hipLaunchKernelGGL(k_swd_merge_pass, dim3(swd_units(cuts, SWD_CHUNK), n_proj), dim3(SWD_THREADS), 0, st, bufs[(passes - s + 1) & 1], n_frames,
                       cuts, run, bufs[(passes - s) & 1]);
  return hipSuccess;
}

void launch_swd_merge(const float* a, long long a_stride, int n, const float* b, long long b_stride, int m, int n_proj, float* out, hipStream_t st) {
  hipLaunchKernelGGL(k_swd_merge, dim3(swd_blocks((long long)n + m, SWD_CHUNK), n_proj), dim3(SWD_THREADS), 0, st, a, a_stride, n, b, b_stride, m, out);
}

void launch_swd_w2sq(const float* u, long long u_stride, int n, const float* v, long long v_stride, int m, int n_proj, double* out, double* work,
                     hipStream_t st) {
  const int blocks = swd_blocks(n > m ? n : m, SWD_THREADS);
  hipLaunchKernelGGL(k_swd_w2sq_partial, dim3(blocks, n_proj), dim3(SWD_THREADS), 0, st, u, u_stride, n, v, v_stride, m, work);
  hipLaunchKernelGGL(k_swd_w2sq_reduce, dim3(swd_blocks(n_proj, 64)), dim3(64), 0, st, work, blocks, n_proj, (double)((long long)n * m), out);
}
