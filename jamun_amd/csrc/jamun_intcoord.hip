// jamun_intcoord.hip — internal coordinates of trajectory frames: distances, bond angles and dihedrals from a table of atom indices.
//
//   k_internal_coords   frames [n_frames, n_atoms, 3] (fp32, any frame / atom stride in floats, the convention of jamun_traj.hip) and a feature
//                       table idx [n_feat][4] (int32; the number of leading non-negative entries of a row decides the feature) ->
//                       out [n_frames][W] (fp32, contiguous), W = n_feat, or 2 n_feat with cossin:
//                         2 indices  distance  |p1 - p0|                                                      cossin: (d, 0)
//                         3 indices  angle at p1: atan2(|a x b|, a.b), a = p0 - p1, b = p2 - p1, in [0, pi]    cossin: (cos, sin)
//                         4 indices  dihedral, mdtraj's form: b1 = p1 - p0, b2 = p2 - p1, b3 = p3 - p2, c1 = b2 x b3, c2 = b1 x b2,
//                                    atan2((b1.c1) |b2|, c1.c2) in (-pi, pi], the IUPAC sign                   cossin: (cos, sin)
//                         0 or 1 indices, or an index outside [0, n_atoms): NaN (both values with cossin); nothing is read for such a row.
//
// ONE LANE PER FRAME, as k_superpose_frames: in a chain [n, T, 3] the frames of one atom are adjacent, so the 64 lanes of a wave read 768
// contiguous bytes per atom.  A workgroup is ONE wave and owns 64 frames; it walks the feature table in tiles of IC_FTILE rows
// (blockIdx.y, then in steps of gridDim.y).  The table row of a feature is the same for every lane: its address depends on the block and
// the loop counter only, so the four indices arrive by a scalar load and the choice of the formula is a scalar branch: no lane diverges.
//
// THE OUTPUT [frame][W] with one lane per frame would be a store of stride W.  The wave's tile (64 frames x up to 2 IC_FTILE values) is
// staged in LDS (rows padded to an odd length: lanes 0..63 of a column hit 64 different banks) and written out with consecutive lanes on
// consecutive floats of a frame's row: pieces of 4 * tile width bytes, and the whole 64 x W block in one piece where W fits a tile.
//
// ARITHMETIC.  The differences of the positions are formed first (fp32: exact or one rounding, and what removes the 0.5 nm a molecule
// lies off the origin), then plain fp32 products and sums in the order written (the library is built with -ffp-contract=off), sqrtf and
// atan2f; never acos (it loses half the digits near 0 and pi), no fast-math intrinsic.  cos and sin come from the atan2 arguments
// themselves, (x, y) / |(x, y)|, scaled by the larger of the two first so that neither square leaves the fp32 range: continuous across
// +-pi, and no second transcendental.  x = y = 0 (coincident atoms, a collinear triple inside a dihedral) gives what atan2f gives, 0 or
// pi by the sign of x, and (cos, sin) = (+-1, 0) with it: finite whenever the differences and their products are (|x| < 1e9 nm).  A feature with a non-finite difference
// (a NaN or Inf coordinate in one of ITS atoms in THIS frame) is NaN — explicitly: atan2f(inf, inf) would be a finite pi / 4 — and lanes
// and features share nothing, so every other value is bit for bit that of the clean run.
//
// No MFMA, no inline assembly, no allocation: every buffer is the caller's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "jamun_internal.h"

namespace {

constexpr int IC_THREADS = 64;              // one wave per workgroup
constexpr int IC_FTILE = JAMUN_INTCOORD_FTILE;  // table rows per tile (jamun_internal.h)
constexpr int IC_ROW = 2 * IC_FTILE + 1;    // floats per staged frame, padded to an odd count
constexpr int IC_MAX_GRID_Y = 1024;         // feature tiles side by side; further tiles are walked in the kernel

struct V3 {
  float x, y, z;
};

__device__ __forceinline__ V3 load3(const float* p) { return {p[0], p[1], p[2]}; }
__device__ __forceinline__ V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ float dot(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ bool finite3(V3 a) { return isfinite(a.x) && isfinite(a.y) && isfinite(a.z); }

// The angle atan2(y, x), or its (cos, sin) from the same two numbers.
__device__ __forceinline__ void emit_angle(float y, float x, bool cossin, float& v0, float& v1) {
  if (!cossin) {
    v0 = atan2f(y, x);
    v1 = 0.0f;
    return;
  }
  const float m = fmaxf(fabsf(x), fabsf(y));
  if (m == 0.0f) {  // atan2f(+-0, +-0) is 0 or pi by the sign of x
    v0 = copysignf(1.0f, x);
    v1 = 0.0f;
    return;
  }
  const float xs = x / m, ys = y / m;  // (one of them is +-1)
  const float r = sqrtf(xs * xs + ys * ys);
  v0 = xs / r;
  v1 = ys / r;
}

__global__ void __launch_bounds__(IC_THREADS)
k_internal_coords(const float* __restrict__ xyz, long long frame_stride, long long atom_stride, int n_atoms, int n_frames,
                  const int* __restrict__ idx, int n_feat, int cossin, float* __restrict__ out) {
  __shared__ float s_out[IC_THREADS * IC_ROW];
  const int lane = threadIdx.x;
  const long long f0 = (long long)blockIdx.x * IC_THREADS;  // first frame of this wave
  const int frames_here = (int)min((long long)IC_THREADS, (long long)n_frames - f0);
  const bool live = lane < frames_here;  // (a lane without a frame keeps to the barriers and touches no memory)
  const float* const x = xyz + (live ? f0 + lane : 0) * frame_stride;
  const int mult = cossin ? 2 : 1;
  const long long W = (long long)n_feat * mult;
  const float nan = __builtin_nanf("");
  const int n_tiles = (n_feat - 1) / IC_FTILE + 1;  // (n_feat >= 1)

  for (int tile = blockIdx.y; tile < n_tiles; tile += gridDim.y) {
    const int j0 = tile * IC_FTILE;
    const int nj = min(IC_FTILE, n_feat - j0);
    for (int j = 0; j < nj; ++j) {
      const int* const row = idx + 4ll * (j0 + j);  // (wave-uniform: scalar loads)
      const int i0 = row[0], i1 = row[1], i2 = row[2], i3 = row[3];
      const int k = i0 < 0 ? 0 : i1 < 0 ? 1 : i2 < 0 ? 2 : i3 < 0 ? 3 : 4;  // leading non-negative entries
      bool in_range = k >= 2 && i0 < n_atoms && i1 < n_atoms;
      if (k >= 3) in_range = in_range && i2 < n_atoms;
      if (k >= 4) in_range = in_range && i3 < n_atoms;
      float v0 = nan, v1 = nan;
      if (in_range && live) {
        const V3 p0 = load3(x + (long long)i0 * atom_stride), p1 = load3(x + (long long)i1 * atom_stride);
        if (k == 2) {
          const V3 d = sub(p1, p0);
          if (finite3(d)) {
            v0 = sqrtf(dot(d, d));
            v1 = 0.0f;
          }
        } else if (k == 3) {
          const V3 p2 = load3(x + (long long)i2 * atom_stride);
          const V3 a = sub(p0, p1), b = sub(p2, p1);
          if (finite3(a) && finite3(b)) {
            const V3 c = cross(a, b);
            emit_angle(sqrtf(dot(c, c)), dot(a, b), cossin != 0, v0, v1);
          }
        } else {
          const V3 p2 = load3(x + (long long)i2 * atom_stride), p3 = load3(x + (long long)i3 * atom_stride);
          const V3 b1 = sub(p1, p0), b2 = sub(p2, p1), b3 = sub(p3, p2);
          if (finite3(b1) && finite3(b2) && finite3(b3)) {
            const V3 c1 = cross(b2, b3), c2 = cross(b1, b2);
            emit_angle(dot(b1, c1) * sqrtf(dot(b2, b2)), dot(c1, c2), cossin != 0, v0, v1);
          }
        }
      }
      if (cossin) {
        s_out[lane * IC_ROW + 2 * j] = v0;
        s_out[lane * IC_ROW + 2 * j + 1] = v1;
      } else {
        s_out[lane * IC_ROW + j] = v0;
      }
    }
    __syncthreads();
    // the tile's [frames_here][tw] values, consecutive lanes on consecutive floats of a frame's row
    const int tw = nj * mult;
    float* const o = out + f0 * W + (long long)j0 * mult;
    for (int e = lane; e < frames_here * tw; e += IC_THREADS) {
      const int t = e / tw, c = e - t * tw;
      o[(long long)t * W + c] = s_out[t * IC_ROW + c];
    }
    __syncthreads();  // (the next tile overwrites s_out)
  }
}

}  // namespace

void launch_internal_coords(const float* xyz, long long frame_stride, long long atom_stride, int n_atoms, int n_frames, const int* idx, int n_feat,
                            int cossin, float* out, hipStream_t st) {
  const int grid_x = (n_frames - 1) / IC_THREADS + 1;  // (1 <= n_frames <= 2^31 - 1: at most 2^25 workgroups)
  const int n_tiles = (n_feat - 1) / IC_FTILE + 1;  // (n_feat >= 1, no overflow near 2^31)
  const int grid_y = n_tiles < IC_MAX_GRID_Y ? n_tiles : IC_MAX_GRID_Y;
  hipLaunchKernelGGL(k_internal_coords, dim3(grid_x, grid_y), dim3(IC_THREADS), 0, st, xyz, frame_stride, atom_stride, n_atoms, n_frames,
                     idx, n_feat, cossin, out);
}
