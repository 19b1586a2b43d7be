// jamun_validity.hip — chemical validity of trajectory frames: per frame the number of non-bonded atom pairs that clash and the number of
// bonds whose length is off, and per bond the number of frames in which it is off.
//
//   k_validity_frames   frames [n_frames, n_atoms, 3] (fp32, any frame / atom stride in floats, the convention of jamun_traj.hip),
//                       clash_s [n (n - 1) / 2] (fp32: one threshold per pair i < j, the upper triangle in row-major order, 0 for a bonded
//                       pair), bonds [B][2] (int32) with bond_lo_s / bond_hi_s [B] (fp32) ->
//                       counts [n_frames][2] (uint32: clashes, bad bonds) and, when asked for, bond_frames [B] (uint32, added to).
//
// EVERY DECISION IS A COMPARISON OF ONE fp32 NUMBER.  s = (dx dx + dy dy) + dz dz with dx = x_j - x_i, every operation in fp32 in this
// order (the library is built with -ffp-contract=off); a pair clashes when s < clash_s, a bond is off when s < bond_lo_s or s > bond_hi_s.
// The thresholds are made on the host (validity.py: `s_below`, `s_above`) such that these are the reference's decisions on
// fl32(sqrt(s)); the kernel needs no square root, and numpy doing the same three multiplications, two additions and one comparison
// counts the same integers.  NaN compares false (no issue), s = +inf is above every bond_hi_s and below no threshold.  Nothing is
// special-cased: a bonded pair has the threshold 0, which no s lies below.
//
// ONE LANE PER FRAME, as k_superpose_frames and k_internal_coords: in a chain [n, T, 3] the frames of one atom are adjacent, so the 64
// lanes of a wave read 768 contiguous bytes per atom.  The pair (i, j) is the same for every lane, so its threshold and the bond rows
// arrive by scalar loads and no lane diverges.
//
// A WORKGROUP owns 64 frames.  It walks the atoms in CHUNKS of VAL_CHUNK: the chunk's positions are staged in LDS as [atom][xyz][lane]
// (consecutive lanes on consecutive words: no bank conflict) and every row i of the triangle that has a partner j > i in the chunk is
// run against it with its own position in registers, so a pair costs three LDS reads and no trip through L1.  A molecule of up to
// VAL_CHUNK atoms is one chunk, and then the bonds read LDS too.  Up to VAL_SPLIT_ATOMS atoms the workgroup is one wave; above, four
// waves share the 64 frames: wave w takes the rows i = w, w + 4, ... (row i has n - 1 - i pairs: interleaved rows level the waves) and
// every fourth bond, and wave 0 adds the four partial counts, passed through LDS.  A lane past n_frames touches no global memory.
//
// counts is written whole by the call.  bond_frames is zeroed by the launcher's caller (a memset queued on the same stream) and receives
// one atomic add per wave and bond: the popcount of the ballot of the lanes whose bond is off (integer adds: exact, the same in every run).
// A bond row with an index outside [0, n_atoms) is skipped and reads nothing.
//
// No MFMA, no inline assembly, no allocation: every buffer is the caller's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "jamun_internal.h"

namespace {

constexpr int VAL_LANES = 64;                           // frames of a workgroup: one per lane of each of its waves
constexpr int VAL_CHUNK = JAMUN_VALIDITY_CHUNK;         // atoms staged in LDS at a time
constexpr int VAL_SPLIT_ATOMS = JAMUN_VALIDITY_SPLIT_ATOMS;  // above this many atoms a workgroup has VAL_SPLIT_WAVES waves
constexpr int VAL_SPLIT_WAVES = 4;

struct V3 {
  float x, y, z;
};

__device__ __forceinline__ float dist2(V3 a, V3 b) {
  const float dx = b.x - a.x, dy = b.y - a.y, dz = b.z - a.z;
  return (dx * dx + dy * dy) + dz * dz;
}

__global__ void __launch_bounds__(VAL_LANES * VAL_SPLIT_WAVES)
k_validity_frames(const float* __restrict__ xyz, long long frame_stride, long long atom_stride, int n_atoms, int n_frames,
                  const float* __restrict__ clash_s, const int* __restrict__ bonds, const float* __restrict__ bond_lo_s,
                  const float* __restrict__ bond_hi_s, int n_bonds, unsigned* __restrict__ counts, unsigned* __restrict__ bond_frames) {
  extern __shared__ float s_mem[];  // [min(n_atoms, VAL_CHUNK)][3][64] positions, then [n_waves][2][64] partial counts
  const int lane = threadIdx.x & (VAL_LANES - 1);
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x / VAL_LANES);  // (uniform: what depends on it stays scalar)
  const int n_waves = (int)blockDim.x / VAL_LANES;
  const int chunk_cap = min(n_atoms, VAL_CHUNK);
  float* const s_pos = s_mem;
  unsigned* const s_part = reinterpret_cast<unsigned*>(s_mem + chunk_cap * 3 * VAL_LANES);
  const long long f0 = (long long)blockIdx.x * VAL_LANES;  // first frame of this workgroup
  const bool live = f0 + lane < n_frames;  // (a lane without a frame keeps to the barriers and touches no global memory)
  const float* const x = xyz + (live ? f0 + lane : 0) * frame_stride;

  int c0 = 0, cn = 0;  // the chunk in LDS: atoms [c0, c0 + cn)
  auto atom = [&](int a) -> V3 {  // (a is wave-uniform: a scalar branch; a dead lane reads the zeros it staged, or nothing)
    if (a >= c0 && a < c0 + cn) {
      const float* const p = s_pos + (a - c0) * 3 * VAL_LANES + lane;
      return {p[0], p[VAL_LANES], p[2 * VAL_LANES]};
    }
    if (!live) return {0.0f, 0.0f, 0.0f};
    const float* const p = x + (long long)a * atom_stride;
    return {p[0], p[1], p[2]};
  };

  unsigned clashes = 0u, bad_bonds = 0u;
  for (int next = 0; next < n_atoms; next += VAL_CHUNK) {
    __syncthreads();  // (every wave is done with the chunk before)
    c0 = next;
    cn = min(VAL_CHUNK, n_atoms - c0);
    for (int a = wave; a < cn; a += n_waves) {
      V3 p = {0.0f, 0.0f, 0.0f};
      if (live) {
        const float* const g = x + (long long)(c0 + a) * atom_stride;
        p = {g[0], g[1], g[2]};
      }
      float* const d = s_pos + a * 3 * VAL_LANES + lane;
      d[0] = p.x;
      d[VAL_LANES] = p.y;
      d[2 * VAL_LANES] = p.z;
    }
    __syncthreads();
    const int c1 = c0 + cn;
    for (int i = wave; i < c1 - 1; i += n_waves) {  // the rows with a partner j > i in this chunk
      const int j0 = max(i + 1, c0);
      const V3 pi = atom(i);
      const int row = i * (2 * n_atoms - i - 1) / 2 - i - 1;  // clash_s[row + j] is the threshold of (i, j); (n_atoms <= 2^15)
      for (int j = j0; j < c1; ++j) {
        const float* const p = s_pos + (j - c0) * 3 * VAL_LANES + lane;
        const V3 pj = {p[0], p[VAL_LANES], p[2 * VAL_LANES]};
        clashes += dist2(pi, pj) < clash_s[row + j] ? 1u : 0u;
      }
    }
  }

  for (int b = wave; b < n_bonds; b += n_waves) {  // (the last chunk is still in LDS: all atoms, where the molecule is one chunk)
    const int i = bonds[2 * b], j = bonds[2 * b + 1];
    if (i < 0 || i >= n_atoms || j < 0 || j >= n_atoms) continue;
    const float s = dist2(atom(i), atom(j));
    const bool off = live && (s < bond_lo_s[b] || s > bond_hi_s[b]);
    bad_bonds += off ? 1u : 0u;
    if (bond_frames) {
      const unsigned k = (unsigned)__popcll(__ballot(off));
      if (k != 0u && lane == 0) atomicAdd(&bond_frames[b], k);
    }
  }

  if (n_waves > 1) {
    s_part[(wave * 2 + 0) * VAL_LANES + lane] = clashes;
    s_part[(wave * 2 + 1) * VAL_LANES + lane] = bad_bonds;
    __syncthreads();
    if (wave != 0) return;
    for (int w = 1; w < n_waves; ++w) {
      clashes += s_part[(w * 2 + 0) * VAL_LANES + lane];
      bad_bonds += s_part[(w * 2 + 1) * VAL_LANES + lane];
    }
  }
  if (live) {
    counts[2 * (f0 + lane)] = clashes;
    counts[2 * (f0 + lane) + 1] = bad_bonds;
  }
}

}  // namespace

void launch_validity_frames(const float* xyz, long long frame_stride, long long atom_stride, int n_atoms, int n_frames, const float* clash_s,
                            const int* bonds, const float* bond_lo_s, const float* bond_hi_s, int n_bonds, unsigned* counts,
                            unsigned* bond_frames, hipStream_t st) {
  const int grid_x = (n_frames - 1) / VAL_LANES + 1;  // (1 <= n_frames <= 2^31 - 1: at most 2^25 workgroups)
  const int n_waves = n_atoms > VAL_SPLIT_ATOMS ? VAL_SPLIT_WAVES : 1;
  const int chunk_cap = n_atoms < VAL_CHUNK ? n_atoms : VAL_CHUNK;
  const size_t lds = ((size_t)chunk_cap * 3 + (size_t)n_waves * 2) * VAL_LANES * sizeof(float);  // (at most 50 KB)
  hipLaunchKernelGGL(k_validity_frames, dim3(grid_x), dim3(VAL_LANES * n_waves), lds, st, xyz, frame_stride, atom_stride, n_atoms, n_frames,
                     clash_s, bonds, bond_lo_s, bond_hi_s, n_bonds, counts, bond_frames);
}
