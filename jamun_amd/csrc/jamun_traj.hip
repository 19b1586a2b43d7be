// jamun_traj.hip — trajectory file encoders: device frames (fp32, nm) -> the bytes jamun_amd/pdb.py writes.
//
//   k_encode_pdb   models first_model .. first_model + F - 1 of ONE molecule as PDB text, byte for byte what save_pdb prints:
//                  "MODEL        {t}\n" (unpadded number: the length varies with t) + a body that is constant per molecule apart from the
//                  3 x 8 coordinate characters of every atom.  The host prints the body once (pdb_model_template) and passes it with the
//                  byte offset of each atom's x field.
//   k_encode_dcd   per frame three Fortran records  int32 4n | n x fp32 (coord * 10.0f) | int32 4n  for X, Y, Z: the `recs` buffer of save_dcd.
//
// Input: base pointer + frame stride + atom stride in floats (the three components of an atom are adjacent), so a [n, T, 3] chain and a
// slice of a [T, sum N, 3] trajectory are both read in place.
//
// Both kernels are pure store streams (PDB: ~80 B out per 12 B in).  k_encode_pdb works on items (frame, body tile of TRAJ_TILE bytes):
// the template tile sits in LDS as an aligned copy; every item assembles its output bytes in a second LDS buffer laid out with the SAME
// 16-byte phase as the global destination (model starts are not aligned: the text of model t starts wherever model t - 1 ended), patches the
// coordinate fields there, and streams the buffer out as aligned 16-byte vector stores with byte stores for the ragged head and tail only.
// The destination offset of a model is closed form (models up to t have t * (14 + body_len) bytes plus their digit counts, summed by decade),
// so no prefix pass runs.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "jamun_internal.h"

namespace {

constexpr int TRAJ_THREADS = 256;
constexpr int TRAJ_TILE = 24576;   // body bytes per item (a multiple of 16); a 166-atom model (~17 KB) is one item
constexpr int TRAJ_HDR_MAX = 48;   // "MODEL        " (13) + up to 19 digits + '\n', rounded up to a multiple of 16
constexpr int TRAJ_MODEL_FIXED = 14;  // bytes of the MODEL line without its digits

// digits of 0 .. x-1 summed: every number has one, and one more for each power of ten it reaches
__host__ __device__ inline long long digit_sum_below(long long x) {
  long long s = x, p = 10;
  for (int k = 1; k <= 18 && x > p; ++k, p *= 10) s += x - p;
  return s;
}
__host__ __device__ inline int digit_count(long long t) {
  int d = 1;
  long long p = 10;
  while (d < 19 && t >= p) {
    ++d;
    p *= 10;
  }
  return d;
}

// f"{v:8.3f}" of a float: q = rint(double(v) * 1000) is exact (24-bit significand x 1000 fits a double) and rint rounds ties to even, as
// Python does on the exact value; '-' iff signbit(v) (covers -0.000).  Returns the 8 characters packed little endian in (lo, hi); ok = false
// (and "   0.000") when the text would not fit 8 characters or v is not finite.
__device__ __forceinline__ bool fmt_8_3(float v, uint32_t& lo, uint32_t& hi) {
  const double q = rint((double)v * 1000.0);
  bool neg = signbit(v);
  const double aq = fabs(q);
  const bool ok = aq <= (neg ? 999999.0 : 9999999.0);  // false for NaN and inf
  const uint32_t u = ok ? (uint32_t)aq : 0u;
  neg = ok && neg;
  const uint32_t ip = u / 1000u, fp = u - ip * 1000u;
  const uint32_t d0 = ip % 10u, d1 = (ip / 10u) % 10u, d2 = (ip / 100u) % 10u, d3 = ip / 1000u;
  const uint32_t c3 = '0' + d0;
  const uint32_t c2 = ip >= 10u ? '0' + d1 : (neg ? '-' : ' ');
  const uint32_t c1 = ip >= 100u ? '0' + d2 : ((neg && ip >= 10u) ? '-' : ' ');
  const uint32_t c0 = ip >= 1000u ? '0' + d3 : ((neg && ip >= 100u) ? '-' : ' ');
  lo = c0 | (c1 << 8) | (c2 << 16) | (c3 << 24);
  hi = (uint32_t)'.' | (('0' + fp / 100u) << 8) | (('0' + (fp / 10u) % 10u) << 16) | (('0' + fp % 10u) << 24);
  return ok;
}

// character q of "MODEL        {t}\n" (d = digits of t)
__device__ __forceinline__ uint32_t model_line_char(int q, long long t, int d) {
  if (q < 5) return (uint32_t)((0x4c45444f4dull >> (8 * q)) & 0xff);  // "MODEL"
  if (q < 13) return ' ';
  if (q == 13 + d) return '\n';
  long long p = 1;
  for (int k = 13 + d - 1 - q; k > 0; --k) p *= 10;
  return '0' + (uint32_t)((t / p) % 10);
}

__global__ void __launch_bounds__(TRAJ_THREADS)
k_encode_pdb(const float* __restrict__ xyz, long long frame_stride, long long atom_stride, int n_atoms, int n_frames, long long first_model,
             const unsigned char* __restrict__ body, int body_len, const int* __restrict__ coord_off, unsigned char* __restrict__ out,
             unsigned int* __restrict__ unencodable) {
  __shared__ __attribute__((aligned(16))) unsigned char s_tmpl[TRAJ_TILE + 16];                // template tile, aligned copy (+ slack for the funnel read)
  __shared__ __attribute__((aligned(16))) unsigned char s_stage[TRAJ_TILE + TRAJ_HDR_MAX + 32];  // output bytes, in the destination's 16-byte phase
  uint32_t* const tmpl32 = reinterpret_cast<uint32_t*>(s_tmpl);
  uint32_t* const stage32 = reinterpret_cast<uint32_t*>(s_stage);
  const int tid = threadIdx.x;
  const int n_tiles = (body_len + TRAJ_TILE - 1) / TRAJ_TILE;
  const long long n_items = (long long)n_frames * n_tiles;
  const long long model_fixed = TRAJ_MODEL_FIXED + (long long)body_len;
  const long long digits_before = digit_sum_below(first_model);
  int loaded = -1;

  for (long long w = blockIdx.x; w < n_items; w += gridDim.x) {
    const long long f = n_tiles == 1 ? w : w / n_tiles;
    const int k = n_tiles == 1 ? 0 : (int)(w - f * n_tiles);
    const int tile_lo = k * TRAJ_TILE;
    const int tile_len = min(TRAJ_TILE, body_len - tile_lo);
    if (k != loaded) {  // (every reader of the previous tile is behind the barrier that ends an item)
      const unsigned char* src = body + tile_lo;
      if ((reinterpret_cast<uintptr_t>(src) & 3) == 0) {
        const uint32_t* src32 = reinterpret_cast<const uint32_t*>(src);
        for (int j = tid; j < (tile_len >> 2); j += TRAJ_THREADS) tmpl32[j] = src32[j];
        for (int j = (tile_len & ~3) + tid; j < tile_len; j += TRAJ_THREADS) s_tmpl[j] = src[j];
      } else {
        for (int j = tid; j < tile_len; j += TRAJ_THREADS) s_tmpl[j] = src[j];
      }
      loaded = k;
      __syncthreads();
    }
    const long long t = first_model + f;
    const int d = digit_count(t);
    const int hl = k == 0 ? TRAJ_MODEL_FIXED + d : 0;  // bytes of the MODEL line in this item
    const long long g0 = f * model_fixed + (digit_sum_below(t) - digits_before) + (k == 0 ? 0 : TRAJ_MODEL_FIXED + d + tile_lo);
    const int len = hl + tile_len;
    const int a = (int)(reinterpret_cast<uintptr_t>(out + g0) & 15);  // stage byte s <-> destination byte g0 + (s - a)

    // 1. template (and MODEL line) into the stage, one aligned dword per lane: two template dwords funnelled by the phase difference
    const int n_dw = (a + len + 3) >> 2;
    for (int j = tid; j < n_dw; j += TRAJ_THREADS) {
      const int q0 = 4 * j - a;  // item-local byte of the dword's first byte
      const int u0 = q0 - hl;    // tile-local
      uint32_t v;
      if (u0 >= 0 && u0 + 4 <= tile_len) {
        const uint64_t pair = (uint64_t)tmpl32[u0 >> 2] | ((uint64_t)tmpl32[(u0 >> 2) + 1] << 32);
        v = (uint32_t)(pair >> (8 * (u0 & 3)));
      } else {
        v = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int q = q0 + i;
          uint32_t c = 0;
          if (q >= 0 && q < len) c = q < hl ? model_line_char(q, t, d) : (uint32_t)s_tmpl[q - hl];
          v |= c << (8 * i);
        }
      }
      stage32[j] = v;
    }
    __syncthreads();

    // 2. coordinate fields of the atoms whose x/y/z text meets this tile (offsets ascend; a field may straddle two tiles)
    int i0 = 0, i1 = n_atoms;
    if (n_tiles > 1) {
      int lo = 0, hi = n_atoms;
      while (lo < hi) {  // first atom whose 24 characters end behind the tile's start
        const int m = (lo + hi) >> 1;
        if (coord_off[m] + 24 > tile_lo) hi = m; else lo = m + 1;
      }
      i0 = lo;
      hi = n_atoms;
      while (lo < hi) {  // first atom whose field starts behind the tile's end
        const int m = (lo + hi) >> 1;
        if (coord_off[m] >= tile_lo + tile_len) hi = m; else lo = m + 1;
      }
      i1 = lo;
    }
    for (int e = tid; e < 3 * (i1 - i0); e += TRAJ_THREADS) {
      const int i = i0 + e / 3, c = e - 3 * (e / 3);
      const float x = xyz[f * frame_stride + (long long)i * atom_stride + c];
      uint32_t lo, hi;
      const bool ok = fmt_8_3(__fmul_rn(x, 10.0f), lo, hi);
      const int u = coord_off[i] + 8 * c - tile_lo;  // tile-local byte of the field's first character
      if (!ok && u >= 0 && u < tile_len) atomicAdd(unencodable, 1u);  // (counted once: in the tile that holds the field's first byte)
      const uint64_t txt = (uint64_t)lo | ((uint64_t)hi << 32);
#pragma unroll
      for (int b = 0; b < 8; ++b)
        if (u + b >= 0 && u + b < tile_len) s_stage[a + hl + u + b] = (unsigned char)(txt >> (8 * b));
    }
    __syncthreads();

    // 3. out: whole 16-byte lines as vector stores; the ragged first and last line byte by byte (their other bytes belong to the neighbours)
    unsigned char* const gbase = out + g0 - a;  // 16-byte aligned
    const int n_lines = (a + len + 15) >> 4;
    for (int l = tid; l < n_lines; l += TRAJ_THREADS) {
      const int b0 = 16 * l;
      if (b0 >= a && b0 + 16 <= a + len) {
        *reinterpret_cast<uint4*>(gbase + b0) = *reinterpret_cast<const uint4*>(s_stage + b0);
      } else {
        for (int b = max(b0, a); b < min(b0 + 16, a + len); ++b) gbase[b] = s_stage[b];
      }
    }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(TRAJ_THREADS)
k_encode_dcd(const float* __restrict__ xyz, long long frame_stride, long long atom_stride, int n_atoms, int n_frames, uint32_t* __restrict__ out,
             int wide) {
  const int rec = n_atoms + 2;  // dwords of one record: marker, n values, marker
  const long long per = 3ll * rec, total = per * n_frames;
  const uint32_t marker = 4u * (uint32_t)n_atoms;
  for (long long g = 4ll * (blockIdx.x * (long long)TRAJ_THREADS + threadIdx.x); g < total; g += 4ll * TRAJ_THREADS * gridDim.x) {
    long long f = g / per;
    int r = (int)(g - f * per);
    int c = r / rec, p = r - c * rec;
    uint32_t v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[i] = marker;
      if (g + i < total && p > 0 && p <= n_atoms) v[i] = __float_as_uint(__fmul_rn(xyz[f * frame_stride + (long long)(p - 1) * atom_stride + c], 10.0f));
      if (++p == rec) {
        p = 0;
        if (++c == 3) {
          c = 0;
          ++f;
        }
      }
    }
    if (wide && g + 4 <= total) {
      *reinterpret_cast<uint4*>(out + g) = make_uint4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (g + i < total) out[g + i] = v[i];
    }
  }
}

}  // namespace

long long pdb_models_nbytes(long long body_len, long long first_model, long long n_frames) {
  return n_frames * (TRAJ_MODEL_FIXED + body_len) + digit_sum_below(first_model + n_frames) - digit_sum_below(first_model);
}

void launch_encode_pdb(const float* xyz, long long frame_stride, long long atom_stride, int n_atoms, int n_frames, long long first_model,
                       const unsigned char* body, int body_len, const int* coord_off, unsigned char* out, unsigned int* unencodable, hipStream_t st) {
  const long long n_items = (long long)n_frames * ((body_len + TRAJ_TILE - 1) / TRAJ_TILE);
  const int grid = (int)std::min<long long>(n_items, 2048);
  hipLaunchKernelGGL(k_encode_pdb, dim3(grid), dim3(TRAJ_THREADS), 0, st, xyz, frame_stride, atom_stride, n_atoms, n_frames, first_model, body, body_len,
                     coord_off, out, unencodable);
}

void launch_encode_dcd(const float* xyz, long long frame_stride, long long atom_stride, int n_atoms, int n_frames, unsigned char* out, hipStream_t st) {
  const long long total = 3ll * (n_atoms + 2) * n_frames;
  const int grid = (int)std::min<long long>((total + 4ll * TRAJ_THREADS - 1) / (4ll * TRAJ_THREADS), 2048);
  const int wide = (reinterpret_cast<uintptr_t>(out) & 15) == 0;
  hipLaunchKernelGGL(k_encode_dcd, dim3(grid), dim3(TRAJ_THREADS), 0, st, xyz, frame_stride, atom_stride, n_atoms, n_frames,
                     reinterpret_cast<uint32_t*>(out), wide);
}
