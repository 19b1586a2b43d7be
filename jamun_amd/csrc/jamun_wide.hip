// jamun_wide.hip — the wide path: a denoiser forward of any hidden width (a x0e + b x1e), any radial size
// (edge_attr_dim) and any embedding width, gfx950.  jamun_sampler_create selects it only for Conv models outside the
// envelope of the compiled-width kernels (jamun_stats.conv_path 3, init_path 6).  No kernel here has a compiled width
// limit; every width enters as a loop bound.
//
//   k_edge_h_wide  radial-MLP hidden layer per edge slot, any H: h~ = [SiLU(c_mask + W1r . basis(d)), 1] (H + 1 rows),
//                  in the [layer][k][slot] layout of k_edge_h, the basis exactly as k_edge_h computes it.
//   k_conv_wide    destination-grouped conv (the association of k_conv): per 32-destination tile and K-slice, each chunk
//                  (u-block x k-subgroup) of A_i[(k,u)] = sum_{e->i} h~_e[k] zeta_e[u] is formed once in LDS by the
//                  forming code of k_conv (jamun_conv_form.h) and then contracted on v_mfma_f32_32x32x2_f32 with EVERY
//                  output column tile: wave w takes tiles w, w + 4, ... over all K-steps of the chunk (one MFMA chain per
//                  tile, no cross-wave reduction) and adds its result to the tile's rows of the slice's partial slab
//                  (written by the slice's first chunk, read-modify-written by the same lanes for the later ones; the read
//                  is requested before the MFMAs).  No atomics: bit-reproducible.
//   k_node_gate_wide  sum of the slabs (fixed order), / max(deg, 1), gate; writes the node update's GEMM operands
//                  Z0 = [act(scalars) | x_in scalars] and Z1[m] = [gated vectors m | x_in vectors m] (zero-padded to K0p / K1p).
//   k_node_lin_wide   [W_self ; W_skip] contraction of Z0 / Z1 on v_mfma_f32_32x32x2_f32, one wave per (32 atoms, output
//                  column tile, plane), K looped; the noise-conditional skip mix in the epilogue.
//   k_head_wide    Lin(hidden -> gate input) . Gate . Lin(mul1 -> 1x1e) . output_gain, one wave per atom, lanes over channels.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "jamun_internal.h"
#include "jamun_conv_form.h"

#define WFSUB(a, b) __fsub_rn((a), (b))
#define WFMUL(a, b) __fmul_rn((a), (b))

// ------------------------------------------------------------------------------------------------
// radial MLP: 64 edge slots per workgroup, 4 waves over the hidden units.  The basis of a chunk of <= 64 radial functions
// is staged in LDS ([r][slot]); W1r[r][k] is a wave-uniform load.  Radial sizes above 64 accumulate over several chunks
// through the output rows (the pre-activation is parked there and activated by the last chunk).
// ------------------------------------------------------------------------------------------------
#define EHW_SLOTS 64
#define EHW_RCH 64
__global__ __launch_bounds__(256) void k_edge_h_wide(EdgeHWideArgs a) {
  __shared__ float s_rad[EHW_RCH * EHW_SLOTS];
  const int tid = threadIdx.x, sl = tid & (EHW_SLOTS - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l = a.layer0 + blockIdx.y;
  const long n_slots = (long)a.n_atoms * a.S;
  const long slot = (long)blockIdx.x * EHW_SLOTS + sl;
  const int i = slot < n_slots ? (int)(slot / a.S) : 0;
  const int t = (int)(slot - (long)i * a.S);
  const bool valid = slot < n_slots && t < a.deg[i];
  float d = 0.f;
  int bonded = 0;
  if (valid) {
    d = a.egeo[slot].w;
    bonded = a.esrc[slot] < 0 ? 1 : 0;
  }
  const int H = a.H, nr = a.nr;
  const float* __restrict__ w1r = a.w1r_all + (size_t)l * H * nr;   // [r][k]
  const float* __restrict__ cm = a.cmask_all + (size_t)l * 2 * H + (size_t)bonded * H;
  float* __restrict__ h = a.h_all + (size_t)blockIdx.y * a.h_layer_stride + slot;
  for (int rc = 0; rc < nr; rc += EHW_RCH) {
    const int rn = nr - rc < EHW_RCH ? nr - rc : EHW_RCH;
    __syncthreads();
    for (int idx = tid; idx < rn * EHW_SLOTS; idx += 256) {
      const int r = idx / EHW_SLOTS, s2 = idx - r * EHW_SLOTS;
      const long sl2 = (long)blockIdx.x * EHW_SLOTS + s2;
      float d2 = 0.f;
      if (sl2 < n_slots) d2 = a.egeo[sl2].w;
      const float diff = WFSUB(d2, a.mu[rc + r]) / a.step;
      s_rad[idx] = expf(-WFMUL(diff, diff)) / 1.12f;
    }
    __syncthreads();
    const bool last = rc + EHW_RCH >= nr;
    for (int k = wave; k < H; k += 4) {
      float acc = rc == 0 ? cm[k] : (valid ? h[(size_t)k * a.h_kstride] : 0.f);
      for (int r = 0; r < rn; ++r) acc = fmaf(w1r[(size_t)(rc + r) * H + k], s_rad[r * EHW_SLOTS + sl], acc);
      if (valid) h[(size_t)k * a.h_kstride] = last ? acc * __frcp_rn(1.f + __expf(-acc)) : acc;
    }
  }
  if (valid && wave == 0) h[(size_t)H * a.h_kstride] = 1.f;  // bias row of the second radial-MLP layer
}

void launch_edge_h_wide(const EdgeHWideArgs& a, int n_layers, hipStream_t st) {
  const long slots = (long)a.n_atoms * a.S;
  hipLaunchKernelGGL(k_edge_h_wide, dim3((unsigned)((slots + EHW_SLOTS - 1) / EHW_SLOTS), n_layers), dim3(256), 0, st, a);
}

// ------------------------------------------------------------------------------------------------
// conv contraction, any width
// ------------------------------------------------------------------------------------------------
template <int RC, int KSUB>
__device__ __forceinline__ void form_any(int ks, int type, float* A_lds, const float4* g_lds, const float* h_lds, const int* blist, int nb,
                                         const ConvArgs& a, int lane, int nu, int xcol) {
  static_assert(KSUB <= 4, "form_any dispatches k-subgroups of 1..4 hidden units");
  switch (ks) {
    case 1: form_dispatch<RC, KSUB, 1>(type, A_lds, g_lds, h_lds, blist, nb, a, lane, nu, xcol); break;
    case 2: form_dispatch<RC, KSUB, (KSUB >= 2 ? 2 : 1)>(type, A_lds, g_lds, h_lds, blist, nb, a, lane, nu, xcol); break;
    case 3: form_dispatch<RC, KSUB, (KSUB >= 3 ? 3 : 1)>(type, A_lds, g_lds, h_lds, blist, nb, a, lane, nu, xcol); break;
    default: form_dispatch<RC, KSUB, (KSUB >= 4 ? 4 : 1)>(type, A_lds, g_lds, h_lds, blist, nb, a, lane, nu, xcol); break;
  }
}

template <int RC, int KSUB>
struct WideLds {
  using L = ConvLds<RC, KSUB>;
  static size_t bytes(int S) {
    const int S4 = (S + 3) & ~3;
    return sizeof(float) * (size_t)(((RC * L::A_PLANE + 3) & ~3) + 32 * S4 * 4 + 32 * S4 * L::HST + 4 * JAMUN_MAX_BATCH);
  }
};

// (scalar rows: ~75 KB of LDS, two workgroups per CU; vector rows: one)
template <int RC, int KSUB>
__global__ __launch_bounds__(256, RC == 1 ? 2 : 1) void k_conv_wide(ConvArgs a, int nt_all) {
  using L = ConvLds<RC, KSUB>;
  extern __shared__ float4 lds4[];
  float* __restrict__ lds = reinterpret_cast<float*>(lds4);
  float* __restrict__ A_lds = lds;                                                             // [RC][KSUB*64+8][33]
  float4* __restrict__ g_lds = reinterpret_cast<float4*>(lds + ((RC * L::A_PLANE + 3) & ~3));  // [32][S4]
  float* __restrict__ h_lds = reinterpret_cast<float*>(g_lds + 32 * a.S4);                     // [32][S4][HST]
  int* __restrict__ b_lds = reinterpret_cast<int*>(h_lds + 32 * a.S4 * L::HST);                // [4 waves][JAMUN_MAX_BATCH]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, hh = lane >> 5;
  const int slice = blockIdx.x % a.n_slices;
  const int tile = blockIdx.x / a.n_slices;
  const int n0 = tile * 32;
  const size_t row_w = (size_t)RC * nt_all * 32;
  float* __restrict__ slab = a.partial + ((size_t)slice * a.n_pad + n0) * row_w;  // the tile's 32 rows of this slice's slab

  const int c_begin = a.slice_ptr[slice], c_end = a.slice_ptr[slice + 1];
  if (c_begin >= c_end) {  // (a slice without hidden units: its slab rows still have to read as zeros)
    for (size_t idx = tid; idx < 32 * row_w; idx += 256) slab[idx] = 0.f;
    return;
  }
  for (int idx = tid; idx < 32 * a.S4; idx += 256) {
    const int il = idx / a.S4, t = idx - il * a.S4;
    const int i = n0 + il;
    float4 rec = make_float4(__int_as_float(0), 0.f, 0.f, 0.f);
    if (i < a.n_atoms && t < a.deg[i]) {
      const size_t e = (size_t)i * a.S + t;
      const float4 geo = a.egeo[e];
      rec = make_float4(__int_as_float((a.esrc[e] & 0x7fffffff) * a.XS * 4), geo.x, geo.y, geo.z);
    }
    g_lds[idx] = rec;
  }
  {
    const int4 cd = a.chunks[c_begin];
    stage_h<RC, KSUB>(h_lds, a, n0, cd.y & 0xffff, cd.y >> 16, tid);
  }
  int* __restrict__ blist = b_lds + wave * JAMUN_MAX_BATCH;
  int nb;
  {
    const int i_l = n0 + wave * 8 + (lane & 7);
    const int dg = (i_l < a.n_atoms) ? a.deg[i_l] : 0;
    const int nbat = dg > 0 ? (dg + 3) >> 2 : 1;
    int pre = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int v = __shfl(nbat, k);
      if (k < (lane & 7)) pre += v;
      tot += v;
    }
    nb = __builtin_amdgcn_readfirstlane(tot);
    int pks[8], nks[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      pks[k] = __shfl(pre, k);
      nks[k] = __shfl(nbat, k);
    }
    for (int b = lane; b < nb; b += 64) {
      int ent = 0;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int pk = pks[k], nk = nks[k];
        if (b >= pk && b < pk + nk) ent = (wave * 8 + k) | (((b - pk) * 4) << 8) | ((b == pk + nk - 1 ? 1 : 0) << 24);
      }
      blist[b] = ent;
    }
  }
  __syncthreads();

  for (int ci = c_begin; ci < c_end; ++ci) {
    const int4 cd = a.chunks[ci];  // {ublk, k0 | ks << 16, first weight group, number of weight groups}
    const int4 ub = a.ublk[cd.x];  // {type, nu, xcol0, width}
    const int type = ub.x, nu = ub.y;
    const int ks = cd.y >> 16;
    const int xcol = a.lane_xoff[cd.x * 64 + lane] + ub.z;
    form_any<RC, KSUB>(ks, type, A_lds, g_lds, h_lds, blist, nb, a, lane, nu, xcol);
    {  // zero the K-step padding rows (K-steps are issued in groups of 4 = 8 rows of A)
      const int kused = ks * nu, kpad = cd.w * 8;
#pragma unroll
      for (int c = 0; c < RC; ++c)
        for (int idx = kused * A_ROW + tid; idx < kpad * A_ROW; idx += 256) A_lds[c * L::A_PLANE + idx] = 0.f;
    }
    __syncthreads();
    if (ci + 1 < c_end) {  // h~ of the next chunk (not read until the next chunk's forming)
      const int4 nx = a.chunks[ci + 1];
      stage_h<RC, KSUB>(h_lds, a, n0, nx.y & 0xffff, nx.y >> 16, tid);
    }
    const int G = cd.w;
    const bool first = ci == c_begin;
    // every output column tile against the formed chunk: wave w takes tiles w, w + 4, ... over all K-steps of the chunk
    for (int t = wave; t < nt_all; t += 4) {
      float* __restrict__ sp = slab + (size_t)t * 32 + r;
      float old[RC][16];  // the slab's running sum of this tile, requested before the MFMAs (0 for the slice's first chunk)
#pragma unroll
      for (int c = 0; c < RC; ++c)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int row = (q & 3) + 8 * (q >> 2) + 4 * hh;
          old[c][q] = first ? 0.f : sp[(size_t)row * row_w + (size_t)c * nt_all * 32];
        }
      f32x16 acc[RC];
#pragma unroll
      for (int c = 0; c < RC; ++c)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[c][q] = 0.f;
      const float4* __restrict__ wp = a.wpack + ((size_t)cd.z * nt_all + t) * 64 + lane;
      auto kgroup = [&](const float4 b, int g) {
        const int q0 = g * 4;
#pragma unroll
        for (int c = 0; c < RC; ++c) {
          const float* __restrict__ Ap = A_lds + c * L::A_PLANE + (2 * q0 + hh) * A_ROW + r;
          const float a0 = Ap[0], a1 = Ap[2 * A_ROW], a2 = Ap[4 * A_ROW], a3 = Ap[6 * A_ROW];
          acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b.x, acc[c], 0, 0, 0);
          acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b.y, acc[c], 0, 0, 0);
          acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(a2, b.z, acc[c], 0, 0, 0);
          acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(a3, b.w, acc[c], 0, 0, 0);
        }
      };
      // two weight registers used in place, alternately (the next group's fragment is requested before this group's MFMAs); G is even
      // (pack_problem pads the chunks of this kernel), so the loop has no odd tail
      float4 b0 = wp[0], b1;
      for (int g = 0; g < G; g += 2) {
        b1 = wp[(size_t)(g + 1) * nt_all * 64];
        kgroup(b0, g);
        b0 = wp[(size_t)(g + 2 < G ? g + 2 : g + 1) * nt_all * 64];
        kgroup(b1, g + 1);
      }
#pragma unroll
      for (int c = 0; c < RC; ++c)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int row = (q & 3) + 8 * (q >> 2) + 4 * hh;
          sp[(size_t)row * row_w + (size_t)c * nt_all * 32] = old[c][q] + acc[c][q];
        }
    }
    __syncthreads();  // (the next chunk's forming overwrites A)
  }
}

size_t conv_wide_lds_bytes(int rc, int S) {
  return rc == 1 ? WideLds<1, JAMUN_WIDE_KSUB0>::bytes(S) : WideLds<3, JAMUN_WIDE_KSUB1>::bytes(S);
}

int launch_conv_wide(const ConvArgs& a, int rc, int nt_all, hipStream_t st) {
  const int grid = a.n_tiles * a.n_slices;
  const size_t smem = conv_wide_lds_bytes(rc, a.S);
  if (smem > JAMUN_MAX_DYN_LDS) return -2;
  if (rc == 1) {
    hipLaunchKernelGGL((k_conv_wide<1, JAMUN_WIDE_KSUB0>), dim3(grid), dim3(256), smem, st, a, nt_all);
    return 0;
  }
  if (rc == 3) {
    hipLaunchKernelGGL((k_conv_wide<3, JAMUN_WIDE_KSUB1>), dim3(grid), dim3(256), smem, st, a, nt_all);
    return 0;
  }
  return -1;
}

int conv_wide_set_max_lds() {
  hipError_t e = hipFuncSetAttribute((const void*)k_conv_wide<1, JAMUN_WIDE_KSUB0>, hipFuncAttributeMaxDynamicSharedMemorySize, JAMUN_MAX_DYN_LDS);
  if (e == hipSuccess)
    e = hipFuncSetAttribute((const void*)k_conv_wide<3, JAMUN_WIDE_KSUB1>, hipFuncAttributeMaxDynamicSharedMemorySize, JAMUN_MAX_DYN_LDS);
  return e == hipSuccess ? 0 : -1;
}

// ------------------------------------------------------------------------------------------------
// node update, any width
// ------------------------------------------------------------------------------------------------
// one thread per element of Z0 [n_atoms][K0p] and Z1 [3][n_atoms][K1p]
__global__ __launch_bounds__(256) void k_node_gate_wide(NodeWideArgs a) {
  const long n0e = (long)a.n_atoms * a.K0p, n1e = 3L * a.n_atoms * a.K1p;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n0e + n1e) return;
  const size_t w0 = (size_t)a.nt0 * 32, w1 = (size_t)3 * a.nt1 * 32;
  auto slab_sum0 = [&](int i, int w) {
    float s = 0.f;
    for (int sl = 0; sl < a.n_slices; ++sl) s += a.partial0[((size_t)sl * a.n_pad + i) * w0 + w];
    return s;
  };
  if (idx < n0e) {
    const int i = (int)(idx / a.K0p), k = (int)(idx - (long)i * a.K0p);
    const float dg = (float)max(a.deg[i], 1);
    float v = 0.f;
    if (k < a.mul0) {
      const float val = slab_sum0(i, k) / dg;
      v = a.cL * (val > 0.f ? val : 0.01f * val);
    } else if (k < a.mul0 + a.in0) {
      v = a.x_in[(size_t)i * a.XSin + (k - a.mul0)];
    }
    a.z0[idx] = v;
    return;
  }
  const long j = idx - n0e;
  const int m = (int)(j / ((long)a.n_atoms * a.K1p));
  const long rem = j - (long)m * a.n_atoms * a.K1p;
  const int i = (int)(rem / a.K1p), k = (int)(rem - (long)i * a.K1p);
  const float dg = (float)max(a.deg[i], 1);
  float v = 0.f;
  if (k < a.mul1) {
    const float gate = a.cS / (1.f + expf(-(slab_sum0(i, a.mul0 + k) / dg)));
    float s = 0.f;
    for (int sl = 0; sl < a.n_slices; ++sl) s += a.partial1[((size_t)sl * a.n_pad + i) * w1 + (size_t)m * a.nt1 * 32 + k];
    v = (s / dg) * gate;
  } else if (k < a.mul1 + a.in1) {
    v = a.x_in[(size_t)i * a.XSin + a.in0 + 3 * (k - a.mul1) + m];
  }
  a.z1[(size_t)m * a.n_pad * a.K1p + (size_t)i * a.K1p + k] = v;
}

// one wave per (32 atoms, job): jobs 0..no0-1 scalar output column tiles, then plane m, vector output column tile t
__global__ __launch_bounds__(64) void k_node_lin_wide(NodeWideArgs a) {
  const int lane = threadIdx.x, r = lane & 31, hh = lane >> 5;
  const int n0 = blockIdx.x * 32, job = blockIdx.y;
  const bool scalar = job < a.no0;
  const int m = scalar ? 0 : (job - a.no0) / a.no1, t = scalar ? job : (job - a.no0) % a.no1;
  const int Kp = scalar ? a.K0p : a.K1p;
  const float* __restrict__ z = scalar ? a.z0 : a.z1 + (size_t)m * a.n_pad * a.K1p;
  const float4* __restrict__ zr = reinterpret_cast<const float4*>(z + (size_t)(n0 + r) * Kp) + hh;  // rows past the last atom are zeros
  const float4* __restrict__ w = (scalar ? a.wn0 : a.wn1) + (size_t)t * (Kp / 8) * 64 + lane;
  f32x16 acc;
#pragma unroll
  for (int q = 0; q < 16; ++q) acc[q] = 0.f;
  const int ng = Kp / 8;
  float4 an = zr[0], bn = w[0];
  for (int g = 0; g < ng; ++g) {
    const float4 av = an, bv = bn;
    const int gn = g + 1 < ng ? g + 1 : g;
    an = zr[2 * gn];
    bn = w[(size_t)gn * 64];
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bv.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bv.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bv.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bv.w, acc, 0, 0, 0);
  }
  const int col = 32 * t + r;
  const bool col_ok = scalar ? col < a.mul0 : col < a.mul1;
  const int o = scalar ? col : a.mul0 + 3 * col + m;
  const int XSo = a.mul0 + 3 * a.mul1;
  const float mw = (a.mix && col_ok) ? a.mix[scalar ? col : a.mul0 + col] : 0.f;
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int i = n0 + (q & 3) + 8 * (q >> 2) + 4 * hh;
    if (col_ok && i < a.n_atoms) {
      float v = acc[q];
      if (a.mix) v = mw * a.x_in[(size_t)i * a.XSin + o] + (1.f - mw) * v;  // hidden layers: x_in is x_old, XSin == XSo
      a.x_out[(size_t)i * XSo + o] = v;
    }
  }
}

void launch_node_wide(const NodeWideArgs& a, hipStream_t st) {
  const long n = (long)a.n_atoms * a.K0p + 3L * a.n_atoms * a.K1p;
  hipLaunchKernelGGL(k_node_gate_wide, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a);
  hipLaunchKernelGGL(k_node_lin_wide, dim3(a.n_pad / 32, a.no0 + 3 * a.no1), dim3(64), 0, st, a);
}

// ------------------------------------------------------------------------------------------------
// output head, any width: one wave per atom; lane w handles vector channels w, w + 64, ...
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_head_wide(HeadArgs a) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= a.n_atoms) return;  // (wave-uniform)
  const int XS = a.mul0 + 3 * a.mul1;
  const float* __restrict__ xi = a.x + (size_t)i * XS;
  float gx = 0.f, gy = 0.f, gz = 0.f;
  for (int w = lane; w < a.mul1; w += 64) {
    float gp = 0.f;
    for (int u = 0; u < a.mul0; ++u) gp = fmaf(a.w_gate[(size_t)u * a.mul1 + w], xi[u], gp);
    float hx = 0.f, hy = 0.f, hz = 0.f;
    for (int u = 0; u < a.mul1; ++u) {
      const float ww = a.w_vec[(size_t)u * a.mul1 + w];
      hx = fmaf(ww, xi[a.mul0 + 3 * u + 0], hx);
      hy = fmaf(ww, xi[a.mul0 + 3 * u + 1], hy);
      hz = fmaf(ww, xi[a.mul0 + 3 * u + 2], hz);
    }
    const float gate = a.cS / (1.f + expf(-gp));
    const float wo = a.w_out[w];
    gx = fmaf(wo, hx * gate, gx);
    gy = fmaf(wo, hy * gate, gy);
    gz = fmaf(wo, hz * gate, gz);
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {  // fixed butterfly: the same order on every run
    gx += __shfl_xor(gx, off);
    gy += __shfl_xor(gy, off);
    gz += __shfl_xor(gz, off);
  }
  if (lane == 0) {
    a.g[(size_t)i * 3 + 0] = gx;
    a.g[(size_t)i * 3 + 1] = gy;
    a.g[(size_t)i * 3 + 2] = gz;
  }
}

void launch_head_wide(const HeadArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(k_head_wide, dim3((a.n_atoms + 3) / 4), dim3(256), 0, st, a);
}
