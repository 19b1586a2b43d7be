// jamun_conv_form.h — the forming half of the destination-grouped general conv (shared by k_conv in jamun_conv.hip and
// k_conv_wide in jamun_wide.hip): per chunk (u-block x k-subgroup) each wave builds the A rows
// A[(kk,u)][atom] = sum_{e->atom} h~_e[k0+kk] zeta_e[u] of 8 destination atoms in LDS (transposed, row stride A_ROW).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "jamun_internal.h"
#include "jamun_dev.h"

#define A_ROW 33

template <int RC, int KSUB>
struct ConvLds {
  static constexpr int A_PLANE = (KSUB * 64 + 8) * A_ROW;  // floats per plane of the transposed A tile
  static constexpr int HST = KSUB <= 2 ? 2 : (KSUB <= 4 ? 4 : 8);  // record stride (floats) of the staged h~ values
};

// One batch = up to 4 in-edges of one destination atom.  load_batch() issues every memory operation of the batch
// (LDS broadcast records + one coalesced global feature load per edge); compute_batch() consumes registers only, so
// two batches can be kept in flight (double buffering below) and the loads of batch b+1 overlap the FMAs of batch b.
template <int RC, int KS, int TYPE>
struct EdgeBatch {
  static constexpr int NX = (TYPE == JAMUN_T_X0 || TYPE == JAMUN_T_X0V) ? 1 : 3;
  float4 gj[4];
  float hk[4][KS];
  float xv[4][NX];
  int il, last;
};

template <int RC, int KSUB, int KS, int TYPE>
__device__ __forceinline__ void load_batch(EdgeBatch<RC, KS, TYPE>& B, int entry, const float4* __restrict__ g_lds,
                                           const float* __restrict__ h_lds, const ConvArgs& a, int xc) {
  using L = ConvLds<RC, KSUB>;
  // entry: il | t0 << 8 | last << 24   (wave-uniform).  Edge slots are padded to a multiple of 4 per atom: padding
  // slots carry h~ = 0 and a valid source row, so no per-edge predicate is needed.
  B.il = entry & 0xff;
  B.last = entry >> 24;
  const int slot0 = B.il * a.S4 + ((entry >> 8) & 0xff);
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    B.gj[u] = g_lds[slot0 + u];
#pragma unroll
    for (int kk = 0; kk < KS; ++kk) B.hk[u][kk] = h_lds[(size_t)(slot0 + u) * L::HST + kk];
  }
  const char* __restrict__ xb = reinterpret_cast<const char*>(a.x) + xc * 4;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int off = __builtin_amdgcn_readfirstlane(__float_as_int(B.gj[u].x));  // byte offset of the source row
    const float* __restrict__ xp = reinterpret_cast<const float*>(xb + off);
#pragma unroll
    for (int q = 0; q < EdgeBatch<RC, KS, TYPE>::NX; ++q) B.xv[u][q] = xp[q];
  }
}

template <int RC, int KSUB, int KS, int TYPE>
__device__ __forceinline__ void compute_batch(const EdgeBatch<RC, KS, TYPE>& B, float (&g)[RC][KS], float* __restrict__ A_lds,
                                              int nu, int lane, bool active, bool is_cross) {
  using L = ConvLds<RC, KSUB>;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    {
      const float4 gj = B.gj[u];
      float z[RC];
      if (TYPE == JAMUN_T_X0) {
        z[0] = B.xv[u][0];
      } else if (TYPE == JAMUN_T_DOT) {
        z[0] = B.xv[u][0] * gj.y + B.xv[u][EdgeBatch<RC, KS, TYPE>::NX > 1 ? 1 : 0] * gj.z + B.xv[u][EdgeBatch<RC, KS, TYPE>::NX > 2 ? 2 : 0] * gj.w;
      } else if (TYPE == JAMUN_T_X0V) {
        const float x0 = B.xv[u][0];
        z[0] = x0 * gj.y;
        if (RC == 3) { z[1 % RC] = x0 * gj.z; z[2 % RC] = x0 * gj.w; }
      } else {  // JAMUN_T_X1C: first half of the lanes x1[u'][m], second half (x1[u'] x vhat)[m]
        const float x0 = B.xv[u][0], x1 = B.xv[u][EdgeBatch<RC, KS, TYPE>::NX > 1 ? 1 : 0], x2 = B.xv[u][EdgeBatch<RC, KS, TYPE>::NX > 2 ? 2 : 0];
        const float cx = x1 * gj.w - x2 * gj.z, cy = x2 * gj.y - x0 * gj.w, cz = x0 * gj.z - x1 * gj.y;
        z[0] = is_cross ? cx : x0;
        if (RC == 3) { z[1 % RC] = is_cross ? cy : x1; z[2 % RC] = is_cross ? cz : x2; }
      }
#pragma unroll
      for (int c = 0; c < RC; ++c)
#pragma unroll
        for (int kk = 0; kk < KS; ++kk) g[c][kk] = fmaf(B.hk[u][kk], z[c], g[c][kk]);
    }
  }
  if (B.last) {  // wave-uniform: this batch closes its destination atom
    if (active) {
#pragma unroll
      for (int c = 0; c < RC; ++c)
#pragma unroll
        for (int kk = 0; kk < KS; ++kk) A_lds[c * L::A_PLANE + (kk * nu + lane) * A_ROW + B.il] = g[c][kk];
    }
#pragma unroll
    for (int c = 0; c < RC; ++c)
#pragma unroll
      for (int kk = 0; kk < KS; ++kk) g[c][kk] = 0.f;
  }
}

template <int RC, int KSUB, int KS, int TYPE>
__device__ __forceinline__ void form_rows(float* __restrict__ A_lds, const float4* __restrict__ g_lds,
                                          const float* __restrict__ h_lds, const int* __restrict__ blist, int nb,
                                          const ConvArgs& a, int lane, int nu, int xcol) {
  const bool active = lane < nu;
  const bool is_cross = (xcol & JAMUN_XOFF_CROSS) != 0;
  const int xc = xcol & 0xffff;
  float g[RC][KS];
#pragma unroll
  for (int c = 0; c < RC; ++c)
#pragma unroll
    for (int kk = 0; kk < KS; ++kk) g[c][kk] = 0.f;
  EdgeBatch<RC, KS, TYPE> B0, B1;
  load_batch<RC, KSUB, KS, TYPE>(B0, __builtin_amdgcn_readfirstlane(blist[0]), g_lds, h_lds, a, xc);
  for (int b = 0; b < nb; b += 2) {
    if (b + 1 < nb) load_batch<RC, KSUB, KS, TYPE>(B1, __builtin_amdgcn_readfirstlane(blist[b + 1]), g_lds, h_lds, a, xc);
    compute_batch<RC, KSUB, KS, TYPE>(B0, g, A_lds, nu, lane, active, is_cross);
    if (b + 2 < nb) load_batch<RC, KSUB, KS, TYPE>(B0, __builtin_amdgcn_readfirstlane(blist[b + 2]), g_lds, h_lds, a, xc);
    if (b + 1 < nb) compute_batch<RC, KSUB, KS, TYPE>(B1, g, A_lds, nu, lane, active, is_cross);
  }
}

template <int RC, int KSUB, int KS>
__device__ __forceinline__ void form_dispatch(int type, float* A_lds, const float4* g_lds, const float* h_lds,
                                              const int* blist, int nb, const ConvArgs& a, int lane, int nu, int xcol) {
  if (RC == 1) {
    if (type == JAMUN_T_X0) form_rows<RC, KSUB, KS, JAMUN_T_X0>(A_lds, g_lds, h_lds, blist, nb, a, lane, nu, xcol);
    else form_rows<RC, KSUB, KS, JAMUN_T_DOT>(A_lds, g_lds, h_lds, blist, nb, a, lane, nu, xcol);
  } else {
    if (type == JAMUN_T_X0V) form_rows<RC, KSUB, KS, JAMUN_T_X0V>(A_lds, g_lds, h_lds, blist, nb, a, lane, nu, xcol);
    else form_rows<RC, KSUB, KS, JAMUN_T_X1C>(A_lds, g_lds, h_lds, blist, nb, a, lane, nu, xcol);
  }
}

// stage the h~ values of one chunk's k-subgroup for every edge slot of the tile
template <int RC, int KSUB>
__device__ __forceinline__ void stage_h(float* __restrict__ h_lds, const ConvArgs& a, int n0, int k0, int ks, int tid) {
  using L = ConvLds<RC, KSUB>;
  const int per_node = a.S4 * ks;
  for (int idx = tid; idx < 32 * per_node; idx += 256) {
    const int il = idx / per_node, rem = idx - il * per_node;
    const int t = rem / ks, kk = rem - t * ks;
    const int i = n0 + il;
    float v = 0.f;  // padding slots (t >= deg) contribute nothing
    if (i < a.n_atoms && t < a.deg[i]) v = a.h[(size_t)(k0 + kk) * a.h_kstride + (size_t)i * a.S + t];
    h_lds[((size_t)il * a.S4 + t) * L::HST + kk] = v;
  }
}

