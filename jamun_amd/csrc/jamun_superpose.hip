// jamun_superpose.hip — rigid superposition of trajectory frames on a reference structure, and the per-frame RMSD to it.
//
//   k_superpose_frames   frames [n_frames, n_atoms, 3] (fp32, any frame / atom stride in floats, the convention of jamun_traj.hip) ->
//                        aligned = R (x - c_x) + c_ref with the proper rotation R (det +1) that minimises sum_i |aligned_i - ref_i|^2, and
//                        rmsd = sqrt(mean_i |aligned_i - ref_i|^2).  What mdtraj's Trajectory.superpose does per frame on the host.
//
// ONE LANE PER FRAME.  In a chain [n, T, 3] the frames of one atom are adjacent (frame stride 3 floats), so the 64 lanes of a wave read
// 768 contiguous bytes per atom and write as many; the loop over atoms runs in registers.  The reference is the same for every lane: a
// workgroup stages it in LDS (tiles of SP_TILE atoms, any n_atoms) and every lane reads the same address (an LDS broadcast, no bank
// conflict).  A workgroup is ONE wave: the frames of a chain are few (20 000 frames = 313 waves for 1024 SIMDs), and waves that share no
// workgroup spread over the CUs; the per-workgroup staging of the reference is n_atoms * 12 bytes out of L2.
//
// Per frame, three passes over its atoms (the frame is read three times and written once; the second and third read hit L2):
//   1. centroid c_x.  The three sums run in fp64: an fp32 running sum over n atoms loses log2(n) bits exactly where the result shifts EVERY
//      atom of the aligned frame.  Everything else is fp32.
//   2. covariance S_ab = sum_i (x_i - c_x)_a (ref_i - c_ref)_b of the CENTRED coordinates (uncentred sums cancel in fp32).
//   3. aligned_i = R (x_i - c_x) + c_ref, written out, and |aligned_i - ref_i|^2 accumulated from those very values (the closed form
//      G_x + G_ref - 2 lambda cancels when the RMSD is small).
// Between 2 and 3: Horn's 4x4 symmetric matrix N(S) (Horn 1987, J. Opt. Soc. Am. A 4, 629); its top eigenvector is the unit quaternion
// of the optimal PROPER rotation (a quaternion cannot describe a reflection: the mirror image of the reference gets the best rotation,
// with rmsd > 0, as mdtraj's rule demands).  The eigenvector comes from SP_SWEEPS cyclic Jacobi sweeps with the rotations accumulated: the
// method has no special direction (a 180 degree turn, w = 0, is a quaternion like any other), handles a degenerate top eigenvalue
// (rank-deficient S: one or two atoms, collinear atoms: it returns SOME optimal rotation) and runs the same instructions in every lane.
// The quaternion is normalised by its norm, never by a component.  A frame with a non-finite value yields a non-finite frame and rmsd and
// nothing else: lanes share nothing but the reference.
//
// The reference centroid is formed once per workgroup, in fp64 in a fixed order, so every workgroup of a launch holds the same value.
// No MFMA, no inline assembly, no allocation: every buffer is the caller's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "jamun_internal.h"
#include "jamun_dev.h"

namespace {

constexpr int SP_THREADS = 64;   // one wave per workgroup
constexpr int SP_TILE = 256;     // reference atoms staged in LDS at a time (3 KiB: LDS never bounds the waves per CU)
constexpr int SP_SWEEPS = 6;     // cyclic Jacobi sweeps (jacobi_rotate, jamun_dev.h) of the 4x4 matrix: fp32 converges in 4 (quadratically); 6 leaves margin for near-degenerate pairs

__global__ void __launch_bounds__(SP_THREADS)
k_superpose_frames(const float* xyz, long long frame_stride, long long atom_stride, int n_atoms, int n_frames, const float* __restrict__ ref,
                   float* out, long long out_frame_stride, long long out_atom_stride, float* __restrict__ rmsd) {
  __shared__ float s_ref[3 * SP_TILE];
  __shared__ double s_sum[3];
  const int tid = threadIdx.x;
  const long long f = (long long)blockIdx.x * SP_THREADS + tid;
  const bool live = f < n_frames;  // (a lane without a frame keeps to the barriers and touches no memory but the reference)
  const float* const x = xyz + (live ? f : 0) * frame_stride;
  float* const o = out + (live ? f : 0) * out_frame_stride;

  // reference centroid: lane t sums atoms t, t + 64, ... in fp64; lanes 0..2 add the 64 partial sums of one component each, in lane order
  {
    __shared__ double s_part[3 * SP_THREADS];
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    for (int i = tid; i < n_atoms; i += SP_THREADS) {
      a0 += (double)ref[3ll * i + 0];
      a1 += (double)ref[3ll * i + 1];
      a2 += (double)ref[3ll * i + 2];
    }
    s_part[tid] = a0;
    s_part[SP_THREADS + tid] = a1;
    s_part[2 * SP_THREADS + tid] = a2;
    __syncthreads();
    if (tid < 3) {
      double a = 0.0;
      for (int l = 0; l < SP_THREADS; ++l) a += s_part[tid * SP_THREADS + l];
      s_sum[tid] = a / (double)n_atoms;
    }
    __syncthreads();
  }
  const float cr0 = (float)s_sum[0], cr1 = (float)s_sum[1], cr2 = (float)s_sum[2];

  // 1. centroid of the frame
  float cx0 = 0.0f, cx1 = 0.0f, cx2 = 0.0f;
  if (live) {
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
#pragma unroll 4
    for (int i = 0; i < n_atoms; ++i) {
      const float* p = x + (long long)i * atom_stride;
      a0 += (double)p[0];
      a1 += (double)p[1];
      a2 += (double)p[2];
    }
    cx0 = (float)(a0 / (double)n_atoms);
    cx1 = (float)(a1 / (double)n_atoms);
    cx2 = (float)(a2 / (double)n_atoms);
  }

  // 2. covariance of the centred coordinates, S_ab = sum_i (x_i - c_x)_a (ref_i - c_ref)_b
  float sxx = 0.0f, sxy = 0.0f, sxz = 0.0f, syx = 0.0f, syy = 0.0f, syz = 0.0f, szx = 0.0f, szy = 0.0f, szz = 0.0f;
  for (int i0 = 0; i0 < n_atoms; i0 += SP_TILE) {
    const int m = min(SP_TILE, n_atoms - i0);
    if (i0 > 0) __syncthreads();  // (every reader of the previous tile is done)
    for (int j = tid; j < 3 * m; j += SP_THREADS) s_ref[j] = ref[3ll * i0 + j];
    __syncthreads();
    if (live) {
#pragma unroll 4
      for (int i = 0; i < m; ++i) {
        const float* p = x + (long long)(i0 + i) * atom_stride;
        const float x0 = p[0] - cx0, x1 = p[1] - cx1, x2 = p[2] - cx2;
        const float r0 = s_ref[3 * i + 0] - cr0, r1 = s_ref[3 * i + 1] - cr1, r2 = s_ref[3 * i + 2] - cr2;
        sxx += x0 * r0;
        sxy += x0 * r1;
        sxz += x0 * r2;
        syx += x1 * r0;
        syy += x1 * r1;
        syz += x1 * r2;
        szx += x2 * r0;
        szy += x2 * r1;
        szz += x2 * r2;
      }
    }
  }

  // Horn's matrix N(S): q^T N q = sum_i (ref_i - c_ref) . R(q) (x_i - c_x) for a unit quaternion q = (w, x, y, z)
  float a00 = sxx + syy + szz, a11 = sxx - syy - szz, a22 = syy - sxx - szz, a33 = szz - sxx - syy;
  float a01 = syz - szy, a02 = szx - sxz, a03 = sxy - syx, a12 = sxy + syx, a13 = szx + sxz, a23 = syz + szy;
  float v00 = 1.0f, v01 = 0.0f, v02 = 0.0f, v03 = 0.0f;  // v[row][column]: the columns become the eigenvectors
  float v10 = 0.0f, v11 = 1.0f, v12 = 0.0f, v13 = 0.0f;
  float v20 = 0.0f, v21 = 0.0f, v22 = 1.0f, v23 = 0.0f;
  float v30 = 0.0f, v31 = 0.0f, v32 = 0.0f, v33 = 1.0f;
  for (int sweep = 0; sweep < SP_SWEEPS; ++sweep) {
    jacobi_rotate(a00, a11, a01, a02, a12, a03, a13, v00, v01, v10, v11, v20, v21, v30, v31);  // (0, 1): other rows 2, 3
    jacobi_rotate(a00, a22, a02, a01, a12, a03, a23, v00, v02, v10, v12, v20, v22, v30, v32);  // (0, 2): other rows 1, 3
    jacobi_rotate(a00, a33, a03, a01, a13, a02, a23, v00, v03, v10, v13, v20, v23, v30, v33);  // (0, 3): other rows 1, 2
    jacobi_rotate(a11, a22, a12, a01, a02, a13, a23, v01, v02, v11, v12, v21, v22, v31, v32);  // (1, 2): other rows 0, 3
    jacobi_rotate(a11, a33, a13, a01, a03, a12, a23, v01, v03, v11, v13, v21, v23, v31, v33);  // (1, 3): other rows 0, 2
    jacobi_rotate(a22, a33, a23, a02, a03, a12, a13, v02, v03, v12, v13, v22, v23, v32, v33);  // (2, 3): other rows 0, 1
  }
  // column of the largest eigenvalue (the first of equals) by a tournament of two-way selects: no runtime-indexed register array
  const bool hi01 = a11 > a00, hi23 = a33 > a22;
  const float t01 = hi01 ? a11 : a00, w01 = hi01 ? v01 : v00, x01 = hi01 ? v11 : v10, y01 = hi01 ? v21 : v20, z01 = hi01 ? v31 : v30;
  const float t23 = hi23 ? a33 : a22, w23 = hi23 ? v03 : v02, x23 = hi23 ? v13 : v12, y23 = hi23 ? v23 : v22, z23 = hi23 ? v33 : v32;
  const bool hi = t23 > t01;
  float qw = hi ? w23 : w01, qx = hi ? x23 : x01, qy = hi ? y23 : y01, qz = hi ? z23 : z01;
  if (!(a00 == a00 && a11 == a11 && a22 == a22 && a33 == a33)) qw = a00 + a11 + a22 + a33;  // a NaN anywhere reaches the output
  const float inv = 1.0f / sqrtf(qw * qw + qx * qx + qy * qy + qz * qz);
  qw *= inv, qx *= inv, qy *= inv, qz *= inv;
  const float r00 = 1.0f - 2.0f * (qy * qy + qz * qz), r01 = 2.0f * (qx * qy - qw * qz), r02 = 2.0f * (qx * qz + qw * qy);
  const float r10 = 2.0f * (qx * qy + qw * qz), r11 = 1.0f - 2.0f * (qx * qx + qz * qz), r12 = 2.0f * (qy * qz - qw * qx);
  const float r20 = 2.0f * (qx * qz - qw * qy), r21 = 2.0f * (qy * qz + qw * qx), r22 = 1.0f - 2.0f * (qx * qx + qy * qy);

  // 3. aligned = R (x - c_x) + c_ref, and the squared distance to the reference from the values written
  float acc = 0.0f;
  for (int i0 = 0; i0 < n_atoms; i0 += SP_TILE) {
    const int m = min(SP_TILE, n_atoms - i0);
    if (n_atoms > SP_TILE) {  // (a single tile is still in LDS from pass 2)
      __syncthreads();
      for (int j = tid; j < 3 * m; j += SP_THREADS) s_ref[j] = ref[3ll * i0 + j];
      __syncthreads();
    }
    if (live) {
#pragma unroll 4
      for (int i = 0; i < m; ++i) {
        const float* p = x + (long long)(i0 + i) * atom_stride;
        float* w = o + (long long)(i0 + i) * out_atom_stride;
        const float x0 = p[0] - cx0, x1 = p[1] - cx1, x2 = p[2] - cx2;
        const float y0 = (r00 * x0 + r01 * x1 + r02 * x2) + cr0;
        const float y1 = (r10 * x0 + r11 * x1 + r12 * x2) + cr1;
        const float y2 = (r20 * x0 + r21 * x1 + r22 * x2) + cr2;
        w[0] = y0;
        w[1] = y1;
        w[2] = y2;
        const float d0 = y0 - s_ref[3 * i + 0], d1 = y1 - s_ref[3 * i + 1], d2 = y2 - s_ref[3 * i + 2];
        acc += d0 * d0 + d1 * d1 + d2 * d2;
      }
    }
  }
  if (live && rmsd) rmsd[f] = sqrtf(acc / (float)n_atoms);
}

}  // namespace

void launch_superpose_frames(const float* xyz, long long frame_stride, long long atom_stride, int n_atoms, int n_frames, const float* ref, float* out,
                             long long out_frame_stride, long long out_atom_stride, float* rmsd, hipStream_t st) {
  const int grid = (n_frames + SP_THREADS - 1) / SP_THREADS;  // (n_frames <= 2^31 - 1: at most 2^25 workgroups)
  hipLaunchKernelGGL(k_superpose_frames, dim3(grid), dim3(SP_THREADS), 0, st, xyz, frame_stride, atom_stride, n_atoms, n_frames, ref, out, out_frame_stride,
                     out_atom_stride, rmsd);
}
