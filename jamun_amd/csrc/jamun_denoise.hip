// jamun_denoise.hip — the two ends of a denoising evaluation (src/jamun/model/denoiser.py:219-297) around the forward: noise a batch of
// clean frames and align the noisy frames on them, and reduce the denoised frames to the per-graph losses.
//
//   k_noise_align    denoiser.py:228-244.  x_c = x - centroid(x) ; y = x_c + sigma noise ; y -= centroid(y) ; y <- R y + t with the proper
//                    rotation R (det +1) and translation t that minimise sum_i |R y_i + t - x_c,i|^2 (utils/align.py:9-56) ; optionally the
//                    RMSD of y to x_c after the step.  The centring steps run only with `mean_center`, the last only with `align`.
//   k_denoise_loss   denoiser.py:262-281.  Per graph: raw = mean_i |xhat_i - x_i|^2 ; scaled_rmsd = mean_i |xhat_i - x_i| / (sigma sqrt 3) ;
//                    loss = raw loss_weight_g / c_out^2.
//
// Both take a ragged batch as k_mean_center takes it (ptr [W + 1], the atoms of a graph adjacent) and give ONE WORKGROUP TO ONE GRAPH: a
// graph of the evaluation is a molecule of tens to hundreds of atoms, a batch holds hundreds of graphs, and nothing crosses a graph.  ptr
// is clamped to [0, n_atoms] and made to ascend, so that no table, whatever it holds, takes an access outside the buffers.
//
// Arithmetic (fp32, the library is compiled with -ffp-contract=off: every product and sum below is rounded on its own):
//   * the centroids of x and of y are those of k_mean_center: a sequential sum in atom order divided by n, so x_c holds the bits of
//     jamun_mean_center(x) and y, without `align`, those of a host that does the same fp32 operations;
//   * the alignment has centroids of its own (of y and of x_c as stored, the same arithmetic; after the centring steps they are rounding
//     residue, without them they carry the translation) and takes the covariance of the CENTRED coordinates.  Its nine sums are formed by
//     every thread over the atoms tid, tid + DN_THREADS, ... and added over the threads in thread order: a fixed order, the same bits in
//     every run, no atomics;
//   * the rotation is the top eigenvector of Horn's 4x4 matrix by DN_SWEEPS cyclic Jacobi sweeps, as in jamun_superpose.hip and for the
//     reasons in its header: a half turn is a quaternion like any other, a rank-deficient covariance (one or two atoms, collinear atoms)
//     gets SOME optimal rotation, and a quaternion cannot describe the reflection an SVD without the determinant fix would return.  Every
//     thread of the workgroup solves the same 4x4 problem from the same nine sums: no broadcast, no divergence;
//   * y <- R (y - c_y) + c_x, the form of R y + t whose rounding does not grow with the distance from the origin;
//   * the RMSD is formed from the values written, per thread over its atoms and over the threads in thread order.
// A graph with a non-finite value gives a non-finite y (with `mean_center` or `align`: all of it) and touches no other graph.  A graph
// without atoms writes nothing.
//
// k_denoise_loss adds the per-atom terms of a graph in atom order in fp32, as scatter_mean forms them on the CPU: the threads of the
// workgroup compute the terms of DL_TILE atoms into LDS, threads 0 and 1 add them one after the other.
// No MFMA, no inline assembly, no allocation: every buffer is the caller's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "jamun_internal.h"
#include "jamun_dev.h"

namespace {

constexpr int DN_THREADS = 128;
constexpr int DN_SWEEPS = 6;  // as SP_SWEEPS (jamun_superpose.hip)
constexpr int DL_THREADS = 64;
constexpr int DL_TILE = 256;

// the atoms [lo, hi) of graph g from a table that may hold anything
__device__ __forceinline__ void graph_range(const int* __restrict__ ptr, int g, int n_atoms, int& lo, int& hi) {
  lo = max(0, min(ptr[g], n_atoms));
  hi = max(lo, min(ptr[g + 1], n_atoms));
}

// (x_c and y may be x and noise themselves: every element is read by the thread that writes it, behind the barrier of the sums that read it)
__global__ void __launch_bounds__(DN_THREADS)
k_noise_align(const float* x, const float* noise, const int* __restrict__ ptr, int n_atoms, float sigma, int mean_center, int align, float* x_c, float* y,
              float* __restrict__ rmsd) {
  __shared__ float s_cen[6];
  __shared__ float s_part[9 * DN_THREADS];
  __shared__ float s_S[9];
  const int tid = threadIdx.x;
  int lo, hi;
  graph_range(ptr, blockIdx.x, n_atoms, lo, hi);
  const int n = hi - lo;
  if (n == 0) return;
  const float fn = (float)n;

  // x_c = x - centroid(x)
  if (mean_center) {
    if (tid < 3) {
      float s = 0.f;
      for (int a = lo; a < hi; ++a) s = s + x[a * 3 + tid];
      s_cen[tid] = s / fn;
    }
    __syncthreads();
  }
  // y = x_c + sigma noise
  for (int a = lo * 3 + tid; a < hi * 3; a += DN_THREADS) {
    const float xc = mean_center ? x[a] - s_cen[a % 3] : x[a];
    const float sn = sigma * noise[a];
    x_c[a] = xc;
    y[a] = xc + sn;
  }
  __syncthreads();  // (the workgroup's own global writes are visible to it behind a barrier)
  // y -= centroid(y)
  if (mean_center) {
    if (tid < 3) {
      float s = 0.f;
      for (int a = lo; a < hi; ++a) s = s + y[a * 3 + tid];
      s_cen[3 + tid] = s / fn;
    }
    __syncthreads();
    for (int a = lo * 3 + tid; a < hi * 3; a += DN_THREADS) y[a] = y[a] - s_cen[3 + a % 3];
    __syncthreads();
  }
  if (!align && !rmsd) return;

  float r00 = 1.f, r01 = 0.f, r02 = 0.f, r10 = 0.f, r11 = 1.f, r12 = 0.f, r20 = 0.f, r21 = 0.f, r22 = 1.f;
  float cy0 = 0.f, cy1 = 0.f, cy2 = 0.f, cx0 = 0.f, cx1 = 0.f, cx2 = 0.f;
  if (align) {
    // the alignment's centroids: threads 0..2 of y, threads 3..5 of x_c
    if (tid < 6) {
      const float* src = tid < 3 ? y : x_c;
      const int d = tid < 3 ? tid : tid - 3;
      float s = 0.f;
      for (int a = lo; a < hi; ++a) s = s + src[a * 3 + d];
      s_cen[tid] = s / fn;
    }
    __syncthreads();
    cy0 = s_cen[0], cy1 = s_cen[1], cy2 = s_cen[2], cx0 = s_cen[3], cx1 = s_cen[4], cx2 = s_cen[5];
    // covariance of the centred coordinates, S_ab = sum_i (y_i - c_y)_a (x_c,i - c_x)_b
    float sxx = 0.f, sxy = 0.f, sxz = 0.f, syx = 0.f, syy = 0.f, syz = 0.f, szx = 0.f, szy = 0.f, szz = 0.f;
    for (int a = lo + tid; a < hi; a += DN_THREADS) {
      const float y0 = y[a * 3] - cy0, y1 = y[a * 3 + 1] - cy1, y2 = y[a * 3 + 2] - cy2;
      const float x0 = x_c[a * 3] - cx0, x1 = x_c[a * 3 + 1] - cx1, x2 = x_c[a * 3 + 2] - cx2;
      sxx += y0 * x0;
      sxy += y0 * x1;
      sxz += y0 * x2;
      syx += y1 * x0;
      syy += y1 * x1;
      syz += y1 * x2;
      szx += y2 * x0;
      szy += y2 * x1;
      szz += y2 * x2;
    }
    s_part[0 * DN_THREADS + tid] = sxx;
    s_part[1 * DN_THREADS + tid] = sxy;
    s_part[2 * DN_THREADS + tid] = sxz;
    s_part[3 * DN_THREADS + tid] = syx;
    s_part[4 * DN_THREADS + tid] = syy;
    s_part[5 * DN_THREADS + tid] = syz;
    s_part[6 * DN_THREADS + tid] = szx;
    s_part[7 * DN_THREADS + tid] = szy;
    s_part[8 * DN_THREADS + tid] = szz;
    __syncthreads();
    if (tid < 9) {
      float s = 0.f;
      for (int l = 0; l < DN_THREADS; ++l) s = s + s_part[tid * DN_THREADS + l];
      s_S[tid] = s;
    }
    __syncthreads();
    sxx = s_S[0], sxy = s_S[1], sxz = s_S[2], syx = s_S[3], syy = s_S[4], syz = s_S[5], szx = s_S[6], szy = s_S[7], szz = s_S[8];

    // Horn's matrix N(S): q^T N q = sum_i (x_c,i - c_x) . R(q) (y_i - c_y) for a unit quaternion q = (w, x, y, z)
    float a00 = sxx + syy + szz, a11 = sxx - syy - szz, a22 = syy - sxx - szz, a33 = szz - sxx - syy;
    float a01 = syz - szy, a02 = szx - sxz, a03 = sxy - syx, a12 = sxy + syx, a13 = szx + sxz, a23 = syz + szy;
    float v00 = 1.0f, v01 = 0.0f, v02 = 0.0f, v03 = 0.0f;  // v[row][column]: the columns become the eigenvectors
    float v10 = 0.0f, v11 = 1.0f, v12 = 0.0f, v13 = 0.0f;
    float v20 = 0.0f, v21 = 0.0f, v22 = 1.0f, v23 = 0.0f;
    float v30 = 0.0f, v31 = 0.0f, v32 = 0.0f, v33 = 1.0f;
    for (int sweep = 0; sweep < DN_SWEEPS; ++sweep) {
      jacobi_rotate(a00, a11, a01, a02, a12, a03, a13, v00, v01, v10, v11, v20, v21, v30, v31);  // (0, 1): other rows 2, 3
      jacobi_rotate(a00, a22, a02, a01, a12, a03, a23, v00, v02, v10, v12, v20, v22, v30, v32);  // (0, 2): other rows 1, 3
      jacobi_rotate(a00, a33, a03, a01, a13, a02, a23, v00, v03, v10, v13, v20, v23, v30, v33);  // (0, 3): other rows 1, 2
      jacobi_rotate(a11, a22, a12, a01, a02, a13, a23, v01, v02, v11, v12, v21, v22, v31, v32);  // (1, 2): other rows 0, 3
      jacobi_rotate(a11, a33, a13, a01, a03, a12, a23, v01, v03, v11, v13, v21, v23, v31, v33);  // (1, 3): other rows 0, 2
      jacobi_rotate(a22, a33, a23, a02, a03, a12, a13, v02, v03, v12, v13, v22, v23, v32, v33);  // (2, 3): other rows 0, 1
    }
    // column of the largest eigenvalue (the first of equals) by a tournament of two-way selects
    const bool hi01 = a11 > a00, hi23 = a33 > a22;
    const float t01 = hi01 ? a11 : a00, w01 = hi01 ? v01 : v00, x01 = hi01 ? v11 : v10, y01 = hi01 ? v21 : v20, z01 = hi01 ? v31 : v30;
    const float t23 = hi23 ? a33 : a22, w23 = hi23 ? v03 : v02, x23 = hi23 ? v13 : v12, y23 = hi23 ? v23 : v22, z23 = hi23 ? v33 : v32;
    const bool top = t23 > t01;
    float qw = top ? w23 : w01, qx = top ? x23 : x01, qy = top ? y23 : y01, qz = top ? z23 : z01;
    if (!(a00 == a00 && a11 == a11 && a22 == a22 && a33 == a33)) qw = a00 + a11 + a22 + a33;  // a NaN anywhere reaches the output
    const float inv = 1.0f / sqrtf(qw * qw + qx * qx + qy * qy + qz * qz);
    qw *= inv, qx *= inv, qy *= inv, qz *= inv;
    r00 = 1.0f - 2.0f * (qy * qy + qz * qz), r01 = 2.0f * (qx * qy - qw * qz), r02 = 2.0f * (qx * qz + qw * qy);
    r10 = 2.0f * (qx * qy + qw * qz), r11 = 1.0f - 2.0f * (qx * qx + qz * qz), r12 = 2.0f * (qy * qz - qw * qx);
    r20 = 2.0f * (qx * qz - qw * qy), r21 = 2.0f * (qy * qz + qw * qx), r22 = 1.0f - 2.0f * (qx * qx + qy * qy);
  }

  // y <- R (y - c_y) + c_x, and the squared distance to x_c from the values written
  float acc = 0.f;
  for (int a = lo + tid; a < hi; a += DN_THREADS) {
    float y0 = y[a * 3], y1 = y[a * 3 + 1], y2 = y[a * 3 + 2];
    if (align) {
      const float c0 = y0 - cy0, c1 = y1 - cy1, c2 = y2 - cy2;
      y0 = (r00 * c0 + r01 * c1 + r02 * c2) + cx0;
      y1 = (r10 * c0 + r11 * c1 + r12 * c2) + cx1;
      y2 = (r20 * c0 + r21 * c1 + r22 * c2) + cx2;
      y[a * 3] = y0;
      y[a * 3 + 1] = y1;
      y[a * 3 + 2] = y2;
    }
    const float d0 = y0 - x_c[a * 3], d1 = y1 - x_c[a * 3 + 1], d2 = y2 - x_c[a * 3 + 2];
    acc += d0 * d0 + d1 * d1 + d2 * d2;
  }
  if (rmsd) {
    __syncthreads();  // (s_part: the covariance's readers are done)
    s_part[tid] = acc;
    __syncthreads();
    if (tid == 0) {
      float s = 0.f;
      for (int l = 0; l < DN_THREADS; ++l) s = s + s_part[l];
      rmsd[blockIdx.x] = sqrtf(s / fn);
    }
  }
}

__global__ void __launch_bounds__(DL_THREADS)
k_denoise_loss(const float* __restrict__ xhat, const float* __restrict__ x_c, const int* __restrict__ ptr, int n_atoms, float rmsd_scale,
               const float* __restrict__ loss_weight, float inv_c_out_sq, float* __restrict__ out) {
  __shared__ float s_r[DL_TILE];
  const int tid = threadIdx.x;
  const int g = blockIdx.x;
  int lo, hi;
  graph_range(ptr, g, n_atoms, lo, hi);
  float sum = 0.f;  // thread 0: of |xhat_i - x_i|^2; thread 1: of |xhat_i - x_i| / (sigma sqrt 3)
  for (int a0 = lo; a0 < hi; a0 += DL_TILE) {
    const int m = min(DL_TILE, hi - a0);
    if (a0 > lo) __syncthreads();  // (the readers of the previous tile are done)
    for (int i = tid; i < m; i += DL_THREADS) {
      const int a = a0 + i;
      const float d0 = xhat[a * 3] - x_c[a * 3], d1 = xhat[a * 3 + 1] - x_c[a * 3 + 1], d2 = xhat[a * 3 + 2] - x_c[a * 3 + 2];
      s_r[i] = d0 * d0 + d1 * d1 + d2 * d2;
    }
    __syncthreads();
    if (tid < 2)
      for (int i = 0; i < m; ++i) sum = sum + (tid == 0 ? s_r[i] : sqrtf(s_r[i]) / rmsd_scale);
  }
  const float cnt = (float)(hi - lo);
  const float mean = sum / (cnt < 1.f ? 1.f : cnt);  // (a graph without atoms: zeros, as scatter_mean gives)
  if (tid == 0) {
    out[3 * g] = mean;
    out[3 * g + 2] = (mean * (loss_weight ? loss_weight[g] : 1.f)) * inv_c_out_sq;
  }
  if (tid == 1) out[3 * g + 1] = mean;
}

}  // namespace

void launch_noise_align(const float* x, const float* noise, const int* ptr, int n_graphs, int n_atoms, float sigma, int mean_center, int align, float* x_c,
                        float* y, float* rmsd, hipStream_t st) {
  hipLaunchKernelGGL(k_noise_align, dim3(n_graphs), dim3(DN_THREADS), 0, st, x, noise, ptr, n_atoms, sigma, mean_center, align, x_c, y, rmsd);
}

void launch_denoise_loss(const float* xhat, const float* x_c, const int* ptr, int n_graphs, int n_atoms, float rmsd_scale, const float* loss_weight,
                         float inv_c_out_sq, float* out, hipStream_t st) {
  hipLaunchKernelGGL(k_denoise_loss, dim3(n_graphs), dim3(DL_THREADS), 0, st, xhat, x_c, ptr, n_atoms, rmsd_scale, loss_weight, inv_c_out_sq, out);
}
