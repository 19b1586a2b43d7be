// jamun_dev.h — THE device helpers of every kernel file of the library (one definition each): the vector typedefs, the MFMA wrappers, the
// f16x3 product macros, readfirstlane, the LDS barrier, absolute-address LDS accesses and constant address-space loads, power-of-two scales, the Jacobi rotation of the 4x4 eigen-solvers
// (jamun_superpose.hip, jamun_denoise.hip).
// The f16x3 split primitives themselves are jamun_split.h (included here).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "jamun_split.h"

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 h2 __attribute__((ext_vector_type(2)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

#define MFMA32(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)
#define MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)
#define MFMA16H(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, (a)), __builtin_bit_cast(h8, (b)), (c), 0, 0, 0)
#define MFMA32H(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(h8, (a)), __builtin_bit_cast(h8, (b)), (c), 0, 0, 0)
// one f16x3 product: lo hi + hi lo + hi hi (fp32 accumulate; the lo lo term is below 2^-24 of the product)
#define M3(ACC, AH_, AL_, BH_, BL_)   \
  ACC = MFMA32H(AL_, BH_, ACC);       \
  ACC = MFMA32H(AH_, BL_, ACC);       \
  ACC = MFMA32H(AH_, BH_, ACC)
// ... or, in the opt-in reduced-precision mode (X1 in scope: "f16x1"), the hi hi product alone: operands rounded to 11 bits, fp32 accumulation — the
// loads, splits and conversions that only feed the dropped products are dead code for the compiler
#define MX(ACC, AH_, AL_, BH_, BL_)                              \
  do {                                                           \
    if constexpr (X1) { ACC = MFMA32H(AH_, BH_, ACC); }          \
    else { M3(ACC, AH_, AL_, BH_, BL_); }                        \
  } while (0)
#define RFL(v) __builtin_amdgcn_readfirstlane(v)
#define LDS_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")
#define MF_SCHED() __builtin_amdgcn_sched_barrier(0)

namespace {

__device__ __forceinline__ float4 lds_f4(int addr) {  // ds_read_b128 from an absolute LDS address
#if defined(__HIP_DEVICE_COMPILE__)
  const f32x4 v = *(const __attribute__((address_space(3))) f32x4*)(unsigned)addr;
  return make_float4(v.x, v.y, v.z, v.w);
#else
  (void)addr;
  return make_float4(0.f, 0.f, 0.f, 0.f);
#endif
}
__device__ __forceinline__ float2 lds_f2(int addr) {
#if defined(__HIP_DEVICE_COMPILE__)
  const f32x2 v = *(const __attribute__((address_space(3))) f32x2*)(unsigned)addr;
  return make_float2(v.x, v.y);
#else
  (void)addr;
  return make_float2(0.f, 0.f);
#endif
}
__device__ __forceinline__ void lds_st4(int addr, const float4& v) {
#if defined(__HIP_DEVICE_COMPILE__)
  *(__attribute__((address_space(3))) f32x4*)(unsigned)addr = f32x4{v.x, v.y, v.z, v.w};
#else
  (void)addr; (void)v;
#endif
}
__device__ __forceinline__ int lds_addr(const void* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (int)(unsigned)(uintptr_t)(const __attribute__((address_space(3))) char*)p;
#else
  (void)p;
  return 0;
#endif
}
// uniform loads through the constant address space: scalar loads into scalar registers
__device__ __forceinline__ int4 ld_const(const int4* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef int i32x4 __attribute__((ext_vector_type(4)));
  const i32x4 v = *(const __attribute__((address_space(4))) i32x4*)(uintptr_t)p;
  return make_int4(v.x, v.y, v.z, v.w);
#else
  return *p;
#endif
}
__device__ __forceinline__ int2 ld_const(const int2* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef int i32x2 __attribute__((ext_vector_type(2)));
  const i32x2 v = *(const __attribute__((address_space(4))) i32x2*)(uintptr_t)p;
  return make_int2(v.x, v.y);
#else
  return *p;
#endif
}
__device__ __forceinline__ float pow2f(int e) { return __uint_as_float((unsigned)(e + 127) << 23); }  // 2^e, -126 <= e <= 127
__device__ __forceinline__ int exp_above(float v) { return (int)((__float_as_uint(v) >> 23) & 0xffu) - 126; }  // v < 2^exp_above(v)
__device__ __forceinline__ int clamp40(int s) { return max(-40, min(40, s)); }
__device__ __forceinline__ int clamp100(int s) { return max(-100, min(100, s)); }

// One Jacobi rotation in the (p, q) plane of the symmetric 4x4 matrix held as scalars: app, aqq, apq and the two other rows' entries
// (arp, arq), (asp, asq); v*p / v*q are columns p and q of the accumulated eigenvector matrix.  t = tan of the rotation angle, the smaller
// root (|t| <= 1); apq == 0 leaves everything as it is (t = 0) without a branch that diverges.
__device__ __forceinline__ void jacobi_rotate(float& app, float& aqq, float& apq, float& arp, float& arq, float& asp, float& asq, float& v0p, float& v0q,
                                              float& v1p, float& v1q, float& v2p, float& v2q, float& v3p, float& v3q) {
  const float theta = (aqq - app) / (2.0f * apq);
  const float root = sqrtf(theta * theta + 1.0f);  // (theta * theta may overflow to inf: t = 0, the right limit)
  float t = (theta < 0.0f ? -1.0f : 1.0f) / (fabsf(theta) + root);
  t = apq == 0.0f ? 0.0f : t;
  const float c = 1.0f / sqrtf(t * t + 1.0f);
  const float s = t * c;
  app = app - t * apq;
  aqq = aqq + t * apq;
  apq = 0.0f;
  float x = arp, y = arq;
  arp = c * x - s * y;
  arq = s * x + c * y;
  x = asp, y = asq;
  asp = c * x - s * y;
  asq = s * x + c * y;
  x = v0p, y = v0q;
  v0p = c * x - s * y;
  v0q = s * x + c * y;
  x = v1p, y = v1q;
  v1p = c * x - s * y;
  v1q = s * x + c * y;
  x = v2p, y = v2q;
  v2p = c * x - s * y;
  v2q = s * x + c * y;
  x = v3p, y = v3q;
  v3p = c * x - s * y;
  v3q = s * x + c * y;
}

}  // namespace
