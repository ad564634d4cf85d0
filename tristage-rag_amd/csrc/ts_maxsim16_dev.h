// The per-k-step arithmetic of the streaming MaxSim kernel (ts_maxsim16.hip), shared with the passage kernel
// (ts_passage.hip) so that both form a cosine from the same instructions: the row norms from the operand values in
// registers, the dot products on the 32x32x16 MFMA (16-bit rows) or the exact-f32 32x32x2 MFMA (f32 rows).
#pragma once
#include "ts_common.h"

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf8 __attribute__((ext_vector_type(8)));
typedef _Float16 h2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf2 __attribute__((ext_vector_type(2)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// sum of squares of the 8 values of one operand register quad.  (Whole-vector casts and
// constant shuffles only: hipcc 7.2 miscompiles __builtin_bit_cast of a[i] inside an
// unrolled loop — every iteration reads element 0; see DESIGN.md "Notes".)
typedef float f32x4v __attribute__((ext_vector_type(4)));
template <int DT> __device__ __forceinline__ float m16_sumsq(const u32x4& a, float s) {
  if constexpr (DT == TS_F32) {
    const f32x4v v = __builtin_bit_cast(f32x4v, a);
    s = fmaf(v[0], v[0], s); s = fmaf(v[1], v[1], s); s = fmaf(v[2], v[2], s); s = fmaf(v[3], v[3], s);
  } else if constexpr (DT == TS_F16) {
    const h8 v = __builtin_bit_cast(h8, a);
    const h2 p0 = __builtin_shufflevector(v, v, 0, 1), p1 = __builtin_shufflevector(v, v, 2, 3);
    const h2 p2 = __builtin_shufflevector(v, v, 4, 5), p3 = __builtin_shufflevector(v, v, 6, 7);
    s = __builtin_amdgcn_fdot2(p0, p0, s, false);
    s = __builtin_amdgcn_fdot2(p1, p1, s, false);
    s = __builtin_amdgcn_fdot2(p2, p2, s, false);
    s = __builtin_amdgcn_fdot2(p3, p3, s, false);
  } else {
    const bf8 v = __builtin_bit_cast(bf8, a);
    const bf2 p0 = __builtin_shufflevector(v, v, 0, 1), p1 = __builtin_shufflevector(v, v, 2, 3);
    const bf2 p2 = __builtin_shufflevector(v, v, 4, 5), p3 = __builtin_shufflevector(v, v, 6, 7);
    s = __builtin_amdgcn_fdot2_f32_bf16(p0, p0, s, false);
    s = __builtin_amdgcn_fdot2_f32_bf16(p1, p1, s, false);
    s = __builtin_amdgcn_fdot2_f32_bf16(p2, p2, s, false);
    s = __builtin_amdgcn_fdot2_f32_bf16(p3, p3, s, false);
  }
  return s;
}
template <int DT>
__device__ __forceinline__ void m16_mma(f32x16& acc, const u32x4& a, const u32x4& b) {
  if constexpr (DT == TS_F32) {
    // fp32 rows: the unit holds 4 consecutive floats; the t-th exact-f32 MFMA (K = 2: this
    // lane's value and its h-partner's) contracts k = 8g + t and 8g + 4 + t — any pairing is
    // fine as long as the query image uses the same one, which it does by construction
    const f32x4v af = __builtin_bit_cast(f32x4v, a), bf = __builtin_bit_cast(f32x4v, b);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af[0], bf[0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af[1], bf[1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af[2], bf[2], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af[3], bf[3], acc, 0, 0, 0);
  } else if constexpr (DT == TS_F16)
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(h8, a), __builtin_bit_cast(h8, b), acc, 0, 0, 0);
  else
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf8, a), __builtin_bit_cast(bf8, b), acc, 0, 0, 0);
}
