// The vocabulary of a 32 x 32 MFMA tile, shared by the dense units that compute on one (biased_attention,
// spatial_encoder3d): the operand vectors, one MFMA per operand type, the accumulator's row layout and its zero.  What
// one operator shapes (its geometry, its fragment loaders, its LDS tiles) stays in that operator's file.  Device code
// only; segment_mm.hip keeps its own Mma<T>, which takes typed operand vectors.
#pragma once
#include "common.h"

namespace dgla {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 b16x8 __attribute__((ext_vector_type(8)));
typedef uint16_t u16x8 __attribute__((ext_vector_type(8)));

// One MFMA per operand type.  Raw is what a lane hands the instruction for A or B: FE consecutive k elements, of which
// put() sets element e.
template <typename T>
struct Mma32;
template <>
struct Mma32<float> {
  static constexpr int KSTEP = 2, FE = 1;
  using Raw = float;
  static __device__ __forceinline__ f32x16 mma(Raw a, Raw b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }
  static __device__ __forceinline__ void put(Raw& f, int e, float x) { f = x; }
};
template <>
struct Mma32<f16_t> {
  static constexpr int KSTEP = 16, FE = 8;
  using Raw = u16x8;
  static __device__ __forceinline__ f32x16 mma(Raw a, Raw b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(h16x8, a), __builtin_bit_cast(h16x8, b), c, 0, 0, 0);
  }
  static __device__ __forceinline__ void put(Raw& f, int e, f16_t x) { f[e] = __builtin_bit_cast(uint16_t, x); }
};
template <>
struct Mma32<bf16_t> {
  static constexpr int KSTEP = 16, FE = 8;
  using Raw = u16x8;
  static __device__ __forceinline__ f32x16 mma(Raw a, Raw b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(b16x8, a), __builtin_bit_cast(b16x8, b), c, 0, 0, 0);
  }
  static __device__ __forceinline__ void put(Raw& f, int e, bf16_t x) { f[e] = x.bits; }
};

// The row of the A operand that register r of a 32 x 32 C tile holds, for lane half g = lane / 32 (the lane's column
// is lane % 32).
__device__ __forceinline__ int mfma_c_row(int r, int g) { return 8 * (r >> 2) + 4 * g + (r & 3); }

__device__ __forceinline__ f32x16 mfma_zero() {
  f32x16 c;
#pragma unroll
  for (int r = 0; r < 16; ++r) c[r] = 0.f;
  return c;
}

}  // namespace dgla
