// The 16 x 16 x 4 matrix-core instruction per precision (qi_csd.hip, qi_beam.hip; qi_whiten.hip pads to its tile): D = A B + C
// with A [16 x 4], B [4 x 16].  Lane l supplies A[l & 15][l >> 4] and B[l >> 4][l & 15] -- the two operands have the same lane
// layout: entry l & 15 of the 16-side at slot l >> 4 of the K side -- and holds four entries of column l & 15 of C/D, whose rows
// differ by precision.
#pragma once
#include "qi_common.hpp"

namespace qi {

constexpr int kMxTile = 16;  // M and N of the instruction: the side of a result tile

typedef float qi_f4 __attribute__((ext_vector_type(4)));
typedef double qi_d4 __attribute__((ext_vector_type(4)));

// accumulator type, one K step of four, consecutive K entries a lane of qi_csd loads (32 bytes), and the row of the tile that
// register `reg` of lane `lane` holds -- the two C/D maps differ
template <typename T>
struct Mx;
template <>
struct Mx<float> {
  using acc = qi_f4;
  static constexpr int V = 4;
  static __device__ __forceinline__ acc mac(float a, float b, acc c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
  // float32 C/D: lane l, register r -> row 4 (l >> 4) + r, column l & 15
  static __device__ __forceinline__ int row(int lane, int reg) { return 4 * (lane >> 4) + reg; }
};
template <>
struct Mx<double> {
  using acc = qi_d4;
  static constexpr int V = 2;
  static __device__ __forceinline__ acc mac(double a, double b, acc c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
  // float64 C/D: lane l, register r -> row (l >> 4) + 4 r, column l & 15
  static __device__ __forceinline__ int row(int lane, int reg) { return (lane >> 4) + 4 * reg; }
};

}  // namespace qi
