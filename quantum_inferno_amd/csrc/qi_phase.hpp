// The phase rule of include/qi_beam.h, written once for every kernel that forms steering factors (qi_beam.hip, qi_steer.hip):
// the product freq * tau in double whatever T is, reduced to [-1/2, 1/2] turns in double, the sine and cosine of the reduced
// turns in T (sincospi): a phase that is an exact multiple of a quarter turn gives exactly +-1 and 0.
#pragma once
#include <hip/hip_runtime.h>

namespace qi {

__device__ __forceinline__ void beam_sincospi(float x, float* s, float* c) { sincospif(x, s, c); }
__device__ __forceinline__ void beam_sincospi(double x, double* s, double* c) { sincospi(x, s, c); }

// exp(2 pi i freq tau) -> (*re, *im)
template <typename T>
__device__ __forceinline__ void beam_factor(double freq, double tau, T* re, T* im) {
  double turns = freq * tau;
  turns -= rint(turns);  // [-1/2, 1/2]
  beam_sincospi((T)(2.0 * turns), im, re);
}

}  // namespace qi
