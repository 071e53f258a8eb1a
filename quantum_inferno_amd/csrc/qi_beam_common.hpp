// What the two forms over a delay grid share (qi_beam.hip: the Bartlett form of include/qi_beam.h; qi_capon.hip: the Capon form
// of include/qi_adaptive.h): the tile and workgroup constants, the LDS pitch, the phase factors' sincospi, the peaks launch,
// the upload of the two host tables, the verdicts on a shape and on a band table, and the scratch layout.  Everything is in
// an unnamed namespace: each of the two files gets kernels and helpers of its own.
#pragma once
#include "qi_host.hpp"
#include "qi_device.hpp"   // kWave
#include "qi_fft_reg.hpp"  // QI_LAUNCH_CHECK
#include "qi_mfma.hpp"     // Mx
#include "qi_beam.h"

namespace {

using namespace qi;
using qi::host::align_up;

constexpr int kBeamTile = 16;     // grid points of a wave, sensors of a row tile (the instruction's N and M)
constexpr int kBeamMaxTiles = QI_BEAM_MAX_SENSORS / kBeamTile;
constexpr int kBeamWavesFew = 2;  // waves per workgroup: few where the workgroups would not fill the chip otherwise
constexpr int kBeamWavesMany = 8;
constexpr int64_t kBeamFill = 512;  // workgroups from which the larger workgroup is taken
constexpr int kPeakThreads = 256;
constexpr int kWordChunk = 256;  // host values per k_beam_put_words launch (2 KiB of kernel arguments)

// entries a row of the matrix takes in LDS
template <typename T>
__host__ __device__ constexpr int beam_ld(int ntile) {
  return ntile * kBeamTile + (sizeof(T) == 4 ? 4 : 0);
}

__device__ __forceinline__ void beam_sincospi(float x, float* s, float* c) { sincospif(x, s, c); }
__device__ __forceinline__ void beam_sincospi(double x, double* s, double* c) { sincospi(x, s, c); }

// np.argmax's order: a NaN before every number, a larger value before a smaller one, a lower index before a higher one
template <typename T>
__device__ __forceinline__ bool beam_before(T va, int64_t ia, T vb, int64_t ib) {
  const bool na = va != va, nb = vb != vb;
  if (na || nb) return na && (!nb || ia < ib);
  return va > vb || (va == vb && ia < ib);
}

template <typename T>
__global__ void __launch_bounds__(kPeakThreads) k_beam_peaks(const T* __restrict__ power, int64_t G, int64_t* __restrict__ index,
                                                            T* __restrict__ value) {
  __shared__ T sv[kPeakThreads];
  __shared__ int64_t si[kPeakThreads];
  const int tid = threadIdx.x;
  const T* __restrict__ row = power + (int64_t)blockIdx.x * G;
  T bv = T(0);
  int64_t bi = -1;  // (none yet: G may be below the thread count)
  for (int64_t g = tid; g < G; g += kPeakThreads) {
    const T v = row[g];
    if (bi < 0 || beam_before(v, g, bv, bi)) {
      bv = v;
      bi = g;
    }
  }
  sv[tid] = bv;
  si[tid] = bi;
  __syncthreads();
  for (int s = kPeakThreads / 2; s > 0; s >>= 1) {
    if (tid < s && si[tid + s] >= 0 && (si[tid] < 0 || beam_before(sv[tid + s], si[tid + s], sv[tid], si[tid]))) {
      sv[tid] = sv[tid + s];
      si[tid] = si[tid + s];
    }
    __syncthreads();
  }
  if (tid == 0) {
    if (index) index[blockIdx.x] = si[0];
    if (value) value[blockIdx.x] = sv[0];
  }
}

// 8-byte host values (frequencies, band offsets) to the device as kernel arguments: stream-ordered, the caller's array is
// free at return
struct WordChunk {
  uint64_t w[kWordChunk];
};
__global__ void __launch_bounds__(kWordChunk) k_beam_put_words(uint64_t* __restrict__ dst, WordChunk c, int count) {
  if ((int)threadIdx.x < count) dst[threadIdx.x] = c.w[threadIdx.x];
}
int put_words(void* dst, const void* src, int64_t count, hipStream_t st) {
  for (int64_t k0 = 0; k0 < count; k0 += kWordChunk) {
    WordChunk c{};
    const int n = (int)std::min<int64_t>(kWordChunk, count - k0);
    std::memcpy(c.w, static_cast<const uint64_t*>(src) + k0, (size_t)n * sizeof(uint64_t));
    k_beam_put_words<<<1, kWordChunk, 0, st>>>(static_cast<uint64_t*>(dst) + k0, c, n);
    QI_LAUNCH_CHECK();
  }
  return QI_OK;
}

// what the size query and the call refuse of a shape (the index arithmetic and the grid stay inside their types)
int beam_shape_check(int dtype, int64_t C, int64_t nf, int64_t G, int64_t nb) {
  QI_REQUIRE(dtype == QI_F32 || dtype == QI_F64, "bad dtype %d", dtype);
  QI_REQUIRE(C >= 1 && C <= QI_BEAM_MAX_SENSORS, "%lld sensors: 1 to %d", (long long)C, QI_BEAM_MAX_SENSORS);
  QI_REQUIRE(nf >= 1 && G >= 1 && nb >= 1, "bad shape: %lld matrices, %lld grid points, %lld bands", (long long)nf, (long long)G,
             (long long)nb);
  QI_REQUIRE(nb <= nf, "%lld bands of %lld matrices", (long long)nb, (long long)nf);
  QI_REQUIRE(nf < (1ll << 40) && G < (1ll << 40) && nb * ceil_div(G, kBeamTile * kBeamWavesFew) < (1ll << 31), "request too large");
  return QI_OK;
}

// what the call refuses of a host band table
int beam_bands_check(const int64_t* band_first, int64_t nf, int64_t nb) {
  if (band_first) {
    QI_REQUIRE(band_first[0] >= 0 && band_first[0] < nf, "band offsets start at %lld: outside 0..%lld", (long long)band_first[0],
               (long long)nf);
    for (int64_t b = 0; b < nb; ++b)
      QI_REQUIRE(band_first[b + 1] > band_first[b], "band offsets are not strictly ascending at band %lld", (long long)b);
    QI_REQUIRE(band_first[nb] <= nf, "band offsets end at %lld, past the %lld matrices", (long long)band_first[nb], (long long)nf);
  } else {
    QI_REQUIRE(nb == nf, "no band table: every matrix is its own band, nb must be nf");
  }
  return QI_OK;
}

size_t beam_freq_bytes(int64_t nf) { return align_up((size_t)nf * sizeof(double)); }
size_t beam_scratch(int64_t nf, int64_t nb) { return beam_freq_bytes(nf) + align_up((size_t)(nb + 1) * sizeof(int64_t)); }

// the two host tables into the scratch, in stream order -> the device copies (first: null without a band table)
int beam_put_tables(void* scratch, const double* freq_hz, int64_t nf, const int64_t* band_first, int64_t nb, hipStream_t st,
                    double** freq, int64_t** first) {
  *freq = static_cast<double*>(scratch);
  *first = band_first ? reinterpret_cast<int64_t*>(static_cast<char*>(scratch) + beam_freq_bytes(nf)) : nullptr;
  QI_TRY(put_words(*freq, freq_hz, nf, st));
  if (band_first) QI_TRY(put_words(*first, band_first, nb + 1, st));
  return QI_OK;
}

// every refusal of a form's call, before anything is launched (matrices: the stack the form reads)
int beam_call_check(int dtype, int64_t C, int64_t nf, int64_t G, int64_t nb, const void* matrices, const double* freq_hz,
                    const void* delays_s, const int64_t* band_first, const void* power, const void* peak_index,
                    const void* peak_value, const void* scratch, int64_t scratch_bytes) {
  QI_TRY(beam_shape_check(dtype, C, nf, G, nb));
  QI_REQUIRE(matrices && freq_hz && delays_s && scratch, "null argument");
  QI_REQUIRE(power, "power is null: nothing to produce");
  QI_TRY(beam_bands_check(band_first, nf, nb));
  QI_TRY(require_scratch(scratch_bytes, (int64_t)beam_scratch(nf, nb)));
  QI_REQUIRE(aligned(matrices, 2 * elem_size(dtype)) && aligned(delays_s, 8) && aligned(power, elem_size(dtype)) &&
                 aligned(peak_index, 8) && aligned(peak_value, elem_size(dtype)) && aligned(scratch, 16),
             "misaligned pointer");
  return QI_OK;
}

// the workgroup size of a form's launch: the larger one from kBeamFill workgroups on
inline bool beam_many(int64_t G, int64_t nb) { return nb * ceil_div(ceil_div(G, kBeamTile), kBeamWavesMany) >= kBeamFill; }

}  // namespace
