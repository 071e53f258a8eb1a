// Delay-and-sum in the time domain (include/qi_timebeam.h): fractional-delay beams of the records of an array, as traces or
// as the beam's power and semblance per sliding window and delay row.
//
// k_time_beam.  A workgroup of 256 threads (four waves) takes kTbRowBlock = 16 delay rows, four per wave, and a run of time:
// one chunk of kTbChunk = 256 samples for the traces, a whole unit (a hop or a window, see the header) chunk by chunk for the
// power.  The delay row is uniform across a wave and time runs across the lanes: a lane owns kTbOwn = 4 consecutive outputs,
// loads T + 3 samples of a sensor and does 4 T fused multiply-adds with them; the taps and the (shift, phase) of the row are
// wave-uniform.  The beam of a chunk lives in registers (4 rows x 4 outputs per lane) while the sensors go by in index order.
//
// LDS.  The sensors are staged `stage` at a time (as many as fit 32 KiB): the chunk and a halo of 2 max_shift + T samples,
// zero outside the record, every load guarded by 0 <= t < n.  A staged sensor is stored de-interleaved in four planes, sample
// j at plane j mod 4, place j / 4: the lanes of a wave read sample 4 lane + s + q, s = shift + max_shift uniform -- plane
// (s + q) mod 4 at place lane + (s + q) / 4, consecutive dwords, no bank conflict whatever the shift (lane-major storage
// would put the lanes four dwords apart: a 4-way conflict of ds_read_b32).  The plane pitch is 8 mod 32 places, so the
// staging writes of 32 consecutive samples fall on 32 different banks too.  Above QI_TIMEBEAM_LDS_MAX_SHIFT the halo stops
// fitting: the same arithmetic then takes each sample with a guarded load through L2 (template parameter STAGED), the same
// bits.  The tables of the workgroup's rows are checked once, before they index anything, and kept in LDS (8 KiB): a row
// with a shift beyond max_shift or a phase outside the bank computes nothing and gives NaN.
//
// Order of the additions (the header's contract): a tap sum runs m = 0 .. T - 1 by fma; the beam adds the sensors in index
// order; a lane adds b^2 of its four outputs, chunk after chunk from the unit's first sample, and y^2 sensor by sensor within
// a chunk; wave_sum folds the lanes in its fixed order.  Nothing of that depends on G, the row's position, n or nwin.  The
// file is compiled without contraction: every fused multiply-add is written out.
//
// k_time_beam_finish.  A workgroup per window: a thread adds the window's units of a row in time order, forms the quotient in
// double, rounds once and keeps np.argmax's candidate; the workgroup folds the candidates.  No atomics anywhere.
#include <algorithm>
#include <type_traits>

#include "qi_common.hpp"
#include "qi_device.hpp"
#include "qi_fft_reg.hpp"  // QI_LAUNCH_CHECK
#include "qi_timebeam.h"

namespace qi {

namespace {

constexpr int kTbThreads = 256;
constexpr int kTbWaves = kTbThreads / kWave;
constexpr int kTbOwn = 4;  // consecutive outputs of a lane
constexpr int kTbChunk = kWave * kTbOwn;
constexpr int kTbRowsPerWave = 4;
constexpr int kTbRowBlock = kTbWaves * kTbRowsPerWave;
constexpr size_t kTbStageBytes = 32 << 10;  // LDS the staged sensors may take
static_assert(kTbChunk == QI_TIMEBEAM_CHUNK && kTbRowBlock == QI_TIMEBEAM_ROW_BLOCK, "the header names the kernel's sizes");
static_assert(QI_BEAM_MAX_SENSORS <= kWave, "a lane per sensor checks a row's tables");

struct TbArgs {
  int64_t n, rows, nrb;         // samples of a record; delay rows; row blocks
  int64_t unit_len, unit_hop;   // samples of a workgroup's run of time, and from one run's start to the next
  int32_t C, P, max_shift;
  int32_t plane, stage;         // places of a plane of a staged sensor; sensors staged at a time
};

__device__ __forceinline__ float tb_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double tb_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }

// TRACES: out [rows][n], the beam over C.  Otherwise out is the power call's scratch [units][rows][2]: (sum b^2, sum y^2).
template <typename T, int TAPS, bool STAGED, bool TRACES>
__global__ void __launch_bounds__(kTbThreads) k_time_beam(const T* __restrict__ x, const T* __restrict__ taps,
                                                          const int32_t* __restrict__ shift, const int32_t* __restrict__ phase,
                                                          T* __restrict__ out, TbArgs a) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  __shared__ int32_t s_off[kTbRowBlock][kWave];  // shift + max_shift (0 .. 2 max_shift) of a good row
  __shared__ int32_t s_phase[kTbRowBlock][kWave];
  __shared__ int32_t s_good[kTbRowBlock];
  T* __restrict__ rec = reinterpret_cast<T*>(lds_raw);
  constexpr int CEN = (TAPS - 1) / 2, NV = TAPS + kTbOwn - 1;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = __builtin_amdgcn_readfirstlane(tid / kWave);
  const int64_t unit = (int64_t)blockIdx.x / a.nrb, row0 = ((int64_t)blockIdx.x % a.nrb) * kTbRowBlock;
  const int C = a.C;

  // ---- the tables of the workgroup's rows, checked before anything is indexed with them: lane = sensor ----
#pragma unroll
  for (int q = 0; q < kTbRowsPerWave; ++q) {
    const int lr = wv * kTbRowsPerWave + q;
    const int64_t g = row0 + lr;
    bool bad = false;
    if (g < a.rows && lane < C) {
      const int32_t s = shift[g * C + lane], p = phase[g * C + lane];
      bad = s > a.max_shift || s < -a.max_shift || p < 0 || p >= a.P;
      s_off[lr][lane] = bad ? 0 : s + a.max_shift;
      s_phase[lr][lane] = bad ? 0 : p;
    }
    const bool any_bad = __ballot(bad) != 0ull;
    if (lane == 0) s_good[lr] = (g < a.rows && !any_bad) ? 1 : 0;
  }
  __syncthreads();

  const int64_t t_begin = unit * a.unit_hop;
  const int64_t t_end = t_begin + a.unit_len < a.n ? t_begin + a.unit_len : a.n;
  T acc_b[kTbRowsPerWave], acc_e[kTbRowsPerWave];
#pragma unroll
  for (int q = 0; q < kTbRowsPerWave; ++q) acc_b[q] = acc_e[q] = T(0);

  for (int64_t t0 = t_begin; t0 < t_end; t0 += kTbChunk) {  // (uniform over the workgroup, as is the sensor loop: barriers inside)
    const int64_t t_lane = t0 + lane * kTbOwn;  // the lane's first output
    T b[kTbRowsPerWave][kTbOwn];
#pragma unroll
    for (int q = 0; q < kTbRowsPerWave; ++q)
#pragma unroll
      for (int r = 0; r < kTbOwn; ++r) b[q][r] = T(0);

    for (int i0 = 0; i0 < C; i0 += a.stage) {
      const int cs = C - i0 < a.stage ? C - i0 : a.stage;
      if constexpr (STAGED) {
        // sample j of a staged sensor is the record's sample t0 - max_shift - CEN + j, 0 <= j < 4 plane
        const int width = 4 * a.plane;
        __syncthreads();  // the readers of the sensors staged before
        for (int idx = tid; idx < cs * width; idx += kTbThreads) {
          const int ii = idx / width, j = idx - ii * width;
          const int64_t t = t0 - a.max_shift - CEN + j;
          const T v = (t >= 0 && t < a.n) ? x[(size_t)(i0 + ii) * (size_t)a.n + (size_t)t] : T(0);
          rec[ii * width + (j & 3) * a.plane + (j >> 2)] = v;
        }
        __syncthreads();
      }
#pragma unroll
      for (int q = 0; q < kTbRowsPerWave; ++q) {
        const int lr = wv * kTbRowsPerWave + q;
        if (!s_good[lr]) continue;  // (uniform over the wave)
        for (int ii = 0; ii < cs; ++ii) {
          const int s = __builtin_amdgcn_readfirstlane(s_off[lr][i0 + ii]);
          const int ph = __builtin_amdgcn_readfirstlane(s_phase[lr][i0 + ii]);
          const T* __restrict__ h = taps + (size_t)ph * TAPS;  // (wave-uniform)
          T v[NV];
          if constexpr (STAGED) {
            const T* __restrict__ sensor = rec + ii * 4 * a.plane + lane;
#pragma unroll
            for (int k = 0; k < NV; ++k) v[k] = sensor[((s + k) & 3) * a.plane + ((s + k) >> 2)];
          } else {
            const int64_t first = t_lane + (int64_t)(s - a.max_shift) - CEN;
            const T* __restrict__ sensor = x + (size_t)(i0 + ii) * (size_t)a.n;
#pragma unroll
            for (int k = 0; k < NV; ++k) {
              const int64_t t = first + k;
              v[k] = (t >= 0 && t < a.n) ? sensor[(size_t)t] : T(0);
            }
          }
          T tap[TAPS];
#pragma unroll
          for (int m = 0; m < TAPS; ++m) tap[m] = h[m];
#pragma unroll
          for (int r = 0; r < kTbOwn; ++r) {
            T y = T(0);
#pragma unroll
            for (int m = 0; m < TAPS; ++m) y = tb_fma(tap[m], v[r + m], y);
            b[q][r] += y;
            if constexpr (!TRACES) acc_e[q] = (t_lane + r < t_end) ? tb_fma(y, y, acc_e[q]) : acc_e[q];
          }
        }
      }
    }

    if constexpr (TRACES) {
#pragma unroll
      for (int q = 0; q < kTbRowsPerWave; ++q) {
        const int lr = wv * kTbRowsPerWave + q;
        const int64_t g = row0 + lr;
        if (g >= a.rows) continue;
        const bool good = s_good[lr] != 0;
#pragma unroll
        for (int r = 0; r < kTbOwn; ++r) {
          const int64_t t = t_lane + r;
          // (IEEE division: a double quotient of two float32 values rounds to the float32 quotient)
          if (t < t_end) out[(size_t)g * (size_t)a.n + (size_t)t] = good ? (T)((double)b[q][r] / (double)C) : (T)__builtin_nan("");
        }
      }
    } else {
#pragma unroll
      for (int q = 0; q < kTbRowsPerWave; ++q)
#pragma unroll
        for (int r = 0; r < kTbOwn; ++r) acc_b[q] = (t_lane + r < t_end) ? tb_fma(b[q][r], b[q][r], acc_b[q]) : acc_b[q];
    }
  }

  if constexpr (!TRACES) {
#pragma unroll
    for (int q = 0; q < kTbRowsPerWave; ++q) {  // (every lane of the wave is here: the loops have reconverged)
      const int lr = wv * kTbRowsPerWave + q;
      const int64_t g = row0 + lr;
      const T sb = wave_sum(acc_b[q]), se = wave_sum(acc_e[q]);
      if (lane == 0 && g < a.rows) {
        const bool good = s_good[lr] != 0;
        T* __restrict__ slot = out + ((size_t)unit * (size_t)a.rows + (size_t)g) * 2;
        slot[0] = good ? sb : (T)__builtin_nan("");
        slot[1] = good ? se : (T)__builtin_nan("");
      }
    }
  }
}

// np.argmax's order: a NaN before every number, a larger value before a smaller one, a lower index before a higher one
template <typename T>
__device__ __forceinline__ bool tb_before(T va, int64_t ia, T vb, int64_t ib) {
  const bool na = va != va, nb = vb != vb;
  if (na || nb) return na && (!nb || ia < ib);
  return va > vb || (va == vb && ia < ib);
}

// sums [units][G][2] -> power [nwin][G], the peak of every window; window w adds the units w .. w + per_window - 1
template <typename T>
__global__ void __launch_bounds__(kTbThreads) k_time_beam_finish(const T* __restrict__ sums, int64_t G, int64_t per_window, double c,
                                                                 double win, int normalize, T* __restrict__ power,
                                                                 int64_t* __restrict__ index, T* __restrict__ value) {
  __shared__ T sv[kTbThreads];
  __shared__ int64_t si[kTbThreads];
  const int tid = threadIdx.x;
  const int64_t w = blockIdx.x;
  T bv = T(0);
  int64_t bi = -1;  // (none yet: G may be below the thread count)
  for (int64_t g = tid; g < G; g += kTbThreads) {
    T sb = T(0), se = T(0);
    for (int64_t j = 0; j < per_window; ++j) {
      const T* __restrict__ slot = sums + ((size_t)(w + j) * (size_t)G + (size_t)g) * 2;
      sb += slot[0];
      se += slot[1];
    }
    const T p = (T)(normalize ? (double)sb / (c * (double)se) : (double)sb / (c * c * win));
    if (power) power[(size_t)w * (size_t)G + (size_t)g] = p;
    if (bi < 0 || tb_before(p, g, bv, bi)) {
      bv = p;
      bi = g;
    }
  }
  if (!index && !value) return;  // (uniform)
  sv[tid] = bv;
  si[tid] = bi;
  __syncthreads();
  for (int s = kTbThreads / 2; s > 0; s >>= 1) {
    if (tid < s && si[tid + s] >= 0 && (si[tid] < 0 || tb_before(sv[tid + s], si[tid + s], sv[tid], si[tid]))) {
      sv[tid] = sv[tid + s];
      si[tid] = si[tid + s];
    }
    __syncthreads();
  }
  if (tid == 0) {
    if (index) index[w] = si[0];
    if (value) value[w] = sv[0];
  }
}

// places of a plane of a staged sensor: the chunk and its halo in four planes, the pitch 8 mod 32
int tb_plane(int64_t max_shift, int64_t T) {
  const int64_t quarter = (kTbChunk + 2 * max_shift + T + 3) / 4;
  return (int)(quarter + ((8 - quarter % 32) + 32) % 32);
}

template <typename T, bool TRACES>
int launch_time_beam(const T* x, const T* taps, const int32_t* shift, const int32_t* phase, T* out, int64_t T_taps, int64_t units,
                     TbArgs a, hipStream_t st) {
  const bool staged = a.max_shift <= QI_TIMEBEAM_LDS_MAX_SHIFT;
  size_t lds = 0;
  a.stage = a.C;
  if (staged) {
    a.plane = tb_plane(a.max_shift, T_taps);
    const size_t sensor = (size_t)4 * a.plane * sizeof(T);
    a.stage = (int32_t)std::min<size_t>((size_t)a.C, std::max<size_t>(1, kTbStageBytes / sensor));
    lds = sensor * a.stage;
  }
  const dim3 grid((unsigned)(units * a.nrb));
  auto go = [&](auto kernel) -> int {
    if (lds) QI_TRY(allow_dynamic_lds(reinterpret_cast<const void*>(kernel), lds));
    kernel<<<grid, kTbThreads, lds, st>>>(x, taps, shift, phase, out, a);
    QI_LAUNCH_CHECK();
    return QI_OK;
  };
  auto by_taps = [&](auto staged_t) -> int {
    constexpr bool S = decltype(staged_t)::value;
    switch (T_taps) {
      case 1: return go(&k_time_beam<T, 1, S, TRACES>);
      case 2: return go(&k_time_beam<T, 2, S, TRACES>);
      case 4: return go(&k_time_beam<T, 4, S, TRACES>);
      case 8: return go(&k_time_beam<T, 8, S, TRACES>);
      default: return go(&k_time_beam<T, 16, S, TRACES>);
    }
  };
  return staged ? by_taps(std::true_type{}) : by_taps(std::false_type{});
}

}  // namespace

TimeBeamUnits time_beam_units(int64_t n, int64_t win, int64_t hop) {
  TimeBeamUnits u;
  u.nwin = 1 + (n - win) / hop;
  const bool by_hop = win % hop == 0 && hop >= kTbChunk;
  u.len = by_hop ? hop : win;
  u.per_window = by_hop ? win / hop : 1;
  u.count = u.nwin - 1 + u.per_window;
  return u;
}

int64_t time_beam_row_blocks(int64_t rows) { return ceil_div(rows, kTbRowBlock); }
int64_t time_beam_chunks(int64_t n) { return ceil_div(n, kTbChunk); }

template <typename T>
int launch_time_beam_power(const T* x, int64_t C, int64_t n, const T* taps, int64_t P, int64_t T_taps, const int32_t* shift,
                           const int32_t* phase, int64_t G, int64_t max_shift, int64_t win, int64_t hop, int normalize, T* power,
                           int64_t* peak_index, T* peak_value, T* sums, hipStream_t st) {
  const TimeBeamUnits u = time_beam_units(n, win, hop);
  TbArgs a{};
  a.n = n;
  a.rows = G;
  a.nrb = time_beam_row_blocks(G);
  a.unit_len = u.len;
  a.unit_hop = hop;
  a.C = (int32_t)C;
  a.P = (int32_t)P;
  a.max_shift = (int32_t)max_shift;
  QI_TRY((launch_time_beam<T, false>(x, taps, shift, phase, sums, T_taps, u.count, a, st)));
  k_time_beam_finish<T><<<dim3((unsigned)u.nwin), kTbThreads, 0, st>>>(sums, G, u.per_window, (double)C, (double)win, normalize != 0,
                                                                      power, peak_index, peak_value);
  QI_LAUNCH_CHECK();
  return QI_OK;
}

template <typename T>
int launch_time_beam_traces(const T* x, int64_t C, int64_t n, const T* taps, int64_t P, int64_t T_taps, const int32_t* shift,
                            const int32_t* phase, int64_t K, int64_t max_shift, T* out, hipStream_t st) {
  TbArgs a{};
  a.n = n;
  a.rows = K;
  a.nrb = time_beam_row_blocks(K);
  a.unit_len = kTbChunk;
  a.unit_hop = kTbChunk;
  a.C = (int32_t)C;
  a.P = (int32_t)P;
  a.max_shift = (int32_t)max_shift;
  return launch_time_beam<T, true>(x, taps, shift, phase, out, T_taps, time_beam_chunks(n), a, st);
}

template int launch_time_beam_power<float>(const float*, int64_t, int64_t, const float*, int64_t, int64_t, const int32_t*, const int32_t*,
                                           int64_t, int64_t, int64_t, int64_t, int, float*, int64_t*, float*, float*, hipStream_t);
template int launch_time_beam_power<double>(const double*, int64_t, int64_t, const double*, int64_t, int64_t, const int32_t*,
                                            const int32_t*, int64_t, int64_t, int64_t, int64_t, int, double*, int64_t*, double*, double*,
                                            hipStream_t);
template int launch_time_beam_traces<float>(const float*, int64_t, int64_t, const float*, int64_t, int64_t, const int32_t*, const int32_t*,
                                            int64_t, int64_t, float*, hipStream_t);
template int launch_time_beam_traces<double>(const double*, int64_t, int64_t, const double*, int64_t, int64_t, const int32_t*,
                                             const int32_t*, int64_t, int64_t, double*, hipStream_t);

}  // namespace qi
