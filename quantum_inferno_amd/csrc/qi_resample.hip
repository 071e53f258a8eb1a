// Resampling of records: utilities.sampling.resample_uneven_timeseries (sampling.py:53-68: np.interp onto np.arange) and
// resample_with_sample_rate (sampling.py:71-83: scipy.signal.resample), restated.
//
// qi_interp_grid: linear interpolation of records with uneven timestamps (knots) onto the even grid x_i = start + i * delta.
// A workgroup of kItThreads lanes owns QI_INTERP_TILE consecutive outputs of one record; the grid is (tiles, records), one
// launch, no scratch, no atomics.  Per workgroup:
//   1 the x of its first and of its last output, by the expression the lanes use (grid_x), so the range below holds every lane's x;
//   2 the knot range: j_lo = the last knot <= x_first (0 when there is none), j_hi = the last knot <= x_last, found by every
//     wave for itself with a 64-ary search in global memory -- lane l probes knot lo + (l + 1) step, a ballot counts the
//     leading lanes whose knot is <= x, four rounds for 2^20 knots instead of twenty dependent loads of a bisection -- so no
//     wave waits for another one and all four hold the same range;
//   3 when the knots j_lo .. min(j_hi + 1, n - 1) are at most QI_INTERP_KNOTS: they and their values (widened to double) go
//     to LDS with coalesced loads, and each lane looks its interval up there: a guess from the output's position in the tile,
//     a galloping step away from it and a bisection of what is left (two or three reads when the rate is near-uniform).
//     Otherwise (heavy downsampling, a gather by nature) the lanes bisect j_lo .. j_hi in global memory;
//   4 np.interp's arithmetic on the interval, every operation rounded on its own; coalesced float64 stores.
// Every search is bounded by the range it was given and every index it forms lies in [0, n - 1], whatever the knots hold
// (unsorted, NaN): a probe that compares false only moves a bound.  Nothing depends on the order of execution: the same
// call gives the same bits.
//
// qi_resample_fft: batched R2C of length n (hipFFT, the plan cache of the plan-less entry points), one kernel that writes the
// m / 2 + 1 bins of the output spectrum (copied, the bin N / 2 of an even N = min(n, m) doubled or halved, zeros above,
// everything times 1 / n), batched C2R of length m.  A transform of one point is the identity and is done by that kernel.
//
// The file is compiled with -ffp-contract=off (_build.py: PER_FILE_FLAGS): the grid and the interpolation are NumPy's bit for
// bit only when no product is fused into a sum.
#include "qi_host.hpp"
#include "qi_device.hpp"   // kWave
#include "qi_fft_reg.hpp"  // QI_LAUNCH_CHECK

namespace qi {

namespace {

// QI_INTERP_TILE = 512 outputs: with 256 lanes (four waves, one per SIMD) a lane forms two outputs a whole row of lanes
// apart, so each store instruction of a wave writes 512 contiguous bytes; the fixed work of a tile (two range searches of
// four dependent probes) is spread over 4 KiB of stores and as many bytes of loads at unit rate.
// QI_INTERP_KNOTS = 5 tiles' worth: at an output rate r times the input's a tile brackets T / r + 2 knots, so resampling
// down to a quarter of the rate, with room for jitter, still streams its knots through LDS; 16 bytes a knot (float64
// timestamp and value) make 40 KiB a workgroup: four workgroups, sixteen waves, on a CU's 160 KiB, enough of them to hide
// one's searches behind the others' loads.
constexpr int kItTile = QI_INTERP_TILE;
constexpr int kItKnots = QI_INTERP_KNOTS;
constexpr int kItThreads = 256;
constexpr int kItVec = kItTile / kItThreads;  // outputs per lane
static_assert(kItTile % kItThreads == 0 && kItThreads % kWave == 0, "whole rows of lanes");
static_assert(kItKnots * 16 <= 64 * 1024, "static LDS of a workgroup");
constexpr int64_t kItMaxRecords = 65535;  // grid.y

struct InterpArgs {
  const void* values;    // [C][n] in the record's type
  const double* knots;   // [n] or [C][n]
  double* out;           // [C][m]
  int64_t knot_stride, n, m;
  double start, delta;
};

// the grid: the product rounded, then the sum (no fused multiply-add in this file)
__device__ __forceinline__ double grid_x(double start, double delta, int64_t i) { return start + (double)i * delta; }

// The last index j in [0, n) with k[j] <= x, -1 when k[0] <= x is false; by the whole wave (every lane active), the same
// value in every lane.  Invariant: lo = -1 or a probed knot <= x; hi = n or a probed knot that is not; the candidates
// lo + 1 .. hi - 1 shrink to less than a 64th per round, every probe lies strictly between lo and hi.
__device__ __forceinline__ int64_t wave_last_le(const double* __restrict__ k, int64_t n, double x) {
  const int lane = threadIdx.x & (kWave - 1);
  int64_t lo = -1, hi = n;
  while (hi - lo > 1) {
    const int64_t span = hi - lo - 1;
    const int64_t step = (span + kWave - 1) / kWave;
    const int64_t p = lo + (int64_t)(lane + 1) * step;
    const bool le = p < hi && k[p] <= x;
    const unsigned long long mask = __builtin_amdgcn_ballot_w64(le);
    const int c = mask == ~0ull ? kWave : __builtin_ctzll(~mask);  // leading lanes whose knot is <= x
    const int64_t first_gt = lo + (int64_t)(c + 1) * step;         // lane c's probe (not <= x), when it has one
    lo += (int64_t)c * step;
    if (c < kWave && first_gt < hi) hi = first_gt;
  }
  return lo;
}

// The last index j in [0, len) with k[j] <= x, 0 when there is none; `guess` in [0, len) or -1.  From a guess: double the
// step away from it until the knot on the far side answers the other way (or the range ends), then bisect.  Every index
// read lies in [0, len).
__device__ __forceinline__ int lane_last_le(const double* k, int len, double x, int guess) {
  int lo = 0, hi = len;  // k[lo] <= x (or lo = 0); hi = len or k[hi] is not <= x
  if (guess >= 0) {
    int step = 1;
    if (k[guess] <= x) {
      lo = guess;
      for (;;) {
        const int q = lo + step;
        if (q >= len) break;
        if (!(k[q] <= x)) {
          hi = q;
          break;
        }
        lo = q;
        step <<= 1;
      }
    } else {
      hi = guess;
      for (;;) {
        const int q = hi - step;
        if (q <= 0) break;
        if (k[q] <= x) {
          lo = q;
          break;
        }
        hi = q;
        step <<= 1;
      }
    }
  }
  while (hi - lo > 1) {
    const int mid = lo + ((hi - lo) >> 1);
    if (k[mid] <= x) lo = mid;
    else hi = mid;
  }
  return lo;
}
// the same over a range of any length in global memory, without a guess
__device__ __forceinline__ int64_t lane_last_le_global(const double* __restrict__ k, int64_t len, double x) {
  int64_t lo = 0, hi = len;
  while (hi - lo > 1) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (k[mid] <= x) lo = mid;
    else hi = mid;
  }
  return lo;
}

// np.interp between knot j and knot j + 1 (`last`: j is the record's last knot)
__device__ __forceinline__ double interp_value(double x, double xj, double fj, double xj1, double fj1, bool last) {
  if (last || xj == x) return fj;
  const double s = (fj1 - fj) / (xj1 - xj);
  double r = s * (x - xj) + fj;
  if (r != r) {
    r = s * (x - xj1) + fj1;
    if (r != r && fj == fj1) r = fj;
  }
  return r;
}

template <typename T>
__global__ void __launch_bounds__(kItThreads) k_interp_grid(InterpArgs a) {
  __shared__ double s_k[kItKnots];
  __shared__ double s_v[kItKnots];
  const int tid = threadIdx.x;
  const int64_t c = blockIdx.y, n = a.n;
  const int64_t i0 = (int64_t)blockIdx.x * kItTile;
  const int64_t i1 = i0 + kItTile < a.m ? i0 + kItTile : a.m;  // (i0 < m: the grid has ceil(m / tile) columns)
  const double* __restrict__ k = a.knots + c * a.knot_stride;
  const T* __restrict__ v = static_cast<const T*>(a.values) + c * n;
  double* __restrict__ out = a.out + c * a.m;

  const double x_first = grid_x(a.start, a.delta, i0), x_last = grid_x(a.start, a.delta, i1 - 1);
  int64_t j_lo = wave_last_le(k, n, x_first), j_hi = wave_last_le(k, n, x_last);
  if (j_lo < 0) j_lo = 0;
  if (j_hi < j_lo) j_hi = j_lo;  // (unsorted knots only)
  const int64_t j_end = j_hi + 1 < n ? j_hi + 1 : n - 1;  // the last knot a lane may read
  const int64_t held = j_end - j_lo + 1;
  const int64_t len = j_hi - j_lo + 1;  // knots a lane's interval may start at
  const bool staged = held <= kItKnots;
  if (staged) {  // (uniform in the workgroup: every wave found the same range)
    for (int q = tid; q < (int)held; q += kItThreads) {
      s_k[q] = k[j_lo + q];
      s_v[q] = (double)v[j_lo + q];
    }
    __syncthreads();
  }
  const double k_first = k[0], k_last = k[n - 1];
  const int tile_n = (int)(i1 - i0);
#pragma unroll
  for (int u = 0; u < kItVec; ++u) {
    const int t = tid + u * kItThreads;
    const int64_t i = i0 + t;
    if (i >= i1) continue;
    const double x = grid_x(a.start, a.delta, i);
    double r;
    if (x > k_last) {
      r = (double)v[n - 1];
    } else if (x < k_first) {
      r = (double)v[0];
    } else if (staged) {
      const int guess = (int)(((int64_t)t * len) / tile_n);  // t < tile_n: in [0, len)
      const int q = lane_last_le(s_k, (int)len, x, guess);
      const bool last = j_lo + q == n - 1;
      const int q1 = last ? q : q + 1;  // q + 1 <= j_end - j_lo: staged
      r = interp_value(x, s_k[q], s_v[q], s_k[q1], s_v[q1], last);
    } else {
      const int64_t j = j_lo + lane_last_le_global(k + j_lo, len, x);
      const bool last = j == n - 1;
      const int64_t j1 = last ? j : j + 1;
      r = interp_value(x, k[j], (double)v[j], k[j1], (double)v[j1], last);
    }
    out[i] = r;
  }
}

// ---- the FFT resampler's spectrum ----------------------------------------------------------------------------------------
constexpr int kRsThreads = 256;

// Y[c][j], j <= m / 2, from X[c][.] (n / 2 + 1 bins; or, when n = 1, from the record itself: its transform).  When m = 1
// the result is the real part of bin 0 (the inverse transform of one point) and goes to `out`.
template <typename T>
__global__ void __launch_bounds__(kRsThreads) k_resample_spectrum(const cplx<T>* __restrict__ X, const T* __restrict__ sig,
                                                                  cplx<T>* __restrict__ Y, T* __restrict__ out, int64_t C,
                                                                  int64_t n, int64_t m) {
  const int64_t nfo = m / 2 + 1, nfi = n / 2 + 1;
  const int64_t N = n < m ? n : m, top = N / 2;
  const T scale = (T)(1.0 / (double)n);
  const int64_t total = C * nfo;
  for (int64_t e = (int64_t)blockIdx.x * kRsThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kRsThreads) {
    const int64_t c = e / nfo, j = e - c * nfo;
    cplx<T> y = mk<T>(T(0), T(0));
    if (j <= top) {
      y = n == 1 ? mk<T>(sig[c], T(0)) : X[c * nfi + j];
      if (j == top && (N & 1) == 0 && n != m) {
        const T w = m < n ? T(2) : T(0.5);
        y.x *= w;
        y.y *= w;
      }
      y.x *= scale;
      y.y *= scale;
    }
    if (m == 1) out[c] = y.x;
    else Y[e] = y;
  }
}

template <typename Transform>
int resample_locked_fft(int device, Transform&& transform) {
  std::lock_guard<std::mutex> lk(g_stft_mu);
  return transform(g_stft_fft[device]);
}

struct ResampleScratch {
  size_t copy, spec_in, spec_out, total;
  ResampleScratch(int dtype, int64_t C, int64_t n, int64_t m) {
    const size_t esz = elem_size(dtype);
    copy = 0;  // the records (the real-to-complex transform may overwrite its input)
    spec_in = copy + host::align_up((size_t)C * n * esz);
    spec_out = spec_in + host::align_up((size_t)C * (n / 2 + 1) * 2 * esz);
    total = spec_out + host::align_up((size_t)C * (m / 2 + 1) * 2 * esz);
  }
};

}  // namespace

}  // namespace qi

using namespace qi;

extern "C" {

int qi_interp_grid(int dtype, int device, const void* values, const void* knots, int64_t knot_stride, int64_t n_channels,
                   int64_t n, double start, double delta, int64_t m, void* out, qi_stream stream) {
  QI_TRY(require_records(dtype, n_channels, n));
  QI_REQUIRE(m >= 0, "bad output length %lld", (long long)m);
  QI_TRY(require_timestamp_stride("knot_stride", knot_stride, n));
  QI_REQUIRE(std::isfinite(start), "start must be finite");
  QI_REQUIRE(std::isfinite(delta) && delta > 0.0, "delta must be finite and positive");
  QI_REQUIRE(values && knots && out, "null argument");
  QI_REQUIRE(n < (1ll << 40) && m < (1ll << 40), "request too large");
  const size_t esz = elem_size(dtype);
  QI_REQUIRE(aligned(values, esz) && aligned(knots, 8) && aligned(out, 8),
             "values, knots and out must be aligned to their element size");
  if (m == 0) return QI_OK;
  DeviceGuard g(device);
  QI_REQUIRE(g.ok, "cannot select device %d", device);
  for (int64_t c0 = 0; c0 < n_channels; c0 += kItMaxRecords) {  // (one launch up to 65535 records: the grid's second extent)
    const int64_t cn = n_channels - c0 < kItMaxRecords ? n_channels - c0 : kItMaxRecords;
    InterpArgs a{};
    a.values = static_cast<const char*>(values) + (size_t)c0 * n * esz;
    a.knots = static_cast<const double*>(knots) + c0 * knot_stride;
    a.out = static_cast<double*>(out) + c0 * m;
    a.knot_stride = knot_stride;
    a.n = n;
    a.m = m;
    a.start = start;
    a.delta = delta;
    const dim3 grid((unsigned)ceil_div(m, kItTile), (unsigned)cn);
    if (dtype == QI_F64) k_interp_grid<double><<<grid, kItThreads, 0, (hipStream_t)stream>>>(a);
    else k_interp_grid<float><<<grid, kItThreads, 0, (hipStream_t)stream>>>(a);
    QI_LAUNCH_CHECK();
  }
  return QI_OK;
}

int64_t qi_resample_fft_scratch_bytes(int dtype, int64_t n_channels, int64_t n, int64_t m) {
  QI_TRY(require_records(dtype, n_channels, n));
  QI_REQUIRE(m >= 1, "bad output length %lld", (long long)m);
  QI_REQUIRE(n < (1ll << 31) && m < (1ll << 31) && n_channels < (1ll << 31) && n_channels * (n > m ? n : m) < (1ll << 40),
             "request too large");
  return (int64_t)ResampleScratch(dtype, n_channels, n, m).total;
}

int qi_resample_fft(int dtype, int device, const void* sig, int64_t n_channels, int64_t n, int64_t m, void* out, void* scratch,
                    int64_t scratch_bytes, qi_stream stream) {
  const int64_t need = qi_resample_fft_scratch_bytes(dtype, n_channels, n, m);
  if (need < 0) return (int)need;
  QI_REQUIRE(sig && out && scratch, "null argument");
  QI_TRY(require_scratch(scratch_bytes, need));
  QI_REQUIRE(aligned(scratch, 16), "scratch must be aligned to 16 bytes");
  DeviceGuard g(device);
  QI_REQUIRE(g.ok, "cannot select device %d", device);
  hipStream_t st = (hipStream_t)stream;
  const ResampleScratch l(dtype, n_channels, n, m);
  char* s = static_cast<char*>(scratch);
  const int64_t C = n_channels;
  return by_dtype(dtype, [&](auto t) -> int {
    using T = decltype(t);
    T* copy = reinterpret_cast<T*>(s + l.copy);
    cplx<T>* X = reinterpret_cast<cplx<T>*>(s + l.spec_in);
    cplx<T>* Y = reinterpret_cast<cplx<T>*>(s + l.spec_out);
    if (n > 1) {
      QI_HIP(hipMemcpyAsync(copy, sig, (size_t)C * n * sizeof(T), hipMemcpyDeviceToDevice, st));
      QI_TRY(resample_locked_fft(device, [&](FftCache& fc) { return fft_r2c<T>(fc, copy, X, n, C, st); }));
    }
    const int64_t total = C * (m / 2 + 1);
    const int64_t blocks = std::min<int64_t>(ceil_div(total, kRsThreads), 2048);
    k_resample_spectrum<T><<<(unsigned)blocks, kRsThreads, 0, st>>>(X, (const T*)sig, Y, (T*)out, C, n, m);
    QI_LAUNCH_CHECK();
    if (m > 1) QI_TRY(resample_locked_fft(device, [&](FftCache& fc) { return fft_c2r<T>(fc, Y, (T*)out, m, C, st); }));
    return QI_OK;
  });
}

}  // extern "C"
