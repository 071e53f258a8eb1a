// Zero-phase IIR filtering of records: scipy.signal.filtfilt / sosfiltfilt semantics (odd extension by `edge` samples,
// steady-state initial conditions, a forward and a backward pass) behind styx_fft.butter_bandpass / butter_highpass /
// butter_lowpass (styx_fft.py:60-149) and utilities.picker.apply_bandpass (picker.py:56-76).
//
// This file is compiled with -ffp-contract=off (_build.py: PER_FILE_FLAGS): every product and every sum of the recurrence is
// rounded on its own, in the order SciPy's lfilter / sosfilt evaluate them, so a float64 result is the reference's bit for bit.
// hipcc fuses a * b + c into one multiply-add otherwise -- through the _rn intrinsics and the contract pragma as well.
//
// A record is strictly sequential in time and any evaluation in blocks (block transition matrices) loses the (b, a) form's
// digits, so the parallelism is across records only: one lane per record, 64 records per wave, one wave per workgroup.
// Coefficients are kernel arguments (uniform: scalar registers), the filter state lives in vector registers.  Time moves
// through LDS in tiles of [64 records][64 samples]: the wave loads a tile row by row (lanes adjacent in time: 512-byte row
// segments), each lane then walks its own row (row stride 65 doubles: conflict-free column reads), and the results go back
// the same way.  The next tile's global loads are issued before the recurrence of the current one and land in registers
// while it runs.  Two launches per call: the forward pass forms the tapered, odd-extended record on the fly from `sig`
// and writes its n + 2 edge results to scratch; the backward pass reads scratch from the end (its first value is the
// y_last the state starts from) and stores only the n kept samples, stopping where the left extension begins.
// With fewer than 64 records the other lanes idle and a call is bound by one record's dependent chain of
// 2 (n + 2 edge) steps.
//
// The kernel is templated on the arithmetic type T.  qi_filtfilt runs it in double whatever the records' type (the
// reference returns float64); qi_decimate (scipy.signal.decimate(x, q, zero_phase=True) behind
// utilities.sampling.decimate_timeseries / _collection, sampling.py:123-146) runs it in the record's type -- SciPy casts
// the sections to it, so a float32 record is extended, filtered and returned in float32, no double anywhere -- and its
// backward pass keeps only the record positions k = 0, q, 2q, ..: the kept values of a tile are gathered from LDS so
// that adjacent lanes store adjacent columns of out [C][ceil(n / q)].
#include "qi_host.hpp"
#include "qi_device.hpp"   // kWave
#include "qi_fft_reg.hpp"  // QI_LAUNCH_CHECK

namespace qi {

namespace {

constexpr int kIirRows = kWave;            // records per workgroup (one wave)
constexpr int kIirTile = 64;               // samples per tile
constexpr int kIirStride = kIirTile + 1;   // values per LDS row: odd, so a column walk is conflict-free in float and double
constexpr int kIirMax = 16;                // largest order of the (b, a) form, most sections of the SOS form

template <typename T>
struct IirTables {
  T coef[6 * kIirMax];  // QI_IIR_BA: b[0..N], a[0..N];  QI_IIR_SOS: [sections][6]
  T zi[2 * kIirMax];    // QI_IIR_BA: [N];  QI_IIR_SOS: [sections][2]
};

// T: the type of the arithmetic, of scratch and of out.  T = double takes float32 or float64 records, T = float float32 ones.
template <typename T>
struct IirArgs {
  const void* sig;      // [C][n] float32 / float64 (forward)
  const double* taper;  // [n] or null (forward); T = double only
  T* scratch;           // [C][n + 2 edge]: written by the forward pass, read by the backward pass
  T* out;               // [C][n], or [C][m] of a decimating backward pass
  int64_t C, n, edge;
  int64_t q, m;         // decimating backward pass: record position k = c q goes to column c < m = ceil(n / q)
  int f32;              // the records are float32
};

// The recurrences.  N: order of the (b, a) form, sections of the SOS form.
template <typename T, int FORM, int N>
struct Iir {
  static constexpr int kState = N;
  static __device__ __forceinline__ void start(T* z, const IirTables<T>& t, T s) {
#pragma unroll
    for (int i = 0; i < N; ++i) z[i] = t.zi[i] * s;
  }
  // transposed direct form II, as lfilter: y = b0 x + z0; z_i = (b_{i+1} x + z_{i+1}) - a_{i+1} y; z_{N-1} = b_N x - a_N y
  static __device__ __forceinline__ T step(T* z, const IirTables<T>& t, T x) {
    const T* b = t.coef;
    const T* a = t.coef + N + 1;
    const T y = b[0] * x + z[0];
#pragma unroll
    for (int i = 0; i < N - 1; ++i) z[i] = (b[i + 1] * x + z[i + 1]) - a[i + 1] * y;
    z[N - 1] = b[N] * x - a[N] * y;
    return y;
  }
};
template <typename T, int N>
struct Iir<T, QI_IIR_SOS, N> {
  static constexpr int kState = 2 * N;
  static __device__ __forceinline__ void start(T* z, const IirTables<T>& t, T s) {
#pragma unroll
    for (int i = 0; i < 2 * N; ++i) z[i] = t.zi[i] * s;
  }
  // as sosfilt, through the sections in order: xn = b0 xc + z0; z0 = (b1 xc - a1 xn) + z1; z1 = b2 xc - a2 xn; xc = xn
  static __device__ __forceinline__ T step(T* z, const IirTables<T>& t, T xc) {
#pragma unroll
    for (int s = 0; s < N; ++s) {
      const T* c = t.coef + 6 * s;
      const T xn = c[0] * xc + z[2 * s];
      z[2 * s] = (c[1] * xc - c[4] * xn) + z[2 * s + 1];
      z[2 * s + 1] = c[2] * xc - c[5] * xn;
      xc = xn;
    }
    return xc;
  }
};

// sample k of a record after the taper: the product is formed in float64 and rounded to the record's type
__device__ __forceinline__ float tapered(const IirArgs<float>& a, int64_t row, int64_t k) {
  return static_cast<const float*>(a.sig)[row * a.n + k];  // (float arithmetic takes no taper)
}
__device__ __forceinline__ double tapered(const IirArgs<double>& a, int64_t row, int64_t k) {
  if (a.f32) {
    const float v = static_cast<const float*>(a.sig)[row * a.n + k];
    return a.taper ? (double)(float)((double)v * a.taper[k]) : (double)v;
  }
  const double v = static_cast<const double*>(a.sig)[row * a.n + k];
  return a.taper ? v * a.taper[k] : v;
}

// position p (0 <= p < n + 2 edge) of the odd extension; x0, xl: the record's tapered first and last sample.  n > edge keeps
// every index inside the record: the left piece reads x[1 .. edge], the right piece x[n - 1 - edge .. n - 2].
template <typename T>
__device__ __forceinline__ T extended(const IirArgs<T>& a, int64_t row, int64_t p, T x0, T xl) {
  const int64_t k = p - a.edge;
  if (k >= 0 && k < a.n) return tapered(a, row, k);
  const T end = k < 0 ? x0 : xl;
  const T v = tapered(a, row, k < 0 ? -k : 2 * a.n - 2 - k);
  if constexpr (sizeof(T) == sizeof(double)) {
    if (a.f32) return (double)(2.0f * (float)end - (float)v);  // a float32 record is extended in float32
  }
  return T(2) * end - v;
}

// BACK: the backward pass.  DECIM (backward pass only): store every q-th record position instead of all of them.
template <typename T, int FORM, int N, bool BACK, bool DECIM>
__global__ void __launch_bounds__(kIirRows) k_iir(IirArgs<T> a, IirTables<T> tab) {
  static_assert(BACK || !DECIM, "only the backward pass decimates");
  using R = Iir<T, FORM, N>;
  __shared__ T tile[kIirRows * kIirStride];
  __shared__ T ends[kIirRows][2];
  const int lane = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * kIirRows;
  const int rows = (int)(a.C - row0 < kIirRows ? a.C - row0 : kIirRows);
  const int64_t ext = a.n + 2 * a.edge;
  const int64_t steps = BACK ? a.n + a.edge : ext;  // the backward pass stops at the first kept sample
  if (!BACK) {
    if (lane < rows) {
      ends[lane][0] = tapered(a, row0 + lane, 0);
      ends[lane][1] = tapered(a, row0 + lane, a.n - 1);
    }
    __syncthreads();
  }
  T stage[kIirRows];
#pragma unroll
  for (int r = 0; r < kIirRows; ++r) stage[r] = T(0);
  // (uniform) the steps of tile t0 are samples of the record itself, or values of the forward pass: such a tile is fetched
  // ahead through registers; the few tiles of the forward pass that touch the extension are formed straight into LDS
  auto plain = [&](int64_t t0) { return BACK || (t0 >= a.edge && t0 + kIirTile <= a.edge + a.n); };
  // step t0 + lane of every record of the workgroup -> stage[record]
  auto fetch = [&](int64_t t0) {
    const int64_t j = t0 + lane;
    if (BACK) {
      if (j < steps) {
#pragma unroll
        for (int r = 0; r < kIirRows; ++r)
          if (r < rows) stage[r] = a.scratch[(row0 + r) * ext + (ext - 1 - j)];  // (r < rows: uniform)
      }
    } else if (plain(t0)) {  // as tapered(); a missing taper multiplies by one, which changes no value
      const int64_t k = j - a.edge;
      if constexpr (sizeof(T) == sizeof(float)) {
        const float* src = static_cast<const float*>(a.sig) + row0 * a.n + k;
#pragma unroll
        for (int r = 0; r < kIirRows; ++r)
          if (r < rows) stage[r] = src[r * a.n];
      } else {
        const double w = a.taper ? a.taper[k] : 1.0;
        if (a.f32) {
          const float* src = static_cast<const float*>(a.sig) + row0 * a.n + k;
#pragma unroll
          for (int r = 0; r < kIirRows; ++r)
            if (r < rows) stage[r] = (double)(float)((double)src[r * a.n] * w);
        } else {
          const double* src = static_cast<const double*>(a.sig) + row0 * a.n + k;
#pragma unroll
          for (int r = 0; r < kIirRows; ++r)
            if (r < rows) stage[r] = src[r * a.n] * w;
        }
      }
    }
  };
  fetch(0);
  T z[R::kState];
#pragma unroll
  for (int i = 0; i < R::kState; ++i) z[i] = T(0);
  for (int64_t t0 = 0; t0 < steps; t0 += kIirTile) {
    if (plain(t0)) {
#pragma unroll
      for (int r = 0; r < kIirRows; ++r) tile[r * kIirStride + lane] = stage[r];
    } else if (t0 + lane < steps) {
#pragma unroll 1
      for (int r = 0; r < rows; ++r) tile[r * kIirStride + lane] = extended(a, row0 + r, t0 + lane, ends[r][0], ends[r][1]);
    }
    __syncthreads();
    if (t0 + kIirTile < steps) fetch(t0 + kIirTile);  // in flight during the recurrence
    const int cnt = (int)(steps - t0 < kIirTile ? steps - t0 : kIirTile);
    if (lane < rows) {
      T* mine = tile + lane * kIirStride;
      if (t0 == 0) R::start(z, tab, mine[0]);  // zi * ext[0] (forward), zi * y_last (backward)
#pragma unroll 4
      for (int k = 0; k < cnt; ++k) mine[k] = R::step(z, tab, mine[k]);
    }
    __syncthreads();
    if constexpr (DECIM) {
      // the tile holds the record positions hi, hi - 1, .., hi - cnt + 1 >= 0 at its indices 0 .. cnt - 1: the phase of the
      // kept ones comes from the position, not from the tile (64 is in general no multiple of q, and the pass runs from
      // the end).  Kept columns c0 .. c1 (c q inside the tile and below n): lane i gathers column c0 + i from LDS.
      const int64_t hi = a.n + a.edge - 1 - t0;
      const int64_t lo = hi - cnt + 1;
      const int64_t c0 = (lo + a.q - 1) / a.q;
      const int64_t c1 = (hi < a.n ? hi : a.n - 1) / a.q;  // < m
      const int64_t c = c0 + lane;
      if (c <= c1) {
        const int at = (int)(hi - c * a.q);  // 0 <= at < cnt as lo <= c q <= hi
        for (int r = 0; r < rows; ++r) a.out[(row0 + r) * a.m + c] = tile[r * kIirStride + at];
      }
    } else if (lane < cnt) {
      const int64_t j = t0 + lane;
      for (int r = 0; r < rows; ++r) {
        const T y = tile[r * kIirStride + lane];
        if (BACK) {
          const int64_t k = ext - 1 - j - a.edge;  // >= 0 as j < n + edge
          if (k < a.n) a.out[(row0 + r) * a.n + k] = y;
        } else {
          a.scratch[(row0 + r) * ext + j] = y;
        }
      }
    }
    __syncthreads();
  }
}

template <typename T, int FORM, int N, bool DECIM>
int launch_passes(const IirArgs<T>& a, const IirTables<T>& tab, hipStream_t st) {
  const unsigned grid = (unsigned)ceil_div(a.C, kIirRows);
  k_iir<T, FORM, N, false, false><<<grid, kIirRows, 0, st>>>(a, tab);
  QI_LAUNCH_CHECK();
  k_iir<T, FORM, N, true, DECIM><<<grid, kIirRows, 0, st>>>(a, tab);
  QI_LAUNCH_CHECK();
  return QI_OK;
}

template <typename T, int FORM, bool DECIM>
int launch_order(int N, const IirArgs<T>& a, const IirTables<T>& tab, hipStream_t st) {
  switch (N) {
#define QI_IIR_CASE(K) \
  case K:              \
    return launch_passes<T, FORM, K, DECIM>(a, tab, st);
    QI_IIR_CASE(1)
    QI_IIR_CASE(2)
    QI_IIR_CASE(3)
    QI_IIR_CASE(4)
    QI_IIR_CASE(5)
    QI_IIR_CASE(6)
    QI_IIR_CASE(7)
    QI_IIR_CASE(8)
    QI_IIR_CASE(9)
    QI_IIR_CASE(10)
    QI_IIR_CASE(11)
    QI_IIR_CASE(12)
    QI_IIR_CASE(13)
    QI_IIR_CASE(14)
    QI_IIR_CASE(15)
    QI_IIR_CASE(16)
#undef QI_IIR_CASE
    default:
      break;
  }
  set_error("filter of %d %s: 1 .. %d", N, FORM == QI_IIR_SOS ? "sections" : "poles", kIirMax);
  return QI_ERR_ARG;
}

}  // namespace

}  // namespace qi

using namespace qi;

extern "C" {

int64_t qi_filtfilt_scratch_bytes(int64_t n_channels, int64_t n, int64_t edge) {
  QI_REQUIRE(n_channels >= 1, "bad record count %lld", (long long)n_channels);
  QI_REQUIRE(edge >= 0 && n > edge, "a record of %lld samples must be longer than the extension of %lld", (long long)n,
             (long long)edge);
  QI_REQUIRE(n < (1ll << 40) && n_channels < (1ll << 40) / (n + 2 * edge), "request too large");
  return n_channels * (n + 2 * edge) * (int64_t)sizeof(double);
}

int qi_filtfilt(int dtype, int device, const void* sig, int64_t n_channels, int64_t n, const void* taper, int form,
                int32_t sections, int32_t order, const double* coef, const double* zi, int64_t edge, void* out, void* scratch,
                int64_t scratch_bytes, qi_stream stream) {
  QI_REQUIRE(dtype == QI_F32 || dtype == QI_F64, "bad dtype %d", dtype);
  QI_REQUIRE(form == QI_IIR_BA || form == QI_IIR_SOS, "bad filter form %d", form);
  QI_REQUIRE(sig && out && scratch && coef && zi, "null argument");
  const int64_t need = qi_filtfilt_scratch_bytes(n_channels, n, edge);
  if (need < 0) return (int)need;
  QI_TRY(require_scratch(scratch_bytes, need));
  QI_REQUIRE(aligned(scratch, 8) && aligned(out, 8), "scratch and out must be aligned to 8 bytes");
  IirTables<double> tab{};
  int N;
  if (form == QI_IIR_BA) {
    QI_REQUIRE(sections == 1, "the (b, a) form is one section (got %d)", (int)sections);
    QI_REQUIRE(order >= 1 && order <= kIirMax, "order %d of the (b, a) form: 1 .. %d", (int)order, kIirMax);
    QI_REQUIRE(coef[order + 1] == 1.0, "a[0] must be 1 (got %g): normalise the coefficients", coef[order + 1]);
    N = order;
    for (int i = 0; i < 2 * (N + 1); ++i) tab.coef[i] = coef[i];
    for (int i = 0; i < N; ++i) tab.zi[i] = zi[i];
  } else {
    QI_REQUIRE(order == 2, "second-order sections have order 2 (got %d)", (int)order);
    QI_REQUIRE(sections >= 1 && sections <= kIirMax, "%d sections: 1 .. %d", (int)sections, kIirMax);
    N = sections;
    for (int s = 0; s < N; ++s) QI_REQUIRE(coef[6 * s + 3] == 1.0, "a[0] of section %d must be 1 (got %g)", s, coef[6 * s + 3]);
    for (int i = 0; i < 6 * N; ++i) tab.coef[i] = coef[i];
    for (int i = 0; i < 2 * N; ++i) tab.zi[i] = zi[i];
  }
  IirArgs<double> a{};
  a.sig = sig;
  a.taper = static_cast<const double*>(taper);
  a.scratch = static_cast<double*>(scratch);
  a.out = static_cast<double*>(out);
  a.C = n_channels;
  a.n = n;
  a.edge = edge;
  a.f32 = dtype == QI_F32;
  DeviceGuard g(device);
  QI_REQUIRE(g.ok, "cannot select device %d", device);
  return form == QI_IIR_BA ? launch_order<double, QI_IIR_BA, false>(N, a, tab, (hipStream_t)stream)
                           : launch_order<double, QI_IIR_SOS, false>(N, a, tab, (hipStream_t)stream);
}

int64_t qi_decimate_columns(int64_t n, int64_t q) {
  QI_REQUIRE(n >= 1 && q >= 1, "decimation of %lld samples by %lld: both must be positive", (long long)n, (long long)q);
  return (n - 1) / q + 1;
}

int64_t qi_decimate_scratch_bytes(int dtype, int64_t n_channels, int64_t n, int64_t edge) {
  QI_REQUIRE(dtype == QI_F32 || dtype == QI_F64, "bad dtype %d", dtype);
  const int64_t as_f64 = qi_filtfilt_scratch_bytes(n_channels, n, edge);  // the same [C][n + 2 edge], in the record's type
  return as_f64 < 0 || dtype == QI_F64 ? as_f64 : as_f64 / 2;
}

int qi_decimate(int dtype, int device, const void* sig, int64_t n_channels, int64_t n, int64_t q, int32_t sections,
                const void* sos, const void* zi, int64_t edge, void* out, void* scratch, int64_t scratch_bytes,
                qi_stream stream) {
  QI_REQUIRE(sig && out && scratch && sos && zi, "null argument");
  const int64_t need = qi_decimate_scratch_bytes(dtype, n_channels, n, edge);
  if (need < 0) return (int)need;
  const int64_t m = qi_decimate_columns(n, q);
  if (m < 0) return (int)m;
  QI_TRY(require_scratch(scratch_bytes, need));
  const size_t esz = elem_size(dtype);
  QI_REQUIRE(aligned(scratch, esz) && aligned(out, esz) && aligned(sig, esz), "sig, scratch and out must be aligned to %d bytes",
             (int)esz);
  QI_REQUIRE(sections >= 1 && sections <= kIirMax, "%d sections: 1 .. %d", (int)sections, kIirMax);
  auto run = [&](auto zero) -> int {
    using T = decltype(zero);
    const T* c = static_cast<const T*>(sos);
    const T* z = static_cast<const T*>(zi);
    IirTables<T> tab{};
    for (int s = 0; s < sections; ++s)
      QI_REQUIRE(c[6 * s + 3] == T(1), "a[0] of section %d must be 1 (got %g)", s, (double)c[6 * s + 3]);
    for (int i = 0; i < 6 * sections; ++i) tab.coef[i] = c[i];
    for (int i = 0; i < 2 * sections; ++i) tab.zi[i] = z[i];
    IirArgs<T> a{};
    a.sig = sig;
    a.taper = nullptr;
    a.scratch = static_cast<T*>(scratch);
    a.out = static_cast<T*>(out);
    a.C = n_channels;
    a.n = n;
    a.edge = edge;
    a.q = q;
    a.m = m;
    a.f32 = dtype == QI_F32;
    DeviceGuard g(device);
    QI_REQUIRE(g.ok, "cannot select device %d", device);
    return launch_order<T, QI_IIR_SOS, true>(sections, a, tab, (hipStream_t)stream);
  };
  return by_dtype(dtype, run);
}

}  // extern "C"
