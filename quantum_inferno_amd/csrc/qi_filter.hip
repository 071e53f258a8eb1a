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
#include "qi_host.hpp"
#include "qi_device.hpp"   // kWave
#include "qi_fft_reg.hpp"  // QI_LAUNCH_CHECK

namespace qi {

namespace {

constexpr int kIirRows = kWave;            // records per workgroup (one wave)
constexpr int kIirTile = 64;               // samples per tile
constexpr int kIirStride = kIirTile + 1;   // doubles per LDS row
constexpr int kIirMax = 16;                // largest order of the (b, a) form, most sections of the SOS form

struct IirTables {
  double coef[6 * kIirMax];  // QI_IIR_BA: b[0..N], a[0..N];  QI_IIR_SOS: [sections][6]
  double zi[2 * kIirMax];    // QI_IIR_BA: [N];  QI_IIR_SOS: [sections][2]
};

struct IirArgs {
  const void* sig;      // [C][n] float32 / float64 (forward)
  const double* taper;  // [n] or null (forward)
  double* scratch;      // [C][n + 2 edge]: written by the forward pass, read by the backward pass
  double* out;          // [C][n] (backward)
  int64_t C, n, edge;
  int f32;              // the records are float32
};

// The recurrences.  N: order of the (b, a) form, sections of the SOS form.
template <int FORM, int N>
struct Iir {
  static constexpr int kState = N;
  static __device__ __forceinline__ void start(double* z, const IirTables& t, double s) {
#pragma unroll
    for (int i = 0; i < N; ++i) z[i] = t.zi[i] * s;
  }
  // transposed direct form II, as lfilter: y = b0 x + z0; z_i = (b_{i+1} x + z_{i+1}) - a_{i+1} y; z_{N-1} = b_N x - a_N y
  static __device__ __forceinline__ double step(double* z, const IirTables& t, double x) {
    const double* b = t.coef;
    const double* a = t.coef + N + 1;
    const double y = b[0] * x + z[0];
#pragma unroll
    for (int i = 0; i < N - 1; ++i) z[i] = (b[i + 1] * x + z[i + 1]) - a[i + 1] * y;
    z[N - 1] = b[N] * x - a[N] * y;
    return y;
  }
};
template <int N>
struct Iir<QI_IIR_SOS, N> {
  static constexpr int kState = 2 * N;
  static __device__ __forceinline__ void start(double* z, const IirTables& t, double s) {
#pragma unroll
    for (int i = 0; i < 2 * N; ++i) z[i] = t.zi[i] * s;
  }
  // as sosfilt, through the sections in order: xn = b0 xc + z0; z0 = (b1 xc - a1 xn) + z1; z1 = b2 xc - a2 xn; xc = xn
  static __device__ __forceinline__ double step(double* z, const IirTables& t, double xc) {
#pragma unroll
    for (int s = 0; s < N; ++s) {
      const double* c = t.coef + 6 * s;
      const double xn = c[0] * xc + z[2 * s];
      z[2 * s] = (c[1] * xc - c[4] * xn) + z[2 * s + 1];
      z[2 * s + 1] = c[2] * xc - c[5] * xn;
      xc = xn;
    }
    return xc;
  }
};

// sample k of a record after the taper: the product is formed in float64 and rounded to the record's type
__device__ __forceinline__ double tapered(const IirArgs& a, int64_t row, int64_t k) {
  if (a.f32) {
    const float v = static_cast<const float*>(a.sig)[row * a.n + k];
    return a.taper ? (double)(float)((double)v * a.taper[k]) : (double)v;
  }
  const double v = static_cast<const double*>(a.sig)[row * a.n + k];
  return a.taper ? v * a.taper[k] : v;
}

// position p (0 <= p < n + 2 edge) of the odd extension; x0, xl: the record's tapered first and last sample.  n > edge keeps
// every index inside the record: the left piece reads x[1 .. edge], the right piece x[n - 1 - edge .. n - 2].
__device__ __forceinline__ double extended(const IirArgs& a, int64_t row, int64_t p, double x0, double xl) {
  const int64_t k = p - a.edge;
  if (k >= 0 && k < a.n) return tapered(a, row, k);
  const double end = k < 0 ? x0 : xl;
  const double v = tapered(a, row, k < 0 ? -k : 2 * a.n - 2 - k);
  if (a.f32) return (double)(2.0f * (float)end - (float)v);  // a float32 record is extended in float32
  return 2.0 * end - v;
}

template <int FORM, int N, bool BACK>
__global__ void __launch_bounds__(kIirRows) k_iir(IirArgs a, IirTables tab) {
  using R = Iir<FORM, N>;
  __shared__ double tile[kIirRows * kIirStride];
  __shared__ double ends[kIirRows][2];
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
  double stage[kIirRows];
#pragma unroll
  for (int r = 0; r < kIirRows; ++r) stage[r] = 0.0;
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
  };
  fetch(0);
  double z[R::kState];
#pragma unroll
  for (int i = 0; i < R::kState; ++i) z[i] = 0.0;
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
      double* mine = tile + lane * kIirStride;
      if (t0 == 0) R::start(z, tab, mine[0]);  // zi * ext[0] (forward), zi * y_last (backward)
#pragma unroll 4
      for (int k = 0; k < cnt; ++k) mine[k] = R::step(z, tab, mine[k]);
    }
    __syncthreads();
    if (lane < cnt) {
      const int64_t j = t0 + lane;
      for (int r = 0; r < rows; ++r) {
        const double y = tile[r * kIirStride + lane];
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

template <int FORM, int N>
int launch_passes(const IirArgs& a, const IirTables& tab, hipStream_t st) {
  const unsigned grid = (unsigned)ceil_div(a.C, kIirRows);
  k_iir<FORM, N, false><<<grid, kIirRows, 0, st>>>(a, tab);
  QI_LAUNCH_CHECK();
  k_iir<FORM, N, true><<<grid, kIirRows, 0, st>>>(a, tab);
  QI_LAUNCH_CHECK();
  return QI_OK;
}

template <int FORM>
int launch_order(int N, const IirArgs& a, const IirTables& tab, hipStream_t st) {
  switch (N) {
#define QI_IIR_CASE(K) \
  case K:              \
    return launch_passes<FORM, K>(a, tab, st);
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
  QI_REQUIRE(scratch_bytes >= need, "scratch of %lld bytes, %lld needed", (long long)scratch_bytes, (long long)need);
  QI_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 7) == 0 && (reinterpret_cast<uintptr_t>(out) & 7) == 0,
             "scratch and out must be aligned to 8 bytes");
  IirTables tab{};
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
  IirArgs a{};
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
  return form == QI_IIR_BA ? launch_order<QI_IIR_BA>(N, a, tab, (hipStream_t)stream)
                           : launch_order<QI_IIR_SOS>(N, a, tab, (hipStream_t)stream);
}

}  // extern "C"
