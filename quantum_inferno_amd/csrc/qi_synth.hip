// Synthetic records from closed formulas: the generators of synth/benchmark_signals.py, synth/synthetic_signals.py and
// synth/blast_gt_pulse.py (qi_synth), and the source / receiver geometry of synth/doppler.py:149-207 (qi_doppler), restated.
//
// qi_synth: a workgroup of kSyThreads lanes forms QI_SYNTH_TILE consecutive samples of one record; the grid is (tiles,
// records), one launch per 65535 records, no scratch, no atomics, no LDS.  Per sample k of record c:
//   1 the time  t = (base(k) - s0) - s1, base one of (double)k / rate, (double)k * step, x[k] (x shared or a row per record);
//   2 the kind's formula in float64 from the record's parameter row (QI_SYNTH_PARAMS values; one row shared by all records
//     or a row per record), in NumPy's order of operations -- the expressions are spelled out in include/qi_tfr.h;
//   3 the envelope: none, tukey(n, alpha)[k], or the gate of benchmark_signals.signal_gate (zero where t < tmin or
//     t > tmax, otherwise times tukey(m, alpha)[k - k0]);
//   4 one rounding to the stored type, real or interleaved complex; coalesced stores.
// A lane's samples lie kSyThreads apart, so a store instruction of a wave writes consecutive addresses.
//
// qi_doppler: the same grid and time axis; per sample the receiver (forward) or source (inverse) time, the range and
// omega / omega_c of doppler._get_final_vals, three float64 stores.
//
// The file is compiled with -ffp-contract=off (_build.py: PER_FILE_FLAGS): every product, sum, quotient and square root is
// an IEEE double operation rounded on its own, so the argument of every sin, cos, exp and log has NumPy's bits and
// everything without a library function is NumPy's result bit for bit.  The one fused operation is written out by hand:
// cube() forms the correctly rounded tau^3 that np.power gives.
#include "qi_host.hpp"
#include "qi_device.hpp"   // kWave
#include "qi_fft_reg.hpp"  // QI_LAUNCH_CHECK

namespace qi {

namespace {

constexpr int kSyTile = QI_SYNTH_TILE;
constexpr int kSyThreads = 256;
constexpr int kSyVec = kSyTile / kSyThreads;  // samples per lane
static_assert(kSyTile % kSyThreads == 0 && kSyThreads % kWave == 0, "whole rows of lanes");
constexpr int kSyP = QI_SYNTH_PARAMS;
constexpr int kDpP = QI_DOPPLER_PARAMS;
constexpr int64_t kSyMaxRecords = 65535;  // grid.y

// float64 constants as NumPy forms them on the host (np.pi, 2 * np.pi, np.sqrt(6.0) and what blast_gt_pulse.py builds of it)
constexpr double kPi = 0x1.921fb54442d18p+1;
constexpr double k2Pi = 0x1.921fb54442d18p+2;
constexpr double kGtA = 0x1.b988e1409212ep+1;    // 1 + sqrt(6)
constexpr double kGtB3 = 0x1.5cc470a049097p+2;   // 3 + sqrt(6)
constexpr double kGtI2 = 0x1.f988e1409212ep+4;   // 4 (3 + 2 sqrt(6))
constexpr double kGtI1 = 0x1.c326a8f06d8e2p+6;   // 6 (9 + 4 sqrt(6))
constexpr double kGtI0 = 0x1.1d93547836c71p+7;   // 12 (7 + 2 sqrt(6))
constexpr double kGtH1 = 0x1.a20bd700c2c3dp-2;   // (a - 1) / 6
constexpr double kGtH2 = 0x1.485cfeb4522aap+5;   // a (2 a + 5)
constexpr double kGtH3 = 0x1.6b26a8f06d8e2p+3;   // 1 + 3 a
constexpr double kSixth = 0x1.5555555555555p-3;  // 1.0 / 6.0
constexpr double kEps = 0x1.0p-52;               // scales_dyadic.get_epsilon()

struct AxisArgs {
  const double* x;  // nullptr, [n] or [C][n]
  int64_t x_stride;
  int axis;
  double value, s0, s1;  // value: the rate or the step
};

struct SynthArgs {
  AxisArgs ax;
  const double* params;  // [QI_SYNTH_PARAMS] or [C][QI_SYNTH_PARAMS]
  int64_t param_stride;
  void* out;  // [C][n] or [C][n][2] in the stored type
  int64_t n;
  int envelope, cplx;
  double alpha, tmin, tmax;
  int64_t k0, m;
};

struct DopplerArgs {
  AxisArgs ax;
  const double* params;  // [QI_DOPPLER_PARAMS] or [C][QI_DOPPLER_PARAMS]
  int64_t param_stride;
  double *time, *range, *omega;  // [C][n] each
  int64_t n;
  int inverse;
};

__device__ __forceinline__ double axis_time(const AxisArgs& a, const double* __restrict__ x, int64_t k) {
  double b;
  if (a.axis == QI_AXIS_RATE) b = (double)k / a.value;
  else if (a.axis == QI_AXIS_STEP) b = (double)k * a.value;
  else b = x[k];
  return (b - a.s0) - a.s1;
}

// scipy.signal.windows.tukey(m, alpha)[j], sym=True
__device__ __forceinline__ double tukey_at(int64_t m, double alpha, int64_t j) {
  if (m == 1 || alpha <= 0.0) return 1.0;
  const double m1 = (double)(m - 1);
  if (alpha >= 1.0) {  // hann -> general_cosine([0.5, 0.5]) over np.linspace(-pi, pi, m)
    const double step = k2Pi / m1;
    const double fac = j == m - 1 ? kPi : (double)j * step + (-kPi);
    return (0.0 + 0.5 * cos(0.0 * fac)) + 0.5 * cos(fac);
  }
  const int64_t width = (int64_t)floor(alpha * m1 / 2.0);
  if (j <= width) return 0.5 * (1.0 + cos(kPi * (-1.0 + 2.0 * (double)j / alpha / m1)));
  if (j >= m - width - 1) return 0.5 * (1.0 + cos(kPi * ((-2.0 / alpha + 1.0) + 2.0 * (double)j / alpha / m1)));
  return 1.0;
}

// the correctly rounded x^3, as np.power(x, 3) gives it: x * x and (x * x) * x without error (two fused products each),
// then one rounding of the sum of the parts
__device__ __forceinline__ double cube(double x) {
  const double h = x * x, l = fma(x, x, -h);
  const double ph = h * x, pl = fma(h, x, -ph);
  return ph + (pl + l * x);
}

// benchmark_signals.signal_gate with fraction_cosine 0: the sample where tmin <= t <= tmax, +0.0 outside
__device__ __forceinline__ double gate0(double v, double t, double tmin, double tmax) {
  return (t < tmin || t > tmax) ? 0.0 : v;
}

template <int KIND>
__device__ __forceinline__ void sample(const double* __restrict__ p, double t, double& re, double& im) {
  im = 0.0;
  if constexpr (KIND == QI_SYNTH_TONE) {
    re = cos(p[0] * t);
  } else if constexpr (KIND == QI_SYNTH_SINES3) {
    const double a = gate0(sin(p[0] * t), t, p[3], p[4]);
    const double b = gate0(sin(p[1] * t), t, p[5], p[6]);
    const double c = gate0(sin(p[2] * t), t, p[7], p[8]);
    re = (a + b) + c;
  } else if constexpr (KIND == QI_SYNTH_01) {
    re = cos(p[0] * t - p[1] * t * t) + cos(p[3] * sin(p[2] * t) + p[4] * t);
  } else if constexpr (KIND == QI_SYNTH_02) {
    double acc = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const double d = t - p[3 * q + 1];
      const double pulse = exp(p[3 * q] * (d * d)) * cos(p[3 * q + 2] * t);
      acc = q == 0 ? pulse : acc + pulse;
    }
    re = acc;
  } else if constexpr (KIND == QI_SYNTH_03) {
    re = cos(p[0] * log(p[1] * t + 1.0)) + cos(p[2] * t + p[3] * (t * t));
  } else if constexpr (KIND == QI_SYNTH_QCHIRP) {
    const double q = t / p[2];
    const double phase = p[0] * t + p[1] * (q * q);
    const double amp = p[3] != 0.0 ? exp(-0.5 * (q * q)) : 1.0;
    re = amp * cos(phase);
    im = amp * sin(phase);
  } else if constexpr (KIND == QI_SYNTH_CHIRP_LINEAR) {
    re = cos(k2Pi * (p[0] * t + p[1] * t * t) + 0.0);
  } else if constexpr (KIND == QI_SYNTH_SAWTOOTH) {
    double tm = fmod(p[0] * t, k2Pi);  // np.mod: the remainder takes the divisor's sign
    if (tm != 0.0) {
      if (tm < 0.0) tm += k2Pi;
    } else {
      tm = 0.0;
    }
    re = (kPi - tm) / kPi;
  } else {
    const double tau = t / p[0] + 1.0;
    const bool one = 0.0 <= tau && tau <= 1.0, two = 1.0 < tau && tau <= kGtA;
    re = 0.0;
    if constexpr (KIND == QI_SYNTH_GT) {
      if (one) re = 1.0 - tau;
      if (two) re = kSixth * (1.0 - tau) * ((kGtA - tau) * (kGtA - tau));
    } else if constexpr (KIND == QI_SYNTH_GT_DERIVATIVE) {
      if (one) re = -1.0;
      if (two) re = -kSixth * (kGtB3 - 3.0 * tau) * (kGtA - tau);
    } else if constexpr (KIND == QI_SYNTH_GT_INTEGRAL) {
      if (one) re = (1.0 - tau / 2.0) * tau;
      if (two) re = -tau / 72.0 * (((3.0 * cube(tau) - kGtI2 * (tau * tau)) + kGtI1 * tau) - kGtI0) + p[1];
    } else {  // QI_SYNTH_GT_HILBERT
      if (one) {
        const double u = 1.0 - tau;
        re = (1.0 + u * log(tau + kEps)) - u * log(u + kEps);
      }
      if (two) {
        const double h21 = kGtH1 * (((kGtH2 - 1.0) + 6.0 * (tau * tau)) - 3.0 * tau * kGtH3);
        const double d = kGtA - tau;
        const double h22 = (tau - 1.0) * (d * d) * (log(d + kEps) - log((tau - 1.0) + kEps));
        re = kSixth * (h21 + h22);
      }
      re = re / kPi;
    }
  }
}

template <typename T, int KIND>
__global__ void __launch_bounds__(kSyThreads) k_synth(SynthArgs a) {
  const int64_t c = blockIdx.y, n = a.n;
  const double* __restrict__ x = a.ax.x ? a.ax.x + c * a.ax.x_stride : nullptr;
  double p[kSyP];
#pragma unroll
  for (int q = 0; q < kSyP; ++q) p[q] = a.params[c * a.param_stride + q];
  T* __restrict__ out = static_cast<T*>(a.out) + c * n * (a.cplx ? 2 : 1);
#pragma unroll
  for (int u = 0; u < kSyVec; ++u) {
    const int64_t k = (int64_t)blockIdx.x * kSyTile + u * kSyThreads + threadIdx.x;
    if (k >= n) continue;
    const double t = axis_time(a.ax, x, k);
    double re, im;
    sample<KIND>(p, t, re, im);
    if (a.envelope == QI_ENVELOPE_TUKEY) {
      const double w = tukey_at(n, a.alpha, k);
      re *= w;
      im *= w;
    } else if (a.envelope == QI_ENVELOPE_GATE) {
      if (t < a.tmin || t > a.tmax) {
        re = 0.0;
        im = 0.0;
      } else if (t >= a.tmin && t <= a.tmax) {  // (a NaN time is neither outside nor inside, as in NumPy)
        int64_t j = k - a.k0;  // in [0, m) when the host counted with the same t(k); held there whatever it passed
        j = j < 0 ? 0 : (j >= a.m ? a.m - 1 : j);
        const double w = tukey_at(a.m, a.alpha, j);
        re *= w;
        im *= w;
      }
    }
    if (a.cplx) {
      out[2 * k] = (T)re;
      out[2 * k + 1] = (T)im;
    } else {
      out[k] = (T)re;
    }
  }
}

// the sum of three products as np.sum adds a row of three
__device__ __forceinline__ double dot3(double a0, double a1, double a2, double b0, double b1, double b2) {
  return (a0 * b0 + a1 * b1) + a2 * b2;
}

__global__ void __launch_bounds__(kSyThreads) k_doppler(DopplerArgs a) {
  const int64_t c = blockIdx.y, n = a.n;
  const double* __restrict__ x = a.ax.x ? a.ax.x + c * a.ax.x_stride : nullptr;
  const double* __restrict__ p = a.params + c * a.param_stride;
  const double cs = p[0], c2 = p[1], denom = p[2];
  const double s0 = p[3], s1 = p[4], s2 = p[5];     // source velocity
  const double v0 = p[6], v1 = p[7], v2 = p[8];     // receiver velocity
  const double r0 = p[9], r1 = p[10], r2 = p[11];   // initial range, source to receiver
#pragma unroll
  for (int u = 0; u < kSyVec; ++u) {
    const int64_t k = (int64_t)blockIdx.x * kSyTile + u * kSyThreads + threadIdx.x;
    if (k >= n) continue;
    const double t = axis_time(a.ax, x, k);
    double q0, q1, q2, term1;
    if (a.inverse) {
      q0 = r0 + v0 * t, q1 = r1 + v1 * t, q2 = r2 + v2 * t;
      term1 = c2 * t - dot3(s0, s1, s2, q0, q1, q2);
    } else {
      q0 = r0 - s0 * t, q1 = r1 - s1 * t, q2 = r2 - s2 * t;
      term1 = c2 * t + dot3(v0, v1, v2, q0, q1, q2);
    }
    term1 = term1 * denom;
    const double rm = sqrt(dot3(q0, q1, q2, q0, q1, q2));
    const double tc = t * cs;
    const double term2 = (rm * rm - tc * tc) * denom;
    const double root = sqrt(term1 * term1 + term2);
    double ts, g0, g1, g2;
    if (a.inverse) {
      ts = term1 - root;
      g0 = q0 - s0 * ts, g1 = q1 - s1 * ts, g2 = q2 - s2 * ts;
    } else {
      ts = term1 + root;
      g0 = q0 + v0 * ts, g1 = q1 + v1 * ts, g2 = q2 + v2 * ts;
    }
    const double rt = sqrt(dot3(g0, g1, g2, g0, g1, g2));
    const double om = (cs - dot3(g0, g1, g2, v0, v1, v2) / rt) / (cs - dot3(g0, g1, g2, s0, s1, s2) / rt);
    a.time[c * n + k] = ts;
    a.range[c * n + k] = rt;
    a.omega[c * n + k] = om;
  }
}

template <typename T>
int launch_synth(int kind, const SynthArgs& a, dim3 grid, hipStream_t st) {
  switch (kind) {
#define QI_SYNTH_CASE(K) \
  case K: k_synth<T, K><<<grid, kSyThreads, 0, st>>>(a); break;
    QI_SYNTH_CASE(QI_SYNTH_TONE)
    QI_SYNTH_CASE(QI_SYNTH_SINES3)
    QI_SYNTH_CASE(QI_SYNTH_01)
    QI_SYNTH_CASE(QI_SYNTH_02)
    QI_SYNTH_CASE(QI_SYNTH_03)
    QI_SYNTH_CASE(QI_SYNTH_QCHIRP)
    QI_SYNTH_CASE(QI_SYNTH_CHIRP_LINEAR)
    QI_SYNTH_CASE(QI_SYNTH_SAWTOOTH)
    QI_SYNTH_CASE(QI_SYNTH_GT)
    QI_SYNTH_CASE(QI_SYNTH_GT_HILBERT)
    QI_SYNTH_CASE(QI_SYNTH_GT_DERIVATIVE)
    QI_SYNTH_CASE(QI_SYNTH_GT_INTEGRAL)
#undef QI_SYNTH_CASE
  }
  QI_LAUNCH_CHECK();
  return QI_OK;
}

// the checks the two entry points share: records, the parameter rows and the time axis
int require_rows(int dtype, int64_t n_channels, int64_t n, const char* stride_name, int64_t param_stride, int64_t width, int axis,
                 double axis_value, const void* x, int64_t x_stride) {
  QI_TRY(require_records(dtype, n_channels, n, 0));
  QI_REQUIRE(param_stride == 0 || param_stride == width, "%s must be 0 (one row for all records) or %lld, got %lld", stride_name,
             (long long)width, (long long)param_stride);
  QI_REQUIRE(axis == QI_AXIS_RATE || axis == QI_AXIS_STEP || axis == QI_AXIS_TIMESTAMPS, "bad axis %d", axis);
  QI_TRY(require_timestamp_stride("x_stride", x_stride, n));
  QI_REQUIRE(axis == QI_AXIS_TIMESTAMPS ? x != nullptr : (x == nullptr && x_stride == 0),
             "x and x_stride go with the timestamp axis: x must be given there, and must be null with x_stride 0 otherwise");
  QI_REQUIRE(axis != QI_AXIS_RATE || axis_value != 0.0, "the rate must not be 0");
  QI_REQUIRE(n < (1ll << 40) && n_channels < (1ll << 31), "request too large");
  return QI_OK;
}

}  // namespace

}  // namespace qi

using namespace qi;

extern "C" {

int qi_synth(int dtype, int device, int kind, int complex_out, const double* params, int64_t param_stride, int axis,
             double axis_value, const double* x, int64_t x_stride, double s0, double s1, int envelope, double alpha, double tmin,
             double tmax, int64_t k0, int64_t m, int64_t n_channels, int64_t n, void* out, qi_stream stream) {
  QI_TRY(require_rows(dtype, n_channels, n, "param_stride", param_stride, kSyP, axis, axis_value, x, x_stride));
  QI_REQUIRE(kind >= 0 && kind < QI_SYNTH_KINDS, "bad kind %d", kind);
  QI_REQUIRE(complex_out == 0 || complex_out == 1, "complex_out must be 0 or 1, got %d", complex_out);
  QI_REQUIRE(envelope == QI_ENVELOPE_NONE || envelope == QI_ENVELOPE_TUKEY || envelope == QI_ENVELOPE_GATE, "bad envelope %d",
             envelope);
  QI_REQUIRE(envelope != QI_ENVELOPE_GATE || (k0 >= 0 && m >= 0 && k0 <= n && m <= n - k0),
             "the gate's samples k0 %lld .. k0 + m, m %lld, must lie in the record", (long long)k0, (long long)m);
  if (n_channels == 0) return QI_OK;
  QI_REQUIRE(params && out, "null argument");
  QI_REQUIRE(aligned(params, 8) && aligned(x, 8) && aligned(out, elem_size(dtype)),
             "params, x and out must be aligned to their element size");
  DeviceGuard g(device);
  QI_REQUIRE(g.ok, "cannot select device %d", device);
  const size_t row_bytes = (size_t)n * elem_size(dtype) * (complex_out ? 2 : 1);
  for (int64_t c0 = 0; c0 < n_channels; c0 += kSyMaxRecords) {  // (one launch up to 65535 records: the grid's second extent)
    const int64_t cn = n_channels - c0 < kSyMaxRecords ? n_channels - c0 : kSyMaxRecords;
    SynthArgs a{};
    a.ax = AxisArgs{x ? x + c0 * x_stride : nullptr, x_stride, axis, axis_value, s0, s1};
    a.params = params + c0 * param_stride;
    a.param_stride = param_stride;
    a.out = static_cast<char*>(out) + (size_t)c0 * row_bytes;
    a.n = n;
    a.envelope = envelope;
    a.cplx = complex_out;
    a.alpha = alpha;
    a.tmin = tmin;
    a.tmax = tmax;
    a.k0 = k0;
    a.m = m > 0 ? m : 1;  // (an empty gate multiplies nothing)
    const dim3 grid((unsigned)ceil_div(n, kSyTile), (unsigned)cn);
    QI_TRY(by_dtype(dtype, [&](auto t) -> int { return launch_synth<decltype(t)>(kind, a, grid, (hipStream_t)stream); }));
  }
  return QI_OK;
}

int qi_doppler(int device, int inverse, const double* params, int64_t param_stride, int axis, double axis_value, const double* x,
               int64_t x_stride, double s0, double s1, int64_t n_channels, int64_t n, double* time_out, double* range_out,
               double* omega_out, qi_stream stream) {
  QI_TRY(require_rows(QI_F64, n_channels, n, "param_stride", param_stride, kDpP, axis, axis_value, x, x_stride));
  QI_REQUIRE(inverse == 0 || inverse == 1, "inverse must be 0 or 1, got %d", inverse);
  if (n_channels == 0) return QI_OK;
  QI_REQUIRE(params && time_out && range_out && omega_out, "null argument");
  QI_REQUIRE(aligned(params, 8) && aligned(x, 8) && aligned(time_out, 8) && aligned(range_out, 8) && aligned(omega_out, 8),
             "params, x and the outputs must be aligned to 8 bytes");
  DeviceGuard g(device);
  QI_REQUIRE(g.ok, "cannot select device %d", device);
  for (int64_t c0 = 0; c0 < n_channels; c0 += kSyMaxRecords) {
    const int64_t cn = n_channels - c0 < kSyMaxRecords ? n_channels - c0 : kSyMaxRecords;
    DopplerArgs a{};
    a.ax = AxisArgs{x ? x + c0 * x_stride : nullptr, x_stride, axis, axis_value, s0, s1};
    a.params = params + c0 * param_stride;
    a.param_stride = param_stride;
    a.time = time_out + c0 * n;
    a.range = range_out + c0 * n;
    a.omega = omega_out + c0 * n;
    a.n = n;
    a.inverse = inverse;
    const dim3 grid((unsigned)ceil_div(n, kSyTile), (unsigned)cn);
    k_doppler<<<grid, kSyThreads, 0, (hipStream_t)stream>>>(a);
    QI_LAUNCH_CHECK();
  }
  return QI_OK;
}

}  // extern "C"
