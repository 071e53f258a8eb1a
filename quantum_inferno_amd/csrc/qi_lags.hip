// Time delays between sensors (include/qi_lags.h): the generalized cross-correlation of every pair of records from the
// cross-spectral matrices, its lag window and the sub-sample peak, in ONE launch.
//
// A workgroup of 256 threads owns one (stack, pair).  It gathers the pair's nfft / 2 + 1 entries S_ij (and S_ii, S_jj where
// the weighting or the normalisation reads them), weights them in registers (in double, rounded once), and folds the
// Hermitian spectrum X[0 .. M], M = L / 2, into the M complex numbers Z'[k] = A[k] + i B[k], A[k] = X[k] + conj X[M - k],
// B[k] = (X[k] - conj X[M - k]) exp(+i pi k / M), whose unnormalised inverse M-point transform is R[2 m] + i R[2 m + 1] -- the
// packing of k_istft_fused (qi_stft_fused.hip).  The transform runs in place in LDS, decimation in frequency, in passes of
// radix 16 on the register butterflies of qi_fft_reg.hpp (the first pass takes the radix 2, 4 or 8 that log2 M leaves over):
// a thread loads its R points a block-stride apart, transforms them in registers, multiplies by W^(j d) and writes them
// back where they came from, so a pass needs one barrier and no second buffer; the result is left in digit-reversed order
// and read through lag_pos().  Twiddles: sincospi of the exact argument 2 j d / block in the element's precision (double
// for float64); a radix-16 pass takes one seed per thread and its powers by products (depth <= 4).
//
// LDS: M + M / 16 complex numbers (one element of padding per 16: the last pass's threads read 16 consecutive elements each,
// a stride of 17 between lanes), at most 4352 x 16 B = 68 KiB in float64 and 34 KiB in float32, and 3.3 KiB of reduction
// slots.  Then, from LDS: the window -max_lag .. +max_lag is scaled, rounded and stored, every thread keeps the first
// maximum of its lags, the workgroup folds them (greater value, then smaller lag), and one thread fits the parabola in
// double.  The correlation never reaches device memory beyond the window.
#include "qi_common.hpp"
#include "qi_device.hpp"
#include "qi_fft_reg.hpp"

namespace qi {

namespace {

constexpr int kLagThreads = 256;
constexpr int kLagWaves = kLagThreads / kWave;

struct LagArgs {
  int64_t C, nf, npair;
  int32_t nfft, M, log2m;  // M = L / 2 complex points
  int32_t bin_lo, bin_hi, weighting, halve, normalize, upsample, max_lag;
};

// element i of the transform's array in LDS: one element of padding per 16
__device__ __forceinline__ int lag_at(int i) { return i + (i >> 4); }

// where the decimation-in-frequency passes leave output e: e = d1 + r1 d2 + r1 r2 d3 ... sits at d1 M / r1 + d2 M / (r1 r2) ...
__device__ __forceinline__ int lag_pos(int e, int log2m) {
  int rem = log2m, p = 0;
  const int l1 = log2m & 3;
  if (l1) {
    rem -= l1;
    p += (e & ((1 << l1) - 1)) << rem;
    e >>= l1;
  }
  while (rem > 0) {
    rem -= 4;
    p += (e & 15) << rem;
    e >>= 4;
  }
  return p;
}

// One pass of radix R over blocks of 2^lg points: point j + t 2^lg / R of every block, t = 0 .. R - 1, in one thread;
// X[d + R k'] of a block is output k' of its sub-block d.  The last pass (blocks of R points) has no twiddles.
template <typename T, int R>
__device__ __forceinline__ void lag_pass(cplx<T>* __restrict__ data, int M, int lg) {
  constexpr int LR = native::ilog2(R);
  const int lq = lg - LR, span = 1 << lq;
  for (int q = threadIdx.x; q < (M >> LR); q += kLagThreads) {
    const int j = q & (span - 1), base = ((q >> lq) << lg) + j;
    cplx<T> v[R];
#pragma unroll
    for (int t = 0; t < R; ++t) v[t] = data[lag_at(base + (t << lq))];
    native::fft_reg<T, R, 1>(v);
    if (lq > 0) {
      const double unit = 2.0 / (double)(1 << lg);  // exp(+2 pi i j d / 2^lg) = sincospi(unit j d), the argument exact
      if constexpr (R == 16) {
        T s, c;
        native::sincospi_as<T>(unit * (double)j, &s, &c);
        native::mul_powers16<T>(v, mk<T>(c, s));
      } else {
#pragma unroll
        for (int d = 1; d < R; ++d) {
          T s, c;
          native::sincospi_as<T>(unit * (double)(j * d), &s, &c);
          v[native::brev(d, LR)] = cmul(v[native::brev(d, LR)], mk<T>(c, s));
        }
      }
    }
#pragma unroll
    for (int d = 0; d < R; ++d) data[lag_at(base + (d << lq))] = v[native::brev(d, LR)];
  }
  __syncthreads();
}

__device__ __forceinline__ bool lag_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }  // false for NaN

template <typename T>
__global__ void __launch_bounds__(kLagThreads) k_pair_lags(const cplx<T>* __restrict__ csd, T* __restrict__ cc, T* __restrict__ peak_lag,
                                                           T* __restrict__ peak_value, LagArgs a) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  __shared__ double s_sum[3][kLagWaves];
  __shared__ double s_best[kLagThreads];
  __shared__ int s_lag[kLagThreads];
  cplx<T>* __restrict__ data = reinterpret_cast<cplx<T>*>(lds_raw);
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid / kWave;
  const int M = a.M, L = 2 * M, half = a.nfft / 2;
  const int64_t stack = blockIdx.x / a.npair, pair = blockIdx.x % a.npair;
  // the pair's records: row i holds the C - 1 - i pairs (i, i + 1) .. (i, C - 1)
  int64_t i = 0, left = pair;
  while (left >= a.C - 1 - i) {
    left -= a.C - 1 - i;
    ++i;
  }
  const int64_t j = i + 1 + left;
  const cplx<T>* __restrict__ S = csd + (size_t)stack * a.nf * a.C * a.C;
  const bool autos = a.weighting == 2 || (a.normalize && a.weighting == 0);

  // ---- gather, weight, fold: thread = bin pair (k, M - k); every bin 0 .. M is formed once ----
  double sum_i = 0.0, sum_j = 0.0, count = 0.0;
  bool bad = false;
  auto bin = [&](int f) -> cplx<T> {
    if (f < a.bin_lo || f >= a.bin_hi) return mk<T>(T(0), T(0));  // (bin_hi <= nfft / 2 + 1: the zero padding too)
    const cplx<T>* __restrict__ m = S + (size_t)f * a.C * a.C;
    const cplx<T> sij = m[i * a.C + j];
    const double re = sij.x, im = sij.y;
    const double h = (a.halve && f > 0 && f < half) ? 0.5 : 1.0, mult = (f == 0 || f == M) ? 1.0 : 2.0;
    bad |= !lag_finite(re) || !lag_finite(im);
    double w = 1.0;
    if (autos) {
      const double aii = m[i * a.C + i].x, ajj = m[j * a.C + j].x;
      bad |= !lag_finite(aii) || !lag_finite(ajj);
      if (a.weighting == 2) {
        w = (aii == 0.0 || ajj == 0.0) ? 0.0 : 1.0 / (sqrt(aii) * sqrt(ajj));
      } else {
        sum_i += mult * (aii * h);
        sum_j += mult * (ajj * h);
      }
    }
    if (a.weighting == 1) {
      const double mag = hypot(re, im);
      w = mag == 0.0 ? 0.0 : 1.0 / mag;
    }
    if (a.weighting != 0 && w != 0.0) count += mult;
    const double xr = re * w * h, xi = im * w * h;
    bad |= !lag_finite(xr) || !lag_finite(xi);
    return mk<T>((T)xr, (T)xi);
  };
  for (int k = tid; k <= M / 2; k += kLagThreads) {
    const int kb = M - k;
    cplx<T> xa = bin(k), xb = kb == k ? xa : bin(kb);
    if (k == 0) {  // the imaginary parts of bins 0 and L / 2 are dropped
      xa.y = T(0);
      xb.y = T(0);
    }
    T s, c;
    native::sincospi_as<T>((double)k / (double)M, &s, &c);  // exp(+i pi k / M)
    const cplx<T> A = mk<T>(xa.x + xb.x, xa.y - xb.y), D = mk<T>(xa.x - xb.x, xa.y + xb.y);
    const cplx<T> B = mk<T>(D.x * c - D.y * s, D.x * s + D.y * c);
    data[lag_at(k)] = mk<T>(A.x - B.y, A.y + B.x);                             // A + i B
    if (k > 0 && kb != k) data[lag_at(kb)] = mk<T>(A.x + B.y, B.x - A.y);  // conj(A - i B)
  }
  // the normalisation's sums: wave sums in a fixed order, then the waves in index order
  const double w0 = wave_sum(sum_i), w1 = wave_sum(sum_j), w2 = wave_sum(count);
  if (lane == 0) {
    s_sum[0][wv] = w0;
    s_sum[1][wv] = w1;
    s_sum[2][wv] = w2;
  }
  const bool poisoned = __syncthreads_or(bad);
  const size_t out = (size_t)blockIdx.x;
  const int nwin = 2 * a.max_lag + 1;
  if (poisoned) {  // (uniform over the workgroup)
    const T nan = (T)__builtin_nan("");
    if (cc)
      for (int q = tid; q < nwin; q += kLagThreads) cc[out * nwin + q] = nan;
    if (tid == 0) {
      if (peak_lag) peak_lag[out] = nan;
      if (peak_value) peak_value[out] = nan;
    }
    return;
  }
  double tot[3];
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    tot[q] = 0.0;
#pragma unroll
    for (int w = 0; w < kLagWaves; ++w) tot[q] += s_sum[q][w];
  }
  double inv = 1.0 / (double)a.nfft;
  if (a.normalize) inv = 1.0 / (a.weighting == 0 ? sqrt(tot[0]) * sqrt(tot[1]) : tot[2]);

  // ---- the inverse transform of M points, in place ----
  int lg = a.log2m;
  switch (lg & 3) {
    case 1: lag_pass<T, 2>(data, M, lg); lg -= 1; break;
    case 2: lag_pass<T, 4>(data, M, lg); lg -= 2; break;
    case 3: lag_pass<T, 8>(data, M, lg); lg -= 3; break;
    default: break;
  }
  for (; lg > 0; lg -= 4) lag_pass<T, 16>(data, M, lg);

  // ---- the window, its first maximum, the parabola ----
  const T* __restrict__ flat = reinterpret_cast<const T*>(data);
  auto r_at = [&](int lag) -> T {  // r[lag mod L], scaled and rounded once
    const int l = lag & (L - 1);
    return (T)((double)flat[2 * lag_at(lag_pos(l >> 1, a.log2m)) + (l & 1)] * inv);
  };
  double best = 0.0;
  int best_q = -1;  // index into the window; a thread's lags ascend, so a strict comparison keeps its first maximum
  for (int q = tid; q < nwin; q += kLagThreads) {
    const T v = r_at(q - a.max_lag);
    if (cc) cc[out * nwin + q] = v;
    if (best_q < 0 || (double)v > best) {
      best = (double)v;
      best_q = q;
    }
  }
  if (!peak_lag && !peak_value) return;
  s_best[tid] = best;
  s_lag[tid] = best_q;
  __syncthreads();
  if (tid != 0) return;
  for (int t = 1; t < kLagThreads && t < nwin; ++t) {  // thread t's first lag is t: only the first nwin threads hold one
    const double v = s_best[t];
    const int q = s_lag[t];
    if (v > best || (v == best && q < best_q)) {
      best = v;
      best_q = q;
    }
  }
  const int l0 = best_q - a.max_lag;
  const double ya = (double)r_at(l0 - 1), yb = best, yc = (double)r_at(l0 + 1);
  // (every product and sum rounded on its own, in the header's order: no fused multiply-add -- the float64 result is
  // then the same bits as the formula evaluated in any IEEE double arithmetic)
  const double den = __dadd_rn(__dsub_rn(ya, __dmul_rn(2.0, yb)), yc), slope = __dsub_rn(ya, yc);
  const double delta = den == 0.0 ? 0.0 : __dmul_rn(0.5, slope) / den;
  if (peak_lag) peak_lag[out] = (T)(__dadd_rn((double)l0, delta) / (double)a.upsample);
  if (peak_value) peak_value[out] = (T)__dsub_rn(yb, __dmul_rn(__dmul_rn(0.25, slope), delta));
}

}  // namespace

// dynamic LDS of a workgroup: the M = L / 2 points and their padding
static size_t pair_lags_lds(int64_t L, size_t complex_bytes) { return (size_t)(L / 2 + L / 32 + 1) * complex_bytes; }

template <typename T>
int launch_pair_lags(const cplx<T>* csd, int64_t nstack, int64_t C, int64_t nfft, int64_t bin_lo, int64_t bin_hi, int weighting,
                     int halve_interior, int normalize, int64_t upsample, int64_t max_lag, T* cc, T* peak_lag, T* peak_value,
                     hipStream_t st) {
  LagArgs a{};
  a.C = C;
  a.nf = nfft / 2 + 1;
  a.npair = C * (C - 1) / 2;
  a.nfft = (int32_t)nfft;
  a.M = (int32_t)(nfft * upsample / 2);
  while ((1 << a.log2m) < a.M) ++a.log2m;
  a.bin_lo = (int32_t)bin_lo;
  a.bin_hi = (int32_t)bin_hi;
  a.weighting = weighting;
  a.halve = halve_interior != 0;
  a.normalize = normalize != 0;
  a.upsample = (int32_t)upsample;
  a.max_lag = (int32_t)max_lag;
  const size_t lds = pair_lags_lds(2 * (int64_t)a.M, sizeof(cplx<T>));
  const auto kernel = &k_pair_lags<T>;
  QI_TRY(allow_dynamic_lds(reinterpret_cast<const void*>(kernel), lds));
  kernel<<<dim3((unsigned)(nstack * a.npair)), kLagThreads, lds, st>>>(csd, cc, peak_lag, peak_value, a);
  QI_LAUNCH_CHECK();
  return QI_OK;
}
template int launch_pair_lags<float>(const float2*, int64_t, int64_t, int64_t, int64_t, int64_t, int, int, int, int64_t, int64_t, float*,
                                     float*, float*, hipStream_t);
template int launch_pair_lags<double>(const double2*, int64_t, int64_t, int64_t, int64_t, int64_t, int, int, int, int64_t, int64_t,
                                      double*, double*, double*, hipStream_t);

}  // namespace qi
