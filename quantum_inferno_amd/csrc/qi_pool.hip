// Pooling of a device panel along time: utilities.sampling.subsample_2d / subsample (sampling.py:14-50,87-120) on
// [rows][n] -> [rows][columns], every n-th column or the average / max / min / median of each window of `factor` columns.
// One launch per call; lanes are adjacent in time.  Three window regimes:
//   factor <= 64      k_pool_seg: a wave loads 64 x 16 bytes of the row (whole windows only), every lane folds its own
//                     elements, and a segmented scan by shuffles finishes the windows inside the wave
//   factor <= 1024    k_pool_win<false>: one wave per window, lane-strided 16-byte loads, wave reduction
//   larger            k_pool_win<true>: one workgroup per window, wave reduction, then the waves in index order
// The median sorts its windows in LDS (k_pool_median, factor <= 4096); "nth" is a gather (k_pool_nth).
// Averages accumulate in float64 in a fixed order (no atomics) and are rounded once; max / min / median / nth return
// input values.  The power of a complex panel is formed as the engines' epilogues form it (qi_device.hpp: norm2, mul_rn).
#include <type_traits>

#include "qi_host.hpp"
#include "qi_device.hpp"
#include "qi_fft_reg.hpp"  // QI_LAUNCH_CHECK

namespace qi {

namespace {

constexpr int kPoolThreads = 256;
constexpr int kPoolWaves = kPoolThreads / kWave;
constexpr int kPoolSegMax = kWave;      // windows up to here are finished inside a wave by the segmented scan
constexpr int kPoolWaveMax = 1024;      // ... up to here by one wave each, longer ones by a workgroup each
constexpr int kPoolMedianMax = 4096;    // elements of the LDS sort
constexpr int64_t kPoolGridMax = 8192;  // workgroups of a launch (the kernels stride over their work)

enum { kOpSum = 0, kOpMax = 1, kOpMin = 2 };

struct D2 {
  double x, y;
};

template <typename T, int KIND>
struct PoolIn {
  using type = cplx<T>;
};
template <typename T>
struct PoolIn<T, QI_POOL_REAL> {
  using type = T;
};

// the value that is pooled: the element itself, or the scaled power of a complex one
__device__ __forceinline__ float pool_value(float v, float) { return v; }
__device__ __forceinline__ double pool_value(double v, double) { return v; }
__device__ __forceinline__ float pool_value(float2 z, float scale) { return mul_rn(scale, norm2(z.x, z.y)); }
__device__ __forceinline__ double pool_value(double2 z, double scale) { return mul_rn(scale, norm2(z.x, z.y)); }

// What a window is folded with.  zero() is the identity that ragged tails feed (the wave reductions of qi_device.hpp need
// every lane), join() is applied in a fixed order, all() leaves the wave's result in every lane.
template <typename T, int KIND, int OP>
struct Red {  // kOpSum of real values or powers
  using In = typename PoolIn<T, KIND>::type;
  using Acc = double;
  using Out = T;
  static __device__ __forceinline__ Acc zero() { return 0.0; }
  static __device__ __forceinline__ Acc lift(In v, T scale) { return (double)pool_value(v, scale); }
  static __device__ __forceinline__ Acc join(Acc a, Acc b) { return a + b; }
  static __device__ __forceinline__ Acc up(Acc a, int d) { return __shfl_up(a, d, kWave); }
  static __device__ __forceinline__ Acc all(Acc a) { return wave_sum(a); }
  static __device__ __forceinline__ Out done(Acc a, int64_t f) { return (T)(a / (double)f); }
};
template <typename T>
struct Red<T, QI_POOL_COMPLEX, kOpSum> {
  using In = cplx<T>;
  using Acc = D2;
  using Out = cplx<T>;
  static __device__ __forceinline__ Acc zero() { return D2{0.0, 0.0}; }
  static __device__ __forceinline__ Acc lift(In v, T) { return D2{(double)v.x, (double)v.y}; }
  static __device__ __forceinline__ Acc join(Acc a, Acc b) { return D2{a.x + b.x, a.y + b.y}; }
  static __device__ __forceinline__ Acc up(Acc a, int d) { return D2{__shfl_up(a.x, d, kWave), __shfl_up(a.y, d, kWave)}; }
  static __device__ __forceinline__ Acc all(Acc a) { return D2{wave_sum(a.x), wave_sum(a.y)}; }
  static __device__ __forceinline__ Out done(Acc a, int64_t f) { return mk<T>((T)(a.x / (double)f), (T)(a.y / (double)f)); }
};
template <typename T, int KIND, bool NEG>
struct RedMax {  // the minimum is the maximum of the negated values, negated back (exact)
  using In = typename PoolIn<T, KIND>::type;
  using Acc = T;
  using Out = T;
  static __device__ __forceinline__ Acc zero() { return -(T)__builtin_huge_val(); }
  static __device__ __forceinline__ Acc lift(In v, T scale) { return NEG ? -pool_value(v, scale) : pool_value(v, scale); }
  static __device__ __forceinline__ Acc join(Acc a, Acc b) { return b > a ? b : a; }
  static __device__ __forceinline__ Acc up(Acc a, int d) { return __shfl_up(a, d, kWave); }
  static __device__ __forceinline__ Acc all(Acc a) { return wave_max(a); }
  static __device__ __forceinline__ Out done(Acc a, int64_t) { return NEG ? -a : a; }
};
template <typename T, int KIND>
struct Red<T, KIND, kOpMax> : RedMax<T, KIND, false> {};
template <typename T, int KIND>
struct Red<T, KIND, kOpMin> : RedMax<T, KIND, true> {};

// V consecutive elements in one load of V * sizeof(E) bytes
template <typename E, int V>
struct alignas(V * sizeof(E)) PoolVec {
  E e[V];
};

// ---- windows of up to 64 columns ------------------------------------------------------------------------------------
// A wave pass covers k = 64 V / f whole windows of one row; lane l holds the positions V l .. V l + V - 1 of the pass
// (one 16-byte load where the pass starts on a 16-byte boundary, element loads where it does not -- with n odd that is
// every other pass at best).  f >= V, so a lane's elements lie in at most two windows: x folds those of the window h of
// its first element, y those of window h + 1, and y moves one lane up.  The lanes whose first element lies in window h
// are consecutive, so an inclusive scan over lanes that stops at the first of them (o = lanes back to it) leaves the
// window's result in the last of them.  Every lane runs every shuffle; positions outside the pass hold the identity.
template <typename T, int KIND, int OP, int V>
__global__ void __launch_bounds__(kPoolThreads) k_pool_seg(const typename PoolIn<T, KIND>::type* __restrict__ in,
                                                           int64_t rows, int64_t n, int f, int64_t cols, T scale,
                                                           typename Red<T, KIND, OP>::Out* __restrict__ out) {
  using R = Red<T, KIND, OP>;
  using In = typename R::In;
  using Acc = typename R::Acc;
  using Vec = PoolVec<In, V>;
  const int lane = threadIdx.x & (kWave - 1);
  const int k = (kWave * V) / f;
  const int64_t chunks = (cols + k - 1) / k;  // passes per row
  const int64_t total = rows * chunks;
  const int64_t nwave = (int64_t)gridDim.x * kPoolWaves;
  const int p0 = V * lane;
  const int h = p0 / f;
  const int o = lane - (h * f + V - 1) / V;
  const bool last = V * (lane + 1) >= (h + 1) * f;
  const int reach = (f + V - 1) / V + 1;  // lanes that can share a window
  for (int64_t c = (int64_t)blockIdx.x * kPoolWaves + threadIdx.x / kWave; c < total; c += nwave) {  // (wave-uniform)
    const int64_t row = c / chunks, w0 = (c - row * chunks) * k;
    const int kk = (int)(cols - w0 < k ? cols - w0 : k);
    const int span = kk * f;  // positions of this pass; w0 f + span <= cols f <= n
    const In* src = in + row * n + w0 * f;
    In e[V] = {};
    if ((reinterpret_cast<uintptr_t>(src) & (sizeof(Vec) - 1)) == 0 && p0 + V <= span) {
      const Vec v = *reinterpret_cast<const Vec*>(src + p0);
#pragma unroll
      for (int i = 0; i < V; ++i) e[i] = v.e[i];
    } else {
#pragma unroll
      for (int i = 0; i < V; ++i)
        if (p0 + i < span) e[i] = src[p0 + i];
    }
    Acc x = R::zero(), y = R::zero();
#pragma unroll
    for (int i = 0; i < V; ++i) {
      if (p0 + i < span) {
        const Acc a = R::lift(e[i], scale);
        if (p0 + i < (h + 1) * f)
          x = R::join(x, a);
        else
          y = R::join(y, a);
      }
    }
    Acc t = R::up(y, 1);
    Acc z = lane > 0 ? R::join(t, x) : x;
    for (int d = 1; d < reach; d <<= 1) {
      t = R::up(z, d);
      if (o >= d) z = R::join(t, z);
    }
    if (last && h < kk) out[row * cols + w0 + h] = R::done(z, f);
  }
}

// ---- longer windows -------------------------------------------------------------------------------------------------
// One wave (BLOCK: one workgroup) per window: the elements before the first 16-byte boundary by the first lanes, 16-byte
// loads strided over the lanes, the elements behind the last whole vector by the first lanes again; then the wave
// reduction, and for a workgroup the waves' results in index order.
template <typename T, int KIND, int OP, bool BLOCK>
__global__ void __launch_bounds__(kPoolThreads) k_pool_win(const typename PoolIn<T, KIND>::type* __restrict__ in,
                                                           int64_t rows, int64_t n, int64_t f, int64_t cols, T scale,
                                                           typename Red<T, KIND, OP>::Out* __restrict__ out) {
  using R = Red<T, KIND, OP>;
  using In = typename R::In;
  using Acc = typename R::Acc;
  constexpr int V = 16 / (int)sizeof(In);
  using Vec = PoolVec<In, V>;
  __shared__ Acc s[kPoolWaves];
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
  const int nt = BLOCK ? kPoolThreads : kWave;
  const int t = BLOCK ? (int)threadIdx.x : lane;
  const int64_t total = rows * cols;
  const int64_t step = BLOCK ? (int64_t)gridDim.x : (int64_t)gridDim.x * kPoolWaves;
  for (int64_t w = BLOCK ? (int64_t)blockIdx.x : (int64_t)blockIdx.x * kPoolWaves + wv; w < total; w += step) {
    const int64_t row = w / cols, j = w - row * cols;
    const In* src = in + row * n + j * f;  // j f + f <= cols f <= n
    int64_t hd = (int64_t)(((16 - (reinterpret_cast<uintptr_t>(src) & 15)) & 15) / sizeof(In));
    if (hd > f) hd = f;
    const int64_t nv = (f - hd) / V, tl = hd + nv * V;
    Acc a = R::zero();
    if (t < hd) a = R::join(a, R::lift(src[t], scale));
    const Vec* vp = reinterpret_cast<const Vec*>(src + hd);
    for (int64_t i = t; i < nv; i += nt) {
      const Vec v = vp[i];
#pragma unroll
      for (int q = 0; q < V; ++q) a = R::join(a, R::lift(v.e[q], scale));
    }
    if (tl + t < f) a = R::join(a, R::lift(src[tl + t], scale));
    a = R::all(a);  // (the loop is uniform over the wave: every lane is here)
    if (BLOCK) {
      if (lane == 0) s[wv] = a;
      __syncthreads();
      if (threadIdx.x == 0) {
        Acc r = s[0];
        for (int q = 1; q < kPoolWaves; ++q) r = R::join(r, s[q]);
        out[w] = R::done(r, f);
      }
      __syncthreads();
    } else if (lane == 0) {
      out[w] = R::done(a, f);
    }
  }
}

// ---- median ---------------------------------------------------------------------------------------------------------
// A workgroup pass takes 4096 / P windows of one row (P: the power of two >= f), each padded to P with +inf, sorts every
// window ascending in LDS (one bitonic network over all of them: the direction comes from the index inside the window)
// and picks the middle.  The loads run along the row; the sort, not the load, is what this kernel spends its time on.
template <typename T, int KIND>
__global__ void __launch_bounds__(kPoolThreads) k_pool_median(const typename PoolIn<T, KIND>::type* __restrict__ in,
                                                              int64_t rows, int64_t n, int f, int lg, int64_t cols, T scale,
                                                              T* __restrict__ out) {
  __shared__ T s[kPoolMedianMax];
  const int P = 1 << lg, per = kPoolMedianMax >> lg;
  const int tid = threadIdx.x;
  const int64_t groups = (cols + per - 1) / per;
  const int64_t total = rows * groups;
  for (int64_t g = blockIdx.x; g < total; g += gridDim.x) {
    const int64_t row = g / groups, w0 = (g - row * groups) * per;
    const int kk = (int)(cols - w0 < per ? cols - w0 : per);
    const int m = kk << lg;  // elements to sort
    const auto* src = in + row * n + w0 * f;
    for (int q = tid; q < m; q += kPoolThreads) {
      const int wi = q >> lg, off = q & (P - 1);
      s[q] = off < f ? pool_value(src[(int64_t)wi * f + off], scale) : (T)__builtin_huge_val();
    }
    __syncthreads();
    for (int k2 = 2; k2 <= P; k2 <<= 1) {
      for (int j = k2 >> 1; j > 0; j >>= 1) {
        for (int q = tid; q < (m >> 1); q += kPoolThreads) {
          const int i = ((q & ~(j - 1)) << 1) | (q & (j - 1));
          const bool asc = ((i & (P - 1)) & k2) == 0;
          const T a = s[i], b = s[i | j];
          if ((a > b) == asc) {
            s[i] = b;
            s[i | j] = a;
          }
        }
        __syncthreads();
      }
    }
    for (int wi = tid; wi < kk; wi += kPoolThreads) {
      const T* sw = s + ((int64_t)wi << lg);
      out[row * cols + w0 + wi] = (f & 1) ? sw[f >> 1] : (sw[(f >> 1) - 1] + sw[f >> 1]) / (T)2;
    }
    __syncthreads();
  }
}

// ---- every n-th column ----------------------------------------------------------------------------------------------
template <typename Out, typename In, typename T>
struct NthPick {  // complex in, real out: the power
  static __device__ __forceinline__ Out get(In v, T scale) { return pool_value(v, scale); }
};
template <typename In, typename T>
struct NthPick<In, In, T> {
  static __device__ __forceinline__ In get(In v, T) { return v; }
};
template <typename In, typename Out, typename T>
__global__ void __launch_bounds__(kPoolThreads) k_pool_nth(const In* __restrict__ in, int64_t rows, int64_t n, int64_t f,
                                                           int64_t cols, T scale, Out* __restrict__ out) {
  const int64_t total = rows * cols;
  for (int64_t i = (int64_t)blockIdx.x * kPoolThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kPoolThreads) {
    const int64_t row = i / cols, j = i - row * cols;  // j f <= (cols - 1) f < n
    out[i] = NthPick<Out, In, T>::get(in[row * n + j * f], scale);
  }
}

inline unsigned pool_grid(int64_t work_per_group_units) {
  return (unsigned)(work_per_group_units > kPoolGridMax ? kPoolGridMax : (work_per_group_units < 1 ? 1 : work_per_group_units));
}

template <typename T, int KIND, int OP>
int launch_pool_windows(const void* in_, int64_t rows, int64_t n, int64_t f, int64_t cols, T scale, void* out_,
                        hipStream_t st) {
  using R = Red<T, KIND, OP>;
  const auto* in = static_cast<const typename R::In*>(in_);
  auto* out = static_cast<typename R::Out*>(out_);
  constexpr int kVec = 16 / (int)sizeof(typename R::In);
  if (f <= kPoolSegMax) {
    if (kVec > 2 && f < kVec) {  // float32 windows of 2 or 3 columns: 8-byte loads, so that a lane still meets two windows at most
      const int64_t k = (kWave * 2) / f;
      k_pool_seg<T, KIND, OP, 2><<<pool_grid(ceil_div(rows * ceil_div(cols, k), kPoolWaves)), kPoolThreads, 0, st>>>(
          in, rows, n, (int)f, cols, scale, out);
    } else {
      const int64_t k = (kWave * kVec) / f;
      k_pool_seg<T, KIND, OP, kVec><<<pool_grid(ceil_div(rows * ceil_div(cols, k), kPoolWaves)), kPoolThreads, 0, st>>>(
          in, rows, n, (int)f, cols, scale, out);
    }
  } else if (f <= kPoolWaveMax) {
    k_pool_win<T, KIND, OP, false><<<pool_grid(ceil_div(rows * cols, kPoolWaves)), kPoolThreads, 0, st>>>(in, rows, n, f, cols,
                                                                                                         scale, out);
  } else {
    k_pool_win<T, KIND, OP, true><<<pool_grid(rows * cols), kPoolThreads, 0, st>>>(in, rows, n, f, cols, scale, out);
  }
  QI_LAUNCH_CHECK();
  return QI_OK;
}

template <typename T, int KIND>
int launch_pool(const void* in_, int64_t rows, int64_t n, int64_t f, int64_t cols, int method, T scale, void* out,
                hipStream_t st) {
  using In = typename PoolIn<T, KIND>::type;
  using NthOut = typename std::conditional<KIND == QI_POOL_POWER, T, In>::type;
  const auto* in = static_cast<const In*>(in_);
  switch (method) {
    case QI_POOL_NTH:
      k_pool_nth<In, NthOut, T><<<pool_grid(ceil_div(rows * cols, kPoolThreads)), kPoolThreads, 0, st>>>(
          in, rows, n, f, cols, scale, static_cast<NthOut*>(out));
      QI_LAUNCH_CHECK();
      return QI_OK;
    case QI_POOL_AVERAGE:
      return launch_pool_windows<T, KIND, kOpSum>(in_, rows, n, f, cols, scale, out, st);
    default:
      break;
  }
  if constexpr (KIND != QI_POOL_COMPLEX) {
    if (method == QI_POOL_MAX) return launch_pool_windows<T, KIND, kOpMax>(in_, rows, n, f, cols, scale, out, st);
    if (method == QI_POOL_MIN) return launch_pool_windows<T, KIND, kOpMin>(in_, rows, n, f, cols, scale, out, st);
    if (method == QI_POOL_MEDIAN) {
      int lg = 1;
      while ((1 << lg) < f) ++lg;
      const int64_t per = kPoolMedianMax >> lg;
      k_pool_median<T, KIND><<<pool_grid(rows * ceil_div(cols, per)), kPoolThreads, 0, st>>>(in, rows, n, (int)f, lg, cols, scale,
                                                                                             static_cast<T*>(out));
      QI_LAUNCH_CHECK();
      return QI_OK;
    }
  }
  set_error("pooling method %d does not apply to this input", method);
  return QI_ERR_ARG;
}

template <typename T>
int pool_dispatch(const void* in, int kind, int64_t rows, int64_t n, int64_t f, int64_t cols, int method, double power_scale,
                  void* out, hipStream_t st) {
  const T scale = (T)host::power_scale_or_default(power_scale);
  if (kind == QI_POOL_REAL) return launch_pool<T, QI_POOL_REAL>(in, rows, n, f, cols, method, scale, out, st);
  if (kind == QI_POOL_COMPLEX) return launch_pool<T, QI_POOL_COMPLEX>(in, rows, n, f, cols, method, scale, out, st);
  return launch_pool<T, QI_POOL_POWER>(in, rows, n, f, cols, method, scale, out, st);
}

}  // namespace

}  // namespace qi

using namespace qi;

extern "C" {

int64_t qi_pool_columns(int64_t n, int64_t factor, int method) {
  QI_REQUIRE(n >= 1, "bad row length %lld", (long long)n);
  QI_REQUIRE(factor >= 2, "pooling factor %lld: 2 or more", (long long)factor);
  QI_REQUIRE(method >= QI_POOL_NTH && method <= QI_POOL_MEDIAN, "unknown pooling method %d", method);
  return method == QI_POOL_NTH ? (n + factor - 1) / factor : n / factor;
}

int qi_pool_panel(int dtype, int device, const void* in, int input_kind, int64_t rows, int64_t n, int64_t factor, int method,
                  double power_scale, void* out, qi_stream stream) {
  QI_REQUIRE(dtype == QI_F32 || dtype == QI_F64, "bad dtype %d", dtype);
  QI_REQUIRE(input_kind >= QI_POOL_REAL && input_kind <= QI_POOL_POWER, "bad input kind %d", input_kind);
  QI_REQUIRE(rows >= 1, "bad panel shape");
  const int64_t cols = qi_pool_columns(n, factor, method);
  if (cols < 0) return (int)cols;
  QI_REQUIRE(input_kind != QI_POOL_COMPLEX || method == QI_POOL_NTH || method == QI_POOL_AVERAGE,
             "complex values have no order: only nth and average pool a complex panel (method %d)", method);
  if (method == QI_POOL_MEDIAN && factor > kPoolMedianMax) {
    set_error("median pooling sorts a window in LDS: factor <= %d (got %lld)", kPoolMedianMax, (long long)factor);
    return QI_ERR_UNSUPPORTED;
  }
  if (cols == 0) return QI_OK;  // factor > n: nothing to write
  QI_REQUIRE(in && out, "null argument");
  DeviceGuard g(device);
  return dtype == QI_F64 ? pool_dispatch<double>(in, input_kind, rows, n, factor, cols, method, power_scale, out, (hipStream_t)stream)
                         : pool_dispatch<float>(in, input_kind, rows, n, factor, cols, method, power_scale, out, (hipStream_t)stream);
}

}  // extern "C"
