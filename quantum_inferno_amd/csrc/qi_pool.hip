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
// qi_pool_strip (k_pool_strip, further down) pools a column range of a complex panel's power: the average and the maximum
// of every window and the range's {max P, sum P, sum P log2 P} per row from ONE read -- what a streamed record keeps of a
// chunk (stream.py: the range a chunk owns).
#include <algorithm>
#include <map>
#include <mutex>
#include <type_traits>
#include <utility>

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

// ---- strips: the windows of a column range and the additive sums of that range, from one read -------------------------
// A row's range [first, first + windows f) is cut into S segments of G consecutive windows; a workgroup takes a segment:
//   kStripLane   f < 64       a thread per window, element loads (the plain path)
//   kStripWave   f <= 1024    a wave per window, the waves take the segment's windows in turn; loads as k_pool_win
//   kStripBlock  larger       the workgroup per window, one after the other
// Every lane folds its elements into the window's sum (float64) and maximum and into its share of the segment's
// {maximum, sum P, sum P log2 P}; a window is finished by the wave reduction (kStripBlock: then the waves in index order),
// the segment's triple the same way at the end.  With S = 1 the triple is the row's; otherwise it goes to `part`
// [rows][S][3] and k_strip_fold adds the segments up, lanes striding over them, then the wave: a fixed order throughout.
enum { kStripLane = 0, kStripWave = 1, kStripBlock = 2 };
constexpr int64_t kStripUnits = 4096;            // segments a launch aims at
constexpr int64_t kStripSlots = 2 * kStripUnits;  // triples of the partials buffer: rows S < rows + kStripUnits, and S > 1 only for rows < kStripUnits

__device__ __forceinline__ double strip_plog2p(float p, const double (*)[2]) { return (double)native::plog2p(p); }
__device__ __forceinline__ double strip_plog2p(double p, const double (*tab)[2]) { return native::plog2p_flat(p, tab); }

template <typename T>
struct StripLane {
  double a;  // sum of P over the lane's elements of this window
  T m;       // their maximum
  double l;  // sum of P log2 P over the lane's elements of the segment
  __device__ __forceinline__ void take(cplx<T> z, T scale, const double (*tab)[2]) {
    const T p = pool_value(z, scale);
    a += (double)p;
    m = p > m ? p : m;
    l += strip_plog2p(p, tab);
  }
};

template <typename T, int MODE>
__global__ void __launch_bounds__(kPoolThreads) k_pool_strip(const cplx<T>* __restrict__ in, int64_t rows, int64_t stride,
                                                             int64_t first, int64_t f, int64_t windows, int64_t G, int64_t S,
                                                             T scale, T* __restrict__ mean, T* __restrict__ mx, int64_t ostride,
                                                             double* __restrict__ part) {
  using In = cplx<T>;
  constexpr int V = 16 / (int)sizeof(In);
  using Vec = PoolVec<In, V>;
  constexpr bool kTab = std::is_same<T, double>::value;  // the float64 logarithm reads its table from LDS (log2_pos)
  __shared__ double ltab[kTab ? 128 : 1][2];
  __shared__ double sa[kPoolWaves], sl[kPoolWaves];
  __shared__ T sm[kPoolWaves];
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
  if constexpr (kTab) {
    (&ltab[0][0])[threadIdx.x] = (&native::kLog2Tab[0][0])[threadIdx.x];  // 256 threads, 128 x 2 entries
    __syncthreads();
  }
  const T low = -(T)__builtin_huge_val();
  const int nt = MODE == kStripBlock ? kPoolThreads : kWave;
  const int t = MODE == kStripBlock ? (int)threadIdx.x : lane;
  for (int64_t u = blockIdx.x; u < rows * S; u += gridDim.x) {  // (uniform over the workgroup)
    const int64_t row = u / S, w0 = (u - row * S) * G;
    const int64_t w1 = w0 + G < windows ? w0 + G : windows;
    const In* base = in + row * stride + first;  // first + w1 f <= first + windows f <= stride
    StripLane<T> x{0.0, low, 0.0};
    double ra = 0.0;  // the lane's share of the segment: sum and maximum (x.l runs on over the windows)
    T rm = low;
    if (MODE == kStripLane) {
      for (int64_t w = w0 + threadIdx.x; w < w1; w += kPoolThreads) {
        const In* src = base + w * f;
        x.a = 0.0;
        x.m = low;
        for (int64_t i = 0; i < f; ++i) x.take(src[i], scale, ltab);
        if (mean) mean[row * ostride + w] = (T)(x.a / (double)f);
        if (mx) mx[row * ostride + w] = x.m;
        ra += x.a;
        rm = x.m > rm ? x.m : rm;
      }
    } else {
      for (int64_t w = w0 + (MODE == kStripBlock ? 0 : wv); w < w1; w += (MODE == kStripBlock ? 1 : kPoolWaves)) {
        const In* src = base + w * f;
        int64_t hd = (int64_t)(((16 - (reinterpret_cast<uintptr_t>(src) & 15)) & 15) / sizeof(In));
        if (hd > f) hd = f;
        const int64_t nv = (f - hd) / V, tl = hd + nv * V;
        x.a = 0.0;
        x.m = low;
        if (t < hd) x.take(src[t], scale, ltab);
        const Vec* vp = reinterpret_cast<const Vec*>(src + hd);
        auto take_vec = [&](const Vec& v) {
#pragma unroll
          for (int q = 0; q < V; ++q) x.take(v.e[q], scale, ltab);
        };
        // four, then two, then one load in flight per lane; the lane's elements are folded in ascending order either way
        int64_t i = t;
        for (; i + 3 * nt < nv; i += 4 * nt) {
          const Vec v0 = vp[i], v1 = vp[i + nt], v2 = vp[i + 2 * nt], v3 = vp[i + 3 * nt];
          take_vec(v0);
          take_vec(v1);
          take_vec(v2);
          take_vec(v3);
        }
        if (i + nt < nv) {
          const Vec v0 = vp[i], v1 = vp[i + nt];
          take_vec(v0);
          take_vec(v1);
          i += 2 * nt;
        }
        if (i < nv) take_vec(vp[i]);
        if (tl + t < f) x.take(src[tl + t], scale, ltab);
        ra += x.a;
        rm = x.m > rm ? x.m : rm;
        if (MODE == kStripWave) {  // (the loop is uniform over the wave: every lane is here)
          if (mean) {
            const double a = wave_sum(x.a);
            if (lane == 0) mean[row * ostride + w] = (T)(a / (double)f);
          }
          if (mx) {
            const T m = wave_max(x.m);
            if (lane == 0) mx[row * ostride + w] = m;
          }
        } else if (mean || mx) {  // (uniform over the workgroup)
          const double a = wave_sum(x.a);
          const T m = wave_max(x.m);
          if (lane == 0) {
            sa[wv] = a;
            sm[wv] = m;
          }
          __syncthreads();
          if (threadIdx.x == 0) {
            double r = sa[0];
            T q = sm[0];
            for (int k = 1; k < kPoolWaves; ++k) {
              r += sa[k];
              q = sm[k] > q ? sm[k] : q;
            }
            if (mean) mean[row * ostride + w] = (T)(r / (double)f);
            if (mx) mx[row * ostride + w] = q;
          }
          __syncthreads();
        }
      }
    }
    if (part) {  // (uniform; the loops above have reconverged)
      const double a = wave_sum(ra), l = wave_sum(x.l);
      const T m = wave_max(rm);
      if (lane == 0) {
        sa[wv] = a;
        sl[wv] = l;
        sm[wv] = m;
      }
      __syncthreads();
      if (threadIdx.x == 0) {
        double r = sa[0], g = sl[0];
        T q = sm[0];
        for (int k = 1; k < kPoolWaves; ++k) {
          r += sa[k];
          g += sl[k];
          q = sm[k] > q ? sm[k] : q;
        }
        part[u * 3 + 0] = (double)q;
        part[u * 3 + 1] = r;
        part[u * 3 + 2] = g;
      }
      __syncthreads();
    }
  }
}

// out[g][0 .. 2] = {max, sum, sum} over the `per` consecutive triples of group g, out[g][3 .. width - 1] = 0: a wave per
// group, lanes striding over the triples, then the wave
__global__ void __launch_bounds__(kPoolThreads) k_strip_fold(const double* __restrict__ part, int64_t groups, int64_t per,
                                                             double* __restrict__ out, int width) {
  const int lane = threadIdx.x & (kWave - 1);
  for (int64_t g = (int64_t)blockIdx.x * kPoolWaves + threadIdx.x / kWave; g < groups; g += (int64_t)gridDim.x * kPoolWaves) {
    double m = -__builtin_huge_val(), s = 0.0, l = 0.0;
    for (int64_t i = lane; i < per; i += kWave) {
      const double* p = part + (g * per + i) * 3;
      m = p[0] > m ? p[0] : m;
      s += p[1];
      l += p[2];
    }
    m = wave_max(m);  // (the loop over g is uniform over the wave)
    s = wave_sum(s);
    l = wave_sum(l);
    if (lane == 0) {
      out[g * width + 0] = m;
      out[g * width + 1] = s;
      out[g * width + 2] = l;
      for (int k = 3; k < width; ++k) out[g * width + k] = 0.0;
    }
  }
}

// The partials of a strip launch with S > 1: one buffer of kStripSlots triples per (device, stream), made at the first such
// call and kept (196 KB).  Launches of one stream run in order, so they share it; other streams have their own.
std::mutex g_strip_mutex;
std::map<std::pair<int, hipStream_t>, double*> g_strip_part;

int strip_partials(int device, hipStream_t st, double** out) {
  std::lock_guard<std::mutex> lock(g_strip_mutex);
  double*& p = g_strip_part[{device, st}];
  if (!p) QI_HIP(hipMalloc((void**)&p, (size_t)kStripSlots * 3 * sizeof(double)));
  *out = p;
  return QI_OK;
}

template <typename T>
int launch_strip(int device, const void* in_, int64_t rows, int64_t stride, int64_t first, int64_t f, int64_t windows,
                 double power_scale, void* mean, void* mx, int64_t ostride, double* sums, hipStream_t st) {
  const T scale = (T)host::power_scale_or_default(power_scale);
  const int mode = f < kPoolSegMax ? kStripLane : (f <= kPoolWaveMax ? kStripWave : kStripBlock);
  const int64_t gmin = mode == kStripLane ? kPoolThreads : (mode == kStripWave ? kPoolWaves : 1);
  const int64_t G = std::max(gmin, ceil_div(rows * windows, kStripUnits));
  const int64_t S = ceil_div(windows, G);
  double* part = sums;
  if (sums && S > 1) {
    QI_REQUIRE(rows * S <= kStripSlots, "strip partials: %lld segments", (long long)(rows * S));
    const int rc = strip_partials(device, st, &part);
    if (rc != QI_OK) return rc;
  }
  const auto* in = static_cast<const cplx<T>*>(in_);
  const unsigned grid = pool_grid(rows * S);
  if (mode == kStripLane)
    k_pool_strip<T, kStripLane><<<grid, kPoolThreads, 0, st>>>(in, rows, stride, first, f, windows, G, S, scale, (T*)mean, (T*)mx,
                                                               ostride, part);
  else if (mode == kStripWave)
    k_pool_strip<T, kStripWave><<<grid, kPoolThreads, 0, st>>>(in, rows, stride, first, f, windows, G, S, scale, (T*)mean, (T*)mx,
                                                               ostride, part);
  else
    k_pool_strip<T, kStripBlock><<<grid, kPoolThreads, 0, st>>>(in, rows, stride, first, f, windows, G, S, scale, (T*)mean, (T*)mx,
                                                                ostride, part);
  QI_LAUNCH_CHECK();
  if (sums && S > 1) {
    k_strip_fold<<<pool_grid(ceil_div(rows, kPoolWaves)), kPoolThreads, 0, st>>>(part, rows, S, sums, 3);
    QI_LAUNCH_CHECK();
  }
  return QI_OK;
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
  return by_dtype(dtype, [&](auto t) {
    return pool_dispatch<decltype(t)>(in, input_kind, rows, n, factor, cols, method, power_scale, out, (hipStream_t)stream);
  });
}

int qi_pool_strip(int dtype, int device, const void* in, int64_t rows, int64_t row_stride, int64_t first, int64_t factor,
                  int64_t windows, double power_scale, void* mean_out, void* max_out, int64_t out_stride, void* sums_out,
                  qi_stream stream) {
  QI_REQUIRE(dtype == QI_F32 || dtype == QI_F64, "bad dtype %d", dtype);
  QI_REQUIRE(in, "null argument");
  QI_REQUIRE(rows >= 1 && row_stride >= 1, "bad panel shape");
  QI_REQUIRE(factor >= 2, "pooling factor %lld: 2 or more", (long long)factor);
  QI_REQUIRE(first >= 0 && windows >= 0 && first <= row_stride && windows <= (row_stride - first) / factor,
             "%lld windows of %lld columns from column %lld do not fit a row of %lld", (long long)windows, (long long)factor,
             (long long)first, (long long)row_stride);
  QI_REQUIRE(!(mean_out || max_out) || out_stride >= windows, "output rows of %lld columns for %lld windows",
             (long long)out_stride, (long long)windows);
  if (windows == 0 || !(mean_out || max_out || sums_out)) return QI_OK;  // nothing to write
  DeviceGuard g(device);
  return by_dtype(dtype, [&](auto t) {
    return launch_strip<decltype(t)>(device, in, rows, row_stride, first, factor, windows, power_scale, mean_out, max_out, out_stride,
                                     static_cast<double*>(sums_out), (hipStream_t)stream);
  });
}

int qi_pool_strip_stats(int device, const void* sums, int64_t records, int64_t bands, void* stats, qi_stream stream) {
  QI_REQUIRE(sums && stats, "null argument");
  QI_REQUIRE(records >= 1 && bands >= 1, "bad shape");
  DeviceGuard g(device);
  k_strip_fold<<<pool_grid(ceil_div(records, kPoolWaves)), kPoolThreads, 0, (hipStream_t)stream>>>(
      static_cast<const double*>(sums), records, bands, static_cast<double*>(stats), 4);
  QI_LAUNCH_CHECK();
  return QI_OK;
}

}  // extern "C"
