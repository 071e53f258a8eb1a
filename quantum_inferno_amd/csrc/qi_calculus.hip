// Integration and differentiation of records: utilities.calculations.integrate_with_cumtrapz_* (calculations.py:16-41:
// scipy.integrate.cumulative_trapezoid(initial=0)), derivative_with_gradient_* (calculations.py:44-63: np.gradient) and
// derivative_with_difference_* (calculations.py:118-157: np.diff), restated.
//
// qi_cumtrapz.  Term i of a record, 0 <= i < n - 1, is d_i * (y[i+1] + y[i]) / 2.0 in SciPy's order and types: the sum in the
// record's type; with timestamps d_i = x[i+1] - x[i] and the product and the halving in float64, with a constant dx both
// in the record's type, dx rounded to it once.  Output 0 is 0, output i + 1 the sum of the terms 0 .. i in the result
// type R (float64 with timestamps, the record's type without).  NumPy adds them left to right; here the order of the
// additions is this tree, a function of n alone -- not of the record count, the record's row, the grid or the run:
//   tiles   the terms are cut into tiles of QI_SCAN_TILE = 4096; a tile's missing terms (the last tile's) are +0.0;
//   lane    lane l of the 256 of a tile owns its terms 16 l .. 16 l + 15 and sums them left to right:
//           r_0 = t_0, r_k = r_(k-1) + t_k; the lane's total is r_15;
//   wave    an inclusive Hillis-Steele scan of the 64 lane totals of a wave: for s = 1, 2, 4, 8, 16, 32 every lane l >= s
//           replaces v_l by v_(l-s) + v_l, all lanes at once; the exclusive value e_l is v_(l-1) of the result, e_0 = 0;
//           the wave's total W_w is v_63;
//   tile    the four wave totals left to right: o_0 = 0, o_1 = W_0, o_2 = W_0 + W_1, o_3 = o_2 + W_2; the tile's total is
//           o_3 + W_3;
//   record  the tile totals left to right: c_0 = 0, c_1 = T_0, c_t = c_(t-1) + T_(t-1);
//   output  out[4096 t + 16 l + k + 1] = (c_t + (o_w + e_l)) + r_k.
// Three launches on the caller's stream: k_scan_totals (a workgroup per tile and record: T_t to scratch [C][tiles]),
// k_scan_carries (a lane per record: T_t replaced by c_t in place), k_scan_store (the terms formed again, not stored and
// re-read: the tree above and the stores).  No atomics, no workgroup waits for another.  A tile's terms are formed with
// coalesced loads and laid in LDS (a pad of one element per sixteen: lane l's run starts at 17 l), summed per lane from
// there, and the outputs go back through the same LDS to coalesced stores.  tests/calculus_cases.py restates the tree in
// NumPy (scan_ref); the device equals it bit for bit.
//
// qi_derivative.  One launch, no scratch; a workgroup owns 1024 consecutive outputs of one record.
//   gradient    np.gradient(y, h) / np.gradient(y, x), edge_order 1.  Uniform: (f[i+1] - f[i-1]) / (2.0 h) inside and
//               (f[1] - f[0]) / h, (f[n-1] - f[n-2]) / h at the ends, in the record's type, 2.0 h formed in double and
//               rounded once.  With timestamps: dx1 = x[i] - x[i-1], dx2 = x[i+1] - x[i], a = -(dx2) / (dx1 (dx1 + dx2)),
//               b = (dx2 - dx1) / (dx1 dx2), c = dx1 / (dx2 (dx1 + dx2)), (a f[i-1] + b f[i]) + c f[i+1] in float64; the ends
//               are the difference in the record's type, widened, over x[1] - x[0] and x[n-1] - x[n-2]; stored in the
//               record's type, as NumPy returns it.
//   difference  (f[i+1] - f[i]) * h in the record's type (h is the FACTOR here: the reference multiplies by the sample
//               rate), or the difference in the record's type, widened, over x[i+1] - x[i] in float64; n - 1 values at
//               columns out_offset .. out_offset + n - 2 of a row of n, the remaining column left alone.
// The file is compiled with -ffp-contract=off and -fhip-fp32-correctly-rounded-divide-sqrt (_build.py: PER_FILE_FLAGS):
// every product, sum and quotient is rounded on its own and the float32 division is IEEE's.
#include "qi_host.hpp"
#include "qi_device.hpp"   // kWave
#include "qi_fft_reg.hpp"  // QI_LAUNCH_CHECK

namespace qi {

namespace {

constexpr int kScTile = QI_SCAN_TILE;
constexpr int kScThreads = 256;
constexpr int kScRun = kScTile / kScThreads;  // consecutive terms of a lane
constexpr int kScWaves = kScThreads / kWave;
constexpr int kScLds = kScTile + kScTile / kScRun;  // one pad per run: lane l's run starts at (kScRun + 1) l
static_assert(kScRun == 16 && kScWaves == 4, "the tree of the header comment");
static_assert(kScLds * 8 <= 64 * 1024, "static LDS of a workgroup");

__device__ __forceinline__ int sc_slot(int i) { return i + (i >> 4); }

struct ScanArgs {
  const void* y;    // [C][n] in the record's type
  const double* x;  // nullptr, [n] or [C][n]
  void* out;        // [C][n] in the result type
  void* scratch;    // [C][tiles] in the result type
  int64_t x_stride, n, tiles;
  double dx;
};

// R: the result type (double with timestamps, Y without)
template <typename Y, bool X>
struct ScanTypes {
  using R = std::conditional_t<X, double, Y>;
};

// The tile's terms into LDS, coalesced; the terms behind the record's last are +0.0.
template <typename Y, bool X, typename R>
__device__ __forceinline__ void scan_terms(const ScanArgs& a, int64_t c, int64_t j0, R* s) {
  const Y* __restrict__ y = static_cast<const Y*>(a.y) + c * a.n;
  const double* __restrict__ x = X ? a.x + c * a.x_stride : nullptr;
  const int64_t terms = a.n - 1;
  const R d = (R)a.dx;
#pragma unroll
  for (int u = 0; u < kScRun; ++u) {
    const int i = (int)threadIdx.x + u * kScThreads;
    const int64_t j = j0 + i;
    R t = R(0);
    if (j < terms) {
      const Y sum = y[j + 1] + y[j];
      if constexpr (X) t = (x[j + 1] - x[j]) * (double)sum / 2.0;
      else t = d * sum / R(2);
    }
    s[sc_slot(i)] = t;
  }
}

// The lane's running sums r[0 .. 15] from LDS; -> its exclusive value inside the wave (e_l) and, in s_w, the wave totals.
template <typename R>
__device__ __forceinline__ R scan_wave(const R* s, R* r, R* s_w) {
  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  const R* mine = s + tid * (kScRun + 1);
  r[0] = mine[0];
#pragma unroll
  for (int k = 1; k < kScRun; ++k) r[k] = r[k - 1] + mine[k];
  R v = r[kScRun - 1];
#pragma unroll
  for (int st = 1; st < kWave; st <<= 1) {
    const R o = __shfl_up(v, st, kWave);
    if (lane >= st) v = o + v;
  }
  R e = __shfl_up(v, 1, kWave);
  if (lane == 0) e = R(0);
  if (lane == kWave - 1) s_w[tid / kWave] = v;
  return e;
}

template <typename Y, bool X>
__global__ void __launch_bounds__(kScThreads) k_scan_totals(ScanArgs a) {
  using R = typename ScanTypes<Y, X>::R;
  __shared__ R s[kScLds];
  __shared__ R s_w[kScWaves];
  const int64_t c = (int64_t)blockIdx.x / a.tiles, t = (int64_t)blockIdx.x - c * a.tiles;
  scan_terms<Y, X, R>(a, c, t * kScTile, s);
  __syncthreads();
  R r[kScRun];
  scan_wave<R>(s, r, s_w);
  __syncthreads();
  if (threadIdx.x == 0) static_cast<R*>(a.scratch)[c * a.tiles + t] = ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
}

// c_0 = 0, c_1 = T_0, c_t = c_(t-1) + T_(t-1): a lane per record, in place.
template <typename R>
__global__ void __launch_bounds__(kWave) k_scan_carries(R* __restrict__ scratch, int64_t C, int64_t tiles) {
  const int64_t c = (int64_t)blockIdx.x * kWave + threadIdx.x;
  if (c >= C) return;
  R* p = scratch + c * tiles;
  R acc = p[0];
  p[0] = R(0);
  for (int64_t t = 1; t < tiles; ++t) {
    const R total = p[t];
    p[t] = acc;
    acc = acc + total;
  }
}

template <typename Y, bool X>
__global__ void __launch_bounds__(kScThreads) k_scan_store(ScanArgs a) {
  using R = typename ScanTypes<Y, X>::R;
  __shared__ R s[kScLds];
  __shared__ R s_w[kScWaves];
  const int tid = threadIdx.x;
  const int64_t c = (int64_t)blockIdx.x / a.tiles, t = (int64_t)blockIdx.x - c * a.tiles;
  const int64_t j0 = t * kScTile;
  scan_terms<Y, X, R>(a, c, j0, s);
  __syncthreads();
  R r[kScRun];
  const R e = scan_wave<R>(s, r, s_w);
  const R carry = static_cast<const R*>(a.scratch)[c * a.tiles + t];
  __syncthreads();
  const int w = tid / kWave;
  R o = R(0);
  if (w >= 1) o = s_w[0];
  if (w >= 2) o = o + s_w[1];
  if (w >= 3) o = o + s_w[2];
  const R base = carry + (o + e);
  R* mine = s + tid * (kScRun + 1);  // (only this lane read these slots)
#pragma unroll
  for (int k = 0; k < kScRun; ++k) mine[k] = base + r[k];
  __syncthreads();
  R* __restrict__ out = static_cast<R*>(a.out) + c * a.n;
  const int64_t terms = a.n - 1;
  if (t == 0 && tid == 0) out[0] = R(0);
#pragma unroll
  for (int u = 0; u < kScRun; ++u) {
    const int i = tid + u * kScThreads;
    const int64_t j = j0 + i;
    if (j < terms) out[j + 1] = s[sc_slot(i)];
  }
}

// ---- derivatives -----------------------------------------------------------------------------------------------------------
constexpr int kDvThreads = 256;
constexpr int kDvTile = 1024;  // outputs of a workgroup

struct DerivArgs {
  const void* y;    // [C][n]
  const double* x;  // nullptr, [n] or [C][n]
  void* out;        // [C][n]: the record's type, float64 for a difference over timestamps
  int64_t x_stride, n, count, chunks, out_offset;  // count: outputs per record (n, or n - 1 differences)
  double h;
};

template <typename Y, bool X, int KIND>
__global__ void __launch_bounds__(kDvThreads) k_derivative(DerivArgs a) {
  using O = std::conditional_t<(X && KIND == QI_DERIV_DIFFERENCE), double, Y>;
  const int64_t c = (int64_t)blockIdx.x / a.chunks, q = (int64_t)blockIdx.x - c * a.chunks;
  const int64_t n = a.n;
  const Y* __restrict__ f = static_cast<const Y*>(a.y) + c * n;
  const double* __restrict__ x = X ? a.x + c * a.x_stride : nullptr;
  O* __restrict__ out = static_cast<O*>(a.out) + c * n + a.out_offset;
  const Y h = (Y)a.h, h2 = (Y)(2.0 * a.h);
#pragma unroll
  for (int u = 0; u < kDvTile / kDvThreads; ++u) {
    const int64_t i = q * kDvTile + u * kDvThreads + threadIdx.x;
    if (i >= a.count) continue;
    if constexpr (KIND == QI_DERIV_DIFFERENCE) {
      const Y d = f[i + 1] - f[i];
      if constexpr (X) out[i] = (double)d / (x[i + 1] - x[i]);
      else out[i] = d * h;
    } else {
      const bool first = i == 0, last = i == n - 1;
      if (first || last) {
        const int64_t k = first ? 0 : n - 2;
        const Y d = f[k + 1] - f[k];
        if constexpr (X) out[i] = (Y)((double)d / (x[k + 1] - x[k]));
        else out[i] = d / h;
      } else if constexpr (X) {
        const double dx1 = x[i] - x[i - 1], dx2 = x[i + 1] - x[i];
        const double ca = -(dx2) / (dx1 * (dx1 + dx2));
        const double cb = (dx2 - dx1) / (dx1 * dx2);
        const double cc = dx1 / (dx2 * (dx1 + dx2));
        out[i] = (Y)((ca * (double)f[i - 1] + cb * (double)f[i]) + cc * (double)f[i + 1]);
      } else {
        out[i] = (f[i + 1] - f[i - 1]) / h2;
      }
    }
  }
}

int64_t scan_tiles(int64_t n) { return n > 1 ? ceil_div(n - 1, kScTile) : 1; }

template <typename Y, bool X>
int launch_scan(const ScanArgs& a, int64_t C, hipStream_t st) {
  using R = typename ScanTypes<Y, X>::R;
  const unsigned grid = (unsigned)(C * a.tiles);
  k_scan_totals<Y, X><<<grid, kScThreads, 0, st>>>(a);
  QI_LAUNCH_CHECK();
  k_scan_carries<R><<<(unsigned)ceil_div(C, kWave), kWave, 0, st>>>(static_cast<R*>(a.scratch), C, a.tiles);
  QI_LAUNCH_CHECK();
  k_scan_store<Y, X><<<grid, kScThreads, 0, st>>>(a);
  QI_LAUNCH_CHECK();
  return QI_OK;
}

template <typename Y, bool X>
int launch_derivative(int kind, const DerivArgs& a, int64_t C, hipStream_t st) {
  const unsigned grid = (unsigned)(C * a.chunks);
  if (kind == QI_DERIV_GRADIENT) k_derivative<Y, X, QI_DERIV_GRADIENT><<<grid, kDvThreads, 0, st>>>(a);
  else k_derivative<Y, X, QI_DERIV_DIFFERENCE><<<grid, kDvThreads, 0, st>>>(a);
  QI_LAUNCH_CHECK();
  return QI_OK;
}

}  // namespace

}  // namespace qi

using namespace qi;

extern "C" {

int64_t qi_cumtrapz_scratch_bytes(int dtype, int64_t n_channels, int64_t n) {
  QI_TRY(require_records(dtype, n_channels, n, 0));
  QI_REQUIRE(n < (1ll << 40) && n_channels < (1ll << 31) && n_channels * scan_tiles(n) < (1ll << 31), "request too large");
  // the tile totals, then carries, in the result type: float64 whenever timestamps are given
  return (int64_t)host::align_up((size_t)(n_channels > 0 ? n_channels : 1) * (size_t)scan_tiles(n) * 8);
}

int qi_cumtrapz(int dtype, int device, const void* y, const void* x, int64_t x_stride, double dx, int64_t n_channels, int64_t n,
                void* out, void* scratch, int64_t scratch_bytes, qi_stream stream) {
  const int64_t need = qi_cumtrapz_scratch_bytes(dtype, n_channels, n);
  if (need < 0) return (int)need;
  QI_TRY(require_timestamp_stride("x_stride", x_stride, n));
  QI_REQUIRE(x || x_stride == 0, "x_stride must be 0 without timestamps");
  if (n_channels == 0) return QI_OK;
  QI_REQUIRE(y && out && scratch, "null argument");
  QI_TRY(require_scratch(scratch_bytes, need));
  const size_t esz = elem_size(dtype);
  QI_REQUIRE(aligned(y, esz) && aligned(x, 8) && aligned(out, x ? 8 : esz) && aligned(scratch, 8),
             "y, x, out and scratch must be aligned to their element size");
  DeviceGuard g(device);
  QI_REQUIRE(g.ok, "cannot select device %d", device);
  ScanArgs a{};
  a.y = y;
  a.x = static_cast<const double*>(x);
  a.out = out;
  a.scratch = scratch;
  a.x_stride = x_stride;
  a.n = n;
  a.tiles = scan_tiles(n);
  a.dx = dx;
  hipStream_t st = (hipStream_t)stream;
  return by_dtype(dtype, [&](auto t) -> int {
    using Y = decltype(t);
    return x ? launch_scan<Y, true>(a, n_channels, st) : launch_scan<Y, false>(a, n_channels, st);
  });
}

int qi_derivative(int dtype, int device, int kind, const void* y, const void* x, int64_t x_stride, double h, int64_t n_channels,
                  int64_t n, void* out, int64_t out_offset, qi_stream stream) {
  QI_TRY(require_records(dtype, n_channels, n, 0));
  QI_REQUIRE(kind == QI_DERIV_GRADIENT || kind == QI_DERIV_DIFFERENCE, "bad kind %d", kind);
  QI_REQUIRE(kind != QI_DERIV_GRADIENT || n >= 2, "bad record length %lld: a gradient needs two samples", (long long)n);
  QI_TRY(require_timestamp_stride("x_stride", x_stride, n));
  QI_REQUIRE(x || x_stride == 0, "x_stride must be 0 without timestamps");
  QI_REQUIRE(out_offset == 0 || (kind == QI_DERIV_DIFFERENCE && out_offset == 1),
             "out_offset must be 0, or 1 for a difference, got %lld", (long long)out_offset);
  const int64_t count = kind == QI_DERIV_GRADIENT ? n : n - 1;
  const int64_t chunks = ceil_div(count, kDvTile);
  QI_REQUIRE(n < (1ll << 40) && n_channels < (1ll << 31) && n_channels * chunks < (1ll << 31), "request too large");
  if (n_channels == 0) return QI_OK;
  QI_REQUIRE(y && out, "null argument");
  const size_t esz = elem_size(dtype);
  QI_REQUIRE(aligned(y, esz) && aligned(x, 8) && aligned(out, x && kind == QI_DERIV_DIFFERENCE ? 8 : esz),
             "y, x and out must be aligned to their element size");
  if (count == 0) return QI_OK;
  DeviceGuard g(device);
  QI_REQUIRE(g.ok, "cannot select device %d", device);
  DerivArgs a{};
  a.y = y;
  a.x = static_cast<const double*>(x);
  a.out = out;
  a.x_stride = x_stride;
  a.n = n;
  a.count = count;
  a.chunks = chunks;
  a.out_offset = out_offset;
  a.h = h;
  hipStream_t st = (hipStream_t)stream;
  return by_dtype(dtype, [&](auto t) -> int {
    using Y = decltype(t);
    return x ? launch_derivative<Y, true>(kind, a, n_channels, st) : launch_derivative<Y, false>(kind, a, n_channels, st);
  });
}

}  // extern "C"
