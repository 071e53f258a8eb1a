// Scaling of records and peak picking: utilities.picker.scale_signal_by_extraction_type and the scipy.signal.find_peaks calls
// behind find_peaks_by_extraction_type / _with_bandpass / find_peaks_with_bits (picker.py:32-53, 79-151), restated.
//
// A record is cut into tiles of QI_PEAKS_TILE samples; a workgroup is ONE wave that owns kPkGroup consecutive tiles of one
// record, four consecutive samples of a tile per lane.  No workgroup ever waits for another one: what a tile needs from other
// tiles it reads from scratch written by an EARLIER launch, so every dependency between tiles is a kernel boundary (no
// look-back, no flag, no atomic).  One call is
//   1 k_peaks_extrema  per tile: nan-ignoring max, min, max |.| of the transformed record u (u = x, or log2(|x| + eps) in
//                      float64), the max of the raw record, and the flags {a NaN, a value that is none} -> scratch
//   2 k_peaks_finish   per record: the tiles' partials in a fixed order -> the divisor of the scaling and the height threshold
//   3 k_peaks_summary  per tile: the scaled values s (stored when `scaled` is asked for) and the tile's summary
//                      {s[first], length of the leading run of equal values, the value that ends that run}
//   4 k_peaks_pick     per tile: rising edges s[i-1] < s[i], the end j of each edge's run of equal values, the test s[j] < s[i],
//                      the height test; counts the peaks whose run STARTS in the tile
//   5 k_peaks_scan     per record: exclusive scan of the tiles' counts in tile order, and counts[record]
//   6 k_peaks_pick     again, now storing: peak m of a tile goes to column offset[tile] + m (only when positions / values are asked for)
// Plateaus: inside a tile the end of a run comes from a suffix-minimum over the lanes' first "next sample differs" positions.
// Only the LAST run of a tile can leave it (its last sample equals the first of the next tile); the wave then follows the
// summaries of the next tiles 64 at a time -- a tile stops the run when its leading run is shorter than the tile or the
// next tile starts with another value -- so a run over a whole 2^20-sample record costs 64 such steps, not a walk of the
// record.  A peak belongs to the tile its run starts in; runs are disjoint and ordered, so the midpoints come out ascending.
// Everything is computed in a fixed order: the same call gives the same bits.
//
// The file is compiled with -ffp-contract=off and correctly rounded float32 division (_build.py: PER_FILE_FLAGS): the
// scaled values of the sig* kinds are NumPy's quotients bit for bit.
#include "qi_host.hpp"
#include "qi_device.hpp"   // kWave
#include "qi_fft_reg.hpp"  // QI_LAUNCH_CHECK

#include <numeric>

namespace qi {

namespace {

constexpr int kPkTile = QI_PEAKS_TILE;        // samples per tile
constexpr int kPkVec = 4;                     // consecutive samples per lane
constexpr int kPkThreads = kPkTile / kPkVec;  // one wave
static_assert(kPkThreads == kWave, "a tile is one wave of four samples per lane");
constexpr int kPkGroup = 4;                   // consecutive tiles per workgroup
constexpr int kPkPart = 5;                    // doubles per tile of launch 1: max u, min u, max |u|, max x, flags
constexpr int kPkSumm = 3;                    // doubles per tile of launch 3: first value, the value ending the leading run, its length
constexpr int kPkRec = 2;                     // doubles per record of launch 2: divisor, height threshold
constexpr int kPkLds = kPkTile + 2 + (kPkTile + 2) / 4 + 1;  // a tile and its two neighbours, one pad word per four values
constexpr int kPkNone = 0x7fffffff;
constexpr int kPkHasNan = 1, kPkHasValue = 2;

struct PeakArgs {
  const void* sig;     // [C][n] in the record's type
  void* scaled;        // [C][n] in the scaled type, or null
  int64_t* positions;  // [C][capacity] or null
  double* values;      // [C][capacity] or null
  int64_t* counts;     // [C]
  double* part;        // scratch [C][tiles][kPkPart]
  double* summ;        // scratch [C][tiles][kPkSumm]
  int64_t* cnt;        // scratch [C][tiles]: peaks per tile, after the scan the column of each tile's first peak
  double* rec;         // scratch [C][kPkRec]
  int64_t C, n, tiles, groups, capacity;
  int scale, height_kind;
  double eps, height;
};

// the scaled type: the record's for the sig* kinds, float64 for the log2* kinds
template <typename T, bool LOG>
struct PkScaled {
  using type = T;
};
template <typename T>
struct PkScaled<T, true> {
  using type = double;
};

__device__ __forceinline__ int pk_at(int m) { return m + (m >> 2); }  // LDS index of tile slot m (slot k + 1 holds sample k)

template <typename T, bool LOG>
__device__ __forceinline__ typename PkScaled<T, LOG>::type pk_transform(T x, double eps) {
  if constexpr (LOG) return log2(fabs((double)x) + eps);
  else return x;
}
// IEEE division in the scaled type, nothing special-cased: 0 / 0, x / 0 and a negative divisor come out as in NumPy
template <typename S>
__device__ __forceinline__ S pk_scale(S u, S d, bool divide) {
  return divide ? u / d : u;
}
// max / min of two values that are no NaN; of +0 and -0 the max is +0 and the min -0, whatever the order of the operands
__device__ __forceinline__ double pk_max(double a, double b) { return (b > a || (b == a && !signbit(b))) ? b : a; }
__device__ __forceinline__ double pk_min(double a, double b) { return (b < a || (b == a && signbit(b))) ? b : a; }

struct PkPart {
  double mx, mn, am, rm;
  int flags;
};
__device__ __forceinline__ PkPart pk_empty() {
  return PkPart{-HUGE_VAL, HUGE_VAL, 0.0, -HUGE_VAL, 0};
}
__device__ __forceinline__ PkPart pk_join(const PkPart& a, const PkPart& b) {
  return PkPart{pk_max(a.mx, b.mx), pk_min(a.mn, b.mn), pk_max(a.am, b.am), pk_max(a.rm, b.rm), a.flags | b.flags};
}
// the partials of the 64 lanes -> every lane's return value, through LDS in a fixed tree
__device__ __forceinline__ PkPart pk_wave_join(PkPart p, PkPart* red) {
  const int tid = threadIdx.x;
  red[tid] = p;
  __syncthreads();
  for (int o = kPkThreads / 2; o > 0; o >>= 1) {
    if (tid < o) red[tid] = pk_join(red[tid], red[tid + o]);
    __syncthreads();
  }
  p = red[0];
  __syncthreads();
  return p;
}

// the tile [t0, t0 + len) of record c and the first tile of the workgroup
#define QI_PK_WORKGROUP()                                                 \
  const int tid = threadIdx.x;                                            \
  const int64_t c = (int64_t)blockIdx.x / a.groups;                       \
  const int64_t g0 = ((int64_t)blockIdx.x % a.groups) * kPkGroup;         \
  const int64_t g1 = g0 + kPkGroup < a.tiles ? g0 + kPkGroup : a.tiles
#define QI_PK_TILE()                                \
  const int64_t t0 = tile * kPkTile;                \
  const int len = (int)(a.n - t0 < kPkTile ? a.n - t0 : kPkTile)

template <typename T, bool LOG>
__global__ void __launch_bounds__(kPkThreads) k_peaks_extrema(PeakArgs a) {
  __shared__ PkPart red[kPkThreads];
  QI_PK_WORKGROUP();
  const T* x = static_cast<const T*>(a.sig) + c * a.n;
  for (int64_t tile = g0; tile < g1; ++tile) {
    QI_PK_TILE();
    PkPart p = pk_empty();
#pragma unroll
    for (int v = 0; v < kPkVec; ++v) {
      const int k = tid + v * kPkThreads;
      if (k < len) {
        const T xv = x[t0 + k];
        if (xv != xv) {  // (u is a NaN exactly when x is)
          p.flags |= kPkHasNan;
        } else {
          const double u = (double)pk_transform<T, LOG>(xv, a.eps);
          p = pk_join(p, PkPart{u, u, fabs(u), (double)xv, kPkHasValue});
        }
      }
    }
    p = pk_wave_join(p, red);
    if (tid == 0) {
      double* out = a.part + (c * a.tiles + tile) * kPkPart;
      out[0] = p.mx;
      out[1] = p.mn;
      out[2] = p.am;
      out[3] = p.rm;
      out[4] = (double)p.flags;
    }
  }
}

template <typename T, bool LOG>
__global__ void __launch_bounds__(kPkThreads) k_peaks_finish(PeakArgs a) {
  using S = typename PkScaled<T, LOG>::type;
  __shared__ PkPart red[kPkThreads];
  const int tid = threadIdx.x;
  const int64_t c = blockIdx.x;
  PkPart p = pk_empty();
  for (int64_t tile = tid; tile < a.tiles; tile += kPkThreads) {
    const double* in = a.part + (c * a.tiles + tile) * kPkPart;
    p = pk_join(p, PkPart{in[0], in[1], in[2], in[3], (int)in[4]});
  }
  p = pk_wave_join(p, red);
  if (tid != 0) return;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  const bool any = p.flags & kPkHasValue, has_nan = p.flags & kPkHasNan;
  // np.nanmax / nanmin / nanmax(abs): the extremum of the values that are no NaN, NaN when there is none
  const double d = !any ? nan : a.scale == QI_PEAK_SIGMIN ? p.mn : a.scale == QI_PEAK_SIGABS ? p.am : p.mx;
  // np.max of the scaled record: NaN as soon as one sample is.  The divisor is itself a value of u (of |u|), so a divisor of
  // 0 or of +-inf makes that sample 0 / 0 or inf / inf; a finite one keeps the order of u (division rounds monotonically)
  // or, when negative, reverses it.
  double top = nan;
  if (!has_nan && any) {
    if (a.scale == QI_PEAK_LOG2) top = p.mx;
    else if (d != 0.0 && fabs(d) != HUGE_VAL) top = (double)((S)(d > 0.0 ? p.mx : p.mn) / (S)d);
  }
  double thr = a.height;  // QI_PEAK_HEIGHT_ABS
  // the differences are formed as NumPy forms them: in the type of the maximum
  if (a.height_kind == QI_PEAK_HEIGHT_BELOW_MAX) thr = (double)((S)top - (S)a.height);
  if (a.height_kind == QI_PEAK_HEIGHT_BELOW_RAW_MAX) thr = (double)((T)(has_nan || !any ? nan : p.rm) - (T)a.height);
  a.rec[c * kPkRec] = d;
  a.rec[c * kPkRec + 1] = thr;
}

// scaled values of the tile into LDS slots 1 .. len (and into `scaled`); with `halo` the neighbours into slots 0 and len + 1
template <typename T, bool LOG, typename S>
__device__ __forceinline__ void pk_load_tile(const PeakArgs& a, S* sm, int64_t c, int64_t t0, int len, bool halo, S* scaled) {
  const int tid = threadIdx.x;
  const T* x = static_cast<const T*>(a.sig) + c * a.n;
  const S d = (S)a.rec[c * kPkRec];  // (exact: the divisor is a value of the scaled type)
  const bool divide = a.scale != QI_PEAK_LOG2;
#pragma unroll
  for (int v = 0; v < kPkVec; ++v) {
    const int k = tid + v * kPkThreads;
    if (k < len) {
      const S s = pk_scale<S>(pk_transform<T, LOG>(x[t0 + k], a.eps), d, divide);
      sm[pk_at(k + 1)] = s;
      if (scaled) scaled[c * a.n + t0 + k] = s;
    }
  }
  if (halo && tid == 0) sm[pk_at(0)] = t0 > 0 ? pk_scale<S>(pk_transform<T, LOG>(x[t0 - 1], a.eps), d, divide) : S(0);
  if (halo && tid == 1)
    sm[pk_at(len + 1)] = t0 + len < a.n ? pk_scale<S>(pk_transform<T, LOG>(x[t0 + len], a.eps), d, divide) : S(0);
}

template <typename T, bool LOG>
__global__ void __launch_bounds__(kPkThreads) k_peaks_summary(PeakArgs a) {
  using S = typename PkScaled<T, LOG>::type;
  __shared__ S sm[kPkLds];
  __shared__ int red[kPkThreads];
  QI_PK_WORKGROUP();
  for (int64_t tile = g0; tile < g1; ++tile) {
    QI_PK_TILE();
    pk_load_tile<T, LOG, S>(a, sm, c, t0, len, false, static_cast<S*>(a.scaled));
    __syncthreads();
    int e = len;  // samples of the leading run: the first k + 1 with s[k + 1] != s[k] (a NaN differs from everything)
#pragma unroll
    for (int v = kPkVec - 1; v >= 0; --v) {
      const int k = tid + v * kPkThreads;
      if (k + 1 < len && sm[pk_at(k + 2)] != sm[pk_at(k + 1)]) e = k + 1;
    }
    red[tid] = e;
    __syncthreads();
    for (int o = kPkThreads / 2; o > 0; o >>= 1) {
      if (tid < o) red[tid] = red[tid + o] < red[tid] ? red[tid + o] : red[tid];
      __syncthreads();
    }
    if (tid == 0) {
      const int lead = red[0];
      double* out = a.summ + (c * a.tiles + tile) * kPkSumm;
      out[0] = (double)sm[pk_at(1)];
      out[1] = lead < len ? (double)sm[pk_at(lead + 1)] : 0.0;
      out[2] = (double)lead;
    }
    __syncthreads();
  }
}

// WRITE = false: count the tile's peaks; WRITE = true: store them from the column the scan gave the tile
template <typename T, bool LOG, bool WRITE>
__global__ void __launch_bounds__(kPkThreads) k_peaks_pick(PeakArgs a) {
  using S = typename PkScaled<T, LOG>::type;
  __shared__ S sm[kPkLds];
  __shared__ int scan[kPkThreads];
  __shared__ int leave_k;      // tile index of the rising edge whose run leaves the tile, or -1
  __shared__ int64_t walk_j;   // where that run ends (the first sample that differs), or -1: it reaches the record's end
  __shared__ double walk_sj;   // the value there
  QI_PK_WORKGROUP();
  const double thr = a.rec[c * kPkRec + 1];
  const bool any_height = a.height_kind == QI_PEAK_HEIGHT_NONE;
  for (int64_t tile = g0; tile < g1; ++tile) {
    QI_PK_TILE();
    pk_load_tile<T, LOG, S>(a, sm, c, t0, len, true, nullptr);
    if (tid == 0) leave_k = -1;
    __syncthreads();
    const int k0 = tid * kPkVec;
    S w[kPkVec + 2];  // samples k0 - 1 .. k0 + 4
#pragma unroll
    for (int j = 0; j < kPkVec + 2; ++j) w[j] = sm[pk_at(k0 + j)];
    bool rise[kPkVec], differs[kPkVec];
    int e = kPkNone;  // the lane's first sample whose successor differs
#pragma unroll
    for (int v = kPkVec - 1; v >= 0; --v) {
      const int k = k0 + v;
      const int64_t i = t0 + k;
      differs[v] = k < len && i + 1 < a.n && w[v + 2] != w[v + 1];
      rise[v] = k < len && i >= 1 && i + 2 <= a.n && w[v] < w[v + 1];
      if (differs[v]) e = k;
    }
    scan[tid] = e;  // suffix minimum over the lanes
    __syncthreads();
    for (int o = 1; o < kPkThreads; o <<= 1) {
      const int t = tid + o < kPkThreads ? scan[tid + o] : kPkNone;
      __syncthreads();
      if (t < scan[tid]) scan[tid] = t;
      __syncthreads();
    }
    const int e_next = tid + 1 < kPkThreads ? scan[tid + 1] : kPkNone;
    __syncthreads();
    int npk = 0, leave_v = -1;
    int64_t ppos[2];  // (two rising edges of four samples at the most)
    double pval[2];
#pragma unroll
    for (int v = 0; v < kPkVec; ++v) {
      if (!rise[v]) continue;
      int kk = kPkNone;
#pragma unroll
      for (int v2 = kPkVec - 1; v2 >= v; --v2)
        if (differs[v2]) kk = k0 + v2;
      if (kk == kPkNone) kk = e_next;
      if (kk == kPkNone) {  // equal up to the tile's last sample and the one behind it
        if (t0 + len < a.n) leave_v = v;  // (else the run reaches the record's last sample: no peak)
        continue;
      }
      const double si = (double)w[v + 1], sj = (double)sm[pk_at(kk + 2)];
      if (sj < si && (any_height || si >= thr) && npk < 2) {
        ppos[npk] = (t0 + k0 + v + t0 + kk) >> 1;  // (i + j - 1) / 2 with j = t0 + kk + 1
        pval[npk] = si;
        ++npk;
      }
    }
    if (leave_v >= 0) leave_k = k0 + leave_v;
    __syncthreads();
    if (leave_k >= 0) {  // (uniform) the wave follows the next tiles' summaries, 64 tiles a step
      const double val = (double)sm[pk_at(leave_k + 1)];
      for (int64_t q0 = tile + 1;; q0 += kPkThreads) {
        const int64_t q = q0 + tid;
        bool stop = true;  // (a lane past the last tile never comes first: the last tile always stops the run)
        int64_t j = -1;
        double sj = 0.0;
        if (q < a.tiles) {
          const double* sq = a.summ + (c * a.tiles + q) * kPkSumm;
          const int64_t lead = (int64_t)sq[2];
          const int64_t lenq = a.n - q * kPkTile < kPkTile ? a.n - q * kPkTile : kPkTile;
          if (lead < lenq) {  // the run ends inside tile q
            j = q * kPkTile + lead;
            sj = sq[1];
          } else if (q + 1 < a.tiles) {  // tile q is all equal: does the next one go on?
            const double f = sq[kPkSumm];
            stop = f != val;
            j = (q + 1) * kPkTile;
            sj = f;
          }
        }
        const unsigned long long mask = __builtin_amdgcn_ballot_w64(stop);
        if (mask != 0ull) {
          if (tid == __builtin_ctzll(mask)) {
            walk_j = j;
            walk_sj = sj;
          }
          break;
        }
      }
      __syncthreads();
      if (leave_v >= 0 && walk_j >= 0) {
        const double si = (double)w[leave_v + 1];
        if (walk_sj < si && (any_height || si >= thr) && npk < 2) {
          ppos[npk] = (t0 + k0 + leave_v + walk_j - 1) >> 1;
          pval[npk] = si;
          ++npk;
        }
      }
    }
    scan[tid] = npk;  // inclusive prefix sum over the lanes
    __syncthreads();
    for (int o = 1; o < kPkThreads; o <<= 1) {
      const int t = tid >= o ? scan[tid - o] : 0;
      __syncthreads();
      scan[tid] += t;
      __syncthreads();
    }
    if constexpr (WRITE) {
      const int64_t col = a.cnt[c * a.tiles + tile] + scan[tid] - npk;
      for (int m = 0; m < npk; ++m) {
        if (col + m < a.capacity) {
          if (a.positions) a.positions[c * a.capacity + col + m] = ppos[m];
          if (a.values) a.values[c * a.capacity + col + m] = pval[m];
        }
      }
    } else if (tid == kPkThreads - 1) {
      a.cnt[c * a.tiles + tile] = scan[tid];
    }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(kPkThreads) k_peaks_scan(PeakArgs a) {
  __shared__ int64_t scan[kPkThreads];
  const int tid = threadIdx.x;
  const int64_t c = blockIdx.x;
  int64_t* cnt = a.cnt + c * a.tiles;
  int64_t carry = 0;
  for (int64_t b = 0; b < a.tiles; b += kPkThreads) {
    const int64_t mine = b + tid < a.tiles ? cnt[b + tid] : 0;
    scan[tid] = mine;
    __syncthreads();
    for (int o = 1; o < kPkThreads; o <<= 1) {
      const int64_t t = tid >= o ? scan[tid - o] : 0;
      __syncthreads();
      scan[tid] += t;
      __syncthreads();
    }
    if (b + tid < a.tiles) cnt[b + tid] = carry + scan[tid] - mine;
    carry += scan[kPkThreads - 1];
    __syncthreads();
  }
  if (tid == 0) a.counts[c] = carry;
}

template <typename T, bool LOG>
int launch_peaks(const PeakArgs& a, hipStream_t st) {
  const unsigned tiles_grid = (unsigned)(a.C * a.groups), rec_grid = (unsigned)a.C;
  k_peaks_extrema<T, LOG><<<tiles_grid, kPkThreads, 0, st>>>(a);
  QI_LAUNCH_CHECK();
  k_peaks_finish<T, LOG><<<rec_grid, kPkThreads, 0, st>>>(a);
  QI_LAUNCH_CHECK();
  k_peaks_summary<T, LOG><<<tiles_grid, kPkThreads, 0, st>>>(a);
  QI_LAUNCH_CHECK();
  k_peaks_pick<T, LOG, false><<<tiles_grid, kPkThreads, 0, st>>>(a);
  QI_LAUNCH_CHECK();
  k_peaks_scan<<<rec_grid, kPkThreads, 0, st>>>(a);
  QI_LAUNCH_CHECK();
  if ((a.positions || a.values) && a.capacity > 0) {
    k_peaks_pick<T, LOG, true><<<tiles_grid, kPkThreads, 0, st>>>(a);
    QI_LAUNCH_CHECK();
  }
  return QI_OK;
}

inline int64_t peak_tiles(int64_t n) { return ceil_div(n, kPkTile); }

}  // namespace

}  // namespace qi

using namespace qi;

extern "C" {

int64_t qi_peaks_scratch_bytes(int dtype, int64_t n_channels, int64_t n) {
  QI_TRY(require_records(dtype, n_channels, n));
  QI_REQUIRE(n < (1ll << 40) && n_channels < (1ll << 31) / ceil_div(peak_tiles(n), kPkGroup), "request too large");
  return (n_channels * peak_tiles(n) * (kPkPart + kPkSumm + 1) + n_channels * kPkRec) * (int64_t)sizeof(double);
}

int qi_find_peaks(int dtype, int device, const void* sig, int64_t n_channels, int64_t n, int scale, double eps, int height_kind,
                  double height, void* scaled, int64_t* positions, double* values, int64_t capacity, int64_t* counts,
                  void* scratch, int64_t scratch_bytes, qi_stream stream) {
  QI_REQUIRE(scale >= QI_PEAK_SIGMAX && scale <= QI_PEAK_LOG2MAX, "bad scaling %d", scale);
  QI_REQUIRE(height_kind >= QI_PEAK_HEIGHT_NONE && height_kind <= QI_PEAK_HEIGHT_BELOW_RAW_MAX, "bad height kind %d", height_kind);
  QI_REQUIRE(sig && counts && scratch, "null argument");
  QI_REQUIRE(capacity >= 0, "negative capacity %lld", (long long)capacity);
  QI_REQUIRE(capacity > 0 || !positions, "positions given with a capacity of 0");
  const int64_t need = qi_peaks_scratch_bytes(dtype, n_channels, n);
  if (need < 0) return (int)need;
  QI_TRY(require_scratch(scratch_bytes, need));
  const bool log = scale == QI_PEAK_LOG2 || scale == QI_PEAK_LOG2MAX;
  QI_REQUIRE(aligned(scratch, 8) && aligned(sig, elem_size(dtype)) && aligned(scaled, log ? 8 : elem_size(dtype)),
             "scratch must be aligned to 8 bytes, sig and scaled to their element size");
  PeakArgs a{};
  a.sig = sig;
  a.scaled = scaled;
  a.positions = positions;
  a.values = values;
  a.counts = counts;
  a.C = n_channels;
  a.n = n;
  a.tiles = peak_tiles(n);
  a.groups = ceil_div(a.tiles, kPkGroup);
  a.capacity = capacity;
  a.scale = scale;
  a.height_kind = height_kind;
  a.eps = host::eps_or_default(eps);
  a.height = height;
  a.part = static_cast<double*>(scratch);
  a.summ = a.part + a.C * a.tiles * kPkPart;
  a.cnt = reinterpret_cast<int64_t*>(a.summ + a.C * a.tiles * kPkSumm);
  a.rec = reinterpret_cast<double*>(a.cnt + a.C * a.tiles);
  DeviceGuard g(device);
  QI_REQUIRE(g.ok, "cannot select device %d", device);
  auto run = [&](auto zero) -> int {
    using T = decltype(zero);
    return log ? launch_peaks<T, true>(a, (hipStream_t)stream) : launch_peaks<T, false>(a, (hipStream_t)stream);
  };
  return by_dtype(dtype, run);
}

int qi_peaks_select_distance(const int64_t* positions, const double* values, int64_t count, int64_t distance, uint8_t* keep) {
  QI_REQUIRE(count >= 0, "bad candidate count %lld", (long long)count);
  QI_REQUIRE(distance >= 1, "`distance` must be greater or equal to 1");
  QI_REQUIRE(count == 0 || (positions && values && keep), "null argument");
  std::vector<int64_t> order((size_t)count);
  std::iota(order.begin(), order.end(), (int64_t)0);
  // ascending by value, equal values in index order; read from its end: the highest first, of equal ones the later first
  std::stable_sort(order.begin(), order.end(), [&](int64_t x, int64_t y) { return values[x] < values[y]; });
  for (int64_t i = 0; i < count; ++i) keep[i] = 1;
  for (int64_t r = count - 1; r >= 0; --r) {
    const int64_t j = order[(size_t)r];
    if (!keep[j]) continue;
    for (int64_t k = j - 1; k >= 0 && positions[j] - positions[k] < distance; --k) keep[k] = 0;
    for (int64_t k = j + 1; k < count && positions[k] - positions[j] < distance; ++k) keep[k] = 0;
  }
  return QI_OK;
}

}  // extern "C"
