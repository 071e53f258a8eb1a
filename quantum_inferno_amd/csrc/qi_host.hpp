// Host side of libqi_tfr.so shared by its translation units: the plan object, the hipFFT plan cache, the stage profiler
// and the functions that cross files (qi_plan_build.hip: tables of a plan; qi_run.hip: launch sequences of the engines;
// qi_api.hip: the plan C ABI; qi_api_ops.hip: the plan-less C ABI).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <mutex>
#include <new>
#include <tuple>
#include <vector>

#include <cstdlib>

#include "qi_common.hpp"
#include "qi_native.hpp"

namespace qi {

struct DeviceGuard {
  int prev = -1;
  bool ok = true;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) ok = hipSetDevice(dev) == hipSuccess;
  }
  ~DeviceGuard() {
    int cur = -1;
    if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
  }
};

// The element type of a C ABI call as a type: calls f(T{}) with T = double for QI_F64 and float otherwise (the entry points
// check the dtype first) -- a generic lambda `[&](auto t) { using T = decltype(t); ... }` states its argument list once.
template <typename F>
inline auto by_dtype(int dtype, F&& f) {
  return dtype == QI_F64 ? f(double{}) : f(float{});
}
inline size_t elem_size(int dtype) { return dtype == QI_F64 ? 8 : 4; }
// p lies on a multiple of `size` bytes (a power of two); a null pointer counts as aligned: optional arguments pass
inline bool aligned(const void* p, size_t size) { return (reinterpret_cast<uintptr_t>(p) & (size - 1)) == 0; }

// ---- the opening of a plan-less record call (records [n_channels][n]; qi_filter, qi_peaks, qi_resample, qi_calculus): each
// sets the last-error text and returns QI_ERR_ARG as QI_REQUIRE does, for the caller's QI_TRY.  What depends on an op's own
// grid arithmetic ("request too large") or tables stays in its file.
// min_records 0: an op that takes an empty batch as a successful no-op
inline int require_records(int dtype, int64_t n_channels, int64_t n, int64_t min_records = 1) {
  QI_REQUIRE(dtype == QI_F32 || dtype == QI_F64, "bad dtype %d", dtype);
  QI_REQUIRE(n_channels >= min_records, "bad record count %lld", (long long)n_channels);
  QI_REQUIRE(n >= 1, "bad record length %lld", (long long)n);
  return QI_OK;
}
inline int require_scratch(int64_t scratch_bytes, int64_t need) {
  QI_REQUIRE(scratch_bytes >= need, "scratch of %lld bytes, %lld needed", (long long)scratch_bytes, (long long)need);
  return QI_OK;
}
// timestamps: a row per record (stride n), or stride 0 -- one row shared by all records, or none where an op can do without;
// `name`: the argument, for the message
inline int require_timestamp_stride(const char* name, int64_t stride, int64_t n) {
  QI_REQUIRE(stride == 0 || stride == n, "%s must be 0 (shared timestamps or none) or n, got %lld", name, (long long)stride);
  return QI_OK;
}

// ---- hipFFT plan cache (one per qi_plan, plus a process-wide one for the plan-less STFT entry) ----
struct FftCache {
  using Key = std::tuple<int, int64_t, int64_t, int64_t>;  // hipfftType, length, batch, distance between transforms
  std::map<Key, hipfftHandle> plans;
  // One work area of work_bytes per stream: the handles are shared, and transforms queued on two streams run side by side --
  // with one area for all of them the later one overwrote the intermediate rows of the earlier one.
  std::map<hipStream_t, void*> work;
  size_t work_bytes = 0;
  std::vector<void*> retired;  // outgrown work areas, freed with the cache

  int get(hipfftType type, int64_t len, int64_t batch, hipfftHandle* out, int64_t dist = 0) {
    if (dist <= 0) dist = len;
    Key k{(int)type, len, batch, dist};
    auto it = plans.find(k);
    if (it != plans.end()) {
      *out = it->second;
      return QI_OK;
    }
    QI_REQUIRE(len > 0 && len < (1ll << 31) && batch > 0 && batch < (1ll << 31), "fft size out of range");
    hipfftHandle h;
    QI_FFT(hipfftCreate(&h));
    QI_FFT(hipfftSetAutoAllocation(h, 0));
    int nn[1] = {(int)len};
    size_t ws = 0;
    QI_REQUIRE(dist >= len && dist < (1ll << 31), "fft distance out of range");
    if (dist == len) QI_FFT(hipfftMakePlanMany(h, 1, nn, nullptr, 1, (int)len, nullptr, 1, (int)len, type, (int)batch, &ws));
    else QI_FFT(hipfftMakePlanMany(h, 1, nn, nn, 1, (int)dist, nn, 1, (int)dist, type, (int)batch, &ws));  // (in place, padded rows)
    if (ws > work_bytes) {
      // growing the work areas happens while a plan warms up, never in steady state.  No synchronisation: the old areas
      // stay allocated (transforms already queued keep using them) until the cache is cleared; `bind` makes the new ones
      for (auto& kv : work) retired.push_back(kv.second);
      work.clear();
      work_bytes = ws;
    }
    plans[k] = h;
    *out = h;
    return QI_OK;
  }
  // Point handle `h` at stream `st` and at that stream's work area (made at the stream's first transform), for the
  // execution the caller queues next.  The caller holds whatever lock guards the cache until that execution is queued.
  int bind(hipfftHandle h, hipStream_t st) {
    if (work_bytes > 0) {
      void*& w = work[st];
      if (!w) QI_HIP(hipMalloc(&w, work_bytes));
      QI_FFT(hipfftSetWorkArea(h, w));
    }
    QI_FFT(hipfftSetStream(h, st));
    return QI_OK;
  }
  void clear() {
    for (auto& kv : plans) hipfftDestroy(kv.second);
    plans.clear();
    for (auto& kv : work) (void)hipFree(kv.second);
    for (void* w : retired) (void)hipFree(w);
    retired.clear();
    work.clear();
    work_bytes = 0;
  }
};

// in-place double-precision transforms of `batch` rows of `len` points that start `dist` elements apart
int fft_z2z_rows(FftCache& fc, double2* data, int64_t len, int64_t dist, int64_t batch, int dir, hipStream_t st);
template <typename T>
int fft_c2c(FftCache& fc, cplx<T>* data, int64_t len, int64_t batch, int dir, hipStream_t st);
template <>
int fft_c2c<float>(FftCache& fc, float2* data, int64_t len, int64_t batch, int dir, hipStream_t st);
template <>
int fft_c2c<double>(FftCache& fc, double2* data, int64_t len, int64_t batch, int dir, hipStream_t st);
template <typename T>
int fft_r2c(FftCache& fc, T* in, cplx<T>* out, int64_t len, int64_t batch, hipStream_t st);
template <>
int fft_r2c<float>(FftCache& fc, float* in, float2* out, int64_t len, int64_t batch, hipStream_t st);
template <>
int fft_r2c<double>(FftCache& fc, double* in, double2* out, int64_t len, int64_t batch, hipStream_t st);
template <typename T>
int fft_c2r(FftCache& fc, cplx<T>* in, T* out, int64_t len, int64_t batch, hipStream_t st);
template <>
int fft_c2r<float>(FftCache& fc, float2* in, float* out, int64_t len, int64_t batch, hipStream_t st);
template <>
int fft_c2r<double>(FftCache& fc, double2* in, double* out, int64_t len, int64_t batch, hipStream_t st);

// ---- optional per-stage timing with HIP events on the caller's stream (bench.py's roofline leg) ----
struct Profiler {
  static constexpr int kStages = QI_STAGE_COUNT;
  bool on = false;
  uint32_t mask = ~0u;  // stages that are timed (bit = stage)
  struct Span {
    int a, b;  // indices into `used`
    int stage;
  };
  std::vector<Span> spans;
  std::vector<hipEvent_t> used;  // events recorded since the last read
  std::vector<hipEvent_t> pool;
  int cur = -1;
  int last = -1;  // the event that closed the previous span, while nothing has been launched since: the next
                  // span starts on it instead of recording another one (every record is a bubble in the stream)

  int record(hipStream_t st) {
    hipEvent_t e = nullptr;
    if (!pool.empty()) {
      e = pool.back();
      pool.pop_back();
    } else if (hipEventCreate(&e) != hipSuccess) {
      return -1;
    }
    (void)hipEventRecord(e, st);
    used.push_back(e);
    return (int)used.size() - 1;
  }
  int period = 1;      // time every period-th transform call only (the others run without any event)
  int64_t tick = 0;
  bool sampled = true;
  void unchain() {  // called at every transform entry point
    last = -1;
    sampled = period <= 1 || tick % period == 0;
    ++tick;
  }
  void unchain_span() { last = -1; }  // the next span is on another stream: do not share an event with it
  void begin(hipStream_t st, int stage) {
    cur = -1;
    if (!on || !sampled || !((mask >> stage) & 1u)) {
      last = -1;
      return;
    }
    cur = last >= 0 ? last : record(st);
  }
  void end(int stage, hipStream_t st) {
    last = -1;
    if (!on || cur < 0) return;
    const int b = record(st);
    if (b >= 0) {
      spans.push_back({cur, b, stage});
      last = b;
    }
    cur = -1;
  }
  void read(double* ms, int64_t* count) {
    for (int i = 0; i < kStages; ++i) {
      ms[i] = 0.0;
      count[i] = 0;
    }
    for (auto& s : spans) {
      float t = 0.f;
      if (hipEventSynchronize(used[s.b]) == hipSuccess && hipEventElapsedTime(&t, used[s.a], used[s.b]) == hipSuccess) {
        ms[s.stage] += t;
        count[s.stage] += 1;
      }
    }
    for (auto e : used) pool.push_back(e);
    used.clear();
    spans.clear();
    cur = last = -1;
  }
  void clear() {
    double ms[kStages];
    int64_t c[kStages];
    read(ms, c);
    for (auto e : pool) (void)hipEventDestroy(e);
    pool.clear();
  }
};

// ---- device tables of the host code --------------------------------------------------------------------------------------
// free a device table and forget it
template <typename P>
inline void free_device(P*& ptr) {
  if (ptr) (void)hipFree(ptr);
  ptr = nullptr;
}
// upload a host table to a freshly allocated device table: the size comes from the vector
template <typename P, typename X>
inline int upload_table(P** dst, const std::vector<X>& v) {
  QI_HIP(hipMalloc((void**)dst, v.size() * sizeof(X)));
  QI_HIP(hipMemcpy(*dst, v.data(), v.size() * sizeof(X), hipMemcpyHostToDevice));
  return QI_OK;
}
// a device buffer that lives as long as one table build: freed on every way out
template <typename X>
struct DeviceTemp {
  X* ptr = nullptr;
  DeviceTemp() = default;
  DeviceTemp(const DeviceTemp&) = delete;
  DeviceTemp& operator=(const DeviceTemp&) = delete;
  ~DeviceTemp() { free_device(ptr); }
};

// hipFFT plans of the plan-less entry points (STFT, Welch, sliding STFT, ShannonFFT): per device, under one mutex
extern std::mutex g_stft_mu;
extern std::map<int, FftCache> g_stft_fft;
const char* last_error();

}  // namespace qi

using namespace qi;  // (internal header of the host translation units only)

// qi_cwt_stx: the CWT run leaves its block launch and its tail to the Stockwell run, which issues them together with
// its own (one launch each: the two block launches share the forward transform of every block)
struct FusedCarry {
  bool active = false;
  size_t ws_used = 0;  // bytes of the workspace the CWT run's scratch occupies (kept until its deferred launches ran)
  native::BlockArgs<float> blk{};
  int demod = 0;
  int64_t ct = 0;
  native::TailCall<float> tail;
  bool has_zoom = false;  // the gather / coarse / interpolation launches of the CWT run are deferred as well
  native::ZoomArgs<float> zoom{};
};

struct qi_plan {
  qi_plan_desc d{};
  int64_t n = 0;
  int64_t L = 0;  // zero-padded length of the linear (styx_cwt) correlation
  void* bank[2] = {nullptr, nullptr};
  int32_t nb[2] = {0, 0};
  int64_t* d_stx_idx = nullptr;
  double* d_stx_coef = nullptr;
  int32_t nb_stx = 0;
  char* ws = nullptr;
  size_t ws_bytes = 0;
  FftCache fft;
  Profiler prof;
  // native engine: per transform kind (0 styx bank, 1 atoms bank, 2 Stockwell) the band descriptors
  struct NativeGroup {  // bands launched together: their wide members share one intermediate buffer
    int32_t first = 0, count = 0;    // range of d_bands
    int32_t gen_first = 0, ngen = 0; // range of d_gen_list (indices relative to `first`)
  };
  struct NativeTable {
    bool ready = false;
    int64_t Lf = 0;
    int32_t nbands = 0, ngen = 0, imd_slots = 0;
    native::BandDesc* d_bands = nullptr;  // grouped order
    int32_t* d_gen_list = nullptr;
    std::vector<NativeGroup> groups;
    void* Hc = nullptr;
    void* Hfull = nullptr;
    native::BandDesc* d_zoom = nullptr;  // bands produced by the zoom engine (qi_zoom.hip), by level
    int32_t* d_zoom_plane_band = nullptr;  // owner band of every coarse plane
    std::vector<std::pair<int32_t, int32_t>> h_zoom;  // (panel row, level) of the zoom bands
    std::vector<int32_t> h_rows;                      // panel rows of the pass-2 bands
    std::vector<int32_t> h_row_mode;                  // ... 0 one-pass loader, 1 general (same order)
    std::vector<int32_t> h_z64;                       // panel rows of the float64 zoom bands, in the order of d_z64
    int32_t nzoom = 0, zoom_count[native::kZoomClasses] = {0, 0, 0, 0, 0, 0, 0};
    // record-spectrum bins the zoom bands read (signed, modulo Lf; a Stockwell row reads k + shift, negative near DC):
    // the most negative and the most positive one (x_lo > x_hi: no zoom band)
    int64_t x_lo = 0, x_hi = -1;
    int64_t zoom_planes = 0;  // 4096-sample planes of coarse storage per record
    int zoom_max_level = 0;
    // float64 zoom (qi_zoom64.hip): the narrow-spectrum bands of a float64 table, by coarse-grid level
    native::BandDesc* d_z64 = nullptr;
    int32_t nz64 = 0, z64_first[native::kZ64Levels] = {}, z64_count[native::kZ64Levels] = {};
    // ... the bands of the three coarsest grids by class of the fine kernel (k_z64_fine: grid, interpolator length); ranges of
    // d_z64, a class's bands lie inside its level's range
    int32_t zf_first[native::kZ64FineClasses] = {}, zf_count[native::kZ64FineClasses] = {};
    double2* d_z64_lane_ph = nullptr;  // [nz64][65] carrier factors of the lanes and the step, per band of d_z64 (Gabor kinds)
    double2* d_z64_wave_ph = nullptr;  // [Lf / kZ64FineWave] carrier factors of the waves
    void release() {
      free_device(d_z64);
      free_device(d_z64_lane_ph);
      free_device(d_z64_wave_ph);
      free_device(d_zoom);
      free_device(d_zoom_plane_band);
      free_device(d_bands);
      free_device(d_gen_list);
      free_device(Hc);
      free_device(Hfull);
      *this = NativeTable();
    }
  } nat[4];  // 0 styx bank (linear, Lf = 2n), 1 atoms bank (circular), 2 Stockwell, 3 styx short-atom bands (circular n)
  // block engine (qi_block.hip): bands whose atoms reach at most 1024 samples, per transform kind, in three
  // groups by reach (256, 512, 1024 samples)
  struct BlockTable {
    bool ready = false;
    int demod = 0;
    void* bank = nullptr;  // [rows][kBlk] complex filter spectra
    int32_t rows = 0;
    // Work items (one per workgroup, most expensive first) in two cuts: [0] few bands per workgroup -- many workgroups,
    // for calls with one or two records --, [1] many bands per workgroup -- fewer forward transforms of the same block
    // and fewer per-time planes, for batches that fill the chip anyway.
    struct ItemList {
      void* d_bands = nullptr;  // native::BlockBandT<T>[]: all reach groups, group by group (cut 1 keeps some bands on long blocks)
      void* d_demod_pow = nullptr;  // float64 Stockwell tables: [bands][16] demodulation factors (BlockArgs::demod_pow)
      void* d_gauss_w = nullptr;    // float64 tables: [bands][kBlk] real Gaussian filter weights (BlockArgs::gauss_w)
      std::vector<std::pair<int32_t, int32_t>> h_bands;  // (panel row, blocks) of the block bands
      struct Route {  // what qi_plan_band_route reports of a block band (host copy of its descriptor's path fields)
        int32_t out_band, wq, analytic, narrow, nowrap;
      };
      std::vector<Route> h_route;
      native::BlockItem* d_items = nullptr;
      int32_t nitems = 0, nplanes = 0;
      int32_t nlong = 0;        // long-block items, at the front of the list
      int32_t nedge_items = 0;  // edge pieces of the split bands, appended to the item list (styx bank)
      bool edge_merged = false;  // one edge item per block for all split bands (k_block_edge) instead of one per band and block
      std::vector<native::BlockItem> h_items;  // host copy of d_items (the joint launch list is made from it)
      std::vector<std::pair<int32_t, int32_t>> h_groups;  // (first band, bands) of every reach group in d_bands
    } var[2];
    // qi_cwt_stx below batch_from records (native_joint_deal): this table's items of the joint dealing (build_joint_items,
    // on first use).  A copy of var[0] -- the same bands, the tables borrowed from it -- with its own d_items / h_items,
    // nitems, nplanes, nlong and nedge_items; a complete item list of the table, so it also serves a launch of its own.
    ItemList joint;
    int64_t max_blocks = 0;  // partial slots a band row needs
    void release() {
      free_device(bank);
      free_device(joint.d_items);
      for (auto& v : var) {
        free_device(v.d_bands);
        free_device(v.d_demod_pow);
        free_device(v.d_gauss_w);
        free_device(v.d_items);
      }
      *this = BlockTable();
    }
  } blk[3];
  // qi_cwt_stx: the settled tile (records per joint tile) of the last request shape; any table change bumps table_gen
  struct {
    int64_t C = -1, tile = 0;
    unsigned flags = 0;
    uint64_t gen = 0;
  } tile_cache;
  uint64_t table_gen = 1;
  int native_block = 1;        // use the block engine for short-atom bands (0: two-pass paths only)
  // qi_cwt_stx: the CWT leaves the zero-padded spectra of the records at the start of the scratch
  const void* shared_sig = nullptr;
  int64_t shared_C = 0;
  bool shared_valid = false;
  int32_t* d_band_slots[3][2] = {};  // per table kind and item cut: partial slots each band's engine writes
  int native_zoom = 1;         // use the zoom engine for narrow-spectrum bands (0: one-pass loader of pass 2)
  int native_zoom_max_level = 3;  // finest coarse grid the zoom engine may use (level 4 costs more in the coarse stage than two-pass saves)
  float* d_zoom_w[native::kZoomClasses] = {};  // interpolation weights per class
  int native_z64 = 1;      // float64: narrow-spectrum bands at the decimated rate (coarse inverse FFT + 16-tap interpolation)
  double* d_z64_w[native::kZ64Levels] = {};  // interpolation weights per coarse-grid level
  double* d_z64f_w[native::kZ64FineClasses] = {};  // lane weights per class of the fine kernel
  double2* d_demod_t1 = nullptr;  // float64 block engine, Stockwell demodulation: exp(-2 pi i 1024 j / n), j < n / 1024
  double2* d_demod_t2 = nullptr;  // ... exp(-2 pi i j / n), j < 1024
  int native_z64_fine = 1;  // 0: every level on k_z64_interp (windows through LDS), as in round 3
  // Stockwell bands that no native engine takes at this record length (the two-pass kernels run 2^20 / 2^21 samples only): when
  // they are the last rows of the table -- the top band of an order-1 or order-2 table, whose frequency window is cut at the
  // Nyquist bins -- the native run leaves them out and a pass of the hipFFT engine over just these rows follows it
  // (run_stx_leftover); any other case hands the whole table to the hipFFT engine as before
  int32_t stx_left_lo = -1, stx_left_n = 0;
  // small-record engine (qi_small.hip): power-of-two records of 2^10 .. 2^13 samples below native_min_log2n on an AUTO plan, per table
  // when its transform (2n points for the styx bank, n otherwise) fits the LDS; reads the hipFFT engine's tables
  void* small_tw = nullptr;    // exp(2 pi i k / 2n), k < n / 8, in the plan's precision (float64 values rounded once); null: no table is small
  int small_chunk_bands = 2;   // bands per workgroup (band chunk): the chunk count is a property of the table and the workspace, never of the call
  int small_joint = 2;         // qi_cwt_stx with both tables small: 0 two separate runs, 1 one forward launch for both, 2 and one tail launch
  int native_min_log2n = 14;    // shortest power-of-two record the zoom / block engines are tried on (below: the hipFFT engine).
                                // float32: 2^14 (round 5: 54 / 69 us per call against 97 / 230 on the hipFFT engine at orders 3 / 12);
                                // float64: 2^15 (at 2^14 the float64 zoom's small grids go through hipFFT launch by launch: slower)
  int native_blk64_narrow = 1;  // float64 block engine: bands whose weights above 2^-52 of the peak span <= 256 bins skip the first pass of the inverse transform (sparse_head16)
  int native_blk64_wtab = 1;  // float64 block engine: Gaussian filter weights from a plan-time table instead of sixteen exp2 per band and thread
  int native_z64_block_from = 4;  // a band that needs coarse-grid level >= this (0-based) goes to the block engine when its atom is short enough
  int native_z64_coarse = 3;  // coarse-grid levels whose coarse stage is one launch of in-LDS plane transforms (the finer ones: hipFFT)
  int native_f64 = 1;      // float64 plans run on the native engines in double arithmetic (2^20 / 2^21-point transforms)
  hipStream_t side = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  // split bands of the styx bank (atoms longer than the record): zoom engine + edge pieces, see split_taper
  int native_split = 1;        // 0: such bands stay on the two-pass kernels
  int64_t native_split_e = 1024;  // taper length in samples (512, 1024 or 2048: the edge pieces' reach group)
  void* split_bank = nullptr;  // [nsplit][2][kBlk] filter spectra of the edge pieces
  int32_t* d_split_bands = nullptr;  // [nsplit] panel rows of the split bands
  std::vector<int32_t> h_split_bands;
  int32_t nsplit = 0;
  FusedCarry carry;
  // joint block launch of qi_cwt_stx (styx + Stockwell tables), built on first use: [0], [1] the tables' item lists of that cut
  // paired chunk by chunk; [kDualJoint] cut 0 dealt table-first (BlockTable::joint)
  static constexpr int kDualJoint = 2;
  native::DualItem* d_dual[3] = {nullptr, nullptr, nullptr};
  int32_t n_dual[3] = {0, 0, 0};
  int32_t n_dual_long[3] = {0, 0, 0};  // long-block items at the front of d_dual
  bool dual_valid[3] = {false, false, false};
  int native_fuse = 4;         // qi_cwt_stx: 1 the block launches and the tails of the two transforms go out back to back, 2 as one
                               // launch each, 3 also the gather and the coarse stage of the zoom engine, 4 and its interpolation
  native::EdgeBand* d_edge = nullptr;  // short-atom bands of table 3
  int32_t nedge = 0;
  int64_t edge_wmax = 0;
  int native_short = 1;  // evaluate short-atom styx bands circularly at length n (0: everything at 2n)
  int native_debug = 0;
  int native_fwd = 1;          // forward transform of the records on the native kernels (0: hipFFT)
  int native_fwd_low = 1;      // ... only the bins near DC when nothing reads the others (forward_low); 0: always every bin
  int native_joint_deal = 1;   // qi_cwt_stx below batch_from records: the joint block launch deals a reach group's styx and Stockwell
                               // bands as one sequence (build_joint_items); 0: the tables' own item lists, paired chunk by chunk
  int native_zoom_merge = 1;   // qi_cwt_stx below batch_from records: a table's zoom classes of equal zoom_steps run as one merged
                               // row with one per-time plane (plan_zoom_rows); 0: a row (and a plane) per class
  unsigned long long* stamps = nullptr;  // diagnostic builds: phase cycle counters of the last pass-2 launch
  unsigned long long* blk_stamps = nullptr;  // idem, last block launch
  int native_group = 0;        // wide bands per launch group (0: all in one group)
  int native_rows = 16;        // consecutive time residues (rows) per pass-2 workgroup: 8 or 16
};

namespace qi {
namespace host {

inline size_t align_up(size_t v, size_t a = 256) { return (v + a - 1) / a * a; }
// qi_host_util.hip: `count` 8-byte host values (doubles and offsets alike, bit for bit) to device memory as kernel arguments,
// 256 per launch: stream-ordered, and the caller's array is free at return
int put_words(void* dst, const void* src, int64_t count, hipStream_t st);
// a request (qi_tfr_out, the plan-less entry points) that leaves power_scale / eps at zero asks for the defaults
inline double power_scale_or_default(double power_scale) { return power_scale == 0.0 ? 1.0 : power_scale; }
inline double eps_or_default(double eps) { return eps == 0.0 ? 2.220446049250313e-16 : eps; }
enum class Kind { Linear, Circular, Stockwell };
// Host sanitizer build (tests/sanitize: the library's host code on a stand-in HIP runtime under AddressSanitizer /
// UBSan): every region a run carves out of the plan's scratch is reported here and checked -- inside the workspace, and
// disjoint from every other live region (`shared`: the spectra a joint qi_cwt_stx tile's second run takes over from its
// first).  The product build compiles these away.
#ifdef QI_HOST_SANITIZE
void layout_begin(const qi_plan* p, const char* run, bool keep_previous);
void layout_note(const qi_plan* p, const char* what, const void* ptr, size_t bytes, bool shared = false);
#define QI_LAYOUT_BEGIN(p, run, keep) ::qi::host::layout_begin(p, run, keep)
#define QI_LAYOUT_NOTE(p, what, ptr, bytes, ...) ::qi::host::layout_note(p, what, ptr, bytes, ##__VA_ARGS__)
#else
#define QI_LAYOUT_BEGIN(p, run, keep) ((void)0)
#define QI_LAYOUT_NOTE(p, what, ptr, bytes, ...) ((void)0)
#endif
// order of the zoom classes in a table's band list (classes 6, 5 and 0 share the coarsest grid)
constexpr int kZoomListOrder[native::kZoomClasses] = {6, 5, 0, 1, 2, 3, 4};

// ---- qi_plan_build.hip: the tables of a plan ---------------------------------------------------------------------------
bool native_len_ok(int64_t Lf);
bool native_wanted(const qi_plan* p, int kind);
// Low-bins forward transform (native::fwd_low_bins): a property of the plan's tables.  table_low_bins: the power of two K
// with every spectrum read of table `kind` in (-K, K), or 0 when the table needs the whole spectrum; forward_low: every
// native table set on the plan allows it, so qi_cwt, qi_stx and qi_cwt_stx all take the same forward path.
int64_t table_low_bins(const qi_plan* p, int kind);
bool forward_low(const qi_plan* p);
int batch_from(const qi_plan* p);
// nothing half-built stays behind: a ready table without its block / split producers would leave panel rows unwritten
void release_styx_extras(qi_plan* p);  // the split and short-atom (edge) members of the styx bank
void drop_gabor_tables(qi_plan* p, int bank);
void drop_stx_tables(qi_plan* p);
void drop_band_slots(qi_plan* p, int kind);
// the four parameter arrays of a Gabor bank as one host table [4][B] (p_re | p_im | omega | amp) and its device copy
int upload_atom_params(int32_t B, const double* p_re, const double* p_im, const double* omega, const double* amp,
                       std::vector<double>* host, DeviceTemp<double>* d_par);
template <typename T>
int build_native_bank(qi_plan* p, int bank, int32_t B, const double* d_par, const double* h_par, hipStream_t st);
template <typename T>
int build_bank(qi_plan* p, int bank, int32_t B, const double* d_par, hipStream_t st);
// the Stockwell table of a plan (native classification, block picks; nat[2] / blk[2]); `sigma`, `shift_index`: host [B]
int build_stx_tables(qi_plan* p, int32_t B, const int64_t* shift_index, const double* sigma, const std::vector<double>& coef);
// Table-first dealing of the joint block launch (item cut 0 of the styx and the Stockwell table, both ready): fills
// blk[0].joint and blk[2].joint and returns the launch's band items in generation order (no edge items; the caller sorts)
int build_joint_items(qi_plan* p, std::vector<native::DualItem>* dual);

// the small-record engine's rule: does table `kind` (0 styx bank, 1 atoms bank, 2 Stockwell) of this plan run on it?  (A
// property of the plan alone; on_small: ... and the table is set)
bool small_wanted(const qi_plan* p, int kind);
bool on_small(const qi_plan* p, int kind);
int build_small_twiddles(qi_plan* p);

// ---- qi_run.hip: launch sequences ----------------------------------------------------------------------------------------
template <typename T>
int run_transform(qi_plan* p, Kind kind, const void* sig_v, int64_t C, const qi_tfr_out* out, hipStream_t st);
template <typename T>
int run_native(qi_plan* p, int kind, const void* sig_v, int64_t C, const qi_tfr_out* out, hipStream_t st,
               bool may_share = false, FusedCarry* defer = nullptr, FusedCarry* finish = nullptr, size_t* probe = nullptr);
template <typename T>
int run_stx_leftover(qi_plan* p, const void* sig, int64_t C, const qi_tfr_out* out, hipStream_t st);
// The small-record engine on one table, or on two tables of the same records (qi_cwt_stx: one forward launch for both).
// *ran = false, nothing launched: the workspace does not hold one record's scratch -- the caller runs the hipFFT engine.
template <typename T>
int run_small(qi_plan* p, int njobs, const int* kinds, const qi_tfr_out* const* outs, const void* sig_v, int64_t C, hipStream_t st,
              bool* ran);
int run_native64(qi_plan* p, int kind, const void* sig_v, int64_t C, const qi_tfr_out* out, hipStream_t st);
int flush_carry(qi_plan* p, FusedCarry* c, hipStream_t st);
// per-time planes of table `kind` (0 styx, 2 Stockwell) in a joint one-record qi_cwt_stx call: two-pass chunks, block planes
// of the dealing in effect, zoom rows (0: the plan runs no joint call); builds the joint item lists when they are the ones used
int64_t joint_planes(qi_plan* p, int kind);

}  // namespace host
}  // namespace qi
