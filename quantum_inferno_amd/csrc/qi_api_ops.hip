// C ABI of libqi_tfr.so, plan-less entry points: STFT / Welch / sliding STFT, tfr_info on caller panels, the 1-D Shannon
// family, widening and log2 helpers, Gabor atoms.
#include "qi_host.hpp"
#include "qi_array.h"
#include "qi_windows.h"
#include "qi_lags.h"
#include "qi_timebeam.h"
#include "qi_squeeze.h"

using namespace qi;
using qi::host::align_up;

extern "C" int64_t qi_stft_segments(int64_t n, int64_t seg, int64_t hop);

namespace {

// ---- the STFT family's two engines: the fused kernels (qi_stft_fused.hip), or frames -> hipFFT -> finish (qi_stft_hipfft.hip) ----
// the fused kernels switched off (development switch, read once per process)
bool stft_fused_off() {
  static const bool off = tune_env("QI_STFT_FUSED") && atoi(tune_env("QI_STFT_FUSED")) == 0;
  return off;
}

// `fused` where the fused kernels take the geometry; when it answers QI_ERR_UNSUPPORTED (a device with less LDS per workgroup
// than the tile needs, an inverse whose halo leaves no hop to own) and everywhere else the three-kernel sequence `hipfft`
template <typename Fused, typename Hipfft>
int fused_or_hipfft(bool takes, Fused&& fused, Hipfft&& hipfft) {
  if (!stft_fused_off() && takes) {
    const int rc = fused();
    if (rc != QI_ERR_UNSUPPORTED) return rc;
  }
  return hipfft();
}

// Scratch of the three-kernel sequence: [C][rows][nfft] reals (frames, or the inverse's slices) | [C][rows][nfft / 2 + 1]
// spectra.  The byte counts a caller is told and the pointers the sequences use both come from here.
struct FftScratch {
  size_t frames = 0, spectra, total;  // byte offsets of the two regions, and the size
  FftScratch(int dtype, int64_t C, int64_t rows, int64_t nfft) {
    const size_t e = dtype == QI_F64 ? 8 : 4;
    spectra = align_up((size_t)C * rows * nfft * e);
    total = spectra + align_up((size_t)C * rows * (nfft / 2 + 1) * 2 * e);
  }
};

// a transform (fft_r2c, fft_c2r) on the plan cache the plan-less entry points share per device, under its mutex
template <typename Transform>
int locked_fft(int device, Transform&& transform) {
  std::lock_guard<std::mutex> lk(g_stft_mu);
  return transform(g_stft_fft[device]);
}

// the hipFFT engine on a request: its frames -> hipFFT -> `finish` on the spectra [C][nseg][nfft / 2 + 1]
template <typename T, typename Finish>
int via_hipfft(int device, const StftRequest& rq, const T* sig, const T* window, char* scratch, hipStream_t st, Finish&& finish) {
  const FftScratch l(sizeof(T) == 8 ? QI_F64 : QI_F32, rq.C, rq.nseg, rq.nfft);
  T* frames = reinterpret_cast<T*>(scratch + l.frames);
  cplx<T>* F = reinterpret_cast<cplx<T>*>(scratch + l.spectra);
  QI_TRY(launch_hipfft_frames<T>(rq, sig, window, frames, st));
  QI_TRY(locked_fft(device, [&](FftCache& fc) { return fft_r2c<T>(fc, frames, F, rq.nfft, rq.C * rq.nseg, st); }));
  return finish(F);
}

// ... finished by the transpose into the panels: Z and / or the real panel R of rq.real_kind
template <typename T>
int stft_hipfft(int device, const StftRequest& rq, const T* sig, const T* window, cplx<T>* Z, T* R, char* scratch, hipStream_t st) {
  return via_hipfft<T>(device, rq, sig, window, scratch, st,
                       [&](const cplx<T>* F) { return launch_hipfft_transpose<T>(rq, F, Z, R, st); });
}

// Scratch of qi_stft_out: [0] the three-kernel path's frames and spectra (qi_stft_scratch_bytes) | [1] the panel when the
// caller keeps none | [2] band partials | [3] statistics partials -- [2] and [3] hold either engine's: per segment group of
// the fused kernel, or per kEpiSpan columns of k_epilogue.  A pooling range call (qi_stft_out_range) has smaller groups --
// more slots -- and, for a pooled maximum from the fused kernel, [4] the groups' maxima of every bin in the record's type.
struct StftOutLayout {
  size_t panel, part_band, part_stat, part_max, total;
};
StftOutLayout stft_out_layout(int dtype, int64_t C, int64_t nseg, int64_t seg, int64_t hop, int64_t nfft, bool want_coef,
                              int64_t pool_factor = 0, bool pool_max = false) {
  const int64_t nf = nfft / 2 + 1;
  const size_t e = dtype == QI_F64 ? 8 : 4;
  int64_t slots = ceil_div(nseg, kEpiSpan);
  const bool fused = stft_fused_supported(dtype, seg, hop, nfft);
  if (fused) slots = std::max(slots, stft_fused_groups(dtype, nfft, nseg, pool_factor));
  StftOutLayout l;
  l.panel = FftScratch(dtype, C, nseg, nfft).total;
  l.part_band = l.panel + (want_coef ? 0 : align_up((size_t)C * nf * nseg * 2 * e));
  l.part_stat = l.part_band + align_up((size_t)C * slots * nf * 8);
  l.part_max = l.part_stat + align_up((size_t)C * slots * 24);
  l.total = l.part_max + (fused && pool_factor > 0 && pool_max ? align_up((size_t)C * slots * nf * e) : 0);
  return l;
}

// The record samples [*lo, *hi) inside [0, n_total) that the segments first .. first + count - 1 cover (segment m: the samples
// [m hop - seg / 2, m hop - seg / 2 + seg)); *hi <= *lo: none, the range lies in the zero extension
void stft_range_interval(int64_t n_total, int64_t seg, int64_t hop, int64_t first, int64_t count, int64_t* lo, int64_t* hi) {
  *lo = std::min(n_total, std::max<int64_t>(0, first * hop - seg / 2));
  *hi = std::min(n_total, (first + count - 1) * hop - seg / 2 + seg);
}

// qi_stft_out and qi_stft_out_range; `rq`: qi_stft's request (eps set), of a range with its own origin, row stride and pooling
template <typename T>
int stft_out_impl(int device, StftRequest rq, const T* sig, const T* window, const qi_tfr_out* out, char* scratch, hipStream_t st) {
  const int64_t C = rq.C, nseg = rq.nseg, nf = rq.nfft / 2 + 1;
  const StftOutLayout l = stft_out_layout(sizeof(T) == 8 ? QI_F64 : QI_F32, C, nseg, rq.seg, rq.hop, rq.nfft, out->coef != nullptr,
                                          rq.pool_factor, rq.pool_max != nullptr);
  cplx<T>* Z = static_cast<cplx<T>*>(out->coef);
  T* bits = static_cast<T*>(out->bits);
  double* part_band = reinterpret_cast<double*>(scratch + l.part_band);
  double* part_stat = reinterpret_cast<double*>(scratch + l.part_stat);
  double* power_band = static_cast<double*>(out->power_band);
  double* stats = static_cast<double*>(out->stats);
  const double power_scale = qi::host::power_scale_or_default(out->power_scale);
  const bool reduce = power_band != nullptr;
  return fused_or_hipfft(
      stft_fused_supported(sizeof(T) == 8 ? QI_F64 : QI_F32, rq.seg, rq.hop, rq.nfft),
      [&] {
        StftRequest red = rq;
        if (reduce) {
          red.part_band = part_band;
          red.part_stat = part_stat;
          red.power_time = out->power_time;
          red.power_band = power_band;
          red.stats = stats;
          red.power_scale = power_scale;
          red.part_max = scratch + l.part_max;
        }
        return launch_stft_fused<T>(red, sig, window, Z, bits, st);
      },
      [&]() -> int {
        // into the caller's panel or the scratch one, then the hipFFT engine's reduction kernels on it
        if (!Z) Z = reinterpret_cast<cplx<T>*>(scratch + l.panel);
        QI_TRY(stft_hipfft<T>(device, rq, sig, window, Z, bits, scratch, st));
        if (!reduce) return QI_OK;
        const int64_t nblk = ceil_div(nseg, kEpiSpan);
        EpiArgs<T> a{};
        a.Y = Z;
        a.L = a.n = nseg;
        a.off = 0;
        a.Ct = C;
        a.Bt = a.B = nf;
        a.j0 = 0;
        a.power_time = static_cast<T*>(out->power_time);
        a.part_band = part_band;
        a.part_stat = part_stat;
        a.tile_b = 0;
        a.ntile_b = 1;
        a.power_scale = (T)power_scale;
        a.eps = (T)rq.eps;
        QI_TRY(launch_epilogue<T>(a, st));
        QI_TRY(launch_finalize(part_band, part_stat, power_band, stats, C, nf, nblk, nblk, st));
        // a range's pooled spectrogram: the strip kernel on the panel's rows (no sums: the epilogue has them)
        if (rq.pool_factor > 0 && (rq.pool_mean || rq.pool_max))
          return qi_pool_strip(sizeof(T) == 8 ? QI_F64 : QI_F32, device, Z, C * nf, nseg, 0, rq.pool_factor, nseg / rq.pool_factor,
                               power_scale, rq.pool_mean, rq.pool_max, nseg / rq.pool_factor, nullptr, (qi_stream)st);
        return QI_OK;
      });
}

}  // namespace

extern "C" {

// ---- STFT ----------------------------------------------------------------------------------------
int64_t qi_stft_segments(int64_t n, int64_t seg, int64_t hop) {
  if (n <= 0 || seg <= 0 || hop <= 0 || hop > seg) return 0;
  const int64_t len0 = n + 2 * (seg / 2);  // boundary='zeros' extends by seg//2 on both sides
  const int64_t nadd = ((hop - ((len0 - seg) % hop)) % hop) % seg;  // padded=True
  return (len0 + nadd - seg) / hop + 1;
}

int64_t qi_stft_scratch_bytes(int dtype, int64_t C, int64_t n, int64_t seg, int64_t hop, int64_t nfft) {
  return (int64_t)FftScratch(dtype, C, qi_stft_segments(n, seg, hop), nfft).total;
}

int qi_stft(int dtype, int device, const void* sig, int64_t C, int64_t n, const void* window, int64_t seg,
            int64_t hop, int64_t nfft, double scale, void* Z, void* bits, double eps, void* scratch,
            int64_t scratch_bytes, qi_stream stream) {
  QI_REQUIRE(sig && window && Z && scratch, "null argument");
  QI_REQUIRE(dtype == QI_F32 || dtype == QI_F64, "bad dtype %d", dtype);
  QI_REQUIRE(C > 0 && n > 0 && seg > 0 && hop > 0 && hop <= seg && nfft >= seg, "bad STFT geometry");
  QI_REQUIRE(scratch_bytes >= qi_stft_scratch_bytes(dtype, C, n, seg, hop, nfft), "scratch too small");
  DeviceGuard g(device);
  hipStream_t st = (hipStream_t)stream;
  StftRequest rq{C, n, seg, hop, nfft, qi_stft_segments(n, seg, hop), seg / 2};
  rq.scale = scale;
  rq.eps = qi::host::eps_or_default(eps);
  return by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    const T *x = (const T*)sig, *w = (const T*)window;
    return fused_or_hipfft(
        stft_fused_supported(dtype, seg, hop, nfft),
        [&] { return launch_stft_fused<T>(rq, x, w, (cplx<T>*)Z, (T*)bits, st); },  // one kernel: segments, transform, store from LDS
        [&] { return stft_hipfft<T>(device, rq, x, w, (cplx<T>*)Z, (T*)bits, (char*)scratch, st); });
  });
}

int64_t qi_stft_out_scratch_bytes(int dtype, int64_t C, int64_t n, int64_t seg, int64_t hop, int64_t nfft, int want_coef,
                                  int want_bits) {
  (void)want_bits;  // (the bits panel is never formed in scratch)
  if (C <= 0 || nfft < seg || qi_stft_segments(n, seg, hop) <= 0) return 0;
  return (int64_t)stft_out_layout(dtype, C, qi_stft_segments(n, seg, hop), seg, hop, nfft, want_coef != 0).total;
}

int qi_stft_out(int dtype, int device, const void* sig, int64_t C, int64_t n, const void* window, int64_t seg, int64_t hop,
                int64_t nfft, double scale, const qi_tfr_out* out, void* scratch, int64_t scratch_bytes, qi_stream stream) {
  QI_REQUIRE(sig && window && out && scratch, "null argument");
  QI_REQUIRE(dtype == QI_F32 || dtype == QI_F64, "bad dtype %d", dtype);
  QI_REQUIRE(C > 0 && n > 0 && seg > 0 && hop > 0 && hop <= seg && nfft >= seg, "bad STFT geometry");
  QI_REQUIRE(out->coef || out->bits || out->power_band || out->power_time || out->stats, "nothing to produce");
  QI_REQUIRE((out->power_band != nullptr) == (out->stats != nullptr), "power_band and stats come together");
  QI_REQUIRE(!out->power_time || out->power_band, "power_time needs power_band and stats");
  QI_REQUIRE(scratch_bytes >= qi_stft_out_scratch_bytes(dtype, C, n, seg, hop, nfft, out->coef != nullptr, out->bits != nullptr),
             "scratch too small");
  DeviceGuard g(device);
  StftRequest rq{C, n, seg, hop, nfft, qi_stft_segments(n, seg, hop), seg / 2};
  rq.scale = scale;
  rq.eps = qi::host::eps_or_default(out->eps);
  return by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    return stft_out_impl<T>(device, rq, (const T*)sig, (const T*)window, out, (char*)scratch, (hipStream_t)stream);
  });
}

// ---- the STFT of a segment range (a streamed record: stream.StftStream) ---------------------------------------------------
int qi_stft_range_samples(int64_t n_total, int64_t seg, int64_t hop, int64_t first_segment, int64_t segments, int64_t* sample0,
                          int64_t* n_avail) {
  QI_REQUIRE(sample0 && n_avail, "null argument");
  const int64_t total = qi_stft_segments(n_total, seg, hop);
  QI_REQUIRE(total > 0, "bad STFT geometry");
  QI_REQUIRE(first_segment >= 0 && segments >= 1 && segments <= total - first_segment,
             "segments %lld .. %lld of a record of %lld", (long long)first_segment, (long long)(first_segment + segments - 1),
             (long long)total);
  int64_t lo, hi;
  stft_range_interval(n_total, seg, hop, first_segment, segments, &lo, &hi);
  *sample0 = lo;
  *n_avail = std::max<int64_t>(0, hi - lo);
  return QI_OK;
}

// every refusal of a range; host arithmetic only
static int stft_range_check(int64_t seg, int64_t hop, int64_t nfft, const qi_stft_range* r) {
  QI_REQUIRE(r, "null argument");
  QI_REQUIRE(seg > 0 && hop > 0 && hop <= seg && nfft >= seg && r->n_total > 0, "bad STFT geometry");
  const int64_t total = qi_stft_segments(r->n_total, seg, hop);
  QI_REQUIRE(r->first_segment >= 0 && r->segments >= 1 && r->segments <= total - r->first_segment,
             "segments %lld .. %lld of a record of %lld", (long long)r->first_segment,
             (long long)(r->first_segment + r->segments - 1), (long long)total);
  QI_REQUIRE(r->sample0 >= 0 && r->n_avail >= 0 && r->n_avail <= r->n_total - r->sample0,
             "samples %lld .. +%lld are not inside a record of %lld", (long long)r->sample0, (long long)r->n_avail,
             (long long)r->n_total);
  QI_REQUIRE(r->row_stride >= r->n_avail, "rows of %lld samples cannot hold %lld", (long long)r->row_stride, (long long)r->n_avail);
  int64_t lo, hi;
  stft_range_interval(r->n_total, seg, hop, r->first_segment, r->segments, &lo, &hi);
  QI_REQUIRE(hi <= lo || (r->sample0 <= lo && hi <= r->sample0 + r->n_avail),
             "the range needs the record samples %lld .. %lld, the rows hold %lld .. %lld", (long long)lo, (long long)hi - 1,
             (long long)r->sample0, (long long)(r->sample0 + r->n_avail) - 1);
  const int64_t F = r->pool_factor;
  QI_REQUIRE(F == 0 || F >= 2, "pooling factor %lld: 0 (none), or 2 or more", (long long)F);
  QI_REQUIRE(F > 0 || !(r->pool_mean || r->pool_max), "pooled outputs without a pooling factor");
  if (F > 0) {
    QI_REQUIRE(r->first_segment % F == 0, "first segment %lld is no multiple of the pooling factor %lld",
               (long long)r->first_segment, (long long)F);
    QI_REQUIRE(r->segments % F == 0 || r->first_segment + r->segments == total,
               "%lld segments are no multiple of the pooling factor %lld and do not end the record", (long long)r->segments,
               (long long)F);
  }
  return QI_OK;
}

int64_t qi_stft_range_scratch_bytes(int dtype, int64_t C, int64_t seg, int64_t hop, int64_t nfft, const qi_stft_range* range,
                                    int want_coef) {
  QI_REQUIRE(dtype == QI_F32 || dtype == QI_F64, "bad dtype %d", dtype);
  QI_REQUIRE(C > 0, "bad channel count");
  QI_TRY(stft_range_check(seg, hop, nfft, range));
  return (int64_t)stft_out_layout(dtype, C, range->segments, seg, hop, nfft, want_coef != 0, range->pool_factor,
                                  range->pool_max != nullptr).total;
}

int qi_stft_out_range(int dtype, int device, const void* sig, int64_t C, const void* window, int64_t seg, int64_t hop, int64_t nfft,
                      double scale, const qi_stft_range* range, const qi_tfr_out* out, void* scratch, int64_t scratch_bytes,
                      qi_stream stream) {
  QI_REQUIRE(window && out && scratch && range, "null argument");
  QI_REQUIRE(dtype == QI_F32 || dtype == QI_F64, "bad dtype %d", dtype);
  QI_REQUIRE(C > 0, "bad channel count");
  QI_TRY(stft_range_check(seg, hop, nfft, range));
  QI_REQUIRE(sig || range->n_avail == 0, "null argument");
  const bool pooled = range->pool_mean || range->pool_max;
  QI_REQUIRE(out->coef || out->bits || out->power_band || out->power_time || out->stats || pooled, "nothing to produce");
  QI_REQUIRE((out->power_band != nullptr) == (out->stats != nullptr), "power_band and stats come together");
  QI_REQUIRE(!out->power_time || out->power_band, "power_time needs power_band and stats");
  QI_REQUIRE(!pooled || out->power_band, "the pooled outputs come with power_band and stats");
  QI_REQUIRE(scratch_bytes >= qi_stft_range_scratch_bytes(dtype, C, seg, hop, nfft, range, out->coef != nullptr), "scratch too small");
  DeviceGuard g(device);
  StftRequest rq{C, range->n_avail, seg, hop, nfft, range->segments, seg / 2 + range->sample0 - range->first_segment * hop};
  rq.scale = scale;
  rq.eps = qi::host::eps_or_default(out->eps);
  rq.row_stride = range->row_stride;
  if (pooled) {
    rq.pool_factor = range->pool_factor;
    rq.pool_mean = range->pool_mean;
    rq.pool_max = range->pool_max;
  }
  return by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    return stft_out_impl<T>(device, rq, (const T*)sig, (const T*)window, out, (char*)scratch, (hipStream_t)stream);
  });
}

// The three-kernel sequence's scratch also holds the fused kernel's [C][groups][nfft / 2 + 1] double partials: groups <= nseg
// and 8 <= 2 sizeof(T), so they are never the larger of the two.
int64_t qi_welch_scratch_bytes(int dtype, int64_t C, int64_t n, int64_t seg, int64_t hop, int64_t nfft) {
  if (n < seg || seg <= 0 || hop <= 0) return 0;
  const int64_t nseg = (n - seg) / hop + 1;
  const size_t fused = align_up((size_t)C * stft_fused_groups(dtype, nfft, nseg) * (nfft / 2 + 1) * 8);
  return (int64_t)std::max(FftScratch(dtype, C, nseg, nfft).total, fused);
}

int qi_welch(int dtype, int device, const void* sig, int64_t C, int64_t n, const void* window, int64_t seg,
             int64_t hop, int64_t nfft, double scale, void* pxx, void* scratch, int64_t scratch_bytes,
             qi_stream stream) {
  QI_REQUIRE(sig && window && pxx && scratch, "null argument");
  QI_REQUIRE(dtype == QI_F32 || dtype == QI_F64, "bad dtype %d", dtype);
  QI_REQUIRE(C > 0 && seg > 0 && n >= seg && hop > 0 && hop <= seg && nfft >= seg, "bad Welch geometry");
  QI_REQUIRE(scratch_bytes >= qi_welch_scratch_bytes(dtype, C, n, seg, hop, nfft), "scratch too small");
  DeviceGuard g(device);
  hipStream_t st = (hipStream_t)stream;
  StftRequest rq{C, n, seg, hop, nfft, (n - seg) / hop + 1, 0};
  rq.scale = scale;
  return by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    const T *x = (const T*)sig, *w = (const T*)window;
    return fused_or_hipfft(
        stft_fused_supported(dtype, seg, hop, nfft),
        // segments, transform, |X|^2 sums in one kernel
        [&] { return launch_welch_fused<T>(rq, x, w, (T*)pxx, (double*)scratch, st); },
        [&] {
          return via_hipfft<T>(device, rq, x, w, (char*)scratch, st,
                               [&](const cplx<T>* F) { return launch_welch_mean<T>(rq, F, (T*)pxx, st); });
        });
  });
}

// ---- cross-spectra of the Welch segments (include/qi_array.h) -----------------------------------------------------------
// Scratch of qi_csd and qi_csd_windows: [0] the three-kernel path's frames and spectra | [1] the coefficient panel
// [C][nfft / 2 + 1][nseg] | [2] the contraction's own (cross_spectra_scratch, cross_spectra_windows_scratch)
struct CsdLayout {
  size_t panel, cross, total;
  CsdLayout(int dtype, int64_t C, int64_t nseg, int64_t nfft, size_t contraction) {
    const int64_t nf = nfft / 2 + 1;
    panel = FftScratch(dtype, C, nseg, nfft).total;
    cross = panel + align_up((size_t)C * nf * nseg * 2 * elem_size(dtype));
    total = cross + contraction;
  }
};
static int csd_geometry_check(int dtype, int64_t C, int64_t n, int64_t seg, int64_t hop, int64_t nfft) {
  QI_REQUIRE(dtype == QI_F32 || dtype == QI_F64, "bad dtype %d", dtype);
  QI_REQUIRE(C > 0 && seg > 0 && n >= seg && hop > 0 && hop <= seg && nfft >= seg, "bad Welch geometry");
  return QI_OK;
}
static int csd_check(int dtype, int64_t C, int64_t n, int64_t seg, int64_t hop, int64_t nfft) {
  QI_TRY(csd_geometry_check(dtype, C, n, seg, hop, nfft));
  // (the shape refusals of the contraction, before anything is launched)
  const int64_t bytes = qi_cross_spectra_scratch_bytes(dtype, C, nfft / 2 + 1, (n - seg) / hop + 1);
  return bytes < 0 ? (int)bytes : QI_OK;
}
// the first step of both: qi_welch's segments as the UNSCALED coefficient panel [C][nfft / 2 + 1][nseg] in the layout's second
// region (the weight of the contraction carries scale^2)
static int csd_panel(int dtype, int device, const StftRequest& rq, const CsdLayout& l, const void* sig, const void* window,
                     void* scratch, hipStream_t st) {
  return by_dtype(dtype, [&](auto t) -> int {
    using T = decltype(t);
    const T *x = (const T*)sig, *win = (const T*)window;
    char* s = (char*)scratch;
    cplx<T>* Z = reinterpret_cast<cplx<T>*>(s + l.panel);
    return fused_or_hipfft(
        stft_fused_supported(dtype, rq.seg, rq.hop, rq.nfft),
        [&] { return launch_stft_fused<T>(rq, x, win, Z, (T*)nullptr, st); },  // the storing form with lead = 0
        [&] { return stft_hipfft<T>(device, rq, x, win, Z, (T*)nullptr, s, st); });
  });
}

int64_t qi_csd_scratch_bytes(int dtype, int64_t C, int64_t n, int64_t seg, int64_t hop, int64_t nfft) {
  QI_TRY(csd_check(dtype, C, n, seg, hop, nfft));
  return (int64_t)CsdLayout(dtype, C, (n - seg) / hop + 1, nfft, cross_spectra_scratch(dtype, C, nfft / 2 + 1)).total;
}

int qi_csd(int dtype, int device, const void* sig, int64_t C, int64_t n, const void* window, int64_t seg, int64_t hop,
           int64_t nfft, double scale, void* csd, void* coherence, void* scratch, int64_t scratch_bytes, qi_stream stream) {
  QI_REQUIRE(sig && window && scratch, "null argument");
  QI_REQUIRE(csd || coherence, "nothing to produce");
  QI_TRY(csd_check(dtype, C, n, seg, hop, nfft));
  const int64_t nseg = (n - seg) / hop + 1, nf = nfft / 2 + 1;
  const CsdLayout l(dtype, C, nseg, nfft, cross_spectra_scratch(dtype, C, nf));
  QI_TRY(require_scratch(scratch_bytes, (int64_t)l.total));
  QI_REQUIRE(aligned(scratch, 16), "misaligned scratch");
  DeviceGuard g(device);
  hipStream_t st = (hipStream_t)stream;
  StftRequest rq{C, n, seg, hop, nfft, nseg, 0};  // qi_welch's segments
  CsdWeight w;
  w.edge = scale * scale / (double)nseg;
  w.paired = 2.0 * w.edge;
  w.nfft = nfft;
  QI_TRY(csd_panel(dtype, device, rq, l, sig, window, scratch, st));
  return by_dtype(dtype, [&](auto t) -> int {
    using T = decltype(t);
    char* s = (char*)scratch;
    return launch_cross_spectra<T>(reinterpret_cast<const cplx<T>*>(s + l.panel), C, nf, nseg, w, (cplx<T>*)csd, (T*)coherence,
                                   s + l.cross + align_up((size_t)nf * 8), st);
  });
}

// ---- the same per sliding window of segments (include/qi_windows.h) -----------------------------------------------------
static int csd_windows_check(int dtype, int64_t C, int64_t n, int64_t seg, int64_t hop, int64_t nfft, int64_t bin_first,
                             int64_t bin_count, int64_t win, int64_t win_hop, int64_t* contraction) {
  QI_TRY(csd_geometry_check(dtype, C, n, seg, hop, nfft));
  *contraction = qi_cross_spectra_windows_scratch_bytes(dtype, C, nfft / 2 + 1, (n - seg) / hop + 1, bin_first, bin_count, win, win_hop);
  return *contraction < 0 ? (int)*contraction : QI_OK;
}

int64_t qi_csd_windows_scratch_bytes(int dtype, int64_t C, int64_t n, int64_t seg, int64_t hop, int64_t nfft, int64_t bin_first,
                                     int64_t bin_count, int64_t win, int64_t win_hop) {
  int64_t contraction = 0;
  QI_TRY(csd_windows_check(dtype, C, n, seg, hop, nfft, bin_first, bin_count, win, win_hop, &contraction));
  return (int64_t)CsdLayout(dtype, C, (n - seg) / hop + 1, nfft, (size_t)contraction).total;
}

int qi_csd_windows(int dtype, int device, const void* sig, int64_t C, int64_t n, const void* window, int64_t seg, int64_t hop,
                   int64_t nfft, double scale, int64_t bin_first, int64_t bin_count, int64_t win, int64_t win_hop, void* csd,
                   void* coherence, void* scratch, int64_t scratch_bytes, qi_stream stream) {
  QI_REQUIRE(sig && window && scratch, "null argument");
  QI_REQUIRE(csd || coherence, "nothing to produce");
  int64_t contraction = 0;
  QI_TRY(csd_windows_check(dtype, C, n, seg, hop, nfft, bin_first, bin_count, win, win_hop, &contraction));
  const int64_t nseg = (n - seg) / hop + 1, nf = nfft / 2 + 1;
  const CsdLayout l(dtype, C, nseg, nfft, (size_t)contraction);
  QI_TRY(require_scratch(scratch_bytes, (int64_t)l.total));
  QI_REQUIRE(aligned(scratch, 16) && aligned(csd, 2 * elem_size(dtype)) && aligned(coherence, elem_size(dtype)), "misaligned pointer");
  DeviceGuard g(device);
  hipStream_t st = (hipStream_t)stream;
  StftRequest rq{C, n, seg, hop, nfft, nseg, 0};  // qi_welch's segments
  CsdWeight w;  // every window averages its own `win` segments
  w.edge = scale * scale / (double)win;
  w.paired = 2.0 * w.edge;
  w.nfft = nfft;
  QI_TRY(csd_panel(dtype, device, rq, l, sig, window, scratch, st));
  return by_dtype(dtype, [&](auto t) -> int {
    using T = decltype(t);
    char* s = (char*)scratch;
    return launch_cross_spectra_windows<T>(reinterpret_cast<const cplx<T>*>(s + l.panel), C, nf, nseg, bin_first, bin_count, win, win_hop,
                                           w, (cplx<T>*)csd, (T*)coherence, s + l.cross + align_up((size_t)bin_count * 8), st);
  });
}

// ---- time delays between the records from their matrices (include/qi_lags.h) --------------------------------------------
static int pair_lags_shape_check(int dtype, int64_t nstack, int64_t C, int64_t nfft, int64_t upsample) {
  QI_REQUIRE(dtype == QI_F32 || dtype == QI_F64, "bad dtype %d", dtype);
  QI_REQUIRE(nstack >= 1 && C >= 2, "bad stack shape: %lld stacks of %lld records (a pair needs two)", (long long)nstack, (long long)C);
  QI_REQUIRE(upsample == 1 || upsample == 2 || upsample == 4 || upsample == 8, "bad upsample %lld (1, 2, 4 or 8)", (long long)upsample);
  QI_REQUIRE(is_pow2(nfft) && nfft * upsample >= 64 && nfft * upsample <= 8192,
             "bad transform length: nfft %lld x upsample %lld must be a power of two in 64 .. 8192", (long long)nfft, (long long)upsample);
  QI_REQUIRE(C <= (1 << 20) && nstack <= (1ll << 40) && (double)nstack * (double)(nfft / 2 + 1) * (double)C * (double)C <= 0x1p40 &&
                 (double)nstack * (double)(C * (C - 1) / 2) < 0x1p31,
             "request too large");
  return QI_OK;
}

int64_t qi_pair_lags_scratch_bytes(int dtype, int64_t nstack, int64_t C, int64_t nfft, int64_t upsample) {
  QI_TRY(pair_lags_shape_check(dtype, nstack, C, nfft, upsample));
  return 0;
}

int qi_pair_lags(int dtype, int device, const void* csd, int64_t nstack, int64_t C, int64_t nfft, int64_t bin_lo, int64_t bin_hi,
                 int weighting, int halve_interior, int normalize, int64_t upsample, int64_t max_lag, void* cc, void* peak_lag,
                 void* peak_value, void* scratch, int64_t scratch_bytes, qi_stream stream) {
  QI_REQUIRE(csd, "null argument");
  QI_REQUIRE(cc || peak_lag || peak_value, "nothing to produce");
  QI_TRY(pair_lags_shape_check(dtype, nstack, C, nfft, upsample));
  QI_REQUIRE(weighting >= 0 && weighting <= 2, "bad weighting %d (0 plain, 1 PHAT, 2 SCOT)", weighting);
  QI_REQUIRE(bin_lo >= 0 && bin_lo <= bin_hi && bin_hi <= nfft / 2 + 1, "bad bin range %lld .. %lld of %lld bins", (long long)bin_lo,
             (long long)bin_hi, (long long)(nfft / 2 + 1));
  QI_REQUIRE(max_lag >= 0 && max_lag <= nfft * upsample / 2 - 1, "bad max_lag %lld (0 .. %lld)", (long long)max_lag,
             (long long)(nfft * upsample / 2 - 1));
  QI_TRY(require_scratch(scratch_bytes, 0));
  const size_t e = elem_size(dtype);
  QI_REQUIRE(aligned(csd, 2 * e) && aligned(cc, e) && aligned(peak_lag, e) && aligned(peak_value, e) && aligned(scratch, 16),
             "misaligned pointer");
  DeviceGuard g(device);
  hipStream_t st = (hipStream_t)stream;
  return by_dtype(dtype, [&](auto t) -> int {
    using T = decltype(t);
    return launch_pair_lags<T>((const cplx<T>*)csd, nstack, C, nfft, bin_lo, bin_hi, weighting, halve_interior, normalize, upsample,
                               max_lag, (T*)cc, (T*)peak_lag, (T*)peak_value, st);
  });
}

// ---- delay-and-sum in the time domain (include/qi_timebeam.h) ------------------------------------------------------------
// what both calls and the size query refuse of the records, the bank and the delay rows (`rows`: G or K)
static int time_beam_shape_check(int dtype, int64_t C, int64_t n, int64_t P, int64_t T, int64_t rows, int64_t max_shift) {
  QI_REQUIRE(dtype == QI_F32 || dtype == QI_F64, "bad dtype %d", dtype);
  QI_REQUIRE(C >= 2 && C <= QI_BEAM_MAX_SENSORS, "%lld sensors: 2 to %d", (long long)C, QI_BEAM_MAX_SENSORS);
  QI_REQUIRE(P >= 1 && P <= QI_TIMEBEAM_MAX_PHASES, "%lld phases in the bank: 1 to %d", (long long)P, QI_TIMEBEAM_MAX_PHASES);
  QI_REQUIRE(T == 1 || T == 2 || T == 4 || T == 8 || T == 16, "%lld taps: 1, 2, 4, 8 or 16", (long long)T);
  QI_REQUIRE(n >= 1 && rows >= 1, "bad shape: %lld samples, %lld delay rows", (long long)n, (long long)rows);
  QI_REQUIRE(n <= (1ll << 40) && rows <= (1ll << 40), "request too large");
  QI_REQUIRE(max_shift >= 0 && max_shift <= QI_TIMEBEAM_MAX_SHIFT, "bad max_shift %lld (0 .. %d)", (long long)max_shift,
             QI_TIMEBEAM_MAX_SHIFT);
  return QI_OK;
}

static int time_beam_power_check(int dtype, int64_t C, int64_t n, int64_t P, int64_t T, int64_t G, int64_t win, int64_t hop,
                                 int64_t max_shift) {
  QI_TRY(time_beam_shape_check(dtype, C, n, P, T, G, max_shift));
  QI_REQUIRE(win >= 1 && win <= n, "bad window of %lld samples in a record of %lld", (long long)win, (long long)n);
  QI_REQUIRE(hop >= 1, "bad hop %lld", (long long)hop);
  const TimeBeamUnits u = time_beam_units(n, win, hop);
  QI_REQUIRE((double)u.count * (double)time_beam_row_blocks(G) < 0x1p31 && u.nwin < (1ll << 31) &&
                 (double)u.count * (double)G < 0x1p40,
             "request too large");
  return QI_OK;
}

int64_t qi_time_beam_power_scratch_bytes(int dtype, int64_t C, int64_t n, int64_t P, int64_t T, int64_t G, int64_t win,
                                         int64_t hop, int64_t max_shift) {
  QI_TRY(time_beam_power_check(dtype, C, n, P, T, G, win, hop, max_shift));
  return (int64_t)align_up((size_t)time_beam_units(n, win, hop).count * (size_t)G * 2 * elem_size(dtype));
}

int qi_time_beam_power(int dtype, int device, const void* x, int64_t C, int64_t n, const void* taps, int64_t P, int64_t T,
                       const void* shift, const void* phase, int64_t G, int64_t max_shift, int64_t win, int64_t hop,
                       int normalize, void* power, void* peak_index, void* peak_value, void* scratch, int64_t scratch_bytes,
                       qi_stream stream) {
  QI_REQUIRE(x && taps && shift && phase && scratch, "null argument");
  QI_REQUIRE(power || peak_index || peak_value, "nothing to produce");
  QI_TRY(time_beam_power_check(dtype, C, n, P, T, G, win, hop, max_shift));
  QI_TRY(require_scratch(scratch_bytes, qi_time_beam_power_scratch_bytes(dtype, C, n, P, T, G, win, hop, max_shift)));
  const size_t e = elem_size(dtype);
  QI_REQUIRE(aligned(x, e) && aligned(taps, e) && aligned(shift, 4) && aligned(phase, 4) && aligned(power, e) &&
                 aligned(peak_index, 8) && aligned(peak_value, e) && aligned(scratch, 16),
             "misaligned pointer");
  DeviceGuard g(device);
  hipStream_t st = (hipStream_t)stream;
  return by_dtype(dtype, [&](auto t) -> int {
    using R = decltype(t);
    return launch_time_beam_power<R>((const R*)x, C, n, (const R*)taps, P, T, (const int32_t*)shift, (const int32_t*)phase, G,
                                     max_shift, win, hop, normalize, (R*)power, (int64_t*)peak_index, (R*)peak_value, (R*)scratch, st);
  });
}

int qi_time_beam_traces(int dtype, int device, const void* x, int64_t C, int64_t n, const void* taps, int64_t P, int64_t T,
                        const void* shift, const void* phase, int64_t K, int64_t max_shift, void* out, qi_stream stream) {
  QI_REQUIRE(x && taps && shift && phase, "null argument");
  QI_REQUIRE(out, "out is null: nothing to produce");
  QI_TRY(time_beam_shape_check(dtype, C, n, P, T, K, max_shift));
  QI_REQUIRE((double)time_beam_chunks(n) * (double)time_beam_row_blocks(K) < 0x1p31, "request too large");
  const size_t e = elem_size(dtype);
  QI_REQUIRE(aligned(x, e) && aligned(taps, e) && aligned(shift, 4) && aligned(phase, 4) && aligned(out, e), "misaligned pointer");
  DeviceGuard g(device);
  hipStream_t st = (hipStream_t)stream;
  return by_dtype(dtype, [&](auto t) -> int {
    using R = decltype(t);
    return launch_time_beam_traces<R>((const R*)x, C, n, (const R*)taps, P, T, (const int32_t*)shift, (const int32_t*)phase, K,
                                      max_shift, (R*)out, st);
  });
}

// ---- synchrosqueezing (include/qi_squeeze.h) -------------------------------------------------------------------------------
// what the three calls and the size query refuse of the shape
static int squeeze_shape_check(int dtype, int64_t C, int64_t nb, int64_t n, int64_t nbin) {
  QI_REQUIRE(dtype == QI_F32 || dtype == QI_F64, "bad dtype %d", dtype);
  QI_REQUIRE(C >= 1 && nb >= 1 && nbin >= 1, "bad shape: %lld records, %lld bands, %lld bins", (long long)C, (long long)nb,
             (long long)nbin);
  QI_REQUIRE(n >= 2, "bad panel length %lld (a column and its partner: 2 at least)", (long long)n);
  QI_REQUIRE(nbin <= QI_SQUEEZE_MAX_BINS, "%lld bins: %d at most", (long long)nbin, QI_SQUEEZE_MAX_BINS);
  QI_REQUIRE(C <= (1ll << 40) && nb <= QI_SQUEEZE_MAX_BANDS && n <= (1ll << 40) && (double)C * (double)nb * (double)n <= 0x1p40 &&
                 (double)C * (double)nbin * (double)n <= 0x1p40 && (double)C * (double)nb * (double)squeeze_tiles(n) < 0x1p31,
             "request too large");
  return QI_OK;
}

// the tables in the scratch: edges [nbin + 1] | carrier [nb] | weight [nb] of the panel's type, each on a multiple of 16 bytes
static SqueezeTables squeeze_layout(int dtype, int64_t nb, int64_t nbin, size_t* total) {
  const size_t e = elem_size(dtype);
  SqueezeTables tb{};
  tb.edges = 0;
  tb.carrier = align_up((size_t)(nbin + 1) * e, 16);
  tb.weight = tb.carrier + align_up((size_t)nb * e, 16);
  *total = align_up(tb.weight + (size_t)nb * e);
  return tb;
}

extern "C++" {  // (templates: C++ linkage)
// the host tables rounded to T into `words` (laid out by `tb`), refused as the header says; a null table: `fill`
template <typename T>
static int squeeze_round(const double* src, int64_t count, double fill, const char* what, std::vector<uint64_t>& words, size_t at) {
  T* dst = reinterpret_cast<T*>(reinterpret_cast<char*>(words.data()) + at);
  for (int64_t i = 0; i < count; ++i) {
    dst[i] = (T)(src ? src[i] : fill);
    QI_REQUIRE(std::isfinite(dst[i]), "%s[%lld] is not finite", what, (long long)i);
  }
  return QI_OK;
}

template <typename T>
static int squeeze_tables(int64_t nb, int64_t nbin, const double* carrier, const double* edges, const double* weight,
                          const SqueezeTables& tb, std::vector<uint64_t>& words) {
  QI_TRY(squeeze_round<T>(carrier, nb, 0.0, "carrier_hz", words, tb.carrier));
  QI_TRY(squeeze_round<T>(weight, nb, 1.0, "weight", words, tb.weight));
  if (!edges) return QI_OK;  // (qi_tfr_ifreq: no bins)
  QI_TRY(squeeze_round<T>(edges, nbin + 1, 0.0, "edges_hz", words, tb.edges));
  const T* e = reinterpret_cast<const T*>(reinterpret_cast<const char*>(words.data()) + tb.edges);
  for (int64_t i = 0; i < nbin; ++i)
    QI_REQUIRE(e[i] < e[i + 1], "edges_hz is not strictly ascending at %lld (as rounded to the panel's precision)", (long long)i);
  return QI_OK;
}
}  // extern "C++"

static int squeeze_rate_check(int dtype, double rate, double floor) {
  const double r = dtype == QI_F64 ? rate : (double)(float)rate, f = dtype == QI_F64 ? floor : (double)(float)floor;
  QI_REQUIRE(std::isfinite(r) && r > 0.0, "bad sample_rate_hz %g (finite and above 0)", rate);
  QI_REQUIRE(floor >= 0.0 && std::isfinite(f), "bad power_floor %g (finite, 0 or more)", floor);
  return QI_OK;
}

// the three calls behind their null checks: want_ifreq / want_out say which kernels run
static int squeeze_run(int dtype, int device, const void* Z, const void* ifreq_in, int64_t C, int64_t nb, int64_t n,
                       const double* carrier, double rate, double floor, bool estimates, const double* edges, int64_t nbin,
                       const double* weight, void* ifreq_out, void* out, void* scratch, int64_t scratch_bytes, qi_stream stream) {
  QI_TRY(squeeze_shape_check(dtype, C, nb, n, nbin));
  if (estimates) QI_TRY(squeeze_rate_check(dtype, rate, floor));
  size_t total = 0;
  SqueezeTables tb = squeeze_layout(dtype, nb, nbin, &total);
  std::vector<uint64_t> words(total / 8);
  QI_TRY(by_dtype(dtype, [&](auto t) -> int { return squeeze_tables<decltype(t)>(nb, nbin, carrier, edges, weight, tb, words); }));
  QI_TRY(require_scratch(scratch_bytes, (int64_t)total));
  const size_t e = elem_size(dtype);
  QI_REQUIRE(aligned(Z, 2 * e) && aligned(ifreq_in, e) && aligned(ifreq_out, e) && aligned(out, 2 * e) && aligned(scratch, 16),
             "misaligned pointer");
  DeviceGuard g(device);
  hipStream_t st = (hipStream_t)stream;
  // the host arrays ride in kernel arguments: stream-ordered, and the caller's arrays are free at return
  QI_TRY(qi::host::put_words(scratch, words.data(), (int64_t)words.size(), st));
  tb.base = scratch;
  return by_dtype(dtype, [&](auto t) -> int {
    using T = decltype(t);
    if (ifreq_out) return launch_tfr_ifreq<T>((const cplx<T>*)Z, C, nb, n, tb, rate, floor, (T*)ifreq_out, st);
    return launch_tfr_squeeze<T>((const cplx<T>*)Z, (const T*)ifreq_in, C, nb, n, nbin, tb, rate, floor, (cplx<T>*)out, st);
  });
}

int64_t qi_tfr_squeeze_scratch_bytes(int dtype, int64_t C, int64_t nb, int64_t n, int64_t nbin) {
  QI_TRY(squeeze_shape_check(dtype, C, nb, n, nbin));
  size_t total = 0;
  squeeze_layout(dtype, nb, nbin, &total);
  return (int64_t)total;
}

int qi_tfr_ifreq(int dtype, int device, const void* Z, int64_t C, int64_t nb, int64_t n, const double* carrier_hz,
                 double sample_rate_hz, double power_floor, void* ifreq, void* scratch, int64_t scratch_bytes, qi_stream stream) {
  QI_REQUIRE(Z && scratch, "null argument");
  QI_REQUIRE(ifreq, "ifreq is null: nothing to produce");
  return squeeze_run(dtype, device, Z, nullptr, C, nb, n, carrier_hz, sample_rate_hz, power_floor, true, nullptr, 1, nullptr, ifreq,
                     nullptr, scratch, scratch_bytes, stream);
}

int qi_tfr_squeeze(int dtype, int device, const void* Z, const void* ifreq, int64_t C, int64_t nb, int64_t n,
                   const double* edges_hz, int64_t nbin, const double* weight, void* out, void* scratch, int64_t scratch_bytes,
                   qi_stream stream) {
  QI_REQUIRE(Z && ifreq && scratch && edges_hz, "null argument");
  QI_REQUIRE(out, "out is null: nothing to produce");
  return squeeze_run(dtype, device, Z, ifreq, C, nb, n, nullptr, 1.0, 0.0, false, edges_hz, nbin, weight, nullptr, out, scratch,
                     scratch_bytes, stream);
}

int qi_tfr_synchrosqueeze(int dtype, int device, const void* Z, int64_t C, int64_t nb, int64_t n, const double* carrier_hz,
                          double sample_rate_hz, double power_floor, const double* edges_hz, int64_t nbin, const double* weight,
                          void* out, void* scratch, int64_t scratch_bytes, qi_stream stream) {
  QI_REQUIRE(Z && scratch && edges_hz, "null argument");
  QI_REQUIRE(out, "out is null: nothing to produce");
  return squeeze_run(dtype, device, Z, nullptr, C, nb, n, carrier_hz, sample_rate_hz, power_floor, true, edges_hz, nbin, weight,
                     nullptr, out, scratch, scratch_bytes, stream);
}

// ---- tfr_info -------------------------------------------------------------------------------------
int64_t qi_power_marginals_scratch_bytes(int64_t C, int64_t B, int64_t n) {
  const int64_t nblk = ceil_div(n, kEpiSpan);
  return (int64_t)(align_up((size_t)C * B * nblk * 8) + align_up((size_t)C * nblk * 24));
}

int qi_power_marginals(int dtype, int device, const void* power, int64_t C, int64_t B, int64_t n, void* power_band,
                       void* power_time, void* stats, void* scratch, int64_t scratch_bytes, qi_stream stream) {
  QI_REQUIRE(power && scratch, "null argument");
  QI_REQUIRE(dtype == QI_F32 || dtype == QI_F64, "bad dtype %d", dtype);
  QI_REQUIRE(C > 0 && B > 0 && n > 0, "bad panel shape");
  QI_REQUIRE(scratch_bytes >= qi_power_marginals_scratch_bytes(C, B, n), "scratch too small");
  DeviceGuard g(device);
  hipStream_t st = (hipStream_t)stream;
  const int64_t nblk = ceil_div(n, kEpiSpan);
  double* pb = reinterpret_cast<double*>(scratch);
  double* ps = reinterpret_cast<double*>((char*)scratch + align_up((size_t)C * B * nblk * 8));
  QI_TRY(by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    return launch_power_marginals<T>((const T*)power, C, B, n, (T*)power_time, pb, ps, st);
  }));
  return launch_finalize(power_band ? pb : nullptr, stats ? ps : nullptr, (double*)power_band, (double*)stats, C, B,
                         nblk, nblk, st);
}

int qi_log2_offset(int dtype, int device, const void* in, void* out, int64_t C, int64_t count, double eps,
                   const void* ref, qi_stream stream) {
  QI_REQUIRE(in && out, "null argument");
  QI_REQUIRE(dtype == QI_F32 || dtype == QI_F64, "bad dtype %d", dtype);
  QI_REQUIRE(C > 0 && count > 0, "bad shape");
  DeviceGuard g(device);
  return by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    return launch_log2_offset<T>((const T*)in, (T*)out, C, count, (T)eps, (const double*)ref, (hipStream_t)stream);
  });
}

int qi_widen(int device, const void* in, void* out, int64_t count, qi_stream stream) {
  QI_REQUIRE(in && out && count > 0, "bad argument");
  DeviceGuard g(device);
  return launch_widen((const float*)in, (double*)out, count, (hipStream_t)stream);
}

int qi_log2_abs(int dtype, int device, const void* in, int is_complex, void* out, int64_t count, double eps,
                qi_stream stream) {
  QI_REQUIRE(in && out, "null argument");
  QI_REQUIRE(dtype == QI_F32 || dtype == QI_F64, "bad dtype %d", dtype);
  QI_REQUIRE(count > 0, "bad shape");
  DeviceGuard g(device);
  return by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    return launch_log2_abs<T>((const T*)in, is_complex, (T*)out, count, (T)eps, (hipStream_t)stream);
  });
}

int qi_shannon_panel(int dtype, int device, const void* power, const void* mult, int mode, int64_t C, int64_t B,
                     int64_t n, double deg_free, void* info, void* shannon_bits, void* isnr, void* esnr,
                     qi_stream stream) {
  QI_REQUIRE(power && mult, "null argument");
  QI_REQUIRE(dtype == QI_F32 || dtype == QI_F64, "bad dtype %d", dtype);
  QI_REQUIRE(mode >= 0 && mode <= 2, "bad mode %d", mode);
  QI_REQUIRE(C > 0 && B > 0 && n > 0 && deg_free > 1.0, "bad shape");
  DeviceGuard g(device);
  return by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    return launch_shannon<T>((const T*)power, (const T*)mult, mode, C, B, n, deg_free, (T*)info, (T*)shannon_bits, (T*)isnr,
                             (T*)esnr, (hipStream_t)stream);
  });
}

// ---- 1-D Shannon family ---------------------------------------------------------------------------------------------
int qi_shannon_1d(int dtype, int device, const void* marginal, int64_t C, int64_t n, void* info, void* entropy,
                  void* isnr, void* esnr, qi_stream stream) {
  QI_REQUIRE(marginal, "null argument");
  QI_REQUIRE(dtype == QI_F32 || dtype == QI_F64, "bad dtype %d", dtype);
  QI_REQUIRE(C > 0 && n > 1, "bad shape");
  DeviceGuard g(device);
  return by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    return launch_shannon_1d<T>((const T*)marginal, C, n, (T*)info, (T*)entropy, (T*)isnr, (T*)esnr, (hipStream_t)stream);
  });
}

int64_t qi_shannon_scratch_bytes(int dtype, int64_t C, int64_t n) {
  if (C <= 0 || n <= 1) return 0;
  const int64_t nf = n / 2 + 1, esz = dtype == QI_F64 ? 8 : 4;
  // partial sums | unwrap turns | a copy of the records (the real-to-complex transform may overwrite its input)
  return (int64_t)(align_up((size_t)C * shannon_spans(n) * 8) + align_up((size_t)C * nf * 4) + align_up((size_t)C * n * esz));
}

int qi_shannon_tdr(int dtype, int device, const void* sig, int64_t C, int64_t n, void* sig_norm, void* marginal,
                   void* scratch, int64_t scratch_bytes, qi_stream stream) {
  QI_REQUIRE(sig && marginal && scratch, "null argument");
  QI_REQUIRE(dtype == QI_F32 || dtype == QI_F64, "bad dtype %d", dtype);
  QI_REQUIRE(C > 0 && n > 1, "bad shape");
  QI_REQUIRE(scratch_bytes >= qi_shannon_scratch_bytes(dtype, C, n), "scratch too small");
  DeviceGuard g(device);
  return by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    return launch_tdr_marginal<T>((const T*)sig, C, n, (T*)sig_norm, (T*)marginal, static_cast<double*>(scratch),
                                  (hipStream_t)stream);
  });
}

int qi_shannon_fft(int dtype, int device, const void* sig, int64_t C, int64_t n, void* spectrum, void* angle,
                   void* marginal, void* scratch, int64_t scratch_bytes, qi_stream stream) {
  QI_REQUIRE(sig && spectrum && marginal && scratch, "null argument");
  QI_REQUIRE(dtype == QI_F32 || dtype == QI_F64, "bad dtype %d", dtype);
  QI_REQUIRE(C > 0 && n > 1, "bad shape");
  QI_REQUIRE(scratch_bytes >= qi_shannon_scratch_bytes(dtype, C, n), "scratch too small");
  DeviceGuard g(device);
  hipStream_t st = (hipStream_t)stream;
  const int64_t nf = n / 2 + 1;
  char* s = static_cast<char*>(scratch);
  double* partial = reinterpret_cast<double*>(s);
  int32_t* turns = reinterpret_cast<int32_t*>(s + align_up((size_t)C * shannon_spans(n) * 8));
  return by_dtype(dtype, [&](auto t) -> int {
    using T = decltype(t);
    T* copy = reinterpret_cast<T*>(s + align_up((size_t)C * shannon_spans(n) * 8) + align_up((size_t)C * nf * 4));
    QI_HIP(hipMemcpyAsync(copy, sig, (size_t)C * n * sizeof(T), hipMemcpyDeviceToDevice, st));
    QI_TRY(locked_fft(device, [&](FftCache& fc) { return fft_r2c<T>(fc, copy, (cplx<T>*)spectrum, n, C, st); }));
    return launch_fft_marginal<T>((cplx<T>*)spectrum, C, nf, (T*)angle, (T*)marginal, partial, turns, st);
  });
}

// ---- sliding-window STFT in scipy.signal.ShortTimeFFT's convention ---------------------------------------------------
int64_t qi_sliding_scratch_bytes(int dtype, int64_t C, int64_t nfft, int64_t n_slices) {
  if (C <= 0 || nfft <= 0 || n_slices <= 0) return 0;
  return (int64_t)FftScratch(dtype, C, n_slices, nfft).total;
}

int qi_sliding_stft(int dtype, int device, const void* sig, int64_t C, int64_t n, const void* window, int64_t seg,
                    int64_t hop, int64_t nfft, int64_t first, int64_t n_slices, int pad_mode, int detrend, int64_t roll,
                    void* Z, void* real_out, int real_kind, void* scratch, int64_t scratch_bytes, qi_stream stream) {
  QI_REQUIRE(sig && window && scratch && (Z || real_out), "null argument");
  QI_REQUIRE(dtype == QI_F32 || dtype == QI_F64, "bad dtype %d", dtype);
  QI_REQUIRE(C > 0 && n > 0 && seg > 0 && hop > 0 && nfft >= seg && n_slices > 0 && roll >= 0 && roll < nfft, "bad shape");
  QI_REQUIRE(pad_mode >= 0 && pad_mode <= 3 && (real_kind == 1 || real_kind == 2 || !real_out), "bad mode");
  QI_REQUIRE(pad_mode < 2 || (-first <= n - 1 && first + (n_slices - 1) * hop + seg - n <= n - 1),
             "reflective padding reaches further than the record is long");
  QI_REQUIRE(scratch_bytes >= qi_sliding_scratch_bytes(dtype, C, nfft, n_slices), "scratch too small");
  DeviceGuard g(device);
  hipStream_t st = (hipStream_t)stream;
  StftRequest rq{C, n, seg, hop, nfft, n_slices, -first};
  rq.pad_mode = pad_mode;
  rq.detrend = detrend;
  rq.real_kind = real_out ? real_kind : 0;
  rq.roll = roll;
  return by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    const T *x = (const T*)sig, *w = (const T*)window;
    return fused_or_hipfft(
        stft_fused_supported(dtype, seg, hop, nfft),
        // one kernel: slices (padding mode, optional detrend), transform, phase roll, [frequency][slice] store
        [&] { return launch_stft_fused<T>(rq, x, w, (cplx<T>*)Z, (T*)real_out, st); },
        [&] { return stft_hipfft<T>(device, rq, x, w, (cplx<T>*)Z, (T*)real_out, (char*)scratch, st); });
  });
}

int qi_sliding_istft(int dtype, int device, const void* S, int64_t C, const void* dual_window, int64_t seg, int64_t hop,
                     int64_t nfft, int64_t first, int64_t n_slices, int64_t roll, int64_t k0, int64_t k1, void* out,
                     void* scratch, int64_t scratch_bytes, qi_stream stream) {
  QI_REQUIRE(S && dual_window && out && scratch, "null argument");
  QI_REQUIRE(dtype == QI_F32 || dtype == QI_F64, "bad dtype %d", dtype);
  QI_REQUIRE(C > 0 && seg > 0 && hop > 0 && nfft >= seg && n_slices > 0 && k1 > k0 && roll >= 0 && roll < nfft, "bad shape");
  QI_REQUIRE(scratch_bytes >= qi_sliding_scratch_bytes(dtype, C, nfft, n_slices), "scratch too small");
  DeviceGuard g(device);
  hipStream_t st = (hipStream_t)stream;
  const FftScratch l(dtype, C, n_slices, nfft);
  return by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    const cplx<T>* spec = (const cplx<T>*)S;
    const T* dual = (const T*)dual_window;
    return fused_or_hipfft(
        true,  // (the launcher knows the geometries it takes: not other transform lengths, nor a halo that fills the LDS)
        // one kernel: fold, inverse transform in LDS, overlap-add in gather form
        [&] { return launch_istft_fused<T>(spec, dual, (T*)out, C, seg, hop, nfft, first, n_slices, roll, k0, k1, st); },
        [&]() -> int {  // un-transpose -> hipFFT -> overlap-add
          T* slices = reinterpret_cast<T*>((char*)scratch + l.frames);
          cplx<T>* F = reinterpret_cast<cplx<T>*>((char*)scratch + l.spectra);
          QI_TRY(launch_sliding_untranspose<T>(spec, F, C, n_slices, nfft / 2 + 1, st));
          QI_TRY(locked_fft(device, [&](FftCache& fc) { return fft_c2r<T>(fc, F, slices, nfft, C * n_slices, st); }));
          return launch_sliding_overlap_add<T>(slices, dual, (T*)out, C, k0, k1, seg, hop, nfft, n_slices, first, roll, st);
        });
  });
}

}  // extern "C"
