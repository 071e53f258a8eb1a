// What tests/sanitize/walk.cpp and tests/sanitize_threads/walk_threads.cpp share: the band-table file of gen_tables.py, and the
// plan-less calls of walk_stft() and walk_records().  Included once per program, inside nothing: everything here is in an
// unnamed namespace.  Test infrastructure; never part of libqi_tfr.so.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "qi_host.hpp"

namespace {

struct Config {
  int32_t order, log2n, dtype, B, B2, flags;  // B: Gabor table, B2: Stockwell table; log2n: -1 where n is no power of two
  int64_t n;
  std::vector<int64_t> records, ws;
  std::vector<double> p_re, p_im, omega, amp, sigma;
  std::vector<int64_t> idx;
};

std::vector<Config> read_tables(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) {
    perror(path);
    exit(2);
  }
  int32_t head[4];
  if (fread(head, 4, 4, f) != 4 || head[0] != 0x51495354 || (head[3] != 2 && head[3] != 3)) exit(2);
  std::vector<Config> out((size_t)head[1]);
  for (auto& c : out) {
    int32_t h[6];
    if (fread(h, 4, 6, f) != 6) exit(2);
    c.order = h[0], c.log2n = h[1], c.dtype = h[2], c.B = h[3], c.B2 = h[4], c.flags = h[5];
    c.n = (int64_t)1 << c.log2n;
    if (head[3] == 3) {  // (format 3, gen_tables.py --engines: the field holds the record length itself)
      c.n = h[1];
      c.log2n = -1;
      for (int k = 0; k < 31; ++k)
        if (c.n == (int64_t)1 << k) c.log2n = k;
    }
    c.records.resize((size_t)head[2]);
    c.ws.resize((size_t)head[2]);
    if (fread(c.records.data(), 8, c.records.size(), f) != c.records.size()) exit(2);
    if (fread(c.ws.data(), 8, c.ws.size(), f) != c.ws.size()) exit(2);
    for (auto* v : {&c.p_re, &c.p_im, &c.omega, &c.amp}) {
      v->resize((size_t)c.B);
      if (fread(v->data(), 8, (size_t)c.B, f) != (size_t)c.B) exit(2);
    }
    c.sigma.resize((size_t)c.B2);
    c.idx.resize((size_t)c.B2);
    if (fread(c.sigma.data(), 8, (size_t)c.B2, f) != (size_t)c.B2) exit(2);
    if (fread(c.idx.data(), 8, (size_t)c.B2, f) != (size_t)c.B2) exit(2);
  }
  fclose(f);
  return out;
}

// The plan-less STFT family (qi_api_ops.hip, the host half of qi_stft_fused.hip): every entry point once per precision on a
// geometry the fused kernels take and on one that goes through frames -> hipFFT -> finish, with scratch of EXACTLY the
// advertised size (AddressSanitizer's malloc: a pointer carved past it that anything touches is a report), so that UBSan and the
// stand-in's launch-geometry check see the request, shape, scratch-layout and launch arithmetic.  Returns the calls made.
// `geos`: the geometries (default: kStftGeos); `st`: the stream of every call; `clear_cache`: a program with one thread frees the
// process-wide hipFFT plans behind itself, one with several does it once at its end.
struct StftGeo {
  int64_t seg, hop, nfft, n;
};
const std::vector<StftGeo> kStftGeos = {{256, 64, 256, 3 * 256 + 1} /* fused */, {200, 50, 300, 601} /* hipFFT */,
                                        {2048, 512, 2048, 3 * 2048 + 1} /* fused, fewer segments per workgroup */};
size_t walk_stft(const std::vector<StftGeo>& geos = kStftGeos, hipStream_t st = nullptr, bool clear_cache = true) {
  using Geo = StftGeo;
  const int64_t C = 3;
  size_t calls = 0;
  auto need = [](int rc, const char* what, int dtype, const Geo& g) {
    if (rc == QI_OK) return;
    fprintf(stderr, "walk: %s (%s, seg %lld hop %lld nfft %lld): %s\n", what, dtype ? "f64" : "f32", (long long)g.seg, (long long)g.hop,
            (long long)g.nfft, qi_last_error());
    exit(1);
  };
  auto dev = [](size_t bytes) {
    void* p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) exit(2);
    return p;
  };
  for (int dtype : {(int)QI_F32, (int)QI_F64})
    for (const Geo& g : geos) {
      const size_t e = dtype == QI_F64 ? 8 : 4;
      const int64_t nf = g.nfft / 2 + 1, nseg = qi_stft_segments(g.n, g.seg, g.hop);
      void *sig = dev(C * g.n * e), *win = dev(g.seg * e), *Z = dev(C * nf * nseg * 2 * e), *bits = dev(C * nf * nseg * e);
      void *pt = dev(C * nseg * e), *pb = dev(C * nf * 8), *stats = dev(C * 4 * 8), *pxx = dev(C * nf * e);
      int64_t sb = qi_stft_scratch_bytes(dtype, C, g.n, g.seg, g.hop, g.nfft);
      void* scratch = dev(sb);
      need(qi_stft(dtype, 0, sig, C, g.n, win, g.seg, g.hop, g.nfft, 0.5, Z, bits, 0.0, scratch, sb, st), "qi_stft", dtype, g);
      (void)hipFree(scratch);
      qi_tfr_out panel{}, bits_only{}, reduced{};
      panel.coef = Z;
      panel.bits = bits;
      panel.power_time = reduced.power_time = pt;
      panel.power_band = reduced.power_band = pb;
      panel.stats = reduced.stats = stats;
      bits_only.bits = bits;
      const struct {
        const qi_tfr_out* out;
        const char* what;
      } forms[] = {{&panel, "qi_stft_out (panels and reductions)"}, {&bits_only, "qi_stft_out (bits only)"}, {&reduced, "qi_stft_out (reductions only)"}};
      for (const auto& f : forms) {
        sb = qi_stft_out_scratch_bytes(dtype, C, g.n, g.seg, g.hop, g.nfft, f.out->coef != nullptr, f.out->bits != nullptr);
        scratch = dev(sb);
        need(qi_stft_out(dtype, 0, sig, C, g.n, win, g.seg, g.hop, g.nfft, 0.5, f.out, scratch, sb, st), f.what, dtype, g);
        (void)hipFree(scratch);
      }
      sb = qi_welch_scratch_bytes(dtype, C, g.n, g.seg, g.hop, g.nfft);
      scratch = dev(sb);
      need(qi_welch(dtype, 0, sig, C, g.n, win, g.seg, g.hop, g.nfft, 0.5, pxx, scratch, sb, st), "qi_welch", dtype, g);
      (void)hipFree(scratch);
      // ShortTimeFFT convention: slices from half a segment in front of the record to half a segment behind it
      const int64_t first = -(g.seg / 2), slices = (g.n + g.seg) / g.hop + 1;
      void *S = dev(C * nf * slices * 2 * e), *R = dev(C * nf * slices * e), *back = dev(C * g.n * e);
      sb = qi_sliding_scratch_bytes(dtype, C, g.nfft, slices);
      scratch = dev(sb);
      need(qi_sliding_stft(dtype, 0, sig, C, g.n, win, g.seg, g.hop, g.nfft, first, slices, 1, 1, g.seg / 2, S, R, 2, scratch, sb, st),
           "qi_sliding_stft", dtype, g);
      need(qi_sliding_istft(dtype, 0, S, C, win, g.seg, g.hop, g.nfft, first, slices, g.seg / 2, 0, g.n, back, scratch, sb, st),
           "qi_sliding_istft", dtype, g);
      calls += 7;
      for (void* q : {sig, win, Z, bits, pt, pb, stats, pxx, S, R, back, scratch}) (void)hipFree(q);
    }
  if (clear_cache)
    for (auto& kv : g_stft_fft) kv.second.clear();  // (the process-wide hipFFT plans: nothing frees them before the leak check)
  return calls;
}

// The plan-less record calls (qi_filter.hip, qi_peaks.hip, qi_resample.hip, qi_calculus.hip): each entry point accepted once per
// precision (the calls with timestamps also with a row per record) on caller buffers and scratch of EXACTLY the sizes the
// ABI states, then every single-fault refusal of tests/test_*_cpu.py through the call itself: QI_ERR_ARG and the word the
// message must hold.  Kernels do not run here, so the exact sizes are seen by the host code only: the size and pointer
// arithmetic under UBSan, the copies and memsets the host issues (qi_resample_fft's copy of the records) under
// AddressSanitizer.  Returns the calls made.
struct Rec {  // the arguments of one record call; an entry point reads the ones it takes
  int dtype = QI_F64, kind = QI_DERIV_GRADIENT;
  int64_t C = 3, n = 300, m = 77, stride = 0, edge = 27, q = 4, offset = 0, capacity = 16, scratch_short = 0;
  double start = 0.25, delta = 0.5;
  bool with_x = false;        // qi_cumtrapz, qi_derivative: timestamps given
  hipStream_t st = nullptr;   // the stream of the call
  const char* null_arg = "";  // the pointer argument passed as null
  template <typename T, typename V>
  Rec with(T Rec::*field, V v) const {
    Rec r = *this;
    r.*field = (T)v;
    return r;
  }
  // sizes of the caller's buffers: the stated ones, for the shapes a call accepts (a refused call touches none of them)
  int64_t e() const { return dtype == QI_F32 ? 4 : 8; }
  int64_t rows(int64_t per_row) const {
    return std::min<int64_t>(std::max<int64_t>(C, 0), 64) * std::min<int64_t>(std::max<int64_t>(per_row, 0), 4096);
  }
};
struct Dev {  // a "device" buffer of exactly `bytes`: AddressSanitizer's malloc behind the stand-in's hipMalloc
  void* p = nullptr;
  explicit Dev(int64_t bytes) {
    if (hipMalloc(&p, (size_t)std::max<int64_t>(bytes, 1)) != hipSuccess) exit(2);
  }
  Dev(const Dev&) = delete;
  ~Dev() { (void)hipFree(p); }
  void* unless(const Rec& r, const char* name) const { return strcmp(r.null_arg, name) ? p : nullptr; }
};
const double kUnitSos64[6] = {1, 0, 0, 1, 0, 0}, kZi64[2] = {0, 0};
const float kUnitSos32[6] = {1, 0, 0, 1, 0, 0}, kZi32[2] = {0, 0};

int rec_filtfilt(const Rec& r) {
  const int64_t need = qi_filtfilt_scratch_bytes(r.C, r.n, r.edge);
  Dev sig(r.rows(r.n) * r.e()), out(r.rows(r.n) * 8), scratch(need - r.scratch_short);
  return qi_filtfilt(r.dtype, 0, sig.unless(r, "sig"), r.C, r.n, nullptr, QI_IIR_SOS, 1, 2, kUnitSos64, kZi64, r.edge, out.unless(r, "out"),
                     scratch.unless(r, "scratch"), need - r.scratch_short, r.st);
}
int rec_decimate(const Rec& r) {
  const int64_t need = qi_decimate_scratch_bytes(r.dtype, r.C, r.n, r.edge);
  Dev sig(r.rows(r.n) * r.e()), out(r.rows(qi_decimate_columns(r.n, r.q)) * r.e()), scratch(need - r.scratch_short);
  const bool f32 = r.dtype == QI_F32;
  return qi_decimate(r.dtype, 0, sig.unless(r, "sig"), r.C, r.n, r.q, 1, f32 ? (const void*)kUnitSos32 : kUnitSos64,
                     f32 ? (const void*)kZi32 : kZi64, r.edge, out.unless(r, "out"), scratch.unless(r, "scratch"), need - r.scratch_short, r.st);
}
int rec_find_peaks(const Rec& r) {
  const int64_t need = qi_peaks_scratch_bytes(r.dtype, r.C, r.n);
  Dev sig(r.rows(r.n) * r.e()), scaled(r.rows(r.n) * r.e()), pos(r.rows(r.capacity) * 8), val(r.rows(r.capacity) * 8), counts(r.rows(1) * 8),
      scratch(need - r.scratch_short);
  return qi_find_peaks(r.dtype, 0, sig.unless(r, "sig"), r.C, r.n, QI_PEAK_SIGMAX, 0.0, QI_PEAK_HEIGHT_NONE, 0.0, scaled.p,
                       static_cast<int64_t*>(pos.p), static_cast<double*>(val.p), r.capacity, static_cast<int64_t*>(counts.unless(r, "counts")),
                       scratch.unless(r, "scratch"), need - r.scratch_short, r.st);
}
int rec_interp_grid(const Rec& r) {
  Dev values(r.rows(r.n) * r.e()), knots((r.stride ? r.rows(r.n) : std::max<int64_t>(r.n, 0)) * 8), out(r.rows(r.m) * 8);
  return qi_interp_grid(r.dtype, 0, values.unless(r, "values"), knots.unless(r, "knots"), r.stride, r.C, r.n, r.start, r.delta, r.m,
                        out.unless(r, "out"), r.st);
}
int rec_resample_fft(const Rec& r) {
  const int64_t need = qi_resample_fft_scratch_bytes(r.dtype, r.C, r.n, r.m);
  Dev sig(r.rows(r.n) * r.e()), out(r.rows(r.m) * r.e()), scratch(need - r.scratch_short);
  return qi_resample_fft(r.dtype, 0, sig.unless(r, "sig"), r.C, r.n, r.m, out.unless(r, "out"), scratch.unless(r, "scratch"),
                         need - r.scratch_short, r.st);
}
int rec_cumtrapz(const Rec& r) {
  const int64_t need = qi_cumtrapz_scratch_bytes(r.dtype, r.C, r.n);
  Dev y(r.rows(r.n) * r.e()), x((r.stride ? r.rows(r.n) : std::max<int64_t>(r.n, 0)) * 8), out(r.rows(r.n) * (r.with_x ? 8 : r.e())),
      scratch(need - r.scratch_short);
  return qi_cumtrapz(r.dtype, 0, y.unless(r, "y"), r.with_x ? x.p : nullptr, r.stride, 1.0, r.C, r.n, out.unless(r, "out"),
                     scratch.unless(r, "scratch"), need - r.scratch_short, r.st);
}
int rec_derivative(const Rec& r) {
  Dev y(r.rows(r.n) * r.e()), x((r.stride ? r.rows(r.n) : std::max<int64_t>(r.n, 0)) * 8),
      out(r.rows(r.n) * (r.with_x && r.kind == QI_DERIV_DIFFERENCE ? 8 : r.e()));
  return qi_derivative(r.dtype, 0, r.kind, y.unless(r, "y"), r.with_x ? x.p : nullptr, r.stride, 1.0, r.C, r.n, out.unless(r, "out"), r.offset,
                       r.st);
}

size_t walk_records(hipStream_t st = nullptr, bool clear_cache = true) {
  struct Case {
    const char* name;
    int (*call)(const Rec&);
    Rec r;
    const char* word;  // of the refusal's message; null: the call is accepted
  };
  std::vector<Case> cases;
  const Rec base = Rec().with(&Rec::st, st);
  for (int dtype : {(int)QI_F32, (int)QI_F64}) {
    const Rec d = base.with(&Rec::dtype, dtype), rows = d.with(&Rec::stride, d.n), timed = rows.with(&Rec::with_x, true);
    cases.insert(cases.end(), {{"qi_filtfilt", rec_filtfilt, d, nullptr},
                               {"qi_decimate", rec_decimate, d, nullptr},
                               {"qi_find_peaks", rec_find_peaks, d, nullptr},
                               {"qi_interp_grid (shared timestamps)", rec_interp_grid, d, nullptr},
                               {"qi_interp_grid (timestamps per record)", rec_interp_grid, rows, nullptr},
                               {"qi_resample_fft", rec_resample_fft, d, nullptr},
                               {"qi_cumtrapz (dx)", rec_cumtrapz, d, nullptr},
                               {"qi_cumtrapz (timestamps per record)", rec_cumtrapz, timed, nullptr},
                               {"qi_derivative (gradient, h)", rec_derivative, d, nullptr},
                               {"qi_derivative (difference, timestamps per record, filled at the start)", rec_derivative,
                                timed.with(&Rec::kind, QI_DERIV_DIFFERENCE).with(&Rec::offset, 1), nullptr}});
  }
  // no records, or one sample and no difference: successful no-ops
  cases.push_back({"qi_cumtrapz (no records)", rec_cumtrapz, base.with(&Rec::C, 0), nullptr});
  cases.push_back({"qi_derivative (no records)", rec_derivative, base.with(&Rec::C, 0), nullptr});
  cases.push_back({"qi_derivative (difference of one sample)", rec_derivative, base.with(&Rec::kind, QI_DERIV_DIFFERENCE).with(&Rec::n, 1), nullptr});
  const double nan = std::nan(""), inf = HUGE_VAL;
  const Rec bad_dtype = base.with(&Rec::dtype, 2), none = base.with(&Rec::C, 0), empty = base.with(&Rec::n, 0),
            short_scratch = base.with(&Rec::scratch_short, 8), x = base.with(&Rec::with_x, true), diff = base.with(&Rec::kind, QI_DERIV_DIFFERENCE);
  auto null = [&](const char* arg) { return base.with(&Rec::null_arg, arg); };
  cases.insert(cases.end(), {
      {"qi_filtfilt", rec_filtfilt, bad_dtype, "dtype"},
      {"qi_filtfilt", rec_filtfilt, none, "record count"},
      {"qi_filtfilt", rec_filtfilt, base.with(&Rec::n, base.edge), "longer"},
      {"qi_filtfilt", rec_filtfilt, base.with(&Rec::edge, -1), "longer"},
      {"qi_filtfilt", rec_filtfilt, null("sig"), "null"},
      {"qi_filtfilt", rec_filtfilt, null("out"), "null"},
      {"qi_filtfilt", rec_filtfilt, null("scratch"), "null"},
      {"qi_filtfilt", rec_filtfilt, short_scratch, "needed"},
      {"qi_decimate", rec_decimate, bad_dtype, "dtype"},
      {"qi_decimate", rec_decimate, none, "record count"},
      {"qi_decimate", rec_decimate, base.with(&Rec::n, base.edge), "longer"},
      {"qi_decimate", rec_decimate, base.with(&Rec::edge, -1), "longer"},
      {"qi_decimate", rec_decimate, base.with(&Rec::q, 0), "positive"},
      {"qi_decimate", rec_decimate, null("sig"), "null"},
      {"qi_decimate", rec_decimate, null("out"), "null"},
      {"qi_decimate", rec_decimate, null("scratch"), "null"},
      {"qi_decimate", rec_decimate, short_scratch, "needed"},
      {"qi_find_peaks", rec_find_peaks, bad_dtype, "dtype"},
      {"qi_find_peaks", rec_find_peaks, none, "record count"},
      {"qi_find_peaks", rec_find_peaks, empty, "record length"},
      {"qi_find_peaks", rec_find_peaks, base.with(&Rec::C, 1ll << 30).with(&Rec::n, 1ll << 20), "too large"},
      {"qi_find_peaks", rec_find_peaks, base.with(&Rec::capacity, -1), "capacity"},
      {"qi_find_peaks", rec_find_peaks, null("sig"), "null"},
      {"qi_find_peaks", rec_find_peaks, null("counts"), "null"},
      {"qi_find_peaks", rec_find_peaks, null("scratch"), "null"},
      {"qi_find_peaks", rec_find_peaks, short_scratch, "needed"},
      {"qi_interp_grid", rec_interp_grid, bad_dtype, "dtype"},
      {"qi_interp_grid", rec_interp_grid, empty, "record length"},
      {"qi_interp_grid", rec_interp_grid, base.with(&Rec::m, -1), "output length"},
      {"qi_interp_grid", rec_interp_grid, none, "record count"},
      {"qi_interp_grid", rec_interp_grid, base.with(&Rec::delta, 0.0), "delta"},
      {"qi_interp_grid", rec_interp_grid, base.with(&Rec::delta, -1.0), "delta"},
      {"qi_interp_grid", rec_interp_grid, base.with(&Rec::delta, nan), "delta"},
      {"qi_interp_grid", rec_interp_grid, base.with(&Rec::delta, inf), "delta"},
      {"qi_interp_grid", rec_interp_grid, base.with(&Rec::start, nan), "start"},
      {"qi_interp_grid", rec_interp_grid, base.with(&Rec::start, -inf), "start"},
      {"qi_interp_grid", rec_interp_grid, base.with(&Rec::stride, 4), "knot_stride"},
      {"qi_interp_grid", rec_interp_grid, base.with(&Rec::stride, -8), "knot_stride"},
      {"qi_interp_grid", rec_interp_grid, null("values"), "null"},
      {"qi_interp_grid", rec_interp_grid, null("knots"), "null"},
      {"qi_interp_grid", rec_interp_grid, null("out"), "null"},
      {"qi_resample_fft", rec_resample_fft, bad_dtype, "dtype"},
      {"qi_resample_fft", rec_resample_fft, none, "record count"},
      {"qi_resample_fft", rec_resample_fft, empty, "record length"},
      {"qi_resample_fft", rec_resample_fft, base.with(&Rec::m, 0), "output length"},
      {"qi_resample_fft", rec_resample_fft, base.with(&Rec::n, 1ll << 31), "too large"},
      {"qi_resample_fft", rec_resample_fft, null("scratch"), "null"},
      {"qi_resample_fft", rec_resample_fft, short_scratch, "needed"},
      {"qi_cumtrapz", rec_cumtrapz, bad_dtype, "dtype"},
      {"qi_cumtrapz", rec_cumtrapz, empty, "record length"},
      {"qi_cumtrapz", rec_cumtrapz, base.with(&Rec::C, -1), "record count"},
      {"qi_cumtrapz", rec_cumtrapz, x.with(&Rec::stride, 4), "x_stride"},
      {"qi_cumtrapz", rec_cumtrapz, x.with(&Rec::stride, -8), "x_stride"},
      {"qi_cumtrapz", rec_cumtrapz, base.with(&Rec::stride, base.n), "x_stride"},
      {"qi_cumtrapz", rec_cumtrapz, null("y"), "null"},
      {"qi_cumtrapz", rec_cumtrapz, null("out"), "null"},
      {"qi_cumtrapz", rec_cumtrapz, null("scratch"), "null"},
      {"qi_cumtrapz", rec_cumtrapz, short_scratch, "needed"},
      {"qi_derivative", rec_derivative, bad_dtype, "dtype"},
      {"qi_derivative", rec_derivative, base.with(&Rec::kind, 2), "kind"},
      {"qi_derivative", rec_derivative, empty, "record length"},
      {"qi_derivative", rec_derivative, base.with(&Rec::n, 1), "gradient"},
      {"qi_derivative", rec_derivative, diff.with(&Rec::n, 0), "record length"},
      {"qi_derivative", rec_derivative, base.with(&Rec::C, -1), "record count"},
      {"qi_derivative", rec_derivative, x.with(&Rec::stride, 4), "x_stride"},
      {"qi_derivative", rec_derivative, base.with(&Rec::stride, base.n), "x_stride"},
      {"qi_derivative", rec_derivative, base.with(&Rec::offset, 1), "out_offset"},
      {"qi_derivative", rec_derivative, diff.with(&Rec::offset, 2), "out_offset"},
      {"qi_derivative", rec_derivative, diff.with(&Rec::offset, -1), "out_offset"},
      {"qi_derivative", rec_derivative, null("y"), "null"},
      {"qi_derivative", rec_derivative, null("out"), "null"}});
  for (const Case& c : cases) {
    const int rc = c.call(c.r);
    if (c.word ? rc == QI_ERR_ARG && strstr(qi_last_error(), c.word) : rc == QI_OK) continue;
    fprintf(stderr, "walk: %s (dtype %d, %lld records of %lld samples): status %d where %s%s was expected: %s\n", c.name, c.r.dtype,
            (long long)c.r.C, (long long)c.r.n, rc, c.word ? "a refusal naming " : "success", c.word ? c.word : "", qi_last_error());
    exit(1);
  }
  if (clear_cache)
    for (auto& kv : g_stft_fft) kv.second.clear();  // (qi_resample_fft's hipFFT plans live in the process-wide cache)
  return cases.size();
}

}  // namespace
