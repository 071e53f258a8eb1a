// Host sanitizer walk of the STFT segment-range entry points (qi_stft_range_samples, qi_stft_range_scratch_bytes,
// qi_stft_out_range): the library's translation units compiled for the HOST ONLY under AddressSanitizer + UBSan and linked with
// the stand-in HIP runtime of tests/sanitize (kernels do not run, device memory is host memory).  Every item of three records
// (two fused geometries, one hipFFT) in both precisions, with and without panels, with pooling factors that give launch groups
// of 1, 2, 4 and the full group, each with rows of exactly n_avail samples (NULL where a range needs none), outputs of exactly
// the stated sizes and scratch of exactly the advertised size; then every single-fault refusal.  Built and run by
// tests/test_stft_stream_sanitize.py on the CPU container; never part of libqi_tfr.so.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "qi_host.hpp"

extern "C" const char* __lsan_default_suppressions() { return "leak:stft_twiddles\nleak:strip_partials\n"; }
extern "C" const char* __lsan_default_options() { return "print_suppressions=0"; }

namespace {

struct Geo {
  int64_t seg, hop, nfft, n, per_item;
};

void* dev(size_t bytes) {
  void* p = nullptr;
  if (hipMalloc(&p, std::max<size_t>(bytes, 1)) != hipSuccess) exit(2);
  return p;
}

[[noreturn]] void die(const char* what, int dtype, const Geo& g, int64_t first, int64_t F) {
  fprintf(stderr, "walk_stream: %s (%s, seg %lld hop %lld nfft %lld, first segment %lld, factor %lld): %s\n", what, dtype ? "f64" : "f32",
          (long long)g.seg, (long long)g.hop, (long long)g.nfft, (long long)first, (long long)F, qi_last_error());
  exit(1);
}

}  // namespace

int main() {
  const Geo geos[] = {{512, 256, 512, 512 + 40 * 256 + 5, 16}, {201, 101, 256, 3001, 12}, {200, 100, 300, 601, 3}, {512, 500, 512, 600, 1}};
  const int64_t C = 3;
  size_t accepted = 0, refused = 0;
  for (int dtype : {(int)QI_F32, (int)QI_F64})
    for (const Geo& g : geos) {
      const size_t e = dtype == QI_F64 ? 8 : 4;
      const int64_t nf = g.nfft / 2 + 1, total = qi_stft_segments(g.n, g.seg, g.hop);
      void* win = dev(g.seg * e);
      for (int64_t F : {(int64_t)0, (int64_t)2, (int64_t)3, (int64_t)4, (int64_t)12, g.per_item})
        for (int64_t first = 0; first < total; first += g.per_item) {
          if (F == 1 || (F > 0 && g.per_item % F != 0)) continue;
          qi_stft_range r{};
          r.n_total = g.n;
          r.first_segment = first;
          r.segments = std::min(g.per_item, total - first);
          if (qi_stft_range_samples(g.n, g.seg, g.hop, first, r.segments, &r.sample0, &r.n_avail) != QI_OK) die("range_samples", dtype, g, first, F);
          r.row_stride = r.n_avail;
          r.pool_factor = F;
          const int64_t windows = F ? r.segments / F : 0;
          void* sig = r.n_avail ? dev(C * r.n_avail * e) : nullptr;
          void *Z = dev(C * nf * r.segments * 2 * e), *bits = dev(C * nf * r.segments * e), *pt = dev(C * r.segments * e);
          void *pb = dev(C * nf * 8), *stats = dev(C * 4 * 8);
          void *mean = windows ? dev(C * nf * windows * e) : nullptr, *mx = windows ? dev(C * nf * windows * e) : nullptr;
          r.pool_mean = mean;
          r.pool_max = mx;
          qi_tfr_out panel{}, reduced{};
          panel.coef = Z;
          panel.bits = bits;
          panel.power_time = reduced.power_time = pt;
          panel.power_band = reduced.power_band = pb;
          panel.stats = reduced.stats = stats;
          for (const qi_tfr_out* out : {&panel, &reduced}) {
            const int64_t sb = qi_stft_range_scratch_bytes(dtype, C, g.seg, g.hop, g.nfft, &r, out->coef != nullptr);
            if (sb < 0) die("scratch_bytes", dtype, g, first, F);
            void* scratch = dev(sb);
            if (qi_stft_out_range(dtype, 0, sig, C, win, g.seg, g.hop, g.nfft, 0.5, &r, out, scratch, sb, nullptr) != QI_OK)
              die("qi_stft_out_range", dtype, g, first, F);
            (void)hipFree(scratch);
            ++accepted;
          }
          // single faults: each refused with QI_ERR_ARG (scratch as large as any accepted call's)
          const int64_t sb = qi_stft_range_scratch_bytes(dtype, C, g.seg, g.hop, g.nfft, &r, 0);
          void* scratch = dev(sb);
          std::vector<qi_stft_range> bad;
          auto with = [&](auto&& edit) {
            qi_stft_range b = r;
            edit(b);
            bad.push_back(b);
          };
          with([](qi_stft_range& b) { b.segments += 1000000; });
          with([](qi_stft_range& b) { b.first_segment = -1; });
          with([](qi_stft_range& b) { b.segments = 0; });
          with([](qi_stft_range& b) { b.row_stride = b.n_avail - 1; });
          with([](qi_stft_range& b) { b.sample0 = -1; });
          with([](qi_stft_range& b) { b.n_avail = b.n_total + 1; });
          with([](qi_stft_range& b) { b.n_total = 0; });
          with([](qi_stft_range& b) { b.pool_factor = 1; });
          if (r.n_avail > 0) {
            with([](qi_stft_range& b) { b.n_avail -= 1; });
            with([](qi_stft_range& b) { b.sample0 += 1, b.n_avail -= 1; });
          }
          if (F > 1 && first + F < total) with([](qi_stft_range& b) { b.first_segment += 1, b.segments = 1; });
          if (F == 0) with([&](qi_stft_range& b) { b.pool_mean = pb; });
          for (const qi_stft_range& b : bad) {
            if (qi_stft_out_range(dtype, 0, sig, C, win, g.seg, g.hop, g.nfft, 0.5, &b, &reduced, scratch, sb, nullptr) != QI_ERR_ARG)
              die("a faulty range was not refused", dtype, g, first, F);
            if (qi_stft_range_scratch_bytes(dtype, C, g.seg, g.hop, g.nfft, &b, 0) != QI_ERR_ARG) die("scratch of a faulty range", dtype, g, first, F);
            ++refused;
          }
          if (sb > 0 && qi_stft_out_range(dtype, 0, sig, C, win, g.seg, g.hop, g.nfft, 0.5, &r, &reduced, scratch, sb - 1, nullptr) != QI_ERR_ARG)
            die("short scratch was not refused", dtype, g, first, F);
          for (void* q : {sig, Z, bits, pt, pb, stats, mean, mx, scratch})
            if (q) (void)hipFree(q);
        }
      (void)hipFree(win);
    }
  for (auto& kv : qi::g_stft_fft) kv.second.clear();  // (the process-wide hipFFT plans: nothing frees them before the leak check)
  printf("{\"ok\": true, \"accepted\": %zu, \"refused\": %zu}\n", accepted, refused);
  return 0;
}
