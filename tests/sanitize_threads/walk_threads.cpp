// Host thread walk: the library's translation units compiled for the HOST ONLY under ThreadSanitizer and linked with the
// stand-in HIP runtime of tests/sanitize (kernels do not run, device memory is host memory), driven through the C ABI by four
// threads at once.  What the threads share is what the library keeps for the process: the hipFFT cache of the plan-less entry
// points and its work areas per stream (g_stft_fft under g_stft_mu), the strip partials per (device, stream) (g_strip_part),
// the static maps of allow_dynamic_lds and stft_twiddles, and -- per thread by design -- the text behind qi_last_error.
// Everything else is a thread's own: its two streams, its plans, its caller buffers.  A barrier releases the threads in front of
// each of the two loops, so that their first uses of the shared state collide.  Per loop a thread makes
//   * the plan-less calls that share process state: walk_stft()'s and walk_records()'s (walk_calls.hpp) -- the short-time family
//     also at a fused nfft no thread has used before (stft_twiddles inserts under contention) and at hipFFT lengths that differ by
//     thread and loop (FftCache::get inserts and grows the work areas while another thread binds) --, qi_shannon_fft, qi_csd,
//     qi_cross_spectra -- and in front of them, straight behind the barrier, qi_pool_strip with S > 1 partials per row on both
//     of its streams (new per loop: g_strip_part inserts under contention), each followed by qi_pool_strip_stats;
//   * plans of its own: one per layout of tests/stream_cases.py's ENGINES (gen_tables.py --engines) and record count, created,
//     given its tables, run (qi_cwt_stx, qi_cwt, qi_stx with panels and with reductions only) and destroyed -- each thread
//     starts at another layout, so one thread builds or destroys while another launches;
//   * one refused call whose message names the thread, and reads its own text back from qi_last_error.
// A race ThreadSanitizer reports in the library's host code is a finding.  Built and run by tests/test_host_threads_sanitize.py
// on the CPU; never part of libqi_tfr.so, never run on a GPU.
#include <atomic>
#include <condition_variable>
#include <mutex>
#include <thread>

#include "qi_array.h"
#include "walk_calls.hpp"

extern "C" size_t qi_fake_hip_launches();
extern "C" int qi_fake_hip_fft_handles();

namespace {

constexpr int kThreads = 4, kLoops = 2;

struct Barrier {  // (C++17: no std::barrier)
  std::mutex mu;
  std::condition_variable cv;
  int waiting = 0, generation = 0;
  void wait() {
    std::unique_lock<std::mutex> lk(mu);
    const int gen = generation;
    if (++waiting == kThreads) {
      waiting = 0;
      ++generation;
      cv.notify_all();
    } else {
      cv.wait(lk, [&] { return gen != generation; });
    }
  }
};

struct Counts {
  size_t plans = 0, plan_calls = 0, stft_calls = 0, record_calls = 0, fft_calls = 0, strip_calls = 0, own_errors = 0;
};

[[noreturn]] void fail(int t, const char* what) {
  fprintf(stderr, "walk_threads: thread %d: %s: %s\n", t, what, qi_last_error());
  exit(1);
}

void* dev(size_t bytes) {
  void* p = nullptr;
  if (hipMalloc(&p, std::max<size_t>(bytes, 1)) != hipSuccess) exit(2);
  return p;
}

// S of launch_strip (qi_pool.hip), as tests/stream_cases.py's strip_segments states it
int64_t strip_segments(int64_t rows, int64_t windows, int64_t factor) {
  const int64_t gmin = factor < 64 ? 256 : (factor <= 1024 ? 4 : 1);
  const int64_t groups = std::max(gmin, (rows * windows + 4095) / 4096);
  return (windows + groups - 1) / groups;
}

// the fused and hipFFT geometries of thread t in loop `loop`, in front of walk_stft()'s own
std::vector<StftGeo> stft_geos(int t, int loop) {
  const int64_t fresh[kThreads] = {64, 128, 512, 1024};  // nfft no other thread uses (walk_stft's own: 256 and 2048)
  const int64_t odd = 300 + 20 * t + 10 * loop;          // no power of two: hipFFT, a length per thread and loop
  std::vector<StftGeo> geos = {{fresh[t], fresh[t] / 4, fresh[t], 3 * fresh[t] + 1}, {200, 50, odd, 601 + t}};
  geos.insert(geos.end(), kStftGeos.begin(), kStftGeos.end());
  return geos;
}

// qi_pool_strip with partials to fold (tests/stream_cases.py: STRIP) on both streams of the thread, then the statistics.  The
// first calls behind a barrier: the streams are new, so every thread inserts into g_strip_part at once, with no lock of the
// stand-in runtime taken in between (the buffers are made in front of the barrier).
struct StripBuffers {
  static constexpr int64_t records = 2, bands = 3, rows = records * bands, stride = 2100, factor = 2, windows = 1050;
  void *in, *mean, *peak, *sums, *stats;
  StripBuffers() : in(dev(rows * stride * 16)), mean(dev(rows * windows * 8)), peak(dev(rows * windows * 8)), sums(dev(rows * 3 * 8)),
                   stats(dev(records * 4 * 8)) {}
  ~StripBuffers() {
    for (void* q : {in, mean, peak, sums, stats}) (void)hipFree(q);
  }
};
void strip_calls(int t, const StripBuffers& b, hipStream_t st, hipStream_t st2, Counts& k) {
  using B = StripBuffers;
  for (int dtype : {(int)QI_F32, (int)QI_F64})
    for (hipStream_t s : {st, st2}) {
      if (qi_pool_strip(dtype, 0, b.in, B::rows, B::stride, 0, B::factor, B::windows, 2.0, b.mean, b.peak, B::windows, b.sums, s) != QI_OK)
        fail(t, "qi_pool_strip");
      if (qi_pool_strip_stats(0, b.sums, B::records, B::bands, b.stats, s) != QI_OK) fail(t, "qi_pool_strip_stats");
      k.strip_calls += 2;
    }
}

void planless_calls(int t, int loop, hipStream_t st, Counts& k) {
  k.stft_calls += walk_stft(stft_geos(t, loop), st, false);
  k.record_calls += walk_records(st, false);
  const int64_t C = 3;
  for (int dtype : {(int)QI_F32, (int)QI_F64}) {
    const size_t e = dtype == QI_F64 ? 8 : 4;
    {  // qi_shannon_fft: a length per thread and loop (a new hipFFT plan each time)
      const int64_t n = 1000 + 14 * t + 100 * loop, nf = n / 2 + 1, sb = qi_shannon_scratch_bytes(dtype, C, n);
      void *sig = dev(C * n * e), *spec = dev(C * nf * 2 * e), *angle = dev(C * nf * e), *marg = dev(C * nf * e), *scratch = dev(sb);
      if (sb < 0 || qi_shannon_fft(dtype, 0, sig, C, n, spec, angle, marg, scratch, sb, st) != QI_OK) fail(t, "qi_shannon_fft");
      for (void* q : {sig, spec, angle, marg, scratch}) (void)hipFree(q);
      ++k.fft_calls;
    }
    for (const StftGeo& g : {StftGeo{256, 128, 256, 3 * 256 + 1}, StftGeo{200, 100, 310 + 20 * t + 10 * loop, 601}}) {  // qi_csd: fused, hipFFT
      const int64_t R = 5, nf = g.nfft / 2 + 1, sb = qi_csd_scratch_bytes(dtype, R, g.n, g.seg, g.hop, g.nfft);
      void *sig = dev(R * g.n * e), *win = dev(g.seg * e), *csd = dev(nf * R * R * 2 * e), *coh = dev(nf * R * R * e), *scratch = dev(sb);
      if (sb < 0 || qi_csd(dtype, 0, sig, R, g.n, win, g.seg, g.hop, g.nfft, 0.5, csd, coh, scratch, sb, st) != QI_OK) fail(t, "qi_csd");
      for (void* q : {sig, win, csd, coh, scratch}) (void)hipFree(q);
      ++k.fft_calls;
    }
    {  // qi_cross_spectra: the matrices, then the coherence with host weights
      const int64_t R = 5, nf = 7, cols = 300, sb = qi_cross_spectra_scratch_bytes(dtype, R, nf, cols);
      const double weight[7] = {0.5, 0.75, 1.0, 1.25, 1.5, 1.75, 2.0};
      void *Z = dev(R * nf * cols * 2 * e), *csd = dev(nf * R * R * 2 * e), *coh = dev(nf * R * R * e), *scratch = dev(sb);
      if (sb < 0 || qi_cross_spectra(dtype, 0, Z, R, nf, cols, nullptr, csd, nullptr, scratch, sb, st) != QI_OK ||
          qi_cross_spectra(dtype, 0, Z, R, nf, cols, weight, nullptr, coh, scratch, sb, st) != QI_OK)
        fail(t, "qi_cross_spectra");
      for (void* q : {Z, csd, coh, scratch}) (void)hipFree(q);
      k.fft_calls += 2;
    }
  }
}

void plan_calls(int t, const std::vector<Config>& configs, hipStream_t st, Counts& k) {
  for (size_t i = 0; i < configs.size(); ++i) {
    const Config& c = configs[(i + (size_t)t) % configs.size()];  // each thread starts at another layout
    const size_t rsz = c.dtype ? 8 : 4, Bm = (size_t)std::max(c.B, c.B2);
    for (size_t r = 0; r < c.records.size(); ++r) {
      const int64_t C = c.records[r], n = c.n;
      if (C <= 0) continue;
      qi_plan_desc desc{};
      desc.n = n;
      desc.dtype = c.dtype;
      desc.engine = QI_ENGINE_AUTO;
      desc.workspace_bytes = c.ws[r];
      qi_plan* p = nullptr;
      if (qi_plan_create(&p, &desc) != QI_OK) fail(t, "qi_plan_create");
      if (qi_plan_set_gabor_bank(p, QI_BANK_STYX, c.B, c.p_re.data(), c.p_im.data(), c.omega.data(), c.amp.data(), st) != QI_OK)
        fail(t, "qi_plan_set_gabor_bank");
      if (qi_plan_set_stx_bands(p, c.B2, c.idx.data(), c.sigma.data()) != QI_OK) fail(t, "qi_plan_set_stx_bands");
      ++k.plans;
      const size_t panel = (size_t)C * Bm * (size_t)n, red_bytes = (size_t)C * (Bm + 4) * 8 + (size_t)C * (size_t)n * rsz;
      void *sig = dev((size_t)C * n * rsz), *coef0 = dev(panel * 2 * rsz), *coef2 = dev(panel * 2 * rsz), *bits = dev(panel * rsz),
           *red = dev(2 * red_bytes);
      auto outs = [&](void* coef, void* b, int which) {
        qi_tfr_out o{};
        o.coef = coef;
        o.bits = b;
        char* base = static_cast<char*>(red) + (size_t)which * red_bytes;
        o.power_time = base;
        o.power_band = base + (size_t)C * n * rsz;
        o.stats = base + (size_t)C * n * rsz + (size_t)C * Bm * 8;
        return o;
      };
      const qi_tfr_out full0 = outs(coef0, bits, 0), full2 = outs(coef2, nullptr, 1), lean0 = outs(nullptr, nullptr, 0),
                       lean2 = outs(nullptr, nullptr, 1);
      if (qi_cwt_stx(p, QI_BANK_STYX, sig, C, &full0, &full2, st) != QI_OK) fail(t, "qi_cwt_stx (panels)");
      if (qi_cwt(p, QI_BANK_STYX, sig, C, &full0, st) != QI_OK) fail(t, "qi_cwt (panels)");
      if (qi_stx(p, sig, C, &full2, st) != QI_OK) fail(t, "qi_stx (panels)");
      if (qi_cwt_stx(p, QI_BANK_STYX, sig, C, &lean0, &lean2, st) != QI_OK) fail(t, "qi_cwt_stx (reductions only)");
      if (qi_cwt(p, QI_BANK_STYX, sig, C, &lean0, st) != QI_OK) fail(t, "qi_cwt (reductions only)");
      if (qi_stx(p, sig, C, &lean2, st) != QI_OK) fail(t, "qi_stx (reductions only)");
      k.plan_calls += 6;
      for (void* q : {sig, coef0, coef2, bits, red}) (void)hipFree(q);
      if (qi_plan_destroy(p) != QI_OK) fail(t, "qi_plan_destroy");
    }
  }
}

// a refusal whose message names the thread and the loop; the text this thread reads back must be its own
void own_error(int t, int loop, Counts& k) {
  const long long bad = -(1000 + 10 * t + loop);
  char want[64];
  snprintf(want, sizeof(want), "bad output length %lld", bad);
  if (qi_resample_fft_scratch_bytes(QI_F64, 1, 100, bad) != QI_ERR_ARG) fail(t, "a negative output length was not refused");
  std::this_thread::yield();
  if (strcmp(qi_last_error(), want) != 0) fail(t, "qi_last_error does not hold this thread's text");
  ++k.own_errors;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: walk_threads engines.bin   (gen_tables.py --engines engines.bin)\n");
    return 2;
  }
  const std::vector<Config> configs = read_tables(argv[1]);
  Barrier barrier;
  Counts counts[kThreads];
  std::vector<std::thread> threads;
  for (int t = 0; t < kThreads; ++t)
    threads.emplace_back([&, t] {
      if (strip_segments(StripBuffers::rows, StripBuffers::windows, StripBuffers::factor) != 5) fail(t, "strip shape: S = 5 partials per row expected");
      for (int loop = 0; loop < kLoops; ++loop) {
        hipStream_t st = nullptr, st2 = nullptr;  // (new ones per loop: the per-stream state is made again)
        if (hipStreamCreateWithFlags(&st, 0) != hipSuccess || hipStreamCreateWithFlags(&st2, 0) != hipSuccess) exit(2);
        {
          const StripBuffers strip;
          barrier.wait();
          strip_calls(t, strip, st, st2, counts[t]);
        }
        planless_calls(t, loop, st, counts[t]);
        plan_calls(t, configs, st, counts[t]);
        own_error(t, loop, counts[t]);
        (void)hipStreamDestroy(st);
        (void)hipStreamDestroy(st2);
      }
    });
  for (auto& th : threads) th.join();
  Counts sum;
  for (const Counts& c : counts) {
    sum.plans += c.plans, sum.plan_calls += c.plan_calls, sum.stft_calls += c.stft_calls, sum.record_calls += c.record_calls;
    sum.fft_calls += c.fft_calls, sum.strip_calls += c.strip_calls, sum.own_errors += c.own_errors;
  }
  size_t cached = 0;
  for (auto& kv : qi::g_stft_fft) {
    cached += kv.second.plans.size();
    kv.second.clear();
  }
  printf("{\"ok\": true, \"threads\": %d, \"loops\": %d, \"layouts\": %zu, \"plans\": %zu, \"plan_calls\": %zu, \"stft_calls\": %zu, "
         "\"record_calls\": %zu, \"fft_calls\": %zu, \"strip_calls\": %zu, \"own_errors\": %zu, \"kernel_launches\": %zu, "
         "\"shared_fft_plans\": %zu, \"fft_handles_left\": %d}\n",
         kThreads, kLoops, configs.size(), sum.plans, sum.plan_calls, sum.stft_calls, sum.record_calls, sum.fft_calls, sum.strip_calls,
         sum.own_errors, qi_fake_hip_launches(), cached, qi_fake_hip_fft_handles());
  return 0;
}
