// Host sanitizer walk ("build variants with -fsanitize=address for host code").  The library's translation units,
// compiled for the HOST ONLY under AddressSanitizer + UndefinedBehaviorSanitizer and linked with a stand-in HIP runtime
// (fake_hip.cpp: kernels do not run, device memory is host memory), are driven through the C ABI over every
//   order 1 .. 12  x  record length 2^14 .. 2^22  x  float32 / float64  x  1 / 4 / 16 / 64 records
// with the band tables the Python host code makes (gen_tables.py) and the scratch TfrPlan.workspace_for sizes for that batch,
// and behind them over the synthetic tables of tests/band_tables.py (not constant-Q; 1 / 4 / 16 records):
// plan build (band assignment, zoom classes, block item lists, split bands), qi_cwt_stx / qi_cwt / qi_stx with several output
// sets -- panels, bits, full and band-only reductions -- (scratch carving, tiles, joint launches, launch geometry).  Checked on the way:
//   * every scratch region a run carves lies inside the workspace and no two live regions overlap (QI_LAYOUT_* hooks in
//     qi_run.hip -> layout_note, qi_host_util.hip);
//   * every table upload stays inside its allocation (AddressSanitizer on the malloc'ed "device" tables);
//   * the block engine's work-item lists: each band's blocks cover the record exactly once, planes and statistics slots are
//     in range and unique, the joint list of qi_cwt_stx holds every item of both tables exactly once;
//   * qi_plan_band_route names exactly one producer for every row of every table, and the producers sum to the band count;
//   * a synthetic table comes out as gen_tables.py says it must (every row on the native engines / the whole table on hipFFT);
//   * degenerate band parameters (sigma or p_re of 0, negative, NaN, inf; NaN omega; a shift index outside [0, n)) are refused
//     with QI_ERR_ARG and a message, and leave the plan's previous table in use;
//   * the plan-less STFT family (qi_stft, qi_stft_out, qi_welch, qi_sliding_stft, qi_sliding_istft) on fused and hipFFT geometries in
//     both precisions, each with scratch of exactly the advertised size (walk_stft);
//   * the plan-less record calls (qi_filtfilt, qi_decimate, qi_find_peaks, qi_interp_grid, qi_resample_fft, qi_cumtrapz,
//     qi_derivative): the host code of an accepted call on buffers of exactly the stated sizes in both precisions, and every
//     single-fault refusal (walk_records);
//   * launch geometry (fake hipLaunchKernel), signed overflow / shifts / misaligned access in the host arithmetic (UBSan).
// Test infrastructure: built and run by tests/test_host_sanitize.py on the CPU container; never part of libqi_tfr.so.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>

#include "qi_host.hpp"
#include "walk_calls.hpp"

extern "C" size_t qi_fake_hip_launches();
// the fused STFT's twiddle tables are kept per device for the life of the process, by design: not a leak to report
extern "C" const char* __lsan_default_suppressions() { return "leak:stft_twiddles\n"; }
extern "C" const char* __lsan_default_options() { return "print_suppressions=0"; }
extern "C" size_t qi_layout_regions_checked();

namespace {

// (Config, read_tables, walk_stft and walk_records: walk_calls.hpp)
[[noreturn]] void die(const char* what, const Config& c, int64_t C) {
  fprintf(stderr, "walk: %s (order %d, 2^%d samples, %s, %lld records): %s\n", what, c.order, c.log2n, c.dtype ? "f64" : "f32",
          (long long)C, qi_last_error());
  exit(1);
}

// the block engine's item lists of table `kind`, cut `v`
void check_block_items(const qi_plan* p, int kind, int v, const Config& c) {
  const auto& bt = p->blk[kind];
  if (!bt.ready) return;
  const auto& il = bt.var[v];
  const int64_t n = p->n;
  const size_t total = (size_t)il.nitems + (size_t)il.nedge_items;
  if (il.h_items.size() != total) die("block item list: host copy and counts disagree", c, 0);
  std::set<int32_t> slots;
  // (band position in the list, block) pairs seen, per reach code
  std::set<std::pair<int64_t, int64_t>> seen;
  std::vector<int64_t> blocks_of_band;  // by list position
  int32_t nlong = 0;
  for (size_t i = 0; i < total; ++i) {
    const auto& it = il.h_items[i];
    if (!slots.insert(it.stat_slot).second || it.stat_slot < 0 || it.stat_slot >= (int32_t)total) die("block items: statistics slot", c, 0);
    if (it.plane < 0 || it.plane >= il.nplanes) die("block items: per-time plane out of range", c, 0);
    if (i < (size_t)il.nitems) {
      if (it.wq != 1 && it.wq != 2 && it.wq != 4 && it.wq != qi::native::kBlkLongWq) die("block items: reach code", c, 0);
      if (it.wq == qi::native::kBlkLongWq) {
        if ((int32_t)i != nlong) die("block items: long-block items must lead the list", c, 0);
        ++nlong;
      }
      const int64_t V = qi::native::block_valid(it.wq), nb = (n + V - 1) / V;
      if (it.block < 0 || it.block >= nb || it.band_count <= 0 || it.band_first < 0) die("block items: block / band range", c, 0);
      for (int32_t b = it.band_first; b < it.band_first + it.band_count; ++b) {
        if (!seen.insert({b, it.block}).second) die("block items: a (band, block) pair twice", c, 0);
        if ((size_t)b >= blocks_of_band.size()) blocks_of_band.resize((size_t)b + 1, 0);
        blocks_of_band[(size_t)b] += 1;
      }
    } else {
      if (it.wq >= 0) die("block items: an edge item without a negative reach code", c, 0);
      const int64_t V = qi::native::block_valid(-it.wq), nb = (n + V - 1) / V;
      if (it.block < 0 || it.block >= nb) die("edge items: block out of range", c, 0);
    }
  }
  if (nlong != il.nlong) die("block items: long-block count", c, 0);
  // every band of the list has ALL blocks of its reach group: band positions are dense, counts equal a group's block count
  for (size_t b = 0; b < blocks_of_band.size(); ++b) {
    const int64_t got = blocks_of_band[b];
    bool ok = false;
    for (int wq : {1, 2, 4, (int)qi::native::kBlkLongWq}) ok = ok || got == (n + qi::native::block_valid(wq) - 1) / qi::native::block_valid(wq);
    if (!ok) die("block items: a band's blocks do not cover the record", c, 0);
  }
  if ((int32_t)blocks_of_band.size() != bt.rows && il.nitems > 0) die("block items: bands of the list vs rows of the table", c, 0);
}

void check_dual_items(const qi_plan* p, int cut, const Config& c) {
  if (!p->dual_valid[cut] || !p->d_dual[cut]) return;
  const auto& l0 = p->blk[0].var[cut];
  const auto& l2 = p->blk[2].var[cut];
  std::set<std::tuple<int, int, int, int>> want0, want2;  // (wq, block, first, count)
  for (int32_t i = 0; i < l0.nitems + l0.nedge_items; ++i) {
    const auto& it = l0.h_items[(size_t)i];
    want0.insert({it.wq, it.block, it.band_first, it.band_count});
  }
  for (int32_t i = 0; i < l2.nitems; ++i) {
    const auto& it = l2.h_items[(size_t)i];
    want2.insert({it.wq, it.block, it.band_first, it.band_count});
  }
  const qi::native::DualItem* d = p->d_dual[cut];  // ("device" memory is host memory here)
  for (int32_t i = 0; i < p->n_dual[cut]; ++i) {
    const auto& it = d[i];
    if (it.wq < 0 || it.count0 > 0) {
      if (want0.erase({it.wq, it.block, it.first0, it.count0}) != 1) die("joint items: a styx item that is not in the styx list (or twice)", c, 0);
    }
    if (it.wq > 0 && it.count2 > 0) {
      if (want2.erase({it.wq, it.block, it.first2, it.count2}) != 1) die("joint items: a Stockwell item that is not in its list (or twice)", c, 0);
    }
  }
  if (!want0.empty() || !want2.empty()) die("joint items: items of a table missing from the joint list", c, 0);
}

// qi_plan_band_route: one producer per row (it returns QI_ERR_STATE otherwise), and per stage as many rows as
// qi_plan_stage_bands counts; written to `dump` when the caller wants the routes
void check_routes(const qi_plan* p, int which, int64_t C, const Config& c, FILE* dump, size_t ci) {
  const int64_t B = qi_plan_bands(p, which);
  int64_t per_stage[QI_STAGE_COUNT] = {};
  for (int64_t j = 0; j < B; ++j) {
    qi_band_route r{};
    if (qi_plan_band_route(p, which, (int32_t)j, C, &r) != QI_OK) die("qi_plan_band_route", c, C);
    if (r.stage != QI_STAGE_ZOOM && r.stage != QI_STAGE_BLOCK && r.stage != QI_STAGE_PASS2 && r.stage != QI_STAGE_INVERSE)
      die("band route: not a producing stage", c, C);
    per_stage[r.stage] += 1;
    if (dump)
      fprintf(dump, "%zu %d %d %lld %d %lld %d %d %d %d\n", ci, c.log2n, c.dtype, (long long)C, which, (long long)j, r.stage, r.cls,
              r.run_cls, r.flags);
  }
  int64_t sum = 0;
  for (int s : {(int)QI_STAGE_ZOOM, (int)QI_STAGE_BLOCK, (int)QI_STAGE_PASS2, (int)QI_STAGE_INVERSE}) {
    if (per_stage[s] != qi_plan_stage_bands(p, which, s)) die("band route: rows per stage differ from qi_plan_stage_bands", c, C);
    sum += per_stage[s];
  }
  if (sum != B) die("band route: the producers do not sum to the band count", c, C);
}

// what gen_tables.py says a synthetic table must come out as: 1 every row on the native engines, 2 the whole table on hipFFT
void check_expectation(const qi_plan* p, int which, int expect, const Config& c, int64_t C) {
  const int64_t B = qi_plan_bands(p, which), inv = qi_plan_stage_bands(p, which, QI_STAGE_INVERSE);
  if (expect == 1 && inv != 0) die("synthetic table: rows on the hipFFT engine where none were expected", c, C);
  if (expect == 2 && inv != B) die("synthetic table: expected the whole table on the hipFFT engine", c, C);
}

// Degenerate band parameters: refused with QI_ERR_ARG and a message; the plan's previous tables stay in use.
size_t check_degenerate(const Config& c) {
  const int64_t n = (int64_t)1 << c.log2n;
  size_t refused = 0;
  qi_plan_desc desc{};
  desc.n = n;
  desc.dtype = c.dtype;
  desc.engine = QI_ENGINE_AUTO;
  desc.workspace_bytes = c.ws[0];
  qi_plan* p = nullptr;
  if (qi_plan_create(&p, &desc) != QI_OK) die("qi_plan_create", c, 1);
  if (qi_plan_set_gabor_bank(p, QI_BANK_STYX, c.B, c.p_re.data(), c.p_im.data(), c.omega.data(), c.amp.data(), nullptr) != QI_OK ||
      qi_plan_set_stx_bands(p, c.B2, c.idx.data(), c.sigma.data()) != QI_OK)
    die("degenerate parameters: the good tables", c, 1);
  const size_t rsz = c.dtype ? 8 : 4;
  void *sig = nullptr, *red = nullptr;
  const size_t Bm = (size_t)std::max(c.B, c.B2);
  if (hipMalloc(&sig, (size_t)n * rsz) != hipSuccess || hipMalloc(&red, (Bm + 4) * 8 + (size_t)n * rsz) != hipSuccess) die("caller buffers", c, 1);
  qi_tfr_out o{};
  o.power_time = red;
  o.power_band = static_cast<char*>(red) + (size_t)n * rsz;
  o.stats = static_cast<char*>(red) + (size_t)n * rsz + Bm * 8;
  auto still_usable = [&]() {
    if (qi_plan_bands(p, 0) != c.B || qi_plan_bands(p, 2) != c.B2) die("degenerate parameters: the previous table is gone", c, 1);
    if (qi_cwt(p, QI_BANK_STYX, sig, 1, &o, nullptr) != QI_OK || qi_stx(p, sig, 1, &o, nullptr) != QI_OK)
      die("degenerate parameters: the previous table no longer runs", c, 1);
  };
  auto refuse = [&](int rc, const char* what) {
    if (rc != QI_ERR_ARG || !qi_last_error() || !qi_last_error()[0]) die(what, c, 1);
    ++refused;
    still_usable();
  };
  const double nan = std::nan(""), inf = HUGE_VAL;
  for (double bad : {0.0, -1.0, nan, inf, -inf}) {
    std::vector<double> sg = c.sigma;
    sg[sg.size() / 2] = bad;
    refuse(qi_plan_set_stx_bands(p, c.B2, c.idx.data(), sg.data()), "a degenerate sigma was not refused");
    std::vector<double> pr = c.p_re;
    pr[pr.size() / 2] = bad;
    refuse(qi_plan_set_gabor_bank(p, QI_BANK_STYX, c.B, pr.data(), c.p_im.data(), c.omega.data(), c.amp.data(), nullptr),
           "a degenerate p_re was not refused");
  }
  for (int which = 0; which < 3; ++which) {  // NaN p_im / omega / amp
    std::vector<double> v[3] = {c.p_im, c.omega, c.amp};
    v[which][0] = nan;
    refuse(qi_plan_set_gabor_bank(p, QI_BANK_STYX, c.B, c.p_re.data(), v[0].data(), v[1].data(), v[2].data(), nullptr),
           "a NaN atom parameter was not refused");
  }
  for (int64_t bad : {(int64_t)-1, n, n + 5, (int64_t)1 << 40}) {
    std::vector<int64_t> ix = c.idx;
    ix.back() = bad;
    refuse(qi_plan_set_stx_bands(p, c.B2, ix.data(), c.sigma.data()), "a shift index outside [0, n) was not refused");
  }
  (void)hipFree(sig);
  (void)hipFree(red);
  if (qi_plan_destroy(p) != QI_OK) die("qi_plan_destroy", c, 1);
  return refused;
}

void check_tables(const qi_plan* p, const Config& c) {
  for (int kind : {0, 2}) {
    const auto& t = p->nat[kind];
    if (!t.ready) continue;
    int64_t planes = 0;
    for (const auto& z : t.h_zoom) planes += ((t.Lf / qi::native::kZoomD) << qi::native::zoom_grid(z.second)) / qi::native::kBlk;
    if (planes != t.zoom_planes || (int32_t)t.h_zoom.size() != t.nzoom) die("zoom table: planes / band count", c, 0);
    // every panel row has exactly one producer: zoom / float64 zoom / block / two-pass (or the hipFFT pass behind the run)
    const int64_t B = kind == 2 ? p->nb_stx : p->nb[kind];
    const int64_t blk = p->blk[kind].ready ? p->blk[kind].rows : 0;
    const int64_t left = kind == 2 ? p->stx_left_n : 0;
    const int64_t shorts = kind == 0 && p->nat[3].ready ? p->nedge : 0;
    if (t.nzoom + t.nz64 + blk + (int64_t)t.h_rows.size() + left + shorts != B) die("table: producers do not add up to the panel's rows", c, 0);
    for (int v = 0; v < 2; ++v) check_block_items(p, kind, v, c);
  }
}


}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: walk tables.bin [max configs (0: all)] [file to write every band's route to: config, log2n, dtype, records, table, band, stage, cls, run_cls, flags]\n");
    return 2;
  }
  const auto configs = read_tables(argv[1]);
  const size_t limit = argc > 2 && atoll(argv[2]) > 0 ? (size_t)atoll(argv[2]) : configs.size();
  FILE* dump = argc > 3 ? fopen(argv[3], "w") : nullptr;
  size_t plans = 0, calls = 0, native = 0, syn_plans = 0, syn_native = 0, refused = 0;
  for (size_t ci = 0; ci < configs.size() && ci < limit; ++ci) {
    const Config& c = configs[ci];
    const int64_t n = (int64_t)1 << c.log2n;
    const size_t rsz = c.dtype ? 8 : 4;
    for (size_t r = 0; r < c.records.size(); ++r) {
      const int64_t C = c.records[r];
      if (C <= 0) continue;  // (a slot this config does not use)
      qi_plan_desc desc{};
      desc.n = n;
      desc.dtype = c.dtype;
      desc.device = 0;
      desc.engine = QI_ENGINE_AUTO;
      desc.workspace_bytes = c.ws[r];
      qi_plan* p = nullptr;
      if (qi_plan_create(&p, &desc) != QI_OK) die("qi_plan_create", c, C);
      if (qi_plan_set_gabor_bank(p, QI_BANK_STYX, c.B, c.p_re.data(), c.p_im.data(), c.omega.data(), c.amp.data(), nullptr) != QI_OK)
        die("qi_plan_set_gabor_bank", c, C);
      if (qi_plan_set_stx_bands(p, c.B2, c.idx.data(), c.sigma.data()) != QI_OK) die("qi_plan_set_stx_bands", c, C);
      ++plans;
      native += p->nat[0].ready && p->nat[2].ready;
      if (c.order == 0) {
        ++syn_plans;
        syn_native += p->nat[0].ready && p->nat[2].ready;
        check_expectation(p, 0, c.flags & 3, c, C);
        check_expectation(p, 2, (c.flags >> 2) & 3, c, C);
      }
      check_tables(p, c);
      check_routes(p, 0, C, c, dump, ci);
      check_routes(p, 2, C, c, dump, ci);
      // caller buffers: records, panels (address-space reservations), reduced products
      void *sig = nullptr, *coef0 = nullptr, *coef2 = nullptr, *bits = nullptr, *red = nullptr;
      const size_t Bm = (size_t)std::max(c.B, c.B2);  // (caller buffers sized for the larger of the two tables)
      const size_t panel = (size_t)C * Bm * n;
      if (hipMalloc(&sig, (size_t)C * n * rsz) != hipSuccess || hipMalloc(&coef0, panel * 2 * rsz) != hipSuccess ||
          hipMalloc(&coef2, panel * 2 * rsz) != hipSuccess || hipMalloc(&bits, panel * rsz) != hipSuccess ||
          hipMalloc(&red, 2 * ((size_t)C * (Bm + 4) * 8 + (size_t)C * n * rsz)) != hipSuccess)
        die("caller buffers", c, C);
      char* rp = static_cast<char*>(red);
      auto outs = [&](void* coef, void* b, bool reductions, int which) {
        qi_tfr_out o{};
        o.coef = coef;
        o.bits = b;
        if (reductions) {
          char* base = rp + (size_t)which * ((size_t)C * (Bm + 4) * 8 + (size_t)C * n * rsz);
          o.power_time = base;
          o.power_band = base + (size_t)C * n * rsz;
          o.stats = base + (size_t)C * n * rsz + (size_t)C * Bm * 8;
        }
        return o;
      };
      const qi_tfr_out a0 = outs(coef0, nullptr, true, 0), a2 = outs(coef2, nullptr, true, 1);
      if (qi_cwt_stx(p, QI_BANK_STYX, sig, C, &a0, &a2, nullptr) != QI_OK) die("qi_cwt_stx", c, C);
      for (int cut = 0; cut < 2; ++cut) check_dual_items(p, cut, c);
      const qi_tfr_out lean0 = outs(nullptr, nullptr, true, 0), lean2 = outs(nullptr, nullptr, true, 1);
      if (qi_cwt_stx(p, QI_BANK_STYX, sig, C, &lean0, &lean2, nullptr) != QI_OK) die("qi_cwt_stx (reductions only)", c, C);
      const qi_tfr_out full = outs(coef0, bits, true, 0), bare = outs(coef2, nullptr, false, 1);
      if (qi_cwt(p, QI_BANK_STYX, sig, C, &full, nullptr) != QI_OK) die("qi_cwt (coefficients, bits, reductions)", c, C);
      if (qi_stx(p, sig, C, &bare, nullptr) != QI_OK) die("qi_stx (coefficients only)", c, C);
      if (qi_stx(p, sig, C, &full, nullptr) != QI_OK) die("qi_stx (coefficients, bits, reductions)", c, C);
      calls += 5;
      {  // band powers and statistics without the per-time marginal (engine: reductions="band", the streaming pipeline's request)
        qi_tfr_out b0 = lean0, b2 = lean2, bf = full;
        b0.power_time = b2.power_time = bf.power_time = nullptr;
        if (qi_cwt_stx(p, QI_BANK_STYX, sig, C, &b0, &b2, nullptr) != QI_OK) die("qi_cwt_stx (band-only reductions)", c, C);
        if (qi_cwt(p, QI_BANK_STYX, sig, C, &bf, nullptr) != QI_OK) die("qi_cwt (coefficients, bits, band-only reductions)", c, C);
        if (qi_stx(p, sig, C, &b2, nullptr) != QI_OK) die("qi_stx (band-only reductions)", c, C);
        calls += 3;
      }
      if ((C == 4 && c.order == 3) || (c.flags & 16)) {  // the atoms bank (cwt_atoms: circular kind) on a few shapes, then the plan's tables again
        if (qi_plan_set_gabor_bank(p, QI_BANK_ATOMS, c.B, c.p_re.data(), c.p_im.data(), c.omega.data(), c.amp.data(), nullptr) != QI_OK)
          die("qi_plan_set_gabor_bank (atoms)", c, C);
        if (c.order == 0) check_expectation(p, 1, c.flags & 3, c, C);
        check_routes(p, 1, C, c, dump, ci);
        if (qi_cwt(p, QI_BANK_ATOMS, sig, C, &full, nullptr) != QI_OK) die("qi_cwt (atoms bank)", c, C);
        ++calls;
      }
      for (void* q : {sig, coef0, coef2, bits, red}) (void)hipFree(q);
      if (qi_plan_destroy(p) != QI_OK) die("qi_plan_destroy", c, C);
    }
    if ((ci & 15) == 15) fprintf(stderr, "walk: %zu of %zu tables done\n", ci + 1, configs.size());
    if (c.order == 0 && (c.flags & 15) == 5) refused += check_degenerate(c);  // (on the synthetic tables that are native on both sides)
  }
  if (dump) fclose(dump);
  const size_t stft_calls = walk_stft(), record_calls = walk_records();
  printf("{\"ok\": true, \"stft_calls\": %zu, \"record_calls\": %zu, \"plans\": %zu, \"plans_on_native_engines\": %zu, \"calls\": %zu, \"kernel_launches\": %zu, \"scratch_regions_checked\": %zu, \"synthetic_plans\": %zu, "
         "\"synthetic_on_native\": %zu, \"degenerate_tables_refused\": %zu}\n",
         stft_calls, record_calls, plans, native, calls, qi_fake_hip_launches(), qi_layout_regions_checked(), syn_plans, syn_native, refused);
  return 0;
}
