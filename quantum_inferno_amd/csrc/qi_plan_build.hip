// The tables of a plan: support analysis of the atom spectra, assignment of every band to an engine (zoom classes, block
// reach groups, split bands, two-pass groups), the device tables and work-item lists of those engines.
#include <algorithm>

#include "qi_host.hpp"

using namespace qi;

namespace qi {
namespace host {

bool native_len_ok(int64_t Lf) { return Lf == (1ll << 20) || Lf == (1ll << 21); }

// low-bins forward transform: the rule (see qi_host.hpp).  Evaluated from the tables on every run, so replacing a table
// re-evaluates it.
int64_t table_low_bins(const qi_plan* p, int kind) {
  const auto& t = p->nat[kind];
  if (!t.ready || p->d.dtype != QI_F32 || !p->native_fwd || !p->native_fwd_low || !native_len_ok(t.Lf)) return 0;
  // the two-pass kernels and the short-atom sub-table read the spectrum as a whole array
  if (!t.h_rows.empty() || (kind == 0 && p->nat[3].ready && p->nedge > 0)) return 0;
  const int64_t kmax = native::fwd_low_bins(t.Lf);  // what the pruned second pass forms: Lf / 64 (2K = Lf / 32 <= Lf / 8)
  int64_t K = 1;
  while (K <= kmax && !(t.x_lo > -K && t.x_hi < K)) K *= 2;
  return K <= kmax ? K : 0;
}
bool forward_low(const qi_plan* p) {
  if (p->d.dtype != QI_F32) return false;
  bool any = false;
  for (int kind = 0; kind < 3; ++kind) {
    if (!p->nat[kind].ready) continue;
    if (table_low_bins(p, kind) == 0) return false;
    any = true;
  }
  return any;
}

// does this plan run transform `kind` (0 styx bank, 1 atoms bank, 2 Stockwell) on the native engine?
bool native_wanted(const qi_plan* p, int kind) {
  if (p->d.engine == QI_ENGINE_HIPFFT) return false;
  const int64_t Lf = kind == 0 ? p->L : p->n;
  if (p->d.dtype == QI_F64 && !p->native_f64) return false;
  if (is_pow2(p->n) && native_len_ok(Lf)) return true;
  // Stockwell and styx tables usually have no band for the two-pass kernels (every band is a zoom, block or split
  // band), and those engines -- in float32 and, since round 4, their float64 twins (float64 zoom, k_block64, split bands) --
  // take any power-of-two length from 2^15: the table build decides
  return kind != 1 && is_pow2(p->n) && p->n >= ((int64_t)1 << p->native_min_log2n) && Lf <= (1ll << 26);
}

// ---- small-record engine: the rule and the twiddle table ---------------------------------------------------------------
bool small_wanted(const qi_plan* p, int kind) {
  if (p->d.engine != QI_ENGINE_AUTO || !p->small_tw || !is_pow2(p->n)) return false;
  if (p->n < (1 << 10) || p->n > (1 << 13) || p->n >= ((int64_t)1 << p->native_min_log2n)) return false;
  return native::small_len_ok(kind == 0 ? p->L : p->n, p->d.dtype == QI_F64 ? sizeof(double2) : sizeof(float2));
}
bool on_small(const qi_plan* p, int kind) {
  const int32_t bands = kind == 2 ? p->nb_stx : p->nb[kind];
  return bands > 0 && !p->nat[kind].ready && small_wanted(p, kind);
}
// exp(2 pi i k / 2n), k < n / 8: what the passes of an n- or 2n-point transform load (their other factors are products)
int build_small_twiddles(qi_plan* p) {
  const int64_t n = p->n;
  if (p->d.engine != QI_ENGINE_AUTO || !is_pow2(n) || n < (1 << 10) || n > (1 << 13)) return QI_OK;
  const int64_t len = 2 * n, count = len / 16;
  std::vector<double2> w((size_t)count);
  for (int64_t k = 0; k < count; ++k) {
    const double ph = 2.0 * M_PI * (double)k / (double)len;
    w[(size_t)k] = make_double2(std::cos(ph), std::sin(ph));
  }
  if (p->d.dtype == QI_F64) return upload_table(reinterpret_cast<double2**>(&p->small_tw), w);
  std::vector<float2> wf((size_t)count);
  for (int64_t k = 0; k < count; ++k) wf[(size_t)k] = make_float2((float)w[(size_t)k].x, (float)w[(size_t)k].y);
  return upload_table(reinterpret_cast<float2**>(&p->small_tw), wf);
}

// Widest spectrum support (bins) of a band that keeps a compact bank row: the one-pass loader's limit, or -- float64 with
// the float64 zoom engine, which then takes every such band -- the widest band its finest grid (Lf / 4 samples) still
// oversamples four times.
bool z64_table(const qi_plan* p, int table) { return p->d.dtype == QI_F64 && p->native_z64 && table != 3; }
int64_t narrow_limit(const qi_plan* p, int table, int64_t Lf) {
  return z64_table(p, table) ? std::max<int64_t>(native::kOnePassMax, Lf >> (9 - native::kZ64Levels)) : native::kOnePassMax;
}

// Records per call from which the block launches use their batch geometry (12 bands per workgroup, long blocks): fewer
// forward transforms and per-time planes against fewer, heavier workgroups.  Measured on one box: with the 18 block bands
// of an order-3 table the batch geometry pays from 8 records (+2 % at 4 and 6 records without it), with the 35 / 46 of
// orders 6 / 12 from 4 (+2-3 % with it).  The same answer for both tables of a joint call.
int batch_from(const qi_plan* p) {
  const int32_t rows = std::max(p->blk[0].ready ? p->blk[0].rows : 0, p->blk[2].ready ? p->blk[2].rows : 0);
  return rows <= 24 ? 8 : 4;
}

// ---- band-to-engine rules: every site that routes a band asks these ---------------------------------------------------
// occupied bins of a support triple {flag, first bin, last bin} (analyse_support)
int64_t support_len(const double* sup) {
  const int64_t lo = (int64_t)sup[1], hi = (int64_t)sup[2];
  return hi >= lo ? hi - lo + 1 : 0;
}
// A band's spectrum support ends where |H| falls below 2^-30 of the row maximum (float32 engines); float64 keeps everything
// above 2^-50.
double support_bits(const qi_plan* p) { return p->d.dtype == QI_F64 ? 50.0 : 30.0; }
// Taps of an atom and Gaussian filter weights below 2^-30 of the peak are dropped (float64: 2^-52).
double drop_bits(bool f64) { return f64 ? 52.0 : 30.0; }

// Zoom engine level of a band with `len` occupied bins out of Lf (-1: not eligible): the coarsest grid
// M_g = (Lf / 64) << g on which the band is oversampled at least 4 times.
int zoom_class(const qi_plan* p, int table, int64_t Lf, int64_t len) {
  if (!p->native_zoom || table == 3 || len <= 0 || Lf % native::kZoomD != 0) return -1;
  const int64_t M0 = Lf / native::kZoomD;
  if (!is_pow2(M0)) return -1;
  // the coarse stage works in 4096-point planes: a short record starts at the first grid level that fills one
  int g_min = 0;
  while ((M0 << g_min) < native::kBlk) ++g_min;
  for (int g = g_min; g < native::kZoomLevels; ++g) {
    if (p->n % ((int64_t)native::kZoomD * native::zoom_steps(g) * 4) != 0) return -1;
    if (native::kZoomOversample * len <= (M0 << g)) {
      // (the finest grid costs more in the coarse stage than the two-pass kernels save -- where those exist; at other
      // lengths it keeps the table off the hipFFT engine)
      if (g > p->native_zoom_max_level && native_len_ok(Lf)) return -1;
      // on the coarsest grid the band may be oversampled far more than 4 times: shorter interpolators (classes 5, 6)
      if (g == 0) {
        if ((int64_t)native::zoom_design_oversampling(6) * len <= M0) return 6;
        if ((int64_t)native::zoom_design_oversampling(5) * len <= M0) return 5;
      }
      return g;
    }
  }
  return -1;
}

// Float64 zoom level of a band with `len` occupied bins out of Lf (-1: the band is not for that engine): the coarsest grid
// (Lf / 64) << g, g < kZ64Levels, that oversamples it four times.  (The finest grid, Lf / 4 samples, is what
// narrow_limit allows at most: at transform lengths below 2^19 the one-pass loader's limit is wider than that.)
int z64_level(const qi_plan* p, int table, int64_t Lf, int64_t len) {
  if (!z64_table(p, table) || len <= 0 || len > narrow_limit(p, table, Lf)) return -1;
  for (int g = 0; g < native::kZ64Levels; ++g)
    if (4 * len <= ((Lf / 64) << g)) return g;
  return -1;
}
// ... and not on one of its finest grids when the block engine can take the band: a band of 65 536 - 131 072 bins costs
// the float64 zoom 13.5 us per record -- a 2^19-point coarse transform and the LDS-window interpolation kernel --
// against 7.4 us on the block engine, measured at order 12 x 4 records: native_z64_block_from
bool z64_level_for_block(const qi_plan* p, int level) { return level >= p->native_z64_block_from; }

// BandDesc::mode of a band that keeps a bank row: 2 + c zoom engine, class c; 0 a compact row (one-pass loader of pass 2;
// float64: the float64 zoom takes it from there, z64_level); 1 a full row for the two-pass kernels
int band_mode(const qi_plan* p, int table, int64_t Lf, int64_t len) {
  const int zc = zoom_class(p, table, Lf, len);
  if (zc >= 0) return 2 + zc;
  return len > 0 && len <= narrow_limit(p, table, Lf) ? 0 : 1;
}

// a band of the block engine
struct BlockPick {
  int32_t band;   // panel row
  int wq;         // reach group: taps within 256 * wq samples (1, 2 or 4)
  int64_t shift;  // Stockwell shift index (0 for Gabor banks)
  // analytic Gaussian filter spectrum (0: read the table row): weight(k) = amp exp2(-(cw (k - kappa))^2)
  int analytic = 0;
  double kappa = 0.0, cw = 0.0, amp = 0.0;
};
int block_group_of(double reach) { return reach <= 256.0 ? 1 : (reach <= 512.0 ? 2 : (reach <= 1024.0 ? 4 : 0)); }
// analytic Gaussian filter spectrum of a pure Gabor atom on the 4096-bin grid: amp sqrt(pi / p) exp(-d^2 / 4p) exp(-i theta / 2)
void gabor_gaussian(BlockPick& pk, double p_re, double om, double am) {
  pk.kappa = om * (double)native::kBlk / (2.0 * M_PI);
  pk.cw = (2.0 * M_PI / (double)native::kBlk) * std::sqrt(M_LOG2E / (4.0 * p_re));
  pk.amp = am * std::sqrt(M_PI / p_re) / (double)native::kBlk;
}
// ... of a Stockwell band: the Gaussian window itself, centred on the band's shift index
void stx_gaussian(BlockPick& pk, int64_t n, double sigma) {
  pk.kappa = (double)pk.shift * (double)native::kBlk / (double)n;
  pk.cw = (2.0 * M_PI / (double)native::kBlk) * sigma * std::sqrt(M_LOG2E / 2.0);
  pk.amp = 1.0 / (double)native::kBlk;
}

// exp(+-2 pi i m / N) from the exact integer phase, evaluated in long double
double2 unit_root(int64_t m, int64_t N, bool negative) {
  const long double two_pi = 6.283185307179586476925286766559005768L;
  const long double ang = (negative ? -two_pi : two_pi) * (long double)(((m % N) + N) % N) / (long double)N;
  return make_double2((double)cosl(ang), (double)sinl(ang));
}

// ---- the band lists of a table -----------------------------------------------------------------------------------------
// Bands marked for the zoom engine (mode 2 + class) leave `bands`, ordered by class.
int upload_zoom_list(qi_plan* p, qi_plan::NativeTable& t, int64_t Lf, std::vector<native::BandDesc>& bands, bool stx) {
  std::vector<native::BandDesc> rest;
  std::vector<std::vector<native::BandDesc>> by_level(native::kZoomClasses);
  for (const auto& d : bands) {
    if (d.mode >= 2) by_level[d.mode - 2].push_back(d);
    else rest.push_back(d);
  }
  // a class with only a few bands is not worth rows of its own in the launch: they join the next class that can carry
  // them -- the 4-tap class the 6-tap one, the 6-tap class the 10-tap class of the same grid, a grid level the next
  // occupied level up (at most two up: each level doubles their coarse grid and adds window samples)
  auto join = [&](int from, int to) {
    by_level[to].insert(by_level[to].begin(), by_level[from].begin(), by_level[from].end());
    by_level[from].clear();
  };
  if (!by_level[6].empty() && by_level[6].size() < 6) join(6, 5);
  if (!by_level[5].empty() && by_level[5].size() < 6) join(5, 0);
  for (int g = 0; g + 1 < native::kZoomLevels; ++g) {
    if (by_level[g].empty() || by_level[g].size() >= 6) continue;
    for (int h = g + 1; h <= g + 2 && h < native::kZoomLevels; ++h)
      if (!by_level[h].empty()) {
        join(g, h);
        break;
      }
  }
  std::vector<native::BandDesc> zoom;
  t.h_zoom.clear();
  t.zoom_planes = 0;
  t.zoom_max_level = 0;
  t.x_lo = 0;
  t.x_hi = -1;
  for (const auto& lvl : by_level)
    for (const auto& d : lvl) {  // bins zoom_gather16 reads: k (+ shift), k in [k_lo, k_lo + k_len)
      const int64_t lo = d.k_lo + (stx ? d.shift : 0), hi = lo + d.k_len - 1;
      if (t.x_lo > t.x_hi) {
        t.x_lo = lo;
        t.x_hi = hi;
      }
      t.x_lo = lo < t.x_lo ? lo : t.x_lo;
      t.x_hi = hi > t.x_hi ? hi : t.x_hi;
    }
  for (int g = 0; g < native::kZoomClasses; ++g) t.zoom_count[g] = (int32_t)by_level[g].size();
  for (int gi = 0; gi < native::kZoomClasses; ++gi) {
    // list order: the short-interpolator classes first, next to the 10-tap class of their grid, so that a call with
    // few records can run all three as one class (kZoomListOrder)
    const int g = kZoomListOrder[gi];
    const int grid = native::zoom_grid(g);
    for (auto d : by_level[g]) {
      d.edge_slot = grid;                 // level of the band's coarse grid
      d.edge = (int32_t)t.zoom_planes;    // first plane of its coarse array
      t.zoom_planes += ((Lf / native::kZoomD) << grid) / native::kBlk;
      if (grid > t.zoom_max_level) t.zoom_max_level = grid;
      zoom.push_back(d);
      t.h_zoom.push_back({d.out_band, g});
    }
  }
  bands.swap(rest);
  if (zoom.empty()) return QI_OK;
  QI_TRY(upload_table(&t.d_zoom, zoom));
  t.nzoom = (int32_t)zoom.size();
  std::vector<int32_t> owner((size_t)t.zoom_planes);
  for (size_t j = 0; j < zoom.size(); ++j) {
    const int64_t planes = ((Lf / native::kZoomD) << zoom[j].edge_slot) / native::kBlk;
    for (int64_t q = 0; q < planes; ++q) owner[(size_t)(zoom[j].edge + q)] = (int32_t)j;
  }
  QI_TRY(upload_table(&t.d_zoom_plane_band, owner));
  for (int g = 0; g < native::kZoomClasses; ++g) {
    // (class 0 also serves the bands of classes 5 and 6 in calls with few records)
    const bool needed = t.zoom_count[g] > 0 || (g == 0 && t.zoom_count[5] + t.zoom_count[6] > 0);
    if (p->d_zoom_w[g] || !needed) continue;
    std::vector<float> w((size_t)64 * native::zoom_taps(g));
    native::zoom_weights(g, 0, w.data());
    QI_TRY(upload_table(&p->d_zoom_w[g], w));
  }
  return QI_OK;
}

// The kZ64FineLevels (two) coarsest grids go through the fine kernel with wave-uniform windows (k_z64_fine), by CLASS =
// (grid, interpolator length): on the coarsest grid, where every narrower band lands, a band oversampled >= 8 / 16 / 32 /
// 64 times takes 12 / 10 / 8 / 6 taps instead of 16 (classes 2..5; the same error bound, see z64f_ntap).  A class of
// fewer than four bands joins the next longer interpolator (class 2 the 16-tap class 0).  Orders the bands of the
// coarsest grid (lvl[0]) by class and uploads the classes' lane weights.
int order_z64_fine_classes(qi_plan* p, qi_plan::NativeTable& t, int64_t Lf, std::vector<std::vector<native::BandDesc>>& lvl) {
  const int64_t M0 = Lf / 64;
  std::vector<std::vector<native::BandDesc>> cls(native::kZ64FineClasses);
  for (const auto& d : lvl[0]) {
    int c = 0;
    for (int q = native::kZ64FineClasses - 1; q >= native::kZ64FineLevels && c == 0; --q)
      if ((int64_t)native::z64f_oversampling(q) * d.k_len <= M0) c = q;
    cls[c].push_back(d);
  }
  for (int q = native::kZ64FineClasses - 1; q >= native::kZ64FineLevels; --q) {
    if (cls[q].empty() || cls[q].size() >= 4) continue;
    const int to = q == native::kZ64FineLevels ? 0 : q - 1;
    cls[to].insert(cls[to].end(), cls[q].begin(), cls[q].end());
    cls[q].clear();
  }
  lvl[0].clear();
  int32_t pos = 0;
  std::vector<int> order0{0};  // list order of the coarsest grid: the 16-tap class, then the shorter interpolators
  for (int c = native::kZ64FineLevels; c < native::kZ64FineClasses; ++c) order0.push_back(c);
  for (int c : order0) {
    t.zf_first[c] = pos;
    t.zf_count[c] = (int32_t)cls[c].size();
    pos += t.zf_count[c];
    lvl[0].insert(lvl[0].end(), cls[c].begin(), cls[c].end());
  }
  for (int g = 1; g < native::kZ64FineLevels && g < native::kZ64Levels; ++g) {
    t.zf_first[g] = pos;
    t.zf_count[g] = (int32_t)lvl[g].size();
    pos += t.zf_count[g];
  }
  for (int c = 0; c < native::kZ64FineClasses; ++c) {
    if (t.zf_count[c] == 0 || p->d_z64f_w[c]) continue;
    std::vector<double> w((size_t)native::z64f_win(c) * 64);
    native::z64_fine_weights(c, w.data());
    QI_TRY(upload_table(&p->d_z64f_w[c], w));
  }
  return QI_OK;
}

// Carrier factors of the fine kernel (Gabor kinds), exact integer phases: per band of `z` exp(2 pi i k_c (lane - e) / Lf) for
// the 64 lanes and the step exp(2 pi i k_c 64 / Lf); per table the waves' factors exp(2 pi i j kZ64FineWave / Lf).  e = 1 for
// the zero-padded kind (the carrier of full-length sample tau - 1).
int upload_z64_carriers(qi_plan::NativeTable& t, int kind, int64_t Lf, const std::vector<native::BandDesc>& z) {
  const int e = kind == 0 ? 1 : 0;
  std::vector<double2> lane(z.size() * 65);
  for (size_t j = 0; j < z.size(); ++j) {
    const int64_t kc = (int64_t)z[j].k_lo + z[j].k_len / 2;
    for (int l = 0; l < 64; ++l) lane[j * 65 + l] = unit_root(kc * (l - e), Lf, false);
    lane[j * 65 + 64] = unit_root(kc * 64, Lf, false);
  }
  const int64_t nw = Lf / native::kZ64FineWave;
  std::vector<double2> wave((size_t)nw);
  for (int64_t j = 0; j < nw; ++j) wave[(size_t)j] = unit_root(j * native::kZ64FineWave, Lf, false);
  QI_TRY(upload_table(&t.d_z64_lane_ph, lane));
  return upload_table(&t.d_z64_wave_ph, wave);
}

// float64: every band with a compact row that the float64 zoom takes (z64_level) leaves `bands`, ordered by grid level.
int upload_z64_list(qi_plan* p, qi_plan::NativeTable& t, int kind, int64_t Lf, std::vector<native::BandDesc>& bands) {
  std::vector<native::BandDesc> rest;
  std::vector<std::vector<native::BandDesc>> lvl(native::kZ64Levels);
  for (const auto& d : bands) {
    const int g = d.mode == 0 ? z64_level(p, kind, Lf, d.k_len) : -1;
    if (g >= 0) lvl[g].push_back(d);
    else rest.push_back(d);
  }
  for (int c = 0; c < native::kZ64FineClasses; ++c) t.zf_first[c] = t.zf_count[c] = 0;
  if (p->native_z64_fine) QI_TRY(order_z64_fine_classes(p, t, Lf, lvl));
  std::vector<native::BandDesc> z;
  for (int g = 0; g < native::kZ64Levels; ++g) {
    t.z64_first[g] = (int32_t)z.size();
    t.z64_count[g] = (int32_t)lvl[g].size();
    z.insert(z.end(), lvl[g].begin(), lvl[g].end());
    if (!lvl[g].empty() && !p->d_z64_w[g]) {
      const int log2d = 6 - g;
      std::vector<double> w((size_t)(1 << log2d) * native::kZ64Taps);
      native::z64_weights(log2d, w.data());
      QI_TRY(upload_table(&p->d_z64_w[g], w));
    }
  }
  t.nz64 = (int32_t)z.size();
  t.h_z64.clear();
  for (const auto& d : z) t.h_z64.push_back(d.out_band);
  if (!z.empty()) QI_TRY(upload_table(&t.d_z64, z));
  if (!z.empty() && p->native_z64_fine && kind != 2) QI_TRY(upload_z64_carriers(t, kind, Lf, z));
  if (tune_env("QI_NATIVE_VERBOSE")) {
    fprintf(stderr, "[qi plan] table %d: float64 zoom bands per level %d %d %d %d %d, two-pass bands %zu; fine classes (taps: bands)", kind,
            t.z64_count[0], t.z64_count[1], t.z64_count[2], t.z64_count[3], t.z64_count[4], rest.size());
    for (int c = 0; c < native::kZ64FineClasses; ++c)
      fprintf(stderr, " %d@L%d: %d", native::z64f_ntap(c), native::z64f_level(c), t.zf_count[c]);
    fprintf(stderr, "\n");
  }
  bands.swap(rest);
  return QI_OK;
}

// Order the bands left for the two-pass kernels into launch groups: the wide bands are dealt out `native_group` per group
// (all in one group when 0) so that a group's intermediate is small enough to stay in the last-level cache between pass 1
// and pass 2; the narrow bands are spread evenly over the groups.
int upload_two_pass_groups(qi_plan* p, qi_plan::NativeTable& t, int64_t Lf, const std::vector<native::BandDesc>& bands) {
  t.h_rows.clear();
  t.h_row_mode.clear();
  for (const auto& d : bands) {
    t.h_rows.push_back(d.out_band);
    t.h_row_mode.push_back(d.mode == 1 ? 1 : 0);
  }
  t.Lf = Lf;
  if (bands.empty()) {  // every band is produced by the block / zoom engines: an empty but valid table
    t.ready = true;
    return QI_OK;
  }
  std::vector<int32_t> wide, narrow;
  for (size_t j = 0; j < bands.size(); ++j) (bands[j].mode == 1 ? wide : narrow).push_back((int32_t)j);
  const int32_t per = p->native_group > 0 ? p->native_group : (int32_t)wide.size();
  const int32_t ngroups = wide.empty() ? 1 : (int32_t)ceil_div((int64_t)wide.size(), per);
  std::vector<native::BandDesc> ordered;
  std::vector<int32_t> gen;
  t.groups.clear();
  size_t wi = 0, ni = 0;
  for (int32_t g = 0; g < ngroups; ++g) {
    qi_plan::NativeGroup grp;
    grp.first = (int32_t)ordered.size();
    grp.gen_first = (int32_t)gen.size();
    int32_t slot = 0;
    for (int32_t q = 0; q < per && wi < wide.size(); ++q, ++wi) {
      native::BandDesc d = bands[wide[wi]];
      d.gen_slot = slot++;
      gen.push_back((int32_t)ordered.size() - grp.first);
      ordered.push_back(d);
    }
    const size_t share = (narrow.size() * (size_t)(g + 1)) / (size_t)ngroups;
    for (; ni < share; ++ni) ordered.push_back(bands[narrow[ni]]);
    grp.count = (int32_t)ordered.size() - grp.first;
    grp.ngen = (int32_t)gen.size() - grp.gen_first;
    if (grp.count > 0) t.groups.push_back(grp);
  }
  QI_TRY(upload_table(&t.d_bands, ordered));
  if (!gen.empty()) QI_TRY(upload_table(&t.d_gen_list, gen));
  t.nbands = (int32_t)bands.size();
  t.ngen = (int32_t)wide.size();
  t.imd_slots = wide.empty() ? 0 : (per < (int32_t)wide.size() ? per : (int32_t)wide.size());
  t.ready = true;
  return QI_OK;
}

// The band lists of table `kind` from its descriptors, engine by engine: the float32 zoom list, the float64 zoom list, the
// launch groups of the two-pass kernels.  `bands[j].out_band` must be set by the caller.
int upload_native_table(qi_plan* p, int kind, int64_t Lf, std::vector<native::BandDesc> bands) {
  auto& t = p->nat[kind];
  if (tune_env("QI_NATIVE_VERBOSE"))
    for (const auto& d : bands)
      fprintf(stderr, "[qi plan] table %d (Lf = %lld) band %d: %s, support [%d, +%d)\n", kind, (long long)Lf, d.out_band,
              d.mode == 0 ? "one-pass loader" : (d.mode == 1 ? "two-pass" : "zoom"), d.k_lo, d.k_len);
  QI_TRY(upload_zoom_list(p, t, Lf, bands, kind == 2));
  if (z64_table(p, kind)) QI_TRY(upload_z64_list(p, t, kind, Lf, bands));
  return upload_two_pass_groups(p, t, Lf, bands);
}

// Support analysis of `count` atom spectra starting at band j0 (rows built in `circular` or linear form).
int analyse_support(qi_plan* p, int circular, int64_t L, int32_t B, int32_t j0, int32_t count, const double* d_par,
                    std::vector<double>* sup, hipStream_t st, double taper_e = 0.0) {
#ifdef QI_HOST_SANITIZE
  // Host sanitizer build (tests/sanitize): no kernel runs there, so the supports are the Gaussian atoms' own -- centre
  // omega L / 2 pi, half-width where exp(-d^2 / 4 p_re) falls below the threshold -- with the whole row for an atom the
  // record cuts off, and a taper's widening (~ 6.6 L / e bins at 2^-30, 13.2 at 2^-50, as the GPU analysis measures it).
  // "Device" memory is host memory in that build: d_par is read directly.
  (void)st;
  (void)circular;
  const double bits = support_bits(p);
  sup->assign((size_t)count * 3, 0.0);
  for (int32_t q = 0; q < count; ++q) {
    const double p_re = d_par[j0 + q], om = d_par[2 * (int64_t)B + j0 + q];
    const double kc = om * (double)L / (2.0 * M_PI), hw = std::sqrt(4.0 * p_re * bits * M_LN2) * (double)L / (2.0 * M_PI);
    const bool cut = p_re * 0.25 * (double)p->n * (double)p->n <= bits * M_LN2;
    double lo = 0.0, hi = (double)(L - 1);
    if (!cut || taper_e > 0.0) {
      const double extra = cut ? (p->d.dtype == QI_F64 ? 13.2 : 6.6) * (double)L / taper_e : 0.0;
      lo = std::floor(kc - hw - extra);
      hi = std::ceil(kc + hw + extra);
      if (hi - lo + 1.0 >= (double)L) {
        lo = 0.0;
        hi = (double)(L - 1);
      }
    }
    (*sup)[3 * (size_t)q] = 1.0;
    (*sup)[3 * (size_t)q + 1] = lo;
    (*sup)[3 * (size_t)q + 2] = hi;
  }
  return QI_OK;
#endif
  const size_t row64 = (size_t)L * sizeof(double2);
  int64_t chunk = (int64_t)((p->ws_bytes - 4096) / row64);
  if (chunk < 1) {
    set_error("workspace too small to build one bank row (%zu bytes needed)", row64);
    return QI_ERR_NOMEM;
  }
  double2* rows = reinterpret_cast<double2*>(p->ws);
  DeviceTemp<double> d_sup;
  QI_HIP(hipMalloc((void**)&d_sup.ptr, (size_t)count * 3 * sizeof(double)));
  const double thr2 = std::ldexp(1.0, -2 * (int)support_bits(p));  // the threshold on |H|^2
  for (int32_t q = 0; q < count; q += (int32_t)chunk) {
    const int nbk = (count - q < chunk) ? count - q : (int)chunk;
    QI_TRY(launch_bank_rows(rows, p->n, L, circular, d_par, d_par + B, d_par + 2 * B, d_par + 3 * B, j0 + q, nbk, st, taper_e));
    QI_TRY(fft_c2c<double>(p->fft, rows, L, nbk, HIPFFT_FORWARD, st));
    QI_TRY(native::launch_band_support(rows, L, nbk, thr2, d_sup.ptr + (size_t)q * 3, st));
  }
  sup->assign((size_t)count * 3, 0.0);
  if (hipStreamSynchronize(st) != hipSuccess ||
      hipMemcpy(sup->data(), d_sup.ptr, sup->size() * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) {
    set_error("support analysis failed: %s", hipGetErrorString(hipGetLastError()));
    return QI_ERR_HIP;
  }
  return QI_OK;
}

// Fill the compact / full-row banks of table `table` for the bands listed in `ids` (global band ids; descriptors in
// `bands`, same order) from freshly built float64 spectra.
template <typename T>
int fill_native_bank(qi_plan* p, int table, int circular, int64_t L, int32_t B, const std::vector<int32_t>& ids,
                     const std::vector<native::BandDesc>& bands, const double* d_par, hipStream_t st) {
  auto& t = p->nat[table];
  const size_t row64 = (size_t)L * sizeof(double2);
  int64_t chunk = (int64_t)((p->ws_bytes - 4096) / row64);
  double2* rows = reinterpret_cast<double2*>(p->ws);
  size_t q = 0;
  while (q < ids.size()) {
    // a run of consecutive band ids, at most `chunk` long (split bands -- tapered rows -- apart from the others)
    size_t r = q + 1;
    const bool tapered = bands[q].add_row != 0;
    while (r < ids.size() && ids[r] == ids[r - 1] + 1 && (int64_t)(r - q) < chunk && (bands[r].add_row != 0) == tapered) ++r;
    const int nbk = (int)(r - q);
    QI_TRY(launch_bank_rows(rows, p->n, L, circular, d_par, d_par + B, d_par + 2 * B, d_par + 3 * B, ids[q], nbk, st,
                            tapered ? (double)p->native_split_e : 0.0));
    QI_TRY(fft_c2c<double>(p->fft, rows, L, nbk, HIPFFT_FORWARD, st));
    for (int jj = 0; jj < nbk; ++jj) {
      const native::BandDesc& d = bands[q + jj];
      if (d.mode != 1) {
        // bands of the zoom engines in the linear (styx) table: panel sample t is full-length sample t + n/2 - 1; the odd
        // sample is a phase ramp on the band's baseband bins, exp(-2 pi i (k - k_c) / L), folded into the compact bank here
        const bool zoomed = d.mode >= 2 || z64_level(p, table, L, d.k_len) >= 0;
        const double ramp = zoomed && !circular ? -1.0 / (double)L : 0.0;
        QI_TRY(native::launch_copy_window<T>(rows + (int64_t)jj * L, static_cast<cplx<T>*>(t.Hc) + d.src_off, d.k_lo,
                                              d.k_len, circular, 1.0 / (double)L, L, st, ramp, d.k_len / 2));
      }
      else
        QI_TRY(native::launch_copy_window<T>(rows + (int64_t)jj * L,
                                              static_cast<cplx<T>*>(t.Hfull) + (int64_t)d.bank_row * L, 0, L, circular,
                                              1.0 / (double)L, L, st));
    }
    q = r;
  }
  return QI_OK;
}

// ---- block engine tables ------------------------------------------------------------------------------------------
// reach groups: taps within 256, 512, 1024 samples (4096-sample blocks), and the long blocks (8192 samples) for the
// narrow Gaussian bands of the 1024-sample group whose spectrum lies in the lower half of the 8192-bin grid
constexpr int kBlockGroups = 4;
constexpr int kBlockGroupWq[kBlockGroups] = {1, 2, 4, native::kBlkLongWq};
constexpr int kBlockMaxWq = 4;  // reach groups above this one (1, 2, 4) prefer the zoom engine when their spectrum fits it
constexpr int kBlockBandsPerWg = 6, kBlockBandsPerWgBatch = 12;  // bands one block workgroup walks at most (each pays one forward transform): item cut 0 / 1

// first bin of the 256-bin window of a long band: centred on the band, kept inside the lower half of the 8192-bin grid
// (the half a long block holds)
int64_t long_window(const BlockPick& pk) {
  return std::min<int64_t>(std::max<int64_t>((int64_t)std::llround(2.0 * pk.kappa) - 128, 0), native::kBlk - 256);
}
// does item cut `cut` run this band in long blocks?  (float32 tables only)
bool long_ok(const qi_plan* p, const BlockPick& pk, int cut) {
  if (cut == 0) return false;  // few records: the long blocks' own launch would cost more than the blocks save
  if (pk.wq != 4 || !pk.analytic) return false;
  if (p->n < 4 * native::kBlkLong) return false;
  const double half8 = std::ceil(std::sqrt(drop_bits(false)) / (0.5 * pk.cw));  // weights >= 2^-30 of the peak on the 8192-bin grid
  const int64_t klo8 = long_window(pk);
  return 2.0 * pk.kappa - half8 - 1.0 >= (double)klo8 && 2.0 * pk.kappa + half8 + 1.0 <= (double)(klo8 + 255);
}

// The descriptor of block band `row` (its pick), on long blocks or not.
template <typename T>
int block_band_desc(const qi_plan* p, const BlockPick& pk, int32_t row, bool is_long, native::BlockBandT<T>* out) {
  // (float64 tables: Gaussian weights in double from every bin -- the shortcuts below drop weights under 2^-30 of the peak)
  constexpr bool F64 = sizeof(T) == 8;
  native::BlockBandT<T>& b = *out;
  memset(&b, 0, sizeof(b));
  b.out_band = pk.band;
  b.bank_row = row;
  b.shift = (int32_t)pk.shift;
  b.analytic = pk.analytic;
  const double grid = is_long ? 2.0 : 1.0;  // the band on the 8192-bin grid of a long block: twice the bins
  const double kappa = grid * pk.kappa, cw = pk.cw / grid;
  b.kappa_int = (int32_t)std::floor(kappa);
  b.kappa_frac = (T)(kappa - std::floor(kappa));
  b.cw = (T)cw;
  b.amp = (T)(pk.amp / grid);
  // weights >= 2^-30 of the peak: |cw dk| <= sqrt(30) (float64: 2^-52)
  const double half = std::ceil(std::sqrt(drop_bits(F64)) / cw);
  if (F64 && !b.analytic) {
    set_error("block engine: float64 tables take analytic (Gaussian) bands only");
    return QI_ERR_STATE;
  }
  // (float64 since round 5: `half` is then the 2^-52 half-width, the weight comes from the table -- bands of the 512- and
  // 1024-sample reach groups; analytic = 2, an aliased spectrum, is not narrow)
  if ((!F64 || (b.analytic == 1 && p->native_blk64_wtab && p->native_blk64_narrow)) && b.analytic && 2.0 * half + 2.0 <= 256.0) {
    b.narrow = 1;
    b.klo = is_long ? (int32_t)long_window(pk)
                    : (int32_t)((((int64_t)std::llround(kappa) - 128) % native::kBlk + native::kBlk) % native::kBlk);
    const int ba = b.klo >> 8;
    b.rot_a[0] = (T)std::cos(2.0 * M_PI * ba / 16.0);
    b.rot_a[1] = (T)std::sin(2.0 * M_PI * ba / 16.0);
    b.rot_b[0] = (T)std::cos(2.0 * M_PI * ((ba + 1) & 15) / 16.0);
    b.rot_b[1] = (T)std::sin(2.0 * M_PI * ((ba + 1) & 15) / 16.0);
    b.rot8_a[0] = (T)std::cos(M_PI * ba / 16.0);  // exp(2 pi i 256 b / 8192)
    b.rot8_a[1] = (T)std::sin(M_PI * ba / 16.0);
    b.rot8_b[0] = (T)std::cos(M_PI * (ba + 1) / 16.0);
    b.rot8_b[1] = (T)std::sin(M_PI * (ba + 1) / 16.0);
  } else if (!F64 && b.analytic && kappa - half - 1.0 >= 0.0 && kappa + half + 1.0 < (double)(native::kBlk / 2)) {
    b.narrow = 2;  // every weight above 2^-30 of the peak lies in the lower half of the block spectrum
  }
  if (b.analytic && b.amp > (T)0 && kappa - half - 1.0 >= 0.0 && kappa + half + 1.0 < (double)native::kBlk) {
    b.nowrap = 1;
    b.la = (T)std::log2(pk.amp / grid);
  }
  for (int k = 0; k < 4; ++k) {
    // r^(2^k), r = exp(-2 pi i idx 256 / n), from the exact integer phase
    const int64_t m = (int64_t)(((__int128)pk.shift * 256 * (1 << k)) % p->n);
    const double ang = -2.0 * M_PI * (double)m / (double)p->n;
    b.rot[2 * k] = (T)std::cos(ang);
    b.rot[2 * k + 1] = (T)std::sin(ang);
  }
  const int64_t m1 = pk.shift % p->n;  // one sample: the odd sample of a long block's pair
  b.rot1[0] = (T)std::cos(-2.0 * M_PI * (double)m1 / (double)p->n);
  b.rot1[1] = (T)std::sin(-2.0 * M_PI * (double)m1 / (double)p->n);
  return QI_OK;
}

// The work items of item cut `cut` of table `kind`: its bands (`list`, group g in [first[g], first[g] + count[g])) dealt to
// workgroups, most expensive first, then the edge items of the split bands.
template <typename T>
std::vector<native::BlockItem> block_cut_items(const qi_plan* p, int kind, int cut, qi_plan::BlockTable::ItemList& il,
                                               const std::vector<native::BlockBandT<T>>& list, const int32_t* first,
                                               const int32_t* count, int64_t split_blocks) {
  std::vector<native::BlockItem> items;
  for (int g = 0; g < kBlockGroups; ++g) {
    if (count[g] == 0) continue;
    // the group's bands are dealt to `nchunk` workgroups per block (each pays one forward transform of the block)
    const int per_wg = cut == 0 ? kBlockBandsPerWg : kBlockBandsPerWgBatch;
    const int32_t nchunk = (int32_t)ceil_div(count[g], per_wg);
    const int64_t nblocks = ceil_div(p->n, native::block_valid(kBlockGroupWq[g]));
    if (tune_env("QI_NATIVE_VERBOSE")) {
      auto count_if = [&](auto pred) { return (int)std::count_if(list.begin() + first[g], list.begin() + first[g] + count[g], pred); };
      fprintf(stderr, "[qi plan] block table %d cut %d, reach <= %d%s: %d bands (%d analytic, %d narrow, %d half) in %d workgroups x %lld blocks\n", kind, cut,
              g == 3 ? 1024 : 256 * (kBlockGroupWq[g] & 15), g == 3 ? " (8192-sample blocks)" : "", count[g],
              count_if([](const native::BlockBandT<T>& b) { return b.analytic != 0; }),
              count_if([](const native::BlockBandT<T>& b) { return b.narrow == 1; }),
              count_if([](const native::BlockBandT<T>& b) { return b.narrow == 2; }), nchunk, (long long)nblocks);
    }
    for (int32_t c = 0; c < nchunk; ++c) {
      const int32_t lo = first[g] + (int32_t)((int64_t)count[g] * c / nchunk);
      const int32_t hi = first[g] + (int32_t)((int64_t)count[g] * (c + 1) / nchunk);
      for (int64_t b = 0; b < nblocks; ++b) items.push_back({kBlockGroupWq[g], (int32_t)b, lo, hi - lo, il.nplanes, 0});
      il.nplanes += 1;
    }
  }
  std::stable_sort(items.begin(), items.end(), [](const native::BlockItem& x, const native::BlockItem& y) {
    const bool lx = x.wq == native::kBlkLongWq, ly = y.wq == native::kBlkLongWq;
    return lx != ly ? lx : x.band_count > y.band_count;
  });
  for (size_t i = 0; i < items.size(); ++i) items[i].stat_slot = (int32_t)i;
  il.nitems = (int32_t)items.size();
  il.nlong = (int32_t)std::count_if(items.begin(), items.end(), [](const native::BlockItem& x) { return x.wq == native::kBlkLongWq; });
  if (kind == 0 && p->nsplit > 0) {
    // the edge items of the split bands ride at the end of the launch (light items: they fill its tail); each split
    // band has a per-time plane and one partial slot per block like the other bands of the launch
    // -- in the table for many records one item per block covers all of them (one plane, one launch of its own)
    const int wq = (int)(p->native_split_e / 512);
    il.edge_merged = cut == 1 || sizeof(T) == 8;  // (float64: always, k_block64_edge)
    if (il.edge_merged) {
      for (int64_t b = 0; b < split_blocks; ++b)
        items.push_back({-wq, (int32_t)b, 0, p->nsplit, il.nplanes, (int32_t)items.size()});
      il.nplanes += 1;
    } else {
      for (int32_t sb = 0; sb < p->nsplit; ++sb) {
        for (int64_t b = 0; b < split_blocks; ++b)
          items.push_back({-wq, (int32_t)b, sb, 0, il.nplanes, (int32_t)items.size()});
        il.nplanes += 1;
      }
    }
    il.nedge_items = (int32_t)items.size() - il.nitems;
  }
  return items;
}

// float64: the bands' real Gaussian filter weights, weight(k) = amp exp2(-(cw dk)^2) with dk = k - kappa wrapped to
// +-kBlk / 2 (Gabor banks: the aliases of the half-sample grid alternate in sign) -- block_bands' formula, in double
std::vector<double> block_gauss_weights(const std::vector<native::BlockBandT<double>>& list, int demod) {
  std::vector<double> gw(list.size() * (size_t)native::kBlk);
  for (size_t q = 0; q < list.size(); ++q) {
    const auto& b = list[q];
    for (int k = 0; k < native::kBlk; ++k) {
      if (b.analytic == 2) {  // an atom shorter than 2.75 samples: every alias that matters, alternating in sign
        double acc = 0.0;
        for (int m = -6; m <= 6; ++m) {
          const double e = (double)b.cw * ((double)(k - b.kappa_int) - (double)b.kappa_frac + (double)native::kBlk * m);
          acc += ((m & 1) && !demod ? -1.0 : 1.0) * std::exp2(-e * e);
        }
        gw[q * native::kBlk + k] = (double)b.amp * acc;
        continue;
      }
      double dk = (double)(k - b.kappa_int) - (double)b.kappa_frac, amp = (double)b.amp;
      if (dk > (double)(native::kBlk / 2)) {
        dk -= (double)native::kBlk;
        if (!demod) amp = -amp;
      }
      if (demod && dk < -(double)(native::kBlk / 2)) dk += (double)native::kBlk;
      const double e = (double)b.cw * dk;
      gw[q * native::kBlk + k] = amp * std::exp2(-e * e);
    }
  }
  return gw;
}

// demodulation tables of the float64 Stockwell bands (exact integer phases): per band exp(-2 pi i idx 256 i / n), i < 16; per
// plan exp(-2 pi i 1024 j / n) and exp(-2 pi i j / n)
int upload_demod_tables(qi_plan* p, qi_plan::BlockTable::ItemList& il, const std::vector<native::BlockBandT<double>>& list) {
  std::vector<double2> pw(list.size() * 16);
  for (size_t q = 0; q < list.size(); ++q)
    for (int i = 0; i < 16; ++i) pw[q * 16 + i] = unit_root((int64_t)(((__int128)list[q].shift * 256 * i) % p->n), p->n, true);
  QI_TRY(upload_table(&il.d_demod_pow, pw));
  if (p->d_demod_t1 || p->n < 1024) return QI_OK;
  std::vector<double2> t1((size_t)(p->n / 1024)), t2(1024);
  for (int64_t j = 0; j < p->n / 1024; ++j) t1[(size_t)j] = unit_root(1024 * j, p->n, true);
  for (int64_t j = 0; j < 1024; ++j) t2[(size_t)j] = unit_root(j, p->n, true);
  QI_TRY(upload_table(&p->d_demod_t1, t1));
  return upload_table(&p->d_demod_t2, t2);
}

// `taps` holds one 4096-sample circular-convolution kernel per pick (float64, on the device, same order):
// transform them, convert to the engine's precision and upload the per-group band lists.
template <typename T>
int finish_block_table(qi_plan* p, int kind, int demod, const std::vector<BlockPick>& picks, double2* taps,
                       hipStream_t st) {
  constexpr bool F64 = sizeof(T) == 8;
  auto& bt = p->blk[kind];
  bt.release();
  for (bool& valid : p->dual_valid) valid = false;
  if (picks.empty()) return QI_OK;
  const int32_t rows = (int32_t)picks.size();
  QI_TRY(fft_c2c<double>(p->fft, taps, native::kBlk, rows, HIPFFT_FORWARD, st));
  if (!demod) QI_TRY(native::launch_block_rotate_rows(taps, rows, st));
  QI_HIP(hipMalloc(&bt.bank, (size_t)rows * native::kBlk * sizeof(cplx<T>)));
  QI_TRY(launch_bank_convert<T>(taps, static_cast<cplx<T>*>(bt.bank), (int64_t)rows * native::kBlk, 0,
                                1.0 / (double)native::kBlk, st));
  bt.rows = rows;
  bt.demod = demod;
  const bool edges = kind == 0 && p->nsplit > 0;
  const int64_t split_blocks = edges ? ceil_div(p->n, native::block_valid((int)(p->native_split_e / 512))) : 0;
  bt.max_blocks = split_blocks;
  for (int v = 0; v < 2; ++v) {
    auto& il = bt.var[v];
    for (int32_t sb = 0; sb < p->nsplit && edges; ++sb) il.h_bands.push_back({p->h_split_bands[sb], (int32_t)split_blocks});
    std::vector<native::BlockBandT<T>> list;
    int32_t group_first[kBlockGroups], group_count[kBlockGroups];
    for (int g = 0; g < kBlockGroups; ++g) {
      group_first[g] = (int32_t)list.size();
      for (int32_t r = 0; r < rows; ++r) {
        const bool is_long = !F64 && long_ok(p, picks[r], v);
        if ((is_long ? native::kBlkLongWq : picks[r].wq) != kBlockGroupWq[g]) continue;  // another group takes this band
        list.emplace_back();
        QI_TRY(block_band_desc<T>(p, picks[r], r, is_long, &list.back()));
      }
      group_count[g] = (int32_t)list.size() - group_first[g];
      il.h_groups.push_back({group_first[g], group_count[g]});
      if (group_count[g] == 0) continue;
      const int64_t nblocks = ceil_div(p->n, native::block_valid(kBlockGroupWq[g]));
      if (nblocks > bt.max_blocks) bt.max_blocks = nblocks;
      for (int32_t q = group_first[g]; q < (int32_t)list.size(); ++q) {
        il.h_bands.push_back({list[q].out_band, (int32_t)nblocks});
        il.h_route.push_back({list[q].out_band, kBlockGroupWq[g], list[q].analytic, list[q].narrow, list[q].nowrap});
      }
    }
    il.h_items = block_cut_items<T>(p, kind, v, il, list, group_first, group_count, split_blocks);
    if constexpr (F64) {
      if (p->native_blk64_wtab && !list.empty()) QI_TRY(upload_table(&il.d_gauss_w, block_gauss_weights(list, demod)));
      if (demod && !list.empty()) QI_TRY(upload_demod_tables(p, il, list));
    }
    QI_TRY(upload_table(&il.d_bands, list));
    QI_TRY(upload_table(&il.d_items, il.h_items));
  }
  QI_HIP(hipStreamSynchronize(st));
  bt.ready = true;
  return QI_OK;
}

// Table-first dealing of the joint block launch of qi_cwt_stx, item cut 0.  A reach group with c0 styx and c2 Stockwell
// bands keeps the workgroups per block of the chunk-by-chunk pairing, W = max of the two tables' chunk counts, but its
// bands are dealt as ONE sequence, styx bands first: W runs whose lengths differ by at most one, a run = one workgroup
// per block with a contiguous styx part and a contiguous Stockwell part (either may be empty).  A table owns one
// per-time plane per run that holds any of its bands: 7 + 7 bands are runs of 7 styx and 7 Stockwell bands, one plane per
// table, where chunks of 4 + 4 and 3 + 3 need two.  The rule depends on the tables alone.  Each table's share is a complete
// item list of its own (BlockTable::joint: planes, statistics slots, long-block items first, the styx table's edge
// items at the end with planes of their own).
int build_joint_items(qi_plan* p, std::vector<native::DualItem>* dual) {
  qi_plan::BlockTable* bt[2] = {&p->blk[0], &p->blk[2]};
  std::vector<native::BlockItem> items[2];
  for (auto* t : bt) {
    if (!t->ready || t->var[0].h_groups.size() != (size_t)kBlockGroups) {
      set_error("block engine: the joint dealing needs both block tables");
      return QI_ERR_STATE;
    }
    free_device(t->joint.d_items);
    t->joint = t->var[0];  // (the bands and their tables stay var[0]'s)
    t->joint.d_items = nullptr;
    t->joint.h_items.clear();
    t->joint.nitems = t->joint.nplanes = t->joint.nlong = t->joint.nedge_items = 0;
  }
  dual->clear();
  for (int g = 0; g < kBlockGroups; ++g) {
    const int32_t f[2] = {bt[0]->var[0].h_groups[g].first, bt[1]->var[0].h_groups[g].first};
    const int32_t c[2] = {bt[0]->var[0].h_groups[g].second, bt[1]->var[0].h_groups[g].second};
    const int32_t total = c[0] + c[1];
    if (total == 0) continue;
    const int32_t W = (int32_t)std::max(ceil_div(c[0], kBlockBandsPerWg), ceil_div(c[1], kBlockBandsPerWg));
    const int64_t nblocks = ceil_div(p->n, native::block_valid(kBlockGroupWq[g]));
    const int32_t planes_before[2] = {bt[0]->joint.nplanes, bt[1]->joint.nplanes};
    for (int32_t r = 0; r < W; ++r) {
      const int32_t lo = (int32_t)((int64_t)total * r / W), hi = (int32_t)((int64_t)total * (r + 1) / W);
      // the run's part of each table: [lo, hi) cut at c0, the Stockwell part counted from its own first band
      const int32_t first[2] = {f[0] + std::min(lo, c[0]), f[1] + std::max(lo, c[0]) - c[0]};
      const int32_t count[2] = {std::min(hi, c[0]) - std::min(lo, c[0]), std::max(hi, c[0]) - std::max(lo, c[0])};
      int32_t plane[2] = {0, 0};
      for (int q = 0; q < 2; ++q)
        if (count[q] > 0) plane[q] = bt[q]->joint.nplanes++;
      for (int64_t b = 0; b < nblocks; ++b) {
        native::DualItem d{kBlockGroupWq[g], (int32_t)b, 0, 0, 0, 0, 0, 0, 0, 0};
        int32_t slot[2] = {0, 0};
        for (int q = 0; q < 2; ++q) {
          if (count[q] == 0) continue;
          slot[q] = (int32_t)items[q].size();  // (dense and unique: the order of the statistics slots is the generation order)
          items[q].push_back({kBlockGroupWq[g], (int32_t)b, first[q], count[q], plane[q], slot[q]});
        }
        if (count[0] > 0) d.first0 = first[0], d.count0 = count[0], d.plane0 = plane[0], d.slot0 = slot[0];
        if (count[1] > 0) d.first2 = first[1], d.count2 = count[1], d.plane2 = plane[1], d.slot2 = slot[1];
        dual->push_back(d);
      }
    }
    if (tune_env("QI_NATIVE_VERBOSE"))
      fprintf(stderr, "[qi plan] joint dealing, reach group %d: %d styx + %d Stockwell bands in %d workgroups x %lld blocks; planes %d + %d (chunk by chunk: %d + %d)\n",
              kBlockGroupWq[g], c[0], c[1], W, (long long)nblocks, bt[0]->joint.nplanes - planes_before[0],
              bt[1]->joint.nplanes - planes_before[1], (int)ceil_div(c[0], kBlockBandsPerWg), (int)ceil_div(c[1], kBlockBandsPerWg));
  }
  for (int q = 0; q < 2; ++q) {
    auto& il = bt[q]->joint;
    std::stable_sort(items[q].begin(), items[q].end(), [](const native::BlockItem& x, const native::BlockItem& y) {
      const bool lx = x.wq == native::kBlkLongWq, ly = y.wq == native::kBlkLongWq;
      return lx != ly ? lx : x.band_count > y.band_count;
    });
    il.nitems = (int32_t)items[q].size();
    il.nlong = (int32_t)std::count_if(items[q].begin(), items[q].end(), [](const native::BlockItem& x) { return x.wq == native::kBlkLongWq; });
    // the edge items of the split bands (styx table): as in var[0], their planes behind the band items' planes
    const auto& src = bt[q]->var[0];
    for (int32_t i = src.nitems; i < src.nitems + src.nedge_items; ++i) {
      native::BlockItem e = src.h_items[(size_t)i];
      e.plane = il.nplanes + (e.plane - src.h_items[(size_t)src.nitems].plane);
      e.stat_slot = (int32_t)items[q].size();
      items[q].push_back(e);
    }
    il.nedge_items = src.nedge_items;
    if (src.nedge_items > 0) il.nplanes += src.nplanes - src.h_items[(size_t)src.nitems].plane;
    il.h_items = items[q];
    if (!il.h_items.empty()) QI_TRY(upload_table(&il.d_items, il.h_items));
  }
  return QI_OK;
}

// Gabor bands (styx bank): taps straight from the atom parameters.
template <typename T>
int build_block_gabor(qi_plan* p, int kind, int32_t B, const std::vector<BlockPick>& picks, const double* d_par,
                      hipStream_t st) {
  if (picks.empty()) {
    p->blk[kind].release();
    return QI_OK;
  }
  double2* taps = reinterpret_cast<double2*>(p->ws);
  if (p->ws_bytes < picks.size() * native::kBlk * sizeof(double2)) {
    set_error("workspace too small for the block-engine taps");
    return QI_ERR_NOMEM;
  }
  DeviceTemp<int32_t> d_ids;
  QI_HIP(hipMalloc((void**)&d_ids.ptr, picks.size() * sizeof(int32_t)));
  size_t r = 0;
  // picks are ordered by group, so each group is one run of rows
  for (int wq : {1, 2, 4}) {
    std::vector<int32_t> ids;
    for (const auto& pk : picks)
      if (pk.wq == wq) ids.push_back(pk.band);
    if (ids.empty()) continue;
    QI_HIP(hipMemcpy(d_ids.ptr + r, ids.data(), ids.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    QI_TRY(native::launch_block_taps_gabor(taps + r * native::kBlk, 256 * wq, d_par, B, d_ids.ptr + r, (int)ids.size(), st));
    r += ids.size();
  }
  const int rc = finish_block_table<T>(p, kind, 0, picks, taps, st);
  (void)hipStreamSynchronize(st);  // (the tap kernels read d_ids)
  return rc;
}

// Stockwell bands: the time-domain kernel is the inverse transform of the band's Gaussian window, computed as the
// reference defines it (on the n signed FFT bins) and modulated to the band's shift index.
template <typename T>
int build_block_stx(qi_plan* p, const std::vector<BlockPick>& picks, const std::vector<double>& coef, hipStream_t st) {
  if (picks.empty()) {
    p->blk[2].release();
    return QI_OK;
  }
  const size_t need = ((size_t)p->n + picks.size() * native::kBlk) * sizeof(double2);
  if (p->ws_bytes < need) {
    set_error("workspace too small for the block-engine taps (%zu bytes needed)", need);
    return QI_ERR_NOMEM;
  }
  double2* row = reinterpret_cast<double2*>(p->ws);
  double2* taps = row + p->n;
  for (size_t r = 0; r < picks.size(); ++r) {
    QI_TRY(native::launch_stx_window_row(row, p->n, coef[picks[r].band], st));
    QI_TRY(fft_c2c<double>(p->fft, row, p->n, 1, HIPFFT_BACKWARD, st));
    QI_TRY(native::launch_block_taps_stx(taps + r * native::kBlk, 256 * picks[r].wq, row, p->n, picks[r].shift, st));
  }
  return finish_block_table<T>(p, 2, 1, picks, taps, st);
}

// Classify bands by spectrum support, allocate and fill one table.
template <typename T>
int make_native_table(qi_plan* p, int table, int circular, int64_t L, int32_t B, const std::vector<int32_t>& ids,
                      const std::vector<double>& sup /*[ids][3]*/, const std::vector<int32_t>& edge_w,
                      const double* d_par, hipStream_t st, const std::vector<int32_t>& add_row = {}) {
  std::vector<native::BandDesc> bands(ids.size());
  int64_t compact = 0;
  int32_t ngen = 0;
  for (size_t q = 0; q < ids.size(); ++q) {
    native::BandDesc& d = bands[q];
    memset(&d, 0, sizeof(d));
    const int64_t len = support_len(&sup[3 * q]);
    d.out_band = ids[q];
    d.edge = edge_w.empty() ? 0 : edge_w[q];
    d.edge_slot = (int32_t)q;  // the edge list is in the order of `ids`
    d.add_row = add_row.empty() ? 0 : add_row[q];
    d.mode = band_mode(p, table, L, len);
    if (d.mode != 1) {
      d.k_lo = (int32_t)(int64_t)sup[3 * q + 1];
      d.k_len = (int32_t)len;
      d.src_off = compact;
      compact += len;
    } else {
      d.bank_row = ngen++;
    }
  }
  auto& t = p->nat[table];
  t.release();
  if (ids.empty()) {  // every band is produced elsewhere (block engine): an empty but valid table
    t.Lf = L;
    t.ready = table != 3;
    return QI_OK;
  }
  if (compact > 0) QI_HIP(hipMalloc(&t.Hc, (size_t)compact * sizeof(cplx<T>)));
  if (ngen > 0) QI_HIP(hipMalloc(&t.Hfull, (size_t)ngen * L * sizeof(cplx<T>)));
  QI_TRY(fill_native_bank<T>(p, table, circular, L, B, ids, bands, d_par, st));
  return upload_native_table(p, table, L, bands);
}

// ---- native bank -------------------------------------------------------------------------------------------------------
struct GaborRoutes {
  std::vector<BlockPick> picks;           // block engine
  std::vector<int32_t> shorts, short_w;   // short atoms (table 3) and their reach in samples
  std::vector<int32_t> keep;              // the bank's own table (zoom, float64 zoom, two-pass; split bands)
};
bool gabor_can_block(const qi_plan* p, int circular) {
  return !circular && p->native_block && is_pow2(p->n) && p->n >= 4 * native::kBlk;
}

// Every band of a Gabor bank to the block engine, the short-atom table or the bank's own table, from its support
// `sup` [B][3] and its parameters `h_par` [4][B].
GaborRoutes classify_gabor_bands(const qi_plan* p, int bank, int64_t L, int32_t B, const std::vector<double>& sup,
                                 const double* h_par) {
  GaborRoutes out;
  const int64_t n = p->n;
  const int circular = bank == QI_BANK_ATOMS;
  const bool f64 = p->d.dtype == QI_F64;
  const bool can_short = !circular && p->native_short && native_len_ok(n) && is_pow2(n);
  const bool can_block = gabor_can_block(p, circular);
  for (int32_t j = 0; j < B; ++j) {
    const int64_t len = support_len(&sup[3 * j]);
    // taps with |x| <= w are above 2^-30 of the atom's peak: exp(-p_re x^2) >= 2^-30 (float64: 2^-52)
    const double w = std::ceil(std::sqrt(drop_bits(f64) * M_LN2 / h_par[j])) + 1.0;
    const int group = can_block ? block_group_of(w) : 0;
    // (a band of the widest reach groups -- half of each 4096-sample block is overlap there -- goes to the zoom
    // engine instead when its spectrum fits one of its grids)
    // (float64: a band the float64 zoom takes stays there, unless it needs one of the finest grids)
    const int z64 = z64_level(p, bank, L, len);
    const bool zoom_first = (z64 >= 0 && !z64_level_for_block(p, z64)) ||
                            (group > kBlockMaxWq && zoom_class(p, bank, L, len) >= 0);
    bool to_block = group > 0 && !zoom_first, wide = band_mode(p, bank, L, len) == 1;
    BlockPick pk{j, group, 0};
    if (to_block) {
      const double p_re = h_par[j], p_im = h_par[B + j], om = h_par[2 * B + j], am = h_par[3 * B + j];
      const bool pure = p_im == 0.0 && p_re > 0.0 && om > 0.0 && om < M_PI;  // a pure Gabor atom, centre frequency inside (0, pi)
      // at least 2.75 samples wide (no alias of its Gaussian spectrum above 1e-16): the Gaussian itself
      if (pure && p_re <= 1.0 / (2.0 * 2.75 * 2.75)) pk.analytic = 1;
      // float64, an atom SHORTER than 2.75 samples (the top band of an order-1 or order-2 table): its sampled spectrum is the
      // Gaussian plus its aliases, sum over m of (-1)^m G(theta + 2 pi m) after the half-sample factor -- still real weights,
      // which the plan-time weight table holds summed (analytic = 2: table only; float32 reads such a band's bank row)
      else if (pure && f64 && p->native_blk64_wtab) pk.analytic = 2;
      if (pk.analytic) gabor_gaussian(pk, p_re, om, am);
      // (the float64 block kernels evaluate Gaussians only: any other band is a short atom if it can be, whatever its spectrum)
      if (f64 && !pk.analytic) to_block = false, wide = true;
    }
    if (to_block) {
      out.picks.push_back(pk);
    } else if (can_short && wide && w <= 8192.0 && w < (double)n / 8) {
      out.shorts.push_back(j);
      out.short_w.push_back((int32_t)w);
    } else {
      out.keep.push_back(j);
    }
  }
  return out;
}

// Bands left for the two-pass kernels because the reference cuts their atoms off at |x| = n / 2 (a spectrum with
// 1 / k side lobes): with the last `e` samples before the cut tapered away the spectrum is narrow enough for the
// zoom engine; what the taper removed is a pair of e-tap filters at lags +-n / 2 (k_block_edge), added back by the
// zoom kernel.  The split bands' rows of `sup` are replaced by the tapered supports.
int find_split_bands(qi_plan* p, int bank, int64_t L, int32_t B, const double* d_par, const std::vector<int32_t>& keep,
                     std::vector<double>* sup, std::vector<int32_t>* split, hipStream_t st) {
  const int64_t se = p->native_split_e;
  if (!(se == 512 || se == 1024 || se == 2048) || p->n < 8 * se) return QI_OK;
  // float64: "the zoom engine" is the float64 zoom
  const bool f64 = p->d.dtype == QI_F64;
  for (int32_t j : keep) {
    const int64_t len = support_len(&(*sup)[3 * j]);
    // (a band the one-pass loader of the two-pass kernels would take stays there only where those kernels exist)
    const int mode = band_mode(p, bank, L, len);
    if (f64 ? z64_level(p, bank, L, len) >= 0 : (mode >= 2 || (mode == 0 && native_len_ok(L)))) continue;
    std::vector<double> part;
    QI_TRY(analyse_support(p, 0, L, B, j, 1, d_par, &part, st, (double)se));
    const int64_t tlen = support_len(part.data());
    if (tune_env("QI_NATIVE_VERBOSE"))
      fprintf(stderr, "[qi plan] band %d: support %lld bins as the reference cuts it, %lld bins tapered over %lld samples\n",
              j, (long long)len, (long long)tlen, (long long)se);
    if (f64 ? z64_level(p, bank, L, tlen) < 0 : zoom_class(p, bank, L, tlen) < 0) continue;
    std::copy(part.begin(), part.end(), sup->begin() + 3 * j);
    split->push_back(j);
  }
  return QI_OK;
}

// filter spectra of the edge pieces of the split bands: taps in float64, transformed, scaled by 1 / 4096
template <typename T>
int build_split_edges(qi_plan* p, int32_t B, const std::vector<int32_t>& split, const double* d_par, hipStream_t st) {
  const size_t rows = split.size() * 2;
  if (p->ws_bytes < rows * native::kBlk * sizeof(double2) + 4096) {
    set_error("workspace too small for the taps of the split bands");
    return QI_ERR_NOMEM;
  }
  double2* taps = reinterpret_cast<double2*>(p->ws);
  QI_TRY(upload_table(&p->d_split_bands, split));
  QI_TRY(native::launch_block_taps_edge(taps, (int)(p->native_split_e / 2), p->n, (double)p->native_split_e, d_par, B,
                                        p->d_split_bands, (int)split.size(), st));
  QI_TRY(fft_c2c<double>(p->fft, taps, native::kBlk, (int64_t)rows, HIPFFT_FORWARD, st));
  QI_HIP(hipMalloc(&p->split_bank, rows * native::kBlk * sizeof(cplx<T>)));
  QI_TRY(launch_bank_convert<T>(taps, static_cast<cplx<T>*>(p->split_bank), (int64_t)rows * native::kBlk, 0,
                                1.0 / (double)native::kBlk, st));
  QI_HIP(hipStreamSynchronize(st));
  p->nsplit = (int32_t)split.size();
  p->h_split_bands = split;
  return QI_OK;
}

// Table 3: the short atoms in their circular (length n) form, and the list k_edge_fix corrects their edges from.
template <typename T>
int build_short_table(qi_plan* p, int32_t B, const std::vector<int32_t>& shorts, const std::vector<int32_t>& short_w,
                      const double* d_par, const double* h_par, hipStream_t st) {
  std::vector<double> sup_s((size_t)shorts.size() * 3);
  size_t q = 0;
  while (q < shorts.size()) {
    size_t r = q + 1;
    while (r < shorts.size() && shorts[r] == shorts[r - 1] + 1) ++r;
    std::vector<double> part;
    QI_TRY(analyse_support(p, 1, p->n, B, shorts[q], (int32_t)(r - q), d_par, &part, st));
    std::copy(part.begin(), part.end(), sup_s.begin() + 3 * q);
    q = r;
  }
  QI_TRY(make_native_table<T>(p, 3, 1, p->n, B, shorts, sup_s, short_w, d_par, st));
  p->nat[3].nbands = B;
  std::vector<native::EdgeBand> eb(shorts.size());
  for (size_t i = 0; i < shorts.size(); ++i) {
    const int32_t j = shorts[i];
    eb[i].out_band = j;
    eb[i].w = short_w[i];
    eb[i].p_re = h_par[j];
    eb[i].p_im = h_par[B + j];
    eb[i].omega = h_par[2 * B + j];
    eb[i].amp = h_par[3 * B + j];
    if (short_w[i] > p->edge_wmax) p->edge_wmax = short_w[i];
  }
  QI_TRY(upload_table(&p->d_edge, eb));
  p->nedge = (int32_t)eb.size();
  return QI_OK;
}

// Native bank.  Every atom spectrum is analysed for its support: a narrow one keeps a compact window (one-pass
// "pruned" bands), a wide one its full row.  For the styx bank (zero-padded linear correlation, Lf = 2n) a band whose
// spectrum is wide but whose ATOM is short in time is not run at 2n at all: it is evaluated as a circular
// correlation of length n (half the bank row, half the intermediate, no discarded outputs) and its first / last W
// samples -- the only ones where circular and linear differ -- are corrected by k_edge_fix.
template <typename T>
int build_native_bank(qi_plan* p, int bank, int32_t B, const double* d_par, const double* h_par, hipStream_t st) {
  const int circular = bank == QI_BANK_ATOMS;
  const bool styx = bank == QI_BANK_STYX;
  const int64_t L = circular ? p->n : p->L;
  std::vector<double> sup;
  QI_TRY(analyse_support(p, circular, L, B, 0, B, d_par, &sup, st));
  GaborRoutes routes = classify_gabor_bands(p, bank, L, B, sup, h_par);
  if (styx) {
    release_styx_extras(p);
    p->nat[3].release();
  }
  std::vector<int32_t> split;
  if (styx && p->native_split && gabor_can_block(p, circular) && !routes.picks.empty())  // (their edge items ride in the block launch)
    QI_TRY(find_split_bands(p, bank, L, B, d_par, routes.keep, &sup, &split, st));
  std::vector<double> sup_keep;
  std::vector<int32_t> add_row;
  for (int32_t j : routes.keep) {
    sup_keep.insert(sup_keep.end(), sup.begin() + 3 * j, sup.begin() + 3 * j + 3);
    const auto it = std::find(split.begin(), split.end(), j);
    add_row.push_back(it == split.end() ? 0 : (int32_t)(it - split.begin()) + 1);
  }
  QI_TRY(make_native_table<T>(p, bank, circular, L, B, routes.keep, sup_keep, {}, d_par, st, add_row));
  if (!split.empty()) QI_TRY(build_split_edges<T>(p, B, split, d_par, st));
  p->nat[bank].nbands = B;  // the table's panel has all B rows even when some are produced by table 3 / the block engine
  if (styx) {
    std::stable_sort(routes.picks.begin(), routes.picks.end(), [](const BlockPick& x, const BlockPick& y) { return x.wq < y.wq; });
    QI_TRY(build_block_gabor<T>(p, 0, B, routes.picks, d_par, st));
    if (!routes.shorts.empty()) QI_TRY(build_short_table<T>(p, B, routes.shorts, routes.short_w, d_par, h_par, st));
  }
  return QI_OK;
}

template <typename T>
int build_bank(qi_plan* p, int bank, int32_t B, const double* d_par, hipStream_t st) {
  const int64_t n = p->n;
  const int circular = bank == QI_BANK_ATOMS;
  const int64_t L = circular ? n : p->L;
  const size_t row64 = (size_t)L * sizeof(double2);
  int64_t chunk = (int64_t)(p->ws_bytes / row64);
  if (chunk < 1) {
    set_error("workspace too small to build one bank row (%zu bytes needed)", row64);
    return QI_ERR_NOMEM;
  }
  if (chunk > B) chunk = B;
  double2* rows = reinterpret_cast<double2*>(p->ws);
  cplx<T>* dst = static_cast<cplx<T>*>(p->bank[bank]);
  for (int32_t j0 = 0; j0 < B; j0 += (int32_t)chunk) {
    const int nbk = (B - j0 < chunk) ? B - j0 : (int)chunk;
    QI_TRY(launch_bank_rows(rows, n, L, circular, d_par, d_par + B, d_par + 2 * B, d_par + 3 * B, j0, nbk, st));
    QI_TRY(fft_c2c<double>(p->fft, rows, L, nbk, HIPFFT_FORWARD, st));
    QI_TRY(launch_bank_convert<T>(rows, dst + (int64_t)j0 * L, (int64_t)nbk * L, circular, 1.0 / (double)L, st));
  }
  return QI_OK;
}

// ---- Stockwell table -----------------------------------------------------------------------------------------------------
struct StxRoutes {
  std::vector<BlockPick> picks;             // block engine
  std::vector<native::BandDesc> bands;      // zoom, float64 zoom, two-pass
};

// Every band to the zoom / float64 zoom, block or two-pass engines from its window (shift index, sigma -> coef).
StxRoutes classify_stx_bands(const qi_plan* p, int32_t B, const int64_t* shift_index, const double* sigma,
                             const std::vector<double>& coef) {
  StxRoutes out;
  const bool f64 = p->d.dtype == QI_F64;
  const bool can_block = p->native_block && p->n >= 4 * native::kBlk;
  for (int32_t j = 0; j < B; ++j) {
    // the band's time-domain kernel is a Gaussian of standard deviation sigma_j samples (above 2^-30 of its peak
    // within sqrt(60 ln 2) sigma); it is only that short if the frequency window has decayed before Nyquist
    const double reach = std::ceil(std::sqrt(2.0 * drop_bits(f64) * M_LN2) * sigma[j]) + 1.0;
    const int group = can_block && sigma[j] >= 2.75 ? block_group_of(reach) : 0;
    // support of exp2(-(coef k)^2) above 2^-30: |k| <= kh = sqrt(30) / coef (float64: above 2^-50); 0 bins stands for a
    // window as wide as the record, which no engine takes as a narrow one
    const double kh = std::floor(std::sqrt(support_bits(p)) / coef[j]);
    const int64_t len = 2 * kh + 1 < (double)p->n ? (int64_t)(2 * kh + 1) : 0;
    // (a band of the float64 zoom's finest grids goes to the block engine when that can take it: native_z64_block_from)
    const int z64 = z64_level(p, 2, p->n, len);
    const bool zoom_first = (z64 >= 0 && !z64_level_for_block(p, z64)) ||
                            (group > kBlockMaxWq && zoom_class(p, 2, p->n, len) >= 0);
    if (group > 0 && !zoom_first) {
      BlockPick pk{j, group, shift_index[j]};
      pk.analytic = 1;
      stx_gaussian(pk, p->n, sigma[j]);
      out.picks.push_back(pk);
      continue;
    }
    out.bands.emplace_back();
    native::BandDesc& d = out.bands.back();
    memset(&d, 0, sizeof(d));
    d.shift = shift_index[j];
    d.coef = coef[j];
    d.out_band = j;
    d.mode = band_mode(p, 2, p->n, len);
    if (d.mode != 1) {
      d.k_lo = -(int32_t)kh;
      d.k_len = 2 * (int32_t)kh + 1;
    }
  }
  return out;
}

// Stockwell bands that need the two-pass kernels at a length they do not run: if they are the last (at most four) rows of the
// table, a pass of the hipFFT engine over those rows follows the native run (run_stx_leftover) and they leave `bands`.
void take_stx_leftover(qi_plan* p, int32_t B, std::vector<native::BandDesc>* bands) {
  p->stx_left_lo = -1;
  p->stx_left_n = 0;
  if (native_len_ok(p->n) || p->d.engine == QI_ENGINE_NATIVE) return;
  int32_t lo = B, cnt = 0;
  for (const auto& d : *bands)
    if (d.mode == 1) {
      ++cnt;
      lo = d.out_band < lo ? d.out_band : lo;
    }
  // (the pass tiles the plan's scratch like the hipFFT engine: one record's spectrum, `cnt` rows and the partial sums
  // of the whole table must fit -- else the whole table goes to the hipFFT engine, which tiles over bands)
  const size_t row = (size_t)p->n * (p->d.dtype == QI_F64 ? sizeof(double2) : sizeof(float2));
  const int64_t nblk_e = ceil_div(p->n, kEpiSpan);
  const size_t part = align_up((size_t)B * nblk_e * 8) + align_up((size_t)B * nblk_e * 24);
  const bool left_fits = p->ws_bytes >= part + 2048 + row * (size_t)(cnt + 1);
  if (cnt > 0 && cnt <= 4 && lo == B - cnt && cnt < B && left_fits) {
    bands->erase(std::remove_if(bands->begin(), bands->end(), [](const native::BandDesc& d) { return d.mode == 1; }), bands->end());
    p->stx_left_lo = lo;
    p->stx_left_n = cnt;
  }
}

// The Stockwell table of a plan: nat[2] and blk[2] are left ready, or empty when the hipFFT engine runs the table.
int build_stx_tables(qi_plan* p, int32_t B, const int64_t* shift_index, const double* sigma, const std::vector<double>& coef) {
  if (!native_wanted(p, 2)) {
    if (p->d.engine != QI_ENGINE_NATIVE) return QI_OK;
    set_error("native engine does not support the Stockwell transform at n = %lld", (long long)p->n);
    return QI_ERR_UNSUPPORTED;
  }
  StxRoutes routes = classify_stx_bands(p, B, shift_index, sigma, coef);
  take_stx_leftover(p, B, &routes.bands);
  bool two_pass_free = true;  // no band for pass 1 / pass 2 (their transform lengths are 2^20 and 2^21 only)
  for (const auto& d : routes.bands) two_pass_free = two_pass_free && d.mode >= 2;
  // (float64: the float64 zoom takes its bands inside upload_native_table -- what it leaves is known afterwards)
  bool native = native_len_ok(p->n) || two_pass_free || z64_table(p, 2);
  int rc = QI_OK;
  if (native) {
    rc = upload_native_table(p, 2, p->n, routes.bands);
    // bands left for the two-pass kernels at a length they do not run: the hipFFT engine takes the table
    if (rc == QI_OK && !native_len_ok(p->n) && !p->nat[2].h_rows.empty()) native = false;
  }
  if (rc == QI_OK && native) {
    p->nat[2].nbands = B;
    rc = p->d.dtype == QI_F64 ? build_block_stx<double>(p, routes.picks, coef, nullptr) : build_block_stx<float>(p, routes.picks, coef, nullptr);
  }
  if (rc != QI_OK || !native) drop_stx_tables(p);
  if (rc == QI_OK && !native && p->d.engine == QI_ENGINE_NATIVE) {
    set_error("native engine: this Stockwell band table needs the two-pass kernels, which run 2^20 / 2^21 samples only");
    return QI_ERR_UNSUPPORTED;
  }
  return rc;
}

// ---- what the C ABI shares with the table builds -------------------------------------------------------------------------
void release_styx_extras(qi_plan* p) {
  free_device(p->split_bank);
  free_device(p->d_split_bands);
  p->h_split_bands.clear();
  p->nsplit = 0;
  free_device(p->d_edge);
  p->nedge = 0;
  p->edge_wmax = 0;
}
void drop_gabor_tables(qi_plan* p, int bank) {
  p->nat[bank].release();
  if (bank != QI_BANK_STYX) return;
  p->blk[0].release();
  p->nat[3].release();
  p->nsplit = 0;  // (the split and edge buffers stay until the next build of the bank releases them)
}
void drop_stx_tables(qi_plan* p) {
  p->nat[2].release();
  p->blk[2].release();
  p->stx_left_n = 0;
}
void drop_band_slots(qi_plan* p, int kind) {
  for (auto*& b : p->d_band_slots[kind]) free_device(b);
}

int upload_atom_params(int32_t B, const double* p_re, const double* p_im, const double* omega, const double* amp,
                       std::vector<double>* host, DeviceTemp<double>* d_par) {
  host->resize((size_t)4 * B);
  const double* parts[4] = {p_re, p_im, omega, amp};
  for (int k = 0; k < 4; ++k) memcpy(host->data() + (size_t)k * B, parts[k], B * sizeof(double));
  return upload_table(&d_par->ptr, *host);
}

template int build_native_bank<float>(qi_plan*, int, int32_t, const double*, const double*, hipStream_t);
template int build_native_bank<double>(qi_plan*, int, int32_t, const double*, const double*, hipStream_t);
template int build_bank<float>(qi_plan*, int, int32_t, const double*, hipStream_t);
template int build_bank<double>(qi_plan*, int, int32_t, const double*, hipStream_t);

}  // namespace host
}  // namespace qi

