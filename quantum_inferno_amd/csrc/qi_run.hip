// Launch sequences of the engines: the hipFFT engine (any length), the native float32 engines (two-pass, zoom, block,
// joint launches of qi_cwt_stx), the float64 native path and the small-record engine.
#include "qi_host.hpp"

using namespace qi;

namespace qi {
namespace host {



struct Tile {
  int64_t Ct, Bt, ntb, nblk;
  size_t off_x, off_y, off_pb, off_ps;
};

// Split the plan's scratch into X [Ct][L], Y [Ct][Bt][L] and the reduction partials.
template <typename T>
int plan_tiles(const qi_plan* p, int64_t C, int64_t B, int64_t L, Tile* t) {
  const size_t row = (size_t)L * sizeof(cplx<T>);
  const int64_t nblk = ceil_div(p->n, kEpiSpan);
  const size_t part = align_up((size_t)B * nblk * 8) + align_up((size_t)B * nblk * 24);  // per channel, ntb <= B
  const size_t per_chan_full = row * (size_t)(B + 1) + part + 2048;
  int64_t Ct, Bt;
  if (per_chan_full <= p->ws_bytes) {
    Bt = B;
    Ct = (int64_t)(p->ws_bytes / per_chan_full);
    if (Ct > C) Ct = C;
  } else {
    Ct = 1;
    if (p->ws_bytes < part + 2 * row + 2048) {
      set_error("workspace of %zu bytes cannot hold one (channel, band) tile of %zu bytes", p->ws_bytes,
                part + 2 * row + 2048);
      return QI_ERR_NOMEM;
    }
    Bt = (int64_t)((p->ws_bytes - part - 2048) / row) - 1;
    if (Bt > B) Bt = B;
  }
  t->Ct = Ct;
  t->Bt = Bt;
  t->ntb = ceil_div(B, Bt);
  t->nblk = nblk;
  size_t o = 0;
  t->off_x = o;
  o += align_up(row * (size_t)Ct);
  t->off_y = o;
  o += align_up(row * (size_t)Ct * (size_t)Bt);
  t->off_pb = o;
  o += align_up((size_t)Ct * B * nblk * 8);
  t->off_ps = o;
  return QI_OK;
}

// ---- what one tile of records (first record c0) is asked to write, and where: filled once per tile, copied into every
// argument block of the tile's launches ----
template <typename T>
struct TileOut {
  cplx<T>* coef;
  T* bits;
  T* time_part;  // where the launches leave their per-time sums: planes in scratch, or the output row itself
  T* out_time;
  double* part_band;  // partial sums in scratch (null: not requested) and the outputs they are finalised into
  double* part_stat;
  double* power_band;
  double* stats;
  T power_scale, eps;
  int64_t B, n, nbk, stat_slots;
  int32_t chunk_total;
  // the panel outputs (every argument block has them) ...
  template <typename A>
  void fill_panel(A& a) const {
    a.coef = coef;
    a.bits = bits;
    a.power_scale = power_scale;
    a.eps = eps;
  }
  // ... and the layout of the reductions' partials (RowArgs, ZoomArgs, BlockArgs, Z64Args)
  template <typename A>
  void fill(A& a) const {
    fill_panel(a);
    a.time_part = time_part;
    a.part_band = part_band;
    a.part_stat = part_stat;
    a.nblk = nbk;
    a.stat_stride = stat_slots;
    a.chunk_total = chunk_total;
  }
};

// `time_planes`: the per-time planes in scratch when the launches of a record write more than one (null: straight to the output)
template <typename T>
TileOut<T> tile_out(const qi_tfr_out* out, int64_t c0, int64_t B, int64_t n, T* time_planes, double* part_band,
                    double* part_stat, int64_t nbk, int64_t stat_slots, int chunk_total) {
  TileOut<T> v{};
  v.coef = out->coef ? static_cast<cplx<T>*>(out->coef) + c0 * B * n : nullptr;
  v.bits = out->bits ? static_cast<T*>(out->bits) + c0 * B * n : nullptr;
  v.out_time = out->power_time ? static_cast<T*>(out->power_time) + c0 * n : nullptr;
  v.time_part = v.out_time && time_planes ? time_planes : v.out_time;
  v.part_band = out->power_band ? part_band : nullptr;
  v.part_stat = out->stats ? part_stat : nullptr;
  v.power_band = out->power_band ? static_cast<double*>(out->power_band) + c0 * B : nullptr;
  v.stats = out->stats ? static_cast<double*>(out->stats) + c0 * 4 : nullptr;
  v.power_scale = (T)power_scale_or_default(out->power_scale);
  v.eps = (T)eps_or_default(out->eps);
  v.B = B;
  v.n = n;
  v.nbk = nbk;
  v.stat_slots = stat_slots;
  v.chunk_total = chunk_total;
  return v;
}

// ---- the hipFFT engine (any length) ----
template <typename T>
struct FftTile {
  Tile tl;
  cplx<T>* X;
  cplx<T>* Y;
  double* part_band;
  double* part_stat;
};

template <typename T>
int fft_tile(qi_plan* p, int64_t C, int64_t B, int64_t L, FftTile<T>* f) {
  QI_TRY(plan_tiles<T>(p, C, B, L, &f->tl));
  const Tile& tl = f->tl;
  f->X = reinterpret_cast<cplx<T>*>(p->ws + tl.off_x);
  f->Y = reinterpret_cast<cplx<T>*>(p->ws + tl.off_y);
  f->part_band = reinterpret_cast<double*>(p->ws + tl.off_pb);
  f->part_stat = reinterpret_cast<double*>(p->ws + tl.off_ps);
  QI_LAYOUT_BEGIN(p, "hipFFT-engine tile", false);
  QI_LAYOUT_NOTE(p, "X", f->X, (size_t)tl.Ct * L * sizeof(cplx<T>));
  QI_LAYOUT_NOTE(p, "Y", f->Y, (size_t)tl.Ct * tl.Bt * L * sizeof(cplx<T>));
  QI_LAYOUT_NOTE(p, "part_band", f->part_band, (size_t)tl.Ct * B * tl.nblk * 8);
  QI_LAYOUT_NOTE(p, "part_stat", f->part_stat, (size_t)tl.Ct * B * tl.nblk * 24);
  return QI_OK;
}

// epilogue of bands [j0, j0 + bt) (band tile tile_b of ntile_b) of ct records in Y [ct][bt][L]; out[t] = Y[(t + off) mod L]
template <typename T>
int launch_fft_epilogue(const TileOut<T>& v, const cplx<T>* Y, int64_t L, int64_t off, int64_t ct, int64_t bt, int64_t j0,
                        int64_t tile_b, int64_t ntile_b, hipStream_t st) {
  EpiArgs<T> a{};
  a.Y = Y;
  a.L = L;
  a.n = v.n;
  a.off = off;
  a.Ct = ct;
  a.Bt = bt;
  a.B = v.B;
  a.j0 = j0;
  v.fill_panel(a);
  a.power_time = v.out_time;
  a.part_band = v.part_band;
  a.part_stat = v.part_stat;
  a.tile_b = tile_b;
  a.ntile_b = ntile_b;
  return launch_epilogue<T>(a, st);
}

template <typename T>
int run_transform(qi_plan* p, Kind kind, const void* sig_v, int64_t C, const qi_tfr_out* out, hipStream_t st) {
  const int64_t n = p->n;
  const T* sig = static_cast<const T*>(sig_v);
  int64_t L, B, off;
  const cplx<T>* H = nullptr;
  if (kind == Kind::Linear) {
    L = p->L;
    B = p->nb[QI_BANK_STYX];
    off = (n - 1) / 2;
    H = static_cast<const cplx<T>*>(p->bank[QI_BANK_STYX]);
  } else if (kind == Kind::Circular) {
    L = n;
    B = p->nb[QI_BANK_ATOMS];
    off = n / 2;
    H = static_cast<const cplx<T>*>(p->bank[QI_BANK_ATOMS]);
  } else {
    L = n;
    B = p->nb_stx;
    off = 0;
  }
  if (B <= 0) {
    set_error("plan has no band table for this transform");
    return QI_ERR_STATE;
  }
  FftTile<T> f;
  QI_TRY(fft_tile<T>(p, C, B, L, &f));
  const Tile& tl = f.tl;
  for (int64_t c0 = 0; c0 < C; c0 += tl.Ct) {
    const int64_t ct = (C - c0 < tl.Ct) ? C - c0 : tl.Ct;
    const TileOut<T> v = tile_out<T>(out, c0, B, n, nullptr, f.part_band, f.part_stat, tl.nblk, tl.ntb * tl.nblk, 1);
    p->prof.begin(st, QI_STAGE_FORWARD);
    QI_TRY(launch_pack_pad<T>(sig + c0 * n, f.X, ct, n, L, st));
    QI_TRY(fft_c2c<T>(p->fft, f.X, L, ct, HIPFFT_FORWARD, st));
    p->prof.end(QI_STAGE_FORWARD, st);
    int64_t tb = 0;
    for (int64_t j0 = 0; j0 < B; j0 += tl.Bt, ++tb) {
      const int64_t bt = (B - j0 < tl.Bt) ? B - j0 : tl.Bt;
      p->prof.begin(st, QI_STAGE_MULTIPLY);
      if (kind == Kind::Stockwell)
        QI_TRY(launch_stx_window<T>(f.X, f.Y, ct, bt, n, p->d_stx_idx + j0, p->d_stx_coef + j0, st));
      else
        QI_TRY(launch_mul_bank<T>(f.X, H + j0 * L, f.Y, ct, bt, L, st));
      p->prof.end(QI_STAGE_MULTIPLY, st);
      p->prof.begin(st, QI_STAGE_INVERSE);
      QI_TRY(fft_c2c<T>(p->fft, f.Y, L, ct * bt, HIPFFT_BACKWARD, st));
      p->prof.end(QI_STAGE_INVERSE, st);
      p->prof.begin(st, QI_STAGE_EPILOGUE);
      QI_TRY(launch_fft_epilogue<T>(v, f.Y, L, off, ct, bt, j0, tb, tl.ntb, st));
      p->prof.end(QI_STAGE_EPILOGUE, st);
    }
    if (v.part_band || v.part_stat)
      QI_TRY(launch_finalize(v.part_band, v.part_stat, v.power_band, v.stats, ct, B, v.nbk, v.stat_slots, st));
    p->prof.unchain();
  }
  return QI_OK;
}

// Stockwell rows [stx_left_lo, nb_stx) behind a native run that left them out (qi_plan::stx_left_*): the hipFFT engine's
// window -> inverse transform -> epilogue over just these rows; the per-time sums are added to the native run's, the rows'
// powers and the panel statistics merged by k_left_merge (fixed order).
namespace {
__global__ void __launch_bounds__(256) k_left_merge(const double* __restrict__ part_band, const double* __restrict__ part_stat,
                                                    double* __restrict__ power_band, double* __restrict__ stats, int64_t B,
                                                    int64_t j0, int64_t bt, int64_t nblk) {
  const int64_t c = blockIdx.x;
  if (threadIdx.x < bt && power_band) {
    const double* q = part_band + (c * B + j0 + threadIdx.x) * nblk;
    double s = 0.0;
    for (int64_t b = 0; b < nblk; ++b) s += q[b];
    power_band[c * B + j0 + threadIdx.x] = s;
  }
  if (threadIdx.x == 64 && stats) {
    const double* q = part_stat + ((c * 2 + 1) * nblk) * 3;  // (the epilogue ran as tile 1 of 2)
    double m = stats[c * 4 + 0], s1 = 0.0, s2 = 0.0;
    for (int64_t b = 0; b < nblk; ++b) {
      m = q[3 * b] > m ? q[3 * b] : m;
      s1 += q[3 * b + 1];
      s2 += q[3 * b + 2];
    }
    stats[c * 4 + 0] = m;
    stats[c * 4 + 1] += s1;
    stats[c * 4 + 2] += s2;
  }
}
}  // namespace

template <typename T>
int run_stx_leftover(qi_plan* p, const void* sig_v, int64_t C, const qi_tfr_out* out, hipStream_t st) {
  const int64_t n = p->n, B = p->nb_stx, j0 = p->stx_left_lo, bt = p->stx_left_n;
  const T* sig = static_cast<const T*>(sig_v);
  FftTile<T> f;
  QI_TRY(fft_tile<T>(p, C, B, n, &f));
  const Tile& tl = f.tl;
  if (tl.Bt < bt) {
    set_error("workspace too small for the %lld Stockwell rows behind the native run", (long long)bt);
    return QI_ERR_NOMEM;
  }
  for (int64_t c0 = 0; c0 < C; c0 += tl.Ct) {
    const int64_t ct = (C - c0 < tl.Ct) ? C - c0 : tl.Ct;
    const TileOut<T> v = tile_out<T>(out, c0, B, n, nullptr, f.part_band, f.part_stat, tl.nblk, 0, 1);
    p->prof.begin(st, QI_STAGE_MULTIPLY);
    QI_TRY(launch_pack_pad<T>(sig + c0 * n, f.X, ct, n, n, st));
    QI_TRY(fft_c2c<T>(p->fft, f.X, n, ct, HIPFFT_FORWARD, st));
    QI_TRY(launch_stx_window<T>(f.X, f.Y, ct, bt, n, p->d_stx_idx + j0, p->d_stx_coef + j0, st));
    p->prof.end(QI_STAGE_MULTIPLY, st);
    p->prof.begin(st, QI_STAGE_INVERSE);
    QI_TRY(fft_c2c<T>(p->fft, f.Y, n, ct * bt, HIPFFT_BACKWARD, st));
    p->prof.end(QI_STAGE_INVERSE, st);
    p->prof.begin(st, QI_STAGE_EPILOGUE);
    // (tile 1 of 2, not the first tile of the panel: the per-time sums are ADDED to what the native run wrote)
    QI_TRY(launch_fft_epilogue<T>(v, f.Y, n, 0, ct, bt, j0, 1, 2, st));
    if (v.part_band || v.part_stat) {
      k_left_merge<<<dim3((unsigned)ct), 256, 0, st>>>(f.part_band, f.part_stat, v.power_band, v.stats, B, j0, bt, tl.nblk);
      QI_HIP(hipGetLastError());
    }
    p->prof.end(QI_STAGE_EPILOGUE, st);
  }
  return QI_OK;
}

template int run_stx_leftover<float>(qi_plan*, const void*, int64_t, const qi_tfr_out*, hipStream_t);
template int run_stx_leftover<double>(qi_plan*, const void*, int64_t, const qi_tfr_out*, hipStream_t);

// the item list of table `kind` behind joint launch list `cut` (an item cut, or qi_plan::kDualJoint: BlockTable::joint)
const qi_plan::BlockTable::ItemList& dual_list(const qi_plan* p, int kind, int cut) {
  return cut == qi_plan::kDualJoint ? p->blk[kind].joint : p->blk[kind].var[cut];
}
// the requests whose tail reads per-time planes of both tables of a joint call with few records: a half of a qi_cwt_stx tile
// (joint_call: with the per-time sums and a reduction) at item cut 0
bool joint_planes_wanted(int kind, int cut, bool joint_call) { return joint_call && cut == 0 && kind != 1; }
// does such a run of table `kind` take its share of the table-first dealing of the block launch?
bool joint_deal_wanted(const qi_plan* p, int kind, int cut, bool joint_call) {
  return joint_planes_wanted(kind, cut, joint_call) && p->native_joint_deal != 0 && p->blk[0].ready && p->blk[2].ready;
}
// Work items of the joint block launch: the items of the styx table (0) and of the Stockwell table (2) on the same
// (reach group, block) are paired chunk by chunk -- one forward transform serves both; what has no partner stays single;
// the edge items of the styx table keep their place at the end.  cut = qi_plan::kDualJoint: item cut 0 dealt table-first
// (build_joint_items), the tables' shares in BlockTable::joint.
int build_dual_items(qi_plan* p, int cut) {
  if (p->dual_valid[cut]) return QI_OK;
  free_device(p->d_dual[cut]);
  p->n_dual[cut] = 0;
  std::map<std::pair<int32_t, int32_t>, std::pair<std::vector<native::BlockItem>, std::vector<native::BlockItem>>> at;
  std::vector<native::DualItem> dual, edge;
  if (cut == qi_plan::kDualJoint) QI_TRY(build_joint_items(p, &dual));
  for (const auto& it : dual_list(p, 0, cut).h_items) {
    if (it.wq < 0) edge.push_back({it.wq, it.block, it.band_first, it.band_count, it.plane, it.stat_slot, 0, 0, 0, 0});
    else if (cut != qi_plan::kDualJoint) at[{it.wq, it.block}].first.push_back(it);
  }
  if (cut != qi_plan::kDualJoint)
    for (const auto& it : p->blk[2].var[cut].h_items) at[{it.wq, it.block}].second.push_back(it);
  for (const auto& kv : at) {
    const auto& a = kv.second.first;
    const auto& b = kv.second.second;
    for (size_t i = 0; i < std::max(a.size(), b.size()); ++i) {
      native::DualItem d{kv.first.first, kv.first.second, 0, 0, 0, 0, 0, 0, 0, 0};
      if (i < a.size()) {
        d.first0 = a[i].band_first;
        d.count0 = a[i].band_count;
        d.plane0 = a[i].plane;
        d.slot0 = a[i].stat_slot;
      }
      if (i < b.size()) {
        d.first2 = b[i].band_first;
        d.count2 = b[i].band_count;
        d.plane2 = b[i].plane;
        d.slot2 = b[i].stat_slot;
      }
      dual.push_back(d);
    }
  }
  std::stable_sort(dual.begin(), dual.end(), [](const native::DualItem& x, const native::DualItem& y) {
    const bool lx = x.wq == native::kBlkLongWq, ly = y.wq == native::kBlkLongWq;
    return lx != ly ? lx : x.count0 + x.count2 > y.count0 + y.count2;
  });
  p->n_dual_long[cut] = (int32_t)std::count_if(dual.begin(), dual.end(), [](const native::DualItem& x) { return x.wq == native::kBlkLongWq; });
  dual.insert(dual.end(), edge.begin(), edge.end());
  if (dual.empty()) return QI_OK;
  QI_TRY(upload_table(&p->d_dual[cut], dual));
  p->n_dual[cut] = (int32_t)dual.size();
  p->dual_valid[cut] = true;
  return QI_OK;
}

int launch_zoom_all(qi_plan* p, const native::ZoomArgs<float>& z, int64_t ct, hipStream_t st) {
  p->prof.begin(st, QI_STAGE_ZOOM_COARSE);
  QI_TRY(native::launch_zoom_coarse_gather<float>(z, ct, st));
  p->prof.end(QI_STAGE_ZOOM_COARSE, st);
  p->prof.begin(st, QI_STAGE_ZOOM);
  QI_TRY(native::launch_zoom<float>(z, ct, st));
  p->prof.end(QI_STAGE_ZOOM, st);
  return QI_OK;
}

// the deferred launches of a CWT run, on their own
int flush_carry(qi_plan* p, FusedCarry* c, hipStream_t st) {
  if (!c || !c->active) return QI_OK;
  c->active = false;
  if (c->has_zoom) {
    c->has_zoom = false;
    QI_TRY(launch_zoom_all(p, c->zoom, c->ct, st));
  }
  p->prof.begin(st, QI_STAGE_BLOCK);
  QI_TRY(native::launch_block<float>(c->blk, c->demod, c->ct, st));
  p->prof.end(QI_STAGE_BLOCK, st);
  p->prof.begin(st, QI_STAGE_EPILOGUE);
  QI_TRY(native::launch_tail<float>(c->tail, st));
  p->prof.end(QI_STAGE_EPILOGUE, st);
  return QI_OK;
}

// ---- stages both native drivers (float32: run_native, float64: run_native64) are made of ----

// two-pass sub-tables: the table itself and, for the styx bank, its wide-spectrum short-atom bands evaluated as
// circular correlations of length n (table 3: half the bank row and intermediate; k_edge_fix restores the zero-padded
// result on their first / last samples)
struct Sub {
  const qi_plan::NativeTable* t;
  int kernel_kind;
  int64_t N1, nblk;
  std::vector<int> nchunk;
};
struct TwoPass {
  std::vector<Sub> subs;
  bool shorts = false;
  int chunk_total = 0;                  // chunks (per-time planes) of all pass-2 launches
  int64_t nblk_max = 0, imd_elems = 0;  // most row groups of a sub-table; elements of the largest intermediate
};

constexpr int kPass2Wgs = 256;  // workgroups a pass-2 or float64 interpolation launch should have at least (band chunks are sized for it)

// G: consecutive time residues (rows) per pass-2 workgroup
TwoPass plan_two_pass(const qi_plan* p, int kind, int64_t C, int G) {
  TwoPass tp;
  tp.subs.push_back({&p->nat[kind], kind, 0, 0, {}});
  tp.shorts = kind == 0 && p->nat[3].ready && p->nedge > 0;
  if (tp.shorts) tp.subs.push_back({&p->nat[3], 1, 0, 0, {}});
  for (auto& sb : tp.subs) {
    sb.N1 = sb.t->Lf / native::kN2;
    sb.nblk = sb.N1 / G;
    if (sb.nblk > tp.nblk_max) tp.nblk_max = sb.nblk;
    if ((int64_t)sb.t->imd_slots * sb.t->Lf > tp.imd_elems) tp.imd_elems = (int64_t)sb.t->imd_slots * sb.t->Lf;
    for (const auto& grp : sb.t->groups) {
      // chunks (workgroups along the band list): enough workgroups to fill the chip
      int nc = (int)ceil_div(kPass2Wgs, sb.nblk * C);
      if (nc < 1) nc = 1;
      if (nc > grp.count) nc = grp.count;
      sb.nchunk.push_back(nc);
      tp.chunk_total += nc;
    }
  }
  return tp;
}

// scratch regions of a native run, each [Ct][...] without per-channel padding
template <typename T>
struct Scratch {
  cplx<T>* X;     // spectra of the records
  cplx<T>* Xn;    // short-atom table: their n-point spectra (the even bins of X)
  cplx<T>* imd;   // intermediate of the two-pass kernels
  cplx<T>* zoom;  // coarse arrays of the zoom engine
  cplx<T>* zadd;  // split bands: the tapered part the zoom launches hand to the block launch's edge items
  char* parts0;   // the partial sums (part_band, part_stat), as one range to clear
  size_t parts_bytes;
  double* part_band;
  double* part_stat;
  T* time_part;
  T* edge_p;
  T* edge_time;
  cplx<T>* edge_z;
};
struct ScratchBytes {  // per record
  size_t x = 0, xn = 0, imd = 0, zoom = 0, add = 0, pb = 0, ps = 0, tp = 0, ep = 0, et = 0, ez = 0;
  size_t per_record() const { return x + xn + imd + zoom + add + pb + ps + tp + ep + et + ez; }
};
// the regions whose size both drivers compute alike (x, imd and zoom are the driver's)
template <typename T>
ScratchBytes scratch_bytes(const qi_plan* p, int64_t n, int64_t B, int64_t nbk, int64_t stat_slots, int chunk_total, bool shorts,
                           bool time_via_part, bool panel, int32_t nsplit) {
  ScratchBytes e;
  e.xn = shorts ? (size_t)n * sizeof(cplx<T>) : 0;
  e.pb = (size_t)B * nbk * 8;
  e.ps = (size_t)stat_slots * 24;
  e.tp = time_via_part ? (size_t)chunk_total * n * sizeof(T) : 0;
  e.ep = shorts ? (size_t)p->nedge * 2 * p->edge_wmax * sizeof(T) : 0;
  e.et = shorts ? (size_t)2 * p->edge_wmax * sizeof(T) : 0;
  e.ez = shorts && !panel ? (size_t)p->nedge * 2 * p->edge_wmax * sizeof(cplx<T>) : 0;  // (no panel: the edge samples' own buffer)
  e.add = (size_t)nsplit * n * sizeof(cplx<T>);
  return e;
}

struct Arena {  // the plan's scratch, handed out front to back in regions of Ct records
  const qi_plan* p;
  char* w;
  int64_t Ct;
  const char* what;
  bool shared_first;  // the first region: spectra the CWT run of a joint tile left behind
  template <typename U>
  U* carve(size_t bytes) {
    char* r = w;
    w += align_up(bytes * Ct);
    QI_LAYOUT_NOTE(p, what, r, bytes * Ct, shared_first);
    shared_first = false;
    return reinterpret_cast<U*>(r);
  }
  // the reductions' partials, the per-time planes and the edge buffers: in this order in both drivers
  template <typename T>
  void carve_reductions(const ScratchBytes& e, Scratch<T>* s) {
    s->parts0 = w;
    s->part_band = carve<double>(e.pb);
    s->part_stat = carve<double>(e.ps);
    s->parts_bytes = (size_t)(w - s->parts0);
    s->time_part = carve<T>(e.tp);
    s->edge_p = carve<T>(e.ep);
    s->edge_time = carve<T>(e.et);
    s->edge_z = e.ez ? carve<cplx<T>>(e.ez) : nullptr;
  }
};

// forward stage: spectra of ct records of n samples, zero-padded to Lf, into s.X (native kernels staged through one slot of
// the intermediate, or pack + hipFFT) and, for the short-atom table, their even bins into s.Xn
// low: only the bins (-K, K) into the compact array (native::fwd_low_bins; forward_low(p) holds, so no short-atom table)
template <typename T>
int launch_spectra(qi_plan* p, const T* sig, int64_t n, int64_t Lf, bool shorts, bool have_spectra, bool low,
                   const Scratch<T>& s, int64_t ct, hipStream_t st) {
  p->prof.begin(st, QI_STAGE_FORWARD);
  if (have_spectra) {
    // X already holds the zero-padded spectra of these records
  } else if (p->native_fwd && native_len_ok(Lf)) {
    native::RowArgs<T> f{};
    f.Lf = Lf;
    f.n = n;
    f.N1 = Lf / native::kN2;
    f.N2 = native::kN2;
    f.imd_slots = 1;
    f.imd = s.imd;
    f.sig = sig;
    f.two_over_len = (float)(2.0 / (double)Lf);
    f.debug = 0;
    QI_TRY(native::launch_forward<T>(f, s.X, ct, st, low));
  } else {
    QI_TRY(launch_pack_pad<T>(sig, s.X, ct, n, Lf, st));
    QI_TRY(fft_c2c<T>(p->fft, s.X, Lf, ct, HIPFFT_FORWARD, st));
  }
  if (shorts) QI_TRY(native::launch_even_bins<T>(s.X, s.Xn, ct, n, st));
  p->prof.end(QI_STAGE_FORWARD, st);
  return QI_OK;
}

// two-pass stage: per sub-table and launch group pass 1 for the wide bands, pass 2 with the fused epilogue for every band.
// stat_nblk: part_stat entries per chunk; diag: hand the kernels the plan's debug mask and stamp buffer (float32)
template <typename T>
int launch_two_pass(qi_plan* p, const TwoPass& tp, const TileOut<T>& v, const Scratch<T>& s, int G, int64_t stat_nblk,
                    bool diag, int64_t ct, hipStream_t st) {
  int chunk_base = 0;
  for (size_t si = 0; si < tp.subs.size(); ++si) {
    const Sub& sb = tp.subs[si];
    const auto& t = *sb.t;
    native::RowArgs<T> a{};
    a.Lf = t.Lf;
    a.n = v.n;
    a.N1 = sb.N1;
    a.N2 = native::kN2;
    a.panel_bands = (int32_t)v.B;
    a.imd_slots = t.imd_slots;
    a.X = si == 0 ? s.X : s.Xn;
    a.Hc = static_cast<const cplx<T>*>(t.Hc);
    a.Hfull = static_cast<const cplx<T>*>(t.Hfull);
    a.imd = s.imd;
    a.inv_len = (T)(1.0 / (double)t.Lf);
    a.two_over_len = (float)(2.0 / (double)t.Lf);
    if (diag) {
      a.debug = p->native_debug;
      a.stamps = p->stamps;
    }
    a.neg_last_row = sb.kernel_kind == 0 ? 1 : 0;
    a.edge_z = s.edge_z;
    a.edge_wmax = p->edge_wmax;
    a.nedge = p->nedge;
    v.fill(a);
    a.stat_nblk = stat_nblk;
    for (size_t g = 0; g < t.groups.size(); ++g) {
      const auto& grp = t.groups[g];
      a.bands = t.d_bands + grp.first;
      a.nbands = grp.count;
      a.gen_list = t.d_gen_list ? t.d_gen_list + grp.gen_first : nullptr;
      a.ngen_launch = grp.ngen;
      a.chunk_base = chunk_base;
      if (grp.ngen > 0) {
        p->prof.begin(st, QI_STAGE_PASS1);
        QI_TRY(native::launch_pass1<T>(a, sb.kernel_kind, ct, st));
        p->prof.end(QI_STAGE_PASS1, st);
      }
      p->prof.begin(st, QI_STAGE_PASS2);
      QI_TRY(native::launch_pass2<T>(a, sb.kernel_kind, G, sb.nchunk[g], ct, st));
      p->prof.end(QI_STAGE_PASS2, st);
      chunk_base += sb.nchunk[g];
    }
  }
  return QI_OK;
}

// what the block launch of both precisions is told (float32 adds its long-block count, float64 its tables)
template <typename T>
native::BlockArgs<T> block_args(const qi_plan* p, const qi_plan::BlockTable& bt, const qi_plan::BlockTable::ItemList& il,
                                const TileOut<T>& v, const T* sig, cplx<T>* zadd, int32_t nsplit, int64_t stat_base,
                                int chunk_base) {
  native::BlockArgs<T> b{};
  b.n = v.n;
  b.nitems = il.nitems;
  b.nedge_items = il.nedge_items;
  b.edge_merged = il.edge_merged ? 1 : 0;
  b.nsplit = nsplit;
  b.edge_band = p->d_split_bands;
  b.edge_bank = static_cast<const cplx<T>*>(p->split_bank);
  b.edge_part = zadd;
  b.panel_bands = (int32_t)v.B;
  b.items = il.d_items;
  b.bands = static_cast<const native::BlockBandT<T>*>(il.d_bands);
  b.bank = static_cast<const cplx<T>*>(bt.bank);
  b.sig = sig;
  v.fill(b);
  b.stat_base = stat_base;
  b.chunk_base = chunk_base;
  b.two_over_n = (float)(2.0 / (double)v.n);
  b.debug = p->native_debug;
  b.stamps = p->blk_stamps;
  return b;
}

// edge stage: the zero-padded result on the first / last samples of the short-atom bands (their partials: the last slot of
// a band's row, the last nedge stat slots)
template <typename T>
int launch_edges(const qi_plan* p, const TileOut<T>& v, const Scratch<T>& s, const T* sig, int64_t ct, hipStream_t st) {
  native::EdgeArgs<T> e{};
  e.bands = p->d_edge;
  e.nedge = p->nedge;
  e.panel_bands = (int32_t)v.B;
  e.n = v.n;
  e.wmax = p->edge_wmax;
  e.stat_slots = v.stat_slots;
  e.sig = sig;
  v.fill_panel(e);
  e.edge_z = s.edge_z;
  e.edge_p = s.edge_p;
  return native::launch_edge<T>(e, ct, v.out_time ? s.edge_time : nullptr, v.part_band, v.nbk, v.nbk - 1, v.part_stat,
                                v.stat_slots - p->nedge, st);
}

// the tail of a tile without short-atom bands (the drivers add edge_time / wmax for a run that has them)
template <typename T>
native::TailCall<T> tail_call(const TileOut<T>& v, int64_t ct, const int32_t* band_slots) {
  native::TailCall<T> t;
  t.time_part = v.time_part;
  t.out_time = v.out_time;
  t.ct = ct;
  t.n = v.n;
  t.chunk_total = v.chunk_total;
  t.part_band = v.part_band;
  t.part_stat = v.part_stat;
  t.power_band = v.power_band;
  t.stats = v.stats;
  t.B = v.B;
  t.nbk = v.nbk;
  t.stat_slots = v.stat_slots;
  t.band_slots = band_slots;
  return t;
}

// epilogue: the per-time planes summed into the output row (when there are planes) and the partial sums finalised, in
// fixed order -- one launch when both are wanted
template <typename T>
int launch_reductions(const native::TailCall<T>& t, bool time_via_part, hipStream_t st) {
  const bool sums = t.part_band || t.part_stat;
  if (time_via_part && sums) return native::launch_tail<T>(t, st);
  if (time_via_part)
    QI_TRY(native::launch_time_reduce<T>(t.time_part, t.out_time, t.ct, t.n, t.chunk_total, t.edge_time, t.wmax, st));
  if (sums)
    QI_TRY(launch_finalize(t.part_band, t.part_stat, t.power_band, t.stats, t.ct, t.B, t.nbk, t.stat_slots, st, t.band_slots));
  return QI_OK;
}

// ---- float32 only: the zoom engine's row budget, the deferring / finishing halves of qi_cwt_stx ----

// rows (band chunks, each with a per-time plane) of one zoom launch, per class
struct ZoomRows {
  int count[native::kZoomClasses] = {}, nchunk[native::kZoomClasses] = {};
  int64_t stat_base[native::kZoomClasses] = {}, groups[native::kZoomClasses] = {};
  int planes = 0;                // rows of all classes
  int64_t stats = 0, slots = 0;  // stat slots of the launch; most partial slots a band fills
  // the merged rows (rows 0 .. merge_nchunk - 1, when merge_mask != 0): the classes of the mask run in them and have no
  // rows of their own; their stat slots come first
  int merge_mask = 0, merge_nchunk = 0;
};

constexpr int kZoomWaves = 2048;    // waves each level of a zoom launch of one table should have at least
constexpr int kZoomWgsJoint = 768;  // workgroups per table in the joint launch of qi_cwt_stx (512 .. 1024 measured within 1.5 %)

// joint: the launch is one half of a joint launch of qi_cwt_stx; merge: a half of a qi_cwt_stx tile at item cut 0 (fewer
// than batch_from records) that is asked for the per-time sums and a reduction (joint_planes_wanted) -- then the classes
// of kZoomMergeClasses, whose rows tile the record alike, run in merged rows when there are two or more of them: one
// per-time plane where each class had one.  A rule of the tables and of that condition alone.
ZoomRows plan_zoom_rows(const qi_plan* p, int kind, int64_t C, bool joint, bool merge) {
  constexpr int NL = native::kZoomClasses;
  const auto& zt = p->nat[kind];
  const int64_t n = p->n;
  ZoomRows r;
  // per-class band counts of this call: with few records the launch cannot afford rows for every class (its workgroup
  // budget is dealt over the rows), so the short-interpolator classes run as part of the 10-tap class of their grid
  // (their bands are oversampled enough for any of the three interpolators)
  for (int g = 0; g < NL; ++g) r.count[g] = zt.zoom_count[g];
  if (C < native::kZoomShortFrom) {
    r.count[0] += r.count[5] + r.count[6];
    r.count[5] = r.count[6] = 0;
  }
  if (zt.nzoom <= 0) return r;
  // one launch for every level: each (level, chunk) pair is a row of the grid and owns a per-time plane
  // All workgroups of the launch should be resident at once (zoom_wgs of them) and finish together: every
  // level starts with one row, then the level whose rows carry the most work per workgroup gets the next one
  // (per band: a little more at the higher levels, half at level 3 and up where a workgroup covers half the samples).
  const double level_cost[NL] = {1.0, 1.08, 1.25, 0.75, 1.0, 0.85, 0.75};
  int64_t wgs = 0;
  for (int g = 0; g < NL; ++g) {
    if (r.count[g] <= 0) continue;
    r.groups[g] = native::zoom_groups(n, g);
    r.nchunk[g] = 1;
    wgs += r.groups[g] * C;
  }
  // (in the joint launch of qi_cwt_stx the rows of both tables queue behind each other: there the split by work wins,
  // measured 3 %; in a launch of one table the per-level rule does, 1.5 %)
  const int64_t zoom_wgs = joint && p->native_fuse > 3 ? kZoomWgsJoint : 0;
  if (zoom_wgs > 0) {
    for (;;) {
      int best = -1;
      double best_load = 0.0;
      for (int g = 0; g < NL; ++g) {
        if (r.count[g] <= 0 || r.nchunk[g] >= r.count[g]) continue;
        const double load = level_cost[g] * (double)ceil_div(r.count[g], r.nchunk[g]);
        if (load > best_load) {
          best_load = load;
          best = g;
        }
      }
      if (best < 0 || wgs + r.groups[best] * C > zoom_wgs) break;
      // (a level that cannot grow any more but carries the largest load ends the search: more rows elsewhere would
      // not shorten the launch)
      bool is_max = true;
      for (int g = 0; g < NL; ++g)
        if (r.count[g] > 0 && level_cost[g] * (double)ceil_div(r.count[g], r.nchunk[g]) > best_load) is_max = false;
      if (!is_max) break;
      r.nchunk[best] += 1;
      wgs += r.groups[best] * C;
    }
  } else {
    for (int g = 0; g < NL; ++g) {
      if (r.count[g] <= 0) continue;
      int nc = (int)ceil_div(kZoomWaves, 4 * r.groups[g] * C);
      if (nc < 1) nc = 1;
      if (nc > r.count[g]) nc = r.count[g];
      r.nchunk[g] = nc;
    }
  }
  // merged rows: the classes of kZoomMergeClasses the call uses, when there are two or more, give up their rows for as many
  // merged rows as the class with the most had (one each at 2^20 samples: one merged row); merged row c walks bands
  // c, c + merge_nchunk, ... of every class of the mask
  int merged = 0;
  for (int g = 0; g < NL; ++g)
    if (r.count[g] > 0 && (native::kZoomMergeClasses >> g & 1)) merged += 1;
  if (merge && p->native_zoom_merge != 0 && merged >= 2) {
    for (int g = 0; g < NL; ++g) {
      if (r.count[g] <= 0 || !(native::kZoomMergeClasses >> g & 1)) continue;
      r.merge_mask |= 1 << g;
      if (r.nchunk[g] > r.merge_nchunk) r.merge_nchunk = r.nchunk[g];
      r.nchunk[g] = 0;
    }
    r.planes = r.merge_nchunk;
    r.stats = (int64_t)r.merge_nchunk * native::zoom_groups(n, 0);  // (every class of the mask has class 0's groups)
  }
  for (int g = 0; g < NL; ++g) {
    if (r.count[g] <= 0) continue;
    r.planes += r.nchunk[g];
    r.stat_base[g] = r.stats;
    r.stats += (int64_t)r.nchunk[g] * r.groups[g];
    if (r.groups[g] > r.slots) r.slots = r.groups[g];
  }
  if (tune_env("QI_NATIVE_VERBOSE"))
    fprintf(stderr, "[qi run] zoom launch of table %d: bands per class %d %d %d %d %d | 6-tap %d 4-tap %d in rows %d %d %d %d %d | %d %d, %d merged rows of classes 0x%x, %d planes\n", kind,
            r.count[0], r.count[1], r.count[2], r.count[3], r.count[4], r.count[5],
            r.count[6], r.nchunk[0], r.nchunk[1], r.nchunk[2], r.nchunk[3], r.nchunk[4], r.nchunk[5], r.nchunk[6], r.merge_nchunk,
            r.merge_mask, r.planes);
  return r;
}

// Every engine writes a dense prefix of its bands' partial slots and all of its stat slots, so nothing has to be
// cleared when the finalisation knows each band's slot count (uploaded here on first use); only the short-atom table
// (a second pass-2 geometry plus the edge slot at the end of the row) keeps the cleared layout.
int upload_band_slots(qi_plan* p, int kind, int cut, int64_t nblk_max, bool blocks) {
  if (p->d_band_slots[kind][cut]) return QI_OK;
  std::vector<int32_t> slots((size_t)p->nat[kind].nbands, 0);
  for (int32_t r : p->nat[kind].h_rows) slots[r] = (int32_t)nblk_max;
  // (a merged row has the groups of its classes' own rows: the same slots under either layout)
  for (const auto& z : p->nat[kind].h_zoom) slots[z.first] = (int32_t)native::zoom_groups(p->n, z.second);
  if (blocks)
    for (const auto& b : p->blk[kind].var[cut].h_bands) slots[b.first] = b.second;
  return upload_table(&p->d_band_slots[kind][cut], slots);
}

// the zoom launch of table `kind` (narrow bands of the main table); stat_base, chunk_base: its first stat slot and plane;
// x_shift: X holds the zero-padded spectra a CWT run left behind (the table's own are their even bins)
native::ZoomArgs<float> zoom_args(const qi_plan* p, int kind, const ZoomRows& r, const TileOut<float>& v, const Scratch<float>& s,
                                  bool x_shift, int32_t nsplit, int64_t stat_base, int chunk_base) {
  using T = float;
  const auto& zt = p->nat[kind];
  const int64_t n = v.n;
  native::ZoomArgs<T> z{};
  z.n = n;
  z.Lf = zt.Lf;
  z.planes = zt.zoom_planes;
  z.nbands = zt.nzoom;
  z.panel_bands = (int32_t)v.B;
  z.bands = zt.d_zoom;
  z.plane_band = zt.d_zoom_plane_band;
  z.X = s.X;
  z.x_shift = x_shift ? 1 : 0;
  z.x_mask = (uint32_t)((forward_low(p) ? native::fwd_low_len(zt.Lf) : zt.Lf) << z.x_shift) - 1u;
  z.Hc = static_cast<const cplx<T>*>(zt.Hc);
  z.coarse = s.zoom;
  z.stx = kind == 2 ? 1 : 0;
  // panel sample t is full-length sample t + off: linear correlation off = n/2 - 1, rolled circular n/2, Stockwell 0
  z.lane_off = kind == 0 ? 1 : 0;
  z.tau_off = kind == 2 ? 0 : n / 2 / native::kZoomD;
  z.inv_len = (T)(1.0 / (double)zt.Lf);
  z.two_over_len = (float)(2.0 / (double)zt.Lf);
  v.fill(z);
  z.chunk_base = chunk_base;
  z.split_part = s.zadd;
  z.split_rows = nsplit;
  z.debug = p->native_debug;
  z.merge_mask = r.merge_mask;
  z.merge_nchunk = r.merge_nchunk;
  z.merge_stat_base = stat_base;  // (the merged rows' slots come first)
  int chunk0 = r.merge_nchunk;
  for (int g = 0; g < native::kZoomClasses; ++g) {
    z.lvl_count[g] = r.count[g];
    z.lvl_chunk0[g] = chunk0;
    z.lvl_nchunk[g] = r.nchunk[g];
    z.lvl_stat_base[g] = stat_base + r.stat_base[g];
    z.lvl_weights[g] = p->d_zoom_w[g];  // (a lane's position in its window does not depend on the kind)
    chunk0 += r.nchunk[g];
  }
  int first = 0;
  for (int gi = 0; gi < native::kZoomClasses; ++gi) {  // positions in the band list (kZoomListOrder): a merged class 0 starts where class 6 does
    const int g = kZoomListOrder[gi];
    z.lvl_first[g] = first;
    first += r.count[g];
    if (g == 0 && r.count[0] != zt.zoom_count[0]) z.lvl_first[0] = 0;
  }
  return z;
}

// zoom stage of a tile.  defer (the CWT half of a joint tile, native_fuse > 2): the Stockwell run of qi_cwt_stx launches
// them with its own; finish (the Stockwell half): the launches the CWT run left, jointly with this table's where the
// tiles match.
int launch_zoom_stage(qi_plan* p, const native::ZoomArgs<float>& z, FusedCarry* defer, FusedCarry* finish,
                      int64_t ct, hipStream_t st) {
  using T = float;
  if (defer) {
    defer->zoom = z;
    defer->has_zoom = true;
    defer->ct = ct;
    return QI_OK;
  }
  const bool joint = finish && finish->has_zoom && finish->ct == ct;
  p->prof.begin(st, QI_STAGE_ZOOM_COARSE);
  if (joint) {
    QI_TRY(native::launch_zoom_coarse_gather2<T>(finish->zoom, z, ct, st));
  } else {
    QI_TRY(native::launch_zoom_coarse_gather<T>(z, ct, st));
  }
  p->prof.end(QI_STAGE_ZOOM_COARSE, st);
  p->prof.begin(st, QI_STAGE_ZOOM);
  const bool joint_fine = joint && p->native_fuse > 3 && (finish->zoom.coef != nullptr) == (z.coef != nullptr) &&
                          (finish->zoom.bits != nullptr) == (z.bits != nullptr);
  if (joint_fine) {
    QI_TRY(native::launch_zoom2<T>(finish->zoom, z, ct, st));
  } else {
    if (joint) QI_TRY(native::launch_zoom<T>(finish->zoom, ct, st));
    QI_TRY(native::launch_zoom<T>(z, ct, st));
  }
  if (joint) finish->has_zoom = false;
  p->prof.end(QI_STAGE_ZOOM, st);
  return QI_OK;
}

// block stage of a tile.  defer: the Stockwell run of qi_cwt_stx launches it; finish: the CWT run's block launch goes out
// with this one -- as one joint launch (the styx and the Stockwell bands of a block from one forward transform; the edge
// items of the split bands ride at its end: they add to the interpolation launch's output, which has run by then) when
// both have the same tile, demodulation and panel outputs.
int launch_block_stage(qi_plan* p, const native::BlockArgs<float>& b, int demod, int cut, FusedCarry* defer, FusedCarry* finish,
                       int64_t ct, hipStream_t st) {
  using T = float;
  if (defer) {
    defer->blk = b;
    defer->demod = demod;
    defer->ct = ct;
    return QI_OK;
  }
  const bool joint = finish && p->native_fuse > 1 && finish->ct == ct && !finish->demod && demod &&
                     (finish->blk.coef != nullptr) == (b.coef != nullptr) && (finish->blk.bits != nullptr) == (b.bits != nullptr);
  p->prof.unchain_span();
  p->prof.begin(st, QI_STAGE_BLOCK);
  if (joint) {
    QI_TRY(build_dual_items(p, cut));
    QI_TRY(native::launch_block_dual<T>(finish->blk, b, p->d_dual[cut], p->n_dual[cut], p->n_dual_long[cut],
                                        dual_list(p, 0, cut).nedge_items, ct, st));
  } else {
    if (finish) QI_TRY(native::launch_block<T>(finish->blk, finish->demod, finish->ct, st));
    QI_TRY(native::launch_block<T>(b, demod, ct, st));
  }
  p->prof.end(QI_STAGE_BLOCK, st);
  p->prof.unchain_span();
  return QI_OK;
}

// the tail the CWT run of qi_cwt_stx left and this (Stockwell) run's own: one launch when their tiles match
int launch_tails(FusedCarry* finish, const native::TailCall<float>& tc, hipStream_t st) {
  finish->active = false;
  const native::TailCall<float>& t0 = finish->tail;
  if (t0.ct == tc.ct && t0.n == tc.n) return native::launch_tail2<float>(t0, tc, st);
  QI_TRY(native::launch_tail<float>(t0, st));
  return native::launch_tail<float>(tc, st);
}

// One transform on the native engine: forward FFT of the records, then per table (the styx bank has two:
// the 2n-point linear part and the n-point circular part for short atoms) pass 1 for the wide bands and pass 2 with
// the fused epilogue for every band, the zoom launch of the narrow bands, the block launch of the short-atom bands, the
// edge correction of the short-atom bands, and a fixed-order finalisation of the reductions.
template <typename T>
int run_native(qi_plan* p, int kind, const void* sig_v, int64_t C, const qi_tfr_out* out, hipStream_t st, bool may_share,
               FusedCarry* defer, FusedCarry* finish, size_t* probe) {
  // probe: only report the scratch bytes one record needs when this run is the `defer` (CWT) or the `finish`
  // (Stockwell, spectra shared) half of a joint qi_cwt_stx tile of C records; nothing is launched
  static_assert(std::is_same<T, float>::value, "the native engine is float32");
  const int64_t n = p->n, B = p->nat[kind].nbands, Lf0 = p->nat[kind].Lf;
  const T* sig = static_cast<const T*>(sig_v);
  const int G = p->native_rows;
  // ---- plan the launches: their chunks (per-time planes) and stat slots follow each other in launch order ----
  const TwoPass tp = plan_two_pass(p, kind, C, G);
  const bool shorts = tp.shorts;
  const int chunk_p2 = tp.chunk_total;
  int chunk_total = chunk_p2;
  // block engine launches (one per reach group): their chunks come after the pass-2 chunks
  const auto& bt = p->blk[kind];
  const bool blocks = kind != 1 && bt.ready;
  const int cut = C >= batch_from(p) ? 1 : 0;  // (both halves of a joint tile see the same C and the same tables)
  // qi_cwt_stx (either half of a joint tile, probes included) at item cut 0, asked for the per-time sums and a reduction (the
  // requests whose block launches can go out as one and whose tail reads per-time planes): the table's share of the
  // table-first dealing -- its planes, statistics slots and items, whatever becomes of the joint launch later (the share is
  // a complete item list)
  const bool joint_deal = joint_deal_wanted(p, kind, cut, (defer || finish) && out->power_time && (out->power_band || out->stats));
  const int list = joint_deal ? qi_plan::kDualJoint : cut;
  if (joint_deal) QI_TRY(build_dual_items(p, list));
  const auto& il = dual_list(p, kind, list);
  int64_t blk_stats = 0, blk_slots = 0;
  if (blocks) {
    chunk_total += il.nplanes;
    blk_stats = il.nitems + il.nedge_items;
    blk_slots = bt.max_blocks;
  }
  // zoom engine launch (narrow bands of the main table): its chunks come last
  const auto& zt = p->nat[kind];
  const bool zoom = zt.nzoom > 0;
  const ZoomRows zr = plan_zoom_rows(p, kind, C, defer || (finish && (finish->active || probe)),
                                     joint_planes_wanted(kind, cut, (defer || finish) && out->power_time && (out->power_band || out->stats)));
  const int chunk_z0 = chunk_total;
  chunk_total += zr.planes;
  int64_t nbk = tp.nblk_max + (shorts ? 1 : 0);  // partial slots per band (last one: edge samples)
  if (blk_slots > nbk) nbk = blk_slots;
  if (zr.slots > nbk) nbk = zr.slots;
  const int64_t p2_stats = (int64_t)chunk_p2 * tp.nblk_max;
  const int64_t stat_slots = p2_stats + blk_stats + zr.stats + (shorts ? p->nedge : 0);
  const bool sums = out->power_band || out->stats;
  const bool time_via_part = out->power_time && (chunk_total > 1 || shorts);
  if (!shorts) QI_TRY(upload_band_slots(p, kind, cut, tp.nblk_max, blocks));  // (shorts: the partials are cleared per tile)
  const int32_t* band_slots = shorts ? nullptr : p->d_band_slots[kind][cut];
  // ---- size the scratch ----
  // qi_cwt_stx: the Stockwell call can take its spectra from the even bins of the zero-padded spectra the CWT call
  // left at the start of the scratch -- when nothing of this table needs the n-point spectrum as an array (every band
  // on the zoom / block engines) and both calls hold all records in one tile
  bool share = may_share && kind == 2 && (probe || (p->shared_valid && p->shared_sig == sig_v && p->shared_C == C)) &&
               p->nat[kind].h_rows.empty() && !shorts;
  const int32_t nsplit = kind == 0 ? p->nsplit : 0;  // split bands: the zoom launch hands its part to the block launch
  ScratchBytes e = scratch_bytes<T>(p, n, B, nbk, stat_slots, chunk_total, shorts, time_via_part, out->coef != nullptr, nsplit);
  // low-bins forward transform (a property of the plan: qi_cwt, qi_stx and both halves of qi_cwt_stx agree): X is the
  // compact array of the bins near DC, and the forward transform stages through half a slot of the intermediate
  const bool low = forward_low(p);
  const int64_t x_len = low ? native::fwd_low_len(Lf0) : Lf0;
  const int64_t fwd_imd = low ? native::fwd_low_rows(Lf0 / native::kN2) * native::kN2 : Lf0;
  if (tune_env("QI_NATIVE_VERBOSE"))
    fprintf(stderr, "[qi run] forward transform of table %d (Lf = %lld): %s, bins read (-%lld, %lld)\n", kind, (long long)Lf0,
            low ? "low bins" : "every bin", (long long)table_low_bins(p, kind), (long long)table_low_bins(p, kind));
  e.x = (size_t)(share ? 2 * x_len : x_len) * sizeof(cplx<T>);
  // (the forward transform of the records stages through one slot of the intermediate)
  e.imd = (size_t)(tp.imd_elems < fwd_imd ? fwd_imd : tp.imd_elems) * sizeof(cplx<T>);
  e.zoom = zoom ? (size_t)zt.zoom_planes * native::kBlk * sizeof(cplx<T>) : 0;
  const size_t per_chan = e.per_record();
  if (probe) {
    *probe = per_chan;
    return QI_OK;
  }
  if (p->ws_bytes < per_chan + 4096) {
    set_error("workspace of %zu bytes cannot hold one record's native scratch of %zu bytes", p->ws_bytes,
              per_chan + 4096);
    return QI_ERR_NOMEM;
  }
  int64_t Ct = (int64_t)((p->ws_bytes - 4096) / per_chan);
  if (Ct > C) Ct = C;
  if (share && Ct != C) {
    set_error("internal: shared spectra need all records in one tile");  // cannot happen: the CWT scratch is larger
    return QI_ERR_STATE;
  }
  // ---- qi_cwt_stx: which half of a joint tile this run is ----
  const bool tail_one = time_via_part && sums;
  // a CWT run whose records fit one tile leaves its block launch and tail to the Stockwell run ...
  const bool deferring = defer && kind == 0 && Ct == C && blocks && !shorts && tail_one;
  // ... which keeps the CWT run's scratch intact (its own follows it; only the spectra are shared) and finishes both
  bool finishing = finish && finish->active && kind == 2 && share && blocks && tail_one;
  if (finishing) {
    const size_t need = align_up(e.x * (size_t)C) + align_up(finish->ws_used) + (per_chan - e.x) * (size_t)C + 64 * 256;
    if (need > p->ws_bytes) finishing = false;
  }
  if (finish && finish->active && !finishing) QI_TRY(flush_carry(p, finish, st));  // before this run reuses the scratch
  if (kind == 0) {  // what this call will leave behind for a following qi_cwt_stx Stockwell call
    p->shared_valid = Ct == C;
    p->shared_sig = sig_v;
    p->shared_C = C;
  } else if (!share) {
    p->shared_valid = false;  // the scratch is about to be overwritten
  }
  // ---- carve the scratch ----
  QI_LAYOUT_BEGIN(p, kind == 0 ? "run_native styx" : (kind == 1 ? "run_native atoms" : "run_native stx"), finishing);
  Arena ar{p, p->ws, Ct, "native scratch", share};
  Scratch<T> s{};
  s.X = ar.carve<cplx<T>>(e.x);
  if (finishing) ar.w = p->ws + align_up(finish->ws_used);
  s.Xn = ar.carve<cplx<T>>(e.xn);
  s.imd = ar.carve<cplx<T>>(e.imd);
  ar.carve_reductions(e, &s);
  s.zoom = e.zoom ? ar.carve<cplx<T>>(e.zoom) : nullptr;
  s.zadd = e.add ? ar.carve<cplx<T>>(e.add) : nullptr;
  // ---- per tile: forward, two-pass, zoom, block, edge, epilogue ----
  for (int64_t c0 = 0; c0 < C; c0 += Ct) {
    const int64_t ct = (C - c0 < Ct) ? C - c0 : Ct;
    const T* sig_t = sig + c0 * n;
    const TileOut<T> v = tile_out<T>(out, c0, B, n, time_via_part ? s.time_part : nullptr, s.part_band, s.part_stat, nbk,
                                     stat_slots, chunk_total);
    if (shorts) QI_HIP(hipMemsetAsync(s.parts0, 0, s.parts_bytes, st));
    QI_TRY(launch_spectra<T>(p, sig_t, n, Lf0, shorts, share, low, s, ct, st));
    QI_TRY(launch_two_pass<T>(p, tp, v, s, G, tp.nblk_max, /*diag=*/true, ct, st));
    if (zoom)
      QI_TRY(launch_zoom_stage(p, zoom_args(p, kind, zr, v, s, share, nsplit, p2_stats + blk_stats, chunk_z0),
                               deferring && p->native_fuse > 2 ? defer : nullptr, finishing ? finish : nullptr, ct, st));
    if (finishing && finish->has_zoom) {  // (this table has no zoom band, or another tiling: the deferred launches alone)
      QI_TRY(launch_zoom_all(p, finish->zoom, finish->ct, st));
      finish->has_zoom = false;
    }
    // (the edge items of the block launch finish the split bands the zoom launch began: it comes after it)
    if (blocks) {
      native::BlockArgs<T> b = block_args<T>(p, bt, il, v, sig_t, s.zadd, nsplit, p2_stats, chunk_p2);
      b.nlong = il.nlong;
      QI_TRY(launch_block_stage(p, b, bt.demod, list, deferring ? defer : nullptr, finishing ? finish : nullptr, ct, st));
    }
    p->prof.begin(st, QI_STAGE_EPILOGUE);
    if (shorts) QI_TRY(launch_edges<T>(p, v, s, sig_t, ct, st));
    native::TailCall<T> tc = tail_call<T>(v, ct, band_slots);
    if (deferring) {
      defer->tail = tc;
      defer->ws_used = (size_t)(ar.w - p->ws);
      defer->active = true;
    } else if (finishing) {
      QI_TRY(launch_tails(finish, tc, st));
    } else {
      tc.edge_time = shorts ? s.edge_time : nullptr;
      tc.wmax = p->edge_wmax;
      QI_TRY(launch_reductions<T>(tc, time_via_part, st));
    }
    p->prof.end(QI_STAGE_EPILOGUE, st);
  }
  return QI_OK;
}

// (the chunk count of run_native for one record of a joint tile, without a run)
int64_t joint_planes(qi_plan* p, int kind) {
  if ((kind != 0 && kind != 2) || p->d.dtype != QI_F32 || !p->native_fuse || !p->nat[0].ready || !p->nat[2].ready || p->stx_left_n != 0)
    return 0;
  const int64_t C = 1;
  const int cut = C >= batch_from(p) ? 1 : 0;
  const bool joint_deal = joint_deal_wanted(p, kind, cut, true);
  int64_t planes = plan_two_pass(p, kind, C, p->native_rows).chunk_total + plan_zoom_rows(p, kind, C, true, joint_planes_wanted(kind, cut, true)).planes;
  if (p->blk[kind].ready) {
    if (joint_deal && build_dual_items(p, qi_plan::kDualJoint) != QI_OK) return 0;
    planes += dual_list(p, kind, joint_deal ? qi_plan::kDualJoint : cut).nplanes;
  }
  return planes;
}

// ---- float64 only: the float64 zoom's rows and launches, the block launch with its side stream ----

// float64 zoom bands.  Coarse stage per grid level (gather, batched transform, pads; the levels' coarse arrays lie side by
// side); fine stage: one k_z64_fine launch per class of the three coarsest grids, its bands dealt to `frow` rows, and one
// k_z64_interp launch per finer level, its bands dealt to `zchunk` workgroups per tile.
struct Z64Rows {
  bool fine = false;  // some band runs on the fine kernel
  int zchunk[native::kZ64Levels] = {};
  int frow[native::kZ64FineClasses] = {};
  size_t z_off[native::kZ64Levels] = {};  // per record: offset (elements) of a level's coarse arrays
  size_t bytes = 0;                        // per record: coarse arrays of all levels
  int chunks = 0;                          // rows (per-time planes) of all fine and interpolation launches
};

Z64Rows plan_z64_rows(const qi_plan* p, const qi_plan::NativeTable& t, int64_t C) {
  using T = double;
  const int64_t n = p->n, Lf = t.Lf;
  Z64Rows r;
  for (int c = 0; c < native::kZ64FineClasses; ++c) r.fine = r.fine || t.zf_count[c] > 0;
  const int64_t tiles_f = n / ((int64_t)native::kZ64FineWave * 4);
  for (int g = 0; g < native::kZ64Levels; ++g) {
    if (t.z64_count[g] == 0) continue;
    r.z_off[g] = r.bytes / sizeof(cplx<T>);
    r.bytes += (size_t)t.z64_count[g] * (size_t)(((Lf / 64) << g) + 2 * native::kZ64Pad) * sizeof(cplx<T>);
    if (r.fine && g < native::kZ64FineLevels) continue;
    int nc = (int)ceil_div(kPass2Wgs, (n / native::kZ64Tile) * C);
    r.zchunk[g] = nc < 1 ? 1 : (nc > t.z64_count[g] ? t.z64_count[g] : nc);
    r.chunks += r.zchunk[g];
  }
  for (int c = 0; c < native::kZ64FineClasses; ++c) {
    if (t.zf_count[c] == 0) continue;
    // rows by work: a class's share of the launch budget (a band costs two fused multiply-adds per window sample plus the
    // epilogue), at least one row
    double work = 0.0, mine = (double)t.zf_count[c] * (2.0 * native::z64f_win(c) + 40.0);
    for (int q = 0; q < native::kZ64FineClasses; ++q) work += (double)t.zf_count[q] * (2.0 * native::z64f_win(q) + 40.0);
    const double want_rows = (double)kPass2Wgs / (double)(tiles_f * C);
    int nr = (int)std::ceil(want_rows * (mine / work));
    r.frow[c] = nr < 1 ? 1 : (nr > t.zf_count[c] ? t.zf_count[c] : nr);
    r.chunks += r.frow[c];
  }
  return r;
}

// float64 zoom stage of a tile: coarse stage of every level, then the fine launches (heaviest classes first) and the
// interpolation launches; their planes follow chunk_base.  stat_nblk: part_stat entries per chunk
int launch_z64_stage(qi_plan* p, int kind, const Z64Rows& r, const TileOut<double>& v, const Scratch<double>& s, int32_t nsplit,
                     int64_t stat_nblk, int chunk_base, int64_t ct, hipStream_t st) {
  using T = double;
  const auto& t = p->nat[kind];
  const int64_t n = v.n, Lf = t.Lf;
  native::Z64Args zl[native::kZ64Levels];
  for (int g = 0; g < native::kZ64Levels; ++g) {
    if (t.z64_count[g] == 0) continue;
    native::Z64Args& z = zl[g];
    z = native::Z64Args{};
    z.Lf = Lf;
    z.n = n;
    z.log2d = 6 - g;
    z.M = Lf >> z.log2d;
    z.kind = kind;
    z.nbands = t.z64_count[g];
    z.panel_bands = (int32_t)v.B;
    z.bands = t.d_z64 + t.z64_first[g];
    z.X = s.X;
    z.Hc = static_cast<const cplx<T>*>(t.Hc);
    z.Z = s.zoom + r.z_off[g] * (size_t)ct;  // (levels side by side: [level][record][band][pad | M | pad])
    z.weights = p->d_z64_w[g];
    z.inv_len = 1.0 / (double)Lf;
    z.two_over_len = (float)(2.0 / (double)Lf);
    z.split_part = s.zadd;
    z.split_rows = nsplit;
    v.fill(z);
    z.nblk = n / native::kZ64Tile;  // (the slots a band fills; its row of part_band has pb_stride)
    z.pb_stride = v.nbk;
    z.stat_nblk = stat_nblk;
    p->prof.begin(st, QI_STAGE_ZOOM_COARSE);
    if (g < p->native_z64_coarse && z.M >= native::kBlk) {  // the coarsest grids: gather, transform and pads in one launch
      QI_TRY(native::launch_z64_coarse(z, ct, st));
    } else {
      QI_TRY(native::launch_z64_gather(z, ct, st));
      QI_TRY(fft_z2z_rows(p->fft, z.Z + native::kZ64Pad, z.M, z.M + 2 * native::kZ64Pad, (int64_t)z.nbands * ct, HIPFFT_BACKWARD, st));
      QI_TRY(native::launch_z64_pad(z.Z, z.M, (int64_t)z.nbands * ct, st));
    }
    p->prof.end(QI_STAGE_ZOOM_COARSE, st);
  }
  p->prof.begin(st, QI_STAGE_ZOOM);
  for (int ci = 0; ci < native::kZ64FineClasses; ++ci) {
    const int c = native::kZ64FineClasses - 1 - ci;  // (the shortest interpolators -- the classes with the most bands -- first)
    if (t.zf_count[c] == 0) continue;
    const int g = native::z64f_level(c);
    native::Z64FineArgs f{};
    f.z = zl[g];
    f.z.bands = t.d_z64 + t.zf_first[c];
    f.z.nbands = t.zf_count[c];
    f.z.nblk = n / native::kZ64FineWave;
    f.z.chunk_base = chunk_base;
    f.cls = c;
    f.nrow = r.frow[c];
    f.lvl_bands = t.z64_count[g];
    f.lvl_index0 = t.zf_first[c] - t.z64_first[g];
    f.w = p->d_z64f_w[c];
    f.lane_ph = t.d_z64_lane_ph ? t.d_z64_lane_ph + (int64_t)t.zf_first[c] * 65 : nullptr;
    f.wave_ph = t.d_z64_wave_ph;
    f.debug = p->native_debug;
    QI_TRY(native::launch_z64_fine(f, ct, st));
    chunk_base += r.frow[c];
  }
  for (int g = 0; g < native::kZ64Levels; ++g) {
    if (r.zchunk[g] == 0) continue;
    zl[g].chunk_base = chunk_base;
    QI_TRY(native::launch_z64_interp(zl[g], r.zchunk[g], ct, st));
    chunk_base += r.zchunk[g];
  }
  p->prof.end(QI_STAGE_ZOOM, st);
  return QI_OK;
}

// float64 block launch (k_block64; the split bands' edge items, k_block64_edge, on the plan's side stream)
int launch_block64(qi_plan* p, native::BlockArgs<double> b, const qi_plan::BlockTable& bt,
                   const qi_plan::BlockTable::ItemList& il, int64_t ct, hipStream_t st) {
  using T = double;
  if (b.nsplit <= 0) b.nedge_items = 0;
  b.edge_wq = (int32_t)(p->native_split_e / 512);
  b.gauss_w = static_cast<const T*>(il.d_gauss_w);
  b.demod_pow = static_cast<const cplx<T>*>(il.d_demod_pow);
  b.demod_t1 = p->d_demod_t1;
  b.demod_t2 = p->d_demod_t2;
  p->prof.begin(st, QI_STAGE_BLOCK);
  if (b.nedge_items > 0 && !p->side) {
    QI_HIP(hipStreamCreateWithFlags(&p->side, hipStreamNonBlocking));
    QI_HIP(hipEventCreateWithFlags(&p->ev_fork, hipEventDisableTiming));
    QI_HIP(hipEventCreateWithFlags(&p->ev_join, hipEventDisableTiming));
  }
  QI_TRY(native::launch_block<T>(b, bt.demod, ct, st, p->side, p->ev_fork, p->ev_join));
  p->prof.end(QI_STAGE_BLOCK, st);
  return QI_OK;
}

// float64 records on the native engines in double arithmetic: forward transform of the records (the two-pass kernels in
// double where they exist, 2^20- and 2^21-point transforms; hipFFT elsewhere); whatever is left on the exact two-pass
// kernels (per launch group pass 1 for the wide bands, pass 2 with the pruned loader and the fused epilogue, 8-row
// workgroups, Cfg<double, 8>); the bands the float64 zoom takes (split bands leave their tapered part in scratch), the block
// engine's bands (k_block64) and the split bands' edge items (k_block64_edge); one tail launch.
int run_native64(qi_plan* p, int kind, const void* sig_v, int64_t C, const qi_tfr_out* out, hipStream_t st) {
  using T = double;
  const auto& t = p->nat[kind];
  const int64_t n = p->n, B = kind == 2 ? p->nb_stx : p->nb[kind], Lf = t.Lf;
  constexpr int G = 8;
  const T* sig = static_cast<const T*>(sig_v);
  // ---- plan the launches: two-pass chunks, then the float64 zoom's rows, then the block engine's planes ----
  const TwoPass tp = plan_two_pass(p, kind, C, G);
  const bool shorts = tp.shorts;
  const Z64Rows zr = plan_z64_rows(p, t, C);
  // partial slots per band: the row groups of the two-pass kernels (the circular sub-table has half as many) or the tiles
  // of the float64 zoom, whichever is more
  // (the fine kernel's waves fill one slot per band and kZ64FineWave samples, k_z64_interp's workgroups one per kZ64Tile)
  const int64_t nblk_z = zr.fine ? n / native::kZ64FineWave : n / native::kZ64Tile;
  int64_t nblk = tp.subs[0].nblk > nblk_z ? tp.subs[0].nblk : nblk_z;
  // block engine (short-atom bands with wide spectra, double arithmetic): its planes and stat slots come last
  const auto& bt = p->blk[kind];
  const bool blocks = kind != 1 && bt.ready;
  if (blocks && bt.max_blocks > nblk) nblk = bt.max_blocks;
  // (some bands leave slots unwritten: the block bands fill one slot per block of their reach group)
  const bool clear_parts = shorts || tp.subs[0].nblk != nblk || blocks;
  const auto& il = bt.var[C >= 4 ? 1 : 0];
  const int chunk_blk = tp.chunk_total + zr.chunks;
  const int chunk_total = chunk_blk + (blocks ? il.nplanes : 0);
  const int64_t blk_stats = blocks ? il.nitems + il.nedge_items : 0;
  const int32_t nsplit = kind == 0 && blocks ? p->nsplit : 0;  // split bands: the zoom launches hand their part to the edge items
  // stat slots: [chunks of the two-pass and zoom launches][nblk], then one per block item, then the edge bands
  const int64_t blk_stat_base = (int64_t)chunk_blk * nblk;
  const int64_t stat_slots = blk_stat_base + blk_stats + (shorts ? p->nedge : 0);
  if (chunk_total == 0) {
    set_error("float64 native table has no band");
    return QI_ERR_STATE;
  }
  const bool time_via_part = out->power_time && (chunk_total > 1 || shorts);
  const int64_t nbk = nblk + (shorts ? 1 : 0);  // partial slots per band (last one: the corrected edge samples)
  // ---- size and carve the scratch ----
  ScratchBytes e = scratch_bytes<T>(p, n, B, nbk, stat_slots, chunk_total, shorts, time_via_part, out->coef != nullptr, nsplit);
  e.x = (size_t)Lf * sizeof(cplx<T>);
  // (a native forward transform of the records stages through one slot of the intermediate)
  e.imd = (size_t)(p->native_fwd && native_len_ok(Lf) && tp.imd_elems < Lf ? Lf : tp.imd_elems) * sizeof(cplx<T>);
  e.zoom = zr.bytes;
  const size_t per_chan = e.per_record();
  if (p->ws_bytes < per_chan + 16384) {
    set_error("workspace of %zu bytes cannot hold one record's float64 scratch of %zu bytes", p->ws_bytes, per_chan + 16384);
    return QI_ERR_NOMEM;
  }
  int64_t Ct = (int64_t)((p->ws_bytes - 16384) / per_chan);
  if (Ct > C) Ct = C;
  p->shared_valid = false;
  QI_LAYOUT_BEGIN(p, kind == 2 ? "run_native64 stx" : "run_native64 gabor", false);
  Arena ar{p, p->ws, Ct, "native64 scratch", false};
  Scratch<T> s{};
  s.X = ar.carve<cplx<T>>(e.x);
  s.Xn = ar.carve<cplx<T>>(e.xn);
  s.imd = ar.carve<cplx<T>>(e.imd);
  s.zoom = ar.carve<cplx<T>>(e.zoom);
  s.zadd = e.add ? ar.carve<cplx<T>>(e.add) : nullptr;
  ar.carve_reductions(e, &s);  // (the partial sums: cleared per tile when the sub-tables fill different numbers of slots)
  // ---- per tile: forward, two-pass, zoom, block, edge, epilogue ----
  for (int64_t c0 = 0; c0 < C; c0 += Ct) {
    const int64_t ct = (C - c0 < Ct) ? C - c0 : Ct;
    const T* sig_t = sig + c0 * n;
    const TileOut<T> v = tile_out<T>(out, c0, B, n, time_via_part ? s.time_part : nullptr, s.part_band, s.part_stat, nbk,
                                     stat_slots, chunk_total);
    if (clear_parts) QI_HIP(hipMemsetAsync(s.parts0, 0, s.parts_bytes, st));
    QI_TRY(launch_spectra<T>(p, sig_t, n, Lf, shorts, false, /*low=*/false, s, ct, st));
    QI_TRY(launch_two_pass<T>(p, tp, v, s, G, nblk, /*diag=*/false, ct, st));
    QI_TRY(launch_z64_stage(p, kind, zr, v, s, nsplit, nblk, tp.chunk_total, ct, st));
    if (blocks)
      QI_TRY(launch_block64(p, block_args<T>(p, bt, il, v, sig_t, s.zadd, nsplit, blk_stat_base, chunk_blk), bt, il, ct, st));
    p->prof.begin(st, QI_STAGE_EPILOGUE);
    if (shorts) QI_TRY(launch_edges<T>(p, v, s, sig_t, ct, st));
    native::TailCall<T> tc = tail_call<T>(v, ct, nullptr);
    tc.edge_time = shorts ? s.edge_time : nullptr;
    tc.wmax = p->edge_wmax;
    QI_TRY(launch_reductions<T>(tc, time_via_part, st));
    p->prof.end(QI_STAGE_EPILOGUE, st);
    p->prof.unchain();
  }
  return QI_OK;
}

// ---- the small-record engine (qi_small.hip) -----------------------------------------------------------------------------
// Per table of a run: forward launch, band launch (nchunk workgroups per record, each with the band's whole row), tail.
// Scratch per record: one spectrum row, one partial per band, three statistics per chunk and -- when the per-time sums are
// wanted and there is more than one chunk -- one per-time plane per chunk.
template <typename T>
struct SmallJob {
  int kind = 0;
  const qi_tfr_out* out = nullptr;
  int64_t L = 0, B = 0, off = 0;
  const cplx<T>* H = nullptr;
  int nchunk = 1;
  bool planes = false;
  size_t bytes(const qi_plan* p, int64_t ct) const {
    return align_up((size_t)L * sizeof(cplx<T>) * ct) + align_up((size_t)B * 8 * ct) + align_up((size_t)nchunk * 24 * ct) +
           (planes ? align_up((size_t)nchunk * p->n * sizeof(T) * ct) : 0);
  }
};

template <typename T>
int run_small(qi_plan* p, int njobs, const int* kinds, const qi_tfr_out* const* outs, const void* sig_v, int64_t C, hipStream_t st,
              bool* ran) {
  const int64_t n = p->n;
  const T* sig = static_cast<const T*>(sig_v);
  *ran = false;
  SmallJob<T> job[2];
  size_t per_record = 0;
  for (int q = 0; q < njobs; ++q) {
    SmallJob<T>& jb = job[q];
    jb.kind = kinds[q];
    jb.out = outs[q];
    jb.L = jb.kind == 0 ? p->L : n;
    jb.B = jb.kind == 2 ? p->nb_stx : p->nb[jb.kind];
    jb.off = jb.kind == 0 ? (n - 1) / 2 : jb.kind == 1 ? n / 2 : 0;  // (run_transform's constants)
    jb.H = jb.kind == 2 ? nullptr : static_cast<const cplx<T>*>(p->bank[jb.kind]);
    if (jb.B <= 0) {
      set_error("plan has no band table for this transform");
      return QI_ERR_STATE;
    }
    // band chunks: small_chunk_bands bands each, fewer (down to one: no planes at all) only when the workspace cannot hold
    // the planes -- the count depends on the table, the workspace and the outputs asked for, never on the records of the call
    jb.nchunk = (int)ceil_div(jb.B, p->small_chunk_bands > 0 ? p->small_chunk_bands : 1);
    for (;;) {
      jb.planes = jb.out->power_time && jb.nchunk > 1;
      if (jb.bytes(p, 1) <= p->ws_bytes || jb.nchunk == 1) break;
      jb.nchunk = (jb.nchunk + 1) / 2;
    }
    per_record += jb.bytes(p, 1);
  }
  if (per_record > p->ws_bytes) return QI_OK;  // (not even one record: the caller's fallback)
  int64_t Ct = (int64_t)(p->ws_bytes / per_record);
  if (Ct > C) Ct = C;
  *ran = true;
  const bool joint_tail = njobs == 2 && p->small_joint > 1;
  for (int64_t c0 = 0; c0 < C; c0 += Ct) {
    const int64_t ct = C - c0 < Ct ? C - c0 : Ct;
    QI_LAYOUT_BEGIN(p, "small-engine tile", false);
    Arena ar{p, p->ws, ct, "small", false};
    cplx<T>* X[2] = {nullptr, nullptr};
    TileOut<T> v[2];
    for (int q = 0; q < njobs; ++q) {
      const SmallJob<T>& jb = job[q];
      X[q] = ar.carve<cplx<T>>((size_t)jb.L * sizeof(cplx<T>));
      double* part_band = ar.carve<double>((size_t)jb.B * 8);
      double* part_stat = ar.carve<double>((size_t)jb.nchunk * 24);
      T* planes = jb.planes ? ar.carve<T>((size_t)jb.nchunk * n * sizeof(T)) : nullptr;
      v[q] = tile_out<T>(jb.out, c0, jb.B, n, planes, part_band, part_stat, 1, jb.nchunk, jb.planes ? jb.nchunk : 1);
    }
    // forward: the zero-padded 2n-point spectra for the styx bank, the n-point spectra for the other tables -- one launch
    cplx<T>*X2 = nullptr, *X1 = nullptr;
    for (int q = 0; q < njobs; ++q) (job[q].kind == 0 ? X2 : X1) = X[q];
    p->prof.begin(st, QI_STAGE_FORWARD);
    QI_TRY(native::launch_small_forward<T>(sig + c0 * n, X2, X1, static_cast<const cplx<T>*>(p->small_tw), 2 * n, n, ct, st));
    p->prof.end(QI_STAGE_FORWARD, st);
    native::TailCall<T> tc[2];
    for (int q = 0; q < njobs; ++q) {
      const SmallJob<T>& jb = job[q];
      native::SmallArgs<T> a{};
      a.X = X[q];
      a.H = jb.H;
      a.stx_idx = p->d_stx_idx;
      a.stx_coef = p->d_stx_coef;
      a.tw = static_cast<const cplx<T>*>(p->small_tw);
      a.tw_shift = jb.L == 2 * n ? 0 : 1;
      a.kind = jb.kind;
      a.n = (int32_t)n;
      a.L = (int32_t)jb.L;
      a.off = (int32_t)jb.off;
      a.B = (int32_t)jb.B;
      a.nchunk = jb.nchunk;
      a.chunk_total = v[q].chunk_total;
      v[q].fill_panel(a);
      a.time_part = v[q].time_part;
      a.part_band = v[q].part_band;
      a.part_stat = v[q].part_stat;
      p->prof.begin(st, QI_STAGE_SMALL);
      QI_TRY(native::launch_small_band<T>(a, ct, st));
      p->prof.end(QI_STAGE_SMALL, st);
      tc[q] = tail_call<T>(v[q], ct, nullptr);
    }
    p->prof.begin(st, QI_STAGE_EPILOGUE);
    auto sums = [](const native::TailCall<T>& t) { return t.part_band || t.part_stat; };
    if (joint_tail && job[0].planes && job[1].planes && sums(tc[0]) && sums(tc[1])) {
      QI_TRY(native::launch_tail2<T>(tc[0], tc[1], st));
    } else {
      for (int q = 0; q < njobs; ++q)
        if (job[q].planes || sums(tc[q])) QI_TRY(launch_reductions<T>(tc[q], job[q].planes, st));
    }
    p->prof.end(QI_STAGE_EPILOGUE, st);
    p->prof.unchain();
  }
  return QI_OK;
}

template int run_small<float>(qi_plan*, int, const int*, const qi_tfr_out* const*, const void*, int64_t, hipStream_t, bool*);
template int run_small<double>(qi_plan*, int, const int*, const qi_tfr_out* const*, const void*, int64_t, hipStream_t, bool*);
template int run_transform<float>(qi_plan*, Kind, const void*, int64_t, const qi_tfr_out*, hipStream_t);
template int run_transform<double>(qi_plan*, Kind, const void*, int64_t, const qi_tfr_out*, hipStream_t);
template int run_native<float>(qi_plan*, int, const void*, int64_t, const qi_tfr_out*, hipStream_t, bool, FusedCarry*, FusedCarry*,
                               size_t*);

}  // namespace host
}  // namespace qi
