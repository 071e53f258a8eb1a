// Cross-spectra between the records of a batch (include/qi_array.h): for every bin f the Hermitian matrix
//   S_f = weight[f] Z_f^H Z_f,  Z_f [segments x records],  S[f][i][j] = weight[f] sum_s conj(Z[i][f][s]) Z[j][f][s]
// (scipy.signal.csd's convention), and the magnitude-squared coherence |S_ij|^2 / (S_ii S_jj) of the finished matrices.
//
// The contraction is a batch of nf complex rank-nseg updates and runs on the matrix cores in the records' precision:
// v_mfma_f32_16x16x4_f32 (bit for bit a k-ordered float32 fmaf chain) and v_mfma_f64_16x16x4_f64.
//
// Tile.  A 16 x 16 tile of record pairs (I, J), J >= I, at one bin f is summed by one WAVE over ALL segments; the segment
// index is the K of the instruction.  Lane l supplies record I + (l & 15) as the A operand and record J + (l & 15) as the B
// operand, both at segment slot l >> 4 -- the two operands have the same lane layout, so a diagonal tile loads one set of
// registers and passes it twice.  A wave takes up to four tiles J of one tile row I (two in float64, one where there is one):
// they share the A operand's loads.  Four real accumulators per tile (independent: they also cover the instruction's 40-cycle
// dependent latency)
//   rr = sum Zr_i Zr_j,  ii = sum Zi_i Zi_j,  ri = sum Zr_i Zi_j,  ir = sum Zi_i Zr_j
// and conj(Z_i) Z_j = (Zr_i - i Zi_i)(Zr_j + i Zi_j) = (Zr_i Zr_j + Zi_i Zi_j) + i (Zr_i Zi_j - Zi_i Zr_j):
//   Re S = rr + ii,  Im S = ri - ir.
// Tiles below the diagonal are not computed: an entry with i < j is stored from its registers to [i][j] and, with the sign
// of the imaginary part flipped, to [j][i]; a diagonal tile stores its upper triangle only, and [i][i] with imaginary part 0.
//
// Loads.  The sum over K has no prescribed order, so lane (record r, slot g) loads V consecutive segments 4 V t + V g ..
// + V - 1 of its record in iteration t (V = 4 float2, 2 double2: 32 bytes a lane) and feeds them as V successive K steps:
// a record's row is read 128 contiguous bytes per iteration, straight from global memory into the operands -- every element
// is used once per tile, so LDS staging would only add a round trip.  Records past C and segments past nseg enter as zero
// operands and are never stored.
//
// Work split.  Grid = (groups of tiles of a tile row, on and above the diagonal) x ceil(nf / 4) workgroups of four waves, a
// wave per bin; no wave shares a sum with another, so there are no partial sums to combine.  The K order of an entry depends
// on nseg alone and each output element of the instruction is its own chain: an entry is a function of its two records,
// whatever the batch, their places in it and the tiles a wave takes.
//
// Windows (include/qi_windows.h).  k_cross_spectra_windows forms one matrix per (window of segments, formed bin) with the same
// wave: the body is qi_csd_wave.inc, included by both kernels, with the window's first segment and length where the panel's 0
// and nseg stand -- a window's sums are k_cross_spectra's on the contiguous slice bit for bit, and what the panel holds past
// the window's end is a zero operand.
//
// Bands (include/qi_bands.h).  k_cross_spectra_bands forms one matrix per (band, window of that band's own length, hop and
// sample stride) of a constant-Q panel with the same wave and the same text: term k of a window is the sample first + k stride
// where the other kernels have segment k, so a window's sums are k_cross_spectra's on the contiguous strided copy bit for
// bit.  With a stride above 1 a lane's V operands are V separate 8- or 16-byte loads instead of one 32-byte run.
#include "qi_host.hpp"
#include "qi_device.hpp"   // kWave
#include "qi_fft_reg.hpp"  // QI_LAUNCH_CHECK
#include "qi_mfma.hpp"     // Mx
#include "qi_array.h"
#include "qi_windows.h"
#include "qi_bands.h"

#include <cstring>
#include <vector>

using namespace qi;
using qi::host::align_up;

namespace {

constexpr int kCsdTile = 16;      // records per tile side (the instruction's M and N)
constexpr int kCsdWaves = 4;      // waves (bins) per workgroup

struct CsdArgs {
  int64_t C, nf, nseg;
  int64_t ntile;  // tiles per matrix side
  int64_t nfb;    // workgroups per tile pair: ceil(nf / kCsdWaves)
  CsdWeight w;
};

__device__ __forceinline__ double csd_weight(const CsdWeight& w, int64_t f, int64_t nf) {
  if (w.table) return w.table[f];
  const bool paired = f > 0 && !(w.nfft % 2 == 0 && f == nf - 1);
  return paired ? w.paired : w.edge;
}

// V consecutive segments from `s` of one record's row; CHECK: the ragged end (segments past nseg are zero operands)
template <typename T, bool CHECK>
__device__ __forceinline__ void csd_load(const cplx<T>* __restrict__ row, bool on, int64_t s, int64_t nseg, cplx<T>* x) {
  constexpr int V = Mx<T>::V;
#pragma unroll
  for (int v = 0; v < V; ++v) {
    const bool in = on && (!CHECK || s + v < nseg);
    x[v] = in ? row[s + v] : mk<T>(T(0), T(0));
  }
}
// the same of a row whose segments lie `step` elements apart (the banded kernel's sample stride)
template <typename T, bool CHECK>
__device__ __forceinline__ void csd_load_strided(const cplx<T>* __restrict__ row, bool on, int64_t s, int64_t nseg, int64_t step,
                                                 cplx<T>* x) {
  constexpr int V = Mx<T>::V;
#pragma unroll
  for (int v = 0; v < V; ++v) {
    const bool in = on && (!CHECK || s + v < nseg);
    x[v] = in ? row[(s + v) * step] : mk<T>(T(0), T(0));
  }
}

// groups of up to `nj` tiles in row ti of the upper triangle of a matrix of `ntile` tiles a side
__host__ __device__ inline int64_t csd_row_groups(int64_t ntile, int64_t ti, int nj) { return (ntile - ti + nj - 1) / nj; }

// NJ: tiles of one tile row a wave takes -- they share the A operand's loads; a matter of registers and traffic, not of results.
// The wave's work is qi_csd_wave.inc, the text that the windowed and the banded kernel below share.
#define CSD_WAVE_LOAD(row, on, out) csd_load<T, CHECK>(row, on, s, len, out)
template <typename T, int NJ>
__global__ void __launch_bounds__(kCsdWaves* kWave) k_cross_spectra(const cplx<T>* __restrict__ Z, cplx<T>* __restrict__ S, CsdArgs a) {
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int64_t f = ((int64_t)blockIdx.x % a.nfb) * kCsdWaves + wv;
  if (f >= a.nf) return;  // (the whole wave)
  int64_t p = (int64_t)blockIdx.x / a.nfb;
  const int64_t first = 0, len = a.nseg, m = f;
  auto weight = [&] { return csd_weight(a.w, f, a.nf); };
#include "qi_csd_wave.inc"
}

// The windowed form (include/qi_windows.h): matrix [w][fr] is the sum over the segments w hop .. w hop + win - 1 of bin
// bin_first + fr.  p.nfb counts the workgroups of the FORMED bins.  The window index runs fastest in the grid: workgroups that
// are resident together read overlapping segments of the same rows, so a line that several windows share is still in cache
// when the next one asks for it (workgroups b and b + 8 share an XCD's L2; neighbours meet in the Infinity Cache).
struct CsdWindowArgs {
  CsdArgs p;
  int64_t bin_first, bin_count, win, hop, nwin;
};

template <typename T, int NJ>
__global__ void __launch_bounds__(kCsdWaves* kWave) k_cross_spectra_windows(const cplx<T>* __restrict__ Z, cplx<T>* __restrict__ S,
                                                                            CsdWindowArgs aw) {
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int64_t wi = (int64_t)blockIdx.x % aw.nwin, rest = (int64_t)blockIdx.x / aw.nwin;
  const int64_t fr = (rest % aw.p.nfb) * kCsdWaves + wv;
  if (fr >= aw.bin_count) return;  // (the whole wave)
  const CsdArgs& a = aw.p;
  int64_t p = rest / a.nfb;
  const int64_t f = aw.bin_first + fr, first = wi * aw.hop, len = aw.win, m = wi * aw.bin_count + fr;
  // a table holds one weight per FORMED bin; without one the one-sided doubling goes by the absolute bin
  auto weight = [&] { return a.w.table ? a.w.table[fr] : csd_weight(a.w, f, a.nf); };
#include "qi_csd_wave.inc"
}

// The banded form (include/qi_bands.h): matrix offset[b] + w of the band-major stack is the sum over the samples
// w hop[b] + k stride[b], k < terms[b], of band band_first + b.  The device tables lie in scratch, put there in stream order
// before the launch: offset [band_count + 1], terms, hop, stride [band_count] int64 and, where the caller gave weights,
// weight [band_count] double.  The matrix index runs fastest in the grid and the four waves of a workgroup take four
// consecutive matrices: adjacent windows of a band read overlapping samples of the same rows.  A wave finds its band by a
// binary search of offset[]: the matrix index is wave-uniform, so the search runs on scalar loads and no lane diverges.
struct CsdBandArgs {
  CsdArgs p;  // C, nf = the panel's bands, nseg = the panel's samples n, ntile; nfb: workgroups per tile group = ceil(total / 4)
  int64_t band_first, band_count, total;
  const int64_t *offset, *terms, *hop, *stride;
  const double* weight;
};

// Waves per SIMD the register allocator is held to, by precision and NJ (profiles/bands_kernel_resources.txt).  Every strided
// load keeps a 64-bit address of its own where the contiguous kernels have one address and immediate offsets; held to these
// counts the kernels stay out of scratch.  The banded launch takes at most two tiles a wave in either precision: at four the
// float32 kernel would be down to one wave.
template <typename T, int NJ>
constexpr int csd_band_waves() {
  return sizeof(T) == 8 ? (NJ == 1 ? 4 : 2) : (NJ == 1 ? 4 : 3);
}

template <typename T, int NJ>
__global__ void __launch_bounds__(kCsdWaves* kWave) __attribute__((amdgpu_waves_per_eu(csd_band_waves<T, NJ>())))
k_cross_spectra_bands(const cplx<T>* __restrict__ Z, cplx<T>* __restrict__ S,
                                                                          CsdBandArgs ab) {
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const CsdArgs& a = ab.p;
  const int64_t m = ((int64_t)blockIdx.x % a.nfb) * kCsdWaves + wv;
  if (m >= ab.total) return;  // (the whole wave)
  int64_t p = (int64_t)blockIdx.x / a.nfb;
  // the band b with offset[b] <= m < offset[b + 1] (every band holds a window: the offsets ascend strictly)
  int64_t lo = 0, hi = ab.band_count;
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (ab.offset[mid] <= m) lo = mid;
    else hi = mid;
  }
  const int64_t b = lo, f = ab.band_first + b;
  const int64_t first = (m - ab.offset[b]) * ab.hop[b], len = ab.terms[b], step = ab.stride[b];
  auto weight = [&] { return ab.weight ? ab.weight[b] : 1.0; };
#undef CSD_WAVE_LOAD
#define CSD_WAVE_LOAD(row, on, out) csd_load_strided<T, CHECK>(row, on, s, len, step, out)
#include "qi_csd_wave.inc"
#undef CSD_WAVE_LOAD
}

// coherence[f][i][j] = |S_ij|^2 / (S_ii S_jj) of the finished matrices, the quotient in double; one segment: the identity's
// value (see include/qi_array.h) -- den / den is 1, or NaN where an auto-power is 0 or not finite
template <typename T>
__global__ void __launch_bounds__(256) k_coherence(const cplx<T>* __restrict__ S, T* __restrict__ coh, int64_t C, int64_t count,
                                                   int one_segment) {
  const int64_t at = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (at >= count) return;
  const int64_t CC = C * C, f = at / CC, ij = at - f * CC, i = ij / C, j = ij - i * C;
  const cplx<T>* __restrict__ Sf = S + f * CC;
  const cplx<T> s = Sf[ij];
  const double den = (double)Sf[i * C + i].x * (double)Sf[j * C + j].x;
  const double num = one_segment ? den : (double)s.x * (double)s.x + (double)s.y * (double)s.y;
  coh[at] = (T)(num / den);
}

// what both entry points refuse of a shape (the matrices' index arithmetic and the grid stay inside their types)
int csd_shape_check(int dtype, int64_t C, int64_t nf, int64_t nseg) {
  QI_REQUIRE(dtype == QI_F32 || dtype == QI_F64, "bad dtype %d", dtype);
  QI_REQUIRE(C > 0 && nf > 0 && nseg > 0, "bad panel shape");
  QI_REQUIRE(C < (1ll << 20) && nf < (1ll << 40) / (C * C), "cross-spectral matrices of %lld bins x %lld^2 records are too large",
             (long long)nf, (long long)C);
  const int64_t ntile = ceil_div(C, kCsdTile);
  QI_REQUIRE(ntile * (ntile + 1) / 2 * ceil_div(nf, kCsdWaves) < (1ll << 31), "request too large");  // (>= the tile groups)
  QI_REQUIRE(C * nf < (1ll << 62) / nseg / 16, "panel too large");
  return QI_OK;
}

// tiles of a tile row a wave takes: one where there is one; else what the accumulators leave room for (4 x 4 registers a
// tile, 8 in float64)
template <typename T>
int csd_tiles_per_wave(int64_t ntile) {
  return ntile == 1 ? 1 : (sizeof(T) == 8 ? 2 : 4);
}
int64_t csd_groups(int64_t ntile, int nj) {
  int64_t groups = 0;
  for (int64_t ti = 0; ti < ntile; ++ti) groups += csd_row_groups(ntile, ti, nj);
  return groups;
}

// what the windowed entry points refuse of a shape, and the number of windows
int csd_windows_check(int dtype, int64_t C, int64_t nf, int64_t nseg, int64_t bin_first, int64_t bin_count, int64_t win, int64_t hop,
                      int64_t* nwin_out) {
  QI_REQUIRE(dtype == QI_F32 || dtype == QI_F64, "bad dtype %d", dtype);
  QI_REQUIRE(C > 0 && nf > 0 && nseg > 0, "bad panel shape");
  QI_REQUIRE(win > 0 && hop > 0, "bad window: %lld segments, hop %lld", (long long)win, (long long)hop);
  QI_REQUIRE(win <= nseg, "window of %lld segments is longer than the panel's %lld", (long long)win, (long long)nseg);
  QI_REQUIRE(bin_count > 0 && bin_first >= 0 && bin_first <= nf - bin_count, "bin range %lld + %lld leaves the panel's %lld bins",
             (long long)bin_first, (long long)bin_count, (long long)nf);
  const int64_t nwin = (nseg - win) / hop + 1;
  QI_REQUIRE(C < (1ll << 20) && bin_count < (1ll << 40) / (C * C) && nwin <= (1ll << 40) / (C * C) / bin_count,
             "cross-spectral matrices of %lld windows x %lld bins x %lld^2 records are too large", (long long)nwin, (long long)bin_count,
             (long long)C);
  const int64_t ntile = ceil_div(C, kCsdTile);
  const int64_t items = ntile * (ntile + 1) / 2 * ceil_div(bin_count, kCsdWaves);  // (>= the tile groups; < 2^40)
  QI_REQUIRE(items < (1ll << 31) && nwin < (1ll << 31) / items, "request too large");
  QI_REQUIRE(C * nf < (1ll << 62) / nseg / 16, "panel too large");
  *nwin_out = nwin;
  return QI_OK;
}

// what the banded entry points refuse of a geometry (include/qi_bands.h); the offsets of the band-major stack, into
// offsets_out [band_count + 1] where there is one, and their total
int csd_bands_layout(int64_t n, int64_t band_count, const int64_t* terms, const int64_t* hop, const int64_t* stride, int64_t* offsets_out,
                     int64_t* total_out) {
  QI_REQUIRE(n > 0 && band_count > 0, "bad band geometry: %lld samples, %lld bands", (long long)n, (long long)band_count);
  QI_REQUIRE(terms && hop && stride, "null band table");
  int64_t total = 0;
  for (int64_t b = 0; b < band_count; ++b) {
    QI_REQUIRE(terms[b] >= 1 && hop[b] >= 1 && stride[b] >= 1, "bad band table: band %lld has %lld terms, hop %lld, stride %lld",
               (long long)b, (long long)terms[b], (long long)hop[b], (long long)stride[b]);
    // span = (terms - 1) stride + 1 <= n, asked without forming a product that could overflow
    QI_REQUIRE(terms[b] - 1 <= (n - 1) / stride[b], "window of band %lld (%lld terms every %lld) is longer than the panel's %lld samples",
               (long long)b, (long long)terms[b], (long long)stride[b], (long long)n);
    const int64_t nwin = (n - ((terms[b] - 1) * stride[b] + 1)) / hop[b] + 1;
    QI_REQUIRE(total <= (1ll << 62) - nwin, "cross-spectral matrices of %lld bands are too large", (long long)band_count);
    if (offsets_out) offsets_out[b] = total;
    total += nwin;
  }
  if (offsets_out) offsets_out[band_count] = total;
  *total_out = total;
  return QI_OK;
}

// what the banded entry points refuse of a shape, and the number of matrices
int csd_bands_check(int dtype, int64_t C, int64_t nb, int64_t n, int64_t band_first, int64_t band_count, const int64_t* terms,
                    const int64_t* hop, const int64_t* stride, int64_t* total_out) {
  QI_REQUIRE(dtype == QI_F32 || dtype == QI_F64, "bad dtype %d", dtype);
  QI_REQUIRE(C > 0 && nb > 0 && n > 0, "bad panel shape");
  QI_REQUIRE(band_count > 0 && band_first >= 0 && band_first <= nb - band_count, "band range %lld + %lld leaves the panel's %lld bands",
             (long long)band_first, (long long)band_count, (long long)nb);
  int64_t total = 0;
  QI_TRY(csd_bands_layout(n, band_count, terms, hop, stride, nullptr, &total));
  QI_REQUIRE(C < (1ll << 20) && total <= (1ll << 40) / (C * C), "cross-spectral matrices of %lld windows x %lld^2 records are too large",
             (long long)total, (long long)C);
  const int64_t ntile = ceil_div(C, kCsdTile);
  const int64_t items = ntile * (ntile + 1) / 2;  // (>= the tile groups; < 2^40)
  QI_REQUIRE(items < (1ll << 31) && ceil_div(total, kCsdWaves) < (1ll << 31) / items, "request too large");
  QI_REQUIRE(C * nb < (1ll << 62) / n / 16, "panel too large");
  *total_out = total;
  return QI_OK;
}

// words of the device tables: offset [band_count + 1] | terms | hop | stride | weight, band_count each
size_t csd_bands_words(int64_t band_count) { return 5 * (size_t)band_count + 1; }
size_t cross_spectra_bands_scratch(int dtype, int64_t C, int64_t band_count, int64_t total) {
  return align_up(csd_bands_words(band_count) * 8) + align_up((size_t)total * C * C * 2 * elem_size(dtype));
}

// `tables`: the device tables in csd_bands_words' order (has_weight: the last of them is filled); terms: the HOST table,
// for the coherence's one-term rule; `matrices`: the second region of the scratch
template <typename T>
int launch_cross_spectra_bands(const cplx<T>* Z, int64_t C, int64_t nb, int64_t n, int64_t band_first, int64_t band_count, int64_t total,
                               const int64_t* tables, bool has_weight, const int64_t* terms, const int64_t* offsets, cplx<T>* csd,
                               T* coherence, void* matrices, hipStream_t st) {
  CsdBandArgs a{};
  a.p.C = C;
  a.p.nf = nb;
  a.p.nseg = n;
  a.p.ntile = ceil_div(C, kCsdTile);
  a.p.nfb = ceil_div(total, kCsdWaves);
  a.band_first = band_first;
  a.band_count = band_count;
  a.total = total;
  a.offset = tables;
  a.terms = a.offset + band_count + 1;
  a.hop = a.terms + band_count;
  a.stride = a.hop + band_count;
  a.weight = has_weight ? reinterpret_cast<const double*>(a.stride + band_count) : nullptr;
  cplx<T>* S = csd ? csd : static_cast<cplx<T>*>(matrices);
  const int nj = a.p.ntile == 1 ? 1 : 2;  // (see csd_band_waves)
  const dim3 grid((unsigned)(csd_groups(a.p.ntile, nj) * a.p.nfb));
  if (nj == 1) k_cross_spectra_bands<T, 1><<<grid, kCsdWaves * kWave, 0, st>>>(Z, S, a);
  else k_cross_spectra_bands<T, 2><<<grid, kCsdWaves * kWave, 0, st>>>(Z, S, a);
  QI_LAUNCH_CHECK();
  if (!coherence) return QI_OK;
  // k_coherence's one-segment rule goes by the launch: one launch per run of bands on the same side of terms == 1 (one in
  // all, unless bands of a single term are mixed with longer ones)
  const int64_t CC = C * C;
  for (int64_t b0 = 0; b0 < band_count;) {
    int64_t b1 = b0 + 1;
    while (b1 < band_count && (terms[b1] == 1) == (terms[b0] == 1)) ++b1;
    const int64_t count = (offsets[b1] - offsets[b0]) * CC;
    k_coherence<T><<<dim3((unsigned)ceil_div(count, 256)), 256, 0, st>>>(S + offsets[b0] * CC, coherence + offsets[b0] * CC, C, count,
                                                                         terms[b0] == 1);
    QI_LAUNCH_CHECK();
    b0 = b1;
  }
  return QI_OK;
}

}  // namespace

namespace qi {

size_t cross_spectra_scratch(int dtype, int64_t C, int64_t nf) {
  return align_up((size_t)nf * 8) + align_up((size_t)nf * C * C * 2 * elem_size(dtype));
}

template <typename T>
int launch_cross_spectra(const cplx<T>* Z, int64_t C, int64_t nf, int64_t nseg, const CsdWeight& w, cplx<T>* csd, T* coherence,
                         void* matrices, hipStream_t st) {
  CsdArgs a{};
  a.C = C;
  a.nf = nf;
  a.nseg = nseg;
  a.ntile = ceil_div(C, kCsdTile);
  a.nfb = ceil_div(nf, kCsdWaves);
  a.w = w;
  cplx<T>* S = csd ? csd : static_cast<cplx<T>*>(matrices);
  const int nj = csd_tiles_per_wave<T>(a.ntile);
  const dim3 grid((unsigned)(csd_groups(a.ntile, nj) * a.nfb));
  if (nj == 1) k_cross_spectra<T, 1><<<grid, kCsdWaves * kWave, 0, st>>>(Z, S, a);
  else if (nj == 2) k_cross_spectra<T, 2><<<grid, kCsdWaves * kWave, 0, st>>>(Z, S, a);
  else k_cross_spectra<T, 4><<<grid, kCsdWaves * kWave, 0, st>>>(Z, S, a);
  QI_LAUNCH_CHECK();
  if (!coherence) return QI_OK;
  const int64_t count = nf * C * C;
  k_coherence<T><<<dim3((unsigned)ceil_div(count, 256)), 256, 0, st>>>(S, coherence, C, count, nseg == 1);
  QI_LAUNCH_CHECK();
  return QI_OK;
}
template int launch_cross_spectra<float>(const float2*, int64_t, int64_t, int64_t, const CsdWeight&, float2*, float*, void*, hipStream_t);
template int launch_cross_spectra<double>(const double2*, int64_t, int64_t, int64_t, const CsdWeight&, double2*, double*, void*,
                                          hipStream_t);

size_t cross_spectra_windows_scratch(int dtype, int64_t C, int64_t bin_count, int64_t nwin) {
  return align_up((size_t)bin_count * 8) + align_up((size_t)nwin * bin_count * C * C * 2 * elem_size(dtype));
}

template <typename T>
int launch_cross_spectra_windows(const cplx<T>* Z, int64_t C, int64_t nf, int64_t nseg, int64_t bin_first, int64_t bin_count, int64_t win,
                                 int64_t hop, const CsdWeight& w, cplx<T>* csd, T* coherence, void* matrices, hipStream_t st) {
  CsdWindowArgs a{};
  a.p.C = C;
  a.p.nf = nf;
  a.p.nseg = nseg;
  a.p.ntile = ceil_div(C, kCsdTile);
  a.p.nfb = ceil_div(bin_count, kCsdWaves);
  a.p.w = w;
  a.bin_first = bin_first;
  a.bin_count = bin_count;
  a.win = win;
  a.hop = hop;
  a.nwin = (nseg - win) / hop + 1;
  cplx<T>* S = csd ? csd : static_cast<cplx<T>*>(matrices);
  const int nj = csd_tiles_per_wave<T>(a.p.ntile);
  const dim3 grid((unsigned)(csd_groups(a.p.ntile, nj) * a.p.nfb * a.nwin));
  if (nj == 1) k_cross_spectra_windows<T, 1><<<grid, kCsdWaves * kWave, 0, st>>>(Z, S, a);
  else if (nj == 2) k_cross_spectra_windows<T, 2><<<grid, kCsdWaves * kWave, 0, st>>>(Z, S, a);
  else k_cross_spectra_windows<T, 4><<<grid, kCsdWaves * kWave, 0, st>>>(Z, S, a);
  QI_LAUNCH_CHECK();
  if (!coherence) return QI_OK;
  const int64_t count = a.nwin * bin_count * C * C;
  k_coherence<T><<<dim3((unsigned)ceil_div(count, 256)), 256, 0, st>>>(S, coherence, C, count, win == 1);
  QI_LAUNCH_CHECK();
  return QI_OK;
}
template int launch_cross_spectra_windows<float>(const float2*, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t,
                                                 const CsdWeight&, float2*, float*, void*, hipStream_t);
template int launch_cross_spectra_windows<double>(const double2*, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t,
                                                  const CsdWeight&, double2*, double*, void*, hipStream_t);

}  // namespace qi

extern "C" {

int64_t qi_cross_spectra_scratch_bytes(int dtype, int64_t C, int64_t nf, int64_t nseg) {
  QI_TRY(csd_shape_check(dtype, C, nf, nseg));
  return (int64_t)cross_spectra_scratch(dtype, C, nf);
}

int qi_cross_spectra(int dtype, int device, const void* Z, int64_t C, int64_t nf, int64_t nseg, const double* weight, void* csd,
                     void* coherence, void* scratch, int64_t scratch_bytes, qi_stream stream) {
  QI_REQUIRE(Z && scratch, "null argument");
  QI_REQUIRE(csd || coherence, "nothing to produce");
  QI_TRY(csd_shape_check(dtype, C, nf, nseg));
  QI_TRY(require_scratch(scratch_bytes, (int64_t)cross_spectra_scratch(dtype, C, nf)));
  QI_REQUIRE(aligned(Z, 2 * elem_size(dtype)) && aligned(csd, 2 * elem_size(dtype)) && aligned(coherence, elem_size(dtype)) &&
                 aligned(scratch, 16),
             "misaligned pointer");
  DeviceGuard g(device);
  hipStream_t st = (hipStream_t)stream;
  CsdWeight w;
  if (weight) {
    // the host array rides in kernel arguments: stream-ordered, and the caller's array is free at return
    double* table = static_cast<double*>(scratch);
    QI_TRY(qi::host::put_words(table, weight, nf, st));
    w.table = table;
  }
  void* matrices = static_cast<char*>(scratch) + align_up((size_t)nf * 8);
  return by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    return launch_cross_spectra<T>((const cplx<T>*)Z, C, nf, nseg, w, (cplx<T>*)csd, (T*)coherence, matrices, st);
  });
}

int64_t qi_cross_spectra_windows_scratch_bytes(int dtype, int64_t C, int64_t nf, int64_t nseg, int64_t bin_first, int64_t bin_count,
                                               int64_t win, int64_t hop) {
  int64_t nwin = 0;
  QI_TRY(csd_windows_check(dtype, C, nf, nseg, bin_first, bin_count, win, hop, &nwin));
  return (int64_t)cross_spectra_windows_scratch(dtype, C, bin_count, nwin);
}

int qi_cross_spectra_windows(int dtype, int device, const void* Z, int64_t C, int64_t nf, int64_t nseg, int64_t bin_first,
                             int64_t bin_count, int64_t win, int64_t hop, const double* weight, void* csd, void* coherence,
                             void* scratch, int64_t scratch_bytes, qi_stream stream) {
  QI_REQUIRE(Z && scratch, "null argument");
  QI_REQUIRE(csd || coherence, "nothing to produce");
  int64_t nwin = 0;
  QI_TRY(csd_windows_check(dtype, C, nf, nseg, bin_first, bin_count, win, hop, &nwin));
  QI_TRY(require_scratch(scratch_bytes, (int64_t)cross_spectra_windows_scratch(dtype, C, bin_count, nwin)));
  QI_REQUIRE(aligned(Z, 2 * elem_size(dtype)) && aligned(csd, 2 * elem_size(dtype)) && aligned(coherence, elem_size(dtype)) &&
                 aligned(scratch, 16),
             "misaligned pointer");
  DeviceGuard g(device);
  hipStream_t st = (hipStream_t)stream;
  CsdWeight w;
  if (weight) {
    // one weight per formed bin; as qi_cross_spectra's, the host array rides in kernel arguments
    double* table = static_cast<double*>(scratch);
    QI_TRY(qi::host::put_words(table, weight, bin_count, st));
    w.table = table;
  }
  void* matrices = static_cast<char*>(scratch) + align_up((size_t)bin_count * 8);
  return by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    return launch_cross_spectra_windows<T>((const cplx<T>*)Z, C, nf, nseg, bin_first, bin_count, win, hop, w, (cplx<T>*)csd,
                                           (T*)coherence, matrices, st);
  });
}

int64_t qi_cross_spectra_bands_layout(int64_t n, int64_t band_count, const int64_t* terms, const int64_t* hop, const int64_t* stride,
                                      int64_t* offsets_out) {
  int64_t total = 0;
  QI_TRY(csd_bands_layout(n, band_count, terms, hop, stride, offsets_out, &total));
  return total;
}

int64_t qi_cross_spectra_bands_scratch_bytes(int dtype, int64_t C, int64_t nb, int64_t n, int64_t band_first, int64_t band_count,
                                             const int64_t* terms, const int64_t* hop, const int64_t* stride) {
  int64_t total = 0;
  QI_TRY(csd_bands_check(dtype, C, nb, n, band_first, band_count, terms, hop, stride, &total));
  return (int64_t)cross_spectra_bands_scratch(dtype, C, band_count, total);
}

int qi_cross_spectra_bands(int dtype, int device, const void* Z, int64_t C, int64_t nb, int64_t n, int64_t band_first,
                           int64_t band_count, const int64_t* terms, const int64_t* hop, const int64_t* stride, const double* weight,
                           void* csd, void* coherence, void* scratch, int64_t scratch_bytes, qi_stream stream) {
  QI_REQUIRE(Z && scratch, "null argument");
  QI_REQUIRE(csd || coherence, "nothing to produce");
  int64_t total = 0;
  QI_TRY(csd_bands_check(dtype, C, nb, n, band_first, band_count, terms, hop, stride, &total));
  QI_TRY(require_scratch(scratch_bytes, (int64_t)cross_spectra_bands_scratch(dtype, C, band_count, total)));
  QI_REQUIRE(aligned(Z, 2 * elem_size(dtype)) && aligned(csd, 2 * elem_size(dtype)) && aligned(coherence, elem_size(dtype)) &&
                 aligned(scratch, 16),
             "misaligned pointer");
  // the device tables, assembled on the host: offset | terms | hop | stride | weight.  As qi_cross_spectra_windows' weights
  // they ride in kernel arguments: stream-ordered, and the caller's arrays are free at return
  const size_t bc = (size_t)band_count;
  std::vector<int64_t> words(csd_bands_words(band_count));
  QI_TRY(csd_bands_layout(n, band_count, terms, hop, stride, words.data(), &total));
  std::memcpy(words.data() + bc + 1, terms, bc * 8);
  std::memcpy(words.data() + 2 * bc + 1, hop, bc * 8);
  std::memcpy(words.data() + 3 * bc + 1, stride, bc * 8);
  if (weight) std::memcpy(words.data() + 4 * bc + 1, weight, bc * 8);
  DeviceGuard g(device);
  hipStream_t st = (hipStream_t)stream;
  QI_TRY(qi::host::put_words(scratch, words.data(), (int64_t)(weight ? words.size() : words.size() - bc), st));
  void* matrices = static_cast<char*>(scratch) + align_up(csd_bands_words(band_count) * 8);
  return by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    return launch_cross_spectra_bands<T>((const cplx<T>*)Z, C, nb, n, band_first, band_count, total, static_cast<const int64_t*>(scratch),
                                         weight != nullptr, terms, words.data(), (cplx<T>*)csd, (T*)coherence, matrices, st);
  });
}

}  // extern "C"
