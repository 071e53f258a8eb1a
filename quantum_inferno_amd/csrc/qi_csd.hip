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
#include "qi_host.hpp"
#include "qi_device.hpp"   // kWave
#include "qi_fft_reg.hpp"  // QI_LAUNCH_CHECK
#include "qi_mfma.hpp"     // Mx
#include "qi_array.h"

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

// groups of up to `nj` tiles in row ti of the upper triangle of a matrix of `ntile` tiles a side
__host__ __device__ inline int64_t csd_row_groups(int64_t ntile, int64_t ti, int nj) { return (ntile - ti + nj - 1) / nj; }

// NJ: tiles of one tile row a wave takes -- they share the A operand's loads; a matter of registers and traffic, not of results
template <typename T, int NJ>
__global__ void __launch_bounds__(kCsdWaves* kWave) k_cross_spectra(const cplx<T>* __restrict__ Z, cplx<T>* __restrict__ S, CsdArgs a) {
  using M = Mx<T>;
  using acc = typename M::acc;
  constexpr int V = M::V, STEP = 4 * V;  // segments of one iteration
  const int lane = threadIdx.x & (kWave - 1);
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int64_t f = ((int64_t)blockIdx.x % a.nfb) * kCsdWaves + wv;
  if (f >= a.nf) return;  // (the whole wave)
  // item -> tile row ti and its group of up to NJ tiles tj0 .. tj0 + nj - 1, tj0 >= ti: the groups row by row of the upper triangle
  int64_t p = (int64_t)blockIdx.x / a.nfb, ti = 0;
  while (p >= csd_row_groups(a.ntile, ti, NJ)) {
    p -= csd_row_groups(a.ntile, ti, NJ);
    ++ti;
  }
  const int64_t tj0 = ti + p * NJ;
  const int nj = (int)(a.ntile - tj0 < NJ ? a.ntile - tj0 : NJ);
  const bool diag0 = tj0 == ti;  // the group's first tile lies on the diagonal: its B operand is the A operand
  const int r = lane & 15, g = lane >> 4;
  // (a record past C: the pointer stays inside the panel, the operand is zero)
  const int64_t ci = ti * kCsdTile + r;
  const bool oni = ci < a.C;
  const cplx<T>* __restrict__ zi = Z + ((oni ? ci : 0) * a.nf + f) * a.nseg;
  const cplx<T>* zj[NJ];
  bool onj[NJ];
#pragma unroll
  for (int q = 0; q < NJ; ++q) {
    const int64_t cj = (tj0 + q) * kCsdTile + r;
    onj[q] = q < nj && cj < a.C;
    zj[q] = Z + ((onj[q] ? cj : 0) * a.nf + f) * a.nseg;
  }
  acc rr[NJ], ii[NJ], ri[NJ], ir[NJ];
#pragma unroll
  for (int q = 0; q < NJ; ++q) rr[q] = ii[q] = ri[q] = ir[q] = acc{0, 0, 0, 0};
  // one iteration's operands: V segments from `s` of the A record and of the B record of every tile of the group
  auto load = [&](auto check, int64_t s, cplx<T>* x, cplx<T>(*y)[V]) {
    constexpr bool CHECK = decltype(check)::value;
    csd_load<T, CHECK>(zi, oni, s, a.nseg, x);
#pragma unroll
    for (int q = 0; q < NJ; ++q) {
      if (q >= nj) break;
      if (q > 0 || !diag0) csd_load<T, CHECK>(zj[q], onj[q], s, a.nseg, y[q]);
    }
  };
  auto tile_steps = [&](int q, const cplx<T>* x, const cplx<T>* y) {
#pragma unroll
    for (int v = 0; v < V; ++v) {
      rr[q] = M::mac(x[v].x, y[v].x, rr[q]);
      ii[q] = M::mac(x[v].y, y[v].y, ii[q]);
      ri[q] = M::mac(x[v].x, y[v].y, ri[q]);
      ir[q] = M::mac(x[v].y, y[v].x, ir[q]);
    }
  };
  auto steps = [&](const cplx<T>* x, const cplx<T>(*y)[V]) {
    if (diag0) tile_steps(0, x, x);  // the diagonal tile: the A operand's registers twice
    else tile_steps(0, x, y[0]);
#pragma unroll
    for (int q = 1; q < NJ; ++q) {
      if (q >= nj) break;
      tile_steps(q, x, y[q]);
    }
  };
  const int64_t full = a.nseg / STEP * STEP, s_lane = g * V;
  cplx<T> xa[V], ya[NJ][V], xb[V], yb[NJ][V];
  int64_t s0 = 0;
  // two iterations' loads are in flight before the first one's products: a wave alone on its SIMD (few records) is bound
  // by the latency of its loads
  for (; s0 + 2 * STEP <= full; s0 += 2 * STEP) {
    load(std::false_type{}, s0 + s_lane, xa, ya);
    load(std::false_type{}, s0 + STEP + s_lane, xb, yb);
    steps(xa, ya);
    steps(xb, yb);
  }
  if (s0 < full) {
    load(std::false_type{}, s0 + s_lane, xa, ya);
    steps(xa, ya);
    s0 += STEP;
  }
  if (s0 < a.nseg) {
    load(std::true_type{}, s0 + s_lane, xa, ya);
    steps(xa, ya);
  }
  const T w = (T)csd_weight(a.w, f, a.nf);
  cplx<T>* __restrict__ Sf = S + f * a.C * a.C;
#pragma unroll
  for (int q = 0; q < NJ; ++q) {
    if (q >= nj) break;
    const bool diag = q == 0 && diag0;
    const int64_t j = (tj0 + q) * kCsdTile + (lane & 15);
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int64_t i = ti * kCsdTile + M::row(lane, reg);
      if (i >= a.C || j >= a.C || (diag && j < i)) continue;
      const T re = (rr[q][reg] + ii[q][reg]) * w;
      const T im = i == j ? T(0) : (ri[q][reg] - ir[q][reg]) * w;
      Sf[i * a.C + j] = mk<T>(re, im);
      if (i != j) Sf[j * a.C + i] = mk<T>(re, -im);
    }
  }
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
  // tiles a wave takes: one where there is one; else what the accumulators leave room for (4 x 4 registers a tile, 8 in float64)
  const int nj = a.ntile == 1 ? 1 : (sizeof(T) == 8 ? 2 : 4);
  int64_t groups = 0;
  for (int64_t ti = 0; ti < a.ntile; ++ti) groups += csd_row_groups(a.ntile, ti, nj);
  const dim3 grid((unsigned)(groups * a.nfb));
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

}  // extern "C"
