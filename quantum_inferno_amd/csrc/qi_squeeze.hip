// Synchrosqueezing of a constant-Q panel (include/qi_squeeze.h): the instantaneous frequency of every coefficient from the
// forward phase difference along time, and the reassignment of the coefficients to frequency bins.
//
// k_squeeze: a lane owns a column.  A workgroup of kSqTile = 256 threads takes one record and 256 consecutive times; lane t
// clears its column of `out`, then walks the bands in ascending order and adds weight[b] Z[c][b][t] into the place of the bin
// the element lands in -- in `out` itself, through L2.  Nobody but the lane ever touches its column, so program order is all
// the ordering there is to keep and the order of the additions is the band order by construction: no atomic, no barrier
// inside the walk.  A lane keeps the sum of the bin it is in in registers while consecutive bands land there; a run starts
// from what `out` holds, so it adds to the earlier bands' sum term by term as the header says, and ends with one store.  The
// lanes of a wave touch 64 consecutive elements of a row each, whatever bin each targets.  One walk, whatever the bin count.
// The other home for the sums -- rows of LDS, [bins of a chunk][tile], streamed out after a walk per chunk -- was built and
// measured first and lost at every bin count, one chunk included (profiles/squeeze_homes_ab.txt).  The edges
// are staged in LDS once per workgroup; a search first asks the bin of the band before.
//
// FUSED (qi_tfr_synchrosqueeze): the frequency comes from sq_ifreq on the lane's coefficient and its neighbour's, which
// arrives by a move across the lanes of the wave; the wave's last lane and the record's last column load theirs.  Otherwise
// (qi_tfr_squeeze) it is read from the caller's array.  k_ifreq (qi_tfr_ifreq) stores what sq_ifreq gives, a thread per
// element.  sq_ifreq and sq_bin are the only places where a frequency or a bin is formed: the fused call equals the
// composition bit for bit.  The file is compiled without contraction: every product and sum is rounded on its own.

#include "qi_common.hpp"
#include "qi_device.hpp"
#include "qi_fft_reg.hpp"  // QI_LAUNCH_CHECK
#include "qi_squeeze.h"

namespace qi {

namespace {

constexpr int kSqTile = 256;
static_assert(kSqTile == QI_SQUEEZE_TILE && kSqTile % kWave == 0, "the header names the kernel's sizes");
template <typename T>
struct SqArgs {
  int64_t nb, n, nbin, ntile;
  const T* edges;    // [nbin + 1]  (device tables, in the caller's scratch)
  const T* carrier;  // [nb]
  const T* weight;   // [nb]
  T rate, floor;
};

__device__ __forceinline__ float sq_atan2(float y, float x) { return atan2f(y, x); }
__device__ __forceinline__ double sq_atan2(double y, double x) { return atan2(y, x); }

// The frequency of one element: z the coefficient of column t, p its partner's (column t + 1, or n - 2 for the last column:
// `last`, the roles swapped).  NaN for an element that is not valid.
template <typename T>
__device__ __forceinline__ T sq_ifreq(cplx<T> z, cplx<T> p, bool last, T carrier, T rate, T floor) {
  const T pz = z.x * z.x + z.y * z.y, pp = p.x * p.x + p.y * p.y;
  const T inf = (T)__builtin_huge_val();
  if (!(pz >= floor && pz < inf && pp >= floor && pp < inf)) return (T)__builtin_nan("");
  const cplx<T> l = last ? z : p, e = last ? p : z;
  const T dr = l.x * e.x + l.y * e.y, di = l.y * e.x - l.x * e.y;
  return carrier + (rate * sq_atan2(di, dr)) * (T)0.15915494309189533577;
}

// (number of edges <= f) - 1 where that is a bin, else -1: NaN, the infinities, below the first edge, at or above the last.
// `hint`: a bin to ask first (the bin of the band before), or -1.
template <typename T>
__device__ __forceinline__ int sq_bin(const T* __restrict__ e, int nbin, T f, int hint) {
  if (!(f >= e[0] && f < e[nbin])) return -1;
  if (hint >= 0 && e[hint] <= f && f < e[hint + 1]) return hint;
  int lo = 0, hi = nbin;  // e[lo] <= f < e[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (e[mid] <= f) lo = mid;
    else hi = mid;
  }
  return lo;
}

// the partner's coefficient of every lane: the neighbour's by a move across the wave (every lane of the wave must be here),
// a load for the wave's last lane and for the record's last column.  `row`: the band's row of the record; z: zero for t >= n.
template <typename T>
__device__ __forceinline__ cplx<T> sq_partner(const cplx<T>* __restrict__ row, cplx<T> z, int64_t t, int64_t n, int lane) {
  cplx<T> p;
  p.x = __shfl_down(z.x, 1);
  p.y = __shfl_down(z.y, 1);
  if (t < n && (lane == kWave - 1 || t == n - 1)) p = row[t + 1 < n ? t + 1 : n - 2];
  return p;
}

template <typename T>
__global__ void __launch_bounds__(kSqTile) k_ifreq(const cplx<T>* __restrict__ Z, T* __restrict__ ifreq, SqArgs<T> a) {
  const int64_t rowi = (int64_t)blockIdx.x / a.ntile, tile = (int64_t)blockIdx.x % a.ntile;  // rowi = c nb + b
  const int64_t t = tile * kSqTile + threadIdx.x;
  const int lane = threadIdx.x & (kWave - 1);
  const cplx<T>* __restrict__ row = Z + (size_t)rowi * (size_t)a.n;
  const bool active = t < a.n;
  const cplx<T> z = active ? row[t] : mk<T>(0, 0);
  const cplx<T> p = sq_partner<T>(row, z, t, a.n, lane);
  if (active) ifreq[(size_t)rowi * (size_t)a.n + (size_t)t] = sq_ifreq<T>(z, p, t == a.n - 1, a.carrier[rowi % a.nb], a.rate, a.floor);
}

template <typename T, bool FUSED>
__global__ void __launch_bounds__(kSqTile) k_squeeze(const cplx<T>* __restrict__ Z, const T* __restrict__ ifreq,
                                                     cplx<T>* __restrict__ out, SqArgs<T> a) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  T* __restrict__ s_edges = reinterpret_cast<T*>(lds_raw);
  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  const int64_t c = (int64_t)blockIdx.x / a.ntile, tile = (int64_t)blockIdx.x % a.ntile;
  const int64_t t = tile * kSqTile + tid;
  const bool active = t < a.n, last = t == a.n - 1;
  const int nbin = (int)a.nbin;
  for (int i = tid; i <= nbin; i += kSqTile) s_edges[i] = a.edges[i];
  __syncthreads();

  const cplx<T>* __restrict__ rec = Z + (size_t)c * (size_t)a.nb * (size_t)a.n;
  const T* __restrict__ frec = FUSED ? nullptr : ifreq + (size_t)c * (size_t)a.nb * (size_t)a.n;
  // the lane's column of the result: bin k at mine[k * n]  (a lane past the record's end never follows it)
  cplx<T>* __restrict__ mine = out + (size_t)c * (size_t)a.nbin * (size_t)a.n + (size_t)(active ? t : 0);
  const size_t pitch = (size_t)a.n;
  if (active)
    for (int k = 0; k < nbin; ++k) mine[(size_t)k * pitch] = mk<T>(0, 0);

  int cur = -1, hint = -1;  // the bin held in `acc`; the bin of the band before
  cplx<T> acc = mk<T>(0, 0);
  cplx<T> z_next = active ? rec[t] : mk<T>(0, 0);
  T f_next = T(0);
  if constexpr (!FUSED) f_next = active ? frec[t] : (T)__builtin_nan("");
  for (int64_t b = 0; b < a.nb; ++b) {  // (uniform: the lanes past the record's end walk along, for the moves across the wave)
    const cplx<T>* __restrict__ row = rec + (size_t)b * (size_t)a.n;
    const cplx<T> z = z_next;
    T f = f_next;
    if (b + 1 < a.nb) {  // the next band's loads, in flight over this band's arithmetic
      z_next = active ? row[(size_t)a.n + (size_t)t] : mk<T>(0, 0);
      if constexpr (!FUSED) f_next = active ? frec[(size_t)(b + 1) * (size_t)a.n + (size_t)t] : (T)__builtin_nan("");
    }
    if constexpr (FUSED) {
      const cplx<T> p = sq_partner<T>(row, z, t, a.n, lane);
      f = active ? sq_ifreq<T>(z, p, last, a.carrier[b], a.rate, a.floor) : (T)__builtin_nan("");
    }
    const int k = sq_bin<T>(s_edges, nbin, f, hint);  // (-1 for a lane past the record's end: its frequency is NaN)
    if (k >= 0) {
      hint = k;
      if (k != cur) {
        if (cur >= 0) mine[(size_t)cur * pitch] = acc;
        acc = mine[(size_t)k * pitch];
        cur = k;
      }
      const T w = a.weight[b];
      const T pr = w * z.x, pi = w * z.y;  // (rounded, then added: the file is compiled without contraction)
      acc.x = acc.x + pr;
      acc.y = acc.y + pi;
    }
  }
  if (cur >= 0) mine[(size_t)cur * pitch] = acc;
}

template <typename T>
SqArgs<T> sq_args(int64_t nb, int64_t n, int64_t nbin, const SqueezeTables& tb, double rate, double floor) {
  SqArgs<T> a{};
  a.nb = nb;
  a.n = n;
  a.nbin = nbin;
  a.ntile = ceil_div(n, kSqTile);
  a.edges = reinterpret_cast<const T*>(static_cast<const char*>(tb.base) + tb.edges);
  a.carrier = reinterpret_cast<const T*>(static_cast<const char*>(tb.base) + tb.carrier);
  a.weight = reinterpret_cast<const T*>(static_cast<const char*>(tb.base) + tb.weight);
  a.rate = (T)rate;
  a.floor = (T)floor;
  return a;
}

}  // namespace

int64_t squeeze_tiles(int64_t n) { return ceil_div(n, kSqTile); }

template <typename T>
int launch_tfr_ifreq(const cplx<T>* Z, int64_t C, int64_t nb, int64_t n, const SqueezeTables& tb, double rate, double floor, T* ifreq,
                     hipStream_t st) {
  const SqArgs<T> a = sq_args<T>(nb, n, 1, tb, rate, floor);
  k_ifreq<T><<<dim3((unsigned)(C * nb * a.ntile)), kSqTile, 0, st>>>(Z, ifreq, a);
  QI_LAUNCH_CHECK();
  return QI_OK;
}

template <typename T>
int launch_tfr_squeeze(const cplx<T>* Z, const T* ifreq, int64_t C, int64_t nb, int64_t n, int64_t nbin, const SqueezeTables& tb,
                       double rate, double floor, cplx<T>* out, hipStream_t st) {
  const SqArgs<T> a = sq_args<T>(nb, n, nbin, tb, rate, floor);
  const size_t lds = (size_t)(nbin + 1) * sizeof(T);  // the edges: 32 KiB at most (QI_SQUEEZE_MAX_BINS)
  const dim3 grid((unsigned)(C * a.ntile));
  if (ifreq) k_squeeze<T, false><<<grid, kSqTile, lds, st>>>(Z, ifreq, out, a);
  else k_squeeze<T, true><<<grid, kSqTile, lds, st>>>(Z, ifreq, out, a);
  QI_LAUNCH_CHECK();
  return QI_OK;
}

template int launch_tfr_ifreq<float>(const float2*, int64_t, int64_t, int64_t, const SqueezeTables&, double, double, float*, hipStream_t);
template int launch_tfr_ifreq<double>(const double2*, int64_t, int64_t, int64_t, const SqueezeTables&, double, double, double*,
                                      hipStream_t);
template int launch_tfr_squeeze<float>(const float2*, const float*, int64_t, int64_t, int64_t, int64_t, const SqueezeTables&, double,
                                       double, float2*, hipStream_t);
template int launch_tfr_squeeze<double>(const double2*, const double*, int64_t, int64_t, int64_t, int64_t, const SqueezeTables&, double,
                                        double, double2*, hipStream_t);

}  // namespace qi
