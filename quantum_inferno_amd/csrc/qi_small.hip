// Small-record engine: records of 2^10 .. 2^13 samples, whose whole transform (L = 2n points for the zero-padded styx
// correlation, L = n for the atoms bank and the Stockwell transform) fits the LDS of one CU.  No decomposition of the time
// axis: one workgroup of L / 16 threads (16 values per thread) forms a band's spectrum product, transforms it back through
// LDS and finishes the band -- panel rows, power, every reduction -- from registers.
//
// The transform is a self-sorting (Stockham) decimation in frequency: L = 16 x 16 [x 16] x R, R in {1, 2, 4, 8}.  A thread
// enters every pass with v[r] = x[tid + r L / 16] (a coalesced read of global memory or of the exchange image), and pass
// i (stride s = 16^i) sends output k of thread tid = q + s p to element q + s (16 p + k) after the twiddle W_L^(s p k).
// The last pass needs neither twiddles nor an exchange: its outputs ARE v[r] = y[tid + r L / 16], natural order.
// Exchange image: element i sits at i ^ ((i >> 4) & 15) -- a permutation inside every aligned run of 16, so the image takes
// exactly L elements, and every lane group of the passes' stores (16 lanes of a ds_write_b64, 8 of a ds_write_b128: element
// stride 16, 16 and 1 in passes 0, 1, 2) and loads (32 consecutive elements per ds_read_b64 group, 16 per ds_read_b128
// group) touches pairwise different bank groups.
// Twiddles: the plan's table exp(2 pi i k / Lt), k < Lt / 16, built in float64 and rounded once; a pass loads W_L^(s p)
// and forms its fifteen powers by products (mul_powers16).  No sincos on the device.
#include "qi_device.hpp"
#include "qi_fft_reg.hpp"
#include "qi_native.hpp"

namespace qi {
namespace native {
namespace {

__device__ __forceinline__ int small_pos(int i) { return i ^ ((i >> 4) & 15); }

template <typename T>
__device__ __forceinline__ cplx<T> conj_if(cplx<T> v, bool c) {
  return mk<T>(v.x, c ? -v.y : v.y);
}

// The radix-16 passes I, I + 1, ... of the L-point transform, then the last pass of radix R = L / 16^passes.
// GUARD: the workgroup has more than L / 16 threads (k_small_fwd's shorter transform); the others only keep the barriers.
template <typename T, int LOG2L, int DIR, bool GUARD, int I>
__device__ __forceinline__ void small_passes(cplx<T> (&v)[16], cplx<T>* __restrict__ buf, const cplx<T>* __restrict__ tw,
                                             int tw_shift, int tid, bool active) {
  constexpr int L = 1 << LOG2L, NT = L / 16, NP16 = LOG2L / 4, RL = 1 << (LOG2L - 4 * NP16);
  if constexpr (I < NP16) {
    constexpr int s = 1 << (4 * I);
    fft_reg<T, 16, DIR>(v);  // v[brev(k)] = output k
    if constexpr (RL == 1 && I == NP16 - 1) {
      cplx<T> t[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) t[k] = v[brev(k, 4)];
#pragma unroll
      for (int k = 0; k < 16; ++k) v[k] = t[k];
    } else {
      const int e = tid & ~(s - 1);  // s p
      const bool live = !GUARD || active;
      const cplx<T> w = tw[live ? (e << tw_shift) : 0];
      mul_powers16<T>(v, conj_if<T>(w, DIR < 0));
      const int base = (tid & (s - 1)) + 16 * e;
      __syncthreads();  // the readers of the previous image are done
      if (live) {
#pragma unroll
        for (int k = 0; k < 16; ++k) buf[small_pos(base + s * k)] = v[brev(k, 4)];
      }
      __syncthreads();
      if (live) {
#pragma unroll
        for (int r = 0; r < 16; ++r) v[r] = buf[small_pos(tid + r * NT)];
      }
      small_passes<T, LOG2L, DIR, GUARD, I + 1>(v, buf, tw, tw_shift, tid, active);
    }
  } else if constexpr (RL > 1) {
    constexpr int G = 16 / RL;  // butterflies of a thread: butterfly g takes v[g + G m], m < RL, and leaves output k in v[g + G k]
#pragma unroll
    for (int g = 0; g < G; ++g) {
      cplx<T> t[RL];
#pragma unroll
      for (int m = 0; m < RL; ++m) t[m] = v[g + G * m];
      fft_reg<T, RL, DIR>(t);
#pragma unroll
      for (int k = 0; k < RL; ++k) v[g + G * k] = t[brev(k, ilog2(RL))];
    }
  }
}

// L-point transform of the workgroup's array: entry v[r] = x[tid + r L / 16], exit v[r] = y[tid + r L / 16],
// y[q] = sum_k x[k] exp(DIR 2 pi i k q / L).  `tw`: exp(2 pi i k / (L << tw_shift)).
template <typename T, int LOG2L, int DIR, bool GUARD = false>
__device__ __forceinline__ void small_fft(cplx<T> (&v)[16], cplx<T>* __restrict__ buf, const cplx<T>* __restrict__ tw,
                                          int tw_shift, int tid, bool active = true) {
  small_passes<T, LOG2L, DIR, GUARD, 0>(v, buf, tw, tw_shift, tid, active);
}

// ---- forward transform: one workgroup per (record, spectrum) ----------------------------------------------------------
template <typename T>
struct SmallFwdArgs {
  const T* sig;          // [ct][n]
  cplx<T>* X[2];         // role 0: [ct][2^LOG2L] spectra, role 1: [ct][2^(LOG2L - 1)]
  const cplx<T>* tw;
  int32_t tw_log2;       // log2 of the twiddle table's period
  int32_t n;
  int32_t role0;         // role of blockIdx.y = 0
};

template <typename T, int LG, bool GUARD>
__device__ __forceinline__ void small_forward_record(const SmallFwdArgs<T>& a, cplx<T>* __restrict__ X, cplx<T>* __restrict__ buf,
                                                     int tid, int64_t c) {
  constexpr int L = 1 << LG, NT = L / 16;
  const bool active = tid < NT;
  const T* __restrict__ sig = a.sig + c * a.n;
  cplx<T> v[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int k = tid + r * NT;
    v[r] = mk<T>(active && k < a.n ? sig[k] : T(0), T(0));  // zero padding of the linear correlation (styx_cwt.py:195-196)
  }
  small_fft<T, LG, -1, GUARD>(v, buf, a.tw, a.tw_log2 - LG, tid, active);
  if (active) {
#pragma unroll
    for (int r = 0; r < 16; ++r) X[c * L + tid + r * NT] = v[r];
  }
}

// Role 0 is the 2^LOG2L-point spectrum, role 1 the 2^(LOG2L - 1)-point one (on the first half of the threads): every call
// -- qi_cwt, qi_stx or both tables of qi_cwt_stx in one launch -- runs a length through the same code, so a record's
// spectrum has the same bits whichever call formed it.
// (float64, LOG2L = 14: the 2^14-point transform does not fit the LDS -- the kernel is the shorter role alone)
template <typename T, int LOG2L>
constexpr bool small_fwd_long() { return (sizeof(cplx<T>) << LOG2L) <= kSmallLdsBytes; }
template <typename T, int LOG2L>
constexpr int small_fwd_threads() { return (1 << (small_fwd_long<T, LOG2L>() ? LOG2L : LOG2L - 1)) / 16; }

template <typename T, int LOG2L>
__global__ void __launch_bounds__((small_fwd_threads<T, LOG2L>())) k_small_fwd(SmallFwdArgs<T> a) {
  extern __shared__ __align__(16) unsigned char small_lds[];
  cplx<T>* buf = reinterpret_cast<cplx<T>*>(small_lds);
  if constexpr (small_fwd_long<T, LOG2L>()) {
    if (a.role0 + (int)blockIdx.y == 0) {
      small_forward_record<T, LOG2L, false>(a, a.X[0], buf, threadIdx.x, blockIdx.x);
      return;
    }
  }
  small_forward_record<T, LOG2L - 1, small_fwd_long<T, LOG2L>()>(a, a.X[1], buf, threadIdx.x, blockIdx.x);
}

// ---- band kernel: workgroup (chunk, record) walks the bands of its chunk --------------------------------------------
// Panel sample t = (m - off) mod L of the inverse transform's Y[m], kept when t < n; a thread holds m = tid + r NT.  The three
// tables' offsets (run_transform's constants) make t a compile-time function of r plus tid:
//   Stockwell (KIND 2, L = n, off = 0)       t = tid + r NT
//   atoms     (KIND 1, L = n, off = n / 2)   t = tid + ((r + 8) mod 16) NT
//   styx      (KIND 0, L = 2n, off = n / 2 - 1 = 4 NT - 1)   t = tid + 1 + (r - 4) NT for r = 3 .. 11: r = 3 keeps the last
//             thread's value alone (t = 0), r = 11 every thread's but the last; the other seven registers are outside the record
template <int KIND, int NT>
__device__ __forceinline__ bool small_out_index(int r, int tid, int* t) {
  if constexpr (KIND == 2) {
    *t = tid + r * NT;
    return true;
  } else if constexpr (KIND == 1) {
    *t = tid + ((r + 8) & 15) * NT;
    return true;
  } else {
    *t = tid + 1 + (r - 4) * NT;
    return r == 3 ? tid == NT - 1 : r == 11 ? tid < NT - 1 : (r > 3 && r < 11);
  }
}

template <typename T, int LOG2L, int KIND, bool COEF, bool BITS>
__global__ void __launch_bounds__((1 << LOG2L) / 16) k_small_band(SmallArgs<T> a) {
  constexpr int L = 1 << LOG2L, NT = L / 16, NW = NT / kWave;
  extern __shared__ __align__(16) unsigned char small_lds[];
  cplx<T>* buf = reinterpret_cast<cplx<T>*>(small_lds);
  __shared__ double s_red[3][NW];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid / kWave;
  const int chunk = blockIdx.x;
  const int64_t c = blockIdx.y;
  const int j_lo = (int)((int64_t)chunk * a.B / a.nchunk), j_hi = (int)((int64_t)(chunk + 1) * a.B / a.nchunk);
  const cplx<T>* __restrict__ X = a.X + c * L;
  const int n = a.n;

  T col[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) col[r] = T(0);
  T mx = T(0);
  double plogp = 0.0;

  for (int j = j_lo; j < j_hi; ++j) {
    cplx<T> v[16];
    if constexpr (KIND == 2) {
      // X[(k + idx_j) mod n] exp2(-(coef_j ks)^2) / n, ks the signed bin of k (k_stx_window's expression)
      const int idx = (int)a.stx_idx[j];
      const T cf = (T)a.stx_coef[j];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int k = tid + r * NT;
        const int ks = (k <= (n - 1) / 2) ? k : k - n;
        const T g = cf * (T)ks;
        const T w = exp2_t(-g * g) * (T(1) / (T)n);
        int src = k + idx;
        if (src >= n) src -= n;
        const cplx<T> x = X[src];
        v[r] = mk<T>(x.x * w, x.y * w);
      }
    } else {
      const cplx<T>* __restrict__ H = a.H + (int64_t)j * L;  // (1 / L folded into the bank)
#pragma unroll
      for (int r = 0; r < 16; ++r) v[r] = cmul(X[tid + r * NT], H[tid + r * NT]);
    }
    small_fft<T, LOG2L, 1>(v, buf, a.tw, a.tw_shift, tid);

    // v[r] = Y[tid + r NT]
    const int64_t orow = (c * a.B + j) * (int64_t)n;
    T rowacc = T(0);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      if (KIND == 0 && (r < 3 || r > 11)) continue;
      int t;
      const bool keep = small_out_index<KIND, NT>(r, tid, &t);
      const cplx<T> z = v[r];
      const T m2 = norm2(z.x, z.y);
      if (keep) {
        if constexpr (COEF) stream_store(a.coef + orow + t, z);
        if constexpr (BITS) a.bits[orow + t] = log2_t(sqrt_t(m2) + a.eps);
      }
      const T p = keep ? mul_rn(a.power_scale, m2) : T(0);
      col[r] += p;
      rowacc += p;
      mx = max_t(mx, p);
      plogp += (double)plog2p(p);
    }
    if (a.part_band) {  // (uniform)
      const double rs = wave_sum((double)rowacc);
      if (lane == 0) s_red[0][wv] = rs;
      __syncthreads();  // (the next write of s_red[0] lies behind the barriers of the next band's transform)
      if (tid == 0) a.part_band[c * a.B + j] = fold_band_sum<NW>(s_red[0]);
    }
  }

  T tot = T(0);
#pragma unroll
  for (int r = 0; r < 16; ++r) tot += col[r];
  if (a.time_part) {
    T* __restrict__ plane = a.time_part + (c * a.chunk_total + chunk) * (int64_t)n;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      if (KIND == 0 && (r < 3 || r > 11)) continue;
      int t;
      if (small_out_index<KIND, NT>(r, tid, &t)) plane[t] = col[r];
    }
  }
  if (a.part_stat) {
    __syncthreads();  // thread 0 is done with the last band's s_red[0]
    const PanelStats ps = fold_stats<NW>(mx, tot, plogp, s_red, tid);
    if (tid == 0) {
      double* o = a.part_stat + (c * a.nchunk + chunk) * 3;
      o[0] = ps.mx;
      o[1] = ps.sum;
      o[2] = ps.plogp;
    }
  }
}

template <typename T, int LOG2L, int KIND>
int launch_band_len(const SmallArgs<T>& a, int64_t ct, hipStream_t st) {
  constexpr size_t lds = ((size_t)1 << LOG2L) * sizeof(cplx<T>);
  return with_panels(a.coef != nullptr, a.bits != nullptr, [&](auto coef, auto bits) -> int {
    auto kern = &k_small_band<T, LOG2L, KIND, decltype(coef)::value, decltype(bits)::value>;
    QI_TRY(allow_dynamic_lds(reinterpret_cast<const void*>(kern), lds));
    kern<<<dim3((unsigned)a.nchunk, (unsigned)ct), (1 << LOG2L) / 16, lds, st>>>(a);
    QI_LAUNCH_CHECK();
    return QI_OK;
  });
}

template <typename T, int KIND>
int launch_band_kind(const SmallArgs<T>& a, int64_t ct, hipStream_t st) {
  // (n = 2^10 .. 2^13: the styx bank's 2n-point transforms start at 2^11, and only they reach 2^14 -- in float32)
  switch (a.L) {
    case 1 << 10:
      if constexpr (KIND != 0) return launch_band_len<T, 10, KIND>(a, ct, st);
      break;
    case 1 << 11: return launch_band_len<T, 11, KIND>(a, ct, st);
    case 1 << 12: return launch_band_len<T, 12, KIND>(a, ct, st);
    case 1 << 13: return launch_band_len<T, 13, KIND>(a, ct, st);
    case 1 << 14:
      if constexpr (KIND == 0 && sizeof(T) == 4) return launch_band_len<T, 14, KIND>(a, ct, st);
      break;
    default: break;
  }
  set_error("small-record engine: no kernel for a %d-point transform of this type", a.L);
  return QI_ERR_UNSUPPORTED;
}

template <typename T, int LOG2L>
int launch_fwd_len(const SmallFwdArgs<T>& a, bool both, int64_t ct, hipStream_t st) {
  const bool long_role = a.role0 == 0;
  const size_t lds = ((size_t)1 << (long_role ? LOG2L : LOG2L - 1)) * sizeof(cplx<T>);
  auto kern = &k_small_fwd<T, LOG2L>;
  QI_TRY(allow_dynamic_lds(reinterpret_cast<const void*>(kern), lds));
  kern<<<dim3((unsigned)ct, both ? 2u : 1u), (1 << (long_role ? LOG2L : LOG2L - 1)) / 16, lds, st>>>(a);
  QI_LAUNCH_CHECK();
  return QI_OK;
}

}  // namespace

bool small_len_ok(int64_t L, size_t elem_bytes) {
  return is_pow2(L) && L >= ((int64_t)1 << kSmallMinLog2) && L <= ((int64_t)1 << kSmallMaxLog2) &&
         (size_t)L * elem_bytes <= kSmallLdsBytes;
}

template <typename T>
int launch_small_band(const SmallArgs<T>& a, int64_t ct, hipStream_t st) {
  if (!small_len_ok(a.L, sizeof(cplx<T>))) {
    set_error("small-record engine: a %d-point transform does not fit the LDS", a.L);
    return QI_ERR_UNSUPPORTED;
  }
  // (the kernels' output maps are compiled for run_transform's offsets)
  const int64_t off = a.kind == 0 ? (a.n - 1) / 2 : a.kind == 1 ? a.n / 2 : 0;
  if (a.kind < 0 || a.kind > 2 || a.L != (a.kind == 0 ? 2 * a.n : a.n) || a.off != off || (a.kind == 2) != (a.H == nullptr)) {
    set_error("small-record engine: table kind %d does not match its transform (L = %d, n = %d, off = %d)", a.kind, a.L, a.n, a.off);
    return QI_ERR_ARG;
  }
  return a.kind == 0 ? launch_band_kind<T, 0>(a, ct, st) : a.kind == 1 ? launch_band_kind<T, 1>(a, ct, st) : launch_band_kind<T, 2>(a, ct, st);
}

template <typename T>
int launch_small_forward(const T* sig, cplx<T>* X2, cplx<T>* X1, const cplx<T>* tw, int64_t tw_len, int64_t n, int64_t ct,
                         hipStream_t st) {
  // X2: the 2n-point spectra (zero-padded records), X1: the n-point spectra; either may be null
  if (!X2 && !X1) return QI_OK;
  if ((X2 && !small_len_ok(2 * n, sizeof(cplx<T>))) || !small_len_ok(n, sizeof(cplx<T>)) || tw_len < 2 * n) {
    set_error("small-record engine: no forward transform for records of %lld samples", (long long)n);
    return QI_ERR_UNSUPPORTED;
  }
  SmallFwdArgs<T> a{};
  a.sig = sig;
  a.X[0] = X2;
  a.X[1] = X1;
  a.tw = tw;
  a.tw_log2 = 0;
  while (((int64_t)1 << a.tw_log2) < tw_len) ++a.tw_log2;
  a.n = (int32_t)n;
  a.role0 = X2 ? 0 : 1;
  const bool both = X2 && X1;
  switch (2 * n) {
    case 1 << 11: return launch_fwd_len<T, 11>(a, both, ct, st);
    case 1 << 12: return launch_fwd_len<T, 12>(a, both, ct, st);
    case 1 << 13: return launch_fwd_len<T, 13>(a, both, ct, st);
    default: return launch_fwd_len<T, 14>(a, both, ct, st);
  }
}

template int launch_small_band<float>(const SmallArgs<float>&, int64_t, hipStream_t);
template int launch_small_band<double>(const SmallArgs<double>&, int64_t, hipStream_t);
template int launch_small_forward<float>(const float*, float2*, float2*, const float2*, int64_t, int64_t, int64_t, hipStream_t);
template int launch_small_forward<double>(const double*, double2*, double2*, const double2*, int64_t, int64_t, int64_t,
                                          hipStream_t);

}  // namespace native
}  // namespace qi
