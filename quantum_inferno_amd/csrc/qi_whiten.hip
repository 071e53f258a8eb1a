// Whitening factors of cross-spectral matrices (include/qi_adaptive.h, qi_csd_whiten): k_csd_whiten factors every matrix once,
// R = S + load I = L L^H, and stores V = L^-H, so that R^-1 = V V^H -- what the Capon form over a delay grid reads
// (k_beam_capon, qi_beam.hip: e^H R^-1 e = |V^H e|^2, a sum of squares).
//
// The factorisation, one matrix per workgroup of four waves, the matrix in LDS (64 KiB at 64 float64 sensors).  Lane i of
// every wave is row i of the matrix, wave w takes the columns j = w (mod 4).  The working matrix is kept TRANSPOSED, row k of
// the LDS image is column k of L: what a step reads of the pivot column is then a row of LDS (neighbouring lanes, neighbouring
// entries) or one entry for the whole wave, and the triangle below the image's diagonal is free for the inverse.
//   Cholesky, right-looking: step k subtracts l_i conj(l_j) of the finished column k from every A[i][j], i >= j > k; the wave
//     that owns column k + 1 scales it at once (its pivot crosses the wave by a lane read), so a step costs one barrier.  The
//     image's diagonal keeps (1 / L[k][k], the pivot).
//   Inverse by substitution, X U = I with U = L^T: the rows of X are independent.  Step m adds x_r[m] U[m][j] to the partial
//     sums Y[r][j], r <= m < j, which live in the free triangle at (j, r); the wave that owns column m + 1 finishes
//     x_r[m + 1] = -Y[r][m + 1] / U[m + 1][m + 1] in place.  One barrier a step.  V = conj(X).
// Every entry's sum runs over k resp. m in ascending order whatever the thread that forms it: the bits depend on the matrix,
// C and the loading alone.  A pivot that is not a positive finite number is noted, the arithmetic runs on (no branch leaves a
// barrier behind), and the matrix's outputs are NaN.  Element (row, col) of the image lies at row CP + (col ^ (row & 15)): a
// walk along a column -- the load of the lower triangle, the store of V -- then meets 16 different 16-byte slots.
#include <cmath>
#include <limits>

#include "qi_host.hpp"
#include "qi_device.hpp"   // kWave
#include "qi_fft_reg.hpp"  // QI_LAUNCH_CHECK
#include "qi_mfma.hpp"     // kMxTile
#include "qi_adaptive.h"   // (and qi_beam.h: QI_BEAM_MAX_SENSORS)

static_assert(QI_BEAM_MAX_SENSORS == 64, "the factorisation's lane map: one lane per row of the matrix");

namespace {

constexpr int kWhitenWaves = 4;

template <typename T>
struct WhitenArgs {
  const cplx<T>* S;  // [nf][C][C]
  cplx<T>* V;        // [nf][C][C]
  int32_t* info;     // [nf] or null
  double loading;
  int C, CP;  // sensors, padded to whole tiles: the side of the LDS image
};

__device__ __forceinline__ float whiten_sqrt(float x) { return sqrtf(x); }
__device__ __forceinline__ double whiten_sqrt(double x) { return sqrt(x); }

template <typename T>
__device__ __forceinline__ bool pivot_bad(T d) {
  return !(d > T(0)) || !(d < std::numeric_limits<T>::infinity());
}

template <typename T>
__global__ void __launch_bounds__(kWhitenWaves* kWave) k_csd_whiten(WhitenArgs<T> a) {
  constexpr int NTHREADS = kWhitenWaves * kWave;
  extern __shared__ __align__(16) unsigned char whiten_lds[];
  cplx<T>* sm = reinterpret_cast<cplx<T>*>(whiten_lds);  // [CP][CP], swizzled
  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  const int wv = __builtin_amdgcn_readfirstlane(tid / kWave);
  const int C = a.C, CP = a.CP;
  auto at = [CP](int row, int col) { return row * CP + (col ^ (row & 15)); };
  const bool in = lane < C;
  // the lower triangle, transposed: A[i][j], i >= j, to (j, i); the diagonal's real part alone
  const cplx<T>* __restrict__ Sf = a.S + (int64_t)blockIdx.x * C * C;
  for (int e = tid; e < C * C; e += NTHREADS) {
    const int i = e / C, j = e - i * C;
    if (j <= i) {
      cplx<T> v = Sf[e];
      if (i == j) v.y = T(0);
      sm[at(j, i)] = v;
    }
  }
  __syncthreads();
  // the loading, and column 0
  if (wv == 0) {
    T d = in ? sm[at(lane, lane)].x : T(0);
    if (a.loading != 0.0) {
      double sum = 0.0;
      for (int i = 0; i < C; ++i) sum += (double)sm[at(i, i)].x;
      const double load = a.loading * (sum / (double)C);
      d = (T)((double)d + load);
    }
    const T d0 = __shfl(d, 0);
    const T s = whiten_sqrt(d0);
    if (lane == 0) {
      sm[at(0, 0)] = mk<T>(T(1) / s, d0);
    } else if (in) {
      const cplx<T> v = sm[at(0, lane)];
      sm[at(0, lane)] = mk<T>(v.x / s, v.y / s);
      sm[at(lane, lane)] = mk<T>(d, T(0));
    }
  }
  __syncthreads();
  for (int k = 0; k + 1 < C; ++k) {
    cplx<T> li = mk<T>(T(0), T(0));
    if (lane > k && in) li = sm[at(k, lane)];
    for (int j = k + 1 + ((wv - (k + 1)) & (kWhitenWaves - 1)); j < C; j += kWhitenWaves) {  // the wave's columns past k
      const bool on = lane >= j && in;
      cplx<T> v = mk<T>(T(0), T(0));
      if (on) {
        const cplx<T> lj = sm[at(k, j)];
        v = sm[at(j, lane)];
        v.x -= li.x * lj.x + li.y * lj.y;
        v.y -= li.y * lj.x - li.x * lj.y;
        if (lane == j) v.y = T(0);
      }
      if (j == k + 1) {  // (the whole wave: j and k are the wave's)
        const T d = __shfl(v.x, j);
        const T s = whiten_sqrt(d);
        if (on) v = lane == j ? mk<T>(T(1) / s, d) : mk<T>(v.x / s, v.y / s);
      }
      if (on) sm[at(j, lane)] = v;
    }
    __syncthreads();
  }
  int bad = 0;  // potrf's info: the first pivot that is not a positive finite number, 1-based
  for (int k = C - 1; k >= 0; --k)
    if (pivot_bad(sm[at(k, k)].y)) bad = k + 1;
  for (int m = 0; m + 1 < C; ++m) {
    cplx<T> x = mk<T>(sm[at(m, m)].x, T(0));  // x_r[m]; lane m: 1 / L[m][m]
    if (lane < m) x = sm[at(m, lane)];
    for (int j = m + 1 + ((wv - (m + 1)) & (kWhitenWaves - 1)); j < C; j += kWhitenWaves) {
      if (lane > m) continue;
      const cplx<T> u = sm[at(m, j)];
      cplx<T> y;
      if (lane == m) {
        y = mk<T>(x.x * u.x, x.x * u.y);
      } else {
        y = sm[at(j, lane)];
        y.x += x.x * u.x - x.y * u.y;
        y.y += x.x * u.y + x.y * u.x;
      }
      if (j == m + 1) {
        const T rd = sm[at(j, j)].x;
        y = mk<T>(T(0) - y.x * rd, T(0) - y.y * rd);
      }
      sm[at(j, lane)] = y;
    }
    __syncthreads();
  }
  const T nan = std::numeric_limits<T>::quiet_NaN();
  cplx<T>* __restrict__ Vf = a.V + (int64_t)blockIdx.x * C * C;
  for (int e = tid; e < C * C; e += NTHREADS) {
    const int r = e / C, c = e - r * C;
    cplx<T> v = mk<T>(T(0), T(0));
    if (c >= r) {
      if (bad) {
        v = mk<T>(nan, nan);
      } else if (c == r) {
        v = mk<T>(sm[at(r, r)].x, T(0));
      } else {
        const cplx<T> x = sm[at(c, r)];
        v = mk<T>(x.x, T(0) - x.y);
      }
    }
    Vf[e] = v;
  }
  if (tid == 0 && a.info) a.info[blockIdx.x] = bad;
}

}  // namespace

extern "C" {

int qi_csd_whiten(int dtype, int device, const void* csd, int64_t C, int64_t nf, double loading, void* whitener, void* info,
                  qi_stream stream) {
  QI_REQUIRE(dtype == QI_F32 || dtype == QI_F64, "bad dtype %d", dtype);
  QI_REQUIRE(C >= 1 && C <= QI_BEAM_MAX_SENSORS, "%lld sensors: 1 to %d", (long long)C, QI_BEAM_MAX_SENSORS);
  QI_REQUIRE(nf >= 1, "bad shape: %lld matrices", (long long)nf);
  QI_REQUIRE(nf < (1ll << 31), "request too large");
  QI_REQUIRE(loading >= 0.0 && std::isfinite(loading), "loading %g: a finite number, 0 or more", loading);
  QI_REQUIRE(csd && whitener, "null argument");
  QI_REQUIRE(aligned(csd, 2 * elem_size(dtype)) && aligned(whitener, 2 * elem_size(dtype)) && aligned(info, 4), "misaligned pointer");
  DeviceGuard guard(device);
  hipStream_t st = (hipStream_t)stream;
  return by_dtype(dtype, [&](auto t) -> int {
    using T = decltype(t);
    WhitenArgs<T> a{};
    a.S = static_cast<const cplx<T>*>(csd);
    a.V = static_cast<cplx<T>*>(whitener);
    a.info = static_cast<int32_t*>(info);
    a.loading = loading;
    a.C = (int)C;
    a.CP = (int)ceil_div(C, kMxTile) * kMxTile;  // whole tiles, as the forms pad it (the swizzle needs a multiple of 16)
    const size_t lds = (size_t)a.CP * a.CP * sizeof(cplx<T>);  // <= 64 KiB
    k_csd_whiten<T><<<dim3((unsigned)nf), kWhitenWaves * kWave, lds, st>>>(a);
    QI_LAUNCH_CHECK();
    return QI_OK;
  });
}

}  // extern "C"
