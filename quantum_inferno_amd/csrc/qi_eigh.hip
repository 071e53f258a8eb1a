// Eigenpairs of Hermitian cross-spectral matrices (include/qi_subspace.h, qi_csd_eigh): k_csd_eigh diagonalises every matrix
// once, S = U diag(w) U^H, w ascending -- what the MUSIC form over a delay grid reads (k_beam_music, qi_beam.hip: the null
// spectrum e^H U_n U_n^H e is a sum of squares over the noise columns of U).
//
// A parallel cyclic two-sided Jacobi iteration, one matrix per workgroup of eight waves, the working matrix A and the
// accumulated rotations V both in LDS (2 x 64 KiB at 64 float64 sensors).  A sweep is a round-robin tournament of n = C
// rounded up to even players: n - 1 steps of n / 2 disjoint pairs (player n - 1 stays, the others turn; step s, pair k:
// (n - 1, s) for k = 0, else (s + k, s - k) mod n - 1; a pair that holds the bye n - 1 >= C is left out).  Wave w takes the
// pairs k = w (mod 8).  For a pair p < q, with A[p][q] = g ph, |ph| = 1:
//   tau = (A[q][q] - A[p][p]) / 2 g,  t = sign(tau) / (|tau| + sqrt(1 + tau^2)),  c = 1 / sqrt(1 + t^2),  s = t c,
//   J = [[c, s ph], [-s conj(ph), c]] on (p, q):  A <- J^H A J,  V <- V J,  A[p][p] -= t g,  A[q][q] += t g,  A[p][q] = 0.
// The parameters of a wave's (up to four) pairs are formed once, lane u those of pair u, and cross the wave by lane reads.
// All column rotations (A J: lane i is row i; V is kept TRANSPOSED, its columns p and q are rows of LDS) happen behind one
// barrier, all row rotations (J^H A: lane j is column j) behind the next: the pairs of a step are disjoint, so no two waves
// touch the same column resp. row, and a pair's parameters are read from its own two columns before it turns them.
// A rotation whose |A[p][q]|^2 is at most eps^2 |A|_F^2 is skipped: if a whole sweep skips, the test below holds already.
// After every sweep the off-diagonal sum of squares and the Frobenius norm are summed in double -- a lane its row over the
// wave's columns in ascending order, the lanes by a butterfly, the waves in ascending order -- so that every thread holds the
// same two numbers and takes the same branch: done when off <= C eps |A|_F (zero sweeps for a diagonal matrix: its bits are
// left alone), info = 1 when the norm is not finite (a NaN or an inf in the triangle that is read) or after kEighSweeps sweeps.
// Every order above depends on C alone: the bits depend on the matrix and C alone.  The diagonal is then sorted by rank
// (stable: equal values keep the order of their positions) and the columns of V follow.  Element (row, col) of either image
// lies at row CP + (col ^ (row & 15)), as in qi_whiten.hip: a walk along a column meets 16 different 16-byte slots.
#include <cmath>
#include <limits>

#include "qi_host.hpp"
#include "qi_device.hpp"   // kWave
#include "qi_fft_reg.hpp"  // QI_LAUNCH_CHECK
#include "qi_mfma.hpp"     // kMxTile
#include "qi_subspace.h"   // (and qi_beam.h: QI_BEAM_MAX_SENSORS)

static_assert(QI_BEAM_MAX_SENSORS == 64, "the solver's lane map: one lane per row of the matrix");

namespace {

constexpr int kEighWaves = 8;
constexpr int kEighSweeps = 40;
constexpr int kEighPairs = QI_BEAM_MAX_SENSORS / 2 / kEighWaves;  // pairs of a wave in a step
constexpr size_t kEighTail = 2 * kEighWaves * sizeof(double) + QI_BEAM_MAX_SENSORS * sizeof(int);  // the norms' partial sums, the order

template <typename T>
struct EighArgs {
  const cplx<T>* S;  // [nf][C][C]
  T* W;              // [nf][C]
  cplx<T>* U;        // [nf][C][C]
  int32_t* info;     // [nf] or null
  int C, CP;  // sensors, padded to whole tiles: the side of the LDS images
};

__device__ __forceinline__ float eigh_sqrt(float x) { return sqrtf(x); }
__device__ __forceinline__ double eigh_sqrt(double x) { return sqrt(x); }

template <typename T>
__global__ void __launch_bounds__(kEighWaves* kWave) k_csd_eigh(EighArgs<T> a) {
  constexpr int NTHREADS = kEighWaves * kWave;
  extern __shared__ __align__(16) unsigned char eigh_lds[];
  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  const int wv = __builtin_amdgcn_readfirstlane(tid / kWave);
  const int C = a.C, CP = a.CP;
  cplx<T>* A = reinterpret_cast<cplx<T>*>(eigh_lds);  // [CP][CP], swizzled
  cplx<T>* Vt = A + CP * CP;                          // [CP][CP], swizzled: row k is column k of V
  double* red = reinterpret_cast<double*>(Vt + CP * CP);  // [kEighWaves][2]
  int* order = reinterpret_cast<int*>(red + 2 * kEighWaves);  // [C]: the position of the value of rank r
  auto at = [CP](int row, int col) { return row * CP + (col ^ (row & 15)); };
  const bool in = lane < C;
  // the Hermitian matrix of the lower triangle and the real part of the diagonal; V = I
  const cplx<T>* __restrict__ Sf = a.S + (int64_t)blockIdx.x * C * C;
  for (int e = tid; e < C * C; e += NTHREADS) {
    const int i = e / C, j = e - i * C;
    if (j <= i) {
      cplx<T> v = Sf[e];
      if (i == j) v.y = T(0);
      A[at(i, j)] = v;
      if (i != j) A[at(j, i)] = mk<T>(v.x, T(0) - v.y);
    }
    Vt[at(i, j)] = mk<T>(i == j ? T(1) : T(0), T(0));
  }
  __syncthreads();
  // (off-diagonal, whole) sums of squares: the same two doubles in every thread
  double off2, fro2;
  auto norms = [&]() {
    double o = 0.0, d = 0.0;
    if (in)
      for (int j = wv; j < C; j += kEighWaves) {
        const cplx<T> v = A[at(lane, j)];
        const double sq = (double)v.x * (double)v.x + (double)v.y * (double)v.y;
        if (j == lane) d += sq;
        else o += sq;
      }
#pragma unroll
    for (int k = 1; k < kWave; k *= 2) {
      o += __shfl_xor(o, k);
      d += __shfl_xor(d, k);
    }
    if (lane == 0) {
      red[2 * wv] = o;
      red[2 * wv + 1] = d;
    }
    __syncthreads();
    o = 0.0;
    d = 0.0;
#pragma unroll
    for (int w = 0; w < kEighWaves; ++w) {
      o += red[2 * w];
      d += red[2 * w + 1];
    }
    off2 = o;
    fro2 = o + d;
    __syncthreads();  // (the partial sums are free again)
  };
  const double eps = (double)std::numeric_limits<T>::epsilon();
  const double tol2 = ((double)C * eps) * ((double)C * eps);
  const int n = C + (C & 1), half = n / 2;
  int bad = 0;
  norms();
  for (int sweep = 0;; ++sweep) {
    if (!(fro2 < std::numeric_limits<double>::infinity())) bad = 1;  // (a NaN too)
    if (bad || off2 <= tol2 * fro2) break;
    if (sweep == kEighSweeps) {
      bad = 1;
      break;
    }
    const double skip2 = eps * eps * fro2;
    for (int s = 0; s < n - 1; ++s) {
      // the parameters: lane u those of the wave's pair u
      int mp = 0, mq = 0, mrot = 0;
      T mc = T(1), msr = T(0), msi = T(0), mdp = T(0), mdq = T(0);
      {
        const int k = wv + kEighWaves * lane;
        if (lane < kEighPairs && k < half) {
          const int x = k == 0 ? n - 1 : (s + k) % (n - 1), y = k == 0 ? s : (s - k + n - 1) % (n - 1);
          mp = x < y ? x : y;
          mq = x < y ? y : x;
          if (mq < C) {
            const T app = A[at(mp, mp)].x, aqq = A[at(mq, mq)].x;
            const cplx<T> g = A[at(mp, mq)];
            const double g2 = (double)g.x * (double)g.x + (double)g.y * (double)g.y;
            if (g2 > skip2) {
              mrot = 1;
              // |g| without its square: scaled by the larger part
              const T big = fmax(fabs(g.x), fabs(g.y)), im = T(1) / big;
              const T ur = g.x * im, ui = g.y * im;
              const T h2 = ur * ur + ui * ui, rh = T(1) / eigh_sqrt(h2);
              const T phr = ur * rh, phi = ui * rh, mod = big * (h2 * rh);
              const T tau = (aqq - app) * (T(0.5) * (im * rh));
              const T t = (tau >= T(0) ? T(1) : T(-1)) / (fabs(tau) + eigh_sqrt(T(1) + tau * tau));
              mc = T(1) / eigh_sqrt(T(1) + t * t);
              const T sn = t * mc;
              msr = sn * phr;
              msi = sn * phi;
              mdp = app - t * mod;
              mdq = aqq + t * mod;
            }
          }
        }
      }
      int p[kEighPairs], q[kEighPairs], rot[kEighPairs];
      T c[kEighPairs], sr[kEighPairs], si[kEighPairs], dp[kEighPairs], dq[kEighPairs];
#pragma unroll
      for (int u = 0; u < kEighPairs; ++u) {
        rot[u] = __shfl(mrot, u);
        p[u] = __shfl(mp, u);
        q[u] = __shfl(mq, u);
        c[u] = __shfl(mc, u);
        sr[u] = __shfl(msr, u);
        si[u] = __shfl(msi, u);
        dp[u] = __shfl(mdp, u);
        dq[u] = __shfl(mdq, u);
      }
      // columns p and q of A and of V (lane: the row):  p' = c p - conj(s ph) q,  q' = s ph p + c q
#pragma unroll
      for (int u = 0; u < kEighPairs; ++u) {
        if (!rot[u] || !in) continue;
        {
          const cplx<T> x = A[at(lane, p[u])], y = A[at(lane, q[u])];
          A[at(lane, p[u])] = mk<T>(c[u] * x.x - (sr[u] * y.x + si[u] * y.y), c[u] * x.y - (sr[u] * y.y - si[u] * y.x));
          A[at(lane, q[u])] = mk<T>((sr[u] * x.x - si[u] * x.y) + c[u] * y.x, (sr[u] * x.y + si[u] * x.x) + c[u] * y.y);
        }
        {
          const cplx<T> x = Vt[at(p[u], lane)], y = Vt[at(q[u], lane)];
          Vt[at(p[u], lane)] = mk<T>(c[u] * x.x - (sr[u] * y.x + si[u] * y.y), c[u] * x.y - (sr[u] * y.y - si[u] * y.x));
          Vt[at(q[u], lane)] = mk<T>((sr[u] * x.x - si[u] * x.y) + c[u] * y.x, (sr[u] * x.y + si[u] * x.x) + c[u] * y.y);
        }
      }
      __syncthreads();
      // rows p and q of A (lane: the column):  p' = c p - s ph q,  q' = conj(s ph) p + c q;  the pair itself is set
#pragma unroll
      for (int u = 0; u < kEighPairs; ++u) {
        if (!rot[u] || !in) continue;
        const cplx<T> x = A[at(p[u], lane)], y = A[at(q[u], lane)];
        cplx<T> np = mk<T>(c[u] * x.x - (sr[u] * y.x - si[u] * y.y), c[u] * x.y - (sr[u] * y.y + si[u] * y.x));
        cplx<T> nq = mk<T>((sr[u] * x.x + si[u] * x.y) + c[u] * y.x, (sr[u] * x.y - si[u] * x.x) + c[u] * y.y);
        if (lane == p[u]) {
          np = mk<T>(dp[u], T(0));
          nq = mk<T>(T(0), T(0));
        } else if (lane == q[u]) {
          np = mk<T>(T(0), T(0));
          nq = mk<T>(dq[u], T(0));
        }
        A[at(p[u], lane)] = np;
        A[at(q[u], lane)] = nq;
      }
      __syncthreads();
    }
    norms();
  }
  // the rank of every diagonal entry: below it the smaller values and the equal ones at lower positions
  const T nan = std::numeric_limits<T>::quiet_NaN();
  if (wv == 0 && in) {
    const T d = A[at(lane, lane)].x;
    int rank = 0;
    for (int j = 0; j < C; ++j) {
      const T dj = A[at(j, j)].x;
      rank += (dj < d || (dj == d && j < lane)) ? 1 : 0;
    }
    if (bad) {
      a.W[(int64_t)blockIdx.x * C + lane] = nan;
    } else {
      order[rank] = lane;
      a.W[(int64_t)blockIdx.x * C + rank] = d;
    }
  }
  __syncthreads();
  cplx<T>* __restrict__ Uf = a.U + (int64_t)blockIdx.x * C * C;
  for (int e = tid; e < C * C; e += NTHREADS) {
    const int r = e / C, col = e - r * C;
    Uf[e] = bad ? mk<T>(nan, nan) : Vt[at(order[col], r)];
  }
  if (tid == 0 && a.info) a.info[blockIdx.x] = bad;
}

}  // namespace

extern "C" {

int qi_csd_eigh(int dtype, int device, const void* csd, int64_t C, int64_t nf, void* eigenvalues, void* eigenvectors, void* info,
                qi_stream stream) {
  QI_REQUIRE(dtype == QI_F32 || dtype == QI_F64, "bad dtype %d", dtype);
  QI_REQUIRE(C >= 1 && C <= QI_BEAM_MAX_SENSORS, "%lld sensors: 1 to %d", (long long)C, QI_BEAM_MAX_SENSORS);
  QI_REQUIRE(nf >= 1, "bad shape: %lld matrices", (long long)nf);
  QI_REQUIRE(nf < (1ll << 31), "request too large");
  QI_REQUIRE(csd && eigenvalues && eigenvectors, "null argument");
  QI_REQUIRE(aligned(csd, 2 * elem_size(dtype)) && aligned(eigenvalues, elem_size(dtype)) && aligned(eigenvectors, 2 * elem_size(dtype)) &&
                 aligned(info, 4),
             "misaligned pointer");
  DeviceGuard guard(device);
  hipStream_t st = (hipStream_t)stream;
  return by_dtype(dtype, [&](auto t) -> int {
    using T = decltype(t);
    EighArgs<T> a{};
    a.S = static_cast<const cplx<T>*>(csd);
    a.W = static_cast<T*>(eigenvalues);
    a.U = static_cast<cplx<T>*>(eigenvectors);
    a.info = static_cast<int32_t*>(info);
    a.C = (int)C;
    a.CP = (int)ceil_div(C, kMxTile) * kMxTile;  // whole tiles (the swizzle needs a multiple of 16)
    const size_t lds = 2 * (size_t)a.CP * a.CP * sizeof(cplx<T>) + kEighTail;  // <= 128 KiB + 384 bytes
    if (lds > 64 * 1024) QI_TRY(allow_dynamic_lds(reinterpret_cast<const void*>(&k_csd_eigh<T>), lds));
    k_csd_eigh<T><<<dim3((unsigned)nf), kEighWaves * kWave, lds, st>>>(a);
    QI_LAUNCH_CHECK();
    return QI_OK;
  });
}

}  // extern "C"
