// Capon (minimum-variance) power of cross-spectral matrices over a grid of delay sets (include/qi_adaptive.h):
//   1 / (e^H R^-1 e),  R = S + load I,  e_i = exp(2 pi i freq tau_i).
// Two kernels.  k_csd_whiten factors every matrix once, R = L L^H, and stores V = L^-H, so that R^-1 = V V^H and
//   D = e^H R^-1 e = |V^H e|^2 = sum_j | sum_i conj(V[i][j]) e_i |^2
// is a sum of squares: never negative, and its rounding error goes with the condition number of L, the square root of R's.
// k_beam_capon forms D for one matrix and 16 grid points as the complex product W = V^H E of a [C x C] and a [C x 16] matrix
// on the matrix cores, in k_beam_power's structure (qi_beam.hip): V in LDS as it lies in memory is the A operand read with
// K = i and M = j, the factors are the B operand in registers, four real accumulators per complex product,
//   rr = sum Vr er,  ii = sum Vi ei,  ir = sum Vi er,  ri = sum Vr ei;   Re W = rr + ii,  Im W = ri - ir
// (the conjugate is the sign of Im W, which the square forgets).  V is upper triangular: row tile tj of W needs the K steps
// t < 4 (tj + 1) alone, 10 of the 16 tile products at 64 sensors.  There is no closing product: a lane squares and adds its
// own result registers, the four K slots of a grid point are added by two exchanges, (0 + 1) + (2 + 3), once per matrix, the
// reciprocal is taken in double and summed in double over the band in ascending f.  The order of the K steps sigma(t, q), the
// phase arithmetic, the padding, the LDS pitch and the work split are k_beam_power's: power[b][g] has the same bits wherever
// grid point g lies in whatever grid, in any band table that holds the band, for either workgroup size.
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
#include "qi_beam_common.hpp"
#include "qi_adaptive.h"

#include <cmath>
#include <limits>

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

template <typename T>
struct CaponArgs {
  const cplx<T>* V;      // [nf][C][C]
  const double* tau;     // [G][C]
  const double* freq;    // [nf] (scratch)
  const int64_t* first;  // [nb + 1] (scratch), or null: band b is matrix b
  T* power;              // [nb][G]
  int64_t C, G;
  int64_t gparts;  // workgroups per band
};

template <typename T, int NW, int NT>
__global__ void __launch_bounds__(NW* kWave) k_beam_capon(CaponArgs<T> a) {
  using M = Mx<T>;
  using acc = typename M::acc;
  constexpr int CP = NT * kBeamTile, LD = beam_ld<T>(NT), KT = 4 * NT;  // padded side, row pitch, K steps
  extern __shared__ __align__(16) unsigned char capon_lds[];
  cplx<T>* sm = reinterpret_cast<cplx<T>*>(capon_lds);  // [CP][LD]
  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  const int wv = __builtin_amdgcn_readfirstlane(tid / kWave);
  const int64_t b = (int64_t)blockIdx.x / a.gparts, part = (int64_t)blockIdx.x % a.gparts;
  const int64_t f0 = a.first ? a.first[b] : b, f1 = a.first ? a.first[b + 1] : b + 1;
  const int C = (int)a.C, col = lane & 15;
  const int64_t g0 = (part * NW + wv) * kBeamTile, g = g0 + col;
  const bool wave_on = g0 < a.G, on = g < a.G;  // (wave_on: the whole wave)
  for (int e = tid; e < CP * LD; e += NW * kWave) sm[e] = mk<T>(T(0), T(0));  // the padding stays zero: no load writes it
  // the delays of the lane's grid point at its sensors, for all matrices
  double tau[KT];
#pragma unroll
  for (int t = 0; t < KT; ++t) {
    const int s = kBeamTile * (t >> 2) + M::row(lane, t & 3);
    tau[t] = on && s < C ? a.tau[g * C + s] : 0.0;
  }
  double sum = 0.0;  // of 1 / D over the band
  for (int64_t f = f0; f < f1; ++f) {
    __syncthreads();  // the previous matrix has been read (first: the zeros are written)
    const cplx<T>* __restrict__ Vf = a.V + f * C * C;
    for (int e = tid; e < C * C; e += NW * kWave) {
      const int i = e / C;
      sm[i * LD + (e - i * C)] = Vf[e];
    }
    __syncthreads();
    if (!wave_on) continue;  // (it keeps taking the barriers)
    const double fr = a.freq[f];
    T er[KT], ei[KT];
#pragma unroll
    for (int t = 0; t < KT; ++t) {
      double turns = fr * tau[t];
      turns -= rint(turns);  // [-1/2, 1/2]
      beam_sincospi((T)(2.0 * turns), &ei[t], &er[t]);
    }
    T d = T(0);
#pragma unroll
    for (int tj = 0; tj < NT; ++tj) {
      acc rr{0, 0, 0, 0}, ii{0, 0, 0, 0}, ir{0, 0, 0, 0}, ri{0, 0, 0, 0};
#pragma unroll
      for (int t = 0; t < 4 * (tj + 1); ++t) {  // V[i][j] = 0 for i > j: the sensors of the tiles up to tj
        const int s = kBeamTile * (t >> 2) + M::row(lane, t & 3);
        const cplx<T> v = sm[s * LD + tj * kBeamTile + col];  // V[i = s][j]: the A operand is V^T, conjugated by the signs
        rr = M::mac(v.x, er[t], rr);
        ii = M::mac(v.y, ei[t], ii);
        ir = M::mac(v.y, er[t], ir);
        ri = M::mac(v.x, ei[t], ri);
      }
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const T wr = rr[reg] + ii[reg], wi = ri[reg] - ir[reg];
        d += wr * wr + wi * wi;
      }
    }
    // the four K slots of a grid point: (0 + 1) + (2 + 3), the same value in all four
    d += __shfl_xor(d, 16);
    d += __shfl_xor(d, 32);
    sum += 1.0 / (double)d;
  }
  if (!wave_on) return;
  if (on && lane < kBeamTile) a.power[b * a.G + g] = (T)sum;
}

template <typename T, int NW>
int launch_beam_capon(const CaponArgs<T>& a, int ntile, int64_t nb, hipStream_t st) {
  const dim3 grid((unsigned)(nb * a.gparts));
  const size_t lds = (size_t)ntile * kBeamTile * beam_ld<T>(ntile) * sizeof(cplx<T>);  // <= 64 KiB
  switch (ntile) {
    case 1: k_beam_capon<T, NW, 1><<<grid, NW * kWave, lds, st>>>(a); break;
    case 2: k_beam_capon<T, NW, 2><<<grid, NW * kWave, lds, st>>>(a); break;
    case 3: k_beam_capon<T, NW, 3><<<grid, NW * kWave, lds, st>>>(a); break;
    default: k_beam_capon<T, NW, kBeamMaxTiles><<<grid, NW * kWave, lds, st>>>(a); break;
  }
  QI_LAUNCH_CHECK();
  return QI_OK;
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
    a.CP = (int)ceil_div(C, kBeamTile) * kBeamTile;
    const size_t lds = (size_t)a.CP * a.CP * sizeof(cplx<T>);  // <= 64 KiB
    k_csd_whiten<T><<<dim3((unsigned)nf), kWhitenWaves * kWave, lds, st>>>(a);
    QI_LAUNCH_CHECK();
    return QI_OK;
  });
}

int64_t qi_beam_capon_scratch_bytes(int dtype, int64_t C, int64_t nf, int64_t G, int64_t nb) {
  QI_TRY(beam_shape_check(dtype, C, nf, G, nb));
  return (int64_t)beam_scratch(nf, nb);
}

int qi_beam_capon(int dtype, int device, const void* whitener, int64_t C, int64_t nf, const double* freq_hz, const void* delays_s,
                  int64_t G, const int64_t* band_first, int64_t nb, void* power, void* peak_index, void* peak_value, void* scratch,
                  int64_t scratch_bytes, qi_stream stream) {
  QI_TRY(beam_call_check(dtype, C, nf, G, nb, whitener, freq_hz, delays_s, band_first, power, peak_index, peak_value, scratch,
                         scratch_bytes));
  DeviceGuard guard(device);
  hipStream_t st = (hipStream_t)stream;
  double* freq;
  int64_t* first;
  QI_TRY(beam_put_tables(scratch, freq_hz, nf, band_first, nb, st, &freq, &first));
  return by_dtype(dtype, [&](auto t) -> int {
    using T = decltype(t);
    const int ntile = (int)ceil_div(C, kBeamTile);
    const bool many = beam_many(G, nb);
    CaponArgs<T> a{};
    a.V = static_cast<const cplx<T>*>(whitener);
    a.tau = static_cast<const double*>(delays_s);
    a.freq = freq;
    a.first = first;
    a.power = static_cast<T*>(power);
    a.C = C;
    a.G = G;
    a.gparts = ceil_div(ceil_div(G, kBeamTile), many ? kBeamWavesMany : kBeamWavesFew);
    QI_TRY((many ? launch_beam_capon<T, kBeamWavesMany>(a, ntile, nb, st) : launch_beam_capon<T, kBeamWavesFew>(a, ntile, nb, st)));
    if (peak_index || peak_value) {
      k_beam_peaks<T><<<dim3((unsigned)nb), kPeakThreads, 0, st>>>(a.power, G, static_cast<int64_t*>(peak_index),
                                                                  static_cast<T*>(peak_value));
      QI_LAUNCH_CHECK();
    }
    return QI_OK;
  });
}

}  // extern "C"
