// Beam weights and beams (include/qi_steer.h): the signal from a direction, where qi_beam.hip gives its power.
// With the phase factors e_i = exp(2 pi i freq[f] tau[k][i]) of bin f and delay row k (qi_phase.hpp):
//
// Weights (k_beam_weights).  Bartlett: a = e / C.  MVDR, from the whiteners V = L^-H of k_csd_whiten (R^-1 = V V^H):
//   u = V^H e,  D = sum_j |u_j|^2,  a = V u / D.
// One launch, a WAVE per bin and tile of 16 delay rows, the bin's whitener in LDS as it lies in memory (beam_walk's image: padded
// to whole tiles with zeros, float32 rows 4 entries longer).  The first product is beam_walk's Capon product W = V^H E with the
// result kept: K step t of a lane in K slot q = l >> 4 is sensor
//   sigma(t, q) = 16 (t / 4) + Mx<T>::row(l, t % 4),
// the sensors of the RESULT rows the lane holds, so after it the lane holds u at exactly the sensors it must supply as the B
// operand of the second product V u -- no exchange between lanes, no LDS round trip.  The second product reads V untransposed,
// A[i][j] = V[i][j]: sixteen lanes read sixteen rows of one column (a pitch of 136 dwords in float32: rows r and r + 8 share a
// pair of banks -- two to four lanes per bank; the kernel is one matrix product per 16 weights rows and not the hot path).
// V is upper triangular: row tile tj of u takes the K steps t < 4 (tj + 1), row tile ti of V u the steps t >= 4 ti.  D is the
// lane's squares in ascending (tile, register) order and the two K-slot exchanges (0 + 1) + (2 + 3), as CaponForm sums it.  The
// quotients are formed in double per component and rounded once.  Without a whitener nothing is loaded and no product runs:
// the lane divides the factors it formed.  A zero component is +0 in both forms (the products' sums start from +0).
//
// Steer (k_beam_steer): out[k][f][t] = sum_i a[f][k][i] Z[i][f][t], per bin a [beams x C] x [C x nt] product.  Orientation:
// BEAMS are the instruction's M and TIME its N.  The loads of Z are the same either way (K slot q of K step s reads sensor
// 4 s + q: sixteen lanes read sixteen consecutive times of one record, four records per load instruction); the stores decide:
// with time as N every result register of a wave is, for four beams, sixteen consecutive complex entries of one row of `out`
// -- whole 128-byte (float32) or 256-byte (float64) runs --, with time as M a lane would hold four consecutive times of one
// beam and a store instruction would touch sixteen rows in 32-byte pieces.  A wave holds the 16 x C weights of its beam tile in
// registers as the A operand (2 ceil(C / 4) registers: 32 at 64 float32 sensors, 64 in float64) and streams kSteerRun tiles of
// 16 times through them -- in float32 the next tile's panel entries are loaded before the current tile's products (another
// 2 x 2 ceil(C / 4) registers) -- with four real accumulators per complex product:
//   rr = sum ar zr,  ii = sum ai zi,  ri = sum ar zi,  ir = sum ai zr;   Re out = rr - ii,  Im out = ri + ir.
// The kernel is compiled per number of K steps, ceil(C / 4) (a branch per step cost the float32 kernel its registers: 256 and
// spills into the accumulator file at 64 sensors, against 148); sensors past C inside the last step are zeros; beams past nbeam
// are zero rows that are never stored; a time past nt reads the row's last entry and is never stored.
//
// Work split of the steer.  An item is a beam tile and a chunk of kSteerRun time tiles of a bin, numbered with the beam tile
// fastest; wave w of a bin (over its workgroups) takes item w.  With four or more beam tiles the waves of a workgroup take the
// SAME chunk, and the re-reads of the panel by beam tiles beyond the first meet the workgroup's own L1.  With one or two, the
// workgroup's four or two chunks of one beam tile interleave their tiles (SteerArgs::weave): its waves read neighbouring
// 16-column runs of a row at the same moment, so a cache line that straddles two tiles -- the rows of a panel are not aligned
// to lines -- is fetched while both halves are wanted.  The workgroup size goes by the number of workgroups (kSteerFill).
// Every output entry is summed by one wave in an order that depends on C alone: neither the workgroup size nor nbeam, nf or
// nt changes a bit.
#include "qi_host.hpp"
#include "qi_device.hpp"   // kWave
#include "qi_fft_reg.hpp"  // QI_LAUNCH_CHECK
#include "qi_mfma.hpp"     // Mx, kMxTile
#include "qi_phase.hpp"    // beam_factor: the phase rule
#include "qi_steer.h"

namespace {

using qi::host::align_up;

constexpr int kSteerTile = kMxTile;  // delay rows / beams and times of a wave's tile, sensors of a row tile of the whitener
constexpr int kSteerMaxTiles = QI_BEAM_MAX_SENSORS / kSteerTile;
constexpr int kWeightWaves = 4;  // waves of a weights workgroup: all load the whitener, each takes a tile of delay rows
constexpr int kSteerRun = 8;     // time tiles a wave streams through its weights
constexpr int kSteerWavesFew = 1;  // waves per steer workgroup: few where the workgroups would not fill the chip otherwise
constexpr int kSteerWavesMany = 4;
constexpr int64_t kSteerFill = 512;  // workgroups from which the larger workgroup is taken
constexpr int64_t kSteerMaxEntries = 1ll << 40;

// entries a row of the whitener takes in LDS (beam_walk's pitch)
template <typename T>
__host__ __device__ constexpr int steer_ld(int ntile) {
  return ntile * kSteerTile + (sizeof(T) == 4 ? 4 : 0);
}

template <typename T>
struct WeightArgs {
  const cplx<T>* V;    // [nf][C][C], or null: Bartlett
  const double* tau;   // [nbeam][C]
  const double* freq;  // [nf] (scratch)
  cplx<T>* w;          // [nf][nbeam][C]
  int64_t C, nbeam;
  int64_t kparts;  // workgroups per bin
};

template <typename T, int NT>
__global__ void __launch_bounds__(kWeightWaves* kWave) k_beam_weights(WeightArgs<T> a) {
  using M = Mx<T>;
  using acc = typename M::acc;
  constexpr int CP = NT * kSteerTile, LD = steer_ld<T>(NT), KT = 4 * NT;  // padded side, row pitch, K steps
  extern __shared__ __align__(16) unsigned char steer_lds[];
  cplx<T>* sm = reinterpret_cast<cplx<T>*>(steer_lds);  // [CP][LD]
  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  const int wv = __builtin_amdgcn_readfirstlane(tid / kWave);
  const int64_t f = (int64_t)blockIdx.x / a.kparts, part = (int64_t)blockIdx.x % a.kparts;
  const int C = (int)a.C, col = lane & 15;
  const int64_t k0 = (part * kWeightWaves + wv) * kSteerTile, k = k0 + col;
  const bool wave_on = k0 < a.nbeam, on = k < a.nbeam;  // (wave_on: the whole wave)
  if (a.V) {
    for (int e = tid; e < CP * LD; e += kWeightWaves * kWave) sm[e] = mk<T>(T(0), T(0));  // the padding stays zero: no load writes it
    __syncthreads();
    const cplx<T>* __restrict__ Vf = a.V + f * C * C;
    for (int e = tid; e < C * C; e += kWeightWaves * kWave) {
      const int i = e / C;
      sm[i * LD + (e - i * C)] = Vf[e];
    }
    __syncthreads();
  }
  if (!wave_on) return;
  // the factors of the lane's delay row at its sensors
  const double fr = a.freq[f];
  int sensor[KT];
  T er[KT], ei[KT];
#pragma unroll
  for (int t = 0; t < KT; ++t) {
    sensor[t] = kSteerTile * (t >> 2) + M::row(lane, t & 3);
    beam_factor<T>(fr, on && sensor[t] < C ? a.tau[k * C + sensor[t]] : 0.0, &er[t], &ei[t]);
  }
  cplx<T>* __restrict__ wk = a.w + (f * a.nbeam + k) * C;
  if (!a.V) {
    if (on) {
#pragma unroll
      for (int t = 0; t < KT; ++t)
        if (sensor[t] < C) wk[sensor[t]] = mk<T>((T)(((double)er[t] + 0.0) / (double)C), (T)(((double)ei[t] + 0.0) / (double)C));
    }
    return;
  }
  // u = V^H e: result row `reg` of tile tj is sensor sigma(4 tj + reg) -- the lane's own K steps of the second product
  T ur[KT], ui[KT];
  T d = T(0);
#pragma unroll
  for (int tj = 0; tj < NT; ++tj) {
    acc rr{0, 0, 0, 0}, ii{0, 0, 0, 0}, ir{0, 0, 0, 0}, ri{0, 0, 0, 0};
#pragma unroll
    for (int t = 0; t < 4 * (tj + 1); ++t) {  // V[i][j] = 0 for i > j: the sensors of the tiles up to tj
      const cplx<T> v = sm[sensor[t] * LD + tj * kSteerTile + col];  // V[i = sigma][j]: the A operand is the transpose
      rr = M::mac(v.x, er[t], rr);
      ii = M::mac(v.y, ei[t], ii);
      ir = M::mac(v.y, er[t], ir);
      ri = M::mac(v.x, ei[t], ri);
    }
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const T wr = rr[reg] + ii[reg], wi = ri[reg] - ir[reg];  // conj(V) e
      ur[4 * tj + reg] = wr;
      ui[4 * tj + reg] = wi;
      d += wr * wr + wi * wi;
    }
  }
  // the four K slots of a delay row: (0 + 1) + (2 + 3), the same value in all four
  d += __shfl_xor(d, 16);
  d += __shfl_xor(d, 32);
  const double den = (double)d;
  // V u: row tile ti, A[i][j] = V[i][j] read untransposed
#pragma unroll
  for (int ti = 0; ti < NT; ++ti) {
    acc rr{0, 0, 0, 0}, ii{0, 0, 0, 0}, ir{0, 0, 0, 0}, ri{0, 0, 0, 0};
#pragma unroll
    for (int t = 4 * ti; t < KT; ++t) {  // V[i][j] = 0 for j < i: the sensors of the tiles from ti on
      const cplx<T> v = sm[(ti * kSteerTile + col) * LD + sensor[t]];
      rr = M::mac(v.x, ur[t], rr);
      ii = M::mac(v.y, ui[t], ii);
      ir = M::mac(v.y, ur[t], ir);
      ri = M::mac(v.x, ui[t], ri);
    }
    if (on) {
#pragma unroll
      for (int reg = 0; reg < 4; ++reg)
        if (sensor[4 * ti + reg] < C)
          wk[sensor[4 * ti + reg]] = mk<T>((T)((double)(rr[reg] - ii[reg]) / den), (T)((double)(ri[reg] + ir[reg]) / den));
    }
  }
}

template <typename T>
struct SteerArgs {
  const cplx<T>* Z;  // [C][nf][nt]
  const cplx<T>* w;  // [nf][nbeam][C]
  cplx<T>* out;      // [nbeam][nf][nt]
  int64_t C, nf, nt, nbeam;
  int64_t btiles, items;  // beam tiles, items of a bin (beam tiles x chunks of time)
  int64_t weave;          // chunks of time whose tiles interleave: chunk c of such a group takes its tiles c, c + weave, ...
  int64_t parts;          // workgroups per bin
};

// The panel entries of one tile of time at the lane's sensors: K step s, K slot q -> sensor 4 s + q.  zt: the bin's row of record
// 0 at the lane's time, clamped into the row (a column past nt is never stored).  Every load is unconditional: a sensor past C
// (in the last K step alone) reads record C - 1 and is replaced by zero (its weight is zero, but 0 x NaN is not).
template <typename T, int KS>
__device__ __forceinline__ void steer_load(const cplx<T>* __restrict__ zt, int64_t row, int C, int q, T* zr, T* zi) {
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    const int sensor = 4 * s + q;
    const cplx<T> v = zt[(int64_t)(sensor < C ? sensor : C - 1) * row];
    zr[s] = sensor < C ? v.x : T(0);
    zi[s] = sensor < C ? v.y : T(0);
  }
}

template <typename T, int NW, int KS>  // KS = ceil(C / 4) K steps: four sensors each
__global__ void __launch_bounds__(NW* kWave) k_beam_steer(SteerArgs<T> a) {
  using M = Mx<T>;
  using acc = typename M::acc;
  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  const int wv = __builtin_amdgcn_readfirstlane(tid / kWave);
  const int64_t f = (int64_t)blockIdx.x / a.parts, part = (int64_t)blockIdx.x % a.parts;
  const int64_t item = part * NW + wv;
  if (item >= a.items) return;
  const int64_t bt = item % a.btiles, chunk = item / a.btiles;
  const int C = (int)a.C, col = lane & 15, q = lane >> 4;
  // the A operand: the weights of beam 16 bt + col at the sensors 4 s + q
  const int64_t kbeam = bt * kSteerTile + col;
  T ar[KS], ai[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    ar[s] = T(0);
    ai[s] = T(0);
    if (kbeam < a.nbeam && 4 * s + q < C) {
      const cplx<T> v = a.w[(f * a.nbeam + kbeam) * C + 4 * s + q];
      ar[s] = v.x;
      ai[s] = v.y;
    }
  }
  const int64_t row = a.nf * a.nt;  // entries between the rows of two records
  const cplx<T>* __restrict__ zf = a.Z + f * a.nt;
  const int64_t t_first = ((chunk / a.weave) * a.weave * kSteerRun + chunk % a.weave) * kSteerTile;
  const int64_t t_step = a.weave * kSteerTile;
  // float32: the next tile is on its way while this one is multiplied; float64 has no registers for it (the weights and one
  // tile are 128 at 64 sensors) and leaves the overlap to the other waves of the SIMD
  constexpr bool kAhead = sizeof(T) == 4;
  const int64_t t_last = a.nt - 1;
  T zr[KS], zi[KS];
  if (kAhead) steer_load<T, KS>(zf + (t_first + col < t_last ? t_first + col : t_last), row, C, q, zr, zi);
#pragma unroll 1
  for (int j = 0; j < kSteerRun; ++j) {
    const int64_t t0 = t_first + (int64_t)j * t_step, tt = t0 + col;
    if (t0 >= a.nt) break;  // (wave-uniform)
    T nr[kAhead ? KS : 1], ni[kAhead ? KS : 1];
    if constexpr (kAhead) {
      if (j + 1 < kSteerRun && t0 + t_step < a.nt)  // (wave-uniform)
        steer_load<T, KS>(zf + (tt + t_step < t_last ? tt + t_step : t_last), row, C, q, nr, ni);
    } else {
      steer_load<T, KS>(zf + (tt < t_last ? tt : t_last), row, C, q, zr, zi);
    }
    acc rr{0, 0, 0, 0}, ii{0, 0, 0, 0}, ir{0, 0, 0, 0}, ri{0, 0, 0, 0};
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      rr = M::mac(ar[s], zr[s], rr);
      ii = M::mac(ai[s], zi[s], ii);
      ri = M::mac(ar[s], zi[s], ri);
      ir = M::mac(ai[s], zr[s], ir);
    }
    if (tt < a.nt) {
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int64_t kb = bt * kSteerTile + M::row(lane, reg);
        if (kb < a.nbeam) a.out[(kb * a.nf + f) * a.nt + tt] = mk<T>(rr[reg] - ii[reg], ri[reg] + ir[reg]);
      }
    }
    if constexpr (kAhead) {
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        zr[s] = nr[s];
        zi[s] = ni[s];
      }
    }
  }
}

// what the calls refuse of a dtype and a sensor count
int steer_array_check(int dtype, int64_t C) {
  QI_REQUIRE(dtype == QI_F32 || dtype == QI_F64, "bad dtype %d", dtype);
  QI_REQUIRE(C >= 1 && C <= QI_BEAM_MAX_SENSORS, "%lld sensors: 1 to %d", (long long)C, QI_BEAM_MAX_SENSORS);
  return QI_OK;
}

// a * b * c <= 2^40 for counts that are at least 1, without overflow
bool steer_fits(int64_t a, int64_t b, int64_t c) {
  return a <= kSteerMaxEntries && b <= kSteerMaxEntries / a && c <= kSteerMaxEntries / (a * b);
}

// what the size query and qi_beam_weights refuse of a shape (the index arithmetic and the grid stay inside their types)
int weights_shape_check(int dtype, int64_t C, int64_t nf, int64_t nbeam) {
  QI_TRY(steer_array_check(dtype, C));
  QI_REQUIRE(nf >= 1 && nbeam >= 1, "bad shape: %lld bins, %lld delay rows", (long long)nf, (long long)nbeam);
  QI_REQUIRE(steer_fits(nf, nbeam, C) && nf * ceil_div(ceil_div(nbeam, kSteerTile), kWeightWaves) < (1ll << 31),
             "request too large: %lld bins x %lld delay rows x %lld sensors", (long long)nf, (long long)nbeam, (long long)C);
  return QI_OK;
}

size_t weights_scratch(int64_t nf) { return align_up((size_t)nf * sizeof(double)); }  // the frequency table

int steer_shape_check(int dtype, int64_t C, int64_t nf, int64_t nt, int64_t nbeam) {
  QI_TRY(steer_array_check(dtype, C));
  QI_REQUIRE(nf >= 1 && nt >= 1 && nbeam >= 1, "bad shape: %lld bins, %lld times, %lld beams", (long long)nf, (long long)nt,
             (long long)nbeam);
  QI_REQUIRE(steer_fits(nf, nt, C) && steer_fits(nf, nt, nbeam) && steer_fits(nf, nbeam, C) &&
                 nf * ceil_div(ceil_div(nbeam, kSteerTile) * (ceil_div(nt, kSteerRun * kSteerTile) + kSteerWavesMany), kSteerWavesFew) < (1ll << 31),
             "request too large: %lld sensors, %lld beams x %lld bins x %lld times", (long long)C, (long long)nbeam, (long long)nf,
             (long long)nt);
  return QI_OK;
}

template <typename T>
int launch_weights(const WeightArgs<T>& a, int ntile, int64_t nf, hipStream_t st) {
  const dim3 grid((unsigned)(nf * a.kparts));
  const size_t lds = a.V ? (size_t)ntile * kSteerTile * steer_ld<T>(ntile) * sizeof(cplx<T>) : 0;  // <= 64 KiB
  switch (ntile) {
    case 1: k_beam_weights<T, 1><<<grid, kWeightWaves * kWave, lds, st>>>(a); break;
    case 2: k_beam_weights<T, 2><<<grid, kWeightWaves * kWave, lds, st>>>(a); break;
    case 3: k_beam_weights<T, 3><<<grid, kWeightWaves * kWave, lds, st>>>(a); break;
    default: k_beam_weights<T, kSteerMaxTiles><<<grid, kWeightWaves * kWave, lds, st>>>(a); break;
  }
  QI_LAUNCH_CHECK();
  return QI_OK;
}

// the kernel of ceil(C / 4) K steps, found by descent from the largest
template <typename T, int NW, int KS = QI_BEAM_MAX_SENSORS / 4>
int launch_steer(const SteerArgs<T>& a, int ksteps, hipStream_t st) {
  if constexpr (KS > 1) {
    if (ksteps < KS) return launch_steer<T, NW, KS - 1>(a, ksteps, st);
  }
  k_beam_steer<T, NW, KS><<<dim3((unsigned)(a.nf * a.parts)), NW * kWave, 0, st>>>(a);
  QI_LAUNCH_CHECK();
  return QI_OK;
}

}  // namespace

extern "C" {

int64_t qi_beam_weights_scratch_bytes(int dtype, int64_t C, int64_t nf, int64_t nbeam) {
  QI_TRY(weights_shape_check(dtype, C, nf, nbeam));
  return (int64_t)weights_scratch(nf);
}

int qi_beam_weights(int dtype, int device, const void* whitener, int64_t C, int64_t nf, const double* freq_hz,
                    const void* delays_s, int64_t nbeam, void* weights, void* scratch, int64_t scratch_bytes, qi_stream stream) {
  QI_TRY(weights_shape_check(dtype, C, nf, nbeam));
  QI_REQUIRE(freq_hz && delays_s && scratch, "null argument");
  QI_REQUIRE(weights, "weights is null: nothing to produce");
  QI_TRY(require_scratch(scratch_bytes, (int64_t)weights_scratch(nf)));
  QI_REQUIRE(aligned(whitener, 2 * elem_size(dtype)) && aligned(delays_s, 8) && aligned(weights, 2 * elem_size(dtype)) &&
                 aligned(scratch, 16),
             "misaligned pointer");
  DeviceGuard guard(device);
  hipStream_t st = (hipStream_t)stream;
  double* freq = static_cast<double*>(scratch);
  QI_TRY(qi::host::put_words(freq, freq_hz, nf, st));
  return by_dtype(dtype, [&](auto t) -> int {
    using T = decltype(t);
    WeightArgs<T> a{};
    a.V = static_cast<const cplx<T>*>(whitener);
    a.tau = static_cast<const double*>(delays_s);
    a.freq = freq;
    a.w = static_cast<cplx<T>*>(weights);
    a.C = C;
    a.nbeam = nbeam;
    a.kparts = ceil_div(ceil_div(nbeam, kSteerTile), kWeightWaves);
    return launch_weights<T>(a, (int)ceil_div(C, kSteerTile), nf, st);
  });
}

int qi_beam_steer(int dtype, int device, const void* Z, int64_t C, int64_t nf, int64_t nt, const void* weights, int64_t nbeam,
                  void* out, qi_stream stream) {
  QI_TRY(steer_shape_check(dtype, C, nf, nt, nbeam));
  QI_REQUIRE(Z && weights, "null argument");
  QI_REQUIRE(out, "out is null: nothing to produce");
  QI_REQUIRE(aligned(Z, 2 * elem_size(dtype)) && aligned(weights, 2 * elem_size(dtype)) && aligned(out, 2 * elem_size(dtype)),
             "misaligned pointer");
  DeviceGuard guard(device);
  hipStream_t st = (hipStream_t)stream;
  return by_dtype(dtype, [&](auto t) -> int {
    using T = decltype(t);
    SteerArgs<T> a{};
    a.Z = static_cast<const cplx<T>*>(Z);
    a.w = static_cast<const cplx<T>*>(weights);
    a.out = static_cast<cplx<T>*>(out);
    a.C = C;
    a.nf = nf;
    a.nt = nt;
    a.nbeam = nbeam;
    a.btiles = ceil_div(nbeam, kSteerTile);
    const int64_t tiles = ceil_div(nt, kSteerTile);
    // the larger workgroup from kSteerFill workgroups on
    const bool many = nf * ceil_div(a.btiles * ceil_div(tiles, kSteerRun), kSteerWavesMany) >= kSteerFill;
    // the waves of a large workgroup that share a beam tile take neighbouring tiles of time at the same moment
    a.weave = many ? std::max<int64_t>(1, kSteerWavesMany / a.btiles) : 1;
    a.items = a.btiles * a.weave * ceil_div(tiles, kSteerRun * a.weave);
    a.parts = ceil_div(a.items, many ? kSteerWavesMany : kSteerWavesFew);
    const int ksteps = (int)ceil_div(C, 4);
    return many ? launch_steer<T, kSteerWavesMany>(a, ksteps, st) : launch_steer<T, kSteerWavesFew>(a, ksteps, st);
  });
}

}  // extern "C"
