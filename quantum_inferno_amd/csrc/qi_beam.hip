// Steered (Bartlett) power of cross-spectral matrices over a grid of delay sets (include/qi_beam.h): for matrix f and grid
// point g, with the phase factors e_i = exp(2 pi i freq[f] tau[g][i]),
//   Q[f][g] = Re e^H S_f e = Re sum_j (sum_i conj(e_i) S[f][i][j]) e_j,
// summed over the matrices of a band and divided by C^2, or by C sum_f tr S_f (the semblance).
//
// The inner sum is, for one matrix and 16 grid points, the complex product W = S_f^T conj(E) of a [C x C] and a [C x 16]
// matrix, K = C, and runs on the matrix cores in the matrices' precision (v_mfma_f32_16x16x4_f32, v_mfma_f64_16x16x4_f64)
// with four real accumulators per complex product, as in qi_csd.hip:
//   rr = sum Sr er,  ii = sum Si ei,  ir = sum Si er,  ri = sum Sr ei;   Re W = rr + ii,  Im W = ir - ri.
// It is S^T and not S that is the A operand because row i of a row-major S is then what sixteen neighbouring lanes read:
// the matrix goes into LDS as it lies in memory.  The form is the same number either way, the real part of e^H S e, also for
// an S that is not Hermitian.
//
// Tile.  A WAVE takes 16 grid points (the instruction's N; lane l: grid point l & 15) and all of S_f.  The sum over K = i has
// no prescribed order, so K step t of a lane in K slot q = l >> 4 is sensor
//   sigma(t, q) = 16 (t / 4) + Mx<T>::row(l, t % 4)
// -- the sensors of the RESULT rows the lane holds, tile by tile (the two precisions differ here, through Mx<T>::row alone).
// The lane forms the factors of its grid point and these 4 ceil(C / 16) sensors in registers, once per matrix; they are the
// B operand of every row tile j of S and, again, the e_j that closes the form on the lane's own result registers:
//   Q_g += Re W[j][g] er_j - Im W[j][g] ei_j.
// No factor is ever written to memory, and none is formed twice.  The four K slots of a grid point are summed at the end, by
// two exchanges between lanes.  Sensors past C are zero rows and columns of the matrix in LDS; grid points past G have zero
// delays and are never stored.
//
// Work split.  A workgroup of NW waves takes one band and NW tiles of grid points and walks the band's matrices in order:
// matrix -> LDS (padded to whole tiles, float32 rows 4 entries longer: the four K slots then read different banks), barrier,
// every wave its products.  The band's trace is summed beside it (lane i: S[f][i][i] over f, then the lanes by a fixed tree).
// Every sum's order depends on C and the band's range alone, every wave sums alone: power[b][g] has the same bits wherever
// grid point g lies in whatever grid, in any band table that holds the band (NW is a matter of occupancy, not of results).
//
// The peaks are a second launch over the finished power: a workgroup per band, np.argmax's rules.
#include "qi_beam_common.hpp"  // the tile constants, beam_ld, beam_sincospi, the peaks, put_words, the verdicts, the scratch

namespace {

template <typename T>
struct BeamArgs {
  const cplx<T>* S;      // [nf][C][C]
  const double* tau;     // [G][C]
  const double* freq;    // [nf] (scratch)
  const int64_t* first;  // [nb + 1] (scratch), or null: band b is matrix b
  T* power;              // [nb][G]
  int64_t C, G;
  int64_t gparts;  // workgroups per band
  int normalize;
};

template <typename T, int NW, int NT>
__global__ void __launch_bounds__(NW* kWave) k_beam_power(BeamArgs<T> a) {
  using M = Mx<T>;
  using acc = typename M::acc;
  constexpr int CP = NT * kBeamTile, LD = beam_ld<T>(NT), KT = 4 * NT;  // padded side, row pitch, K steps
  extern __shared__ __align__(16) unsigned char beam_lds[];
  cplx<T>* sm = reinterpret_cast<cplx<T>*>(beam_lds);  // [CP][LD]
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
  T q = T(0), trace = T(0);
  for (int64_t f = f0; f < f1; ++f) {
    __syncthreads();  // the previous matrix has been read (first: the zeros are written)
    const cplx<T>* __restrict__ Sf = a.S + f * C * C;
    for (int e = tid; e < C * C; e += NW * kWave) {
      const int i = e / C;
      sm[i * LD + (e - i * C)] = Sf[e];
    }
    __syncthreads();
    if (!wave_on) continue;  // (it keeps taking the barriers)
    if (lane < C) trace += sm[lane * LD + lane].x;
    const double fr = a.freq[f];
    T er[KT], ei[KT];
#pragma unroll
    for (int t = 0; t < KT; ++t) {
      double turns = fr * tau[t];
      turns -= rint(turns);  // [-1/2, 1/2]
      beam_sincospi((T)(2.0 * turns), &ei[t], &er[t]);
    }
#pragma unroll
    for (int tj = 0; tj < NT; ++tj) {
      acc rr{0, 0, 0, 0}, ii{0, 0, 0, 0}, ir{0, 0, 0, 0}, ri{0, 0, 0, 0};
#pragma unroll
      for (int t = 0; t < KT; ++t) {
        const int s = kBeamTile * (t >> 2) + M::row(lane, t & 3);
        const cplx<T> v = sm[s * LD + tj * kBeamTile + col];  // S[i = s][j]: the A operand is S^T
        rr = M::mac(v.x, er[t], rr);
        ii = M::mac(v.y, ei[t], ii);
        ir = M::mac(v.y, er[t], ir);
        ri = M::mac(v.x, ei[t], ri);
      }
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {  // result row reg of tile tj is sensor sigma(4 tj + reg): the lane holds its factor
        const T wr = rr[reg] + ii[reg], wi = ir[reg] - ri[reg];
        q += wr * er[4 * tj + reg] - wi * ei[4 * tj + reg];
      }
    }
  }
  if (!wave_on) return;
  // the four K slots of a grid point: (0 + 1) + (2 + 3), the same value in all four
  q += __shfl_xor(q, 16);
  q += __shfl_xor(q, 32);
  double den = (double)C * (double)C;
  if (a.normalize) {
#pragma unroll
    for (int d = 1; d < kWave; d *= 2) trace += __shfl_xor(trace, d);
    den = (double)C * (double)trace;
  }
  if (on && lane < kBeamTile) a.power[b * a.G + g] = (T)((double)q / den);
}

template <typename T, int NW>
int launch_beam_power(const BeamArgs<T>& a, int ntile, int64_t nb, hipStream_t st) {
  const dim3 grid((unsigned)(nb * a.gparts));
  const size_t lds = (size_t)ntile * kBeamTile * beam_ld<T>(ntile) * sizeof(cplx<T>);  // <= 64 KiB
  switch (ntile) {
    case 1: k_beam_power<T, NW, 1><<<grid, NW * kWave, lds, st>>>(a); break;
    case 2: k_beam_power<T, NW, 2><<<grid, NW * kWave, lds, st>>>(a); break;
    case 3: k_beam_power<T, NW, 3><<<grid, NW * kWave, lds, st>>>(a); break;
    default: k_beam_power<T, NW, kBeamMaxTiles><<<grid, NW * kWave, lds, st>>>(a); break;
  }
  QI_LAUNCH_CHECK();
  return QI_OK;
}

}  // namespace

extern "C" {

int64_t qi_beam_power_scratch_bytes(int dtype, int64_t C, int64_t nf, int64_t G, int64_t nb) {
  QI_TRY(beam_shape_check(dtype, C, nf, G, nb));
  return (int64_t)beam_scratch(nf, nb);
}

int qi_beam_power(int dtype, int device, const void* csd, int64_t C, int64_t nf, const double* freq_hz, const void* delays_s,
                  int64_t G, const int64_t* band_first, int64_t nb, int normalize, void* power, void* peak_index,
                  void* peak_value, void* scratch, int64_t scratch_bytes, qi_stream stream) {
  QI_TRY(beam_call_check(dtype, C, nf, G, nb, csd, freq_hz, delays_s, band_first, power, peak_index, peak_value, scratch,
                         scratch_bytes));
  DeviceGuard guard(device);
  hipStream_t st = (hipStream_t)stream;
  double* freq;
  int64_t* first;
  QI_TRY(beam_put_tables(scratch, freq_hz, nf, band_first, nb, st, &freq, &first));
  return by_dtype(dtype, [&](auto t) -> int {
    using T = decltype(t);
    const int ntile = (int)ceil_div(C, kBeamTile);
    const int64_t tiles = ceil_div(G, kBeamTile);
    const bool many = beam_many(G, nb);
    BeamArgs<T> a{};
    a.S = static_cast<const cplx<T>*>(csd);
    a.tau = static_cast<const double*>(delays_s);
    a.freq = freq;
    a.first = first;
    a.power = static_cast<T*>(power);
    a.C = C;
    a.G = G;
    a.gparts = ceil_div(tiles, many ? kBeamWavesMany : kBeamWavesFew);
    a.normalize = normalize != 0;
    QI_TRY((many ? launch_beam_power<T, kBeamWavesMany>(a, ntile, nb, st) : launch_beam_power<T, kBeamWavesFew>(a, ntile, nb, st)));
    if (peak_index || peak_value) {
      k_beam_peaks<T><<<dim3((unsigned)nb), kPeakThreads, 0, st>>>(a.power, G, static_cast<int64_t*>(peak_index),
                                                                  static_cast<T*>(peak_value));
      QI_LAUNCH_CHECK();
    }
    return QI_OK;
  });
}

}  // extern "C"
