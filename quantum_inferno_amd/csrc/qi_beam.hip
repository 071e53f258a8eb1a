// The forms of cross-spectral matrices over a grid of delay sets: one walk over a band's matrices, three forms at its ends.
// With the phase factors e_i = exp(2 pi i freq[f] tau[g][i]) of matrix f and grid point g:
//
// Bartlett, the steered power (include/qi_beam.h, k_beam_power):
//   Q[f][g] = Re e^H S_f e = Re sum_j (sum_i conj(e_i) S[f][i][j]) e_j,
// summed over the matrices of a band and divided by C^2, or by C sum_f tr S_f (the semblance).
//
// Capon, the minimum-variance power (include/qi_adaptive.h, k_beam_capon):
//   1 / (e^H R^-1 e),  R = S + load I.
// k_csd_whiten (qi_whiten.hip) factors every matrix once, R = L L^H, and stores V = L^-H, so that R^-1 = V V^H and
//   D = e^H R^-1 e = |V^H e|^2 = sum_j | sum_i conj(V[i][j]) e_i |^2
// is a sum of squares: never negative, and its rounding error goes with the condition number of L, the square root of R's.
//
// MUSIC, the reciprocal of the null spectrum (include/qi_subspace.h, k_beam_music):
//   C / (e^H P e),  P = U_n U_n^H the projector onto the noise subspace.
// k_csd_eigh (qi_eigh.hip) diagonalises every matrix once, S = U diag(w) U^H with w ascending, so that with m = C - n_sources
//   D = e^H P e = sum_{j < m} | sum_i conj(U[i][j]) e_i |^2
// is Capon's sum of squares over the first m columns of a full matrix.
//
// The walk (beam_walk).  The inner sum is, for one matrix and 16 grid points, a complex product of a [C x C] and a [C x 16]
// matrix, K = C -- Bartlett: W = S_f^T conj(E); Capon: W = V^H E -- and runs on the matrix cores in the matrices' precision
// (v_mfma_f32_16x16x4_f32, v_mfma_f64_16x16x4_f64) with four real accumulators per complex product, as in qi_csd.hip:
//   rr = sum Mr er,  ii = sum Mi ei,  ir = sum Mi er,  ri = sum Mr ei;   Re W = rr + ii,
//   Im W = ir - ri (Bartlett),  Im W = ri - ir (Capon: the conjugate is the sign of Im W, which the square forgets).
// It is S^T and not S that is the A operand because row i of a row-major S is then what sixteen neighbouring lanes read:
// the matrix goes into LDS as it lies in memory (V likewise: the A operand read with K = i and M = j).  The Bartlett form is
// the same number either way, the real part of e^H S e, also for an S that is not Hermitian.
//
// Tile.  A WAVE takes 16 grid points (the instruction's N; lane l: grid point l & 15) and all of the matrix.  The sum over
// K = i has no prescribed order, so K step t of a lane in K slot q = l >> 4 is sensor
//   sigma(t, q) = 16 (t / 4) + Mx<T>::row(l, t % 4)
// -- the sensors of the RESULT rows the lane holds, tile by tile (the two precisions differ here, through Mx<T>::row alone).
// The lane forms the factors of its grid point and these 4 ceil(C / 16) sensors in registers, once per matrix; they are the
// B operand of every row tile j of the matrix.  No factor is ever written to memory, and none is formed twice.  The four K
// slots of a grid point are summed by two exchanges between lanes, (0 + 1) + (2 + 3).  Sensors past C are zero rows and columns
// of the matrix in LDS; grid points past G have zero delays and are never stored.
//
// The forms.  Bartlett: the factors are, again, the e_j that closes the form on the lane's own result registers,
//   Q_g += Re W[j][g] er_j - Im W[j][g] ei_j;
// every row tile takes all K steps; the exchanges come once, at the band's end.  The band's trace is summed beside it (lane
// i: S[f][i][i] over f, then the lanes by a fixed tree), and the quotient is taken in double.  Capon: V is upper triangular,
// row tile tj of W needs the K steps t < 4 (tj + 1) alone, 10 of the 16 tile products at 64 sensors.  There is no closing
// product: a lane squares and adds its own result registers, the four K slots are added once per matrix, the reciprocal is
// taken in double and summed in double over the band in ascending f.  MUSIC: U is full, every row tile takes all K steps as
// Bartlett's; a lane squares and adds its result registers as Capon's, those of the columns j < m alone (it knows the column
// each register holds); D is summed in double over the band and C n_b is divided by the sum, once.
//
// Work split.  A workgroup of NW waves takes one band and NW tiles of grid points and walks the band's matrices in order:
// matrix -> LDS (padded to whole tiles, float32 rows 4 entries longer: the four K slots then read different banks), barrier,
// every wave its products.  Every sum's order depends on C and the band's range alone, every wave sums alone: power[b][g] of
// either form has the same bits wherever grid point g lies in whatever grid, in any band table that holds the band, for
// either workgroup size (NW is a matter of occupancy, not of results).  The order of the K steps, the phase arithmetic, the
// padding, the LDS pitch and the work split are written once, in the walk: the two forms cannot differ in them.
//
// The peaks are a second launch over the finished power: a workgroup per band, np.argmax's rules.
//
// Host side, once for all forms: the verdicts on a shape, a band table and a call, the scratch layout (the frequency table,
// then the band offsets), the upload of the two host tables (qi::host::put_words), the choice of the workgroup size, the
// dispatch on the tile count and the peaks launch.
#include <type_traits>

#include "qi_host.hpp"
#include "qi_device.hpp"   // kWave
#include "qi_fft_reg.hpp"  // QI_LAUNCH_CHECK
#include "qi_mfma.hpp"     // Mx, kMxTile
#include "qi_phase.hpp"    // beam_factor: the phase rule
#include "qi_beam.h"
#include "qi_adaptive.h"
#include "qi_subspace.h"

namespace {

using qi::host::align_up;

constexpr int kBeamTile = kMxTile;  // grid points of a wave, sensors of a row tile (the instruction's N and M)
constexpr int kBeamMaxTiles = QI_BEAM_MAX_SENSORS / kBeamTile;
constexpr int kBeamWavesFew = 2;  // waves per workgroup: few where the workgroups would not fill the chip otherwise
constexpr int kBeamWavesMany = 8;
constexpr int64_t kBeamFill = 512;  // workgroups from which the larger workgroup is taken
constexpr int kPeakThreads = 256;

// entries a row of the matrix takes in LDS
template <typename T>
__host__ __device__ constexpr int beam_ld(int ntile) {
  return ntile * kBeamTile + (sizeof(T) == 4 ? 4 : 0);
}

template <typename T>
struct BeamArgs {
  const cplx<T>* M;      // [nf][C][C]: the matrices S (Bartlett), the whiteners V (Capon), the eigenvectors U (MUSIC)
  const double* tau;     // [G][C]
  const double* freq;    // [nf] (scratch)
  const int64_t* first;  // [nb + 1] (scratch), or null: band b is matrix b
  T* power;              // [nb][G]
  int64_t C, G;
  int64_t gparts;  // workgroups per band
  int normalize;   // (Bartlett alone)
  int n_sources;   // (MUSIC alone)
};

// A form: the state of a lane over its band; begin, before the first matrix; matrix_in, once the matrix lies in LDS; the K steps row tile tj takes, a
// compile-time function of the unrolled tj (the factors stay in registers); tile, on the finished products of a row tile
// (result row reg of tile tj is sensor sigma(4 tj + reg): the lane holds its factor); matrix_out, after the last tile; result,
// what the lanes of the first K slot store.
template <typename T>
struct BartlettForm {
  using acc = typename Mx<T>::acc;
  T q = T(0), trace = T(0);
  static constexpr int ksteps(int tj, int nt) { return 4 * nt; }
  __device__ __forceinline__ void begin(const BeamArgs<T>&, int) {}
  __device__ __forceinline__ void matrix_in(const cplx<T>* sm, int ld, int lane, int C) {
    if (lane < C) trace += sm[lane * ld + lane].x;
  }
  __device__ __forceinline__ void tile(int tj, const acc& rr, const acc& ii, const acc& ir, const acc& ri, const T* er, const T* ei) {
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const T wr = rr[reg] + ii[reg], wi = ir[reg] - ri[reg];
      q += wr * er[4 * tj + reg] - wi * ei[4 * tj + reg];
    }
  }
  __device__ __forceinline__ void matrix_out() {}
  __device__ __forceinline__ T result(const BeamArgs<T>& a, int C) {
    // the four K slots of a grid point: (0 + 1) + (2 + 3), the same value in all four
    q += __shfl_xor(q, 16);
    q += __shfl_xor(q, 32);
    double den = (double)C * (double)C;
    if (a.normalize) {
#pragma unroll
      for (int d = 1; d < kWave; d *= 2) trace += __shfl_xor(trace, d);
      den = (double)C * (double)trace;
    }
    return (T)((double)q / den);
  }
};

template <typename T>
struct CaponForm {
  using acc = typename Mx<T>::acc;
  double sum = 0.0;  // of 1 / D over the band
  T d;
  static constexpr int ksteps(int tj, int nt) { return 4 * (tj + 1); }  // V[i][j] = 0 for i > j: the sensors of the tiles up to tj
  __device__ __forceinline__ void begin(const BeamArgs<T>&, int) {}
  __device__ __forceinline__ void matrix_in(const cplx<T>*, int, int, int) { d = T(0); }
  __device__ __forceinline__ void tile(int, const acc& rr, const acc& ii, const acc& ir, const acc& ri, const T*, const T*) {
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const T wr = rr[reg] + ii[reg], wi = ri[reg] - ir[reg];
      d += wr * wr + wi * wi;
    }
  }
  __device__ __forceinline__ void matrix_out() {
    // the four K slots of a grid point: (0 + 1) + (2 + 3), the same value in all four
    d += __shfl_xor(d, 16);
    d += __shfl_xor(d, 32);
    sum += 1.0 / (double)d;
  }
  __device__ __forceinline__ T result(const BeamArgs<T>&, int) { return (T)sum; }
};

template <typename T>
struct SubspaceForm {
  using acc = typename Mx<T>::acc;
  double sum = 0.0;  // of D over the band
  T d;
  int count = 0;  // matrices of the band
  int left[4];    // noise columns from the lane's result row `reg` of tile 0 on: m - row
  static constexpr int ksteps(int tj, int nt) { return 4 * nt; }  // U is full
  __device__ __forceinline__ void begin(const BeamArgs<T>& a, int lane) {
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) left[reg] = (int)a.C - a.n_sources - Mx<T>::row(lane, reg);
  }
  __device__ __forceinline__ void matrix_in(const cplx<T>*, int, int, int) { d = T(0); }
  __device__ __forceinline__ void tile(int tj, const acc& rr, const acc& ii, const acc& ir, const acc& ri, const T*, const T*) {
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const T wr = rr[reg] + ii[reg], wi = ri[reg] - ir[reg];
      if (kBeamTile * tj < left[reg]) d += wr * wr + wi * wi;  // column j = 16 tj + row < m
    }
  }
  __device__ __forceinline__ void matrix_out() {
    // the four K slots of a grid point: (0 + 1) + (2 + 3), the same value in all four
    d += __shfl_xor(d, 16);
    d += __shfl_xor(d, 32);
    sum += (double)d;
    ++count;
  }
  __device__ __forceinline__ T result(const BeamArgs<T>&, int C) { return (T)(((double)C * (double)count) / sum); }
};

template <typename T, int NW, int NT, typename Form>
__device__ __forceinline__ void beam_walk(const BeamArgs<T>& a) {
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
  Form form;
  form.begin(a, lane);
  for (int64_t f = f0; f < f1; ++f) {
    __syncthreads();  // the previous matrix has been read (first: the zeros are written)
    const cplx<T>* __restrict__ Mf = a.M + f * C * C;
    for (int e = tid; e < C * C; e += NW * kWave) {
      const int i = e / C;
      sm[i * LD + (e - i * C)] = Mf[e];
    }
    __syncthreads();
    if (!wave_on) continue;  // (it keeps taking the barriers)
    form.matrix_in(sm, LD, lane, C);
    const double fr = a.freq[f];
    T er[KT], ei[KT];
#pragma unroll
    for (int t = 0; t < KT; ++t) beam_factor<T>(fr, tau[t], &er[t], &ei[t]);
#pragma unroll
    for (int tj = 0; tj < NT; ++tj) {
      acc rr{0, 0, 0, 0}, ii{0, 0, 0, 0}, ir{0, 0, 0, 0}, ri{0, 0, 0, 0};
#pragma unroll
      for (int t = 0; t < Form::ksteps(tj, NT); ++t) {
        const int s = kBeamTile * (t >> 2) + M::row(lane, t & 3);
        const cplx<T> v = sm[s * LD + tj * kBeamTile + col];  // M[i = s][j]: the A operand is the transpose
        rr = M::mac(v.x, er[t], rr);
        ii = M::mac(v.y, ei[t], ii);
        ir = M::mac(v.y, er[t], ir);
        ri = M::mac(v.x, ei[t], ri);
      }
      form.tile(tj, rr, ii, ir, ri, er, ei);
    }
    form.matrix_out();
  }
  if (!wave_on) return;
  const T p = form.result(a, C);
  if (on && lane < kBeamTile) a.power[b * a.G + g] = p;
}

template <typename T, int NW, int NT>
__global__ void __launch_bounds__(NW* kWave) k_beam_power(BeamArgs<T> a) {
  beam_walk<T, NW, NT, BartlettForm<T>>(a);
}
template <typename T, int NW, int NT>
__global__ void __launch_bounds__(NW* kWave) k_beam_capon(BeamArgs<T> a) {
  beam_walk<T, NW, NT, CaponForm<T>>(a);
}
template <typename T, int NW, int NT>
__global__ void __launch_bounds__(NW* kWave) k_beam_music(BeamArgs<T> a) {
  beam_walk<T, NW, NT, SubspaceForm<T>>(a);
}

// np.argmax's order: a NaN before every number, a larger value before a smaller one, a lower index before a higher one
template <typename T>
__device__ __forceinline__ bool beam_before(T va, int64_t ia, T vb, int64_t ib) {
  const bool na = va != va, nb = vb != vb;
  if (na || nb) return na && (!nb || ia < ib);
  return va > vb || (va == vb && ia < ib);
}

template <typename T>
__global__ void __launch_bounds__(kPeakThreads) k_beam_peaks(const T* __restrict__ power, int64_t G, int64_t* __restrict__ index,
                                                            T* __restrict__ value) {
  __shared__ T sv[kPeakThreads];
  __shared__ int64_t si[kPeakThreads];
  const int tid = threadIdx.x;
  const T* __restrict__ row = power + (int64_t)blockIdx.x * G;
  T bv = T(0);
  int64_t bi = -1;  // (none yet: G may be below the thread count)
  for (int64_t g = tid; g < G; g += kPeakThreads) {
    const T v = row[g];
    if (bi < 0 || beam_before(v, g, bv, bi)) {
      bv = v;
      bi = g;
    }
  }
  sv[tid] = bv;
  si[tid] = bi;
  __syncthreads();
  for (int s = kPeakThreads / 2; s > 0; s >>= 1) {
    if (tid < s && si[tid + s] >= 0 && (si[tid] < 0 || beam_before(sv[tid + s], si[tid + s], sv[tid], si[tid]))) {
      sv[tid] = sv[tid + s];
      si[tid] = si[tid + s];
    }
    __syncthreads();
  }
  if (tid == 0) {
    if (index) index[blockIdx.x] = si[0];
    if (value) value[blockIdx.x] = sv[0];
  }
}

// what the size query and the call refuse of a shape (the index arithmetic and the grid stay inside their types)
int beam_shape_check(int dtype, int64_t C, int64_t nf, int64_t G, int64_t nb) {
  QI_REQUIRE(dtype == QI_F32 || dtype == QI_F64, "bad dtype %d", dtype);
  QI_REQUIRE(C >= 1 && C <= QI_BEAM_MAX_SENSORS, "%lld sensors: 1 to %d", (long long)C, QI_BEAM_MAX_SENSORS);
  QI_REQUIRE(nf >= 1 && G >= 1 && nb >= 1, "bad shape: %lld matrices, %lld grid points, %lld bands", (long long)nf, (long long)G,
             (long long)nb);
  QI_REQUIRE(nb <= nf, "%lld bands of %lld matrices", (long long)nb, (long long)nf);
  QI_REQUIRE(nf < (1ll << 40) && G < (1ll << 40) && nb * ceil_div(G, kBeamTile * kBeamWavesFew) < (1ll << 31), "request too large");
  return QI_OK;
}

// what the call refuses of a host band table
int beam_bands_check(const int64_t* band_first, int64_t nf, int64_t nb) {
  if (band_first) {
    QI_REQUIRE(band_first[0] >= 0 && band_first[0] < nf, "band offsets start at %lld: outside 0..%lld", (long long)band_first[0],
               (long long)nf);
    for (int64_t b = 0; b < nb; ++b)
      QI_REQUIRE(band_first[b + 1] > band_first[b], "band offsets are not strictly ascending at band %lld", (long long)b);
    QI_REQUIRE(band_first[nb] <= nf, "band offsets end at %lld, past the %lld matrices", (long long)band_first[nb], (long long)nf);
  } else {
    QI_REQUIRE(nb == nf, "no band table: every matrix is its own band, nb must be nf");
  }
  return QI_OK;
}

// the scratch: the frequency table, then the band offsets
size_t beam_freq_bytes(int64_t nf) { return align_up((size_t)nf * sizeof(double)); }
size_t beam_scratch(int64_t nf, int64_t nb) { return beam_freq_bytes(nf) + align_up((size_t)(nb + 1) * sizeof(int64_t)); }

// every refusal of a form's call, before anything is launched (matrices: the stack the form reads)
int beam_call_check(int dtype, int64_t C, int64_t nf, int64_t G, int64_t nb, const void* matrices, const double* freq_hz,
                    const void* delays_s, const int64_t* band_first, const void* power, const void* peak_index,
                    const void* peak_value, const void* scratch, int64_t scratch_bytes) {
  QI_TRY(beam_shape_check(dtype, C, nf, G, nb));
  QI_REQUIRE(matrices && freq_hz && delays_s && scratch, "null argument");
  QI_REQUIRE(power, "power is null: nothing to produce");
  QI_TRY(beam_bands_check(band_first, nf, nb));
  QI_TRY(require_scratch(scratch_bytes, (int64_t)beam_scratch(nf, nb)));
  QI_REQUIRE(aligned(matrices, 2 * elem_size(dtype)) && aligned(delays_s, 8) && aligned(power, elem_size(dtype)) &&
                 aligned(peak_index, 8) && aligned(peak_value, elem_size(dtype)) && aligned(scratch, 16),
             "misaligned pointer");
  return QI_OK;
}

template <typename Form, typename T, int NW, int NT>
constexpr auto form_kernel() {
  if constexpr (std::is_same<Form, CaponForm<T>>::value) return &k_beam_capon<T, NW, NT>;
  else if constexpr (std::is_same<Form, SubspaceForm<T>>::value) return &k_beam_music<T, NW, NT>;
  else return &k_beam_power<T, NW, NT>;
}

template <typename Form, typename T, int NW>
int launch_form(const BeamArgs<T>& a, int ntile, int64_t nb, hipStream_t st) {
  const dim3 grid((unsigned)(nb * a.gparts));
  const size_t lds = (size_t)ntile * kBeamTile * beam_ld<T>(ntile) * sizeof(cplx<T>);  // <= 64 KiB
  switch (ntile) {
    case 1: form_kernel<Form, T, NW, 1>()<<<grid, NW * kWave, lds, st>>>(a); break;
    case 2: form_kernel<Form, T, NW, 2>()<<<grid, NW * kWave, lds, st>>>(a); break;
    case 3: form_kernel<Form, T, NW, 3>()<<<grid, NW * kWave, lds, st>>>(a); break;
    default: form_kernel<Form, T, NW, kBeamMaxTiles>()<<<grid, NW * kWave, lds, st>>>(a); break;
  }
  QI_LAUNCH_CHECK();
  return QI_OK;
}

// a form's call: the refusals, the two host tables into the scratch in stream order, the form over every band, the peaks
template <template <typename> class Form>
int beam_form(int dtype, int device, const void* matrices, int64_t C, int64_t nf, const double* freq_hz, const void* delays_s,
              int64_t G, const int64_t* band_first, int64_t nb, int normalize, int n_sources, void* power, void* peak_index,
              void* peak_value, void* scratch, int64_t scratch_bytes, qi_stream stream) {
  QI_TRY(beam_call_check(dtype, C, nf, G, nb, matrices, freq_hz, delays_s, band_first, power, peak_index, peak_value, scratch,
                         scratch_bytes));
  DeviceGuard guard(device);
  hipStream_t st = (hipStream_t)stream;
  double* freq = static_cast<double*>(scratch);
  int64_t* first = band_first ? reinterpret_cast<int64_t*>(static_cast<char*>(scratch) + beam_freq_bytes(nf)) : nullptr;
  QI_TRY(qi::host::put_words(freq, freq_hz, nf, st));
  if (band_first) QI_TRY(qi::host::put_words(first, band_first, nb + 1, st));
  return by_dtype(dtype, [&](auto t) -> int {
    using T = decltype(t);
    const int ntile = (int)ceil_div(C, kBeamTile);
    const int64_t tiles = ceil_div(G, kBeamTile);
    // the larger workgroup from kBeamFill workgroups on
    const bool many = nb * ceil_div(tiles, kBeamWavesMany) >= kBeamFill;
    BeamArgs<T> a{};
    a.M = static_cast<const cplx<T>*>(matrices);
    a.tau = static_cast<const double*>(delays_s);
    a.freq = freq;
    a.first = first;
    a.power = static_cast<T*>(power);
    a.C = C;
    a.G = G;
    a.gparts = ceil_div(tiles, many ? kBeamWavesMany : kBeamWavesFew);
    a.normalize = normalize != 0;
    a.n_sources = n_sources;
    QI_TRY((many ? launch_form<Form<T>, T, kBeamWavesMany>(a, ntile, nb, st) : launch_form<Form<T>, T, kBeamWavesFew>(a, ntile, nb, st)));
    if (peak_index || peak_value) {
      k_beam_peaks<T><<<dim3((unsigned)nb), kPeakThreads, 0, st>>>(a.power, G, static_cast<int64_t*>(peak_index),
                                                                  static_cast<T*>(peak_value));
      QI_LAUNCH_CHECK();
    }
    return QI_OK;
  });
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
  return beam_form<BartlettForm>(dtype, device, csd, C, nf, freq_hz, delays_s, G, band_first, nb, normalize, 0, power, peak_index,
                                 peak_value, scratch, scratch_bytes, stream);
}

int64_t qi_beam_capon_scratch_bytes(int dtype, int64_t C, int64_t nf, int64_t G, int64_t nb) {
  QI_TRY(beam_shape_check(dtype, C, nf, G, nb));
  return (int64_t)beam_scratch(nf, nb);
}

int qi_beam_capon(int dtype, int device, const void* whitener, int64_t C, int64_t nf, const double* freq_hz, const void* delays_s,
                  int64_t G, const int64_t* band_first, int64_t nb, void* power, void* peak_index, void* peak_value, void* scratch,
                  int64_t scratch_bytes, qi_stream stream) {
  return beam_form<CaponForm>(dtype, device, whitener, C, nf, freq_hz, delays_s, G, band_first, nb, 0, 0, power, peak_index, peak_value,
                              scratch, scratch_bytes, stream);
}

int64_t qi_beam_music_scratch_bytes(int dtype, int64_t C, int64_t nf, int64_t G, int64_t nb) {
  QI_TRY(beam_shape_check(dtype, C, nf, G, nb));
  return (int64_t)beam_scratch(nf, nb);
}

int qi_beam_music(int dtype, int device, const void* eigenvectors, int64_t C, int64_t nf, int64_t n_sources, const double* freq_hz,
                  const void* delays_s, int64_t G, const int64_t* band_first, int64_t nb, void* power, void* peak_index,
                  void* peak_value, void* scratch, int64_t scratch_bytes, qi_stream stream) {
  QI_TRY(beam_shape_check(dtype, C, nf, G, nb));
  QI_REQUIRE(n_sources >= 0 && n_sources < C, "%lld sources for %lld sensors: 0 to %lld", (long long)n_sources, (long long)C,
             (long long)(C - 1));
  return beam_form<SubspaceForm>(dtype, device, eigenvectors, C, nf, freq_hz, delays_s, G, band_first, nb, 0, (int)n_sources, power,
                                 peak_index, peak_value, scratch, scratch_bytes, stream);
}

}  // extern "C"
