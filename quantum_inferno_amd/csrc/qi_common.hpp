// Shared helpers for libqi_tfr.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <hipfft/hipfft.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "qi_tfr.h"

namespace qi {

void set_error(const char* fmt, ...);
const char* tune_env(const char* name);  // development switch (read only when QI_TUNE is set; qi_api.hip)

#define QI_HIP(call)                                                                        \
  do {                                                                                      \
    hipError_t e_ = (call);                                                                 \
    if (e_ != hipSuccess) {                                                                 \
      ::qi::set_error("%s:%d %s -> %s", __FILE__, __LINE__, #call, hipGetErrorString(e_)); \
      return QI_ERR_HIP;                                                                    \
    }                                                                                       \
  } while (0)

#define QI_FFT(call)                                                              \
  do {                                                                            \
    hipfftResult r_ = (call);                                                     \
    if (r_ != HIPFFT_SUCCESS) {                                                   \
      ::qi::set_error("%s:%d %s -> hipfft %d", __FILE__, __LINE__, #call, (int)r_); \
      return QI_ERR_FFT;                                                          \
    }                                                                             \
  } while (0)

#define QI_TRY(call)        \
  do {                      \
    int s_ = (call);        \
    if (s_ != QI_OK) return s_; \
  } while (0)

#define QI_REQUIRE(cond, ...)       \
  do {                              \
    if (!(cond)) {                  \
      ::qi::set_error(__VA_ARGS__); \
      return QI_ERR_ARG;            \
    }                               \
  } while (0)

template <typename T>
struct c2;
template <>
struct c2<float> {
  using type = float2;
};
template <>
struct c2<double> {
  using type = double2;
};
template <typename T>
using cplx = typename c2<T>::type;

template <typename T>
__host__ __device__ inline cplx<T> mk(T re, T im) {
  cplx<T> v;
  v.x = re;
  v.y = im;
  return v;
}
template <typename C>
__host__ __device__ inline C cmul(C a, C b) {
  C r;
  r.x = a.x * b.x - a.y * b.y;
  r.y = a.x * b.y + a.y * b.x;
  return r;
}

// Allow kernel `fn` `bytes` of dynamic LDS on the CURRENT device.  hipFuncSetAttribute acts on the current device's
// function object only, so the raised limits are kept per (device, function); a request above what the device offers
// returns QI_ERR_UNSUPPORTED instead of a launch error (qi_kernels.hip).
int allow_dynamic_lds(const void* fn, size_t bytes);

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
inline bool is_pow2(int64_t v) { return v > 0 && (v & (v - 1)) == 0; }
inline int64_t next_pow2(int64_t v) {
  int64_t p = 1;
  while (p < v) p <<= 1;
  return p;
}

// Time samples one epilogue workgroup owns (256 threads x 4 consecutive samples).
constexpr int kEpiThreads = 256;
constexpr int kEpiVec = 4;
constexpr int kEpiSpan = kEpiThreads * kEpiVec;

// ---- launchers implemented in qi_kernels.hip (all asynchronous on `st`) ------------------------
template <typename T>
int launch_pack_pad(const T* sig, cplx<T>* X, int64_t C, int64_t n, int64_t L, hipStream_t st);

int launch_bank_rows(double2* rows, int64_t n, int64_t L, int circular, const double* p_re, const double* p_im,
                     const double* omega, const double* amp, int j0, int nb, hipStream_t st, double taper_e = 0.0,
                     const double* xs = nullptr);
template <typename T>
int launch_bank_convert(const double2* F, cplx<T>* bank, int64_t count, int conj, double scale, hipStream_t st);

template <typename T>
int launch_mul_bank(const cplx<T>* X, const cplx<T>* H, cplx<T>* Y, int64_t Ct, int64_t Bt, int64_t L, hipStream_t st);
template <typename T>
int launch_stx_window(const cplx<T>* X, cplx<T>* Y, int64_t Ct, int64_t Bt, int64_t n, const int64_t* idx,
                      const double* coef, hipStream_t st);

template <typename T>
struct EpiArgs {
  const cplx<T>* Y;  // [Ct][Bt][L]
  int64_t L, n, off; // out[t] = Y[(t + off) mod L]
  int64_t Ct, Bt;    // tile extents
  int64_t B;         // bands in the whole panel
  int64_t j0;        // first band of this tile
  cplx<T>* coef;     // [Ct][B][n] (already offset to the tile's first channel) or null
  T* bits;           // idem
  T* power_time;     // [Ct][n] or null
  double* part_band; // [Ct][B][nblk] or null
  double* part_stat; // [Ct][ntile_b][nblk][3] or null
  int64_t tile_b;    // index of this band tile
  int64_t ntile_b;
  T power_scale;
  T eps;
};
template <typename T>
int launch_epilogue(const EpiArgs<T>& a, hipStream_t st);
// the inverse of the ShortTimeFFT-convention transform on hipFFT (qi_stft_hipfft.hip)
template <typename T>
int launch_sliding_untranspose(const cplx<T>* S, cplx<T>* F, int64_t C, int64_t nseg, int64_t nf, hipStream_t st);
template <typename T>
int launch_sliding_overlap_add(const T* slices, const T* dual, T* out, int64_t C, int64_t k0, int64_t k1, int64_t seg,
                               int64_t hop, int64_t nfft, int64_t nseg, int64_t first, int64_t roll, hipStream_t st);

// 1-D Shannon family (qi_shannon1d.hip)
int64_t shannon_spans(int64_t n);
template <typename T>
int launch_shannon_1d(const T* m, int64_t C, int64_t n, T* info, T* entropy, T* isnr, T* esnr, hipStream_t st);
template <typename T>
int launch_tdr_marginal(const T* sig, int64_t C, int64_t n, T* sig_norm, T* marginal, double* partial, hipStream_t st);
template <typename T>
int launch_fft_marginal(const cplx<T>* X, int64_t C, int64_t nf, T* angle, T* marginal, double* partial, int32_t* turns,
                        hipStream_t st);

int launch_finalize(const double* part_band, const double* part_stat, double* power_band, double* stats, int64_t C,
                    int64_t B, int64_t nblk, int64_t nstat, hipStream_t st, const int32_t* band_slots = nullptr);

// fused STFT (qi_stft_fused.hip): frames, transform and [frequency][time] store in one kernel
bool stft_fused_supported(int dtype, int64_t seg, int64_t hop, int64_t nfft);
// segment groups (workgroups) per record of a fused launch; 0: the transform length has no fused shape
// (pool_factor > 0: of a launch that pools windows of that many segments)
int64_t stft_fused_groups(int dtype, int64_t nfft, int64_t nseg, int64_t pool_factor = 0);
// One forward call of the family, on either engine.  The mode fields default to qi_stft's own call (zeros past the record,
// segment mean removed, coefficient and log2-bits panels); Welch, the ShortTimeFFT convention and the reductions set only what
// they mean.  (The hipFFT engine reads the geometry, scale, eps and the ShortTimeFFT fields; its reductions are kernels of
// their own on the panel.)
struct StftRequest {
  int64_t C, n, seg, hop, nfft, nseg;
  // samples of extension in front of the record (seg / 2 for the STFT, 0 Welch, -first sliding; a segment range: the signed
  // origin seg / 2 + sample0 - first_segment hop, `n` the samples a row holds and `nseg` the range's segments)
  int64_t lead;
  double scale = 1.0, eps = 0.0;
  // Welch: [C][groups][nfft / 2 + 1] doubles of scratch for the groups' sums of |X|^2 (groups = stft_fused_groups()); no panel
  double* welch_part = nullptr;
  // scipy.signal.ShortTimeFFT's convention (qi_sliding_stft): record extension past its ends (0 zeros, 1 edge, 2 / 3 even / odd
  // reflection), mean removal, left rotation of the slice, what the real output holds (0 log2 bits, 1 |X|, 2 |X|^2)
  int32_t pad_mode = 0, detrend = 1, real_kind = 0;
  int64_t roll = 0;
  // reductions of the panel from the kernel's registers (qi_stft_out), asked for by power_band: part_band [C][groups][nfft / 2 + 1]
  // and part_stat [C][groups][3] doubles of scratch; power_band [C][nfft / 2 + 1] and stats [C][4] float64, power_time [C][nseg]
  // in the record's precision or null.  Z and bits may then be null (no panel is stored).
  double *part_band = nullptr, *part_stat = nullptr;
  void* power_time = nullptr;
  double *power_band = nullptr, *stats = nullptr;
  double power_scale = 1.0;
  int64_t row_stride = -1;  // samples between the rows of `sig`; < 0: n
  // time pooling of P from the reductions form's registers (qi_stft_out_range): windows of pool_factor consecutive segments,
  // pool_mean / pool_max [C][nfft / 2 + 1][nseg / pool_factor] in the record's precision (either may be null); part_max
  // [C][groups][nfft / 2 + 1] of the record's type beside part_band.  The workgroups then hold min(launch group, largest
  // power of two dividing pool_factor) segments, so that each lies inside one window (stft_fused_groups with the factor).
  int64_t pool_factor = 0;
  void *pool_mean = nullptr, *pool_max = nullptr, *part_max = nullptr;
};
template <typename T>
int launch_stft_fused(const StftRequest& rq, const T* sig, const T* win, cplx<T>* Z, T* bits, hipStream_t st);
// fused inverse of the ShortTimeFFT-convention transform (QI_ERR_UNSUPPORTED, with no error text, where it does not apply)
template <typename T>
int launch_istft_fused(const cplx<T>* S, const T* dual, T* out, int64_t C, int64_t seg, int64_t hop, int64_t nfft, int64_t first,
                       int64_t nseg, int64_t roll, int64_t k0, int64_t k1, hipStream_t st);
// Welch mean on the fused kernel (`part`: [C][stft_fused_groups()][nfft / 2 + 1] doubles of scratch; rq.scale: 1 / sum(window))
template <typename T>
int launch_welch_fused(const StftRequest& rq, const T* sig, const T* win, T* pxx, double* part, hipStream_t st);
// the hipFFT engine's forward kernels (qi_stft_hipfft.hip).  frames [C][nseg][nfft]: the request's segments (extension,
// mean removal, window, roll); F [C][nseg][nfft / 2 + 1] spectra -> rq.scale F as [C][nfft / 2 + 1][nseg] in Z and / or
// its real panel by rq.real_kind in R (either may be null), or -> Welch's mean pxx [C][nfft / 2 + 1]
template <typename T>
int launch_hipfft_frames(const StftRequest& rq, const T* sig, const T* win, T* frames, hipStream_t st);
template <typename T>
int launch_hipfft_transpose(const StftRequest& rq, const cplx<T>* F, cplx<T>* Z, T* R, hipStream_t st);
template <typename T>
int launch_welch_mean(const StftRequest& rq, const cplx<T>* F, T* pxx, hipStream_t st);

// cross-spectra of a panel (qi_csd.hip; include/qi_array.h).  The weight of bin f: table[f] (a DEVICE array) when there is
// one, else `paired` for the bins a one-sided spectrum doubles (0 < f, and f < nfft / 2 for an even nfft) and `edge` for the rest
struct CsdWeight {
  const double* table = nullptr;
  double edge = 1.0, paired = 1.0;
  int64_t nfft = 0;
};
// bytes of launch_cross_spectra's scratch: nf doubles (a caller's weights) | [nf][C][C] complex (the matrices when csd is null)
size_t cross_spectra_scratch(int dtype, int64_t C, int64_t nf);
// Z [C][nf][nseg] -> csd [nf][C][C] and / or coherence [nf][C][C] (either may be null); `matrices`: the second region of the scratch
template <typename T>
int launch_cross_spectra(const cplx<T>* Z, int64_t C, int64_t nf, int64_t nseg, const CsdWeight& w, cplx<T>* csd, T* coherence,
                         void* matrices, hipStream_t st);
// the windowed form (include/qi_windows.h): csd / coherence [nwin][bin_count][C][C], nwin = (nseg - win) / hop + 1; w.table
// holds one weight per FORMED bin, w.edge / w.paired go by the absolute bin.  Scratch: bin_count doubles | the matrices
size_t cross_spectra_windows_scratch(int dtype, int64_t C, int64_t bin_count, int64_t nwin);
template <typename T>
int launch_cross_spectra_windows(const cplx<T>* Z, int64_t C, int64_t nf, int64_t nseg, int64_t bin_first, int64_t bin_count, int64_t win,
                                 int64_t hop, const CsdWeight& w, cplx<T>* csd, T* coherence, void* matrices, hipStream_t st);
// pair correlations and their peaks from a stack of matrices (qi_lags.hip; include/qi_lags.h): csd [nstack][nfft / 2 + 1][C][C]
// -> cc [nstack][npair][2 max_lag + 1], peak_lag and peak_value [nstack][npair] (any may be null); the arguments are the
// checked ones of qi_pair_lags.  One launch, a workgroup per (stack, pair), no scratch.
template <typename T>
int launch_pair_lags(const cplx<T>* csd, int64_t nstack, int64_t C, int64_t nfft, int64_t bin_lo, int64_t bin_hi, int weighting,
                     int halve_interior, int normalize, int64_t upsample, int64_t max_lag, T* cc, T* peak_lag, T* peak_value,
                     hipStream_t st);

// delay-and-sum in the time domain (qi_timebeam.hip; include/qi_timebeam.h); the arguments are the checked ones of
// qi_time_beam_power and qi_time_beam_traces.  How the power call cuts the record: `count` units of `len` samples a hop
// apart, window w the sum of the units w .. w + per_window - 1; its scratch `sums` is [count][G][2] of the records' type.
struct TimeBeamUnits {
  int64_t nwin, len, per_window, count;
};
TimeBeamUnits time_beam_units(int64_t n, int64_t win, int64_t hop);
int64_t time_beam_row_blocks(int64_t rows);  // workgroups across the delay rows
int64_t time_beam_chunks(int64_t n);         // workgroups of the traces call along time
template <typename T>
int launch_time_beam_power(const T* x, int64_t C, int64_t n, const T* taps, int64_t P, int64_t T_taps, const int32_t* shift,
                           const int32_t* phase, int64_t G, int64_t max_shift, int64_t win, int64_t hop, int normalize, T* power,
                           int64_t* peak_index, T* peak_value, T* sums, hipStream_t st);
template <typename T>
int launch_time_beam_traces(const T* x, int64_t C, int64_t n, const T* taps, int64_t P, int64_t T_taps, const int32_t* shift,
                            const int32_t* phase, int64_t K, int64_t max_shift, T* out, hipStream_t st);

// synchrosqueezing (qi_squeeze.hip; include/qi_squeeze.h); the arguments are the checked ones of the three calls.  The
// tables lie in the caller's scratch, rounded to the panel's type: byte offsets from `base` of edges [nbin + 1], carrier
// [nb] and weight [nb].  launch_tfr_squeeze with a null ifreq forms the frequencies itself (the fused call).
struct SqueezeTables {
  const void* base;
  size_t edges, carrier, weight;
};
int64_t squeeze_tiles(int64_t n);  // workgroups along time
template <typename T>
int launch_tfr_ifreq(const cplx<T>* Z, int64_t C, int64_t nb, int64_t n, const SqueezeTables& tb, double rate, double floor, T* ifreq,
                     hipStream_t st);
template <typename T>
int launch_tfr_squeeze(const cplx<T>* Z, const T* ifreq, int64_t C, int64_t nb, int64_t n, int64_t nbin, const SqueezeTables& tb,
                       double rate, double floor, cplx<T>* out, hipStream_t st);

template <typename T>
int launch_power_marginals(const T* P, int64_t C, int64_t B, int64_t n, T* power_time, double* part_band,
                           double* part_stat, hipStream_t st);
template <typename T>
int launch_log2_offset(const T* in, T* out, int64_t C, int64_t count, T eps, const double* ref, hipStream_t st);
int launch_widen(const float* in, double* out, int64_t count, hipStream_t st);
template <typename T>
int launch_log2_abs(const T* in, int is_complex, T* out, int64_t count, T eps, hipStream_t st);
template <typename T>
int launch_shannon(const T* P, const T* mult, int mode, int64_t C, int64_t B, int64_t n, double deg, T* info, T* sb,
                   T* isnr, T* esnr, hipStream_t st);

}  // namespace qi
