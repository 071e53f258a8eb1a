/*
 * qi_array.h -- C ABI of libqi_tfr.so, part two: operations ACROSS the records of a batch (a sensor array's channels).
 *
 * Everything of qi_tfr.h holds here: its types and status codes, caller-owned device pointers, asynchronous calls on the
 * given stream with no host synchronisation and no allocation, qi_last_error() for the message (per thread).  Both calls are
 * plan-less: they may be made from several host threads at once, each on its own stream and buffers (qi_csd shares the
 * per-device hipFFT handles of qi_tfr.h's short-time family, locked inside).  The reference
 * (quantum-inferno) has no cross-channel product; the calls below restate scipy.signal.csd and scipy.signal.coherence,
 * the siblings of the scipy.signal.welch call behind styx_fft.welch_power_pow2 (styx_fft.py:230-266).
 *
 * Contract on the results (both calls, csd and coherence alike)
 *  - an entry [f][i][j] with i <= j is a function of the records i and j alone: the same bits in any batch, at any
 *    position in the batch and on any run.  The sums over the segments are formed in the records' precision on the matrix
 *    cores (v_mfma_f32_16x16x4_f32: a float32 fused-multiply-add chain; v_mfma_f64_16x16x4_f64), in an order that depends
 *    on n_seg alone;
 *  - [f][j][i] is the conjugate of [f][i][j] bit for bit (the coherence: the same bits);
 *  - the imaginary part of csd[f][i][i] is exactly 0, its real part is >= 0 for weights >= 0;
 *  - coherence[f][i][j] = |S_ij|^2 / (S_ii S_jj), the quotient formed in double and rounded once to the records' type.  A
 *    bin whose auto-power is 0 gives NaN, as SciPy's division does.  With ONE segment the estimate is the identity
 *    |conj(a) b|^2 = |a|^2 |b|^2, and the call returns what that identity gives and rounding would blur: exactly 1 (NaN
 *    where an auto-power is 0 or not finite).
 */
#ifndef QI_ARRAY_H
#define QI_ARRAY_H

#include "qi_tfr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* S[f][i][j] = weight[f] * sum_s conj(Z[i][f][s]) * Z[j][f][s]            (scipy.signal.csd's convention: conj(X) Y)
 * Z: [C][nf][nseg] complex of `dtype`, s contiguous (the panel layout of qi_stft, qi_cwt and qi_stx: [channel][band][time]);
 * weight: nf doubles on the HOST or NULL (= 1), rounded to `dtype` before it multiplies the sum -- it reaches the device
 * as kernel arguments, in stream order: the array may be reused as soon as the call returns;
 * csd: [nf][C][C] complex, one Hermitian matrix per bin; coherence: [nf][C][C] real, |S_ij|^2 / (S_ii S_jj); either may be
 * NULL, not both.  scratch: caller-owned device buffer of qi_cross_spectra_scratch_bytes() (the weights, and the matrices
 * when only the coherence is asked for), aligned to 16; the size query is host only and returns a negative qi_status for
 * an unknown dtype, a shape below 1 or one whose matrices pass 2^40 entries.  One launch for the matrices (a wave per bin
 * and 16 x 16 tile of record pairs, tiles on and above the diagonal only), one for the coherence. */
int64_t qi_cross_spectra_scratch_bytes(int dtype, int64_t C, int64_t nf, int64_t nseg);
int qi_cross_spectra(int dtype, int device, const void* Z, int64_t C, int64_t nf, int64_t nseg, const double* weight,
                     void* csd, void* coherence, void* scratch, int64_t scratch_bytes, qi_stream stream);

/* scipy.signal.csd(x_i, x_j, window, nperseg=seg, noverlap=seg-hop, nfft, detrend="constant", return_onesided=True,
 * average="mean") for every pair of the C records: qi_welch's segments (no extension, no padding, mean removed), `scale` as
 * qi_welch's (1 / sum(window) for scaling="spectrum", sqrt(1 / (fs sum(window^2))) for "density"); and scipy.signal.coherence
 * of the same segments.  sig: [C][n] real, window: [seg] real (device); csd: [nfft/2+1][C][C] complex, coherence:
 * [nfft/2+1][C][C] real, either may be NULL, not both.  Two steps: the unscaled coefficient panel of the segments
 * [C][nfft/2+1][n_seg], n_seg = (n - seg) / hop + 1, into scratch (the fused kernel at its transform lengths, frames ->
 * hipFFT -> transpose elsewhere), then qi_cross_spectra's kernels on it with weight[f] = scale^2 / n_seg, doubled for the
 * bins 0 < f < nfft/2 of the one-sided spectrum (every f > 0 when nfft is odd).  scratch: qi_csd_scratch_bytes(), aligned
 * to 16. */
int64_t qi_csd_scratch_bytes(int dtype, int64_t C, int64_t n, int64_t seg, int64_t hop, int64_t nfft);
int qi_csd(int dtype, int device, const void* sig, int64_t C, int64_t n, const void* window, int64_t seg, int64_t hop,
           int64_t nfft, double scale, void* csd, void* coherence, void* scratch, int64_t scratch_bytes, qi_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* QI_ARRAY_H */
