/*
 * qi_lags.h -- C ABI of libqi_tfr.so, part eight: TIME DELAYS BETWEEN SENSORS from the cross-spectral matrices of qi_array.h
 * and qi_windows.h.  The generalized cross-correlation (plain, PHAT or SCOT weighted) of every pair of records, its lag
 * window, and the sub-sample position and height of its peak -- the input of a least-squares slowness fit (the PMCC / TDOA
 * family), with no slowness grid -- in ONE launch: a workgroup per (stack, pair) gathers the pair's bins, weights them in
 * registers, transforms them in LDS and reduces the window; the correlation never reaches device memory beyond the window
 * asked for.
 *
 * Everything of qi_tfr.h and qi_array.h holds here: caller-owned device pointers, an asynchronous call on the given stream
 * with no host synchronisation and no allocation, every refusal made before anything is launched, qi_last_error() for the
 * message (per thread); the call is plan-less and may be made from several host threads at once.
 *
 * Input.  csd: [nstack][nf][C][C] complex of `dtype`, nf = nfft / 2 + 1 -- the layout of qi_csd and qi_cross_spectra
 * (nstack = 1) and of the windowed calls with all bins (nstack = windows).  Only entries [i][j] with i <= j are read, and of
 * a diagonal entry only the real part.
 *
 * Pairs.  Every i < j, row-major: p = i C - i (i + 1) / 2 + (j - i - 1), npair = C (C - 1) / 2.
 *
 * Per bin.  X[f] = S_ij[f] W[f] h[f] for bin_lo <= f < bin_hi and 0 elsewhere, with
 *   weighting 0:        W = 1;
 *   weighting 1 (PHAT): W = 1 / |S_ij|, 0 where |S_ij| = 0;
 *   weighting 2 (SCOT): W = 1 / (sqrt(S_ii) sqrt(S_jj)), 0 where either auto-power is 0;
 *   h[f] = 0.5 for 0 < f < nfft / 2 when halve_interior != 0 (exact: it undoes the one-sided doubling of qi_csd's weights, so
 *   that weighting 0 gives the two-sided correlation), 1 otherwise.
 * The weights are formed in double and X is rounded once to `dtype`.
 *
 * Transform.  L = nfft upsample, a power of two, 64 <= L <= 8192, upsample in {1, 2, 4, 8}.  With m[f] the multiplicity of
 * bin f in the two-sided spectrum of length L (1 for f = 0 and f = L / 2, 2 otherwise) and Re' dropping the imaginary parts
 * of bins 0 and L / 2 as numpy.fft.irfft does,
 *   R[l] = sum_f m[f] Re'(X[f] exp(2 pi i f l / L)) = L irfft(X zero-padded to L / 2 + 1 bins, n = L)[l],
 *   r[l] = R[l] / nfft                                   (normalize = 0: irfft(..) upsample),
 *   r[l] = R[l] / sqrt(sum_f m[f] a_i[f]  sum_f m[f] a_j[f])   (normalize != 0, weighting 0; a_i[f] = S_ii[f] h[f] in the band:
 *          the product of the two zero-lag auto-correlations -- r is the correlation coefficient),
 *   r[l] = R[l] / sum_f m[f] [W[f] != 0]                 (normalize != 0, PHAT and SCOT: the count of non-zero two-sided bins
 *          of the band; a PHAT peak is then at most 1).
 * A divisor of 0 (an empty band) gives NaN.  The sums run in double in an order fixed by L alone; r is rounded once to `dtype`.
 *
 * Sign.  With S_ij = conj(X_i) X_j (qi_array.h), r[l] peaks at positive l when record j lags record i: the lag of a plane
 * wave is tau_j - tau_i of plane_wave_delays.
 *
 * Outputs (any may be NULL, not all).
 *   cc          [nstack][npair][2 max_lag + 1] real: r at the lags -max_lag .. +max_lag, in samples of the finer grid (1 /
 *               upsample of a record's), taken circularly (lag -l is r[L - l]); 0 <= max_lag <= L / 2 - 1.
 *   peak_lag    [nstack][npair] real, in samples of the RECORDS: the first maximum of the window in lag order (numpy.argmax's
 *               rule) at lag l0, refined by the parabola through b = r[l0] and its neighbours a = r[l0 - 1], c = r[l0 + 1] --
 *               taken circularly from the full r, so they exist at +-max_lag too: delta = 0.5 (a - c) / (a - 2 b + c), 0
 *               where the denominator is 0; peak_lag = (l0 + delta) / upsample.
 *   peak_value  [nstack][npair] real: the parabola's vertex b - 0.25 (a - c) delta.
 * The parabola is formed in double from the rounded a, b, c and rounded once.
 *
 * Contract on the results
 *  - The three outputs of (stack, pair) are a function of that pair's entries S_ij -- and S_ii, S_jj where the weighting or
 *    the normalisation reads them -- in [bin_lo, bin_hi) and of the scalar arguments alone: the same bits for any nstack, C,
 *    position in the stack and run.  An entry outside the band is never looked at (NaN and Inf included).
 *  - A (stack, pair) whose band holds a non-finite value among the entries it reads gives NaN in all three outputs and
 *    disturbs no other pair.
 *  - No atomics; every output element has one writer.
 */
#ifndef QI_LAGS_H
#define QI_LAGS_H

#include "qi_tfr.h"
#include "qi_array.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QI_LAG_PLAIN 0
#define QI_LAG_PHAT 1
#define QI_LAG_SCOT 2

/* The call needs no scratch today: the query (host only) returns 0 for a request the call takes and the negative qi_status
 * for one it refuses.  Refused: an unknown dtype; nstack below 1 or C below 2 (one record has no pair); nfft or upsample not as above;
 * more than 2^31 - 1 workgroups (nstack npair); more than 2^40 entries in csd; and by the call an unknown weighting, a bin
 * range that leaves 0 .. nfft / 2 + 1 or is reversed (bin_lo = bin_hi is an empty band), max_lag outside 0 .. L / 2 - 1, null
 * csd, no output, misaligned pointers, a scratch_bytes below the query's answer.  scratch may be NULL. */
int64_t qi_pair_lags_scratch_bytes(int dtype, int64_t nstack, int64_t C, int64_t nfft, int64_t upsample);
int qi_pair_lags(int dtype, int device, const void* csd, int64_t nstack, int64_t C, int64_t nfft, int64_t bin_lo, int64_t bin_hi,
                 int weighting, int halve_interior, int normalize, int64_t upsample, int64_t max_lag, void* cc, void* peak_lag,
                 void* peak_value, void* scratch, int64_t scratch_bytes, qi_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* QI_LAGS_H */
