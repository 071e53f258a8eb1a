/*
 * qi_bands.h -- C ABI of libqi_tfr.so, part nine: cross-spectral matrices of a CONSTANT-Q panel, every band in a window, hop
 * and sample stride of its own.  qi_windows.h gives every bin one window and one hop, which is right for an STFT; the bands
 * of a CWT or Stockwell panel [C][nb][n] span octaves, and array work on them (PMCC's band table, smoothed wavelet coherence)
 * wants a window proportional to the band's period.  One launch forms the matrices of every band; the ragged, band-major
 * stack [total][C][C] is, with the band's frequency repeated per window and every matrix its own band, a valid input of
 * qi_beam_power, qi_csd_whiten + qi_beam_capon and qi_csd_eigh + qi_beam_music.
 *
 * Everything of qi_tfr.h and qi_array.h holds here: caller-owned device pointers, asynchronous calls on the given stream
 * with no host synchronisation and no allocation, every refusal made before anything is launched, qi_last_error() for the
 * message (per thread); the calls are plan-less and may be made from several host threads at once.
 *
 * Geometry, per formed band b of band_first .. band_first + band_count - 1: three HOST tables of band_count int64 each,
 * terms[b] >= 1, stride[b] >= 1, hop[b] >= 1.  Window w of band b sums the samples w hop[b] + k stride[b], k = 0 ..
 * terms[b] - 1; its span is span[b] = (terms[b] - 1) stride[b] + 1 <= n; nwin[b] = (n - span[b]) / hop[b] + 1;
 * offset[0] = 0, offset[b + 1] = offset[b] + nwin[b], total = offset[band_count].  A hop greater than the span leaves gaps;
 * samples after a band's last window are ignored.  The stride is for the low bands, whose coefficients are oversampled by
 * orders of magnitude: it thins the sum, it does not average.
 *
 * Contract on the results
 *  - Matrix offset[b] + w of csd and of coherence equals BIT FOR BIT what qi_cross_spectra returns for a contiguous copy of
 *    Z[:, band_first + b : band_first + b + 1, w hop[b] : w hop[b] + span[b] : stride[b]] with the weight weight[b].
 *  - With stride[b] == 1, band b's block equals BIT FOR BIT qi_cross_spectra_windows(..., bin_first = band_first + b,
 *    bin_count = 1, win = terms[b], hop = hop[b]) with that weight.
 *  - Hence everything of qi_array.h: an entry is a function of its two records' sampled values, terms[b] and weight[b] alone
 *    -- the same bits for any n, band position, window position, neighbouring bands' geometry and run; [j][i] is the exact
 *    conjugate of [i][j]; the diagonal is real (imaginary part +0); a band of one term (terms[b] == 1) has coherence exactly
 *    1 (NaN where an auto-power is 0 or not finite).
 *  - A sample that no term reads never enters a sum, NaN and Inf included: the samples between strided terms, those in the
 *    gaps of a hop greater than the span, those past a band's last window, and the bands that are not formed.
 *  - Every window is summed on its own from the panel by qi_cross_spectra's multiply-add chains, term k where that call has
 *    segment k: no atomics, no partial sums shared between windows or split across waves, no running update.
 */
#ifndef QI_BANDS_H
#define QI_BANDS_H

#include "qi_tfr.h"
#include "qi_array.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host only: the offsets of the band-major stack.  Writes the band_count + 1 values offset[0 .. band_count] to offsets_out
 * (which may be NULL) and returns total, or the negative qi_status of a refused geometry: n or band_count below 1, a null
 * table, a table entry below 1, a span longer than n. */
int64_t qi_cross_spectra_bands_layout(int64_t n, int64_t band_count, const int64_t* terms, const int64_t* hop, const int64_t* stride,
                                      int64_t* offsets_out);

/* S[offset[b] + w][i][j] = weight[b] * sum_{k < terms[b]} conj(Z[i][band_first + b][w hop[b] + k stride[b]]) *
 *                                                              Z[j][band_first + b][w hop[b] + k stride[b]]
 * Z: [C][nb][n] complex of `dtype` (device); terms, hop, stride: band_count int64 each on the HOST; weight: band_count
 * doubles on the HOST, one per FORMED band, or NULL (= 1), rounded to `dtype` before it multiplies the sum.  The host arrays
 * reach the device as kernel arguments, in stream order: they may be reused as soon as the call returns.  csd:
 * [total][C][C] complex; coherence: [total][C][C] real; either may be NULL, not both.  scratch: caller-owned device buffer
 * of qi_cross_spectra_bands_scratch_bytes() (the tables, the weights, and the matrices when only the coherence is asked
 * for), aligned to 16.  Refused (the size query, host only, returns the negative qi_status, with the verdict and the message
 * of the call): an unknown dtype; C, nb, n or band_count below 1; a band range that leaves 0..nb; a null table; a table entry
 * below 1; a span longer than n; more than 2^40 matrix entries; a grid that passes 2^31; and by the call null or misaligned
 * pointers and a short or misaligned scratch.  One launch for the matrices (a wave per matrix and group of 16 x 16 tiles of
 * record pairs, the four waves of a workgroup on four consecutive matrices of the stack: adjacent windows of a band find the
 * lines they share in cache), one for the coherence -- one per run of bands on the same side of terms == 1 where bands of
 * one term are mixed with longer ones. */
int64_t qi_cross_spectra_bands_scratch_bytes(int dtype, int64_t C, int64_t nb, int64_t n, int64_t band_first, int64_t band_count,
                                             const int64_t* terms, const int64_t* hop, const int64_t* stride);
int qi_cross_spectra_bands(int dtype, int device, const void* Z, int64_t C, int64_t nb, int64_t n, int64_t band_first,
                           int64_t band_count, const int64_t* terms, const int64_t* hop, const int64_t* stride, const double* weight,
                           void* csd, void* coherence, void* scratch, int64_t scratch_bytes, qi_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* QI_BANDS_H */
