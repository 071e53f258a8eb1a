/*
 * qi_windows.h -- C ABI of libqi_tfr.so, part seven: cross-spectral matrices per SLIDING WINDOW of segments, the time-resolved
 * form of qi_array.h.  One matrix per (window, bin) instead of one per bin for the whole record: the stack
 * [window][bin][C][C], window-major, is with the frequency table repeated per window and one band per (window, band) a valid
 * input of qi_beam_power, qi_csd_whiten + qi_beam_capon and qi_csd_eigh + qi_beam_music -- a detection timeline (back
 * azimuth, trace velocity, semblance per window and band) from one contraction launch and one form call.
 *
 * Everything of qi_tfr.h and qi_array.h holds here: caller-owned device pointers, asynchronous calls on the given stream
 * with no host synchronisation and no allocation, every refusal made before anything is launched, qi_last_error() for the
 * message (per thread); both calls are plan-less and may be made from several host threads at once (qi_csd_windows shares
 * the per-device hipFFT handles of qi_tfr.h's short-time family, locked inside).
 *
 * Windows.  nwin = (nseg - win) / hop + 1; window w holds the segments w hop .. w hop + win - 1.  A hop greater than win
 * leaves gaps; segments after the last window are ignored.  Only the bins bin_first .. bin_first + bin_count - 1 are formed.
 *
 * Contract on the results
 *  - csd[w][f][i][j] and coherence[w][f][i][j] equal BIT FOR BIT what qi_cross_spectra returns for a contiguous copy of
 *    Z[:, bin_first : bin_first + bin_count, w hop : w hop + win] with the same weights.  A segment at or past the window's
 *    end contributes nothing, whatever the panel holds there (NaN and Inf included).
 *  - Hence everything of qi_array.h: an entry is a function of its two records' `win` segments alone -- the same bits for
 *    any nseg, hop, bin range, window position and run; [j][i] is the exact conjugate of [i][j]; the diagonal is real
 *    (imaginary part +0); one segment per window (win = 1) gives coherence exactly 1 (NaN where an auto-power is 0 or not
 *    finite).
 *  - Every window is summed on its own from the panel, by qi_cross_spectra's multiply-add chains started at the window's
 *    first segment: no atomics, no partial sums shared between windows, no running add-new / subtract-old update (which would
 *    make a window depend on its predecessors and cancel catastrophically).
 */
#ifndef QI_WINDOWS_H
#define QI_WINDOWS_H

#include "qi_tfr.h"
#include "qi_array.h"

#ifdef __cplusplus
extern "C" {
#endif

/* S[w][f][i][j] = weight[f] * sum_{s = w hop}^{w hop + win - 1} conj(Z[i][bin_first + f][s]) * Z[j][bin_first + f][s]
 * Z: [C][nf][nseg] complex of `dtype`, as qi_cross_spectra takes it; weight: bin_count doubles on the HOST, one per FORMED
 * bin, or NULL (= 1), rounded to `dtype` before it multiplies the sum -- it reaches the device as kernel arguments, in stream
 * order: the array may be reused as soon as the call returns; csd: [nwin][bin_count][C][C] complex; coherence:
 * [nwin][bin_count][C][C] real; either may be NULL, not both.  scratch: caller-owned device buffer of
 * qi_cross_spectra_windows_scratch_bytes() (the weights, and the matrices when only the coherence is asked for), aligned to
 * 16.  Refused (the size query, host only, returns the negative qi_status): an unknown dtype; C, nf, nseg, win, hop or
 * bin_count below 1; win > nseg; a bin range that leaves 0..nf; more than 2^40 matrix entries; a grid that passes 2^31; and
 * by the call null or misaligned pointers and a short or misaligned scratch.  One launch for the matrices (a wave per
 * window, bin and group of 16 x 16 tiles of record pairs; windows adjacent in the grid, so overlapping windows find the
 * lines they share in cache), one for the coherence. */
int64_t qi_cross_spectra_windows_scratch_bytes(int dtype, int64_t C, int64_t nf, int64_t nseg, int64_t bin_first, int64_t bin_count,
                                               int64_t win, int64_t hop);
int qi_cross_spectra_windows(int dtype, int device, const void* Z, int64_t C, int64_t nf, int64_t nseg, int64_t bin_first,
                             int64_t bin_count, int64_t win, int64_t hop, const double* weight, void* csd, void* coherence,
                             void* scratch, int64_t scratch_bytes, qi_stream stream);

/* scipy.signal.csd / scipy.signal.coherence (qi_csd's conventions: segments of `seg` samples every `hop`, mean removed,
 * `window`, nfft, one-sided, average="mean") of the sub-record that each window of `win` consecutive segments, every win_hop
 * segments, spans.  Two steps: qi_csd's first step -- the unscaled coefficient panel [C][nfft / 2 + 1][n_seg], n_seg =
 * (n - seg) / hop + 1, into scratch -- then the windowed contraction over the bins bin_first .. bin_first + bin_count - 1
 * with weight = scale^2 / win, doubled for the bins 0 < f < nfft / 2 of the one-sided spectrum (every f > 0 when nfft is
 * odd) by their ABSOLUTE index.  sig: [C][n] real, window: [seg] real (device); csd: [nwin][bin_count][C][C] complex,
 * coherence: [nwin][bin_count][C][C] real, nwin = (n_seg - win) / win_hop + 1; either may be NULL, not both.  With win =
 * n_seg and all bins the result is qi_csd's bit for bit.  scratch: qi_csd_windows_scratch_bytes(), aligned to 16. */
int64_t qi_csd_windows_scratch_bytes(int dtype, int64_t C, int64_t n, int64_t seg, int64_t hop, int64_t nfft, int64_t bin_first,
                                     int64_t bin_count, int64_t win, int64_t win_hop);
int qi_csd_windows(int dtype, int device, const void* sig, int64_t C, int64_t n, const void* window, int64_t seg, int64_t hop,
                   int64_t nfft, double scale, int64_t bin_first, int64_t bin_count, int64_t win, int64_t win_hop, void* csd,
                   void* coherence, void* scratch, int64_t scratch_bytes, qi_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* QI_WINDOWS_H */
