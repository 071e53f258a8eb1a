/*
 * qi_beam.h -- C ABI of libqi_tfr.so, part three: what consumes the cross-spectral matrices of qi_array.h.
 *
 * Everything of qi_tfr.h holds here: its types and status codes, caller-owned device pointers, asynchronous calls on the
 * given stream with no host synchronisation and no allocation, qi_last_error() for the message (per thread).  The call is
 * plan-less and keeps no state: it may be made from several host threads at once, each on its own stream and buffers.  The
 * reference (quantum-inferno) has no array processing; the call below is the conventional (Bartlett) frequency-domain
 * beamformer over a grid of candidate delay sets -- for a plane wave, a grid of slowness vectors.
 *
 * Contract on the result
 *  - power[b][g] is a function of the band's matrices, their frequencies and row g of the delays alone: the same bits for any
 *    G, at any position in the grid, in any band table that holds the same band, and on any run.  There are no atomics; the
 *    sums run in `dtype` on the matrix cores (v_mfma_f32_16x16x4_f32, v_mfma_f64_16x16x4_f64) in an order that depends on C
 *    and the band's range of matrices alone;
 *  - the phase freq * tau is formed in double whatever `dtype` is, reduced to [-1/2, 1/2] turns in double, and the sine and
 *    cosine of the reduced turns are taken in `dtype` (sincospi): a phase that is an exact multiple of a quarter turn gives
 *    exactly +-1 and 0.  A matrix's factors come from its own frequency alone (no recurrence from bin to bin);
 *  - the quotient that normalises is formed in double from the finished sums and rounded once to `dtype`.
 */
#ifndef QI_BEAM_H
#define QI_BEAM_H

#include "qi_tfr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QI_BEAM_MAX_SENSORS 64 /* one matrix of float64 is 64 KiB of LDS */

/* Steered power of nf cross-spectral matrices over G delay sets, summed over nb bands of consecutive matrices.
 *   e[f][g][i] = exp(2 pi i freq_hz[f] delays_s[g][i])
 *   Q[f][g]    = Re sum_ij conj(e[f][g][i]) csd[f][i][j] e[f][g][j]      (csd as qi_cross_spectra / qi_csd write it:
 *                conj(X_i) X_j -- a plane wave that reaches sensor i later by tau_i gives Q = C^2 |X0|^2 at delays tau)
 *   normalize = 0: power[b][g] = (sum_{f in band b} Q[f][g]) / C^2
 *   normalize = 1: power[b][g] = sum_f Q[f][g] / (C sum_f tr csd[f])      (the semblance, in [0, 1] for Hermitian
 *                positive semi-definite matrices; NaN where the band's total auto-power is 0)
 * csd: [nf][C][C] complex of `dtype`, the whole matrix is read (one that is not Hermitian gives the real part of the form);
 * C <= QI_BEAM_MAX_SENSORS.  freq_hz: nf doubles on the HOST, the frequency of matrix f (any table: STFT bins, CWT bands).
 * delays_s: [G][C] DOUBLES on the device whatever `dtype` is, seconds.  band_first: nb + 1 strictly ascending offsets into
 * 0..nf on the HOST (band b holds the matrices band_first[b] .. band_first[b + 1] - 1), or NULL: every matrix its own band
 * (nb = nf).  Both host arrays reach the device as kernel arguments, in stream order: they may be reused as soon as the call
 * returns.  power: [nb][G] real of `dtype`.  peak_index: [nb] int64 or NULL, the index of the first maximum of power[b] --
 * of the first NaN if there is one (np.argmax); peak_value: [nb] real of `dtype` or NULL, that entry.
 * scratch: caller-owned device buffer of qi_beam_power_scratch_bytes() (the two host tables), aligned to 16.  The size query
 * is host only and gives the call's verdicts on the shape: a negative qi_status for an unknown dtype, C < 1 or
 * C > QI_BEAM_MAX_SENSORS, nf, G or nb below 1, nb above nf.  The call also refuses offsets that do not start inside 0..nf,
 * are not strictly ascending or end past nf, a NULL band_first with nb != nf, a NULL power, and scratch that is too small
 * or misaligned -- all before anything is launched.  One launch for the power (a workgroup per band and tile of grid
 * points), one for the peaks. */
int64_t qi_beam_power_scratch_bytes(int dtype, int64_t C, int64_t nf, int64_t G, int64_t nb);
int qi_beam_power(int dtype, int device, const void* csd, int64_t C, int64_t nf, const double* freq_hz, const void* delays_s,
                  int64_t G, const int64_t* band_first, int64_t nb, int normalize, void* power, void* peak_index,
                  void* peak_value, void* scratch, int64_t scratch_bytes, qi_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* QI_BEAM_H */
