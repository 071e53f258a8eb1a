/*
 * qi_squeeze.h -- C ABI of libqi_tfr.so, part eleven: SYNCHROSQUEEZING of a constant-Q panel.  The instantaneous frequency of
 * every coefficient of a CWT or Stockwell panel is estimated from the panel's own phase (the forward difference along time),
 * and the coefficient is moved to the frequency bin where that estimate lies: reassignment along frequency, column by
 * column.  qi_tfr_ifreq gives the estimates, qi_tfr_squeeze moves a panel by estimates it is handed, qi_tfr_synchrosqueeze
 * does both in one pass over the panel, with no [C][nb][n] intermediate in device memory.
 *
 * Everything of qi_tfr.h and qi_array.h holds here: caller-owned device pointers, asynchronous calls on the given stream with
 * no host synchronisation and no allocation, every refusal made before anything is launched, qi_last_error() for the message
 * (per thread); the calls are plan-less and may be made from several host threads at once.
 *
 * Common definitions
 *   Z        [C][nb][n] complex of `dtype` (QI_F32 or QI_F64), time contiguous: the layout the plans store and
 *            qi_cross_spectra_bands reads.  n >= 2.
 *   carrier_hz  nb doubles on the HOST or NULL (= 0): the frequency at which band b's coefficients have been demodulated.  A
 *            CWT panel turns at the signal's own frequency: 0.  A Stockwell panel whose band b was shifted by idx[b] bins of an
 *            n-point spectrum turns at f - idx[b] sample_rate / n: the carrier is that SNAPPED bin frequency, not the band's
 *            nominal centre.
 *   edges_hz nbin + 1 doubles on the HOST, 1 <= nbin <= QI_SQUEEZE_MAX_BINS: the bins' edges.
 *   weight   nb doubles on the HOST or NULL (= 1): a factor per band.
 *   Every host value is rounded to `dtype` once, before it is checked or used; all arithmetic is in `dtype`, every product and
 *   sum rounded on its own (no fused multiply-add).  The host arrays reach the device as kernel arguments, in stream order:
 *   they may be reused as soon as the call returns.
 *   scratch  caller-owned device buffer of qi_tfr_squeeze_scratch_bytes() bytes, aligned to 16: the tables.
 *
 * The frequency of element (c, b, t).  Its partner is the column u = t + 1; the last column, t = n - 1, takes u = n - 2 with the
 * roles swapped, so that the difference is always later times conj(earlier):
 *   d     = Z[later] conj(Z[earlier])          re d = lr er + li ei,  im d = li er - lr ei
 *   ifreq = carrier[b] + (rate * atan2(im d, re d)) * (1 / (2 pi))      (1 / (2 pi) rounded to `dtype`)
 * The element is VALID iff p_t >= floor && p_t < inf && p_u >= floor && p_u < inf, with p = re^2 + im^2 in `dtype`: a NaN
 * fails every comparison, and a power that overflows `dtype` counts as not finite although the coefficient is finite (in
 * float32 a modulus above 1.8e19).  An element that is not valid has the frequency NaN.
 *
 * The bin of a frequency f: k(f) = (number of edges <= f) - 1, compared in `dtype`; the element lands in bin k iff
 * 0 <= k < nbin.  Bins are right-open: f == edges[nbin] is dropped, and so are NaN and both infinities.
 *
 *   out[c][k][t] = sum over the bands b whose element (c, b, t) lands in k of weight[b] Z[c][b][t]
 * per component: each product is rounded, THEN added; the terms are added in ascending b, starting from +0.  Every element
 * of out is written, zeros where nothing lands: the caller clears nothing.
 *
 * Contract on the results
 *  - ifreq[c][b][t] depends on the two coefficients of columns t and its partner in band b of record c, carrier[b], the rate
 *    and the floor alone.
 *  - out[c][k][t] depends on columns t and its partner of record c, on the tables and on `dtype` alone: the same bits for any
 *    C, any position of the record in the batch, any position of the column in a tile of the kernel and any run, and the same bits in any longer panel that holds the same two columns side by side (the last column of a
 *    panel excepted: its partner lies before it).
 *  - qi_tfr_synchrosqueeze equals qi_tfr_ifreq followed by qi_tfr_squeeze BIT FOR BIT: both run the same two device
 *    functions, one for the frequency and one for the bin.
 *  - No atomics: a column of a record has one lane that owns it, and that lane adds the bands in their order.
 *  - A coefficient that is not moved (not valid, or out of the edges' range) enters nothing, NaN and Inf included.  A
 *    coefficient that is moved enters by IEEE arithmetic: a NaN or an infinite component that lands poisons its bin.
 *
 * Out of scope: STFT panels (a hop above one sample aliases the phase difference), the derivative-wavelet estimator,
 * reconstruction weights and the inverse, penalised ridge tracking, reassignment along time, streamed records.
 */
#ifndef QI_SQUEEZE_H
#define QI_SQUEEZE_H

#include "qi_tfr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QI_SQUEEZE_MAX_BINS 4096
/* the band tables ride in kernel arguments, 2 KiB a launch: a bound on the bands keeps that short */
#define QI_SQUEEZE_MAX_BANDS 65536
/* columns of a record one workgroup takes, a lane per column */
#define QI_SQUEEZE_TILE 256

/* Bytes of scratch the three calls need (host only); the negative qi_status, with the message set, for a shape they refuse:
 * an unknown dtype; C, nb or nbin below 1; n below 2; nbin above QI_SQUEEZE_MAX_BINS; nb above QI_SQUEEZE_MAX_BANDS; more than
 * 2^40 elements in the panel or in the result; more than 2^31 - 1 workgroups (C nb ceil(n / QI_SQUEEZE_TILE)).  qi_tfr_ifreq has no nbin: it needs the
 * answer for nbin = 1, and takes any larger scratch. */
int64_t qi_tfr_squeeze_scratch_bytes(int dtype, int64_t C, int64_t nb, int64_t n, int64_t nbin);

/* ifreq [C][nb][n] real of `dtype`.  Refused: what the size query refuses; a carrier that is not finite; a rate that is not
 * finite or not above 0 (as rounded); a power_floor that is negative, NaN or (as rounded) infinite; null Z or scratch; a null
 * ifreq ("nothing to produce"); misaligned pointers (Z: the complex element; ifreq: the element; scratch: 16); a short
 * scratch.  One launch behind the tables', a thread per element. */
int qi_tfr_ifreq(int dtype, int device, const void* Z, int64_t C, int64_t nb, int64_t n, const double* carrier_hz,
                 double sample_rate_hz, double power_floor, void* ifreq, void* scratch, int64_t scratch_bytes, qi_stream stream);

/* out [C][nbin][n] complex of `dtype`, from the frequencies it is handed: ifreq [C][nb][n] real of `dtype` on the device.
 * Refused: what the size query refuses; a null edges_hz; edges that are not finite or not strictly ascending (as rounded);
 * a weight that is not finite; null Z, ifreq or scratch; a null out ("nothing to produce"); misaligned pointers; a short
 * scratch.  One launch behind the tables': a workgroup per record and tile of QI_SQUEEZE_TILE columns. */
int qi_tfr_squeeze(int dtype, int device, const void* Z, const void* ifreq, int64_t C, int64_t nb, int64_t n,
                   const double* edges_hz, int64_t nbin, const double* weight, void* out, void* scratch, int64_t scratch_bytes,
                   qi_stream stream);

/* Both in one pass: the frequency of an element is formed in registers, from the lane's coefficient and its neighbour's (a
 * move across the lanes of the wave, one more load at a wave's last lane), and never stored.  Refused: what either call
 * refuses of the arguments it shares with it. */
int qi_tfr_synchrosqueeze(int dtype, int device, const void* Z, int64_t C, int64_t nb, int64_t n, const double* carrier_hz,
                          double sample_rate_hz, double power_floor, const double* edges_hz, int64_t nbin, const double* weight,
                          void* out, void* scratch, int64_t scratch_bytes, qi_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* QI_SQUEEZE_H */
