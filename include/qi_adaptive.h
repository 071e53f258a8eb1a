/*
 * qi_adaptive.h -- C ABI of libqi_tfr.so, part four: the adaptive (Capon, minimum-variance) beamformer on the cross-spectral
 * matrices of qi_array.h, beside the conventional one of qi_beam.h.
 *
 * Everything of qi_tfr.h holds here: its types and status codes, caller-owned device pointers, asynchronous calls on the
 * given stream with no host synchronisation and no allocation, qi_last_error() for the message (per thread).  The calls are
 * plan-less and keep no state: they may be made from several host threads at once, each on its own stream and buffers.  The
 * reference (quantum-inferno) has no array processing.
 *
 * Capon's power at a delay set is 1 / (e^H R^-1 e) with R the (diagonally loaded) cross-spectral matrix.  It is computed in
 * two calls: qi_csd_whiten factors every matrix once, R = L L^H, and stores V = L^-H (R^-1 = V V^H); qi_beam_capon forms
 * e^H R^-1 e = |V^H e|^2, a sum of squares, for every grid point on the matrix cores.
 *
 * Contract on the results
 *  - whitener[f] is a function of csd[f], C and `loading` alone: the same bits for any nf, at any position in the stack, on
 *    any run.  There are no atomics, and the order of every sum is fixed by C;
 *  - power[b][g] is a function of the band's whiteners, their frequencies and row g of the delays alone: the same bits for any
 *    G, at any position in the grid, in any band table that holds the same band, for either workgroup size, on any run;
 *  - the phase freq * tau is formed and reduced exactly as qi_beam.h states it (double product, reduced to [-1/2, 1/2] turns
 *    in double, sincospi in `dtype`): a phase that is an exact multiple of a quarter turn gives exactly +-1 and 0.
 */
#ifndef QI_ADAPTIVE_H
#define QI_ADAPTIVE_H

#include "qi_tfr.h"
#include "qi_beam.h" /* QI_BEAM_MAX_SENSORS */

#ifdef __cplusplus
extern "C" {
#endif

/* Whitening factors of nf Hermitian matrices: for every matrix f
 *   R_f = S_f + load_f I,   load_f = loading * (sum_i Re S_f[i][i]) / C     (loading >= 0, relative to the mean auto-power)
 *   R_f = L L^H (Cholesky),  whitener[f] = V_f = L^-H:  R_f^-1 = V V^H  and  V^H R_f V = I.
 * csd: [nf][C][C] complex of `dtype` as qi_csd / qi_cross_spectra write it, 1 <= C <= QI_BEAM_MAX_SENSORS.  ONLY THE LOWER
 * TRIANGLE (i >= j) AND THE REAL PART OF THE DIAGONAL ARE READ: the matrix is taken as Hermitian.  The mean diagonal and
 * load_f are formed in double (the diagonal summed in ascending i); the loaded diagonal is rounded once to `dtype`;
 * loading == 0 leaves the diagonal's bits alone.
 * whitener: [nf][C][C] complex of `dtype`, row-major, upper triangular; the strictly lower part is written as zeros.
 * info: [nf] int32 on the device, or NULL: LAPACK's potrf convention -- 0 for success, k (1-based) for the first pivot that is
 * not a positive finite number.  For such a matrix every entry of whitener[f] on or above the diagonal is NaN (the lower zeros
 * stay): Capon's power is NaN there.  The call still returns QI_OK: a singular matrix is data, not an error.
 * Refused before the device is touched, with a negative status and a message: an unknown dtype, C outside
 * 1..QI_BEAM_MAX_SENSORS, nf < 1, a `loading` that is negative or not finite, a NULL csd or whitener, misaligned pointers.
 * One launch, a workgroup per matrix, the matrix in LDS. */
int qi_csd_whiten(int dtype, int device, const void* csd, int64_t C, int64_t nf, double loading, void* whitener, void* info,
                  qi_stream stream);

/* Capon power of nf whitened matrices over G delay sets, summed over nb bands of consecutive matrices.
 *   e[f][g][i]  = exp(2 pi i freq_hz[f] delays_s[g][i])                           (as in qi_beam.h)
 *   D[f][g]     = sum_j | sum_i conj(V_f[i][j]) e[f][g][i] |^2                    (= e^H R_f^-1 e, never negative)
 *   power[b][g] = sum_{f in band b} 1 / D[f][g]
 * in the units of qi_beam_power with normalize = 0: a plane wave of auto-power p in white noise sigma gives p + sigma / C at
 * its own delays; 1 / D <= e^H R e / C^2, the conventional power of the same loaded matrices.  D is summed in `dtype` on the
 * matrix cores, the reciprocal is taken in double, the band sum runs in double in ascending f and is rounded once to `dtype`;
 * IEEE throughout: D = 0 gives inf, a NaN stays a NaN (a band that holds a matrix qi_csd_whiten flagged is NaN).
 * whitener: [nf][C][C] complex of `dtype` as qi_csd_whiten writes it: upper triangular WITH the zeros below the diagonal (the
 * 16 x 16 blocks below the diagonal blocks are skipped, the diagonal blocks are read whole).  freq_hz: nf doubles on the HOST.  delays_s: [G][C] DOUBLES
 * on the device.  band_first: nb + 1 strictly ascending offsets into 0..nf on the HOST, or NULL: every matrix its own band
 * (nb = nf).  Both host arrays reach the device as kernel arguments, in stream order.  power: [nb][G] real of `dtype`.
 * peak_index: [nb] int64 or NULL, the index of the first maximum of power[b] -- of the first NaN if there is one (np.argmax);
 * peak_value: [nb] real of `dtype` or NULL, that entry.  scratch: caller-owned device buffer of
 * qi_beam_capon_scratch_bytes(), aligned to 16.  The size query, the refusals and the scratch are those of qi_beam_power and
 * qi_beam_power_scratch_bytes (qi_beam.h), word for word.  There is no semblance: it needs the traces, which the whitener does
 * not carry.  One launch for the power (a workgroup per band and tile of grid points), one for the peaks. */
int64_t qi_beam_capon_scratch_bytes(int dtype, int64_t C, int64_t nf, int64_t G, int64_t nb);
int qi_beam_capon(int dtype, int device, const void* whitener, int64_t C, int64_t nf, const double* freq_hz, const void* delays_s,
                  int64_t G, const int64_t* band_first, int64_t nb, void* power, void* peak_index, void* peak_value, void* scratch,
                  int64_t scratch_bytes, qi_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* QI_ADAPTIVE_H */
