/*
 * qi_subspace.h -- C ABI of libqi_tfr.so, part five: the eigenpairs of the cross-spectral matrices of qi_array.h and the
 * subspace (MUSIC) beamformer on them, beside the conventional one of qi_beam.h and the adaptive one of qi_adaptive.h.
 *
 * Everything of qi_tfr.h holds here: its types and status codes, caller-owned device pointers, asynchronous calls on the
 * given stream with no host synchronisation and no allocation, qi_last_error() for the message (per thread).  The calls are
 * plan-less and keep no state: they may be made from several host threads at once, each on its own stream and buffers.  The
 * reference (quantum-inferno) has no array processing.
 *
 * MUSIC's power at a delay set is C / (e^H P e) with P the projector onto the noise subspace of the cross-spectral matrix:
 * the span of the eigenvectors of its C - n_sources smallest eigenvalues.  It is computed in two calls: qi_csd_eigh
 * diagonalises every matrix once, S = U diag(w) U^H; qi_beam_music forms e^H P e = sum_{j < C - n_sources} |U_j^H e|^2, a sum
 * of squares, for every grid point on the matrix cores.  The eigenpairs are useful on their own (the number of sources,
 * principal-component coherence, subspace whitening).
 *
 * Contract on the results
 *  - eigenvalues[f], eigenvectors[f] and info[f] are functions of csd[f] and C alone: the same bits for any nf, at any position
 *    in the stack, on any run.  There are no atomics; the order of the rotations and of every sum is fixed by C;
 *  - power[b][g] is a function of the band's eigenvectors, their frequencies, n_sources and row g of the delays alone: the same
 *    bits for any G, at any position in the grid, in any band table that holds the same band, for either workgroup size, on
 *    any run;
 *  - the phase freq * tau is formed and reduced exactly as qi_beam.h states it (double product, reduced to [-1/2, 1/2] turns
 *    in double, sincospi in `dtype`): a phase that is an exact multiple of a quarter turn gives exactly +-1 and 0.
 */
#ifndef QI_SUBSPACE_H
#define QI_SUBSPACE_H

#include "qi_tfr.h"
#include "qi_beam.h" /* QI_BEAM_MAX_SENSORS */

#ifdef __cplusplus
extern "C" {
#endif

/* Eigenpairs of nf Hermitian matrices: for every matrix f,  S_f = U_f diag(w_f) U_f^H,  U_f^H U_f = I.
 * csd: [nf][C][C] complex of `dtype` as qi_csd / qi_cross_spectra write it, 1 <= C <= QI_BEAM_MAX_SENSORS.  ONLY THE LOWER
 * TRIANGLE (i >= j) AND THE REAL PART OF THE DIAGONAL ARE READ: the matrix is taken as Hermitian.
 * eigenvalues: [nf][C] real of `dtype`, ascending; equal values keep the order of the diagonal positions they converged at (a
 * stable sort).  eigenvectors: [nf][C][C] complex of `dtype`, row-major: column j is the unit eigenvector of eigenvalues[f][j]
 * (numpy.linalg.eigh's layout).  The phase of a column is whatever the iteration leaves: a function of the matrix alone.
 * The iteration is a cyclic two-sided Jacobi iteration in `dtype` (the norms of its stopping test in double); it stops when
 * the off-diagonal part is at most C eps times the Frobenius norm, eps the spacing of `dtype` at 1: the eigenvalues are then
 * within a few C eps |S_f|_F of the exact ones, and U^H U - I within a few sweeps times C eps.  A matrix that is diagonal in
 * the triangle that is read is left alone: its eigenvalues are the sorted diagonal bit for bit, its eigenvectors the columns of
 * a permutation matrix.  float32: a matrix whose entries' magnitudes lie outside the normal range of float32 may not converge.
 * info: [nf] int32 on the device, or NULL: 0 for a matrix that converged, 1 for one whose off-diagonal part did not fall under
 * the threshold within the cap of 40 sweeps -- every matrix with an entry that is not finite in the triangle that is read
 * ends here.  For info == 1 every eigenvalue and every entry of eigenvectors[f] is NaN: MUSIC's power is NaN there.  The call
 * still returns QI_OK: a bad matrix is data, not an error.
 * Refused before the device is touched, with a negative status and a message: an unknown dtype, C outside
 * 1..QI_BEAM_MAX_SENSORS, nf < 1, a NULL csd, eigenvalues or eigenvectors, misaligned pointers.
 * One launch, a workgroup per matrix, the matrix and the rotations in LDS (up to 128 KiB). */
int qi_csd_eigh(int dtype, int device, const void* csd, int64_t C, int64_t nf, void* eigenvalues, void* eigenvectors, void* info,
                qi_stream stream);

/* MUSIC power of nf diagonalised matrices over G delay sets, over nb bands of consecutive matrices.
 *   e[f][g][i]  = exp(2 pi i freq_hz[f] delays_s[g][i])                           (as in qi_beam.h)
 *   m           = C - n_sources                                                   (noise columns: the m smallest eigenvalues)
 *   D[f][g]     = sum_{j < m} | sum_i conj(U_f[i][j]) e[f][g][i] |^2              (= e^H P_noise e, in [0, C])
 *   power[b][g] = C * n_b / sum_{f in band b} D[f][g]                             (n_b matrices in the band)
 * the reciprocal of the band's mean null spectrum: dimensionless and >= 1 up to rounding; a steering vector wholly inside the
 * noise subspace gives 1, n_sources == 0 gives 1 everywhere (the completeness of U), a source gives a large value.  D is
 * summed in `dtype` on the matrix cores, the band sum runs in double in ascending f, the division is taken once in double and
 * rounded once to `dtype`; IEEE throughout: a zero sum gives inf, a NaN stays a NaN (a band that holds a matrix qi_csd_eigh
 * flagged is NaN).
 * eigenvectors: [nf][C][C] complex of `dtype` as qi_csd_eigh writes it, the whole matrix is read; the columns from m on do not
 * contribute.  n_sources: 0 <= n_sources < C, one number for all matrices.  freq_hz: nf doubles on the HOST.  delays_s: [G][C]
 * DOUBLES on the device.  band_first: nb + 1 strictly ascending offsets into 0..nf on the HOST, or NULL: every matrix its own
 * band (nb = nf).  Both host arrays reach the device as kernel arguments, in stream order.  power: [nb][G] real of `dtype`.
 * peak_index: [nb] int64 or NULL, the index of the first maximum of power[b] -- of the first NaN if there is one (np.argmax);
 * peak_value: [nb] real of `dtype` or NULL, that entry.  scratch: caller-owned device buffer of
 * qi_beam_music_scratch_bytes(), aligned to 16.  The size query, the refusals and the scratch are those of qi_beam_power and
 * qi_beam_power_scratch_bytes (qi_beam.h), word for word; an n_sources outside 0..C-1 is refused as well.  One launch for the
 * power (a workgroup per band and tile of grid points), one for the peaks. */
int64_t qi_beam_music_scratch_bytes(int dtype, int64_t C, int64_t nf, int64_t G, int64_t nb);
int qi_beam_music(int dtype, int device, const void* eigenvectors, int64_t C, int64_t nf, int64_t n_sources, const double* freq_hz,
                  const void* delays_s, int64_t G, const int64_t* band_first, int64_t nb, void* power, void* peak_index,
                  void* peak_value, void* scratch, int64_t scratch_bytes, qi_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* QI_SUBSPACE_H */
