/*
 * qi_steer.h -- C ABI of libqi_tfr.so, part six: beam weights over a set of delay rows and their application to a stored
 * coefficient panel -- the signal from a direction, where qi_beam.h, qi_adaptive.h and qi_subspace.h give its power.
 *
 * Everything of qi_tfr.h holds here: its types and status codes, caller-owned device pointers, asynchronous calls on the
 * given stream with no host synchronisation and no allocation, qi_last_error() for the message (per thread).  The calls are
 * plan-less and keep no state: they may be made from several host threads at once, each on its own stream and buffers.
 *
 * Conventions, those of qi_array.h and qi_beam.h: S = conj(Z_i) Z_j, e[f][k][i] = exp(2 pi i freq_hz[f] delays_s[k][i]).
 * The beam is out[k][f][t] = sum_i weights[f][k][i] Z[i][f][t] -- NO conjugate: with S as above, mean_t |out|^2 = a^H S a
 * for a = weights[f][k], and a plane wave that reaches sensor i later by tau_i (Z_i = X0 exp(-2 pi i f tau_i)) is aligned
 * by a = e / C.
 *
 * Contract on the results
 *  - weights[f][k] is a function of whitener[f], freq_hz[f], C and row k of the delays alone; out[k][f][t] is a function of
 *    weights[f][k] and the column Z[:, f, t] alone: the same bits for any nbeam, nf and nt, at any position, on any run.
 *    There are no atomics; the sums run in `dtype` on the matrix cores (v_mfma_f32_16x16x4_f32, v_mfma_f64_16x16x4_f64) in an
 *    order that depends on C alone;
 *  - the phase is formed exactly as qi_beam.h states it: the product in double whatever `dtype` is, reduced to [-1/2, 1/2]
 *    turns in double, sincospi of the reduced turns in `dtype`;
 *  - the quotients e / C and (V u) / D are formed in double per component and rounded once to `dtype`; a component that is
 *    zero is +0;
 *  - IEEE rules hold throughout: a whitener that qi_csd_whiten flagged (NaN) gives NaN weights for that bin and NaN beams in
 *    that bin alone, a NaN in one column of the panel stays in that column, and the calls still return QI_OK.
 */
#ifndef QI_STEER_H
#define QI_STEER_H

#include "qi_tfr.h"
#include "qi_beam.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Beam weights of nf bins over nbeam delay rows.
 *   whitener == NULL: the conventional (Bartlett, delay-and-sum) weights a = e / C.
 *   whitener: [nf][C][C] complex of `dtype`, the V = L^-H of qi_csd_whiten (R^-1 = V V^H, upper triangular; the whole
 *   matrix is read): the minimum-variance distortionless-response (MVDR) weights
 *     u = V^H e,  D = sum_j |u_j|^2,  a = V u / D = R^-1 e / (e^H R^-1 e)
 *   -- the a that minimises a^H R a under e^H a = 1; a^H R a = 1 / D is the power qi_beam_capon gives.
 * 1 <= C <= QI_BEAM_MAX_SENSORS.  freq_hz: nf doubles on the HOST; they reach the device through the scratch in stream
 * order and may be reused as soon as the call returns.  delays_s: [nbeam][C] DOUBLES on the device whatever `dtype` is,
 * seconds.  weights: [nf][nbeam][C] complex of `dtype`.  scratch: caller-owned device buffer of
 * qi_beam_weights_scratch_bytes() (the frequency table), aligned to 16.  The size query is host only and gives the call's
 * verdicts on the shape: a negative qi_status for an unknown dtype, C out of range, nf or nbeam below 1, or nf * nbeam * C
 * past 2^40 entries.  The call also refuses a NULL freq_hz, delays_s, weights or scratch, misaligned pointers and scratch
 * that is too small -- all before anything is launched.  One launch: a wave per bin and tile of 16 delay rows. */
int64_t qi_beam_weights_scratch_bytes(int dtype, int64_t C, int64_t nf, int64_t nbeam);
int qi_beam_weights(int dtype, int device, const void* whitener, int64_t C, int64_t nf, const double* freq_hz,
                    const void* delays_s, int64_t nbeam, void* weights, void* scratch, int64_t scratch_bytes, qi_stream stream);

/* Beams of a panel: out[k][f][t] = sum_i weights[f][k][i] Z[i][f][t].  Z: [C][nf][nt] complex of `dtype` (an STFT, CWT or
 * Stockwell panel of C records); weights: [nf][nbeam][C] complex of `dtype` -- qi_beam_weights' or any others: the call is a
 * general per-bin mixing of a panel's records; out: [nbeam][nf][nt] complex of `dtype`, which must not overlap Z.
 * 1 <= C <= QI_BEAM_MAX_SENSORS; nf, nt and nbeam at least 1, any nbeam (taken in tiles of 16).  Refused before anything is
 * launched: an unknown dtype, C out of range, counts below 1, C * nf * nt, nbeam * nf * nt or nf * nbeam * C past 2^40
 * entries, a NULL Z, weights or out, misaligned pointers.  One launch: a workgroup per bin and run of time. */
int qi_beam_steer(int dtype, int device, const void* Z, int64_t C, int64_t nf, int64_t nt, const void* weights, int64_t nbeam,
                  void* out, qi_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* QI_STEER_H */
