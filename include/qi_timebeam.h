/*
 * qi_timebeam.h -- C ABI of libqi_tfr.so, part ten: DELAY-AND-SUM IN THE TIME DOMAIN.  The records of an array are delayed by
 * whole samples plus a fraction (a polyphase interpolator bank), summed, and either kept as beam traces or reduced to the
 * beam's power and semblance per sliding window and delay row -- the time-domain F detector's input -- with no cross-spectral
 * matrix, no segment and no narrow-band assumption: a delay may be any number of samples.  The records are staged once per
 * workgroup in LDS; no [G][n] intermediate reaches device memory.
 *
 * Everything of qi_tfr.h and qi_array.h holds here: caller-owned device pointers, asynchronous calls on the given stream with
 * no host synchronisation and no allocation, every refusal made before anything is launched, qi_last_error() for the message
 * (per thread); the calls are plan-less and may be made from several host threads at once.
 *
 * Common definitions
 *   x      [C][n] real of `dtype` (QI_F32 or QI_F64), 2 <= C <= QI_BEAM_MAX_SENSORS: the records.
 *   taps   [P][T] real of `dtype` on the device, 1 <= P <= QI_TIMEBEAM_MAX_PHASES, T in {1, 2, 4, 8, 16}: the interpolator
 *          bank, row p the filter of the fraction p / P; c = (T - 1) / 2 (integer division) is the tap that sits on the sample.
 *   shift  [rows][C] int32 on the device: whole samples;   phase [rows][C] int32 on the device, 0 .. P - 1.
 *   max_shift  0 .. QI_TIMEBEAM_MAX_SHIFT, declared by the caller: the largest |shift| of a row that is computed.
 *
 *   y[g][i][t] = sum_{m < T} taps[phase[g][i]][m] x[i][t + shift[g][i] + m - c]     (x = 0 outside 0 .. n - 1; every tap is
 *                applied, zero or not; m ascending from 0, every step one fused multiply-add)
 *   b[g][t]    = sum_i y[g][i][t]                                                   (i ascending from 0)
 *
 * A row g with any |shift| > max_shift or any phase outside 0 .. P - 1 gives NaN in everything computed from that row and
 * disturbs nothing else.  No address outside the records' buffer is ever formed into a load, for any int32 content of the
 * two tables: the tables are checked before they index anything, and every read of a record is either a staged copy whose
 * loads are guarded by 0 <= t < n or a guarded load itself.  Up to max_shift = QI_TIMEBEAM_LDS_MAX_SHIFT the records' chunk
 * and its halo of 2 max_shift + T samples are staged in LDS; above it the same arithmetic reads the records through L2 --
 * slower, the same bits.
 *
 * qi_time_beam_power.  Windows w = 0 .. nwin - 1, nwin = 1 + (n - win) / hop, cover t in [w hop, w hop + win); 1 <= win <= n,
 * hop >= 1.
 *   B[w][g] = sum_t b[g][t]^2          E[w][g] = sum_t sum_i y[g][i][t]^2
 *   normalize = 0: power[w][g] = B / (C^2 win)          (the mean square of the beam)
 *   normalize != 0: power[w][g] = B / (C E)             (the semblance, in [0, 1]; NaN where E = 0)
 * The sums run in `dtype`; the quotient is formed in double from the finished sums and rounded once.
 *   power       [nwin][G] real of `dtype`
 *   peak_index  [nwin] int64, peak_value [nwin] real of `dtype`: the first maximum of power[w] in grid order, or the first
 *               NaN if there is one -- qi_beam_power's rule.
 * Any of the three may be NULL, not all.  Two launches: the sums of every (unit of time, row) into scratch, then one
 * workgroup per window that adds a window's units, divides and picks the peak.  A unit is a hop where hop divides win and is
 * at least QI_TIMEBEAM_CHUNK samples -- no sample is then processed twice -- and the window itself otherwise.
 *
 * qi_time_beam_traces.  out[k][t] = b[k][t] / C for t in 0 .. n - 1, [K][n] of `dtype` (the quotient rounded once, IEEE
 * division).  One launch, no scratch.
 *
 * Contract on the results
 *  - power[w][g] is a function of row g of the two tables, the bank, C, win, hop and the samples that window reads, alone: the
 *    same bits for any G, any position of the row in the grid, any nwin, either side of QI_TIMEBEAM_LDS_MAX_SHIFT and any
 *    run.  Window w of a record has the same bits as window w - k of the record's copy from sample k hop on, whenever no read
 *    of that window reaches before that sample.  The order of the additions depends on C, T, win and hop and on nothing else.
 *  - out[k][t] is a function of row k of the two tables, the bank, C and the samples its taps read: the same bits for any K,
 *    any position of the row and any run.
 *  - A NaN sample makes NaN exactly those power[w][g] and out[k][t] whose taps touch it (a tap of value zero touches too);
 *    an infinite sample propagates by IEEE arithmetic.  A sample no tap reads is never looked at.
 *  - No atomics; every output element has one writer.
 */
#ifndef QI_TIMEBEAM_H
#define QI_TIMEBEAM_H

#include "qi_tfr.h"
#include "qi_beam.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QI_TIMEBEAM_MAX_PHASES 256
#define QI_TIMEBEAM_MAX_TAPS 16
#define QI_TIMEBEAM_MAX_SHIFT (1 << 20)
/* up to this max_shift the records are staged in LDS (a halo of 2 max_shift + T samples beside the chunk); above it the
 * same arithmetic reads them through L2 */
#define QI_TIMEBEAM_LDS_MAX_SHIFT 1024
/* samples of a record one workgroup stages and works through at a time, and delay rows it takes */
#define QI_TIMEBEAM_CHUNK 256
#define QI_TIMEBEAM_ROW_BLOCK 16

/* Bytes of scratch qi_time_beam_power needs (host only); the negative qi_status, with the message set, for a request the
 * call refuses.  Refused: an unknown dtype; C outside 2 .. QI_BEAM_MAX_SENSORS; P outside 1 .. QI_TIMEBEAM_MAX_PHASES; T not
 * 1, 2, 4, 8 or 16; n or G below 1 or above 2^40; win outside 1 .. n; hop below 1; max_shift outside 0 ..
 * QI_TIMEBEAM_MAX_SHIFT; more than 2^31 - 1 workgroups in either launch.  The call also refuses null x, taps, shift, phase
 * or scratch, no output at all, misaligned pointers (x, taps, power, peak_value: the element; shift, phase: 4; peak_index:
 * 8; scratch: 16) and a scratch_bytes below the query's answer. */
int64_t qi_time_beam_power_scratch_bytes(int dtype, int64_t C, int64_t n, int64_t P, int64_t T, int64_t G, int64_t win,
                                         int64_t hop, int64_t max_shift);
int qi_time_beam_power(int dtype, int device, const void* x, int64_t C, int64_t n, const void* taps, int64_t P, int64_t T,
                       const void* shift, const void* phase, int64_t G, int64_t max_shift, int64_t win, int64_t hop,
                       int normalize, void* power, void* peak_index, void* peak_value, void* scratch, int64_t scratch_bytes,
                       qi_stream stream);

/* Refused: what the size query refuses of dtype, C, P, T, n, K (for G) and max_shift; null x, taps, shift, phase or out;
 * misaligned pointers; more than 2^31 - 1 workgroups (ceil(n / QI_TIMEBEAM_CHUNK) ceil(K / QI_TIMEBEAM_ROW_BLOCK)). */
int qi_time_beam_traces(int dtype, int device, const void* x, int64_t C, int64_t n, const void* taps, int64_t P, int64_t T,
                        const void* shift, const void* phase, int64_t K, int64_t max_shift, void* out, qi_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* QI_TIMEBEAM_H */
