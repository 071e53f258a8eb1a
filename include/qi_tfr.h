/*
 * qi_tfr.h -- C ABI of libqi_tfr.so, the MI355X (gfx950) time-frequency hot path.
 *
 * The reference (ISLA-UH/quantum-inferno v1.1.3) is pure Python and has no FFI; the
 * boundary a maintainer would bind is therefore the set of public Python functions
 * cited on each entry point below (paths relative to quantum_inferno/ in the reference).
 * INTEGRATION.md shows the ctypes stub for each.
 *
 * Conventions
 *  - plain C: pointers, sizes, doubles.  No torch / hip types in any signature
 *    (qi_stream is a hipStream_t passed as void*; NULL = the default stream).
 *  - every data pointer is a CALLER-OWNED DEVICE pointer on the plan's device; band
 *    tables passed to the qi_plan_set_* calls are HOST pointers (float64 / int64),
 *    because band and index selection stays on the host in float64 (bit-exact with the
 *    reference, scales_dyadic.py:355-393, styx_stx.py:233).
 *  - every call returns 0 on success or a negative qi_status; qi_last_error() gives the
 *    message for the calling thread (qi_last_error is per thread: a refusal on another thread
 *    never changes it).  Nothing throws, nothing aborts.
 *  - host threads: the plan-less entry points (everything that takes no qi_plan) may be called
 *    from several host threads at once, each on its own stream and its own buffers; what they
 *    keep per device (hipFFT handles and a work area per stream, strip partials per stream,
 *    twiddle tables) is locked inside.  A plan belongs to ONE host thread and stream at a time:
 *    it has one scratch; threads each make their own plan, and different plans may be created,
 *    used and destroyed side by side (tests/test_gpu_threads.py, tests/sanitize_threads/).
 *  - transforms are asynchronous on the given stream and do no host synchronisation;
 *    a plan is thread-compatible (one plan per host thread / stream).  The calls that upload
 *    host tables -- qi_plan_set_gabor_bank, qi_gabor_atoms, qi_gabor_atoms_at -- wait for the
 *    stream before they return (their uploads live in temporaries).
 *  - panels are [channel][band][time], C-contiguous, band frequency ascending, as the
 *    reference returns them for one channel (styx_cwt.py:198, styx_stx.py:236).
 *  - dtype selects the arithmetic: QI_F32 (float / float2) or QI_F64 (double / double2).
 */
#ifndef QI_TFR_H
#define QI_TFR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QI_TFR_ABI_VERSION 1

typedef struct qi_plan qi_plan; /* opaque */
typedef void* qi_stream;        /* hipStream_t */

typedef enum { QI_F32 = 0, QI_F64 = 1 } qi_dtype;

typedef enum {
  QI_OK = 0,
  QI_ERR_ARG = -1,     /* bad argument (null pointer, size, dtype, band count)        */
  QI_ERR_STATE = -2,   /* plan is missing the table this call needs                   */
  QI_ERR_HIP = -3,     /* a HIP runtime call failed                                   */
  QI_ERR_FFT = -4,     /* hipFFT failed                                               */
  QI_ERR_NOMEM = -5,   /* workspace budget too small for one (channel, band) tile     */
  QI_ERR_UNSUPPORTED = -6
} qi_status;

/* Gabor-bank slots of a plan */
typedef enum {
  QI_BANK_STYX = 0,  /* styx_cwt.py:147-198  zero-padded linear correlation, L = 2n      */
  QI_BANK_ATOMS = 1  /* cwt_atoms.py:406-421 circular correlation of length n, roll n/2  */
} qi_bank;

/* FFT engine behind a plan */
typedef enum {
  QI_ENGINE_AUTO = 0,   /* native kernels when n is a supported power of two (the small-record engine at
                           2^10 .. 2^13 samples, see qi_plan_band_route), else hipFFT */
  QI_ENGINE_HIPFFT = 1, /* batched hipFFT + hand-written multiply / epilogue kernels      */
  QI_ENGINE_NATIVE = 2  /* hand-written LDS FFT passes with fused multiply and epilogue   */
} qi_engine;

typedef struct {
  int64_t n;               /* samples per record (any n >= 2 for hipFFT; 2^k for native)  */
  int32_t dtype;           /* qi_dtype                                                     */
  int32_t device;          /* HIP device ordinal                                           */
  int32_t engine;          /* qi_engine                                                    */
  int32_t flags;           /* reserved: must be 0 (qi_plan_create rejects anything else)   */
  int64_t workspace_bytes; /* scratch budget owned by the plan; 0 = default (2 GiB)        */
} qi_plan_desc;

/* What a transform should produce.  Every pointer is optional (NULL = not produced).
 * P = power_scale * |z|^2 is the power the reductions are taken over (the reference's
 * callers use 2|z|^2, docs/examples_tutorial/e00_intro_set/s04_tone_tfr.py:92). */
typedef struct {
  void* coef;         /* [C][B][n] complex  TFR coefficients                                      */
  void* bits;         /* [C][B][n] real     log2(|z| + eps)        utilities/rescaling.py:13-20   */
  void* power_band;   /* [C][B]    float64  sum over time of P     tfr_info.py:93 (before log2)   */
  void* power_time;   /* [C][n]    real     sum over bands of P    tfr_info.py:91 (before log2)   */
  void* stats;        /* [C][4]    float64  {max P, sum P, sum P*log2(P), 0}  tfr_info.py:65-79,231 */
  double power_scale; /* 0 is read as 1                                                           */
  double eps;         /* epsilon inside the log2 of `bits`; 0 is read as 2^-52 (scales_dyadic.py:16) */
} qi_tfr_out;

/* ---- library ------------------------------------------------------------------------ */
int qi_abi_version(void);
const char* qi_last_error(void);
/* Name of the code object's GPU target ("gfx950") and of the device actually present. */
int qi_device_info(int device, char* name, size_t name_len, int64_t* hbm_bytes, int32_t* compute_units);

/* ---- plans -------------------------------------------------------------------------- */
int qi_plan_create(qi_plan** plan, const qi_plan_desc* desc);
int qi_plan_destroy(qi_plan* plan);

/* Gabor atom bank, built on the device in float64 exactly as the reference builds it in
 * the time domain and transformed once per plan:
 *   atom_j[k] = amp_j * exp(-(p_re_j + i p_im_j) x_k^2) * exp(i omega_j x_k),  x_k = k - (n-1)/2
 * styx_cwt.py:68-144 (p_re = 1/(2 s^2), p_im = 0, omega = 2 pi f / fs, amp by dictionary_type);
 * cwt_atoms.py:16-50,202-238 (p = (1 - i shift gamma/pi)/(2 s^2), omega = M_q / s).
 * Host arrays of length B (float64). */
int qi_plan_set_gabor_bank(qi_plan* plan, int bank, int32_t n_bands, const double* p_re, const double* p_im,
                           const double* omega, const double* amp, qi_stream stream);

/* The same atoms in the time domain, float64, for inspection (styx_cwt.wavelet_centered_4cwt,
 * styx_cwt.py:113-144; cwt_atoms.chirp_centered_4cwt, cwt_atoms.py:303-340): out [B][n] complex128
 * (device).  Parameter arrays are host float64 of length B, as above. */
int qi_gabor_atoms(int device, int64_t n, int32_t n_bands, const double* p_re, const double* p_im,
                   const double* omega, const double* amp, void* out, qi_stream stream);

/* The same on the caller's own sample positions x [n] (device, float64; x_k = fs * (t_k - t_offset) in samples):
 * styx_cwt.wavelet_complex on an arbitrary time axis (styx_cwt.py:58-110), cwt_atoms.chirp_complex (cwt_atoms.py:16-50). */
int qi_gabor_atoms_at(int device, int64_t n, int32_t n_bands, const double* p_re, const double* p_im,
                      const double* omega, const double* amp, const void* x, void* out, qi_stream stream);

/* Stockwell band table: shift index idx_j = argmin_k |fftfreq_k - f_j| and Gaussian width
 * sigma_j = M / (2 pi f_j / fs); the window exp(-sigma_j^2 omega_k^2 / 2), omega_k = 2 pi fftfreq_k / fs,
 * is regenerated in registers.  styx_stx.py:216-234.  Host arrays of length B. */
int qi_plan_set_stx_bands(qi_plan* plan, int32_t n_bands, const int64_t* shift_index, const double* sigma);

int64_t qi_plan_bands(const qi_plan* plan, int which /* qi_bank, or 2 for the STX table */);
/* Bands of table `which` whose coefficients are produced by the kernels of profiling stage `stage` (qi_stage below:
 * PASS2 or BLOCK on the native engine, SMALL on the small-record engine -- the table's whole band count --, INVERSE on the
 * hipFFT engine); used to price a stage's algorithmic bytes. */
int64_t qi_plan_stage_bands(const qi_plan* plan, int which, int stage);

/* Forward transform of a float32 plan on the native engines (a read-only query).  When every native table set on the plan
 * reads the record spectrum only near DC -- all bands on the zoom, block and split engines, no two-pass row, no short-atom
 * sub-table, transform lengths 2^20 / 2^21 -- the forward transform forms only the bins (-Lf / 64, Lf / 64) of each
 * table's Lf-point spectrum ("low-bins" path; qi_cwt, qi_stx and qi_cwt_stx of one plan always take the same path).
 * Returns 0 when the plan runs the full transform (or table `which` is not set); otherwise the power of two K of table
 * `which` with every bin its bands read inside (-K, K), K <= Lf / 64. */
int64_t qi_plan_forward_low(const qi_plan* plan, int which /* as qi_plan_bands */);

/* Per-time planes table `which` (QI_BANK_STYX or 2, the Stockwell table) writes in a joint one-record qi_cwt_stx call of a
 * float32 plan on the native engines: the planes the summing tail reads for that table (two-pass chunks, the block
 * launch's planes under the dealing in effect, the zoom launch's rows).  0 when the plan runs no joint call.  Builds the
 * joint launch's item lists on first use, like the call itself. */
int64_t qi_plan_joint_planes(qi_plan* plan, int which);

/* Which kernels produce row `band` of table `which` in a call of `records` records (a read-only query: tests and
 * diagnostics use it to tell which path a band takes; it changes nothing).  `records` means the records that go through
 * together: a call whose records do not fit the plan's scratch runs in tiles, and each tile takes the route of its own
 * record count.
 *   stage    qi_stage below: ZOOM, BLOCK, PASS2, SMALL, or INVERSE (the hipFFT engine: the whole table, or the pass behind
 *            the native run)
 *            SMALL: the small-record engine runs the whole table.  Size rule: the plan is QI_ENGINE_AUTO, n is a power of two
 *            with 2^10 <= n <= 2^13 (and below the length from which zoom / block are tried), and the L complex values of the
 *            table's transform -- L = 2n for QI_BANK_STYX, n for QI_BANK_ATOMS and the STX table -- fit 128 KiB: every float32
 *            table; every float64 table but QI_BANK_STYX at n = 2^13, which stays on the hipFFT engine.  A call whose
 *            workspace cannot hold one record's scratch (a spectrum row, the reduction slots, the per-time planes) runs on the
 *            hipFFT engine, whose tables such a plan keeps.
 *   cls      ZOOM, float32: the band's class 0..6 in the table, after small classes have joined their neighbours
 *            (0..4 coarse-grid level with the 10-tap interpolator, 5 / 6 the 6- / 4-tap classes of level 0);
 *            ZOOM, float64: the coarse-grid level 0..4;  BLOCK: reach group 1, 2, 4, or 8 (8192-sample long blocks)
 *   run_cls  ZOOM, float32: the class the band runs as in this call (classes 5 and 6 run as 0 in calls of few
 *            records); ZOOM, float64: the class of the fine kernel, or -1 (k_z64_interp);  otherwise = cls
 *            (SMALL: cls = run_cls = log2 L, flags = 0)
 *   flags    QI_ROUTE_* bits */
typedef struct {
  int32_t stage, cls, run_cls, flags;
} qi_band_route;
#define QI_ROUTE_ANALYTIC(f) ((f) & 3)        /* BLOCK: 0 filter spectrum from the bank row, 1 Gaussian, 2 aliased Gaussian */
#define QI_ROUTE_NARROW(f) (((f) >> 2) & 3)   /* BLOCK: 0 full spectrum, 1 a 256-bin window, 2 the lower half               */
#define QI_ROUTE_NOWRAP 16                    /* BLOCK: weights without wrap-around logic                                    */
#define QI_ROUTE_SPLIT 32                     /* ZOOM: split band (tapered atom on the zoom engine + edge pieces)            */
#define QI_ROUTE_PASS2_KIND(f) (((f) >> 6) & 3) /* PASS2: 0 one-pass loader, 1 general (two passes), 2 short-atom table      */
#define QI_ROUTE_BEHIND 256                   /* INVERSE: Stockwell row of the hipFFT pass behind the native run             */
#define QI_ROUTE_F64_ZOOM 512                 /* ZOOM: the float64 zoom engine                                               */
int qi_plan_band_route(const qi_plan* plan, int which, int32_t band, int64_t records, qi_band_route* route);

/* ---- measurement ------------------------------------------------------------------- */
/* Stages of one transform call, timed with HIP events on the caller's stream when profiling is on
 * (bench.py's roofline leg; off by default, two event records per stage launch when on). */
typedef enum {
  QI_STAGE_FORWARD = 0,  /* pack + forward FFT of the records                                  */
  QI_STAGE_MULTIPLY = 1, /* spectrum x atom bank, or shifted spectrum x Gaussian (hipFFT engine) */
  QI_STAGE_INVERSE = 2,  /* batched inverse FFT (hipFFT engine)                                  */
  QI_STAGE_EPILOGUE = 3, /* crop / power / entropy epilogue (hipFFT engine)                      */
  QI_STAGE_PASS1 = 4,    /* native engine: fused multiply + first FFT pass                       */
  QI_STAGE_PASS2 = 5,    /* native engine: second FFT pass + fused epilogue                      */
  QI_STAGE_BLOCK = 6,    /* native engine: short-atom bands by overlap-save blocks (forward, filter, inverse,  */
                         /* epilogue in one kernel)                                                             */
  QI_STAGE_ZOOM = 7,     /* native engine: narrow-band panels, interpolation kernel (one span per launch)       */
  QI_STAGE_ZOOM_COARSE = 8, /* native engine: baseband gather + batched coarse inverse FFT of the zoom bands     */
  QI_STAGE_SMALL = 9,    /* small-record engine: spectrum product, in-LDS inverse transform and fused epilogue of  */
                         /* every band in one kernel (its forward launch is timed as FORWARD, its tail as EPILOGUE) */
  QI_STAGE_COUNT = 10
} qi_stage;
/* enable: 0 off; low 16 bits: 1 every stage, otherwise a mask with bit (stage + 1) set for each stage to time (every
 * recorded event is a small bubble in the stream, so a caller that wants one stage asks for that one); high 16 bits:
 * sampling period P (0 or 1: every transform call; P: every P-th call of qi_cwt / qi_stx is timed, the others run
 * without events).  Enabling or disabling also clears the counters. */
int qi_plan_profile(qi_plan* plan, int enable);
/* Sum of elapsed milliseconds and number of launches per stage since the last read; waits for the
 * recorded events.  Arrays of QI_STAGE_COUNT entries. */
int qi_plan_profile_read(qi_plan* plan, double* stage_ms, int64_t* stage_launches, int32_t n_stages);

/* ---- transforms --------------------------------------------------------------------- */
/* styx_cwt.cwt_complex_any_scale_pow2 (styx_cwt.py:147-198, cwt_type="fft") when bank = QI_BANK_STYX;
 * cwt_atoms.cwt_chirp_complex (cwt_atoms.py:343-444, cwt_type="fft") when bank = QI_BANK_ATOMS.
 * sig: [C][n] real. */
int qi_cwt(qi_plan* plan, int bank, const void* sig, int64_t n_channels, const qi_tfr_out* out, qi_stream stream);

/* styx_stx.stx_complex_any_scale_pow2 (styx_stx.py:195-236).  sig: [C][n] real. */
int qi_stx(qi_plan* plan, const void* sig, int64_t n_channels, const qi_tfr_out* out, qi_stream stream);

/* Both of the above on the same records in one call (bank = QI_BANK_STYX): the results are those of qi_cwt followed by
 * qi_stx to within float rounding -- the Stockwell bands may be formed from the even bins of the zero-padded spectrum
 * the CWT has just made instead of a second forward transform, and when the records fit one workspace tile the two
 * transforms share their kernel launches stage by stage (one forward transform per 4096-sample block for the bands of
 * both), so out_cwt is complete only when the call's work on `stream` is (the tutorials run both on every record,
 * s04_tone_tfr.py:84-112). */
int qi_cwt_stx(qi_plan* plan, int bank, const void* sig, int64_t n_channels, const qi_tfr_out* out_cwt,
               const qi_tfr_out* out_stx, qi_stream stream);

/* styx_fft.stft_complex_pow2 / stft_from_sig (styx_fft.py:14-57,152-187): scipy.signal.stft with
 * boundary="zeros", padded=True, detrend="constant", one-sided.  window: [seg] real (device);
 * scale multiplies every coefficient (1/sum(window), times 2 sqrt(pi)/seg for stft_from_sig).
 * Z: [C][nfft/2+1][n_seg] complex, bits: same shape real or NULL.  n_seg as qi_stft_segments().
 * scratch: caller-owned device buffer of qi_stft_scratch_bytes() (windowed frames + their spectra). */
int64_t qi_stft_segments(int64_t n, int64_t seg, int64_t hop);
int64_t qi_stft_scratch_bytes(int dtype, int64_t n_channels, int64_t n, int64_t seg, int64_t hop, int64_t nfft);
int qi_stft(int dtype, int device, const void* sig, int64_t n_channels, int64_t n, const void* window, int64_t seg,
            int64_t hop, int64_t nfft, double scale, void* Z, void* bits, double eps, void* scratch,
            int64_t scratch_bytes, qi_stream stream);

/* styx_fft.welch_power_pow2 (styx_fft.py:230-266): scipy.signal.welch, detrend="constant", scaling="spectrum",
 * average="mean", one-sided, no boundary extension.  Pxx: [C][nfft/2+1] real.  scale = 1/sum(window). */
int64_t qi_welch_scratch_bytes(int dtype, int64_t n_channels, int64_t n, int64_t seg, int64_t hop, int64_t nfft);
int qi_welch(int dtype, int device, const void* sig, int64_t n_channels, int64_t n, const void* window, int64_t seg,
             int64_t hop, int64_t nfft, double scale, void* pxx, void* scratch, int64_t scratch_bytes,
             qi_stream stream);

/* ---- tfr_info reductions on a caller-supplied power panel P [C][B][n] (real) ---------- */
/* Marginals in one pass: power_band [C][B] f64, power_time [C][n] real, stats [C][4] f64
 * {max, sum, sum P log2 P, 0}.  tfr_info.py:82-94 (the sums / max under the log2). */
int qi_power_marginals(int dtype, int device, const void* power, int64_t n_channels, int64_t n_bands, int64_t n,
                       void* power_band, void* power_time, void* stats, void* scratch, int64_t scratch_bytes,
                       qi_stream stream);
int64_t qi_power_marginals_scratch_bytes(int64_t n_channels, int64_t n_bands, int64_t n);

/* out[i] = log2(in[i] + eps) - ref[c]   (tfr_info.py:65-79 with ref = log2(max + eps));
 * `ref` is a device array [C] float64 or NULL (= 0).  Elements per channel = count. */
int qi_log2_offset(int dtype, int device, const void* in, void* out, int64_t n_channels, int64_t count, double eps,
                   const void* ref, qi_stream stream);

/* out[i] = (double) in[i] for `count` float32 values (a complex64 panel is 2 * count floats): the reference returns
 * complex128 panels / float64 bits whatever the record's dtype (styx_cwt.py:195-198, styx_stx.py:228, cwt_atoms.py:408,442);
 * the wrappers compute float32 records in float32 and widen on the device before the copy to the host. */
int qi_widen(int device, const void* in, void* out, int64_t count, qi_stream stream);

/* out[i] = log2(|in[i]| + eps) for `count` real (is_complex = 0) or complex (1; dtype is the real type) values:
 * utilities.rescaling.to_log2_with_epsilon (utilities/rescaling.py:13-20) on a device array. */
int qi_log2_abs(int dtype, int device, const void* in, int is_complex, void* out, int64_t count, double eps,
                qi_stream stream);

/* ShannonStft family (tfr_info.py:203-260) on P [C][B][n]:
 *   pdf = P * mult, mult = 1/sum(P)            (mode 0, shannon_stft_from_tfr_power)
 *                        = 1/sum_axis0 + eps64  (mode 1, ShannonStftPerTime,  deg_free = B)
 *                        = 1/sum_axis1 + eps64  (mode 2, ShannonStftPerFreq,  deg_free = n)
 *   info = -log2(pdf + eps64); shannon_bits = pdf*info; isnr = log2(D) - info; esnr = shannon_bits/(log2(D)/D)
 * mult: device [C] (mode 0), [C][n] (mode 1) or [C][B] (mode 2), real.  Outputs optional. */
int qi_shannon_panel(int dtype, int device, const void* power, const void* mult, int mode, int64_t n_channels,
                     int64_t n_bands, int64_t n, double deg_free, void* info, void* shannon_bits, void* isnr,
                     void* esnr, qi_stream stream);

/* ---- sliding-window STFT in scipy.signal.ShortTimeFFT's convention (utilities/short_time_fft.py:20-175) ------------
 * Slice q (0 <= q < n_slices) covers the padded record from sample first + q * hop (first <= 0: ShortTimeFFT's
 * p_min * hop - seg // 2); pad_mode 0 zeros, 1 edge, 2 even, 3 odd reflection; detrend 1 removes each slice's mean
 * (stft_detrend(detr="constant")); the windowed slice is rotated left by `roll` before the transform (ShortTimeFFT's
 * phase_shift = 0 convention: roll = seg // 2).  window: [seg] real, already scaled (ShortTimeFFT.scale_to).  Z: [C][nfft/2+1]
 * [n_slices] complex or NULL; real_out: same shape real or NULL, real_kind 1 = |Z| (stft_tukey), 2 = |Z|^2
 * (spectrogram_tukey). */
int64_t qi_sliding_scratch_bytes(int dtype, int64_t n_channels, int64_t nfft, int64_t n_slices);
int qi_sliding_stft(int dtype, int device, const void* sig, int64_t n_channels, int64_t n, const void* window,
                    int64_t seg, int64_t hop, int64_t nfft, int64_t first, int64_t n_slices, int pad_mode, int detrend,
                    int64_t roll, void* Z, void* real_out, int real_kind, void* scratch, int64_t scratch_bytes,
                    qi_stream stream);
/* ShortTimeFFT.istft (istft_tukey, short_time_fft.py:112-137): out[c][k - k0] for k0 <= k < k1 = sum over the slices
 * covering k of irfft(S[:, q]) (rotated back by `roll`) [k - (first + q hop)] * dual_window[k - (first + q hop)].
 * S: [C][nfft/2+1][n_slices]. */
int qi_sliding_istft(int dtype, int device, const void* S, int64_t n_channels, const void* dual_window, int64_t seg,
                     int64_t hop, int64_t nfft, int64_t first, int64_t n_slices, int64_t roll, int64_t k0, int64_t k1,
                     void* out, void* scratch, int64_t scratch_bytes, qi_stream stream);

/* ---- 1-D Shannon information of a record and of its spectrum (tfr_info.py:97-200) --------------------------------
 * Shannon / get_info_and_entropy_32 (tfr_info.py:97-133) on marginals [C][n]: info = -log2(m + eps32),
 * entropy = m * info, isnr = log2(n) - info, esnr = entropy / (log2(n) / n).  Any output may be NULL. */
int qi_shannon_1d(int dtype, int device, const void* marginal, int64_t n_channels, int64_t n, void* info, void* entropy,
                  void* isnr, void* esnr, qi_stream stream);
/* scratch for the two calls below */
int64_t qi_shannon_scratch_bytes(int dtype, int64_t n_channels, int64_t n);
/* ShannonTDR (tfr_info.py:138-147): sig_norm = sig / sqrt(sum sig^2) (may be NULL), marginal = sig_norm^2.  [C][n]. */
int qi_shannon_tdr(int dtype, int device, const void* sig, int64_t n_channels, int64_t n, void* sig_norm, void* marginal,
                   void* scratch, int64_t scratch_bytes, qi_stream stream);
/* ShannonFFT (tfr_info.py:163-183): spectrum = rfft(sig) [C][n/2+1] complex, angle = np.unwrap(np.angle(spectrum))
 * (may be NULL), marginal = |spectrum|^2 / sum |spectrum|^2. */
int qi_shannon_fft(int dtype, int device, const void* sig, int64_t n_channels, int64_t n, void* spectrum, void* angle,
                   void* marginal, void* scratch, int64_t scratch_bytes, qi_stream stream);

/* ---- pooling along time (utilities/sampling.py) -------------------------------------------------------------------- */
typedef enum { QI_POOL_NTH = 0, QI_POOL_AVERAGE = 1, QI_POOL_MAX = 2, QI_POOL_MIN = 3, QI_POOL_MEDIAN = 4 } qi_pool_method;
typedef enum { QI_POOL_REAL = 0,     /* real in  -> real out                                   */
               QI_POOL_COMPLEX = 1,  /* complex in -> complex out; NTH and AVERAGE only        */
               QI_POOL_POWER = 2     /* complex in -> real out, of P = power_scale * |z|^2     */ } qi_pool_input;

/* columns of the result: ceil(n / factor) for NTH, floor(n / factor) otherwise (sampling.py:106-120: the tail that does
 * not fill a window is dropped, except for "nth"); negative qi_status for factor < 2, n < 1 or an unknown method.  Host only. */
int64_t qi_pool_columns(int64_t n, int64_t factor, int method);

/* utilities.sampling.subsample_2d / subsample (sampling.py:14-50,87-120) on a device panel in [rows][n] -> out [rows][columns],
 * both C-contiguous; rows = channels * bands.  power_scale: 0 is read as 1 (QI_POOL_POWER only).  One kernel launch, no
 * atomics: the average accumulates in float64 in a fixed order and is rounded once, the other methods return input values
 * (the median of an even window the mean of its two middle values, in the input precision).  MEDIAN sorts each window in
 * LDS and takes factor <= 4096 (QI_ERR_UNSUPPORTED above); a result of 0 columns is a successful no-op. */
int qi_pool_panel(int dtype, int device, const void* in, int input_kind, int64_t rows, int64_t n, int64_t factor,
                  int method, double power_scale, void* out, qi_stream stream);

/* A column range of a complex device panel in [rows][row_stride], pooled as subsample_2d pools it (sampling.py:87-120:
 * "average" and "max" of P = power_scale * |z|^2; 0 is read as 1) and summed as the transforms' reductions sum it
 * (tfr_info.py:203-236: the entropy of a panel from sum P and sum P log2 P), all from ONE read of the range: the columns
 * [first, first + windows * factor) of every row, any `first`, any factor >= 2.  mean_out, max_out: real [rows][out_stride],
 * one value per window (the average accumulated in float64 and rounded once, the maximum an input value); sums_out: float64
 * [rows][3] = {max P, sum P, sum P log2 P} over the range, 0 log2 0 = 0.  Any of the three may be NULL.  No atomics, a fixed
 * order of summation: the same call gives the same bits.  windows = 0 is a successful no-op.  With sums_out and few rows the
 * per-row sums are finished by a second small launch from a 196 KB buffer the library keeps per (device, stream). */
int qi_pool_strip(int dtype, int device, const void* in, int64_t rows, int64_t row_stride, int64_t first, int64_t factor,
                  int64_t windows, double power_scale, void* mean_out, void* max_out, int64_t out_stride, void* sums_out,
                  qi_stream stream);
/* qi_pool_strip's sums [records][bands][3] -> a transform's statistics [records][4] = {max over bands, sum, sum, 0}
 * (qi_tfr_out.stats), float64, in a fixed order. */
int qi_pool_strip_stats(int device, const void* sums, int64_t records, int64_t bands, void* stats, qi_stream stream);

/* ---- STFT with the plan transforms' outputs --------------------------------------------------------------------------
 * qi_stft's transform (styx_fft.stft_complex_pow2 / stft_from_sig) into a qi_tfr_out: any of coef (= Z [C][nfft/2+1][n_seg])
 * and bits may be NULL -- no panel is stored then --, and the reductions of P = power_scale |Z|^2 come from the kernel that forms the
 * coefficients: power_band [C][nfft/2+1] float64 (sum over the segments), power_time [C][n_seg] in the record's precision
 * (sum over the bins), stats [C][4] float64 {max P, sum P, sum P log2 P, 0} (tfr_info.py:65-94,203-236, whose 2-D entropy
 * classes are named after this transform).  power_band and stats come together; power_time may be NULL beside them.  All
 * five NULL is QI_ERR_ARG.  No atomics, fixed orders of summation: a record's reductions are the same bits alone and in a
 * batch, with both panels stored and with none.  With coef and bits only the call is qi_stft.  eps as in qi_stft.
 * Power-of-two nfft of 64 .. 4096 (float64: .. 2048) run one fused kernel and a small tail; other lengths form the panel
 * with hipFFT (in `coef`, or in scratch) and reduce it with the hipFFT engine's epilogue.
 * scratch: caller-owned device buffer of qi_stft_out_scratch_bytes() for the same want_coef = (coef != NULL). */
int64_t qi_stft_out_scratch_bytes(int dtype, int64_t n_channels, int64_t n, int64_t seg, int64_t hop, int64_t nfft,
                                  int want_coef, int want_bits);
int qi_stft_out(int dtype, int device, const void* sig, int64_t n_channels, int64_t n, const void* window, int64_t seg,
                int64_t hop, int64_t nfft, double scale, const qi_tfr_out* out, void* scratch, int64_t scratch_bytes,
                qi_stream stream);

/* ---- zero-phase IIR filtering (styx_fft.py:60-149 butter_bandpass / butter_highpass / butter_lowpass: scipy.signal.filtfilt;
 * utilities/picker.py:56-76 apply_bandpass: scipy.signal.sosfiltfilt) ----------------------------------------------------
 * Per record: x[k] <- x[k] * taper[k] when a taper is given (the product formed in float64 and rounded to the record's
 * type); the odd extension [2 x[0] - x[edge] .. 2 x[0] - x[1], x, 2 x[n-1] - x[n-2] .. 2 x[n-1] - x[n-1-edge]] in the
 * record's type; then in float64 the recurrence over the extension from the state zi * ext[0], the recurrence over the
 * reversed result from the state zi * (its last value), and out[k] = the second pass's value at extended position edge + k.
 *   QI_IIR_BA  (N = order):  y = b0 x + z0;  z_i = (b_{i+1} x + z_{i+1}) - a_{i+1} y  (i < N - 1);  z_{N-1} = b_N x - a_N y
 *   QI_IIR_SOS (per sample through the sections in order):  xn = b0 xc + z0;  z0 = (b1 xc - a1 xn) + z1;  z1 = b2 xc - a2 xn;  xc = xn
 * Every product and sum is rounded on its own (no fused multiply-add), in this order: scipy.signal.lfilter's / sosfilt's,
 * so a float64 result is SciPy's bit for bit for the same tables.
 * sig [C][n] in dtype (device), any n > edge >= 0; taper [n] float64 (device) or NULL; out [C][n] float64 whatever the
 * dtype (the reference returns float64 for float32 records too).  coef, zi: HOST float64 --
 *   QI_IIR_BA:  coef [2][order + 1] = b then a, zi [order] (scipy.signal.lfilter_zi); sections = 1, 1 <= order <= 16
 *   QI_IIR_SOS: coef [sections][6] = b0 b1 b2 a0 a1 a2, zi [sections][2] (sosfilt_zi); order = 2, 1 <= sections <= 16
 * with a0 = 1 in every section (QI_ERR_ARG otherwise).  edge: samples of extension at each end (filtfilt's padlen:
 * 3 max(len(a), len(b)); sosfiltfilt's: 3 (2 sections + 1 - min(#(b2 == 0), #(a2 == 0)))).
 * scratch: caller-owned device buffer of qi_filtfilt_scratch_bytes() (the forward pass's n + 2 edge values per record),
 * aligned to 8 bytes.  Two kernel launches (forward, backward), no atomics; the same call gives the same bits.  One lane
 * per record: a call of fewer than 64 records takes as long as one of 64 (a record is sequential in time). */
typedef enum { QI_IIR_BA = 0, QI_IIR_SOS = 1 } qi_iir_form;
int64_t qi_filtfilt_scratch_bytes(int64_t n_channels, int64_t n, int64_t edge);
int qi_filtfilt(int dtype, int device, const void* sig, int64_t n_channels, int64_t n, const void* taper, int form,
                int32_t sections, int32_t order, const double* coef, const double* zi, int64_t edge, void* out,
                void* scratch, int64_t scratch_bytes, qi_stream stream);

/* ---- zero-phase decimation (utilities/sampling.py:123-146 decimate_timeseries / decimate_timeseries_collection:
 * scipy.signal.decimate(x, q, zero_phase=True) = sosfiltfilt with the order-8 Chebyshev type I sections, then every q-th sample) ----
 * Per record, ALL in the record's type T (SciPy casts the sections to it; no float64 intermediate for a float32 record):
 * the odd extension by `edge` samples, the QI_IIR_SOS recurrence above over the extension from the state zi * ext[0], the
 * same over the reversed result from the state zi * (its last value), every product and sum rounded on its own in T; then
 * out[c] = the second pass's value at extended position edge + c q, c = 0 .. qi_decimate_columns(n, q) - 1.  For the same
 * tables the result is SciPy's bit for bit in float32 and in float64; in float64 it is qi_filtfilt's every q-th sample.
 * sig [C][n] in dtype (device), any n > edge >= 0, any q >= 1; out [C][ceil(n / q)] in dtype (device).  sos [sections][6]
 * = b0 b1 b2 a0 a1 a2 with a0 = 1, zi [sections][2]: HOST arrays in dtype (float for QI_F32, double for QI_F64),
 * 1 <= sections <= 16.  scratch: caller-owned device buffer of qi_decimate_scratch_bytes() (the forward pass's
 * n + 2 edge values per record in dtype: QI_F32 needs half of QI_F64); sig, out and scratch aligned to the size of dtype.
 * Two kernel launches, no atomics; the backward pass stores only the kept samples, adjacent lanes adjacent columns.
 * qi_decimate_columns: ceil(n / q), negative qi_status for n < 1 or q < 1.  Both size queries are host only. */
int64_t qi_decimate_columns(int64_t n, int64_t q);
int64_t qi_decimate_scratch_bytes(int dtype, int64_t n_channels, int64_t n, int64_t edge);
int qi_decimate(int dtype, int device, const void* sig, int64_t n_channels, int64_t n, int64_t q, int32_t sections,
                const void* sos, const void* zi, int64_t edge, void* out, void* scratch, int64_t scratch_bytes,
                qi_stream stream);

/* ---- scaling and peak picking (utilities/picker.py:32-53 scale_signal_by_extraction_type; picker.py:79-151
 * find_peaks_by_extraction_type, _with_bandpass, find_peaks_with_bits: scipy.signal.find_peaks with height / distance) ------
 * Per record x [n], independently of every other record:
 *  scaling   u = x for the SIG* kinds, u = log2(|x| + eps) in float64 for the LOG2* kinds (eps: 0 is read as 2^-52), and
 *            s = u / nanmax(u) (SIGMAX, LOG2MAX), u / nanmin(u) (SIGMIN), u / nanmax(|u|) (SIGABS), u (LOG2).  The scaled type
 *            is the record's for SIG* and float64 for LOG2*.  The division is IEEE division in that type, no reciprocal and no
 *            special case: a divisor of 0 gives +-inf and NaN, a negative one reverses the order, a record of NaNs stays NaN.
 *  maxima    sample i, 1 <= i <= n - 2, opens a peak when s[i-1] < s[i]; with j the first index behind i with s[j] != s[i]
 *            (at most n - 1) it is a peak when s[j] < s[i], reported at (i + j - 1) / 2 rounded down: the middle of a
 *            plateau of any length; one that starts at sample 0 or reaches sample n - 1 is none.  A NaN compares false.
 *  height    the peak's value, widened to float64, is tested with >= against: nothing (NONE); `height` (ABS); max(s) - height
 *            (BELOW_MAX); max(x) - height (BELOW_RAW_MAX: the maximum of the record itself, the peaks still those of s).  Both
 *            maxima are np.max -- NaN when a sample is, and then there is no peak -- and the difference is formed in the
 *            type of the maximum (the scaled type, the record's type), per record, on the device.
 * Outputs (device; any but counts may be NULL): scaled [C][n] in the scaled type; positions int64 [C][capacity] ascending and
 * values float64 [C][capacity], the scaled value at each peak; counts int64 [C], the peaks found even when more than
 * capacity -- columns from min(count, capacity) on are not written.  positions with capacity 0 is QI_ERR_ARG; with
 * positions and values NULL the call is the scaling (and the count).  Any n >= 1 (n < 3: no peak).
 * Records are cut into tiles of QI_PEAKS_TILE samples.  Five or six kernel launches, four reads of the record (extrema;
 * scaled values and tile summaries; count; store), no atomics and no waiting of one workgroup for another: a plateau that
 * leaves its tile is followed through the summaries the previous launch left in scratch.  The same call gives the same bits.
 * scratch: caller-owned device buffer of qi_peaks_scratch_bytes() bytes, aligned to 8 (host only; negative qi_status for an unknown
 * dtype, n_channels < 1 or n < 1). */
#define QI_PEAKS_TILE 256
typedef enum { QI_PEAK_SIGMAX = 0, QI_PEAK_SIGMIN = 1, QI_PEAK_SIGABS = 2, QI_PEAK_LOG2 = 3, QI_PEAK_LOG2MAX = 4 } qi_peak_scale;
typedef enum { QI_PEAK_HEIGHT_NONE = 0, QI_PEAK_HEIGHT_ABS = 1, QI_PEAK_HEIGHT_BELOW_MAX = 2,
               QI_PEAK_HEIGHT_BELOW_RAW_MAX = 3 } qi_peak_height;
int64_t qi_peaks_scratch_bytes(int dtype, int64_t n_channels, int64_t n);
int qi_find_peaks(int dtype, int device, const void* sig, int64_t n_channels, int64_t n, int scale, double eps, int height_kind,
                  double height, void* scaled, int64_t* positions, double* values, int64_t capacity, int64_t* counts,
                  void* scratch, int64_t scratch_bytes, qi_stream stream);
/* scipy.signal.find_peaks(distance=) on HOST arrays of `count` candidates, positions ascending: from the highest value to
 * the lowest, each candidate still kept removes every other one closer than `distance` samples; keep[i] = 1 for the kept.
 * Among equal values the LATER candidate goes first (a stable ascending sort read from its end; SciPy's own order there is
 * that of an unstable argsort and not defined).  distance < 1 is QI_ERR_ARG with SciPy's message.  Host only, plain C++. */
int qi_peaks_select_distance(const int64_t* positions, const double* values, int64_t count, int64_t distance, uint8_t* keep);

/* ---- resampling (utilities/sampling.py:53-68 resample_uneven_timeseries: np.interp onto np.arange; sampling.py:71-83
 * resample_with_sample_rate: scipy.signal.resample) ---------------------------------------------------------------------------
 * Linear interpolation of records with uneven timestamps onto an even grid, np.interp's semantics.  Per record, with knots
 * xp [n] (float64 timestamps, expected non-decreasing, duplicates allowed) and values fp [n] widened to double, output i is
 *   x = start + (double)i * delta                      (the product rounded first, then the sum: np.arange's values)
 *   x > xp[n-1]: fp[n-1];   x < xp[0]: fp[0];   otherwise with j the last index with xp[j] <= x
 *   j == n-1 or xp[j] == x: fp[j]
 *   else s = (fp[j+1] - fp[j]) / (xp[j+1] - xp[j]),  r = s * (x - xp[j]) + fp[j];  if r is NaN: r = s * (x - xp[j+1]) + fp[j+1];
 *        if that is NaN too and fp[j] == fp[j+1]: r = fp[j]
 * every operation an IEEE double operation rounded on its own (no fused multiply-add, a true division): NumPy's bits.
 * values [C][n] in dtype (device); knots float64 (device): knot_stride 0 = [n], shared by all records, knot_stride n =
 * [C][n], a row of timestamps per record (anything else: QI_ERR_ARG); out [C][m] float64 whatever the dtype (np.interp
 * returns float64 for float32 data).  Any n >= 1, any m >= 0 (m = 0: a successful no-op), delta finite and > 0, start finite.
 * A workgroup forms QI_INTERP_TILE consecutive outputs of one record: it brackets them in the knots with two bounded searches
 * in global memory, then stages the bracketing knots and values in LDS when they are at most QI_INTERP_KNOTS (upsampling, unit
 * rate, downsampling to about a quarter of the rate) and searches there; otherwise its lanes bisect in global memory.  One
 * kernel launch (per 65535 records), no scratch, no atomics; the same call gives the same bits.  The order of the timestamps
 * is not checked, as np.interp does not check it: with unsorted or NaN timestamps the values are undefined, but every search
 * is bounded and every index it forms lies in [0, n-1]. */
#define QI_INTERP_TILE 512   /* outputs of one workgroup */
#define QI_INTERP_KNOTS 2560 /* knots a workgroup stages in LDS */
int qi_interp_grid(int dtype, int device, const void* values, const void* knots, int64_t knot_stride, int64_t n_channels,
                   int64_t n, double start, double delta, int64_t m, void* out, qi_stream stream);

/* scipy.signal.resample(x, m) of real records along time, no window, domain="time": the m / 2 + 1 bins of the output spectrum
 * are the input's bins 0 .. N / 2, N = min(n, m) -- for an even N the bin N / 2 times 2 when m < n, times 0.5 when n < m --
 * and zeros above; the result is the inverse real transform of length m times m / n.  sig [C][n] -> out [C][m], both in
 * dtype (SciPy keeps float32 for float32 records).  Any n >= 1, any m >= 1 (below 2^31).  A batched real-to-complex hipFFT
 * of length n, one kernel for the spectrum (it also applies the 1 / n), a batched complex-to-real hipFFT of length m.
 * scratch: caller-owned device buffer of qi_resample_fft_scratch_bytes() bytes (a copy of the records and the two spectra),
 * aligned to 16 (host only; negative qi_status for an unknown dtype, n_channels < 1, n < 1, m < 1 or sizes out of range). */
int64_t qi_resample_fft_scratch_bytes(int dtype, int64_t n_channels, int64_t n, int64_t m);
int qi_resample_fft(int dtype, int device, const void* sig, int64_t n_channels, int64_t n, int64_t m, void* out,
                    void* scratch, int64_t scratch_bytes, qi_stream stream);

/* ---- integration and differentiation (utilities/calculations.py:16-63, 118-157: scipy.integrate.cumulative_trapezoid with
 * initial=0, np.gradient with edge_order 1, np.diff) -----------------------------------------------------------------------
 * Cumulative trapezoid of records y [C][n] (device, dtype).  x NULL: a constant spacing dx; otherwise float64 timestamps
 * (device), x_stride 0 = [n], shared by all records, x_stride n = [C][n], a row per record (anything else: QI_ERR_ARG).
 * Term i, 0 <= i < n - 1, in SciPy's order and types, every operation rounded on its own:
 *   with x:  (x[i+1] - x[i]) * (double)(y[i+1] + y[i]) / 2.0     the sum in dtype first, the rest float64; out is float64
 *   with dx: (T)dx * (y[i+1] + y[i]) / 2                          all in dtype T, dx rounded to it once; out is in dtype
 * out [C][n] (device): out[0] = 0, out[i+1] = the sum of the terms 0 .. i.  The terms are SciPy's bits; the order in which
 * they are added is not NumPy's left-to-right one but a fixed tree that depends on n alone (not on C, on the record's row,
 * on the grid or on the run), R the result type:
 *   the terms are cut into tiles of QI_SCAN_TILE; the last tile's missing terms are +0.0;
 *   lane l (of 256) of a tile sums its terms 16 l .. 16 l + 15 left to right: r_0 = t_0, r_k = r_(k-1) + t_k;
 *   the 64 lane totals r_15 of a wave go through an inclusive Hillis-Steele scan, steps 1, 2, 4, 8, 16, 32 (at step s
 *     every lane l >= s takes v_(l-s) + v_l, all at once); e_l = the scanned value of lane l - 1, e_0 = 0; W_w = that of lane 63;
 *   the four wave totals left to right: o_0 = 0, o_1 = W_0, o_2 = W_0 + W_1, o_3 = o_2 + W_2; the tile's total T = o_3 + W_3;
 *   the tile totals of a record left to right: c_0 = 0, c_1 = T_0, c_t = c_(t-1) + T_(t-1);
 *   out[QI_SCAN_TILE t + 16 l + k + 1] = (c_t + (o_w + e_l)) + r_k.
 * Three kernel launches (tile totals; carries per record; the terms again, the scan and the stores), no atomics, no waiting
 * of one workgroup for another; the same call gives the same bits.  Any n >= 1 (n = 1: out[0] = 0); n_channels = 0 is a
 * successful no-op; a refused call writes nothing.
 * scratch: caller-owned device buffer of qi_cumtrapz_scratch_bytes() bytes ([C][tiles] of float64), aligned to 8 (host only;
 * negative qi_status for an unknown dtype, n_channels < 0, n < 1 or sizes out of range). */
#define QI_SCAN_TILE 4096
int64_t qi_cumtrapz_scratch_bytes(int dtype, int64_t n_channels, int64_t n);
int qi_cumtrapz(int dtype, int device, const void* y, const void* x, int64_t x_stride, double dx, int64_t n_channels, int64_t n,
                void* out, void* scratch, int64_t scratch_bytes, qi_stream stream);

/* Derivative of records y [C][n] (device, dtype T); x and x_stride as above; one kernel launch, no scratch; NumPy's bits.
 * QI_DERIV_GRADIENT (n >= 2, out_offset 0): out [C][n] in dtype.
 *   x NULL: out[i] = (y[i+1] - y[i-1]) / (T)(2.0 * h) inside, (y[1] - y[0]) / (T)h and (y[n-1] - y[n-2]) / (T)h at the ends.
 *   with x: dx1 = x[i] - x[i-1], dx2 = x[i+1] - x[i], a = -(dx2) / (dx1 * (dx1 + dx2)), b = (dx2 - dx1) / (dx1 * dx2),
 *           c = dx1 / (dx2 * (dx1 + dx2)), out[i] = (T)((a * y[i-1] + b * y[i]) + c * y[i+1]) in float64 inside; at the ends
 *           (T)((double)(y[1] - y[0]) / (x[1] - x[0])) and the same of the last two samples, the difference in dtype.
 *           (np.gradient itself takes the first form when all x[i+1] - x[i] are equal: that choice is the caller's.)
 * QI_DERIV_DIFFERENCE (n >= 1): n - 1 values, written to columns out_offset .. out_offset + n - 2 of out [C][n], out_offset 0
 *   or 1; the column left over (n - 1 or 0: the fill slot) is not written.
 *   x NULL: (y[i+1] - y[i]) * (T)h in dtype -- h is the FACTOR here (np.diff(y) * sample_rate); out is in dtype.
 *   with x: (double)(y[i+1] - y[i]) / (x[i+1] - x[i]), the difference in dtype; out is float64.
 * Equal timestamps divide by zero as in NumPy (inf, NaN).  n_channels = 0 is a successful no-op; a refused call writes nothing. */
typedef enum { QI_DERIV_GRADIENT = 0, QI_DERIV_DIFFERENCE = 1 } qi_deriv_kind;
int qi_derivative(int dtype, int device, int kind, const void* y, const void* x, int64_t x_stride, double h, int64_t n_channels,
                  int64_t n, void* out, int64_t out_offset, qi_stream stream);

/* ---- synthetic records (synth/benchmark_signals.py, synth/synthetic_signals.py, synth/blast_gt_pulse.py, synth/doppler.py) ----
 * qi_synth writes records out [C][n] (complex_out 0) or [C][n][2] interleaved (complex_out 1; the imaginary part is 0 for every
 * kind but QI_SYNTH_QCHIRP) in dtype (device) from a closed formula.  Sample k of record c is evaluated in float64 and rounded
 * once to dtype.  Every operation below is an IEEE double operation rounded on its own (no fused multiply-add, true divisions),
 * so the argument of every sin, cos, exp and log is NumPy's bit for bit; kinds without one are NumPy's result bit for bit.
 * Parameters: params (device, float64), QI_SYNTH_PARAMS values per row; param_stride 0 = one row for all records,
 *   QI_SYNTH_PARAMS = a row per record (anything else: QI_ERR_ARG).  p0 .. p11 below are the row's values.
 * Time: t = (base(k) - s0) - s1, each subtraction rounded on its own, with base(k) by `axis`:
 *   QI_AXIS_RATE        (double)k / axis_value       np.arange(n) / rate          x NULL, x_stride 0
 *   QI_AXIS_STEP        (double)k * axis_value       np.arange(n) * step          x NULL, x_stride 0
 *   QI_AXIS_TIMESTAMPS  x[k]                         x float64 (device): x_stride 0 = [n] shared, x_stride n = [C][n]
 *   s0 and s1 are the caller's (time[-1] / 2.0, sensor_epoch_s[0], ...; 0.0 subtracts nothing).
 * Kinds, v = the sample (sq(u) = u * u):
 *   QI_SYNTH_TONE          cos(p0 * t)                                                      p0 = 2 pi f_c
 *   QI_SYNTH_SINES3        (g0 + g1) + g2, g_i = sin(p_i * t) where p(3+2i) <= t <= p(4+2i), +0.0 elsewhere (rectangular gates)
 *   QI_SYNTH_01            cos(p0 * t - (p1 * t) * t) + cos(p3 * sin(p2 * t) + p4 * t)
 *   QI_SYNTH_02            ((u0 + u1) + u2) + u3, u_q = exp(p(3q) * sq(t - p(3q+1))) * cos(p(3q+2) * t)
 *   QI_SYNTH_03            cos(p0 * log(p1 * t + 1.0)) + cos(p2 * t + p3 * sq(t))
 *   QI_SYNTH_QCHIRP        q = t / p2, phase = p0 * t + p1 * sq(q), amp = p3 != 0 ? exp(-0.5 * sq(q)) : 1;
 *                          v = (amp * cos(phase), amp * sin(phase))     p0 omega, p1 gamma / 2, p2 the chirp scale, p3 gauss
 *   QI_SYNTH_CHIRP_LINEAR  cos(2 pi * (p0 * t + (p1 * t) * t) + 0.0)     p0 = f0, p1 = beta / 2 (scipy.signal.chirp, linear, phi 0)
 *   QI_SYNTH_SAWTOOTH      r = fmod(p0 * t, 2 pi); r < 0: r += 2 pi; r == 0: r = +0.0; v = (pi - r) / pi   (sawtooth, width 0;
 *                          with the timestamp axis, s0 = s1 = 0 and p0 = 1 the "timestamps" are a phase record)
 *   QI_SYNTH_GT, _GT_HILBERT, _GT_DERIVATIVE, _GT_INTEGRAL: tau = t / p0 + 1.0 (p0 a quarter of the pseudo period), a = 1 + sqrt(6);
 *     on 0 <= tau <= 1 and on 1 < tau <= a the expressions of blast_gt_pulse.py:23-71, 140-196 in their written order, +0.0
 *     elsewhere; tau^3 of the integral correctly rounded; p1 = the integral's integration_constant, added on 1 < tau <= a.
 * Envelope, applied to v:
 *   QI_ENVELOPE_NONE
 *   QI_ENVELOPE_TUKEY  v * tukey(n, alpha)[k]: scipy.signal.windows.tukey, symmetric (alpha <= 0 or n == 1: ones; alpha >= 1: Hann)
 *   QI_ENVELOPE_GATE   benchmark_signals.signal_gate: +0.0 where t < tmin or t > tmax; v * tukey(m, alpha)[k - k0] where
 *                      tmin <= t <= tmax.  k0 = the first included sample and m = their count are the caller's, found with the
 *                      same rounded t(k); 0 <= k0, 0 <= m, k0 + m <= n (anything else: QI_ERR_ARG).
 * A workgroup forms QI_SYNTH_TILE consecutive samples of one record.  One kernel launch (per 65535 records), no scratch, no
 * atomics; the same call gives the same bits.  Any n >= 1; n_channels = 0 is a successful no-op; a refused call writes nothing. */
#define QI_SYNTH_TILE 1024  /* samples of one workgroup */
#define QI_SYNTH_PARAMS 12  /* float64 values of a parameter row of qi_synth */
#define QI_DOPPLER_PARAMS 12 /* float64 values of a parameter row of qi_doppler */
typedef enum { QI_SYNTH_TONE = 0, QI_SYNTH_SINES3 = 1, QI_SYNTH_01 = 2, QI_SYNTH_02 = 3, QI_SYNTH_03 = 4, QI_SYNTH_QCHIRP = 5,
               QI_SYNTH_CHIRP_LINEAR = 6, QI_SYNTH_SAWTOOTH = 7, QI_SYNTH_GT = 8, QI_SYNTH_GT_HILBERT = 9,
               QI_SYNTH_GT_DERIVATIVE = 10, QI_SYNTH_GT_INTEGRAL = 11, QI_SYNTH_KINDS = 12 } qi_synth_kind;
typedef enum { QI_AXIS_RATE = 0, QI_AXIS_STEP = 1, QI_AXIS_TIMESTAMPS = 2 } qi_synth_axis;
typedef enum { QI_ENVELOPE_NONE = 0, QI_ENVELOPE_TUKEY = 1, QI_ENVELOPE_GATE = 2 } qi_synth_envelope;
int qi_synth(int dtype, int device, int kind, int complex_out, const double* params, int64_t param_stride, int axis,
             double axis_value, const double* x, int64_t x_stride, double s0, double s1, int envelope, double alpha, double tmin,
             double tmax, int64_t k0, int64_t m, int64_t n_channels, int64_t n, void* out, qi_stream stream);

/* doppler._get_final_vals (doppler.py:149-207) for a row of times per record; the axis, x, s0 and s1 as for qi_synth.  A
 * parameter row (param_stride 0 or QI_DOPPLER_PARAMS) is c, c2, denom, the source velocity s[3], the receiver velocity v[3]
 * and the initial range r[3] = receiver - source: c2 = c**2 and denom = 1. / (c**2 - speed**2) (the receiver's speed forward,
 * the source's inverse) are the caller's, by the reference's own expressions.  dot(a, b) = (a0 b0 + a1 b1) + a2 b2.  Per sample:
 *   forward:  q = r - s * t;  term1 = (c2 * t + dot(v, q)) * denom        inverse:  q = r + v * t;  term1 = (c2 * t - dot(s, q)) * denom
 *   rm = sqrt(dot(q, q));  term2 = (rm * rm - (t * c) * (t * c)) * denom;  root = sqrt(term1 * term1 + term2)
 *   forward:  time = term1 + root;  g = q + v * time                     inverse:  time = term1 - root;  g = q - s * time
 *   range = sqrt(dot(g, g));  omega = (c - dot(g, v) / range) / (c - dot(g, s) / range)
 * every operation an IEEE double operation rounded on its own.  time_out, range_out, omega_out: [C][n] float64 (device).  One
 * kernel launch (per 65535 records), no scratch, no atomics; n_channels = 0 is a successful no-op; a refused call writes nothing. */
int qi_doppler(int device, int inverse, const double* params, int64_t param_stride, int axis, double axis_value, const double* x,
               int64_t x_stride, double s0, double s1, int64_t n_channels, int64_t n, double* time_out, double* range_out,
               double* omega_out, qi_stream stream);

/* ---- the STFT of a segment range: a record that is streamed through the device piece by piece --------------------------------
 * The record has n_total samples and qi_stft_segments(n_total, seg, hop) segments; segment m covers the record samples
 * [m hop - seg / 2, m hop - seg / 2 + seg), and samples outside [0, n_total) are zeros that count in the segment mean (the
 * boundary extension and padded=True of qi_stft).  A segment depends on its own samples only, so the ranges of a record
 * give the coefficients of the one-call transform, and their sums add up to its reductions.
 *   first_segment, segments     the range; the outputs are those of the qi_stft_out form with n_seg = segments: coef / bits
 *                               [C][nfft/2+1][segments], power_band [C][nfft/2+1] and stats over these segments only,
 *                               power_time [C][segments]
 *   sample0, n_avail, row_stride  row c of sig holds the record samples sample0 .. sample0 + n_avail - 1 at
 *                               sig[c * row_stride + i]; nothing outside [0, n_avail) of a row is read.  Every record sample
 *                               that a segment of the range covers must lie in that interval (qi_stft_range_samples gives the
 *                               smallest one); n_avail = 0 is valid for a range inside the zero extension (sig may then be NULL)
 *   pool_factor F               0: no pooling (pool_mean and pool_max NULL); F >= 2: pool_mean / pool_max, real
 *                               [C][nfft/2+1][segments / F] in the record's precision, either may be NULL -- the average
 *                               (accumulated in float64 in a fixed order, rounded once) and the maximum (one of the values)
 *                               of P = power_scale |Z|^2 over the windows of F consecutive segments.  first_segment % F == 0
 *                               and segments % F == 0, except that a range ending at the record's last segment may be ragged:
 *                               its incomplete window is dropped (utilities/sampling.py:106-120).  They come with power_band.
 * Anything else is QI_ERR_ARG, found on the host before any device call.  At the fused transform lengths the pooled values
 * leave the kernel as the per-workgroup sums (and maxima) of every bin -- a workgroup holds min(its usual count, the largest
 * power of two dividing F) consecutive segments -- and one small kernel folds F / that many groups in index order: no panel
 * is stored, no atomics.  Other lengths pool the hipFFT panel (in coef, or in scratch) with the strip kernel.  With
 * first_segment = 0, every segment, sample0 = 0, n_avail = row_stride = n_total and F = 0 the call is the qi_stft_out form:
 * the same launches, the same bits.  The ShortTimeFFT-convention pad modes are not offered for ranges. */
typedef struct qi_stft_range {
  int64_t n_total;
  int64_t first_segment, segments;
  int64_t sample0, n_avail, row_stride;
  int64_t pool_factor;
  void* pool_mean;
  void* pool_max;
} qi_stft_range;
/* the smallest sample interval of a range: *sample0 its first record sample, *n_avail their count (0: none).  Host only. */
int qi_stft_range_samples(int64_t n_total, int64_t seg, int64_t hop, int64_t first_segment, int64_t segments, int64_t* sample0,
                          int64_t* n_avail);
/* scratch of qi_stft_out_range for this range and want_coef = (coef != NULL); a negative qi_status for a range it refuses */
int64_t qi_stft_range_scratch_bytes(int dtype, int64_t n_channels, int64_t seg, int64_t hop, int64_t nfft,
                                    const qi_stft_range* range, int want_coef);
int qi_stft_out_range(int dtype, int device, const void* sig, int64_t n_channels, const void* window, int64_t seg, int64_t hop,
                      int64_t nfft, double scale, const qi_stft_range* range, const qi_tfr_out* out, void* scratch,
                      int64_t scratch_bytes, qi_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* QI_TFR_H */
