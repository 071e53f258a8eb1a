"""ctypes binding of libqi_tfr.so (include/qi_tfr.h, qi_array.h, qi_beam.h, qi_adaptive.h, qi_subspace.h, qi_steer.h, qi_windows.h,
qi_lags.h, qi_bands.h, qi_timebeam.h, qi_squeeze.h).  There is no CPU fallback: if the
library is missing or no HIP device is present, every transform raises."""
import ctypes as C
import os

import torch  # first: its bundled HIP runtime must be the one libqi_tfr.so resolves against

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("QI_TFR_LIB") or os.path.join(_HERE, "libqi_tfr.so")  # QI_TFR_LIB: diagnostic builds

QI_F32, QI_F64 = 0, 1
QI_BANK_STYX, QI_BANK_ATOMS, QI_TABLE_STX = 0, 1, 2
QI_ENGINE_AUTO, QI_ENGINE_HIPFFT, QI_ENGINE_NATIVE = 0, 1, 2
STAGES = ("forward", "multiply", "inverse", "epilogue", "pass1", "pass2", "block", "zoom", "zoom_coarse", "small")
# qi_band_route.flags (QI_ROUTE_* of include/qi_tfr.h)
QI_POOL_NTH, QI_POOL_AVERAGE, QI_POOL_MAX, QI_POOL_MIN, QI_POOL_MEDIAN = 0, 1, 2, 3, 4
QI_POOL_REAL, QI_POOL_COMPLEX, QI_POOL_POWER = 0, 1, 2
QI_IIR_BA, QI_IIR_SOS = 0, 1
QI_PEAK_SIGMAX, QI_PEAK_SIGMIN, QI_PEAK_SIGABS, QI_PEAK_LOG2, QI_PEAK_LOG2MAX = 0, 1, 2, 3, 4
QI_PEAK_HEIGHT_NONE, QI_PEAK_HEIGHT_ABS, QI_PEAK_HEIGHT_BELOW_MAX, QI_PEAK_HEIGHT_BELOW_RAW_MAX = 0, 1, 2, 3
PEAKS_TILE = 256  # samples per tile of qi_find_peaks (QI_PEAKS_TILE of include/qi_tfr.h)
INTERP_TILE, INTERP_KNOTS = 512, 2560  # outputs of a workgroup of qi_interp_grid, knots it stages in LDS (QI_INTERP_TILE, QI_INTERP_KNOTS)
SCAN_TILE = 4096  # terms of one tile of qi_cumtrapz's summation tree (QI_SCAN_TILE)
QI_DERIV_GRADIENT, QI_DERIV_DIFFERENCE = 0, 1
SYNTH_TILE, SYNTH_PARAMS, DOPPLER_PARAMS = 1024, 12, 12  # samples of a workgroup of qi_synth, values of a parameter row (QI_SYNTH_TILE, QI_SYNTH_PARAMS, QI_DOPPLER_PARAMS)
SYNTH_KINDS = ("tone", "sines3", "synth_01", "synth_02", "synth_03", "quantum_chirp", "chirp_linear", "sawtooth", "gt", "gt_hilbert",
               "gt_derivative", "gt_integral")  # qi_synth_kind, in its order
QI_AXIS_RATE, QI_AXIS_STEP, QI_AXIS_TIMESTAMPS = 0, 1, 2
QI_ENVELOPE_NONE, QI_ENVELOPE_TUKEY, QI_ENVELOPE_GATE = 0, 1, 2
IIR_MAX = 16  # largest order of the (b, a) form, most second-order sections (qi_filtfilt)
POOL_MEDIAN_MAX = 4096  # longest window the median sorts (qi_pool_panel)
ROUTE_NOWRAP, ROUTE_SPLIT, ROUTE_BEHIND, ROUTE_F64_ZOOM = 16, 32, 256, 512


def route_analytic(flags):
    return flags & 3


def route_narrow(flags):
    return (flags >> 2) & 3


def route_pass2_kind(flags):
    return (flags >> 6) & 3


class QiError(RuntimeError):
    pass


class PlanDesc(C.Structure):
    _fields_ = [
        ("n", C.c_int64),
        ("dtype", C.c_int32),
        ("device", C.c_int32),
        ("engine", C.c_int32),
        ("flags", C.c_int32),
        ("workspace_bytes", C.c_int64),
    ]


class BandRoute(C.Structure):
    _fields_ = [("stage", C.c_int32), ("cls", C.c_int32), ("run_cls", C.c_int32), ("flags", C.c_int32)]


class TfrOut(C.Structure):
    _fields_ = [
        ("coef", C.c_void_p),
        ("bits", C.c_void_p),
        ("power_band", C.c_void_p),
        ("power_time", C.c_void_p),
        ("stats", C.c_void_p),
        ("power_scale", C.c_double),
        ("eps", C.c_double),
    ]


class StftRange(C.Structure):
    _fields_ = [
        ("n_total", C.c_int64),
        ("first_segment", C.c_int64),
        ("segments", C.c_int64),
        ("sample0", C.c_int64),
        ("n_avail", C.c_int64),
        ("row_stride", C.c_int64),
        ("pool_factor", C.c_int64),
        ("pool_mean", C.c_void_p),
        ("pool_max", C.c_void_p),
    ]


_P = C.c_void_p
_D = C.POINTER(C.c_double)
_I64 = C.POINTER(C.c_int64)
_i64, _i32, _int, _dbl = C.c_int64, C.c_int32, C.c_int, C.c_double

# name -> (restype, argtypes); mirrors include/qi_tfr.h one to one
PROTOTYPES = {
    "qi_abi_version": (_int, []),
    "qi_last_error": (C.c_char_p, []),
    "qi_device_info": (_int, [_int, C.c_char_p, C.c_size_t, _I64, C.POINTER(_i32)]),
    "qi_plan_create": (_int, [C.POINTER(_P), C.POINTER(PlanDesc)]),
    "qi_plan_destroy": (_int, [_P]),
    "qi_plan_set_gabor_bank": (_int, [_P, _int, _i32, _D, _D, _D, _D, _P]),
    "qi_gabor_atoms": (_int, [_int, _i64, _i32, _D, _D, _D, _D, _P, _P]),
    "qi_gabor_atoms_at": (_int, [_int, _i64, _i32, _D, _D, _D, _D, _P, _P, _P]),
    "qi_plan_set_stx_bands": (_int, [_P, _i32, _I64, _D]),
    "qi_plan_bands": (_i64, [_P, _int]),
    "qi_plan_stage_bands": (_i64, [_P, _int, _int]),
    "qi_plan_forward_low": (_i64, [_P, _int]),
    "qi_plan_joint_planes": (_i64, [_P, _int]),
    "qi_plan_band_route": (_int, [_P, _int, _i32, _i64, C.POINTER(BandRoute)]),
    "qi_plan_profile": (_int, [_P, _int]),
    "qi_plan_profile_read": (_int, [_P, _D, _I64, _i32]),
    "qi_cwt": (_int, [_P, _int, _P, _i64, C.POINTER(TfrOut), _P]),
    "qi_stx": (_int, [_P, _P, _i64, C.POINTER(TfrOut), _P]),
    "qi_cwt_stx": (_int, [_P, _int, _P, _i64, C.POINTER(TfrOut), C.POINTER(TfrOut), _P]),
    "qi_stft_segments": (_i64, [_i64, _i64, _i64]),
    "qi_stft_scratch_bytes": (_i64, [_int, _i64, _i64, _i64, _i64, _i64]),
    "qi_stft": (_int, [_int, _int, _P, _i64, _i64, _P, _i64, _i64, _i64, _dbl, _P, _P, _dbl, _P, _i64, _P]),
    "qi_stft_out_scratch_bytes": (_i64, [_int, _i64, _i64, _i64, _i64, _i64, _int, _int]),
    "qi_stft_out": (_int, [_int, _int, _P, _i64, _i64, _P, _i64, _i64, _i64, _dbl, C.POINTER(TfrOut), _P, _i64, _P]),
    "qi_welch_scratch_bytes": (_i64, [_int, _i64, _i64, _i64, _i64, _i64]),
    "qi_welch": (_int, [_int, _int, _P, _i64, _i64, _P, _i64, _i64, _i64, _dbl, _P, _P, _i64, _P]),
    "qi_power_marginals": (_int, [_int, _int, _P, _i64, _i64, _i64, _P, _P, _P, _P, _i64, _P]),
    "qi_power_marginals_scratch_bytes": (_i64, [_i64, _i64, _i64]),
    "qi_log2_offset": (_int, [_int, _int, _P, _P, _i64, _i64, _dbl, _P, _P]),
    "qi_widen": (_int, [_int, _P, _P, _i64, _P]),
    "qi_log2_abs": (_int, [_int, _int, _P, _int, _P, _i64, _dbl, _P]),
    "qi_shannon_panel": (_int, [_int, _int, _P, _P, _int, _i64, _i64, _i64, _dbl, _P, _P, _P, _P, _P]),
    "qi_sliding_scratch_bytes": (_i64, [_int, _i64, _i64, _i64]),
    "qi_sliding_stft": (_int, [_int, _int, _P, _i64, _i64, _P, _i64, _i64, _i64, _i64, _i64, _int, _int, _i64, _P, _P, _int, _P, _i64, _P]),
    "qi_sliding_istft": (_int, [_int, _int, _P, _i64, _P, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _P, _P, _i64, _P]),
    "qi_shannon_1d": (_int, [_int, _int, _P, _i64, _i64, _P, _P, _P, _P, _P]),
    "qi_shannon_scratch_bytes": (_i64, [_int, _i64, _i64]),
    "qi_shannon_tdr": (_int, [_int, _int, _P, _i64, _i64, _P, _P, _P, _i64, _P]),
    "qi_shannon_fft": (_int, [_int, _int, _P, _i64, _i64, _P, _P, _P, _P, _i64, _P]),
    "qi_pool_columns": (_i64, [_i64, _i64, _int]),
    "qi_pool_panel": (_int, [_int, _int, _P, _int, _i64, _i64, _i64, _int, _dbl, _P, _P]),
    "qi_pool_strip": (_int, [_int, _int, _P, _i64, _i64, _i64, _i64, _i64, _dbl, _P, _P, _i64, _P, _P]),
    "qi_pool_strip_stats": (_int, [_int, _P, _i64, _i64, _P, _P]),
    "qi_filtfilt_scratch_bytes": (_i64, [_i64, _i64, _i64]),
    "qi_filtfilt": (_int, [_int, _int, _P, _i64, _i64, _P, _int, _i32, _i32, _D, _D, _i64, _P, _P, _i64, _P]),
    "qi_decimate_columns": (_i64, [_i64, _i64]),
    "qi_decimate_scratch_bytes": (_i64, [_int, _i64, _i64, _i64]),
    "qi_decimate": (_int, [_int, _int, _P, _i64, _i64, _i64, _i32, _P, _P, _i64, _P, _P, _i64, _P]),
    "qi_peaks_scratch_bytes": (_i64, [_int, _i64, _i64]),
    "qi_find_peaks": (_int, [_int, _int, _P, _i64, _i64, _int, _dbl, _int, _dbl, _P, _P, _P, _i64, _P, _P, _i64, _P]),
    "qi_peaks_select_distance": (_int, [_P, _P, _i64, _i64, _P]),
    "qi_interp_grid": (_int, [_int, _int, _P, _P, _i64, _i64, _i64, _dbl, _dbl, _i64, _P, _P]),
    "qi_resample_fft_scratch_bytes": (_i64, [_int, _i64, _i64, _i64]),
    "qi_resample_fft": (_int, [_int, _int, _P, _i64, _i64, _i64, _P, _P, _i64, _P]),
    "qi_cumtrapz_scratch_bytes": (_i64, [_int, _i64, _i64]),
    "qi_cumtrapz": (_int, [_int, _int, _P, _P, _i64, _dbl, _i64, _i64, _P, _P, _i64, _P]),
    "qi_derivative": (_int, [_int, _int, _int, _P, _P, _i64, _dbl, _i64, _i64, _P, _i64, _P]),
    "qi_synth": (_int, [_int, _int, _int, _int, _P, _i64, _int, _dbl, _P, _i64, _dbl, _dbl, _int, _dbl, _dbl, _dbl, _i64, _i64, _i64, _i64, _P, _P]),
    "qi_doppler": (_int, [_int, _int, _P, _i64, _int, _dbl, _P, _i64, _dbl, _dbl, _i64, _i64, _P, _P, _P, _P]),
    "qi_stft_range_samples": (_int, [_i64, _i64, _i64, _i64, _i64, _I64, _I64]),
    "qi_stft_range_scratch_bytes": (_i64, [_int, _i64, _i64, _i64, _i64, C.POINTER(StftRange), _int]),
    "qi_stft_out_range": (_int, [_int, _int, _P, _i64, _P, _i64, _i64, _i64, _dbl, C.POINTER(StftRange), C.POINTER(TfrOut), _P, _i64, _P]),
}

# include/qi_array.h (operations across the records of a batch), one to one
ARRAY_PROTOTYPES = {
    "qi_cross_spectra_scratch_bytes": (_i64, [_int, _i64, _i64, _i64]),
    "qi_cross_spectra": (_int, [_int, _int, _P, _i64, _i64, _i64, _D, _P, _P, _P, _i64, _P]),
    "qi_csd_scratch_bytes": (_i64, [_int, _i64, _i64, _i64, _i64, _i64]),
    "qi_csd": (_int, [_int, _int, _P, _i64, _i64, _P, _i64, _i64, _i64, _dbl, _P, _P, _P, _i64, _P]),
}

# include/qi_beam.h (what consumes the cross-spectral matrices), one to one
BEAM_PROTOTYPES = {
    "qi_beam_power_scratch_bytes": (_i64, [_int, _i64, _i64, _i64, _i64]),
    "qi_beam_power": (_int, [_int, _int, _P, _i64, _i64, _D, _P, _i64, _I64, _i64, _int, _P, _P, _P, _P, _i64, _P]),
}
BEAM_MAX_SENSORS = 64  # QI_BEAM_MAX_SENSORS

# include/qi_adaptive.h (the Capon beamformer: whitening factors of the matrices, and their form over the grid), one to one
ADAPTIVE_PROTOTYPES = {
    "qi_csd_whiten": (_int, [_int, _int, _P, _i64, _i64, _dbl, _P, _P, _P]),
    "qi_beam_capon_scratch_bytes": (_i64, [_int, _i64, _i64, _i64, _i64]),
    "qi_beam_capon": (_int, [_int, _int, _P, _i64, _i64, _D, _P, _i64, _I64, _i64, _P, _P, _P, _P, _i64, _P]),
}

# include/qi_subspace.h (the eigenpairs of the matrices, and the MUSIC form of their noise subspace over the grid), one to one
SUBSPACE_PROTOTYPES = {
    "qi_csd_eigh": (_int, [_int, _int, _P, _i64, _i64, _P, _P, _P, _P]),
    "qi_beam_music_scratch_bytes": (_i64, [_int, _i64, _i64, _i64, _i64]),
    "qi_beam_music": (_int, [_int, _int, _P, _i64, _i64, _i64, _D, _P, _i64, _I64, _i64, _P, _P, _P, _P, _i64, _P]),
}

# include/qi_steer.h (beam weights over delay rows, Bartlett or MVDR, and their application to a panel), one to one
STEER_PROTOTYPES = {
    "qi_beam_weights_scratch_bytes": (_i64, [_int, _i64, _i64, _i64]),
    "qi_beam_weights": (_int, [_int, _int, _P, _i64, _i64, _D, _P, _i64, _P, _P, _i64, _P]),
    "qi_beam_steer": (_int, [_int, _int, _P, _i64, _i64, _i64, _P, _i64, _P, _P]),
}

# include/qi_windows.h (cross-spectral matrices per sliding window of segments), one to one
WINDOW_PROTOTYPES = {
    "qi_cross_spectra_windows_scratch_bytes": (_i64, [_int, _i64, _i64, _i64, _i64, _i64, _i64, _i64]),
    "qi_cross_spectra_windows": (_int, [_int, _int, _P, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _D, _P, _P, _P, _i64, _P]),
    "qi_csd_windows_scratch_bytes": (_i64, [_int, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64]),
    "qi_csd_windows": (_int, [_int, _int, _P, _i64, _i64, _P, _i64, _i64, _i64, _dbl, _i64, _i64, _i64, _i64, _P, _P, _P, _i64, _P]),
}

# include/qi_lags.h (pair correlations of the matrices: lag windows and sub-sample peaks), one to one
LAG_PROTOTYPES = {
    "qi_pair_lags_scratch_bytes": (_i64, [_int, _i64, _i64, _i64, _i64]),
    "qi_pair_lags": (_int, [_int, _int, _P, _i64, _i64, _i64, _i64, _i64, _int, _int, _int, _i64, _i64, _P, _P, _P, _P, _i64, _P]),
}
LAG_WEIGHTINGS = ("plain", "phat", "scot")  # QI_LAG_PLAIN, QI_LAG_PHAT, QI_LAG_SCOT

# include/qi_bands.h (cross-spectral matrices of a constant-Q panel, every band in its own window, hop and stride), one to one
BAND_PROTOTYPES = {
    "qi_cross_spectra_bands_layout": (_i64, [_i64, _i64, _I64, _I64, _I64, _I64]),
    "qi_cross_spectra_bands_scratch_bytes": (_i64, [_int, _i64, _i64, _i64, _i64, _i64, _I64, _I64, _I64]),
    "qi_cross_spectra_bands": (_int, [_int, _int, _P, _i64, _i64, _i64, _i64, _i64, _I64, _I64, _I64, _D, _P, _P, _P, _i64, _P]),
}

# include/qi_timebeam.h (delay-and-sum in the time domain: beam traces, power and semblance per sliding window), one to one
TIMEBEAM_PROTOTYPES = {
    "qi_time_beam_power_scratch_bytes": (_i64, [_int, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64]),
    "qi_time_beam_power": (_int, [_int, _int, _P, _i64, _i64, _P, _i64, _i64, _P, _P, _i64, _i64, _i64, _i64, _int, _P, _P, _P, _P, _i64, _P]),
    "qi_time_beam_traces": (_int, [_int, _int, _P, _i64, _i64, _P, _i64, _i64, _P, _P, _i64, _i64, _P, _P]),
}
TIMEBEAM_MAX_PHASES, TIMEBEAM_TAPS = 256, (1, 2, 4, 8, 16)  # QI_TIMEBEAM_MAX_PHASES; the bank's lengths
TIMEBEAM_MAX_SHIFT, TIMEBEAM_LDS_MAX_SHIFT = 1 << 20, 1024  # QI_TIMEBEAM_MAX_SHIFT, QI_TIMEBEAM_LDS_MAX_SHIFT

# include/qi_squeeze.h (synchrosqueezing: instantaneous frequencies of a panel, reassignment to frequency bins), one to one
SQUEEZE_PROTOTYPES = {
    "qi_tfr_squeeze_scratch_bytes": (_i64, [_int, _i64, _i64, _i64, _i64]),
    "qi_tfr_ifreq": (_int, [_int, _int, _P, _i64, _i64, _i64, _D, _dbl, _dbl, _P, _P, _i64, _P]),
    "qi_tfr_squeeze": (_int, [_int, _int, _P, _P, _i64, _i64, _i64, _D, _i64, _D, _P, _P, _i64, _P]),
    "qi_tfr_synchrosqueeze": (_int, [_int, _int, _P, _i64, _i64, _i64, _D, _dbl, _dbl, _D, _i64, _D, _P, _P, _i64, _P]),
}
SQUEEZE_MAX_BINS, SQUEEZE_MAX_BANDS, SQUEEZE_TILE = 4096, 65536, 256  # QI_SQUEEZE_MAX_BINS, QI_SQUEEZE_MAX_BANDS, QI_SQUEEZE_TILE

_lib = None


def _hip_runtimes_mapped():
    try:
        with open("/proc/self/maps") as fh:
            return sorted({ln.split()[-1] for ln in fh if "libamdhip64" in ln})
    except OSError:
        return []


def load():
    """Load the shared library (once) and attach the prototypes."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise QiError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback."
        )
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in {**PROTOTYPES, **ARRAY_PROTOTYPES, **BEAM_PROTOTYPES, **ADAPTIVE_PROTOTYPES, **SUBSPACE_PROTOTYPES,
                               **STEER_PROTOTYPES, **WINDOW_PROTOTYPES, **LAG_PROTOTYPES, **BAND_PROTOTYPES, **TIMEBEAM_PROTOTYPES,
                               **SQUEEZE_PROTOTYPES}.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    rts = _hip_runtimes_mapped()
    if len(rts) > 1:
        raise QiError(f"two HIP runtimes are mapped ({rts}); libqi_tfr.so must share torch's")
    _lib = lib
    return lib


def check(rc):
    if rc != 0:
        msg = load().qi_last_error()
        raise QiError(f"libqi_tfr error {rc}: {msg.decode() if msg else '?'}")


def require_gpu():
    if not torch.cuda.is_available():
        raise QiError("no HIP device visible: the TFR transforms run only on the GPU (no CPU fallback)")
    return load()


def darr(a):
    import numpy as np

    a = np.ascontiguousarray(a, dtype=np.float64)
    return a, a.ctypes.data_as(_D)


def iarr(a):
    import numpy as np

    a = np.ascontiguousarray(a, dtype=np.int64)
    return a, a.ctypes.data_as(_I64)


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def stream_ptr(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def dtype_code(dtype):
    """QI_F64 for torch.float64, QI_F32 otherwise (the callers hold float32 or float64 by then: engine.as_signal)."""
    return QI_F64 if dtype == torch.float64 else QI_F32


def scratch(query, device, *args):
    """Scratch of one plan-less call -> (uint8 tensor on `device`, byte count for the call).  query: the library's
    qi_*_scratch_bytes to ask with `args`; a request it refuses (a negative answer) raises QiError.  The tensor holds at
    least one byte, so `ptr` of it is never null for a request the library accepts with no scratch at all."""
    nbytes = int(query(*args))
    if nbytes < 0:
        check(nbytes)
    return torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device), nbytes


def call(fn, device, *args):
    """A plan-less entry point `fn` on the current stream of `device`: every one of them takes the stream last.  torch gets
    the device as its index: an int is taken as it is, a torch.device is examined again by each of the two calls."""
    index = device.index
    with torch.cuda.device(index):
        check(fn(*args, stream_ptr(index)))
