"""Subsampling of records and panels along time (mirror of quantum_inferno/utilities/sampling.py:14-50,87-120): every
n-th sample, or the average / median / max / min of each window of `subsample_factor` samples.  The work is one kernel of
the library (qi_pool_panel) on the device: NumPy in -> NumPy out, CUDA tensor in -> CUDA tensor out, float32 and float64
(complex64 / complex128 for "nth" and "average") kept.  A leading channel axis is accepted: [C, n] records, [C, B, n]
panels.

Decimation (mirror of sampling.py:123-146, scipy.signal.decimate(x, q, zero_phase=True)): decimate_timeseries for one
record [n], decimate_timeseries_collection for records [C, n] along axis 1.  The anti-alias filter -- order-8 Chebyshev
type I, 0.05 dB ripple, cut-off 0.8 / q of Nyquist, as second-order sections -- is designed on the host in NumPy
(iir_design.decimator); the zero-phase filter and the every-q-th store are two launches of the library (qi_decimate), in
the record's own precision as in SciPy: float32 records are filtered and returned in float32, float64 in float64, anything
else (integers, float16) as float64.  A record must be 28 samples or longer.

Resampling (mirror of sampling.py:53-83).  resample_uneven_timeseries is linear interpolation, not a Fourier method: records
[n] or [C, n] with shared uneven timestamps onto np.arange(t[0], t[-1], 1 / rate) by np.interp's rule, one kernel of the
library (qi_interp_grid), float64 out whatever comes in and NumPy's bits.  resample_with_sample_rate is the Fourier
resampler, scipy.signal.resample(x, int(n * new_rate / rate)): two hipFFT transforms and one kernel between them
(qi_resample_fft), float32 records kept in float32.

There is no CPU fallback.  Not part of this: decimate's other parameters (the reference fixes ftype, n and zero_phase),
scipy.signal.resample's window, domain and complex input, np.interp's left / right / period."""
import math
import operator
import warnings
from typing import Tuple

import numpy as np
import torch

from .. import _lib, engine
from . import iir_design

SUBSAMPLE_METHODS = ["average", "median", "max", "min", "nth"]
_METHOD_CODE = {"nth": _lib.QI_POOL_NTH, "average": _lib.QI_POOL_AVERAGE, "max": _lib.QI_POOL_MAX, "min": _lib.QI_POOL_MIN,
                "median": _lib.QI_POOL_MEDIAN}


def pool_rows(x, factor, method, kind=_lib.QI_POOL_REAL, power_scale=1.0, out=None):
    """qi_pool_panel on a contiguous device tensor [..., n]: pooled along the last axis on the current stream, nothing
    synchronised.  kind: QI_POOL_REAL (real in, real out), QI_POOL_COMPLEX (complex in and out), QI_POOL_POWER (complex
    in, real power_scale * |z|^2 out).  out: a contiguous tensor [..., columns] to write into."""
    lib = _lib.require_gpu()
    code = _METHOD_CODE[method] if isinstance(method, str) else int(method)
    n = x.shape[-1]
    cols = int(lib.qi_pool_columns(n, int(factor), code))
    if cols < 0:
        _lib.check(cols)
    if x.is_complex() != (kind != _lib.QI_POOL_REAL):
        raise ValueError("a complex panel pools as QI_POOL_COMPLEX or QI_POOL_POWER, a real one as QI_POOL_REAL")
    rdtype = x.real.dtype if x.is_complex() else x.dtype
    if rdtype not in (torch.float32, torch.float64):
        raise TypeError(f"unsupported dtype {x.dtype}: float32 / float64 and their complex types")
    odtype = x.dtype if kind != _lib.QI_POOL_POWER else rdtype
    x = x.contiguous()
    if out is None:
        out = torch.empty(x.shape[:-1] + (cols,), dtype=odtype, device=x.device)
    elif out.shape != x.shape[:-1] + (cols,) or out.dtype != odtype or not out.is_contiguous() or out.device != x.device:
        raise ValueError(f"out must be a contiguous {odtype} tensor of shape {tuple(x.shape[:-1]) + (cols,)}")
    rows = x.numel() // n if n else 0
    if rows == 0:
        return out
    _lib.call(lib.qi_pool_panel, x.device, _lib.dtype_code(rdtype), x.device.index, _lib.ptr(x), kind, rows, n, int(factor), code,
              float(power_scale), _lib.ptr(out))
    return out


def _pool(array, subsample_factor, method, what):
    """Shared body of subsample / subsample_2d: the reference's argument handling, then pool_rows."""
    if method not in SUBSAMPLE_METHODS:
        warnings.warn(f"method {method} not recognized, using 'nth' method", UserWarning, stacklevel=3)
        method = "nth"
    was_numpy = not isinstance(array, torch.Tensor)
    t = torch.from_numpy(np.ascontiguousarray(array)) if was_numpy else array
    if t.dtype not in (torch.float32, torch.float64, torch.complex64, torch.complex128):
        t = t.to(torch.float64)  # (the reference's NumPy reductions return float64 for integer input)
    if t.is_complex() and method not in ("nth", "average"):
        raise ValueError(f"complex {what}: only 'nth' and 'average' apply (complex values have no order), got '{method}'")
    _lib.require_gpu()
    if not t.is_cuda:
        t = t.cuda()
    out = pool_rows(t, subsample_factor, method, _lib.QI_POOL_COMPLEX if t.is_complex() else _lib.QI_POOL_REAL)
    return out.cpu().numpy() if was_numpy else out


def subsample(timeseries, sample_rate_hz: float, subsample_factor: int, method: str = "nth") -> Tuple[np.ndarray, float]:
    """Subsample a time series [n] (or records [C, n]) by the given method (default: every n-th sample); the tail that does
    not fill a window is dropped, except for "nth".  A factor below 2 returns the input (sampling.py:14-50).
    -> (subsampled series, new sample rate)"""
    if subsample_factor < 2:
        warnings.warn("subsample factor is less than 2, returning the original signal", UserWarning, stacklevel=2)
        return timeseries, sample_rate_hz
    if np.ndim(timeseries) not in (1, 2):
        raise ValueError(f"timeseries must be [n] or [channels, n], got shape {tuple(np.shape(timeseries))}")
    return _pool(timeseries, subsample_factor, method, "timeseries"), sample_rate_hz / subsample_factor


def subsample_2d(array, subsample_factor: int, method: str = "nth"):
    """Subsample a panel [B, n] (or [C, B, n]) along its last axis (sampling.py:87-120); see `subsample`."""
    if subsample_factor < 2:
        warnings.warn("subsample factor is less than 2, returning the original signal", UserWarning, stacklevel=2)
        return array
    if np.ndim(array) not in (2, 3):
        raise ValueError(f"array must be [bands, n] or [channels, bands, n], got shape {tuple(np.shape(array))}")
    return _pool(array, subsample_factor, method, "array")


def _decimate(records, decimation_factor, ndim, what):
    """Shared body of decimate_timeseries / decimate_timeseries_collection: SciPy's argument handling, the design on the
    host, then engine.zero_phase_decimate."""
    q = operator.index(decimation_factor)  # TypeError for a factor that is no integer, as scipy.signal.decimate
    if q < 1:
        raise ValueError(f"decimation_factor must be a positive integer, got {q}")
    shape = tuple(records.shape) if isinstance(records, torch.Tensor) else np.shape(records)
    if len(shape) != ndim:
        raise ValueError(f"{what} must be {ndim}-D, got shape {shape}")
    dtype = records.dtype if isinstance(records, torch.Tensor) else np.asarray(records).dtype
    real = np.float32 if dtype in (torch.float32, np.float32) else np.float64
    sos, zi, edge = iir_design.decimator(q, real)
    iir_design.check_length(shape[-1], edge)
    return engine.zero_phase_decimate(records, q, sos, zi, edge)


def decimate_timeseries(timeseries, decimation_factor: int):
    """Decimate a time series [n] by the given factor as scipy.signal.decimate(timeseries, decimation_factor,
    zero_phase=True) does (sampling.py:123-133); the time series must be 28 samples or longer.
    -> decimated signal [ceil(n / decimation_factor)]"""
    return _decimate(timeseries, decimation_factor, 1, "timeseries")


def decimate_timeseries_collection(timeseries_collection, decimation_factor: int):
    """Decimate a collection [C, n] of time series with the same sample rate at once, along axis 1 (sampling.py:136-146);
    each must be 28 samples or longer.
    -> decimated signals [C, ceil(n / decimation_factor)]"""
    return _decimate(timeseries_collection, decimation_factor, 2, "timeseries_collection")


def even_grid(first_s, last_s, sample_rate_hz):
    """np.arange(first_s, last_s, 1 / sample_rate_hz) as (start, delta, m): its values are start + i * delta, i < m, with
    m = max(ceil((last - first) / step), 0) and delta = (first + step) - first -- what NumPy's fill loop computes, which
    differs from the step itself at epoch-sized timestamps."""
    first_s, last_s = float(first_s), float(last_s)
    rate = float(sample_rate_hz)
    step = 1.0 / rate if rate != 0.0 else math.inf
    if not (math.isfinite(first_s) and math.isfinite(last_s) and math.isfinite(step) and step > 0.0):
        raise ValueError(f"no even grid from {first_s} to {last_s} at {sample_rate_hz} Hz: the ends and the rate must be finite, "
                         "the rate positive")
    m = max(math.ceil((last_s - first_s) / step), 0)
    delta = (first_s + step) - first_s
    if m > 0 and not delta > 0.0:
        raise ValueError(f"a step of {step} s is lost in the rounding of timestamps near {first_s} s")
    return first_s, delta, m


def resample_uneven_timeseries(timeseries, timestamps_s, new_sample_rate_hz=None):
    """Resample a time series [n] (or records [C, n] with the same timestamps) with uneven timestamps onto an even grid by
    linear interpolation (sampling.py:53-68): np.interp(np.arange(t[0], t[-1], 1 / rate), timestamps_s, timeseries).  With
    new_sample_rate_hz None the rate is the average one, 1 / mean(diff(timestamps_s)): NumPy's for NumPy timestamps; for
    CUDA timestamps it is evaluated on the device and only the first and last timestamp and the rate come to the host.
    float32 stays float32 on the way in, anything but float32 and float64 is read as float64; the result is float64.
    -> (resampled series [m] or [C, m], new sample rate)"""
    shape = tuple(timeseries.shape) if isinstance(timeseries, torch.Tensor) else np.shape(timeseries)
    if len(shape) not in (1, 2):
        raise ValueError(f"timeseries must be [n] or [channels, n], got shape {shape}")
    tshape = tuple(timestamps_s.shape) if isinstance(timestamps_s, torch.Tensor) else np.shape(timestamps_s)
    if len(tshape) != 1 or tshape[0] != shape[-1] or tshape[0] < 1:
        raise ValueError(f"timestamps_s must be 1-D with one timestamp per sample, got shape {tshape} for a timeseries of shape {shape}")
    if isinstance(timestamps_s, torch.Tensor):
        t = timestamps_s.to(torch.float64)
        ends = [t[0], t[-1]]
        if new_sample_rate_hz is None:
            ends.append(1 / torch.mean(torch.diff(t)))
        ends = torch.stack(ends).cpu().tolist()  # the only values that cross to the host
        first, last = ends[0], ends[1]
        if new_sample_rate_hz is None:
            new_sample_rate_hz = ends[2]
    else:
        t = np.asarray(timestamps_s, dtype=np.float64)
        first, last = t[0], t[-1]
        if new_sample_rate_hz is None:
            with np.errstate(all="ignore"), warnings.catch_warnings():
                warnings.simplefilter("ignore")
                new_sample_rate_hz = 1 / np.mean(np.diff(t))
    start, delta, m = even_grid(first, last, new_sample_rate_hz)
    return engine.interp_to_grid(timeseries, t, start, delta, m), new_sample_rate_hz


def resample_with_sample_rate(timeseries, sample_rate_hz: float, new_sample_rate_hz: float):
    """Resample a time series [n] (or records [C, n], along the last axis) to a new sample rate as scipy.signal.resample
    does (sampling.py:71-83), to int(n * new_sample_rate_hz / sample_rate_hz) samples.
    -> (resampled series, new sample rate)"""
    shape = tuple(timeseries.shape) if isinstance(timeseries, torch.Tensor) else np.shape(timeseries)
    if len(shape) not in (1, 2):
        raise ValueError(f"timeseries must be [n] or [channels, n], got shape {shape}")
    new_length = int(shape[-1] * new_sample_rate_hz / sample_rate_hz)
    if new_length < 1:
        raise ValueError(f"the new length int({shape[-1]} * {new_sample_rate_hz} / {sample_rate_hz}) = {new_length} must be at least 1")
    return engine.fft_resample(timeseries, new_length), new_sample_rate_hz
