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

There is no CPU fallback.  The reference's FFT resamplers (resample_with_sample_rate, resample_uneven_timeseries) are
not part of this, nor are decimate's other parameters (the reference fixes ftype, n and zero_phase)."""
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
    with torch.cuda.device(x.device):
        _lib.check(lib.qi_pool_panel(_lib.QI_F64 if rdtype == torch.float64 else _lib.QI_F32, x.device.index, _lib.ptr(x), kind,
                                     rows, n, int(factor), code, float(power_scale), _lib.ptr(out), _lib.stream_ptr(x.device)))
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
