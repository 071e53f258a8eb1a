"""Point-count rounding used to size the STFT segment (mirror of the two functions of
quantum_inferno/utilities/calculations.py that sit on the TFR path, :160-205), and the module's array functions
(:16-157): integration and differentiation of records on the device.

integrate_with_cumtrapz_* is scipy.integrate.cumulative_trapezoid(initial=0): one library call of three launches
(qi_cumtrapz).  The trapezoid terms are SciPy's bit for bit; the running sum is not NumPy's left-to-right one but a
parallel scan whose order of additions depends on the record length alone (include/qi_tfr.h writes the tree down), so a
record gives the same bits alone, in any batch and on every run, within rounding of SciPy's.  derivative_with_gradient_* is
np.gradient (edge_order 1) and derivative_with_difference_* np.diff times the rate or over np.diff of the timestamps, one
launch each (qi_derivative), NumPy's bits.  The fill of the difference functions is taken from the derivative on the
device: exact for every type but "mean", which is a PyTorch reduction (within rounding of np.mean).

Records are 1-D [n], as in the reference, or [C, n] along the last axis; timestamps [n] (or [C, n], a row per record).
NumPy in -> NumPy out, CUDA tensor in -> CUDA tensor out.  Result types are the reference's: float64 whenever timestamps
are given (np.gradient excepted: it keeps the record's type); with a sample rate float32 records stay float32 -- unless
the rate is a NumPy float64 scalar, which NumPy does not treat as a weak scalar: the record is widened to float64 first
(the gradient is then rounded back to float32, as NumPy stores it).  The same widening serves float32 records whose
timestamps are evenly spaced to the bit, where np.gradient divides by the float64 spacing.  In these two corners the
values are those of the float64 computation, not always NumPy's last bit.  There is no CPU fallback: only records
shorter than two samples, which have no derivative, are answered on the host as the reference answers them."""
import numpy as np
import torch

from .. import engine

FILL_LOCATIONS = ["start", "end"]
FILL_TYPES = ["zero", "nan", "mean", "median", "min", "max", "tail", "head"]
ROUNDING_TYPES = ["floor", "ceil", "round", "ceil_power_of_two", "floor_power_of_two"]
OUTPUT_TYPES = ["points", "log2", "pow2"]


def round_value(value: float, rounding_type: str = "round") -> int:
    """Round to an int by the named rule; "round" is half-to-even (ref calculations.py:160-184)."""
    if rounding_type not in ROUNDING_TYPES:
        raise ValueError(f"Invalid rounding type {rounding_type}, must be one of {ROUNDING_TYPES}")
    if rounding_type == "floor":
        return int(np.floor(value))
    if rounding_type == "ceil":
        return int(np.ceil(value))
    if rounding_type == "round":
        return int(np.round(value))
    exponent = np.ceil(np.log2(value)) if rounding_type == "ceil_power_of_two" else np.floor(np.log2(value))
    return 2 ** int(exponent)


def get_num_points(sample_rate_hz: float, duration_s: float, rounding_type: str, output_unit: str) -> int:
    """Points (or their log2 / pow2) in duration_s at sample_rate_hz (ref calculations.py:187-205)."""
    if output_unit not in OUTPUT_TYPES:
        raise ValueError(f"Invalid output unit {output_unit}, must be one of {OUTPUT_TYPES}")
    points = sample_rate_hz * duration_s
    if output_unit == "log2":
        points = np.log2(points)
    elif output_unit == "pow2":
        points = 2 ** points
    return round_value(points, rounding_type)


# ---- integration ----------------------------------------------------------------------------------------------------------
def _is_weak(scalar):
    """A Python number, which NumPy lets take the array's precision; a NumPy scalar keeps its own."""
    return type(scalar) in (int, float)


def _widen_for(scalar, timeseries):
    """The record as float64 when it is float32 and `scalar` is a NumPy scalar that promotes it (np.float64)."""
    dtype = timeseries.dtype if isinstance(timeseries, torch.Tensor) else np.asarray(timeseries).dtype
    if dtype not in (torch.float32, np.float32) or _is_weak(scalar) or np.result_type(np.float32, scalar) != np.float64:
        return timeseries, False
    wide = timeseries.to(torch.float64) if isinstance(timeseries, torch.Tensor) else np.asarray(timeseries, dtype=np.float64)
    return wide, True


def _length(timeseries):
    shape = tuple(timeseries.shape) if isinstance(timeseries, torch.Tensor) else np.shape(timeseries)
    if len(shape) not in (1, 2):
        raise ValueError(f"timeseries must be [n] or [channels, n], got shape {shape}")
    return shape[-1]


def _cumtrapz(timeseries, timestamps_s, dx, initial_value):
    if _length(timeseries) == 0:
        raise ValueError("At least one point is required along `axis`.")
    if initial_value is not None:  # SciPy 1.15 takes no other start than 0
        if initial_value != 0:
            raise ValueError("`initial` must be `None` or `0`.")
        if not np.isscalar(initial_value):
            raise ValueError("`initial` parameter should be a scalar.")
    result = engine.cumulative_trapezoid(timeseries, timestamps_s, dx)
    return result if initial_value is not None else result[..., 1:]


def integrate_with_cumtrapz_timestamps_s(timestamps_s, timeseries, initial_value: float = 0):
    """Cumulative trapezoid integration of a time series [n] (or records [C, n]) over its timestamps in seconds, as
    scipy.integrate.cumulative_trapezoid(y=timeseries, x=timestamps_s, initial=initial_value) (calculations.py:16-27).
    -> integrated waveform, float64, the first value 0"""
    return _cumtrapz(timeseries, timestamps_s, 1.0, initial_value)


def integrate_with_cumtrapz_sample_rate_hz(sample_rate_hz: float, timeseries, initial_value: float = 0):
    """Cumulative trapezoid integration of a time series [n] (or records [C, n]) sampled at sample_rate_hz, as
    scipy.integrate.cumulative_trapezoid(y=timeseries, dx=1 / sample_rate_hz, initial=initial_value) (calculations.py:30-41).
    -> integrated waveform in the record's type, the first value 0"""
    dx = 1 / sample_rate_hz
    timeseries, _ = _widen_for(dx, timeseries)
    return _cumtrapz(timeseries, None, dx, initial_value)


# ---- derivatives ----------------------------------------------------------------------------------------------------------
def _even_spacing(timestamps_s):
    """The spacing when timestamps [n] are evenly spaced to the bit (np.gradient then uses its formula for even samples),
    else None.  Device timestamps: two numbers cross to the host."""
    if isinstance(timestamps_s, torch.Tensor):
        if timestamps_s.dim() != 1 or timestamps_s.shape[0] < 2:
            return None
        d = torch.diff(timestamps_s.to(torch.float64))
        even, spacing = torch.stack([(d == d[0]).all().to(torch.float64), d[0]]).cpu().tolist()
        return spacing if even else None
    t = np.asarray(timestamps_s, dtype=np.float64)
    if t.ndim != 1 or len(t) < 2:
        return None
    d = np.diff(t)
    return float(d[0]) if (d == d[0]).all() else None


def _gradient_wide(timeseries, h):
    """np.gradient of a float32 record with a float64 spacing: computed in float64, stored as float32."""
    wide = timeseries.to(torch.float64) if isinstance(timeseries, torch.Tensor) else np.asarray(timeseries, dtype=np.float64)
    result = engine.derivative(wide, None, h, "gradient")
    return result.to(torch.float32) if isinstance(result, torch.Tensor) else result.astype(np.float32)


def derivative_with_gradient_timestamps_s(timestamps_s, timeseries):
    """Derivative of a time series [n] (or records [C, n]) over its timestamps in seconds as np.gradient(timeseries,
    timestamps_s) (calculations.py:44-52), in the record's type.  Timestamps [C, n], a row per record, always take the
    formula for uneven samples."""
    _length(timeseries)
    spacing = _even_spacing(timestamps_s)
    if spacing is None:
        return engine.derivative(timeseries, timestamps_s, 1.0, "gradient")
    tshape = tuple(timestamps_s.shape)
    if tshape[0] != _length(timeseries):
        raise ValueError("when 1d, distances must match the length of the corresponding dimension")
    dtype = timeseries.dtype if isinstance(timeseries, torch.Tensor) else np.asarray(timeseries).dtype
    if dtype in (torch.float32, np.float32):
        return _gradient_wide(timeseries, spacing)
    return engine.derivative(timeseries, None, spacing, "gradient")


def derivative_with_gradient_sample_rate_hz(sample_rate_hz: float, timeseries):
    """Derivative of a time series [n] (or records [C, n]) sampled at sample_rate_hz as np.gradient(timeseries,
    1 / sample_rate_hz) (calculations.py:55-63), in the record's type."""
    _length(timeseries)
    h = 1 / sample_rate_hz
    if _widen_for(h, timeseries)[1]:
        return _gradient_wide(timeseries, float(h))
    return engine.derivative(timeseries, None, h, "gradient")


def get_fill_from_filling_method(array_1d: np.ndarray, fill_type: str) -> float:
    """The value that pads `array_1d` for the fill type, one of FILL_TYPES (calculations.py:66-96); on the host."""
    if len(np.shape(array_1d)) != 1:
        raise ValueError(f"array_1d has shape {np.shape(array_1d)} but should be a 1D array")
    if fill_type not in FILL_TYPES:
        raise ValueError(f"Invalid fill type {fill_type}, must be one of {FILL_TYPES}")
    if fill_type == "zero":
        return 0
    if fill_type == "nan":
        return np.nan
    if fill_type == "tail":
        return array_1d[-1]
    if fill_type == "head":
        return array_1d[0]
    return {"mean": np.mean, "median": np.median, "min": np.min, "max": np.max}[fill_type](array_1d)


def append_fill(array_1d: np.ndarray, fill_value: float, fill_loc: str) -> np.ndarray:
    """`array_1d` with the fill value put in front ("start") or behind ("end") (calculations.py:99-115); on the host."""
    if fill_loc not in FILL_LOCATIONS:
        raise ValueError(f"Invalid fill location {fill_loc}, must be one of {FILL_LOCATIONS}")
    return np.insert(array_1d, 0, fill_value) if fill_loc == "start" else np.append(array_1d, fill_value)


def _median_rows(d):
    """np.median along the rows of d [C, m], m >= 1: the middle value or the mean of the two middle ones, NaN where a row
    holds one."""
    ordered, _ = torch.sort(d, dim=1)  # (NaN sorts last)
    m = d.shape[1]
    low, high = ordered[:, (m - 1) // 2], ordered[:, m // 2]
    middle = (low + high) / 2 if m % 2 == 0 else low
    return torch.where(torch.isnan(ordered[:, -1]), torch.full_like(middle, float("nan")), middle)


def _difference(timeseries, timestamps_s, factor, fill_type, fill_loc):
    """Shared body of the two difference functions: the differences by qi_derivative into a row of n columns, the fill
    from them on the device."""
    n = _length(timeseries)
    if fill_type not in FILL_TYPES:
        raise ValueError(f"Invalid fill type {fill_type}, must be one of {FILL_TYPES}")
    if fill_loc not in FILL_LOCATIONS:
        raise ValueError(f"Invalid fill location {fill_loc}, must be one of {FILL_LOCATIONS}")
    if n < 2:  # no difference to take: the reference's expressions on the host, with whatever NumPy says to an empty array
        was_tensor = isinstance(timeseries, torch.Tensor)
        y = timeseries.cpu().numpy() if was_tensor else np.asarray(timeseries)
        if y.ndim != 1:
            raise ValueError(f"records of {n} samples have no difference")
        if timestamps_s is None:
            d = np.diff(y) * factor
        else:
            d = np.diff(y) / np.diff(timestamps_s.cpu().numpy() if isinstance(timestamps_s, torch.Tensor) else timestamps_s)
        result = append_fill(d, get_fill_from_filling_method(d, fill_type), fill_loc)
        return torch.from_numpy(result).to(timeseries.device) if was_tensor else result
    x, was_numpy, was_1d = engine.as_signal(timeseries)
    out = engine.derivative(x, timestamps_s, factor, "difference", fill_loc)
    slot, first = (0, 1) if fill_loc == "start" else (n - 1, 0)
    d = out[:, first:first + n - 1]
    if fill_type == "nan":
        out[:, slot] = float("nan")
    elif fill_type != "zero":  # (engine.derivative left 0 there)
        fill = {"mean": lambda: d.mean(dim=1), "median": lambda: _median_rows(d), "min": lambda: torch.amin(d, dim=1),
                "max": lambda: torch.amax(d, dim=1), "tail": lambda: d[:, -1], "head": lambda: d[:, 0]}[fill_type]()
        out[:, slot] = fill
    if fill_loc == "end" and fill_type in ("zero", "nan"):
        out = out.to(torch.float64)  # np.append of a Python number gives float64
    return engine.finish(out, was_numpy, was_1d)


def derivative_with_difference_timestamps_s(timestamps_s, timeseries, fill_type: str = "zero", fill_loc: str = "end"):
    """Derivative of a time series [n] (or records [C, n]) as np.diff(timeseries) / np.diff(timestamps_s), padded to the
    length of the input with the fill type (FILL_TYPES, default "zero") at the fill location (FILL_LOCATIONS, default
    "end") (calculations.py:118-136).  -> derivative waveform, float64"""
    return _difference(timeseries, timestamps_s, 1.0, fill_type, fill_loc)


def derivative_with_difference_sample_rate_hz(sample_rate_hz: float, timeseries, fill_type: str = "zero", fill_loc: str = "end"):
    """Derivative of a time series [n] (or records [C, n]) as np.diff(timeseries) * sample_rate_hz, padded to the length of
    the input with the fill type (FILL_TYPES, default "zero") at the fill location (FILL_LOCATIONS, default "end")
    (calculations.py:139-157).  -> derivative waveform in the record's type (float64 for "zero" and "nan" at "end", as
    np.append gives it)"""
    timeseries, _ = _widen_for(sample_rate_hz, timeseries)
    return _difference(timeseries, None, sample_rate_hz, fill_type, fill_loc)
