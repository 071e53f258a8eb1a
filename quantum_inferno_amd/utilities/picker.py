"""Band-pass, scaling and peak picking of records (mirror of quantum_inferno/utilities/picker.py:32-209): the reference's
scipy.signal.butter(output="sos") + sosfiltfilt, with the design restated on the host (iir_design) and the filter on the
device (qi_filtfilt), and its scale_signal_by_extraction_type + scipy.signal.find_peaks calls on the device
(qi_find_peaks); the package imports no SciPy.  A record [n] gives one int64 index array, records [C, n] a list of C
arrays; NumPy in -> NumPy out, CUDA tensor in -> CUDA tensors out.  The peak finders need the counts on the host to cut
the index arrays, so each synchronises once (NumPy callers then receive the indices themselves): a pipeline that stays on
the device calls engine.find_peaks, which synchronises nothing.  The reference's *args cannot be used (a positional
argument collides with height= / distance= and raises TypeError there); the wrappers take none.  Scalar heights and
None only.  find_sample_rate_hz_from_timestamps is left out: it needs the reference's date_time module, which this
package does not have."""
import ctypes as C
import operator
from typing import Optional, Tuple, Union

import numpy as np
import torch

from .. import _lib, engine
from . import iir_design

INPUT_SCALE_TYPE = ["amplitude", "log2"]
EXTRACTION_TYPE = ["sigmax", "sigmin", "sigabs", "log2", "log2max"]


def _extraction(extraction_type):
    if extraction_type not in EXTRACTION_TYPE:
        print("Invalid extraction type.  Defaulting to sigmax.")
        return "sigmax"
    return extraction_type


def _no_args(name, args):
    if args:
        raise TypeError(f"{name}() takes no extra positional arguments ({len(args)} given): in the reference they collide "
                        "with the keywords it passes to scipy.signal.find_peaks")


def _height(height):
    """(height_kind, height) of the `height` of the *_by_extraction_type functions."""
    if height is None:
        return "none", 0.0
    if np.ndim(height) != 0:
        raise TypeError("height must be a number or None")
    return "abs", float(height)


def _check_records(timeseries):
    if np.ndim(timeseries) not in (1, 2):
        raise ValueError(f"timeseries must be [n] or [channels, n], got shape {tuple(np.shape(timeseries))}")
    if np.shape(timeseries)[-1] < 1:
        raise ValueError("a record must hold at least one sample")


def _rows(positions, counts, was_numpy, was_1d):
    """Device results of engine.find_peaks -> one index array per record (the one synchronisation: the counts)."""
    counts = counts.cpu().numpy()
    if was_numpy:
        host = positions[:, : int(counts.max(initial=0))].cpu().numpy()
        rows = [host[r, : counts[r]].copy() for r in range(len(counts))]
    else:
        rows = [positions[r, : int(counts[r])] for r in range(len(counts))]
    return rows[0] if was_1d else rows


def _is_numpy(timeseries):
    return not isinstance(timeseries, torch.Tensor)


def scale_signal_by_extraction_type(in_signal, extraction_type: str = "sigmax"):
    """Normalize the signal [n] (or every row of [C, n]) by the extraction type: x / nanmax(x) ("sigmax"), x / nanmin(x)
    ("sigmin"), x / nanmax(|x|) ("sigabs"), log2(|x| + eps) ("log2"), that / its nanmax ("log2max").  The sig* results
    have the signal's type (float32 stays float32), the log2* results are float64.  Nothing is synchronised."""
    extraction_type = _extraction(extraction_type)
    _check_records(in_signal)
    scaled = engine.find_peaks(in_signal, extraction_type, want_scaled=True, capacity=0)[3]
    return engine.finish(scaled, _is_numpy(in_signal), np.ndim(in_signal) == 1)


def _bandpass_tables(timeseries, filter_band, sample_rate_hz, filter_order):
    """The checks of apply_bandpass and its design: -> (sos, zi, edge)."""
    if filter_band[0] < 0 or filter_band[1] > sample_rate_hz / 2:
        raise ValueError(f"Invalid bandpass filter band, {filter_band}, for sample rate {sample_rate_hz}")
    if filter_band[0] >= filter_band[1]:
        raise ValueError(f"Invalid bandpass filter band, {filter_band}, the lower bound must be less than the upper bound")
    if np.ndim(timeseries) not in (1, 2):
        raise ValueError(f"timeseries must be [n] or [channels, n], got shape {tuple(np.shape(timeseries))}")
    sos = iir_design.butter_sos(filter_order, [2 * f / sample_rate_hz for f in filter_band], "bandpass")
    edge = iir_design.sosfiltfilt_edge(sos)
    iir_design.check_length(np.shape(timeseries)[-1], edge)
    return sos, iir_design.sosfilt_zi(sos), edge


def apply_bandpass(timeseries, filter_band: Tuple[float, float], sample_rate_hz: float, filter_order: int = 7):
    """Apply a zero-phase Butterworth band-pass in second-order sections to the timeseries [n] (or to every row of
    [C, n]); the record must be longer than the extension (46 values for the default order).
    -> float64, NumPy in -> NumPy out, CUDA tensor in -> CUDA tensor out."""
    sos, zi, edge = _bandpass_tables(timeseries, filter_band, sample_rate_hz, filter_order)
    return engine.zero_phase_filter(timeseries, "sos", sos, zi, edge)


def find_peaks_by_extraction_type_with_bandpass(timeseries, filter_band: Tuple[float, float], sample_rate_hz: float,
                                                filter_order: int = 7, extraction_type: str = "sigmax",
                                                height: Optional[float] = 0.7, *args):
    """Find peaks in the band-passed, normalized timeseries: apply_bandpass, then the scaling and scipy.signal.find_peaks(
    height=height) on its float64 device result; the filtered record never leaves the device."""
    _no_args("find_peaks_by_extraction_type_with_bandpass", args)
    kind, h = _height(height)
    extraction_type = _extraction(extraction_type)
    sos, zi, edge = _bandpass_tables(timeseries, filter_band, sample_rate_hz, filter_order)
    records = engine.as_signal(timeseries)[0]  # [C, n] on the device: a NumPy record goes there once
    filtered = engine.zero_phase_filter(records, "sos", sos, zi, edge)
    positions, _, counts = engine.find_peaks(filtered, extraction_type, kind, h)
    return _rows(positions, counts, _is_numpy(timeseries), np.ndim(timeseries) == 1)


def find_peaks_by_extraction_type(timeseries, extraction_type: str = "sigmax", height: Optional[float] = 0.7, *args):
    """Find peaks in the normalized timeseries: scipy.signal.find_peaks(scale_signal_by_extraction_type(timeseries,
    extraction_type), height=height)[0]."""
    _no_args("find_peaks_by_extraction_type", args)
    kind, h = _height(height)
    extraction_type = _extraction(extraction_type)
    _check_records(timeseries)
    positions, _, counts = engine.find_peaks(timeseries, extraction_type, kind, h)
    return _rows(positions, counts, _is_numpy(timeseries), np.ndim(timeseries) == 1)


def select_by_distance(positions, values, distance: int):
    """scipy.signal.find_peaks' distance rule on host arrays of candidates, positions ascending (qi_peaks_select_distance):
    -> boolean keep mask.  From the highest value down, every kept candidate removes those closer than `distance`
    samples; among equal values the later one goes first."""
    distance = operator.index(distance)
    if distance < 1:
        raise ValueError("`distance` must be greater or equal to 1")
    positions = np.ascontiguousarray(positions, dtype=np.int64)
    values = np.ascontiguousarray(values, dtype=np.float64)
    if positions.ndim != 1 or positions.shape != values.shape:
        raise ValueError("positions and values must be 1-D arrays of the same length")
    keep = np.zeros(positions.shape[0], dtype=np.uint8)
    _lib.check(_lib.load().qi_peaks_select_distance(positions.ctypes.data_as(C.c_void_p), values.ctypes.data_as(C.c_void_p),
                                                    positions.shape[0], distance, keep.ctypes.data_as(C.c_void_p)))
    return keep.astype(bool)


def find_peaks_with_bits(timeseries, sample_rate_hz: float, scaling_type: str = "amplitude", threshold_bits: Optional[int] = 1,
                         time_distance_seconds: Optional[float] = 0.1, *args):
    """Find peaks of log2(|timeseries| + eps) that reach max(log2(..)) - threshold_bits (scaling_type "log2") or
    max(timeseries) - 2 ** threshold_bits (anything else, as the reference: "amplitude") and are at least
    int(time_distance_seconds * sample_rate_hz) samples apart.  The maxima, the scaling and the picking run on the device;
    the distance rule runs on the host on the picked candidates (it is sequential, and the indices go to the host anyway)."""
    _no_args("find_peaks_with_bits", args)
    distance = int(time_distance_seconds * sample_rate_hz)
    if distance < 1:
        raise ValueError("`distance` must be greater or equal to 1")
    _check_records(timeseries)
    if scaling_type == "log2":
        kind, h = "below_max", float(threshold_bits)
    else:
        kind, h = "below_raw_max", float(2 ** threshold_bits)
    positions, values, counts = engine.find_peaks(timeseries, "log2", kind, h)
    counts = counts.cpu().numpy()
    most = int(counts.max(initial=0))
    pos, val = positions[:, :most].cpu().numpy(), values[:, :most].cpu().numpy()
    rows = []
    for r in range(len(counts)):
        p = pos[r, : counts[r]]
        rows.append(p[select_by_distance(p, val[r, : counts[r]], distance)])
    if not _is_numpy(timeseries):
        rows = [torch.from_numpy(p).to(positions.device) for p in rows]
    return rows[0] if np.ndim(timeseries) == 1 else rows


def extract_signal_index_with_buffer(sample_rate_hz: float, peak: int, intro_buffer_s: float, outro_buffer_s: float) -> Tuple[int, int]:
    """Start and end index of the signal around the peak, with a buffer in seconds before and after it."""
    if intro_buffer_s < 0 or outro_buffer_s < 0:
        raise ValueError(f"Negative intro_buffer_s or outro_buffer_s, {intro_buffer_s}, {outro_buffer_s}")
    return peak - int(intro_buffer_s * sample_rate_hz), peak + int(outro_buffer_s * sample_rate_hz)


def extract_signal_with_buffer_seconds(timeseries, sample_rate_hz: float, peak: int, intro_buffer_s: float, outro_buffer_s: float):
    """The signal around the peak with a buffer in seconds, cut at the ends of the timeseries (a view of a NumPy array or
    of a tensor)."""
    intro_index, outro_index = extract_signal_index_with_buffer(sample_rate_hz, peak, intro_buffer_s, outro_buffer_s)
    if intro_index < 0:
        print(f"Warning: intro buffer exceeds the signal length, intro_index: {intro_index}")
        intro_index = 0
    if outro_index > len(timeseries):
        print(f"Warning: outro buffer exceeds the signal length, outro_index: {outro_index}")
        outro_index = len(timeseries)
    return timeseries[intro_index:outro_index]


def find_peaks_to_comb_function(timeseries, peaks: Union[list, int, np.ndarray]):
    """A comb of the timeseries' length with 1 at the peak locations and 0 elsewhere: float64, a NumPy array for a NumPy
    timeseries, a tensor on the timeseries' device for a tensor."""
    if isinstance(peaks, (np.ndarray, torch.Tensor)):
        peaks = peaks.tolist()
    if isinstance(timeseries, torch.Tensor):
        comb_function = torch.zeros(len(timeseries), dtype=torch.float64, device=timeseries.device)
    else:
        comb_function = np.zeros(len(timeseries))
    comb_function[peaks] = 1
    return comb_function
