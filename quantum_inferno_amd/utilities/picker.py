"""Band-pass of a record before picking (mirror of quantum_inferno/utilities/picker.py:56-76): the reference's
scipy.signal.butter(output="sos") + sosfiltfilt, with the design restated on the host (iir_design) and the filter on the
device (qi_filtfilt).  Only apply_bandpass: the peak finders of the reference's module are not part of this."""
from typing import Tuple

import numpy as np

from .. import engine
from . import iir_design


def apply_bandpass(timeseries, filter_band: Tuple[float, float], sample_rate_hz: float, filter_order: int = 7):
    """Apply a zero-phase Butterworth band-pass in second-order sections to the timeseries [n] (or to every row of
    [C, n]); the record must be longer than the extension (46 values for the default order).
    -> float64, NumPy in -> NumPy out, CUDA tensor in -> CUDA tensor out."""
    if filter_band[0] < 0 or filter_band[1] > sample_rate_hz / 2:
        raise ValueError(f"Invalid bandpass filter band, {filter_band}, for sample rate {sample_rate_hz}")
    if filter_band[0] >= filter_band[1]:
        raise ValueError(f"Invalid bandpass filter band, {filter_band}, the lower bound must be less than the upper bound")
    if np.ndim(timeseries) not in (1, 2):
        raise ValueError(f"timeseries must be [n] or [channels, n], got shape {tuple(np.shape(timeseries))}")
    sos = iir_design.butter_sos(filter_order, [2 * f / sample_rate_hz for f in filter_band], "bandpass")
    edge = iir_design.sosfiltfilt_edge(sos)
    iir_design.check_length(np.shape(timeseries)[-1], edge)
    return engine.zero_phase_filter(timeseries, "sos", sos, iir_design.sosfilt_zi(sos), edge)
