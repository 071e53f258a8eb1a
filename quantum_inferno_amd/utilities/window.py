"""Tapers (mirror of quantum_inferno/utilities/window.py): Tukey windows the size of a record, and windows of ones with a
Tukey taper of a given number of samples or duration at both ends.  Host only, NumPy, scipy.signal.windows.tukey's bits
(short_time_fft.tukey_window_symmetric restates it)."""
import numpy as np

from .short_time_fft import tukey_window_symmetric


def get_tukey(array: np.ndarray, alpha: float = 0.5) -> np.ndarray:
    """Symmetric Tukey (tapered cosine) window with as many points as `array` has elements; alpha is the fraction of the
    window inside the cosine tapers, shared between head and tail: 0 is a rectangular window, 1 a Hann window."""
    return tukey_window_symmetric(int(np.size(array)), alpha)


def get_tukey_by_buffer_num(array: np.ndarray, taper_num: int, alpha: float = 0.5) -> np.ndarray:
    """Window of len(array) points: the two halves of a Tukey window of 2 * taper_num points at the ends and ones
    between them.  An array shorter than 2 * taper_num gets a Tukey window over its whole length, with a printed warning."""
    if len(array) < taper_num * 2:
        print(f"Warning: array length {len(array)} is less than taper_num {taper_num * 2}. Using full array length.")
        return get_tukey(array, alpha=alpha)
    ends = tukey_window_symmetric(taper_num * 2, alpha)
    return np.concatenate((ends[:taper_num], np.ones(len(array) - taper_num * 2), ends[taper_num:]))


def get_tukey_by_buffer_s(array: np.ndarray, taper_s: float, sample_rate_hz: float, alpha: float = 0.5) -> np.ndarray:
    """get_tukey_by_buffer_num with a taper of taper_s seconds at sample_rate_hz: int(taper_s * sample_rate_hz) points."""
    return get_tukey_by_buffer_num(array, int(taper_s * sample_rate_hz), alpha=alpha)
