"""The GT blast pulse of Garces (2019), its Hilbert transform, derivative, integral and spectrum (mirror of
quantum_inferno/synth/blast_gt_pulse.py), behind the reference's names, signatures, defaults and return types.  The pulse
family is evaluated on the device (engine.synthesize, kinds "gt", "gt_hilbert", "gt_derivative", "gt_integral": the pulse, its
derivative and its integral are NumPy's results bit for bit), noise and the anti-alias filter run there too, and the record
comes to the host once.  The spectrum is host NumPy.  NumPy in, NumPy out."""
from typing import Optional, Tuple, Union

import numpy as np
import torch

from .. import engine
from .synthetic_signals import white_noise_fbits, antialias_half_nyquist, _check_noise, _finish_aa  # noqa: F401


def _times(time_center_s) -> np.ndarray:
    t = np.asarray(time_center_s, dtype=np.float64)
    if t.ndim != 1 or t.size < 1:
        raise ValueError(f"time_center_s must be a record [n] of at least one sample, got shape {t.shape}")
    return t


def _pulse(kind, time_center_s, pseudo_period_s, constant=0.0) -> np.ndarray:
    t = _times(time_center_s)
    return engine.synthesize(kind, [pseudo_period_s / 4.0, constant], t.size, axis=("timestamps", t)).cpu().numpy()


def gt_blast_period_center(time_center_s: np.ndarray, pseudo_period_s: float) -> np.ndarray:
    """The GT blast pulse at the given centred times for a pseudo period in seconds."""
    return _pulse("gt", time_center_s, pseudo_period_s)


def gt_hilbert_blast_period_center(time_center_s: np.ndarray, pseudo_period_s: float) -> np.ndarray:
    """The Hilbert transform of the GT blast pulse."""
    return _pulse("gt_hilbert", time_center_s, pseudo_period_s)


def _gt_noise(axis, n, pseudo_period_s, noise_std_loss_bits, noise, generator) -> np.ndarray:
    sig_gt = engine.synthesize("gt", [pseudo_period_s / 4.0], n, axis=axis)
    return _finish_aa(sig_gt, noise_std_loss_bits, noise, generator)


def gt_blast_center_fast(
    frequency_peak_hz: float = 6.3, sample_rate_hz: float = 100.0, noise_std_loss_bits: float = 16., *, noise=None,
    generator: Optional[torch.Generator] = None
) -> Tuple[np.ndarray, np.ndarray]:
    """GT pulse of 16 periods of the peak frequency in white noise, anti-aliased -> (centred time in seconds, pulse).  noise,
    generator: see synthetic_signals (the draw is torch.randn's, not NumPy's)."""
    return _centered(int(16 / frequency_peak_hz * sample_rate_hz), frequency_peak_hz, sample_rate_hz, noise_std_loss_bits, noise, generator)


def gt_blast_center_noise(
    duration_s: float = 16., frequency_peak_hz: float = 6.3,
    sample_rate_hz: float = 100., noise_std_loss_bits: float = 16., *, noise=None, generator: Optional[torch.Generator] = None
) -> Tuple[np.ndarray, np.ndarray]:
    """GT pulse of the given duration in white noise, anti-aliased -> (centred time in seconds, pulse).  noise, generator: see
    synthetic_signals (the draw is torch.randn's, not NumPy's)."""
    return _centered(int(duration_s * sample_rate_hz), frequency_peak_hz, sample_rate_hz, noise_std_loss_bits, noise, generator)


def _centered(points, frequency_peak_hz, sample_rate_hz, noise_std_loss_bits, noise, generator):
    _check_noise(noise, generator)
    time_center_s = np.arange(points) / sample_rate_hz
    half = time_center_s[-1] / 2.0  # (IndexError for no points, as the reference)
    time_center_s -= half
    return time_center_s, _gt_noise(("rate", sample_rate_hz, half), points, 1 / frequency_peak_hz, noise_std_loss_bits, noise, generator)


def gt_blast_center_noise_uneven(
    sensor_epoch_s: np.array, noise_std_loss_bits: float = 2., frequency_center_hz: Optional[float] = None, *, noise=None,
    generator: Optional[torch.Generator] = None
) -> np.ndarray:
    """GT pulse at even or uneven sensor timestamps (epoch seconds), centred on their middle, in white noise, anti-aliased.
    noise, generator: see synthetic_signals (the draw is torch.randn's, not NumPy's)."""
    _check_noise(noise, generator)
    epoch = _times(sensor_epoch_s)
    time_duration_s = epoch[-1] - epoch[0]
    pseudo_period_s = 1 / frequency_center_hz if frequency_center_hz else time_duration_s / 4.0
    return _gt_noise(("timestamps", epoch, epoch[0], time_duration_s / 2.0), epoch.size, pseudo_period_s, noise_std_loss_bits, noise, generator)


def gt_blast_derivative_period_center(time_center_s: np.ndarray, pseudo_period_s: float) -> np.ndarray:
    """Derivative of the GT pulse with respect to tau (the jump at the onset is not in it)."""
    return _pulse("gt_derivative", time_center_s, pseudo_period_s)


def _integral_branches(tau):
    """The two branches of the integral for a few values of tau, on the host."""
    r6 = np.sqrt(6)
    first = (1.0 - tau / 2.0) * tau
    second = -tau / 72.0 * (3 * tau ** 3 - 4 * (3 + 2 * r6) * tau ** 2 + 6 * (9 + 4 * r6) * tau - 12 * (7 + 2 * r6))
    return first, second


def gt_blast_integral_period_center(time_center_s: np.ndarray, pseudo_period_s: float) -> np.ndarray:
    """Integral of the GT pulse over tau, continuous at the zero crossing: the constant that joins the last sample of the
    positive phase to the first of the negative phase is found on the host from those two samples.  IndexError, as the
    reference, when either phase holds no sample."""
    t = _times(time_center_s)
    tau = t / (pseudo_period_s / 4.0) + 1.0
    positive = np.where((0.0 <= tau) & (tau <= 1.0))[0]
    negative = np.where((1.0 < tau) & (tau <= 1 + np.sqrt(6.0)))[0]
    last, first = positive[-1:], negative[:1]
    if last.size == 0 or first.size == 0:
        raise IndexError(f"index {-1 if last.size == 0 else 0} is out of bounds for axis 0 with size 0")
    integration_constant = _integral_branches(tau[last])[0][0] - _integral_branches(tau[first])[1][0]
    return _pulse("gt_integral", t, pseudo_period_s, integration_constant)


def gt_blast_center_integral_and_derivative(
    frequency_peak_hz: float, sample_rate_hz: float
) -> Tuple[float, np.ndarray, np.ndarray, np.ndarray]:
    """Two periods of the GT pulse, its integral and its derivative over tau -> (tau, pulse, integral, derivative); the
    derivative's sample before the peak carries the estimate of the onset's jump."""
    pseudo_period_s = 1 / frequency_peak_hz
    time_center_s = np.arange(int(2 / frequency_peak_hz * sample_rate_hz)) / sample_rate_hz
    time_center_s -= time_center_s[-1] / 2.0
    tau_center = time_center_s / (pseudo_period_s / 4.0)
    sig_gt = gt_blast_period_center(time_center_s, pseudo_period_s)
    sig_gt_i = gt_blast_integral_period_center(time_center_s, pseudo_period_s)
    sig_gt_d = gt_blast_derivative_period_center(time_center_s, pseudo_period_s)
    sig_gt_d[np.argmax(sig_gt) - 1] = np.max(np.diff(sig_gt)) / np.mean(np.diff(tau_center))
    return tau_center, sig_gt, sig_gt_i, sig_gt_d


def gt_blast_ft(frequency_peak_hz: float, frequency_hz: Union[float, np.ndarray]) -> Union[float, complex, np.ndarray]:
    """Fourier transform of the GT pulse at the given frequencies (host only)."""
    w = 0.5 * np.pi * frequency_hz / frequency_peak_hz
    r6 = np.sqrt(6.0)
    positive = (1.0 - 1j * w - np.exp(-1j * w)) / w ** 2.0
    inner = 1j * w * r6 + 3.0 + np.exp(1j * w * r6) * (3.0 * w ** 2.0 + 1j * w * 2.0 * r6 - 3.0)
    negative = np.exp(-1j * w * (1 + r6)) / (3.0 * w ** 4.0) * inner
    return (positive + negative) * np.pi / (2 * np.pi * frequency_peak_hz)


def gt_blast_spectral_density(
    frequency_peak_hz: float, frequency_hz: Union[float, np.ndarray]
) -> Tuple[Union[float, np.ndarray], float]:
    """Spectral density of the GT pulse -> (density at the given frequencies, its maximum) (host only)."""
    ft = gt_blast_ft(frequency_peak_hz, frequency_hz)
    density = 2 * np.abs(ft * np.conj(ft))
    return density, np.max(density)
