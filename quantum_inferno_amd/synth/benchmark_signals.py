"""Benchmark signals (mirror of quantum_inferno/synth/benchmark_signals.py): the quantized Gabor chirp, four synthetic test
signals and the well-tempered tone, behind the reference's names, signatures, defaults, printed warnings and return types.  The
oversampled waveform is made on the device by one kernel (engine.synthesize: the formula, the gates and the Tukey taper), the
decimation by the oversampling factor runs there (engine.zero_phase_decimate, scipy.signal.decimate's filter), and the record
comes to the host once, at the end.  NumPy in, NumPy out."""
from typing import Optional, Tuple

import numpy as np
import torch

from .. import engine
from ..utilities import iir_design
from ..utilities.window import get_tukey
from . import synthetic_signals

DEFAULT_TIME_SAMPLE_INTERVAL = 1e-3
DEFAULT_TIME_DURATION = 1.0
DEFAULT_OVERSAMPLE_SCALE = 2


def signal_gate(wf: np.ndarray, t: np.ndarray, tmin: float, tmax: float, fraction_cosine: float = 0) -> np.ndarray:
    """Zero the waveform outside tmin <= t <= tmax and multiply what is inside by a Tukey window over it (0: rectangular,
    1: Hann), in place, on the host -> the waveform.  The generators below apply the same gate in their kernel."""
    inside = np.logical_and(t >= tmin, t <= tmax)
    wf[np.logical_or(t < tmin, t > tmax)] = 0.0
    wf[inside] *= get_tukey(np.empty(int(inside.sum())), fraction_cosine)
    return wf


def oversample_time(time_duration: float, time_sample_interval: float, oversample_scale: float) -> np.ndarray:
    """Timestamps of the duration at oversample_scale times the sample rate (host only)."""
    interval, points = _oversampled(time_duration, time_sample_interval, oversample_scale)
    return np.arange(points) * interval


def _oversampled(time_duration, time_sample_interval, oversample_scale):
    interval = time_sample_interval / oversample_scale
    return interval, int(time_duration / interval)


def _decimated(oversampled: torch.Tensor, q: int) -> np.ndarray:
    """scipy.signal.decimate(x, q) of float64 records on the device -> the host, one copy."""
    sos, zi, edge = iir_design.decimator(q, np.float64)
    iir_design.check_length(oversampled.shape[-1], edge)
    return engine.zero_phase_decimate(oversampled, q, sos, zi, edge).cpu().numpy()


def quantum_chirp(
    omega: float,
    order: float = 12.0,
    gamma: float = 0.0,
    gauss: bool = True,
    oversample_scale: int = DEFAULT_OVERSAMPLE_SCALE,
) -> Tuple[np.ndarray, int]:
    """Complex tone (gamma 0) or sweep of centre frequency omega < pi radians per sample, order-th octave band, under a
    Gauss envelope or none, on a power of two of points -> (waveform, that power of two)."""
    if omega >= 0.8 * np.pi:
        print("Omega >= 0.8*pi (AA*Nyquist), reset to pi * 2**(-1/N")
        omega = np.pi * 2 ** (-1 / order)
    scale = 3.0 / 4.0 * np.pi * order / omega
    chirp_scale = scale * np.sqrt(1 + gamma ** 2)
    window_support_pow2 = 2 ** int((np.ceil(np.log2(2.0 * np.pi * chirp_scale))))
    points = oversample_scale * window_support_pow2
    centre = np.arange(points)[-1] / 2  # time0[-1] / 2
    wf = engine.synthesize("quantum_chirp", [omega, 0.5 * gamma, chirp_scale, 1.0 if gauss else 0.0], points,
                           axis=("step", 1.0, centre), complex_out=True)
    parts = torch.view_as_real(wf).T.contiguous()  # real and imaginary part as two records
    parts = _decimated(parts, oversample_scale)
    return parts[0] + 1j * parts[1], window_support_pow2


def _synth(kind, row, gate, time_sample_interval, time_duration, oversample_scale):
    interval, points = _oversampled(time_duration, time_sample_interval, oversample_scale)
    if points < 1:
        raise ValueError("the duration holds no sample")
    wf = engine.synthesize(kind, row, points, axis=("step", interval), envelope=("gate", 0.0, 1.0, 0.05) if gate else None)
    synth_wf = _decimated(wf, oversample_scale)
    return synth_wf, np.arange(len(synth_wf)) * time_sample_interval


def synth_00(
    frequency_0: float = 100.0,
    frequency_1: float = 200.0,
    frequency_2: float = 400.0,
    time_start_2: float = 0.25,
    time_stop_2: float = 0.4,
    time_sample_interval: float = DEFAULT_TIME_SAMPLE_INTERVAL,
    time_duration: float = DEFAULT_TIME_DURATION,
    oversample_scale: int = DEFAULT_OVERSAMPLE_SCALE,
) -> Tuple[np.ndarray, np.ndarray]:
    """Three gated sine waves -- the first over [0, 0.5] s, the second over [0.5, 1] s, the third over its own interval --
    summed, tapered over [0, 1] s, oversampled and decimated -> (waveform, timestamps)."""
    row = [2.0 * np.pi * frequency_0, 2.0 * np.pi * frequency_1, 2.0 * np.pi * frequency_2, 0, 0.5, 0.5, 1.0, time_start_2, time_stop_2]
    return _synth("sines3", row, True, time_sample_interval, time_duration, oversample_scale)


def synth_01(
    a: float = 100.0,
    b: float = 20.0,
    f: float = 5.0,
    time_sample_interval: float = DEFAULT_TIME_SAMPLE_INTERVAL,
    time_duration: float = DEFAULT_TIME_DURATION,
    oversample_scale: int = DEFAULT_OVERSAMPLE_SCALE,
) -> Tuple[np.ndarray, np.ndarray]:
    """A falling linear sweep plus a tone with sinusoidal frequency modulation, tapered, oversampled and decimated ->
    (waveform, timestamps)."""
    row = [a * np.pi, b * np.pi, np.pi * f, 4.0 * np.pi, np.pi * 80.0]
    return _synth("synth_01", row, True, time_sample_interval, time_duration, oversample_scale)


def synth_02(
    t1: float = 0.3,
    t2: float = 0.7,
    t3: float = 0.5,
    f1: float = 45.0,
    f2: float = 75.0,
    f3: float = 15.0,
    time_sample_interval: float = DEFAULT_TIME_SAMPLE_INTERVAL,
    time_duration: float = DEFAULT_TIME_DURATION,
    oversample_scale: int = DEFAULT_OVERSAMPLE_SCALE,
) -> Tuple[np.ndarray, np.ndarray]:
    """Four Gauss pulses at three times and three frequencies, oversampled and decimated -> (waveform, timestamps)."""
    row = [-35.0 * np.pi, t1, np.pi * f1, -35.0 * np.pi, t2, np.pi * f1, -55.0 * np.pi, t3, np.pi * f2, -45.0 * np.pi, t3, np.pi * f3]
    return _synth("synth_02", row, False, time_sample_interval, time_duration, oversample_scale)


def synth_03(
    a: float = 30.0,
    b: float = 40.0,
    c: float = 150.0,
    time_sample_interval: float = DEFAULT_TIME_SAMPLE_INTERVAL,
    time_duration: float = DEFAULT_TIME_DURATION,
    oversample_scale: int = DEFAULT_OVERSAMPLE_SCALE,
) -> Tuple[np.ndarray, np.ndarray]:
    """A logarithmic sweep plus a rising linear sweep, tapered, oversampled and decimated -> (waveform, timestamps)."""
    row = [20.0 * np.pi, a, b * np.pi, c * np.pi]
    return _synth("synth_03", row, True, time_sample_interval, time_duration, oversample_scale)


def well_tempered_tone(
    frequency_sample_rate_hz: float = 800.0,
    frequency_center_hz: float = 60.0,
    time_duration_s: float = 10.24,
    time_fft_s: float = 0.64,
    use_fft_frequency: bool = True,
    add_noise_taper_aa: bool = False,
    output_desc: bool = False,
    *,
    noise=None,
    generator: Optional[torch.Generator] = None,
) -> Tuple[np.ndarray, np.ndarray, int, float, float, float]:
    """Tone of unit amplitude on a power of two of samples, by default at the FFT bin nearest the centre frequency ->
    (waveform, timestamps, FFT points, sample rate, FFT centre frequency, FFT resolution).  add_noise_taper_aa adds white
    noise 8 bits down and a 10 % Tukey taper; as in the reference the anti-aliased record is not the one returned, so the
    filter is not run.  noise, generator: see synthetic_signals (the draw is torch.randn's, not NumPy's)."""
    synthetic_signals._check_noise(noise, generator)
    frequency_resolution_hz = 1.0 / time_fft_s
    time_duration_nd = 2 ** (int(np.log2(time_duration_s * frequency_sample_rate_hz)))
    time_fft_nd = 2 ** (int(np.log2(time_fft_s * frequency_sample_rate_hz)))
    if time_duration_nd != time_duration_s * frequency_sample_rate_hz:
        print(
            f"Warning: The time duration {time_duration_s} s with given sample rate doesn't produce data points "
            f"that are power of two, adjusting time duration to {time_duration_nd} s"
        )
    if time_fft_nd != time_fft_s * frequency_sample_rate_hz:
        print(
            f"Warning: fft duration {time_fft_s} s with given sample rate doesn't produce data points "
            f"that are power of two, adjusting fft duration to {time_fft_nd} s"
        )
    frequency_fft_pos_hz = np.fft.rfftfreq(time_fft_nd, d=1 / frequency_sample_rate_hz)
    frequency_center_fft_hz = frequency_fft_pos_hz[np.argmin(np.abs(frequency_fft_pos_hz - frequency_center_hz))]
    frequency_resolution_fft_hz = frequency_sample_rate_hz / time_fft_nd
    time_s = np.arange(time_duration_nd) / frequency_sample_rate_hz
    f_c = (frequency_center_fft_hz if use_fft_frequency else frequency_center_hz) / frequency_sample_rate_hz
    mic = engine.synthesize("tone", [2.0 * np.pi * f_c], time_duration_nd, axis=("step", 1.0))
    if add_noise_taper_aa:
        mic = mic + synthetic_signals._noise_like(mic, 8.0, noise, generator)
        mic = mic * torch.from_numpy(get_tukey(time_s, alpha=0.1)).to(mic.device)
    mic_sig = mic.cpu().numpy()
    if output_desc:
        print("WELL TEMPERED TONE SYNTHETIC")
        print("Nyquist frequency:", frequency_sample_rate_hz / 2)
        print("Nominal signal frequency, hz:", frequency_center_hz)
        print("FFT signal frequency, hz:", frequency_center_fft_hz)
        print("Nominal spectral resolution, hz", frequency_resolution_hz)
        print("FFT spectral resolution, hz", frequency_resolution_fft_hz)
        print("Number of signal points:", time_duration_nd)
        print("log2(points):", np.log2(time_duration_nd))
        print("Number of FFT points:", time_fft_nd)
        print("log2(FFT points):", np.log2(time_fft_nd))
    return mic_sig, time_s, time_fft_nd, frequency_sample_rate_hz, frequency_center_fft_hz, frequency_resolution_fft_hz
