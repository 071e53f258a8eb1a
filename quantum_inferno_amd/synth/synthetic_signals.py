"""Synthetic signals (mirror of quantum_inferno/synth/synthetic_signals.py): chirps and sawtooth waves in white noise, behind the
reference's names, signatures, defaults and return types.  The waveform is made on the device (engine.synthesize: the linear
chirp of scipy.signal.chirp, the sawtooth of scipy.signal.sawtooth(width=0), the Tukey taper applied in the same kernel), the
noise is added and the anti-alias filter (order-4 Butterworth at half of Nyquist, scipy.signal.filtfilt) runs there
(engine.zero_phase_filter), and the record comes to the host once, at the end.  NumPy in, NumPy out.

Noise.  The functions that add noise take two keyword-only arguments the reference does not have: `noise`, an array or tensor
of standard-normal variates used instead of drawing, and `generator`, a torch.Generator.  Without either the draw is
torch.randn's on the device: it is NOT NumPy's stream, so np.random.seed has no effect on it and a record differs from the
reference's by its noise.  The standard deviation is np.std's (population)."""
from typing import Optional, Tuple, Union

import numpy as np
import torch

from .. import engine, scales_dyadic
from ..utilities import iir_design, window


def gabor_grain_frequencies(
    frequency_order_input: float,
    frequency_low_input: float,
    frequency_high_input: float,
    frequency_sample_rate_input: float,
    frequency_base_input: float = scales_dyadic.Slice.G2,
    frequency_ref_input: float = 1.0,
) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Centre, start and end frequencies of the bands between the two limits (host only)."""
    table = scales_dyadic.band_frequency_low_high(frequency_order_input, frequency_base_input, frequency_ref_input,
                                                  frequency_low_input, frequency_high_input, frequency_sample_rate_input)
    return table[5], table[6], table[7]


def _standard_normal(shape, device, noise, generator):
    """Standard-normal variates [shape] in float64 on `device`: the caller's `noise`, or a draw (torch.randn) with `generator`."""
    if noise is not None:
        z = noise if isinstance(noise, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(noise, dtype=np.float64))
        if z.numel() != int(np.prod(shape)):
            raise ValueError(f"noise must hold {int(np.prod(shape))} values, got shape {tuple(z.shape)}")
        return z.to(device=device, dtype=torch.float64).reshape(shape)
    if generator is not None and generator.device.type != "cuda":  # a host generator: drawn there, copied once
        return torch.randn(shape, dtype=torch.float64, generator=generator).to(device)
    return torch.randn(shape, dtype=torch.float64, device=device, generator=generator)


def _noise_like(sig: torch.Tensor, std_bit_loss: float, noise, generator) -> torch.Tensor:
    """white_noise_fbits for a float64 record on the device: nothing crosses to the host."""
    if noise is not None and generator is not None:
        raise ValueError("give noise or a generator, not both")
    scale = torch.std(sig, unbiased=False) / 2.0 ** std_bit_loss
    return scale * _standard_normal(tuple(sig.shape), sig.device, noise, generator)


def _check_noise(noise, generator):
    if noise is not None and generator is not None:
        raise ValueError("give noise or a generator, not both")
    if generator is not None and not isinstance(generator, torch.Generator):
        raise TypeError(f"generator must be a torch.Generator, got {type(generator).__name__}")


def _points(duration_points) -> int:
    n = int(duration_points)
    if n < 1:
        raise ValueError(f"duration_points must be at least 1, got {duration_points}")
    return n


def _finish_aa(wf: torch.Tensor, noise_std_loss_bits, noise, generator) -> np.ndarray:
    """+ white noise, the anti-alias filter, one copy to the host."""
    white = wf + _noise_like(wf, noise_std_loss_bits, noise, generator)
    return antialias_half_nyquist(white).cpu().numpy()


def _linear_chirp(n: int, sample_rate_hz: float, frequency_start_hz: float, frequency_end_hz: float) -> torch.Tensor:
    """scipy.signal.chirp(np.arange(n) / rate, f0, t[-1], f1, "linear") times tukey(n, 0.25), on the device."""
    t1 = float((n - 1) / sample_rate_hz)
    if t1 == 0.0:
        raise ZeroDivisionError("float division by zero")  # (scipy's beta = (f1 - f0) / t1 for a one-sample record)
    f0, f1 = float(frequency_start_hz), float(frequency_end_hz)
    beta = (f1 - f0) / t1
    return engine.synthesize("chirp_linear", [f0, 0.5 * beta], n, axis=("rate", sample_rate_hz), envelope=("tukey", 0.25))


def chirp_noise_16bit(
    duration_points: int = 2 ** 12,
    sample_rate_hz: float = 80.0,
    noise_std_loss_bits: float = 4.0,
    frequency_center_hz: Optional[float] = None,
    *,
    noise=None,
    generator: Optional[torch.Generator] = None,
) -> np.ndarray:
    """Linear chirp from half the centre frequency to a quarter of the sample rate under a 25 % Tukey taper, white noise
    noise_std_loss_bits below its standard deviation, anti-aliased; float16 as the reference returns it.  noise, generator:
    see the module's docstring (the draw is torch.randn's, not NumPy's)."""
    _check_noise(noise, generator)
    n = _points(duration_points)
    if not frequency_center_hz:
        frequency_center_hz = 8.0 / (duration_points / sample_rate_hz)
    wf = _linear_chirp(n, sample_rate_hz, 0.5 * frequency_center_hz, sample_rate_hz / 4.0)
    return _finish_aa(wf, noise_std_loss_bits, noise, generator).astype(np.float16)


def _sawtooth(axis, omega: float, n: int) -> torch.Tensor:
    return engine.synthesize("sawtooth", [omega], n, axis=axis, envelope=("tukey", 0.25))


def sawtooth_noise_16bit(
    duration_points: int = 2 ** 12,
    sample_rate_hz: float = 80.0,
    noise_std_loss_bits: float = 4.0,
    frequency_center_hz: Optional[float] = None,
    *,
    noise=None,
    generator: Optional[torch.Generator] = None,
) -> np.ndarray:
    """Falling sawtooth (width 0) at the centre frequency under a 25 % Tukey taper, white noise, anti-aliased; float16.
    noise, generator: see the module's docstring (the draw is torch.randn's, not NumPy's)."""
    _check_noise(noise, generator)
    n = _points(duration_points)
    frequency_center_hz = frequency_center_hz if frequency_center_hz else 8.0 / (duration_points / sample_rate_hz)
    wf = _sawtooth(("rate", sample_rate_hz), 2 * np.pi * frequency_center_hz, n)
    return _finish_aa(wf, noise_std_loss_bits, noise, generator).astype(np.float16)


def sawtooth_doppler_noise_16bit(phase_radians: np.ndarray, noise_std_loss_bits: float = 4.0, *, noise=None,
                                 generator: Optional[torch.Generator] = None) -> np.ndarray:
    """The same sawtooth from a time-varying phase in radians.  float64: the reference drops its float16 cast, and so does
    this.  noise, generator: see the module's docstring (the draw is torch.randn's, not NumPy's)."""
    _check_noise(noise, generator)
    if np.ndim(phase_radians) != 1 or np.size(phase_radians) < 1:
        raise ValueError(f"phase_radians must be a record [n], got shape {tuple(np.shape(phase_radians))}")
    wf = _sawtooth(("timestamps", phase_radians), 1.0, int(np.size(phase_radians)))
    return _finish_aa(wf, noise_std_loss_bits, noise, generator)


def chirp_linear_in_noise(
    snr_bits: float,
    sample_rate_hz: float,
    duration_s: float,
    frequency_start_hz: float,
    frequency_end_hz: float,
    intro_s: Union[int, float],
    outro_s: Union[int, float],
    *,
    noise=None,
    generator: Optional[torch.Generator] = None,
) -> Tuple[np.ndarray, np.ndarray]:
    """Tapered linear chirp between intro_s and outro_s seconds of zeros, white noise snr_bits below the standard deviation
    of the whole record -> (waveform, time in seconds).  noise, generator: see the module's docstring."""
    _check_noise(noise, generator)
    n = _points(sample_rate_hz * duration_s)
    wf = _linear_chirp(n, sample_rate_hz, frequency_start_hz, frequency_end_hz)
    zeros = [torch.zeros(int(s * sample_rate_hz), dtype=torch.float64, device=wf.device) for s in (intro_s, outro_s)]
    sig = torch.cat((zeros[0], wf, zeros[1]))
    synth_wf = (sig + _noise_like(sig, snr_bits, noise, generator)).cpu().numpy()
    return synth_wf, np.arange(len(synth_wf)) / sample_rate_hz


def white_noise_fbits(sig: np.ndarray, std_bit_loss: float, *, noise=None, generator: Optional[torch.Generator] = None) -> np.ndarray:
    """White noise of zero mean whose standard deviation is std_bit_loss bits below that of `sig` (np.std, population), one
    value per element of sig, drawn on the device.  The draw is torch.randn's, NOT NumPy's stream; noise, generator: see the
    module's docstring."""
    _check_noise(noise, generator)
    record = engine.as_signal(np.ravel(sig))[0][0].to(torch.float64)
    return _noise_like(record, std_bit_loss, noise, generator).cpu().numpy()


def taper_tukey(sig_or_time: np.ndarray, fraction_cosine: float) -> np.ndarray:
    """Symmetric Tukey window with as many points as the array has elements: 0 is rectangular, 1 a Hann window (host only)."""
    return window.get_tukey(sig_or_time, fraction_cosine)


def antialias_half_nyquist(synth, filter_order: int = 4):
    """Zero-phase Butterworth low-pass with -3 dB at a quarter of the sample rate, on the device (qi_filtfilt).  NumPy in ->
    NumPy out; a CUDA tensor stays one."""
    b, a = iir_design.butter_ba(filter_order, 0.5, "lowpass")
    edge = iir_design.filtfilt_edge(b, a)
    shape = tuple(synth.shape) if isinstance(synth, torch.Tensor) else np.shape(synth)
    n = shape[-1] if shape else 0
    iir_design.check_length(n, edge)
    return engine.zero_phase_filter(synth, "ba", np.stack([b, a]), iir_design.lfilter_zi(b, a), edge)


def frequency_algebraic_nth(frequency_geometric: np.ndarray, band_order_nth: float) -> np.ndarray:
    """Algebraic centre frequencies of constant-Q bands of the given order from the geometric ones (host only)."""
    return frequency_geometric * (np.sqrt(1 + 1 / (8 * band_order_nth ** 2)))
