"""
Short-time Fourier transform on the GPU behind the reference's signatures
(quantum_inferno/styx_fft.py).  The reference calls scipy.signal.stft(boundary="zeros", padded=True,
detrend="constant", return_onesided=True); here the zero-extended segments are mean-removed and
windowed by a HIP kernel, transformed as one batched real FFT and written frequency x time.
"""
from dataclasses import dataclass

import ctypes as C
import numpy as np
import torch

from . import _lib, engine
from .scales_dyadic import cycles_from_order, get_epsilon
from .utilities.calculations import get_num_points


def tukey_window_periodic(points: int, alpha: float) -> np.ndarray:
    """scipy.signal.get_window(("tukey", alpha), points): the periodic (fftbins) Tukey taper, i.e. the
    symmetric window of points + 1 samples without its last one.  alpha >= 1 is the periodic Hann."""
    if alpha <= 0:
        return np.ones(points)
    sym = points + 1
    k = np.arange(0, sym)
    if alpha >= 1.0:
        phase = np.linspace(-np.pi, np.pi, sym)
        return (0.5 + 0.5 * np.cos(phase))[:-1]
    ramp = int(np.floor(alpha * (sym - 1) / 2.0))
    rise = 0.5 * (1 + np.cos(np.pi * (-1 + 2.0 * k[: ramp + 1] / alpha / (sym - 1))))
    flat = np.ones(sym - 2 * ramp - 2)
    fall = 0.5 * (1 + np.cos(np.pi * (-2.0 / alpha + 1 + 2.0 * k[sym - ramp - 1 :] / alpha / (sym - 1))))
    return np.concatenate((rise, flat, fall))[:-1]


def gaussian_window_periodic(points: int, sigma: float) -> np.ndarray:
    """scipy.signal.get_window(("gaussian", sigma), points) (periodic)."""
    k = np.arange(0, points + 1) - points / 2.0
    return np.exp(-(k ** 2) / (2 * sigma * sigma))[:-1]


def stft_segment_points(frequency_sample_rate_hz, band_order_nth, center_frequency_hz=None, octaves_below_center=4):
    """Power-of-two segment length that holds M cycles of the averaging frequency (ref styx_fft.py:31-41)."""
    if center_frequency_hz is None:
        center_frequency_hz = frequency_sample_rate_hz * 0.075
    duration_s = cycles_from_order(band_order_nth) / (center_frequency_hz / octaves_below_center)
    return 2 ** get_num_points(frequency_sample_rate_hz, duration_s, "ceil", "log2")


def _butter_filtfilt(sig_wf, filter_order, wn, btype, tukey_alpha):
    """Shared body of butter_bandpass / butter_highpass / butter_lowpass: signal.butter(output="ba"), the symmetric Tukey
    taper and signal.filtfilt of the reference, on every row of sig_wf (engine.zero_phase_filter)."""
    from .utilities import iir_design
    from .utilities.short_time_fft import tukey_window_symmetric

    if np.ndim(sig_wf) not in (1, 2):
        raise ValueError(f"signal must be 1-D [n] or 2-D [channels, n], got shape {tuple(np.shape(sig_wf))}")
    b, a = iir_design.butter_ba(filter_order, wn, btype)
    edge = iir_design.filtfilt_edge(b, a)
    n = np.shape(sig_wf)[-1]
    iir_design.check_length(n, edge)
    return engine.zero_phase_filter(sig_wf, "ba", np.stack([b, a]), iir_design.lfilter_zi(b, a), edge,
                                    taper=tukey_window_symmetric(n, tukey_alpha))


def butter_bandpass(sig_wf, frequency_sample_rate_hz: float, frequency_cut_low_hz, frequency_cut_high_hz, filter_order: int = 4,
                    tukey_alpha: float = 0.5):
    """Zero-phase Butterworth band-pass of a Tukey-tapered record (ref styx_fft.py:60-90); a [C, n] input filters every
    row.  A high cut-off at or above Nyquist is replaced by half of Nyquist, with the reference's warning.
    -> float64, NumPy in -> NumPy out, CUDA tensor in -> CUDA tensor out."""
    nyquist = 0.5 * frequency_sample_rate_hz
    edge_low = frequency_cut_low_hz / nyquist
    edge_high = frequency_cut_high_hz / nyquist
    if edge_high >= 1:
        print(f"Warning: Frequency cutoff {frequency_cut_high_hz} greater than Nyquist {nyquist} Hz, using half Nyquist")
        edge_high = 0.5  # Half of nyquist
    return _butter_filtfilt(sig_wf, filter_order, [edge_low, edge_high], "bandpass", tukey_alpha)


def butter_highpass(sig_wf, frequency_sample_rate_hz: float, frequency_cut_low_hz, filter_order: int = 4, tukey_alpha: float = 0.5):
    """Zero-phase Butterworth high-pass of a Tukey-tapered record (ref styx_fft.py:93-120); see butter_bandpass."""
    edge_low = frequency_cut_low_hz / (0.5 * frequency_sample_rate_hz)
    if edge_low >= 1:
        raise ValueError(f"Frequency cutoff {frequency_cut_low_hz} is greater than Nyquist {0.5*frequency_sample_rate_hz}")
    return _butter_filtfilt(sig_wf, filter_order, [edge_low], "highpass", tukey_alpha)


def butter_lowpass(sig_wf, frequency_sample_rate_hz: float, frequency_cut_high_hz, filter_order: int = 4, tukey_alpha: float = 0.5):
    """Zero-phase Butterworth low-pass of a Tukey-tapered record (ref styx_fft.py:123-149); see butter_bandpass."""
    edge_high = frequency_cut_high_hz / (0.5 * frequency_sample_rate_hz)
    if edge_high >= 1:
        raise ValueError(f"Frequency cutoff {frequency_cut_high_hz} is greater than Nyquist {0.5*frequency_sample_rate_hz}")
    return _butter_filtfilt(sig_wf, filter_order, [edge_high], "lowpass", tukey_alpha)


def _frame_count(n, seg, hop):
    """Segments of scipy.signal.stft(boundary="zeros", padded=True), as qi_stft_segments counts them: host arithmetic."""
    if n <= 0 or seg <= 0 or not 0 < hop <= seg:
        return 0
    length = n + 2 * (seg // 2)
    length += (-(length - seg) % hop) % seg
    return (length - seg) // hop + 1


def _run_window(window64, rdtype):
    """The window as a run in `rdtype` holds it: SciPy rounds it to the output precision before using and summing it
    (_spectral_helper)."""
    win = np.asarray(window64, dtype=np.float64)
    return np.ascontiguousarray(win if rdtype == torch.float64 else win.astype(np.float32))


def _order_segment(n, fs, band_order_nth, center_frequency_hz=None, octaves_below_center=4):
    """stft_from_sig's segment for a record of n samples, or its refusal."""
    seg = stft_segment_points(fs, band_order_nth, center_frequency_hz, octaves_below_center)
    if n < seg:
        raise ValueError(f"Signal length: {n} is less than time_fft_nd: {seg}")
    return seg


@dataclass(frozen=True, eq=False)
class StftGeometry:
    """What scipy.signal.stft(boundary="zeros", padded=True, scaling="spectrum") makes of a record length and a window, once
    for every caller: host arithmetic, no device and no library.  `window` is the host array in the run's precision, `scale`
    1 / sum(window) of that array times the caller's factor, `n_seg` the segments, `n_f` = nfft // 2 + 1."""

    seg: int
    hop: int
    nfft: int
    n_seg: int
    n_f: int
    scale: float
    window: np.ndarray
    time_s: np.ndarray
    frequency_hz: np.ndarray

    @classmethod
    def from_window(cls, n, fs, window64, overlap_points, nfft_points, extra_scale=1.0, rdtype=torch.float32):
        """A float64 `window` [seg] with overlap and transform length as stft_complex_pow2 hands them to SciPy."""
        n, fs, seg, nfft = int(n), float(fs), len(window64), int(nfft_points)
        hop = seg - int(overlap_points)
        if not 0 < hop <= seg:
            raise ValueError("noverlap must be less than nperseg.")
        if nfft < seg:
            raise ValueError("nfft must be greater than or equal to nperseg.")
        win = _run_window(window64, engine._real_dtype(rdtype))
        scale = float(np.sqrt(1.0 / np.sum(win.astype(np.float64)) ** 2)) * extra_scale
        padded = n + 2 * (seg // 2)
        padded += (-(padded - seg) % hop) % seg
        time_s = np.arange(seg / 2, padded - seg / 2 + 1, hop) / fs - (seg / 2) / fs
        return cls(seg, hop, nfft, _frame_count(n, seg, hop), nfft // 2 + 1, float(scale), win, time_s, np.fft.rfftfreq(nfft, 1 / fs))

    @classmethod
    def from_order(cls, n, fs, band_order_nth, center_frequency_hz=None, octaves_below_center=4, rdtype=torch.float32):
        """stft_from_sig's: periodic Hann of the order's segment, half overlap, scale 2 sqrt(pi) / segment."""
        seg = _order_segment(int(n), fs, band_order_nth, center_frequency_hz, octaves_below_center)
        return cls.from_window(n, fs, tukey_window_periodic(seg, 1.0), seg // 2, seg, 2 * np.sqrt(np.pi) / seg, rdtype)


def _stft_out(lib, sig, window, g, res, scratch=None):
    """qi_stft_out of geometry `g` on a [C, n] device tensor into the buffers of `res` (a TfrResult: any of coef, bits, the
    reductions); `scratch`: a kept buffer of qi_stft_out_scratch_bytes for this request, or None."""
    n_ch, n = sig.shape
    dev = sig.device
    code = _lib.dtype_code(sig.dtype)
    if scratch is None:
        scratch, _ = _lib.scratch(lib.qi_stft_out_scratch_bytes, dev, code, n_ch, n, g.seg, g.hop, g.nfft, res.coef is not None,
                                  res.bits is not None)
    desc = engine.out_descriptor(res, get_epsilon())
    _lib.call(lib.qi_stft_out, dev, code, dev.index, _lib.ptr(sig), n_ch, n, _lib.ptr(window), g.seg, g.hop, g.nfft, g.scale,
              C.byref(desc), _lib.ptr(scratch), scratch.numel())
    return res


def _stft_result(frequency_hz, n_ch, n_f, n_seg, rdtype, dev, coef, bits, reductions, power_scale, reduced_out=None):
    """New output buffers of one qi_stft_out request; the reductions as TfrPlan lays them out (engine.reduced_views)."""
    res = engine.TfrResult(frequency_hz=frequency_hz, power_scale=power_scale)
    if coef:
        res.coef = torch.empty((n_ch, n_f, n_seg), dtype=engine._complex_of(rdtype), device=dev)
    if bits:
        res.bits = torch.empty((n_ch, n_f, n_seg), dtype=rdtype, device=dev)
    if reductions:
        res.reduced, res.power_band, res.power_time, res.stats = engine.reduced_views(
            n_ch, n_f, n_seg, rdtype, dev, reductions, reduced_out)
    return res


def _stft_call(sig_wf, geometry, want_bits=False, _reduce=None):
    """One transform of `sig_wf`; geometry: (n, rdtype) -> the StftGeometry of such records.  -> (frequency_hz, time_s, z, bits);
    _reduce: None, or the options of a reduced product -- dict(coef=True, bits=want_bits, reductions=True, power_scale=1.0)
    -- and the return value is then (frequency_hz, time_s, TfrResult) with device tensors [C, ...]."""
    lib = _lib.require_gpu()
    sig, was_numpy, was_1d = engine.as_signal(sig_wf)
    n_ch, n = sig.shape
    g = geometry(n, sig.dtype)
    dev = sig.device
    win_d = torch.from_numpy(g.window).to(dev)
    if _reduce is not None:
        res = _stft_result(g.frequency_hz, n_ch, g.n_f, g.n_seg, sig.dtype, dev, _reduce.get("coef", True),
                           _reduce.get("bits", want_bits), _reduce.get("reductions", True), _reduce.get("power_scale", 1.0))
        return g.frequency_hz, g.time_s, _stft_out(lib, sig, win_d, g, res)
    z = torch.empty((n_ch, g.n_f, g.n_seg), dtype=engine._complex_of(sig.dtype), device=dev)
    bits = torch.empty((n_ch, g.n_f, g.n_seg), dtype=sig.dtype, device=dev) if want_bits else None
    code = _lib.dtype_code(sig.dtype)
    scratch, nbytes = _lib.scratch(lib.qi_stft_scratch_bytes, dev, code, n_ch, n, g.seg, g.hop, g.nfft)
    _lib.call(lib.qi_stft, dev, code, dev.index, _lib.ptr(sig), n_ch, n, _lib.ptr(win_d), g.seg, g.hop, g.nfft, g.scale, _lib.ptr(z),
              _lib.ptr(bits), float(get_epsilon()), _lib.ptr(scratch), nbytes)
    return g.frequency_hz, g.time_s, engine.finish(z, was_numpy, was_1d), engine.finish(bits, was_numpy, was_1d)


def _stft_windowed(sig_wf, fs, window64, segment_points, overlap_points, nfft_points, extra_scale=1.0, want_bits=False,
                   _reduce=None):
    """_stft_call with the geometry of a float64 window [segment_points]."""
    if len(window64) != int(segment_points):
        raise ValueError(f"a window of {len(window64)} points for segments of {int(segment_points)}")
    return _stft_call(sig_wf, lambda n, rdtype: StftGeometry.from_window(n, fs, window64, overlap_points, nfft_points, extra_scale,
                                                                         rdtype), want_bits, _reduce)


def _stft_from_order(sig_wf, order_args, **options):
    """_stft_call with stft_from_sig's geometry; order_args: (fs, band_order_nth, center_frequency_hz, octaves_below_center).
    A record shorter than the segment is refused before the device is asked for."""
    _order_segment(sig_wf.shape[-1] if hasattr(sig_wf, "shape") else len(sig_wf), *order_args)
    return _stft_call(sig_wf, lambda n, rdtype: StftGeometry.from_order(n, *order_args, rdtype=rdtype), **options)


def _shrunk_segment(sig_wf, segment_points):
    """scipy.signal.stft shortens nperseg to the record when the record is shorter, with a warning
    (SciPy 1.15 signal/_spectral_py.py:_triage_segments); the window is then made for the shorter segment."""
    n = sig_wf.shape[-1] if hasattr(sig_wf, "shape") else len(sig_wf)
    if int(segment_points) > n:
        import warnings

        warnings.warn(f"nperseg = {int(segment_points)} is greater than input length  = {n}, using nperseg = {n}")
        return n
    return int(segment_points)


class StftPlan:
    """stft_from_sig for batches of records of one shape with every buffer kept between calls (window on the device,
    outputs, scratch): the per-call work is the kernels alone.  Results are those of stft_from_sig (ref
    styx_fft.py:14-57); `run` returns (stft_complex [C, nfft/2+1, segments], stft_bits)."""

    def __init__(self, n, channels, frequency_sample_rate_hz, band_order_nth, dtype=torch.float32, device=None):
        self._lib = _lib.require_gpu()
        self.n, self.channels, self.fs = int(n), int(channels), float(frequency_sample_rate_hz)
        self.rdtype = engine._real_dtype(dtype)
        self._geometry = g = StftGeometry.from_order(self.n, self.fs, band_order_nth, rdtype=self.rdtype)
        self.seg, self.hop, self.nfft, self.n_seg, self.n_f, self.scale = g.seg, g.hop, g.nfft, g.n_seg, g.n_f, g.scale
        self.time_s, self.frequency_hz = g.time_s, g.frequency_hz
        self.device = torch.device(device) if device is not None else engine.default_device()
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.window = torch.from_numpy(g.window).to(self.device)
        self.code = _lib.dtype_code(self.rdtype)
        self.z = torch.empty((self.channels, self.n_f, self.n_seg), dtype=engine._complex_of(self.rdtype), device=self.device)
        self.bits = torch.empty((self.channels, self.n_f, self.n_seg), dtype=self.rdtype, device=self.device)
        self.scratch_bytes = int(self._lib.qi_stft_scratch_bytes(self.code, self.channels, self.n, self.seg, self.hop, self.nfft))
        self.scratch = torch.empty(max(self.scratch_bytes, 1), dtype=torch.uint8, device=self.device)
        self._reduced, self._out_scratch = {}, None  # buffers of `reduce`, made on its first call

    @property
    def points(self):
        """complex coefficients one call produces"""
        return self.channels * self.n_f * self.n_seg

    def run(self, sig):
        if sig.shape != (self.channels, self.n) or sig.dtype != self.rdtype or not sig.is_cuda:
            raise ValueError(f"signal must be a [{self.channels}, {self.n}] {self.rdtype} CUDA tensor")
        _lib.call(self._lib.qi_stft, self.device, self.code, self.device.index, _lib.ptr(sig), self.channels, self.n,
                  _lib.ptr(self.window), self.seg, self.hop, self.nfft, self.scale, _lib.ptr(self.z), _lib.ptr(self.bits),
                  float(get_epsilon()), _lib.ptr(self.scratch), self.scratch_bytes)
        return self.z, self.bits

    def reduce(self, sig, coef=False, bits=False, reductions=True, power_scale=1.0, reduced_out=None):
        """The reduced product of the transform -- power_band [C, n_f] and stats [C, 4] float64, power_time [C, n_seg]
        (reductions="band": without it) of P = power_scale |Z|^2 -- from the kernel that forms the coefficients, with the
        panels (`coef`, `bits`: the buffers `run` fills) stored only when asked for (qi_stft_out).  The three reductions are
        views into one dist.reduced_slots(C, n_f, n_seg) buffer, as TfrPlan's are, kept between calls like the plan's other
        buffers (or `reduced_out`)."""
        if sig.shape != (self.channels, self.n) or sig.dtype != self.rdtype or not sig.is_cuda:
            raise ValueError(f"signal must be a [{self.channels}, {self.n}] {self.rdtype} CUDA tensor")
        res = engine.TfrResult(frequency_hz=self.frequency_hz, power_scale=power_scale, coef=self.z if coef else None,
                               bits=self.bits if bits else None)
        if reductions:
            key = "band" if reductions == "band" else "all"
            views = None if reduced_out is not None else self._reduced.get(key)
            if views is None:
                views = engine.reduced_views(self.channels, self.n_f, self.n_seg, self.rdtype, self.device, reductions, reduced_out)
                if reduced_out is None:
                    self._reduced[key] = views
            res.reduced, res.power_band, res.power_time, res.stats = views
        if self._out_scratch is None:  # one scratch for `run` and every form of `reduce` (the form without a panel asks for most)
            nbytes = int(self._lib.qi_stft_out_scratch_bytes(self.code, self.channels, self.n, self.seg, self.hop, self.nfft, 0, 0))
            if nbytes > self.scratch.numel():
                self.scratch = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            self._out_scratch = self.scratch
        return _stft_out(self._lib, sig, self.window, self._geometry, res, self._out_scratch)


def range_samples(n_total, seg, hop, first_segment, segments):
    """(sample0, n_avail): the smallest interval of record samples that the segments first_segment .. first_segment +
    segments - 1 need -- segment m covers [m hop - seg // 2, m hop - seg // 2 + seg), cut to [0, n_total); n_avail = 0 for a
    range that lies in the zero extension (qi_stft_range_samples restated: host arithmetic)."""
    lo = min(n_total, max(0, first_segment * hop - seg // 2))
    hi = min(n_total, (first_segment + segments - 1) * hop - seg // 2 + seg)
    return lo, max(0, hi - lo)


class StftRangePlan:
    """The STFT of a record that is too long for the device, one range of segments at a time (qi_stft_out_range): a segment
    depends on its own samples only, so the ranges of a record give the coefficients of the one-call transform and their
    sums add up to its reductions (stream.StftStream feeds the ranges, stream.StftRecord adds them up).

    Geometry: stft_from_sig's from `band_order_nth` (periodic Hann, half overlap, scale 2 sqrt(pi) / segment), or an explicit
    `window` [seg] (float64 NumPy) with `overlap_points` / `nfft_points` as stft_complex_pow2 takes them (`extra_scale`
    multiplies 1 / sum(window)).  Building a plan is host work; the device is asked for at the first `segment_range`."""

    def __init__(self, n_total, frequency_sample_rate_hz, band_order_nth=None, window=None, overlap_points=None, nfft_points=None,
                 extra_scale=1.0, dtype=torch.float32, device=None):
        self.n_total, self.fs = int(n_total), float(frequency_sample_rate_hz)
        if (band_order_nth is None) == (window is None):
            raise ValueError("give band_order_nth (stft_from_sig's geometry) or a window, not both")
        self.rdtype = engine._real_dtype(dtype)
        if window is None:
            g = StftGeometry.from_order(self.n_total, self.fs, band_order_nth, rdtype=self.rdtype)
        else:
            win64 = np.asarray(window, dtype=np.float64)
            if win64.ndim != 1 or len(win64) < 1:
                raise ValueError("window must be 1-D")
            seg = len(win64)
            if self.n_total < seg:
                raise ValueError(f"record of {self.n_total} samples is shorter than the segment of {seg}")
            g = StftGeometry.from_window(self.n_total, self.fs, win64, int(seg / 2) if overlap_points is None else overlap_points,
                                         int(2 ** np.ceil(np.log2(seg))) if nfft_points is None else nfft_points, extra_scale,
                                         self.rdtype)
        self._geometry = g
        self.seg, self.hop, self.nfft, self.n_seg, self.n_f, self.scale = g.seg, g.hop, g.nfft, g.n_seg, g.n_f, g.scale
        self.time_s, self.frequency_hz = g.time_s, g.frequency_hz
        self._device = device
        self.code = _lib.dtype_code(self.rdtype)
        self._lib, self.device, self.window, self._scratch = None, None, None, None

    def check_range(self, first_segment, segments, sample0, n_avail, pooled=None, pooled_methods=("average",)):
        """The refusals of a range that need no device: ValueError.  -> the pooled windows of the range (0 without pooling)."""
        first_segment, segments, sample0, n_avail = int(first_segment), int(segments), int(sample0), int(n_avail)
        if first_segment < 0 or segments < 1 or first_segment + segments > self.n_seg:
            raise ValueError(f"segments {first_segment} .. {first_segment + segments - 1} of a record of {self.n_seg}")
        if sample0 < 0 or n_avail < 0 or sample0 + n_avail > self.n_total:
            raise ValueError(f"samples {sample0} .. +{n_avail} are not inside a record of {self.n_total}")
        lo, need = range_samples(self.n_total, self.seg, self.hop, first_segment, segments)
        if need > 0 and not (sample0 <= lo and lo + need <= sample0 + n_avail):
            raise ValueError(f"the range needs the record samples {lo} .. {lo + need - 1}, the rows hold {sample0} .. {sample0 + n_avail - 1}")
        if pooled is None:
            return 0
        pooled = int(pooled)
        engine.check_pooled_methods(pooled_methods)
        if pooled < 2:
            raise ValueError(f"pooling factor {pooled}: 2 or more")
        if first_segment % pooled:
            raise ValueError(f"first segment {first_segment} is no multiple of the pooling factor {pooled}")
        if segments % pooled and first_segment + segments != self.n_seg:
            raise ValueError(f"{segments} segments are no multiple of the pooling factor {pooled} and do not end the record")
        return segments // pooled

    def segment_range(self, rows, first_segment, segments, sample0, n_total=None, coef=False, bits=False, reductions=True,
                      pooled=None, pooled_methods=("average",), power_scale=1.0, n_avail=None):
        """The segments first_segment .. first_segment + segments - 1 of the record from `rows` [C, width], a device tensor
        whose row c holds the record samples sample0 .. sample0 + n_avail - 1 (n_avail: default what a row can hold of the
        record; nothing past it is read; rows may be a view with a longer row stride).  -> TfrResult of the range: coef /
        bits [C, n_f, segments] when asked for, power_band / stats over these segments, power_time [C, segments]
        (reductions="band": without it), and with pooled=F `pooled` {method: [C, n_f, segments // F]}, the average / maximum
        of P = power_scale |Z|^2 over the windows of F consecutive segments (first_segment and segments multiples of F; the
        range that ends the record may be ragged, its incomplete window is dropped).  Host-side refusals are ValueErrors
        raised before the device is touched."""
        if n_total is not None and int(n_total) != self.n_total:
            raise ValueError(f"the plan is for records of {self.n_total} samples, not {n_total}")
        if not isinstance(rows, torch.Tensor) or rows.dim() != 2 or rows.dtype != self.rdtype:
            raise ValueError(f"rows must be a 2-D {self.rdtype} tensor [channels, samples]")
        if rows.shape[1] > 1 and rows.stride(1) != 1:
            raise ValueError("the samples of a row must be contiguous")
        first_segment, segments, sample0 = int(first_segment), int(segments), int(sample0)
        if n_avail is None:
            n_avail = max(0, min(rows.shape[1], self.n_total - sample0))
        n_avail = int(n_avail)
        n_ch, stride = rows.shape[0], (rows.stride(0) if rows.shape[0] > 1 else max(rows.shape[1], rows.stride(0)))
        if n_avail > rows.shape[1] or stride < n_avail:
            raise ValueError(f"rows of {rows.shape[1]} samples (stride {stride}) cannot hold {n_avail}")
        windows = self.check_range(first_segment, segments, sample0, n_avail, pooled, pooled_methods)
        if pooled is not None and not reductions:
            raise ValueError("the pooled outputs come with the reductions")
        if not (coef or bits or reductions):
            raise ValueError("nothing to produce")
        self._lib = _lib.require_gpu()
        if not rows.is_cuda:
            raise ValueError("rows must be a CUDA tensor")
        if self.window is None or self.device != rows.device:
            self.device = rows.device
            self.window = torch.from_numpy(self._geometry.window).to(self.device)
        dev = self.device
        res = _stft_result(self.frequency_hz, n_ch, self.n_f, segments, self.rdtype, dev, coef, bits, reductions, power_scale)
        rng = _lib.StftRange(n_total=self.n_total, first_segment=first_segment, segments=segments, sample0=sample0, n_avail=n_avail,
                             row_stride=stride, pool_factor=0)
        if pooled is not None:
            res.pooled = {m: torch.empty((n_ch, self.n_f, windows), dtype=self.rdtype, device=dev) for m in pooled_methods}
            rng.pool_factor = int(pooled)
            rng.pool_mean, rng.pool_max = _lib.ptr(res.pooled.get("average")), _lib.ptr(res.pooled.get("max"))
        nbytes = int(self._lib.qi_stft_range_scratch_bytes(self.code, n_ch, self.seg, self.hop, self.nfft, C.byref(rng), int(bool(coef))))
        if nbytes < 0:
            _lib.check(nbytes)
        if self._scratch is None or self._scratch.numel() < nbytes or self._scratch.device != dev:
            self._scratch = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
        desc = engine.out_descriptor(res, get_epsilon())
        _lib.call(self._lib.qi_stft_out_range, dev, self.code, dev.index, _lib.ptr(rows), n_ch, _lib.ptr(self.window), self.seg,
                  self.hop, self.nfft, self.scale, C.byref(rng), C.byref(desc), _lib.ptr(self._scratch), self._scratch.numel())
        return res


def stft_complex_pow2(
    sig_wf,
    frequency_sample_rate_hz: float,
    segment_points: int,
    overlap_points: int = None,
    nfft_points: int = None,
    alpha: float = 0.25,
):
    """Tukey-window STFT with 50 % overlap by default, last axis (ref styx_fft.py:152-187).
    :return: frequency_stft_hz, time_stft_s, stft_complex [(nfft/2+1) x segments]"""
    if nfft_points is None:
        nfft_points = int(2 ** np.ceil(np.log2(segment_points)))
    if overlap_points is None:
        overlap_points = int(segment_points / 2)
    segment_points = _shrunk_segment(sig_wf, segment_points)
    window = tukey_window_periodic(int(segment_points), alpha)
    f, t, z, _ = _stft_windowed(sig_wf, frequency_sample_rate_hz, window, segment_points, overlap_points, nfft_points)
    return f, t, z


def gtx_complex_pow2(
    sig_wf,
    frequency_sample_rate_hz: float,
    segment_points: int,
    gaussian_sigma: int = None,
    overlap_points: int = None,
    nfft_points: int = None,
):
    """Gaussian-window STFT (ref styx_fft.py:190-227).  :return: frequency_hz, time_s, stft_complex"""
    if nfft_points is None:
        nfft_points = int(2 ** np.ceil(np.log2(segment_points)))
    if overlap_points is None:
        overlap_points = int(segment_points / 2)
    if gaussian_sigma is None:
        gaussian_sigma = int(segment_points / 4)
    segment_points = _shrunk_segment(sig_wf, segment_points)
    window = gaussian_window_periodic(int(segment_points), gaussian_sigma)
    f, t, z, _ = _stft_windowed(sig_wf, frequency_sample_rate_hz, window, segment_points, overlap_points, nfft_points)
    return f, t, z


def stft_from_sig(
    sig_wf,
    frequency_sample_rate_hz: float,
    band_order_nth: float,
    center_frequency_hz: float = None,
    octaves_below_center: int = 4,
):
    """Order-N standardised STFT: periodic-Hann segments sized from N, scaled by 2 sqrt(pi) / segment,
    with its log2 amplitude bits (ref styx_fft.py:14-57).
    :return: stft_complex, stft_bits, time_stft_s, frequency_stft_hz  (note the order)"""
    f, t, z, bits = _stft_from_order(sig_wf, (frequency_sample_rate_hz, band_order_nth, center_frequency_hz, octaves_below_center),
                                     want_bits=True)
    return z, bits, t, f


def stft_reductions_from_sig(
    sig_wf,
    frequency_sample_rate_hz: float,
    band_order_nth: float,
    center_frequency_hz: float = None,
    octaves_below_center: int = 4,
    power_scale: float = 1.0,
):
    """The reduced product of stft_from_sig's panel (same segments, window and scale) without the panel: the marginals
    and entropy sums of P = power_scale |stft_complex|^2 (tfr_info.py:82-94,203-236) from the transform kernel itself.
    sig_wf: [n] or [C, n], NumPy or CUDA tensor.
    :return: TfrResult (device tensors power_band [C, n_f], power_time [C, n_seg], stats [C, 4]), time_stft_s,
        frequency_stft_hz"""
    f, t, res = _stft_from_order(sig_wf, (frequency_sample_rate_hz, band_order_nth, center_frequency_hz, octaves_below_center),
                                 _reduce=dict(coef=False, bits=False, power_scale=power_scale))
    return res, t, f


def welch_power_pow2(
    sig_wf,
    frequency_sample_rate_hz: float,
    segment_points: int,
    nfft_points: int = None,
    overlap_points: int = None,
    alpha: float = 0.25,
):
    """Welch power spectrum: mean over 50 %-overlapped Tukey segments of the one-sided |FFT|^2, "spectrum" scaling
    (ref styx_fft.py:230-266).  :return: frequency_welch_hz, welch_power [nfft/2+1] (or [channels x ...])"""
    lib = _lib.require_gpu()
    if nfft_points is None:
        nfft_points = int(2 ** np.ceil(np.log2(segment_points)))
    if overlap_points is None:
        overlap_points = int(segment_points / 2)
    sig, was_numpy, was_1d = engine.as_signal(sig_wf)
    n_ch, n = sig.shape
    seg, nfft = int(segment_points), int(nfft_points)
    hop = seg - int(overlap_points)
    if n < seg:
        raise ValueError(f"Signal length: {n} is less than the segment: {seg}")
    if not 0 < hop <= seg:
        raise ValueError("noverlap must be less than nperseg.")
    win = _run_window(tukey_window_periodic(seg, alpha), sig.dtype)
    scale = float(1.0 / np.sum(win.astype(np.float64)))
    win_d = torch.from_numpy(win).to(sig.device)
    code = _lib.dtype_code(sig.dtype)
    pxx = torch.empty((n_ch, nfft // 2 + 1), dtype=sig.dtype, device=sig.device)
    scratch, nbytes = _lib.scratch(lib.qi_welch_scratch_bytes, sig.device, code, n_ch, n, seg, hop, nfft)
    _lib.call(lib.qi_welch, sig.device, code, sig.device.index, _lib.ptr(sig), n_ch, n, _lib.ptr(win_d), seg, hop, nfft, scale,
              _lib.ptr(pxx), _lib.ptr(scratch), nbytes)
    return np.fft.rfftfreq(nfft, 1 / frequency_sample_rate_hz), engine.finish(pxx, was_numpy, was_1d)


def _csd_request(sig, frequency_sample_rate_hz, segment_points, nfft_points, overlap_points, alpha, scaling):
    """The argument checks of qi_csd and qi_csd_windows on a [C, n] device tensor, with welch_power_pow2's conventions ->
    (seg, hop, nfft, fs, the window on the device, scale)."""
    if nfft_points is None:
        nfft_points = int(2 ** np.ceil(np.log2(segment_points)))
    if overlap_points is None:
        overlap_points = int(segment_points / 2)
    n_ch, n = sig.shape
    seg, nfft = int(segment_points), int(nfft_points)
    hop = seg - int(overlap_points)
    if n < seg:
        raise ValueError(f"Signal length: {n} is less than the segment: {seg}")
    if not 0 < hop <= seg:
        raise ValueError("noverlap must be less than nperseg.")
    if nfft < seg:
        raise ValueError("nfft must be greater than or equal to nperseg.")
    fs = float(frequency_sample_rate_hz)
    win = _run_window(tukey_window_periodic(seg, alpha), sig.dtype)
    win64 = win.astype(np.float64)
    if scaling == "spectrum":
        scale = float(1.0 / np.sum(win64))
    elif scaling == "density":
        scale = float(np.sqrt(1.0 / (fs * np.sum(win64 * win64))))
    else:
        raise ValueError(f"Unknown scaling: {scaling!r}")
    return seg, hop, nfft, fs, torch.from_numpy(win).to(sig.device), scale


def _csd_matrices(sig, frequency_sample_rate_hz, segment_points, nfft_points, overlap_points, alpha, scaling, want_csd, want_coherence):
    """qi_csd on a [C, n] device tensor with welch_power_pow2's conventions -> (frequency_hz, csd [nf, C, C] or None,
    coherence [nf, C, C] or None), device tensors in the records' precision."""
    lib = _lib.require_gpu()
    seg, hop, nfft, fs, win_d, scale = _csd_request(sig, frequency_sample_rate_hz, segment_points, nfft_points, overlap_points, alpha,
                                                    scaling)
    n_ch, n = sig.shape
    dev, n_f = sig.device, nfft // 2 + 1
    code = _lib.dtype_code(sig.dtype)
    csd = torch.empty((n_f, n_ch, n_ch), dtype=engine._complex_of(sig.dtype), device=dev) if want_csd else None
    coherence = torch.empty((n_f, n_ch, n_ch), dtype=sig.dtype, device=dev) if want_coherence else None
    scratch, nbytes = _lib.scratch(lib.qi_csd_scratch_bytes, dev, code, n_ch, n, seg, hop, nfft)
    _lib.call(lib.qi_csd, dev, code, dev.index, _lib.ptr(sig), n_ch, n, _lib.ptr(win_d), seg, hop, nfft, scale, _lib.ptr(csd),
              _lib.ptr(coherence), _lib.ptr(scratch), nbytes)
    return np.fft.rfftfreq(nfft, 1 / fs), csd, coherence


def csd_matrix_pow2(
    sig_wf,
    frequency_sample_rate_hz: float,
    segment_points: int,
    nfft_points: int = None,
    overlap_points: int = None,
    alpha: float = 0.25,
    scaling: str = "spectrum",
):
    """Cross-spectral matrix of the records of one batch [C x n]: scipy.signal.csd(x_i, x_j) of every pair with
    welch_power_pow2's segments (Tukey window, 50 % overlap by default, mean removed, one-sided, average="mean");
    scaling "spectrum" (1 / sum(w)^2) or "density" (1 / (fs sum(w^2))).  The diagonal is the Welch spectrum of each record.
    :return: frequency_hz, csd [(nfft/2+1) x C x C] complex, Hermitian per bin (csd[f, j, i] is conj(csd[f, i, j]) bit for bit)"""
    sig, was_numpy, _ = engine.as_signal(sig_wf)
    f, csd, _ = _csd_matrices(sig, frequency_sample_rate_hz, segment_points, nfft_points, overlap_points, alpha, scaling, True, False)
    return f, engine.finish(csd, was_numpy, False)


def coherence_matrix_pow2(
    sig_wf,
    frequency_sample_rate_hz: float,
    segment_points: int,
    nfft_points: int = None,
    overlap_points: int = None,
    alpha: float = 0.25,
):
    """Magnitude-squared coherence |S_ij|^2 / (S_ii S_jj) between the records of one batch [C x n]: scipy.signal.coherence of
    every pair, with csd_matrix_pow2's segments.  A bin whose auto-power is 0 is NaN; one segment gives 1.
    :return: frequency_hz, coherence [(nfft/2+1) x C x C]"""
    sig, was_numpy, _ = engine.as_signal(sig_wf)
    f, _, coh = _csd_matrices(sig, frequency_sample_rate_hz, segment_points, nfft_points, overlap_points, alpha, "spectrum", False, True)
    return f, engine.finish(coh, was_numpy, False)


def _csd_window_matrices(sig, frequency_sample_rate_hz, segment_points, window_segments, window_hop_segments, nfft_points, overlap_points,
                         alpha, scaling, frequency_range_hz, want_csd, want_coherence, bins_of=None):
    """qi_csd_windows on a [C, n] device tensor, _csd_matrices' twin -> (frequency_hz [bins] of the formed bins,
    window_time_s [nwin], csd [nwin, bins, C, C] or None, coherence [nwin, bins, C, C] or None).  bins_of: instead of
    frequency_range_hz, a function of the whole frequency table -> (first, count) of the bins to form."""
    lib = _lib.require_gpu()
    seg, hop, nfft, fs, win_d, scale = _csd_request(sig, frequency_sample_rate_hz, segment_points, nfft_points, overlap_points, alpha,
                                                    scaling)
    n_ch, n = sig.shape
    n_seg = (n - seg) // hop + 1
    win = int(window_segments)
    win_hop = max(1, win // 2) if window_hop_segments is None else int(window_hop_segments)
    if win < 1 or win_hop < 1 or win > n_seg:
        raise ValueError(f"a window of {win} segments every {win_hop} does not fit the record's {n_seg} segments")
    f = np.fft.rfftfreq(nfft, 1 / fs)
    first, count = (0, f.size) if bins_of is None else bins_of(f)
    if frequency_range_hz is not None:
        lo, hi = (float(v) for v in frequency_range_hz)
        first, last = np.searchsorted(f, [lo, hi], side="left")  # lo <= f < hi
        first, count = int(first), int(last - first)
        if count < 1:
            raise ValueError(f"no bin of the {f.size} lies in {lo} <= f < {hi} Hz")
    n_win = (n_seg - win) // win_hop + 1
    dev, code = sig.device, _lib.dtype_code(sig.dtype)
    scratch, nbytes = _lib.scratch(lib.qi_csd_windows_scratch_bytes, dev, code, n_ch, n, seg, hop, nfft, first, count, win, win_hop)
    csd = torch.empty((n_win, count, n_ch, n_ch), dtype=engine._complex_of(sig.dtype), device=dev) if want_csd else None
    coherence = torch.empty((n_win, count, n_ch, n_ch), dtype=sig.dtype, device=dev) if want_coherence else None
    _lib.call(lib.qi_csd_windows, dev, code, dev.index, _lib.ptr(sig), n_ch, n, _lib.ptr(win_d), seg, hop, nfft, scale, first, count,
              win, win_hop, _lib.ptr(csd), _lib.ptr(coherence), _lib.ptr(scratch), nbytes)
    # the centre of the samples a window spans: its first sample w win_hop hop, its length (win - 1) hop + seg
    time_s = (np.arange(n_win, dtype=np.float64) * (win_hop * hop) + ((win - 1) * hop + seg) / 2) / fs
    return f[first:first + count], time_s, csd, coherence


def csd_windows_pow2(
    sig_wf,
    frequency_sample_rate_hz: float,
    segment_points: int,
    window_segments: int,
    window_hop_segments: int = None,
    nfft_points: int = None,
    overlap_points: int = None,
    alpha: float = 0.25,
    scaling: str = "spectrum",
    frequency_range_hz=None,
):
    """csd_matrix_pow2 per sliding window of the record's Welch segments: window w is scipy.signal.csd of the sub-record
    that the segments w * window_hop_segments .. + window_segments - 1 span (window_hop_segments: None for
    max(1, window_segments // 2)); segments after the last window are ignored.  frequency_range_hz: (lo, hi) -- only the bins
    lo <= f < hi are formed -- or None (all).  One window over every segment is csd_matrix_pow2 bit for bit.
    :return: frequency_hz [bins], window_time_s [nwin] (the centre of the samples each window spans),
        csd [nwin x bins x C x C] complex, Hermitian per window and bin"""
    sig, was_numpy, _ = engine.as_signal(sig_wf)
    f, t, csd, _ = _csd_window_matrices(sig, frequency_sample_rate_hz, segment_points, window_segments, window_hop_segments, nfft_points,
                                        overlap_points, alpha, scaling, frequency_range_hz, True, False)
    return f, t, engine.finish(csd, was_numpy, False)


def coherence_windows_pow2(
    sig_wf,
    frequency_sample_rate_hz: float,
    segment_points: int,
    window_segments: int,
    window_hop_segments: int = None,
    nfft_points: int = None,
    overlap_points: int = None,
    alpha: float = 0.25,
    frequency_range_hz=None,
):
    """coherence_matrix_pow2 per sliding window of the record's Welch segments, with csd_windows_pow2's windows and bins.
    One segment per window gives 1.
    :return: frequency_hz [bins], window_time_s [nwin], coherence [nwin x bins x C x C]"""
    sig, was_numpy, _ = engine.as_signal(sig_wf)
    f, t, _, coh = _csd_window_matrices(sig, frequency_sample_rate_hz, segment_points, window_segments, window_hop_segments, nfft_points,
                                        overlap_points, alpha, "spectrum", frequency_range_hz, False, True)
    return f, t, engine.finish(coh, was_numpy, False)


def pair_lags_pow2(
    sig_wf,
    frequency_sample_rate_hz: float,
    segment_points: int,
    nfft_points: int = None,
    overlap_points: int = None,
    alpha: float = 0.25,
    band_hz=None,
    weighting: str = "phat",
    upsample: int = 1,
    max_lag_s: float = None,
    window_segments: int = None,
    window_hop_segments: int = None,
):
    """Time delays between every pair of records of one batch [C x n] from the peak of their generalized cross-correlation
    (engine.pair_lags on csd_matrix_pow2's matrices, or on csd_windows_pow2's -- one set of delays per sliding window -- when
    window_segments is given): the delay of pair (i, j), i < j, is positive when record j lags record i -- tau_j - tau_i of
    beamform.plane_wave_delays for a plane wave -- and feeds beamform.slowness_from_lags.  band_hz: (lo, hi), the bins
    lo <= f < hi enter the correlation, or None (all); weighting "plain", "phat" or "scot"; the correlation is normalised
    (plain: the correlation coefficient; phat / scot: a peak of at most 1).  upsample: 1, 2, 4 or 8, the zero padding of the
    spectrum: the peak is searched on a grid of 1 / (upsample fs) seconds and refined by a three-point parabola.  max_lag_s:
    the largest delay searched, None for all of the correlation.
    The correlation of Welch segments is CIRCULAR over nfft_points: a delay d and the delay d - nfft_points / fs are the same
    peak, and the two ends of a segment correlate with each other.  nfft_points >= 2 * segment_points makes it linear.
    :return: lag_s [npair] (or [nwin x npair]) seconds, peak_value of the same shape, pairs [npair x 2] int64 (the (i, j) of
        every column, in the order (0, 1), (0, 2) .. (C - 2, C - 1)); with window_segments also window_time_s [nwin] last"""
    sig, was_numpy, _ = engine.as_signal(sig_wf)
    args = (frequency_sample_rate_hz, segment_points)
    if window_segments is None:
        f, csd, _ = _csd_matrices(sig, *args, nfft_points, overlap_points, alpha, "spectrum", True, False)
        time_s = None
    else:
        f, time_s, csd, _ = _csd_window_matrices(sig, *args, window_segments, window_hop_segments, nfft_points, overlap_points, alpha,
                                                 "spectrum", None, True, False)
    fs, up = float(frequency_sample_rate_hz), int(upsample)
    bins = None
    if band_hz is not None:
        lo, hi = np.searchsorted(f, [float(band_hz[0]), float(band_hz[1])], side="left")  # lo <= f < hi
        if hi <= lo:
            raise ValueError(f"no bin of the {f.size} lies in {band_hz[0]} <= f < {band_hz[1]} Hz")
        bins = (int(lo), int(hi))
    largest = (f.size - 1) * up - 1
    max_lag = largest if max_lag_s is None else min(largest, int(np.floor(float(max_lag_s) * fs * up)))
    # (the one-sided doubling of the matrices is undone for the plain correlation; under PHAT and SCOT it cancels by itself)
    lag, value, _ = engine.pair_lags(csd, bins=bins, weighting=weighting, halve_interior=weighting == "plain", normalize=True, upsample=up,
                                     max_lag=max_lag)
    rows, cols = np.triu_indices(sig.shape[0], 1)
    out = (engine.finish(lag / fs, was_numpy, False), engine.finish(value, was_numpy, False), np.stack([rows, cols], axis=1).astype(np.int64))
    return out if time_s is None else out + (time_s,)


def _csd_pairs(sig_x, sig_y, want_coherence, *args):
    """The pair forms: row c of sig_x against row c of sig_y, from the matrices of the stacked records [x ; y] -- the entries
    (c, C + c), which are the matrix forms' bits (an entry is a function of its two records alone)."""
    x, x_numpy, was_1d = engine.as_signal(sig_x)
    y, y_numpy, _ = engine.as_signal(sig_y, device=x.device)
    if x.shape != y.shape or np.ndim(sig_x) != np.ndim(sig_y):
        raise ValueError(f"sig_x and sig_y must have the same shape, got {tuple(np.shape(sig_x))} and {tuple(np.shape(sig_y))}")
    if x.dtype != y.dtype:
        x, y = x.to(torch.float64), y.to(torch.float64)
    n_ch = x.shape[0]
    f, csd, coh = _csd_matrices(torch.cat([x, y]), *args, not want_coherence, want_coherence)
    full = coh if want_coherence else csd
    rows = torch.arange(n_ch, device=full.device)
    pairs = full[:, rows, rows + n_ch].transpose(0, 1).contiguous()  # [C, nf]
    return f, engine.finish(pairs, x_numpy and y_numpy, was_1d)


def csd_pow2(
    sig_x,
    sig_y,
    frequency_sample_rate_hz: float,
    segment_points: int,
    nfft_points: int = None,
    overlap_points: int = None,
    alpha: float = 0.25,
    scaling: str = "spectrum",
):
    """scipy.signal.csd(sig_x, sig_y) with csd_matrix_pow2's conventions: a 1-D pair, or two equal-shaped batches [C x n]
    paired row by row.  :return: frequency_hz, csd [nfft/2+1] (or [C x ...]) complex"""
    return _csd_pairs(sig_x, sig_y, False, frequency_sample_rate_hz, segment_points, nfft_points, overlap_points, alpha, scaling)


def coherence_pow2(
    sig_x,
    sig_y,
    frequency_sample_rate_hz: float,
    segment_points: int,
    nfft_points: int = None,
    overlap_points: int = None,
    alpha: float = 0.25,
):
    """scipy.signal.coherence(sig_x, sig_y) with coherence_matrix_pow2's conventions: a 1-D pair, or two equal-shaped batches
    paired row by row.  :return: frequency_hz, coherence [nfft/2+1] (or [C x ...])"""
    return _csd_pairs(sig_x, sig_y, True, frequency_sample_rate_hz, segment_points, nfft_points, overlap_points, alpha, "spectrum")
