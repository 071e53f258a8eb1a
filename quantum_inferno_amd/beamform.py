"""
Frequency-wavenumber (f-k) analysis of a sensor array: steered power of the cross-spectral matrices over a grid of
slowness vectors (engine.beam_power, include/qi_beam.h), Capon's minimum-variance power over the same grid
(engine.csd_whiten and engine.capon_power, include/qi_adaptive.h), and the MUSIC power of the matrices' noise subspaces
(engine.csd_eigh and engine.music_power, include/qi_subspace.h) -- and, once the map has a peak, the signal from that
direction: beam panels and beam waveforms with Bartlett or MVDR weights (engine.beam_weights and engine.beam_steer,
include/qi_steer.h).  fk_timeline_pow2 runs the three power forms per sliding window of the record
(styx_fft.csd_windows_pow2's matrices, include/qi_windows.h): a detection timeline; fk_timeline_cq is its constant-Q twin on
the CWT or Stockwell panel, every band in a window of so many of its own periods (constant_q_windows, band_window_times;
engine.cross_spectra_bands' matrices, include/qi_bands.h).  Without a grid, slowness_from_lags
fits the slowness vector to the pair delays of styx_fft.pair_lags_pow2 (the peaks of the generalized cross-correlations,
include/qi_lags.h) and lag_closure is their consistency check.  In the time domain, with no matrix, segment or narrow-band
assumption: fisher_timeline, the sliding delay-and-sum F detector, and beam_traces_delay, beam waveforms for delays of any
length (engine.time_beam_power and engine.time_beam_traces, include/qi_timebeam.h).  The reference (quantum-inferno) has no
array processing; the conventions below are the usual ones of infrasound and seismic array work.

Geometry.  Positions are [C, 2] metres (x east, y north).  A slowness vector s [s/m] points the way the wave TRAVELS; a
plane wave reaches sensor i later by tau_i = s . r_i seconds.  The back azimuth is where it comes FROM: the direction of
-s in degrees clockwise from north; the trace velocity is 1 / |s|.

The helpers are host code on torch float64; only plane_wave_delays' result and the work of fk_power_pow2,
capon_power_pow2, music_power_pow2, fk_timeline_pow2, fk_timeline_cq, beam_stft_pow2, beam_traces_tukey, fisher_timeline and
beam_traces_delay are on the device.
"""
import numpy as np
import torch

from . import engine, styx_fft
from .utilities import short_time_fft


def _host64(a, cols, what):
    t = a.detach().cpu() if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64)))
    t = t.to(torch.float64)
    if t.dim() != 2 or t.shape[1] != cols or t.shape[0] < 1:
        raise ValueError(f"{what} must be [count, {cols}], got shape {tuple(t.shape)}")
    return t


def slowness_grid(max_slowness_s_per_m: float, points: int) -> torch.Tensor:
    """A square grid of points x points slowness vectors from -max to +max on both axes -> [points^2, 2] (s_x, s_y); the
    x component (east) runs fastest: vector (ix, iy) is row iy * points + ix."""
    if points < 1 or not max_slowness_s_per_m > 0:
        raise ValueError("slowness_grid needs points >= 1 and a positive largest slowness")
    axis = torch.linspace(-float(max_slowness_s_per_m), float(max_slowness_s_per_m), int(points), dtype=torch.float64)
    if points == 1:
        axis = torch.zeros(1, dtype=torch.float64)
    sy, sx = torch.meshgrid(axis, axis, indexing="ij")
    return torch.stack([sx.reshape(-1), sy.reshape(-1)], dim=1)


def polar_slowness_grid(back_azimuth_deg, trace_velocity_m_s) -> torch.Tensor:
    """Slowness vectors of every (trace velocity, back azimuth) pair -> [len(velocity) * len(azimuth), 2]; the back azimuth
    runs fastest.  s = -(sin az, cos az) / v: the wave travels away from where it comes from."""
    az = torch.deg2rad(torch.as_tensor(np.atleast_1d(np.asarray(back_azimuth_deg, dtype=np.float64))))
    v = torch.as_tensor(np.atleast_1d(np.asarray(trace_velocity_m_s, dtype=np.float64)))
    if az.numel() < 1 or v.numel() < 1 or not bool((v > 0).all()):
        raise ValueError("polar_slowness_grid needs back azimuths and positive trace velocities")
    sx = -torch.sin(az)[None, :] / v[:, None]
    sy = -torch.cos(az)[None, :] / v[:, None]
    return torch.stack([sx.reshape(-1), sy.reshape(-1)], dim=1)


def plane_wave_delays(positions_m, slowness, device=None) -> torch.Tensor:
    """tau[g, i] = s_g . r_i seconds -> [G, C] float64 on the device: the delays_s of engine.beam_power."""
    r = _host64(positions_m, 2, "positions_m")
    s = _host64(slowness, 2, "slowness")
    tau = s[:, 0:1] * r[:, 0][None, :] + s[:, 1:2] * r[:, 1][None, :]
    return tau.contiguous().to(device if device is not None else engine.default_device())


def back_azimuth_and_velocity(slowness):
    """-> (back azimuth in degrees clockwise from north in [0, 360), trace velocity in m/s) of slowness vectors [..., 2]
    (torch float64 on the host).  A zero vector (vertical incidence) has azimuth 0 and infinite velocity."""
    s = slowness.detach().cpu() if isinstance(slowness, torch.Tensor) else torch.from_numpy(np.asarray(slowness, dtype=np.float64))
    s = s.to(torch.float64)
    if s.shape[-1] != 2:
        raise ValueError(f"slowness must be [..., 2], got shape {tuple(s.shape)}")
    az = torch.remainder(torch.rad2deg(torch.atan2(-s[..., 0], -s[..., 1])), 360.0)
    norm = torch.hypot(s[..., 0], s[..., 1])
    az = torch.where(norm == 0, torch.zeros_like(az), az)
    return az, 1.0 / norm


def band_offsets(frequency_hz, edges_hz) -> np.ndarray:
    """Offsets of the bands edges[b] <= f < edges[b + 1] into an ascending frequency table -> int64 [len(edges)], the
    `bands` of engine.beam_power.  Every band must hold a bin."""
    f = np.asarray(frequency_hz, dtype=np.float64)
    edges = np.asarray(edges_hz, dtype=np.float64)
    if f.ndim != 1 or edges.ndim != 1 or edges.size < 2 or np.any(np.diff(f) <= 0):
        raise ValueError("band_offsets needs an ascending frequency table and at least two edges")
    first = np.searchsorted(f, edges, side="left").astype(np.int64)
    if np.any(np.diff(first) <= 0):
        raise ValueError(f"a band of {edges.tolist()} Hz holds no bin of the table")
    return first


def _array_matrices(sig_wf, frequency_sample_rate_hz, positions_m, slowness, segment_points, overlap_points, nfft_points, alpha,
                    band_edges_hz):
    """What the *_pow2 functions do before their form: records [C x n] -> (was_numpy, bin frequencies, cross-spectral
    matrices on the device, band offsets or None, band_frequency_ranges, delays on the device), the positions checked against
    the records."""
    sig, was_numpy, _ = engine.as_signal(sig_wf)
    f, csd, _ = styx_fft._csd_matrices(sig, frequency_sample_rate_hz, segment_points, nfft_points, overlap_points, alpha, "spectrum",
                                       True, False)
    if band_edges_hz is None:
        bands, ranges = None, np.stack([f, f], axis=1)
    else:
        bands = band_offsets(f, band_edges_hz)
        ranges = np.stack([f[bands[:-1]], f[bands[1:] - 1]], axis=1)
    tau = plane_wave_delays(positions_m, slowness, sig.device)
    if tau.shape[1] != sig.shape[0]:
        raise ValueError(f"{tau.shape[1]} positions for {sig.shape[0]} records")
    return was_numpy, f, csd, bands, ranges, tau


def fk_power_pow2(
    sig_wf,
    frequency_sample_rate_hz: float,
    positions_m,
    slowness,
    segment_points: int,
    overlap_points: int = None,
    nfft_points: int = None,
    alpha: float = 0.25,
    band_edges_hz=None,
    normalize: bool = True,
):
    """f-k power of the records of one array [C x n]: styx_fft.csd_matrix_pow2's cross-spectral matrices (Welch segments,
    Tukey window, spectrum scaling), steered over the slowness vectors [G, 2] and summed over the bands between
    band_edges_hz (None: every bin its own band).  normalize: the semblance (in [0, 1]) instead of the power.  Neither the
    segments' panel nor the matrices leave the device.
    :return: band_frequency_ranges [nb x 2] (first and last bin frequency of every band), power [nb x G], peak_index [nb]
        (row of `slowness` with the largest power in the band), peak_value [nb]"""
    was_numpy, f, csd, bands, ranges, tau = _array_matrices(sig_wf, frequency_sample_rate_hz, positions_m, slowness, segment_points,
                                                            overlap_points, nfft_points, alpha, band_edges_hz)
    power, index, value = engine.beam_power(csd, f, tau, bands=bands, normalize=normalize, peaks=True)
    return ranges, engine.finish(power, was_numpy, False), engine.finish(index, was_numpy, False), engine.finish(value, was_numpy, False)


def capon_power_pow2(
    sig_wf,
    frequency_sample_rate_hz: float,
    positions_m,
    slowness,
    segment_points: int,
    overlap_points: int = None,
    nfft_points: int = None,
    alpha: float = 0.25,
    band_edges_hz=None,
    loading: float = 1e-2,
):
    """Capon (minimum-variance) f-k power of the records of one array [C x n], fk_power_pow2's twin: the same cross-spectral
    matrices, loaded on the diagonal with `loading` times their mean auto-power and factored once per bin
    (engine.csd_whiten), then 1 / (e^H R^-1 e) over the slowness vectors [G, 2], summed over the bands between band_edges_hz
    (engine.capon_power).  The power has fk_power_pow2's units with normalize=False and never exceeds it; there is no
    semblance.  Neither the panel, the matrices nor their factors leave the device: only the power, the peaks and info do.
    A matrix averaged over fewer segments than there are sensors is singular: such records need loading > 0.  A bin whose
    loaded matrix still does not factor has info != 0, and the band that holds it is NaN (its peak the first NaN).
    :return: band_frequency_ranges [nb x 2], power [nb x G], peak_index [nb], peak_value [nb] as fk_power_pow2 returns them,
        info [bins] int32: 0, or the 1-based pivot at which the bin's factorisation failed"""
    was_numpy, f, csd, bands, ranges, tau = _array_matrices(sig_wf, frequency_sample_rate_hz, positions_m, slowness, segment_points,
                                                            overlap_points, nfft_points, alpha, band_edges_hz)
    whitener, info = engine.csd_whiten(csd, loading=loading, info=True)
    power, index, value = engine.capon_power(whitener, f, tau, bands=bands, peaks=True)
    return (ranges, engine.finish(power, was_numpy, False), engine.finish(index, was_numpy, False), engine.finish(value, was_numpy, False),
            engine.finish(info, was_numpy, False))


def music_power_pow2(
    sig_wf,
    frequency_sample_rate_hz: float,
    positions_m,
    slowness,
    segment_points: int,
    overlap_points: int = None,
    nfft_points: int = None,
    alpha: float = 0.25,
    band_edges_hz=None,
    n_sources: int = 1,
):
    """MUSIC f-k power of the records of one array [C x n], capon_power_pow2's twin: the same cross-spectral matrices,
    diagonalised once per bin (engine.csd_eigh), then C / (e^H P e) over the slowness vectors [G, 2] with P the projector onto
    the eigenvectors of the C - n_sources smallest eigenvalues, averaged over the bands between band_edges_hz
    (engine.music_power).  The power is dimensionless, at least 1 and large where a steering vector leaves the noise subspace:
    it locates up to n_sources < C uncorrelated sources and says nothing of their strength.  There is no loading: a matrix
    averaged over fewer segments than there are sensors has zero eigenvalues, which belong to the noise subspace as they are.
    Neither the panel, the matrices nor their eigenpairs leave the device: only the power, the peaks and info do.  A bin whose
    matrix does not diagonalise (one that holds a value that is not finite) has info != 0, and the band that holds it is NaN
    (its peak the first NaN).
    :return: band_frequency_ranges [nb x 2], power [nb x G], peak_index [nb], peak_value [nb] as fk_power_pow2 returns them,
        info [bins] int32: 0, or 1 where the bin's matrix did not converge"""
    was_numpy, f, csd, bands, ranges, tau = _array_matrices(sig_wf, frequency_sample_rate_hz, positions_m, slowness, segment_points,
                                                            overlap_points, nfft_points, alpha, band_edges_hz)
    _, vectors, info = engine.csd_eigh(csd, info=True)
    power, index, value = engine.music_power(vectors, n_sources, f, tau, bands=bands, peaks=True)
    return (ranges, engine.finish(power, was_numpy, False), engine.finish(index, was_numpy, False), engine.finish(value, was_numpy, False),
            engine.finish(info, was_numpy, False))


TIMELINE_METHODS = ("bartlett", "capon", "music")


def fk_timeline_pow2(
    sig_wf,
    frequency_sample_rate_hz: float,
    positions_m,
    slowness,
    segment_points: int,
    window_segments: int,
    window_hop_segments: int = None,
    overlap_points: int = None,
    nfft_points: int = None,
    alpha: float = 0.25,
    band_edges_hz=None,
    method: str = "bartlett",
    normalize: bool = True,
    loading: float = 1e-2,
    n_sources: int = 1,
):
    """Detection timeline of the records of one array [C x n]: fk_power_pow2 (method "bartlett"), capon_power_pow2 ("capon")
    or music_power_pow2 ("music") per sliding window of the record's Welch segments -- when did something arrive, and from
    where.  styx_fft.csd_windows_pow2's matrices (window_segments segments every window_hop_segments, None for half a
    window) are formed in one launch for the bins of the bands only, and the form runs once on the stack of all windows:
    window w's band b is band w * nb + b of a table in which the frequencies repeat per window.  normalize (bartlett only):
    the semblance instead of the power; the other methods have none and refuse normalize=False.  Nothing but the results
    leaves the device.  back_azimuth_and_velocity(slowness[peak_index]) gives the timeline's azimuth and velocity columns,
    fisher_from_semblance(peak_value, C) its F ratio.
    :return: window_time_s [nwin], band_frequency_ranges [nb x 2], power [nwin x nb x G], peak_index [nwin x nb],
        peak_value [nwin x nb], info: None for bartlett, [nwin x bins] int32 for capon / music (as those functions return it)"""
    if method not in TIMELINE_METHODS:
        raise ValueError(f"method must be one of {TIMELINE_METHODS}, got {method!r}")
    if method != "bartlett" and not normalize:
        raise ValueError(f"normalize belongs to the bartlett method: there is no {method} semblance to leave out")
    sig, was_numpy, _ = engine.as_signal(sig_wf)
    table = {}

    def bins_of(f):
        # only the bins of the bands are formed: one window's last band is followed by the next window's first
        table["bands"] = None if band_edges_hz is None else band_offsets(f, band_edges_hz)
        return (0, f.size) if table["bands"] is None else (int(table["bands"][0]), int(table["bands"][-1] - table["bands"][0]))

    f, time_s, csd, _ = styx_fft._csd_window_matrices(sig, frequency_sample_rate_hz, segment_points, window_segments, window_hop_segments,
                                                      nfft_points, overlap_points, alpha, "spectrum", None, True, False, bins_of=bins_of)
    n_win, bins, n_ch, _ = csd.shape
    if table["bands"] is None:
        bands, n_b, ranges = None, bins, np.stack([f, f], axis=1)
    else:
        local = table["bands"] - table["bands"][0]
        n_b = local.size - 1
        ranges = np.stack([f[local[:-1]], f[local[1:] - 1]], axis=1)
        bands = np.concatenate([(np.arange(n_win, dtype=np.int64)[:, None] * bins + local[None, :-1]).reshape(-1), [n_win * bins]])
    tau = plane_wave_delays(positions_m, slowness, sig.device)
    if tau.shape[1] != n_ch:
        raise ValueError(f"{tau.shape[1]} positions for {n_ch} records")
    stack, f_all, info = csd.reshape(n_win * bins, n_ch, n_ch), np.tile(f, n_win), None
    if method == "bartlett":
        power, index, value = engine.beam_power(stack, f_all, tau, bands=bands, normalize=normalize, peaks=True)
    elif method == "capon":
        whitener, info = engine.csd_whiten(stack, loading=loading, info=True)
        power, index, value = engine.capon_power(whitener, f_all, tau, bands=bands, peaks=True)
    else:
        _, vectors, info = engine.csd_eigh(stack, info=True)
        power, index, value = engine.music_power(vectors, n_sources, f_all, tau, bands=bands, peaks=True)
    return (time_s, ranges, engine.finish(power.reshape(n_win, n_b, -1), was_numpy, False),
            engine.finish(index.reshape(n_win, n_b), was_numpy, False), engine.finish(value.reshape(n_win, n_b), was_numpy, False),
            None if info is None else engine.finish(info.reshape(n_win, bins), was_numpy, False))


def constant_q_windows(frequency_hz, frequency_sample_rate_hz: float, n: int, window_cycles: float, hop_fraction: float = 0.5,
                       max_terms: int = 4096):
    """The window geometry of engine.cross_spectra_bands for a constant-Q band table (host code): band b's window spans
    window_cycles of its own periods, span = round(window_cycles * fs / f_b) samples (at least 1); it is summed at every
    stride-th sample, stride = max(1, ceil(span / max_terms)), terms = (span - 1) // stride + 1; windows start every
    hop = max(1, round(hop_fraction * span)) samples.  max_terms: None for no stride.
    max_terms is a cap on work, not a measured number.  A window of window_cycles periods of a band of quality Q holds on the
    order of window_cycles / Q independent samples -- the coefficients of a band decorrelate over the atom's duration, about
    Q periods -- so 4096 terms oversample it by two orders of magnitude at every order the project uses; the stride thins
    the low bands' sums (10^5 consecutive samples of a 2^20-sample order-3 panel) and leaves every window of up to 4096
    samples as it is.
    :return: bins = (first, count): the contiguous range of bands whose span fits in n; terms, hop, stride [count] int64 of
        those bands.  Raises ValueError if no band fits or the bands that fit are not contiguous."""
    f = np.asarray(frequency_hz, dtype=np.float64)
    fs = float(frequency_sample_rate_hz)
    if f.ndim != 1 or f.size < 1 or not np.all(f > 0) or not fs > 0 or not window_cycles > 0 or not hop_fraction > 0 or int(n) < 1:
        raise ValueError("constant_q_windows needs positive band frequencies, a sample rate, window_cycles, hop_fraction and n")
    if max_terms is not None and int(max_terms) < 1:
        raise ValueError(f"max_terms must be at least 1 or None, got {max_terms}")
    span = np.maximum(1, np.rint(float(window_cycles) * fs / f)).astype(np.int64)
    stride = np.ones_like(span) if max_terms is None else np.maximum(1, -(-span // int(max_terms)))
    terms = (span - 1) // stride + 1
    hop = np.maximum(1, np.rint(float(hop_fraction) * span)).astype(np.int64)
    fits = np.flatnonzero(span <= int(n))
    if fits.size == 0:
        raise ValueError(f"no band's window of {window_cycles} periods fits in {n} samples")
    first, count = int(fits[0]), int(fits.size)
    if fits[-1] - fits[0] + 1 != count:
        raise ValueError("the bands whose window fits the record are not a contiguous range of the table")
    cut = slice(first, first + count)
    return (first, count), terms[cut].copy(), hop[cut].copy(), stride[cut].copy()


def band_window_times(offsets, terms, hop, stride, frequency_sample_rate_hz: float) -> np.ndarray:
    """The centre, in seconds, of the samples that every matrix of engine.cross_spectra_bands' stack spans: row
    offsets[b] + w covers the samples w * hop[b] .. w * hop[b] + span[b] - 1, span[b] = (terms[b] - 1) * stride[b] + 1, and
    its time is (w * hop[b] + span[b] / 2) / fs -- styx_fft.csd_windows_pow2's convention.  -> [total] float64."""
    off, t, h, s = (np.asarray(a, dtype=np.int64) for a in (offsets, terms, hop, stride))
    if off.ndim != 1 or off.size < 2 or not (t.shape == h.shape == s.shape == (off.size - 1,)) or off[0] != 0 or np.any(np.diff(off) < 1):
        raise ValueError("band_window_times needs count + 1 ascending offsets from 0 and three tables of count values")
    n_win = np.diff(off)
    w = np.arange(off[-1], dtype=np.int64) - np.repeat(off[:-1], n_win)
    span = (t - 1) * s + 1
    return (w * np.repeat(h, n_win) + np.repeat(span, n_win) / 2.0) / float(frequency_sample_rate_hz)


def fk_timeline_cq(
    sig_wf,
    frequency_sample_rate_hz: float,
    positions_m,
    slowness,
    band_order_nth: float,
    window_cycles: float,
    hop_fraction: float = 0.5,
    max_terms: int = 4096,
    transform: str = "cwt",
    method: str = "bartlett",
    normalize: bool = True,
    loading: float = 1e-2,
    n_sources: int = 1,
):
    """Constant-Q detection timeline of the records of one array [C x n], n a power of two: fk_timeline_pow2 on the order-N
    CWT (transform "cwt", styx_cwt's atoms with the "norm" dictionary) or Stockwell transform ("stx") instead of the STFT,
    every band in a window of window_cycles of its own periods (constant_q_windows) -- PMCC's geometry: short windows where
    the periods are short.  The panel of all records comes from a borrowed plan and stays on the device; the matrices of all
    bands and windows are one launch (engine.cross_spectra_bands, weight 1 / terms: the window's mean); the form (method
    "bartlett", "capon" or "music", with fk_timeline_pow2's arguments and checks) runs once on the flat stack, every matrix
    its own band, with the band's centre frequency repeated per window.  Nothing but the results leaves the device.

    The narrow-band assumption.  A band's matrices are steered by exp(-i 2 pi f_b tau) at its centre frequency f_b alone.
    That holds while the delays across the array are short against the atom's duration, f_b * max|tau| << Q (Q about
    0.375 * band_order_nth periods to one standard deviation of the envelope): beyond it the records' atoms no longer overlap, the
    coherence falls and the peak flattens -- widen the bands' atoms (a higher order) or shrink the array.

    Conjugation.  The atoms are exp(+i omega t) under a Gaussian and the panel is the record's correlation with them, so a
    record that arrives later by tau has its coefficients multiplied by exp(-i 2 pi f_b tau), as an STFT's are: with
    csd[i, j] = conj(Z_i) Z_j the form e^H S e of engine.beam_power, e_i = exp(2 pi i f tau_i), peaks at the wave's own
    slowness, and the delays are passed as plane_wave_delays gives them, not negated (tests/test_bands_cpu.py pins it with the
    CPU restatement's float64 CWT of a plane wave).
    :return: frequency_hz [count] of the bands whose window fits the record, offsets [count + 1] (band b's windows are the
        rows offsets[b] .. offsets[b + 1] - 1 of what follows), window_time_s [total], power [total x G], peak_index [total],
        peak_value [total], info: None for bartlett, [total] int32 for capon / music"""
    from . import styx_cwt, styx_stx

    if method not in TIMELINE_METHODS:
        raise ValueError(f"method must be one of {TIMELINE_METHODS}, got {method!r}")
    if method != "bartlett" and not normalize:
        raise ValueError(f"normalize belongs to the bartlett method: there is no {method} semblance to leave out")
    if transform not in ("cwt", "stx"):
        raise ValueError(f"transform must be 'cwt' or 'stx', got {transform!r}")
    sig, was_numpy, _ = engine.as_signal(sig_wf)
    n_ch, n = sig.shape
    tau = plane_wave_delays(positions_m, slowness, sig.device)
    if tau.shape[1] != n_ch:
        raise ValueError(f"{tau.shape[1]} positions for {n_ch} records")
    if transform == "cwt":
        res = styx_cwt._cwt_panel(band_order_nth, sig, frequency_sample_rate_hz)
    else:
        res = styx_stx._stx_panel(band_order_nth, sig, frequency_sample_rate_hz)
    f_hz = np.asarray(res.frequency_hz, dtype=np.float64)
    bins, terms, hop, stride = constant_q_windows(f_hz, frequency_sample_rate_hz, n, window_cycles, hop_fraction, max_terms)
    offsets, stack = engine.cross_spectra_bands(res.coef, terms, hop, stride, weight=1.0 / terms, bins=bins)
    f_b = f_hz[bins[0]:bins[0] + bins[1]]
    f_all, info = np.repeat(f_b, np.diff(offsets)), None
    if method == "bartlett":
        power, index, value = engine.beam_power(stack, f_all, tau, normalize=normalize, peaks=True)
    elif method == "capon":
        whitener, info = engine.csd_whiten(stack, loading=loading, info=True)
        power, index, value = engine.capon_power(whitener, f_all, tau, peaks=True)
    else:
        _, vectors, info = engine.csd_eigh(stack, info=True)
        power, index, value = engine.music_power(vectors, n_sources, f_all, tau, peaks=True)
    time_s = band_window_times(offsets, terms, hop, stride, frequency_sample_rate_hz)
    return (f_b, offsets, time_s, engine.finish(power, was_numpy, False), engine.finish(index, was_numpy, False),
            engine.finish(value, was_numpy, False), None if info is None else engine.finish(info, was_numpy, False))


def fisher_from_semblance(semblance, sensors: int):
    """The frequency-domain F ratio of a steered band from its semblance s (fk_power_pow2's and fk_timeline_pow2's
    normalize=True value): F = (C - 1) s / (1 - s), the beam's power over the residual's per degree of freedom, for C sensors.
    s = 0 gives 0, s = 1 / C (uncorrelated records) gives 1, s = 1 gives inf, NaN stays NaN.  Host or device arithmetic on
    whatever came in: a NumPy array, a tensor or a number.  With back_azimuth_and_velocity(slowness[peak_index]) these are
    the columns of a detection timeline."""
    c = int(sensors)
    if c < 2:
        raise ValueError(f"the F ratio needs at least two sensors, got {sensors}")
    if isinstance(semblance, torch.Tensor):
        return (c - 1) * semblance / (1 - semblance)
    s = np.asarray(semblance, dtype=np.float64) if not isinstance(semblance, np.ndarray) else semblance
    with np.errstate(divide="ignore", invalid="ignore"):
        return (c - 1) * s / (1 - s)


def _lags64(lags_s, what="lags_s"):
    t = lags_s if isinstance(lags_s, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(lags_s, dtype=np.float64)))
    if t.dim() < 1 or t.shape[-1] < 1:
        raise ValueError(f"{what} must be [..., pairs], got shape {tuple(t.shape)}")
    return t.to(torch.float64)


def slowness_from_lags(lags_s, positions_m, weights=None):
    """The slowness vector that fits the pair delays of styx_fft.pair_lags_pow2 in the weighted least-squares sense:
    lag_ij = s . (r_j - r_i) for every pair i < j in the order (0, 1), (0, 2) .. (C - 2, C - 1) -- two unknowns, the 2 x 2
    normal equations solved in closed form.  lags_s: [..., C (C - 1) / 2] seconds, NumPy or a tensor on any device (leading
    dimensions, the windows of a timeline, are a batch); positions_m: [C, 2]; weights: None (1), or non-negative values
    [pairs] or [..., pairs] (peak values, say).  Collinear sensors leave s undetermined: NaN.
    -> (slowness [..., 2], rms_residual_s [...]: the root of the weighted mean squared lag_ij - s . (r_j - r_i)), torch float64
    on the device of the lags.  back_azimuth_and_velocity takes the slowness."""
    lag = _lags64(lags_s)
    r = _host64(positions_m, 2, "positions_m")
    rows, cols = np.triu_indices(r.shape[0], 1)
    if lag.shape[-1] != rows.size:
        raise ValueError(f"{r.shape[0]} positions make {rows.size} pairs, lags_s holds {lag.shape[-1]}")
    d = (r[cols] - r[rows]).to(lag.device)  # [pairs, 2]
    w = torch.ones_like(lag) if weights is None else torch.broadcast_to(_lags64(weights, "weights").to(lag.device), lag.shape)
    dx, dy = d[:, 0], d[:, 1]
    axx, axy, ayy = (w * dx * dx).sum(-1), (w * dx * dy).sum(-1), (w * dy * dy).sum(-1)
    bx, by = (w * dx * lag).sum(-1), (w * dy * lag).sum(-1)
    det = axx * ayy - axy * axy
    det = torch.where(det == 0, torch.full_like(det, float("nan")), det)
    s = torch.stack([(ayy * bx - axy * by) / det, (axx * by - axy * bx) / det], dim=-1)
    res = lag - (s[..., 0:1] * dx + s[..., 1:2] * dy)
    return s, torch.sqrt((w * res * res).sum(-1) / w.sum(-1))


def lag_closure(lags_s, sensors: int):
    """The closure of pair delays around every triplet of sensors i < j < k: tau_ij + tau_jk - tau_ik, 0 for the delays of
    one plane wave and for any set of delays that are differences of per-sensor times -- the consistency check of the PMCC
    family.  lags_s: [..., C (C - 1) / 2] in styx_fft.pair_lags_pow2's pair order, NumPy or tensor.
    -> [..., C (C - 1) (C - 2) / 6] torch float64 on the device of the lags, triplets in the order (0, 1, 2), (0, 1, 3) .."""
    c = int(sensors)
    lag = _lags64(lags_s)
    if c < 3 or lag.shape[-1] != c * (c - 1) // 2:
        raise ValueError(f"a closure needs three sensors and their C (C - 1) / 2 delays, got {sensors} sensors and {lag.shape[-1]} delays")
    pair = lambda i, j: i * c - i * (i + 1) // 2 + (j - i - 1)  # noqa: E731
    trip = [(i, j, k) for i in range(c) for j in range(i + 1, c) for k in range(j + 1, c)]
    ij, jk, ik = (torch.tensor([pair(*t) for t in sel], dtype=torch.int64, device=lag.device)
                  for sel in ([(i, j) for i, j, k in trip], [(j, k) for i, j, k in trip], [(i, k) for i, j, k in trip]))
    return lag[..., ij] + lag[..., jk] - lag[..., ik]


BEAM_METHODS = ("bartlett", "capon")


def _panel_weights(panel, frequency_hz, positions_m, slowness, method, loading):
    """The weights step of beam_stft_pow2 and beam_traces_tukey: panel [C, nf, segments] on the device -> (weights
    [nf, K, C], info [nf] or None).  bartlett: e / C.  capon: the MVDR weights of the panel's own cross-spectral matrices
    (engine.cross_spectra with weight 1 / segments), loaded and factored once per bin (engine.csd_whiten)."""
    if method not in BEAM_METHODS:
        raise ValueError(f"method must be one of {BEAM_METHODS}, got {method!r}")
    n_ch, n_f, n_seg = panel.shape
    tau = plane_wave_delays(positions_m, slowness, panel.device)
    if tau.shape[1] != n_ch:
        raise ValueError(f"{tau.shape[1]} positions for {n_ch} records")
    if method == "bartlett":
        return engine.beam_weights(frequency_hz, tau, sensors=n_ch, dtype=panel.real.dtype), None
    csd = engine.cross_spectra(panel, weight=np.full(n_f, 1.0 / n_seg))
    whitener, info = engine.csd_whiten(csd, loading=loading, info=True)
    return engine.beam_weights(frequency_hz, tau, whitener=whitener), info


def beam_stft_pow2(
    sig_wf,
    frequency_sample_rate_hz: float,
    positions_m,
    slowness,
    segment_points: int,
    overlap_points: int = None,
    nfft_points: int = None,
    alpha: float = 0.25,
    method: str = "bartlett",
    loading: float = 1e-2,
):
    """Beam panels of the records of one array [C x n]: styx_fft.stft_complex_pow2's panel of every record, mixed per bin with
    the weights of each slowness vector [K, 2] (engine.beam_steer): beams[k] is the STFT of the signal that travels with
    slowness[k].  method "bartlett": delay-and-sum, weights e / C with e_i = exp(2 pi i f tau_i), tau = plane_wave_delays.
    method "capon": the minimum-variance distortionless-response (MVDR) weights R^-1 e / (e^H R^-1 e) of the panel's own
    cross-spectral matrices (their mean over the segments), loaded on the diagonal with `loading` times the mean auto-power
    (engine.csd_whiten): unit gain towards slowness[k], the least power from everywhere else.  With fewer segments than a
    few times the sensors MVDR also cancels part of the wanted signal; raise `loading` towards Bartlett.  The delay is applied
    as a phase per bin of each segment -- a circular shift inside the windowed segment -- so the delays across the array must
    be short against the segment.  Neither the panel, the matrices nor the weights leave the device.
    :return: frequency_hz [nf], time_s [segments], beams [K x nf x segments] complex, info: None (bartlett) or [nf] int32
        (capon: 0, or the 1-based pivot at which the bin's factorisation failed; such a bin's beams are NaN)"""
    sig, was_numpy, _ = engine.as_signal(sig_wf)
    f, t, panel = styx_fft.stft_complex_pow2(sig, frequency_sample_rate_hz, segment_points, overlap_points, nfft_points, alpha)
    weights, info = _panel_weights(panel, f, positions_m, slowness, method, loading)
    beams = engine.beam_steer(panel, weights)
    return f, t, engine.finish(beams, was_numpy, False), (None if info is None else engine.finish(info, was_numpy, False))


def beam_traces_tukey(
    sig_wf,
    sample_rate_hz: float,
    positions_m,
    slowness,
    segment_length: int,
    overlap_length: int,
    tukey_alpha: float = 0.25,
    method: str = "bartlett",
    loading: float = 1e-2,
):
    """Beam waveforms of the records of one array [C x n], one real trace per slowness vector [K, 2]: frequency-domain
    delay-and-sum through the invertible transform of utilities.short_time_fft.  The complex ShortTimeFFT-convention panel of
    every record (symmetric Tukey window, zero padding, no detrend), the weights of beam_stft_pow2 (method "bartlett" or
    "capon" with `loading`), engine.beam_steer, and istft_tukey's inverse of every beam panel.  The delay is a phase ramp per
    segment: a circular shift inside each windowed segment, not a shift of the record, so the delays across the array must be
    short against the segment (a plane wave across 60 m at 800 Hz, delays of up to 53 samples: 5 % relative RMS error at
    segments of 1024 with overlap 768 -- the records' own noise floor is 4.5 % --, 16 % at 256 / 128).  With few segments
    Capon cancels part of the signal (13 % in the same case at loading 0.1, 19 segments).  Zero delays give the mean of the
    records.  Nothing but the traces and info leaves the device.  For delays that are not short against a segment -- an
    array of 1 km has hundreds of samples -- beam_traces_delay shifts the records themselves: any delay length, no segment.
    :return: timestamps [samples] (istft_tukey's: up to the last window index), traces [K x samples] real, info: None
        (bartlett) or [bins] int32 as beam_stft_pow2 returns it"""
    sig, was_numpy, _ = engine.as_signal(sig_wf)
    obj = short_time_fft.get_stft_object_tukey(sample_rate_hz, tukey_alpha, segment_length, overlap_length, "magnitude")
    panel = short_time_fft._forward(obj, sig, "zeros", False, 0)
    weights, info = _panel_weights(panel, obj.f, positions_m, slowness, method, loading)
    beams = engine.beam_steer(panel, weights)
    timestamps, traces = short_time_fft.istft_tukey(beams, sample_rate_hz, tukey_alpha, segment_length, overlap_length, "magnitude")
    return timestamps, engine.finish(traces, was_numpy, False), (None if info is None else engine.finish(info, was_numpy, False))


def _quantized_plane_waves(sig, sample_rate_hz, positions_m, slowness, phases, taps, beta):
    """The tables of fisher_timeline and beam_traces_delay: the plane-wave delays of every slowness vector for the records
    `sig` [C, n] on the device, quantised to 1 / phases of a sample, and the interpolator bank in the records' precision."""
    tau = plane_wave_delays(positions_m, slowness, sig.device)
    if tau.shape[1] != sig.shape[0]:
        raise ValueError(f"{tau.shape[1]} positions for {sig.shape[0]} records")
    shift, phase, reach = engine.quantize_delays(tau, sample_rate_hz, phases, device=sig.device)
    return shift, phase, engine.delay_bank(phases, taps, beta, sig.dtype), reach


def fisher_timeline(
    sig_wf,
    frequency_sample_rate_hz: float,
    positions_m,
    slowness,
    window_points: int,
    hop_points: int = None,
    phases: int = 64,
    taps: int = 8,
    beta: float = 5.0,
    band_hz=None,
):
    """The time-domain F detector of the records of one array [C x n]: per sliding window of window_points samples
    (hop_points apart, window_points // 2 by default) and slowness vector [G, 2] the records are delayed by
    plane_wave_delays -- whole samples plus 1 / phases of a sample through a Kaiser-windowed sinc bank of `taps` taps
    (engine.delay_bank, engine.quantize_delays) --, summed, and the beam's power is held against the total:
    semblance = sum_t (sum_i y_i)^2 / (C sum_t sum_i y_i^2) (engine.time_beam_power).  No cross-spectral matrix and no Welch
    panel stand between the records and the value: a window may be as short as one sample, a delay as long as the record,
    and nothing assumes a narrow band.  band_hz: (low, high) passes the records through the zero-phase Butterworth band-pass
    of utilities.picker.apply_bandpass on the device first (they become float64).  fisher is the F ratio of the best
    slowness, fisher_from_semblance(peak_value, C); back_azimuth_and_velocity(slowness[peak_index]) completes the detection
    timeline.  Content near Nyquist is attenuated by the interpolator (see beam_traces_delay).
    :return: time_s [nwin] (window centres, host float64), semblance [nwin x G], peak_index [nwin] int64, peak_value [nwin],
        fisher [nwin].  NumPy in -> NumPy out, CUDA tensor in -> CUDA tensor out."""
    sig, was_numpy, _ = engine.as_signal(sig_wf)
    if band_hz is not None:
        from .utilities import picker

        sig = picker.apply_bandpass(sig, (float(band_hz[0]), float(band_hz[1])), frequency_sample_rate_hz)
    win = int(window_points)
    hop = max(win // 2, 1) if hop_points is None else int(hop_points)
    shift, phase, bank, reach = _quantized_plane_waves(sig, frequency_sample_rate_hz, positions_m, slowness, phases, taps, beta)
    semblance, index, value = engine.time_beam_power(sig, shift, phase, bank, win, hop, reach, normalize=True, peaks=True)
    time_s = (np.arange(semblance.shape[0], dtype=np.float64) * hop + 0.5 * (win - 1)) / float(frequency_sample_rate_hz)
    fisher = fisher_from_semblance(value, sig.shape[0])
    return (time_s, engine.finish(semblance, was_numpy, False), engine.finish(index, was_numpy, False),
            engine.finish(value, was_numpy, False), engine.finish(fisher, was_numpy, False))


def beam_traces_delay(sig_wf, sample_rate_hz: float, positions_m, slowness, phases: int = 64, taps: int = 8, beta: float = 5.0):
    """Beam waveforms of the records of one array [C x n], one real trace per slowness vector [K, 2]: delay-and-sum in the
    time domain (engine.time_beam_traces).  Record i is read at t + tau_i, tau = plane_wave_delays -- a shift of the record
    itself by whole samples, zeros beyond its ends, plus 1 / phases of a sample through a Kaiser-windowed sinc bank of `taps`
    taps (engine.delay_bank) -- and the mean over the sensors is the trace.  Where it beats beam_traces_tukey: any delay
    length and no segment -- nothing is circular, so an aperture of hundreds of samples costs no more than one of three, and
    the plane-wave case of that docstring (delays of up to 53 samples) comes out at the records' own noise floor (4.5 %) once
    its content lies below half of Nyquist.  Where it does not: the interpolator is short, and content near Nyquist is
    attenuated and slightly dispersed -- on full-band white records the same trace is 15.8 % from the source with 8 taps
    and 12.0 % with 16, against 5 % for beam_traces_tukey at segments of 1024; band-limit first, or raise `taps`.  Only
    delay-and-sum: MVDR weights stay with beam_traces_tukey.  Zero delays give the mean of the records.
    :return: traces [K x n] real.  NumPy in -> NumPy out, CUDA tensor in -> CUDA tensor out."""
    sig, was_numpy, _ = engine.as_signal(sig_wf)
    shift, phase, bank, reach = _quantized_plane_waves(sig, sample_rate_hz, positions_m, slowness, phases, taps, beta)
    return engine.finish(engine.time_beam_traces(sig, shift, phase, bank, reach), was_numpy, False)
