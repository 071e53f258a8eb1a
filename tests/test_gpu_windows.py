"""Cross-spectra per sliding window on the device (-m gpu): the contract of include/qi_windows.h.  Every shape of
tests/window_cases.py in both precisions: engine.cross_spectra_windows against the stack of engine.cross_spectra on the
contiguous slices, bit for bit (the one test that carries the contract); data planted past the windows' ends; NaN locality;
independence of position, hop, panel length and bin range; exact integer panels; mirror, diagonal and one-segment windows;
styx_fft.csd_windows_pow2 / coherence_windows_pow2 against csd_matrix_pow2 and the float64 restatement of the Welch segments;
beamform.fk_timeline_pow2 on the two-source case for all three methods."""
import functools

import numpy as np
import pytest
import torch

import beam_cases as bc
import csd_cases as cc
import window_cases as wc

from quantum_inferno_amd import beamform, engine, styx_fft

pytestmark = pytest.mark.gpu

DTYPES = wc.DTYPES
COH_TOL = {"float32": cc.COH32_TOL, "float64": 4e-8}  # tests/test_gpu_csd.py's coherence bounds


def ctype(dtype):
    return np.complex64 if dtype == "float32" else np.complex128


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


def device_panel(z, dtype):
    return torch.from_numpy(np.ascontiguousarray(z).astype(ctype(dtype))).cuda()


def run(panel, shape, weight="own", **kw):
    """engine.cross_spectra_windows of a device panel at the shape's windows and bins -> (csd, coherence) NumPy arrays."""
    w = wc.weights(shape) if isinstance(weight, str) else weight
    csd, coh = engine.cross_spectra_windows(panel, shape.win, kw.get("hop", shape.hop), weight=w, bins=kw.get("bins", shape.bins),
                                            coherence=True)
    return csd.cpu().numpy(), coh.cpu().numpy()


@functools.lru_cache(maxsize=None)
def windowed(cid, dtype):
    """(csd, coherence) [nwin, count, C, C] of a shape case on its random panel: computed once, shared, left unchanged."""
    shape = wc.by_id(cid)
    csd, coh = run(device_panel(wc.panel(shape), dtype), shape)
    assert csd.shape == coh.shape == (shape.nwin, shape.bins[1], shape.C, shape.C)
    assert csd.dtype == ctype(dtype) and coh.dtype == np.dtype(dtype)
    csd.setflags(write=False)
    coh.setflags(write=False)
    return csd, coh


# ---- the contract: the slice call's bits ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_bit_equal_to_cross_spectra_of_the_slices(dtype):
    """The panels are random in every segment: data past a window's end, before its start and in other bins is there to leak."""
    for shape in wc.SHAPES:
        panel = device_panel(wc.panel(shape), dtype)
        first, count = shape.bins
        csd, coh = windowed(shape.id, dtype)
        for w in range(shape.nwin):
            cut = panel[:, first:first + count, w * shape.hop:w * shape.hop + shape.win].contiguous()
            want, want_coh = engine.cross_spectra(cut, weight=wc.weights(shape), coherence=True)
            assert same_bits(csd[w], want.cpu().numpy()), (shape.id, w)
            assert same_bits(coh[w], want_coh.cpu().numpy()), (shape.id, w)
        assert np.isfinite(csd).all() and np.isfinite(coh).all(), shape.id
        ref = wc.restate(wc.panel(shape), first, count, shape.win, shape.hop, wc.weights(shape))
        assert np.abs(csd - ref).max() <= wc.TOL[dtype] * np.abs(ref).max(), shape.id


@pytest.mark.parametrize("dtype", DTYPES)
def test_without_weights_without_bins_and_either_output_alone(dtype):
    from quantum_inferno_amd import _lib

    lib = _lib.require_gpu()
    shape = wc.by_id(next(s.id for s in wc.SHAPES if s.C == 17 and s.win == 17))
    panel = device_panel(wc.panel(shape), dtype)
    csd, coh = engine.cross_spectra_windows(panel, shape.win, shape.hop, coherence=True)
    assert csd.shape == (shape.nwin, shape.nf, 17, 17) and torch.equal(engine.cross_spectra_windows(panel, shape.win, shape.hop), csd)
    for w in range(shape.nwin):
        cut = panel[:, :, w * shape.hop:w * shape.hop + shape.win].contiguous()
        assert torch.equal(csd[w], engine.cross_spectra(cut))
    # the default hop is half a window
    half = engine.cross_spectra_windows(panel, shape.win)
    assert half.shape[0] == (shape.nseg - shape.win) // (shape.win // 2) + 1
    # NumPy in -> NumPy out
    host = engine.cross_spectra_windows(panel.cpu().numpy(), shape.win, shape.hop)
    assert isinstance(host, np.ndarray) and same_bits(host, csd.cpu().numpy())
    # the coherence alone goes through the scratch matrices
    code = _lib.dtype_code(coh.dtype)
    alone = torch.full_like(coh, 0.3125)
    scratch, nbytes = _lib.scratch(lib.qi_cross_spectra_windows_scratch_bytes, panel.device, code, 17, shape.nf, shape.nseg, 0, shape.nf,
                                   shape.win, shape.hop)
    _lib.call(lib.qi_cross_spectra_windows, panel.device, code, panel.device.index, _lib.ptr(panel), 17, shape.nf, shape.nseg, 0, shape.nf,
              shape.win, shape.hop, None, None, _lib.ptr(alone), _lib.ptr(scratch), nbytes)
    assert torch.equal(alone, coh)
    for bad in (dict(window_segments=shape.nseg + 1), dict(window_segments=0), dict(window_segments=3, hop_segments=0),
                dict(window_segments=3, bins=(0, shape.nf + 1)), dict(window_segments=3, bins=(-1, 1))):
        with pytest.raises(_lib.QiError):
            engine.cross_spectra_windows(panel, **bad)
    with pytest.raises(ValueError):
        engine.cross_spectra_windows(panel, 3, weight=np.ones(shape.nf + 1))


# ---- the window's end ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_what_lies_outside_the_windows_is_never_read_into_a_sum(dtype):
    """Every segment that no window covers set to NaN; and the segment just past each window's end, where it belongs to no
    other window, scaled by 1e30: the results keep their bits and stay finite."""
    planted = 0
    for shape in wc.SHAPES:
        z = wc.panel(shape)
        cov = wc.covered(shape.nseg, shape.win, shape.hop)
        want = windowed(shape.id, dtype)
        if not cov.all():
            nan = z.copy()
            nan[:, :, ~cov] = np.nan + 1j * np.nan
            got = run(device_panel(nan, dtype), shape)
            assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]), shape.id
            planted += 1
        ends = [w * shape.hop + shape.win for w in range(shape.nwin)]
        free = [e for e in ends if e < shape.nseg and not cov[e]]
        if free:
            big = z.copy()
            big[:, :, free] *= 1e30
            got = run(device_panel(big, dtype), shape)
            assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]), shape.id
            assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all(), shape.id
    assert planted >= 10


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_nan_stays_in_its_windows_records_and_bin(dtype):
    for shape in wc.SHAPES:
        first, count = shape.bins
        r, f, s = shape.C - 1, count // 2, min(shape.hop, shape.nseg - 1)
        assert wc.covered(shape.nseg, shape.win, shape.hop)[s] or shape.hop > shape.win
        z = wc.panel(shape)
        z[r, first + f, s] = np.nan
        if first > 0:
            z[0, first - 1, :] = np.nan  # a bin that is not formed
        csd, coh = run(device_panel(z, dtype), shape)
        want = np.zeros(csd.shape, dtype=bool)
        for w in range(shape.nwin):
            if w * shape.hop <= s < w * shape.hop + shape.win:
                want[w, f, r, :] = want[w, f, :, r] = True
        assert np.array_equal(np.isnan(csd.real) | np.isnan(csd.imag), want), shape.id
        assert np.array_equal(np.isnan(coh), want), shape.id
        clean = windowed(shape.id, dtype)
        assert np.array_equal(bits(csd[~want]), bits(clean[0][~want])) and np.array_equal(bits(coh[~want]), bits(clean[1][~want])), shape.id


# ---- position and table independence ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_window_has_the_same_bits_wherever_it_lies(dtype):
    """A panel periodic in time with period hop: all windows are equal.  And on the random panel the same window comes out
    the same under twice the hop, a shorter panel and all bins."""
    for shape in wc.SHAPES:
        z = wc.panel(shape)
        periodic = z[:, :, np.arange(shape.nseg) % shape.hop] if shape.hop < shape.nseg else z
        csd, coh = run(device_panel(periodic, dtype), shape)
        for w in range(1, shape.nwin):
            assert same_bits(csd[w], csd[0]) and same_bits(coh[w], coh[0]), (shape.id, w)
        base = windowed(shape.id, dtype)
        first, count = shape.bins
        # twice the hop, the segments after the last window cut off, every bin formed with its own weight
        last = (shape.nwin - 1) // 2
        nseg = 2 * last * shape.hop + shape.win
        weight = np.linspace(2.1, 3.3, shape.nf)
        weight[first:first + count] = wc.weights(shape)
        other = run(device_panel(z[:, :, :nseg], dtype), shape, weight=weight, hop=2 * shape.hop, bins=(0, shape.nf))
        assert other[0].shape == (last + 1, shape.nf, shape.C, shape.C)
        for k in (0, 1):
            assert same_bits(other[k][:, first:first + count], base[k][0:2 * last + 1:2]), (shape.id, k)


# ---- exact integer panels ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", (False, True), ids=("unit", "weighted"))
@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_integer_panels(dtype, weighted):
    """A row / column swap, the conjugation sign, a window that starts or ends one segment off and the mirror all show as a
    wrong integer."""
    nf, nseg = 3, 61
    for C in (2, 5, 17, 64):
        z = wc.integer_panel(C, nf, nseg)
        panel = device_panel(z, dtype)
        for win, hop in ((1, 20), (7, 9), (16, 15), (33, 7), (40, 21)):
            weight = 0.25 * (1 + np.arange(2)) if weighted else None  # (exact in float32, and so is every product with it)
            csd = engine.cross_spectra_windows(panel, win, hop, weight=weight, bins=(1, 2)).cpu().numpy()
            want = wc.restate(z, 1, 2, win, hop, weight)
            assert np.abs(want.real).max() < 2 ** 24 and np.array_equal(want, np.rint(want.real * 4) / 4 + 1j * np.rint(want.imag * 4) / 4)
            assert np.array_equal(csd, want.astype(ctype(dtype))), (C, win, hop, np.argwhere(csd != want)[:4])


# ---- mirror, diagonal, one segment ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_mirror_diagonal_and_one_segment_windows(dtype):
    ones = 0
    for shape in wc.SHAPES:
        csd, coh = windowed(shape.id, dtype)
        i, j = np.triu_indices(shape.C, 1)
        assert same_bits(csd[:, :, j, i], np.conj(csd[:, :, i, j])), shape.id
        assert same_bits(coh, np.swapaxes(coh, 2, 3)), shape.id
        diag = csd[:, :, np.arange(shape.C), np.arange(shape.C)]
        assert np.array_equal(bits(diag.imag), bits(np.zeros_like(diag.imag))) and np.all(diag.real > 0), shape.id  # +0, bit for bit
        if shape.win == 1:
            assert np.all(coh == 1), shape.id
            ones += 1
        elif shape.C > 1:
            assert np.any(coh != 1), shape.id
    assert ones >= 3


# ---- csd_windows_pow2 and coherence_windows_pow2 --------------------------------------------------------------------------------------
PATH_CASES = ("c5_n4096_seg256", "c3_n1000_seg100_nfft128")  # the fused and the hipFFT path
PATH_WINDOWS = {"c5_n4096_seg256": (16, 4), "c3_n1000_seg100_nfft128": (9, 4)}  # (segments, hop) of 31 and of 19 segments


def args(case):
    return dict(segment_points=case.seg, nfft_points=case.nfft, overlap_points=case.overlap, alpha=cc.ALPHA)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cid", PATH_CASES)
def test_one_window_over_every_segment_is_csd_matrix_pow2(cid, dtype):
    case = cc.by_id(cid)
    assert case.path == ("fused" if cid == PATH_CASES[0] else "hipfft")
    x = cc.records(case).astype(dtype)
    nseg = cc.segments(case)
    for scaling in cc.SCALINGS:
        f, want = styx_fft.csd_matrix_pow2(x, cc.FS, scaling=scaling, **args(case))
        f_w, t, got = styx_fft.csd_windows_pow2(x, cc.FS, window_segments=nseg, scaling=scaling, **args(case))
        assert np.array_equal(f_w, f) and got.shape == (1,) + want.shape and same_bits(got[0], want), scaling
        assert t.tolist() == [((nseg - 1) * cc.hop(case) + case.seg) / 2 / cc.FS]
    _, want = styx_fft.coherence_matrix_pow2(x, cc.FS, **args(case))
    _, _, got = styx_fft.coherence_windows_pow2(x, cc.FS, window_segments=nseg, window_hop_segments=3, **args(case))
    assert same_bits(got[0], want)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cid", PATH_CASES)
def test_windows_of_welch_segments_against_the_restatement(cid, dtype):
    case = cc.by_id(cid)
    x = cc.records(case)
    win, hop = PATH_WINDOWS[cid]
    nseg, nf = cc.segments(case), case.nfft // 2 + 1
    nwin = wc.windows(nseg, win, hop)
    assert nwin >= 3 and (nseg - win) % hop > 0
    z = cc.panel(x.astype(np.float64), case)
    f_all = np.fft.rfftfreq(case.nfft, 1 / cc.FS)
    for scaling in cc.SCALINGS:
        for rng_hz, (first, count) in ((None, (0, nf)), ((f_all[3], f_all[nf - 2]), (3, nf - 5)), ((f_all[nf - 4] - 1.0, cc.FS), (nf - 4, 4))):
            f, t, got = styx_fft.csd_windows_pow2(x.astype(dtype), cc.FS, window_segments=win, window_hop_segments=hop, scaling=scaling,
                                                  frequency_range_hz=rng_hz, **args(case))
            assert np.array_equal(f, f_all[first:first + count]) and got.shape == (nwin, count, case.C, case.C) and got.dtype == ctype(dtype)
            assert np.array_equal(t, (np.arange(nwin) * hop * cc.hop(case) + ((win - 1) * cc.hop(case) + case.seg) / 2) / cc.FS)
            weight = cc.bin_weights(case.nfft, win, cc.scale2(cc.window_of(case), scaling))[first:first + count]
            ref = wc.restate(z, first, count, win, hop, weight)
            err = float(np.abs(got - ref).max() / np.abs(ref).max())
            print(f"{cid} {dtype} {scaling} bins {first}+{count}: max |dS| / max |S| = {err:.3g} (bound {wc.TOL[dtype]:g})")
            assert err <= wc.TOL[dtype], (scaling, first, err)
    f, t, coh = styx_fft.coherence_windows_pow2(x.astype(dtype), cc.FS, window_segments=win, window_hop_segments=hop, **args(case))
    ref = wc.restate(z, 0, nf, win, hop)
    floor = min(cc.auto_power_floor(r) for r in ref)
    want = np.stack([cc.coherence_of(r) for r in ref])
    err = float(np.nanmax(np.abs(coh - want)))
    print(f"{cid} {dtype}: windowed coherence against the restatement: {err:.3g} (bound {COH_TOL[dtype]:g}); smallest auto-power over "
          f"its record's largest {floor:.3g}")
    assert coh.shape == (nwin, nf, case.C, case.C) and coh.dtype == np.dtype(dtype) and np.isfinite(coh).all()
    assert err <= COH_TOL[dtype], err
    with pytest.raises(ValueError):
        styx_fft.csd_windows_pow2(x, cc.FS, window_segments=win, frequency_range_hz=(10.0, 10.5), **args(case))
    with pytest.raises(ValueError):
        styx_fft.csd_windows_pow2(x, cc.FS, window_segments=nseg + 1, **args(case))


# ---- the timeline -----------------------------------------------------------------------------------------------------------------------
def timeline(method, dtype, **kw):
    extra = dict(bartlett={}, capon=dict(loading=wc.TL_CAPON_LOADING), music=dict(n_sources=1))[method]
    x = torch.from_numpy(wc.timeline_records().astype(dtype)).cuda()
    return beamform.fk_timeline_pow2(x, bc.PW_FS, bc.PW_POSITIONS_M, bc.pw_slowness(), wc.TL_SEG, wc.TL_WIN, wc.TL_HOP,
                                     overlap_points=wc.TL_OVERLAP, band_edges_hz=wc.timeline_edges_hz(), method=method, **extra, **kw)


def form(method, stack, freq, tau, bands):
    if method == "bartlett":
        return engine.beam_power(stack, freq, tau, bands=bands, normalize=True, peaks=True) + (None,)
    if method == "capon":
        whitener, info = engine.csd_whiten(stack, loading=wc.TL_CAPON_LOADING, info=True)
        return engine.capon_power(whitener, freq, tau, bands=bands, peaks=True) + (info,)
    _, vectors, info = engine.csd_eigh(stack, info=True)
    return engine.music_power(vectors, 1, freq, tau, bands=bands, peaks=True) + (info,)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("method", beamform.TIMELINE_METHODS)
def test_timeline_of_two_sources(method, dtype):
    time_s, ranges, power, index, value, info = timeline(method, dtype)
    ref = wc.timeline_power(method)
    nwin, nb, G = ref.shape
    assert np.array_equal(time_s, wc.timeline_times()) and ranges.tolist() == [[25.0, 71.875], [75.0, 121.875], [125.0, 221.875], [225.0, 225.0]]
    for t in (power, index, value):
        assert isinstance(t, torch.Tensor) and t.is_cuda
    assert power.shape == (nwin, nb, G) and index.shape == value.shape == (nwin, nb) and index.dtype == torch.int64
    assert power.dtype == value.dtype == (torch.float32 if dtype == "float32" else torch.float64)
    if method == "bartlett":
        assert info is None
    else:
        assert info.shape == (nwin, 65) and info.dtype == torch.int32 and not info.any()
    got = power.cpu().numpy()
    err = float(np.abs(got - ref).max() / np.abs(ref).max())
    print(f"timeline {method} {dtype}: max |d power| / max power = {err:.3g} (bound {wc.TOL[dtype]:g})")
    assert err <= wc.TOL[dtype], err
    idx = index.cpu().numpy()
    assert (idx[list(wc.TL_FIRST)] == wc.TL_POINTS[0]).all() and (idx[list(wc.TL_SECOND)] == wc.TL_POINTS[1]).all()
    assert np.array_equal(idx, np.argmax(got, axis=2)) and np.array_equal(value.cpu().numpy(), got.max(axis=2))
    # window w alone: the form on its own matrices, with the band table of one window
    x = torch.from_numpy(wc.timeline_records().astype(dtype)).cuda()
    f, _, csd = styx_fft.csd_windows_pow2(x, bc.PW_FS, wc.TL_SEG, wc.TL_WIN, wc.TL_HOP, overlap_points=wc.TL_OVERLAP,
                                          frequency_range_hz=(25.0, 226.0))
    s_ref, f_ref, bands = wc.timeline_matrices()
    assert np.array_equal(f, f_ref) and csd.shape == s_ref.shape
    tau = beamform.plane_wave_delays(bc.PW_POSITIONS_M, bc.pw_slowness(), x.device)
    for w in (0, 5, 7, 13):
        p, i, v, flags = form(method, csd[w], f, tau, bands)
        assert torch.equal(p, power[w]) and torch.equal(i, index[w]) and torch.equal(v, value[w]), w
        assert flags is None or torch.equal(flags, info[w])
    # the timeline's columns
    az, vel = beamform.back_azimuth_and_velocity(beamform._host64(bc.pw_slowness(), 2, "slowness")[index.cpu()])
    for rows, point in ((wc.TL_FIRST, wc.TL_POINTS[0]), (wc.TL_SECOND, wc.TL_POINTS[1])):
        sx, sy = bc.pw_slowness()[point]
        assert np.allclose(az[list(rows)].numpy(), np.degrees(np.arctan2(-sx, -sy)) % 360.0, rtol=0, atol=1e-9)
        assert np.allclose(vel[list(rows)].numpy(), 1.0 / np.hypot(sx, sy), rtol=1e-12)
    if method == "bartlett":
        fisher = beamform.fisher_from_semblance(value, 5)
        assert torch.equal(fisher, 4 * value / (1 - value)) and bool((fisher[list(wc.TL_FIRST)] > 1).all())


def test_timeline_arguments():
    x = wc.timeline_records()[:, :2048].astype(np.float32)
    base = dict(overlap_points=wc.TL_OVERLAP, band_edges_hz=wc.timeline_edges_hz())
    for bad in (dict(method="fisher"), dict(method="capon", normalize=False), dict(method="music", normalize=False)):
        with pytest.raises(ValueError):
            beamform.fk_timeline_pow2(x, bc.PW_FS, bc.PW_POSITIONS_M, bc.pw_slowness(), wc.TL_SEG, 4, **{**base, **bad})
    with pytest.raises(ValueError):
        beamform.fk_timeline_pow2(x, bc.PW_FS, bc.PW_POSITIONS_M[:4], bc.pw_slowness(), wc.TL_SEG, 4, **base)
    # NumPy in -> NumPy out; no bands: every bin its own; the power instead of the semblance
    t, ranges, power, index, value, info = beamform.fk_timeline_pow2(x, bc.PW_FS, bc.PW_POSITIONS_M, bc.pw_slowness(), wc.TL_SEG, 4,
                                                                     overlap_points=wc.TL_OVERLAP, normalize=False)
    nwin = (15 - 4) // 2 + 1
    assert all(isinstance(a, np.ndarray) for a in (t, ranges, power, index, value)) and info is None
    assert power.shape == (nwin, 129, 81) and index.shape == (nwin, 129) and ranges.shape == (129, 2) and len(t) == nwin
    f, _, csd = styx_fft.csd_windows_pow2(x, bc.PW_FS, wc.TL_SEG, 4, overlap_points=wc.TL_OVERLAP)
    want = engine.beam_power(csd[2], f, bc.pw_delays(), normalize=False)
    assert same_bits(power[2], want)
