"""Windowed cross-spectra without a GPU: the exports of include/qi_windows.h and the census of tests/window_stream_cases.py
against that header, the refusals of qi_cross_spectra_windows and qi_csd_windows and the size queries' verdicts, the shape
table's coverage, the NumPy restatement of tests/window_cases.py against its identities, fisher_from_semblance, and the
two-source timeline case restated in float64 for all three methods."""
import ctypes
import os

import numpy as np

import window_cases as wc
import window_stream_cases as wsc
from stream_table import header_functions, stream_functions

ROOT = wc.ROOT
HEADER = "qi_windows.h"
OTHER_HEADERS = ("qi_tfr.h", "qi_array.h", "qi_beam.h", "qi_adaptive.h", "qi_subspace.h", "qi_steer.h")
NAMES = {"qi_cross_spectra_windows_scratch_bytes", "qi_cross_spectra_windows", "qi_csd_windows_scratch_bytes", "qi_csd_windows"}
IDENTITY_TOL = 1e-12


# ---- the header, the exports, the stream census ---------------------------------------------------------------------------------------
def test_library_exports_the_windows_header():
    from quantum_inferno_amd import _lib

    declared = set(header_functions(HEADER))
    assert declared == NAMES
    assert declared == set(_lib.WINDOW_PROTOTYPES)
    for table in (_lib.PROTOTYPES, _lib.ARRAY_PROTOTYPES, _lib.BEAM_PROTOTYPES, _lib.ADAPTIVE_PROTOTYPES, _lib.SUBSPACE_PROTOTYPES,
                  _lib.STEER_PROTOTYPES):
        assert not declared & set(table)
    for other in OTHER_HEADERS:
        assert not declared & set(header_functions(other)), other
    lib = _lib.load()
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in include/qi_windows.h but not exported"
        assert len(_lib.WINDOW_PROTOTYPES[name][1]) == len(header_functions(HEADER)[name].split(",")), name
    with open(os.path.join(ROOT, "include", "qi_windows.h")) as fh:
        text = fh.read()
    assert '#include "qi_tfr.h"' in text and '#include "qi_array.h"' in text and "BIT FOR BIT" in text


def test_every_stream_entry_point_has_a_case_and_nothing_else_is_named():
    assert wsc.TABLE.header == HEADER
    assert stream_functions(HEADER) == ["qi_cross_spectra_windows", "qi_csd_windows"]
    assert wsc.TABLE.named_functions() == stream_functions(HEADER)


def test_stream_case_table():
    assert wsc.TABLE.ids() == ["cross_spectra_windows-matrices", "cross_spectra_windows-coherence", "csd_windows-fused-matrices",
                               "csd_windows-fused-coherence", "csd_windows-hipfft-matrices", "csd_windows-hipfft-coherence"]
    for case in wsc.TABLE.cases:
        assert case.functions and callable(case.build) and case.asynchronous and case.engine is None, case.id
    assert wsc.TABLE.by_id("cross_spectra_windows-coherence").build.args == (True,)
    assert wsc.TABLE.by_id("csd_windows-hipfft-matrices").build.args == ("hipfft", False)
    assert (wsc.COLUMNS - wsc.WINDOW) // wsc.HOP + 1 == 16 and (wsc.COLUMNS - wsc.WINDOW) % wsc.HOP > 0


def test_shape_cases_cover_every_edge():
    s = wc.SHAPES
    assert {x.C for x in s} == set(wc.RECORD_COUNTS) == {1, 2, 5, 16, 17, 33, 64}
    assert {x.win for x in s} == set(wc.WINS) == {1, 3, 7, 8, 9, 16, 17, 31, 32, 33, 40}
    for C in (5, 17, 64):
        assert {x.win for x in s if x.C == C} == set(wc.WINS), C
    assert {x.nf for x in s} == {1, 5, 9}
    hops = set()
    for x in s:
        hops |= {k for k, h in (("1", 1), ("3", 3), ("win", x.win), ("win+3", x.win + 3)) if x.hop == h}
        assert wc.windows(x.nseg, x.win, x.hop) == x.nwin >= 2 and x.nseg == (x.nwin - 1) * x.hop + x.win + x.rest, x.id
        assert 0 <= x.rest < x.hop and 0 <= x.bins[0] and x.bins[1] >= 1 and x.bins[0] + x.bins[1] <= x.nf, x.id
    assert hops == set(wc.HOPS)
    assert any(x.rest == 0 for x in s) and any(x.rest == x.hop - 1 > 0 for x in s)
    assert any(x.hop > x.win and not wc.covered(x.nseg, x.win, x.hop).all() for x in s)  # gaps that no window holds
    assert {wc.range_kind(x) for x in s} == set(wc.RANGES)
    assert len(set(wc.ids())) == len(s) <= 40


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
GOOD = dict(dtype=None, C=2, nf=4, nseg=10, first=1, count=2, win=4, hop=3)
SHAPE_REFUSALS = (
    (dict(dtype=7), "dtype"), (dict(C=0), "panel shape"), (dict(nf=0), "panel shape"), (dict(nseg=0), "panel shape"),
    (dict(win=0), "window"), (dict(hop=0), "window"), (dict(win=11), "longer"), (dict(count=0), "bin range"),
    (dict(first=-1), "bin range"), (dict(first=3, count=2), "bin range"), (dict(first=4, count=1), "bin range"),
    (dict(C=64, nf=1 << 20, first=0, count=1 << 20, nseg=1 << 12, win=1, hop=1), "too large"),  # 2^44 entries
    (dict(C=64, nf=4, first=0, count=4, nseg=1 << 30, win=1, hop=1), "too large"),  # 2^44 entries, by the windows
    (dict(C=1 << 20), "too large"),
    (dict(C=1, nf=1 << 33, first=0, count=1 << 33, nseg=1, win=1, hop=1), "too large"),  # the grid passes 2^31
    (dict(C=1, nf=1 << 31, first=0, count=4, nseg=1 << 30, win=1, hop=1), "too large"),  # the panel's index arithmetic
)


def _windows_args(a):
    return (a["dtype"], a["C"], a["nf"], a["nseg"], a["first"], a["count"], a["win"], a["hop"])


def test_cross_spectra_windows_refusals_without_a_gpu():
    """Refused before the device is touched: the pointers are never followed (this machine may have no GPU at all)."""
    from quantum_inferno_amd import _lib

    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    odd = ctypes.c_void_p(ctypes.addressof(buf) + 4)
    good = {**GOOD, "dtype": _lib.QI_F32}

    def call(a, z=p, weight=None, csd=p, coh=p, scratch=p, nbytes=1 << 20):
        d, *rest = _windows_args(a)
        return lib.qi_cross_spectra_windows(d, 0, z, *rest, weight, csd, coh, scratch, nbytes, None)

    for change, what in SHAPE_REFUSALS:
        assert call({**good, **change}) < 0, change
        assert what in lib.qi_last_error().decode(), (change, lib.qi_last_error())
    for kw in (dict(z=None), dict(scratch=None)):
        assert call(good, **kw) < 0 and b"null" in lib.qi_last_error(), kw
    assert call(good, csd=None, coh=None) < 0 and b"nothing" in lib.qi_last_error()
    for kw in (dict(z=odd), dict(csd=odd), dict(coh=ctypes.c_void_p(ctypes.addressof(buf) + 2)),
               dict(scratch=ctypes.c_void_p(ctypes.addressof(buf) + 8))):
        assert call(good, **kw) < 0 and b"misaligned" in lib.qi_last_error(), kw
    assert call({**good, "dtype": _lib.QI_F64}, csd=ctypes.c_void_p(ctypes.addressof(buf) + 8)) < 0 and b"misaligned" in lib.qi_last_error()
    need = lib.qi_cross_spectra_windows_scratch_bytes(*_windows_args(good))
    assert need >= 2 * 8 + 3 * 2 * 4 * 8  # the weights and three windows' matrices
    assert call(good, nbytes=0) < 0 and b"scratch" in lib.qi_last_error()
    assert call(good, nbytes=need - 1) < 0 and b"scratch" in lib.qi_last_error()


def test_csd_windows_refusals_without_a_gpu():
    from quantum_inferno_amd import _lib

    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    good = dict(dtype=_lib.QI_F32, C=2, n=1024, seg=64, hop=32, nfft=64, first=1, count=8, win=4, win_hop=2)

    def args(a):
        return (a["dtype"], a["C"], a["n"], a["seg"], a["hop"], a["nfft"], a["first"], a["count"], a["win"], a["win_hop"])

    def call(a, sig=p, window=p, csd=p, coh=p, scratch=p, nbytes=1 << 30):
        d, C, n, seg, hop, nfft, first, count, win, win_hop = args(a)
        return lib.qi_csd_windows(d, 0, sig, C, n, window, seg, hop, nfft, 1.0, first, count, win, win_hop, csd, coh, scratch, nbytes, None)

    for change, what in ((dict(dtype=7), "dtype"), (dict(C=0), "Welch"), (dict(n=63), "Welch"), (dict(hop=0), "Welch"), (dict(hop=65), "Welch"),
                         (dict(nfft=32), "Welch"), (dict(win=0), "window"), (dict(win_hop=0), "window"), (dict(win=32), "longer"),
                         (dict(count=0), "bin range"), (dict(first=30, count=4), "bin range"), (dict(first=-1), "bin range")):
        bad = {**good, **change}
        assert call(bad) < 0, change
        msg = lib.qi_last_error()
        assert what in msg.decode(), (change, msg)
        assert lib.qi_csd_windows_scratch_bytes(*args(bad)) == call(bad) and lib.qi_last_error() == msg, change
    for kw in (dict(sig=None), dict(window=None), dict(scratch=None)):
        assert call(good, **kw) < 0 and b"null" in lib.qi_last_error(), kw
    assert call(good, csd=None, coh=None) < 0 and b"nothing" in lib.qi_last_error()
    for kw in (dict(csd=ctypes.c_void_p(ctypes.addressof(buf) + 4)), dict(coh=ctypes.c_void_p(ctypes.addressof(buf) + 2)),
               dict(scratch=ctypes.c_void_p(ctypes.addressof(buf) + 8))):
        assert call(good, **kw) < 0 and b"misaligned" in lib.qi_last_error(), kw
    need = lib.qi_csd_windows_scratch_bytes(*args(good))
    n_seg = (1024 - 64) // 32 + 1
    assert need >= 2 * 33 * n_seg * 8 + ((n_seg - 4) // 2 + 1) * 8 * 4 * 8  # the panel and the matrices
    assert call(good, nbytes=need - 1) < 0 and b"scratch" in lib.qi_last_error()
    # all bins, one window over every segment: the panel part of qi_csd's scratch, and a contraction's part of the same size
    whole = lib.qi_csd_windows_scratch_bytes(_lib.QI_F32, 2, 1024, 64, 32, 64, 0, 33, n_seg, 1)
    assert whole == lib.qi_csd_scratch_bytes(_lib.QI_F32, 2, 1024, 64, 32, 64)


def test_size_query_gives_the_calls_verdicts():
    from quantum_inferno_amd import _lib

    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    for change, _ in SHAPE_REFUSALS:
        a = {**GOOD, "dtype": _lib.QI_F64, **change}
        got = lib.qi_cross_spectra_windows_scratch_bytes(*_windows_args(a))
        msg = lib.qi_last_error()
        assert got < 0 and msg, change
        d, *rest = _windows_args(a)
        rc = lib.qi_cross_spectra_windows(d, 0, p, *rest, None, p, p, p, 1 << 20, None)
        assert rc == got and lib.qi_last_error() == msg, change

    def matrices(dtype, C, nf, nseg, first, count, win, hop):
        """The windows the query counts: its bytes less the weights, over one window's (1 KiB here, above the two regions'
        padding)."""
        one = count * C * C * 2 * (8 if dtype == _lib.QI_F64 else 4)
        got = lib.qi_cross_spectra_windows_scratch_bytes(dtype, C, nf, nseg, first, count, win, hop)
        assert got > 0 and one == 1024 and (got - count * 8) % one < 512
        return (got - count * 8) // one

    for nseg, win, hop, nwin in ((10, 10, 1, 1), (10, 10, 7, 1), (10, 4, 7, 1), (10, 4, 6, 2), (10, 4, 1, 7), (10, 1, 1, 10),
                                 (10, 3, 4, 2), (11, 3, 4, 3), (1, 1, 5, 1)):
        assert matrices(_lib.QI_F64, 4, 4, nseg, 0, 4, win, hop) == nwin, (nseg, win, hop)
        assert wc.windows(nseg, win, hop) == nwin
    # 2^40 entries: the last shape accepted
    assert lib.qi_cross_spectra_windows_scratch_bytes(_lib.QI_F32, 64, 1 << 14, 1 << 14, 0, 1 << 14, 1, 1) > 0
    assert lib.qi_cross_spectra_windows_scratch_bytes(_lib.QI_F32, 64, 1 << 14, (1 << 14) + 1, 0, 1 << 14, 1, 1) < 0


# ---- the restatement against its identities -------------------------------------------------------------------------------------------
def test_restatement_identities():
    worst = 0.0
    for shape in wc.SHAPES:
        z = wc.panel(shape)
        first, count = shape.bins
        w = wc.weights(shape)
        s = wc.restate(z, first, count, shape.win, shape.hop, w)
        assert s.shape == (shape.nwin, count, shape.C, shape.C)
        for k in range(shape.nwin):
            cut = z[:, first:first + count, k * shape.hop:k * shape.hop + shape.win]
            want = np.einsum("ifs,jfs->fij", np.conj(cut), cut) * w[:, None, None]
            assert np.array_equal(s[k], want), (shape.id, k)
        assert np.array_equal(s, np.conj(np.swapaxes(s, 2, 3))) or np.abs(s - np.conj(np.swapaxes(s, 2, 3))).max() <= IDENTITY_TOL * np.abs(s).max()
        if shape.hop == shape.win and shape.rest == 0:
            # abutting windows that use up the panel: their unweighted sum is the whole-record matrix
            whole = np.einsum("ifs,jfs->fij", np.conj(z), z)[first:first + count]
            err = float(np.abs(wc.restate(z, first, count, shape.win, shape.hop).sum(axis=0) - whole).max() / np.abs(whole).max())
            worst = max(worst, err)
            assert err <= IDENTITY_TOL, shape.id
    assert any(x.hop == x.win and x.rest == 0 for x in wc.SHAPES)
    print(f"sum of abutting windows against the whole record, of the largest entry: {worst:.3g}; bound {IDENTITY_TOL:g}")


def test_integer_panel_sums_are_exact_in_float32():
    for C in (5, 17, 64):
        z = wc.integer_panel(C, 5, 60)
        assert np.abs(z.real).max() <= 3 and np.abs(z.imag).max() <= 3
        s = wc.restate(z, 0, 5, 40, 10)
        assert np.array_equal(s, np.rint(s.real) + 1j * np.rint(s.imag)) and max(np.abs(s.real).max(), np.abs(s.imag).max()) < 2 ** 24
        assert not np.array_equal(s, np.swapaxes(s, 2, 3)) and not np.array_equal(s[0], s[1])


def test_fisher_from_semblance():
    import torch

    from quantum_inferno_amd import beamform

    C = 5
    got = beamform.fisher_from_semblance(np.array([0.0, 1 / C, 1.0, np.nan, 0.5]), C)
    assert got[0] == 0.0 and abs(got[1] - 1.0) <= 1e-15 and np.isposinf(got[2]) and np.isnan(got[3]) and got[4] == C - 1
    t = beamform.fisher_from_semblance(torch.tensor([0.0, 1.0, float("nan"), 0.5], dtype=torch.float32), C)
    assert isinstance(t, torch.Tensor) and t.dtype == torch.float32
    assert t[0] == 0 and torch.isposinf(t[1]) and torch.isnan(t[2]) and t[3] == C - 1
    assert beamform.fisher_from_semblance(0.5, 2) == 1.0
    doc = beamform.fisher_from_semblance.__doc__
    assert "F ratio" in doc and "back_azimuth_and_velocity(slowness[peak_index])" in doc


# ---- the timeline case, restated in float64 -------------------------------------------------------------------------------------------
def test_timeline_case_geometry():
    import csd_cases as cc

    case = wc.timeline_case()
    assert wc.timeline_records().shape == (5, 8192) and cc.segments(case) == 63
    assert wc.windows(63, wc.TL_WIN, wc.TL_HOP) == 14 == len(wc.timeline_times())
    hop = wc.TL_SEG - wc.TL_OVERLAP
    for w in range(14):
        lo, hi = w * wc.TL_HOP * hop, (w * wc.TL_HOP + wc.TL_WIN - 1) * hop + wc.TL_SEG  # the samples the window spans
        assert (hi <= wc.TL_HALF) == (w in wc.TL_FIRST) and (lo >= wc.TL_HALF) == (w in wc.TL_SECOND), w
        assert wc.timeline_times()[w] == (lo + hi) / 2 / 800.0
    s, freq, bands = wc.timeline_matrices()
    assert s.shape == (14, 65, 5, 5) and bands.tolist() == [0, 16, 32, 64, 65] and freq[0] == 25.0 and freq[-1] == 225.0


def test_timeline_peaks_follow_the_source():
    """Windows 0-5 peak at grid point 25 and windows 8-13 at grid point 55, in all four bands and for all three methods; the
    smallest peak over its runner-up is 1.06 (the semblance, band 3), far above any float32 deviation."""
    smallest = {}
    for method in ("bartlett", "capon", "music"):
        p = wc.timeline_power(method)
        assert p.shape == (14, 4, 81) and np.isfinite(p).all()
        idx, ratio = wc.peak_ratios(p)
        assert (idx[list(wc.TL_FIRST)] == wc.TL_POINTS[0]).all() and (idx[list(wc.TL_SECOND)] == wc.TL_POINTS[1]).all(), method
        asserted = ratio[list(wc.TL_FIRST) + list(wc.TL_SECOND)]
        at = np.unravel_index(np.argmin(asserted), asserted.shape)
        smallest[method] = float(asserted.min())
        print(f"{method}: smallest peak over runner-up {asserted.min():.4f} (band {at[1]}); the straddling windows peak at "
              f"{idx[6].tolist()} and {idx[7].tolist()}")
        assert asserted.min() >= wc.TL_MARGIN, method
    assert min(smallest.values()) == smallest["bartlett"]
