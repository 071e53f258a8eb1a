"""Banded cross-spectra without a GPU: the exports of include/qi_bands.h and the census of tests/band_stream_cases.py against
that header, the refusals of qi_cross_spectra_bands and its size query's verdicts, qi_cross_spectra_bands_layout against the
restatement of tests/band_cases.py, the shape table's coverage, the NumPy restatement against einsums on explicit slices,
beamform.constant_q_windows and band_window_times on a worked table, and the plane-wave case restated in float64 on the
oracle's CWT."""
import ctypes
import os

import numpy as np
import pytest

import band_cases as bd
import band_stream_cases as bsc
import beam_cases as bc
from stream_table import header_functions, stream_functions

ROOT = bd.ROOT
HEADER = "qi_bands.h"
OTHER_HEADERS = ("qi_tfr.h", "qi_array.h", "qi_beam.h", "qi_adaptive.h", "qi_subspace.h", "qi_steer.h", "qi_windows.h", "qi_lags.h")
NAMES = {"qi_cross_spectra_bands_layout", "qi_cross_spectra_bands_scratch_bytes", "qi_cross_spectra_bands"}


def i64(values):
    a = np.ascontiguousarray(values, dtype=np.int64)
    return a, a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))


# ---- the header, the exports, the stream census ---------------------------------------------------------------------------------------
def test_library_exports_the_bands_header():
    from quantum_inferno_amd import _lib

    declared = set(header_functions(HEADER))
    assert declared == NAMES
    assert declared == set(_lib.BAND_PROTOTYPES)
    for table in (_lib.PROTOTYPES, _lib.ARRAY_PROTOTYPES, _lib.BEAM_PROTOTYPES, _lib.ADAPTIVE_PROTOTYPES, _lib.SUBSPACE_PROTOTYPES,
                  _lib.STEER_PROTOTYPES, _lib.WINDOW_PROTOTYPES, _lib.LAG_PROTOTYPES):
        assert not declared & set(table)
    for other in OTHER_HEADERS:
        assert not declared & set(header_functions(other)), other
    lib = _lib.load()
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in include/qi_bands.h but not exported"
        assert len(_lib.BAND_PROTOTYPES[name][1]) == len(header_functions(HEADER)[name].split(",")), name
    with open(os.path.join(ROOT, "include", HEADER)) as fh:
        text = fh.read()
    assert '#include "qi_tfr.h"' in text and '#include "qi_array.h"' in text and "BIT FOR BIT" in text
    with open(os.path.join(ROOT, "quantum_inferno_amd", "_build.py")) as fh:
        assert '"qi_bands.h"' in fh.read()


def test_every_stream_entry_point_has_a_case_and_nothing_else_is_named():
    assert bsc.TABLE.header == HEADER
    assert stream_functions(HEADER) == ["qi_cross_spectra_bands"]
    assert bsc.TABLE.named_functions() == stream_functions(HEADER)


def test_stream_case_table():
    import stream_order as so

    assert bsc.TABLE.ids() == ["cross_spectra_bands-matrices", "cross_spectra_bands-coherence"]
    for case in bsc.TABLE.cases:
        assert case.functions and callable(case.build) and case.asynchronous and case.engine is None, case.id
    assert bsc.TABLE.by_id("cross_spectra_bands-coherence").build.args == (True,)
    assert bsc.windows() == [16, 6, 61] and len({*bsc.TERMS}) == len({*bsc.HOP}) == len({*bsc.STRIDE}) == 3
    assert bsc.TABLE not in so.TABLES  # (that tuple's census is pinned elsewhere; the banded cases run in tests/test_gpu_bands.py)


def test_shape_cases_cover_every_edge():
    s = bd.SHAPES
    assert {x.C for x in s} == set(bd.RECORD_COUNTS) == {1, 2, 5, 16, 17, 33, 64}
    assert {t for x in s for t in x.terms} == set(bd.TERMS) == {1, 3, 16, 17, 31, 33, 40, 200}
    for C in (5, 17, 64):
        assert {x.terms[0] for x in s if x.C == C} == set(bd.TERMS), C
    assert {t for x in s for t in x.stride} == set(bd.STRIDES) == {1, 2, 3, 7}
    assert {x.bins[1] for x in s} == {1, 2, 3, 4, 5, 6} and max(x.nb for x in s) == 9 and max(x.n for x in s) <= 700
    hops = set()
    for x in s:
        first, count = x.bins
        assert len(x.terms) == len(x.hop) == len(x.stride) == count and 0 <= first and first + count <= x.nb, x.id
        assert np.all(bd.span_of(x.terms, x.stride) <= x.n) and np.all(np.diff(bd.offsets_of(x)) >= 1), x.id
        for kinds in bd.hop_kinds(x):
            assert kinds, x.id
            hops |= kinds
    assert hops == set(bd.HOPS)
    assert any(x.bins[1] >= 3 and len(set(x.terms)) == len(set(x.hop)) == len(set(x.stride)) == x.bins[1] for x in s)  # all tables differ
    assert any(1 in np.diff(bd.offsets_of(x)) and x.bins[1] > 1 for x in s)  # a single window in some band
    assert any(any(h > sp for h, sp in zip(x.hop, bd.span_of(x.terms, x.stride))) and not bd.read(x).all() for x in s)  # gaps
    assert any(int(bd.span_of(x.terms, x.stride).max()) == x.n for x in s)  # a window that is the whole record
    assert sum(1 for x in s if set(x.stride) == {1} and x.bins[1] > 1) >= 3  # held against the windowed call
    assert any(x.bins[0] > 0 for x in s) and any(x.bins[0] + x.bins[1] < x.nb for x in s)
    assert len(set(bd.ids())) == len(s) <= 40


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
GOOD = dict(dtype=None, C=2, nb=4, n=100, first=1, count=2, terms=(10, 4), hop=(5, 3), stride=(2, 7))
SHAPE_REFUSALS = (
    (dict(dtype=7), "dtype"), (dict(C=0), "panel shape"), (dict(nb=0), "panel shape"), (dict(n=0), "panel shape"),
    (dict(count=0, terms=(), hop=(), stride=()), "band range"), (dict(first=-1), "band range"), (dict(first=3), "band range"),
    (dict(first=4, count=1, terms=(1,), hop=(1,), stride=(1,)), "band range"),
    (dict(terms=(10, 0)), "band table"), (dict(hop=(0, 3)), "band table"), (dict(stride=(2, -1)), "band table"),
    (dict(terms=None), "null band table"), (dict(hop=None), "null band table"), (dict(stride=None), "null band table"),
    (dict(terms=(51, 4)), "longer"), (dict(terms=(10, 101), stride=(2, 1)), "longer"), (dict(stride=(12, 7)), "longer"),
    (dict(terms=(10, 4), stride=(2, 1 << 62)), "longer"),  # (no product overflows on the way)
    (dict(C=64, nb=2, first=0, n=1 << 30, terms=(1, 1), hop=(1, 1), stride=(1, 1)), "too large"),  # 2^43 entries
    (dict(C=1 << 20), "too large"),
    (dict(C=1, nb=2, first=0, n=1 << 34, terms=(1, 1), hop=(1, 1), stride=(1, 1)), "too large"),  # the grid passes 2^31
    (dict(C=1, nb=1 << 31, first=0, n=1 << 30, terms=(1, 1), hop=(1 << 20, 1 << 20), stride=(1, 1)), "too large"),  # the panel's index arithmetic
)


def _args(a):
    """(scalars before the tables, the three table pointers, the arrays that back them)."""
    keep = [None if a[k] is None else i64(a[k]) for k in ("terms", "hop", "stride")]
    ptrs = [None if k is None else k[1] for k in keep]
    return (a["dtype"], a["C"], a["nb"], a["n"], a["first"], a["count"]), ptrs, keep


def test_cross_spectra_bands_refusals_without_a_gpu():
    """Refused before the device is touched: the pointers are never followed (a host without a GPU runs this test).  The size
    query gives the call's status and message."""
    from quantum_inferno_amd import _lib

    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    odd = ctypes.c_void_p(ctypes.addressof(buf) + 4)

    def call(a, z=p, weight=None, csd=p, coh=p, scratch=p, nbytes=1 << 20):
        (d, *rest), ptrs, keep = _args(a)
        return lib.qi_cross_spectra_bands(d, 0, z, *rest, *ptrs, weight, csd, coh, scratch, nbytes, None)

    def query(a):
        scalars, ptrs, keep = _args(a)
        return lib.qi_cross_spectra_bands_scratch_bytes(*scalars, *ptrs)

    for code in (_lib.QI_F32, _lib.QI_F64):
        good = {**GOOD, "dtype": code}
        for change, what in SHAPE_REFUSALS:
            bad = {**good, **change}
            rc = call(bad)
            msg = lib.qi_last_error()
            assert rc < 0 and what in msg.decode(), (change, msg)
            assert query(bad) == rc and lib.qi_last_error() == msg, change
        for kw in (dict(z=None), dict(scratch=None)):
            assert call(good, **kw) < 0 and b"null" in lib.qi_last_error(), kw
        assert call(good, csd=None, coh=None) < 0 and b"nothing" in lib.qi_last_error()
        for kw in (dict(z=odd), dict(csd=odd), dict(coh=ctypes.c_void_p(ctypes.addressof(buf) + 2)),
                   dict(scratch=ctypes.c_void_p(ctypes.addressof(buf) + 8))):
            assert call(good, **kw) < 0 and b"misaligned" in lib.qi_last_error(), kw
        need = query(good)
        total = int(bd.layout(100, (10, 4), (5, 3), (2, 7))[-1])
        assert total == 17 + 27
        assert need >= (5 * 2 + 1) * 8 + total * 2 * 2 * 2 * (8 if code == _lib.QI_F64 else 4)  # the tables, the weights, the matrices
        assert call(good, nbytes=0) < 0 and b"scratch" in lib.qi_last_error()
        assert call(good, nbytes=need - 1) < 0 and b"scratch" in lib.qi_last_error()
    assert call({**GOOD, "dtype": _lib.QI_F64}, csd=ctypes.c_void_p(ctypes.addressof(buf) + 8)) < 0 and b"misaligned" in lib.qi_last_error()


# ---- the layout -----------------------------------------------------------------------------------------------------------------------
def lib_layout(lib, n, terms, hop, stride, want_offsets=True):
    (t, tp), (h, hp), (s, sp) = i64(terms), i64(hop), i64(stride)
    out = np.full(len(t) + 1, -7, dtype=np.int64)
    total = lib.qi_cross_spectra_bands_layout(n, len(t), tp, hp, sp, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)) if want_offsets else None)
    return int(total), out


def test_layout_equals_the_restatement():
    from quantum_inferno_amd import _lib

    lib = _lib.load()
    for x in bd.SHAPES:
        want = bd.offsets_of(x)
        total, got = lib_layout(lib, x.n, x.terms, x.hop, x.stride)
        assert total == want[-1] and np.array_equal(got, want), x.id
        assert lib_layout(lib, x.n, x.terms, x.hop, x.stride, want_offsets=False)[0] == total
    edges = (
        (100, (100,), (1,), (1,), [0, 1]),                      # span == n
        (100, (34,), (5,), (3,), [0, 1]),                       # span == n by the stride
        (100, (34, 33), (1, 1), (3, 3), [0, 1, 5]),             # span n and span n - 3
        (100, (10, 10), (101, 1 << 40), (1, 2), [0, 1, 2]),     # hop > n: one window
        (100, (1, 1, 1), (1, 7, 100), (1, 9, 1 << 50), [0, 100, 115, 116]),  # terms == 1: the stride does not matter
        (1, (1,), (1,), (1,), [0, 1]),
    )
    for n, terms, hop, stride, want in edges:
        total, got = lib_layout(lib, n, terms, hop, stride)
        assert total == want[-1] and got.tolist() == want, (n, terms, hop, stride)
        assert np.array_equal(bd.layout(n, terms, hop, stride), want)
    for n, terms, hop, stride, what in ((0, (1,), (1,), (1,), "geometry"), (100, (101,), (1,), (1,), "longer"), (100, (34,), (1,), (4,), "longer"),
                                        (100, (0,), (1,), (1,), "band table"), (100, (1,), (0,), (1,), "band table"), (100, (1,), (1,), (0,), "band table")):
        assert lib_layout(lib, n, terms, hop, stride)[0] < 0 and what in lib.qi_last_error().decode(), (n, terms, hop, stride)
    assert lib.qi_cross_spectra_bands_layout(100, 0, None, None, None, None) < 0 and b"geometry" in lib.qi_last_error()
    assert lib.qi_cross_spectra_bands_layout(100, 1, None, None, None, None) < 0 and b"null" in lib.qi_last_error()


def test_the_last_shape_under_2_to_40_entries_is_accepted_and_the_next_refused():
    from quantum_inferno_amd import _lib

    lib = _lib.load()
    count = 1 << 14
    ones = i64(np.ones(count, dtype=np.int64))

    def query(n, C=64):
        return lib.qi_cross_spectra_bands_scratch_bytes(_lib.QI_F32, C, count, n, 0, count, ones[1], ones[1], ones[1])

    # 2^14 bands of 2^14 one-term windows each, 64^2 entries a matrix: 2^40 entries
    got = query(1 << 14)
    assert got >= (5 * count + 1) * 8 + (1 << 40) * 8
    assert query((1 << 14) + 1) < 0 and b"too large" in lib.qi_last_error()
    # one more window in one band alone
    hop = i64(np.ones(count, dtype=np.int64))
    terms = i64(np.concatenate([[1], np.full(count - 1, 2)]))
    assert lib.qi_cross_spectra_bands_scratch_bytes(_lib.QI_F32, 64, count, (1 << 14) + 1, 0, count, terms[1], hop[1], ones[1]) < 0
    assert b"too large" in lib.qi_last_error()
    terms = i64(np.full(count, 2))
    assert lib.qi_cross_spectra_bands_scratch_bytes(_lib.QI_F32, 64, count, (1 << 14) + 1, 0, count, terms[1], hop[1], ones[1]) > 0


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def test_restatement_against_einsum_on_explicit_slices():
    for x in bd.SHAPES:
        z = bd.panel(x)
        first, count = x.bins
        w = bd.weights(x)
        off, s = bd.restate(z, first, x.terms, x.hop, x.stride, w)
        assert np.array_equal(off, bd.offsets_of(x)) and s.shape == (off[-1], x.C, x.C), x.id
        for b in range(count):
            for k in {0, (off[b + 1] - off[b]) // 2, off[b + 1] - off[b] - 1}:
                idx = k * x.hop[b] + np.arange(x.terms[b]) * x.stride[b]
                assert idx[-1] < x.n and idx[-1] - idx[0] + 1 == bd.span_of(x.terms, x.stride)[b]
                cut = z[:, first + b, :][:, idx]
                want = np.einsum("is,js->ij", np.conj(cut), cut) * w[b]
                assert np.array_equal(s[off[b] + k], want), (x.id, b, k)
            last = (off[b + 1] - off[b] - 1) * x.hop[b] + bd.span_of(x.terms, x.stride)[b]
            assert last <= x.n < last + x.hop[b], (x.id, b)  # no window is left out
        assert np.abs(s - np.conj(np.swapaxes(s, 1, 2))).max() <= 1e-12 * np.abs(s).max()
        one = [m for b in range(count) if x.terms[b] == 1 for m in range(off[b], off[b + 1])]
        if one and x.C > 1:
            assert np.abs(bd.coherence_of(s[one]) - 1).max() <= 1e-12, x.id


def test_integer_panel_sums_are_exact_in_float32():
    for C in (5, 17, 64):
        z = bd.integer_panel(C, 4, 620)
        assert np.abs(z.real).max() <= 3 and np.abs(z.imag).max() <= 3
        off, s = bd.restate(z, 1, (200, 40, 1), (7, 100, 300), (3, 7, 2))
        assert np.array_equal(s, np.rint(s.real) + 1j * np.rint(s.imag)) and max(np.abs(s.real).max(), np.abs(s.imag).max()) < 2 ** 24
        assert not np.array_equal(s, np.swapaxes(s, 1, 2)) and not np.array_equal(s[0], s[1]) and not np.array_equal(s[off[1]], s[off[1] + 1])


# ---- the window tables ----------------------------------------------------------------------------------------------------------------
def test_constant_q_windows_on_a_worked_table():
    from quantum_inferno_amd import beamform

    f = np.array([1.0, 2.0, 10.0, 50.0, 400.0, 4000.0])
    # fs 1000, 20 periods: spans 20000, 10000, 2000, 400, 50, 5
    bins, terms, hop, stride = beamform.constant_q_windows(f, 1000.0, 10000, 20.0, max_terms=100)
    assert bins == (1, 5)
    assert stride.tolist() == [100, 20, 4, 1, 1] and terms.tolist() == [100, 100, 100, 50, 5] and hop.tolist() == [5000, 1000, 200, 25, 2]
    assert all(a.dtype == np.int64 for a in (terms, hop, stride))
    assert np.all((terms - 1) * stride + 1 <= [10000, 2000, 400, 50, 5])
    bins, terms, hop, stride = beamform.constant_q_windows(f, 1000.0, 10000, 20.0, hop_fraction=0.01, max_terms=None)
    assert bins == (1, 5) and stride.tolist() == [1] * 5 and terms.tolist() == [10000, 2000, 400, 50, 5] and hop.tolist() == [100, 20, 4, 1, 1]
    # a cap that does not divide the span: the last term stays inside it
    bins, terms, hop, stride = beamform.constant_q_windows([3.0], 1000.0, 1 << 20, 20.0)
    assert bins == (0, 1) and stride.tolist() == [2] and terms.tolist() == [3334] and (terms[0] - 1) * 2 + 1 <= 6667
    # a descending table: the range that fits lies at its start
    assert beamform.constant_q_windows(f[::-1], 1000.0, 10000, 20.0)[0] == (0, 5)
    assert [a.tolist() for a in beamform.constant_q_windows([7.0], 1000.0, 1 << 16, 1e-9)[1:]] == [[1], [1], [1]]  # at least one sample
    for bad in (dict(frequency_hz=[1.0], n=100), dict(frequency_hz=[400.0, 1.0, 400.0]), dict(frequency_hz=[0.0, 400.0]),
                dict(frequency_hz=f, max_terms=0), dict(frequency_hz=f, window_cycles=0.0), dict(frequency_hz=f, hop_fraction=0.0)):
        args = {**dict(frequency_sample_rate_hz=1000.0, n=10000, window_cycles=20.0), **bad}
        with pytest.raises(ValueError):
            beamform.constant_q_windows(**args)
    doc = beamform.constant_q_windows.__doc__
    assert "cap on work, not a measured number" in doc and "two orders of magnitude" in doc


def test_band_window_times_on_a_worked_table():
    from quantum_inferno_amd import beamform

    terms, hop, stride = np.array([3, 1, 4]), np.array([4, 5, 20]), np.array([2, 9, 1])
    off = bd.layout(12, terms, hop, stride)
    assert off.tolist() == [0, 2, 5, 6]
    t = beamform.band_window_times(off, terms, hop, stride, 10.0)
    # spans 5, 1, 4: centres of [0, 5), [4, 9); [0, 1), [5, 6), [10, 11); [0, 4)
    assert t.dtype == np.float64 and t.tolist() == [0.25, 0.65, 0.05, 0.55, 1.05, 0.2]
    for bad in ((off[:-1], terms, hop, stride), (off + 1, terms, hop, stride), (off, terms[:2], hop, stride), ([0, 2, 2, 3], terms, hop, stride)):
        with pytest.raises(ValueError):
            beamform.band_window_times(*bad, 10.0)


# ---- the plane-wave case, restated in float64 -------------------------------------------------------------------------------------------
def test_plane_wave_case_peaks_at_the_true_slowness_not_its_negative():
    """The conjugation convention of beamform.fk_timeline_cq, pinned: the oracle's order-12 CWT of the five delayed records,
    the restated matrices (weight 1 / terms), the restated semblance with the delays as plane_wave_delays gives them.  65 bands
    fit (7.9 .. 316 Hz, 1 .. 80 windows of 40 periods each, summed at up to 64 terms).  Measured here: in 57 bands every window
    peaks at the source's grid point, each at least beam_cases.PW_MARGIN above its runner-up -- every band up to 178 Hz, and
    199.5 and 251 Hz; the smallest margin of a window among them is 0.015 (105.9 Hz; 0.017 at 70.8 Hz), the largest band's
    0.33 (56 Hz).  The eight bands of 188 Hz and above that fail are where the narrow-band assumption ends:
    f * max|tau| there is above 3 periods, against an atom of 4.5 periods to one standard deviation.  With the delays negated
    no band qualifies."""
    x = bd.pw_records()
    own = bd.pw_delays()[bc.pw_true_index()]
    assert x.shape == (5, bd.PW_N) and 12 < np.abs(own).max() * bc.PW_FS < 14  # the source's largest delay, in samples
    f, z = bd.pw_oracle()
    geometry = bd.pw_geometry(f, bd.PW_MAX_TERMS)
    (first, count), terms, hop, stride = geometry
    assert first + count == len(f) and count >= 60 and stride.max() > 1 and terms.max() <= bd.PW_MAX_TERMS
    off, power = bd.pw_power(z, f, geometry)
    assert power.shape == (off[-1], 81) and np.isfinite(power).all() and power.max() <= 1 + 1e-12
    rows = bd.pw_margins(off, power)
    asserted = bd.pw_asserted(rows)
    print("band: Hz, windows, every window at the source, smallest margin")
    for b, (ok, margin) in enumerate(rows):
        print(f"{b}: {f[first + b]:.1f} {off[b + 1] - off[b]} {ok} {margin:.4f}{' *' if b in asserted else ''}")
    print(f"{len(asserted)} bands asserted; smallest margin {min(rows[b][1] for b in asserted):.4f}, bound {bc.PW_MARGIN:g}")
    assert len(asserted) >= bd.PW_MIN_BANDS and tuple(asserted) == bd.pw_asserted_bands()
    for b in asserted:
        assert (np.argmax(power[off[b]:off[b + 1]], axis=1) == bc.pw_true_index()).all(), b
    # the other sign: the panel's phase does not run that way
    bins, terms, hop, stride = geometry
    _, s = bd.restate(z, bins[0], terms, hop, stride, 1.0 / terms)
    flipped = bc.restate(s, np.repeat(f[first:first + count], np.diff(off)), -bd.pw_delays(), normalize=True)
    assert not bd.pw_asserted(bd.pw_margins(off, flipped))
    mirror = (8 - bc.PW_TRUE[1]) * 9 + (8 - bc.PW_TRUE[0])  # the grid is symmetric: -s is a grid point
    assert (np.argmax(flipped[off[asserted[0]]:off[asserted[0] + 1]], axis=1) == mirror).all()
