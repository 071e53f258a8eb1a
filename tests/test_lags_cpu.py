"""Pair lags without a GPU: the exports of include/qi_lags.h and the census of tests/lag_stream_cases.py against that header,
the refusals of qi_pair_lags and the size query's verdicts, the NumPy restatement of tests/lag_cases.py against a time-domain
numpy.correlate, the conditions the GPU tests rely on (held on the restatement: the peak's margins, the exact spectra, the
tie, the impulse), and the host helpers beamform.slowness_from_lags and beamform.lag_closure."""
import ctypes
import os
import re

import numpy as np

import lag_cases as lc
import lag_stream_cases as lsc
from stream_table import header_functions, stream_functions

ROOT = lc.ROOT
HEADER = "qi_lags.h"
OTHER_HEADERS = ("qi_tfr.h", "qi_array.h", "qi_beam.h", "qi_adaptive.h", "qi_subspace.h", "qi_steer.h", "qi_windows.h")
NAMES = {"qi_pair_lags_scratch_bytes", "qi_pair_lags"}


# ---- the header, the exports, the stream census ---------------------------------------------------------------------------------------
def test_library_exports_the_lags_header():
    from quantum_inferno_amd import _lib

    declared = set(header_functions(HEADER))
    assert declared == NAMES
    assert declared == set(_lib.LAG_PROTOTYPES)
    for table in (_lib.PROTOTYPES, _lib.ARRAY_PROTOTYPES, _lib.BEAM_PROTOTYPES, _lib.ADAPTIVE_PROTOTYPES, _lib.SUBSPACE_PROTOTYPES,
                  _lib.STEER_PROTOTYPES, _lib.WINDOW_PROTOTYPES):
        assert not declared & set(table)
    for other in OTHER_HEADERS:
        assert not declared & set(header_functions(other)), other
    lib = _lib.load()
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in include/qi_lags.h but not exported"
        assert getattr(lib, name).argtypes == _lib.LAG_PROTOTYPES[name][1], f"{name}: load() did not attach the table"
        assert len(_lib.LAG_PROTOTYPES[name][1]) == len(header_functions(HEADER)[name].split(",")), name
    with open(os.path.join(ROOT, "include", "qi_lags.h")) as fh:
        text = fh.read()
    assert '#include "qi_tfr.h"' in text and '#include "qi_array.h"' in text
    assert _lib.LAG_WEIGHTINGS == lc.WEIGHTINGS
    for k, name in enumerate(("QI_LAG_PLAIN", "QI_LAG_PHAT", "QI_LAG_SCOT")):
        assert re.search(rf"#define {name} {k}\b", text), name


def test_every_stream_entry_point_has_a_case_and_nothing_else_is_named():
    assert lsc.TABLE.header == HEADER
    assert stream_functions(HEADER) == ["qi_pair_lags"]
    assert lsc.TABLE.named_functions() == stream_functions(HEADER)
    assert lsc.TABLE.ids() == ["pair_lags-f64-plain-all", "pair_lags-f32-phat-peaks", "pair_lags-f64-phat-cc", "pair_lags-f32-plain-cc"]
    for case in lsc.TABLE.cases:
        assert case.functions and callable(case.build) and case.asynchronous and case.engine is None, case.id


def test_case_table_covers_what_the_kernel_branches_on():
    cases = lc.CASES
    assert {(c.L, c.upsample) for c in cases} == {(64, 1), (128, 1), (2048, 1), (2048, 4), (8192, 1), (8192, 4)}
    for key in {(c.L, c.upsample) for c in cases}:
        mine = [c for c in cases if (c.L, c.upsample) == key]
        assert {c.weighting for c in mine} == {0, 1, 2} and key[0] // 2 - 1 in {c.max_lag for c in mine} and len({c.max_lag for c in mine}) >= 3, key
    assert {c.max_lag for c in cases} >= {0, 1, 17, 31, 63, 1023, 4095}
    assert {c.C for c in cases} == {2, 3, 5, 17} and {c.nstack for c in cases} == {1, 3}
    assert {c.bins for c in cases} == set(lc.BIN_KINDS)
    assert {(c.weighting, c.halve, c.normalize) for c in cases} >= {(w, h, n) for w in (0, 1, 2) for h, n in ((True, True), (False, False))}
    for w in (0, 1, 2):
        assert {(c.halve, c.normalize) for c in cases if c.weighting == w} == {(True, True), (True, False), (False, True), (False, False)}, w
    nf = 65
    assert [lc.bin_range(k, nf) for k in lc.BIN_KINDS] == [(0, 65), (1, 65), (0, 40), (8, 40), (8, 65)]
    assert len(set(lc.ids())) == len(cases) <= 24
    # log2 of the complex transform's length modulo 4: the first pass of radix 2, 4 and none (8: the edge cases' L = 256)
    assert {(int(np.log2(c.L)) - 1) % 4 for c in cases} == {0, 1, 2}
    for C in (2, 3, 5, 17):
        i, j = lc.pair_table(C)
        assert [lc.pair_index(C, a, b) for a, b in zip(i, j)] == list(range(C * (C - 1) // 2))


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
GOOD = dict(dtype=None, nstack=2, C=3, nfft=64, lo=1, hi=30, weighting=1, up=4, max_lag=20)
SHAPE_REFUSALS = (
    (dict(dtype=7), "dtype"), (dict(nstack=0), "stack shape"), (dict(C=1), "stack shape"), (dict(C=0), "stack shape"),
    (dict(up=3), "upsample"), (dict(up=0), "upsample"), (dict(up=16), "upsample"), (dict(nfft=48), "transform length"),
    (dict(nfft=8), "transform length"), (dict(nfft=4096), "transform length"), (dict(nfft=0), "transform length"),
    (dict(C=1 << 21), "too large"), (dict(nstack=1 << 30, C=64), "too large"), (dict(nstack=1 << 22, C=1024), "too large"),
)
CALL_REFUSALS = (
    (dict(weighting=3), "weighting"), (dict(weighting=-1), "weighting"), (dict(lo=-1), "bin range"), (dict(hi=34), "bin range"),
    (dict(lo=31), "bin range"), (dict(max_lag=-1), "max_lag"), (dict(max_lag=128), "max_lag"),
)


def test_pair_lags_refusals_without_a_gpu():
    """Refused before the device is touched: the pointers are never followed (this machine may have no GPU at all)."""
    from quantum_inferno_amd import _lib

    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    good = {**GOOD, "dtype": _lib.QI_F32}

    def call(a, csd=p, cc=p, lag=p, value=p, scratch=p, nbytes=0):
        return lib.qi_pair_lags(a["dtype"], 0, csd, a["nstack"], a["C"], a["nfft"], a["lo"], a["hi"], a["weighting"], 1, 1, a["up"],
                                a["max_lag"], cc, lag, value, scratch, nbytes, None)

    def query(a):
        return lib.qi_pair_lags_scratch_bytes(a["dtype"], a["nstack"], a["C"], a["nfft"], a["up"])

    for change, what in SHAPE_REFUSALS:
        bad = {**good, **change}
        got = query(bad)
        msg = lib.qi_last_error()
        assert got < 0 and what in msg.decode(), (change, msg)
        assert call(bad) == got and lib.qi_last_error() == msg, change
    assert query(good) == 0 and query({**good, "dtype": _lib.QI_F64, "nfft": 2048, "up": 4}) == 0 and query({**good, "nfft": 16}) == 0
    for change, what in CALL_REFUSALS:
        assert call({**good, **change}) < 0, change
        assert what in lib.qi_last_error().decode(), (change, lib.qi_last_error())
    assert call(good, csd=None) < 0 and b"null" in lib.qi_last_error()
    assert call(good, cc=None, lag=None, value=None) < 0 and b"nothing" in lib.qi_last_error()
    assert call(good, nbytes=-1) < 0 and b"scratch" in lib.qi_last_error()
    for kw in (dict(csd=ctypes.c_void_p(ctypes.addressof(buf) + 4)), dict(cc=ctypes.c_void_p(ctypes.addressof(buf) + 2)),
               dict(lag=ctypes.c_void_p(ctypes.addressof(buf) + 1)), dict(value=ctypes.c_void_p(ctypes.addressof(buf) + 3)),
               dict(scratch=ctypes.c_void_p(ctypes.addressof(buf) + 8))):
        assert call(good, **kw) < 0 and b"misaligned" in lib.qi_last_error(), kw
    assert call({**good, "dtype": _lib.QI_F64}, lag=ctypes.c_void_p(ctypes.addressof(buf) + 4)) < 0 and b"misaligned" in lib.qi_last_error()


# ---- the restatement against the time domain --------------------------------------------------------------------------------------------
def test_restatement_is_the_time_domain_correlation():
    """Records of 24 samples in transforms of 64: the circular correlation is the linear one, numpy.correlate's."""
    rng = np.random.default_rng(20260304)
    n, nfft, C = 24, 64, 4
    x = rng.standard_normal((C, n))
    X = np.fft.rfft(x, nfft, axis=-1)
    s = np.einsum("if,jf->fij", np.conj(X), X)[None]
    rows, cols = lc.pair_table(C)
    worst = 0.0
    for doubled in (False, True):
        t = s.copy()
        if doubled:
            t[:, 1:-1] *= 2.0  # the one-sided weights, undone by halve_interior (exactly)
        res = lc.restate(t, None, 0, doubled, False, 1, n - 1)
        ref = lc.restate(s, None, 0, False, False, 1, n - 1)
        assert np.array_equal(res.r, ref.r)
        for p, (i, j) in enumerate(zip(rows, cols)):
            want = np.correlate(x[j], x[i], "full")  # lag l at index l + n - 1: sum_t x_i[t] x_j[t + l]
            worst = max(worst, float(np.abs(res.cc[0, p] - want).max() / np.abs(want).max()))
            assert res.index[0, p] == np.argmax(want) - (n - 1)
    assert worst <= 1e-13, worst
    coef = lc.restate(s, None, 0, False, True, 1, n - 1)
    for p, (i, j) in enumerate(zip(rows, cols)):
        want = np.correlate(x[j], x[i], "full") / np.sqrt((x[i] ** 2).sum() * (x[j] ** 2).sum())
        assert np.abs(coef.cc[0, p] - want).max() <= 1e-13 and np.abs(coef.cc).max() <= 1.0
    # a record against its own delayed copy, zero-padded fourfold: the peak sits at four times the delay, positive: j lags i
    y = np.stack([np.r_[x[0], np.zeros(5)], np.r_[np.zeros(5), x[0]]])
    Y = np.fft.rfft(y, nfft, axis=-1)
    up = lc.restate(np.einsum("if,jf->fij", np.conj(Y), Y)[None], None, 0, False, True, 4, None)
    assert up.index[0, 0] == 20 and abs(up.peak_lag[0, 0] - 5.0) <= 1e-12 and abs(up.peak_value[0, 0] - 1.0) <= 1e-12
    print(f"restatement against numpy.correlate, of the largest sample: {worst:.3g}")


def test_parity_fixtures_hold_their_conditions():
    """What tests/test_gpu_lags.py relies on: the maximum stands MARGIN of the peak above every non-adjacent sample of the
    window, and above its two neighbours by far more than twice the float32 tolerance on cc (so an error within the tolerance
    cannot move the integer index); the planted delay of every pair lies in the window and is recovered within the
    parabola's bias, which is below 0.13 samples of the finer grid."""
    worst_far, worst_near, worst_bias = np.inf, np.inf, 0.0
    for case in lc.CASES:
        s, d = lc.matrices(case.id)
        res = lc.restated(case.id)
        assert s.shape == (case.nstack, case.L // case.upsample // 2 + 1, case.C, case.C) and np.isfinite(res.r).all(), case.id
        far, near = lc.margins(res)
        assert far >= lc.MARGIN, (case.id, far)
        assert near >= 20 * 2 * lc.TOL["float32"] * np.abs(res.r).max() / res.peak_value.min(), (case.id, near)
        rows, cols = lc.pair_table(case.C)
        planted = d[:, cols] - d[:, rows]
        assert np.abs(planted).max() <= case.max_lag and np.isfinite(res.bound).all(), case.id
        bias = np.abs(res.peak_lag * case.upsample - planted)
        assert (np.abs(res.index - planted) <= 0.5 + 1e-9).all(), case.id  # the nearest sample of the finer grid
        worst_far, worst_near, worst_bias = min(worst_far, far), min(worst_near, near), max(worst_bias, float(bias.max()))
    assert worst_bias <= 0.13, worst_bias
    fractions = np.concatenate([np.abs(np.modf(lc.matrices(c.id)[1])[0]).ravel() for c in lc.CASES])
    assert (fractions == 0).any() and (fractions > 0.05).any()
    print(f"smallest margin over non-adjacent samples {worst_far:.3g} (bound {lc.MARGIN:g}), over the neighbours {worst_near:.3g}; "
          f"largest parabola bias {worst_bias:.3g} samples of the finer grid")


def test_exact_spectra_restate_exactly():
    for nfft, up in ((64, 1), (64, 2), (4096, 1), (4096, 2)):
        s = lc.exact_matrices(nfft, up)
        for halve in (False, True):
            res = lc.restate(s, None, 0, halve, False, up, None)
            want = lc.exact_correlation(s, up, halve)
            assert np.array_equal(res.r, want), (nfft, up, halve)
            assert np.array_equal(want * nfft * 2, np.rint(want * nfft * 2)) and np.abs(want * nfft).max() < 2 ** 10
            assert len({tuple(row) for row in want.reshape(-1, want.shape[-1])[:, :4]}) == want.shape[0] * want.shape[1]


def test_tie_and_impulse_restated():
    # two bins, 0 and nfft / 2: r[l] = (x0 + xn (-1)^l) / nfft -- every even lag ties; the smallest wins
    nfft = 64
    s = np.zeros((1, 33, 2, 2), dtype=np.complex128)
    s[0, 0, 0, 1], s[0, 32, 0, 1] = 5, 3
    res = lc.restate(s, None, 0, False, False, 1, 5)
    assert res.cc[0, 0].tolist() == [2 / 64, 8 / 64] * 5 + [2 / 64] and res.index[0, 0] == -4 and res.delta[0, 0] == 0
    assert res.peak_lag[0, 0] == -4 and res.peak_value[0, 0] == 8 / 64
    # a flat spectrum under PHAT, not halved: the unit impulse
    flat = np.zeros((1, 33, 2, 2), dtype=np.complex128)
    flat[0, :, 0, 1] = 3.0
    imp = lc.restate(flat, None, 1, False, True, 1, None)
    want = np.zeros(63)
    want[31] = 1.0
    assert np.array_equal(imp.cc[0, 0], want) and imp.peak_lag[0, 0] == 0 and imp.peak_value[0, 0] == 1.0


def test_edge_fixtures_peak_where_they_should():
    for nfft, max_lag, delay in ((64, 5, -5), (64, 5, 5), (64, 31, 31), (64, 31, -31), (256, 9, 9)):
        res = lc.restate(lc.delayed_pair(nfft, delay), None, 1, False, True, 1, max_lag)
        far, near = lc.margins(res)
        assert res.index[0, 0] == delay and far >= lc.MARGIN and near >= lc.MARGIN, (nfft, delay, far, near)
        assert abs(res.peak_value[0, 0] - 1.0) <= 1e-12 and abs(res.peak_lag[0, 0] - delay) <= 1e-12


def test_non_finite_entries_poison_their_pair_alone():
    case = lc.by_id("L64_u1_c5_s1_mfull_scot_h1n0_no_dc")
    s = lc.matrices(case.id)[0].copy()
    clean = lc.restated(case.id)
    lo, hi = lc.bin_range(case.bins, 33)
    s[0, 10, 1, 3] = np.nan
    s[0, 0, 0, 1] = np.inf  # outside the band (bin 0 of "no_dc"): not looked at
    res = lc.restate(s, (lo, hi), case.weighting, case.halve, case.normalize, case.upsample, case.max_lag)
    p = lc.pair_index(5, 1, 3)
    keep = np.arange(10) != p
    assert np.isnan(res.cc[0, p]).all() and np.isnan(res.peak_lag[0, p]) and np.isnan(res.peak_value[0, p])
    assert np.array_equal(res.cc[0, keep], clean.cc[0, keep]) and np.array_equal(res.peak_lag[0, keep], clean.peak_lag[0, keep])
    s[0, 20, 2, 2] = np.nan  # an auto-power: every SCOT pair of record 2
    res = lc.restate(s, (lo, hi), case.weighting, case.halve, case.normalize, case.upsample, case.max_lag)
    hit = np.array([2 in (i, j) or (i, j) == (1, 3) for i, j in zip(*lc.pair_table(5))])
    assert np.isnan(res.peak_lag[0]).tolist() == hit.tolist()


# ---- the host helpers ---------------------------------------------------------------------------------------------------------------------
POSITIONS_M = np.array([[0.0, 0.0], [32.0, 4.0], [-12.0, 24.0], [-20.0, -16.0], [8.0, -28.0]])
SLOWNESS = np.array([[3 / 1024, -5 / 2048], [-1 / 512, 1 / 4096]])  # dyadic: every product and sum below is exact in float64


def exact_lags():
    rows, cols = lc.pair_table(len(POSITIONS_M))
    return (POSITIONS_M[cols] - POSITIONS_M[rows]) @ SLOWNESS.T  # [pairs, 2 windows]


def test_slowness_from_lags_recovers_a_known_slowness_exactly():
    import torch

    from quantum_inferno_amd import beamform

    lags = exact_lags()
    s, rms = beamform.slowness_from_lags(lags[:, 0], POSITIONS_M)
    assert isinstance(s, torch.Tensor) and s.dtype == torch.float64 and s.shape == (2,) and rms.shape == ()
    assert s.tolist() == SLOWNESS[0].tolist() and float(rms) == 0.0
    s, rms = beamform.slowness_from_lags(torch.from_numpy(lags.T.copy()), POSITIONS_M, weights=np.arange(1.0, 11.0))
    assert s.shape == (2, 2) and s.tolist() == SLOWNESS.tolist() and rms.tolist() == [0.0, 0.0]
    # one bad pair: a weight of 0 takes it out, a weight of 1 shows in the residual
    off = lags[:, 0].copy()
    off[3] += 0.5
    w = np.ones(10)
    w[3] = 0.0
    s, rms = beamform.slowness_from_lags(off, POSITIONS_M, weights=w)
    assert s.tolist() == SLOWNESS[0].tolist() and float(rms) == 0.0
    s, rms = beamform.slowness_from_lags(off, POSITIONS_M)
    assert float(rms) > 0.1 and s.tolist() != SLOWNESS[0].tolist()
    az, v = beamform.back_azimuth_and_velocity(beamform.slowness_from_lags(lags[:, 0], POSITIONS_M)[0])
    assert abs(float(v) - 1.0 / np.hypot(*SLOWNESS[0])) <= 1e-9 and abs(float(az) - np.degrees(np.arctan2(-3 / 1024, 5 / 2048)) % 360) <= 1e-9
    line = np.array([[0.0, 0.0], [1.0, 1.0], [3.0, 3.0]])  # collinear: the normal equations are singular
    s, _ = beamform.slowness_from_lags(np.array([1.0, 3.0, 2.0]), line)
    assert torch.isnan(s).all()
    for bad in (dict(lags_s=np.zeros(9), positions_m=POSITIONS_M), dict(lags_s=np.zeros(10), positions_m=POSITIONS_M[:, :1])):
        try:
            beamform.slowness_from_lags(**bad)
        except ValueError:
            continue
        raise AssertionError(bad)


def test_lag_closure_is_zero_on_exact_delays():
    import torch

    from quantum_inferno_amd import beamform

    lags = exact_lags()
    closure = beamform.lag_closure(lags.T.copy(), 5)
    assert closure.shape == (2, 10) and closure.dtype == torch.float64 and (closure == 0).all()
    off = lags[:, 0].copy()
    off[lc.pair_index(5, 1, 3)] += 0.25  # the pair (1, 3) sits in the triplets (0, 1, 3), (1, 2, 3) and (1, 3, 4)
    trip = [(i, j, k) for i in range(5) for j in range(i + 1, 5) for k in range(j + 1, 5)]
    got = beamform.lag_closure(off, 5).tolist()
    want = [0.25 if (t[0], t[1]) == (1, 3) or (t[1], t[2]) == (1, 3) else -0.25 if (t[0], t[2]) == (1, 3) else 0.0 for t in trip]
    assert got == want and sorted(got) == [-0.25] + [0.0] * 7 + [0.25] * 2
    for bad in ((lags[:, 0], 4), (lags[:3, 0], 2)):
        try:
            beamform.lag_closure(*bad)
        except ValueError:
            continue
        raise AssertionError(bad)


def test_python_surface_documents_its_conventions():
    from quantum_inferno_amd import engine, styx_fft

    doc = styx_fft.pair_lags_pow2.__doc__
    assert "CIRCULAR over nfft_points" in doc and "nfft_points >= 2 * segment_points makes it linear" in doc
    assert "record j lags record i" in doc and "record j lags record i" in engine.pair_lags.__doc__
