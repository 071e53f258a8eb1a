"""Time-domain delay-and-sum without a GPU: the exports of include/qi_timebeam.h and the census of
tests/timebeam_stream_cases.py against that header, every refusal of the two calls and the size query's verdicts, the case
table's coverage and the conditions the GPU tests rely on (the peak's margin in every window), engine.delay_bank and
engine.quantize_delays against the restatements of tests/timebeam_cases.py, and the plane wave of tests/beam_cases.py through
the restatement: the F detector's peak and the beam traces."""
import ctypes
import os
import re

import numpy as np
import pytest

import timebeam_cases as tb
import timebeam_stream_cases as tsc
from stream_table import header_functions, stream_functions

from quantum_inferno_amd._lib import TIMEBEAM_PROTOTYPES  # noqa: F401  (the feature's table: without it nothing here has a subject)

ROOT = tb.ROOT
HEADER = "qi_timebeam.h"
OTHER_HEADERS = ("qi_tfr.h", "qi_array.h", "qi_beam.h", "qi_adaptive.h", "qi_subspace.h", "qi_steer.h", "qi_windows.h", "qi_lags.h",
                 "qi_bands.h")
NAMES = {"qi_time_beam_power_scratch_bytes", "qi_time_beam_power", "qi_time_beam_traces"}


# ---- the header, the exports, the stream census ---------------------------------------------------------------------------------------
def test_library_exports_the_timebeam_header():
    from quantum_inferno_amd import _lib

    declared = set(header_functions(HEADER))
    assert declared == NAMES
    assert declared == set(_lib.TIMEBEAM_PROTOTYPES)
    for table in (_lib.PROTOTYPES, _lib.ARRAY_PROTOTYPES, _lib.BEAM_PROTOTYPES, _lib.ADAPTIVE_PROTOTYPES, _lib.SUBSPACE_PROTOTYPES,
                  _lib.STEER_PROTOTYPES, _lib.WINDOW_PROTOTYPES, _lib.LAG_PROTOTYPES, _lib.BAND_PROTOTYPES):
        assert not declared & set(table)
    for other in OTHER_HEADERS:
        assert not declared & set(header_functions(other)), other
    lib = _lib.load()
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in include/qi_timebeam.h but not exported"
        assert getattr(lib, name).argtypes == _lib.TIMEBEAM_PROTOTYPES[name][1], f"{name}: load() did not attach the table"
        assert len(_lib.TIMEBEAM_PROTOTYPES[name][1]) == len(header_functions(HEADER)[name].split(",")), name
    text = tb.header_text()
    assert '#include "qi_tfr.h"' in text and '#include "qi_beam.h"' in text and "Contract on the results" in text
    for name, value in (("QI_TIMEBEAM_MAX_PHASES", _lib.TIMEBEAM_MAX_PHASES), ("QI_TIMEBEAM_MAX_TAPS", max(_lib.TIMEBEAM_TAPS)),
                        ("QI_TIMEBEAM_LDS_MAX_SHIFT", tb.LDS_MAX_SHIFT), ("QI_TIMEBEAM_CHUNK", tb.CHUNK), ("QI_TIMEBEAM_ROW_BLOCK", tb.ROW_BLOCK)):
        assert re.search(rf"#define {name} {value}\b", text), name
    assert re.search(r"#define QI_TIMEBEAM_MAX_SHIFT \(1 << 20\)", text) and tb.MAX_SHIFT == _lib.TIMEBEAM_MAX_SHIFT == 1 << 20
    assert _lib.TIMEBEAM_LDS_MAX_SHIFT == tb.LDS_MAX_SHIFT and _lib.BEAM_MAX_SENSORS == tb.MAX_SENSORS
    with open(os.path.join(ROOT, "quantum_inferno_amd", "_build.py")) as fh:
        build = fh.read()
    assert '"qi_timebeam.h"' in build and '"qi_timebeam.hip"' in build
    with open(os.path.join(ROOT, "quantum_inferno_amd", "csrc", "qi_api_ops.hip")) as fh:
        assert '#include "qi_timebeam.h"' in fh.read()  # included where the other plan-less headers are


def test_every_stream_entry_point_has_a_case_and_nothing_else_is_named():
    import stream_order as so

    assert tsc.TABLE.header == HEADER
    assert stream_functions(HEADER) == ["qi_time_beam_power", "qi_time_beam_traces"]
    assert tsc.TABLE.named_functions() == stream_functions(HEADER)
    assert tsc.TABLE.ids() == ["time_beam_power-f64-hop-sums", "time_beam_traces-f32"]
    for case in tsc.TABLE.cases:
        assert len(case.functions) == 1 and callable(case.build) and case.asynchronous and case.engine is None, case.id
    assert tsc.HOP >= tb.CHUNK and tsc.WIN % tsc.HOP == 0 and tsc.ROWS > 2 * tb.ROW_BLOCK and tsc.SAMPLES % tb.CHUNK
    assert tsc.TABLE not in so.TABLES  # (that tuple's census is pinned elsewhere; these cases run in tests/test_gpu_timebeam.py)


def test_case_table_covers_what_the_kernel_branches_on():
    cases = tb.CASES
    assert {c.n for c in cases} >= {700, 2048, 3001} | {tb.CHUNK - 1, tb.CHUNK, tb.CHUNK + 1}
    assert {c.C for c in cases} == {2, 3, 5, 17, 64}
    assert {c.G for c in cases} >= {1, 7, 65, 257} | {tb.ROW_BLOCK - 1, tb.ROW_BLOCK, tb.ROW_BLOCK + 1}
    assert {(c.win, c.hop) for c in cases} >= {(64, 32), (100, 37), (1, 1), (2048, 1)}
    assert {c.win for c in cases} >= {tb.CHUNK - 1, tb.CHUNK, tb.CHUNK + 1}
    assert {(c.P, c.T) for c in cases} == set(tb.BANKS)
    # windows from per-hop sums (the hop divides the window and is a chunk or more) with one, two and more hops per window
    by_hop = [c for c in cases if c.win % c.hop == 0 and c.hop >= tb.CHUNK]
    assert {c.win // c.hop for c in by_hop} == {1, 2} and any(c.reach > tb.LDS_MAX_SHIFT for c in by_hop)
    assert {c.reach for c in cases} == {tb.SHIFT, tb.LDS_MAX_SHIFT, tb.LDS_MAX_SHIFT + 1, tb.MAX_SHIFT}
    assert len(set(tb.ids())) == len(cases) <= 24 and max(c.n for c in cases) <= 3001
    for c in cases:
        x, taps, shift, phase = tb.inputs(c.id)
        assert x.shape == (c.C, c.n) and taps.shape == (c.P, c.T) and shift.shape == phase.shape == (c.G, c.C)
        assert np.abs(shift).max() <= tb.SHIFT <= c.reach and phase.min() >= 0 and phase.max() < c.P
        # rows reach past both ends of the record
        assert (shift < 0).any() and (shift > 0).any() and c.win <= c.n


def test_peak_margins_hold_in_every_window(capsys):
    """What lets the GPU test hold peak_index to the restatement's in every window: the best value lies further above the
    runner-up than the float32 tolerance.  The one exception is the window of one sample, where a random row can tie the
    true one by chance: there the GPU test compares the windows whose margin holds, and this test counts them."""
    tol = tb.TOL["float32"]
    for c in tb.CASES:
        r = tb.restated(c.id)
        for name, power in (("mean square", r.mean_square), ("semblance", r.semblance)):
            m = tb.margins(power) / tb.largest(power)
            with capsys.disabled():
                print(f"timebeam margins {c.id:40s} {name:11s} smallest {m.min():.3g} of the largest value, {int((m > tol).sum())} of {len(m)} windows")
            if c.win == 1:
                assert (m > tol).mean() > 0.95, (c.id, name)
            else:
                assert m.min() > 100 * tol, (c.id, name)
                index, _ = tb.peaks_of(power)
                assert c.G == 1 or (index == tb.true_row(c)).all(), (c.id, name)
        assert np.isfinite(r.traces).all()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
GOOD = dict(dtype=None, C=3, n=1000, P=64, T=8, G=20, reach=60, win=100, hop=37)
SHAPE_REFUSALS = (
    (dict(dtype=7), "dtype"), (dict(C=1), "sensors"), (dict(C=0), "sensors"), (dict(C=65), "sensors"), (dict(P=0), "phases"),
    (dict(P=257), "phases"), (dict(T=0), "taps"), (dict(T=3), "taps"), (dict(T=32), "taps"), (dict(n=0), "bad shape"),
    (dict(G=0), "bad shape"), (dict(G=-1), "bad shape"), (dict(reach=-1), "max_shift"), (dict(reach=(1 << 20) + 1), "max_shift"),
    (dict(n=(1 << 40) + 1, win=1), "too large"), (dict(G=(1 << 40) + 1), "too large"),
)
POWER_REFUSALS = (
    (dict(win=0), "window"), (dict(win=1001), "window"), (dict(hop=0), "hop"), (dict(hop=-3), "hop"),
    (dict(n=1 << 30, win=1, hop=1, G=64), "too large"),  # 2^30 units x 4 row blocks: the grid passes 2^31 - 1
    (dict(n=1 << 32, win=1, hop=1, G=1), "too large"),   # 2^32 windows
)


def test_refusals_without_a_gpu():
    """Refused before the device is touched: the pointers are never followed (a host without a GPU runs this test).  The size
    query gives the call's status and message."""
    from quantum_inferno_amd import _lib

    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    base = ctypes.addressof(buf)
    p = ctypes.c_void_p(base)

    def at(offset):
        return ctypes.c_void_p(base + offset)

    def power(a, x=p, taps=p, shift=p, phase=p, out=p, index=p, value=p, scratch=p, nbytes=1 << 40):
        return lib.qi_time_beam_power(a["dtype"], 0, x, a["C"], a["n"], taps, a["P"], a["T"], shift, phase, a["G"], a["reach"], a["win"],
                                      a["hop"], 1, out, index, value, scratch, nbytes, None)

    def traces(a, x=p, taps=p, shift=p, phase=p, out=p):
        return lib.qi_time_beam_traces(a["dtype"], 0, x, a["C"], a["n"], taps, a["P"], a["T"], shift, phase, a["G"], a["reach"], out, None)

    def query(a):
        return lib.qi_time_beam_power_scratch_bytes(a["dtype"], a["C"], a["n"], a["P"], a["T"], a["G"], a["win"], a["hop"], a["reach"])

    for code in (_lib.QI_F32, _lib.QI_F64):
        good = {**GOOD, "dtype": code}
        for change, what in SHAPE_REFUSALS + POWER_REFUSALS:
            bad = {**good, **change}
            got = query(bad)
            msg = lib.qi_last_error()
            assert got < 0 and what in msg.decode(), (change, msg)
            assert power(bad) == got and lib.qi_last_error() == msg, change
        for change, what in SHAPE_REFUSALS:
            assert traces({**good, **change}) < 0 and what in lib.qi_last_error().decode(), (change, lib.qi_last_error())
        assert traces({**good, "n": 1 << 40, "G": 1 << 20}) < 0 and b"too large" in lib.qi_last_error()  # 2^32 x 2^16 workgroups
        # the size query's verdicts: [units][G][2] elements, rounded up to the library's alignment
        e = 4 if code == _lib.QI_F32 else 8
        nwin = tb.windows(good["n"], good["win"], good["hop"])
        need = query(good)
        assert nwin * good["G"] * 2 * e <= need < nwin * good["G"] * 2 * e + 512
        by_hop = query({**good, "n": 4096, "win": 1024, "hop": 256})  # 13 windows from 16 per-hop sums
        assert 16 * good["G"] * 2 * e <= by_hop < 16 * good["G"] * 2 * e + 512
        assert query({**good, "reach": 1 << 20}) == need and query({**good, "reach": 0, "P": 1, "T": 1}) == need
        for kw in (dict(x=None), dict(taps=None), dict(shift=None), dict(phase=None), dict(scratch=None)):
            assert power(good, **kw) < 0 and b"null" in lib.qi_last_error(), kw
        assert power(good, out=None, index=None, value=None) < 0 and b"nothing" in lib.qi_last_error()
        assert power(good, nbytes=need - 1) < 0 and b"scratch" in lib.qi_last_error()
        assert power(good, nbytes=0) < 0 and b"scratch" in lib.qi_last_error()
        for kw in (dict(x=at(2)), dict(taps=at(1)), dict(shift=at(2)), dict(phase=at(1)), dict(out=at(2)), dict(index=at(4)),
                   dict(value=at(3)), dict(scratch=at(8))):
            assert power(good, **kw) < 0 and b"misaligned" in lib.qi_last_error(), kw
        for kw in (dict(x=None), dict(taps=None), dict(shift=None), dict(phase=None)):
            assert traces(good, **kw) < 0 and b"null" in lib.qi_last_error(), kw
        assert traces(good, out=None) < 0 and b"nothing" in lib.qi_last_error()
        for kw in (dict(x=at(2)), dict(taps=at(1)), dict(shift=at(2)), dict(phase=at(1)), dict(out=at(2))):
            assert traces(good, **kw) < 0 and b"misaligned" in lib.qi_last_error(), kw
    f64 = {**GOOD, "dtype": _lib.QI_F64}
    assert power(f64, x=at(4)) < 0 and b"misaligned" in lib.qi_last_error()
    assert traces(f64, out=at(4)) < 0 and b"misaligned" in lib.qi_last_error()


# ---- the host helpers -----------------------------------------------------------------------------------------------------------------
def test_delay_bank_is_the_restated_bank():
    from quantum_inferno_amd import engine

    for P, T in tb.BANKS + ((7, 4), (256, 16), (1, 2)):
        for beta in (5.0, 8.6):
            got = engine.delay_bank(P, T, beta, "float64")
            want = tb.bank(P, T, beta)
            assert tuple(got.shape) == (P, T) and not got.is_cuda
            assert np.array_equal(got.numpy(), want), (P, T, beta)  # bit for bit
            impulse = np.zeros(T)
            impulse[(T - 1) // 2] = 1.0
            assert np.array_equal(want[0], impulse)
            assert np.abs(want.sum(axis=1) - 1.0).max() <= 1e-15
            assert np.array_equal(engine.delay_bank(P, T, beta, "float32").numpy(), want.astype(np.float32))
    # half a sample: the symmetric filter; a quarter and three quarters mirror each other
    h = tb.bank(64, 8)
    assert np.allclose(h[32], h[32][::-1], atol=1e-16) and np.allclose(h[16][1:], h[48][::-1][1:], atol=1e-3)
    assert engine.delay_bank().shape == (64, 8) and engine.delay_bank().dtype.is_floating_point
    for bad in (dict(phases=2, taps=1), dict(taps=3), dict(phases=0), dict(phases=257), dict(taps=32)):
        with pytest.raises(ValueError):
            engine.delay_bank(**bad)


def test_quantize_delays_is_the_restatement():
    from quantum_inferno_amd import engine

    rate, P = 800.0, 64
    tau = np.array([[0.0, -0.0834, 0.0667], [0.5 / (rate * P), -0.5 / (rate * P), 1.5 / (rate * P)],  # half-way: rounds up
                    [1234.5678, -987.654321, 1.0 / rate], [-1.0 / rate, -1.0 / (rate * P), 63.0 / (rate * P)]])
    shift, phase, reach = engine.quantize_delays(tau, rate, P, device="cpu")
    ws, wp, wr = tb.quantize(tau, rate, P)
    assert shift.dtype == phase.dtype == __import__("torch").int32 and isinstance(reach, int)
    assert np.array_equal(shift.numpy(), ws) and np.array_equal(phase.numpy(), wp) and reach == wr == 987654
    assert phase.min() >= 0 and phase.max() < P
    assert shift[1].tolist() == [0, 0, 0] and phase[1].tolist() == [1, 0, 2]
    assert shift[3].tolist() == [-1, -1, 0] and phase[3].tolist() == [0, 63, 63]
    assert np.array_equal((ws * P + wp) / (rate * P), np.floor(tau * rate * P + 0.5) / (rate * P))
    s1, p1, r1 = engine.quantize_delays(tau, rate, 1, device="cpu")  # whole samples
    assert not p1.any() and np.array_equal(s1.numpy(), np.floor(tau * rate + 0.5).astype(np.int64)) and r1 == 987654
    # the plane-wave grid of tests/beam_cases.py: delays of up to 53 samples at the source's slowness
    shift, phase, reach = tb.pw_tables(64)
    assert np.abs(shift[tb.pw_true_index()]).max() in (53, 54) and reach < 120
    with pytest.raises(ValueError):
        engine.quantize_delays(np.zeros(3), rate, P, device="cpu")
    with pytest.raises(ValueError):
        engine.quantize_delays(np.array([[np.nan, 0.0]]), rate, P, device="cpu")


# ---- the restatement itself -------------------------------------------------------------------------------------------------------------
def test_restatement_against_a_convolution():
    """One row, one sensor pair: y is numpy.convolve of the zero-extended record with the reversed filter, shifted."""
    rng = np.random.default_rng(20261021)
    n, T, P = 300, 8, 64
    x = rng.standard_normal((2, n))
    taps = tb.bank(P, T)
    shift, phase = np.array([[17, -23]]), np.array([[5, 40]])
    y = tb.delayed(x, taps, shift[0], phase[0])
    c = (T - 1) // 2
    for i in range(2):
        full = np.convolve(np.concatenate([np.zeros(100), x[i], np.zeros(100)]), taps[phase[0, i]][::-1])  # full[j] = sum_m h[m] z[j - (T - 1) + m]
        want = full[100 + shift[0, i] - c + T - 1:][:n]
        assert np.abs(y[i] - want).max() < 1e-14
    r = tb.restate(x, taps, shift, phase, 23, 50, 25)
    b = y.sum(axis=0)
    assert np.allclose(r.traces[0], b / 2) and r.semblance.shape == (11, 1)
    assert np.allclose(r.mean_square[3, 0], np.sum(b[75:125] ** 2) / (4 * 50))
    assert np.allclose(r.semblance[3, 0], np.sum(b[75:125] ** 2) / (2 * np.sum(y[:, 75:125] ** 2)))
    assert np.isnan(tb.restate(x, taps, shift, phase, 22, 50, 25).traces).all()  # |shift| beyond max_shift
    assert np.isnan(tb.restate(x, taps, shift, np.array([[5, 64]]), 23, 50, 25).semblance).all()
    # a NaN under a zero tap still poisons; a sample no tap reads does not
    xn = x.copy()
    xn[0, 40] = np.nan
    yn = tb.delayed(xn, taps, np.array([0, 0]), np.array([0, 0]))  # the impulse: seven taps are zero
    assert np.isnan(yn[0]).sum() == T and not np.isnan(yn[1]).any()
    read = tb.samples_read(n, T, shift, phase, P, 23)
    assert not read[0, :17 - c].any() and read[0, 17 - c:].all() and read[1, :n - 23 + T - 1 - c].all() and not read[1, n - 23 + T - 1 - c:].any()
    # the exact cases stay below 2^24, and a row wholly off the record is zero
    for C in (2, 4, 16):
        x, shift, phase = tb.exact_inputs(C)
        traces, power = tb.exact_restate(x, shift, 64, 32)
        assert not traces[-1].any() and not power[:, -1].any() and np.array_equal(traces[0], x.mean(axis=0))
        r = tb.restate(x, np.ones((1, 1)), shift, phase, x.shape[1], 64, 32)
        assert np.array_equal(r.traces, traces) and np.array_equal(r.mean_square, power) and np.isnan(r.semblance[:, -1]).all()


# ---- the plane wave -----------------------------------------------------------------------------------------------------------------------
def test_plane_wave_detector_in_the_restatement(capsys):
    """The F detector on the plane wave of tests/beam_cases.py: the semblance peaks at the source's slowness in every window, by
    PW_MARGIN at least (measured: 0.66, 0.52 and 0.385 for the three windows with the 64 x 8 bank; whole-sample delays keep the
    peak too)."""
    assert [tb.windows(tb.PW_N, w, h) for w, h in tb.PW_WINDOWS] == [31, 109, 127]
    for win, hop in tb.PW_WINDOWS:
        for P, T in (tb.PW_BANK, (1, 1)):
            r = tb.pw_restated(win, hop, P, T)
            index, value = tb.peaks_of(r.semblance)
            margin = float(tb.margins(r.semblance).min())
            with capsys.disabled():
                print(f"timebeam plane wave win {win} hop {hop} bank {P} x {T}: margin over the runner-up {margin:.3f}, peak {value.min():.3f} .. {value.max():.3f}")
            assert (index == tb.pw_true_index()).all(), (win, hop, P, T)
            assert margin >= tb.PW_MARGIN, (win, hop, P, T)
            assert np.nanmax(r.semblance) <= 1.0 + 1e-12 and np.nanmin(r.semblance) >= 0.0


def test_plane_wave_traces_in_the_restatement(capsys):
    """The trace at the source's slowness lies at the records' own noise floor once the content is below half of Nyquist
    (0.0455 of the source's RMS; the floor 0.1 sqrt(0.5) / sqrt(5) over the source's RMS there is 0.0457), the centre trace far
    from it (0.89).  On the full-band white records the interpolator's roll-off near Nyquist shows: 0.158 with 8 taps, 0.120
    with 16 -- the documented limit."""
    rows, (shift, phase, reach) = tb.pw_steer_tables(tb.PW_BANK[0])
    records, source = tb.pw_low_passed()
    traces = tb.restate(records, tb.bank(*tb.PW_BANK), shift, phase, reach, tb.PW_N, 1).traces
    at_source, at_centre = tb.rms_from(traces[0], source), tb.rms_from(traces[1], source)
    floor = 0.1 * np.sqrt(0.5) / np.sqrt(5) / np.sqrt(np.mean(source[tb.PW_INTERIOR:-tb.PW_INTERIOR] ** 2))
    white = {T: tb.relative_rms(tb.restate(tb.pw_records(), tb.bank(64, T), shift, phase, reach, tb.PW_N, 1).traces[0], tb.PW_INTERIOR) for T in (8, 16)}
    with capsys.disabled():
        print(f"timebeam plane wave traces: low-passed {at_source:.4f} at the source (floor {floor:.4f}), {at_centre:.3f} at the centre; "
              f"white records {white[8]:.3f} with 8 taps, {white[16]:.3f} with 16")
    assert at_source <= 0.05 and at_centre >= 0.8
    assert 0.04 < floor < 0.05 and white[16] < white[8] < 0.2
