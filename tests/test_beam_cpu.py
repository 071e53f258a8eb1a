"""Beamforming without a GPU: the exports of include/qi_beam.h and the census of tests/beam_stream_cases.py against that
header, the size query's verdicts, the NumPy restatement of qi_beam_power (tests/beam_cases.py) against delay-and-sum in the
frequency domain, the plane-wave case in the restatements, and the float32 restatement's distance from the float64 one."""
import os
import re

import numpy as np

import beam_cases as bc
import beam_stream_cases as bsc
import csd_cases as cc
from stream_table import header_functions, stream_functions

ROOT = bc.ROOT
HEADER = "qi_beam.h"


def test_library_exports_the_beam_header():
    from quantum_inferno_amd import _lib

    declared = set(header_functions(HEADER))
    assert declared == {"qi_beam_power_scratch_bytes", "qi_beam_power"}
    assert declared == set(_lib.BEAM_PROTOTYPES)
    assert not declared & set(_lib.PROTOTYPES) and not declared & set(_lib.ARRAY_PROTOTYPES)
    assert not declared & set(header_functions("qi_array.h")) and not declared & set(header_functions("qi_tfr.h"))
    lib = _lib.load()
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in include/qi_beam.h but not exported"
    with open(os.path.join(ROOT, "include", "qi_beam.h")) as fh:
        assert re.search(r"#define\s+QI_BEAM_MAX_SENSORS\s+%d\b" % _lib.BEAM_MAX_SENSORS, fh.read())
    assert _lib.BEAM_MAX_SENSORS == bc.MAX_SENSORS == 64


def test_size_query_verdicts_without_a_gpu():
    from quantum_inferno_amd import _lib

    lib = _lib.load()
    query = lib.qi_beam_power_scratch_bytes
    good = (_lib.QI_F64, 64, 33, 300, 4)
    size = query(*good)
    assert size > 0 and size % 256 == 0 and size >= 33 * 8 + 5 * 8
    for bad, what in (((_lib.QI_F64, 0, 33, 300, 4), "C = 0"), ((_lib.QI_F64, 65, 33, 300, 4), "C = 65"),
                      ((_lib.QI_F64, 64, 33, 0, 4), "G = 0"), ((_lib.QI_F64, 64, 33, 300, 0), "nb = 0"),
                      ((_lib.QI_F64, 64, 0, 300, 4), "nf = 0"), ((7, 64, 33, 300, 4), "dtype 7")):
        assert query(*bad) < 0, what
        assert lib.qi_last_error(), what
    assert query(_lib.QI_F32, 1, 1, 1, 1) > 0


def test_every_stream_entry_point_has_a_case_and_nothing_else_is_named():
    assert bsc.TABLE.header == HEADER
    assert stream_functions(HEADER) == ["qi_beam_power"]
    assert bsc.TABLE.named_functions() == stream_functions(HEADER)


def test_stream_case_table():
    assert bsc.TABLE.ids() == ["beam-bins", "beam-bands-semblance-peaks"]
    for case in bsc.TABLE.cases:
        assert case.functions and callable(case.build) and case.asynchronous and case.engine is None, case.id


def test_shape_cases_touch_every_value():
    assert {s.C for s in bc.SHAPES} == {1, 5, 16, 17, 33, 64}
    assert {s.G for s in bc.SHAPES} == {1, 15, 16, 17, 37, 300}
    assert {s.nf for s in bc.SHAPES} == {1, 7, 33}
    assert {s.bands for s in bc.SHAPES} == {None, (0, 1, 7), (0, 3, 4, 33)}
    assert len(bc.SHAPES) == len(set(bc.ids())) == 12
    for s in bc.SHAPES:
        assert s.bands is None or s.bands[-1] <= s.nf


def test_restatement_is_delay_and_sum_of_one_segment():
    """One segment: S_ij = w conj(X_i) X_j, so Q = w |sum_j X_j e_j|^2 -- the coefficients steered and summed, no matrix."""
    case = cc.by_id("c2_n256_one_segment")
    assert cc.segments(case) == 1
    x = cc.records(case).astype(np.float64)
    z = cc.panel(x, case)[:, :, 0]  # [C, nf]
    s = cc.restate(x, case, "spectrum")
    w = cc.bin_weights(case.nfft, 1, cc.scale2(cc.window_of(case), "spectrum"))
    freq = np.fft.rfftfreq(case.nfft, 1 / cc.FS)
    tau = np.random.default_rng(5).uniform(-bc.MAX_DELAY_S, bc.MAX_DELAY_S, (37, case.C))
    e = np.exp(2j * np.pi * freq[:, None, None] * tau[None, :, :])  # (not reduced: the other way to the same phase)
    want = w[:, None] * np.abs(np.einsum("jf,fgj->fg", z, e)) ** 2 / case.C ** 2
    got = bc.restate(s, freq, tau)
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"restatement against delay-and-sum of one segment: max |d| / max = {err:.3g}")
    assert err <= 1e-13
    # and the bands are sums of bins, the semblance their quotient by C tr S
    first = [0, 3, 4, 33, 129]
    band = bc.restate(s, freq, tau, first)
    assert np.allclose(band, np.stack([want[a:b].sum(axis=0) for a, b in zip(first[:-1], first[1:])]), rtol=1e-12, atol=0)
    sem = bc.restate(s, freq, tau, first, normalize=True)
    tr = np.real(np.einsum("fii->f", s))
    assert np.allclose(sem * np.array([tr[a:b].sum() for a, b in zip(first[:-1], first[1:])])[:, None] / case.C, band, rtol=1e-12, atol=0)
    assert sem.max() <= 1 + 1e-12 and sem.min() >= -1e-12


def test_plane_wave_in_the_restatements():
    case = bc.pw_case()
    x = bc.pw_records()
    freq = np.fft.rfftfreq(case.nfft, 1 / bc.PW_FS)
    tau = bc.pw_delays()
    true = bc.pw_true_index()
    assert tau.shape == (81, 5) and true == 25 and np.allclose(bc.pw_slowness()[true], (2.25e-3, -1.5e-3))
    assert 50.0 <= np.ptp(bc.PW_POSITIONS_M, axis=0).max() <= 70.0
    s = cc.restate(x, case, "spectrum")
    sem = bc.restate(s, freq, tau, bc.PW_BANDS, normalize=True)
    assert sem.shape == (4, 81)
    for b, row in enumerate(sem):
        order = np.argsort(row)
        print(f"plane wave, band {b}: best semblance {row[order[-1]]:.3f} at {order[-1]}, runner-up {row[order[-2]]:.3f}")
        assert order[-1] == true, b
        assert row[order[-1]] >= row[order[-2]] + bc.PW_MARGIN, b
    sem32 = bc.restate32(s, freq, tau, bc.PW_BANDS, normalize=True)
    assert sem32.dtype == np.float32 and np.array_equal(np.argmax(sem32, axis=1), np.full(4, true))
    az, v = bc.pw_true_azimuth_velocity()
    assert abs(az - 303.69) < 0.01 and abs(v - 369.8) < 0.1


def test_float32_restatement_deviation():
    worst, at = 0.0, None
    for shape in bc.SHAPES:
        s, freq, tau = bc.inputs(shape, np.float32)
        for normalize in (False, True):
            ref = bc.restate(s, freq, tau, shape.bands, normalize)
            got = bc.restate32(s, freq, tau, shape.bands, normalize)
            assert got.dtype == np.float32 and got.shape == ref.shape and np.isfinite(ref).all()
            err = float(np.abs(got - ref).max() / (1.0 if normalize else np.abs(ref).max()))
            print(f"{shape.id} {'semblance' if normalize else 'power'}: float32 restatement against float64: {err:.4g}")
            assert err <= bc.TOL["float32"] / 16, shape.id
            if err > worst:
                worst, at = err, shape.id
    print(f"largest: {worst:.4g} ({at}); the constant {bc.BEAM32_RESTATEMENT:g}; bound {bc.TOL['float32'] / 16:g}")
    assert worst <= bc.BEAM32_RESTATEMENT <= 1.05 * worst, worst  # the constant is the measurement, rounded up
    assert bc.BEAM32_RESTATEMENT <= bc.TOL["float32"] / 16


def test_exact_case_is_exact():
    """The GPU test's expectation stands on integers: every factor a unit, every sum below 2^24."""
    for C in (17, 33):
        s, freq, tau, turns4 = bc.exact_inputs(C, 33, 37)
        assert np.array_equal(s, np.conj(np.swapaxes(s, 1, 2))) and np.abs(s.real).max() <= 8 and np.abs(s.imag).max() <= 8
        assert not np.array_equal(s.real, np.swapaxes(s.real, 1, 2)[:, ::-1, ::-1])
        assert np.array_equal(4 * bc.reduced_turns(freq, tau) % 4, turns4 % 4)
        assert set(np.unique(turns4)) == {0, 1, 2, 3}
        q, tr = bc.exact_sums(s, turns4, (0, 3, 4, 33))
        assert np.array_equal(bc.restate(s, freq, tau, (0, 3, 4, 33)), q / C ** 2)
