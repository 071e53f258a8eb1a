"""Capon beamforming without a GPU: the exports of include/qi_adaptive.h and the census of tests/adaptive_stream_cases.py
against that header, the size query's verdicts against qi_beam_power_scratch_bytes', qi_csd_whiten's refusals, the NumPy
restatements of tests/capon_cases.py against their identities (V^H R V = I, 1 / Re e^H inv(R) e, Capon <= Bartlett), the
plane-wave case, the float32 restatements' distance from the float64 ones, the exact case's integers and `info`."""
import ctypes
import os

import numpy as np

import adaptive_stream_cases as asc
import beam_cases as bc
import capon_cases as cpc
import csd_cases as cc
from stream_table import header_functions, stream_functions

ROOT = bc.ROOT
HEADER = "qi_adaptive.h"


def test_library_exports_the_adaptive_header():
    from quantum_inferno_amd import _lib

    declared = set(header_functions(HEADER))
    assert declared == {"qi_csd_whiten", "qi_beam_capon_scratch_bytes", "qi_beam_capon"}
    assert declared == set(_lib.ADAPTIVE_PROTOTYPES)
    for table in (_lib.PROTOTYPES, _lib.ARRAY_PROTOTYPES, _lib.BEAM_PROTOTYPES):
        assert not declared & set(table)
    for other in ("qi_tfr.h", "qi_array.h", "qi_beam.h"):
        assert not declared & set(header_functions(other)), other
    lib = _lib.load()
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in include/qi_adaptive.h but not exported"
        assert len(_lib.ADAPTIVE_PROTOTYPES[name][1]) == len(header_functions(HEADER)[name].split(",")), name
    with open(os.path.join(ROOT, "include", "qi_adaptive.h")) as fh:
        text = fh.read()
    assert '#include "qi_tfr.h"' in text and "LOWER" in text  # the types; that only the lower triangle is read


def test_every_stream_entry_point_has_a_case_and_nothing_else_is_named():
    assert asc.TABLE.header == HEADER
    assert stream_functions(HEADER) == ["qi_beam_capon", "qi_csd_whiten"]
    assert asc.TABLE.named_functions() == stream_functions(HEADER)


def test_stream_case_table():
    assert asc.TABLE.ids() == ["whiten-info", "capon-bins", "capon-bands-peaks"]
    for case in asc.TABLE.cases:
        assert case.functions and callable(case.build) and case.asynchronous and case.engine is None, case.id
    for a in asc.definite_pair("float64", (47, 0)):
        assert np.linalg.eigvalsh(a).min() >= 1.0 and np.array_equal(a, np.conj(np.swapaxes(a, 1, 2)))


def test_size_query_verdicts_are_the_beam_power_ones():
    from quantum_inferno_amd import _lib

    lib = _lib.load()
    for shape in ((_lib.QI_F64, 64, 33, 300, 4), (_lib.QI_F32, 1, 1, 1, 1), (_lib.QI_F64, 0, 33, 300, 4), (_lib.QI_F64, 65, 33, 300, 4),
                  (_lib.QI_F64, 64, 33, 0, 4), (_lib.QI_F64, 64, 33, 300, 0), (_lib.QI_F64, 64, 0, 300, 4), (7, 64, 33, 300, 4),
                  (_lib.QI_F32, 5, 7, 15, 8), (_lib.QI_F32, 5, 1 << 40, 15, 2)):
        want = lib.qi_beam_power_scratch_bytes(*shape)
        want_msg = lib.qi_last_error() if want < 0 else None
        got = lib.qi_beam_capon_scratch_bytes(*shape)
        assert got == want, shape
        if want < 0:
            assert lib.qi_last_error() == want_msg and want_msg, shape
    assert lib.qi_beam_capon_scratch_bytes(_lib.QI_F64, 64, 33, 300, 4) > 0 > lib.qi_beam_capon_scratch_bytes(_lib.QI_F64, 65, 33, 300, 4)


def test_whiten_refusals_without_a_gpu():
    """Refused before the device is touched: the pointers are never followed (this machine may have no GPU at all)."""
    from quantum_inferno_amd import _lib

    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    good = dict(dtype=_lib.QI_F32, C=2, nf=1, loading=0.0)
    for change, what in ((dict(C=0), "sensors"), (dict(C=65), "sensors"), (dict(nf=0), "matrices"), (dict(loading=-1e-3), "loading"),
                         (dict(loading=float("nan")), "loading"), (dict(loading=float("inf")), "loading"), (dict(dtype=7), "dtype")):
        a = {**good, **change}
        rc = lib.qi_csd_whiten(a["dtype"], 0, p, a["C"], a["nf"], a["loading"], p, None, None)
        assert rc < 0, change
        assert what in lib.qi_last_error().decode(), (change, lib.qi_last_error())
    assert lib.qi_csd_whiten(_lib.QI_F32, 0, None, 2, 1, 0.0, p, None, None) < 0 and b"null" in lib.qi_last_error()
    assert lib.qi_csd_whiten(_lib.QI_F32, 0, p, 2, 1, 0.0, None, None, None) < 0 and b"null" in lib.qi_last_error()
    odd = ctypes.c_void_p(ctypes.addressof(buf) + 4)
    assert lib.qi_csd_whiten(_lib.QI_F32, 0, odd, 2, 1, 0.0, p, None, None) < 0 and b"misaligned" in lib.qi_last_error()
    assert lib.qi_csd_whiten(_lib.QI_F32, 0, p, 2, 1, 0.0, p, ctypes.c_void_p(ctypes.addressof(buf) + 2), None) < 0
    assert b"misaligned" in lib.qi_last_error()


def test_restatement_identities():
    for shape in bc.SHAPES:
        s, freq, tau = cpc.inputs(shape, np.float64)
        assert np.array_equal(s, np.conj(np.swapaxes(s, 1, 2)))
        r = cpc.loaded(s, cpc.LOADING)
        eig = np.linalg.eigvalsh(r)
        assert eig.min() > 0 and (eig.max(axis=1) / eig.min(axis=1)).max() < 100.0, shape.id
        if shape.C > 1:
            plain = np.linalg.eigvalsh(s)
            assert np.allclose(plain[:, 0], 1.0, rtol=1e-10) and np.allclose(plain[:, -1], 100.0, rtol=1e-10), shape.id
        v = cpc.whiten(s, cpc.LOADING)
        assert np.array_equal(v, np.triu(v)) and cpc.residual(v, r) <= 1e-12, shape.id
        steps, info = cpc.whiten_steps(s, cpc.LOADING, np.float64)  # the kernel's algorithm in double: the same factor
        assert not info.any() and np.abs(steps - v).max() <= 1e-12 * np.abs(v).max(), shape.id
        got = cpc.capon(v, freq, tau, shape.bands)
        e = np.exp(2j * np.pi * freq[:, None, None] * tau[None, :, :])  # (not reduced: the other way to the same phase)
        d = np.real(np.einsum("fgi,fij,fgj->fg", np.conj(e), np.linalg.inv(r), e))
        first = bc.band_table(shape.bands, shape.nf)
        want = np.stack([(1.0 / d[a:b]).sum(axis=0) for a, b in zip(first[:-1], first[1:])])
        assert np.allclose(got, want, rtol=1e-9, atol=0), shape.id
        bartlett = cpc.bartlett_of_loaded(s, cpc.LOADING, freq, tau, shape.bands)
        assert np.all(got <= bartlett * (1 + 1e-12)), shape.id  # Cauchy-Schwarz: 1 / (e^H inv(R) e) <= e^H R e / C^2


def test_plane_wave_in_the_restatements():
    case = bc.pw_case()
    freq = np.fft.rfftfreq(case.nfft, 1 / bc.PW_FS)
    tau = bc.pw_delays()
    true = bc.pw_true_index()
    s = cc.restate(bc.pw_records(), case, "spectrum")
    assert cc.segments(case) == 31 and s.shape[1] == 5
    power = cpc.capon(cpc.whiten(s, cpc.LOADING), freq, tau, bc.PW_BANDS)
    bartlett = cpc.bartlett_of_loaded(s, cpc.LOADING, freq, tau, bc.PW_BANDS)
    assert power.shape == (4, 81) and np.all(power <= bartlett * (1 + 1e-12))
    worst = np.inf
    for b in range(4):
        at, ratio = cpc.peak_ratio(power[b])
        at_b, ratio_b = cpc.peak_ratio(bartlett[b])
        print(f"plane wave, band {b}: Capon peak / runner-up {ratio:.2f} at {at}; Bartlett {ratio_b:.2f} at {at_b}")
        assert at == true and at_b == true, b
        assert ratio >= cpc.PW_RATIO, b
        worst = min(worst, ratio)
    assert 4.5 <= worst <= 4.6  # the measured worst, band 3: 4.56
    p32 = cpc.capon32(cpc.whiten32(s, cpc.LOADING), freq, tau, bc.PW_BANDS)
    assert p32.dtype == np.float32 and np.array_equal(np.argmax(p32, axis=1), np.full(4, true))


def test_float32_restatement_deviation():
    worst_p, worst_r, at_p, at_r = 0.0, 0.0, None, None
    for shape in bc.SHAPES:
        s, freq, tau = cpc.inputs(shape, np.float32)
        r = cpc.loaded(s, cpc.LOADING, np.float32)
        ref = cpc.capon(cpc.whiten(s, cpc.LOADING, np.float32), freq, tau, shape.bands)
        v32 = cpc.whiten32(s, cpc.LOADING)
        got = cpc.capon32(v32, freq, tau, shape.bands)
        assert v32.dtype == np.complex64 and got.dtype == np.float32 and got.shape == ref.shape and np.isfinite(ref).all()
        err = float(np.abs(got - ref).max() / np.abs(ref).max())
        res = cpc.residual(v32, r)
        print(f"{shape.id}: float32 restatement against float64: power {err:.4g}, max |V^H R V - I| {res:.4g}")
        assert err <= bc.TOL["float32"] / 16 and res <= bc.TOL["float32"] / 16, shape.id
        if err > worst_p:
            worst_p, at_p = err, shape.id
        if res > worst_r:
            worst_r, at_r = res, shape.id
    print(f"largest: power {worst_p:.4g} ({at_p}), the constant {cpc.CAPON32_RESTATEMENT:g}; residual {worst_r:.4g} ({at_r}), the constant "
          f"{cpc.WHITEN32_RESIDUAL:g}; bound {bc.TOL['float32'] / 16:g}")
    assert worst_p <= cpc.CAPON32_RESTATEMENT <= 1.05 * worst_p, worst_p  # the constants are the measurements, rounded up
    assert worst_r <= cpc.WHITEN32_RESIDUAL <= 1.05 * worst_r, worst_r
    assert max(cpc.CAPON32_RESTATEMENT, cpc.WHITEN32_RESIDUAL) <= bc.TOL["float32"] / 16


def test_exact_case_is_exact():
    """The GPU test's expectation stands on integers: every pivot 1, every entry of V a unit, every D an integer."""
    nf, G = 33, 37
    for C in (17, 33):
        s, low, freq, tau, turns4 = cpc.exact_inputs(C, nf, G)
        assert np.array_equal(s, np.conj(np.swapaxes(s, 1, 2))) and np.array_equal(s, np.rint(s.real) + 1j * np.rint(s.imag))
        assert np.abs(s).max() <= 2 and set(np.unique(np.abs(np.diagonal(low, -1, 1, 2)))) == {1.0}
        assert len(np.unique(np.diagonal(low, -1, 1, 2))) == 4
        upper = np.triu(np.ones((C, C), dtype=bool))
        want = cpc.whiten(s, 0.0)
        for dtype in (np.float32, np.float64):
            v, info = cpc.whiten_steps(s, 0.0, dtype)  # in float32 arithmetic too
            assert not info.any() and np.array_equal(v, want), (C, dtype)
            assert np.array_equal(np.abs(v)[:, upper], np.ones((nf, upper.sum()))) and not v[:, ~upper].any()
            assert np.array_equal(v, np.rint(v.real) + 1j * np.rint(v.imag))
        assert np.array_equal(4 * bc.reduced_turns(freq, tau) % 4, turns4 % 4)
        e = cpc.exact_factors(turns4)
        w = np.einsum("fij,fgi->fgj", np.conj(want), e)
        d = (w.real ** 2 + w.imag ** 2).sum(axis=-1)
        assert np.array_equal(d, np.rint(d)) and 0 < d.min() and d.max() <= sum(j * j for j in range(1, C + 1)) <= 12529
        power = cpc.capon(want, freq, tau, (0, 3, 4, 33), e=e)
        assert np.isfinite(power).all() and power.shape == (3, G)


def test_info_restated():
    for C in (5, 17):
        for name, matrix, loading, want in cpc.info_cases(C):
            for dtype in (np.float32, np.float64):
                v, info = cpc.whiten_steps(matrix[None], loading, dtype)
                assert info.dtype == np.int32 and info[0] == want, (name, C, dtype, info)
                upper = np.triu(np.ones((C, C), dtype=bool))
                if want:
                    assert np.isnan(v[0][upper].real).all() and np.isnan(v[0][upper].imag).all() and not v[0][~upper].any(), name
                else:
                    assert cpc.residual(v, cpc.loaded(matrix[None], loading)) <= 1e-5, name
