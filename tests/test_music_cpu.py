"""MUSIC beamforming without a GPU: the exports of include/qi_subspace.h and the census of tests/subspace_stream_cases.py
against that header, qi_csd_eigh's refusals, the size query's verdicts against qi_beam_power_scratch_bytes', qi_beam_music's
verdict on n_sources, the NumPy restatements of tests/music_cases.py against their identities (U^H U = I, S U = U diag(w),
C n_b / sum Re e^H (I - U_s U_s^H) e), the float32 restatements' distance from the float64 ones, the plane-wave case and a
two-wave case, the exact (diagonal) cases and `info`."""
import ctypes
import functools
import os

import numpy as np

import beam_cases as bc
import capon_cases as cpc
import csd_cases as cc
import music_cases as mc
import subspace_stream_cases as ssc
from stream_table import header_functions, stream_functions

ROOT = bc.ROOT
HEADER = "qi_subspace.h"
OTHER_HEADERS = ("qi_tfr.h", "qi_array.h", "qi_beam.h", "qi_adaptive.h")
STEPS64_MATRICES = 5  # matrices of a stack the kernel's algorithm is restated on in double (each is solved alone)


# ---- 1, 2: the header, the exports, the stream census ---------------------------------------------------------------------------------
def test_library_exports_the_subspace_header():
    from quantum_inferno_amd import _lib

    declared = set(header_functions(HEADER))
    assert declared == {"qi_csd_eigh", "qi_beam_music_scratch_bytes", "qi_beam_music"}
    assert declared == set(_lib.SUBSPACE_PROTOTYPES)
    for table in (_lib.PROTOTYPES, _lib.ARRAY_PROTOTYPES, _lib.BEAM_PROTOTYPES, _lib.ADAPTIVE_PROTOTYPES):
        assert not declared & set(table)
    for other in OTHER_HEADERS:
        assert not declared & set(header_functions(other)), other
    lib = _lib.load()
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in include/qi_subspace.h but not exported"
        assert len(_lib.SUBSPACE_PROTOTYPES[name][1]) == len(header_functions(HEADER)[name].split(",")), name
    with open(os.path.join(ROOT, "include", "qi_subspace.h")) as fh:
        text = fh.read()
    assert '#include "qi_tfr.h"' in text and '#include "qi_beam.h"' in text and "LOWER" in text  # that only the lower triangle is read


def test_every_stream_entry_point_has_a_case_and_nothing_else_is_named():
    assert ssc.TABLE.header == HEADER
    assert stream_functions(HEADER) == ["qi_beam_music", "qi_csd_eigh"]
    assert ssc.TABLE.named_functions() == stream_functions(HEADER)


def test_stream_case_table():
    by_id = ssc.TABLE.by_id
    assert ssc.TABLE.ids() == ["eigh-info", "music-bins", "music-bands-peaks"]
    for case in ssc.TABLE.cases:
        assert case.functions and callable(case.build) and case.asynchronous and case.engine is None, case.id
    dtypes = {c.id: c.build.args[0] for c in ssc.TABLE.cases}
    assert dtypes == {"eigh-info": "float32", "music-bins": "float64", "music-bands-peaks": "float32"}
    assert by_id("music-bins").build.args[1:] == (None, False) and by_id("music-bands-peaks").build.args[1:] == ((0, 3, 4, 33), True)
    assert 0 <= ssc.SOURCES < ssc.SENSORS


# ---- 3: refusals ----------------------------------------------------------------------------------------------------------------------
def test_eigh_refusals_without_a_gpu():
    """Refused before the device is touched: the pointers are never followed (this machine may have no GPU at all)."""
    from quantum_inferno_amd import _lib

    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    good = dict(dtype=_lib.QI_F32, C=2, nf=1)
    for change, what in ((dict(C=0), "sensors"), (dict(C=65), "sensors"), (dict(nf=0), "matrices"), (dict(dtype=7), "dtype")):
        a = {**good, **change}
        rc = lib.qi_csd_eigh(a["dtype"], 0, p, a["C"], a["nf"], p, p, None, None)
        assert rc < 0, change
        assert what in lib.qi_last_error().decode(), (change, lib.qi_last_error())
    for args in ((None, p, p), (p, None, p), (p, p, None)):
        assert lib.qi_csd_eigh(_lib.QI_F32, 0, args[0], 2, 1, args[1], args[2], None, None) < 0 and b"null" in lib.qi_last_error()
    odd = ctypes.c_void_p(ctypes.addressof(buf) + 4)
    assert lib.qi_csd_eigh(_lib.QI_F32, 0, odd, 2, 1, p, p, None, None) < 0 and b"misaligned" in lib.qi_last_error()
    assert lib.qi_csd_eigh(_lib.QI_F32, 0, p, 2, 1, p, odd, None, None) < 0 and b"misaligned" in lib.qi_last_error()
    assert lib.qi_csd_eigh(_lib.QI_F64, 0, p, 2, 1, odd, p, None, None) < 0 and b"misaligned" in lib.qi_last_error()
    assert lib.qi_csd_eigh(_lib.QI_F32, 0, p, 2, 1, p, p, ctypes.c_void_p(ctypes.addressof(buf) + 2), None) < 0
    assert b"misaligned" in lib.qi_last_error()


def test_size_query_verdicts_are_the_beam_power_ones():
    from quantum_inferno_amd import _lib

    lib = _lib.load()
    for shape in ((_lib.QI_F64, 64, 33, 300, 4), (_lib.QI_F32, 1, 1, 1, 1), (_lib.QI_F64, 0, 33, 300, 4), (_lib.QI_F64, 65, 33, 300, 4),
                  (_lib.QI_F64, 64, 33, 0, 4), (_lib.QI_F64, 64, 33, 300, 0), (_lib.QI_F64, 64, 0, 300, 4), (7, 64, 33, 300, 4),
                  (_lib.QI_F32, 5, 7, 15, 8), (_lib.QI_F32, 5, 1 << 40, 15, 2)):
        want = lib.qi_beam_power_scratch_bytes(*shape)
        want_msg = lib.qi_last_error() if want < 0 else None
        got = lib.qi_beam_music_scratch_bytes(*shape)
        assert got == want, shape
        if want < 0:
            assert lib.qi_last_error() == want_msg and want_msg, shape
    assert lib.qi_beam_music_scratch_bytes(_lib.QI_F64, 64, 33, 300, 4) > 0 > lib.qi_beam_music_scratch_bytes(_lib.QI_F64, 65, 33, 300, 4)


def test_music_refuses_a_source_count_outside_its_range_without_a_gpu():
    from quantum_inferno_amd import _lib

    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    f_host, f_ptr = _lib.darr([1.0])
    for C, n in ((5, -1), (5, 5), (1, 1), (64, 64), (5, 1 << 40)):
        rc = lib.qi_beam_music(_lib.QI_F32, 0, p, C, 1, n, f_ptr, p, 3, None, 1, p, None, None, p, 64, None)
        assert rc < 0 and "sources" in lib.qi_last_error().decode(), (C, n, lib.qi_last_error())
    # the shape's verdict comes first, as in the size query
    assert lib.qi_beam_music(_lib.QI_F32, 0, p, 65, 1, 1, f_ptr, p, 3, None, 1, p, None, None, p, 64, None) < 0
    assert b"sensors" in lib.qi_last_error()


# ---- 4: identities of the float64 restatements --------------------------------------------------------------------------------------------
def test_restatement_identities():
    for shape in bc.SHAPES:
        s, freq, tau, k = mc.inputs(shape, np.float64)
        C = shape.C
        assert np.array_equal(s, np.conj(np.swapaxes(s, 1, 2))) and k == min(2, C - 1)
        w, u = mc.eigh64(s)
        ortho, pairs = mc.residuals(w, u, s)
        assert ortho <= 1e-12 and pairs <= 1e-12 and np.all(np.diff(w, axis=1) >= 0), shape.id
        assert w[:, :C - k].min() >= 1.0 and (C == 1 or (w[:, :C - k].max() <= 2.0 and w[:, C - k:].min() >= 50.0)), shape.id
        # the kernel's algorithm in double: the same eigenvalues, the same noise subspace
        head = s[:STEPS64_MATRICES]
        ws, us, info, sweeps = mc.eigh_steps(head, np.float64)
        assert not info.any() and sweeps.max() <= 12, (shape.id, sweeps)
        assert np.all(np.diff(ws, axis=1) >= 0)
        assert np.abs(ws - np.linalg.eigvalsh(mc.hermitian_of_lower(head))).max() <= 1e-12 * np.abs(w).max(), shape.id
        o, p = mc.residuals(ws, us, head)
        assert o <= 1e-12 and p <= 1e-12, shape.id
        assert np.abs(mc.noise_projector(us, k) - mc.noise_projector(u[:STEPS64_MATRICES], k)).max() <= 1e-12, shape.id
        print(f"{shape.id}: the kernel's algorithm in double: {sweeps.min()}..{sweeps.max()} sweeps")
        # the form against the other way to the same number: the signal projector, the phase not reduced
        got = mc.music(u, k, freq, tau, shape.bands)
        e = np.exp(2j * np.pi * freq[:, None, None] * tau[None, :, :])
        us_ = u[:, :, C - k:]
        proj = np.eye(C)[None] - us_ @ np.conj(np.swapaxes(us_, 1, 2))
        d = np.real(np.einsum("fgi,fij,fgj->fg", np.conj(e), proj, e))
        first = bc.band_table(shape.bands, shape.nf)
        want = np.stack([C * (b - a) / d[a:b].sum(axis=0) for a, b in zip(first[:-1], first[1:])])
        assert np.allclose(got, want, rtol=1e-9, atol=0), shape.id
        assert got.min() >= 1 - 1e-12, shape.id
        assert np.abs(mc.music(u, 0, freq, tau, shape.bands) - 1).max() <= 1e-12, shape.id  # the completeness of U


# ---- 5: float32 against float64 -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def float32_deviations():
    out = {}
    for shape in bc.SHAPES:
        s, freq, tau, k = mc.inputs(shape, np.float32)
        w64, u64 = mc.eigh64(s)
        w, u, info, sweeps = mc.eigh_steps(s, np.float32)
        assert w.dtype == np.float32 and u.dtype == np.complex64 and not info.any(), shape.id
        got = mc.music32(u, k, freq, tau, shape.bands)
        ref = mc.music(u64, k, freq, tau, shape.bands)
        assert got.dtype == np.float32 and got.shape == ref.shape and np.isfinite(ref).all()
        out[shape.id] = (float(np.abs(w - w64).max() / np.abs(w64).max()), float(np.abs(mc.noise_projector(u, k) - mc.noise_projector(u64, k)).max()),
                         float(np.abs(1.0 / got.astype(np.float64) - 1.0 / ref).max()), int(sweeps.min()), int(sweeps.max()))
    return out


def test_float32_restatement_deviation():
    worst, at = [0.0, 0.0, 0.0], [None, None, None]
    for cid, dev in float32_deviations().items():
        print(f"{cid}: float32 restatement against float64: eigenvalues / max {dev[0]:.4g}, noise projector {dev[1]:.4g}, 1 / power {dev[2]:.4g}; "
              f"{dev[3]}..{dev[4]} sweeps")
        assert max(dev[:3]) <= bc.TOL["float32"], cid
        for n in range(3):
            if dev[n] > worst[n]:
                worst[n], at[n] = dev[n], cid
    consts = (mc.EIGH32_VALUES, mc.EIGH32_PROJECTOR, mc.MUSIC32_RECIPROCAL)
    print("largest: " + ", ".join(f"{w:.4g} ({a})" for w, a in zip(worst, at)) + "; the constants " + ", ".join(f"{c:g}" for c in consts)
          + f"; bound {bc.TOL['float32']:g}")
    for w, c in zip(worst, consts):
        assert w <= c <= 1.05 * w, (w, c)  # the constants are the measurements, rounded up
    assert max(consts) <= bc.TOL["float32"]


# ---- 6: plane waves ---------------------------------------------------------------------------------------------------------------------
def test_plane_wave_in_the_restatements():
    case = bc.pw_case()
    freq = np.fft.rfftfreq(case.nfft, 1 / bc.PW_FS)
    tau = bc.pw_delays()
    true = bc.pw_true_index()
    s = cc.restate(bc.pw_records(), case, "spectrum")
    power = mc.music(mc.eigh64(s)[1], 1, freq, tau, bc.PW_BANDS)
    capon = cpc.capon(cpc.whiten(s, cpc.LOADING), freq, tau, bc.PW_BANDS)
    assert power.shape == (4, 81) and power.min() >= 1 - 1e-12
    for b in range(4):
        at, ratio = mc.peak_ratio(power[b])
        at_c, ratio_c = cpc.peak_ratio(capon[b])
        print(f"plane wave, band {b}: MUSIC peak / runner-up {ratio:.2f} at {at}; Capon {ratio_c:.2f} at {at_c}")
        assert at == true and at_c == true, b
        assert ratio > ratio_c, b  # one source, the right count: sharper than Capon on the same matrices
    w32, u32, info, _ = mc.eigh_steps(s, np.float32)
    p32 = mc.music32(u32, 1, freq, tau, bc.PW_BANDS)
    assert not info.any() and p32.dtype == np.float32 and np.array_equal(np.argmax(p32, axis=1), np.full(4, true))


def test_two_plane_waves_in_the_restatements():
    """Two uncorrelated waves on the five-sensor array, n_sources = 2: the two largest local maxima of the map are the two
    true grid points in every band, the third at least four times lower (measured: 19 to 35 times in the three wide bands, 5.7
    in the one-bin band).  Bartlett on the same matrices is printed beside it."""
    case = bc.pw_case()
    freq = np.fft.rfftfreq(case.nfft, 1 / bc.PW_FS)
    tau = bc.pw_delays()
    true = mc.two_wave_indices()
    assert true == [25, 32] and bc.pw_true_index() in true
    s = cc.restate(mc.two_wave_records(), case, "spectrum")
    power = mc.music(mc.eigh64(s)[1], 2, freq, tau, bc.PW_BANDS)
    bartlett = bc.restate(s, freq, tau, bc.PW_BANDS)
    for b in range(4):
        top = mc.local_maxima(power[b])
        top_b = mc.local_maxima(bartlett[b])
        margin = float(power[b][top[1]] / power[b][top[2]])
        print(f"two waves, band {b}: MUSIC local maxima {top[:4]}, second / third {margin:.1f}; Bartlett local maxima {top_b[:4]}, second / third "
              f"{float(bartlett[b][top_b[1]] / bartlett[b][top_b[2]]):.2f}")
        assert sorted(top[:2]) == true and margin >= 4.0, b
    w32, u32, info, _ = mc.eigh_steps(s, np.float32)
    p32 = mc.music32(u32, 2, freq, tau, bc.PW_BANDS)
    assert not info.any() and all(sorted(mc.local_maxima(row)[:2]) == true for row in p32)


# ---- 7: the exact cases -----------------------------------------------------------------------------------------------------------------
def test_exact_cases_are_exact():
    """Diagonal matrices: no rotation is taken, in either precision."""
    nf, G = 9, 37
    for C in (5, 17, 64):
        s, want_w, want_u, freq, tau, turns4 = mc.exact_inputs(C, nf, G)
        assert np.isnan(s[:, 0, C - 1]).all() and np.array_equal(np.sort(want_w, axis=1), want_w)
        assert all(len(set(row)) == C for row in want_w[:-1]) and len(set(want_w[-1])) == C - 1  # one repeated value
        rep = np.flatnonzero(want_w[-1][1:] == want_w[-1][:-1])[0]
        assert want_u[-1][0, rep] == 1 and want_u[-1][C - 1, rep + 1] == 1  # a stable sort: the lower position first
        assert np.array_equal(want_u.sum(axis=1), np.ones((nf, C))) and np.array_equal(want_u.sum(axis=2), np.ones((nf, C)))
        assert np.array_equal(np.einsum("fij,fj->fi", want_u, want_w).real, np.real(s[:, np.arange(C), np.arange(C)]))
        for dtype in (np.float32, np.float64):
            w, u, info, sweeps = mc.eigh_steps(s, dtype)
            assert not info.any() and not sweeps.any(), (C, dtype)
            assert w.dtype == dtype and np.array_equal(w, want_w) and np.array_equal(u, want_u), (C, dtype)
        assert np.array_equal(4 * bc.reduced_turns(freq, tau) % 4, turns4 % 4)
        e = mc.exact_factors(turns4)
        for k in (0, 1, C - 1):
            d = mc.null_spectrum(want_u, k, freq, tau, e=e)
            assert np.array_equal(d, np.full((nf, G), float(C - k))), (C, k)
            for bands in (None, (0, 3, 4, 9)):
                power = mc.music(want_u, k, freq, tau, bands, e=e)
                assert np.array_equal(power, np.full(power.shape, float(C) / float(C - k))), (C, k, bands)


# ---- 8: info ------------------------------------------------------------------------------------------------------------------------------
def test_info_restated():
    for C in (5, 17):
        cases = mc.info_cases(C)
        assert [c[2] for c in cases] == [1, 0, 1, 0] and len(cases) == 4
        clean = mc.eigh_steps(mc.info_base(C)[None], np.float64)
        for name, matrix, want in cases:
            assert not np.isfinite(matrix).all(), name
            for dtype in (np.float32, np.float64):
                w, u, info, _ = mc.eigh_steps(matrix[None], dtype)
                assert info.dtype == np.int32 and info[0] == want, (name, C, dtype, info)
                if want:
                    assert np.isnan(w).all() and np.isnan(u.real).all() and np.isnan(u.imag).all(), name
                elif dtype == np.float64:  # the value above the diagonal is not read
                    assert np.array_equal(w, clean[0]) and np.array_equal(u, clean[1]), name
                else:
                    assert max(mc.residuals(w, u, mc.info_base(C)[None])) <= bc.TOL["float32"], name
