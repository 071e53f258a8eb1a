"""Beam weights and beam steering without a GPU: the exports of include/qi_steer.h and the census of
tests/steer_stream_cases.py against that header, the refusals of qi_beam_weights and qi_beam_steer and the size query's
verdicts, the NumPy restatements of tests/steer_cases.py against their identities (e^H a = 1, a^H R a = 1 / D,
mean_t |out|^2 = a^H S a), the float32 restatements' distance from the float64 ones, and the plane-wave and zero-delay cases
through the oracle's ShortTimeFFT-convention transform."""
import ctypes
import functools
import os

import numpy as np

import beam_cases as bc
import capon_cases as cpc
import steer_cases as stc
import steer_stream_cases as ssc
from stream_table import header_functions, stream_functions

ROOT = bc.ROOT
HEADER = "qi_steer.h"
OTHER_HEADERS = ("qi_tfr.h", "qi_array.h", "qi_beam.h", "qi_adaptive.h", "qi_subspace.h")
IDENTITY_TOL = 1e-12


# ---- 1, 2: the header, the exports, the stream census ---------------------------------------------------------------------------------
def test_library_exports_the_steer_header():
    from quantum_inferno_amd import _lib

    declared = set(header_functions(HEADER))
    assert declared == {"qi_beam_weights_scratch_bytes", "qi_beam_weights", "qi_beam_steer"}
    assert declared == set(_lib.STEER_PROTOTYPES)
    for table in (_lib.PROTOTYPES, _lib.ARRAY_PROTOTYPES, _lib.BEAM_PROTOTYPES, _lib.ADAPTIVE_PROTOTYPES, _lib.SUBSPACE_PROTOTYPES):
        assert not declared & set(table)
    for other in OTHER_HEADERS:
        assert not declared & set(header_functions(other)), other
    lib = _lib.load()
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in include/qi_steer.h but not exported"
        assert len(_lib.STEER_PROTOTYPES[name][1]) == len(header_functions(HEADER)[name].split(",")), name
    with open(os.path.join(ROOT, "include", "qi_steer.h")) as fh:
        text = fh.read()
    assert '#include "qi_tfr.h"' in text and '#include "qi_beam.h"' in text and "NO conjugate" in text


def test_every_stream_entry_point_has_a_case_and_nothing_else_is_named():
    assert ssc.TABLE.header == HEADER
    assert stream_functions(HEADER) == ["qi_beam_steer", "qi_beam_weights"]
    assert ssc.TABLE.named_functions() == stream_functions(HEADER)


def test_stream_case_table():
    by_id = ssc.TABLE.by_id
    assert ssc.TABLE.ids() == ["weights-capon", "weights-bartlett", "steer-f32", "steer-f64"]
    for case in ssc.TABLE.cases:
        assert case.functions and callable(case.build) and case.asynchronous and case.engine is None, case.id
    assert by_id("weights-capon").build.args == ("float32", True) and by_id("weights-bartlett").build.args == ("float64", False)
    assert by_id("steer-f32").build.args == ("float32",) and by_id("steer-f64").build.args == ("float64",)
    assert ssc.BEAMS == 17


def test_shape_cases_cover_every_edge():
    assert {s.C for s in stc.SHAPES} == {1, 5, 16, 17, 33, 64} and {s.nbeam for s in stc.SHAPES} == {1, 15, 16, 17, 37}
    assert {s.nf for s in stc.SHAPES} == {1, 7, 33} and {s.nt for s in stc.SHAPES} >= {1, 15, 16, 17, 64, 65, 300}
    assert len(set(stc.ids())) == len(stc.SHAPES)


# ---- 3: refusals ----------------------------------------------------------------------------------------------------------------------
def test_weights_refusals_without_a_gpu():
    """Refused before the device is touched: the pointers are never followed (this machine may have no GPU at all)."""
    from quantum_inferno_amd import _lib

    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    odd = ctypes.c_void_p(ctypes.addressof(buf) + 4)
    f_host, f_ptr = _lib.darr([1.0])
    good = dict(dtype=_lib.QI_F32, C=2, nf=1, nbeam=3)

    def call(a, whitener=p, freq=f_ptr, tau=p, weights=p, scratch=p, nbytes=256):
        return lib.qi_beam_weights(a["dtype"], 0, whitener, a["C"], a["nf"], freq, tau, a["nbeam"], weights, scratch, nbytes, None)

    for change, what in ((dict(C=0), "sensors"), (dict(C=65), "sensors"), (dict(nf=0), "bins"), (dict(nbeam=0), "delay rows"),
                         (dict(dtype=7), "dtype"), (dict(nf=1 << 30, nbeam=1 << 30), "too large")):
        for whitener in (p, None):
            assert call({**good, **change}, whitener=whitener) < 0, change
            assert what in lib.qi_last_error().decode(), (change, lib.qi_last_error())
    for kw in (dict(freq=None), dict(tau=None), dict(weights=None), dict(scratch=None)):
        assert call(good, **kw) < 0 and b"null" in lib.qi_last_error(), kw
    for kw in (dict(whitener=odd), dict(weights=odd), dict(tau=odd), dict(scratch=ctypes.c_void_p(ctypes.addressof(buf) + 8))):
        assert call(good, **kw) < 0 and b"misaligned" in lib.qi_last_error(), kw
    assert call({**good, "dtype": _lib.QI_F64}, weights=ctypes.c_void_p(ctypes.addressof(buf) + 8)) < 0 and b"misaligned" in lib.qi_last_error()
    assert call(good, nbytes=0) < 0 and b"scratch" in lib.qi_last_error()
    assert call(good, nbytes=lib.qi_beam_weights_scratch_bytes(_lib.QI_F32, 2, 1, 3) - 1) < 0 and b"scratch" in lib.qi_last_error()


def test_steer_refusals_without_a_gpu():
    from quantum_inferno_amd import _lib

    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    odd = ctypes.c_void_p(ctypes.addressof(buf) + 4)
    good = dict(dtype=_lib.QI_F32, C=2, nf=1, nt=4, nbeam=3)

    def call(a, z=p, weights=p, out=p):
        return lib.qi_beam_steer(a["dtype"], 0, z, a["C"], a["nf"], a["nt"], weights, a["nbeam"], out, None)

    for change, what in ((dict(C=0), "sensors"), (dict(C=65), "sensors"), (dict(nf=0), "bins"), (dict(nt=0), "times"),
                         (dict(nbeam=0), "beams"), (dict(dtype=7), "dtype"), (dict(nf=1 << 20, nt=1 << 20), "too large"),
                         (dict(nf=1 << 20, nbeam=1 << 20), "too large"), (dict(nt=1 << 20, nbeam=1 << 21), "too large")):
        assert call({**good, **change}) < 0, change
        assert what in lib.qi_last_error().decode(), (change, lib.qi_last_error())
    for kw in (dict(z=None), dict(weights=None), dict(out=None)):
        assert call(good, **kw) < 0 and b"null" in lib.qi_last_error(), kw
    for kw in (dict(z=odd), dict(weights=odd), dict(out=odd)):
        assert call(good, **kw) < 0 and b"misaligned" in lib.qi_last_error(), kw
    assert call({**good, "dtype": _lib.QI_F64}, out=ctypes.c_void_p(ctypes.addressof(buf) + 8)) < 0 and b"misaligned" in lib.qi_last_error()


def test_size_query_gives_the_calls_verdicts():
    from quantum_inferno_amd import _lib

    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    f_host, f_ptr = _lib.darr([1.0])
    for shape in ((_lib.QI_F64, 0, 33, 300), (_lib.QI_F64, 65, 33, 300), (_lib.QI_F64, 64, 0, 300), (_lib.QI_F64, 64, 33, 0),
                  (7, 64, 33, 300), (_lib.QI_F32, 5, 1 << 30, 1 << 30), (_lib.QI_F32, 64, 1 << 40, 1)):
        got = lib.qi_beam_weights_scratch_bytes(*shape)
        msg = lib.qi_last_error()
        assert got < 0 and msg, shape
        rc = lib.qi_beam_weights(shape[0], 0, p, shape[1], shape[2], f_ptr, p, shape[3], p, p, 1 << 20, None)
        assert rc == got and lib.qi_last_error() == msg, shape
    assert lib.qi_beam_weights_scratch_bytes(_lib.QI_F64, 64, 33, 300) >= 33 * 8
    assert lib.qi_beam_weights_scratch_bytes(_lib.QI_F32, 1, 1, 1) >= 8
    assert lib.qi_beam_weights_scratch_bytes(_lib.QI_F32, 64, 1 << 20, 1 << 14) > 0  # 2^40 entries: the last shape accepted


# ---- 4: identities of the float64 restatement -----------------------------------------------------------------------------------------
def test_restatement_identities():
    worst = [0.0, 0.0, 0.0, 0.0]
    for shape in stc.SHAPES:
        s, freq, tau, z = stc.inputs(shape, np.float64)
        v = cpc.whiten(s, stc.LOADING)
        a = stc.weights(freq, tau, v)
        assert a.shape == (shape.nf, shape.nbeam, shape.C)
        # the distortionless constraint, and the output power against Capon's
        unit = float(np.abs(stc.gain(freq, tau, a) - 1).max())
        inv_d = cpc.capon(v, freq, tau)  # [nf, nbeam]: 1 / D
        power = float(np.abs(stc.output_power(a, cpc.loaded(s, stc.LOADING)) / inv_d - 1).max())
        # loading 0, S from the panel itself: the beam's mean power is 1 / D (needs nt >= C: a definite S)
        own = 0.0
        if shape.nt >= 2 * shape.C:
            sz = stc.cross_spectra(z)
            vz = cpc.whiten(sz, 0.0)
            beams = stc.steer(z, stc.weights(freq, tau, vz))
            mean = (beams.real ** 2 + beams.imag ** 2).mean(axis=2).T  # [nf, nbeam]
            own = float(np.abs(mean / cpc.capon(vz, freq, tau) - 1).max())
        # Bartlett: the beam's mean power is beam_cases.restate of the panel's own S
        sz = stc.cross_spectra(z)
        b = stc.steer(z, stc.weights(freq, tau))
        mean_b = (b.real ** 2 + b.imag ** 2).mean(axis=2).T
        want_b = bc.restate(sz, freq, tau)
        bartlett = float(np.abs(mean_b - want_b).max() / np.abs(want_b).max())
        assert float(np.abs(stc.gain(freq, tau, stc.weights(freq, tau)) - 1).max()) <= IDENTITY_TOL
        print(f"{shape.id}: |e^H a - 1| {unit:.3g}, |a^H R a D - 1| {power:.3g}, own S: |mean |out|^2 D - 1| {own:.3g}, Bartlett "
              f"|mean |out|^2 - e^H S e / C^2| / max {bartlett:.3g}")
        for n, val in enumerate((unit, power, own, bartlett)):
            worst[n] = max(worst[n], val)
        assert max(unit, power, own, bartlett) <= IDENTITY_TOL, shape.id
    print("largest: " + ", ".join(f"{w:.3g}" for w in worst) + f"; bound {IDENTITY_TOL:g}")


# ---- 5: float32 against float64 -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def float32_deviations():
    out = {}
    for shape in stc.SHAPES:
        s, freq, tau, z = stc.inputs(shape, np.float32)
        s64, _, _, z64 = stc.inputs(shape, np.float64)
        a64 = stc.weights(freq, tau, cpc.whiten(s64, stc.LOADING))
        a32 = stc.weights32(freq, tau, cpc.whiten32(s, stc.LOADING))
        assert a32.dtype == np.complex64 and a32.shape == a64.shape and np.isfinite(a64).all()
        y64, y32 = stc.steer(z64, a64), stc.steer32(z, a32)
        b64, b32 = stc.steer(z64, stc.weights(freq, tau)), stc.steer32(z, stc.weights32(freq, tau))
        assert y32.dtype == np.complex64 and b32.dtype == np.complex64
        out[shape.id] = (float(np.abs(a32 - a64).max() / np.abs(a64).max()), float(np.abs(y32 - y64).max() / np.abs(y64).max()),
                         float(np.abs(b32 - b64).max() / np.abs(b64).max()))
    return out


def test_float32_restatement_deviation():
    worst, at = [0.0, 0.0, 0.0], [None, None, None]
    for cid, dev in float32_deviations().items():
        print(f"{cid}: float32 restatement against float64, of the largest modulus: MVDR weights {dev[0]:.4g}, MVDR beams {dev[1]:.4g}, "
              f"Bartlett beams {dev[2]:.4g}")
        assert max(dev) <= bc.TOL["float32"], cid
        for n in range(3):
            if dev[n] > worst[n]:
                worst[n], at[n] = dev[n], cid
    consts = (stc.MVDR32_WEIGHTS, stc.MVDR32_BEAMS, stc.BARTLETT32_BEAMS)
    print("largest: " + ", ".join(f"{w:.4g} ({a})" for w, a in zip(worst, at)) + "; the constants " + ", ".join(f"{c:g}" for c in consts)
          + f"; bound {bc.TOL['float32'] / 16:g}")
    for w, c in zip(worst, consts):
        assert w <= c <= 1.05 * w, (w, c)  # the constants are the measurements, rounded up
    assert max(consts) <= bc.TOL["float32"] / 16


# ---- 6: the exact cases --------------------------------------------------------------------------------------------------------------------
def test_exact_cases_are_exact():
    for C in (5, 17, 33, 64):
        a, z, out = stc.exact_steer_inputs(C, 37, 3, 40)
        assert np.array_equal(stc.steer32(z, a).astype(np.complex128), out), C
    for C in (16, 64):
        _, freq, tau, turns4 = bc.exact_inputs(C, 9, 37)
        want = stc.unit_weights(turns4, C)
        assert np.array_equal(stc.weights(freq, tau, e=cpc.exact_factors(turns4)), want), C
        # (weights32 takes its factors from cos and sin of 2 pi t, which are not exact at quarter turns: the device's sincospi is)
        eye = np.broadcast_to(np.eye(C, dtype=np.complex128), (9, C, C))
        assert np.array_equal(stc.weights(freq, tau, eye, e=cpc.exact_factors(turns4)), want), C  # D = C exactly


# ---- 7: the plane wave and zero delays, on the oracle -------------------------------------------------------------------------------------
def test_plane_wave_trace_on_the_oracle():
    """Bartlett at segments of 1024 with overlap 768: the trace at the true slowness is the source to within 0.065 relative RMS
    over the interior (measured 0.0534; the records' own noise leaves 0.1 / sqrt(5) = 0.0447), the trace at the grid centre is
    not (measured 0.903).  At 256 / 128 the delays (up to 53 samples) are no longer short against the segment: printed.  With
    few segments Capon cancels part of the signal: printed."""
    seg, overlap = stc.PW_TRACE_SEG, stc.PW_TRACE_OVERLAP
    _, traces = stc.oracle_traces(seg, overlap)
    true, centre = stc.relative_rms(traces[0], seg), stc.relative_rms(traces[1], seg)
    delays = np.abs(bc.pw_delays(stc.pw_steer_rows())[0]).max() * bc.PW_FS
    print(f"plane wave, Bartlett, segments {seg} / overlap {overlap} ({stc.oracle_panel(seg, overlap)[1].shape[2]} segments): relative RMS "
          f"distance from the source {true:.4f} at the true slowness, {centre:.4f} at the grid centre; own-noise floor "
          f"{bc.PW_OWN / np.sqrt(len(bc.PW_POSITIONS_M)):.4f}; delays of up to {delays:.1f} samples")
    assert true <= stc.PW_TRUE_MAX and centre >= stc.PW_CENTRE_MIN
    short = stc.relative_rms(stc.oracle_traces(*stc.PW_TRACE_SHORT)[1][0], stc.PW_TRACE_SHORT[0])
    print(f"plane wave, Bartlett, segments {stc.PW_TRACE_SHORT[0]} / overlap {stc.PW_TRACE_SHORT[1]}: {short:.4f} at the true slowness")
    capon = stc.relative_rms(stc.oracle_traces(seg, overlap, "capon", stc.PW_CAPON_LOADING)[1][0], seg)
    print(f"plane wave, Capon at loading {stc.PW_CAPON_LOADING}, segments {seg} / overlap {overlap}: {capon:.4f} at the true slowness")


def test_zero_delays_give_the_mean_of_the_records():
    seg, overlap = stc.PW_TRACE_SEG, stc.PW_TRACE_OVERLAP
    o, z = stc.oracle_panel(seg, overlap)
    _, traces = stc.oracle_traces(seg, overlap, zero_delays=True)
    last = (z.shape[2] - 1) * o.hop
    want = o.istft(o.stft(bc.pw_records().mean(axis=0)), last)
    err = float(np.abs(traces[0] - want).max() / np.abs(want).max())
    print(f"zero delays: the Bartlett trace against stft -> istft of the records' mean, of its maximum: {err:.3g}")
    assert err <= IDENTITY_TOL
