"""Beam weights and beam steering on the device (-m gpu): qi_beam_weights and qi_beam_steer against the NumPy restatements of
tests/steer_cases.py at ragged and full tiles in both precisions, the exact cases bit for bit (Gaussian-integer weights and
panels: one result-row map used for the other puts three of four results in the wrong beam; quarter-turn delays; an identity
whitener), the determinism contract of include/qi_steer.h, the NaN rules, the refusals, and beamform.beam_stft_pow2 and
beam_traces_tukey end to end against the oracle's transforms.

The bounds are the project's reduction tolerances, 1e-4 (float32) and 1e-10 (float64) of the case's largest modulus, also for
max |e^H a - 1| and max |a^H R a D - 1|; the traces: 10 x (2e-5 | 1e-11) of the trace's maximum, as
test_istft_random_spectrum_vs_oracle asks of the inverse transform."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import beam_cases as bc
import capon_cases as cpc
import steer_cases as stc

from quantum_inferno_amd import _lib, beamform, engine

pytestmark = pytest.mark.gpu

DTYPES = bc.DTYPES
TRACE_TOL = {"float32": 10 * 2e-5, "float64": 10 * 1e-11}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def case(cid, dtype):
    """What the device reads and the float64 restatements on those values: computed once, shared, left unchanged ->
    (csd, freq, tau, panel, whitener, MVDR weights, MVDR beams, Bartlett weights, Bartlett beams)."""
    shape = stc.by_id(cid)
    s, freq, tau, z = stc.inputs(shape, dtype)
    v = stc.whiteners(shape, dtype).astype(bc.complex_of(dtype))
    a = stc.weights(freq, tau, v)
    b = stc.weights(freq, tau)
    out = (s, freq, tau, z, v, a, stc.steer(z, a), b, stc.steer(z, b))
    for x in out:
        x.setflags(write=False)
    return out


def rel(got, want):
    return float(np.abs(got.astype(np.complex128) - want).max() / np.abs(want).max())


# ---- against the restatement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cid", stc.ids())
def test_weights_and_beams_match_the_restatement(cid, dtype):
    shape = stc.by_id(cid)
    s, freq, tau, z, v, ref_a, ref_y, ref_b, ref_yb = case(cid, dtype)
    ctype = bc.complex_of(dtype)
    a = engine.beam_weights(freq, tau, whitener=v)
    b = engine.beam_weights(freq, tau, sensors=shape.C, dtype=dtype)
    assert a.dtype == ctype and a.shape == (shape.nf, shape.nbeam, shape.C) and b.dtype == ctype and b.shape == a.shape
    y, yb = engine.beam_steer(z, a), engine.beam_steer(z, b)
    fed = engine.beam_steer(z, ref_a.astype(ctype))  # the steer alone, fed the restated weights
    assert y.dtype == ctype and y.shape == (shape.nbeam, shape.nf, shape.nt) and yb.shape == y.shape and fed.shape == y.shape
    err = dict(mvdr_w=rel(a, ref_a), bartlett_w=rel(b, ref_b), mvdr_y=rel(y, ref_y), bartlett_y=rel(yb, ref_yb), fed_y=rel(fed, ref_y))
    unit = float(np.abs(stc.gain(freq, tau, a) - 1).max())
    power = float(np.abs(stc.output_power(a, cpc.loaded(s, stc.LOADING, dtype)) / cpc.capon(v, freq, tau) - 1).max())
    print(f"{cid} {dtype}: of the largest modulus: MVDR weights {err['mvdr_w']:.3g}, Bartlett weights {err['bartlett_w']:.3g}, MVDR beams "
          f"{err['mvdr_y']:.3g} (fed the restated weights {err['fed_y']:.3g}), Bartlett beams {err['bartlett_y']:.3g}; max |e^H a - 1| "
          f"{unit:.3g}, max |a^H R a D - 1| {power:.3g}")
    tol = bc.TOL[dtype]
    assert max(err.values()) <= tol and unit <= tol and power <= tol, (cid, dtype, err, unit, power)
    assert np.isfinite(a.view(dtype)).all() and np.isfinite(y.view(dtype)).all()


# ---- the exact cases --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", (5, 17, 33, 64))
def test_integer_beams_bit_for_bit(C, dtype):
    """Gaussian-integer weights that depend asymmetrically on (k, i), an integer panel, every sum below 2^24."""
    ctype = bc.complex_of(dtype)
    for nbeam, nf, nt in ((37, 3, 40), (16, 2, 129)):
        a, z, want = stc.exact_steer_inputs(C, nbeam, nf, nt)
        got = engine.beam_steer(z.astype(ctype), a.astype(ctype))
        assert same_bits(got, want.astype(ctype)), (C, dtype, nbeam, np.argwhere(got != want)[:4])


@pytest.mark.parametrize("dtype", DTYPES)
def test_quarter_turn_weights_bit_for_bit(dtype):
    """Bartlett weights at quarter-turn delays are the exact units over C (C = 16, 64: the quotient is exact too); an identity
    whitener gives Bartlett's weights bit for bit at any C (D = C exactly, every zero a +0)."""
    ctype = bc.complex_of(dtype)
    nf, nbeam = 9, 37
    for C in (5, 16, 17, 64):
        _, freq, tau, turns4 = bc.exact_inputs(C, nf, nbeam)
        assert np.array_equal(4 * bc.reduced_turns(freq, tau) % 4, turns4 % 4)
        b = engine.beam_weights(freq, tau, dtype=dtype)
        if C in (16, 64):
            assert same_bits(b, stc.unit_weights(turns4, C).astype(ctype)), (C, dtype)
        else:
            assert rel(b, stc.unit_weights(turns4, C)) <= np.finfo(dtype).eps, (C, dtype)
        eye = np.ascontiguousarray(np.broadcast_to(np.eye(C, dtype=ctype), (nf, C, C)))
        assert same_bits(engine.beam_weights(freq, tau, whitener=eye), b), (C, dtype)


# ---- determinism ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_weights_are_a_function_of_their_own_row_and_bin(dtype):
    for cid in ("c64_k37_f33_t300", "c17_k17_f33_t17", "c5_k37_f33_t300"):
        shape = stc.by_id(cid)
        s, freq, tau, z, v = case(cid, dtype)[:5]
        for whitener in (v, None):
            kw = dict(whitener=whitener) if whitener is not None else dict(dtype=dtype)
            full = engine.beam_weights(freq, tau, **kw)
            assert same_bits(engine.beam_weights(freq, tau, **kw), full), cid  # a second run
            for k in sorted({0, shape.nbeam // 2, shape.nbeam - 1}):
                alone = engine.beam_weights(freq, tau[k:k + 1], **kw)  # a row alone
                assert same_bits(alone[:, 0], full[:, k]), (cid, k)
            moved = engine.beam_weights(freq, tau[::-1].copy(), **kw)  # every row moved
            assert same_bits(moved[:, ::-1], full), cid
            larger = engine.beam_weights(freq, np.concatenate([tau[3:], tau, tau[:5]]), **kw)  # within a larger nbeam
            assert same_bits(larger[:, shape.nbeam - 3:2 * shape.nbeam - 3], full), cid
            f = shape.nf // 2  # a bin alone
            kw1 = dict(whitener=whitener[f:f + 1]) if whitener is not None else dict(dtype=dtype)
            assert same_bits(engine.beam_weights(freq[f:f + 1], tau, **kw1)[0], full[f]), cid


@pytest.mark.parametrize("dtype", DTYPES)
def test_beams_are_a_function_of_their_own_weights_and_column(dtype):
    for cid in ("c64_k37_f33_t300", "c5_k37_f33_t2700", "c17_k17_f33_t17"):
        shape = stc.by_id(cid)
        z, a = case(cid, dtype)[3], case(cid, dtype)[5].astype(bc.complex_of(dtype))
        full = engine.beam_steer(z, a)
        assert same_bits(engine.beam_steer(z, a), full), cid  # a second run
        for k in sorted({0, shape.nbeam // 2, shape.nbeam - 1}):  # a beam alone
            assert same_bits(engine.beam_steer(z, a[:, k:k + 1])[0], full[k]), (cid, k)
        assert same_bits(engine.beam_steer(z, a[:, ::-1].copy())[::-1], full), cid  # every beam moved
        for lo, hi in ((0, 1), (shape.nt // 3, shape.nt // 3 + 17), (shape.nt - 5, shape.nt), (1, shape.nt)):  # a column range alone
            hi = min(hi, shape.nt)
            part = engine.beam_steer(np.ascontiguousarray(z[:, :, lo:hi]), a)
            assert same_bits(part, np.ascontiguousarray(full[:, :, lo:hi])), (cid, lo, hi)
        f = shape.nf // 2  # a bin alone
        assert same_bits(engine.beam_steer(np.ascontiguousarray(z[:, f:f + 1]), a[f:f + 1])[:, 0], full[:, f]), cid


# ---- NaN rules --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_flagged_bin_is_nan_and_no_other(dtype):
    for cid in ("c17_k17_f33_t17", "c64_k16_f1_t65", "c5_k37_f33_t300"):
        shape = stc.by_id(cid)
        s, freq, tau, z = stc.inputs(shape, dtype)
        clean = engine.beam_weights(freq, tau, whitener=engine.csd_whiten(s, loading=stc.LOADING))
        bad = shape.nf // 2
        s = s.copy()
        s[bad] = 0  # no pivot: info 1
        v, info = engine.csd_whiten(s, loading=stc.LOADING, info=True)
        assert info[bad] == 1 and not np.delete(info, bad).any()
        a = engine.beam_weights(freq, tau, whitener=v)
        y = engine.beam_steer(z, a)
        assert np.isnan(a[bad].real).all() and np.isnan(a[bad].imag).all() and np.isnan(y[:, bad].real).all() and np.isnan(y[:, bad].imag).all()
        assert np.isfinite(np.delete(a, bad, axis=0).view(dtype)).all() and np.isfinite(np.delete(y, bad, axis=1).view(dtype)).all(), cid
        good = [f for f in range(shape.nf) if f != bad]
        assert same_bits(a[good], clean[good]), cid  # (one bin: nothing else to compare)


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_nan_in_a_panel_column_stays_in_that_column(dtype):
    for cid in ("c17_k17_f33_t17", "c64_k37_f33_t300"):
        shape = stc.by_id(cid)
        z, a = case(cid, dtype)[3].copy(), case(cid, dtype)[5].astype(bc.complex_of(dtype))
        full = engine.beam_steer(z, a)
        f, t, i = shape.nf // 2, shape.nt // 2, shape.C - 1
        z[i, f, t] = np.nan
        y = engine.beam_steer(z, a)
        assert np.isnan(y[:, f, t].real).all() and np.isnan(y[:, f, t].imag).all()
        y[:, f, t] = full[:, f, t]
        assert same_bits(y, full), cid


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    lib = _lib.load()
    dev = engine.default_device()
    C, nf, nt, nbeam = 5, 3, 20, 4
    fill = 0.3125
    w = torch.full((nf, nbeam, C, 2), fill, dtype=torch.float32, device=dev)
    out = torch.full((nbeam, nf, nt, 2), fill, dtype=torch.float32, device=dev)
    z = torch.ones((C, nf, nt, 2), dtype=torch.float32, device=dev)
    tau = torch.zeros((nbeam, C), dtype=torch.float64, device=dev)
    scratch = torch.empty(1024, dtype=torch.uint8, device=dev)
    f_host, f_ptr = _lib.darr(np.arange(1.0, nf + 1))
    p = _lib.ptr
    stream = _lib.stream_ptr(dev.index)
    odd = ctypes.c_void_p(w.data_ptr() + 4)
    for args in ((7, p(None), C, nf, f_ptr, p(tau), nbeam, p(w), p(scratch), 1024), (0, p(None), 65, nf, f_ptr, p(tau), nbeam, p(w), p(scratch), 1024),
                 (0, p(None), C, nf, None, p(tau), nbeam, p(w), p(scratch), 1024), (0, p(None), C, nf, f_ptr, p(tau), nbeam, p(w), p(scratch), 8),
                 (0, p(None), C, nf, f_ptr, p(tau), nbeam, odd, p(scratch), 1024), (0, p(None), C, nf, f_ptr, p(tau), 0, p(w), p(scratch), 1024)):
        assert lib.qi_beam_weights(args[0], dev.index, *args[1:], stream) < 0 and lib.qi_last_error(), args
    for args in ((7, p(z), C, nf, nt, p(w), nbeam, p(out)), (0, p(z), 0, nf, nt, p(w), nbeam, p(out)), (0, p(z), C, nf, 0, p(w), nbeam, p(out)),
                 (0, None, C, nf, nt, p(w), nbeam, p(out)), (0, p(z), C, nf, nt, odd, nbeam, p(out))):
        assert lib.qi_beam_steer(args[0], dev.index, *args[1:], stream) < 0 and lib.qi_last_error(), args
    torch.cuda.synchronize()
    assert bool((w == fill).all()) and bool((out == fill).all())
    with pytest.raises(ValueError):
        engine.beam_steer(np.zeros((C, nf, nt), np.complex64), np.zeros((nf, nbeam, C), np.complex128))
    with pytest.raises(ValueError):
        engine.beam_weights(np.arange(1.0, 4.0), np.zeros((nbeam, C)), sensors=C + 1)
    with pytest.raises(_lib.QiError):
        engine.beam_weights(np.arange(1.0, 4.0), np.zeros((nbeam, 65)))


def test_numpy_in_numpy_out_tensor_in_tensor_out():
    s, freq, tau, z, v = case("c5_k15_f7_t15", "float32")[:5]
    a = engine.beam_weights(freq, tau, whitener=v)
    a_dev = engine.beam_weights(freq, torch.from_numpy(tau).cuda(), whitener=torch.from_numpy(v).cuda())
    assert isinstance(a, np.ndarray) and isinstance(a_dev, torch.Tensor) and a_dev.is_cuda and same_bits(a_dev.cpu().numpy(), a)
    b_dev = engine.beam_weights(freq, torch.from_numpy(tau).cuda())
    assert isinstance(b_dev, torch.Tensor) and b_dev.dtype == torch.complex64 and same_bits(b_dev.cpu().numpy(), engine.beam_weights(freq, tau))
    y, y_dev = engine.beam_steer(z, a), engine.beam_steer(torch.from_numpy(z).cuda(), a_dev)
    assert isinstance(y, np.ndarray) and isinstance(y_dev, torch.Tensor) and y_dev.is_cuda and same_bits(y_dev.cpu().numpy(), y)


# ---- end to end --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stft_reference(method):
    """beam_stft_pow2 restated on the oracle's panels of the plane-wave records: computed once, shared, left unchanged."""
    from oracle import tfr_oracle as orc

    parts = [orc.stft_complex_pow2(x, bc.PW_FS, bc.PW_SEG, bc.PW_OVERLAP) for x in bc.pw_records()]
    f, t, z = parts[0][0], parts[0][1], np.stack([p[2] for p in parts])
    a, _ = stc.panel_weights(z, f, bc.pw_delays(stc.pw_steer_rows()), method, stc.PW_CAPON_LOADING)
    beams = stc.steer(z, a)
    beams.setflags(write=False)
    return f, t, beams


@pytest.mark.parametrize("dtype", DTYPES)
def test_beam_stft_pow2_end_to_end(dtype):
    x = bc.pw_records().astype(dtype)
    power = {}
    for method in stc_methods():
        f_ref, t_ref, ref = stft_reference(method)
        f, t, beams, info = beamform.beam_stft_pow2(x, bc.PW_FS, bc.PW_POSITIONS_M, stc.pw_steer_rows(), bc.PW_SEG, bc.PW_OVERLAP, method=method,
                                                    loading=stc.PW_CAPON_LOADING)
        assert isinstance(beams, np.ndarray) and beams.dtype == bc.complex_of(dtype) and beams.shape == ref.shape == (2, len(f), len(t))
        assert np.allclose(f, f_ref) and np.allclose(t, t_ref)
        err = rel(beams, ref)
        print(f"beam_stft_pow2 {method} {dtype}: beams against the restatement on the oracle's panels, of the largest modulus {err:.3g}")
        assert err <= bc.TOL[dtype], (method, dtype)
        if method == "capon":
            assert info.dtype == np.int32 and info.shape == (len(f),) and not info.any()
        else:
            assert info is None
        power[method] = (beams.real.astype(np.float64) ** 2 + beams.imag.astype(np.float64) ** 2).mean(axis=2)[0]  # at the steered point
    assert np.all(power["capon"] <= power["bartlett"] * (1 + bc.TOL[dtype])), dtype  # minimum variance under the same constraint


def stc_methods():
    return beamform.BEAM_METHODS


@pytest.mark.parametrize("dtype", DTYPES)
def test_beam_traces_tukey_end_to_end(dtype):
    x = bc.pw_records().astype(dtype)
    seg, overlap = stc.PW_TRACE_SEG, stc.PW_TRACE_OVERLAP
    rows = stc.pw_steer_rows()
    for method in stc_methods():
        _, ref = stc.oracle_traces(seg, overlap, method, stc.PW_CAPON_LOADING)
        ts, traces, info = beamform.beam_traces_tukey(x, bc.PW_FS, bc.PW_POSITIONS_M, rows, seg, overlap, stc.PW_TRACE_ALPHA, method=method,
                                                      loading=stc.PW_CAPON_LOADING)
        assert isinstance(traces, np.ndarray) and traces.dtype == np.dtype(dtype) and traces.shape == ref.shape and len(ts) == ref.shape[1]
        err = max(float(np.abs(traces[k] - ref[k]).max() / np.abs(ref[k]).max()) for k in range(2))
        print(f"beam_traces_tukey {method} {dtype}: traces against the oracle's istft of the restated beams, of the trace's maximum {err:.3g}")
        assert err <= TRACE_TOL[dtype], (method, dtype)
        true = stc.relative_rms(traces[0].astype(np.float64), seg)
        if method == "bartlett":
            centre = stc.relative_rms(traces[1].astype(np.float64), seg)
            print(f"beam_traces_tukey bartlett {dtype}: relative RMS distance from the source {true:.4f} at the true slowness, {centre:.4f} at the centre")
            assert info is None and true <= stc.PW_TRUE_MAX and centre >= stc.PW_CENTRE_MIN
        else:
            print(f"beam_traces_tukey capon {dtype} at loading {stc.PW_CAPON_LOADING}: {true:.4f} at the true slowness")
            assert info.dtype == np.int32 and not info.any()
    # zero delays: the mean of the records through stft and istft
    _, ref0 = stc.oracle_traces(seg, overlap, zero_delays=True)
    _, mean, _ = beamform.beam_traces_tukey(x, bc.PW_FS, bc.PW_POSITIONS_M, np.zeros((1, 2)), seg, overlap, stc.PW_TRACE_ALPHA)
    err0 = float(np.abs(mean[0] - ref0[0]).max() / np.abs(ref0[0]).max())
    print(f"beam_traces_tukey {dtype}: zero delays against the oracle's stft -> istft of the records' mean, of its maximum {err0:.3g}")
    assert err0 <= TRACE_TOL[dtype]
    # a CUDA tensor in: CUDA tensors out, the same bits
    _, dev_traces, _ = beamform.beam_traces_tukey(torch.from_numpy(x).cuda(), bc.PW_FS, bc.PW_POSITIONS_M, np.zeros((1, 2)), seg, overlap,
                                                  stc.PW_TRACE_ALPHA)
    assert isinstance(dev_traces, torch.Tensor) and dev_traces.is_cuda and same_bits(dev_traces.cpu().numpy(), mean)
