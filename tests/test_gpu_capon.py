"""Capon beamforming on the device (-m gpu): qi_csd_whiten and qi_beam_capon against the NumPy restatements of
tests/capon_cases.py at ragged and full tiles in both precisions, an exact case bit for bit, the determinism contracts of
include/qi_adaptive.h, `info` and the NaN rules, Capon <= Bartlett against engine.beam_power, the plane-wave case end to end
through beamform.capon_power_pow2, and the refusals."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import beam_cases as bc
import capon_cases as cpc
import csd_cases as cc

from quantum_inferno_amd import _lib, beamform, engine

pytestmark = pytest.mark.gpu

DTYPES = bc.DTYPES


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def reference(cid, dtype):
    """The float64 restatements on the values the device reads (the loaded diagonal rounded once to dtype): computed once,
    shared, left unchanged -> (R, V, power)."""
    shape = bc.by_id(cid)
    s, freq, tau = cpc.inputs(shape, dtype)
    r = cpc.loaded(s, cpc.LOADING, dtype)
    v = cpc.whiten(s, cpc.LOADING, dtype)
    power = cpc.capon(v, freq, tau, shape.bands)
    for a in (r, v, power):
        a.setflags(write=False)
    return r, v, power


# ---- against the restatement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cid", bc.ids())
def test_whitener_and_power_match_the_restatement(cid, dtype):
    shape = bc.by_id(cid)
    s, freq, tau = cpc.inputs(shape, dtype)
    bands = None if shape.bands is None else list(shape.bands)
    nb = shape.nf if bands is None else len(bands) - 1
    r, ref_v, ref_p = reference(cid, dtype)
    v, info = engine.csd_whiten(s, loading=cpc.LOADING, info=True)
    assert v.dtype == s.dtype and v.shape == s.shape and info.dtype == np.int32 and not info.any()
    lower = np.tril(np.ones((shape.C, shape.C), dtype=bool), -1)
    assert not bits(v[:, lower]).any()  # the strictly lower part: zeros, bit for bit
    err_v = float(np.abs(v - ref_v).max() / np.abs(ref_v).max())
    res = cpc.residual(v, r)
    got, index, value = engine.capon_power(v, freq, tau, bands=bands, peaks=True)
    assert got.dtype == np.dtype(dtype) and got.shape == (nb, shape.G) == ref_p.shape
    err_p = float(np.abs(got.astype(np.float64) - ref_p).max() / np.abs(ref_p).max())
    print(f"{cid} {dtype}: whitener / max {err_v:.3g}, max |V^H R V - I| {res:.3g}, power / max power {err_p:.3g}")
    assert err_v <= bc.TOL[dtype] and res <= bc.TOL[dtype] and err_p <= bc.TOL[dtype], (cid, dtype)
    assert np.isfinite(got).all() and got.min() > 0
    want_index, want_value = bc.peaks_of(got)
    assert index.dtype == np.int64 and np.array_equal(index, want_index) and same_bits(value, want_value)


# ---- the exact case -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", (17, 33))
def test_exact_integer_case_bit_for_bit(C, dtype):
    """Every pivot is 1, every entry of V a unit of the Gaussian integers and every D an integer of at most 12 529: a wrong
    triangle, conjugate, operand or result-row map shows as a wrong integer."""
    nf, G = 33, 37
    s, _, freq, tau, turns4 = cpc.exact_inputs(C, nf, G)
    want_v, want_info = cpc.whiten_steps(s, 0.0, dtype)
    v, info = engine.csd_whiten(s.astype(bc.complex_of(dtype)), loading=0.0, info=True)
    assert not info.any() and not want_info.any()
    assert same_bits(v, want_v), (C, dtype, np.argwhere(v != want_v)[:4])
    assert np.array_equal(v, cpc.whiten(s, 0.0))  # and the float64 statement's integers
    e = cpc.exact_factors(turns4)
    for bands in (None, [0, 3, 4, 33]):
        want = cpc.capon(want_v, freq, tau, bands, e=e).astype(dtype)
        power = engine.capon_power(v, freq, tau, bands=bands)
        assert same_bits(power, want), (C, dtype, bands, np.argwhere(power != want)[:4])


# ---- determinism --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_grid_point_has_the_same_bits_wherever_it_is_computed(dtype):
    shape = bc.by_id("c64_g300_f33_b3")
    s, freq, tau = cpc.inputs(shape, dtype)
    bands = list(shape.bands)
    v = engine.csd_whiten(s, loading=cpc.LOADING)
    full = engine.capon_power(v, freq, tau, bands=bands)
    assert same_bits(engine.capon_power(v, freq, tau, bands=bands), full)  # a second run
    moved = engine.capon_power(v, freq, np.roll(tau, 41, axis=0), bands=bands)  # every row at another position
    assert same_bits(np.roll(moved, -41, axis=1), full)
    for g in (0, 17, 143, 299):
        alone = engine.capon_power(v, freq, tau[g:g + 1], bands=bands)  # G = 1
        assert same_bits(alone[:, 0], full[:, g]), g
    # the band 4..32 in another table that holds it among others, and as the only band
    other = engine.capon_power(v, freq, tau, bands=[0, 1, 2, 4, 33])
    assert same_bits(other[3], full[2])
    assert same_bits(engine.capon_power(v, freq, tau, bands=[4, 33])[0], full[2])
    # per matrix against a table of one-matrix bands
    assert same_bits(engine.capon_power(v, freq, tau[:37]), engine.capon_power(v, freq, tau[:37], bands=list(range(shape.nf + 1))))


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_matrix_has_the_same_whitener_wherever_it_is_factored(dtype):
    for cid in ("c64_g300_f33_b3", "c17_g17_f33_b3", "c5_g300_f33"):
        s, _, _ = cpc.inputs(bc.by_id(cid), dtype)
        full = engine.csd_whiten(s, loading=cpc.LOADING)
        assert same_bits(engine.csd_whiten(s, loading=cpc.LOADING), full)  # a second run
        for f in (0, 7, 32):
            assert same_bits(engine.csd_whiten(s[f:f + 1], loading=cpc.LOADING)[0], full[f]), (cid, f)  # alone
        assert same_bits(engine.csd_whiten(s[::-1].copy(), loading=cpc.LOADING)[::-1], full)  # at another position
        # only the lower triangle and the real part of the diagonal are read
        hurt = s.copy()
        hurt[:, np.triu(np.ones(s.shape[1:], dtype=bool), 1)] = np.nan
        hurt.imag[:, np.arange(s.shape[1]), np.arange(s.shape[1])] = 3.0
        assert same_bits(engine.csd_whiten(hurt, loading=cpc.LOADING), full)


@pytest.mark.parametrize("dtype", DTYPES)
def test_host_tables_of_more_than_one_upload_chunk(dtype):
    """257 matrices A A^H + I, every one its own band: the frequency table goes to the device in two chunks of kernel
    arguments, 256 values and one (an explicit band table of 258 offsets: 256 and two).  A band's power depends on its own
    matrices alone (include/qi_adaptive.h), so the call has the bits of the calls on matrices 0 .. 255 and on matrix 256."""
    nf, C, G = 257, 5, 15
    rng = np.random.default_rng([37, nf, C, G])
    a = rng.standard_normal((nf, C, C)) + 1j * rng.standard_normal((nf, C, C))
    s = (a @ np.conj(a.transpose(0, 2, 1)) + np.eye(C)).astype(bc.complex_of(dtype))
    freq = rng.uniform(1.0, 40.0, nf)  # (no two alike: a value of the wrong chunk shows)
    tau = rng.uniform(-bc.MAX_DELAY_S, bc.MAX_DELAY_S, (G, C))
    v, info = engine.csd_whiten(s, info=True)
    assert not info.any()
    whole = engine.capon_power(v, freq, tau, peaks=True)
    head = engine.capon_power(v[:256], freq[:256], tau, peaks=True)
    last = engine.capon_power(v[256:], freq[256:], tau, peaks=True)
    assert whole[0].shape == (nf, G) and np.isfinite(whole[0]).all() and whole[0].min() > 0
    for w, h, t in zip(whole, head, last):
        assert same_bits(w, np.concatenate([h, t]))
    table = engine.capon_power(v, freq, tau, bands=np.arange(nf + 1), peaks=True)
    assert all(same_bits(t, w) for t, w in zip(table, whole))


def test_tensors_in_tensors_out_and_both_workgroup_sizes():
    """CUDA tensors stay on the device; a grid that takes the larger workgroup agrees bit for bit with a part of it that
    takes the smaller one."""
    shape = bc.by_id("c16_g37_f33_b3")
    s, freq, _ = cpc.inputs(shape, "float32")
    tau = np.random.default_rng(3).uniform(-bc.MAX_DELAY_S, bc.MAX_DELAY_S, (8200, shape.C))
    s_dev, tau_dev = torch.from_numpy(s).cuda(), torch.from_numpy(tau.astype(np.float32)).cuda()  # (float32 delays are widened)
    v, info = engine.csd_whiten(s_dev, loading=cpc.LOADING, info=True)
    assert v.is_cuda and v.dtype == torch.complex64 and info.is_cuda and info.dtype == torch.int32 and not info.any()
    power, index, value = engine.capon_power(v, freq, tau_dev, peaks=True)
    assert power.is_cuda and power.dtype == torch.float32 and power.shape == (shape.nf, 8200) and index.dtype == torch.int64
    part = engine.capon_power(v, freq, tau_dev[4100:4200])
    assert torch.equal(part, power[:, 4100:4200])
    assert torch.equal(index, torch.argmax(power, dim=1)) and torch.equal(value, power.max(dim=1).values)


# ---- info and NaN -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_info_and_nan_inside_a_stack(dtype):
    shape = bc.by_id("c17_g17_f33_b3")
    s, freq, tau = cpc.inputs(shape, dtype)
    bands = [0, 3, 4, 8, 33]
    cases = {name: (m.astype(s.dtype), loading, want) for name, m, loading, want in cpc.info_cases(shape.C)}
    clean_v = engine.csd_whiten(s, loading=0.0)
    clean_p = engine.capon_power(clean_v, freq, tau, bands=bands)
    hurt = s.copy()
    at = {1: "rank one, no loading", 3: "zero", 5: "NaN diagonal"}
    for f, name in at.items():
        assert cases[name][1] == 0.0
        hurt[f] = cases[name][0]
    v, info = engine.csd_whiten(hurt, loading=0.0, info=True)
    want_info = np.zeros(shape.nf, dtype=np.int32)
    for f, name in at.items():
        want_info[f] = cases[name][2]
    assert np.array_equal(info, want_info), info
    upper = np.triu(np.ones((shape.C, shape.C), dtype=bool))
    good = np.setdiff1d(np.arange(shape.nf), list(at))
    assert same_bits(v[good], clean_v[good])  # the neighbours' bits
    for f in at:
        assert np.isnan(v[f][upper].real).all() and np.isnan(v[f][upper].imag).all() and not bits(v[f][~upper]).any(), f
    power, index, value = engine.capon_power(v, freq, tau, bands=bands, peaks=True)
    assert np.isnan(power[:3]).all() and np.array_equal(index[:3], [0, 0, 0]) and np.isnan(value[:3]).all()  # the first NaN
    assert same_bits(power[3], clean_p[3]) and index[3] == np.argmax(clean_p[3]) and np.array_equal(index, np.argmax(power, axis=1))
    # the rank-one matrix, loaded by half its mean auto-power, factors
    name = "rank one, loaded"
    hurt = s.copy()
    hurt[1] = cases[name][0]
    v, info = engine.csd_whiten(hurt, loading=cases[name][1], info=True)
    assert cases[name][2] == 0 and not info.any() and np.isfinite(v.real).all() and np.isfinite(v.imag).all()
    assert cpc.residual(v[1:2], cpc.loaded(hurt[1:2], cases[name][1], dtype)) <= bc.TOL[dtype]
    assert np.isfinite(engine.capon_power(v, freq, tau, bands=bands)).all()


# ---- Capon <= Bartlett ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cid", ("c5_g15_f7_b2", "c17_g17_f33_b3", "c64_g300_f33_b3", "c33_g15_f33"))
def test_capon_never_exceeds_bartlett_on_the_loaded_matrices(cid, dtype):
    shape = bc.by_id(cid)
    s, freq, tau = cpc.inputs(shape, dtype)
    bands = None if shape.bands is None else list(shape.bands)
    r = cpc.loaded(s, cpc.LOADING, dtype).astype(s.dtype)
    bartlett = engine.beam_power(r, freq, tau, bands=bands).astype(np.float64)
    capon = engine.capon_power(engine.csd_whiten(s, loading=cpc.LOADING), freq, tau, bands=bands).astype(np.float64)
    slack = 2 * bc.TOL[dtype] * np.abs(bartlett).max()  # the two tolerances, each relative to the largest power
    print(f"{cid} {dtype}: largest Capon / Bartlett {float((capon / bartlett).max()):.4f}, smallest {float((capon / bartlett).min()):.4g}")
    assert np.all(capon <= bartlett + slack), (cid, dtype)


# ---- the plane wave, end to end -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def plane_wave_reference():
    freq = np.fft.rfftfreq(bc.PW_SEG, 1 / bc.PW_FS)
    s = cc.restate(bc.pw_records(), bc.pw_case(), "spectrum")
    ref = cpc.capon(cpc.whiten(s, cpc.LOADING), freq, bc.pw_delays(), bc.PW_BANDS)
    ref.setflags(write=False)
    return ref


@pytest.mark.parametrize("dtype", DTYPES)
def test_plane_wave_end_to_end(dtype):
    x = bc.pw_records().astype(dtype)
    slowness = beamform.slowness_grid(bc.PW_MAX_SLOWNESS, bc.PW_GRID_POINTS)
    freq = np.fft.rfftfreq(bc.PW_SEG, 1 / bc.PW_FS)
    edges = [freq[k] for k in bc.PW_BANDS]
    ranges, power, index, value, info = beamform.capon_power_pow2(x, bc.PW_FS, bc.PW_POSITIONS_M, slowness, bc.PW_SEG, bc.PW_OVERLAP,
                                                                 band_edges_hz=edges)
    assert np.array_equal(ranges, [[freq[a], freq[b - 1]] for a, b in zip(bc.PW_BANDS[:-1], bc.PW_BANDS[1:])])
    assert power.shape == (4, 81) and power.dtype == np.dtype(dtype) and info.shape == (len(freq),) and info.dtype == np.int32
    assert not info.any()
    assert np.array_equal(index, np.full(4, bc.pw_true_index())), index
    assert np.array_equal(value, power[np.arange(4), index])
    ratios = [cpc.peak_ratio(row.astype(np.float64))[1] for row in power]
    ref = plane_wave_reference()
    err = float(np.abs(power - ref).max() / np.abs(ref).max())
    print(f"plane wave {dtype}: power / max against the restatement of the float64 records: {err:.3g}; peak / runner-up "
          + ", ".join(f"{r:.2f}" for r in ratios))
    assert min(ratios) >= cpc.PW_RATIO
    if dtype == "float64":  # (the float32 records are other records: their matrices differ by float32 rounding times the condition)
        assert err <= bc.TOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
def test_fewer_segments_than_sensors_without_loading_is_flagged(dtype):
    """Three segments for five sensors: the matrices have rank 3, and without loading pivots 4 and 5 are rounding noise."""
    x = bc.pw_records().astype(dtype)
    slowness = beamform.slowness_grid(bc.PW_MAX_SLOWNESS, bc.PW_GRID_POINTS)
    ranges, power, index, value, info = beamform.capon_power_pow2(x, bc.PW_FS, bc.PW_POSITIONS_M, slowness, 2048, 1024, loading=0.0)
    assert info.shape == (1025,) and power.shape == (1025, 81) and info.any() and info.max() <= 5 and info.min() >= 0
    bad = info != 0
    print(f"three segments, five sensors, no loading, {dtype}: {int(bad.sum())} of 1025 bins flagged, pivots {sorted(set(info[bad].tolist()))}")
    assert np.isnan(power[bad]).all()
    assert np.array_equal(index, np.argmax(power, axis=1)) and np.all(index[bad] == 0)
    # with the default loading every bin factors
    _, power, _, _, info = beamform.capon_power_pow2(x, bc.PW_FS, bc.PW_POSITIONS_M, slowness, 2048, 1024)
    assert not info.any() and np.isfinite(power).all()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    shape = bc.by_id("c5_g15_f7_b2")
    s, freq, tau = cpc.inputs(shape, "float32")
    with pytest.raises(_lib.QiError, match="sensors"):
        engine.capon_power(np.zeros((2, 65, 65), dtype=np.complex64), [1.0, 2.0], np.zeros((3, 65)))
    with pytest.raises(_lib.QiError, match="sensors"):
        engine.csd_whiten(np.zeros((2, 65, 65), dtype=np.complex64))
    for loading in (-1e-3, float("nan"), float("inf")):
        with pytest.raises(_lib.QiError, match="loading"):
            engine.csd_whiten(s, loading=loading)
    with pytest.raises(ValueError):
        engine.csd_whiten(np.zeros((2, 5, 4), dtype=np.complex64))
    v = engine.csd_whiten(s, loading=cpc.LOADING)
    for bands in ([0, 4, 2, 7], [0, 3, 3, 7], [7, 8], [0, 3, 8], [-1, 3]):
        with pytest.raises(_lib.QiError, match="band offsets"):
            engine.capon_power(v, freq, tau, bands=bands)
    # through the C ABI: refused before anything is queued -- the buffers keep their fill
    lib = _lib.require_gpu()
    dev = engine.default_device()
    s_dev, v_dev, tau_dev = torch.from_numpy(s).to(dev), torch.from_numpy(v).to(dev), torch.from_numpy(tau).to(dev)
    index = torch.full((shape.nf,), -7, dtype=torch.int64, device=dev)
    info = torch.full((shape.nf,), -7, dtype=torch.int32, device=dev)
    out = torch.full_like(s_dev, 0.3125)
    scratch, nbytes = _lib.scratch(lib.qi_beam_capon_scratch_bytes, dev, _lib.QI_F32, shape.C, shape.nf, shape.G, shape.nf)
    f_host, f_ptr = _lib.darr(freq)
    with pytest.raises(_lib.QiError, match="null"):
        _lib.call(lib.qi_csd_whiten, dev, _lib.QI_F32, dev.index, _lib.ptr(s_dev), shape.C, shape.nf, 0.0, None, _lib.ptr(info))
    with pytest.raises(_lib.QiError, match="loading"):
        _lib.call(lib.qi_csd_whiten, dev, _lib.QI_F32, dev.index, _lib.ptr(s_dev), shape.C, shape.nf, -1.0, _lib.ptr(out), _lib.ptr(info))
    with pytest.raises(_lib.QiError, match="misaligned"):
        _lib.call(lib.qi_csd_whiten, dev, _lib.QI_F32, dev.index, _lib.ptr(s_dev), shape.C, shape.nf, 0.0, ctypes.c_void_p(out.data_ptr() + 4),
                  _lib.ptr(info))
    with pytest.raises(_lib.QiError, match="power is null"):
        _lib.call(lib.qi_beam_capon, dev, _lib.QI_F32, dev.index, _lib.ptr(v_dev), shape.C, shape.nf, f_ptr, _lib.ptr(tau_dev), shape.G,
                  None, shape.nf, None, _lib.ptr(index), None, _lib.ptr(scratch), nbytes)
    power = torch.empty((shape.nf, shape.G), dtype=torch.float32, device=dev)
    with pytest.raises(_lib.QiError, match="scratch"):
        _lib.call(lib.qi_beam_capon, dev, _lib.QI_F32, dev.index, _lib.ptr(v_dev), shape.C, shape.nf, f_ptr, _lib.ptr(tau_dev), shape.G,
                  None, shape.nf, _lib.ptr(power), _lib.ptr(index), None, _lib.ptr(scratch), nbytes - 1)
    with pytest.raises(_lib.QiError, match="misaligned"):
        off = ctypes.c_void_p(scratch.data_ptr() + 8)
        _lib.call(lib.qi_beam_capon, dev, _lib.QI_F32, dev.index, _lib.ptr(v_dev), shape.C, shape.nf, f_ptr, _lib.ptr(tau_dev), shape.G,
                  None, shape.nf, _lib.ptr(power), _lib.ptr(index), None, off, nbytes)
    torch.cuda.synchronize()
    assert torch.equal(index, torch.full_like(index, -7)) and torch.equal(info, torch.full_like(info, -7))
    assert torch.equal(out, torch.full_like(out, 0.3125))
