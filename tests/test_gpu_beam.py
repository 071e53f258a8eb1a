"""Beamforming on the device (-m gpu): qi_beam_power against the NumPy restatement of tests/beam_cases.py at ragged and full
tiles in both precisions, an exact case bit for bit, the determinism contract of include/qi_beam.h, the peak rules, the
plane-wave case end to end through beamform.fk_power_pow2, and the refusals."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import beam_cases as bc
import csd_cases as cc

from quantum_inferno_amd import _lib, beamform, engine

pytestmark = pytest.mark.gpu

DTYPES = bc.DTYPES


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def reference(cid, dtype, normalize):
    """The float64 restatement on the values the device reads: computed once, shared, left unchanged."""
    shape = bc.by_id(cid)
    s, freq, tau = bc.inputs(shape, dtype)
    ref = bc.restate(s, freq, tau, shape.bands, normalize)
    ref.setflags(write=False)
    return ref


# ---- against the restatement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cid", bc.ids())
def test_power_and_semblance_match_the_restatement(cid, dtype):
    shape = bc.by_id(cid)
    s, freq, tau = bc.inputs(shape, dtype)
    bands = None if shape.bands is None else list(shape.bands)
    nb = shape.nf if bands is None else len(bands) - 1
    for normalize in (False, True):
        ref = reference(cid, dtype, normalize)
        got, index, value = engine.beam_power(s, freq, tau, bands=bands, normalize=normalize, peaks=True)
        assert got.dtype == np.dtype(dtype) and got.shape == (nb, shape.G) == ref.shape
        scale = 1.0 if normalize else np.abs(ref).max()
        err = float(np.abs(got.astype(np.float64) - ref).max() / scale)
        print(f"{cid} {dtype} {'semblance (absolute)' if normalize else 'power / max power'}: {err:.3g}")
        assert err <= bc.TOL[dtype], (cid, dtype, normalize)
        if normalize:
            assert np.isfinite(got).all() and got.max() <= 1 + bc.TOL[dtype] and got.min() >= -bc.TOL[dtype]
        want_index, want_value = bc.peaks_of(got)
        assert index.dtype == np.int64 and np.array_equal(index, want_index) and same_bits(value, want_value)


# ---- the exact case -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", (17, 33))
def test_exact_integer_case_bit_for_bit(C, dtype):
    """Every factor is +-1 or +-i and every sum an integer below 2^24: an operand or a result-row map of the other precision,
    a conjugation or a transposed matrix shows as a wrong integer."""
    nf, G = 33, 37
    s, freq, tau, turns4 = bc.exact_inputs(C, nf, G)
    for bands in (None, [0, 3, 4, 33]):
        q, tr = bc.exact_sums(s, turns4, bands)
        power = engine.beam_power(s.astype(bc.complex_of(dtype)), freq, tau, bands=bands)
        assert same_bits(power, (q / float(C * C)).astype(dtype)), (C, dtype, bands, np.argwhere(power != (q / C ** 2).astype(dtype))[:4])
        sem = engine.beam_power(s.astype(bc.complex_of(dtype)), freq, tau, bands=bands, normalize=True)
        assert same_bits(sem, (q / (float(C) * tr[:, None])).astype(dtype)), (C, dtype, bands)


# ---- determinism --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_grid_point_has_the_same_bits_wherever_it_is_computed(dtype):
    shape = bc.by_id("c64_g300_f33_b3")
    s, freq, tau = bc.inputs(shape, dtype)
    bands = list(shape.bands)
    full = engine.beam_power(s, freq, tau, bands=bands, normalize=True)
    assert same_bits(engine.beam_power(s, freq, tau, bands=bands, normalize=True), full)  # a second run
    moved = engine.beam_power(s, freq, np.roll(tau, 41, axis=0), bands=bands, normalize=True)  # every row at another position
    assert same_bits(np.roll(moved, -41, axis=1), full)
    for g in (0, 17, 143, 299):
        alone = engine.beam_power(s, freq, tau[g:g + 1], bands=bands, normalize=True)  # G = 1
        assert same_bits(alone[:, 0], full[:, g]), g
    # the band 4..32 in another table that holds it among others, and as the only band
    other = engine.beam_power(s, freq, tau, bands=[0, 1, 2, 4, 33], normalize=True)
    assert same_bits(other[3], full[2])
    assert same_bits(engine.beam_power(s, freq, tau, bands=[4, 33], normalize=True)[0], full[2])
    # and unnormalised, per matrix against a table of one-matrix bands
    assert same_bits(engine.beam_power(s, freq, tau[:37]), engine.beam_power(s, freq, tau[:37], bands=list(range(shape.nf + 1))))


@pytest.mark.parametrize("dtype", DTYPES)
def test_equal_delay_rows_give_equal_bits_and_the_lower_peak(dtype):
    shape = bc.by_id("c17_g17_f33_b3")
    s, freq, tau = bc.inputs(shape, dtype)
    bands = list(shape.bands)
    power = engine.beam_power(s, freq, tau, bands=bands)
    best = np.argmax(power, axis=1)
    for b in range(len(bands) - 1):
        twice = tau.copy()
        lo, hi = sorted((int(best[b]), (int(best[b]) + 9) % shape.G))
        twice[lo] = twice[hi] = tau[best[b]]
        got, index, value = engine.beam_power(s, freq, twice, bands=bands, peaks=True)
        assert same_bits(got[:, lo], got[:, hi]) and same_bits(got[:, lo], power[:, best[b]])
        assert index[b] == lo and value[b] == got[b, lo]


@pytest.mark.parametrize("dtype", DTYPES)
def test_host_tables_of_more_than_one_upload_chunk(dtype):
    """257 matrices, every one its own band: the frequency table goes to the device in two chunks of kernel arguments, 256
    values and one (an explicit band table of 258 offsets: 256 and two).  A band's power depends on its own matrices alone
    (include/qi_beam.h), so the call has the bits of the calls on matrices 0 .. 255 and on matrix 256."""
    nf, C, G = 257, 5, 15
    rng = np.random.default_rng([31, nf, C, G])
    a = rng.standard_normal((nf, C, C)) + 1j * rng.standard_normal((nf, C, C))
    s = (a @ np.conj(a.transpose(0, 2, 1)) + np.eye(C)).astype(bc.complex_of(dtype))
    freq = rng.uniform(1.0, 40.0, nf)  # (no two alike: a value of the wrong chunk shows)
    tau = rng.uniform(-bc.MAX_DELAY_S, bc.MAX_DELAY_S, (G, C))
    for normalize in (False, True):
        whole = engine.beam_power(s, freq, tau, normalize=normalize, peaks=True)
        head = engine.beam_power(s[:256], freq[:256], tau, normalize=normalize, peaks=True)
        last = engine.beam_power(s[256:], freq[256:], tau, normalize=normalize, peaks=True)
        assert whole[0].shape == (nf, G) and np.isfinite(whole[0]).all()
        for w, h, t in zip(whole, head, last):
            assert same_bits(w, np.concatenate([h, t])), normalize
        table = engine.beam_power(s, freq, tau, bands=np.arange(nf + 1), normalize=normalize, peaks=True)
        assert all(same_bits(t, w) for t, w in zip(table, whole)), normalize


# ---- peaks ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_peak_rules_with_nan(dtype):
    shape = bc.by_id("c5_g300_f33")
    s, freq, tau = bc.inputs(shape, dtype)
    bands = [0, 3, 4, 33]
    # a NaN delay in row 3: column 3 is NaN in every band, and the first NaN is the peak
    bad = tau.copy()
    bad[3, 2] = np.nan
    bad[200, 0] = np.nan
    power, index, value = engine.beam_power(s, freq, bad, bands=bands, normalize=True, peaks=True)
    assert np.isnan(power[:, 3]).all() and np.isnan(power[:, 200]).all() and np.isfinite(np.delete(power, (3, 200), axis=1)).all()
    assert np.array_equal(index, [3, 3, 3]) and np.isnan(value).all()
    assert np.array_equal(index, np.argmax(power, axis=1))
    # a NaN matrix: its band's row is NaN and its index 0; the other bands are untouched
    clean = engine.beam_power(s, freq, tau, bands=bands)
    hurt = s.copy()
    hurt[3, 1, 2] = np.nan
    power, index, value = engine.beam_power(hurt, freq, tau, bands=bands, peaks=True)
    assert np.isnan(power[1]).all() and index[1] == 0 and np.isnan(value[1])
    assert same_bits(power[[0, 2]], clean[[0, 2]]) and np.array_equal(index[[0, 2]], np.argmax(clean[[0, 2]], axis=1))
    # a band whose matrices are all zero: the semblance is NaN, the power 0
    zero = s.copy()
    zero[0:3] = 0
    sem, index, value = engine.beam_power(zero, freq, tau, bands=bands, normalize=True, peaks=True)
    assert np.isnan(sem[0]).all() and index[0] == 0 and np.isfinite(sem[1:]).all()
    assert np.array_equal(engine.beam_power(zero, freq, tau, bands=bands)[0], np.zeros(shape.G, dtype=dtype))


def test_tensors_in_tensors_out_and_large_grids():
    """CUDA tensors stay on the device; a grid of several workgroups of both sizes agrees with itself in parts."""
    shape = bc.by_id("c16_g37_f33_b3")
    s, freq, _ = bc.inputs(shape, "float32")
    tau = np.random.default_rng(3).uniform(-bc.MAX_DELAY_S, bc.MAX_DELAY_S, (8200, shape.C))
    s_dev, tau_dev = torch.from_numpy(s).cuda(), torch.from_numpy(tau.astype(np.float32)).cuda()  # (float32 delays are widened)
    power, index, value = engine.beam_power(s_dev, freq, tau_dev, peaks=True)
    assert power.is_cuda and power.dtype == torch.float32 and power.shape == (shape.nf, 8200) and index.dtype == torch.int64
    part = engine.beam_power(s_dev, freq, tau_dev[4100:4200])
    assert torch.equal(part, power[:, 4100:4200])
    assert torch.equal(index, torch.argmax(power, dim=1)) and torch.equal(value, power.max(dim=1).values)


# ---- the plane wave, end to end -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_plane_wave_end_to_end(dtype):
    x = bc.pw_records().astype(dtype)
    slowness = beamform.slowness_grid(bc.PW_MAX_SLOWNESS, bc.PW_GRID_POINTS)
    assert np.allclose(slowness.numpy(), bc.pw_slowness(), rtol=0, atol=1e-18)
    freq = np.fft.rfftfreq(bc.PW_SEG, 1 / bc.PW_FS)
    edges = [freq[k] for k in bc.PW_BANDS]
    assert np.array_equal(beamform.band_offsets(freq, edges), bc.PW_BANDS)
    ranges, power, index, value = beamform.fk_power_pow2(x, bc.PW_FS, bc.PW_POSITIONS_M, slowness, bc.PW_SEG, bc.PW_OVERLAP,
                                                         band_edges_hz=edges)
    assert np.array_equal(ranges, [[freq[a], freq[b - 1]] for a, b in zip(bc.PW_BANDS[:-1], bc.PW_BANDS[1:])])
    assert power.shape == (4, 81) and power.dtype == np.dtype(dtype)
    assert np.array_equal(index, np.full(4, bc.pw_true_index())), index
    assert np.array_equal(value, power[np.arange(4), index]) and value.min() > 0.5 and power.max() <= 1 + bc.TOL[dtype]
    ref = bc.restate(cc.restate(bc.pw_records(), bc.pw_case(), "spectrum"), freq, bc.pw_delays(), bc.PW_BANDS, normalize=True)
    print(f"plane wave {dtype}: semblance against the restatement of the float64 records: {float(np.abs(power - ref).max()):.3g}; "
          f"best {value.min():.3f} .. {value.max():.3f}")
    az, v = beamform.back_azimuth_and_velocity(slowness[torch.from_numpy(index)])
    want_az, want_v = bc.pw_true_azimuth_velocity()
    assert np.allclose(az.numpy(), want_az, rtol=0, atol=1e-9) and np.allclose(v.numpy(), want_v, rtol=1e-12)
    # polar grids: the source's (azimuth, velocity) steered directly is the same row of delays
    polar = beamform.polar_slowness_grid([0.0, want_az, 90.0], [340.0, want_v])
    assert polar.shape == (6, 2) and np.allclose(polar[4].numpy(), bc.pw_slowness()[bc.pw_true_index()], rtol=1e-12)
    tau = beamform.plane_wave_delays(bc.PW_POSITIONS_M, slowness)
    assert tau.is_cuda and tau.dtype == torch.float64 and np.allclose(tau.cpu().numpy(), bc.pw_delays(), rtol=0, atol=1e-15)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    shape = bc.by_id("c5_g15_f7_b2")
    s, freq, tau = bc.inputs(shape, "float32")
    with pytest.raises(_lib.QiError, match="sensors"):
        engine.beam_power(np.zeros((2, 65, 65), dtype=np.complex64), [1.0, 2.0], np.zeros((3, 65)))
    for bands in ([0, 4, 2, 7], [0, 3, 3, 7], [7, 8], [0, 3, 8], [-1, 3]):
        with pytest.raises(_lib.QiError, match="band offsets"):
            engine.beam_power(s, freq, tau, bands=bands)
    # power = NULL through the C ABI: refused before anything is queued -- the peak buffers keep their fill
    lib = _lib.require_gpu()
    dev = engine.default_device()
    s_dev, tau_dev = torch.from_numpy(s).to(dev), torch.from_numpy(tau).to(dev)
    index = torch.full((shape.nf,), -7, dtype=torch.int64, device=dev)
    scratch, nbytes = _lib.scratch(lib.qi_beam_power_scratch_bytes, dev, _lib.QI_F32, shape.C, shape.nf, shape.G, shape.nf)
    f_host, f_ptr = _lib.darr(freq)
    with pytest.raises(_lib.QiError, match="power is null"):
        _lib.call(lib.qi_beam_power, dev, _lib.QI_F32, dev.index, _lib.ptr(s_dev), shape.C, shape.nf, f_ptr, _lib.ptr(tau_dev), shape.G,
                  None, shape.nf, 0, None, _lib.ptr(index), None, _lib.ptr(scratch), nbytes)
    with pytest.raises(_lib.QiError, match="scratch"):
        power = torch.empty((shape.nf, shape.G), dtype=torch.float32, device=dev)
        _lib.call(lib.qi_beam_power, dev, _lib.QI_F32, dev.index, _lib.ptr(s_dev), shape.C, shape.nf, f_ptr, _lib.ptr(tau_dev), shape.G,
                  None, shape.nf, 0, _lib.ptr(power), _lib.ptr(index), None, _lib.ptr(scratch), nbytes - 1)
    with pytest.raises(_lib.QiError, match="misaligned"):
        off = ctypes.c_void_p(scratch.data_ptr() + 8)
        _lib.call(lib.qi_beam_power, dev, _lib.QI_F32, dev.index, _lib.ptr(s_dev), shape.C, shape.nf, f_ptr, _lib.ptr(tau_dev), shape.G,
                  None, shape.nf, 0, _lib.ptr(power), _lib.ptr(index), None, off, nbytes)
    torch.cuda.synchronize()
    assert torch.equal(index, torch.full_like(index, -7))
