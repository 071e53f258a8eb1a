"""MUSIC beamforming on the device (-m gpu): qi_csd_eigh and qi_beam_music against the NumPy restatements of
tests/music_cases.py at ragged and full tiles in both precisions, the exact (diagonal) cases bit for bit, the determinism
contracts of include/qi_subspace.h, `info` and the NaN rules, rank-deficient matrices, n_sources = 0, the plane-wave case end to
end through beamform.music_power_pow2, and the refusals.

The bounds are the project's reduction tolerances, 1e-4 (float32) and 1e-10 (float64): the eigenvalues as a fraction of the
largest, max |U^H U - I|, max |S U - U diag(w)| over the largest eigenvalue, the noise projector and 1 / power absolute (the
reciprocal: the power itself is unboundedly sensitive where the null spectrum goes to 0)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import beam_cases as bc
import csd_cases as cc
import music_cases as mc

from quantum_inferno_amd import _lib, beamform, engine

pytestmark = pytest.mark.gpu

DTYPES = bc.DTYPES


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def reference(cid, dtype):
    """The float64 restatements on the values the device reads: computed once, shared, left unchanged ->
    (eigenvalues, eigenvectors, noise projector, 1 / power)."""
    shape = bc.by_id(cid)
    s, freq, tau, k = mc.inputs(shape, dtype)
    w, u = mc.eigh64(s)
    out = (w, u, mc.noise_projector(u, k), 1.0 / mc.music(u, k, freq, tau, shape.bands))
    for a in out:
        a.setflags(write=False)
    return out


# ---- against the restatement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cid", bc.ids())
def test_eigenpairs_and_power_match_the_restatement(cid, dtype):
    shape = bc.by_id(cid)
    s, freq, tau, k = mc.inputs(shape, dtype)
    bands = None if shape.bands is None else list(shape.bands)
    nb = shape.nf if bands is None else len(bands) - 1
    ref_w, ref_u, ref_proj, ref_inv = reference(cid, dtype)
    w, u, info = engine.csd_eigh(s, info=True)
    assert w.dtype == np.dtype(dtype) and w.shape == (shape.nf, shape.C) and u.dtype == s.dtype and u.shape == s.shape
    assert info.dtype == np.int32 and not info.any()
    assert np.all(np.diff(w, axis=1) >= 0)
    err_w = float(np.abs(w - ref_w).max() / np.abs(ref_w).max())
    ortho, pairs = mc.residuals(w, u, s)
    err_proj = float(np.abs(mc.noise_projector(u, k) - ref_proj).max())
    # the form fed the restated eigenvectors, and end to end through the kernel's own
    fed = engine.music_power(ref_u.astype(s.dtype), k, freq, tau, bands=bands)
    got, index, value = engine.music_power(u, k, freq, tau, bands=bands, peaks=True)
    assert got.dtype == np.dtype(dtype) and got.shape == (nb, shape.G) == ref_inv.shape == fed.shape
    err_fed = float(np.abs(1.0 / fed.astype(np.float64) - ref_inv).max())
    err_end = float(np.abs(1.0 / got.astype(np.float64) - ref_inv).max())
    print(f"{cid} {dtype}: eigenvalues / max {err_w:.3g}, max |U^H U - I| {ortho:.3g}, max |S U - U w| / max w {pairs:.3g}, noise projector "
          f"{err_proj:.3g}, 1 / power: fed the restated eigenvectors {err_fed:.3g}, end to end {err_end:.3g}")
    tol = bc.TOL[dtype]
    assert err_w <= tol and ortho <= tol and pairs <= tol and err_proj <= tol and err_fed <= tol and err_end <= tol, (cid, dtype)
    assert np.isfinite(got).all() and got.min() >= 1 - tol
    want_index, want_value = bc.peaks_of(got)
    assert index.dtype == np.int64 and np.array_equal(index, want_index) and same_bits(value, want_value)


@pytest.mark.parametrize("dtype", DTYPES)
def test_no_sources_gives_one(dtype):
    for cid in ("c5_g15_f7_b2", "c64_g300_f33_b3", "c17_g1_f7"):
        shape = bc.by_id(cid)
        s, freq, tau, _ = mc.inputs(shape, dtype)
        _, u = engine.csd_eigh(s)
        power = engine.music_power(u, 0, freq, tau, bands=None if shape.bands is None else list(shape.bands))
        err = float(np.abs(power.astype(np.float64) - 1).max())
        print(f"{cid} {dtype}: n_sources = 0, max |power - 1| {err:.3g}")
        assert err <= bc.TOL[dtype], (cid, dtype)


# ---- the exact cases --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", (5, 17, 64))
def test_diagonal_matrices_bit_for_bit(C, dtype):
    """No rotation is taken: the eigenvalues are the sorted diagonal, the eigenvectors the columns of a permutation matrix (the
    repeated value of the last matrix: the lower position first).  With quarter-turn phases every |U_j^H e|^2 is 1: D = m."""
    nf, G = 9, 37
    s, want_w, want_u, freq, tau, turns4 = mc.exact_inputs(C, nf, G)
    w, u, info = engine.csd_eigh(s.astype(bc.complex_of(dtype)), info=True)
    assert not info.any()
    assert same_bits(w, want_w.astype(dtype)), (C, dtype)
    assert same_bits(u, want_u.astype(bc.complex_of(dtype))), (C, dtype, np.argwhere(u != want_u)[:4])
    assert np.array_equal(4 * bc.reduced_turns(freq, tau) % 4, turns4 % 4)
    for k in (0, 1, C - 1):
        for bands in (None, [0, 3, 4, 9]):
            power = engine.music_power(u, k, freq, tau, bands=bands)
            want = np.full(power.shape, np.dtype(dtype).type(float(C) / float(C - k)))  # C n_b / (n_b m), rounded once
            assert same_bits(power, want), (C, dtype, k, bands)


# ---- determinism --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_matrix_has_the_same_eigenpairs_wherever_it_is_solved(dtype):
    for cid in ("c64_g300_f33_b3", "c17_g17_f33_b3", "c5_g300_f33"):
        s, _, _, _ = mc.inputs(bc.by_id(cid), dtype)
        full = engine.csd_eigh(s, info=True)
        again = engine.csd_eigh(s, info=True)  # a second run
        assert all(same_bits(a, b) for a, b in zip(again, full)), cid
        for f in (0, 7, 32):
            alone = engine.csd_eigh(s[f:f + 1], info=True)
            assert all(same_bits(a[0], b[f]) for a, b in zip(alone, full)), (cid, f)
        moved = engine.csd_eigh(s[::-1].copy(), info=True)  # at another position
        assert all(same_bits(a[::-1], b) for a, b in zip(moved, full)), cid
        # only the lower triangle and the real part of the diagonal are read
        hurt = s.copy()
        hurt[:, np.triu(np.ones(s.shape[1:], dtype=bool), 1)] = np.nan
        hurt.imag[:, np.arange(s.shape[1]), np.arange(s.shape[1])] = 3.0
        assert all(same_bits(a, b) for a, b in zip(engine.csd_eigh(hurt, info=True), full)), cid


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_grid_point_has_the_same_bits_wherever_it_is_computed(dtype):
    shape = bc.by_id("c64_g300_f33_b3")
    s, freq, tau, k = mc.inputs(shape, dtype)
    bands = list(shape.bands)
    _, u = engine.csd_eigh(s)
    full = engine.music_power(u, k, freq, tau, bands=bands)
    assert same_bits(engine.music_power(u, k, freq, tau, bands=bands), full)  # a second run
    moved = engine.music_power(u, k, freq, np.roll(tau, 41, axis=0), bands=bands)  # every row at another position
    assert same_bits(np.roll(moved, -41, axis=1), full)
    for g in (0, 17, 143, 299):
        alone = engine.music_power(u, k, freq, tau[g:g + 1], bands=bands)  # G = 1
        assert same_bits(alone[:, 0], full[:, g]), g
    # the band 4..32 in another table that holds it among others, and as the only band
    other = engine.music_power(u, k, freq, tau, bands=[0, 1, 2, 4, 33])
    assert same_bits(other[3], full[2])
    assert same_bits(engine.music_power(u, k, freq, tau, bands=[4, 33])[0], full[2])
    # a grid that takes the larger workgroup (33 bands x 300 tiles of 16 over 8 waves) against the smaller one's rows
    wide = np.concatenate([tau] * 16)
    per_bin = engine.music_power(u, k, freq, tau)
    assert same_bits(engine.music_power(u, k, freq, wide)[:, 4500:4800], per_bin)


# ---- info and NaN -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_info_and_nan_inside_a_stack(dtype):
    """The four cases of music_cases.info_cases inside a stack: a NaN or an inf below the diagonal ends at info 1 and NaN
    outputs, the same value above the diagonal is not read."""
    shape = bc.by_id("c17_g17_f33_b3")
    s, freq, tau, k = mc.inputs(shape, dtype)
    bands = [0, 3, 4, 8, 33]
    cases = mc.info_cases(shape.C)
    at = {1: 0, 2: 1, 3: 2, 5: 2, 9: 3}  # matrix -> case
    clean_s, hurt = s.copy(), s.copy()
    for f, c in at.items():
        clean_s[f] = mc.info_base(shape.C).astype(s.dtype)
        hurt[f] = cases[c][1].astype(s.dtype)
    clean = engine.csd_eigh(clean_s, info=True)
    clean_p = engine.music_power(clean[1], k, freq, tau, bands=bands)
    assert not clean[2].any() and np.isfinite(clean_p).all()
    w, u, info = engine.csd_eigh(hurt, info=True)
    want_info = np.zeros(shape.nf, dtype=np.int32)
    for f, c in at.items():
        want_info[f] = cases[c][2]
    assert np.array_equal(info, want_info) and sorted(np.flatnonzero(info)) == [1, 3, 5], info
    good = info == 0
    assert same_bits(w[good], clean[0][good]) and same_bits(u[good], clean[1][good])  # the neighbours' bits, the ignored values
    assert np.isnan(w[~good]).all() and np.isnan(u[~good].real).all() and np.isnan(u[~good].imag).all()
    power, index, value = engine.music_power(u, k, freq, tau, bands=bands, peaks=True)
    assert np.isnan(power[:3]).all() and np.array_equal(index[:3], [0, 0, 0]) and np.isnan(value[:3]).all()  # the first NaN
    assert same_bits(power[3], clean_p[3]) and index[3] == np.argmax(clean_p[3]) and np.array_equal(index, np.argmax(power, axis=1))


# ---- the plane wave, end to end -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_plane_wave_end_to_end(dtype):
    x = bc.pw_records().astype(dtype)
    slowness = beamform.slowness_grid(bc.PW_MAX_SLOWNESS, bc.PW_GRID_POINTS)
    freq = np.fft.rfftfreq(bc.PW_SEG, 1 / bc.PW_FS)
    edges = [freq[k] for k in bc.PW_BANDS]
    ranges, power, index, value, info = beamform.music_power_pow2(x, bc.PW_FS, bc.PW_POSITIONS_M, slowness, bc.PW_SEG, bc.PW_OVERLAP,
                                                                 band_edges_hz=edges, n_sources=1)
    assert np.array_equal(ranges, [[freq[a], freq[b - 1]] for a, b in zip(bc.PW_BANDS[:-1], bc.PW_BANDS[1:])])
    assert power.shape == (4, 81) and power.dtype == np.dtype(dtype) and info.shape == (len(freq),) and info.dtype == np.int32
    assert not info.any()
    assert np.array_equal(index, np.full(4, bc.pw_true_index())), index
    assert np.array_equal(value, power[np.arange(4), index])
    ratios = [mc.peak_ratio(row.astype(np.float64))[1] for row in power]
    print(f"plane wave {dtype}: peak / runner-up " + ", ".join(f"{r:.2f}" for r in ratios))
    if dtype == "float64":  # (the float32 records are other records)
        s = cc.restate(bc.pw_records(), bc.pw_case(), "spectrum")
        ref = 1.0 / mc.music(mc.eigh64(s)[1], 1, freq, bc.pw_delays(), bc.PW_BANDS)
        assert float(np.abs(1.0 / power - ref).max()) <= bc.TOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
def test_fewer_segments_than_sensors_converges(dtype):
    """Three segments for five sensors: the matrices have rank 3 at most, two eigenvalues are rounding noise around 0.  There is
    no loading here and none is needed: every bin converges."""
    x = bc.pw_records().astype(dtype)
    slowness = beamform.slowness_grid(bc.PW_MAX_SLOWNESS, bc.PW_GRID_POINTS)
    ranges, power, index, value, info = beamform.music_power_pow2(x, bc.PW_FS, bc.PW_POSITIONS_M, slowness, 2048, 1024)
    assert info.shape == (1025,) and power.shape == (1025, 81) and not info.any()
    assert np.isfinite(power).all() and power.min() >= 1 - bc.TOL[dtype]
    assert np.array_equal(index, np.argmax(power, axis=1))
    csd = beamform._array_matrices(x, bc.PW_FS, bc.PW_POSITIONS_M, slowness, 2048, 1024, None, 0.25, None)[2]  # (on the device)
    w, u, s = (t.cpu().numpy() for t in (*engine.csd_eigh(csd), csd))
    small = float(np.abs(w[:, :2]).max() / np.abs(w).max())
    print(f"three segments, five sensors, {dtype}: largest of the two null eigenvalues / largest eigenvalue {small:.3g}")
    assert small <= bc.TOL[dtype] and mc.residuals(w, u, s)[0] <= bc.TOL[dtype]


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    shape = bc.by_id("c5_g15_f7_b2")
    s, freq, tau, k = mc.inputs(shape, "float32")
    with pytest.raises(_lib.QiError, match="sensors"):
        engine.music_power(np.zeros((2, 65, 65), dtype=np.complex64), 1, [1.0, 2.0], np.zeros((3, 65)))
    with pytest.raises(_lib.QiError, match="sensors"):
        engine.csd_eigh(np.zeros((2, 65, 65), dtype=np.complex64))
    with pytest.raises(ValueError):
        engine.csd_eigh(np.zeros((2, 5, 4), dtype=np.complex64))
    _, u = engine.csd_eigh(s)
    for n in (-1, shape.C, shape.C + 3):
        with pytest.raises(_lib.QiError, match="sources"):
            engine.music_power(u, n, freq, tau)
    with pytest.raises(ValueError):
        engine.music_power(u, 1.5, freq, tau)
    for bands in ([0, 4, 2, 7], [0, 3, 3, 7], [7, 8], [0, 3, 8], [-1, 3]):
        with pytest.raises(_lib.QiError, match="band offsets"):
            engine.music_power(u, k, freq, tau, bands=bands)
    # through the C ABI: refused before anything is queued -- the buffers keep their fill
    lib = _lib.require_gpu()
    dev = engine.default_device()
    s_dev, u_dev, tau_dev = torch.from_numpy(s).to(dev), torch.from_numpy(u).to(dev), torch.from_numpy(tau).to(dev)
    index = torch.full((shape.nf,), -7, dtype=torch.int64, device=dev)
    info = torch.full((shape.nf,), -7, dtype=torch.int32, device=dev)
    out = torch.full_like(s_dev, 0.3125)
    values = torch.full((shape.nf, shape.C), 0.3125, dtype=torch.float32, device=dev)
    scratch, nbytes = _lib.scratch(lib.qi_beam_music_scratch_bytes, dev, _lib.QI_F32, shape.C, shape.nf, shape.G, shape.nf)
    f_host, f_ptr = _lib.darr(freq)
    with pytest.raises(_lib.QiError, match="null"):
        _lib.call(lib.qi_csd_eigh, dev, _lib.QI_F32, dev.index, _lib.ptr(s_dev), shape.C, shape.nf, _lib.ptr(values), None, _lib.ptr(info))
    with pytest.raises(_lib.QiError, match="null"):
        _lib.call(lib.qi_csd_eigh, dev, _lib.QI_F32, dev.index, _lib.ptr(s_dev), shape.C, shape.nf, None, _lib.ptr(out), _lib.ptr(info))
    with pytest.raises(_lib.QiError, match="misaligned"):
        _lib.call(lib.qi_csd_eigh, dev, _lib.QI_F32, dev.index, _lib.ptr(s_dev), shape.C, shape.nf, _lib.ptr(values),
                  ctypes.c_void_p(out.data_ptr() + 4), _lib.ptr(info))
    power = torch.full((shape.nf, shape.G), 0.3125, dtype=torch.float32, device=dev)
    with pytest.raises(_lib.QiError, match="sources"):
        _lib.call(lib.qi_beam_music, dev, _lib.QI_F32, dev.index, _lib.ptr(u_dev), shape.C, shape.nf, shape.C, f_ptr, _lib.ptr(tau_dev),
                  shape.G, None, shape.nf, _lib.ptr(power), _lib.ptr(index), None, _lib.ptr(scratch), nbytes)
    with pytest.raises(_lib.QiError, match="power is null"):
        _lib.call(lib.qi_beam_music, dev, _lib.QI_F32, dev.index, _lib.ptr(u_dev), shape.C, shape.nf, 1, f_ptr, _lib.ptr(tau_dev), shape.G,
                  None, shape.nf, None, _lib.ptr(index), None, _lib.ptr(scratch), nbytes)
    with pytest.raises(_lib.QiError, match="scratch"):
        _lib.call(lib.qi_beam_music, dev, _lib.QI_F32, dev.index, _lib.ptr(u_dev), shape.C, shape.nf, 1, f_ptr, _lib.ptr(tau_dev), shape.G,
                  None, shape.nf, _lib.ptr(power), _lib.ptr(index), None, _lib.ptr(scratch), nbytes - 1)
    with pytest.raises(_lib.QiError, match="misaligned"):
        off = ctypes.c_void_p(scratch.data_ptr() + 8)
        _lib.call(lib.qi_beam_music, dev, _lib.QI_F32, dev.index, _lib.ptr(u_dev), shape.C, shape.nf, 1, f_ptr, _lib.ptr(tau_dev), shape.G,
                  None, shape.nf, _lib.ptr(power), _lib.ptr(index), None, off, nbytes)
    torch.cuda.synchronize()
    assert torch.equal(index, torch.full_like(index, -7)) and torch.equal(info, torch.full_like(info, -7))
    assert torch.equal(out, torch.full_like(out, 0.3125)) and torch.equal(values, torch.full_like(values, 0.3125))
    assert torch.equal(power, torch.full_like(power, 0.3125))
