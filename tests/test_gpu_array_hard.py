"""The array factorisations on the device (-m gpu) on the matrices their own tests never draw and at every sensor count:
qi_csd_eigh on the families of tests/array_hard_cases.py (repeated, rank-one, graded, indefinite and paired spectra, a dead
sensor, twin sensors, two sub-arrays, equal entries) at sensor counts on both sides of every tile and schedule boundary; the
solver, the whitener and the four grid kernels at every C of 1 .. 64; exact rescales by powers of two, bit for bit; the
whitener at condition numbers 1e4 and 1e10; potrf's info at a chosen pivot; and the closed forms of the rank-one matrix through
csd_eigh -> music_power and csd_whiten -> capon_power.

The bounds are the project's reduction tolerances (beam_cases.TOL), which the restatements meet four times over on these
inputs (tests/test_array_hard_cpu.py) -- except on the ill-conditioned whitener, where the bound is 16 times the deviation
recorded from the restatement in the same precision.  Whenever info is 0 the outputs must be finite."""
import functools

import numpy as np
import pytest

import array_hard_cases as ahc
import beam_cases as bc
import capon_cases as cpc
import music_cases as mc
import steer_cases as stc

from quantum_inferno_amd import engine

pytestmark = pytest.mark.gpu

DTYPES = bc.DTYPES
FAMILY_SENSORS = (2, 3, 4, 8, 15, 31, 32, 47, 48, 49, 63, 64)
WORST = {}  # (test, dtype) -> {figure: (value, case)}: the largest measured so far, printed as it grows


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


def finite(a):
    a = np.asarray(a)
    return bool(np.isfinite(a.real).all() and np.isfinite(a.imag).all())


def note(test, dtype, case, **figures):
    """Keeps the largest of every figure per test and dtype, and prints the table."""
    table = WORST.setdefault((test, dtype), {})
    for name, value in figures.items():
        if name not in table or value > table[name][0]:
            table[name] = (float(value), case)
    print(f"{test} {dtype}, largest so far: " + "; ".join(f"{n} {v:.3g} ({c})" for n, (v, c) in table.items()))


@functools.lru_cache(maxsize=None)
def family_reference(C, dtype):
    """np.linalg.eigh of the values the device reads: computed once, shared, left unchanged."""
    w, u = mc.eigh64(ahc.families(C, dtype))
    w.setflags(write=False)
    u.setflags(write=False)
    return w, u


# ---- 1: eigenpairs on every family ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", FAMILY_SENSORS)
def test_eigenpairs_of_every_family(C, dtype):
    s = ahc.families(C, dtype)
    ref_w, ref_u = family_reference(C, dtype)
    w, u, info = engine.csd_eigh(s, info=True)
    tol = bc.TOL[dtype]
    assert w.dtype == np.dtype(dtype) and w.shape == s.shape[:2] and u.dtype == s.dtype and u.shape == s.shape
    assert info.dtype == np.int32 and not info.any(), (C, dtype, dict(zip(ahc.FAMILIES, info.tolist())))
    assert finite(w) and finite(u), (C, dtype)
    assert np.all(np.diff(w, axis=1) >= 0), (C, dtype)
    values, ortho, pairs = ahc.eigen_deviations(w, u, s)
    stack = mc.residuals(w, u, s)  # (the two residuals over the stack as a whole: never above the per-matrix ones)
    proj = {}
    for name, cols in ahc.subspaces(C):
        f = ahc.index_of(name)
        proj[name] = float(np.abs(ahc.projector(u[f], cols) - ahc.projector(ref_u[f], cols)).max())
    dead = u[ahc.index_of("dead_sensor")][:, 0].astype(np.complex128)
    unit = np.zeros(C)
    unit[C // 2] = 1
    dead_err = float(np.abs(np.abs(dead) - unit).max())  # the unit vector C // 2 up to phase
    twin = u[ahc.index_of("twin_sensors")][:, 0].astype(np.complex128)
    twin_err = float(np.abs(twin[0] + twin[C - 1]) + np.abs(np.delete(twin, [0, C - 1])).max(initial=0) + abs(abs(twin[0]) - np.sqrt(0.5)))
    case = f"C = {C}"
    print(f"{case} {dtype}: per family " + ", ".join(f"{n}: {a:.2g} / {b:.2g} / {c:.2g}" for n, a, b, c in zip(ahc.FAMILIES, values, ortho, pairs)))
    note("eigenpairs", dtype, case, eigenvalues=values.max(), ortho=ortho.max(), pairs=pairs.max(), projector=max(proj.values()),
         dead_vector=dead_err, twin_vector=twin_err)
    for f, name in enumerate(ahc.FAMILIES):
        assert values[f] <= tol and ortho[f] <= tol and pairs[f] <= tol, (C, dtype, name, values[f], ortho[f], pairs[f])
    assert max(stack) <= tol, (C, dtype, stack)
    for name, err in proj.items():
        assert err <= tol, (C, dtype, name, err)
    assert dead_err <= tol and twin_err <= tol, (C, dtype, dead_err, twin_err)


# ---- 2: every sensor count --------------------------------------------------------------------------------------------------------------
def count_stack(C, dtype):
    """[3, C, C]: repeated, indefinite and a plain definite matrix (condition 100; C = 1: the 1 x 1 matrix 1)."""
    s = ahc.families(C, dtype)
    return np.concatenate([s[[ahc.index_of("repeated"), ahc.index_of("indefinite")]], ahc.conditioned(C, dtype, 100.0)])


@pytest.mark.parametrize("dtype", DTYPES)
def test_solver_and_whitener_at_every_sensor_count(dtype):
    tol = bc.TOL[dtype]
    for C in range(1, bc.MAX_SENSORS + 1):
        case = f"C = {C}"
        s = count_stack(C, dtype)
        w, u, info = engine.csd_eigh(s, info=True)
        assert not info.any() and finite(w) and finite(u) and np.all(np.diff(w, axis=1) >= 0), (case, dtype, info)
        values, ortho, pairs = ahc.eigen_deviations(w, u, s)
        definite = s[2:]
        v, vinfo = engine.csd_whiten(definite, loading=cpc.LOADING, info=True)
        assert not vinfo.any() and finite(v), (case, dtype, vinfo)
        assert not bits(v[:, np.tril(np.ones((C, C), dtype=bool), -1)]).any(), (case, dtype)
        res = cpc.residual(v, cpc.loaded(definite, cpc.LOADING, dtype))
        note("every count, factorisations", dtype, case, eigenvalues=values.max(), ortho=ortho.max(), pairs=pairs.max(), whitener=res)
        assert values.max() <= tol and ortho.max() <= tol and pairs.max() <= tol and res <= tol, (case, dtype, values, ortho, pairs, res)


@pytest.mark.parametrize("dtype", DTYPES)
def test_grid_kernels_at_every_sensor_count(dtype):
    tol = bc.TOL[dtype]
    ctype = bc.complex_of(dtype)
    for C in range(1, bc.MAX_SENSORS + 1):
        case = f"C = {C}"
        s = count_stack(C, dtype)
        freq, tau = ahc.grid(C, 3)
        k = mc.sources_of(C)
        # Bartlett on the three matrices
        ref = bc.restate(s, freq, tau)
        got = engine.beam_power(s, freq, tau)
        assert got.shape == ref.shape == (3, ahc.G) and got.dtype == np.dtype(dtype) and finite(got), (case, dtype)
        beam = float(np.abs(got - ref).max() / np.abs(ref).max())
        # Capon and the MVDR weights on the definite one's whitener, restated in float64 on the values the device reads
        definite, f1 = s[2:], freq[2:]
        ref_v = cpc.whiten(definite, cpc.LOADING, dtype)
        ref_p = cpc.capon(ref_v, f1, tau)
        v = engine.csd_whiten(definite, loading=cpc.LOADING)
        got_p = engine.capon_power(v, f1, tau)
        assert got_p.shape == ref_p.shape == (1, ahc.G) and finite(got_p) and got_p.min() > 0, (case, dtype)
        capon = float(np.abs(got_p - ref_p).max() / np.abs(ref_p).max())
        ref_a = stc.weights(f1, tau, ref_v)
        a = engine.beam_weights(f1, tau, whitener=v)
        assert a.shape == ref_a.shape == (1, ahc.G, C) and a.dtype == ctype and finite(a), (case, dtype)
        weights = float(np.abs(a - ref_a).max() / np.abs(ref_a).max())
        gain = float(np.abs(stc.gain(f1, tau, a) - 1).max())
        # MUSIC: the form fed np.linalg.eigh's vectors on all three; end to end where the count of sources makes the subspace sharp
        ref_u = mc.eigh64(s)[1]
        ref_inv = 1.0 / mc.music(ref_u, k, freq, tau)
        fed = engine.music_power(ref_u.astype(ctype), k, freq, tau)
        assert fed.shape == ref_inv.shape == (3, ahc.G) and finite(fed), (case, dtype)
        music = float(np.abs(1.0 / fed.astype(np.float64) - ref_inv).max())
        end = engine.music_power(engine.csd_eigh(s[:1])[1], k, freq[:1], tau)
        music_end = float(np.abs(1.0 / end.astype(np.float64) - ref_inv[:1]).max())
        note("every count, grid kernels", dtype, case, bartlett=beam, capon=capon, mvdr_weights=weights, mvdr_gain=gain, music_fed=music, music_end=music_end)
        assert beam <= tol and capon <= tol and weights <= tol and gain <= tol and music <= tol and music_end <= tol, (
            case, dtype, dict(bartlett=beam, capon=capon, mvdr_weights=weights, mvdr_gain=gain, music_fed=music, music_end=music_end))


# ---- 3: exact rescales ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", ahc.SCALE_SENSORS)
def test_solver_is_covariant_with_a_power_of_two(C, dtype):
    """A square, a norm or a threshold formed in the matrix's precision breaks this: in float32 the square of an entry times
    2^60 overflows, and at 2^-60 the squares of the small entries are flushed to zero and their rotations are never taken."""
    rt = np.dtype(dtype).type
    s = ahc.families(C, dtype)
    w, u, info = engine.csd_eigh(s, info=True)
    assert not info.any() and finite(w) and finite(u)
    for k in ahc.EIGH_SCALES[dtype]:
        ws, us, infos = engine.csd_eigh((s * rt(2.0) ** k).astype(s.dtype), info=True)
        assert not infos.any(), (C, dtype, k, dict(zip(ahc.FAMILIES, infos.tolist())))
        differ = [name for f, name in enumerate(ahc.FAMILIES) if not (same_bits(us[f], u[f]) and same_bits(ws[f], (w[f] * rt(2.0) ** k).astype(dtype)))]
        assert not differ, (C, dtype, k, differ)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", ahc.SCALE_SENSORS)
def test_whitener_is_covariant_with_a_power_of_four(C, dtype):
    rt = np.dtype(dtype).type
    s = ahc.families(C, dtype)
    upper = np.triu(np.ones((C, C), dtype=bool))
    v, info = engine.csd_whiten(s, loading=cpc.LOADING, info=True)
    good = info == 0
    assert np.array_equal(info, cpc.whiten_steps(s, cpc.LOADING, dtype)[1]) and good.sum() == len(s) - 1, (C, dtype, info)
    assert finite(v[good])
    for k in ahc.WHITEN_SCALES[dtype]:
        vs, infos = engine.csd_whiten((s * rt(4.0) ** k).astype(s.dtype), loading=cpc.LOADING, info=True)
        assert np.array_equal(infos, info), (C, dtype, k, infos)
        differ = [name for f, name in enumerate(ahc.FAMILIES) if good[f] and not same_bits(vs[f], (v[f] * rt(2.0) ** -k).astype(s.dtype))]
        assert not differ, (C, dtype, k, differ)
        assert np.isnan(vs[~good][:, upper].real).all() and np.isnan(vs[~good][:, upper].imag).all() and not bits(vs[~good][:, ~upper]).any()


# ---- 4: the ill-conditioned whitener ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", ahc.WHITEN_SENSORS)
def test_ill_conditioned_whitener(C, dtype):
    s = ahc.conditioned(C, dtype)
    freq, tau = ahc.grid(C, 1)
    v, info = engine.csd_whiten(s, loading=0.0, info=True)
    assert not info.any() and finite(v), (C, dtype, info)
    res = cpc.residual(v, cpc.loaded(s, 0.0))
    power = engine.capon_power(v, freq, tau)
    assert finite(power) and power.min() > 0
    ref = 1.0 / cpc.capon(cpc.whiten(s, 0.0), freq, tau)
    rec = float(np.abs(1.0 / power.astype(np.float64) - ref).max() / np.abs(ref).max())
    bounds = ahc.RESTATEMENT_MARGIN * ahc.WHITEN_HARD_RESIDUAL[dtype], ahc.RESTATEMENT_MARGIN * ahc.CAPON_HARD_RECIPROCAL[dtype]
    print(f"C = {C} {dtype}: condition {ahc.CONDITION[dtype]:g}: max |V^H R V - I| {res:.3g} (bound {bounds[0]:.3g}), 1 / power over the largest "
          f"{rec:.3g} (bound {bounds[1]:.3g})")
    note("ill-conditioned whitener", dtype, f"C = {C}", residual=res, reciprocal=rec)
    assert res <= bounds[0] and rec <= bounds[1], (C, dtype, res, rec)


# ---- 5: potrf's info ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", ahc.WHITEN_SENSORS)
def test_info_is_the_first_bad_pivot(C, dtype):
    ks = ahc.bad_pivots(C)
    at = dict(zip((1, 2, 4, 7), ks))  # matrix -> the pivot that fails; the first, the last and the ones between are good
    clean_s = ahc.definite_stack(C, 9, dtype)
    hurt = clean_s.copy()
    for f, k in at.items():
        hurt[f] = ahc.first_bad_pivot(C, k).astype(hurt.dtype)
    clean, clean_info = engine.csd_whiten(clean_s, loading=0.0, info=True)
    assert not clean_info.any() and finite(clean)
    v, info = engine.csd_whiten(hurt, loading=0.0, info=True)
    want = np.zeros(len(hurt), dtype=np.int32)
    for f, k in at.items():
        want[f] = k
    assert info.dtype == np.int32 and np.array_equal(info, want), (C, dtype, info)
    upper = np.triu(np.ones((C, C), dtype=bool))
    for f in at:
        assert np.isnan(v[f][upper].real).all() and np.isnan(v[f][upper].imag).all() and not bits(v[f][~upper]).any(), (C, dtype, f)
    good = want == 0
    assert same_bits(v[good], clean[good]), (C, dtype)


# ---- 6: the closed forms, end to end --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", ahc.WHITEN_SENSORS)
def test_rank_one_closed_forms_end_to_end(C, dtype):
    x = ahc.rank_one_vector(C)
    s = ahc.families(C, dtype)[ahc.index_of("rank_one")][None]
    freq, tau = ahc.grid(C, 1)
    e = ahc.factors(freq, tau)
    w, u, info = engine.csd_eigh(s, info=True)
    assert not info.any() and finite(w) and finite(u)
    power = engine.music_power(u, 1, freq, tau)
    assert finite(power)
    music = float(np.abs(1.0 / power.astype(np.float64) - ahc.music_rank_one(x, e) / C).max())
    v, info = engine.csd_whiten(s, loading=0.5, info=True)
    assert not info.any() and finite(v)
    power = engine.capon_power(v, freq, tau)
    assert finite(power)
    want = 1.0 / ahc.capon_rank_one(x, e, 0.5)
    capon = float(np.abs(power.astype(np.float64) - want).max() / want.max())
    note("rank-one closed forms", dtype, f"C = {C}", music_reciprocal=music, capon_power=capon)
    assert music <= bc.TOL[dtype] and capon <= bc.TOL[dtype], (C, dtype, music, capon)
