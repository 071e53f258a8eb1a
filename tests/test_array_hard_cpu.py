"""The hard inputs of tests/array_hard_cases.py without a GPU: what the families are (spectra, ranks, null vectors, blocks), that
the solver's restatement converges on every one of them well inside the sweep cap and inside a quarter of the reduction
tolerance, the recorded deviations against their recomputation, first_bad_pivot's info in the Cholesky restatement, the exact
rescales the GPU test relies on (and one that does not hold), and the closed forms of the rank-one matrix against the float64
restatements."""
import functools

import numpy as np
import pytest

import array_hard_cases as ahc
import beam_cases as bc
import capon_cases as cpc
import music_cases as mc

DTYPES = bc.DTYPES


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


# ---- the inputs are what they say -----------------------------------------------------------------------------------------------------
def test_families_are_what_they_say():
    for C in (1, 2, 3, 8, 17, 64):
        s = ahc.families(C, np.float64)
        assert s.shape == (len(ahc.FAMILIES), C, C) and s.dtype == np.complex128
        assert np.array_equal(s, np.conj(np.swapaxes(s, 1, 2))) and np.isfinite(s.view(np.float64)).all()
        s32 = ahc.families(C, np.float32)
        assert s32.dtype == np.complex64 and np.array_equal(s32, np.conj(np.swapaxes(s32, 1, 2)))
        w = dict(zip(ahc.FAMILIES, np.linalg.eigvalsh(s)))
        k = mc.sources_of(C)
        top = {name: max(np.abs(v).max(), 1e-300) for name, v in w.items()}
        assert np.abs(w["repeated"][:C - k] - 1.5).max() <= 1e-13 and (k == 0 or (51.5 <= w["repeated"][C - k] and w["repeated"][-1] <= 101.5))
        x = ahc.rank_one_vector(C)
        assert np.abs(w["rank_one"][:-1]).max(initial=0) <= 1e-13 * top["rank_one"] and abs(w["rank_one"][-1] - np.sum(np.abs(x) ** 2)) <= 1e-13 * top["rank_one"]
        assert np.allclose(w["graded"][::-1], ahc._powers(1e-12, C), rtol=1e-3, atol=0)
        assert np.allclose(np.linalg.eigvalsh(s32[ahc.index_of("graded")].astype(np.complex128))[::-1], ahc._powers(1e-6, C), rtol=0.2, atol=0)
        assert np.abs(w["indefinite"]).max() <= 100 and (C < 8 or (w["indefinite"][0] < 0 < w["indefinite"][-1]))
        m = np.arange(C) // 2 + 1.0
        assert np.allclose(w["pairs"], np.where(np.arange(C) % 2 == 0, m, m * (1 + 1e-3)), rtol=1e-12, atol=0)
        dead, twin, two = (s[ahc.index_of(n)] for n in ("dead_sensor", "twin_sensors", "two_subarrays"))
        assert not dead[C // 2].any() and not dead[:, C // 2].any() and abs(w["dead_sensor"][0]) <= 1e-13 * top["dead_sensor"]
        assert np.array_equal(twin[C - 1], twin[0]) and np.array_equal(twin[:, C - 1], twin[:, 0])
        if C > 1:
            assert w["dead_sensor"][1] >= 1 - 1e-12 and w["twin_sensors"][1] >= 1 - 1e-12  # the gap above the null vector
            assert abs(w["twin_sensors"][0]) <= 1e-13 * top["twin_sensors"]
            null = np.zeros(C)
            null[0], null[C - 1] = 1, -1
            assert np.abs(twin @ null).max() == 0
            odd = np.arange(C) % 2 == 1
            assert not two[np.ix_(odd, ~odd)].any() and (C < 4 or np.abs(two[np.ix_(odd, odd)]).min() > 0) and np.abs(two[np.ix_(~odd, ~odd)]).min() > 0
        assert w["two_subarrays"][0] >= 1 - 1e-12 and w["two_subarrays"][-1] <= 100 + 1e-12
        assert np.array_equal(s[ahc.index_of("all_equal")], np.full((C, C), 3.0))
        for dtype, cond in (("float32", 1e4), ("float64", 1e10)):
            lam = np.linalg.eigvalsh(ahc.conditioned(C, dtype).astype(np.complex128))[0]
            assert np.allclose(lam, ahc._powers(cond, C), rtol=1e-3 if dtype == "float32" else 1e-6, atol=0), (C, dtype)
        assert np.allclose(np.linalg.eigvalsh(ahc.conditioned(C, "float64", 100.0)[0]), ahc._powers(100.0, C), rtol=1e-12, atol=0)
        for name, cols in ahc.subspaces(C):
            assert name in ahc.FAMILIES and cols.stop - cols.start >= 1
    assert len(ahc.subspaces(1)) == 4 and len(ahc.subspaces(2)) == 5
    assert ahc.EIGH_SCALES == {"float32": (60, -60), "float64": (300, -300)} and ahc.WHITEN_SCALES == {"float32": (30, -30), "float64": (250, -250)}


# ---- the solver's restatement on the families -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def eigen_runs(dtype):
    """{C: (the three deviations [nfam] each, sweeps [nfam], info [nfam], the worst projector deviation)} of eigh_steps on the families."""
    out = {}
    for C in ahc.CPU_SENSORS:
        s = ahc.families(C, dtype)
        w, u, info, sweeps = mc.eigh_steps(s, dtype)
        assert w.dtype == np.dtype(dtype) and np.all(np.diff(w, axis=1) >= 0), (C, dtype)
        u64 = mc.eigh64(s)[1]
        proj = max(float(np.abs(ahc.projector(u[ahc.index_of(n)], c) - ahc.projector(u64[ahc.index_of(n)], c)).max()) for n, c in ahc.subspaces(C))
        out[C] = (ahc.eigen_deviations(w, u, s), sweeps, info, proj)
    return out


def worst_of(runs, n):
    """(the largest n-th deviation, its case) over all C and families."""
    C, f = max(((C, f) for C in runs for f in range(len(ahc.FAMILIES))), key=lambda cf: runs[cf[0]][0][n][cf[1]])
    return float(runs[C][0][n][f]), f"{ahc.FAMILIES[f]}, C = {C}"


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_restatement_converges_on_every_family(dtype):
    runs = eigen_runs(dtype)
    bound = bc.TOL[dtype] / 4
    for C, (dev, sweeps, info, proj) in runs.items():
        print(f"C = {C} {dtype}: sweeps {sweeps.tolist()}; eigenvalues {dev[0].max():.3g}, max |U^H U - I| {dev[1].max():.3g}, max |S U - U w| "
              f"{dev[2].max():.3g}, projectors {proj:.3g}")
        assert not info.any(), (C, dtype, info)
        assert sweeps.max() <= ahc.SWEEPS_MOST, (C, dtype, sweeps)
        for n in range(3):
            assert dev[n].max() <= bound, (C, dtype, n, ahc.FAMILIES[int(np.argmax(dev[n]))])
        assert proj <= bound, (C, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_recorded_eigenpair_deviations(dtype):
    runs = eigen_runs(dtype)
    for n, const in enumerate((ahc.EIGH_HARD_VALUES, ahc.EIGH_HARD_ORTHO, ahc.EIGH_HARD_PAIRS)):
        got, at = worst_of(runs, n)
        print(f"{dtype}: deviation {n}: {got:.4g} ({at}); the constant {const[dtype]:g}; bound {bc.TOL[dtype] / 4:g}")
        assert got <= const[dtype] <= 1.25 * got, (dtype, n, got, at)
        assert const[dtype] <= bc.TOL[dtype] / 4


@pytest.mark.parametrize("dtype", DTYPES)
def test_recorded_whitener_deviations(dtype):
    runs = {C: ahc.whitener_deviations(C, dtype) for C in ahc.WHITEN_SENSORS}
    for C, (info, res, rec) in runs.items():
        print(f"C = {C} {dtype}: conditioned {ahc.CONDITION[dtype]:g}: max |V^H R V - I| {res:.4g}, 1 / power over the largest {rec:.4g}")
        assert info == 0, (C, dtype)
    eps = float(np.finfo(dtype).eps)
    for n, const in ((1, ahc.WHITEN_HARD_RESIDUAL), (2, ahc.CAPON_HARD_RECIPROCAL)):
        got = max(r[n] for r in runs.values())
        assert got <= const[dtype] <= 1.25 * got, (dtype, n, got)
        assert const[dtype] <= eps * ahc.CONDITION[dtype]  # rounding times the condition number, no more
    assert ahc.RESTATEMENT_MARGIN == 16


# ---- potrf's info ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_first_bad_pivot_in_the_restatement(dtype):
    for C in ahc.WHITEN_SENSORS:
        ks = ahc.bad_pivots(C)
        assert ks == (1, 2, C // 2 + 1, C) and len(set(ks)) == 4
        stack = np.stack([ahc.first_bad_pivot(C, k) for k in ks])
        assert np.array_equal(stack, np.conj(np.swapaxes(stack, 1, 2)))
        v, info = cpc.whiten_steps(stack.astype(bc.complex_of(dtype)), 0.0, dtype)
        assert info.tolist() == list(ks), (C, dtype, info)
        upper = np.triu(np.ones((C, C), dtype=bool))
        assert np.isnan(v[:, upper].real).all() and np.isnan(v[:, upper].imag).all() and not v[:, ~upper].any()
        for k, m in zip(ks, stack):  # LAPACK's own verdict: the leading minor of order k is not positive definite, the one before is
            assert np.linalg.eigvalsh(m[:k, :k])[0] < 0 and (k == 1 or np.linalg.eigvalsh(m[:k - 1, :k - 1])[0] > 0), (C, k)


# ---- exact rescales -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_solver_restated_is_covariant_with_a_power_of_two(dtype):
    for C in ahc.SCALE_SENSORS:
        s = ahc.families(C, dtype)
        w, u, info, sweeps = mc.eigh_steps(s, dtype)
        assert not info.any()
        for k in ahc.EIGH_SCALES[dtype]:
            scaled = (s * np.dtype(dtype).type(2.0) ** k).astype(s.dtype)
            assert np.isfinite(scaled.view(dtype)).all() and np.array_equal(scaled != 0, s != 0)
            ws, us, infos, sweepss = mc.eigh_steps(scaled, dtype)
            assert not infos.any() and np.array_equal(sweepss, sweeps), (C, dtype, k)
            assert same_bits(us, u), (C, dtype, k, [ahc.FAMILIES[f] for f in range(len(s)) if not same_bits(us[f], u[f])])
            assert same_bits(ws, (w * np.dtype(dtype).type(2.0) ** k).astype(dtype)), (C, dtype, k)


def test_the_double_norms_underflow_at_two_to_the_minus_500():
    """Why float64's exponent stops at 300: at 2^-500 the squares of the double-precision norms underflow, and the restatement
    no longer does to the small matrix what it does to the large one."""
    s = ahc.families(5, "float64")
    w, u, info, sweeps = mc.eigh_steps(s, "float64")
    ws, us, infos, sweepss = mc.eigh_steps(s * 2.0 ** -500, "float64")
    assert not (np.array_equal(sweepss, sweeps) and same_bits(us, u) and same_bits(ws, w * 2.0 ** -500))


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_whitener_restated_is_covariant_with_a_power_of_four(dtype):
    upper = None
    for C in ahc.SCALE_SENSORS:
        s = ahc.families(C, dtype)
        v, info = cpc.whiten_steps(s, cpc.LOADING, dtype)
        good = info == 0
        assert info[ahc.index_of("indefinite")] != 0 and good.sum() == len(s) - 1, (C, dtype, info)  # every other family factors, loaded
        assert np.isfinite(v[good].view(dtype)).all()
        for k in ahc.WHITEN_SCALES[dtype]:
            scaled = (s * np.dtype(dtype).type(4.0) ** k).astype(s.dtype)
            assert np.isfinite(scaled.view(dtype)).all() and np.array_equal(scaled != 0, s != 0)
            vs, infos = cpc.whiten_steps(scaled, cpc.LOADING, dtype)
            assert np.array_equal(infos, info), (C, dtype, k)
            assert same_bits(vs[good], (v[good] * np.dtype(dtype).type(2.0) ** -k).astype(s.dtype)), (C, dtype, k)
            upper = np.triu(np.ones((C, C), dtype=bool))
            assert np.isnan(vs[~good][:, upper].real).all() and not vs[~good][:, ~upper].any()


# ---- the closed forms ---------------------------------------------------------------------------------------------------------------
def test_closed_forms_of_the_rank_one_matrix():
    for C in ahc.WHITEN_SENSORS:
        x = ahc.rank_one_vector(C)
        s = ahc.families(C, "float64")[ahc.index_of("rank_one")][None]
        freq, tau = ahc.grid(C, 1)
        e = ahc.factors(freq, tau)
        music = 1.0 / mc.music(mc.eigh64(s)[1], 1, freq, tau)
        want = ahc.music_rank_one(x, e) / C
        assert want.shape == music.shape == (1, ahc.G) and want.min() >= 0 and want.max() <= 1
        assert np.abs(music - want).max() <= 1e-12, C
        for loading in (0.5, cpc.LOADING):
            capon = cpc.capon(cpc.whiten(s, loading), freq, tau)
            want = 1.0 / ahc.capon_rank_one(x, e, loading)
            assert np.abs(capon - want).max() <= 1e-12 * want.max(), (C, loading)
        # and the algorithms restated in double
        w, u, info, _ = mc.eigh_steps(s, np.float64)
        assert not info.any() and np.abs(1.0 / mc.music(u, 1, freq, tau) - ahc.music_rank_one(x, e) / C).max() <= 1e-12, C
        v, info = cpc.whiten_steps(s, 0.5, np.float64)
        want = 1.0 / ahc.capon_rank_one(x, e, 0.5)
        assert not info.any() and np.abs(cpc.capon(v, freq, tau) - want).max() <= 1e-12 * want.max(), C
