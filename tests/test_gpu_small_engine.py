"""GPU tests (-m gpu) of the small-record engine: power-of-two records of 2^10 .. 2^13 samples on an AUTO plan, whose whole
transform runs in the LDS of one CU (csrc/qi_small.hip).

Records are seeded standard_normal + 0.3 (three channels, non-zero mean), rounded to float32 so that both precisions see
the same values; the comparator is the float64 CPU oracle.  Tolerances are the project's:

                coefficients    bits                              reductions
    float64     1e-11 max       1e-9 where |z| >= 1.5e-2 max      1e-10
    float32     2e-5 max        1e-3 where |z| >= 1e-3 max        1e-4

The bits mask may leave out at most a quarter of a panel.  sum P log2 P has terms of both signs, so its error is taken
relative to sum |P log2 P| (as test_gpu_requests.check_direct does); every other reduction is compared value by value.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import tfr_oracle as orc
from test_gpu_requests import FS, STX, STYX, ATOMS, assert_native, atom_tables

from quantum_inferno_amd import _lib, engine, scales_dyadic, styx_cwt, styx_stx
from quantum_inferno_amd.utilities.sampling import pool_rows

pytestmark = pytest.mark.gpu

CHANNELS = 3
DTYPES = (np.float32, np.float64)
NAMES = {STYX: "styx", ATOMS: "atoms", STX: "stx"}


def on_small(dtype, which, log2n):
    """The size rule: n = 2^10 .. 2^13 and L complex values (L = 2n for the styx bank, n otherwise) within 128 KiB."""
    length = (2 if which == STYX else 1) << log2n
    return 10 <= log2n <= 13 and length * (16 if dtype == np.float64 else 8) <= 128 * 1024


def rule_cases(orders):
    return [(dt, w, lg, o) for dt in DTYPES for w in (STYX, ATOMS, STX) for lg in (10, 11, 12, 13) for o in orders(lg)
            if on_small(dt, w, lg)]


@functools.lru_cache(maxsize=None)
def records(log2n):
    rng = np.random.default_rng(1000 + log2n)
    return (rng.standard_normal((CHANNELS, 1 << log2n)) + 0.3).astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def reference(which, log2n, order, shift=0.0):
    """Float64 oracle panel [channels, bands, n] of the module's records."""
    x = records(log2n)
    if which == STYX:
        return np.stack([orc.cwt_fft(order, xi, FS)[2] for xi in x])
    if which == STX:
        return np.stack([orc.stx_fft(order, xi, FS)[2] for xi in x])
    return np.stack([orc.cwt_chirp_fft(xi, FS, order, index_shift=shift)[0] for xi in x])


def make_plan(dtype, which, log2n, order, eng=_lib.QI_ENGINE_AUTO, shift=0.0, workspace=None, every=False):
    """A plan with table `which` (every: all three tables) -> (plan, bands of `which`)."""
    n = 1 << log2n
    f_styx = scales_dyadic.log_frequency_hz_from_fft_points(FS, n, order)
    f_atoms, tabs = atom_tables(n, order, shift)
    nb = {STYX: len(f_styx), STX: len(f_styx), ATOMS: len(f_atoms)}
    ws = workspace or engine.TfrPlan.workspace_for(n, max(nb.values()), dtype, CHANNELS)
    plan = engine.TfrPlan(n, dtype, None, ws, eng)
    if every or which == STYX:
        plan.set_styx_bank(order, FS)
    if every or which == STX:
        plan.set_stx_bands(order, FS)
    if every or which == ATOMS:
        plan.set_gabor_bank(ATOMS, f_atoms, *tabs)
    return plan, nb[which]


def signal(dtype, log2n):
    return torch.from_numpy(records(log2n).astype(dtype)).cuda()


def run(plan, which, sig, **kw):
    return {STYX: plan.cwt, ATOMS: plan.cwt_atoms, STX: plan.stx}[which](sig, **kw)


def tolerances(dtype):
    """(coefficients / max, bits, bits floor / max, reductions)"""
    return (1e-11, 1e-9, 1.5e-2, 1e-10) if dtype == np.float64 else (2e-5, 1e-3, 1e-3, 1e-4)


def check_against(res, ref, dtype, what, power_scale=1.0, eps=orc.EPS64, band_only=False):
    tc, tb, floor, tr = tolerances(dtype)
    top = np.abs(ref).max()
    if res.coef is not None:
        err = np.abs(res.coef.cpu().numpy() - ref).max() / top
        print(f"{what}: coef err / max {err:.3e}")
        assert err <= tc, (what, err)
    mag = np.abs(ref)
    if res.bits is not None:
        sel = mag >= floor * top
        assert sel.mean() >= 0.75, (what, sel.mean())
        d = np.abs(res.bits.cpu().numpy().astype(np.float64) - np.log2(mag + eps))[sel].max()
        print(f"{what}: bits err {d:.3e} on {sel.mean():.3f} of the panel")
        assert d <= tb, (what, d)
    p = power_scale * mag ** 2
    if res.power_band is not None:
        e = np.abs(res.power_band.cpu().numpy() / p.sum(axis=2) - 1).max()
        print(f"{what}: power_band rel err {e:.3e}")
        assert e <= tr, (what, "power_band", e)
    if not band_only and res.power_time is not None:
        e = np.abs(res.power_time.cpu().numpy().astype(np.float64) / p.sum(axis=1) - 1).max()
        print(f"{what}: power_time rel err {e:.3e}")
        assert e <= tr, (what, "power_time", e)
    if res.stats is not None:
        st = res.stats.cpu().numpy()
        plogp = p * np.log2(np.where(p > 0, p, 1.0))
        e0 = np.abs(st[:, 0] / p.max(axis=(1, 2)) - 1).max()
        e1 = np.abs(st[:, 1] / p.sum(axis=(1, 2)) - 1).max()
        e2 = (np.abs(st[:, 2] - plogp.sum(axis=(1, 2))) / np.abs(plogp).sum(axis=(1, 2))).max()
        print(f"{what}: stats rel err max {e0:.3e} sum {e1:.3e} plogp {e2:.3e}")
        assert max(e0, e1, e2) <= tr, (what, "stats", e0, e1, e2)


# ---- 1. route -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("log2n", (10, 11, 12, 13))
def test_route_inside_the_rule(dtype, log2n):
    for order in (3, 12):
        plan, _ = make_plan(dtype, STYX, log2n, order, every=True)
        small, inverse = plan.stage_bands("small"), plan.stage_bands("inverse")
        for which in (STYX, ATOMS, STX):
            nb = len(plan.freq[which])
            log2len = log2n + (1 if which == STYX else 0)
            if on_small(dtype, which, log2n):
                assert small[which] == nb and inverse[which] == 0, (which, order, small, inverse)
                for band in (0, nb - 1):
                    assert plan.band_route(which, band) == ("small", log2len, log2len, 0), (which, order, band)
            else:  # float64 styx at 2^13: the 2^14-point transform does not fit
                assert dtype == np.float64 and which == STYX and log2n == 13
                assert small[which] == 0 and inverse[which] == nb
                assert plan.band_route(which, 0)[0] == "inverse"
        plan.close()


def test_route_borders_keep_their_engine():
    def census(n, dtype, eng=_lib.QI_ENGINE_AUTO):
        nb = len(scales_dyadic.log_frequency_hz_from_fft_points(FS, n, 3))
        plan = engine.TfrPlan(n, dtype, None, engine.TfrPlan.workspace_for(n, nb, dtype), eng)
        plan.set_styx_bank(3, FS)
        plan.set_stx_bands(3, FS)
        return plan, nb

    for n, dtype, eng in ((1 << 9, np.float32, _lib.QI_ENGINE_AUTO), (3000, np.float32, _lib.QI_ENGINE_AUTO),
                          (3000, np.float64, _lib.QI_ENGINE_AUTO), (1 << 14, np.float64, _lib.QI_ENGINE_AUTO),
                          (1 << 11, np.float32, _lib.QI_ENGINE_HIPFFT), (1 << 11, np.float64, _lib.QI_ENGINE_HIPFFT)):
        plan, nb = census(n, dtype, eng)
        for which in (STYX, STX):
            assert plan.stage_bands("small")[which] == 0 and plan.stage_bands("inverse")[which] == nb, (n, dtype, eng, which)
            assert plan.band_route(which, nb - 1) == ("inverse", 0, 0, 0)
        plan.close()
    plan, nb = census(1 << 14, np.float32)  # zoom / block
    for which in (STYX, STX):
        assert plan.stage_bands("small")[which] == 0
        assert_native(plan, which, nb)
    plan.close()


# ---- 2. every instantiation against the oracle ----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,which,log2n,order", rule_cases(lambda lg: (12, 3) if lg in (10, 13) else (12,)))
def test_against_the_oracle(dtype, which, log2n, order):
    what = f"{NAMES[which]} 2^{log2n} o{order} {np.dtype(dtype).name}"
    plan, nb = make_plan(dtype, which, log2n, order)
    assert plan.stage_bands("small")[which] == nb
    sig = signal(dtype, log2n)
    ref = reference(which, log2n, order)
    check_against(run(plan, which, sig, coef=True, bits=True, reductions=True), ref, dtype, what)
    band = run(plan, which, sig, coef=False, reductions="band")
    assert band.coef is None and band.power_time is None
    check_against(band, ref, dtype, what + " band")
    scaled = run(plan, which, sig, coef=True, bits=True, reductions=True, power_scale=2.0, eps=2.0 ** -20)
    check_against(scaled, ref, dtype, what + " scale 2", power_scale=2.0, eps=2.0 ** -20)
    plan.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
def test_chirped_atoms_against_the_oracle(dtype):
    plan, nb = make_plan(dtype, ATOMS, 11, 12, shift=1.0)
    assert plan.stage_bands("small")[ATOMS] == nb
    res = plan.cwt_atoms(signal(dtype, 11), coef=True, bits=True, reductions=True)
    check_against(res, reference(ATOMS, 11, 12, 1.0), dtype, f"atoms shift 1 {np.dtype(dtype).name}")
    plan.close()


# ---- 3. against the hipFFT engine, row by row -------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,which,log2n,order", rule_cases(lambda lg: (12,)))
def test_rows_against_the_hipfft_engine(dtype, which, log2n, order):
    sig = signal(dtype, log2n)
    plan, nb = make_plan(dtype, which, log2n, order)
    assert plan.stage_bands("small")[which] == nb
    got = run(plan, which, sig, coef=True).coef.to(torch.complex128)
    plan.close()
    plan, _ = make_plan(dtype, which, log2n, order, eng=_lib.QI_ENGINE_HIPFFT)
    assert plan.stage_bands("inverse")[which] == nb
    want = run(plan, which, sig, coef=True).coef.to(torch.complex128)
    plan.close()
    rel = (got - want).abs().amax(dim=-1) / want.abs().amax(dim=-1)
    worst = float(rel.max())
    print(f"{NAMES[which]} 2^{log2n} {np.dtype(dtype).name}: worst row err / row max {worst:.3e}")
    assert worst <= tolerances(dtype)[0], (np.unravel_index(int(rel.argmax()), tuple(rel.shape)), worst)


# ---- 4. determinism and independence ------------------------------------------------------------------------------------------
def same(a, b):
    for name in ("coef", "bits", "power_band", "power_time", "stats", "reduced"):
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None) == (y is None), name
        if x is not None:
            assert torch.equal(x, y), name


@pytest.mark.parametrize("dtype,which,log2n", [(np.float32, STYX, 13), (np.float32, STX, 10), (np.float32, ATOMS, 12),
                                               (np.float64, STYX, 12), (np.float64, STX, 13), (np.float64, ATOMS, 10)])
def test_reproducible_and_independent_of_the_batch(dtype, which, log2n):
    order = 12
    plan, nb = make_plan(dtype, which, log2n, order)
    assert plan.stage_bands("small")[which] == nb
    sig = signal(dtype, log2n)
    kw = dict(coef=True, bits=True, reductions=True)
    first = run(plan, which, sig, **kw)
    same(run(plan, which, sig, **kw), first)
    for c in range(CHANNELS):
        one = run(plan, which, sig[c : c + 1], **kw)
        for name in ("coef", "bits", "power_band", "power_time", "stats"):
            assert torch.equal(getattr(one, name)[0], getattr(first, name)[c]), (name, c)
    plan.close()
    # a workspace that holds one record
    n = 1 << log2n
    plan, _ = make_plan(dtype, which, log2n, order, workspace=engine.TfrPlan.workspace_for(n, nb, dtype, 1))
    same(run(plan, which, sig, **kw), first)
    plan.close()
    # ... and one that cannot hold all three: a spectrum row and at most one per-time plane per band, a quarter more
    esz = 16 if dtype == np.float64 else 8
    per = (2 * n if which == STYX else n) * esz + nb * 32 + nb * n * (esz // 2) + 1024
    tight = per + per // 4
    if tight >= 2 * n * 16:  # (the bank build needs one float64 row)
        plan, _ = make_plan(dtype, which, log2n, order, workspace=tight)
        assert plan.stage_bands("small")[which] == nb
        same(run(plan, which, sig, **kw), first)
        plan.close()


# ---- 5. joint call ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,log2n", [(np.float32, 10), (np.float32, 13), (np.float64, 12)])
def test_joint_call_equals_the_separate_calls(dtype, log2n):
    plan, nb = make_plan(dtype, STYX, log2n, 12, every=True)
    assert plan.stage_bands("small")[STYX] == nb and plan.stage_bands("small")[STX] == nb
    sig = signal(dtype, log2n)
    for kw in (dict(coef=True, bits=True, reductions=True), dict(coef=False, reductions=True)):
        c0, s0 = plan.cwt(sig, **kw), plan.stx(sig, **kw)
        c1, s1 = plan.cwt_stx(sig, **kw)
        same(c1, c0)
        same(s1, s0)
    plan.close()


# ---- 6. pooled ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
def test_pooled_equals_pool_rows_of_the_stored_panel(dtype):
    plan, _ = make_plan(dtype, STYX, 12, 12, every=True)
    sig = signal(dtype, 12)
    for which in (STYX, ATOMS, STX):
        assert plan.stage_bands("small")[which] == len(plan.freq[which])
        panel = run(plan, which, sig, coef=True).coef
        assert torch.equal(plan.pooled(which, sig, 64, "average"), pool_rows(panel, 64, "average", _lib.QI_POOL_POWER, 1.0))
    plan.close()


# ---- 7. zero records and the drop-in ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
def test_zero_record(dtype):
    plan, _ = make_plan(dtype, STYX, 11, 3, every=True)
    zero = torch.zeros((1, 1 << 11), dtype=torch.float64 if dtype == np.float64 else torch.float32, device="cuda")
    for which in (STYX, ATOMS, STX):
        assert plan.stage_bands("small")[which] == len(plan.freq[which])
        res = run(plan, which, zero, coef=True, bits=True, reductions=True)
        assert float(res.coef.abs().max()) == 0.0 and float(res.stats[0, 1]) == 0.0
        assert float(res.power_time.abs().max()) == 0.0 and float(res.power_band.abs().max()) == 0.0
    plan.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
def test_drop_in_wrappers_at_2048(dtype):
    x = records(11)[0].astype(dtype)
    tol = tolerances(dtype)[0]
    f, _, c = styx_cwt.cwt_complex_any_scale_pow2(3, x, FS)
    ref = orc.cwt_fft(3, x.astype(np.float64), FS)[2]
    assert isinstance(c, np.ndarray) and c.dtype == np.complex128 and c.shape == ref.shape
    err = np.abs(c - ref).max() / np.abs(ref).max()
    assert err <= tol, ("cwt", err)
    _, _, s = styx_stx.stx_complex_any_scale_pow2(3, x, FS)
    ref = orc.stx_fft(3, x.astype(np.float64), FS)[2]
    assert isinstance(s, np.ndarray) and s.dtype == np.complex128 and s.shape == ref.shape
    err = np.abs(s - ref).max() / np.abs(ref).max()
    assert err <= tol, ("stx", err)
    engine.clear_plans()
