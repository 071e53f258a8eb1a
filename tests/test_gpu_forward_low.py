"""GPU tests (-m gpu) of the low-bins forward transform of float32 native runs: a plan whose tables read the record
spectrum only near DC (every band on the zoom, block and split engines) forms just the bins (-Lf/64, Lf/64) of it
(qi_native.hip: k_pass1<LOW>, k_fwd2_low) instead of all of them.  Checked against the full transform of the same library
(development switch QI_NATIVE_FWD_LOW=0, the path the reference fixtures of test_gpu_parity pin), at the smallest shapes
that reach every variant -- the native forward transform exists at Lf = 2^20 and 2^21 only: n = 2^19 (CWT at Lf = 2^20,
one-phase first pass) and n = 2^20 (CWT at Lf = 2^21, two phases; Stockwell at Lf = 2^20), order 3, 1 and 4 records
(launch_forward changes its launch configuration below 4 records).

Tolerances: both paths are exact transforms of the same record in float32 and differ by rounding only: panels within 2e-6
of the panel maximum, reductions at the tolerances test_gpu_parity.test_fused_cwt_stx_call_matches_separate_calls uses for
two compilations of the same arithmetic.
"""
import numpy as np
import pytest
import torch

from quantum_inferno_amd import _lib, engine, scales_dyadic

pytestmark = pytest.mark.gpu

FS, ORDER = 1000.0, 3
STYX, STX = _lib.QI_BANK_STYX, _lib.QI_TABLE_STX


def make_plan(monkeypatch, n, order, channels, tables=("styx", "stx"), low=True):
    """A float32 plan with the named tables; low=False: created under QI_NATIVE_FWD_LOW=0 (the switch is read at creation)."""
    if not low:
        monkeypatch.setenv("QI_TUNE", "1")
        monkeypatch.setenv("QI_NATIVE_FWD_LOW", "0")
    nb = len(scales_dyadic.log_frequency_hz_from_fft_points(FS, n, order))
    plan = engine.TfrPlan(n, torch.float32, None, engine.TfrPlan.workspace_for(n, nb, torch.float32, channels))
    if not low:
        monkeypatch.delenv("QI_NATIVE_FWD_LOW")
        monkeypatch.delenv("QI_TUNE")
    if "styx" in tables:
        plan.set_styx_bank(order, FS)
    if "stx" in tables:
        plan.set_stx_bands(order, FS)
    return plan


def hard_record(n, lf, k, channels, seed=11):
    """Records that put energy where the pruning can go wrong, for a table whose reads lie in (-k, k) of its lf-point
    spectrum: a DC offset (the lowest Stockwell rows read it through negative bins), a tone at bin k - 1 (the upper edge of
    the highest zoom band's support), a tone just above k (which must not leak in) and seeded noise."""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    x = np.empty((channels, n), dtype=np.float64)
    for c in range(channels):
        x[c] = (0.7 + 0.1 * c
                + np.cos(2 * np.pi * (k - 1) / lf * t + 0.3 * c)
                + 0.8 * np.cos(2 * np.pi * (k + 3) / lf * t + 1.1)
                + 0.5 * np.cos(2 * np.pi * (0.31 * k) / lf * t + 0.2 * c)
                + 0.25 * rng.standard_normal(n))
    return torch.from_numpy(x.astype(np.float32)).cuda()


def assert_close(low, full, what):
    scale = float(full.coef.abs().max())
    err = float((low.coef - full.coef).abs().max()) / scale
    print(f"{what}: low against full, max error / panel max {err:.3e}")
    assert err <= 2e-6, (what, err)
    assert torch.allclose(low.power_band, full.power_band, rtol=1e-5), what
    assert torch.allclose(low.power_time, full.power_time, rtol=1e-4, atol=1e-7 * float(full.power_time.max())), what
    assert torch.allclose(low.stats[:, :3], full.stats[:, :3], rtol=1e-5), what


def zoom_rows(plan, which, records):
    """Rows of table `which` the zoom engine alone produces (not the split bands: their edge pieces come from the block launch)."""
    rows = []
    for j in range(len(plan.freq[which])):
        stage, _, _, flags = plan.band_route(which, j, records)
        if stage == "zoom" and not flags & _lib.ROUTE_SPLIT:
            rows.append(j)
    return rows


@pytest.mark.parametrize("channels", [1, 4])
def test_low_path_matches_full_path_cwt_half_million(monkeypatch, channels):
    """n = 2^19: the CWT's forward transform at Lf = 2^20 (N1 = 1024, one-phase first pass); the Stockwell table of this
    length has no native forward transform, so the plan holds the styx bank alone."""
    n = 1 << 19
    low = make_plan(monkeypatch, n, ORDER, channels, tables=("styx",))
    full = make_plan(monkeypatch, n, ORDER, channels, tables=("styx",), low=False)
    k = low.forward_low(STYX)
    assert k > 0 and full.forward_low(STYX) == 0
    x = hard_record(n, 2 * n, k, channels)
    assert_close(low.cwt(x, coef=True, reductions=True), full.cwt(x, coef=True, reductions=True), f"cwt 2^19 x {channels}")
    low.close()
    full.close()


@pytest.mark.parametrize("channels", [1, 4])
def test_low_path_matches_full_path_million(monkeypatch, channels):
    """n = 2^20: cwt (Lf = 2^21, the two phases of the first pass), stx (Lf = 2^20) and cwt_stx (the Stockwell rows read the
    CWT's low bins at twice their index)."""
    n = 1 << 20
    low = make_plan(monkeypatch, n, ORDER, channels)
    full = make_plan(monkeypatch, n, ORDER, channels, low=False)
    kc, ks = low.forward_low(STYX), low.forward_low(STX)
    assert kc > 0 and ks > 0 and full.forward_low(STYX) == 0 and full.forward_low(STX) == 0
    for what, x in (("cwt tones", hard_record(n, 2 * n, kc, channels)), ("stx tones", hard_record(n, n, ks, channels, seed=12))):
        assert_close(low.cwt(x, coef=True, reductions=True), full.cwt(x, coef=True, reductions=True), f"cwt, {what} x {channels}")
        assert_close(low.stx(x, coef=True, reductions=True), full.stx(x, coef=True, reductions=True), f"stx, {what} x {channels}")
        lc, ls = low.cwt_stx(x, coef=True, reductions=True)
        fc, fs_ = full.cwt_stx(x, coef=True, reductions=True)
        assert_close(lc, fc, f"cwt_stx cwt, {what} x {channels}")
        assert_close(ls, fs_, f"cwt_stx stx, {what} x {channels}")
        del lc, ls, fc, fs_
    low.close()
    full.close()


@pytest.mark.parametrize("channels", [1, 4])
def test_low_path_bit_equalities(channels):
    """On the low path: a second call reproduces the first bit for bit; the CWT's zoom rows are bit-equal between cwt and
    cwt_stx (one forward path per plan, one arithmetic per bin); stx after cwt_stx equals stx before it."""
    n = 1 << 20
    nb = len(scales_dyadic.log_frequency_hz_from_fft_points(FS, n, ORDER))
    plan = engine.TfrPlan(n, torch.float32, None, engine.TfrPlan.workspace_for(n, nb, torch.float32, channels))
    plan.set_styx_bank(ORDER, FS)
    plan.set_stx_bands(ORDER, FS)
    k = plan.forward_low(STYX)
    assert k > 0 and plan.forward_low(STX) > 0
    x = hard_record(n, 2 * n, k, channels, seed=13)
    c1 = plan.cwt(x, coef=True, reductions=True)
    c2 = plan.cwt(x, coef=True, reductions=True)
    assert torch.equal(c1.coef, c2.coef) and torch.equal(c1.reduced, c2.reduced)
    s1 = plan.stx(x, coef=True, reductions=True)
    fc, fs_ = plan.cwt_stx(x, coef=True, reductions=True)
    rows = zoom_rows(plan, STYX, channels)
    assert len(rows) >= 4
    assert torch.equal(fc.coef[:, rows], c1.coef[:, rows])
    ac, as_ = plan.cwt_stx(x, coef=True, reductions=True)
    assert torch.equal(ac.coef, fc.coef) and torch.equal(as_.coef, fs_.coef)
    assert torch.equal(ac.reduced, fc.reduced) and torch.equal(as_.reduced, fs_.reduced)
    s2 = plan.stx(x, coef=True, reductions=True)
    assert torch.equal(s2.coef, s1.coef) and torch.equal(s2.reduced, s1.reduced)
    plan.close()


def top_zoom_bin(plan, which, lf, n, order):
    """Centre bin, in the table's lf-point spectrum, of the highest band the zoom engine takes (0: it takes none)."""
    f = scales_dyadic.log_frequency_hz_from_fft_points(FS, n, order)
    zoom = [f[j] for j in range(len(f)) if plan.band_route(which, j, 1)[0] == "zoom"]
    return max(zoom) * lf / FS if zoom else 0.0


def must_be_full(plan, n, orders):
    """The plan rule restated from outside: a table with two-pass rows, or with a zoom band centred at or beyond Lf / 64,
    keeps the full transform.  orders: {table: order of its band table}."""
    two_pass = sum(plan.stage_bands("pass2")[which] for which in orders)
    beyond = any(top_zoom_bin(plan, which, lf, n, orders[which]) >= lf // 64 for which, lf in ((STYX, 2 * n), (STX, n)) if which in orders)
    return two_pass > 0 or beyond


def test_plan_rule(monkeypatch):
    """Which plans take the low path (qi_plan_forward_low): order 3 at 2^20 does, with a power-of-two K <= Lf / 64 above the
    highest zoom band's centre bin and within a factor 4 of it (a band of these tables is narrower than its centre
    frequency) for both tables; a plan with two-pass rows or with zoom bands beyond Lf / 64 (orders 1, 2 and 12) keeps the
    full transform; replacing a qualifying table by one that does not flips the plan, the other table's results stay within
    tolerance, and putting the table back restores the low path and its bits."""
    n = 1 << 20
    plan = make_plan(monkeypatch, n, ORDER, 1)
    for which, lf in ((STYX, 2 * n), (STX, n)):
        k = plan.forward_low(which)
        top = top_zoom_bin(plan, which, lf, n, ORDER)
        print(f"order {ORDER}, table {which}: K = {k}, highest zoom band at bin {top:.1f}, Lf / 64 = {lf // 64}")
        assert k > 0 and k & (k - 1) == 0 and k <= lf // 64
        assert top < k <= 4 * top
    x = hard_record(n, n, plan.forward_low(STX), 1, seed=14)
    before = plan.stx(x, coef=True, reductions=True)
    before_c = plan.cwt(x, coef=True, reductions=True)
    flipped = 0
    for order in (1, 2, 12):
        plan.set_styx_bank(order, FS)
        full = must_be_full(plan, n, {STYX: order, STX: ORDER})
        got = (plan.forward_low(STYX), plan.forward_low(STX))
        print(f"styx bank of order {order} beside the order-{ORDER} Stockwell table: must be full {full}, K = {got}")
        assert (got == (0, 0)) == full, (order, got)
        if full:
            flipped += 1
            assert_close(plan.stx(x, coef=True, reductions=True), before, f"stx after the order-{order} bank flipped the plan")
    assert flipped > 0
    plan.set_styx_bank(ORDER, FS)
    assert plan.forward_low(STYX) > 0 and plan.forward_low(STX) > 0
    assert torch.equal(plan.cwt(x, coef=True, reductions=True).coef, before_c.coef)
    plan.close()
    for order in (1, 2, 12):
        plan = make_plan(monkeypatch, n, order, 1)
        full = must_be_full(plan, n, {STYX: order, STX: order})
        got = (plan.forward_low(STYX), plan.forward_low(STX))
        print(f"order {order}: must be full {full}, K = {got}")
        assert full, order  # (two-pass rows at orders 1 and 2, zoom bands beyond Lf / 64 at order 12)
        assert got == (0, 0), (order, got)
        plan.close()
