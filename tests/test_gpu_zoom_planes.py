"""GPU tests (-m gpu) of the merged zoom rows of float32 joint calls (plan.cwt_stx below batch_from records; qi_run.hip:
plan_zoom_rows; qi_zoom.hip: zoom_merged): the zoom classes of a table whose rows tile the record alike (equal zoom_steps)
share their rows, one workgroup walking its bands of each class into ONE per-time plane and one statistics slot, against a
row and a plane per class (development switch QI_NATIVE_ZOOM_MERGE=0, read when a plan is created).

Shapes: n = 2^16 and 2^18, orders 3 and 12 (order 12 reaches zoom levels >= 3 at these lengths: merged rows and rows of one
class in one launch), 1 and 3 records of orc.synth_chirp.  Which rows the zoom launch makes or begins is read from
plan.band_route.  A case's plans and results are formed once and shared by its tests.

Tolerances.  A band's arithmetic does not depend on the row that carries it, and its partial sums keep their
slots: panels and power_band are bit-equal.  The per-time sums and the statistics are regrouped float32 / float64 sums: the
tolerances of test_gpu_parity.test_fused_cwt_stx_call_matches_separate_calls.  Rows against the oracle: the per-row bound
of the native-engine parity tests (test_gpu_parity.TOL), as test_gpu_onerec_planes holds its rows to.
"""
import functools
import os

import numpy as np
import pytest
import torch

from conftest import relmax
from oracle import tfr_oracle as orc
from test_gpu_parity import TOL

from quantum_inferno_amd import _lib, engine, scales_dyadic

pytestmark = pytest.mark.gpu

FS = 1000.0
STYX, STX = _lib.QI_BANK_STYX, _lib.QI_TABLE_STX
CASES = [(16, 3), (16, 12), (18, 3), (18, 12)]
RECORDS = 3
# plan variants: development switches set while the plan is created.  "apart": the two halves' zoom launches go out one
# after the other (QI_NATIVE_FUSE=3), so a table's merged rows run in a launch of its own ("apart_off": its plane count
# without merging)
VARIANTS = {"new": {}, "off": {"QI_NATIVE_ZOOM_MERGE": "0"}, "apart": {"QI_NATIVE_FUSE": "3"},
            "apart_off": {"QI_NATIVE_FUSE": "3", "QI_NATIVE_ZOOM_MERGE": "0"}}


def zoom_steps(cls):
    """Wave-steps per wave of a row of zoom class `cls` (qi_native.hpp: zoom_steps): rows of equal steps tile the record alike."""
    grid = cls if cls < 5 else 0
    return 16 if grid <= 2 else 64 >> grid


def make_plan(n, order, switches):
    """A float32 plan with both tables, sized for RECORDS records; switches: development switches set while it is created."""
    names = ("QI_TUNE",) + tuple(switches)
    saved = {k: os.environ.get(k) for k in names} if switches else {}
    for k, v in switches.items():
        os.environ["QI_TUNE"] = "1"
        os.environ[k] = v
    try:
        nb = len(scales_dyadic.log_frequency_hz_from_fft_points(FS, n, order))
        plan = engine.TfrPlan(n, torch.float32, None, engine.TfrPlan.workspace_for(n, nb, torch.float32, RECORDS))
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    plan.set_styx_bank(order, FS)
    plan.set_stx_bands(order, FS)
    return plan


def zoom_routes(plan, which, records):
    """Rows of table `which` the zoom launch makes (or, split rows, begins): {row: (class it runs as, split)}."""
    rows = {}
    for j in range(len(plan.freq[which])):
        stage, _, run, flags = plan.band_route(which, j, records)
        if stage == "zoom":
            rows[j] = (run, bool(flags & _lib.ROUTE_SPLIT))
    return rows


@functools.lru_cache(maxsize=None)
def case(log2n, order):
    """The records of a case and, per plan variant, the joint call on one and on all records, the per-table plane counts, the
    zoom routes and the single-table calls; kept for every test of the case and never changed."""
    n = 1 << log2n
    x = torch.from_numpy(np.stack([orc.synth_chirp(n, FS, c, RECORDS, np.float32) for c in range(RECORDS)])).cuda()
    out = {"x": x}
    for name, switches in VARIANTS.items():
        plan = make_plan(n, order, switches)
        out[name] = {"planes": {which: plan.joint_planes(which) for which in (STYX, STX)}}
        if name in ("new", "off"):
            out[name]["alone"] = (plan.cwt(x[:1], coef=True, reductions=True), plan.stx(x[:1], coef=True, reductions=True))
        if name != "apart_off":
            out[name]["one"] = plan.cwt_stx(x[:1], coef=True, reductions=True)
            out[name]["all"] = plan.cwt_stx(x, coef=True, reductions=True)
        if name == "new":
            out[name]["one_again"] = plan.cwt_stx(x[:1], coef=True, reductions=True)
            out[name]["row1"] = plan.cwt_stx(x[1:2], coef=True, reductions=True)
            out[name]["routes"] = {which: zoom_routes(plan, which, 1) for which in (STYX, STX)}
        torch.cuda.synchronize()
        plan.close()
    return out


@pytest.mark.parametrize("log2n,order", CASES)
@pytest.mark.parametrize("key", ["one", "all"])
def test_merged_rows_match_rows_of_their_own(log2n, order, key):
    """Merged rows against QI_NATIVE_ZOOM_MERGE=0, 1 and 3 records: panels and power_band bit for bit, the regrouped sums
    within the tolerances of the fused-call test."""
    c = case(log2n, order)
    for t, name in ((0, "cwt"), (1, "stx")):
        new, old = c["new"][key][t], c["off"][key][t]
        what = (log2n, order, key, name)
        assert torch.equal(new.coef, old.coef), what
        assert torch.equal(new.power_band, old.power_band), what
        diff = float((new.power_time - old.power_time).abs().max()) / float(old.power_time.max())
        print(f"2^{log2n} order {order} {key} {name}: power_time of merged rows against rows of their own, max difference / max {diff:.3e}")
        assert torch.allclose(new.power_time, old.power_time, rtol=1e-4, atol=1e-7 * float(old.power_time.max())), what
        assert torch.allclose(new.stats[:, :3], old.stats[:, :3], rtol=1e-5), what


@pytest.mark.parametrize("log2n,order", CASES)
@pytest.mark.parametrize("key", ["one", "all"])
def test_merged_rows_in_a_launch_of_one_table(log2n, order, key):
    """The zoom launches of the two halves one after the other (QI_NATIVE_FUSE=3; a launch of one table deals its rows by
    another rule, so the sums are regrouped) against the joint launch, merged rows in both: panels and power_band bit for
    bit, the sums within the tolerances of the fused-call test; its merged rows save planes like the joint launch's."""
    c = case(log2n, order)
    for t, which in ((0, STYX), (1, STX)):
        new, apart = c["new"][key][t], c["apart"][key][t]
        what = (log2n, order, key, which)
        assert torch.equal(new.coef, apart.coef) and torch.equal(new.power_band, apart.power_band), what
        assert torch.allclose(new.power_time, apart.power_time, rtol=1e-4, atol=1e-7 * float(new.power_time.max())), what
        assert torch.allclose(new.stats[:, :3], apart.stats[:, :3], rtol=1e-5), what
        merged, rows = c["apart"]["planes"][which], c["apart_off"]["planes"][which]
        assert merged <= rows and (merged < rows) == (c["new"]["planes"][which] < c["off"]["planes"][which]), (what, merged, rows)


@pytest.mark.parametrize("log2n,order", CASES)
def test_merging_writes_fewer_planes(log2n, order):
    """qi_plan_joint_planes: never more planes than with the switch off; fewer for every table with two or more zoom
    classes of equal zoom_steps (one record: the classes the rows run as)."""
    c = case(log2n, order)
    for which in (STYX, STX):
        routes = c["new"]["routes"][which]
        classes = {run for run, _ in routes.values()}
        steps = [zoom_steps(g) for g in classes]
        mergeable = any(steps.count(s) >= 2 for s in steps)
        planes = {v: c[v]["planes"][which] for v in ("new", "off")}
        print(f"2^{log2n} order {order} table {which}: zoom classes {sorted(classes)}, per-time planes {planes}")
        assert 0 < planes["new"] <= planes["off"], (log2n, order, which, planes)
        if mergeable:
            assert planes["new"] < planes["off"], (log2n, order, which, planes)


@pytest.mark.parametrize("log2n,order", CASES)
def test_calls_repeat_and_records_stand_alone(log2n, order):
    """A second call reproduces the first bit for bit; a record stays what it is alone as row 1 of the 3-record call: the
    panel and power_band bit for bit, the per-time sums and the statistics at the rtol 1e-5 of
    test_gpu_onerec_planes.test_calls_repeat_and_records_stand_alone (the zoom launch deals its bands to rows by the call's
    record count, so the sums over bands are grouped differently -- with merged rows as without)."""
    c = case(log2n, order)["new"]
    for t in (0, 1):
        a, b = c["one"][t], c["one_again"][t]
        assert torch.equal(a.coef, b.coef) and torch.equal(a.reduced, b.reduced), (log2n, order, t)
        alone, batch = c["row1"][t], c["all"][t]
        assert torch.equal(alone.coef[0], batch.coef[1]), (log2n, order, t)
        assert torch.equal(alone.power_band[0], batch.power_band[1]), (log2n, order, t)
        diff = float((alone.power_time[0] - batch.power_time[1]).abs().max()) / float(alone.power_time.max())
        print(f"2^{log2n} order {order} table {t}: power_time alone against row 1 of {RECORDS}, max difference / max {diff:.3e}")
        assert torch.allclose(alone.power_time[0], batch.power_time[1], rtol=1e-5, atol=1e-7 * float(alone.power_time.max()))
        assert torch.allclose(alone.stats[0], batch.stats[1], rtol=1e-5), (log2n, order, t)


@pytest.mark.parametrize("log2n,order", CASES)
def test_single_table_calls_keep_their_rows(log2n, order):
    """plan.cwt and plan.stx alone run a row per class whatever the switch says: bit-equal between the two plans."""
    c = case(log2n, order)
    for t in (0, 1):
        new, old = c["new"]["alone"][t], c["off"]["alone"][t]
        assert torch.equal(new.coef, old.coef) and torch.equal(new.reduced, old.reduced), (log2n, order, t)


@pytest.mark.parametrize("log2n,order", CASES)
def test_zoom_and_split_rows_against_the_oracle(log2n, order):
    """Zoom rows of both tables (the lowest, the middle and the highest of the rows the zoom launch finishes, and every split
    row up to three) of record 0 of the joint call against the float64 oracle on the same float32 record, at the per-row
    bound of the native-engine parity tests."""
    c = case(log2n, order)
    x0 = c["x"][0].cpu().numpy().astype(np.float64)
    for t, which, oracle in ((0, STYX, orc.cwt_fft), (1, STX, orc.stx_fft)):
        routes = c["new"]["routes"][which]
        whole = sorted(j for j, (_, split) in routes.items() if not split)
        split = sorted(j for j, (_, s) in routes.items() if s)
        assert len(whole) >= 3, (log2n, order, which)
        pick = sorted({whole[0], whole[len(whole) // 2], whole[-1], *split[:3]})
        _, _, want = oracle(order, x0, FS, bands=pick)
        got = c["new"]["one"][t].coef[0][torch.tensor(pick, device="cuda")].cpu().numpy()
        for i, j in enumerate(pick):
            err = relmax(got[i], want[i])
            print(f"2^{log2n} order {order} table {which} row {j} (class {routes[j][0]}, split {routes[j][1]}): error against the oracle {err:.3e}")
            assert err <= TOL[np.float32]["coef"], (log2n, order, which, j, err)
