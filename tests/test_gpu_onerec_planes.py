"""GPU tests (-m gpu) of the table-first dealing of the joint block launch of float32 joint calls (plan.cwt_stx below
batch_from records; qi_plan_build.hip: build_joint_items): a reach group's styx and Stockwell bands are dealt as one
sequence, so that a table writes one per-time plane per run that holds any of its bands, against the chunk-by-chunk
pairing of the tables' own item lists (development switch QI_NATIVE_JOINT_DEAL=0, read when a plan is created).

Shapes: n = 2^16 and 2^18, orders 3 and 12 (36 block bands per table: every reach group needs several workgroups in both
tables), 1 and 3 records of orc.synth_chirp.  A case's plans and results are formed once and shared by its tests.

Tolerances.  A band's arithmetic does not depend on the item that carries it, and its per-block partial sums are added in
block order under either dealing: panels and power_band are bit-equal.  The per-time sums and the statistics are regrouped
float32 / float64 sums: the tolerances of test_gpu_parity.test_fused_cwt_stx_call_matches_separate_calls.  Block rows
against the oracle: the per-row bound of the native-engine parity tests (test_gpu_parity.TOL).
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


def make_plan(n, order, switch=None):
    """A float32 plan with both tables, sized for RECORDS records; switch: a development switch set to 0 while it is created."""
    saved = {k: os.environ.get(k) for k in ("QI_TUNE", switch)} if switch else {}
    if switch:
        os.environ["QI_TUNE"] = "1"
        os.environ[switch] = "0"
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


def block_rows(plan, which, records):
    """Rows of table `which` the block launch's band items produce (not the split bands, which the zoom launch begins)."""
    rows = []
    for j in range(len(plan.freq[which])):
        stage, _, _, flags = plan.band_route(which, j, records)
        if stage == "block" and not flags & _lib.ROUTE_SPLIT:
            rows.append(j)
    return rows


@functools.lru_cache(maxsize=None)
def case(log2n, order):
    """The records of a case and, per plan variant ('new', 'old'), the joint call on one and on all records, the per-table
    plane counts, the block rows and the single-table calls; kept for every test of the case and never changed."""
    n = 1 << log2n
    x = torch.from_numpy(np.stack([orc.synth_chirp(n, FS, c, RECORDS, np.float32) for c in range(RECORDS)])).cuda()
    out = {"x": x}
    for name, switch in (("new", None), ("old", "QI_NATIVE_JOINT_DEAL")):
        plan = make_plan(n, order, switch)
        out[name] = {
            "planes": {which: plan.joint_planes(which) for which in (STYX, STX)},
            "one": plan.cwt_stx(x[:1], coef=True, reductions=True),
            "one_again": plan.cwt_stx(x[:1], coef=True, reductions=True),
            "row1": plan.cwt_stx(x[1:2], coef=True, reductions=True),
            "all": plan.cwt_stx(x, coef=True, reductions=True),
            "block_rows": {which: block_rows(plan, which, 1) for which in (STYX, STX)},
            "alone": (plan.cwt(x[:1], coef=True, reductions=True), plan.stx(x[:1], coef=True, reductions=True)),
        }
        torch.cuda.synchronize()
        plan.close()
    return out


@pytest.mark.parametrize("log2n,order", CASES)
@pytest.mark.parametrize("key", ["one", "all"])
def test_joint_dealing_matches_chunk_pairing(log2n, order, key):
    """Table-first dealing against QI_NATIVE_JOINT_DEAL=0, 1 and 3 records: panels and power_band bit for bit, the regrouped
    sums within the tolerances of the fused-call test."""
    c = case(log2n, order)
    for t, name in ((0, "cwt"), (1, "stx")):
        new, old = c["new"][key][t], c["old"][key][t]
        what = (log2n, order, key, name)
        assert torch.equal(new.coef, old.coef), what
        assert torch.equal(new.power_band, old.power_band), what
        diff = float((new.power_time - old.power_time).abs().max()) / float(old.power_time.max())
        print(f"2^{log2n} order {order} {key} {name}: power_time of the two dealings, max difference / max {diff:.3e}")
        assert torch.allclose(new.power_time, old.power_time, rtol=1e-4, atol=1e-7 * float(old.power_time.max())), what
        assert torch.allclose(new.stats[:, :3], old.stats[:, :3], rtol=1e-5), what


def test_joint_dealing_writes_no_more_planes():
    """qi_plan_joint_planes: never more planes than the chunk-by-chunk pairing for any tested table, fewer for at least one."""
    fewer = 0
    for log2n, order in CASES:
        c = case(log2n, order)
        for which in (STYX, STX):
            new, old = c["new"]["planes"][which], c["old"]["planes"][which]
            print(f"2^{log2n} order {order} table {which}: per-time planes {old} -> {new}")
            assert 0 < new <= old, (log2n, order, which, new, old)
            fewer += new < old
    assert fewer >= 1


@pytest.mark.parametrize("log2n,order", CASES)
def test_calls_repeat_and_records_stand_alone(log2n, order):
    """A second call reproduces the first bit for bit; a record stays what it is alone as row 1 of the 3-record call: the
    panel and power_band bit for bit.  Its per-time sums and statistics are bit-equal under neither dealing and were not
    before it: the zoom launch deals its bands to rows by the call's record count (plan_zoom_rows), so the sums over bands
    are grouped differently -- test_gpu_parity.test_native_engine_batches_match_single_records holds them to rtol 1e-5 for
    that reason, and so does this test (measured: at most 8.5e-7 of the maximum); the block launch's dealing adds no
    dependence on the records (the item lists are the plan's)."""
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
def test_single_table_calls_keep_their_item_lists(log2n, order):
    """plan.cwt and plan.stx alone run the tables' own item lists whatever the switch says: bit-equal between the two plans."""
    c = case(log2n, order)
    for t in (0, 1):
        new, old = c["new"]["alone"][t], c["old"]["alone"][t]
        assert torch.equal(new.coef, old.coef) and torch.equal(new.reduced, old.reduced), (log2n, order, t)


@pytest.mark.parametrize("log2n,order", CASES)
def test_block_rows_against_the_oracle(log2n, order):
    """Block rows of both tables (the lowest, the middle and the highest the block launch takes) of record 0 of the joint call
    against the float64 oracle on the same float32 record, at the per-row bound of the native-engine parity tests."""
    c = case(log2n, order)
    x0 = c["x"][0].cpu().numpy().astype(np.float64)
    for t, which, oracle in ((0, STYX, orc.cwt_fft), (1, STX, orc.stx_fft)):
        rows = c["new"]["block_rows"][which]
        assert len(rows) >= 3, (log2n, order, which)
        pick = sorted({rows[0], rows[len(rows) // 2], rows[-1]})
        _, _, want = oracle(order, x0, FS, bands=pick)
        got = c["new"]["one"][t].coef[0][torch.tensor(pick, device="cuda")].cpu().numpy()
        for i, j in enumerate(pick):
            err = relmax(got[i], want[i])
            print(f"2^{log2n} order {order} table {which} row {j}: error against the oracle {err:.3e}")
            assert err <= TOL[np.float32]["coef"], (log2n, order, which, j, err)
