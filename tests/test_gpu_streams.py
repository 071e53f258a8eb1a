"""Every entry point orders its work on the caller's stream (-m gpu).

include/qi_tfr.h promises that every transform is asynchronous on the given stream and does no host synchronisation, and
the record ops, TfrPlan.pooled and pooled_strip repeat it.  On PyTorch's default stream -- the null stream on ROCm, where
the rest of the suite runs -- a launch without its stream argument, a synchronous memset, a hipFFT handle left on the stream
of an earlier call or a side stream that is not rejoined cannot be seen: the wrong stream is the right one.  Here every
case of tests/stream_cases.py runs on a side stream whose input is still being written when the call is made, with the
harness of tests/stream_order.py (the delayed producer, the side streams shown independent of the default stream, the
record in profiles/stream_order.txt); the harness's positive control is here.  tests/test_gpu_header_streams.py does the
first of these tests for the tables of the other headers.

Both record sets are legal inputs of the op and every buffer is allocated before any stream reads it: no case faults, a
defect shows as a mismatch.
"""
import numpy as np
import pytest
import torch

import stream_cases as sc
import stream_order as so
from stream_order import FLOOR_MS, behind_producer, delay, delay_ms_for, keep, mismatches, released_together, same_bits, side_streams

from quantum_inferno_amd import engine, stream, styx_fft

pytestmark = pytest.mark.gpu

T = sc.TABLE


@pytest.fixture(scope="module", autouse=True)
def _plans_and_log():
    yield
    torch.cuda.synchronize()
    sc.close_plans()
    so.clear_cases()
    so.write_log()


def test_control_misordered_call_reads_stale():
    """The harness's positive control: the producer is delayed on a side stream and the op (qi_derivative) is called on the
    default stream, so it is NOT ordered behind the producer and must read A.  It shows on this runtime that the side stream
    the harness hands out does not block against the null stream and that the harness sees a launch on the wrong stream.
    Both buffers hold legal records throughout."""
    cid = "gradient_h"
    assert T.by_id(cid).functions == ("qi_derivative",)
    b, a_dev, b_dev = so.built(T, cid)
    want, stale, host = so.serial(T, cid)
    (s,) = side_streams(1)
    x = a_dev.clone()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        delay().queue(delay_ms_for(host))
        x.copy_(b_dev)
        written = torch.cuda.Event()
        written.record(s)
    got = keep(b.op(x))  # the default stream: the wrong one
    torch.cuda.default_stream().synchronize()
    finished_first = not written.query()
    s.synchronize()
    so.LOG["control"] = f"misordered qi_derivative finished before the producer: {finished_first}; read stale: {not mismatches(got, stale)}"
    assert finished_first, so.NO_SIDE_STREAM
    assert not mismatches(got, stale) and mismatches(got, want)
    assert same_bits(x, b_dev)


@pytest.mark.parametrize("cid", T.ids())
def test_ordered_behind_a_delayed_producer(cid):
    so.ordered_behind_producer(T, cid)


@pytest.mark.parametrize("cid", T.ids())
def test_alternating_streams(cid):
    """One plan or op instance on default, s1, default, s2 with the records rotated, each call behind a delayed producer on
    its own stream: the hipfftSetStream of the cached handles, the strip partials kept per stream and the plan's side
    stream with its events across changes of stream.  A plan has one scratch (the header: one plan per stream), so each
    stream first waits -- on the device, with an event -- for the call before it, as a caller who moves a plan to another
    stream must; the host never waits, and every call is queued while its own input is unwritten."""
    b, a_dev, b_dev = so.built(T, cid)
    want, stale, host = so.serial(T, cid)
    ms = delay_ms_for(host)
    s1, s2 = side_streams(2)
    streams = [torch.cuda.default_stream(), s1, torch.cuda.default_stream(), s2]
    sources, wants = [b_dev, a_dev, b_dev, a_dev], [want, stale, want, stale]
    xs = [(a_dev if src is b_dev else b_dev).clone() for src in sources]
    torch.cuda.synchronize()
    results, before = [], None
    for s, x, src in zip(streams, xs, sources):
        if before is not None:
            s.wait_event(before)
        results.append(behind_producer(b.op, s, x, src, ms)[0])
        before = torch.cuda.Event()
        before.record(s)
    for s in streams[1:]:
        s.synchronize()
    for k, (got, ref) in enumerate(zip(results, wants)):
        assert not mismatches(got, ref), f"{cid}: call {k} (0 and 2 on the default stream) differs in outputs {mismatches(got, ref)}"


@pytest.mark.parametrize("cid", sc.SHARED_STATE)
def test_two_streams_released_together(cid):
    """Two streams wait for one event behind a delay, then each runs the same plan-less op at the same shape on its own
    records: the hipFFT handles the library keeps per device (re-pointed with hipfftSetStream on every call) and the strip
    partials kept per (device, stream) are shared process-wide state.  Whether the two calls overlap on the device is up to
    the scheduler, so this test can pass by luck; it cannot fail without a defect.  One run, no repetition."""
    b, a_dev, b_dev = so.built(T, cid)
    want, stale, _ = so.serial(T, cid)
    released_together((b.op, b.op), (a_dev, b_dev), (stale, want), cid)


def test_two_plans_released_together():
    """The same with two TfrPlans on two streams: the hipFFT-engine plan at n = 3000 and the float64 plan at 2^15, whose
    block launch forks to the plan's own side stream.  As above: it can pass by luck, it cannot fail without a defect."""
    cids = ("cwt_stx-f32_n3000-all-r1", "cwt_stx-f64_n32768-all-r1")
    ops, inputs, wants = [], [], []
    for cid in cids:
        b, _, b_dev = so.built(T, cid)
        ops.append(b.op)
        inputs.append(b_dev)
        wants.append(so.serial(T, cid)[0])
    released_together(ops, inputs, wants, "two plans")


def _item_tensors(items):
    out = []
    for it in items:
        for res in (getattr(it, "cwt", None), getattr(it, "stx", None), getattr(it, "stft", None)):
            if res is None:
                continue
            out += [t for t in (res.power_band, res.power_time, res.stats) if t is not None]
            out += [res.pooled[m] for m in sorted(res.pooled or {})]
    return tuple(out)


def test_pipelines_under_a_busy_current_stream():
    """StreamPipeline, StftStream and PlanRing built and run while the current stream is a side stream with a delay pending:
    _Staging's `allocated`, `copied` and `consumed` events and PlanRing's wait_stream order them behind it.  Every item or
    result is bit-equal to the run on the default stream."""
    n, hop, records = 4096, 2048, 3
    host = sc.noise(30, (records, n + 2 * hop), np.float64)
    nb = len(engine.scales.log_frequency_hz_from_fft_points(sc.FS, n, sc.ORDER))
    plan = engine.TfrPlan(n, torch.float64, None, engine.TfrPlan.workspace_for(n, nb, torch.float64, 2))
    plan.set_styx_bank(sc.ORDER, sc.FS)
    plan.set_stx_bands(sc.ORDER, sc.FS)
    seg = 256
    host32 = sc.noise(31, (records, 16 * seg + 1), np.float32)
    stft_plan = styx_fft.StftRangePlan(host32.shape[1], sc.FS, window=styx_fft.tukey_window_periodic(seg, 0.25),
                                       overlap_points=seg // 2, nfft_points=seg, dtype=torch.float32)
    ring = engine.PlanRing(2048, torch.float32, setup=lambda p: (p.set_styx_bank(sc.ORDER, sc.FS), p.set_stx_bands(sc.ORDER, sc.FS)),
                           depth=2, wait_input=True)
    ring_a, ring_b = (torch.from_numpy(r).cuda() for r in sc.record_pair((1, 2048), "float32", 32))

    def pipelines():
        """Built here, under whatever stream is current."""
        both = list(stream.StreamPipeline(plan, host, hop, block=2, transforms=("cwt", "stx")).run())
        pooled = list(stream.StreamPipeline(plan, host, hop, block=2, pooled=64, pooled_methods=("average", "max")).run())
        stft = list(stream.StftStream(stft_plan, host32, segments_per_item=8, block=2, pooled=2, pooled_methods=("average", "max")).run())
        assert len(both) == len(pooled) == 6 and len(stft) > 2
        return keep(_item_tensors(both) + _item_tensors(pooled) + _item_tensors(stft))

    def ring_call(x):
        res_c, res_s, done = ring.cwt_stx(x, coef=True, reductions=True)
        done.synchronize()
        return keep(sc._tensors(res_c, res_s))

    want = pipelines()
    ring_want = ring_call(ring_b)
    torch.cuda.synchronize()
    (s,) = side_streams(1)
    x = ring_a.clone()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        delay().queue(FLOOR_MS)
        got = pipelines()
        delay().queue(FLOOR_MS)
        x.copy_(ring_b)  # the ring's record is written by the delayed producer
        ring_got = ring_call(x)
    s.synchronize()
    ring.close()
    plan.close()
    assert not mismatches(got, want), mismatches(got, want)
    assert not mismatches(ring_got, ring_want), mismatches(ring_got, ring_want)
