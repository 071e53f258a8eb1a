"""Every entry point orders its work on the caller's stream (-m gpu).

include/qi_tfr.h promises that every transform is asynchronous on the given stream and does no host synchronisation, and
the record ops, TfrPlan.pooled and pooled_strip repeat it.  On PyTorch's default stream -- the null stream on ROCm, where
the rest of the suite runs -- a launch without its stream argument, a synchronous memset, a hipFFT handle left on the stream
of an earlier call or a side stream that is not rejoined cannot be seen: the wrong stream is the right one.  Here every
case of tests/stream_cases.py runs on a side stream `s` whose input is still being written when the call is made:

    s:  [delay: a chain of in-place passes over a 256 MiB tensor] [op(A) ...] [x <- B] (written) [op(x) ...]

`x` holds record set A until the copy runs; the call on A in front keeps the op's own state busy (see behind_producer).  A launch that is not ordered behind `s` reads A (or a buffer still holding
FILL) and the result differs from the serial result on B bit for bit; a call that waits on the host returns after
`written` has completed, and `early` is false.  The delay is sized per case: ten times the host time of the warm call on
the default stream, at least FLOOR_MS; the chain is timed once per session with events, never by the code under test.
The measured times, the delays and whether `early` held go to profiles/stream_order.txt when every case has run.

Both record sets are legal inputs of the op and every buffer is allocated before any stream reads it: no case faults, a
defect shows as a mismatch.
"""
import functools
import math
import os
import time

import numpy as np
import pytest
import torch

import stream_cases as sc

from quantum_inferno_amd import engine, stream, styx_fft

pytestmark = pytest.mark.gpu

FLOOR_MS = 20.0  # a short op's host time is microseconds: ten times that is timer noise, not a delay
MARGIN = 10      # delay / host time of the call: covers the jitter of the host's enqueue time
LOG_PATH = os.environ.get("QI_STREAM_ORDER_LOG") or os.path.join(sc.ROOT, "profiles", "stream_order.txt")
_LOG = {}


class Delay:
    """Ordinary queued device work of a known duration: in-place passes over one large tensor, timed once with events."""

    def __init__(self):
        self.buf = torch.zeros(64 << 20, dtype=torch.int32, device="cuda")  # 256 MiB: a pass is hundreds of microseconds
        for _ in range(5):
            self.buf.add_(1)
        torch.cuda.synchronize()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self.timed = 50
        start.record()
        for _ in range(self.timed):
            self.buf.add_(1)
        stop.record()
        stop.synchronize()
        self.pass_ms = start.elapsed_time(stop) / self.timed
        assert 0.01 < self.pass_ms < 50.0, self.pass_ms

    def passes(self, ms):
        return int(math.ceil(ms / self.pass_ms))

    def queue(self, ms):
        """On the current stream."""
        for _ in range(self.passes(ms)):
            self.buf.add_(1)


@functools.lru_cache(maxsize=None)
def delay():
    return Delay()


@pytest.fixture(scope="module", autouse=True)
def _plans_and_log():
    yield
    torch.cuda.synchronize()
    sc.close_plans()
    serial.cache_clear()
    built.cache_clear()
    ordered = [cid for cid in sc.ids() if cid in _LOG]
    if len(ordered) == len(sc.ids()):  # (a partial run does not overwrite the record of a whole one)
        d = delay()
        lines = [f"stream order: {len(ordered)} cases of tests/stream_cases.py behind a delayed producer (tests/test_gpu_streams.py)",
                 f"delay chain: {d.timed} in-place passes over 256 MiB timed with events on the default stream: {d.pass_ms:.4f} ms per pass",
                 f"delay = max({FLOOR_MS:g} ms, {MARGIN} x host time of the warm call on the default stream)",
                 "", f"{'case':44s} {'async':>5s} {'host ms':>9s} {'delay ms':>9s} {'passes':>6s} {'early':>5s}"]
        for cid in ordered:
            r = _LOG[cid]
            lines.append(f"{cid:44s} {str(r['asynchronous']):>5s} {r['host_ms']:9.3f} {r['delay_ms']:9.2f} {r['passes']:6d} {str(r['early']):>5s}")
        lines += ["", "notes of the builds (what each plan's own queries said):"] + sorted({_LOG[cid]["note"] for cid in ordered if _LOG[cid]["note"]})
        lines += [""] + [f"{k}: {v}" for k, v in sorted(_LOG.items()) if k not in ordered]
        with open(LOG_PATH, "w") as fh:
            fh.write("\n".join(lines) + "\n")


@functools.lru_cache(maxsize=None)
def built(cid):
    """(Built, A on the device, B on the device) of a case, shared by the tests of this module."""
    b = sc.by_id(cid).build()
    assert b.a.shape == b.b.shape and b.a.dtype == b.b.dtype and np.isfinite(b.a).all() and np.isfinite(b.b).all(), cid
    dev = [torch.from_numpy(np.ascontiguousarray(r)).cuda() for r in (b.a, b.b)]
    torch.cuda.synchronize()
    return b, dev[0], dev[1]


def same_bits(x, y):
    """Equal as integers: equal NaN patterns count as equal, +0 and -0 do not."""
    if x.dtype != y.dtype or x.shape != y.shape:
        return False
    xr, yr = (torch.view_as_real(t) if t.is_complex() else t for t in (x, y))
    return torch.equal(xr.contiguous().view(torch.uint8), yr.contiguous().view(torch.uint8))


def mismatches(got, want):
    assert len(got) == len(want), (len(got), len(want))
    return [k for k, (g, w) in enumerate(zip(got, want)) if not same_bits(g, w)]


def keep(outputs):
    """Copies on the current stream: the closures' kept buffers may be written again by the next call."""
    return tuple(t.clone() for t in outputs)


@functools.lru_cache(maxsize=None)
def serial(cid):
    """(want = op(B), stale = op(A), host seconds of the second, warm, call) on the default stream."""
    b, a_dev, b_dev = built(cid)
    torch.cuda.synchronize()
    want = keep(b.op(b_dev))  # also the warm call: lazy hipFFT plans, per-stream buffers, the caching allocator
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = b.op(a_dev)
    host = time.perf_counter() - t0  # the enqueue alone: nothing is synchronised
    stale = keep(out)
    torch.cuda.synchronize()
    assert mismatches(stale, want), f"{cid}: the results on A and on B are the same bits: the case has no power"
    return want, stale, host


def delay_ms_for(host_seconds):
    return max(FLOOR_MS, MARGIN * host_seconds * 1e3)


def behind_producer(op, s, x, src, ms, before=None):
    """On stream `s`: the delay, x <- src, then op(x) while x is still unwritten -> (copies of the outputs, early, copies
    of the outputs of op(before)).  `before`: a buffer that already holds the other record set; the op runs on it first,
    behind the same delay, so that whatever the op keeps between calls (partial sums a memset clears, scratch, handles) is
    still in use by a queued call when the call under test is made -- a clear or a launch that leaves the stream then meets
    the earlier call's work instead of an idle device."""
    with torch.cuda.stream(s):
        delay().queue(ms)
        first = keep(op(before)) if before is not None else None
        x.copy_(src)
        written = torch.cuda.Event()
        written.record(s)
        got = op(x)
        early = not written.query()
        return keep(got), early, first


def test_control_misordered_call_reads_stale():
    """The harness's positive control: the producer is delayed on a side stream and the op (qi_derivative) is called on the
    default stream, so it is NOT ordered behind the producer and must read A.  It shows on this runtime that a PyTorch side
    stream does not block against the null stream and that the harness sees a launch on the wrong stream.  Both buffers hold
    legal records throughout."""
    cid = "gradient_h"
    assert sc.by_id(cid).functions == ("qi_derivative",)
    b, a_dev, b_dev = built(cid)
    want, stale, host = serial(cid)
    s = torch.cuda.Stream()
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
    _LOG["control"] = f"misordered qi_derivative finished before the producer: {finished_first}; read stale: {not mismatches(got, stale)}"
    assert finished_first, "the default stream waited for the side stream: the harness cannot see a misordered launch here"
    assert not mismatches(got, stale) and mismatches(got, want)
    assert same_bits(x, b_dev)


@pytest.mark.parametrize("cid", sc.ids())
def test_ordered_behind_a_delayed_producer(cid):
    case = sc.by_id(cid)
    b, a_dev, b_dev = built(cid)
    want, stale, host = serial(cid)
    ms = delay_ms_for(host)
    s = torch.cuda.Stream()
    x = a_dev.clone()
    torch.cuda.synchronize()
    got, early, first = behind_producer(b.op, s, x, b_dev, ms, before=a_dev)
    s.synchronize()  # this stream only, never the device
    _LOG[cid] = dict(asynchronous=case.asynchronous, host_ms=host * 1e3, delay_ms=ms, passes=delay().passes(ms), early=early, note=b.note)
    assert not mismatches(first, stale), f"{cid}: the call queued in front (on A) differs from its serial result in {mismatches(first, stale)}"
    bad = mismatches(got, want)
    assert not bad, f"{cid}: outputs {bad} differ from the serial result (equal to the stale one: {[k for k in bad if same_bits(got[k], stale[k])]})"
    if case.asynchronous:
        assert early, f"{cid}: the call returned after its input was written ({host * 1e3:.3f} ms warm, delay {ms:.1f} ms): it waited on the host"


@pytest.mark.parametrize("cid", sc.ids())
def test_alternating_streams(cid):
    """One plan or op instance on default, s1, default, s2 with the records rotated, each call behind a delayed producer on
    its own stream: the hipfftSetStream of the cached handles, the strip partials kept per stream and the plan's side
    stream with its events across changes of stream.  A plan has one scratch (the header: one plan per stream), so each
    stream first waits -- on the device, with an event -- for the call before it, as a caller who moves a plan to another
    stream must; the host never waits, and every call is queued while its own input is unwritten."""
    b, a_dev, b_dev = built(cid)
    want, stale, host = serial(cid)
    ms = delay_ms_for(host)
    streams = [torch.cuda.default_stream(), torch.cuda.Stream(), torch.cuda.default_stream(), torch.cuda.Stream()]
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


def released_together(ops, inputs, wants, what):
    s0, s1, s2 = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    gate = torch.cuda.Event()
    with torch.cuda.stream(s0):
        delay().queue(FLOOR_MS)
        gate.record(s0)
    results = []
    for s, op, x in zip((s1, s2), ops, inputs):
        with torch.cuda.stream(s):
            s.wait_event(gate)
            results.append(keep(op(x)))
    s1.synchronize()
    s2.synchronize()
    for k, (got, ref) in enumerate(zip(results, wants)):
        assert not mismatches(got, ref), f"{what}: stream {k + 1} differs in outputs {mismatches(got, ref)}"


@pytest.mark.parametrize("cid", sc.SHARED_STATE)
def test_two_streams_released_together(cid):
    """Two streams wait for one event behind a delay, then each runs the same plan-less op at the same shape on its own
    records: the hipFFT handles the library keeps per device (re-pointed with hipfftSetStream on every call) and the strip
    partials kept per (device, stream) are shared process-wide state.  Whether the two calls overlap on the device is up to
    the scheduler, so this test can pass by luck; it cannot fail without a defect.  One run, no repetition."""
    b, a_dev, b_dev = built(cid)
    want, stale, _ = serial(cid)
    released_together((b.op, b.op), (a_dev, b_dev), (stale, want), cid)


def test_two_plans_released_together():
    """The same with two TfrPlans on two streams: the hipFFT-engine plan at n = 3000 and the float64 plan at 2^15, whose
    block launch forks to the plan's own side stream.  As above: it can pass by luck, it cannot fail without a defect."""
    cids = ("cwt_stx-f32_n3000-all-r1", "cwt_stx-f64_n32768-all-r1")
    ops, inputs, wants = [], [], []
    for cid in cids:
        b, _, b_dev = built(cid)
        ops.append(b.op)
        inputs.append(b_dev)
        wants.append(serial(cid)[0])
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
    s = torch.cuda.Stream()
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
