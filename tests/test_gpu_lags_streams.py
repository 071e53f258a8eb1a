"""qi_pair_lags orders its work on the caller's stream (-m gpu): every case of tests/lag_stream_cases.py behind the delayed
producer of tests/test_gpu_streams.py (its harness and its positive control are there), as tests/test_gpu_windows_streams.py
does for the windowed cross-spectra.  Per case: every output equals the serial result on B bit for bit, differs from the stale
result on A, and the call returned before its input was written: all are asynchronous."""
import functools
import time

import numpy as np
import pytest
import torch

import lag_stream_cases as lsc

from test_gpu_streams import behind_producer, delay_ms_for, keep, same_bits

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def built(cid):
    b = lsc.by_id(cid).build()
    assert b.a.shape == b.b.shape and b.a.dtype == b.b.dtype and np.isfinite(b.a).all() and np.isfinite(b.b).all(), cid
    dev = [torch.from_numpy(np.ascontiguousarray(r)).cuda() for r in (b.a, b.b)]  # (complex matrices as interleaved values)
    torch.cuda.synchronize()
    return b, dev[0], dev[1]


def differing(got, want):
    assert len(got) == len(want)
    return [k for k, (g, w) in enumerate(zip(got, want)) if not same_bits(g, w)]


@functools.lru_cache(maxsize=None)
def serial(cid):
    """(want = op(B), stale = op(A), host seconds of the second, warm, call) on the default stream."""
    b, a_dev, b_dev = built(cid)
    torch.cuda.synchronize()
    want = keep(b.op(b_dev))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = b.op(a_dev)
    host = time.perf_counter() - t0
    stale = keep(out)
    torch.cuda.synchronize()
    assert differing(stale, want) == list(range(len(want))), f"{cid}: an output on A equals the one on B: the case has no power"
    for t in want + stale:
        assert torch.isfinite(t).all() and not (t == lsc.FILL).any(), cid
    return want, stale, host


@pytest.mark.parametrize("cid", lsc.ids())
def test_ordered_behind_a_delayed_producer(cid):
    case = lsc.by_id(cid)
    b, a_dev, b_dev = built(cid)
    want, stale, host = serial(cid)
    ms = delay_ms_for(host)
    s = torch.cuda.Stream()
    x = a_dev.clone()
    torch.cuda.synchronize()
    got, early, first = behind_producer(b.op, s, x, b_dev, ms, before=a_dev)
    s.synchronize()  # this stream only, never the device
    assert not differing(first, stale), f"{cid}: the call queued in front (on A) differs from its serial result"
    bad = differing(got, want)
    assert not bad, f"{cid}: outputs {bad} differ from the serial result (equal to the stale one: {[k for k in bad if same_bits(got[k], stale[k])]})"
    assert case.asynchronous and early, f"{cid}: the call returned after its input was written ({host * 1e3:.3f} ms warm, delay {ms:.1f} ms)"
