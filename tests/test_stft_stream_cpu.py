"""The streamed STFT without a GPU: which segments and samples an item carries (stream.segment_items against a brute-force
listing and against the library's host-only qi_stft_range_samples), the refusals that are decided on the host (ValueError in
Python, QI_ERR_ARG from qi_stft_out_range before any device call), and the assemblers (stream.StftRecord, PooledRecord.merge)
fed CPU tensors as items."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import stft_cases as sc
import stft_stream_cases as ss
from conftest import ROOT

from quantum_inferno_amd import _lib, stream, styx_fft


def test_header_library_and_binding_agree():
    header = open(os.path.join(ROOT, "include", "qi_tfr.h")).read()
    lib = _lib.load()
    assert lib.qi_abi_version() == 1
    for name in ("qi_stft_range_samples", "qi_stft_range_scratch_bytes", "qi_stft_out_range"):
        assert re.search(rf"\b{name}\s*\(", header), f"{name} is not declared"
        assert hasattr(lib, name) and name in _lib.PROTOTYPES
    fields = re.search(r"typedef struct qi_stft_range \{([^}]*)\} qi_stft_range;", header).group(1)
    names = re.findall(r"(\w+)\s*[,;]", fields)
    assert names == [f for f, _ in _lib.StftRange._fields_]
    assert C.sizeof(_lib.StftRange) == 9 * 8


@pytest.mark.parametrize("n_total,seg,hop,per", ss.ITEM_CASES)
def test_segment_items(n_total, seg, hop, per):
    lib = _lib.load()
    items = stream.segment_items(n_total, seg, hop, per)
    n_seg = sc.frame_count(n_total, seg, hop)
    assert n_seg == int(lib.qi_stft_segments(n_total, seg, hop)) == styx_fft._frame_count(n_total, seg, hop)
    # consecutive runs: every segment in exactly one item
    owner = np.zeros(n_seg, dtype=np.int64)
    nxt = 0
    for first, count, _, _ in items:
        assert first == nxt and 1 <= count <= per
        owner[first : first + count] += 1
        nxt = first + count
    assert nxt == n_seg and np.all(owner == 1)
    assert all(count == per for _, count, _, _ in items[:-1])
    for i, (first, count, sample0, n_avail) in enumerate(items):
        lo, hi = ss.brute_interval(n_total, seg, hop, first, count)
        if lo is None:
            assert n_avail == 0 and 0 <= sample0 <= n_total, (i, sample0, n_avail)
        else:  # every in-record sample of its segments, and not one more at either end
            assert (sample0, sample0 + n_avail) == (lo, hi), (i, sample0, n_avail, lo, hi)
        s0, na = C.c_int64(-1), C.c_int64(-1)
        assert lib.qi_stft_range_samples(n_total, seg, hop, first, count, C.byref(s0), C.byref(na)) == 0
        assert (s0.value, na.value) == (sample0, n_avail), i
        assert (sample0, n_avail) == styx_fft.range_samples(n_total, seg, hop, first, count)
    # neighbours overlap by seg - hop samples where neither is cut by an end of the record
    for (f0, c0, s0, n0), (f1, _, s1, n1) in zip(items[:-1], items[1:]):
        if f1 * hop - seg // 2 >= 0 and (f0 + c0 - 1) * hop - seg // 2 + seg <= n_total:
            assert s0 + n0 - s1 == seg - hop


def test_segment_items_known_answers():
    assert [(f, c) for f, c, _, _ in stream.segment_items(10757, 512, 256, 16)] == [(0, 16), (16, 16), (32, 12)]
    assert stream.segment_items(10757, 512, 256, 16)[1][2:] == (16 * 256 - 256, 15 * 256 + 512)
    # hop > seg / 2: the last padded segment starts past the record and needs no sample
    last = stream.segment_items(600, 512, 500, 1)[-1]
    assert sc.last_segment_all_zero(600, 512, 500) and last[3] == 0
    with pytest.raises(ValueError, match="segments_per_item"):
        stream.segment_items(10757, 512, 256, 0)
    with pytest.raises(ValueError):
        stream.segment_items(0, 512, 256, 4)


def test_range_samples_refusals():
    lib = _lib.load()
    s0, na = C.c_int64(), C.c_int64()
    for first, count in ((-1, 2), (0, 0), (40, 5), (44, 1)):
        assert lib.qi_stft_range_samples(10757, 512, 256, first, count, C.byref(s0), C.byref(na)) == -1, (first, count)
    assert lib.qi_stft_range_samples(10757, 512, 256, 0, 1, None, C.byref(na)) == -1


def _range(**kw):
    base = dict(n_total=10757, first_segment=16, segments=16, sample0=3840, n_avail=4352, row_stride=4352, pool_factor=0)
    base.update(kw)
    return _lib.StftRange(**base)


def test_c_refusals_need_no_device():
    """Every refusal of a range is decided before the device is chosen: QI_ERR_ARG with pointers that are never followed."""
    lib = _lib.load()
    buf = np.full(64, 7.0)
    p = buf.ctypes.data_as(C.c_void_p)
    out = _lib.TfrOut(power_band=p, stats=p, power_scale=1.0)

    def call(rng, dtype=_lib.QI_F32, out=out, scratch_bytes=1 << 40):
        return lib.qi_stft_out_range(dtype, 0, p, 3, p, 512, 256, 512, 1.0, C.byref(rng), C.byref(out), p, scratch_bytes, None)

    assert int(lib.qi_stft_range_scratch_bytes(_lib.QI_F32, 3, 512, 256, 512, C.byref(_range()), 0)) > 0
    for bad, word in ((dict(sample0=3841, n_avail=4351), b"needs the record samples"),  # one needed sample short in front
                      (dict(n_avail=4351), b"needs the record samples"),  # ... and behind
                      (dict(n_avail=0), b"needs the record samples"),
                      (dict(first_segment=32, segments=13), b"segments"),  # past the last segment
                      (dict(first_segment=44, segments=1), b"segments"),
                      (dict(segments=0), b"segments"),
                      (dict(first_segment=-1), b"segments"),
                      (dict(row_stride=4351), b"rows of"),
                      (dict(sample0=-1), b"not inside"),
                      (dict(sample0=10000, n_avail=758), b"not inside"),
                      (dict(n_total=0), b"geometry"),
                      (dict(pool_factor=1), b"pooling factor"),
                      (dict(pool_factor=-4), b"pooling factor"),
                      (dict(pool_factor=3), b"no multiple"),  # first_segment % F != 0
                      (dict(pool_factor=16, segments=12, n_avail=11 * 256 + 512), b"do not end the record"),
                      (dict(pool_mean=p), b"without a pooling factor")):
        rng = _range(**bad)
        assert call(rng) == -1 and word in lib.qi_last_error(), (bad, lib.qi_last_error())
        assert int(lib.qi_stft_range_scratch_bytes(_lib.QI_F32, 3, 512, 256, 512, C.byref(rng), 0)) == -1, bad
    assert call(_range(), dtype=2) == -1 and b"dtype" in lib.qi_last_error()
    assert call(_range(), out=_lib.TfrOut()) == -1 and b"nothing to produce" in lib.qi_last_error()
    assert call(_range(pool_factor=4, pool_mean=p), out=_lib.TfrOut(coef=p)) == -1 and b"come with" in lib.qi_last_error()
    assert call(_range(), scratch_bytes=16) == -1 and b"scratch" in lib.qi_last_error()
    assert (buf == 7.0).all()


def test_python_refusals_come_before_the_device():
    """ValueError for what the host can decide -- raised with CPU tensors, so no device call came first."""
    win = styx_fft.tukey_window_periodic(512, 1.0)
    plan = styx_fft.StftRangePlan(10757, sc.FS, window=win, overlap_points=256, nfft_points=512)
    assert (plan.seg, plan.hop, plan.nfft, plan.n_seg, plan.n_f) == (512, 256, 512, 44, 257)
    assert len(plan.time_s) == 44 and len(plan.frequency_hz) == 257
    rows = torch.zeros((3, 4352), dtype=torch.float32)
    for kw, word in ((dict(first_segment=16, segments=16, sample0=3841), "needs the record samples"),
                     (dict(first_segment=32, segments=13, sample0=7936), "segments"),
                     (dict(first_segment=16, segments=16, sample0=3840, pooled=3), "multiple"),
                     (dict(first_segment=16, segments=12, sample0=3840, pooled=8), "do not end the record"),
                     (dict(first_segment=16, segments=16, sample0=3840, pooled=1), "pooling factor"),
                     (dict(first_segment=16, segments=16, sample0=3840, pooled=4, pooled_methods=("median",)), "pooled_methods"),
                     (dict(first_segment=16, segments=16, sample0=3840, pooled=4, reductions=False, coef=True), "reductions"),
                     (dict(first_segment=16, segments=16, sample0=3840, reductions=False), "nothing to produce"),
                     (dict(first_segment=16, segments=16, sample0=3840, n_avail=5000), "cannot hold"),
                     (dict(first_segment=16, segments=16, sample0=3840, n_total=999), "plan is for")):
        with pytest.raises(ValueError, match=word):
            plan.segment_range(rows, **kw)
    with pytest.raises(ValueError, match="2-D"):
        plan.segment_range(rows.double(), 16, 16, 3840)
    with pytest.raises(ValueError, match="contiguous"):
        plan.segment_range(torch.zeros((3, 8704))[:, ::2], 16, 16, 3840)
    with pytest.raises(ValueError):
        styx_fft.StftRangePlan(10757, sc.FS)  # neither an order nor a window
    with pytest.raises(ValueError):
        styx_fft.StftRangePlan(10757, sc.FS, window=win, overlap_points=512)
    with pytest.raises(ValueError):
        styx_fft.StftRangePlan(10757, sc.FS, window=win, nfft_points=256)
    with pytest.raises(ValueError, match="less than"):
        styx_fft.StftRangePlan(100, sc.FS, 1)
    by_order = styx_fft.StftRangePlan(385, sc.FS, 1)  # stft_from_sig's geometry from the order
    assert (by_order.seg, by_order.hop, by_order.nfft) == (sc.PLAN_ORDERS[1], sc.PLAN_ORDERS[1] // 2, sc.PLAN_ORDERS[1])
    host = np.zeros((3, 10757), dtype=np.float32)
    with pytest.raises(ValueError, match="multiple"):
        stream.StftStream(plan, host, segments_per_item=16, pooled=3, device="cpu")
    with pytest.raises(ValueError, match="pooled_methods"):
        stream.StftStream(plan, host, segments_per_item=16, pooled=4, pooled_methods=("min",), device="cpu")
    with pytest.raises(ValueError, match="segments_per_item"):
        stream.StftStream(plan, host, segments_per_item=0, device="cpu")
    with pytest.raises(ValueError, match="samples"):
        stream.StftStream(plan, host[:, :-1], segments_per_item=16, device="cpu")
    pipe = stream.StftStream(plan, host, segments_per_item=16, block=2, pooled=4, device="cpu")
    assert [i[:4] for i in pipe.items] == [(0, 2, 0, 16), (0, 2, 16, 16), (0, 2, 32, 12), (2, 1, 0, 16), (2, 1, 16, 16), (2, 1, 32, 12)]


# ---- the assemblers ----------------------------------------------------------------------------------------------------------
N_CH, N_F, N_SEG, F = 5, 7, 44, 4


def _fake_items(exact):
    """Items of a [5 channels, 44 segments] record set in blocks of 2 channels and ranges of 16 segments, block-major.
    exact: values that are small multiples of 2^-10, so that every order of summation gives the same bits."""
    rng = np.random.default_rng(11)
    draw = (lambda *s: np.round(rng.random(s) * 1024) / 1024) if exact else (lambda *s: rng.random(s) + 0.1)
    items = []
    for c0 in range(0, N_CH, 2):
        cb = min(2, N_CH - c0)
        for first in range(0, N_SEG, 16):
            count = min(16, N_SEG - first)
            res = ss.FakeResult(torch.from_numpy(draw(cb, N_F)), torch.from_numpy(np.concatenate([draw(cb, 3), np.zeros((cb, 1))], 1)),
                                torch.from_numpy(draw(cb, count).astype(np.float32)),
                                {m: torch.from_numpy(draw(cb, N_F, count // F).astype(np.float32)) for m in ("average", "max")})
            items.append(stream.StftItem(len(items), c0, cb, first, count, 0, 0, res, first // F, count // F))
    return items


def _assemble(items, skip=()):
    rec = stream.StftRecord(N_CH, N_F, N_SEG, pooled=F, methods=("average", "max"))
    for it in items:
        if it.index not in skip:
            rec.add(it)
    return rec


def _same(a, b):
    ok = torch.equal(a.power_band, b.power_band) and torch.equal(a.stats, b.stats)
    ok = ok and torch.equal(torch.isnan(a.power_time), torch.isnan(b.power_time))
    ok = ok and torch.equal(torch.nan_to_num(a.power_time), torch.nan_to_num(b.power_time))
    for m in a.panel:
        ok = ok and torch.equal(torch.isnan(a.panel[m]), torch.isnan(b.panel[m]))
        ok = ok and torch.equal(torch.nan_to_num(a.panel[m]), torch.nan_to_num(b.panel[m]))
    return ok


@pytest.mark.parametrize("split,exact", [(6, False), (3, False), (4, True), (1, True)])
def test_stft_record_merge_equals_one_assembler(split, exact):
    """Two rank shares merged are the assembler that was fed everything, bit for bit: splits at a channel-block boundary
    (items 0 - 5 | 6 - 8, 0 - 2 | 3 - 8) with any values, splits inside a block with values whose sums are exact (a record's
    sums are then added in another order)."""
    items = _fake_items(exact)
    assert len(items) == 9
    whole = _assemble(items)
    merged = _assemble(items[:split]).merge(_assemble(items[split:]))
    assert _same(merged, whole)
    assert not torch.isnan(whole.power_time).any() and not any(torch.isnan(p).any() for p in whole.panel.values())
    # by position: what an item carried is where it belongs
    it = items[4]
    assert torch.equal(whole.power_time[2:4, 16:32], it.stft.power_time) and torch.equal(whole.panel["max"][2:4, :, 4:8], it.stft.pooled["max"])
    res = whole.result()
    assert res.power_band is whole.power_band and res.stats is whole.stats and res.pooled is whole.panel
    ref_band = sum(i.stft.power_band.numpy() for i in items if i.first_channel == 2)
    assert np.allclose(whole.power_band[2:4].numpy(), ref_band, rtol=1e-14)
    assert np.array_equal(whole.stats[2:4, 0].numpy(), np.max([i.stft.stats[:, 0].numpy() for i in items if i.first_channel == 2], axis=0))
    assert torch.all(res.total_power == whole.stats[:, 1])


def test_nan_stays_where_nobody_added():
    items = _fake_items(False)
    a, b = _assemble(items[:3], skip=(1,)), _assemble(items[3:], skip=(8,))
    merged = a.merge(b)
    # item 1: channels 0 - 1, segments 16 .. 31; item 8: channel 4, segments 32 .. 43
    gap = torch.zeros((N_CH, N_SEG), dtype=torch.bool)
    gap[0:2, 16:32] = True
    gap[4, 32:44] = True
    assert torch.equal(torch.isnan(merged.power_time), gap)
    for m in ("average", "max"):
        assert torch.equal(torch.isnan(merged.panel[m]), gap[:, None, ::F].expand(N_CH, N_F, N_SEG // F))
    with pytest.raises(ValueError):
        merged.merge(stream.StftRecord(N_CH, N_F, N_SEG, pooled=F, methods=("average",)))
    with pytest.raises(ValueError, match="pooled strips"):
        bare = stream.StftItem(0, 0, 2, 0, 16, 0, 0, ss.FakeResult(items[0].stft.power_band, items[0].stft.stats, items[0].stft.power_time))
        stream.StftRecord(N_CH, N_F, N_SEG, pooled=F).add(bare)
    # without pooling and without per-time power: the sums alone
    small = stream.StftRecord(N_CH, N_F, N_SEG, keep_time=False)
    small.add(items[0])
    assert small.power_time is None and small.result().pooled is None and torch.equal(small.power_band[0:2], items[0].stft.power_band)


def _pooled_item(index, c0, cb, w0, nw, draw):
    res = ss.FakeResult(torch.from_numpy(draw(cb, N_F)), torch.from_numpy(np.concatenate([draw(cb, 3), np.zeros((cb, 1))], 1)),
                        pooled={"average": torch.from_numpy(draw(cb, N_F, nw).astype(np.float32))})
    return stream.StreamItem(index, c0, cb, index, 0, res, None, w0, nw)


def test_pooled_record_merge():
    """PooledRecord.merge: rank shares of a chunked record (split at a channel-block boundary) merged are the one assembler,
    bit for bit; columns nobody added stay NaN."""
    rng = np.random.default_rng(5)
    draw = lambda *s: rng.random(s) + 0.1
    items = [_pooled_item(i, c0, 2, w0, 3, draw) for i, (c0, w0) in enumerate((c0, w0) for c0 in (0, 2) for w0 in (0, 3, 6))]

    def assemble(part):
        rec = stream.PooledRecord(4, N_F, 10, dtype=torch.float32)
        for it in part:
            rec.add(it, "cwt")
        return rec

    whole, merged = assemble(items), assemble(items[:3]).merge(assemble(items[3:]))
    assert torch.equal(merged.power_band, whole.power_band) and torch.equal(merged.stats, whole.stats)
    nan = torch.isnan(whole.panel["average"])
    assert torch.equal(torch.isnan(merged.panel["average"]), nan) and torch.equal(merged.panel["average"][~nan], whole.panel["average"][~nan])
    assert nan[:, :, 9].all() and not nan[:, :, :9].any()  # (window 9 belongs to no item)
    assert merged.frequency_hz is not None
    empty = stream.PooledRecord(4, N_F, 10, dtype=torch.float32).merge(assemble(items[:3]))
    assert torch.equal(empty.power_band, assemble(items[:3]).power_band) and torch.isnan(empty.panel["average"][2:]).all()
    with pytest.raises(ValueError):
        whole.merge(stream.PooledRecord(4, N_F, 11, dtype=torch.float32))
