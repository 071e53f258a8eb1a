"""The streamed STFT on the GPU (-m gpu): qi_stft_out_range through styx_fft.StftRangePlan, stream.StftStream and
stream.StftRecord against the float64 oracle panel of the WHOLE record (tests/stft_stream_cases.py has the cases, the
references and the bounds).  Which branch each group is there for:

  test_full_range_is_the_one_call_transform
      first_segment = 0, every segment, sample0 = 0, n_avail = row_stride = n_total, no pooling: the five outputs of the
      one-call transform (qi_stft_out through _stft_windowed) bit for bit, with both panels and with none; a fused PLAIN
      shape, a general fused shape, a hipFFT shape, and stft_from_sig's geometry from the order.
  test_ranges
      items of 16 / 16 / 12 segments (and the other shapes' items) plus one single-segment item, each staged in rows wider
      than n_avail whose unused part is NaN (a read past n_avail shows in the output): the signed origin, the row stride,
      the guarded loaders at both record ends and at a range's own ends, an odd sample0 (seg201_hop101: `whole` false), the
      frames kernel's stride (seg200_nfft300).  Coefficients and bits against the oracle's columns at
      test_gpu_stft_shapes.py's bounds; the assembled reductions through check_reduced.
  test_pooled
      F = 4, 16, 32, 12 at nfft 512 (groups of 4, 16, 16, 4 segments; F = 32: two groups per window) and F = 2, 8, 3 at nfft
      4096 on 24 segments (float32: groups of 2, 2, 1 from the fused kernel; float64: the hipFFT panel and the strip kernel),
      mean and max (the MX instantiations), no coef buffer; a ragged last window dropped; the same call twice; an aligned
      sub-range gives the same windows (for F = 32 it holds no complete window at all).
  test_stft_stream
      a host record set through the double buffering with a ragged last channel block, world = 1 against the references and
      world = 2 merged against world = 1.
  test_refusals
      what the issue lists, with device buffers: QI_ERR_ARG / ValueError, and nothing written.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import stft_cases as sc
import stft_reduced_cases as rc
import stft_stream_cases as ss
from test_gpu_parity import TOL, check_bits
from test_gpu_stft_shapes import check_panels

from quantum_inferno_amd import _lib, stream, styx_fft

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
IDS = ["f64", "f32"]
TORCH = {np.float64: torch.float64, np.float32: torch.float32}
BOTH = ("average", "max")


def make_plan(shape, dtype):
    n = record_length(shape)
    return styx_fft.StftRangePlan(n, sc.FS, dtype=TORCH[dtype], **ss.plan_arguments(shape))


def record_length(shape):
    return shape.case.n


def one_call(shape, dtype, x, **options):
    """The one-call transform of the whole record (qi_stft_out) with the wrappers' window and scale"""
    seg, hop, nfft = ss.geometry(shape)
    kw = ss.plan_arguments(shape)
    return styx_fft._stft_windowed(x, sc.FS, kw["window"], seg, seg - hop, nfft, extra_scale=kw.get("extra_scale", 1.0),
                                   _reduce=options)[2]


def staged(x, sample0, n_avail, extra=37):
    """Device rows [C, n_avail + extra] holding x[:, sample0 : sample0 + n_avail] and NaN behind it"""
    rows = torch.full((x.shape[0], n_avail + extra), float("nan"), dtype=x.dtype, device="cuda")
    rows[:, :n_avail] = x[:, sample0 : sample0 + n_avail]
    return rows


def as_numpy(rec_or_res):
    r = rec_or_res
    pt = None if r.power_time is None else r.power_time.cpu().numpy()
    ent = r.entropy_bits.cpu().numpy() if hasattr(r, "entropy_bits") else r.result().entropy_bits.cpu().numpy()
    return r.power_band.cpu().numpy(), pt, r.stats.cpu().numpy(), ent


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", ss.SHAPES, ids=lambda s: s.name)
def test_full_range_is_the_one_call_transform(shape, dtype):
    x = torch.from_numpy(ss.record(shape, dtype)).cuda()
    plan = make_plan(shape, dtype)
    for panels in (True, False):
        want = one_call(shape, dtype, x, coef=panels, bits=panels)
        got = plan.segment_range(x, 0, plan.n_seg, 0, coef=panels, bits=panels)
        if panels:
            assert torch.equal(got.coef, want.coef) and torch.equal(got.bits, want.bits), shape.name
        else:
            assert got.coef is None and got.bits is None
        assert torch.equal(got.power_band, want.power_band) and torch.equal(got.power_time, want.power_time), (shape.name, panels)
        assert torch.equal(got.stats, want.stats), (shape.name, panels)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_full_range_from_the_order(dtype):
    """stft_from_sig's geometry from band_order_nth: the panels of stft_from_sig, the reductions of stft_reductions_from_sig"""
    seg = sc.PLAN_ORDERS[1]
    case = sc.FromSig(seg, 3 * seg + 1)
    x = torch.from_numpy(sc.from_sig_record(case, dtype)).cuda()
    plan = styx_fft.StftRangePlan(case.n, sc.FS, 1, dtype=TORCH[dtype])
    z, bits, t, f = styx_fft.stft_from_sig(x, sc.FS, 1)
    want, _, _ = styx_fft.stft_reductions_from_sig(x, sc.FS, 1)
    got = plan.segment_range(x, 0, plan.n_seg, 0, coef=True, bits=True)
    assert np.array_equal(plan.time_s, t) and np.array_equal(plan.frequency_hz, f)
    assert torch.equal(got.coef, z) and torch.equal(got.bits, bits)
    assert torch.equal(got.power_band, want.power_band) and torch.equal(got.power_time, want.power_time) and torch.equal(got.stats, want.stats)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", ss.SHAPES, ids=lambda s: s.name)
def test_ranges(shape, dtype):
    tol = TOL[dtype]
    seg, hop, nfft = ss.geometry(shape)
    x_host = ss.record(shape, dtype)
    x = torch.from_numpy(x_host).cuda()
    z_ref = ss.reference(shape, dtype)
    plan = make_plan(shape, dtype)
    items = stream.segment_items(x.shape[1], seg, hop, shape.per_item)
    if shape is ss.SHAPES[0]:
        assert [(f, c) for f, c, _, _ in items] == [(0, 16), (16, 16), (32, 12)]
    single = 17 if plan.n_seg > 17 else 5
    lone = (single, 1) + styx_fft.range_samples(x.shape[1], seg, hop, single, 1)
    if shape.name == "seg201_hop101":
        assert lone[2] % 2 == 1 and items[1][2] % 2 == 1  # off the aligned fast path
    record = stream.StftRecord(sc.CHANNELS, plan.n_f, plan.n_seg, dtype=TORCH[dtype], device="cuda")
    for i, (first, count, sample0, n_avail) in enumerate(items + [lone]):
        rows = staged(x, sample0, n_avail)
        res = plan.segment_range(rows, first, count, sample0, coef=True, bits=True, n_avail=n_avail)
        z, bits = res.coef.cpu().numpy(), res.bits.cpu().numpy()
        assert np.all(np.isfinite(z)) and np.all(np.isfinite(bits)) and torch.isfinite(res.power_time).all(), (shape.name, i)
        cols = z_ref[:, :, first : first + count]
        check_panels(z, cols, tol["coef"], f"{shape.name} item {i}")
        for c in range(sc.CHANNELS):
            check_bits(bits[c], cols[c], tol)
        # the reductions do not depend on whether the panels are stored
        bare = plan.segment_range(rows, first, count, sample0, n_avail=n_avail)
        assert torch.equal(bare.power_band, res.power_band) and torch.equal(bare.stats, res.stats) and torch.equal(bare.power_time, res.power_time)
        if i < len(items):
            record.add(stream.StftItem(i, 0, sc.CHANNELS, first, count, sample0, n_avail, bare))
    assert not torch.isnan(record.power_time).any()
    rc.check_reduced(*as_numpy(record), rc.reduce_reference(z_ref), dtype, shape.name)


def pooled_params():
    out = [pytest.param(ss.Shape("seg512_n10757", ss.RECORD, 16), f, id=f"nfft512-F{f}") for f in ss.POOL_512]
    return out + [pytest.param(ss.Shape("seg4096_24", ss.LONG, 8), f, id=f"nfft4096-F{f}") for f in ss.POOL_4096]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape,factor", pooled_params())
def test_pooled(shape, factor, dtype):
    x = torch.from_numpy(ss.record(shape, dtype)).cuda()
    z_ref = ss.reference(shape, dtype)
    plan = make_plan(shape, dtype)
    n_seg = plan.n_seg
    assert n_seg == z_ref.shape[-1] == (44 if shape.case is ss.RECORD else 24)
    power_scale = 0.5
    res = plan.segment_range(x, 0, n_seg, 0, pooled=factor, pooled_methods=BOTH, power_scale=power_scale)
    assert res.coef is None and res.bits is None
    mean_ref, max_ref = ss.pooled_reference(z_ref, factor, power_scale)
    assert mean_ref.shape[-1] == n_seg // factor >= 1
    ss.check_pooled(res.pooled["average"].cpu().numpy(), mean_ref, dtype, f"{shape.name} F {factor} mean")
    ss.check_pooled(res.pooled["max"].cpu().numpy(), max_ref, dtype, f"{shape.name} F {factor} max")
    # smaller groups, another order of summation: the reductions hold their bounds
    rc.check_reduced(res.power_band.cpu().numpy(), res.power_time.cpu().numpy(), res.stats.cpu().numpy(), res.entropy_bits.cpu().numpy(),
                     rc.reduce_reference(z_ref, power_scale), dtype, f"{shape.name} F {factor}")
    again = plan.segment_range(x, 0, n_seg, 0, pooled=factor, pooled_methods=BOTH, power_scale=power_scale)
    for m in BOTH:
        assert torch.equal(again.pooled[m], res.pooled[m]), (factor, m)
    assert torch.equal(again.power_band, res.power_band) and torch.equal(again.stats, res.stats)
    # one method alone (the mean needs no maxima from the kernel) gives the same bits
    mean_only = plan.segment_range(x, 0, n_seg, 0, pooled=factor, pooled_methods=("average",), power_scale=power_scale)
    max_only = plan.segment_range(x, 0, n_seg, 0, pooled=factor, pooled_methods=("max",), power_scale=power_scale)
    assert torch.equal(mean_only.pooled["average"], res.pooled["average"]) and torch.equal(max_only.pooled["max"], res.pooled["max"])
    # an aligned sub-range, staged on its own (other alignments: the loaders may take another path, the last bits may differ):
    # the same windows of the record; for F = 32 it holds no complete window at all
    first, count = factor, min(2 * factor, n_seg - factor)
    sample0, n_avail = styx_fft.range_samples(x.shape[1], plan.seg, plan.hop, first, count)
    part = plan.segment_range(staged(x, sample0, n_avail), first, count, sample0, pooled=factor, pooled_methods=BOTH,
                              power_scale=power_scale, n_avail=n_avail)
    w0, nw = first // factor, count // factor
    assert nw == (0 if factor == 32 else (1 if factor == 16 else 2))
    for m, ref in zip(BOTH, (mean_ref, max_ref)):
        assert part.pooled[m].shape == (sc.CHANNELS, plan.n_f, nw)
        if nw:
            ss.check_pooled(part.pooled[m].cpu().numpy(), ref[:, :, w0 : w0 + nw], dtype, f"{shape.name} F {factor} part {m}")


def run_stream(plan, host, rank, world, record):
    pipe = stream.StftStream(plan, host, segments_per_item=16, block=2, pooled=4, pooled_methods=BOTH, device="cuda")
    seen = []
    for item in pipe.run(rank, world):
        record.add(item)
        seen.append((item.first_channel, item.channels, item.first_segment, item.segments))
    return seen


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_stft_stream(dtype):
    shape = ss.SHAPES[0]
    host = ss.record(shape, dtype)  # [3, 10757] on the host
    z_ref = ss.reference(shape, dtype)
    plan = make_plan(shape, dtype)
    new = lambda: stream.StftRecord(sc.CHANNELS, plan.n_f, plan.n_seg, pooled=4, methods=BOTH, dtype=TORCH[dtype], device="cuda")
    whole = new()
    seen = run_stream(plan, host, 0, 1, whole)
    assert seen == [(0, 2, 0, 16), (0, 2, 16, 16), (0, 2, 32, 12), (2, 1, 0, 16), (2, 1, 16, 16), (2, 1, 32, 12)]
    assert not torch.isnan(whole.power_time).any() and not any(torch.isnan(p).any() for p in whole.panel.values())
    rc.check_reduced(*as_numpy(whole), rc.reduce_reference(z_ref), dtype, "streamed")
    mean_ref, max_ref = ss.pooled_reference(z_ref, 4)
    assert whole.panel["average"].shape == (sc.CHANNELS, plan.n_f, 11)
    ss.check_pooled(whole.panel["average"].cpu().numpy(), mean_ref, dtype, "streamed mean")
    ss.check_pooled(whole.panel["max"].cpu().numpy(), max_ref, dtype, "streamed max")
    res = whole.result()
    assert res.power_per_band_bits().shape == (sc.CHANNELS, plan.n_f) and torch.equal(res.total_power, whole.stats[:, 1])
    # two ranks, merged
    halves = [new(), new()]
    parts = [run_stream(plan, host, r, 2, halves[r]) for r in range(2)]
    assert parts[0] + parts[1] == seen and parts[0] and parts[1]
    assert torch.isnan(halves[0].power_time[2]).all() and torch.isnan(halves[1].panel["max"][:2]).all()
    merged = halves[0].merge(halves[1])
    assert torch.equal(merged.power_band, whole.power_band) and torch.equal(merged.stats, whole.stats)
    assert torch.equal(merged.power_time, whole.power_time)
    for m in BOTH:
        assert torch.equal(merged.panel[m], whole.panel[m]), m
    # the restart cursor: from item 4 on
    pipe = stream.StftStream(plan, host, segments_per_item=16, block=2, device="cuda")
    tail = list(pipe.run(first_item=4))
    assert [(i.index, i.first_channel, i.first_segment) for i in tail] == [(4, 2, 16), (5, 2, 32)]
    assert tail[0].stft.pooled is None and tail[0].windows is None


def test_refusals():
    lib = _lib.require_gpu()
    shape, dtype = ss.SHAPES[0], np.float32
    x = torch.from_numpy(ss.record(shape, dtype)).cuda()
    plan = make_plan(shape, dtype)
    first, count, sample0, n_avail = stream.segment_items(x.shape[1], 512, 256, 16)[1]
    rows = staged(x, sample0, n_avail)
    for kw in (dict(first_segment=first, segments=count, sample0=sample0 + 1),  # needs a sample that is not supplied
               dict(first_segment=first, segments=count, sample0=sample0, n_avail=n_avail - 1),
               dict(first_segment=first + 2, segments=count, sample0=sample0, pooled=4),  # first_segment % F != 0
               dict(first_segment=32, segments=13, sample0=7936)):  # past the last segment
        with pytest.raises(ValueError):
            plan.segment_range(rows, **kw)
    # the library's own refusals, with device buffers: QI_ERR_ARG and nothing written
    plan.segment_range(rows, first, count, sample0, n_avail=n_avail)  # (the plan's window is on the device now)
    band = torch.full((3, 257), 7.0, dtype=torch.float64, device="cuda")
    stats = torch.full((3, 4), 7.0, dtype=torch.float64, device="cuda")
    pooled = torch.full((3, 257, 4), 7.0, dtype=torch.float32, device="cuda")
    scratch = torch.empty(1 << 24, dtype=torch.uint8, device="cuda")
    out = _lib.TfrOut(power_band=_lib.ptr(band), stats=_lib.ptr(stats), power_scale=1.0)

    def call(**kw):
        base = dict(n_total=x.shape[1], first_segment=first, segments=count, sample0=sample0, n_avail=n_avail,
                    row_stride=rows.stride(0), pool_factor=0)
        base.update(kw)
        rng = _lib.StftRange(**base)
        return lib.qi_stft_out_range(_lib.QI_F32, 0, _lib.ptr(rows), 3, _lib.ptr(plan.window), 512, 256, 512, plan.scale, C.byref(rng),
                                     C.byref(out), _lib.ptr(scratch), scratch.numel(), _lib.stream_ptr(x.device))

    for bad in (dict(sample0=sample0 + 1, n_avail=n_avail - 1), dict(n_avail=n_avail - 1),
                dict(first_segment=first + 2, pool_factor=4, pool_mean=_lib.ptr(pooled)), dict(first_segment=32, segments=13),
                dict(row_stride=n_avail - 1)):
        assert call(**bad) == -1, bad
        with pytest.raises(_lib.QiError):
            _lib.check(-1)
    torch.cuda.synchronize()
    assert bool((band == 7.0).all()) and bool((stats == 7.0).all()) and bool((pooled == 7.0).all())
    assert call() == 0  # the accepted call, for contrast
    torch.cuda.synchronize()
    assert bool((band != 7.0).all())
