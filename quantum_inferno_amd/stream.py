"""Long records as overlapped power-of-two chunks (BASELINE config 5: 24 h of 800 Hz infrasound = 69 120 000
samples per channel, 1024 channels, chunks of 2^20 with a hop of 2^19, float64).

A TFR of a chunk depends on that chunk only, so (channel block, chunk) pairs are independent work items like channels:
no exchange between them, and a run can restart at any item from its index alone (the only state a streaming run
carries).  The records stay on the HOST (a NumPy array or memmap: 1024 x 69.12 M float64 is 566 GB, twice an HBM);
`StreamPipeline` moves one item at a time through two pinned staging buffers and two device buffers: the host-to-device
copy of item k + 1 runs on a copy stream while item k is transformed, so PCIe (8 MB per record and chunk, ~0.2 ms) hides
behind the transforms (~6 ms per record and chunk in float64).  Only the REDUCED product of a chunk is kept -- no panel
is ever stored (coef=False): per-band power, per-time power, max / total / entropy sums.  Items are dealt to ranks by
`dist.shard` (one process per GPU, no data-path collective; the reduced products are gathered as in dist.py).

With hop < chunk the chunks overlap, so those per-chunk sums count most of the record twice, and no chunk product is a
picture of the record.  `StreamPipeline(pooled=factor)` closes both: every pooling window of `factor` samples of the
RECORD is owned by exactly one chunk (`owned_windows`), an item keeps the pooled power strips and the sums of the range
its chunk owns (`TfrPlan.pooled_strip`: the chunk's panel goes through a staging tensor on the device, tile by tile), and
`PooledRecord` puts the strips side by side and adds the sums up: a display-resolution panel, band powers and entropy of
the whole record.

The STFT streams by SEGMENT ranges instead (`segment_items`, `StftStream`, `StftRecord`; styx_fft.StftRangePlan): a segment
depends on its own samples only, so an item's coefficients are those of the one-call transform of the whole record, every
segment belongs to exactly one item, and the items' sums add up to the record's reductions with nothing counted twice."""
from dataclasses import dataclass
from typing import Iterator, List, Optional, Tuple

import numpy as np
import torch

from . import dist as qdist
from . import engine


def chunk_starts(n_total: int, chunk: int, hop: int) -> np.ndarray:
    """Start sample of every chunk: 0, hop, 2 hop, ... while a whole chunk fits, plus one last chunk flush with the
    end of the record when the tail is not covered (it overlaps its predecessor by more than chunk - hop)."""
    if n_total < chunk:
        raise ValueError(f"record of {n_total} samples is shorter than one chunk of {chunk}")
    if not 0 < hop <= chunk:
        raise ValueError("hop must be in (0, chunk]")
    starts = np.arange(0, n_total - chunk + 1, hop, dtype=np.int64)
    if starts[-1] + chunk < n_total:
        starts = np.append(starts, n_total - chunk)
    return starts


def owned_windows(n_total: int, chunk: int, hop: int, factor: int) -> Tuple[np.ndarray, np.ndarray]:
    """Which chunk owns which pooling windows of a record: -> (starts [K], edges [K + 1]), int64.  The windows are
    [w factor, (w + 1) factor) in record time for w < n_total // factor (the ragged tail is dropped, as subsample_2d drops
    it); chunk i (starting at starts[i] = chunk_starts(...)[i]) owns the samples [edges[i], edges[i + 1]): edges[0] = 0,
    edges[K] = (n_total // factor) factor, and between two chunks the edge is the middle of their overlap, rounded down
    to a window boundary -- the owned range stays away from the chunk ends, where a transform of the chunk differs most
    from one of the record.  Chunk i's first window is edges[i] // factor, its window count (edges[i + 1] - edges[i]) //
    factor, its offset inside the chunk edges[i] - starts[i] (any value: the last chunk is flush with the record end).
    ValueError when a window lies in no single chunk (hop == chunk with a factor that does not divide the hop, or an
    overlap shorter than about two windows)."""
    factor = int(factor)
    if factor < 2:
        raise ValueError(f"pooling factor {factor}: 2 or more")
    starts = chunk_starts(n_total, chunk, hop)
    k = len(starts)
    edges = np.empty(k + 1, dtype=np.int64)
    edges[0] = 0
    edges[k] = (n_total // factor) * factor
    mid = (starts[1:] + starts[:-1] + chunk) // 2
    edges[1:k] = (mid // factor) * factor
    # (mid <= n_total and mid <= starts[i - 1] + chunk: the edges rise and end inside the chunk before them)
    if np.any(edges[:k] < starts):
        raise ValueError(f"pooling factor {factor}: some window of {factor} samples lies in no single chunk of {chunk} samples "
                         f"(hop {hop}); the overlap chunk - hop must hold about two windows, or the factor divide the hop")
    return starts, edges


def iter_chunks(sig, chunk: int, hop: int, first_chunk: int = 0) -> Iterator[Tuple[int, int, torch.Tensor]]:
    """Yield (chunk index, start sample, view [channels, chunk]) from chunk `first_chunk` on (the restart cursor)."""
    t = sig if isinstance(sig, torch.Tensor) else torch.from_numpy(np.asarray(sig))
    if t.dim() == 1:
        t = t.unsqueeze(0)
    starts = chunk_starts(t.shape[-1], chunk, hop)
    for i in range(first_chunk, len(starts)):
        s = int(starts[i])
        yield i, s, t[:, s : s + chunk]


def work_items(n_channels: int, block: int, n_total: int, chunk: int, hop: int) -> List[Tuple[int, int, int, int]]:
    """Every (first channel, channel count, chunk index, start sample) of a [n_channels, n_total] record set, channel
    blocks of `block` records, block-major (a rank's contiguous share then walks whole blocks through their chunks)."""
    starts = chunk_starts(n_total, chunk, hop)
    items = []
    for c0 in range(0, n_channels, block):
        cb = min(block, n_channels - c0)
        for i, s in enumerate(starts):
            items.append((c0, cb, i, int(s)))
    return items


def rank_items(items, rank: int, world: int):
    """The contiguous share of `items` that `rank` of `world` owns (dist.shard)."""
    first, count = qdist.shard(len(items), rank, world)
    return items[first : first + count]


def stream_reduced(plan: engine.TfrPlan, sig, hop: int, which: str = "cwt", first_chunk: int = 0, power_scale=1.0):
    """Run `plan.cwt` / `plan.stx` over every chunk of a long [channels, n_total] record and keep only the reduced
    product per chunk (per-band power, max / total / entropy sums): yields (chunk index, start, TfrResult).  The
    yielded reduced product is a copy (a consumer may keep every item); no panel is stored."""
    fn = {"cwt": plan.cwt, "stx": plan.stx, "cwt_atoms": plan.cwt_atoms}[which]
    scratch = None
    for i, start, view in iter_chunks(sig, plan.n, hop, first_chunk):
        x = view.to(device=plan.device, dtype=plan.rdtype, non_blocking=True).contiguous()
        scratch = fn(x, coef=False, reductions=True, power_scale=power_scale, out=scratch)
        yield i, start, _copy_reduced(scratch)


def _copy_reduced(res: engine.TfrResult) -> engine.TfrResult:
    """A result that owns its reduced product (the buffers of `res` are written again by the next item)."""
    out = engine.TfrResult(frequency_hz=res.frequency_hz, power_scale=res.power_scale)
    out.reduced = res.reduced.clone()
    n_ch, n_b = res.power_band.shape
    o1 = out.reduced.numel() - n_ch * (n_b + 4)
    o2 = o1 + n_ch * n_b
    n = res.power_time.shape[1]
    out.power_time = out.reduced[:o1].view(res.power_time.dtype)[: n_ch * n].view(n_ch, n)
    out.power_band = out.reduced[o1:o2].view(n_ch, n_b)
    out.stats = out.reduced[o2:].view(n_ch, 4)
    return out


@dataclass
class StreamItem:
    index: int          # position in the item list (the restart cursor: pass index + 1 as `first_item`)
    first_channel: int
    channels: int
    chunk: int
    start: int          # first sample of the chunk
    cwt: Optional[engine.TfrResult]
    stx: Optional[engine.TfrResult]
    window0: Optional[int] = None  # pooled=factor: first pooling window of the record that this chunk owns ...
    windows: Optional[int] = None  # ... and how many (owned_windows)


class _Staging:
    """The double buffering of a streamed record set: two pinned host buffers and two device buffers [block, width], a copy
    stream and three events -- `stage(j, rows)` gathers one item's host rows into pinned buffer j and queues its copy to
    device buffer j on the copy stream; the consumer's stream waits for `copied[j]` before it reads device buffer j and
    records `consumed[j]` behind the last launch that does.  (StreamPipeline and StftStream.)"""

    def __init__(self, block, width, rdtype, device):
        np_dtype = np.float64 if rdtype == torch.float64 else np.float32
        self.gpu = torch.device(device).type == "cuda"
        self.pinned = [torch.empty((block, width), dtype=rdtype) for _ in range(2)]
        if self.gpu:
            self.pinned = [p.pin_memory() for p in self.pinned]
        self.pinned_np = [p.numpy() for p in self.pinned]
        assert self.pinned_np[0].dtype == np_dtype
        self.dev = [torch.empty((block, width), dtype=rdtype, device=device) for _ in range(2)]
        self.copy_stream = torch.cuda.Stream(device=device) if self.gpu else None
        # the device buffers come from the caching allocator of the current stream, which hands out a freed block at once:
        # work queued there before may still read or write that memory, so the copy stream's first writes wait for it
        self.allocated = torch.cuda.Event() if self.gpu else None
        if self.gpu:
            self.allocated.record(torch.cuda.current_stream(device))
        self.copied = [torch.cuda.Event() for _ in range(2)] if self.gpu else None    # H2D of buffer j done
        self.consumed = [torch.cuda.Event() for _ in range(2)] if self.gpu else None  # launches that read buffer j done
        self.used = [False, False]

    def stage(self, j, rows):
        """Host rows [cb, w] (w <= width: the first w samples of the buffers' rows) into pinned buffer j, then to device buffer j."""
        cb, w = rows.shape
        full = w == self.pinned[j].shape[1]
        pin_np = self.pinned_np[j][:cb] if full else self.pinned_np[j][:cb, :w]
        pin, dev = (self.pinned[j][:cb], self.dev[j][:cb]) if full else (self.pinned[j][:cb, :w], self.dev[j][:cb, :w])
        if not self.gpu:
            np.copyto(pin_np, rows, casting="same_kind")
            dev.copy_(pin)
            return
        if self.used[j]:
            self.copied[j].synchronize()  # the previous copy out of this pinned buffer has finished
        np.copyto(pin_np, rows, casting="same_kind")
        with torch.cuda.stream(self.copy_stream):
            if self.used[j]:
                self.copy_stream.wait_event(self.consumed[j])  # the launches that read device buffer j are done
            else:
                self.copy_stream.wait_event(self.allocated)  # what was queued where device buffer j was allocated is done
            if w > 0:
                dev.copy_(pin, non_blocking=True)
            self.copied[j].record(self.copy_stream)
        self.used[j] = True


def _merge_panels(mine, other):
    """What `other` filled where `mine` holds NaN (nobody added there), in place"""
    for m in mine:
        gap = torch.isnan(mine[m])
        mine[m][gap] = other[m].to(mine[m].device)[gap]


def _host_records(host_records):
    """The records of a stream as [channels, n_total]: an ndarray / memmap, or any object with a 2-D `shape` that answers
    [channel slice, sample slice] with an array (a rank of the 24 h job materialises only the records it owns)."""
    sig = host_records if hasattr(host_records, "shape") and hasattr(host_records, "__getitem__") else np.asarray(host_records)
    return sig[None, :] if len(sig.shape) == 1 else sig


def _pump(staging, items, host_rows, launch, device):
    """The double-buffered walk of `items` through `staging`: host_rows(item) are the host rows an item carries,
    launch(item, device buffer) queues its work on the current stream of `device` once the rows are there.  Yields (position,
    item, what launch returned) after the NEXT item has been staged: its host gather (a 134 MB memcpy at 16 float64 records of
    2^20 samples: milliseconds of host time) and its copy to the device run after this item's launches are queued, so they
    overlap its transforms even when the consumer waits for every item before asking for the next."""
    if not items:
        return
    compute = torch.cuda.current_stream(device) if staging.gpu else None
    staging.stage(0, host_rows(items[0]))
    for k, item in enumerate(items):
        j = k & 1
        if staging.gpu:
            compute.wait_event(staging.copied[j])
        out = launch(item, staging.dev[j])
        if staging.gpu:
            staging.consumed[j].record(compute)
        if k + 1 < len(items):
            staging.stage(j ^ 1, host_rows(items[k + 1]))
        yield k, item, out


class _RecordSums:
    """What the assemblers of a streamed record set share: power_band [n_channels, n_bands] and stats [n_channels, 4] float64
    added up over the items (sums added, maxima compared), the pooled strips side by side in `panel[method]` [n_channels,
    n_bands, n_windows] (NaN where nothing was added), and the frequency_hz / power_scale the items carry."""

    def __init__(self, n_channels, n_bands, n_windows, methods, dtype, device):
        self.methods = tuple(methods)
        self.panel = {m: torch.full((n_channels, n_bands, n_windows), float("nan"), dtype=dtype, device=device) for m in self.methods}
        self.power_band = torch.zeros((n_channels, n_bands), dtype=torch.float64, device=device)
        self.stats = torch.zeros((n_channels, 4), dtype=torch.float64, device=device)
        self.frequency_hz = None
        self.power_scale = 1.0

    def _add(self, item, res):
        """The strips and sums of one item's result `res`; -> the item's channel slice"""
        ch = slice(item.first_channel, item.first_channel + item.channels)
        for m in self.methods:
            self.panel[m][ch, :, item.window0 : item.window0 + item.windows] = res.pooled[m]
        self.power_band[ch] += res.power_band
        self.stats[ch, 1:3] += res.stats[:, 1:3]
        self.stats[ch, 0] = torch.maximum(self.stats[ch, 0], res.stats[:, 0])
        self.frequency_hz, self.power_scale = res.frequency_hz, res.power_scale
        return ch

    def _merge(self, other):
        """Another assembler of the same record set (the caller has compared the shapes) into this one"""
        _merge_panels(self.panel, other.panel)
        self.power_band += other.power_band
        self.stats[:, 1:3] += other.stats[:, 1:3]
        self.stats[:, 0] = torch.maximum(self.stats[:, 0], other.stats[:, 0])
        if self.frequency_hz is None:
            self.frequency_hz, self.power_scale = other.frequency_hz, other.power_scale
        return self


class PooledRecord(_RecordSums):
    """Assembles the items of a `StreamPipeline(pooled=factor)` run into the pooled panel and the reductions of the whole
    record set: `add(item, "cwt")` puts the item's strips at [first_channel : first_channel + channels, :, window0 :
    window0 + windows], adds its band powers, sum P and sum P log2 P, and keeps the larger maximum.  `panel[method]` is
    the [n_channels, n_bands, n_windows] panel (n_windows = n_total // factor), `result()` a TfrResult of the whole record
    (power_band, stats -> total_power, entropy_bits, power_per_band_bits()).  One assembler per transform.

    Strips carry their own position, so a rank that owns only some of the items fills only its part: the columns nobody
    added stay NaN and the sums hold what was added.  `merge(other)` combines the assemblers of several ranks: the columns
    that are NaN here are taken from the other, the sums added, the maxima compared (a record whose items were split between
    two ranks has its sums added in another order than one assembler would: equal up to rounding, and bit for bit where
    every record's items came from one rank)."""

    def __init__(self, n_channels, n_bands, n_windows, methods=("average",), dtype=torch.float32, device=None):
        super().__init__(n_channels, n_bands, n_windows, methods, dtype, device)

    def add(self, item: "StreamItem", which: str = "cwt"):
        res = {"cwt": item.cwt, "stx": item.stx}[which]
        if res is None or res.pooled is None or item.windows is None:
            raise ValueError(f"item {item.index} carries no pooled {which} strips (StreamPipeline(pooled=factor))")
        self._add(item, res)

    def merge(self, other: "PooledRecord"):
        if self.methods != other.methods or any(self.panel[m].shape != other.panel[m].shape for m in self.methods):
            raise ValueError("the assemblers are not of one record set: methods or panel shapes differ")
        return self._merge(other)

    def result(self) -> engine.TfrResult:
        return engine.TfrResult(frequency_hz=self.frequency_hz, power_band=self.power_band, stats=self.stats,
                                power_scale=self.power_scale, pooled=self.panel)


class StreamPipeline:
    """Double-buffered host -> device streaming of (channel block, chunk) items through a plan.

        plan = TfrPlan(1 << 20, torch.float64, ...); plan.set_styx_bank(12, 800.0); plan.set_stx_bands(12, 800.0)
        pipe = StreamPipeline(plan, host_records, hop=1 << 19, block=16, transforms=("cwt", "stx"))
        for item in pipe.run(rank=r, world=w):          # item.cwt.power_band [channels, bands], .entropy_bits, ...
            ...

    `host_records`: NumPy array / memmap [channels, n_total] (any real dtype; converted to the plan's on the way into
    the pinned buffer).  Every yielded item owns its reduced products.  keep_time=False: the per-time power of a chunk
    (8 MB per record in float64) is neither kept nor computed (`reductions="band"`: band powers, maximum, total, entropy).

    pooled=factor: every item keeps, per transform, what the range its chunk OWNS contributes to the record (owned_windows;
    a ValueError of that rule is raised here): `item.cwt.pooled[method]` [channels, bands, item.windows], the strips of the
    record's pooled power panel from window `item.window0` on (pooled_methods out of "average", "max"), and `power_band` /
    `stats` over the owned range only, so that they add up over the items of a record (`PooledRecord`); `power_time` is
    None.  Each transform then stores its panel in the plan's staging tensor, tile by tile (TfrPlan.pooled_strip)."""

    def __init__(self, plan: engine.TfrPlan, host_records, hop: int, block: int = 16, transforms=("cwt", "stx"),
                 power_scale: float = 1.0, keep_time: bool = True, pooled: Optional[int] = None, pooled_methods=("average",)):
        self.plan, self.hop, self.block = plan, int(hop), int(block)
        self.pooled, self.pooled_methods = (None if pooled is None else int(pooled)), tuple(pooled_methods)
        self.sig = _host_records(host_records)
        self.transforms = tuple(transforms)
        for t in self.transforms:
            if t not in ("cwt", "stx"):
                raise ValueError(f"unknown transform {t!r}: 'cwt' and / or 'stx'")
        self.power_scale, self.keep_time = power_scale, keep_time
        # (no per-time power kept: it is not computed either -- no per-time planes written or summed, round 5)
        self._reductions = True if keep_time else "band"
        self.items = work_items(self.sig.shape[0], self.block, self.sig.shape[1], plan.n, self.hop)
        if self.pooled is not None:
            engine.check_pooled_methods(self.pooled_methods)
            self._starts, self._edges = owned_windows(self.sig.shape[1], plan.n, self.hop, self.pooled)
        # (a plan on the CPU exists only as the stand-in of bench.py --stub: the item walk without streams or pinning)
        self._staging = _Staging(self.block, plan.n, plan.rdtype, plan.device)
        self._out = {}  # (transform, channels) -> result buffers reused item after item

    def _launch(self, item, dev):
        """The transforms of one item on its rows in device buffer `dev`: -> ({transform: result}, window0, windows)"""
        _, cb, chunk, s = item
        x = dev[:cb]
        res = {}
        if self.pooled is not None:
            e0, e1 = int(self._edges[chunk]), int(self._edges[chunk + 1])
            w0, nw = e0 // self.pooled, (e1 - e0) // self.pooled
            for t in self.transforms:
                which = engine._lib.QI_BANK_STYX if t == "cwt" else engine._lib.QI_TABLE_STX
                strips, band, stats = self.plan.pooled_strip(which, x, self.pooled, e0 - s, nw, self.pooled_methods, self.power_scale)
                res[t] = engine.TfrResult(frequency_hz=self.plan.freq[which], power_band=band, stats=stats,
                                          power_scale=self.power_scale, pooled=strips)
            return res, w0, nw
        if self.transforms == ("cwt", "stx"):
            key = ("both", cb)
            self._out[key] = self.plan.cwt_stx(x, coef=False, reductions=self._reductions, power_scale=self.power_scale,
                                               out=self._out.get(key))
            res["cwt"], res["stx"] = self._out[key]
        else:
            for t in self.transforms:
                key = (t, cb)
                fn = self.plan.cwt if t == "cwt" else self.plan.stx
                self._out[key] = fn(x, coef=False, reductions=self._reductions, power_scale=self.power_scale, out=self._out.get(key))
                res[t] = self._out[key]
        return res, None, None

    def run(self, rank: int = 0, world: int = 1, first_item: int = 0) -> Iterator[StreamItem]:
        mine = rank_items(self.items, rank, world)[first_item:]
        rows = lambda item: self.sig[item[0] : item[0] + item[1], item[3] : item[3] + self.plan.n]
        for k, (c0, cb, chunk, s), (res, w0, nw) in _pump(self._staging, mine, rows, self._launch, self.plan.device):
            if self.pooled is None:  # (pooled_strip's outputs are new tensors: the item owns them; these are the plan's buffers)
                res = {t: self._keep(r) for t, r in res.items()}
            yield StreamItem(first_item + k, c0, cb, chunk, s, res.get("cwt"), res.get("stx"), w0, nw)

    def _keep(self, res):
        if self.keep_time:
            return _copy_reduced(res)
        small = engine.TfrResult(frequency_hz=res.frequency_hz, power_scale=res.power_scale)
        small.power_band, small.stats = res.power_band.clone(), res.stats.clone()
        return small


# ---- the streamed STFT: items own SEGMENT ranges ------------------------------------------------------------------------------
def segment_items(n_total: int, seg: int, hop: int, segments_per_item: int) -> List[Tuple[int, int, int, int]]:
    """The segments of a record's STFT (scipy.signal.stft, boundary="zeros", padded=True: styx_fft) as consecutive runs of
    `segments_per_item`: -> [(first_segment, segments, sample0, n_avail)].  Every segment lies in exactly one item; an item
    carries the smallest interval of record samples its segments need (styx_fft.range_samples: neighbouring items overlap by
    seg - hop samples; n_avail = 0 where a last padded segment lies in the zero extension).  Host arithmetic only."""
    from .styx_fft import _frame_count, range_samples

    per = int(segments_per_item)
    if per < 1:
        raise ValueError(f"segments_per_item {segments_per_item}: 1 or more")
    n_seg = _frame_count(int(n_total), int(seg), int(hop))
    if n_seg < 1:
        raise ValueError(f"no STFT segments for n = {n_total}, segment {seg}, hop {hop}")
    items = []
    for first in range(0, n_seg, per):
        count = min(per, n_seg - first)
        items.append((first, count) + range_samples(int(n_total), int(seg), int(hop), first, count))
    return items


@dataclass
class StftItem:
    index: int          # position in the item list (the restart cursor: pass index + 1 as `first_item`)
    first_channel: int
    channels: int
    first_segment: int
    segments: int
    sample0: int        # first record sample the item carried ...
    n_avail: int        # ... and how many
    stft: engine.TfrResult  # of the range: power_band / stats over its segments, power_time [channels, segments], pooled strips
    window0: Optional[int] = None  # pooled=factor: first pooling window of the record in `stft.pooled` ...
    windows: Optional[int] = None  # ... and how many


class StftStream:
    """Double-buffered host -> device streaming of (channel block, segment range) items through a styx_fft.StftRangePlan.

        plan = styx_fft.StftRangePlan(n_total, 800.0, 12)
        pipe = StftStream(plan, host_records, segments_per_item=4096, block=16, pooled=64, pooled_methods=("average", "max"))
        record = StftRecord(channels, plan.n_f, plan.n_seg, pooled=64, methods=("average", "max"), dtype=plan.rdtype, device="cuda")
        for item in pipe.run(rank=r, world=w):
            record.add(item)

    `host_records` as StreamPipeline takes them.  An STFT segment depends on its own samples only, so -- unlike a chunk of the
    CWT -- the items' coefficients are those of the one-call transform of the whole record, and their sums add up to its
    reductions in another order of summation.  Every yielded item owns its products; no panel is stored.  keep_time=False:
    no per-time power.  pooled=factor: `item.stft.pooled[method]` [channels, n_f, item.windows], the record's pooled
    spectrogram from window item.window0 on; segments_per_item must be a multiple of the factor."""

    def __init__(self, stft_plan, host_records, segments_per_item: int, block: int = 16, pooled: Optional[int] = None,
                 pooled_methods=("average",), keep_time: bool = True, power_scale: float = 1.0, device=None):
        self.plan, self.block, self.per = stft_plan, int(block), int(segments_per_item)
        self.pooled, self.pooled_methods = (None if pooled is None else int(pooled)), tuple(pooled_methods)
        self.keep_time, self.power_scale = keep_time, power_scale
        self.sig = _host_records(host_records)
        if self.sig.shape[1] != stft_plan.n_total:
            raise ValueError(f"records of {self.sig.shape[1]} samples, the plan is for {stft_plan.n_total}")
        if self.block < 1:
            raise ValueError(f"block {block}: 1 or more")
        self.ranges = segment_items(stft_plan.n_total, stft_plan.seg, stft_plan.hop, self.per)
        if self.pooled is not None:
            engine.check_pooled_methods(self.pooled_methods)
            if self.pooled < 2:
                raise ValueError(f"pooling factor {self.pooled}: 2 or more")
            if self.per % self.pooled:
                raise ValueError(f"segments_per_item {self.per} is no multiple of the pooling factor {self.pooled}")
        n_ch = self.sig.shape[0]
        # block-major, as work_items: a rank's contiguous share walks whole blocks through their ranges
        self.items = [(c0, min(self.block, n_ch - c0)) + r for c0 in range(0, n_ch, self.block) for r in self.ranges]
        self.device = torch.device(device) if device is not None else engine.default_device()
        self._width = max(1, max(r[3] for r in self.ranges))
        self._staging = None  # (the pinned and device buffers are made by the first run)

    def _launch(self, item, dev):
        _, cb, first, count, s0, n_avail = item
        return self.plan.segment_range(dev[:cb], first, count, s0, reductions=True if self.keep_time else "band", pooled=self.pooled,
                                       pooled_methods=self.pooled_methods, power_scale=self.power_scale, n_avail=n_avail)

    def run(self, rank: int = 0, world: int = 1, first_item: int = 0) -> Iterator[StftItem]:
        mine = rank_items(self.items, rank, world)[first_item:]
        if mine and self._staging is None:
            self._staging = _Staging(self.block, self._width, self.plan.rdtype, self.device)
        rows = lambda item: self.sig[item[0] : item[0] + item[1], item[4] : item[4] + item[5]]
        for k, (c0, cb, first, count, s0, n_avail), res in _pump(self._staging, mine, rows, self._launch, self.device):
            w0, nw = (None, None) if self.pooled is None else (first // self.pooled, count // self.pooled)
            yield StftItem(first_item + k, c0, cb, first, count, s0, n_avail, res, w0, nw)  # (segment_range's outputs are new tensors)


class StftRecord(_RecordSums):
    """Assembles the items of an `StftStream` run into the products of the whole record set: `add(item)` puts the item's
    pooled strips at [channels, :, window0 : window0 + windows] and its per-time power at [channels, first_segment :
    first_segment + segments], adds its band powers, sum P and sum P log2 P, and keeps the larger maximum (PooledRecord's
    rules).  `panel[method]` is [n_channels, n_f, n_segments // pooled], `power_time` [n_channels, n_segments] (keep_time),
    both NaN where nothing was added; `result()` a TfrResult of the whole record (total_power, entropy_bits,
    power_per_band_bits()).  `merge(other)` combines the assemblers of several ranks as PooledRecord.merge does."""

    def __init__(self, n_channels, n_f, n_segments, pooled=None, methods=("average",), keep_time=True, dtype=torch.float32,
                 device=None):
        self.pooled = None if pooled is None else int(pooled)
        super().__init__(n_channels, n_f, 0 if pooled is None else n_segments // self.pooled, methods if pooled is not None else (),
                         dtype, device)
        self.power_time = torch.full((n_channels, n_segments), float("nan"), dtype=dtype, device=device) if keep_time else None

    def add(self, item: "StftItem"):
        res = item.stft
        if res is None or res.power_band is None:
            raise ValueError(f"item {item.index} carries no reductions")
        if self.methods and (res.pooled is None or item.windows is None):
            raise ValueError(f"item {item.index} carries no pooled strips (StftStream(pooled=factor))")
        if self.power_time is not None and res.power_time is None:
            raise ValueError(f"item {item.index} carries no per-time power (StftStream(keep_time=True))")
        ch = self._add(item, res)
        if self.power_time is not None:
            self.power_time[ch, item.first_segment : item.first_segment + item.segments] = res.power_time

    def merge(self, other: "StftRecord"):
        if (self.methods != other.methods or self.power_band.shape != other.power_band.shape
                or any(self.panel[m].shape != other.panel[m].shape for m in self.methods)
                or (self.power_time is None) != (other.power_time is None)
                or (self.power_time is not None and self.power_time.shape != other.power_time.shape)):
            raise ValueError("the assemblers are not of one record set: methods or shapes differ")
        if self.power_time is not None:
            _merge_panels({"t": self.power_time}, {"t": other.power_time})
        return self._merge(other)

    def result(self) -> engine.TfrResult:
        return engine.TfrResult(frequency_hz=self.frequency_hz, power_band=self.power_band, power_time=self.power_time,
                                stats=self.stats, power_scale=self.power_scale, pooled=self.panel if self.methods else None)
