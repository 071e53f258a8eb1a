#!/usr/bin/env python3
"""Time the streamed STFT on an MI355X: a float32 record set in stft_from_sig's geometry (order 12 at 800 Hz) that stays on
the host and goes through stream.StftStream item by item.

    (stream)  StftStream.run over the whole record set: host clock from the first stage to the synchronise behind the last
              item, per item; pooled strips (average and maximum) and the reductions, no panel
    (kernels) the same item's device work alone: StftRangePlan.segment_range on rows that are already on the device, a pair
              of events around each call -- the share of (stream) that is NOT this is the time outside the kernels (host
              gather, copy, launches, allocation of the item's outputs)
    (floor)   the same record set resident on the device through StftPlan.reduce (reductions only, no pooling, no panel),
              per item's worth of segments
    (pooled)  one item's pooled spectrogram from the kernel's partial sums (segment_range, no coef buffer) against the
              composition the library had before: qi_stft_out with coef, then qi_pool_strip on the panel -- alternating

    python tools/stft_stream_bench.py [--out profiles/stft_stream.txt] [--reps 15] [--channels 16] [--items 4]

Three warm-up passes of each form; medians with the lowest and highest.  Nothing is asserted about the times."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from quantum_inferno_amd import _lib, stream, styx_fft  # noqa: E402

FS, ORDER, PER_ITEM, FACTOR, BLOCK = 800.0, 12, 1024, 64, 16
METHODS = ("average", "max")


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def med(ts):
    return f"{statistics.median(ts):.3f} ({min(ts):.3f} .. {max(ts):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "stft_stream.txt"))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--channels", type=int, default=16)
    ap.add_argument("--items", type=int, default=4, help="segment ranges per record (each of 1024 segments)")
    a = ap.parse_args()
    lib = _lib.require_gpu()
    hop = styx_fft.stft_segment_points(FS, ORDER) // 2
    channels, n = a.channels, (a.items * PER_ITEM - 1) * hop  # a.items x PER_ITEM segments exactly
    host = np.random.default_rng(7).standard_normal((channels, n)).astype(np.float32)
    plan = styx_fft.StftRangePlan(n, FS, ORDER, dtype=torch.float32)
    pipe = stream.StftStream(plan, host, PER_ITEM, block=BLOCK, pooled=FACTOR, pooled_methods=METHODS, device="cuda")
    n_items = len(pipe.items)
    lines = [f"streamed STFT, {torch.cuda.get_device_name(0)}: [{channels}, {n}] float32 on the host, order {ORDER} at {FS:g} Hz "
             f"(segments of {plan.seg}, hop {plan.hop}, {plan.n_seg} segments, {plan.n_f} bins); items of {BLOCK} records x {PER_ITEM} "
             f"segments ({n_items} items, the widest carries {pipe._width} samples per record); pooling factor {FACTOR}, average and "
             f"maximum; ms, median (min .. max) of {a.reps}"]

    # (stream) the whole run, per item
    def run_stream():
        rec = stream.StftRecord(channels, plan.n_f, plan.n_seg, pooled=FACTOR, methods=METHODS, dtype=torch.float32, device="cuda")
        t0 = time.perf_counter()
        for item in pipe.run():
            rec.add(item)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n_items, rec

    for _ in range(3):
        run_stream()
    per_item = [run_stream()[0] for _ in range(a.reps)]

    # (kernels) a full item's device work alone
    c0, cb, first, count, s0, n_avail = pipe.items[min(1, n_items - 1)]
    rows = torch.from_numpy(host[c0 : c0 + cb, s0 : s0 + n_avail]).cuda()
    call = lambda: plan.segment_range(rows, first, count, s0, pooled=FACTOR, pooled_methods=METHODS, n_avail=n_avail)
    for _ in range(3):
        call()
    kernels = [timed(call)[0] for _ in range(a.reps)]

    # (floor) the record set resident on the device, StftPlan.reduce
    whole = styx_fft.StftPlan(n, channels, FS, ORDER, torch.float32)
    x = torch.from_numpy(host).cuda()
    for _ in range(3):
        whole.reduce(x)
    floor = [timed(lambda: whole.reduce(x))[0] / n_items for _ in range(a.reps)]
    del whole
    torch.cuda.empty_cache()

    lines.append(f"  (stream)  per item, host clock over the whole run      {med(per_item)}")
    lines.append(f"  (kernels) one item's segment_range on device rows      {med(kernels)}")
    share = 1.0 - statistics.median(kernels) / statistics.median(per_item)
    lines.append(f"            share of an item's time outside the kernels   {100 * share:.1f} %")
    lines.append(f"  (floor)   StftPlan.reduce on the resident set, per item {med(floor)}   (stream / floor = "
                 f"{statistics.median(per_item) / statistics.median(floor):.2f})")

    # (pooled) from the kernel's partials, against qi_stft_out with coef followed by qi_pool_strip
    n3 = (PER_ITEM - 1) * plan.hop
    x3 = torch.from_numpy(host[:BLOCK, :n3]).cuda()
    cb3 = x3.shape[0]
    new_plan = styx_fft.StftRangePlan(n3, FS, ORDER, dtype=torch.float32)
    old_plan = styx_fft.StftPlan(n3, cb3, FS, ORDER, torch.float32)
    assert new_plan.n_seg == old_plan.n_seg == PER_ITEM
    windows = PER_ITEM // FACTOR
    mean = torch.empty((cb3, plan.n_f, windows), dtype=torch.float32, device="cuda")
    peak = torch.empty_like(mean)

    def new():
        return new_plan.segment_range(x3, 0, PER_ITEM, 0, pooled=FACTOR, pooled_methods=METHODS)

    def old():
        res = old_plan.reduce(x3, coef=True)
        with torch.cuda.device(0):
            _lib.check(lib.qi_pool_strip(old_plan.code, 0, _lib.ptr(res.coef), cb3 * plan.n_f, PER_ITEM, 0, FACTOR, windows, 1.0,
                                         _lib.ptr(mean), _lib.ptr(peak), windows, None, _lib.stream_ptr(x3.device)))
        return res

    for _ in range(3):
        got, _ = new(), old()
    torch.cuda.synchronize()
    err = float((got.pooled["average"] - mean).abs().max() / mean.abs().max())
    ts = {"new": [], "old": []}
    for _ in range(a.reps):
        ts["new"].append(timed(new)[0])
        ts["old"].append(timed(old)[0])
    lines.append(f"  (pooled)  one item [{cb3}, {n3}] -> [{cb3}, {plan.n_f}, {windows}] average and maximum with the reductions:")
    lines.append(f"            from the kernel's partial sums, no panel         {med(ts['new'])}")
    lines.append(f"            qi_stft_out with coef, then qi_pool_strip        {med(ts['old'])}   (old / new = "
                 f"{statistics.median(ts['old']) / statistics.median(ts['new']):.2f}; largest difference of the averages "
                 f"{err:.1e} of their maximum)")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
