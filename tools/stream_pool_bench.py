#!/usr/bin/env python3
"""Time the strip kernel of a streamed record (qi_pool_strip) and what pooled streaming costs per item, on an MI355X.

    python tools/stream_pool_bench.py [--out profiles/stream_pool.txt] [--reps 15] [--items 5] [--part kernel|pipeline|all]

Kernel A/B, same process, same panel: a [167, 2^20] complex panel, owned range the middle 2^19 columns, factors 256 and
4096.  New path: ONE qi_pool_strip launch on the panel that writes the averages, the maxima and the per-row sums of the
range.  Old path: what the library could do before on a range that is already contiguous -- two qi_pool_panel launches
(average, max) in QI_POOL_POWER mode on a contiguous copy of the range; the copy and the sums (which the old path cannot
produce) are not counted, which favours the old path.  The two alternate call by call; each call is timed by a pair of
events after three warm-up calls of each; the median of the repeats is reported with the lowest and the highest.  GB/s
are the bytes the strip kernel has to move (the range read once, the outputs written once) over its time.  The one launch
must not be slower than the two: the tool exits with an error if it is.  The strip kernel is also timed without the sums
(no logarithm) and with the sums alone.

Pipeline cost: BASELINE configs[4]'s item (16 float64 records of 2^20 samples, hop 2^19, order 12, 800 Hz, CWT +
Stockwell), `--items` timed items after two warm-up items: StreamPipeline(pooled=4096) against the default pipeline
(keep_time=False), host clock around the item loop; and its split, timed by events on one item's records: the transforms
with a stored panel (the tile loop alone), the strip kernel (pooled_strip minus that), the rest (pipeline minus
pooled_strip)."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from quantum_inferno_amd import _lib, engine, scales_dyadic, stream  # noqa: E402
from quantum_inferno_amd.utilities import sampling  # noqa: E402

ROWS, N, FIRST, SPAN = 167, 1 << 20, 1 << 18, 1 << 19
FACTORS = (256, 4096)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def med(ts):
    return f"{statistics.median(ts):8.3f} ms ({min(ts):.3f} .. {max(ts):.3f})"


def kernel_ab(reps, lines):
    lib = _lib.load()
    slower = []
    for cdt in (torch.complex64, torch.complex128):
        rdt = torch.float32 if cdt == torch.complex64 else torch.float64
        code = _lib.QI_F32 if rdt == torch.float32 else _lib.QI_F64
        g = torch.Generator(device="cuda").manual_seed(7)
        z = torch.view_as_complex(torch.randn((ROWS, N, 2), generator=g, dtype=rdt, device="cuda"))
        own = z[:, FIRST : FIRST + SPAN].contiguous()
        for f in FACTORS:
            w = SPAN // f
            mean = torch.empty((ROWS, w), dtype=rdt, device="cuda")
            peak = torch.empty((ROWS, w), dtype=rdt, device="cuda")
            sums = torch.empty((ROWS, 3), dtype=torch.float64, device="cuda")
            st = _lib.stream_ptr(z.device)

            def strip(m=mean, p=peak, s=sums):
                _lib.check(lib.qi_pool_strip(code, 0, _lib.ptr(z), ROWS, N, FIRST, f, w, 1.0, _lib.ptr(m), _lib.ptr(p), w, _lib.ptr(s), st))

            def two():
                return (sampling.pool_rows(own, f, "average", _lib.QI_POOL_POWER, 1.0),
                        sampling.pool_rows(own, f, "max", _lib.QI_POOL_POWER, 1.0))

            variants = {"all": strip, "no sums": lambda: strip(s=None), "sums only": lambda: strip(m=None, p=None)}
            for _ in range(3):
                for fn in variants.values():
                    fn()
                a, b = two()
            strip()
            torch.cuda.synchronize()
            assert torch.equal(peak, b), "the two paths disagree on the maxima"
            err = float((mean.double() - a.double()).abs().max() / b.double().max())
            ts = {k: [] for k in variants}
            t2 = []
            for _ in range(reps):
                for k, fn in variants.items():
                    ts[k].append(timed(fn)[0])
                t2.append(timed(two)[0])
            nbytes = ROWS * SPAN * z.element_size() + 2 * mean.numel() * mean.element_size() + sums.numel() * 8
            mk, mo = statistics.median(ts["all"]), statistics.median(t2)
            lines.append(f"[{ROWS}, 2^20] {str(cdt)[6:]}, columns 2^18 .. 2^18 + 2^19, factor {f}: qi_pool_strip (average + max + sums, one launch) "
                         f"{med(ts['all'])} = {nbytes / mk / 1e6:6.0f} GB/s of required bytes | two qi_pool_panel launches on the contiguous range "
                         f"{med(t2)} | ratio {mo / mk:.2f} | averages differ by {err:.1e} of the maximum")
            lines.append(f"    qi_pool_strip without the sums {med(ts['no sums'])}; the sums alone {med(ts['sums only'])}")
            if mk > mo:
                slower.append(lines[-2])
        del z, own
        torch.cuda.empty_cache()
    return slower


def pipeline_cost(items, lines):
    n, hop, fs, order, n_ch, factor = 1 << 20, 1 << 19, 800.0, 12, 16, 4096
    n_b = len(scales_dyadic.log_frequency_hz_from_fft_points(fs, n, order))
    warm = 2
    total = n + (warm + items - 1) * hop
    rng = np.random.default_rng(5)
    host = rng.standard_normal((n_ch, total))
    plan = engine.TfrPlan(n, torch.float64, "cuda:0", engine.TfrPlan.workspace_for(n, n_b, torch.float64, n_ch, cap_bytes=32 << 30))
    plan.set_styx_bank(order, fs)
    plan.set_stx_bands(order, fs)

    def per_item(**kw):
        it = stream.StreamPipeline(plan, host, hop, block=n_ch, keep_time=False, **kw).run()
        for _ in range(warm):
            next(it)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        done = 0
        for item in it:
            float(item.cwt.stats[0, 1])  # (touch the result: the item is complete)
            done += 1
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / done, done

    base, done = per_item()
    pooled, _ = per_item(pooled=factor, pooled_methods=("average", "max"))
    x = torch.from_numpy(host[:, hop : hop + n]).cuda()
    first, windows = hop // 2, hop // factor
    both = (_lib.QI_BANK_STYX, _lib.QI_TABLE_STX)

    def strips():
        for which in both:
            plan.pooled_strip(which, x, factor, first, windows, ("average", "max"))

    def panels():
        for which in both:
            for _ in plan._staged_panels(which, plan._signal(x), True, 1.0, 0.0, 1 << 30):
                pass

    for _ in range(2):
        strips()
        panels()
    ts, tp = [], []
    for _ in range(items):
        ts.append(timed(strips)[0])
        tp.append(timed(panels)[0])
    ms, mp = statistics.median(ts), statistics.median(tp)
    lines.append(f"StreamPipeline, {n_ch} float64 records x 2^20, hop 2^19, order {order} ({n_b} bands), CWT + Stockwell, {done} timed items: "
                 f"default (no panel stored) {base:.1f} ms per item | pooled={factor}, average + max {pooled:.1f} ms per item ({pooled / base:.2f} x)")
    lines.append(f"    split of the pooled item: transforms with a stored panel, one record per tile {mp:.1f} ms | strip kernel "
                 f"{ms - mp:.1f} ms ({2 * n_ch} launches on [{n_b}, 2^20] complex128, {windows} windows from column {first}) | rest "
                 f"(host gather, copy, result tensors) {pooled - ms:.1f} ms")
    plan.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "stream_pool.txt"))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--items", type=int, default=5)
    ap.add_argument("--part", choices=("kernel", "pipeline", "all"), default="all")
    a = ap.parse_args()
    _lib.require_gpu()
    lines = [f"pooled strips of a streamed record, {torch.cuda.get_device_name(0)}; median (min .. max) of {a.reps} calls, the paths alternating"]
    slower = []
    if a.part in ("kernel", "all"):
        slower = kernel_ab(a.reps, lines)
    if a.part in ("pipeline", "all"):
        pipeline_cost(a.items, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)
    if slower:
        sys.exit("qi_pool_strip is slower than two qi_pool_panel launches:\n" + "\n".join(slower))


if __name__ == "__main__":
    main()
