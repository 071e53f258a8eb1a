"""Device time of the scaling and peak picking (qi_find_peaks): 1, 64 and 1024 records of 2^20 samples, float32 and
float64, "sigmax" with height 0.7 on band-limited noise (white noise through a 16-sample moving average, made on the
device), timed with device events after warm-up, median of 20 calls.  Per call: the time, the bytes the design has to
move through HBM over the time against the 8 TB/s peak -- four reads of the record (extrema; tile summaries; count;
store: two more than the two any picker needs, one for the divisor and one to pick) plus the per-tile scratch and the
positions, values and counts -- and the candidates found.  Beside it the PyTorch composition on the same records: amax, a
divide, two shifted comparisons and nonzero; it sees strict maxima only -- no plateaus, so it is not the same function -- and
returns one index list for the whole batch.  SciPy's find_peaks on this host, where SciPy is importable (4 records).

    python tools/peaks_bench.py [--out profiles/peaks_kernel.txt] [--records 1 64 1024] [--log2n 20] [--reps 20]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from quantum_inferno_amd import _lib  # noqa: E402

HBM_PEAK = 8.0e12  # bytes per second
HEIGHT = 0.7
SMOOTH = 16


def band_limited(records, n, tdtype, dev):
    gen = torch.Generator(device=dev).manual_seed(records)
    x = torch.randn((records, n + SMOOTH - 1), dtype=tdtype, device=dev, generator=gen)
    return torch.nn.functional.avg_pool1d(x[:, None, :], SMOOTH, stride=1)[:, 0, :].contiguous()


def scipy_ms(x_host):
    try:
        import scipy.signal as signal
    except ImportError:
        return None
    t0 = time.perf_counter()
    for row in x_host:
        signal.find_peaks(row / np.nanmax(row), height=HEIGHT)
    return (time.perf_counter() - t0) * 1e3 / len(x_host)


def timed(call, dev, warmup, reps):
    for _ in range(warmup):
        call()
    torch.cuda.synchronize(dev)
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--records", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    lib = _lib.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    n = 1 << args.log2n
    tiles = -(-n // _lib.PEAKS_TILE)
    lines = [f"qi_find_peaks, sigmax, height {HEIGHT}, records of 2^{args.log2n} samples of band-limited noise ({SMOOTH}-sample moving "
             f"average), {torch.cuda.get_device_name(dev)}; device events, median (min .. max) of {args.reps} calls after {args.warmup}"]
    for tdtype, code in ((torch.float32, _lib.QI_F32), (torch.float64, _lib.QI_F64)):
        size = torch.empty(0, dtype=tdtype).element_size()
        host = None
        for records in args.records:
            x = band_limited(records, n, tdtype, dev)
            if host is None:
                host = scipy_ms(x[:4].cpu().numpy())
                lines.append(f"{str(tdtype).split('.')[-1]}: " + ("SciPy not importable on this host" if host is None else
                                                                   f"SciPy find_peaks on this host, one core: {host:.2f} ms per record"))
            cap = 4096  # columns per record: the picks above the height are a few hundred; the counts say if more were found
            positions = torch.empty((records, cap), dtype=torch.int64, device=dev)
            values = torch.empty((records, cap), dtype=torch.float64, device=dev)
            counts = torch.zeros((records,), dtype=torch.int64, device=dev)
            nbytes = int(lib.qi_peaks_scratch_bytes(code, records, n))
            scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)

            def native():
                _lib.check(lib.qi_find_peaks(code, dev.index, _lib.ptr(x), records, n, _lib.QI_PEAK_SIGMAX, 0.0, _lib.QI_PEAK_HEIGHT_ABS,
                                             HEIGHT, None, _lib.ptr(positions), _lib.ptr(values), cap, _lib.ptr(counts), _lib.ptr(scratch),
                                             nbytes, _lib.stream_ptr(dev)))

            med, lo, hi = timed(native, dev, args.warmup, args.reps)
            found = counts.cpu().numpy()
            stored = int(np.minimum(found, cap).sum())
            # four reads of the record; per tile 5 doubles written and read, 3 written (read only behind a plateau), the count
            # written, scanned in place and read; the stored peaks; the counts
            moved = records * (4.0 * n * size + tiles * 8.0 * (5 + 5 + 3 + 1 + 2 + 1) + 8.0) + stored * 16.0
            line = (f"  {records:5d} records, qi_find_peaks: {med:9.3f} ms ({lo:.3f} .. {hi:.3f}) per call | {moved / 1e9:7.3f} GB required = "
                    f"{moved / (med * 1e-3) / 1e9:8.1f} GB/s = {100.0 * moved / (med * 1e-3) / HBM_PEAK:6.2f} % of the 8 TB/s peak | "
                    f"{int(found.sum())} candidates ({found.min()} .. {found.max()} per record, {cap} columns)")
            if host is not None:
                line += f" | {host * records / med:7.1f} x the host's {host * records:.0f} ms"
            lines.append(line)
            print(line, flush=True)

            def composed():
                s = x / x.amax(dim=1, keepdim=True)
                mid = s[:, 1:-1]
                return torch.nonzero((mid > s[:, :-2]) & (mid > s[:, 2:]) & (mid >= HEIGHT))

            cmed, clo, chi = timed(composed, dev, args.warmup, args.reps)
            strict = int(composed().shape[0])
            line = (f"  {records:5d} records, PyTorch amax / divide / shifted comparisons / nonzero (strict maxima only, no plateaus; "
                    f"nonzero synchronises): {cmed:9.3f} ms ({clo:.3f} .. {chi:.3f}) per call, {strict} picks | native / composed = "
                    f"{med / cmed:.3f}")
            lines.append(line)
            print(line, flush=True)
            del x, positions, values, scratch
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
