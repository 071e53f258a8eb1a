"""Device time of the resamplers.  qi_interp_grid: 1, 64 and 1024 records of 2^20 knots at a mean 800 Hz whose steps are
jittered by +-30 % (shared timestamps), onto grids at 1, 4 and 1/4 times that rate, float32 and float64 values, timed with
device events after warm-up, median of 20 calls.  Per call: the time and the bytes any interpolator has to move through
HBM, n (8 + sizeof T) + 8 m per record (the shared timestamps counted once per record, as each record's workgroups read
them), over the time against the 8 TB/s peak.  Beside it, in the same job, the PyTorch composition on the device
(torch.searchsorted on the grid, two gathers each of knots and values, the arithmetic of np.interp without its NaN
branches) and np.interp on one core of this host (one record).  qi_resample_fft: 2^20 -> 2^19 and 2^20 -> 3 * 2^18 samples
against torch.fft.rfft / slice or pad / torch.fft.irfft.

    python tools/resample_bench.py [--out profiles/resample_kernel.txt] [--records 1 64 1024] [--log2n 20] [--reps 20]"""
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
FS = 800.0
RATES = (("x 1", 1.0), ("x 4", 4.0), ("x 1/4", 0.25))


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


def grid(first, last, rate):
    step = 1.0 / rate
    return first, (first + step) - first, max(int(np.ceil((last - first) / step)), 0)


def interp_part(lib, dev, args, lines):
    n = 1 << args.log2n
    rng = np.random.default_rng(20)
    ts_host = np.concatenate([[0.0], np.cumsum((1.0 + 0.3 * rng.uniform(-1.0, 1.0, n - 1)) / FS)])
    ts = torch.from_numpy(ts_host).to(dev)
    for tdtype, code in ((torch.float32, _lib.QI_F32), (torch.float64, _lib.QI_F64)):
        size = torch.empty(0, dtype=tdtype).element_size()
        name = str(tdtype).split(".")[-1]
        for label, factor in RATES:
            start, delta, m = grid(ts_host[0], ts_host[-1], FS * factor)
            y_host = rng.standard_normal(n).astype(np.float32 if tdtype == torch.float32 else np.float64)
            xg = start + np.arange(m, dtype=np.float64) * delta
            t0 = time.perf_counter()
            want = np.interp(xg, ts_host, y_host)
            host = (time.perf_counter() - t0) * 1e3
            lines.append(f"{name}, {label}: {m} outputs per record; np.interp on this host, one core: {host:.2f} ms per record")
            for records in args.records:
                if records * (n * size + 8 * m) > args.max_bytes:
                    lines.append(f"  {records:5d} records: skipped, {records * (n * size + 8 * m) / 1e9:.1f} GB of records and results")
                    continue
                gen = torch.Generator(device=dev).manual_seed(records)
                y = torch.randn((records, n), dtype=tdtype, device=dev, generator=gen)
                y[0] = torch.from_numpy(y_host).to(dev)
                out = torch.empty((records, m), dtype=torch.float64, device=dev)

                def native():
                    _lib.check(lib.qi_interp_grid(code, dev.index, _lib.ptr(y), _lib.ptr(ts), 0, records, n, start, delta, m,
                                                  _lib.ptr(out), _lib.stream_ptr(dev)))

                med, lo, hi = timed(native, dev, args.warmup, args.reps)
                same = bool(np.array_equal(out[0].cpu().numpy(), want))
                moved = records * (n * (8.0 + size) + 8.0 * m)
                line = (f"  {records:5d} records, qi_interp_grid: {med:9.3f} ms ({lo:.3f} .. {hi:.3f}) per call | {moved / 1e9:7.3f} GB required = "
                        f"{moved / (med * 1e-3) / 1e9:8.1f} GB/s = {100.0 * moved / (med * 1e-3) / HBM_PEAK:6.2f} % of the 8 TB/s peak | "
                        f"record 0 {'equals' if same else 'DIFFERS FROM'} np.interp | {host * records / med:7.1f} x the host's {host * records:.0f} ms")
                lines.append(line)
                print(line, flush=True)
                xd = torch.from_numpy(xg).to(dev)

                def composed():
                    j = (torch.searchsorted(ts, xd, right=True) - 1).clamp_(0, n - 2)
                    x0, x1 = ts[j], ts[j + 1]
                    f0, f1 = y[:, j].to(torch.float64), y[:, j + 1].to(torch.float64)
                    return (f1 - f0) / (x1 - x0) * (xd - x0) + f0

                creps = args.reps if records <= 64 else max(args.reps // 4, 1)  # (tens of GB of temporaries per call)
                try:
                    cmed, clo, chi = timed(composed, dev, 1 if records > 64 else args.warmup, creps)
                    line = (f"  {records:5d} records, PyTorch searchsorted / gathers / arithmetic (no NaN branches, grid made beforehand): "
                            f"{cmed:9.3f} ms ({clo:.3f} .. {chi:.3f}) per call, {creps} calls | native / composed = {med / cmed:.3f}")
                except torch.cuda.OutOfMemoryError:
                    line = f"  {records:5d} records, PyTorch composition: out of memory"
                lines.append(line)
                print(line, flush=True)
                del y, out, xd
                torch.cuda.empty_cache()


def fft_part(lib, dev, args, lines):
    n = 1 << args.log2n
    for tdtype, code in ((torch.float32, _lib.QI_F32), (torch.float64, _lib.QI_F64)):
        name = str(tdtype).split(".")[-1]
        size = torch.empty(0, dtype=tdtype).element_size()
        for m in (n // 2, 3 * n // 4):
            for records in args.records:
                nbytes = int(lib.qi_resample_fft_scratch_bytes(code, records, n, m))
                if nbytes + records * (n + m) * size > args.max_bytes:
                    lines.append(f"{name} {n} -> {m}, {records:5d} records: skipped, {nbytes / 1e9:.1f} GB of scratch")
                    continue
                gen = torch.Generator(device=dev).manual_seed(records)
                x = torch.randn((records, n), dtype=tdtype, device=dev, generator=gen)
                out = torch.empty((records, m), dtype=tdtype, device=dev)
                scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)

                def native():
                    _lib.check(lib.qi_resample_fft(code, dev.index, _lib.ptr(x), records, n, m, _lib.ptr(out), _lib.ptr(scratch), nbytes,
                                                   _lib.stream_ptr(dev)))

                def composed():
                    X = torch.fft.rfft(x, dim=1)[:, :m // 2 + 1].clone()
                    X[:, m // 2] *= 2.0
                    return torch.fft.irfft(X, m, dim=1) * (m / n)

                med, lo, hi = timed(native, dev, args.warmup, args.reps)
                cmed, clo, chi = timed(composed, dev, args.warmup, args.reps)
                ref = composed()
                err = float((out - ref).abs().max() / ref.abs().max())
                moved = records * (n + m) * size
                line = (f"{name} {n} -> {m}, {records:5d} records, qi_resample_fft: {med:9.3f} ms ({lo:.3f} .. {hi:.3f}) per call | records in "
                        f"and out {moved / 1e9:7.3f} GB = {moved / (med * 1e-3) / 1e9:8.1f} GB/s | torch.fft.rfft / irfft: {cmed:9.3f} ms "
                        f"({clo:.3f} .. {chi:.3f}) | native / composed = {med / cmed:.3f} | max difference {err:.2e} of the maximum")
                lines.append(line)
                print(line, flush=True)
                del x, out, scratch, ref
                torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--records", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--max-bytes", type=float, default=120e9, help="shapes whose buffers exceed this are skipped and said so")
    ap.add_argument("--skip-fft", action="store_true")
    args = ap.parse_args()
    lib = _lib.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    lines = [f"qi_interp_grid (tile {_lib.INTERP_TILE} outputs, {_lib.INTERP_KNOTS} knots in LDS) and qi_resample_fft, records of "
             f"2^{args.log2n} samples, {torch.cuda.get_device_name(dev)}; device events, median (min .. max) of {args.reps} calls "
             f"after {args.warmup}"]
    interp_part(lib, dev, args, lines)
    if not args.skip_fft:
        fft_part(lib, dev, args, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
