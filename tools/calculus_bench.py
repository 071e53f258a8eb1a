"""Device time of qi_cumtrapz and qi_derivative.  1, 64 and 1024 records of 2^20 samples, float32 and float64, with a
constant spacing and with shared float64 timestamps, timed with device events after warm-up, median of 20 calls.  Per call:
the time and the bytes the operation has to move through HBM -- every input read once (the shared timestamps once per
record, as each record's workgroups read them) and the output written once -- over the time against the 8 TB/s peak.
qi_cumtrapz reads its inputs twice (tile totals, then the scan), so its share of the peak by the bytes it does move is
higher than the one printed.  Beside it, in the same job, the PyTorch composition on the device (torch.cumsum of the
terms; sliced differences for the derivatives) and SciPy / NumPy on one core of this host (one record).

    python tools/calculus_bench.py [--out profiles/calculus_kernel.txt] [--records 1 64 1024] [--log2n 20] [--reps 20]"""
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


def host_time(call):
    t0 = time.perf_counter()
    call()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--records", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    try:
        import scipy.integrate as si
    except ImportError:
        si = None
    lib = _lib.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    n = 1 << args.log2n
    rng = np.random.default_rng(21)
    ts_host = np.concatenate([[0.0], np.cumsum((1.0 + 0.3 * rng.uniform(-1.0, 1.0, n - 1)) / FS)])
    ts = torch.from_numpy(ts_host).to(dev)
    lines = [f"qi_cumtrapz (tiles of {_lib.SCAN_TILE} terms, three launches) and qi_derivative (one launch), records of 2^{args.log2n} "
             f"samples, {torch.cuda.get_device_name(dev)}; device events, median (min .. max) of {args.reps} calls after {args.warmup}; "
             "required bytes: inputs read once, output written once"]

    def emit(line):
        lines.append(line)
        print(line, flush=True)

    for tdtype, code in ((torch.float32, _lib.QI_F32), (torch.float64, _lib.QI_F64)):
        size = torch.empty(0, dtype=tdtype).element_size()
        name = str(tdtype).split(".")[-1]
        y_host = rng.standard_normal(n).astype(np.float32 if size == 4 else np.float64)
        for stamped in (False, True):
            x = ts if stamped else None
            xh = ts_host if stamped else None
            what = "timestamps" if stamped else "constant spacing"
            host = {}
            if si is not None:
                host["cumtrapz"] = host_time(lambda: si.cumulative_trapezoid(y_host, x=xh, dx=1 / FS, initial=0))
            host["gradient"] = host_time(lambda: np.gradient(y_host, xh) if stamped else np.gradient(y_host, 1 / FS))
            host["difference"] = host_time(lambda: np.diff(y_host) / np.diff(xh) if stamped else np.diff(y_host) * FS)
            emit(f"{name}, {what}: one record on one core of this host: " + ", ".join(f"{k} {v:.2f} ms" for k, v in host.items())
                 + ("" if si is not None else ", cumtrapz not measured yet (no SciPy here)"))
            for records in args.records:
                gen = torch.Generator(device=dev).manual_seed(records)
                y = torch.randn((records, n), dtype=tdtype, device=dev, generator=gen)
                y[0] = torch.from_numpy(y_host).to(dev)
                osize = {"cumtrapz": 8 if stamped else size, "gradient": size, "difference": 8 if stamped else size}
                nbytes = int(lib.qi_cumtrapz_scratch_bytes(code, records, n))
                scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
                outs = {k: torch.empty((records, n), dtype=torch.float64 if v == 8 else torch.float32, device=dev) for k, v in osize.items()}

                def cumtrapz():
                    _lib.check(lib.qi_cumtrapz(code, dev.index, _lib.ptr(y), _lib.ptr(x), 0, 1 / FS, records, n, _lib.ptr(outs["cumtrapz"]),
                                               _lib.ptr(scratch), nbytes, _lib.stream_ptr(dev)))

                def gradient():
                    _lib.check(lib.qi_derivative(code, dev.index, _lib.QI_DERIV_GRADIENT, _lib.ptr(y), _lib.ptr(x), 0, 1 / FS, records, n,
                                                 _lib.ptr(outs["gradient"]), 0, _lib.stream_ptr(dev)))

                def difference():
                    _lib.check(lib.qi_derivative(code, dev.index, _lib.QI_DERIV_DIFFERENCE, _lib.ptr(y), _lib.ptr(x), 0, FS, records, n,
                                                 _lib.ptr(outs["difference"]), 0, _lib.stream_ptr(dev)))

                def t_cumtrapz():
                    s = y[:, 1:] + y[:, :-1]
                    terms = (x[1:] - x[:-1]) * s / 2.0 if stamped else (1 / FS) * s / 2.0
                    return torch.cumsum(terms, dim=1)

                def t_gradient():
                    if not stamped:
                        return (y[:, 2:] - y[:, :-2]) / (2.0 / FS)
                    d = x[1:] - x[:-1]
                    dx1, dx2 = d[:-1], d[1:]
                    return -(dx2) / (dx1 * (dx1 + dx2)) * y[:, :-2] + (dx2 - dx1) / (dx1 * dx2) * y[:, 1:-1] + dx1 / (dx2 * (dx1 + dx2)) * y[:, 2:]

                def t_difference():
                    d = y[:, 1:] - y[:, :-1]
                    return d / (x[1:] - x[:-1]) if stamped else d * FS

                for key, native, composed in (("cumtrapz", cumtrapz, t_cumtrapz), ("gradient", gradient, t_gradient),
                                              ("difference", difference, t_difference)):
                    med, lo, hi = timed(native, dev, args.warmup, args.reps)
                    moved = records * n * (size + (8 if stamped else 0) + osize[key])
                    line = (f"  {records:5d} records, {key:10s}: {med:9.3f} ms ({lo:.3f} .. {hi:.3f}) per call | {moved / 1e9:7.3f} GB required = "
                            f"{moved / (med * 1e-3) / 1e9:8.1f} GB/s = {100.0 * moved / (med * 1e-3) / HBM_PEAK:6.2f} % of the 8 TB/s peak")
                    try:
                        cmed, clo, chi = timed(composed, dev, args.warmup, args.reps)
                        line += f" | PyTorch composition {cmed:9.3f} ms ({clo:.3f} .. {chi:.3f}), native / composed = {med / cmed:.3f}"
                    except torch.cuda.OutOfMemoryError:
                        line += " | PyTorch composition: out of memory"
                    if key in host:
                        line += f" | {host[key] * records / med:7.1f} x the host's {host[key] * records:.0f} ms"
                    emit(line)
                del y, outs, scratch
                torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
