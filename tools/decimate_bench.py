"""Device time of the zero-phase decimation (qi_decimate): 1, 64 and 1024 records of 2^20 samples, float32 and float64,
q = 8, timed with device events after warm-up, median of 20 calls.  Per call: the time, records x input samples per
second, and the bytes the two passes move through HBM (record read, n + 2 edge values written and read back, n / q values
written) over the 8 TB/s peak.  Beside the float64 figures the composition the library offered before: zero_phase_filter with
the same sections (qi_filtfilt: a full [C][n] float64 result), then pool_rows "nth" (qi_pool_panel), which writes and
re-reads the full result.  The same decimation through SciPy on this host, where SciPy is importable (4 records; it is
not needed otherwise).

    python tools/decimate_bench.py [--out profiles/decimate_kernel.txt] [--records 1 64 1024] [--log2n 20] [--q 8] [--reps 20]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from quantum_inferno_amd import _lib, engine  # noqa: E402
from quantum_inferno_amd.utilities import iir_design  # noqa: E402
from quantum_inferno_amd.utilities.sampling import pool_rows  # noqa: E402

HBM_PEAK = 8.0e12  # bytes per second


def scipy_ms(n, q, dtype, records=4):
    try:
        import scipy.signal as signal
    except ImportError:
        return None
    x = np.random.default_rng(1).standard_normal((records, n)).astype(dtype)
    t0 = time.perf_counter()
    signal.decimate(x, q, axis=1, zero_phase=True)
    return (time.perf_counter() - t0) * 1e3 / records


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
    ap.add_argument("--q", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    lib = _lib.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    n, q = 1 << args.log2n, args.q
    m = int(lib.qi_decimate_columns(n, q))
    lines = [f"zero-phase decimation by {q}, records of 2^{args.log2n} samples -> {m}, {torch.cuda.get_device_name(dev)}; device "
             f"events, median (min .. max) of {args.reps} calls after {args.warmup}"]
    for tdtype, real, code in ((torch.float32, np.float32, _lib.QI_F32), (torch.float64, np.float64, _lib.QI_F64)):
        sos, zi, edge = iir_design.decimator(q, real)
        host = scipy_ms(n, q, real)
        host_txt = "SciPy not importable on this host" if host is None else f"SciPy on this host, one core: {host:.1f} ms per record"
        size = np.dtype(real).itemsize
        lines.append(f"{np.dtype(real).name}: order-8 Chebyshev type I, 4 second-order sections, extension {edge} ({host_txt})")
        for records in args.records:
            gen = torch.Generator(device=dev).manual_seed(records)
            x = torch.randn((records, n), dtype=tdtype, device=dev, generator=gen)
            out = torch.empty((records, m), dtype=tdtype, device=dev)
            nbytes = int(lib.qi_decimate_scratch_bytes(code, records, n, edge))
            scratch = torch.empty(nbytes // size, dtype=tdtype, device=dev)

            def fused():
                _lib.check(lib.qi_decimate(code, dev.index, _lib.ptr(x), records, n, q, sos.shape[0], sos.ctypes.data,
                                           zi.ctypes.data, edge, _lib.ptr(out), _lib.ptr(scratch), nbytes, _lib.stream_ptr(dev)))

            med, lo, hi = timed(fused, dev, args.warmup, args.reps)
            moved = records * float(size) * (n + 2 * (n + 2 * edge) + m)
            line = (f"  {records:5d} records, qi_decimate: {med:9.3f} ms ({lo:.3f} .. {hi:.3f}) per call = {records * n / med / 1e3:10.1f} M "
                    f"record-samples/s | {moved / 1e9:7.3f} GB through HBM = {moved / (med * 1e-3) / 1e9:8.1f} GB/s = "
                    f"{100.0 * moved / (med * 1e-3) / HBM_PEAK:6.3f} % of the 8 TB/s peak")
            if host is not None:
                line += f" | {host * records / med:7.1f} x the host's {host * records:.0f} ms"
            lines.append(line)
            print(line, flush=True)
            del scratch
            if tdtype == torch.float64:
                def composed():
                    pool_rows(engine.zero_phase_filter(x, "sos", sos, zi, edge), q, "nth", out=out)

                if q >= 2:
                    cmed, clo, chi = timed(composed, dev, args.warmup, args.reps)
                    cmoved = records * 8.0 * (n + 2 * (n + 2 * edge) + n + n + m)
                    line = (f"  {records:5d} records, zero_phase_filter + pool_rows 'nth': {cmed:9.3f} ms ({clo:.3f} .. {chi:.3f}) per call | "
                            f"{cmoved / 1e9:7.3f} GB through HBM | fused / composed = {med / cmed:.3f}")
                    lines.append(line)
                    print(line, flush=True)
            del x, out
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
