"""Device time of the zero-phase filter (qi_filtfilt): 1, 64 and 1024 float64 records of 2^20 samples through the order-4
Butterworth band-pass in (b, a) form (styx_fft.butter_bandpass's filter) and the order-7 band-pass in 7 second-order
sections (picker.apply_bandpass's), timed with device events after warm-up, median of 20 calls.  Per call: the time, records x
samples per second, and the bytes the two passes move through HBM (record read, n + 2 edge values written and read back,
result written) over the 8 TB/s peak.  Beside it the same filter through SciPy on this host, where SciPy is importable
(4 records; it is not needed otherwise).

    python tools/filter_bench.py [--out profiles/filter_kernel.txt] [--records 1 64 1024] [--log2n 20] [--reps 20]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from quantum_inferno_amd import _lib  # noqa: E402
from quantum_inferno_amd.utilities import iir_design  # noqa: E402

HBM_PEAK = 8.0e12  # bytes per second


def filters():
    b, a = iir_design.butter_ba(4, (0.05, 0.2), "bandpass")
    sos = iir_design.butter_sos(7, (0.2, 0.4), "bandpass")
    return [("band-pass order 4, (b, a) form of order 8", _lib.QI_IIR_BA, np.stack([b, a]), iir_design.lfilter_zi(b, a),
             iir_design.filtfilt_edge(b, a), 1, len(a) - 1),
            ("band-pass order 7, 7 second-order sections", _lib.QI_IIR_SOS, sos, iir_design.sosfilt_zi(sos),
             iir_design.sosfiltfilt_edge(sos), sos.shape[0], 2)]


def scipy_ms(form, coef, n, records=4):
    try:
        import scipy.signal as signal
    except ImportError:
        return None
    x = np.random.default_rng(1).standard_normal((records, n))
    t0 = time.perf_counter()
    if form == _lib.QI_IIR_BA:
        signal.filtfilt(coef[0], coef[1], x)
    else:
        signal.sosfiltfilt(coef, x)
    return (time.perf_counter() - t0) * 1e3 / records


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--records", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    lib = _lib.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    n = 1 << args.log2n
    lines = [f"zero-phase filter, float64 records of 2^{args.log2n} samples, {torch.cuda.get_device_name(dev)}; device events, "
             f"median (min .. max) of {args.reps} calls after {args.warmup}"]
    for label, form, coef, zi, edge, sections, order in filters():
        host = scipy_ms(form, coef, n)
        host_txt = "SciPy not importable on this host" if host is None else f"SciPy on this host, one core: {host:.1f} ms per record"
        lines.append(f"{label}, extension {edge} ({host_txt})")
        coef = np.ascontiguousarray(coef, dtype=np.float64)
        zi = np.ascontiguousarray(zi, dtype=np.float64)
        for records in args.records:
            gen = torch.Generator(device=dev).manual_seed(records)
            x = torch.randn((records, n), dtype=torch.float64, device=dev, generator=gen)
            out = torch.empty_like(x)
            nbytes = int(lib.qi_filtfilt_scratch_bytes(records, n, edge))
            scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)

            def call():
                _lib.check(lib.qi_filtfilt(_lib.QI_F64, dev.index, _lib.ptr(x), records, n, None, form, sections, order,
                                           coef.ctypes.data_as(_lib._D), zi.ctypes.data_as(_lib._D), edge, _lib.ptr(out),
                                           _lib.ptr(scratch), nbytes, _lib.stream_ptr(dev)))

            for _ in range(args.warmup):
                call()
            torch.cuda.synchronize(dev)
            ms = []
            for _ in range(args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                call()
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            med = float(np.median(ms))
            moved = records * 8.0 * (n + 2 * (n + 2 * edge) + n)
            line = (f"  {records:5d} records: {med:9.3f} ms ({min(ms):.3f} .. {max(ms):.3f}) per call = {records * n / med / 1e3:10.1f} M "
                    f"record-samples/s | {moved / 1e9:7.3f} GB through HBM = {moved / (med * 1e-3) / 1e9:8.1f} GB/s = "
                    f"{100.0 * moved / (med * 1e-3) / HBM_PEAK:6.3f} % of the 8 TB/s peak")
            if host is not None:
                line += f" | {host * records / med:7.1f} x the host's {host * records:.0f} ms"
            lines.append(line)
            print(line, flush=True)
            del x, out, scratch
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
