"""Device time of qi_tfr_ifreq, qi_tfr_squeeze and qi_tfr_synchrosqueeze on order-12 CWT panels of 2^20 samples, against the
bytes the fused call must move and against the PyTorch composition of the same method, tools/timebeam_bench.py's method:
device events after warm-up, median (min .. max) of 20 calls, everything in the same job.

The panel is the plan's own (a chirp in noise through plan.cwt, 167 bands at 800 Hz); 1 and 16 records; scales.squeeze_bin_edges
with 1 and 8 bins per band; float32 and float64.  Beside the fused call's time: the rate at which it moves the bytes it must
move, (nb + nbin) n complex values per record -- the panel read once, the result written once --, the two-call composition
(qi_tfr_ifreq then qi_tfr_squeeze, which stores and re-reads [C, nb, n] frequencies), and the PyTorch composition: angle of
the lagged product, bucketize, scatter_add_ into a cleared result.  The PyTorch composition materialises several [C, nb, n]
intermediates, so it runs on one record and its time is scaled to the record count -- the scaled figure is marked.  A shape
whose buffers pass MEMORY_BUDGET is not run and is listed as such.

The second table is the fused call on one record over the bin count alone (edges even in log f over the panel's bands).
Nothing here is gated: the numbers are recorded, the shapes where the call loses included.

    python tools/squeeze_bench.py [--out profiles/squeeze_kernel.txt] [--records 1 16] [--reps 20] [--log2n 20]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from quantum_inferno_amd import engine  # noqa: E402
from quantum_inferno_amd import scales_dyadic as scales  # noqa: E402

FS, ORDER = 800.0, 12
MEMORY_BUDGET = 96 << 30
SWEEP_BINS = (16, 32, 48, 64, 96, 128, 167, 334)


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


def fmt(t):
    return f"{t[0]:9.3f} ms ({t[1]:.3f} .. {t[2]:.3f})"


def records(n_ch, n, dtype, dev):
    rng = np.random.default_rng(20261021)
    t = np.arange(n) / FS
    chirp = np.sin(2 * np.pi * (10.0 * t + 0.5 * (110.0 / t[-1]) * t * t))
    return torch.from_numpy((chirp[None] + 0.5 * rng.standard_normal((n_ch, n))).astype(dtype)).to(dev)


def panel_of(sig):
    n = sig.shape[1]
    f_hz = scales.log_frequency_hz_from_fft_points(FS, n, ORDER)
    plan = engine.TfrPlan(n, sig.dtype, sig.device, engine.TfrPlan.workspace_for(n, len(f_hz), sig.dtype))
    try:
        plan.set_styx_bank(ORDER, FS, "norm")
        res = plan.cwt(sig, coef=True)
        torch.cuda.synchronize(sig.device)
        return np.asarray(res.frequency_hz, dtype=np.float64), res.coef
    finally:
        plan.close()


def torch_composition(z, edges, out):
    """The method in PyTorch: the frequencies from the angle of the lagged product, the bins by bucketize, the sums by
    scatter_add_ (atomics: the order of the additions is the run's)."""
    n = z.shape[-1]
    d = z[..., 1:] * z[..., :-1].conj()
    d = torch.cat([d, d[..., n - 2:n - 1]], dim=-1)
    f = torch.angle(d) * (FS / (2.0 * np.pi))
    k = torch.bucketize(f, edges, right=True) - 1
    inside = (k >= 0) & (k < edges.numel() - 1)
    src = torch.view_as_real(z * inside)
    index = k.clamp_(0, edges.numel() - 2).unsqueeze(-1).expand(-1, -1, -1, 2)
    out.zero_()
    torch.view_as_real(out).scatter_add_(1, index, src)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--records", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--log2n", type=int, default=20)
    args = ap.parse_args()
    dev = engine.default_device()
    n = 1 << args.log2n
    lines = [f"squeeze_bench: order-{ORDER} CWT panels of 2^{args.log2n} samples at {FS:g} Hz, median (min .. max) of {args.reps} calls, device events",
             f"device: {torch.cuda.get_device_name(dev)}", ""]

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say(f"{'dtype':8s} {'C':>3s} {'bins':>5s} {'ifreq':>30s} {'squeeze':>30s} {'fused':>30s} {'GB/s must-move':>15s} {'two calls / fused':>18s} {'torch':>30s} {'torch / fused':>14s}")
    for name in ("float32", "float64"):
        rdtype = torch.float32 if name == "float32" else torch.float64
        e = 4 if name == "float32" else 8
        for n_ch in args.records:
            nb = len(scales.log_frequency_hz_from_fft_points(FS, n, ORDER))
            for per in (1, 8):
                nbin = nb * per
                need = n_ch * n * (nb * 2 * e + nb * e + nbin * 2 * e)  # the panel, the frequencies, the result
                if need > MEMORY_BUDGET:
                    say(f"{name:8s} {n_ch:3d} {nbin:5d}   not run: the panel, the frequencies and the result take {need / 2**30:.0f} GiB")
                    continue
                f_hz, z = panel_of(records(n_ch, n, name, dev))
                edges, _ = scales.squeeze_bin_edges(f_hz, per)
                ifreq = engine.instantaneous_frequency(z, FS)
                t_i = timed(lambda: engine.instantaneous_frequency(z, FS), dev, 3, args.reps)
                t_s = timed(lambda: engine.squeeze(z, ifreq, edges), dev, 3, args.reps)
                t_f = timed(lambda: engine.synchrosqueeze(z, FS, edges), dev, 3, args.reps)
                del ifreq
                must = n_ch * n * (nb + nbin) * 2 * e
                z1 = z[:1].contiguous()
                edges_t = torch.from_numpy(edges.astype(name)).to(dev)
                out1 = torch.empty((1, nbin, n), dtype=z.dtype, device=dev)
                t_t = timed(lambda: torch_composition(z1, edges_t, out1), dev, 2, max(3, args.reps // 4))
                scaled = tuple(v * n_ch for v in t_t)
                say(f"{name:8s} {n_ch:3d} {nbin:5d} {fmt(t_i)} {fmt(t_s)} {fmt(t_f)} {must / t_f[0] / 1e6:15.0f} {(t_i[0] + t_s[0]) / t_f[0]:18.2f} "
                    f"{fmt(scaled)}{'*' if n_ch > 1 else ' '} {scaled[0] / t_f[0]:13.2f}")
                del z, z1, out1
                torch.cuda.empty_cache()
    say("(* one record's time scaled to the record count)")
    say("")
    say("the fused call over the bin count: one record")
    say(f"{'dtype':8s} {'bins':>5s} {'fused':>30s} {'GB/s must-move':>15s}")
    for name in ("float32", "float64"):
        e = 4 if name == "float32" else 8
        f_hz, z = panel_of(records(1, n, name, dev))
        for nbin in SWEEP_BINS:
            edges = np.geomspace(f_hz[0] / 1.05, f_hz[-1] * 1.05, nbin + 1)
            t_f = timed(lambda: engine.synchrosqueeze(z, FS, edges), dev, 2, args.reps)
            say(f"{name:8s} {nbin:5d} {fmt(t_f)} {n * (len(f_hz) + nbin) * 2 * e / t_f[0] / 1e6:15.0f}")
        del z
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
