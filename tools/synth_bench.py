"""Device time of qi_synth and qi_doppler.  1, 64 and 1024 records of 2^20 samples with a parameter row per record; the tone,
the linear chirp under its Tukey taper, synth_01 under its gate, the GT pulse and the forward doppler geometry; float32 and
float64 stores (doppler: three float64 outputs); timed with device events after warm-up, median of 20 calls.  Per call: the
time and the bytes stored over the time against the 8 TB/s peak (nothing is read but a parameter row).  Beside it, in the
same job, the PyTorch composition of the same formula in float64 on the device -- timed twice, so that the spread between
its repeated runs is known -- and NumPy on one core of this host (one record).

    python tools/synth_bench.py [--out profiles/synth_kernel.txt] [--records 1 64 1024] [--log2n 20] [--reps 20]
    python tools/synth_bench.py --once 64      (every kernel once at 64 records, float64: the run a counter collection wraps)"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from quantum_inferno_amd import _lib, engine  # noqa: E402
from quantum_inferno_amd.synth import doppler as qd  # noqa: E402

HBM_PEAK = 8.0e12  # bytes per second
RATE = 800.0
PI = np.pi


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


def tukey_torch(n, alpha, dev):
    k = torch.arange(n, dtype=torch.float64, device=dev)
    width = int(np.floor(alpha * (n - 1) / 2.0))
    head = 0.5 * (1 + torch.cos(PI * (-1 + 2.0 * k / alpha / (n - 1))))
    tail = 0.5 * (1 + torch.cos(PI * (-2.0 / alpha + 1 + 2.0 * k / alpha / (n - 1))))
    return torch.where(k <= width, head, torch.where(k >= n - width - 1, tail, torch.ones_like(k)))


def host_gt(t, quarter, a):
    tau = t / quarter + 1.0
    out = np.zeros(len(t))
    one, two = (0.0 <= tau) & (tau <= 1.0), (1.0 < tau) & (tau <= a)
    out[one] = 1.0 - tau[one]
    out[two] = 1.0 / 6.0 * (1.0 - tau[two]) * (a - tau[two]) ** 2
    return out


def cases(records, n, dev):
    """name -> (kind, parameter rows [C, p], axis, envelope, PyTorch composition (rows on the device, t [n]) -> [C, n], NumPy of one record)."""
    f = np.linspace(0.8, 1.25, records)[:, None]
    t_last = (n - 1) / RATE
    span = n / RATE
    tone = np.array([[2.0 * PI * 60.0 / RATE]]) * f
    chirp = np.concatenate([5.0 * f, 0.5 * ((RATE / 4.0 - 5.0 * f) / t_last)], axis=1)
    s01 = np.array([[100.0 * PI / span, 20.0 * PI / span ** 2, PI * 5.0 / span, 4.0 * PI, PI * 80.0 / span]]) * np.concatenate([f, f, f, f * 0 + 1, f], axis=1)
    gt = np.concatenate([(span / 8.0) * f, 0 * f], axis=1)
    window = tukey_torch(n, 0.25, dev)
    gate = tukey_torch(n, 0.05, dev)
    a = float(1 + np.sqrt(6.0))

    index = torch.arange(n, dtype=torch.float64, device=dev)

    def c_tone(p, t):
        return torch.cos(p[:, :1] * index)

    def c_chirp(p, t):
        return torch.cos((2 * PI) * (p[:, :1] * t + p[:, 1:2] * t * t)) * window

    def c_s01(p, t):
        return (torch.cos(p[:, :1] * t - p[:, 1:2] * t * t) + torch.cos(p[:, 3:4] * torch.sin(p[:, 2:3] * t) + p[:, 4:5] * t)) * gate

    def c_gt(p, t):
        tau = (t - span / 2.0) / p[:, :1] + 1.0
        return torch.where((0.0 <= tau) & (tau <= 1.0), 1.0 - tau,
                           torch.where((1.0 < tau) & (tau <= a), (1.0 / 6.0) * (1.0 - tau) * (a - tau) ** 2, torch.zeros_like(tau)))

    tn = np.arange(n) / RATE
    return {
        "tone": ("tone", tone, ("step", 1.0), None, c_tone, lambda: np.cos(tone[0, 0] * np.arange(n))),
        "chirp_linear": ("chirp_linear", chirp, ("rate", RATE), ("tukey", 0.25), c_chirp,
                         lambda: np.cos(2 * PI * (chirp[0, 0] * tn + chirp[0, 1] * tn * tn)) * window.cpu().numpy()),
        "synth_01": ("synth_01", s01, ("rate", RATE), ("gate", 0.0, span, 0.05), c_s01,
                     lambda: (np.cos(s01[0, 0] * tn - s01[0, 1] * tn * tn) + np.cos(s01[0, 3] * np.sin(s01[0, 2] * tn) + s01[0, 4] * tn)) * gate.cpu().numpy()),
        "gt": ("gt", gt, ("rate", RATE, span / 2.0), None, c_gt, lambda: host_gt(tn - span / 2.0, gt[0, 0], a)),
    }


def native_synth(lib, dev, kind, rows, n, axis, env, tdtype):
    """The C call alone: parameter rows and the output on the device already, the gate's span found once."""
    p = torch.from_numpy(np.ascontiguousarray(np.pad(rows, ((0, 0), (0, _lib.SYNTH_PARAMS - rows.shape[1]))))).to(dev)
    out = torch.empty((rows.shape[0], n), dtype=tdtype, device=dev)
    code, value = engine.SYNTH_AXES[axis[0]], float(axis[1])
    s0 = float(axis[2]) if len(axis) > 2 else 0.0
    e, alpha, tmin, tmax, k0, m = 0, 0.0, 0.0, 0.0, 0, 0
    if env is not None:
        e, alpha = engine.SYNTH_ENVELOPES[env[0]], float(env[-1])
        if env[0] == "gate":
            tmin, tmax = float(env[1]), float(env[2])
            k0, m = engine.gate_span(n, axis, tmin, tmax)

    def call():
        _lib.call(lib.qi_synth, dev, _lib.dtype_code(tdtype), dev.index, engine.SYNTH_KINDS[kind], 0, _lib.ptr(p), _lib.SYNTH_PARAMS, code, value,
                  None, 0, s0, 0.0, e, alpha, tmin, tmax, k0, m, rows.shape[0], n, _lib.ptr(out))

    return call, (p, out)


def native_doppler(lib, dev, rows, n):
    p = torch.from_numpy(rows).to(dev)
    outs = [torch.empty((rows.shape[0], n), dtype=torch.float64, device=dev) for _ in range(3)]

    def call():
        _lib.call(lib.qi_doppler, dev, dev.index, 0, _lib.ptr(p), _lib.DOPPLER_PARAMS, _lib.QI_AXIS_RATE, RATE, None, 0, 0.0, 0.0, rows.shape[0], n,
                  *(_lib.ptr(o) for o in outs))

    return call, (p, outs)


def doppler_rows(records):
    return np.stack([qd.geometry_row(340., 68., 3.0 + c % 5, np.array([-1000., 10., 150.]), np.array([1000., 10., 150.]),
                                     np.array([-50. + c, 30., 2.]), np.array([80., -20., 2.])) for c in range(records)])


def doppler_torch(p, t):
    c, c2, denom = p[:, 0:1], p[:, 1:2], p[:, 2:3]
    s, v, r = [p[:, 3 + d:4 + d] for d in range(3)], [p[:, 6 + d:7 + d] for d in range(3)], [p[:, 9 + d:10 + d] for d in range(3)]
    q = [r[d] - s[d] * t for d in range(3)]
    term1 = (c2 * t + (v[0] * q[0] + v[1] * q[1] + v[2] * q[2])) * denom
    rm2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2]
    term2 = (rm2 - (t * c) ** 2) * denom
    ts = term1 + torch.sqrt(term1 * term1 + term2)
    g = [q[d] + v[d] * ts for d in range(3)]
    rt = torch.sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2])
    om = (c - (g[0] * v[0] + g[1] * v[1] + g[2] * v[2]) / rt) / (c - (g[0] * s[0] + g[1] * s[1] + g[2] * s[2]) / rt)
    return ts, rt, om


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--records", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--once", type=int, default=0)
    args = ap.parse_args()
    lib = _lib.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    n = 1 << args.log2n
    t = torch.arange(n, dtype=torch.float64, device=dev) / RATE
    if args.once:
        for name, (kind, rows, axis, env, _, _) in cases(args.once, n, dev).items():
            engine.synthesize(kind, rows, n, axis=axis, envelope=env)
        engine.doppler(doppler_rows(args.once), n, ("rate", RATE))
        torch.cuda.synchronize(dev)
        return
    lines = [f"qi_synth and qi_doppler (tiles of {_lib.SYNTH_TILE} samples, one launch), records of 2^{args.log2n} samples, a parameter row per "
             f"record, {torch.cuda.get_device_name(dev)}; device events, median (min .. max) of {args.reps} calls after {args.warmup}; bytes: "
             "the stores (nothing is read but the parameter rows); the PyTorch composition (float64 on the device, same formula) is timed twice"]

    def emit(line):
        lines.append(line)
        print(line, flush=True)

    for records in args.records:
        table = cases(records, n, dev)
        for name, (kind, rows, axis, env, composed, host) in table.items():
            p = torch.from_numpy(rows).to(dev)
            for tdtype in (torch.float32, torch.float64):
                size = 4 if tdtype == torch.float32 else 8
                call, keep = native_synth(lib, dev, kind, rows, n, axis, env, tdtype)
                med, lo, hi = timed(call, dev, args.warmup, args.reps)
                del keep
                stored = records * n * size
                line = (f"  {records:5d} records, {name:12s} {str(tdtype).split('.')[-1]}: {med:9.3f} ms ({lo:.3f} .. {hi:.3f}) per call | {stored / 1e9:6.3f} GB "
                        f"stored = {stored / (med * 1e-3) / 1e9:7.1f} GB/s = {100.0 * stored / (med * 1e-3) / HBM_PEAK:5.2f} % of the 8 TB/s peak")
                try:
                    runs = [timed(lambda: composed(p, t).to(tdtype), dev, args.warmup, args.reps) for _ in range(2)]
                    cmed = min(r[0] for r in runs)
                    spread = abs(runs[0][0] - runs[1][0])
                    verdict = "" if records == 1 or med <= cmed + spread else "  ** SLOWER than the composition by more than its spread **"
                    line += (f" | PyTorch composition {runs[0][0]:9.3f} and {runs[1][0]:9.3f} ms (spread {spread:.3f}), native / composed = "
                             f"{med / cmed:.3f}{verdict}")
                except torch.cuda.OutOfMemoryError:
                    line += " | PyTorch composition: out of memory"
                torch.cuda.empty_cache()
                if host is not None and tdtype == torch.float64:
                    h = host_time(host)
                    line += f" | {h * records / med:8.1f} x NumPy on one host core ({h:.1f} ms a record)"
                emit(line)
        rows = doppler_rows(records)
        p = torch.from_numpy(rows).to(dev)
        call, keep = native_doppler(lib, dev, rows, n)
        med, lo, hi = timed(call, dev, args.warmup, args.reps)
        del keep
        stored = records * n * 24
        line = (f"  {records:5d} records, doppler forward float64: {med:9.3f} ms ({lo:.3f} .. {hi:.3f}) per call | {stored / 1e9:6.3f} GB stored = "
                f"{stored / (med * 1e-3) / 1e9:7.1f} GB/s = {100.0 * stored / (med * 1e-3) / HBM_PEAK:5.2f} % of the 8 TB/s peak")
        try:
            runs = [timed(lambda: doppler_torch(p, t), dev, args.warmup, args.reps) for _ in range(2)]
            cmed = min(r[0] for r in runs)
            spread = abs(runs[0][0] - runs[1][0])
            verdict = "" if records == 1 or med <= cmed + spread else "  ** SLOWER than the composition by more than its spread **"
            line += (f" | PyTorch composition {runs[0][0]:9.3f} and {runs[1][0]:9.3f} ms (spread {spread:.3f}), native / composed = {med / cmed:.3f}"
                     f"{verdict}")
        except torch.cuda.OutOfMemoryError:
            line += " | PyTorch composition: out of memory"
        torch.cuda.empty_cache()
        tn = np.arange(n) / RATE
        def host_doppler():
            r = rows[0]
            q = r[9:12][None, :] - r[3:6][None, :] * tn[:, None]
            term1 = (r[1] * tn + np.sum(r[6:9][None, :] * q, 1)) * r[2]
            term2 = (np.sum(q * q, 1) - (tn * r[0]) ** 2) * r[2]
            ts = term1 + np.sqrt(term1 ** 2 + term2)
            g = q + r[6:9][None, :] * ts[:, None]
            rt = np.sqrt(np.sum(g * g, 1))
            return (r[0] - np.sum(g * r[6:9][None, :], 1) / rt) / (r[0] - np.sum(g * r[3:6][None, :], 1) / rt)

        h = host_time(host_doppler)
        line += f" | {h * records / med:8.1f} x NumPy on one host core ({h:.1f} ms a record)"
        emit(line)
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
