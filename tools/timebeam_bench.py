"""Device time of qi_time_beam_power and qi_time_beam_traces against the PyTorch composition of the same arithmetic,
tools/lags_bench.py's method: device events after warm-up, median (min .. max) of 20 calls, both in the same job.

Records of 2^20 samples at 200 Hz from 4, 16 and 64 sensors scattered over 1 km; 1024 and 4096 delay rows, square slowness
grids of 32 x 32 and 64 x 64 points up to 3 ms/m (delays of hundreds of samples); windows of 4096 samples every 2048; a bank
of 64 phases x 8 taps; float32 and float64.  The traces call at 1, 16 and 64 rows.  Beside every time the share of the
157 TF/s float32 vector peak (float64: half of it), counting 2 C (T + 1) + 2 flop per (row, sample).

The composition: per sensor the gather of the zero-padded record at t + shift + m - c for every tap, the product with the
row's taps, the sums over taps and sensors, the squares, and the window sums through unfold.  It has to materialise
[rows, n] intermediates, so it runs on a block of COMPOSITION_ROWS rows (fewer for 64 sensors would change nothing: its time
is linear in rows) and its time is scaled to the row count -- the scaled figure is marked.  beamform.fk_timeline_pow2
(Bartlett, one band) on the same record is context, not a yardstick: it answers a narrower question from Welch panels.
Nothing here is gated: the numbers are recorded, the shapes where the call loses included.

    python tools/timebeam_bench.py [--out profiles/timebeam_kernel.txt] [--sensors 4 16 64] [--rows 1024 4096] [--reps 20]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from quantum_inferno_amd import beamform, engine  # noqa: E402

N, FS, WIN, HOP, PHASES, TAPS = 1 << 20, 200.0, 4096, 2048, 64, 8
APERTURE_M, MAX_SLOWNESS = 1000.0, 3e-3
COMPOSITION_ROWS = 16
TRACE_ROWS = (1, 16, 64)
PEAK_TF = {torch.float32: 157.0, torch.float64: 78.5}


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
    return f"{t[0]:10.3f} ms ({t[1]:.3f} .. {t[2]:.3f})"


def delayed_rows(x, taps, shift, phase, reach):
    """(b [rows, n], e [rows, n]): the beam and the delayed records' summed squares, in PyTorch."""
    n_ch, n = x.shape
    n_taps = taps.shape[1]
    pad = reach + n_taps
    xp = torch.nn.functional.pad(x, (pad, pad))
    t = torch.arange(n, device=x.device)
    b = torch.zeros((shift.shape[0], n), dtype=x.dtype, device=x.device)
    e = torch.zeros_like(b)
    for i in range(n_ch):
        base = t[None, :] + shift[:, i:i + 1].long() + (pad - (n_taps - 1) // 2)
        h = taps[phase[:, i].long()]
        y = torch.zeros_like(b)
        for m in range(n_taps):
            y += h[:, m:m + 1] * xp[i][base + m]
        b += y
        e += y * y
    return b, e


def composition_power(x, taps, shift, phase, reach):
    b, e = delayed_rows(x, taps, shift, phase, reach)
    big_b, big_e = (b * b).unfold(1, WIN, HOP).sum(-1), e.unfold(1, WIN, HOP).sum(-1)
    return (big_b / (x.shape[0] * big_e)).T


def composition_traces(x, taps, shift, phase, reach):
    return delayed_rows(x, taps, shift, phase, reach)[0] / x.shape[0]


def share(rows, n_ch, ms, dtype):
    flop = rows * N * (2.0 * n_ch * (TAPS + 1) + 2.0)
    return flop / (ms * 1e-3) / 1e12, 100.0 * flop / (ms * 1e-3) / 1e12 / PEAK_TF[dtype]


def array_of(n_ch):
    rng = np.random.default_rng([53, n_ch])
    return rng.uniform(-0.5 * APERTURE_M, 0.5 * APERTURE_M, (n_ch, 2))


def rows_for(dev, dtype, n_ch, row_counts, reps, lines):
    name = "float32" if dtype == torch.float32 else "float64"
    gen = torch.Generator(device=dev).manual_seed(59 * n_ch)
    x = torch.randn((n_ch, N), dtype=dtype, device=dev, generator=gen)
    positions = array_of(n_ch)
    bank = engine.delay_bank(PHASES, TAPS, 5.0, dtype).to(dev)
    for rows in row_counts:
        slowness = beamform.slowness_grid(MAX_SLOWNESS, int(round(rows ** 0.5)))
        shift, phase, reach = engine.quantize_delays(beamform.plane_wave_delays(positions, slowness, dev), FS, PHASES, device=dev)
        call = lambda: engine.time_beam_power(x, shift, phase, bank, WIN, HOP, reach, normalize=True, peaks=True)  # noqa: E731
        got = call()[0]
        block = slice(rows // 2, rows // 2 + COMPOSITION_ROWS)
        comp = lambda: composition_power(x, bank, shift[block], phase[block], reach)  # noqa: E731
        want = comp()
        dev_max = float((got[:, block] - want).abs().max())
        t_call = timed(call, dev, 2, reps)
        t_comp = timed(comp, dev, 1, max(3, reps // 5))
        scaled = t_comp[0] * rows / COMPOSITION_ROWS
        tf, pct = share(rows, n_ch, t_call[0], dtype)
        lines += [f"{name} C = {n_ch}, G = {rows} (max_shift {reach}), {got.shape[0]} windows of {WIN} every {HOP}",
                  f"  qi_time_beam_power    {fmt(t_call)}   {tf:7.2f} TF/s, {pct:5.1f} % of the vector peak",
                  f"  PyTorch composition   {scaled:10.3f} ms SCALED from {fmt(t_comp)} for {COMPOSITION_ROWS} rows   x {scaled / t_call[0]:.2f}",
                  f"  (semblance against the composition on those rows: {dev_max:.2g})", ""]
        print("\n".join(lines[-5:]), flush=True)
        del got, want
    # the traces call
    slowness = beamform.slowness_grid(MAX_SLOWNESS, 8)
    shift, phase, reach = engine.quantize_delays(beamform.plane_wave_delays(positions, slowness, dev), FS, PHASES, device=dev)
    for k in TRACE_ROWS:
        s, p = shift[:k].contiguous(), phase[:k].contiguous()
        call = lambda: engine.time_beam_traces(x, s, p, bank, reach)  # noqa: E731
        block = slice(0, min(k, COMPOSITION_ROWS))
        comp = lambda: composition_traces(x, bank, s[block], p[block], reach)  # noqa: E731
        dev_max = float((call()[block] - comp()).abs().max())
        t_call = timed(call, dev, 2, reps)
        t_comp = timed(comp, dev, 1, max(3, reps // 5))
        scaled = t_comp[0] * k / (block.stop - block.start)
        tf, pct = share(k, n_ch, t_call[0], dtype)
        lines += [f"{name} C = {n_ch}, K = {k} traces (max_shift {reach})",
                  f"  qi_time_beam_traces   {fmt(t_call)}   {tf:7.2f} TF/s, {pct:5.1f} % of the vector peak",
                  f"  PyTorch composition   {scaled:10.3f} ms{' SCALED' if k > COMPOSITION_ROWS else ''} from {fmt(t_comp)} for {block.stop} rows   x {scaled / t_call[0]:.2f}",
                  f"  (traces against the composition on those rows: {dev_max:.2g})", ""]
        print("\n".join(lines[-5:]), flush=True)
    # context: the frequency-domain timeline on the same record, windows of the same length
    try:
        grid = beamform.slowness_grid(MAX_SLOWNESS, 32)
        fk = lambda: beamform.fk_timeline_pow2(x, FS, positions, grid, 512, 15, 8, band_edges_hz=[FS / 16, FS / 4])  # noqa: E731
        windows = fk()[2].shape[0]
        lines += [f"{name} C = {n_ch}: context, beamform.fk_timeline_pow2 (Bartlett, one band {FS / 16:g} .. {FS / 4:g} Hz, segments of 512, "
                  f"{windows} windows of 15 segments every 8, G = 1024)", f"  fk_timeline_pow2      {fmt(timed(fk, dev, 1, max(3, reps // 4)))}", ""]
    except Exception as err:  # (context only: the record says why it is missing)
        lines += [f"{name} C = {n_ch}: context, beamform.fk_timeline_pow2: not measured ({type(err).__name__}: {err})", ""]
    print("\n".join(lines[-3:]), flush=True)
    del x
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "timebeam_kernel.txt"))
    ap.add_argument("--sensors", type=int, nargs="+", default=[4, 16, 64])
    ap.add_argument("--rows", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--dtypes", nargs="+", default=["float32", "float64"])
    ap.add_argument("--reps", type=int, default=20)
    opt = ap.parse_args()
    dev = engine.default_device()
    lines = [f"qi_time_beam_power and qi_time_beam_traces on {torch.cuda.get_device_name(dev)}: records of {N} samples at {FS:g} Hz, sensors over "
             f"{APERTURE_M:g} m, slowness up to {MAX_SLOWNESS * 1e3:g} ms/m, bank {PHASES} x {TAPS}; median (min .. max) of {opt.reps} calls, device "
             "events, both forms in the same job",
             f"flop: 2 C (T + 1) + 2 per (row, sample); vector peak {PEAK_TF[torch.float32]:g} TF/s float32, {PEAK_TF[torch.float64]:g} float64",
             f"x: the composition's time over the call's (below 1: the call loses); the composition runs {COMPOSITION_ROWS} rows and is scaled to the row count",
             ""]
    for name in opt.dtypes:
        for n_ch in opt.sensors:
            rows_for(dev, torch.float32 if name == "float32" else torch.float64, n_ch, opt.rows, opt.reps, lines)
            with open(opt.out, "w") as fh:  # (kept up to date: a job that runs out of time leaves what it measured)
                fh.write("\n".join(lines) + "\n")
    print(opt.out)


if __name__ == "__main__":
    main()
