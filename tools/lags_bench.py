"""Device time of qi_pair_lags against the PyTorch composition it replaces, tools/windows_bench.py's method: device events
after warm-up, median (min .. max) of 20 calls, both in the same job.  Matrices of 1025 bins (nfft 2048) of 4, 16 and 64
sensors, stacks of 1 and 32, float32 and float64; upsample 1 and 4, max_lag 64, PHAT weights over the bins 16 .. 900, halved
and normalised, every output.  The composition: the pair gather csd[:, :, i, j], the weights, torch.fft.irfft of the padded
spectrum, the window, argmax, three gathers and the parabola.  Nothing here is gated: the numbers are recorded, the shapes
where the call loses included.  Beside every time the bytes the call must read (the pairs' entries in the band, once) over it.

    python tools/lags_bench.py [--out profiles/lags_kernel.txt] [--sensors 4 16 64] [--stacks 1 32] [--reps 20]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from quantum_inferno_amd import engine  # noqa: E402

NFFT, MAX_LAG, BINS = 2048, 64, (16, 900)
UPSAMPLES = (1, 4)


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


def composition(csd, rows, cols, upsample):
    """engine.pair_lags(csd, bins=BINS, weighting="phat", upsample=upsample, max_lag=MAX_LAG, want_cc=True) in PyTorch."""
    n_f = csd.shape[1]
    L = NFFT * upsample
    x = csd[:, :, rows, cols].transpose(1, 2)  # [nstack, npair, nf]
    f = torch.arange(n_f, device=csd.device)
    band = (f >= BINS[0]) & (f < BINS[1])
    half = torch.where((f > 0) & (f < NFFT // 2), 0.5, 1.0).to(x.real.dtype)
    mag = x.abs()
    live = band & (mag > 0)
    x = torch.where(live, x / torch.where(live, mag, torch.ones_like(mag)), torch.zeros_like(x)) * half
    mult = torch.where((f == 0) | (f == L // 2), 1.0, 2.0).to(x.real.dtype)
    count = (live * mult).sum(-1, keepdim=True)
    r = torch.fft.irfft(x, n=L, dim=-1) * L / count
    cc = torch.cat([r[..., L - MAX_LAG:], r[..., :MAX_LAG + 1]], dim=-1)
    l0 = cc.argmax(-1) - MAX_LAG
    a, b, c = (r.gather(-1, ((l0 + k) % L)[..., None])[..., 0] for k in (-1, 0, 1))
    den = a - 2 * b + c
    delta = torch.where(den == 0, torch.zeros_like(den), 0.5 * (a - c) / den)
    return (l0 + delta) / upsample, b - 0.25 * (a - c) * delta, cc


def rows_for(dev, dtype, C, nstack, reps, lines):
    n_f = NFFT // 2 + 1
    gen = torch.Generator(device=dev).manual_seed(73 * C + nstack)
    csd = torch.view_as_complex(torch.randn((nstack, n_f, C, C, 2), dtype=dtype, device=dev, generator=gen))
    i, j = np.triu_indices(C, 1)
    rows, cols = torch.from_numpy(i).to(dev), torch.from_numpy(j).to(dev)
    name = "float32" if dtype == torch.float32 else "float64"
    read_mb = nstack * i.size * (BINS[1] - BINS[0]) * 2 * csd.real.element_size() / 1e6
    for up in UPSAMPLES:
        kw = dict(bins=BINS, weighting="phat", halve_interior=True, normalize=True, upsample=up, max_lag=MAX_LAG, want_cc=True)
        got = engine.pair_lags(csd, **kw)
        want = composition(csd, rows, cols, up)
        scale = float(want[2].abs().max())
        dev_cc = float((got[2] - want[2]).abs().max()) / scale
        same_peak = float(((got[0] - want[0]).abs() * up < 0.5).double().mean())
        t_call = timed(lambda: engine.pair_lags(csd, **kw), dev, 3, reps)
        t_torch = timed(lambda: composition(csd, rows, cols, up), dev, 3, reps)
        lines += [f"{name} C = {C} ({i.size} pairs), nstack {nstack}, upsample {up} (L = {NFFT * up}): {nstack * i.size} workgroups, "
                  f"{read_mb:.2f} MB of entries in the band",
                  f"  qi_pair_lags          {fmt(t_call)}   {read_mb / t_call[0] / 1e3:.4f} TB/s of entries",
                  f"  PyTorch composition   {fmt(t_torch)}   x {t_torch[0] / t_call[0]:.2f}",
                  f"  (cc against the composition: {dev_cc:.2g} of its largest sample; {100 * same_peak:.1f} % of the peaks within half a sample)", ""]
        print("\n".join(lines[-5:]), flush=True)
        del got, want
    del csd
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lags_kernel.txt"))
    ap.add_argument("--sensors", type=int, nargs="+", default=[4, 16, 64])
    ap.add_argument("--stacks", type=int, nargs="+", default=[1, 32])
    ap.add_argument("--reps", type=int, default=20)
    opt = ap.parse_args()
    dev = engine.default_device()
    lines = [f"qi_pair_lags on {torch.cuda.get_device_name(dev)}: matrices of {NFFT // 2 + 1} bins, PHAT over the bins {BINS[0]} .. {BINS[1]}, "
             f"max_lag {MAX_LAG}, every output; median (min .. max) of {opt.reps} calls, device events, both forms in the same job",
             "x: the composition's time over the call's (below 1: the call loses)", ""]
    for dtype in (torch.float32, torch.float64):
        for C in opt.sensors:
            for nstack in opt.stacks:
                rows_for(dev, dtype, C, nstack, opt.reps, lines)
    with open(opt.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(opt.out)


if __name__ == "__main__":
    main()
