"""Device time of qi_cross_spectra_windows against what it replaces, tools/csd_bench.py's method: device events after warm-up,
median (min .. max).  A stored panel of 1025 bins x 1023 segments of 4, 16 and 64 records, float32 and float64; windows of
(8, 4), (32, 16), (128, 64) and (128, 128) segments (length, hop); 64 bins of the panel, and all bins at 16 records.  Beside
every shape, in the same job:
  loop    today's composition: per window panel[:, f0:f1, s:s+L].contiguous() and engine.cross_spectra
  einsum  torch.einsum on panel.unfold(2, L, hop)
  whole   at hop = L, qi_cross_spectra of the whole panel's bins: the same arithmetic, 1 / nwin of the stores
Then beamform.fk_timeline_pow2 whole at 16 records, 64 bins, (32, 16), split into panel, contraction, form and the form's
host-table upload launches (their count times the time of one, measured as qi_cross_spectra's weight upload).  Nothing here is
gated: the numbers are recorded, the shapes where the new call loses included.

    python tools/windows_bench.py [--out profiles/windows_kernel.txt] [--records 4 16 64] [--reps 10]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from quantum_inferno_amd import _lib, beamform, engine, styx_fft  # noqa: E402

BINS, SEGMENTS = 1025, 1023
WINDOWS = ((8, 4), (32, 16), (128, 64), (128, 128))
BAND = (16, 64)  # the 64 bins
FS, SEG, HOP = 800.0, 2048, 1024


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


def contraction_rows(lib, dev, dtype, C, reps, lines):
    rng = np.random.default_rng([71, C])
    ctype = engine._complex_of(dtype)
    z = torch.from_numpy(rng.standard_normal((C, BINS, SEGMENTS, 2)).astype(np.float32)).to(dev)
    z = torch.view_as_complex(z).to(ctype).contiguous()
    code = _lib.dtype_code(dtype)
    name = "float32" if dtype == torch.float32 else "float64"
    for first, count in ((BAND,) if C != 16 else (BAND, (0, BINS))):
        for win, hop in WINDOWS:
            nwin = (SEGMENTS - win) // hop + 1
            csd = torch.empty((nwin, count, C, C), dtype=ctype, device=dev)
            scratch, nbytes = _lib.scratch(lib.qi_cross_spectra_windows_scratch_bytes, dev, code, C, BINS, SEGMENTS, first, count, win, hop)

            def windows():
                _lib.call(lib.qi_cross_spectra_windows, dev, code, dev.index, _lib.ptr(z), C, BINS, SEGMENTS, first, count, win, hop, None,
                          _lib.ptr(csd), None, _lib.ptr(scratch), nbytes)

            def loop():
                for w in range(nwin):
                    engine.cross_spectra(z[:, first:first + count, w * hop:w * hop + win].contiguous())

            def einsum():
                u = z[:, first:first + count].unfold(2, win, hop)
                return torch.einsum("ifwk,jfwk->wfij", u.conj(), u)

            t_win = timed(windows, dev, 2, reps)
            t_loop = timed(loop, dev, 1, 3)
            t_ein = timed(einsum, dev, 1, max(3, reps // 2))
            out_mb = nwin * count * C * C * 2 * (4 if dtype == torch.float32 else 8) / 1e6
            lines += [f"{name} C = {C}, bins {first}+{count}, windows of {win} every {hop}: {nwin} windows, {out_mb:.1f} MB of matrices",
                      f"  qi_cross_spectra_windows        {fmt(t_win)}   {out_mb / t_win[0] / 1e3:.3f} TB/s of stores",
                      f"  loop of slices + cross_spectra  {fmt(t_loop)}   x {t_loop[0] / t_win[0]:.1f}",
                      f"  torch.einsum on unfold          {fmt(t_ein)}   x {t_ein[0] / t_win[0]:.2f}"]
            if hop == win:
                part = z[:, first:first + count].contiguous()
                s2, n2 = _lib.scratch(lib.qi_cross_spectra_scratch_bytes, dev, code, C, count, SEGMENTS)
                one = torch.empty((count, C, C), dtype=ctype, device=dev)

                def whole():
                    _lib.call(lib.qi_cross_spectra, dev, code, dev.index, _lib.ptr(part), C, count, SEGMENTS, None, _lib.ptr(one), None,
                              _lib.ptr(s2), n2)

                t_whole = timed(whole, dev, 2, reps)
                lines.append(f"  qi_cross_spectra, whole record  {fmt(t_whole)}   x {t_whole[0] / t_win[0]:.2f}")
                del part, s2, one
            lines.append("")
            print("\n".join(lines[-6:]), flush=True)
            del csd, scratch
            torch.cuda.empty_cache()


def timeline_rows(lib, dev, reps, lines):
    C, win, hop = 16, 32, 16
    n = (SEGMENTS - 1) * HOP + SEG
    rng = np.random.default_rng([72, C])
    x = torch.from_numpy(rng.standard_normal((C, n)).astype(np.float32)).to(dev)
    positions = rng.uniform(-50.0, 50.0, (C, 2))
    slowness = beamform.slowness_grid(3e-3, 21)
    f_all = np.fft.rfftfreq(SEG, 1 / FS)
    edges = f_all[[BAND[0] + 16 * k for k in range(5)]]  # four bands of 16 bins
    nwin = (SEGMENTS - win) // hop + 1
    matrices = nwin * BAND[1]

    def wall(call):
        call()
        torch.cuda.synchronize(dev)
        ms = []
        for _ in range(reps):
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize(dev)
            ms.append(1e3 * (time.perf_counter() - t0))
        return float(np.median(ms)), min(ms), max(ms)

    for method in beamform.TIMELINE_METHODS:
        t = wall(lambda: beamform.fk_timeline_pow2(x, FS, positions, slowness, SEG, win, hop, band_edges_hz=edges, method=method))
        lines.append(f"fk_timeline_pow2 {method:8s} whole, host clock  {fmt(t)}")
    t_mat = wall(lambda: styx_fft.csd_windows_pow2(x, FS, SEG, win, hop, frequency_range_hz=(edges[0], edges[-1])))
    _, _, z = styx_fft.stft_complex_pow2(x, FS, SEG, SEG - HOP, SEG, 0.25)
    z = z[:, :, :SEGMENTS].contiguous()
    t_con = timed(lambda: engine.cross_spectra_windows(z, win, hop, bins=BAND), dev, 2, reps)
    f, _, csd = styx_fft.csd_windows_pow2(x, FS, SEG, win, hop, frequency_range_hz=(edges[0], edges[-1]))
    stack = csd.reshape(matrices, C, C)
    tau = beamform.plane_wave_delays(positions, slowness, dev)
    bands = np.concatenate([(np.arange(nwin)[:, None] * BAND[1] + 16 * np.arange(4)[None, :]).reshape(-1), [matrices]])
    t_form = timed(lambda: engine.beam_power(stack, np.tile(f, nwin), tau, bands=bands, normalize=True, peaks=True), dev, 2, reps)
    # one upload launch: the weights of qi_cross_spectra on a panel of one record and one segment, 4096 bins = 16 launches
    tiny = torch.ones((1, 4096, 1), dtype=torch.complex64, device=dev)
    weights = np.ones(4096)
    t_up = timed(lambda: engine.cross_spectra(tiny, weight=weights), dev, 3, 4 * reps)
    t_none = timed(lambda: engine.cross_spectra(tiny), dev, 3, 4 * reps)
    per = max(t_up[0] - t_none[0], 0.0) / 16
    launches = -(-matrices // 256) + -(-len(bands) // 256)
    lines += [f"csd_windows_pow2 (panel + contraction), host clock  {fmt(t_mat)}",
              f"  contraction alone on a stored panel, device       {fmt(t_con)}",
              f"  panel (the difference)                             {t_mat[0] - t_con[0]:9.3f} ms",
              f"form (engine.beam_power on {matrices} matrices, {len(bands) - 1} bands, {slowness.shape[0]} grid points), device  {fmt(t_form)}",
              f"  its host-table uploads: {launches} launches of 256 values x {1e3 * per:.1f} us each (measured as 16 weight launches of "
              f"qi_cross_spectra: {fmt(t_up)} against {fmt(t_none)} without) = {launches * per:.3f} ms = "
              f"{100 * launches * per / t_form[0]:.1f} % of the form", ""]
    print("\n".join(lines[-9:]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "windows_kernel.txt"))
    ap.add_argument("--records", type=int, nargs="+", default=[4, 16, 64])
    ap.add_argument("--reps", type=int, default=10)
    opt = ap.parse_args()
    lib = _lib.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    lines = [f"qi_cross_spectra_windows on {torch.cuda.get_device_name(dev)}: a stored panel of {BINS} bins x {SEGMENTS} segments; median "
             f"(min .. max) of {opt.reps} calls, device events (the loop: 3 calls; the einsum: {max(3, opt.reps // 2)})",
             "x: the yardstick's time over the windowed call's (below 1: the windowed call loses)", ""]
    for dtype in (torch.float32, torch.float64):
        for C in opt.records:
            contraction_rows(lib, dev, dtype, C, opt.reps, lines)
    timeline_rows(lib, dev, opt.reps, lines)
    with open(opt.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(opt.out)


if __name__ == "__main__":
    main()
