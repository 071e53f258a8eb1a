"""Device time of qi_beam_power.  1025 matrices (the bins of tools/csd_bench.py's shape) of C = 4, 16, 64 sensors over grids of
1024 and 4096 delay sets, every matrix its own band and eight bands, float32 and float64; timed with device events after
warm-up, median of 20 calls.  Per shape: the call (power and peaks), its matrix-pipe rate -- 8 real multiply-adds per complex
product; 'formed' counts what the kernel multiplies, sensors padded to whole 16-tiles and grid points to whole 16-tiles,
'useful' the C^2 G products per matrix -- for float32 as a fraction of the 157.3 TF matrix peak, and beside it the PyTorch
composition: the steering tensor exp(2 pi i f tau) [bins, G, C], a batched matrix product with the matrices, the product with the
tensor again summed over the sensors, and the band sums, in chunks of bins that keep the tensor below --chunk-mb.  The
composition is timed over fewer calls (--baseline-reps).  Appends the deviations of tests/test_gpu_beam.py's shapes from the
NumPy restatement.  Nothing here is gated: the numbers are recorded.

    python tools/beam_bench.py [--out profiles/beam_kernel.txt] [--sensors 4 16 64] [--grid 1024 4096] [--reps 20]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from quantum_inferno_amd import _lib, engine  # noqa: E402

import beam_cases as bc  # noqa: E402

F32_MATRIX_PEAK = 157.3e12  # FLOP per second
NF, FS, NFFT, BANDS = 1025, 800.0, 2048, 8


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


def composition(s, freq_d, tau, band_id, nb, chunk):
    """The same power in PyTorch: the steering tensor of `chunk` bins at a time (the phase in double in both precisions: float32 would lose it)."""
    out = torch.zeros((nb, tau.shape[0]), dtype=torch.float64 if s.dtype == torch.complex128 else torch.float32, device=s.device)
    for f0 in range(0, s.shape[0], chunk):
        f1 = min(f0 + chunk, s.shape[0])
        turns = freq_d[f0:f1, None, None] * tau[None, :, :]
        e = torch.polar(torch.ones_like(turns), 2 * np.pi * (turns - torch.round(turns))).to(s.dtype)  # [bins, G, C]
        q = (torch.bmm(e.conj(), s[f0:f1]) * e).sum(dim=-1).real
        out.index_add_(0, band_id[f0:f1], q)
    return out / float(s.shape[1]) ** 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "beam_kernel.txt"))
    ap.add_argument("--sensors", type=int, nargs="+", default=[4, 16, 64])
    ap.add_argument("--grid", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--baseline-reps", type=int, default=5)
    ap.add_argument("--chunk-mb", type=int, default=512)
    ap.add_argument("--no-deviations", action="store_true")
    opt = ap.parse_args()
    lib = _lib.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    freq = np.fft.rfftfreq(NFFT, 1 / FS)
    assert len(freq) == NF
    freq_d = torch.from_numpy(freq).to(dev)
    f_host, f_ptr = _lib.darr(freq)
    tables = {"per bin": None, f"{BANDS} bands": np.linspace(0, NF, BANDS + 1).astype(np.int64)}
    lines = [f"qi_beam_power on {torch.cuda.get_device_name(dev)}: {NF} matrices, delays uniform in +-{bc.MAX_DELAY_S} s; median (min .. max) of "
             f"{opt.reps} calls (the composition: {opt.baseline_reps}), device events",
             "FLOP = 8 per complex product: 'formed' pads sensors and grid points to whole 16-tiles (what the kernel multiplies), 'useful' is",
             "8 C^2 G per matrix; float32 peak = 157.3 TF (matrix pipe).  The composition builds the steering tensor [bins, G, C] in chunks of",
             f"at most {opt.chunk_mb} MB, then torch.bmm, a product and a sum, and index_add_ for the bands", ""]
    for dtype in (torch.float32, torch.float64):
        name = "float32" if dtype == torch.float32 else "float64"
        code, csize = _lib.dtype_code(dtype), (8 if dtype == torch.float32 else 16)
        for C in opt.sensors:
            rng = np.random.default_rng([13, C])
            z = rng.standard_normal((NF, C, 4)) + 1j * rng.standard_normal((NF, C, 4))
            s = torch.from_numpy(np.einsum("fis,fjs->fij", np.conj(z), z)).to(dev).to(engine._complex_of(dtype))
            for G in opt.grid:
                tau = torch.from_numpy(rng.uniform(-bc.MAX_DELAY_S, bc.MAX_DELAY_S, (G, C))).to(dev)
                for label, table in tables.items():
                    nb = NF if table is None else len(table) - 1
                    b_host, b_ptr = (None, None) if table is None else _lib.iarr(table)
                    power = torch.empty((nb, G), dtype=dtype, device=dev)
                    index = torch.empty(nb, dtype=torch.int64, device=dev)
                    value = torch.empty(nb, dtype=dtype, device=dev)
                    scratch, nbytes = _lib.scratch(lib.qi_beam_power_scratch_bytes, dev, code, C, NF, G, nb)

                    def call():
                        _lib.call(lib.qi_beam_power, dev, code, dev.index, _lib.ptr(s), C, NF, f_ptr, _lib.ptr(tau), G, b_ptr, nb, 0,
                                  _lib.ptr(power), _lib.ptr(index), _lib.ptr(value), _lib.ptr(scratch), nbytes)

                    t = timed(call, dev, 3, opt.reps)
                    band_id = torch.from_numpy(np.searchsorted(bc.band_table(table, NF), np.arange(NF), side="right") - 1).to(dev)
                    chunk = max(1, min(NF, (opt.chunk_mb << 20) // (G * C * csize)))
                    t_comp = timed(lambda: composition(s, freq_d, tau, band_id, nb, chunk), dev, 1, opt.baseline_reps)
                    ref = composition(s, freq_d, tau, band_id, nb, chunk)
                    dev_err = float((power.double() - ref.double()).abs().max() / ref.double().abs().max())
                    pad = lambda v: -(-v // 16) * 16  # noqa: E731
                    formed, useful, sec = 8.0 * pad(C) ** 2 * pad(G) * NF, 8.0 * C * C * G * NF, t[0] * 1e-3
                    rate = f"formed {formed / sec / 1e12:7.2f} TF" + (f" = {100 * formed / sec / F32_MATRIX_PEAK:5.1f} % of peak" if dtype == torch.float32 else "")
                    lines += [f"{name} C = {C:2d} G = {G:4d} {label:8s}  qi_beam_power {t[0]:9.3f} ms ({t[1]:.3f} .. {t[2]:.3f})   {rate}, "
                              f"useful {useful / sec / 1e12:7.2f} TF   composition ({chunk} bins a chunk) {t_comp[0]:9.3f} ms "
                              f"({t_comp[1]:.3f} .. {t_comp[2]:.3f}) = {t_comp[0] / t[0]:6.2f} x   |d| / max against it {dev_err:.2g}"]
                    print(lines[-1], flush=True)
                    del power, scratch, ref
                torch.cuda.empty_cache()
        lines.append("")
    if not opt.no_deviations:
        lines += ["deviation from the float64 NumPy restatement at the shapes of tests/test_gpu_beam.py (tests/beam_cases.py): power as a fraction of the",
                  "shape's largest power, semblance absolute; the bounds are 1e-4 (float32) and 1e-10 (float64)"]
        for dtype in bc.DTYPES:
            worst = [0.0, 0.0]
            for shape in bc.SHAPES:
                s, fr, tau = bc.inputs(shape, dtype)
                bands = None if shape.bands is None else list(shape.bands)
                for k, normalize in enumerate((False, True)):
                    ref = bc.restate(s, fr, tau, bands, normalize)
                    got = engine.beam_power(s, fr, tau, bands=bands, normalize=normalize).astype(np.float64)
                    worst[k] = max(worst[k], float(np.abs(got - ref).max() / (1.0 if normalize else np.abs(ref).max())))
            lines.append(f"  {dtype}: power {worst[0]:.3g}, semblance {worst[1]:.3g}")
        lines.append(f"  the float32 NumPy restatement itself (CPU): {bc.BEAM32_RESTATEMENT:g}")
    with open(opt.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(opt.out)


if __name__ == "__main__":
    main()
