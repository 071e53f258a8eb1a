"""Device time of qi_csd_whiten and qi_beam_capon.  1025 matrices (the bins of tools/csd_bench.py's shape) of C = 4, 16, 64
sensors over grids of 1024 and 4096 delay sets, every matrix its own band, float32 and float64; timed with device events after
warm-up, median (min .. max) of 20 calls.  Per shape: the factorisation alone, the form alone (power and peaks), and two
yardsticks.  The first is qi_beam_power (power and peaks) on the same shape, its calls alternating with the form's in the same
loop: the Capon form multiplies 10 of the Bartlett form's 16 tile products at 64 sensors and has no closing product.  The
second is the PyTorch composition: torch.linalg.cholesky of the loaded matrices, torch.linalg.solve_triangular for L^-1, the
steering tensor exp(2 pi i f tau) [bins, G, C] in chunks of bins that keep it below --chunk-mb, a batched matrix product, the
squared modulus, the sum, the reciprocal and index_add_; timed over fewer calls (--baseline-reps).  Printed beside them: the
ratios, and the factorisation's share of the two calls together at the smaller grid.  Appends the deviations of
tests/test_gpu_capon.py's shapes from the NumPy restatements.  Nothing here is gated: the numbers are recorded.

    python tools/capon_bench.py [--out profiles/capon_kernel.txt] [--sensors 4 16 64] [--grid 1024 4096] [--reps 20]"""
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
import capon_cases as cpc  # noqa: E402

NF, FS, NFFT = 1025, 800.0, 2048


def event_ms(call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def timed(calls, dev, warmup, reps):
    """The calls alternate inside every repeat -> per call (median, min, max) ms."""
    for _ in range(warmup):
        for call in calls:
            call()
    torch.cuda.synchronize(dev)
    ms = [[] for _ in calls]
    for _ in range(reps):
        for k, call in enumerate(calls):
            ms[k].append(event_ms(call))
    return [(float(np.median(m)), min(m), max(m)) for m in ms]


def composition(s, loading, freq_d, tau, band_id, nb, chunk):
    """The same power in PyTorch (the phase in double in both precisions: float32 would lose it)."""
    C = s.shape[1]
    load = loading * torch.diagonal(s, dim1=1, dim2=2).real.mean(dim=1)
    r = s + load[:, None, None] * torch.eye(C, dtype=s.dtype, device=s.device)
    low = torch.linalg.cholesky(r)
    winv = torch.linalg.solve_triangular(low, torch.eye(C, dtype=s.dtype, device=s.device).expand_as(low), upper=False)  # L^-1 = V^H
    out = torch.zeros((nb, tau.shape[0]), dtype=torch.float64, device=s.device)
    for f0 in range(0, s.shape[0], chunk):
        f1 = min(f0 + chunk, s.shape[0])
        turns = freq_d[f0:f1, None, None] * tau[None, :, :]
        e = torch.polar(torch.ones_like(turns), 2 * np.pi * (turns - torch.round(turns))).to(s.dtype)  # [bins, G, C]
        w = torch.bmm(e, winv[f0:f1].transpose(1, 2))  # [bins, G, C]: (L^-1 e)_j
        d = (w.real * w.real + w.imag * w.imag).sum(dim=-1)
        out.index_add_(0, band_id[f0:f1], 1.0 / d.double())
    return out


def fmt(t):
    return f"{t[0]:9.3f} ms ({t[1]:.3f} .. {t[2]:.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "capon_kernel.txt"))
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
    band_id = torch.arange(NF, device=dev)
    lines = [f"python tools/capon_bench.py --sensors {' '.join(map(str, opt.sensors))} --grid {' '.join(map(str, opt.grid))} --reps {opt.reps} "
             f"--baseline-reps {opt.baseline_reps} --chunk-mb {opt.chunk_mb}",
             f"qi_csd_whiten and qi_beam_capon on {torch.cuda.get_device_name(dev)}: {NF} matrices, every matrix its own band, loading "
             f"{cpc.LOADING:g}, delays uniform in +-{bc.MAX_DELAY_S} s;",
             f"median (min .. max) of {opt.reps} calls (the composition: {opt.baseline_reps}), device events; qi_beam_capon and qi_beam_power (both with "
             "the peaks) alternate in one loop.",
             "The composition: torch.linalg.cholesky, solve_triangular, the steering tensor [bins, G, C] in chunks of at most "
             f"{opt.chunk_mb} MB, torch.bmm, |.|^2, a sum, the reciprocal, index_add_", ""]
    for dtype in (torch.float32, torch.float64):
        name = "float32" if dtype == torch.float32 else "float64"
        code, csize = _lib.dtype_code(dtype), (8 if dtype == torch.float32 else 16)
        for C in opt.sensors:
            rng = np.random.default_rng([13, C])
            z = rng.standard_normal((NF, C, 2 * C)) + 1j * rng.standard_normal((NF, C, 2 * C))
            s = torch.from_numpy(np.einsum("fis,fjs->fij", np.conj(z), z) / (2 * C)).to(dev).to(engine._complex_of(dtype))
            v = torch.empty_like(s)
            info = torch.empty(NF, dtype=torch.int32, device=dev)

            def whiten():
                _lib.call(lib.qi_csd_whiten, dev, code, dev.index, _lib.ptr(s), C, NF, cpc.LOADING, _lib.ptr(v), _lib.ptr(info))

            t_w = timed([whiten], dev, 3, opt.reps)[0]
            assert not bool(info.any())
            for G in opt.grid:
                tau = torch.from_numpy(rng.uniform(-bc.MAX_DELAY_S, bc.MAX_DELAY_S, (G, C))).to(dev)
                power, other = torch.empty((NF, G), dtype=dtype, device=dev), torch.empty((NF, G), dtype=dtype, device=dev)
                index = torch.empty(NF, dtype=torch.int64, device=dev)
                value = torch.empty(NF, dtype=dtype, device=dev)
                scratch, nbytes = _lib.scratch(lib.qi_beam_capon_scratch_bytes, dev, code, C, NF, G, NF)

                def capon():
                    _lib.call(lib.qi_beam_capon, dev, code, dev.index, _lib.ptr(v), C, NF, f_ptr, _lib.ptr(tau), G, None, NF,
                              _lib.ptr(power), _lib.ptr(index), _lib.ptr(value), _lib.ptr(scratch), nbytes)

                def bartlett():
                    _lib.call(lib.qi_beam_power, dev, code, dev.index, _lib.ptr(s), C, NF, f_ptr, _lib.ptr(tau), G, None, NF, 0,
                              _lib.ptr(other), _lib.ptr(index), _lib.ptr(value), _lib.ptr(scratch), nbytes)

                t_c, t_b = timed([capon, bartlett], dev, 3, opt.reps)
                chunk = max(1, min(NF, (opt.chunk_mb << 20) // (G * C * csize)))
                t_comp = timed([lambda: composition(s, cpc.LOADING, freq_d, tau, band_id, NF, chunk)], dev, 1, opt.baseline_reps)[0]
                ref = composition(s, cpc.LOADING, freq_d, tau, band_id, NF, chunk)
                dev_err = float((power.double() - ref).abs().max() / ref.abs().max())
                both = t_w[0] + t_c[0]
                lines += [f"{name} C = {C:2d} G = {G:4d}  qi_csd_whiten {fmt(t_w)}  qi_beam_capon {fmt(t_c)}  qi_beam_power {fmt(t_b)}: Capon form / Bartlett "
                          f"{t_c[0] / t_b[0]:5.2f}   composition ({chunk} bins a chunk) {fmt(t_comp)} = {t_comp[0] / both:6.2f} x the two calls   "
                          f"factorisation's share of the two calls {100 * t_w[0] / both:5.1f} %   |d| / max against the composition {dev_err:.2g}"]
                print(lines[-1], flush=True)
                del power, other, scratch, ref
            torch.cuda.empty_cache()
        lines.append("")
    if not opt.no_deviations:
        lines += ["deviation from the float64 NumPy restatements at the shapes of tests/test_gpu_capon.py (tests/capon_cases.py): the whitener as a fraction",
                  "of its largest entry, max |V^H R V - I|, the power as a fraction of the shape's largest; the bounds are 1e-4 (float32) and 1e-10 (float64)"]
        for dtype in bc.DTYPES:
            worst = [0.0, 0.0, 0.0]
            for shape in bc.SHAPES:
                s, fr, tau = cpc.inputs(shape, dtype)
                bands = None if shape.bands is None else list(shape.bands)
                ref_v = cpc.whiten(s, cpc.LOADING, dtype)
                v = engine.csd_whiten(s, loading=cpc.LOADING)
                ref = cpc.capon(ref_v, fr, tau, bands)
                got = engine.capon_power(v, fr, tau, bands=bands).astype(np.float64)
                worst[0] = max(worst[0], float(np.abs(v - ref_v).max() / np.abs(ref_v).max()))
                worst[1] = max(worst[1], cpc.residual(v, cpc.loaded(s, cpc.LOADING, dtype)))
                worst[2] = max(worst[2], float(np.abs(got - ref).max() / np.abs(ref).max()))
            lines.append(f"  {dtype}: whitener {worst[0]:.3g}, residual {worst[1]:.3g}, power {worst[2]:.3g}")
        lines.append(f"  the float32 NumPy restatements themselves (CPU): power {cpc.CAPON32_RESTATEMENT:g}, residual {cpc.WHITEN32_RESIDUAL:g}")
    with open(opt.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(opt.out)


if __name__ == "__main__":
    main()
