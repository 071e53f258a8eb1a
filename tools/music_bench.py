"""Device time of qi_csd_eigh and qi_beam_music.  1025 matrices (the bins of tools/csd_bench.py's shape) of C = 4, 16, 64
sensors over grids of 1024 and 4096 delay sets, every matrix its own band, float32 and float64; timed with device events after
warm-up, median (min .. max) of 20 calls.  Per shape: the eigen-solver alone beside torch.linalg.eigh on the same stack, the
form alone (power and peaks) with qi_beam_capon's calls (on qi_csd_whiten's factors of the same matrices) alternating in the
same loop, and the two calls together against the PyTorch composition: torch.linalg.eigh, the steering tensor
exp(2 pi i f tau) [bins, G, C] in chunks of bins that keep it below --chunk-mb, a batched matrix product with the noise columns,
the squared modulus, the sum and the quotient; timed over fewer calls (--baseline-reps).  The matrices are Z Z^H / 2C of complex
noise plus two plane waves of 30 times the noise power: n_sources = min(2, C - 1).  Appends the deviations of
tests/test_gpu_music.py's shapes from the NumPy restatements.  Nothing here is gated: the numbers are recorded.

    python tools/music_bench.py [--out profiles/music_kernel.txt] [--sensors 4 16 64] [--grid 1024 4096] [--reps 20]"""
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
import music_cases as mc  # noqa: E402

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


def composition(s, k, freq_d, tau, chunk):
    """The same power in PyTorch, every matrix its own band (the phase in double in both precisions)."""
    C = s.shape[1]
    _, u = torch.linalg.eigh(s)
    noise = u[:, :, :C - k]
    out = torch.empty((s.shape[0], tau.shape[0]), dtype=torch.float64, device=s.device)
    for f0 in range(0, s.shape[0], chunk):
        f1 = min(f0 + chunk, s.shape[0])
        turns = freq_d[f0:f1, None, None] * tau[None, :, :]
        e = torch.polar(torch.ones_like(turns), 2 * np.pi * (turns - torch.round(turns))).to(s.dtype)  # [bins, G, C]
        w = torch.bmm(e, noise[f0:f1].conj())  # [bins, G, m]: conj of U_j^H e
        out[f0:f1] = C / (w.real * w.real + w.imag * w.imag).sum(dim=-1).double()
    return out


def fmt(t):
    return f"{t[0]:9.3f} ms ({t[1]:.3f} .. {t[2]:.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "music_kernel.txt"))
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
    lines = [f"python tools/music_bench.py --sensors {' '.join(map(str, opt.sensors))} --grid {' '.join(map(str, opt.grid))} --reps {opt.reps} "
             f"--baseline-reps {opt.baseline_reps} --chunk-mb {opt.chunk_mb}",
             f"qi_csd_eigh and qi_beam_music on {torch.cuda.get_device_name(dev)}: {NF} matrices, every matrix its own band, n_sources = "
             f"min(2, C - 1), delays uniform in +-{bc.MAX_DELAY_S} s;",
             f"median (min .. max) of {opt.reps} calls (torch.linalg.eigh and the composition: {opt.baseline_reps}), device events; qi_beam_music and "
             "qi_beam_capon (both with the peaks) alternate in one loop.",
             "The composition: torch.linalg.eigh, the steering tensor [bins, G, C] in chunks of at most "
             f"{opt.chunk_mb} MB, torch.bmm with the noise columns, |.|^2, a sum, the quotient", ""]
    for dtype in (torch.float32, torch.float64):
        name = "float32" if dtype == torch.float32 else "float64"
        code, csize = _lib.dtype_code(dtype), (8 if dtype == torch.float32 else 16)
        for C in opt.sensors:
            k = min(2, C - 1)
            rng = np.random.default_rng([17, C])
            z = rng.standard_normal((NF, C, 2 * C)) + 1j * rng.standard_normal((NF, C, 2 * C))
            a = np.exp(2j * np.pi * rng.uniform(0, 1, (NF, C, k)))  # the sources' steering vectors
            s_host = np.einsum("fis,fjs->fij", np.conj(z), z) / (2 * C) + 30.0 * np.einsum("fik,fjk->fij", a, np.conj(a))
            s = torch.from_numpy(s_host).to(dev).to(engine._complex_of(dtype))
            w = torch.empty((NF, C), dtype=dtype, device=dev)
            u, v = torch.empty_like(s), torch.empty_like(s)
            info = torch.empty(NF, dtype=torch.int32, device=dev)

            def eigh():
                _lib.call(lib.qi_csd_eigh, dev, code, dev.index, _lib.ptr(s), C, NF, _lib.ptr(w), _lib.ptr(u), _lib.ptr(info))

            t_e = timed([eigh], dev, 3, opt.reps)[0]
            assert not bool(info.any())
            t_t = timed([lambda: torch.linalg.eigh(s)], dev, 1, opt.baseline_reps)[0]
            w_ref = torch.linalg.eigh(s)[0]
            err_w = float((w.double() - w_ref.double()).abs().max() / w_ref.abs().max())
            lines += [f"{name} C = {C:2d}  qi_csd_eigh {fmt(t_e)}  torch.linalg.eigh {fmt(t_t)} = {t_t[0] / t_e[0]:7.2f} x qi_csd_eigh   "
                      f"|d eigenvalues| / max against torch {err_w:.2g}"]
            print(lines[-1], flush=True)
            _lib.call(lib.qi_csd_whiten, dev, code, dev.index, _lib.ptr(s), C, NF, cpc.LOADING, _lib.ptr(v), _lib.ptr(info))
            for G in opt.grid:
                tau = torch.from_numpy(rng.uniform(-bc.MAX_DELAY_S, bc.MAX_DELAY_S, (G, C))).to(dev)
                power, other = torch.empty((NF, G), dtype=dtype, device=dev), torch.empty((NF, G), dtype=dtype, device=dev)
                index = torch.empty(NF, dtype=torch.int64, device=dev)
                value = torch.empty(NF, dtype=dtype, device=dev)
                scratch, nbytes = _lib.scratch(lib.qi_beam_music_scratch_bytes, dev, code, C, NF, G, NF)

                def music():
                    _lib.call(lib.qi_beam_music, dev, code, dev.index, _lib.ptr(u), C, NF, k, f_ptr, _lib.ptr(tau), G, None, NF,
                              _lib.ptr(power), _lib.ptr(index), _lib.ptr(value), _lib.ptr(scratch), nbytes)

                def capon():
                    _lib.call(lib.qi_beam_capon, dev, code, dev.index, _lib.ptr(v), C, NF, f_ptr, _lib.ptr(tau), G, None, NF,
                              _lib.ptr(other), _lib.ptr(index), _lib.ptr(value), _lib.ptr(scratch), nbytes)

                t_m, t_c = timed([music, capon], dev, 3, opt.reps)
                chunk = max(1, min(NF, (opt.chunk_mb << 20) // (G * C * csize)))
                t_comp = timed([lambda: composition(s, k, freq_d, tau, chunk)], dev, 1, opt.baseline_reps)[0]
                ref = composition(s, k, freq_d, tau, chunk)
                music()
                dev_err = float((1.0 / power.double() - 1.0 / ref).abs().max())
                both = t_e[0] + t_m[0]
                lines += [f"{name} C = {C:2d} G = {G:4d}  qi_beam_music {fmt(t_m)}  qi_beam_capon {fmt(t_c)}: MUSIC form / Capon form {t_m[0] / t_c[0]:5.2f}   "
                          f"composition ({chunk} bins a chunk) {fmt(t_comp)} = {t_comp[0] / both:6.2f} x the two calls   "
                          f"solver's share of the two calls {100 * t_e[0] / both:5.1f} %   |d 1 / power| against the composition {dev_err:.2g}"]
                print(lines[-1], flush=True)
                del power, other, scratch, ref
            torch.cuda.empty_cache()
        lines.append("")
    if not opt.no_deviations:
        lines += ["deviation from the float64 NumPy restatements at the shapes of tests/test_gpu_music.py (tests/music_cases.py): the eigenvalues as a",
                  "fraction of the largest, max |U^H U - I|, max |S U - U w| / max w, the noise projector, 1 / power fed the restated eigenvectors and",
                  "end to end; the bounds are 1e-4 (float32) and 1e-10 (float64)"]
        for dtype in bc.DTYPES:
            worst = [0.0] * 6
            for shape in bc.SHAPES:
                s, fr, tau, k = mc.inputs(shape, dtype)
                bands = None if shape.bands is None else list(shape.bands)
                w64, u64 = mc.eigh64(s)
                ref = 1.0 / mc.music(u64, k, fr, tau, bands)
                w, u = engine.csd_eigh(s)
                fed = engine.music_power(u64.astype(s.dtype), k, fr, tau, bands=bands).astype(np.float64)
                got = engine.music_power(u, k, fr, tau, bands=bands).astype(np.float64)
                ortho, pairs = mc.residuals(w, u, s)
                now = (float(np.abs(w - w64).max() / np.abs(w64).max()), ortho, pairs, float(np.abs(mc.noise_projector(u, k) - mc.noise_projector(u64, k)).max()),
                       float(np.abs(1.0 / fed - ref).max()), float(np.abs(1.0 / got - ref).max()))
                worst = [max(a, b) for a, b in zip(worst, now)]
            lines.append(f"  {dtype}: eigenvalues {worst[0]:.3g}, orthogonality {worst[1]:.3g}, pairs {worst[2]:.3g}, projector {worst[3]:.3g}, "
                         f"1 / power fed {worst[4]:.3g}, end to end {worst[5]:.3g}")
        lines.append(f"  the float32 NumPy restatements themselves (CPU): eigenvalues {mc.EIGH32_VALUES:g}, projector {mc.EIGH32_PROJECTOR:g}, "
                     f"1 / power {mc.MUSIC32_RECIPROCAL:g}")
    with open(opt.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(opt.out)


if __name__ == "__main__":
    main()
