"""Device time of qi_csd and of its contraction (qi_cross_spectra) alone.  2, 16 and 64 records of 2^20 samples, segments and
transforms of 2048 points at half overlap (1023 segments, 1025 bins), float32 and float64; timed with device events after
warm-up, median of 20 calls.  Per shape: qi_csd whole (csd and coherence), the contraction alone on a stored panel with its
FLOP rate (8 real multiply-adds per complex product, the pairs i <= j the kernel forms, and all C^2 pairs) as a fraction of
the 157 TF float32 matrix peak, and the panel's bytes over its time against 8 TB/s; beside it the PyTorch composition
stft_complex_pow2 -> torch.einsum, whole and the einsum alone.  Appends the float32 coherence tolerance's provenance
(tests/csd_cases.py).  Nothing here is gated: the numbers are recorded.

    python tools/csd_bench.py [--out profiles/csd_kernel.txt] [--records 2 16 64] [--log2n 20] [--reps 20]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from quantum_inferno_amd import _lib, engine, styx_fft  # noqa: E402

import csd_cases as cc  # noqa: E402

F32_MATRIX_PEAK = 157.3e12  # FLOP per second
HBM_PEAK = 8.0e12  # bytes per second
FS, SEG, HOP, NFFT, ALPHA = 800.0, 2048, 1024, 2048, 0.25


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "csd_kernel.txt"))
    ap.add_argument("--records", type=int, nargs="+", default=[2, 16, 64])
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--reps", type=int, default=20)
    opt = ap.parse_args()
    lib = _lib.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    n, n_f = 1 << opt.log2n, NFFT // 2 + 1
    n_seg = (n - SEG) // HOP + 1
    lines = [f"qi_csd / qi_cross_spectra on {torch.cuda.get_device_name(dev)}: records of 2^{opt.log2n} samples, seg = nfft = {NFFT}, hop {HOP}: "
             f"{n_seg} segments x {n_f} bins; median (min .. max) of {opt.reps} calls, device events",
             "contraction FLOP = 8 per complex product and segment: 'formed' counts the pairs i <= j of the 16 x 16 tiles on and above the",
             "diagonal (what the kernel multiplies, padding included), 'useful' all C^2 pairs; peak = 157.3 TF (float32 matrix pipe), 8 TB/s", ""]
    for dtype in (torch.float32, torch.float64):
        for C in opt.records:
            rng = np.random.default_rng([7, C])
            x = torch.from_numpy(rng.standard_normal((C, n)).astype(np.float32)).to(dev).to(dtype)
            code, esz = _lib.dtype_code(dtype), (4 if dtype == torch.float32 else 8)
            win = styx_fft._run_window(styx_fft.tukey_window_periodic(SEG, ALPHA), dtype)
            scale = float(1.0 / np.sum(win.astype(np.float64)))
            win_d = torch.from_numpy(win).to(dev)
            csd = torch.empty((n_f, C, C), dtype=engine._complex_of(dtype), device=dev)
            coh = torch.empty((n_f, C, C), dtype=dtype, device=dev)
            scratch, nbytes = _lib.scratch(lib.qi_csd_scratch_bytes, dev, code, C, n, SEG, HOP, NFFT)

            def whole():
                _lib.call(lib.qi_csd, dev, code, dev.index, _lib.ptr(x), C, n, _lib.ptr(win_d), SEG, HOP, NFFT, scale, _lib.ptr(csd),
                          _lib.ptr(coh), _lib.ptr(scratch), nbytes)

            t_whole = timed(whole, dev, 3, opt.reps)
            del scratch
            # the contraction alone, on a stored panel of the same shape (Welch segments: the STFT panel cut to n_seg columns)
            _, _, z = styx_fft.stft_complex_pow2(x, FS, SEG, SEG - HOP, NFFT, ALPHA)
            z = z[:, :, :n_seg].contiguous()
            s2, n2 = _lib.scratch(lib.qi_cross_spectra_scratch_bytes, dev, code, C, n_f, n_seg)

            def contraction():
                _lib.call(lib.qi_cross_spectra, dev, code, dev.index, _lib.ptr(z), C, n_f, n_seg, None, _lib.ptr(csd), None, _lib.ptr(s2), n2)

            t_con = timed(contraction, dev, 3, opt.reps)
            tiles = -(-C // 16)
            formed = 8.0 * 256 * (tiles * (tiles + 1) // 2) * n_f * n_seg
            useful = 8.0 * C * C * n_f * n_seg
            panel_bytes = 2.0 * esz * C * n_f * n_seg
            sec = t_con[0] * 1e-3

            def composition():
                _, _, zz = styx_fft.stft_complex_pow2(x, FS, SEG, SEG - HOP, NFFT, ALPHA)
                return torch.einsum("ifs,jfs->fij", zz.conj(), zz)

            def einsum_alone():
                return torch.einsum("ifs,jfs->fij", z.conj(), z)

            t_comp = timed(composition, dev, 2, opt.reps)
            t_ein = timed(einsum_alone, dev, 2, opt.reps)
            name = "float32" if dtype == torch.float32 else "float64"
            lines += [f"{name} C = {C}",
                      f"  qi_csd (csd + coherence)        {t_whole[0]:9.3f} ms ({t_whole[1]:.3f} .. {t_whole[2]:.3f})",
                      f"  qi_cross_spectra alone          {t_con[0]:9.3f} ms ({t_con[1]:.3f} .. {t_con[2]:.3f})   "
                      f"formed {formed / sec / 1e12:7.2f} TF = {100 * formed / sec / F32_MATRIX_PEAK:5.1f} % of peak, useful {useful / sec / 1e12:7.2f} TF; "
                      f"panel {panel_bytes / 1e6:.1f} MB at {panel_bytes / sec / 1e12:.3f} TB/s = {100 * panel_bytes / sec / HBM_PEAK:5.1f} % of 8 TB/s",
                      f"  stft_complex_pow2 + torch.einsum {t_comp[0]:8.3f} ms ({t_comp[1]:.3f} .. {t_comp[2]:.3f})",
                      f"  torch.einsum alone              {t_ein[0]:9.3f} ms ({t_ein[1]:.3f} .. {t_ein[2]:.3f})", ""]
            print("\n".join(lines[-6:]), flush=True)
            del z, s2, csd, coh, x
            torch.cuda.empty_cache()
    lines += ["float32 coherence tolerance of tests/test_gpu_csd.py (tests/csd_cases.py, computed by NumPy on the CPU):",
              f"  largest deviation of the float32 restatement's coherence from the SciPy fixture over all cases: measured 5.839e-07, "
              f"constant {cc.COH32_RESTATEMENT:g}",
              f"  x 16 (a float32 FFT rounds once per stage, the restatement once) = {cc.COH32_TOL:.4g}; the cap derived from the contract is 4e-2"]
    with open(opt.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(opt.out)


if __name__ == "__main__":
    main()
