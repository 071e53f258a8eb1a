"""Device time of qi_beam_steer and qi_beam_weights.  A panel of 1025 bins x 1023 segments (tools/csd_bench.py's shape) of
C = 4, 16, 64 records, nbeam = 1, 16, 64 beams, float32 and float64; timed with device events after warm-up, median
(min .. max) of 20 calls.  qi_beam_steer: the time, the bytes the call must move (the panel read once, the beams written) per
second against the 8 TB/s HBM peak, and torch.einsum("fki,ift->kft") on the same tensors (fewer calls: --baseline-reps).
qi_beam_weights: the time with whiteners (MVDR; qi_csd_whiten's factors of Z Z^H / 2C of complex noise) and without (Bartlett),
and the PyTorch composition of the MVDR weights: the steering tensor exp(2 pi i f tau) [bins, nbeam, C] with the phase in
double, two torch.bmm, the sum of squares and the division.  Appends the deviations of tests/test_gpu_steer.py's shapes from
the NumPy restatements.  Nothing here is gated: the numbers are recorded.

    python tools/steer_bench.py [--out profiles/steer_kernel.txt] [--sensors 4 16 64] [--beams 1 16 64] [--reps 20]"""
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
import steer_cases as stc  # noqa: E402

NF, NT, FS, NFFT = 1025, 1023, 800.0, 2048
HBM_PEAK = 8.0e12  # bytes per second


def event_ms(call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def timed(call, dev, warmup, reps):
    for _ in range(warmup):
        call()
    torch.cuda.synchronize(dev)
    ms = [event_ms(call) for _ in range(reps)]
    return float(np.median(ms)), min(ms), max(ms)


def mvdr_composition(v, freq_d, tau):
    """The MVDR weights in PyTorch (the phase in double in both precisions)."""
    turns = freq_d[:, None, None] * tau[None, :, :]
    e = torch.polar(torch.ones_like(turns), 2 * np.pi * (turns - torch.round(turns))).to(v.dtype)  # [bins, nbeam, C]
    u = torch.bmm(e, v.conj())  # [bins, nbeam, C]: u_j = sum_i conj(V_ij) e_i
    d = (u.real * u.real + u.imag * u.imag).sum(dim=-1, keepdim=True)
    return torch.bmm(u, v.transpose(1, 2)) / d  # a_i = sum_j V_ij u_j / D


def fmt(t):
    return f"{t[0]:8.3f} ms ({t[1]:.3f} .. {t[2]:.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "steer_kernel.txt"))
    ap.add_argument("--sensors", type=int, nargs="+", default=[4, 16, 64])
    ap.add_argument("--beams", type=int, nargs="+", default=[1, 16, 64])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--baseline-reps", type=int, default=5)
    ap.add_argument("--no-deviations", action="store_true")
    opt = ap.parse_args()
    lib = _lib.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    freq = np.fft.rfftfreq(NFFT, 1 / FS)
    assert len(freq) == NF
    freq_d = torch.from_numpy(freq).to(dev)
    f_host, f_ptr = _lib.darr(freq)
    lines = [f"python tools/steer_bench.py --sensors {' '.join(map(str, opt.sensors))} --beams {' '.join(map(str, opt.beams))} --reps {opt.reps} "
             f"--baseline-reps {opt.baseline_reps}",
             f"qi_beam_steer and qi_beam_weights on {torch.cuda.get_device_name(dev)}: a panel of {NF} bins x {NT} segments, delays uniform in "
             f"+-{bc.MAX_DELAY_S} s;",
             f"median (min .. max) of {opt.reps} calls (torch.einsum and the composition: {opt.baseline_reps}), device events.",
             f"required bytes: the panel read once and the beams written; the HBM peak is {HBM_PEAK / 1e12:g} TB/s.",
             "The weights' composition: the steering tensor [bins, nbeam, C] (phase in double), torch.bmm with conj(V), |.|^2 and a sum, "
             "torch.bmm with V^T, the division", ""]
    torch.manual_seed(41)
    for dtype in (torch.float32, torch.float64):
        name = "float32" if dtype == torch.float32 else "float64"
        ctype = engine._complex_of(dtype)
        code, csize = _lib.dtype_code(dtype), (8 if dtype == torch.float32 else 16)
        for C in opt.sensors:
            rng = np.random.default_rng([41, C])
            z = torch.view_as_complex(torch.randn((C, NF, NT, 2), dtype=dtype, device=dev))
            n = rng.standard_normal((NF, C, 2 * C)) + 1j * rng.standard_normal((NF, C, 2 * C))
            s = torch.from_numpy(np.einsum("fis,fjs->fij", np.conj(n), n) / (2 * C)).to(dev).to(ctype)
            v = torch.empty_like(s)
            info = torch.empty(NF, dtype=torch.int32, device=dev)
            _lib.call(lib.qi_csd_whiten, dev, code, dev.index, _lib.ptr(s), C, NF, cpc.LOADING, _lib.ptr(v), _lib.ptr(info))
            assert not bool(info.any())
            for K in opt.beams:
                tau = torch.from_numpy(rng.uniform(-bc.MAX_DELAY_S, bc.MAX_DELAY_S, (K, C))).to(dev)
                w = torch.empty((NF, K, C), dtype=ctype, device=dev)
                wb = torch.empty_like(w)
                out = torch.empty((K, NF, NT), dtype=ctype, device=dev)
                scratch, nbytes = _lib.scratch(lib.qi_beam_weights_scratch_bytes, dev, code, C, NF, K)

                def mvdr():
                    _lib.call(lib.qi_beam_weights, dev, code, dev.index, _lib.ptr(v), C, NF, f_ptr, _lib.ptr(tau), K, _lib.ptr(w),
                              _lib.ptr(scratch), nbytes)

                def bartlett():
                    _lib.call(lib.qi_beam_weights, dev, code, dev.index, None, C, NF, f_ptr, _lib.ptr(tau), K, _lib.ptr(wb), _lib.ptr(scratch),
                              nbytes)

                def steer():
                    _lib.call(lib.qi_beam_steer, dev, code, dev.index, _lib.ptr(z), C, NF, NT, _lib.ptr(w), K, _lib.ptr(out))

                t_m, t_b = timed(mvdr, dev, 3, opt.reps), timed(bartlett, dev, 3, opt.reps)
                t_comp = timed(lambda: mvdr_composition(v, freq_d, tau), dev, 1, opt.baseline_reps)
                ref_w = mvdr_composition(v, freq_d, tau)
                err_w = float((w.to(torch.complex128) - ref_w.to(torch.complex128)).abs().max() / ref_w.abs().max())
                t_s = timed(steer, dev, 3, opt.reps)
                t_e = timed(lambda: torch.einsum("fki,ift->kft", w, z), dev, 1, opt.baseline_reps)
                ref = torch.einsum("fki,ift->kft", w, z)
                err_s = float((out - ref).abs().max() / ref.abs().max())
                need = (C + K) * NF * NT * csize
                rate = need / (t_s[0] * 1e-3)
                lines += [f"{name} C = {C:2d} nbeam = {K:2d}  qi_beam_steer {fmt(t_s)}  {need / 1e6:7.1f} MB required = {rate / 1e12:5.2f} TB/s "
                          f"({100 * rate / HBM_PEAK:4.1f} % of the peak)   torch.einsum {fmt(t_e)} = {t_e[0] / t_s[0]:6.2f} x qi_beam_steer   "
                          f"|d beams| / max against einsum {err_s:.2g}",
                          f"{name} C = {C:2d} nbeam = {K:2d}  qi_beam_weights MVDR {fmt(t_m)}  Bartlett {fmt(t_b)}   composition {fmt(t_comp)} = "
                          f"{t_comp[0] / t_m[0]:6.2f} x the MVDR call   |d weights| / max against the composition {err_w:.2g}"]
                print(lines[-2], flush=True)
                print(lines[-1], flush=True)
                del w, wb, out, ref, ref_w
            del z, s, v
            torch.cuda.empty_cache()
        lines.append("")
    if not opt.no_deviations:
        lines += ["deviation from the float64 NumPy restatements at the shapes of tests/test_gpu_steer.py (tests/steer_cases.py), of the case's largest",
                  "modulus: the MVDR weights, the Bartlett weights, the MVDR beams end to end, the Bartlett beams; max |e^H a - 1| and",
                  "max |a^H R a D - 1|; the bounds are 1e-4 (float32) and 1e-10 (float64)"]
        for dtype in bc.DTYPES:
            worst = [0.0] * 6
            for shape in stc.SHAPES:
                s, fr, tau, z = stc.inputs(shape, dtype)
                v = stc.whiteners(shape, dtype).astype(bc.complex_of(dtype))
                ref_a, ref_b = stc.weights(fr, tau, v), stc.weights(fr, tau)
                a, b = engine.beam_weights(fr, tau, whitener=v), engine.beam_weights(fr, tau, dtype=dtype)
                y, yb = engine.beam_steer(z, a), engine.beam_steer(z, b)
                ref_y, ref_yb = stc.steer(z, ref_a), stc.steer(z, ref_b)
                now = (float(np.abs(a - ref_a).max() / np.abs(ref_a).max()), float(np.abs(b - ref_b).max() / np.abs(ref_b).max()),
                       float(np.abs(y - ref_y).max() / np.abs(ref_y).max()), float(np.abs(yb - ref_yb).max() / np.abs(ref_yb).max()),
                       float(np.abs(stc.gain(fr, tau, a) - 1).max()),
                       float(np.abs(stc.output_power(a, cpc.loaded(s, stc.LOADING, dtype)) / cpc.capon(v, fr, tau) - 1).max()))
                worst = [max(p, q) for p, q in zip(worst, now)]
            lines.append(f"  {dtype}: MVDR weights {worst[0]:.3g}, Bartlett weights {worst[1]:.3g}, MVDR beams {worst[2]:.3g}, Bartlett beams {worst[3]:.3g}, "
                         f"|e^H a - 1| {worst[4]:.3g}, |a^H R a D - 1| {worst[5]:.3g}")
        lines.append(f"  the float32 NumPy restatements themselves (CPU): MVDR weights {stc.MVDR32_WEIGHTS:g}, MVDR beams {stc.MVDR32_BEAMS:g}, "
                     f"Bartlett beams {stc.BARTLETT32_BEAMS:g}")
    with open(opt.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(opt.out)


if __name__ == "__main__":
    main()
