#!/usr/bin/env python3
"""Time the STFT's reduced product on an MI355X at the BASELINE configs[2] STFT shape (64 x 2^20 samples, order 12, float32:
2048-sample segments, a 64 x 1025 x 1025 panel) and at 4 x 2^20 float64:

    (run)  StftPlan.run: both panels stored, no reductions (the reference point)
    (a)    the same product without qi_stft_out: StftPlan.run, power_scale |Z|^2 as a PyTorch expression, qi_power_marginals
    (b)    StftPlan.reduce(coef=False, bits=False): the reductions from the transform kernel, no panel
    (c)    StftPlan.reduce(coef=True, bits=True): both panels and the reductions

    python tools/stft_reduced_bench.py [--out profiles/stft_reduced.txt] [--reps 15]

The four alternate call by call in one process; each call is timed by a pair of events after three warm-up calls of each,
and the median of the repeats is reported with the lowest and the highest.  The bytes are those each form has to move (the
record once, the panels it stores, its partial sums); nothing is asserted about the times."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from quantum_inferno_amd import _lib, styx_fft  # noqa: E402

SHAPES = [(64, 1 << 20, 12, torch.float32), (4, 1 << 20, 12, torch.float64)]
FS, POWER_SCALE = 1000.0, 2.0


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def marginals_of(lib, plan, power, band, time, stats, scratch):
    with torch.cuda.device(plan.device):
        _lib.check(lib.qi_power_marginals(plan.code, plan.device.index, _lib.ptr(power), plan.channels, plan.n_f, plan.n_seg,
                                          _lib.ptr(band), _lib.ptr(time), _lib.ptr(stats), _lib.ptr(scratch), scratch.numel(),
                                          _lib.stream_ptr(plan.device)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "stft_reduced.txt"))
    ap.add_argument("--reps", type=int, default=15)
    a = ap.parse_args()
    lib = _lib.require_gpu()
    lines = [f"reduced product of the STFT, {torch.cuda.get_device_name(0)}; median (min .. max) of {a.reps} calls in ms, the four "
             "forms alternating call by call in one process"]
    for channels, n, order, rdt in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(7)
        x = torch.randn((channels, n), generator=g, dtype=rdt, device="cuda")
        plan = styx_fft.StftPlan(n, channels, FS, order, rdt)
        e = 4 if rdt == torch.float32 else 8
        cells = channels * plan.n_f * plan.n_seg
        # segment groups per record, from the partial sums' share of the scratch ([C][groups][n_f] + [C][groups][3] doubles)
        groups = int(lib.qi_stft_out_scratch_bytes(plan.code, channels, n, plan.seg, plan.hop, plan.nfft, 1, 1)
                     - lib.qi_stft_scratch_bytes(plan.code, channels, n, plan.seg, plan.hop, plan.nfft)) // (channels * (plan.n_f + 3) * 8)
        band = torch.empty((channels, plan.n_f), dtype=torch.float64, device="cuda")
        time_ = torch.empty((channels, plan.n_seg), dtype=rdt, device="cuda")
        stats = torch.empty((channels, 4), dtype=torch.float64, device="cuda")
        mscratch = torch.empty(int(lib.qi_power_marginals_scratch_bytes(channels, plan.n_f, plan.n_seg)), dtype=torch.uint8, device="cuda")

        def form_run():
            return plan.run(x)

        def form_a():
            z, _ = plan.run(x)
            power = POWER_SCALE * (z.real ** 2 + z.imag ** 2)
            marginals_of(lib, plan, power, band, time_, stats, mscratch)
            return band, time_, stats

        def form_b():
            return plan.reduce(x, coef=False, bits=False, power_scale=POWER_SCALE)

        def form_c():
            return plan.reduce(x, coef=True, bits=True, power_scale=POWER_SCALE)

        forms = (("run", form_run), ("a", form_a), ("b", form_b), ("c", form_c))
        for _ in range(3):
            for _, fn in forms:
                fn()
        torch.cuda.synchronize()
        # the forms agree: (b) against (a), (c)'s panels against run's
        ref_band, ref_time, ref_stats = (v.clone() for v in form_a())
        res = form_b()
        err = max(float((res.power_band - ref_band).abs().max() / ref_band.abs().max()),
                  float((res.power_time.double() - ref_time.double()).abs().max() / ref_time.double().abs().max()),
                  float(((res.stats - ref_stats).abs()[:, :2] / ref_stats[:, :2]).max()))
        z0, b0 = (v.clone() for v in form_run())
        full = form_c()
        same = bool(torch.equal(full.coef, z0) and torch.equal(full.bits, b0))
        times = {name: [] for name, _ in forms}
        for _ in range(a.reps):
            for name, fn in forms:
                times[name].append(timed(fn)[0])
        record, panels, partials = channels * n * e, cells * 3 * e, channels * groups * (plan.n_f + 3) * 8
        nbytes = {"run": record + panels, "a": record + panels + cells * (2 * e + e + e), "b": record + partials,
                  "c": record + panels + partials}
        lines.append(f"[{channels} x {n}] {str(rdt)[6:]}, order {order}: {plan.seg}-sample segments, panel [{channels}, {plan.n_f}, "
                     f"{plan.n_seg}], {groups} segment groups per record")
        for name, _ in forms:
            t = times[name]
            med = statistics.median(t)
            lines.append(f"  ({name:3s}) {med:8.3f} ms ({min(t):.3f} .. {max(t):.3f})   {nbytes[name] / 1e6:9.1f} MB to move = "
                         f"{nbytes[name] / med / 1e6:6.0f} GB/s")
        mr, mb, mc = (statistics.median(times[k]) for k in ("run", "b", "c"))
        lines.append(f"  (b) / run = {mb / mr:.3f}; (c) - run = {mc - mr:+.3f} ms for {partials / 1e6:.2f} MB of partial sums and the tail "
                     f"launch; (a) / (b) = {statistics.median(times['a']) / mb:.2f}")
        lines.append(f"  (b) against (a): largest relative difference of the marginals, max P and sum P {err:.1e}; (c)'s panels equal to "
                     f"run's bit for bit: {same}")
        del plan, x
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
