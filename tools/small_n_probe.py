#!/usr/bin/env python3
"""Records of 2^10 .. 2^13 samples, one record per call: the small-record engine (AUTO plan) against the hipFFT engine
(a QI_ENGINE_HIPFFT plan: the path these sizes took before the small engine) and, where they can run, against the zoom /
block engines forced by QI_NATIVE_MIN_LOG2N -- for float32 and float64, orders 3 and 12, the styx CWT, the Stockwell
transform and the atoms bank.  The engines alternate inside every repetition (blocks of CALLS calls each); a figure is the
median over ROUNDS repetitions of the per-call time, taken REPEATS times: the median of those medians is printed with their
spread (max - min).  Then the three variants of the joint call (QI_SMALL_JOINT = 0 separate runs, 1 one forward launch,
2 and one tail launch) at 2^10 and 2^13.
usage (GPU box): python tools/small_n_probe.py [--quick]"""
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import quantum_inferno_amd as qi  # noqa: E402
from quantum_inferno_amd import _lib, cwt_atoms, scales_dyadic  # noqa: E402

FS = 1000.0
QUICK = "--quick" in sys.argv
CALLS, ROUNDS, REPEATS = (20, 3, 2) if QUICK else (50, 7, 3)
NAMES = {0: "cwt", 1: "atoms", 2: "stx"}


def atom_tables(n, order):
    _, f_min = cwt_atoms.chirp_scales_from_duration(order, n / FS, 0.0)
    o, _, _, _, f_desc, _, _ = cwt_atoms.chirp_frequency_bands(order, f_min, FS, FS / 2.0, 0.0)
    f = np.flip(f_desc)
    return f, cwt_atoms._atom_tables(o, f, FS, 0.0, scales_dyadic.Slice.G2, "norm")


def make_plan(n, dt, order, engine=_lib.QI_ENGINE_AUTO, env=None):
    """A plan with all three tables; env: development switches in force while the plan is made."""
    for k, v in (env or {}).items():
        os.environ[k] = v
    try:
        f, tabs = atom_tables(n, order)
        nb = max(len(f), len(scales_dyadic.log_frequency_hz_from_fft_points(FS, n, order)))
        plan = qi.TfrPlan(n, dt, "cuda:0", qi.TfrPlan.workspace_for(n, nb, dt, 1), engine)
        plan.set_styx_bank(order, FS)
        plan.set_stx_bands(order, FS)
        plan.set_gabor_bank(1, f, *tabs)
    finally:
        for k in env or {}:
            del os.environ[k]
    return plan


def call(plan, which, x, out=None):
    return {0: plan.cwt, 1: plan.cwt_atoms, 2: plan.stx}[which](x, coef=True, reductions=True, out=out)


def block_us(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(CALLS):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / CALLS * 1e6


def alternating(fns):
    """-> per function (median of REPEATS medians, spread of those medians), the functions alternating in every round"""
    for fn in fns:
        for _ in range(10):
            fn()
    medians = [[] for _ in fns]
    for _ in range(REPEATS):
        rounds = [[] for _ in fns]
        for _ in range(ROUNDS):
            for i, fn in enumerate(fns):
                rounds[i].append(block_us(fn))
        for i in range(len(fns)):
            medians[i].append(statistics.median(rounds[i]))
    return [(statistics.median(m), max(m) - min(m)) for m in medians]


def main():
    print(f"# {torch.cuda.get_device_name(0)}; one record per call, coef + reductions; per-call us = median of {REPEATS} medians of "
          f"{ROUNDS} alternating blocks of {CALLS} calls (+- spread of the medians)")
    print("# launches per call on the small engine: forward + band + tail = 3")
    print("dtype log2n order table bands | small us | hipfft us | ratio | faster by more than the spread | zoom/block us | worst row err")
    slower = []
    for dt in (torch.float32, torch.float64):
        for log2n in (10, 11, 12, 13):
            for order in (3, 12):
                n = 1 << log2n
                x = torch.from_numpy((np.random.default_rng(log2n).standard_normal((1, n)) + 0.3)).to(dt).cuda()
                auto = make_plan(n, dt, order)
                ref = make_plan(n, dt, order, _lib.QI_ENGINE_HIPFFT)
                forced = make_plan(n, dt, order, env={"QI_TUNE": "1", "QI_NATIVE_MIN_LOG2N": "10"})
                for which in (0, 2, 1):
                    nb = len(auto.freq[which])
                    a, b = call(auto, which, x), call(ref, which, x)
                    err = float(((a.coef - b.coef).abs().amax(dim=2) / b.coef.abs().amax(dim=2)).max())
                    fns = [lambda: call(auto, which, x, a), lambda: call(ref, which, x, b)]
                    native = sum(forced.stage_bands(s)[which] for s in ("zoom", "block", "pass2")) == nb
                    if native:
                        c = call(forced, which, x)
                        fns.append(lambda: call(forced, which, x, c))
                    t = alternating(fns)
                    engine_small = auto.stage_bands("small")[which] == nb
                    win = t[0][0] + t[0][1] + t[1][1] < t[1][0]
                    if engine_small and not win:
                        slower.append((dt, log2n, order, NAMES[which]))
                    print(f"{'f64' if dt == torch.float64 else 'f32'} {log2n} {order:2d} {NAMES[which]:5s} {nb:3d} | "
                          f"{t[0][0]:7.1f} +-{t[0][1]:4.1f}{'' if engine_small else ' (hipfft)'} | {t[1][0]:7.1f} +-{t[1][1]:4.1f} | "
                          f"{t[1][0] / t[0][0]:5.2f}x | {'yes' if win else 'NO'} | "
                          + (f"{t[2][0]:7.1f} +-{t[2][1]:4.1f}" if native else "    n/a") + f" | {err:.1e}", flush=True)
                for p in (auto, ref, forced):
                    p.close()
    print(f"# shapes where the small engine is not faster than the hipFFT plan by more than the spread: {slower or 'none'}")
    print("\n# joint call qi_cwt_stx (coef + reductions): separate runs | one forward launch | and one tail launch, us per call")
    for dt in (torch.float32, torch.float64):
        for log2n in (10, 13):
            for order in (3, 12):
                n = 1 << log2n
                if dt == torch.float64 and log2n == 13:
                    continue  # (the styx table of a float64 plan at 2^13 stays on the hipFFT engine: no joint run)
                x = torch.from_numpy((np.random.default_rng(log2n).standard_normal((1, n)) + 0.3)).to(dt).cuda()
                plans = [make_plan(n, dt, order, env={"QI_TUNE": "1", "QI_SMALL_JOINT": str(v)}) for v in (0, 1, 2)]
                outs = [p.cwt_stx(x, coef=True, reductions=True) for p in plans]
                t = alternating([(lambda p=p, o=o: p.cwt_stx(x, coef=True, reductions=True, out=o)) for p, o in zip(plans, outs)])
                print(f"{'f64' if dt == torch.float64 else 'f32'} {log2n} {order:2d} | " + " | ".join(f"{m:7.1f} +-{s:4.1f}" for m, s in t), flush=True)
                for p in plans:
                    p.close()


if __name__ == "__main__":
    main()
