#!/usr/bin/env python3
"""Every output of the short-time Fourier family, as .npy files, for a bit-for-bit comparison of two libraries.

    python tools/stft_family_dump.py dump --root TREE --out DIR     run the package of TREE (default: this tree), dump into DIR
    python tools/stft_family_dump.py compare DIR_A DIR_B [label]    np.array_equal on every file; exit status 1 on a difference

The rows are those of tests/stft_cases.py, tests/stft_stream_cases.py and the smallest shapes of tests/test_gpu_stream_pool.py
of THIS tree (both libraries see the same cases), through the public API: the wrappers, the plans and the pipelines, and the C
ABI for the complex output of qi_sliding_stft, which no wrapper returns.  Both precisions.  With QI_TUNE=1 QI_STFT_FUSED=0 in
the environment every shape takes the hipFFT engine.
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dump(root, out):
    sys.path[:0] = [root, os.path.join(HERE, "tests")]
    import torch

    import stft_cases as sc
    import stft_stream_cases as ssc
    from quantum_inferno_amd import _lib, engine, scales_dyadic, stream, styx_fft
    from quantum_inferno_amd.utilities import short_time_fft as stf

    os.makedirs(out, exist_ok=True)
    count = [0]

    def save(name, a):
        if isinstance(a, torch.Tensor):
            a = a.detach().cpu().numpy()
        np.save(os.path.join(out, name + ".npy"), np.ascontiguousarray(a))
        count[0] += 1

    def save_result(name, res):
        for field in ("coef", "bits", "power_band", "power_time", "stats"):
            if getattr(res, field) is not None:
                save(f"{name}__{field}", getattr(res, field))
        for m, strip in (res.pooled or {}).items():
            save(f"{name}__pooled_{m}", strip)

    lib = _lib.require_gpu()
    for dtype in sc.DTYPES:
        d = np.dtype(dtype).name
        tdtype = torch.float64 if dtype == np.float64 else torch.float32
        # ---- stft_from_sig, its reductions, stft_complex_pow2 / gtx_complex_pow2, Welch
        for case in sc.from_sig_cases():
            x = sc.from_sig_record(case, dtype)
            z, bits, t, f = styx_fft.stft_from_sig(x, sc.FS, *sc.SEGMENT_ARGS[case.seg])
            for key, a in (("z", z), ("bits", bits), ("t", t), ("f", f)):
                save(f"from_sig_{sc.from_sig_id(case)}_{d}__{key}", a)
            res, _, _ = styx_fft.stft_reductions_from_sig(x, sc.FS, *sc.SEGMENT_ARGS[case.seg], power_scale=2.0)
            save_result(f"from_sig_reduced_{sc.from_sig_id(case)}_{d}", res)
        for case in sc.SPECTRAL_CASES:
            fn = styx_fft.stft_complex_pow2 if case.fn == "stft" else styx_fft.gtx_complex_pow2
            kw = dict(overlap_points=case.overlap, nfft_points=case.nfft)
            f, t, z = fn(sc.spectral_record(case, dtype), sc.FS, case.seg, **kw)
            for key, a in (("z", z), ("t", t), ("f", f)):
                save(f"spectral_{case.name}_{d}__{key}", a)
        for case in sc.WELCH_CASES:
            f, p = styx_fft.welch_power_pow2(sc.welch_record(case, dtype), sc.FS, case.seg, case.nfft, case.overlap)
            save(f"welch_{case.name}_{d}__f", f)
            save(f"welch_{case.name}_{d}__pxx", p)
        # ---- the ShortTimeFFT convention: forward real panels, the complex panel, the inverse
        for seg in sc.SLIDING_SEGS:
            x = sc.sliding_record(seg, dtype)
            for scaling in ("magnitude", "psd"):
                for padding in sc.PADDINGS:
                    _, _, mag = stf.stft_tukey(x, sc.FS, sc.ALPHA, seg, 3 * seg // 4, scaling, padding)
                    _, _, sxx = stf.spectrogram_tukey(x, sc.FS, sc.ALPHA, seg, 3 * seg // 4, scaling, padding)
                    save(f"sliding_seg{seg}_{scaling}_{padding}_{d}__mag", mag)
                    save(f"sliding_seg{seg}_{scaling}_{padding}_{d}__sxx", sxx)
        for seg in sc.SLIDING_COMPLEX_SEGS:
            obj = stf.get_stft_object_tukey(sc.FS, sc.ALPHA, seg, 3 * seg // 4, "magnitude")
            x = torch.from_numpy(sc.sliding_record(seg, dtype)).cuda()
            n_ch, n = x.shape
            n_slices, first = obj.p_max(n) - obj.p_min, obj.p_min * obj.hop - obj.m_num_mid
            code = _lib.dtype_code(x.dtype)
            win = torch.from_numpy(obj.win).to(device="cuda", dtype=x.dtype)
            z = torch.empty((n_ch, obj.f_pts, n_slices), dtype=engine._complex_of(tdtype), device="cuda")
            nbytes = int(lib.qi_sliding_scratch_bytes(code, n_ch, obj.mfft, n_slices))
            scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
            _lib.check(lib.qi_sliding_stft(code, 0, _lib.ptr(x), n_ch, n, _lib.ptr(win), obj.m_num, obj.hop, obj.mfft, first, n_slices,
                                           0, 0, obj.m_num_mid, _lib.ptr(z), None, 1, _lib.ptr(scratch), nbytes,
                                           _lib.stream_ptr(x.device)))
            save(f"sliding_complex_seg{seg}_{d}__z", z)
        for seg, hop in sc.ISTFT_SHAPES:
            _, y = stf.istft_tukey(sc.istft_spectrum(seg, hop, dtype), sc.FS, sc.ALPHA, seg, seg - hop)
            save(f"istft_seg{seg}_hop{hop}_{d}__x", y)
        # ---- StftPlan.run and every form of StftPlan.reduce
        for order, seg in sorted(sc.PLAN_ORDERS.items()):
            x = torch.from_numpy(sc.record(3 * seg + 1, [6, seg], dtype)).cuda()
            plan = styx_fft.StftPlan(x.shape[1], x.shape[0], sc.FS, order, tdtype)
            z, bits = plan.run(x)
            save(f"plan_o{order}_{d}__z", z)
            save(f"plan_o{order}_{d}__bits", bits)
            save(f"plan_o{order}_{d}__t", plan.time_s)
            save(f"plan_o{order}_{d}__f", plan.frequency_hz)
            for coef in (False, True):
                for bits_ in (False, True):
                    for reductions in (True, "band", False):
                        if coef or bits_ or reductions:
                            res = plan.reduce(x, coef=coef, bits=bits_, reductions=reductions, power_scale=0.5)
                            save_result(f"plan_o{order}_reduce_c{int(coef)}b{int(bits_)}r{reductions}_{d}", res)
        # ---- StftStream + StftRecord
        for shape in ssc.SHAPES + (ssc.Shape("long", ssc.LONG, 8),):
            host = ssc.record(shape, dtype)
            for pooled in (2, None):
                plan = styx_fft.StftRangePlan(host.shape[1], sc.FS, dtype=tdtype, **ssc.plan_arguments(shape))
                per = shape.per_item + (shape.per_item % 2 if pooled else 0)
                pipe = stream.StftStream(plan, host, per, block=2, pooled=pooled, pooled_methods=("average", "max"), power_scale=2.0)
                rec = stream.StftRecord(host.shape[0], plan.n_f, plan.n_seg, pooled=pooled, methods=("average", "max"), dtype=tdtype,
                                        device="cuda")
                for item in pipe.run():
                    rec.add(item)
                name = f"stft_stream_{shape.name}_pooled{pooled}_{d}"
                save_result(name, rec.result())
                save(name + "__t", plan.time_s)
                save(name + "__f", plan.frequency_hz)
        # ---- StreamPipeline (default, keep_time=False, pooled) + PooledRecord on the small-record shape
        chunk, hop, n_total, factor, block, order, records = 1024, 512, 5000, 24, 2, 3, 2
        host = np.random.default_rng([7, n_total]).standard_normal((records, n_total)).astype(dtype)
        nb = len(scales_dyadic.log_frequency_hz_from_fft_points(sc.FS, chunk, order))
        plan = engine.TfrPlan(chunk, dtype, None, engine.TfrPlan.workspace_for(chunk, nb, dtype, block))
        plan.set_styx_bank(order, sc.FS)
        plan.set_stx_bands(order, sc.FS)
        for label, kw in (("default", {}), ("band", dict(keep_time=False))):
            for item in stream.StreamPipeline(plan, host, hop, block=block, **kw).run():
                save_result(f"pipeline_{label}_{d}_item{item.index}_cwt", item.cwt)
                save_result(f"pipeline_{label}_{d}_item{item.index}_stx", item.stx)
        recs = {t: stream.PooledRecord(records, nb, n_total // factor, ("average", "max"), tdtype, "cuda") for t in ("cwt", "stx")}
        for item in stream.StreamPipeline(plan, host, hop, block=block, pooled=factor, pooled_methods=("average", "max")).run():
            for t in recs:
                recs[t].add(item, t)
        for t in recs:
            save_result(f"pipeline_pooled_{d}_{t}", recs[t].result())
        plan.close()
    torch.cuda.synchronize()
    print(f"dumped {count[0]} arrays into {out} (QI_STFT_FUSED={os.environ.get('QI_STFT_FUSED', 'unset')})")


def compare(a, b, label):
    names = sorted(set(os.listdir(a)) | set(os.listdir(b)))
    equal = 0
    for name in names:
        pa, pb = os.path.join(a, name), os.path.join(b, name)
        if not (os.path.exists(pa) and os.path.exists(pb)):
            print(f"  {label:<8} {name:<72} only in {a if os.path.exists(pa) else b}")
            continue
        xa, xb = np.load(pa), np.load(pb)
        same = xa.dtype == xb.dtype and xa.shape == xb.shape and np.array_equal(xa, xb, equal_nan=True)
        equal += same
        print(f"  {label:<8} {name:<72} {str(xa.dtype):<10} shape {str(xa.shape):<18} equal {same}")
    print(f"{label:<8} every dumped array equal: {equal == len(names)} ({equal} of {len(names)} arrays)")
    return equal == len(names)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    p = sub.add_parser("dump")
    p.add_argument("--root", default=HERE)
    p.add_argument("--out", required=True)
    p = sub.add_parser("compare")
    p.add_argument("a")
    p.add_argument("b")
    p.add_argument("label", nargs="?", default="family")
    args = ap.parse_args()
    if args.cmd == "dump":
        dump(os.path.abspath(args.root), args.out)
    else:
        sys.exit(0 if compare(args.a, args.b, args.label) else 1)
