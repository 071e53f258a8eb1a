"""Device time of qi_cross_spectra_bands against what it replaces, tools/windows_bench.py's method: device events after
warm-up, median (min .. max).  The order-12 Stockwell panel of 4, 16 and 64 records of 2^18 samples (float32), every band in a
window of 20 of its periods every 10 (beamform.constant_q_windows), summed at up to 4096 terms (max_terms 4096: the low bands
are strided) and at every sample (max_terms None).  Beside every shape, in the same job:
  loop    the parent's composition, stride 1 only: engine.cross_spectra_windows once per band
  einsum  torch.einsum on panel[:, b].unfold per band (strided where the band is)
  bytes   what the call must read (every sample some term reads, once) and write, against the 8 TB/s peak
Then the longest band alone, whose windows are one wave each: with and without the stride.  Nothing here is gated: the numbers
are recorded, the shapes where the new call loses included.

    python tools/bands_bench.py [--out profiles/bands_kernel.txt] [--records 4 16 64] [--reps 20]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from quantum_inferno_amd import _lib, beamform, engine, styx_stx  # noqa: E402

N, ORDER, FS, CYCLES = 1 << 18, 12, 800.0, 20.0
PEAK_TBS = 8.0


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


def samples_read(n, terms, hop, stride):
    """Distinct samples of one record's row that some term of some window reads, per band."""
    out = []
    for t, h, s in zip(terms, hop, stride):
        n_win = (n - ((t - 1) * s + 1)) // h + 1
        idx = (np.arange(n_win, dtype=np.int64)[:, None] * h + np.arange(t, dtype=np.int64)[None, :] * s).ravel()
        out.append(np.unique(idx).size)
    return np.array(out, dtype=np.int64)


def banded_call(lib, dev, z, bins, terms, hop, stride):
    """The C call alone on preallocated outputs -> (closure, offsets)."""
    C, nb, n = z.shape
    code = _lib.dtype_code(torch.float32)
    first, count = bins
    tables = [_lib.iarr(t) for t in (terms, hop, stride)]
    (_, tp), (_, hp), (_, sp) = tables
    offsets = np.empty(count + 1, dtype=np.int64)
    total = int(lib.qi_cross_spectra_bands_layout(n, count, tp, hp, sp, offsets.ctypes.data_as(_lib._I64)))
    csd = torch.empty((total, C, C), dtype=z.dtype, device=dev)
    scratch, nbytes = _lib.scratch(lib.qi_cross_spectra_bands_scratch_bytes, dev, code, C, nb, n, first, count, tp, hp, sp)

    def call():
        assert tables
        _lib.call(lib.qi_cross_spectra_bands, dev, code, dev.index, _lib.ptr(z), C, nb, n, first, count, tp, hp, sp, None, _lib.ptr(csd),
                  None, _lib.ptr(scratch), nbytes)

    return call, offsets


def rows(lib, dev, C, reps, lines):
    rng = np.random.default_rng([73, C])
    x = torch.from_numpy(rng.standard_normal((C, N)).astype(np.float32)).to(dev)
    res = styx_stx._stx_panel(ORDER, x, FS)
    z, f = res.coef, np.asarray(res.frequency_hz, dtype=np.float64)
    nb = z.shape[1]
    for max_terms in (4096, None):
        bins, terms, hop, stride = beamform.constant_q_windows(f, FS, N, CYCLES, 0.5, max_terms)
        first, count = bins
        call, off = banded_call(lib, dev, z, bins, terms, hop, stride)
        total = int(off[-1])
        t_call = timed(call, dev, 2, reps)
        read_mb = float(samples_read(N, terms, hop, stride).sum()) * C * 8 / 1e6
        out_mb = total * C * C * 8 / 1e6
        floor_ms = (read_mb + out_mb) / 1e6 / PEAK_TBS * 1e3
        lines += [f"float32 C = {C}, {count} of {nb} bands ({f[first]:.2f} .. {f[first + count - 1]:.1f} Hz), max_terms {max_terms}: {total} matrices, "
                  f"terms {int(terms.min())} .. {int(terms.max())}, stride 1 .. {int(stride.max())} ({int((stride > 1).sum())} bands strided)",
                  f"  qi_cross_spectra_bands           {fmt(t_call)}",
                  f"  must read {read_mb:.1f} MB and write {out_mb:.1f} MB: {floor_ms:.4f} ms at {PEAK_TBS:g} TB/s; the call takes x {t_call[0] / floor_ms:.0f} of that, "
                  f"{(read_mb + out_mb) / t_call[0] / 1e3:.3f} TB/s"]

        def einsum():
            for b in range(count):
                span = (int(terms[b]) - 1) * int(stride[b]) + 1
                u = z[:, first + b].unfold(1, span, int(hop[b]))[:, :, ::int(stride[b])]
                torch.einsum("iwk,jwk->wij", u.conj(), u)

        t_ein = timed(einsum, dev, 1, 3)
        lines.append(f"  torch.einsum on unfold per band  {fmt(t_ein)}   x {t_ein[0] / t_call[0]:.2f}")
        if max_terms is None:
            def loop():
                for b in range(count):
                    engine.cross_spectra_windows(z, int(terms[b]), int(hop[b]), bins=(first + b, 1))

            t_loop = timed(loop, dev, 1, 3)
            lines.append(f"  loop of cross_spectra_windows    {fmt(t_loop)}   x {t_loop[0] / t_call[0]:.2f}   ({count} calls)")
        # the longest band alone: every window is one wave's chain per tile group
        one, one_off = banded_call(lib, dev, z, (first, 1), terms[:1], hop[:1], stride[:1])
        t_one = timed(one, dev, 2, reps)
        lines += [f"  the longest band alone ({f[first]:.2f} Hz: {int(one_off[-1])} windows of {int(terms[0])} terms every {int(stride[0])} samples)  {fmt(t_one)}",
                  ""]
        print("\n".join(lines[-7:]), flush=True)
        del call, one
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bands_kernel.txt"))
    ap.add_argument("--records", type=int, nargs="+", default=[4, 16, 64])
    ap.add_argument("--reps", type=int, default=20)
    opt = ap.parse_args()
    lib = _lib.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    lines = [f"qi_cross_spectra_bands on {torch.cuda.get_device_name(dev)}: the order-{ORDER} Stockwell panel of records of 2^18 samples at {FS:g} Hz, "
             f"windows of {CYCLES:g} periods every {CYCLES / 2:g}; median (min .. max) of {opt.reps} calls, device events (the loop and the einsum: 3 calls)",
             "x: the yardstick's time over the banded call's (below 1: the banded call loses)", ""]
    for C in opt.records:
        rows(lib, dev, C, opt.reps, lines)
    with open(opt.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(opt.out)


if __name__ == "__main__":
    main()
