#!/usr/bin/env python3
"""Band tables for the host sanitizer walk (tests/sanitize/walk.cpp): for every (order, record length, precision) the host
arrays the C ABI takes -- qi_plan_set_gabor_bank (styx bank: p_re, p_im, omega, amp), qi_plan_set_stx_bands (shift index,
sigma) -- and the workspace TfrPlan.workspace_for sizes for 1 / 4 / 16 / 64 records, as one little-endian binary file.
Behind them the synthetic tables of tests/band_tables.py (not constant-Q: sweeps of atom length against centre frequency,
population, single-band and large linear tables), both precisions, 1 / 4 / 16 records.
Runs in the ordinary interpreter (no sanitizer): the library's own host modules make the tables.

File: int32 {magic, configs, record slots, 2}; per config int32 {order (0: synthetic), log2n, dtype, B of the Gabor table,
B of the Stockwell table, flags}, int64 records[slots] (0: slot unused), int64 workspace[slots], float64 p_re, p_im, omega,
amp [B], float64 sigma [B stx], int64 shift index [B stx].  flags: bits 0-1 what the Gabor table must come out as (0 anything,
1 every row on the native engines, 2 the whole table on the hipFFT engine), bits 2-3 the same for the Stockwell table, bit 4:
the Gabor table is set on the atoms bank as well.  Prints {"synthetic_plans", "synthetic_on_native"} for the test."""
import json
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401  (engine imports it)

from quantum_inferno_amd import engine, scales_dyadic as scales  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tests"))
import band_tables as bt  # noqa: E402

ORDERS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12]
LOG2N = [14, 15, 16, 17, 18, 19, 20, 21, 22]
RECORDS = [1, 4, 16, 64]


SYN_RECORDS = [1, 4, 16, 0]
EXPECT = {None: 0, "native": 1, "fallback": 2}


def write_config(fh, order, log2n, dtype, records, gabor, stx, flags, n=None):
    """n: the record length itself goes into the log2n field (format 3: engine_layouts)."""
    if n is None:
        n = 1 << log2n
    else:
        log2n = n
    idx, sigma = stx
    nb = max(len(gabor["p_re"]), len(sigma))
    td = torch.float64 if dtype else torch.float32
    ws = [int(engine.TfrPlan.workspace_for(n, nb, td, max(c, 1), cap_bytes=48 << 30)) for c in records]
    fh.write(struct.pack("<6i", order, log2n, dtype, len(gabor["p_re"]), len(sigma), flags))
    fh.write(struct.pack(f"<{len(records)}q", *records))
    fh.write(struct.pack(f"<{len(records)}q", *ws))
    for a in (gabor["p_re"], gabor["p_im"], gabor["omega"], gabor["amp"], sigma):
        fh.write(np.ascontiguousarray(a, dtype="<f8").tobytes())
    fh.write(np.ascontiguousarray(idx, dtype="<i8").tobytes())


def synthetic_configs():
    """(log2n, dtype, Gabor table, Stockwell table, flags): every table of tests/band_tables.py, a Gabor one paired with
    a Stockwell one of the same length and precision."""
    gab, stx = {}, {}
    for name, log2n, f64, bank, table, expect in bt.gabor_cases():
        gab.setdefault((log2n, int(f64)), []).append((table, EXPECT[expect] | (16 if bank == 1 else 0)))
    for name, log2n, f64, table, expect in bt.stx_cases():
        stx.setdefault((log2n, int(f64)), []).append((table, EXPECT[expect] << 2))
    for f64 in (0, 1):
        n = 1 << 16
        # population, single-band and large linear tables (what they come out as is the GPU census's business)
        for k, where in ((0, "last"), (4, "last"), (5, "last"), (4, "middle")):
            stx[(16, f64)].append((bt.stx_two_pass_population(n, k, where), (1 if k == 0 else 0) << 2))
        stx[(16, f64)].append((bt.linear_stx_table(n)[1:], 1 << 2))
        for kind in ("zoom", "block", "split"):
            gab[(16, f64)].append((bt.single_band(kind, n), 0))
    out = []
    for key in sorted(set(gab) | set(stx)):
        g, s = gab.get(key, []), stx.get(key, [])
        for i in range(max(len(g), len(s))):
            gt, gf = g[i] if i < len(g) else (bt.single_band("block", 1 << key[0]), 0)
            st, sf = s[i] if i < len(s) else (bt.stx_sweep(1 << key[0], 2, sigma_lo=4.0), 0)
            out.append((key[0], key[1], gt, st, gf | sf))
    return out


def main(path):
    fs = 1000.0
    with open(path, "wb") as fh:
        syn = synthetic_configs()
        fh.write(struct.pack("<4i", 0x51495354, len(ORDERS) * len(LOG2N) * 2 + len(syn), len(RECORDS), 2))
        for order in ORDERS:
            for log2n in LOG2N:
                n = 1 << log2n
                f_hz, p_re, p_im, omega, amp, _ = engine.styx_bank_tables(order, n, fs)
                idx = scales.stx_shift_indices(f_hz, n, fs).astype(np.int64)
                sigma = (scales.cycles_from_order(order) / (2 * np.pi * f_hz / fs)).astype(np.float64)
                for dtype in (0, 1):  # QI_F32, QI_F64
                    write_config(fh, order, log2n, dtype, RECORDS, dict(p_re=p_re, p_im=p_im, omega=omega, amp=amp),
                                 (idx, sigma), 0)
        for log2n, dtype, gabor, stx, flags in syn:
            write_config(fh, 0, log2n, dtype, SYN_RECORDS, gabor, stx, flags)
    used = sum(1 for c in SYN_RECORDS if c > 0)
    both = sum(1 for c in syn if (c[4] & 3) == 1 and ((c[4] >> 2) & 3) == 1)
    print(json.dumps({"synthetic_plans": len(syn) * used, "synthetic_on_native_at_least": both * used}))


def engine_layouts(path):
    """`--engines`: one layout per engine of tests/stream_cases.py's ENGINES (float32 at 2^14, float64 at 2^15, 2^11 in both
    precisions, 3000 samples on the hipFFT engine) at its order, for 1 and 8 records (RECORD_COUNTS) -- the tables of
    tests/sanitize_threads/walk_threads.cpp.  Format 3: the field that holds log2n elsewhere holds the record length."""
    import stream_cases as sc

    fs = sc.FS
    with open(path, "wb") as fh:
        fh.write(struct.pack("<4i", 0x51495354, len(sc.ENGINES), len(sc.RECORD_COUNTS), 3))
        for dtype, n, _ in sc.ENGINES.values():
            f_hz, p_re, p_im, omega, amp, _ = engine.styx_bank_tables(sc.ORDER, n, fs)
            idx = scales.stx_shift_indices(f_hz, n, fs).astype(np.int64)
            sigma = (scales.cycles_from_order(sc.ORDER) / (2 * np.pi * f_hz / fs)).astype(np.float64)
            write_config(fh, sc.ORDER, 0, int(dtype == "float64"), list(sc.RECORD_COUNTS), dict(p_re=p_re, p_im=p_im, omega=omega, amp=amp),
                         (idx, sigma), 0, n=n)
    print(json.dumps({"layouts": [[dtype, n] for dtype, n, _ in sc.ENGINES.values()], "records": list(sc.RECORD_COUNTS)}))


if __name__ == "__main__":
    if sys.argv[1] == "--engines":
        engine_layouts(sys.argv[2])
    else:
        main(sys.argv[1])
