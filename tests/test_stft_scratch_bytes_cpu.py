"""What the STFT family's *_scratch_bytes functions return (pure host functions, no GPU): equal, row by row, to the table
tests/golden/stft_scratch_bytes.json, recorded from the library as it stood before its three-kernel scratch layout was written
once (one struct behind the byte counts and behind the pointers the entry points carve).  Every geometry of
tests/stft_cases.py -- stft_from_sig, spectral, Welch, ShortTimeFFT convention forward and inverse -- in both precisions at
1 and 3 records.  `python tests/test_stft_scratch_bytes_cpu.py OUT.json` writes the table of the library in use
(QI_TFR_LIB selects another build)."""
import json
import os
import sys

from conftest import GOLDEN  # (puts the repository root on sys.path)

import stft_cases as sc

from oracle import tfr_oracle as orc
from quantum_inferno_amd import _lib

TABLE = os.path.join(GOLDEN, "stft_scratch_bytes.json")
RECORDS = (1, 3)


def geometries():
    """(kind, name, seg, hop, nfft, n) of the forward families; (kind, name, nfft, slices) of the sliding one."""
    stft = [(sc.from_sig_id(c), c.seg, c.seg // 2, c.seg, c.n) for c in sc.from_sig_cases()]
    for c in sc.SPECTRAL_CASES:
        seg, overlap, nfft = sc.spectral_geometry(c)
        stft.append((c.name, seg, seg - overlap, nfft, c.n))
    welch = []
    for c in sc.WELCH_CASES:
        seg, overlap, nfft = sc.welch_geometry(c)
        welch.append((c.name, seg, seg - overlap, nfft, c.n))
    sliding = []
    shapes = [(seg, seg - 3 * seg // 4) for seg in sorted(set(sc.SLIDING_SEGS + sc.SLIDING_COMPLEX_SEGS))] + list(sc.ISTFT_SHAPES)
    for seg, hop in shapes:
        obj = orc.SlidingStft(sc.FS, sc.ALPHA, seg, seg - hop)
        sliding.append((f"seg{seg}_hop{hop}", obj.mfft, obj.p_max(3 * seg + 1) - obj.p_min))
    return stft, welch, sliding


def table(lib):
    """{"function dtype records case": bytes} of the library `lib`."""
    stft, welch, sliding = geometries()
    out = {}
    for dname, code in (("f32", _lib.QI_F32), ("f64", _lib.QI_F64)):
        for C in RECORDS:
            for name, seg, hop, nfft, n in stft:
                out[f"qi_stft_scratch_bytes {dname} C{C} {name}"] = int(lib.qi_stft_scratch_bytes(code, C, n, seg, hop, nfft))
                for want_coef in (0, 1):
                    out[f"qi_stft_out_scratch_bytes coef{want_coef} {dname} C{C} {name}"] = int(
                        lib.qi_stft_out_scratch_bytes(code, C, n, seg, hop, nfft, want_coef, 0))
            for name, seg, hop, nfft, n in welch:
                out[f"qi_welch_scratch_bytes {dname} C{C} {name}"] = int(lib.qi_welch_scratch_bytes(code, C, n, seg, hop, nfft))
            for name, nfft, slices in sliding:
                out[f"qi_sliding_scratch_bytes {dname} C{C} {name}"] = int(lib.qi_sliding_scratch_bytes(code, C, nfft, slices))
    return out


def test_scratch_bytes_equal_the_recorded_table():
    want = json.load(open(TABLE))
    got = table(_lib.load())
    assert sorted(got) == sorted(want)
    assert len(got) > 400 and all(v > 0 for v in want.values())
    differ = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not differ, differ


if __name__ == "__main__":
    json.dump(table(_lib.load()), open(sys.argv[1], "w"), indent=0, sort_keys=True)
