"""Cases and references of the STFT's reduced product (qi_stft_out; a plain helper module beside stft_cases.py, whose
records and float64 oracle panels it reduces).  Used by tests/test_gpu_stft_reduced.py (GPU) and
tests/test_stft_reduced_cpu.py (CPU: the references themselves).

Reference: P = power_scale |Z_ref|^2 of the case's oracle panel, reduced in NumPy float64:
power_band = P.sum(-1), power_time = P.sum(-2), stats = (P.max(), P.sum(), sum P log2 P with 0 log 0 = 0).

Bounds (DESIGN s2, the reduction contract: float64 1e-10, float32 1e-4): the marginals by max |error| / max |reference| of
the array; max P and sum P relative to themselves; sum P log2 P relative to sum |P log2 P| (the signed sum can cancel --
powers above and below 1 -- so it is no yardstick for its own error); the entropy within 20 x the contract in absolute
bits, as test_gpu_parity.py holds the plans' entropy.
"""
import collections

import numpy as np

import stft_cases as sc

RED_TOL = {np.float64: 1e-10, np.float32: 1e-4}

Reduced = collections.namedtuple("Reduced", "power_band power_time stats abs_plogp entropy_bits")


def reduce_reference(z_ref, power_scale=1.0):
    """The reduced product of a float64 oracle panel [C, f, t]."""
    p = power_scale * (z_ref.real ** 2 + z_ref.imag ** 2)
    plogp = np.zeros_like(p)
    np.multiply(p, np.log2(p, where=p > 0, out=np.zeros_like(p)), out=plogp)
    s, spl = p.sum(axis=(-2, -1)), plogp.sum(axis=(-2, -1))
    stats = np.stack([p.max(axis=(-2, -1)), s, spl], axis=-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        ent = np.log2(s) - spl / s
    return Reduced(p.sum(-1), p.sum(-2), stats, np.abs(plogp).sum(axis=(-2, -1)), ent)


def check_reduced(power_band, power_time, stats, entropy_bits, ref, dtype, what):
    """NumPy arrays of one call against `ref` (a Reduced); every figure is in the assertion message."""
    tol = RED_TOL[dtype]
    assert power_band.shape == ref.power_band.shape and power_band.dtype == np.float64, what
    assert stats.shape == ref.stats.shape[:-1] + (4,) and stats.dtype == np.float64, what
    for c in range(ref.stats.shape[0]):
        eb = np.max(np.abs(power_band[c] - ref.power_band[c])) / ref.power_band[c].max()
        assert eb <= tol, (what, c, "power_band", eb)
        if power_time is not None:
            assert power_time.shape == ref.power_time.shape and power_time.dtype == dtype, what
            et = np.max(np.abs(power_time[c].astype(np.float64) - ref.power_time[c])) / ref.power_time[c].max()
            assert et <= tol, (what, c, "power_time", et)
        em = abs(stats[c, 0] - ref.stats[c, 0]) / ref.stats[c, 0]
        es = abs(stats[c, 1] - ref.stats[c, 1]) / ref.stats[c, 1]
        el = abs(stats[c, 2] - ref.stats[c, 2]) / ref.abs_plogp[c]
        assert em <= tol and es <= tol and el <= tol, (what, c, "max / sum / sum p log2 p", em, es, el)
        assert stats[c, 3] == 0.0, what
        if entropy_bits is not None:
            eh = abs(entropy_bits[c] - ref.entropy_bits[c])
            assert eh <= 20 * tol, (what, c, "entropy bits", eh)


# ---- 1. every fused transform length, PLAIN form (one segment group: 7 - 9 segments, 3 at n = seg) -------------------------
def plain_cases(dtype):
    return [case for case in sc.from_sig_cases() if case.seg in sc.FUSED_LENGTHS[dtype]]


# ---- 2. several groups and a ragged last one ----------------------------------------------------------------------------
GROUP_CASES = (sc.FromSig(512, 512 + 40 * 256 + 5),  # 44 segments: groups of 16, 16, 12 at G = 16
               sc.FromSig(64, 40 * 64 + 1))  # 82 segments

# ---- 3. general kernel form (seg < nfft, any hop), through _stft_windowed -------------------------------------------------
GENERAL_NAMES = ("seg64_nfft512", "seg100_hop1", "seg201_hop101", "seg96_hop96", "gtx_seg201")
# ---- 4. hipFFT path: (SPECTRAL_CASES name, dtypes) and the stft_from_sig row past the fused lengths ---------------------
HIPFFT_SPECTRAL = (("seg200_nfft300", sc.DTYPES), ("seg3000", (np.float64,)))
HIPFFT_FROM_SIG = sc.FromSig(8192, 3 * 8192 + 1)


def spectral_case(name):
    return next(case for case in sc.SPECTRAL_CASES if case.name == name)


def from_sig_reduced(case, dtype, power_scale=1.0):
    return reduce_reference(sc.from_sig_reference(case, dtype)[2], power_scale)


def spectral_reduced(case, dtype, power_scale=1.0):
    return reduce_reference(sc.spectral_reference(case, dtype)[2], power_scale)


def every_reference():
    """(id, Reduced) of every case the GPU tests compare against."""
    for dtype in sc.DTYPES:
        tag = "f64" if dtype == np.float64 else "f32"
        for case in plain_cases(dtype) + list(GROUP_CASES) + [HIPFFT_FROM_SIG]:
            yield f"{sc.from_sig_id(case)}-{tag}", from_sig_reduced(case, dtype)
        for name in GENERAL_NAMES:
            yield f"{name}-{tag}", spectral_reduced(spectral_case(name), dtype)
        for name, dtypes in HIPFFT_SPECTRAL:
            if dtype in dtypes:
                yield f"{name}-{tag}", spectral_reduced(spectral_case(name), dtype)
