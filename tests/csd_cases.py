"""Cases of the cross-spectrum tests and a NumPy restatement of qi_csd's semantics (include/qi_array.h) without SciPy, shared
by the CPU and GPU tests, tools/gen_golden_csd.py and tools/csd_bench.py.

The records of a case come from `records`: two shared noise sources, the second lagged by LAG samples, mixed into every
record with weights from uniform(-1, 1), plus OWN x independent noise -- every pair is partly coherent, with a phase that
the lag turns with frequency, so a swapped pair, a wrong conjugation or a transposed matrix shows.  The values are rounded
to float32 once and stored in the fixture: the float32 and the float64 runs read the same numbers, SciPy read them as
float64.

tests/golden/csd.npz holds, per case, the records and scipy.signal.csd (both scalings) and scipy.signal.coherence of every
pair i <= j (SciPy's [j][i] is the conjugate of its [i][j] to rounding, which the generator asserts; the library's is the
conjugate bit for bit, which the GPU test asserts, so the upper triangle checks the whole matrix), for the C = 33 case the
full rows ROWS33 only.
"""
import collections
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "csd.npz")
FS = 800.0
ALPHA = 0.25
LAG = 7
OWN = 0.7
SEED = 11
SCALINGS = ("spectrum", "density")
ROWS33 = (0, 15, 16, 32)
FLOOR = 1e-2  # every auto-power is at least this fraction of its record's maximum over the bins: no bin is masked anywhere
# The float32 coherence tolerance.  COH32_RESTATEMENT: the largest deviation from the SciPy fixture, over all cases, of the
# coherence of restate(dtype=float32) -- frames, mean and window in float32, the transform rounded to complex64 once, products
# and sums in float32 in segment order -- as NumPy gave it on the CPU (5.839e-07, the C = 17 case; tests/test_csd_cpu.py
# computes it again and holds the constant to it).  Times 16: the restatement rounds the transform once, a float32 FFT of up
# to 2^11 points once per stage.  Never above the derived 4 eps / m = 4e-2 (eps = 1e-4, m = FLOOR).
COH32_RESTATEMENT = 5.84e-7
COH32_TOL = 16 * COH32_RESTATEMENT

Case = collections.namedtuple("Case", "id C n seg overlap nfft path rows")
CASES = (
    Case("c5_n4096_seg256", 5, 4096, 256, 128, 256, "fused", None),
    Case("c17_n2048_seg64_nfft128", 17, 2048, 64, 48, 128, "fused", None),
    Case("c3_n1000_seg100_nfft128", 3, 1000, 100, 50, 128, "hipfft", None),  # a segment that is no power of two
    Case("c33_n1024_seg64", 33, 1024, 64, 32, 64, "fused", ROWS33),
    Case("c2_n256_one_segment", 2, 256, 256, 0, 256, "fused", None),  # one segment: the coherence is 1
)


def ids():
    return [c.id for c in CASES]


def by_id(cid):
    return next(c for c in CASES if c.id == cid)


def hop(case):
    return case.seg - case.overlap


def segments(case):
    return (case.n - case.seg) // hop(case) + 1


def records(case):
    """[C, n] float32 (float64 values rounded once)."""
    rng = np.random.default_rng([SEED, case.C, case.n])
    common = rng.standard_normal((2, case.n))
    mix = rng.uniform(-1, 1, (case.C, 2))
    own = rng.standard_normal((case.C, case.n))
    lagged = np.roll(common[1], LAG)
    x = mix[:, :1] * common[0] + mix[:, 1:] * lagged + OWN * own
    return np.ascontiguousarray(x.astype(np.float32))


def tukey_periodic(points, alpha):
    """scipy.signal.get_window(("tukey", alpha), points) restated (the library's own restatement is checked against SciPy in
    tests/test_host_cpu.py; this one is checked against the fixture through `restate`)."""
    sym = points + 1
    k = np.arange(sym)
    ramp = int(np.floor(alpha * (sym - 1) / 2.0))
    w = np.ones(sym)
    w[: ramp + 1] = 0.5 * (1 + np.cos(np.pi * (-1 + 2.0 * k[: ramp + 1] / alpha / (sym - 1))))
    w[sym - ramp - 1:] = 0.5 * (1 + np.cos(np.pi * (-2.0 / alpha + 1 + 2.0 * k[sym - ramp - 1:] / alpha / (sym - 1))))
    return w[:-1]


def scale2(window64, scaling):
    """What multiplies the mean over the segments of conj(X_i) X_j: scipy.signal.csd's `scale`."""
    if scaling == "spectrum":
        return 1.0 / np.sum(window64) ** 2
    assert scaling == "density", scaling
    return 1.0 / (FS * np.sum(window64 * window64))


def bin_weights(nfft, nseg, s2):
    """weight[f] of qi_csd: scale^2 / n_seg, doubled for the bins a one-sided spectrum holds twice."""
    w = np.full(nfft // 2 + 1, s2 / nseg)
    w[1:(-1 if nfft % 2 == 0 else None)] *= 2.0
    return w


def panel(x, case, dtype=np.float64):
    """The unscaled coefficient panel [C, nf, n_seg] of the Welch segments: frames, mean removal and window in `dtype`, the
    transform in float64 and rounded ONCE to the complex type of `dtype`."""
    x = np.asarray(x, dtype=dtype)
    w = tukey_periodic(case.seg, ALPHA).astype(dtype)
    idx = np.arange(segments(case))[:, None] * hop(case) + np.arange(case.seg)[None, :]
    frames = x[:, idx]
    frames = frames - frames.mean(axis=-1, keepdims=True, dtype=dtype)
    frames = (frames * w).astype(dtype)
    z = np.fft.rfft(frames.astype(np.float64), case.nfft)  # [C, n_seg, nf]
    return np.ascontiguousarray(np.swapaxes(z, 1, 2)).astype(np.complex64 if dtype == np.float32 else np.complex128)


def window_of(case, dtype=np.float64):
    return tukey_periodic(case.seg, ALPHA).astype(dtype)


def restate(x, case, scaling, dtype=np.float64):
    """csd [nf, C, C] of the records.  float64: einsum.  float32: every product and sum in float32 (complex64), the segments
    in order -- what rounding in the records' precision alone costs."""
    z = panel(x, case, dtype)
    w = bin_weights(case.nfft, segments(case), scale2(window_of(case, dtype).astype(np.float64), scaling))
    if dtype == np.float64:
        s = np.einsum("ifs,jfs->fij", np.conj(z), z)
        return s * w[:, None, None]
    s = np.zeros((z.shape[1], case.C, case.C), dtype=np.complex64)
    for m in range(z.shape[2]):
        s += np.conj(z[:, :, m].T[:, :, None]) * z[:, :, m].T[:, None, :]
    return s * w.astype(np.float32)[:, None, None]


def coherence_of(s):
    """|S_ij|^2 / (S_ii S_jj) in float64."""
    s = np.asarray(s).astype(np.complex128)
    d = np.real(np.einsum("fii->fi", s))
    with np.errstate(all="ignore"):
        return (s.real ** 2 + s.imag ** 2) / (d[:, :, None] * d[:, None, :])


def auto_power_floor(s_full):
    """min over records of (min over bins / max over bins) of the auto-power."""
    d = np.real(np.einsum("fii->fi", s_full))
    return float((d.min(axis=0) / d.max(axis=0)).min())


# ---- the fixture's layout ---------------------------------------------------------------------------------------------------
def triangle(C):
    return np.triu_indices(C)


def pack(full, case):
    """[nf, C, C] -> what the fixture keeps of it."""
    if case.rows is not None:
        return np.ascontiguousarray(full[:, list(case.rows), :])
    i, j = triangle(case.C)
    return np.ascontiguousarray(full[:, i, j])


def key(case, what):
    return f"{case.id}|{what}"


def expected(golden, case, what):
    """The fixture's `what` ("csd_spectrum", "csd_density", "coherence") as (entries [nf, ...], selector): `selector(full)`
    cuts the same entries out of a full [nf, C, C] result."""
    return golden[key(case, what)], (lambda full: pack(np.asarray(full), case))

