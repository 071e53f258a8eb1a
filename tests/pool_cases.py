"""Cases and a NumPy restatement of time pooling (utilities.sampling.subsample / subsample_2d of the reference), shared by
the CPU and the GPU tests: a window of `factor` consecutive samples becomes one value, the incomplete last window is
dropped, and "nth" keeps every factor-th sample (the incomplete last window included).  The fixture
tests/golden/subsample.npz (tools/gen_golden_pool.py) holds the reference's own results for the same inputs."""
import numpy as np

METHODS = ("nth", "average", "max", "min", "median")
FACTORS = (2, 3, 7, 64, 65, 100, 1000, 1031, 2000)
LENGTHS = (1031, 4096)  # odd and prime: no row after the first is 16-byte aligned, every tail ragged; 4096: windows end with the row
ROWS = 3
DTYPES = ("float32", "float64")
METHOD_CODE = {"nth": 0, "average": 1, "max": 2, "min": 3, "median": 4}  # qi_pool_method


def columns(n, factor, method):
    return len(range(0, n, factor)) if method == "nth" else n // factor


def pool_ref(a, factor, method):
    """Pooling of the last axis of `a` (any leading axes) in a's own precision, as NumPy computes it."""
    a = np.asarray(a)
    if method == "nth":
        return a[..., ::factor]
    cols = a.shape[-1] // factor
    w = a[..., : cols * factor].reshape(a.shape[:-1] + (cols, factor))
    if method == "average":
        return w.mean(axis=-1)
    if method == "median":
        return np.median(w, axis=-1)
    return w.max(axis=-1) if method == "max" else w.min(axis=-1)


def key(dtype, n, factor, method, one_d=False):
    return f"{'s1' if one_d else 's2'}_{dtype}_n{n}_f{factor}_{method}"


def noise(seed, shape, dtype, complex_=False):
    """Seeded white noise with a non-zero mean."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape) + 0.5
    if complex_:
        x = x + 1j * (rng.standard_normal(shape) - 0.25)
        return x.astype(np.complex64 if np.dtype(dtype) == np.float32 else np.complex128)
    return x.astype(dtype)
