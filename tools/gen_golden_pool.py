"""Generator of tests/golden/subsample.npz -- TEST INFRASTRUCTURE, run where the reference package is installed or
checked out (QI_REFERENCE names its directory).  Feeds the reference's utilities.sampling.subsample_2d / subsample seeded
inputs and stores the inputs with the reference's results; nothing of the reference itself is copied.

    python tools/gen_golden_pool.py

The inputs are seeded noise on a grid of 2^-10 (a few significant bits per value), which keeps the compressed fixture
under 1 MB; the pooled values are whatever the reference returns for them."""
import io
import os
import sys
from contextlib import redirect_stdout

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.environ.get("QI_REFERENCE", "/root/reference"))

from quantum_inferno.utilities import sampling  # noqa: E402

import pool_cases as pc  # noqa: E402


def main():
    d = {}
    for di, dtype in enumerate(pc.DTYPES):
        for n in pc.LENGTHS:
            x = np.round(pc.noise(1000 * di + n, (pc.ROWS, n), np.float64) * 1024.0) / 1024.0
            x = x.astype(dtype)
            d[f"in_{dtype}_n{n}"] = x
            for f in pc.FACTORS:
                for m in pc.METHODS:
                    with redirect_stdout(io.StringIO()):
                        two = sampling.subsample_2d(x.copy(), f, m)
                        one, rate = sampling.subsample(x[0].copy(), 800.0, f, m)
                    assert rate == 800.0 / f
                    assert two.dtype == x.dtype and one.dtype == x.dtype, (dtype, n, f, m, two.dtype, one.dtype)
                    d[pc.key(dtype, n, f, m)] = np.ascontiguousarray(two)
                    d[pc.key(dtype, n, f, m, one_d=True)] = np.ascontiguousarray(one)
    path = os.path.join(ROOT, "tests", "golden", "subsample.npz")
    np.savez_compressed(path, versions=np.array([np.__version__, "quantum-inferno 1.1.3"]), **d)
    print(f"{path}: {os.path.getsize(path) / 1e6:.3f} MB, {len(d)} arrays")


if __name__ == "__main__":
    main()
