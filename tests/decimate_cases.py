"""Cases of the decimation tests and a NumPy restatement of qi_decimate's semantics (include/qi_tfr.h), shared by the CPU
and GPU tests and by tools/gen_golden_decimate.py.  The restatement is filter_cases' plain loop over time, here with every
table, state, product and sum in the record's own type T (float32 or float64), then every q-th sample."""
import numpy as np

import filter_cases as fc

RECORDS = fc.RECORDS
FACTORS = (1, 2, 5, 13)
DTYPES = ("float64", "float32")
# the shortest legal record (edge + 1); n + 2 edge = 320 = exactly 5 time tiles of 64; a short one; a prime (every tile ragged)
LENGTHS = (28, 266, 300, 1031)
EDGE = 27
SECTIONS = 4
EPS = {"float64": 2.0 ** -52, "float32": 2.0 ** -23}


def cases():
    """(q, dtype, n) of every case of the fixture."""
    return [(q, dtype, n) for q in FACTORS for dtype in DTYPES for n in LENGTHS]


def columns(n, q):
    return -(-n // q)


def table_key(q, dtype, what):
    return f"q{q}_{dtype}_{what}"


def key(q, dtype, n, what):
    return f"q{q}_{dtype}_n{n}_{what}"


def tables(g, q, dtype):
    """(sos [4, 6], zi [4, 2], edge) of factor q in `dtype`, as the C ABI takes them."""
    return (np.ascontiguousarray(g[table_key(q, dtype, "sos")]), np.ascontiguousarray(g[table_key(q, dtype, "zi")]),
            int(g[table_key(q, dtype, "edge")]))


def seed(q, dtype, n):
    return 7000000 + 100000 * DTYPES.index(dtype) + 1000 * q + n


def decimate_ref(x, q, sos, zi, edge):
    """qi_decimate's semantics on records x [R, n] of type T: -> [R, ceil(n / q)] of type T, nothing wider on the way."""
    x = np.asarray(x)
    t = x.dtype
    assert x.ndim == 2 and t in (np.float32, np.float64) and x.shape[1] > edge and q >= 1
    sos = np.asarray(sos)
    zi = np.asarray(zi)
    assert sos.dtype == t and zi.dtype == t, "the tables come in the record's type"
    two = t.type(2)
    ext = np.concatenate((two * x[:, :1] - x[:, edge:0:-1], x, two * x[:, -1:] - x[:, -2:-(edge + 2):-1]), axis=1)
    assert ext.dtype == t
    y = fc._pass_sos(ext, sos, zi[None, :, :] * ext[:, 0][:, None, None])
    y = fc._pass_sos(y[:, ::-1], sos, zi[None, :, :] * y[:, -1][:, None, None])[:, ::-1]
    assert y.dtype == t
    return np.ascontiguousarray(y[:, edge:edge + x.shape[1]:q])
