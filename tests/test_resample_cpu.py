"""Resampling without a GPU: the fixture tests/golden/resample.npz (tools/gen_golden_resample.py) is complete, the NumPy
restatements of qi_interp_grid and qi_resample_fft (resample_cases.interp_ref, fft_resample_ref) reproduce the reference's
recorded results, the restated grid equals np.arange, the C ABI declares and exports the new entry points,
qi_resample_fft_scratch_bytes gives its values and refusals, the argument checks of qi_interp_grid that come before the
device refuse, and the wrappers raise their argument errors before the device is needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import resample_cases as rc
from quantum_inferno_amd import _lib, engine
from quantum_inferno_amd.utilities import sampling

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("qi_interp_grid", "qi_resample_fft_scratch_bytes", "qi_resample_fft")


@pytest.fixture(scope="module")
def g(golden):
    return golden("resample.npz")


def interp_inputs():
    """(fixture key, timestamps, values, rate asked for) of every interpolation case the fixture holds."""
    for n, rk in rc.interp_cases():
        ts, y = rc.uneven_record(n, *rc.fixture_combo(n, rk))
        yield rc.interp_key(n, rk), ts, y, rc.RATES[rk]
    for dtype in rc.DTYPES:
        ts, y = rc.on_grid_record(dtype)
        for rate in rc.ON_GRID_RATES:
            yield f"interp_ongrid_{dtype}_{int(rate)}", ts, y, rate


def test_fixture_is_complete(g):
    keys = set(g.files) - {"versions"}
    want = set()
    for key, ts, y, rate in interp_inputs():
        want |= {key, key + "_rate"}
        assert g[key].dtype == np.float64 and g[key].ndim == 1
        if rate is not None:
            assert float(g[key + "_rate"]) == rate
    for n, m in rc.FFT_SHAPES:
        for dtype in rc.DTYPES:
            want.add(rc.fft_key(n, m, dtype))
            assert g[rc.fft_key(n, m, dtype)].shape == (m,) and g[rc.fft_key(n, m, dtype)].dtype == np.dtype(dtype)
    assert keys == want
    assert sorted(rc.LENGTHS) == sorted({1, 2, 3, rc.T - 1, rc.T, rc.T + 1, 3 * rc.T + 17})
    assert len(rc.interp_cases()) == 4 * len(rc.LENGTHS) - 1
    # every length and every rate meets both dtypes and both epochs
    for n in rc.LENGTHS[1:]:
        assert {rc.fixture_combo(n, rk) for rk in rc.RATES} == set(rc.COMBOS)
    for rk in rc.RATES:
        assert {rc.fixture_combo(n, rk) for n in rc.LENGTHS} == set(rc.COMBOS)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "resample.npz")) <= os.path.getsize(
        os.path.join(ROOT, "tests", "golden", "peaks.npz"))


def test_fixture_holds_the_records_built_to_break_the_kernel(g):
    for dtype in rc.DTYPES:
        ts, y = rc.uneven_record(rc.T + 1, dtype, 0.0)
        assert np.isnan(y).sum() == 2 and np.isinf(y).sum() == 4 and y[90] == y[91] == np.inf
        assert np.all(np.diff(ts) >= 0) and (np.diff(ts) == 0).sum() == 8 and ts[40] == ts[43] and ts[rc.T - 6] == ts[rc.T - 2]
        ts, y = rc.on_grid_record(dtype)
        for rate in rc.ON_GRID_RATES:
            x = rc.grid_values(*rc.grid_ref(ts[0], ts[-1], rate))
            assert np.isin(x, ts).sum() == len(ts) - 1  # the xp[j] == x branch, on every knot but the last
    out = g[rc.interp_key(rc.T + 1, "x2.37")]
    assert np.isnan(out).any() and np.isinf(out).any()
    assert len(g[rc.interp_key(1, "x1")]) == 0 and len(g[rc.interp_key(2, "x2.37")]) >= 2


def test_interpolation_restatement_equals_the_reference_bit_for_bit(g):
    for key, ts, y, rate in interp_inputs():
        got_rate = float(g[key + "_rate"])
        if rate is None:
            assert got_rate == 1 / np.mean(np.diff(ts))
        start, delta, m = rc.grid_ref(ts[0], ts[-1], got_rate)
        assert m == len(g[key]), key
        assert rc.same_bits(rc.interp_ref(rc.grid_values(start, delta, m), ts, y), g[key]), key


def test_grid_restatement_and_the_module_helper_equal_arange():
    for key, ts, y, rate in interp_inputs():
        rate = 1 / np.mean(np.diff(ts)) if rate is None else rate
        want = np.arange(ts[0], ts[-1], 1 / rate)
        for grid in (rc.grid_ref, sampling.even_grid):
            start, delta, m = grid(ts[0], ts[-1], rate)
            assert m == len(want) and np.array_equal(rc.grid_values(start, delta, m), want), (key, grid.__name__)
    assert sampling.even_grid(3.0, 3.0, 10.0)[2] == 0 and sampling.even_grid(3.0, 2.0, 10.0)[2] == 0
    assert rc.grid_ref(3.0, 2.0, 10.0)[2] == 0


def test_fft_restatement_equals_the_reference(g):
    for n, m in rc.FFT_SHAPES:
        for dtype in rc.DTYPES:
            x = rc.fft_record(n, m, dtype)
            want = g[rc.fft_key(n, m, dtype)]
            got = rc.fft_resample_ref(x, m)
            if dtype == "float64":
                assert rc.same_bits(got, want), (n, m)
            else:
                assert np.max(np.abs(got - want)) <= 2e-5 * np.max(np.abs(want)), (n, m)
            rows, factors = rc.fft_batch(n, m, dtype, 5)
            assert rows.dtype == np.dtype(dtype) and np.array_equal(rows.astype(np.float64), factors[:, None] * x[None, :])
    rows, factors = rc.fft_batch(1000, 441, "float64", 3)  # a power of two of either sign goes through the transform exactly
    assert rc.same_bits(rc.fft_resample_ref(rows, 441), factors[:, None] * g[rc.fft_key(1000, 441, "float64")][None, :])


def test_header_library_and_binding_agree():
    header = open(os.path.join(ROOT, "include", "qi_tfr.h")).read()
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", header), f"{name} is not declared"
        assert hasattr(lib, name) and name in _lib.PROTOTYPES
    assert int(re.search(r"#define\s+QI_INTERP_TILE\s+(\d+)", header).group(1)) == _lib.INTERP_TILE == rc.T
    assert int(re.search(r"#define\s+QI_INTERP_KNOTS\s+(\d+)", header).group(1)) == _lib.INTERP_KNOTS == rc.K
    assert rc.K > rc.T and rc.K * 16 <= 64 * 1024
    assert lib.qi_abi_version() == 1


def test_fft_scratch_bytes():
    lib = _lib.load()

    def up(v):
        return -(-v // 256) * 256

    for dtype, esz in ((_lib.QI_F32, 4), (_lib.QI_F64, 8)):
        for c, n, m in ((1, 1, 1), (1, 1, 5), (3, 1024, 512), (65, 1009, 1013), (1024, 1 << 20, 3 << 18)):
            want = up(c * n * esz) + up(c * (n // 2 + 1) * 2 * esz) + up(c * (m // 2 + 1) * 2 * esz)
            assert lib.qi_resample_fft_scratch_bytes(dtype, c, n, m) == want, (dtype, c, n, m)
    assert lib.qi_resample_fft_scratch_bytes(2, 1, 100, 50) == -1 and b"dtype" in lib.qi_last_error()
    assert lib.qi_resample_fft_scratch_bytes(_lib.QI_F32, 0, 100, 50) == -1
    assert lib.qi_resample_fft_scratch_bytes(_lib.QI_F64, 1, 0, 50) == -1
    assert lib.qi_resample_fft_scratch_bytes(_lib.QI_F64, 1, 100, 0) == -1
    assert lib.qi_resample_fft_scratch_bytes(_lib.QI_F64, 1, 1 << 31, 8) == -1 and b"too large" in lib.qi_last_error()
    assert lib.qi_resample_fft_scratch_bytes(_lib.QI_F64, 1 << 30, 1 << 20, 8) == -1 and b"too large" in lib.qi_last_error()
    # the call itself refuses the same and a short or absent scratch, before it touches the device
    buf = np.zeros(64)
    p = buf.ctypes.data_as(C.c_void_p)
    assert lib.qi_resample_fft(_lib.QI_F64, 0, p, 1, 8, 0, p, p, 1 << 20, None) == -1
    assert lib.qi_resample_fft(_lib.QI_F64, 0, p, 1, 8, 4, p, None, 1 << 20, None) == -1 and b"null" in lib.qi_last_error()
    assert lib.qi_resample_fft(_lib.QI_F64, 0, p, 1, 8, 4, p, p, 16, None) == -1 and b"needed" in lib.qi_last_error()


def test_interp_grid_refuses_bad_arguments_before_the_device():
    lib = _lib.load()
    buf = np.zeros(64)
    p = buf.ctypes.data_as(C.c_void_p)

    def call(dtype=_lib.QI_F64, values=p, knots=p, stride=0, c=1, n=8, start=0.0, delta=1.0, m=4, out=p):
        return lib.qi_interp_grid(dtype, 0, values, knots, stride, c, n, start, delta, m, out, None)

    for bad, word in ((dict(dtype=2), b"dtype"), (dict(n=0), b"record length"), (dict(m=-1), b"output length"),
                      (dict(c=0), b"record count"), (dict(delta=0.0), b"delta"), (dict(delta=-1.0), b"delta"),
                      (dict(delta=float("nan")), b"delta"), (dict(delta=float("inf")), b"delta"),
                      (dict(start=float("nan")), b"start"), (dict(start=float("-inf")), b"start"), (dict(stride=4), b"knot_stride"),
                      (dict(stride=-8), b"knot_stride"), (dict(values=None), b"null"), (dict(knots=None), b"null"),
                      (dict(out=None), b"null")):
        assert call(**bad) == -1 and word in lib.qi_last_error(), bad


def test_wrappers_refuse_bad_arguments_before_the_device():
    x = np.linspace(-1.0, 1.0, 400)
    t = np.arange(400) / 100.0
    with pytest.raises(ValueError, match="must be at least 1"):
        sampling.resample_with_sample_rate(x, 1000.0, 2.0)
    with pytest.raises(ValueError, match=r"\[n\] or \[channels, n\]"):
        sampling.resample_with_sample_rate(np.zeros((2, 3, 4)), 10.0, 5.0)
    with pytest.raises(ValueError, match="must be at least 1"):
        engine.fft_resample(x, 0)
    with pytest.raises(ValueError, match="one timestamp per sample"):
        sampling.resample_uneven_timeseries(x, t[:-1])
    with pytest.raises(ValueError, match="one timestamp per sample"):
        sampling.resample_uneven_timeseries(np.stack([x, x]), np.stack([t, t]))
    with pytest.raises(ValueError, match=r"\[n\] or \[channels, n\]"):
        sampling.resample_uneven_timeseries(np.zeros((2, 3, 4)), np.zeros(4))
    with pytest.raises(ValueError, match="no even grid"):
        sampling.resample_uneven_timeseries(x, t, 0.0)
    with pytest.raises(ValueError, match="no even grid"):
        sampling.resample_uneven_timeseries(x[:1], t[:1])  # one sample has no average rate
    with pytest.raises(ValueError, match="lost in the rounding"):
        sampling.resample_uneven_timeseries(x, 1e17 + 1000.0 * t, 100.0)
    with pytest.raises(ValueError, match="delta must be finite and positive"):
        engine.interp_to_grid(x, t, 0.0, 0.0, 10)
    with pytest.raises(ValueError, match="start must be finite"):
        engine.interp_to_grid(x, t, float("inf"), 0.01, 10)
    with pytest.raises(ValueError, match="m must not be negative"):
        engine.interp_to_grid(x, t, 0.0, 0.01, -1)
    with pytest.raises(ValueError, match="timestamps must be"):
        engine.interp_to_grid(x, np.stack([t, t]), 0.0, 0.01, 10)
    with pytest.raises(ValueError, match="timestamps must be"):
        engine.interp_to_grid(torch.zeros(3, 400), torch.zeros(2, 400), 0.0, 0.01, 10)
    assert "not a Fourier method" in sampling.__doc__
