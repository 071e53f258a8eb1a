"""Integration and differentiation without a GPU: the NumPy restatements of qi_cumtrapz and qi_derivative
(calculus_cases.terms_ref, scan_ref, gradient_ref, difference_ref) against SciPy, NumPy and the reference's recorded results
(tests/golden/calculus.npz, tools/gen_golden_calculus.py): the terms, the gradient and the difference bit for bit; the
summation tree equal to the reference on exactly summable records, inside the bound that holds for any order of summation on
random ones, and with the reference's NaN and infinities; the project's tolerances met by the reference itself on the
records the GPU test uses.  The C ABI declares and exports the new entry points, the size query and the argument checks answer
without a device, the wrappers raise their errors before the device is needed, the fill helpers and the tapers equal the
reference's results."""
import ctypes as C
import os
import re
import warnings

import numpy as np
import pytest
import scipy.integrate
import torch

import calculus_cases as cc
from quantum_inferno_amd import _lib, engine
from quantum_inferno_amd.utilities import calculations, window

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("qi_cumtrapz_scratch_bytes", "qi_cumtrapz", "qi_derivative")


@pytest.fixture(scope="module")
def g(golden):
    return golden("calculus.npz")


def layouts_of(n, records):
    for layout in cc.LAYOUTS:
        yield layout, cc.timestamps(n, layout, records)


def test_restated_terms_equal_scipy_bit_for_bit():
    for dtype in cc.DTYPES:
        for n in cc.LENGTHS:
            y = cc.random_records(n, dtype, 3)
            for layout, ts in layouts_of(n, 3):
                dx = 1 / cc.FS
                want = scipy.integrate.cumulative_trapezoid(y, x=ts, dx=dx, initial=0)
                terms = cc.terms_ref(y, ts, dx)
                assert terms.dtype == want.dtype == np.dtype("float64" if ts is not None else dtype), (dtype, n, layout)
                assert terms.shape == (3, n - 1)
                # SciPy's result is np.cumsum of its terms, left to right: the same terms give the same bits
                got = np.concatenate([np.zeros((3, 1), terms.dtype), np.cumsum(terms, axis=1)], axis=1)
                assert cc.same_bits(got, want), (dtype, n, layout)
                if n == 2:
                    assert cc.same_bits(terms[:, 0], want[:, 1])
    # a float32 sum is rounded to float32 before the float64 product
    y = np.array([[1.0, 2.0 ** -24 * 3]], dtype=np.float32)
    assert cc.terms_ref(y, np.array([0.0, 2.0]))[0, 0] == np.float64(np.float32(1.0) + np.float32(2.0 ** -24 * 3))


def test_restated_derivatives_equal_numpy_bit_for_bit():
    for dtype in cc.DTYPES:
        for n in cc.LENGTHS[1:]:
            y = cc.random_records(n, dtype, 3, salt=1)
            for layout, ts in layouts_of(n, 3):
                for r in range(3):
                    t = None if ts is None else (ts if ts.ndim == 1 else ts[r])
                    if t is None:
                        want = np.gradient(y[r], 1 / cc.FS)
                        got = cc.gradient_ref(y, None, 1 / cc.FS)[r]
                        dwant = np.diff(y[r]) * cc.FS
                        dgot = cc.difference_ref(y, None, cc.FS)[r]
                    else:
                        even = n == 2 or bool((np.diff(t) == np.diff(t)[0]).all())
                        assert even == (n == 2)  # jittered: np.gradient takes its uneven formula
                        want = np.gradient(y[r], t) if not even else cc.gradient_ref(y[r], t)
                        got = cc.gradient_ref(y, ts)[r]
                        dwant = np.diff(y[r]) / np.diff(t)
                        dgot = cc.difference_ref(y, ts)[r]
                        assert dgot.dtype == np.float64
                    assert want.dtype == np.dtype(dtype) and cc.same_bits(got, want), (dtype, n, layout, r)
                    assert cc.same_bits(dgot, dwant), (dtype, n, layout, r)
    # duplicate timestamps divide by zero as NumPy does
    y = np.array([1.0, 2.0, 2.0, 5.0, 4.0], dtype=np.float32)
    t = np.array([0.0, 1.0, 1.0, 1.0, 3.0])
    with np.errstate(all="ignore"):
        assert cc.same_bits(cc.gradient_ref(y, t), np.gradient(y, t)) and cc.same_bits(cc.difference_ref(y, t), np.diff(y) / np.diff(t))
    assert np.isinf(cc.difference_ref(y, t)).any() and np.isnan(cc.difference_ref(y, t)).any()


def test_tree_equals_the_reference_on_exactly_summable_records(g):
    for dtype in cc.DTYPES:
        for n in cc.LENGTHS:
            y = cc.exact_record(n, dtype)[None, :]
            got = cc.cumtrapz_ref(y, None, 1 / cc.EXACT_RATE)[0]
            want = g[cc.exact_key(n, dtype, "rate")]
            assert got.dtype == want.dtype == np.dtype(dtype) and np.array_equal(got, want), (dtype, n)
            for epoch in (False, True):
                got = cc.cumtrapz_ref(y, cc.exact_timestamps(n, epoch))[0]
                assert got.dtype == np.float64 and np.array_equal(got, g[cc.exact_key(n, dtype, "ts")]), (dtype, n, epoch)
            assert np.array_equal(want.astype(np.float64), g[cc.exact_key(n, dtype, "ts")])
            assert np.array_equal(want, cc.exact_sums(cc.terms_ref(y, None, 1 / cc.EXACT_RATE))[0])  # the reference is exact here


def test_both_orders_of_summation_stay_inside_the_bound_and_the_project_tolerances():
    """|result - exact| <= i u sum_(j <= i) |t_j| after i additions, for any order: the backstop.  And the figures the GPU
    test asserts (cc.TOL, of the result's maximum) are met by the reference itself on the records that test uses."""
    for dtype in cc.DTYPES:
        for n in cc.LENGTHS[1:] + (cc.LONG,):
            records = 1 if n == cc.LONG else 3
            y = cc.random_records(n, dtype, records)
            layouts = (("dx", None),) if n == cc.LONG else layouts_of(n, records)
            for layout, ts in layouts:
                terms = cc.terms_ref(y, ts, 1 / cc.FS)
                u = cc.UNIT[str(terms.dtype)]
                exact = cc.exact_sums(terms)
                bound = np.arange(n) * u * np.concatenate([np.zeros((records, 1)), np.cumsum(np.abs(terms.astype(np.float64)), axis=1)], axis=1)
                reference = scipy.integrate.cumulative_trapezoid(y, x=ts, dx=1 / cc.FS, initial=0)
                tree = cc.scan_ref(terms)
                scale = np.max(np.abs(exact), axis=1)
                for name, result in (("reference", reference), ("tree", tree)):
                    err = np.abs(result.astype(np.float64) - exact)
                    assert np.all(err <= bound), (name, dtype, n, layout)
                    worst = np.max(err, axis=1)  # (two zero-mean samples integrate to 0: nothing to divide by)
                    assert np.all(worst <= cc.TOL[str(terms.dtype)] * scale), (name, dtype, n, layout, worst / scale)


def test_tree_gives_the_reference_nan_and_infinities(g):
    for dtype in cc.DTYPES:
        rows = cc.special_records(dtype)
        assert rows.shape == (len(cc.SPECIAL_AT) * 3 + 4, cc.SPECIAL_N)
        for form, ts in (("rate", None), ("ts", cc.timestamps(cc.SPECIAL_N, "shared0"))):
            want = g[f"special_{dtype}_{form}"]
            got = cc.classes(cc.cumtrapz_ref(rows, ts, 1 / cc.FS))
            assert want.shape == got.shape and np.array_equal(got, want), (dtype, form)
            assert {1, 2, 3} <= set(np.unique(want)) and (want[:, 0] == 0).all()
            # a NaN at the last sample of the first tile's terms reaches only what lies behind it
            row = list(cc.SPECIAL_AT).index(cc.T) * 3
            assert (want[row, :cc.T] == 0).all() and (want[row, cc.T:] == 1).all()


def test_header_library_and_binding_agree():
    header = open(os.path.join(ROOT, "include", "qi_tfr.h")).read()
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", header), f"{name} is not declared"
        assert hasattr(lib, name) and name in _lib.PROTOTYPES
    assert int(re.search(r"#define\s+QI_SCAN_TILE\s+(\d+)", header).group(1)) == _lib.SCAN_TILE == cc.T == 4096
    assert cc.T == cc.LANES * cc.RUN and cc.LANES % cc.WAVE == 0
    assert re.search(r"QI_DERIV_GRADIENT\s*=\s*0\s*,\s*QI_DERIV_DIFFERENCE\s*=\s*1", header)
    assert (_lib.QI_DERIV_GRADIENT, _lib.QI_DERIV_DIFFERENCE) == (0, 1)
    assert engine.DERIVATIVE_KINDS == {"gradient": 0, "difference": 1}
    assert lib.qi_abi_version() == 1


def test_scratch_bytes_and_refused_arguments():
    lib = _lib.load()

    def up(v):
        return -(-v // 256) * 256

    for dtype in (_lib.QI_F32, _lib.QI_F64):
        for c, n, tiles in ((1, 1, 1), (1, 2, 1), (1, cc.T + 1, 1), (1, cc.T + 2, 2), (3, 2 * cc.T + 1, 2), (65, 3 * cc.T + 17, 4),
                            (1024, 1 << 20, 256), (1, cc.LONG, 258), (0, 100, 1)):
            assert lib.qi_cumtrapz_scratch_bytes(dtype, c, n) == up(max(c, 1) * tiles * 8), (dtype, c, n)
    assert lib.qi_cumtrapz_scratch_bytes(2, 1, 100) == -1 and b"dtype" in lib.qi_last_error()
    assert lib.qi_cumtrapz_scratch_bytes(_lib.QI_F32, -1, 100) == -1 and b"record count" in lib.qi_last_error()
    assert lib.qi_cumtrapz_scratch_bytes(_lib.QI_F64, 1, 0) == -1 and b"record length" in lib.qi_last_error()
    assert lib.qi_cumtrapz_scratch_bytes(_lib.QI_F64, 1, 1 << 40) == -1 and b"too large" in lib.qi_last_error()
    assert lib.qi_cumtrapz_scratch_bytes(_lib.QI_F64, 1 << 30, 1 << 20) == -1 and b"too large" in lib.qi_last_error()
    buf = np.full(64, 7.0)
    p = buf.ctypes.data_as(C.c_void_p)

    def cumtrapz(dtype=_lib.QI_F64, y=p, x=None, stride=0, c=1, n=8, out=p, scratch=p, nbytes=512):
        return lib.qi_cumtrapz(dtype, 0, y, x, stride, 1.0, c, n, out, scratch, nbytes, None)

    for bad, word in ((dict(dtype=2), b"dtype"), (dict(n=0), b"record length"), (dict(c=-1), b"record count"),
                      (dict(x=p, stride=4), b"x_stride"), (dict(x=p, stride=-8), b"x_stride"), (dict(stride=8), b"x_stride"),
                      (dict(y=None), b"null"), (dict(out=None), b"null"), (dict(scratch=None), b"null"), (dict(nbytes=16), b"needed")):
        assert cumtrapz(**bad) == -1 and word in lib.qi_last_error(), bad
    assert cumtrapz(c=0) == 0 and cumtrapz(c=0, y=None, out=None, scratch=None) == 0  # no records: a successful no-op

    def derivative(dtype=_lib.QI_F64, kind=0, y=p, x=None, stride=0, c=1, n=8, out=p, offset=0):
        return lib.qi_derivative(dtype, 0, kind, y, x, stride, 1.0, c, n, out, offset, None)

    for bad, word in ((dict(dtype=2), b"dtype"), (dict(kind=2), b"kind"), (dict(n=0), b"record length"), (dict(n=1), b"gradient"),
                      (dict(kind=1, n=0), b"record length"), (dict(c=-1), b"record count"), (dict(x=p, stride=4), b"x_stride"),
                      (dict(stride=8), b"x_stride"), (dict(offset=1), b"out_offset"), (dict(kind=1, offset=2), b"out_offset"),
                      (dict(kind=1, offset=-1), b"out_offset"), (dict(y=None), b"null"), (dict(out=None), b"null")):
        assert derivative(**bad) == -1 and word in lib.qi_last_error(), bad
    assert derivative(c=0) == 0 and derivative(kind=1, n=1) == 0  # no records, or one sample and no difference: no-ops
    assert (buf == 7.0).all()


def test_wrappers_refuse_bad_arguments_before_the_device():
    y = np.linspace(-1.0, 1.0, 400)
    t = np.arange(400) / 100.0
    for value in (1, 0.5, -1.0):
        with pytest.raises(ValueError, match="`initial` must be `None` or `0`."):
            calculations.integrate_with_cumtrapz_sample_rate_hz(100.0, y, value)
        with pytest.raises(ValueError, match="`initial` must be `None` or `0`."):
            calculations.integrate_with_cumtrapz_timestamps_s(t, y, initial_value=value)
    with pytest.raises(ValueError, match="At least one point is required"):
        calculations.integrate_with_cumtrapz_sample_rate_hz(100.0, np.zeros(0))
    with pytest.raises(ValueError, match=r"\[n\] or \[channels, n\]"):
        calculations.integrate_with_cumtrapz_sample_rate_hz(100.0, np.zeros((2, 3, 4)))
    with pytest.raises(ValueError, match="timestamps must be"):
        calculations.integrate_with_cumtrapz_timestamps_s(t[:-1], y)
    with pytest.raises(ValueError, match="timestamps must be"):
        engine.cumulative_trapezoid(torch.zeros(3, 400), torch.zeros(2, 400))
    with pytest.raises(ValueError, match="timestamps must be"):
        engine.derivative(y, np.stack([t, t]))
    with pytest.raises(ValueError, match="kind must be one of"):
        engine.derivative(y, kind="central")
    with pytest.raises(ValueError, match="fill_at must be"):
        engine.derivative(y, kind="difference", fill_at="middle")
    # one sample has no gradient: NumPy's message
    for call in (lambda: calculations.derivative_with_gradient_sample_rate_hz(100.0, y[:1]),
                 lambda: calculations.derivative_with_gradient_timestamps_s(t[:1], y[:1]), lambda: engine.derivative(y[:1])):
        with pytest.raises(ValueError, match="Shape of array too small to calculate a numerical gradient"):
            call()
    with pytest.raises(ValueError, match="Shape of array too small"):
        np.gradient(y[:1], 0.01)
    for fn, first in ((calculations.derivative_with_difference_sample_rate_hz, 100.0), (calculations.derivative_with_difference_timestamps_s, t)):
        with pytest.raises(ValueError, match=r"Invalid fill type mode, must be one of \['zero', 'nan', 'mean', 'median', 'min', 'max', 'tail', 'head'\]"):
            fn(first, y, "mode")
        with pytest.raises(ValueError, match=r"Invalid fill location middle, must be one of \['start', 'end'\]"):
            fn(first, y, "zero", "middle")
    with pytest.raises(ValueError, match=r"array_1d has shape \(2, 3\) but should be a 1D array"):
        calculations.get_fill_from_filling_method(np.zeros((2, 3)), "zero")
    with pytest.raises(ValueError, match="Invalid fill type mode"):
        calculations.get_fill_from_filling_method(np.zeros(3), "mode")
    with pytest.raises(ValueError, match="Invalid fill location middle"):
        calculations.append_fill(np.zeros(3), 0.0, "middle")
    assert calculations.FILL_LOCATIONS == list(cc.FILL_LOCATIONS) and calculations.FILL_TYPES == list(cc.FILL_TYPES)


def test_one_sample_is_answered_as_the_reference_answers_it(g):
    """np.diff of one sample is empty: "zero" and "nan" pad it, "mean" and "median" give NaN (NumPy warns), "min" and "max"
    raise NumPy's ValueError and "head" and "tail" its IndexError -- on the host, no device needed."""
    y = np.array([1.5])
    for fill_loc in cc.FILL_LOCATIONS:
        for fill_type in ("zero", "nan", "mean", "median"):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                got = calculations.derivative_with_difference_sample_rate_hz(cc.FS, y, fill_type, fill_loc)
                got_t = calculations.derivative_with_difference_timestamps_s(np.array([3.0]), y, fill_type, fill_loc)
            assert cc.same_bits(got, g[f"one_{fill_type}_{fill_loc}"]) and cc.same_bits(got_t, got), (fill_type, fill_loc)
            assert got.shape == (1,)
        for fill_type in ("min", "max"):
            with pytest.raises(ValueError, match="zero-size array"):
                calculations.derivative_with_difference_sample_rate_hz(cc.FS, y, fill_type, fill_loc)
        for fill_type in ("head", "tail"):
            with pytest.raises(IndexError):
                calculations.derivative_with_difference_sample_rate_hz(cc.FS, y, fill_type, fill_loc)
    # the integral of one sample is its start
    assert np.array_equal(scipy.integrate.cumulative_trapezoid(y, dx=1.0, initial=0), [0.0])
    assert np.array_equal(cc.cumtrapz_ref(y[None, :])[0], [0.0])


def test_fill_helpers_equal_the_reference_on_the_host(g):
    for dtype in cc.DTYPES:
        for with_nan in (False, True):
            y = cc.fill_record(dtype, with_nan)
            for form, d in (("rate", cc.difference_ref(y, None, cc.FS)), ("ts", cc.difference_ref(y, cc.fill_timestamps()))):
                for fill_type in cc.FILL_TYPES:
                    for fill_loc in cc.FILL_LOCATIONS:
                        got = calculations.append_fill(d, calculations.get_fill_from_filling_method(d, fill_type), fill_loc)
                        want = g[cc.fill_key(dtype, form, fill_type, fill_loc, with_nan)]
                        assert len(want) == cc.FILL_N and cc.same_bits(got, want), (dtype, form, fill_type, fill_loc, with_nan)
    # np.append of a Python number widens a float32 derivative, np.insert does not: the result types the wrappers follow
    assert g[cc.fill_key("float32", "rate", "zero", "end")].dtype == np.float64
    assert g[cc.fill_key("float32", "rate", "nan", "end")].dtype == np.float64
    assert g[cc.fill_key("float32", "rate", "zero", "start")].dtype == np.float32
    assert g[cc.fill_key("float32", "rate", "mean", "end")].dtype == np.float32
    assert np.isnan(g[cc.fill_key("float64", "rate", "median", "end", True)][-1])


def test_tapers_equal_the_reference_bit_for_bit(g, capsys):
    for points, alpha in cc.WINDOW_CASES:
        got = window.get_tukey(np.zeros(points), alpha)
        assert cc.same_bits(got, g[f"tukey_{points}_{alpha}"]), (points, alpha)
    assert cc.same_bits(window.get_tukey(np.zeros((4, 16)), 0.5), window.get_tukey(np.zeros(64), 0.5))  # np.size of the array
    capsys.readouterr()
    for points, taper_num, alpha in cc.BUFFER_CASES:
        got = window.get_tukey_by_buffer_num(np.zeros(points), taper_num, alpha)
        assert len(got) == points and cc.same_bits(got, g[f"buffer_{points}_{taper_num}_{alpha}"]), (points, taper_num, alpha)
    for points, taper_s, rate, alpha in cc.BUFFER_S_CASES:
        got = window.get_tukey_by_buffer_s(np.zeros(points), taper_s, rate, alpha)
        assert len(got) == points and cc.same_bits(got, g[f"buffer_s_{points}_{taper_s}_{rate}_{alpha}"]), (points, taper_s)
    printed = capsys.readouterr().out.splitlines()
    assert printed == list(g["window_warnings"]) and len(printed) == 3
    assert printed[0] == "Warning: array length 20 is less than taper_num 22. Using full array length."
