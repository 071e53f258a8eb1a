"""Integration and differentiation on the GPU.  qi_cumtrapz through ctypes: bit for bit against the NumPy restatement of its
summation tree (calculus_cases.scan_ref) for every record length, record count, dtype and timestamp layout of the matrix
and one record of more than 256 tiles; equal to the reference's recorded results (tests/golden/calculus.npz) on exactly
summable records; the reference's NaN and infinities; the same bits for a record alone, in row 0 and in row 64 of 65 and
on a second call; within the project's tolerances of the exact running sum.  qi_derivative of both kinds bit for bit
against NumPy itself.  Refused calls write nothing.  The six reference-signature wrappers end to end.  Every buffer is
pre-filled with a sentinel and carries a guard element."""
import numpy as np
import pytest
import torch

import calculus_cases as cc
from quantum_inferno_amd import _lib, engine
from quantum_inferno_amd.utilities import calculations

pytestmark = pytest.mark.gpu

GUARD = 1          # elements behind each buffer that the call must leave alone
FILL = 2.0 ** 100  # (a float32 as well; no result comes near it)


@pytest.fixture(scope="module")
def g(golden):
    return golden("calculus.npz")


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def cumtrapz(y, x=None, dx=1.0, expect=0, override=None):
    """qi_cumtrapz on device tensors y [C, n], x None, [n] or [C, n] -> out [C, n] on the host, after checking that every
    output was written and no guard was.  `expect`: the status the call must return (then -> None); `override`: arguments
    of the C call to replace (the buffers stay those of the shapes given here)."""
    lib = _lib.require_gpu()
    d = y.device
    n_ch, n = y.shape
    code = _lib.QI_F64 if y.dtype == torch.float64 else _lib.QI_F32
    need = int(lib.qi_cumtrapz_scratch_bytes(code, n_ch, n))
    assert need > 0
    out = torch.full((n_ch * n + GUARD,), FILL, dtype=torch.float64 if x is not None else y.dtype, device=d)
    scratch = torch.full((need // 8 + GUARD,), FILL, dtype=torch.float64, device=d)
    a = dict(dtype=code, y=_lib.ptr(y), x=_lib.ptr(x), stride=n if x is not None and x.dim() == 2 else 0, dx=float(dx), c=n_ch, n=n,
             out=_lib.ptr(out), scratch=_lib.ptr(scratch), nbytes=need)
    a.update(override or {})
    keep = y.clone()
    with torch.cuda.device(d):
        rc_ = lib.qi_cumtrapz(a["dtype"], d.index, a["y"], a["x"], a["stride"], a["dx"], a["c"], a["n"], a["out"], a["scratch"],
                              a["nbytes"], _lib.stream_ptr(d))
    torch.cuda.synchronize(d)
    assert rc_ == expect, (rc_, lib.qi_last_error())
    assert out[-1].item() == FILL and scratch[-1].item() == FILL, "a guard was written"
    assert torch.equal(y.view(torch.int32), keep.view(torch.int32)), "the records were overwritten"
    if expect != 0:
        assert (out == FILL).all() and (scratch == FILL).all(), "a refused call wrote"
        return None
    got = out[:-GUARD].view(n_ch, n).cpu().numpy()
    assert not (got == FILL).any(), "an output was not written"
    return got


def derivative(kind, y, x=None, h=1.0, offset=0, expect=0, override=None):
    """qi_derivative on device tensors -> out [C, n] on the host with the fill slot of a difference still the sentinel."""
    lib = _lib.require_gpu()
    d = y.device
    n_ch, n = y.shape
    code = _lib.QI_F64 if y.dtype == torch.float64 else _lib.QI_F32
    difference = kind == _lib.QI_DERIV_DIFFERENCE
    out = torch.full((n_ch * n + GUARD,), FILL, dtype=torch.float64 if difference and x is not None else y.dtype, device=d)
    a = dict(dtype=code, kind=kind, y=_lib.ptr(y), x=_lib.ptr(x), stride=n if x is not None and x.dim() == 2 else 0, h=float(h), c=n_ch,
             n=n, out=_lib.ptr(out), offset=offset)
    a.update(override or {})
    with torch.cuda.device(d):
        rc_ = lib.qi_derivative(a["dtype"], d.index, a["kind"], a["y"], a["x"], a["stride"], a["h"], a["c"], a["n"], a["out"], a["offset"],
                                _lib.stream_ptr(d))
    torch.cuda.synchronize(d)
    assert rc_ == expect, (rc_, lib.qi_last_error())
    assert out[-1].item() == FILL, "the guard was written"
    if expect != 0:
        assert (out == FILL).all(), "a refused call wrote"
        return None
    got = out[:-GUARD].view(n_ch, n).cpu().numpy()
    if difference:
        slot = 0 if offset else n - 1
        assert (got[:, slot] == FILL).all(), "the fill slot was written"
        got = np.delete(got, slot, axis=1)
    assert not (got == FILL).any(), "an output was not written"
    return got


def report(where, got, want):
    if not cc.same_bits(got, want):
        with np.errstate(all="ignore"):
            fin = np.isfinite(want) & np.isfinite(got)
            diff = np.max(np.abs(got[fin].astype(np.float64) - want[fin]), initial=0.0)
        print(f"{where}: dtypes {got.dtype} / {want.dtype}, max |difference| {diff:.3e}, "
              f"{int(np.sum(got != want))} of {want.size} differ (bit for bit asked)")
    assert cc.same_bits(got, want), where


@pytest.mark.parametrize("dtype", cc.DTYPES)
def test_scan_equals_the_restatement_bit_for_bit_and_meets_the_tolerances(dtype):
    worst = {"float64": 0.0, "float32": 0.0}
    cases = [(n, records, layout) for n in cc.LENGTHS for records in cc.RECORDS for layout in cc.LAYOUTS]
    cases += [(cc.LONG, 1, "dx"), (cc.LONG, 1, "shared0")]
    for n, records, layout in cases:
        y = cc.random_records(n, dtype, records)
        ts = cc.timestamps(n, layout, records)
        got = cumtrapz(dev(y), dev(ts), 1 / cc.FS)
        terms = cc.terms_ref(y, ts, 1 / cc.FS)
        report(f"{dtype} n {n} records {records} {layout}", got, cc.scan_ref(terms))
        exact = cc.exact_sums(terms)
        err, scale = np.max(np.abs(got.astype(np.float64) - exact), axis=1), np.max(np.abs(exact), axis=1)
        tol = cc.TOL[str(got.dtype)]
        if np.any(scale > 0):
            worst[str(got.dtype)] = max(worst[str(got.dtype)], np.max(err[scale > 0] / scale[scale > 0]))
        assert np.all(err <= tol * scale), (n, records, layout, err / scale)
    print(f"{dtype} records: largest deviation from the exact running sum, of the result's maximum: "
          f"float64 results {worst['float64']:.3e} (bound {cc.TOL['float64']:.0e}), float32 results {worst['float32']:.3e} "
          f"(bound {cc.TOL['float32']:.0e})")


@pytest.mark.parametrize("dtype", cc.DTYPES)
def test_exactly_summable_records_equal_the_reference(g, dtype):
    for n in cc.LENGTHS:
        y, factors = cc.batch_of(cc.exact_record(n, dtype), 3)
        got = cumtrapz(dev(y), None, 1 / cc.EXACT_RATE)
        want = g[cc.exact_key(n, dtype, "rate")]
        assert got.dtype == want.dtype and np.array_equal(got, factors[:, None] * want[None, :]), (dtype, n)
        for epoch in (False, True):
            ts = cc.exact_timestamps(n, epoch)
            want = factors[:, None] * g[cc.exact_key(n, dtype, "ts")][None, :]
            assert np.array_equal(cumtrapz(dev(y), dev(ts)), want), (dtype, n, epoch)
            assert np.array_equal(cumtrapz(dev(y), dev(np.tile(ts, (3, 1)))), want), (dtype, n, epoch)


@pytest.mark.parametrize("dtype", cc.DTYPES)
def test_nan_and_infinities_where_the_reference_has_them(g, dtype):
    rows = cc.special_records(dtype)
    for form, ts in (("rate", None), ("ts", cc.timestamps(cc.SPECIAL_N, "shared0"))):
        got = cumtrapz(dev(rows), dev(ts), 1 / cc.FS)
        assert np.array_equal(cc.classes(got), g[f"special_{dtype}_{form}"]), (dtype, form)
        report(f"{dtype} special {form}", got, cc.cumtrapz_ref(rows, ts, 1 / cc.FS))


@pytest.mark.parametrize("dtype", cc.DTYPES)
def test_a_record_gives_the_same_bits_alone_and_in_any_row(dtype):
    n = 3 * cc.T + 17
    others = cc.random_records(n, dtype, 65, salt=2)
    one = cc.random_records(n, dtype, 1)
    for layout in ("dx", "sharedE", "rowsE"):
        ts = cc.timestamps(n, layout, 65)
        rows = ts is not None and ts.ndim == 2
        alone = cumtrapz(dev(one), dev(ts[40:41] if rows else ts), 1 / cc.FS)
        for row in (0, 64):
            batch = others.copy()
            batch[row] = one[0]
            tsb = ts
            if rows:
                tsb = ts.copy()
                tsb[row] = ts[40]
            got = cumtrapz(dev(batch), dev(tsb), 1 / cc.FS)
            assert cc.same_bits(got[row], alone[0]), (dtype, layout, row)
            assert cc.same_bits(cumtrapz(dev(batch), dev(tsb), 1 / cc.FS), got), (dtype, layout, row)  # a second call


@pytest.mark.parametrize("dtype", cc.DTYPES)
def test_derivatives_equal_numpy_bit_for_bit(dtype):
    grad, diff = _lib.QI_DERIV_GRADIENT, _lib.QI_DERIV_DIFFERENCE
    for n in cc.LENGTHS[1:]:
        for records in cc.RECORDS:
            y = cc.random_records(n, dtype, records, salt=1)
            for layout in cc.LAYOUTS:
                ts = cc.timestamps(n, layout, records)
                where = f"{dtype} n {n} records {records} {layout}"
                got = derivative(grad, dev(y), dev(ts), 1 / cc.FS)
                for r in {0, records // 2, records - 1}:
                    t = None if ts is None else (ts if ts.ndim == 1 else ts[r])
                    with np.errstate(all="ignore"):
                        want = np.gradient(y[r], 1 / cc.FS) if t is None else (np.gradient(y[r], t) if n > 2 else cc.gradient_ref(y[r], t))
                        dwant = np.diff(y[r]) * cc.FS if t is None else np.diff(y[r]) / np.diff(t)
                    report(where + f" gradient, record {r}", got[r], want)
                report(where + " gradient", got, cc.gradient_ref(y, ts, 1 / cc.FS))
                for offset in (0, 1):
                    got = derivative(diff, dev(y), dev(ts), cc.FS, offset)
                    report(where + f" difference at {offset}", got, cc.difference_ref(y, ts, cc.FS))
                    report(where + f" difference at {offset}, record {r} against NumPy", got[r], dwant)
    # duplicate timestamps: division by zero gives inf and NaN where NumPy gives them
    n = 1025
    y = cc.random_records(n, dtype, 3, salt=4)
    ts = cc.timestamps(n, "sharedE")
    ts[40:44] = ts[40]
    ts[1000] = ts[999]
    y[:, 41] = y[:, 40]  # 0 / 0
    with np.errstate(all="ignore"):
        want = np.stack([np.gradient(row, ts) for row in y])
        dwant = np.stack([np.diff(row) / np.diff(ts) for row in y])
    assert np.isinf(want).any() and np.isnan(want).any() and np.isinf(dwant).any() and np.isnan(dwant).any()
    report(f"{dtype} duplicate timestamps, gradient", derivative(grad, dev(y), dev(ts)), want)
    report(f"{dtype} duplicate timestamps, difference", derivative(diff, dev(y), dev(ts), 1.0, 1), dwant)
    assert derivative(diff, dev(y[:, :1]), None, cc.FS).shape == (3, 0)  # one sample: no difference, nothing written


def test_refused_calls_write_nothing():
    lib = _lib.require_gpu()
    y = dev(cc.random_records(cc.T + 2, "float64", 2))
    ts = dev(cc.timestamps(cc.T + 2, "shared0"))
    for bad, word in ((dict(dtype=2), b"dtype"), (dict(n=0), b"record length"), (dict(c=-1), b"record count"),
                      (dict(stride=cc.T), b"x_stride"), (dict(y=None), b"null"), (dict(out=None), b"null"),
                      (dict(scratch=None), b"null"), (dict(nbytes=8), b"needed")):
        assert cumtrapz(y, ts, expect=-1, override=bad) is None
        assert word in lib.qi_last_error(), bad
    assert cumtrapz(y, None, expect=-1, override=dict(stride=cc.T + 2)) is None and b"x_stride" in lib.qi_last_error()
    for bad, word in ((dict(dtype=2), b"dtype"), (dict(kind=2), b"kind"), (dict(n=0), b"record length"), (dict(n=1), b"gradient"),
                      (dict(c=-1), b"record count"), (dict(stride=3), b"x_stride"), (dict(offset=1), b"out_offset"),
                      (dict(kind=1, offset=2), b"out_offset"), (dict(y=None), b"null"), (dict(out=None), b"null")):
        assert derivative(_lib.QI_DERIV_GRADIENT, y, ts, expect=-1, override=bad) is None
        assert word in lib.qi_last_error(), bad


def test_no_records_is_a_successful_no_op():
    lib = _lib.require_gpu()
    d = torch.device("cuda", torch.cuda.current_device())
    buf = torch.full((64,), FILL, dtype=torch.float64, device=d)
    p = _lib.ptr(buf)
    with torch.cuda.device(d):
        assert lib.qi_cumtrapz(_lib.QI_F64, d.index, p, None, 0, 1.0, 0, 8, p, p, 512, _lib.stream_ptr(d)) == 0
        assert lib.qi_derivative(_lib.QI_F64, d.index, 0, p, None, 0, 1.0, 0, 8, p, 0, _lib.stream_ptr(d)) == 0
        assert lib.qi_derivative(_lib.QI_F64, d.index, 1, p, None, 0, 1.0, 0, 8, p, 1, _lib.stream_ptr(d)) == 0
    torch.cuda.synchronize(d)
    assert (buf == FILL).all()
    assert engine.cumulative_trapezoid(torch.zeros((0, 8), device=d)).shape == (0, 8)
    assert engine.derivative(torch.zeros((0, 8), device=d), kind="difference").shape == (0, 8)


def test_integration_wrappers_end_to_end(g):
    for dtype in cc.DTYPES:
        tdtype = torch.float64 if dtype == "float64" else torch.float32
        for n in cc.WRAP_LENGTHS:
            y = cc.random_records(n, dtype)[0]
            ts = cc.timestamps(n, "sharedE")
            batch, factors = cc.batch_of(y, 3)
            for form, first, want1 in (("rate", cc.FS, g[f"rand_{dtype}_rate_n{n}"]), ("ts", ts, g[f"rand_{dtype}_ts_n{n}"])):
                fn = calculations.integrate_with_cumtrapz_sample_rate_hz if form == "rate" else calculations.integrate_with_cumtrapz_timestamps_s
                tree = cc.cumtrapz_ref(y[None, :], ts if form == "ts" else None, 1 / cc.FS)[0]
                tol = cc.TOL[str(want1.dtype)] * np.max(np.abs(want1))
                got = fn(first, y)
                assert isinstance(got, np.ndarray) and got.shape == (n,)
                report(f"{dtype} {form} n {n} NumPy 1-D", got, tree)
                assert got.dtype == want1.dtype and np.max(np.abs(got.astype(np.float64) - want1)) <= tol
                got = fn(first, batch)
                report(f"{dtype} {form} n {n} NumPy 2-D", got, cc.cumtrapz_ref(batch, ts if form == "ts" else None, 1 / cc.FS))
                tfirst = dev(first) if form == "ts" else first
                got = fn(tfirst, dev(y))
                assert got.is_cuda and got.shape == (n,) and got.dtype == (torch.float64 if form == "ts" else tdtype)
                report(f"{dtype} {form} n {n} tensor 1-D", got.cpu().numpy(), tree)
                got = fn(tfirst, dev(batch))
                assert got.is_cuda and got.shape == (3, n)
                assert np.max(np.abs(got.cpu().numpy().astype(np.float64) - factors[:, None] * want1[None, :])) <= 4 * tol
                assert fn(first, y, initial_value=None).shape == (n - 1,)
    # a NumPy float64 rate is no weak scalar: the reference returns float64 for a float32 record, and so does the wrapper
    y = cc.random_records(1025, "float32")[0]
    got = calculations.integrate_with_cumtrapz_sample_rate_hz(np.float64(cc.FS), y)
    want = g["rand_float32_rate_n1025"].astype(np.float64)
    assert got.dtype == np.float64 and np.max(np.abs(got - want)) <= cc.TOL["float32"] * np.max(np.abs(want))
    got = calculations.integrate_with_cumtrapz_sample_rate_hz(cc.FS, (y * 1000).astype(np.int16))  # integers are read as float64
    assert got.dtype == np.float64 and got.shape == (1025,)
    per_record = engine.cumulative_trapezoid(dev(cc.batch_of(y, 3)[0]), dev(cc.timestamps(1025, "rowsE", 3)))
    assert per_record.is_cuda and per_record.dtype == torch.float64 and per_record.shape == (3, 1025)


def test_derivative_wrappers_end_to_end(g):
    for dtype in cc.DTYPES:
        n = cc.GRAD_N
        y = cc.random_records(n, dtype)[0]
        ts = cc.timestamps(n, "sharedE")
        batch, factors = cc.batch_of(y, 3)
        for form, first in (("rate", cc.FS), ("ts", ts)):
            fn = calculations.derivative_with_gradient_sample_rate_hz if form == "rate" else calculations.derivative_with_gradient_timestamps_s
            want = g[f"grad_{dtype}_{form}_n{n}"]
            got = fn(first, y)
            assert isinstance(got, np.ndarray)
            report(f"gradient {dtype} {form} NumPy 1-D", got, want)
            report(f"gradient {dtype} {form} NumPy 2-D", fn(first, batch), (factors[:, None] * want[None, :]).astype(want.dtype))
            tfirst = dev(first) if form == "ts" else first
            got = fn(tfirst, dev(y))
            assert got.is_cuda
            report(f"gradient {dtype} {form} tensor 1-D", got.cpu().numpy(), want)
            report(f"gradient {dtype} {form} tensor 2-D", fn(tfirst, dev(batch)).cpu().numpy(), (factors[:, None] * want[None, :]).astype(want.dtype))
        # evenly spaced timestamps: np.gradient's formula for even samples (float64 records: its bits)
        even = 100.0 + np.arange(n) / 1024.0
        got = calculations.derivative_with_gradient_timestamps_s(even, y)
        want = np.gradient(y, even)
        if dtype == "float64":
            report("gradient over even timestamps", got, want)
            report("gradient over even timestamps, tensors", calculations.derivative_with_gradient_timestamps_s(dev(even), dev(y)).cpu().numpy(), want)
        else:
            assert got.dtype == np.float32 and np.max(np.abs(got - want)) <= 2.0 ** -23 * np.max(np.abs(want))
        for with_nan in (False, True):
            y = cc.fill_record(dtype, with_nan)
            ts = cc.fill_timestamps()
            batch, factors = cc.batch_of(y, 3)
            for form, first in (("rate", cc.FS), ("ts", ts)):
                fn = calculations.derivative_with_difference_sample_rate_hz if form == "rate" else calculations.derivative_with_difference_timestamps_s
                tfirst = dev(first) if form == "ts" else first
                for fill_type in cc.FILL_TYPES:
                    for fill_loc in cc.FILL_LOCATIONS:
                        want = g[cc.fill_key(dtype, form, fill_type, fill_loc, with_nan)]
                        where = f"difference {dtype} {form} {fill_type} {fill_loc} nan {with_nan}"
                        slot = 0 if fill_loc == "start" else cc.FILL_N - 1
                        want2 = (factors[:, None] * want[None, :]).astype(want.dtype)
                        if fill_type == "zero":
                            want2[:, slot] = 0.0  # (not -0.0)
                        if fill_type in ("min", "max"):  # a negative factor swaps them
                            d = np.delete(want2, slot, axis=1)
                            with np.errstate(all="ignore"):
                                want2[:, slot] = np.min(d, axis=1) if fill_type == "min" else np.max(d, axis=1)
                        results = ((fn(first, y, fill_type, fill_loc), want), (fn(tfirst, dev(y), fill_type, fill_loc).cpu().numpy(), want),
                                   (fn(first, batch, fill_type, fill_loc), want2),
                                   (fn(tfirst, dev(batch), fill_type, fill_loc).cpu().numpy(), want2))
                        for got, wanted in results:
                            if fill_type == "mean" and not with_nan:
                                # any order of summation is within n u mean|d| of the mean
                                d = np.delete(np.atleast_2d(wanted), slot, axis=1).astype(np.float64)
                                bound = cc.FILL_N * cc.UNIT[str(wanted.dtype)] * np.mean(np.abs(d), axis=1)
                                fills = np.atleast_2d(got)[:, slot].astype(np.float64) - np.atleast_2d(wanted)[:, slot]
                                print(f"{where}: mean off by {np.max(np.abs(fills)):.3e} (bound {np.min(bound):.3e})")
                                assert np.all(np.abs(fills) <= bound), where
                                got = got.copy()
                                got[..., slot] = wanted[..., slot]
                            report(where, got, wanted)
