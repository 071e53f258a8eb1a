"""Decimation on the GPU: qi_decimate through ctypes with the fixture's tables against the reference's results bit for bit
(every factor, length and dtype of tests/golden/decimate.npz, 1, 3 and 65 records), its determinism, the cross-check
against the merged zero-phase filter, its argument checks, and the reference-signature wrappers end to end."""
import numpy as np
import pytest
import torch

import decimate_cases as dc
from quantum_inferno_amd import _lib, engine
from quantum_inferno_amd.utilities import sampling

pytestmark = pytest.mark.gpu

GUARD = 1  # columns of out past the result that the call must leave alone


def decimate(x, q, sos, zi, edge, n=None, extra_scratch=0, short_scratch=0, expect=0):
    """qi_decimate on a device tensor x [C, n] -> the whole out buffer [C * m + GUARD] of x's dtype, pre-filled with NaN
    (device); `expect`: the status the call must return."""
    lib = _lib.require_gpu()
    dev = x.device
    n_ch = x.shape[0]
    n = x.shape[1] if n is None else n
    real = np.float64 if x.dtype == torch.float64 else np.float32
    code = _lib.QI_F64 if x.dtype == torch.float64 else _lib.QI_F32
    sos = np.ascontiguousarray(sos, dtype=real)
    zi = np.ascontiguousarray(zi, dtype=real)
    size = x.element_size()
    need = int(lib.qi_decimate_scratch_bytes(code, n_ch, n, edge))
    words = (need // size if need > 0 else n_ch * (n + 2 * abs(edge))) + extra_scratch
    m = dc.columns(n, max(q, 1))
    scratch = torch.full((words,), float("nan"), dtype=x.dtype, device=dev)
    out = torch.full((n_ch * m + GUARD,), float("nan"), dtype=x.dtype, device=dev)
    with torch.cuda.device(dev):
        rc = lib.qi_decimate(code, dev.index, _lib.ptr(x), n_ch, n, q, sos.shape[0], sos.ctypes.data, zi.ctypes.data, edge,
                             _lib.ptr(out), _lib.ptr(scratch), words * size - short_scratch, _lib.stream_ptr(dev))
    torch.cuda.synchronize(dev)
    assert rc == expect, (rc, lib.qi_last_error())
    return out


def result(out, n_ch):
    """The [C, m] result of decimate()'s buffer, after checking that every column is written and the guard is not."""
    body, guard = out[:-GUARD], out[-GUARD:]
    assert torch.isnan(guard).all(), "the guard column was written"
    assert not torch.isnan(body).any(), "a column of the result was not written"
    return body.view(n_ch, -1)


def same_bits(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    bits = torch.int64 if a.dtype == torch.float64 else torch.int32
    return torch.equal(a.contiguous().view(bits), b.contiguous().view(bits))


@pytest.mark.parametrize("dtype", dc.DTYPES)
@pytest.mark.parametrize("q", dc.FACTORS)
def test_decimate_equals_the_reference_bit_for_bit(golden, q, dtype):
    g = golden("decimate.npz")
    sos, zi, edge = dc.tables(g, q, dtype)
    for n in dc.LENGTHS:
        x = torch.from_numpy(g[dc.key(q, dtype, n, "x")]).cuda()
        y = torch.from_numpy(g[dc.key(q, dtype, n, "y")]).cuda()
        for records in (1, dc.RECORDS):
            out = result(decimate(x[:records].contiguous(), q, sos, zi, edge), records)
            assert out.dtype == x.dtype and tuple(out.shape) == (records, dc.columns(n, q))
            diff = (out - y[:records]).abs().max().item()
            print(f"q={q} {dtype} n={n} records={records}: max |difference| {diff:.3e}")
            assert same_bits(out, y[:records]), (q, dtype, n, records, diff)


@pytest.mark.parametrize("dtype", dc.DTYPES)
@pytest.mark.parametrize("q", dc.FACTORS)
def test_batch_across_a_wavefront(golden, q, dtype):
    """65 records, the fixture's three cyclically, row r scaled by 2^(r mod 4): every row is the fixture's result times the
    same power of two, bit for bit (a lane mistake, or one in the second workgroup, shows)."""
    g = golden("decimate.npz")
    sos, zi, edge = dc.tables(g, q, dtype)
    rows = torch.arange(65, device="cuda")
    for n in dc.LENGTHS:
        x = torch.from_numpy(g[dc.key(q, dtype, n, "x")]).cuda()
        y = torch.from_numpy(g[dc.key(q, dtype, n, "y")]).cuda()
        gain = torch.pow(2.0, (rows % 4).to(x.dtype))[:, None]
        xb = (x[rows % dc.RECORDS] * gain).contiguous()  # exact: a power of two
        out = result(decimate(xb, q, sos, zi, edge), 65)
        want = y[rows % dc.RECORDS] * gain
        bad = [r for r in range(65) if not same_bits(out[r], want[r])]
        assert not bad, (q, dtype, n, bad)


def test_same_bits_when_repeated_and_with_more_scratch(golden):
    g = golden("decimate.npz")
    for q, dtype in ((5, "float64"), (13, "float32")):
        sos, zi, edge = dc.tables(g, q, dtype)
        x = torch.from_numpy(g[dc.key(q, dtype, 1031, "x")]).cuda()
        y = torch.from_numpy(g[dc.key(q, dtype, 1031, "y")]).cuda()
        first = result(decimate(x, q, sos, zi, edge), dc.RECORDS)
        assert same_bits(first, y)
        assert same_bits(result(decimate(x, q, sos, zi, edge), dc.RECORDS), first)
        assert same_bits(result(decimate(x, q, sos, zi, edge, extra_scratch=4099), dc.RECORDS), first)


@pytest.mark.parametrize("q", dc.FACTORS)
def test_float64_is_the_merged_filter_every_qth_sample(golden, q):
    """The decimating store against the kernel that stores every sample: in float64 the two are the same arithmetic."""
    g = golden("decimate.npz")
    sos, zi, edge = dc.tables(g, q, "float64")
    for n in dc.LENGTHS:
        x = torch.from_numpy(g[dc.key(q, "float64", n, "x")]).cuda()
        full = engine.zero_phase_filter(x, "sos", sos, zi, edge)
        assert full.dtype == torch.float64 and tuple(full.shape) == (dc.RECORDS, n)
        out = result(decimate(x, q, sos, zi, edge), dc.RECORDS)
        assert same_bits(out, full[:, ::q].contiguous()), (q, n)
        assert same_bits(engine.zero_phase_decimate(x, q, sos, zi, edge), out), (q, n)


def test_bad_arguments_are_refused(golden):
    g = golden("decimate.npz")
    lib = _lib.load()
    sos, zi, edge = dc.tables(g, 5, "float64")
    x = torch.from_numpy(g[dc.key(5, "float64", 300, "x")]).cuda()
    decimate(x, 5, sos, zi, edge, n=edge, expect=-1)  # n == edge: QI_ERR_ARG
    assert b"longer than the extension" in lib.qi_last_error()
    result(decimate(x, 5, sos, zi, edge, n=edge + 1), dc.RECORDS)  # the shortest legal record (of the same buffer)
    decimate(x, 0, sos, zi, edge, expect=-1)  # q == 0
    decimate(x, -2, sos, zi, edge, expect=-1)
    decimate(x, 5, np.tile(sos, (5, 1))[:17], np.zeros((17, 2)), edge, expect=-1)  # 17 sections
    bad = sos.copy()
    bad[2, 3] = 0.5
    decimate(x, 5, bad, zi, edge, expect=-1)  # a0 != 1
    decimate(x, 5, sos, zi, edge, short_scratch=1, expect=-1)  # scratch one byte short
    assert b"scratch" in lib.qi_last_error()
    sos32, zi32, _ = dc.tables(g, 5, "float32")
    x32 = x.to(torch.float32)
    decimate(x32, 5, sos32, zi32, edge, short_scratch=1, expect=-1)
    result(decimate(x32, 5, sos32, zi32, edge), dc.RECORDS)


@pytest.mark.parametrize("dtype", dc.DTYPES)
@pytest.mark.parametrize("q", dc.FACTORS)
def test_wrappers_end_to_end(golden, q, dtype):
    """Design on this host, filter and decimation on the device, against the reference's results: within
    4 sens + 16 eps_T of each record's largest value (sens: what one ulp of T in every table entry does to the
    reference's own result; eps_T = 2^-52 or 2^-23; 0 is expected where NumPy reproduces the tables' bits)."""
    g = golden("decimate.npz")
    for n in dc.LENGTHS:
        x = g[dc.key(q, dtype, n, "x")]
        y = g[dc.key(q, dtype, n, "y")]
        tol = (4.0 * g[dc.key(q, dtype, n, "sens")] + 16.0 * dc.EPS[dtype]) * np.max(np.abs(y.astype(np.float64)), axis=1)
        rows = sampling.decimate_timeseries_collection(x, q)  # NumPy [C, n] in
        assert isinstance(rows, np.ndarray) and rows.dtype == x.dtype and rows.shape == y.shape
        one = sampling.decimate_timeseries(x[1], q)  # NumPy [n] in
        assert isinstance(one, np.ndarray) and one.dtype == x.dtype and one.shape == (dc.columns(n, q),)
        dev = sampling.decimate_timeseries_collection(torch.from_numpy(x).cuda(), q)  # CUDA tensor in
        assert isinstance(dev, torch.Tensor) and dev.is_cuda and dev.dtype == torch.from_numpy(x).dtype
        assert tuple(dev.shape) == y.shape
        err = np.max(np.abs(rows.astype(np.float64) - y.astype(np.float64)), axis=1)
        print(f"q={q} {dtype} n={n}: max |difference| {err.max():.3e}, bound {tol.min():.3e}")
        assert np.all(err <= tol), (q, dtype, n, err, tol)
        assert np.array_equal(one, rows[1])
        assert np.array_equal(dev.cpu().numpy(), rows)


def test_integer_records_are_filtered_as_float64(golden):
    g = golden("decimate.npz")
    x = np.round(g[dc.key(5, "float64", 300, "x")] * 1024.0)  # whole numbers (the records lie on a grid of 2^-10)
    ints = x.astype(np.int16)
    assert np.array_equal(ints.astype(np.float64), x)
    want = sampling.decimate_timeseries_collection(x, 5)
    got = sampling.decimate_timeseries_collection(ints, 5)
    assert got.dtype == np.float64 and np.array_equal(got, want)
    one = sampling.decimate_timeseries(ints[2], 5)
    assert one.dtype == np.float64 and np.array_equal(one, want[2])
    dev = sampling.decimate_timeseries_collection(torch.from_numpy(ints).cuda(), 5)
    assert dev.dtype == torch.float64 and np.array_equal(dev.cpu().numpy(), want)
