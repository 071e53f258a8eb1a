"""GPU tests (-m gpu) of time pooling: the kernel (qi_pool_panel) against the fixture of the reference's results and the
NumPy restatement of tests/pool_cases.py, complex and power inputs, the median's window limit, run-to-run determinism,
TfrPlan.pooled against the float64 oracle and against the plan's other outputs, and the utilities.sampling wrappers.

Bounds.  nth / max / min / median return input values: bit-exact.  An average is held to the reductions contract (DESIGN
section 2): 1e-4 (float32) / 1e-10 (float64) of the panel maximum, against the float64 mean of the same inputs.  A pooled
power of a transform is held to what the coefficient contract eps (2e-5 / 1e-11 of the panel maximum) implies:
||z + d|^2 - |z|^2| <= (2 eps + eps^2) max|z|^2, and average / max / min / median are 1-Lipschitz in the sup norm.
"""
import functools

import numpy as np
import pytest
import torch

import pool_cases as pc
from oracle import tfr_oracle as orc
from test_gpu_requests import STX, STYX, assert_native, styx_stx_plan

from quantum_inferno_amd import _lib, engine
from quantum_inferno_amd.utilities import sampling

pytestmark = pytest.mark.gpu

FS = 1000.0
REAL, COMPLEX, POWER = _lib.QI_POOL_REAL, _lib.QI_POOL_COMPLEX, _lib.QI_POOL_POWER


def red_tol(dtype):
    return 1e-10 if np.dtype(dtype) in (np.dtype(np.float64), np.dtype(np.complex128)) else 1e-4


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def two_panels(x):
    """[2, 3, n]: the fixture's rows and a second, different panel behind them (rows = 2 * 3)."""
    return np.ascontiguousarray(np.stack([x, -x[::-1] + 0.125]))


def check_real_case(x, f, m):
    """One (input, factor, method) on the device against the restatement; returns the device's result."""
    got = sampling.pool_rows(dev(x), f, m).cpu().numpy()
    want = pc.pool_ref(x, f, m)
    where = (x.dtype, x.shape, f, m)
    assert got.dtype == x.dtype and got.shape == want.shape == x.shape[:-1] + (pc.columns(x.shape[-1], f, m),), where
    if m != "average":
        assert np.array_equal(got, want), where
    elif got.size:
        err = np.max(np.abs(got - pc.pool_ref(x.astype(np.float64), f, m))) / np.max(np.abs(x))
        assert err <= red_tol(x.dtype), (where, err)
    return got


# ---- 1. the kernel against the fixture and the restatement ----------------------------------------------------------
@pytest.mark.parametrize("n", pc.LENGTHS)
@pytest.mark.parametrize("dtype", pc.DTYPES)
def test_kernel_against_fixture(golden, dtype, n):
    g = golden("subsample.npz")
    x = g[f"in_{dtype}_n{n}"]
    for f in pc.FACTORS:
        for m in pc.METHODS:
            ref = g[pc.key(dtype, n, f, m)]
            got = check_real_case(x, f, m)
            if m == "average":
                if ref.size:
                    exact = pc.pool_ref(x.astype(np.float64), f, m)
                    assert np.max(np.abs(ref - exact)) <= red_tol(dtype) * np.max(np.abs(x)), (dtype, n, f)
            else:
                assert np.array_equal(got, ref), (dtype, n, f, m)
            x6 = two_panels(x)
            got6 = check_real_case(x6, f, m)
            assert np.array_equal(got6[0], got), (dtype, n, f, m)  # the same rows give the same bits wherever they lie
    # a record: one row
    for f in (7, 100):
        assert np.array_equal(sampling.pool_rows(dev(x[0]), f, "max").cpu().numpy(), g[pc.key(dtype, n, f, "max", one_d=True)])


# ---- 2. complex and power inputs -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", pc.LENGTHS)
@pytest.mark.parametrize("dtype", pc.DTYPES)
def test_complex_and_power_inputs(dtype, n):
    z3 = pc.noise(7 * n + (dtype == "float64"), (pc.ROWS, n), dtype, complex_=True)
    for z in (z3, two_panels(z3)):
        zd = dev(z)
        z64 = z.astype(np.complex128)
        top = np.max(np.abs(z64))
        for f in pc.FACTORS:
            got = sampling.pool_rows(zd, f, "nth", COMPLEX).cpu().numpy()
            assert got.dtype == z.dtype and np.array_equal(got, z[..., ::f]), (dtype, n, f)
            got = sampling.pool_rows(zd, f, "average", COMPLEX).cpu().numpy()
            want = pc.pool_ref(z64, f, "average")
            assert got.dtype == z.dtype and got.shape == want.shape, (dtype, n, f)
            if got.size:
                assert np.max(np.abs(got - want)) <= red_tol(dtype) * top, (dtype, n, f, np.max(np.abs(got - want)) / top)
            for scale in (0.0, 2.0):
                p64 = (scale if scale else 1.0) * (z64.real ** 2 + z64.imag ** 2)
                for m in pc.METHODS:
                    got = sampling.pool_rows(zd, f, m, POWER, scale).cpu().numpy()
                    want = pc.pool_ref(p64, f, m)
                    assert got.dtype == np.dtype(dtype) and got.shape == want.shape, (dtype, n, f, m)
                    if got.size:
                        err = np.max(np.abs(got - want)) / np.max(p64)
                        assert err <= red_tol(dtype), (dtype, n, f, m, scale, err)
    lib = _lib.load()
    out = torch.empty((pc.ROWS, n // 4), dtype=zd.dtype, device="cuda")
    z3d = dev(z3)
    for code in (_lib.QI_POOL_MAX, _lib.QI_POOL_MIN, _lib.QI_POOL_MEDIAN):
        rc = lib.qi_pool_panel(_lib.QI_F64 if dtype == "float64" else _lib.QI_F32, 0, _lib.ptr(z3d), COMPLEX, pc.ROWS, n, 4, code,
                               1.0, _lib.ptr(out), None)
        assert rc == -1, code  # QI_ERR_ARG
    with pytest.raises(_lib.QiError):
        sampling.pool_rows(z3d, 4, "max", COMPLEX)


# ---- 3. the median's window limit ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", pc.DTYPES)
def test_median_limit(dtype):
    x = pc.noise(99, (pc.ROWS, 8200), dtype)
    got = sampling.pool_rows(dev(x), 4096, "median").cpu().numpy()
    assert got.shape == (pc.ROWS, 2) and np.array_equal(got, pc.pool_ref(x, 4096, "median"))
    assert _lib.POOL_MEDIAN_MAX == 4096
    with pytest.raises(_lib.QiError, match="4096"):
        sampling.pool_rows(dev(x), 4097, "median")
    # the other methods have no such limit
    assert np.array_equal(sampling.pool_rows(dev(x), 4097, "max").cpu().numpy(), pc.pool_ref(x, 4097, "max"))


# ---- 4. determinism --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", pc.DTYPES)
def test_average_is_deterministic(golden, dtype):
    g = golden("subsample.npz")
    for n in pc.LENGTHS:
        xd = dev(two_panels(g[f"in_{dtype}_n{n}"]))
        zd = dev(pc.noise(5, (pc.ROWS, n), dtype, complex_=True))
        for f in pc.FACTORS:
            for t, kind in ((xd, REAL), (zd, COMPLEX), (zd, POWER)):
                a = sampling.pool_rows(t, f, "average", kind)
                b = sampling.pool_rows(t, f, "average", kind)
                assert torch.equal(torch.view_as_real(a) if a.is_complex() else a, torch.view_as_real(b) if b.is_complex() else b), (dtype, n, f, kind)


# ---- 5. plan.pooled against the CPU oracle ---------------------------------------------------------------------------
CHANNELS, ORDER = 3, 3


def records(n, dtype):
    return pc.noise(n, (CHANNELS, n), dtype)  # three-channel seeded noise, mean 0.5


@functools.lru_cache(maxsize=None)
def oracle_panels(n, dtype):
    """{which: complex128 [C, B, n]} of the float64 oracle on the records as the device sees them."""
    x = records(n, dtype).astype(np.float64)
    return {STYX: np.stack([orc.cwt_fft(ORDER, x[c], FS)[2] for c in range(CHANNELS)]),
            STX: np.stack([orc.stx_fft(ORDER, x[c], FS)[2] for c in range(CHANNELS)])}


def coef_eps(dtype):
    return 1e-11 if dtype == "float64" else 2e-5


def check_pooled_power(plan, which, n, dtype, f, m, tile_bytes, scale=2.0):
    ref = oracle_panels(n, dtype)[which]
    p = scale * (ref.real ** 2 + ref.imag ** 2)
    want = pc.pool_ref(p, f, m)
    sig = dev(records(n, dtype))
    got = plan.pooled(which, sig, f, m, power_scale=scale, tile_bytes=tile_bytes)
    assert got.dtype == sig.dtype and tuple(got.shape) == want.shape, (which, n, dtype, f, m)
    e = coef_eps(dtype)
    err = np.abs(got.cpu().numpy().astype(np.float64) - want).reshape(CHANNELS, -1).max(axis=1) / np.max(p)
    assert np.all(err <= 2 * e + e * e), (which, n, dtype, f, m, err)  # (per channel: a slice-offset error shows in 1 and 2)


def check_pooled_bits(plan, which, n, dtype, f, tile_bytes):
    ref = oracle_panels(n, dtype)[which]
    mag = np.abs(ref)
    floor, tol = (1.5e-2, 1e-9) if dtype == "float64" else (1e-3, 1e-3)
    cols = n // f
    keep = (mag[..., : cols * f].reshape(mag.shape[:-1] + (cols, f)) >= floor * mag.max()).all(axis=-1)
    share = 1.0 - keep.mean()
    assert share <= 0.5, f"{share:.3f} of the windows hold a coefficient under the floor"
    want = pc.pool_ref(np.log2(mag + orc.EPS64), f, "max")
    got = plan.pooled(which, dev(records(n, dtype)), f, "max", quantity="bits", tile_bytes=tile_bytes).cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.dtype(dtype)
    d = np.abs(got.astype(np.float64) - want)[keep]
    assert d.max() <= tol, (which, n, dtype, f, float(d.max()), f"masked share {share:.3f}")


@pytest.mark.parametrize("dtype", pc.DTYPES)
def test_pooled_on_hipfft_engine(dtype):
    n = 1000
    plan, nb = styx_stx_plan(n, ORDER, np.dtype(dtype).type, _lib.QI_ENGINE_HIPFFT, CHANNELS)
    one = nb * n * (16 if dtype == "float64" else 8)
    for which in (STYX, STX):
        for m in ("average", "max", "min", "median", "nth"):
            check_pooled_power(plan, which, n, dtype, 7, m, one)
        check_pooled_power(plan, which, n, dtype, 7, "average", 1 << 30)
        check_pooled_bits(plan, which, n, dtype, 7, one // 2)
    plan.close()
    assert plan._stage is None


@pytest.mark.parametrize("dtype,log2n", [("float32", 14), ("float64", 15)])
def test_pooled_on_native_engines(dtype, log2n):
    n = 1 << log2n
    plan, nb = styx_stx_plan(n, ORDER, np.dtype(dtype).type, _lib.QI_ENGINE_AUTO, CHANNELS)
    one = nb * n * (16 if dtype == "float64" else 8)  # one record per tile: three tiles
    for which in (STYX, STX):
        assert_native(plan, which, nb)
        for f in (64, 100):
            for m in ("average", "max"):
                check_pooled_power(plan, which, n, dtype, f, m, one)
            check_pooled_bits(plan, which, n, dtype, f, one // 2)
    plan.close()


# ---- 6. consistency with the plan's other outputs ---------------------------------------------------------------------
@pytest.mark.parametrize("dtype,log2n", [("float32", 14), ("float64", 15)])
def test_pooled_consistent_with_panel_and_reductions(dtype, log2n):
    n = 1 << log2n
    plan, nb = styx_stx_plan(n, ORDER, np.dtype(dtype).type, _lib.QI_ENGINE_AUTO, CHANNELS)
    sig = dev(records(n, dtype))
    scale = 2.0
    for which, run in ((STYX, plan.cwt), (STX, plan.stx)):
        full = run(sig, coef=True, reductions=True, power_scale=scale)
        for f, m in ((64, "average"), (100, "max"), (100, "median"), (1000, "min"), (64, "nth"), (n, "average")):
            a = plan.pooled(which, sig, f, m, power_scale=scale, tile_bytes=1 << 30)
            b = sampling.pool_rows(run(sig, coef=True).coef, f, m, POWER, scale)
            assert torch.equal(a, b), (which, f, m)
        avg = plan.pooled(which, sig, 64, "average", power_scale=scale)
        band = avg.double().sum(dim=-1) * 64
        err = float((band - full.power_band).abs().max() / full.power_band.max())
        assert err <= red_tol(dtype), (which, err)
    plan.close()


# ---- 7. the wrappers -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", pc.DTYPES)
def test_wrappers(dtype):
    x = pc.noise(3, (2, pc.ROWS, 1031), dtype)
    for f, m in ((7, "median"), (64, "average"), (100, "max"), (3, "nth"), (65, "min")):
        tol = red_tol(dtype) * np.max(np.abs(x)) if m == "average" else 0.0
        for arr in (x[0], x, x[0, 0], x[:, 0]):
            want = pc.pool_ref(arr, f, m)
            if arr.ndim >= 2:
                got = sampling.subsample_2d(arr, f, m)
                assert isinstance(got, np.ndarray) and got.dtype == arr.dtype and np.max(np.abs(got - want)) <= tol, (f, m, arr.shape)
                got = sampling.subsample_2d(dev(arr), f, m)
                assert isinstance(got, torch.Tensor) and got.is_cuda and got.cpu().numpy().dtype == arr.dtype
                assert np.max(np.abs(got.cpu().numpy() - want)) <= tol, (f, m, arr.shape)
            if arr.ndim <= 2:
                got, rate = sampling.subsample(arr, 800.0, f, m)
                assert rate == 800.0 / f
                assert isinstance(got, np.ndarray) and got.dtype == arr.dtype and np.max(np.abs(got - want)) <= tol, (f, m, arr.shape)
                got, rate = sampling.subsample(dev(arr), 800.0, f, m)
                assert rate == 800.0 / f and isinstance(got, torch.Tensor) and got.is_cuda
                assert np.max(np.abs(got.cpu().numpy() - want)) <= tol, (f, m, arr.shape)
    z = pc.noise(4, (pc.ROWS, 1031), dtype, complex_=True)
    assert np.array_equal(sampling.subsample_2d(z, 7, "nth"), z[:, ::7])
    got = sampling.subsample_2d(z, 7, "average")
    assert got.dtype == z.dtype and np.max(np.abs(got - pc.pool_ref(z.astype(np.complex128), 7, "average"))) <= red_tol(dtype) * np.max(np.abs(z))
    with pytest.warns(UserWarning):
        assert np.array_equal(sampling.subsample_2d(x[0], 7, "mode"), x[0][:, ::7])  # an unknown method is read as "nth"
    with pytest.raises(ValueError):
        sampling.subsample_2d(z, 7, "median")
    assert sampling.subsample_2d(x[0], 2000, "max").shape == (pc.ROWS, 0)
    assert sampling.subsample_2d(x[0], 2000, "nth").shape == (pc.ROWS, 1)
