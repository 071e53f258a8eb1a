"""GPU tests (-m gpu) of pooled panels and whole-record sums of a streamed record: the strip kernel (qi_pool_strip) against
the restatement of tests/pool_cases.py and the existing pooling kernel, its determinism, records stitched from the chunks'
owned ranges (stream.owned_windows, StreamPipeline(pooled=...), PooledRecord) against the float64 oracle on the
small-record and the native engines, TfrPlan.pooled_strip against the plan's own panel, the additivity of the items'
sums, and the unchanged default pipeline.

Bounds.  A maximum is an input value: bit-exact.  An average is held to the reductions contract of test_gpu_pool.py: 1e-4
(float32) / 1e-10 (float64) of the maximum power, against the float64 mean.  The sums are held to test_gpu_requests.
check_direct's 10 rt (1e-4 / 1e-9) of the sum of the absolute terms.  A pooled power of a transform is held to what the
coefficient contract e (2e-5 / 1e-11 of the panel maximum) implies, (2 e + e^2) max p (test_gpu_pool.check_pooled_power);
a band power over m owned samples to m times that."""
import functools

import numpy as np
import pytest
import torch

import pool_cases as pc
from oracle import tfr_oracle as orc
from test_gpu_requests import STX, STYX, _knobs, assert_native, styx_stx_plan

from quantum_inferno_amd import _lib, stream
from quantum_inferno_amd.utilities import sampling

pytestmark = pytest.mark.gpu

FS = 1000.0
ORDER = 3
POWER = _lib.QI_POOL_POWER
SENTINEL = -7.0


def red_tol(dtype):
    return 1e-10 if np.dtype(dtype) == np.dtype(np.float64) else 1e-4


def sum_tol(dtype):
    return 1e-9 if np.dtype(dtype) == np.dtype(np.float64) else 1e-4  # check_direct's 10 rt


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def strip(zd, first, f, windows, scale, mean=True, peak=True, sums=True, pad=0, dtype_code=None, null_in=False, stride=None):
    """One qi_pool_strip call on a complex device tensor [rows, stride] -> (rc, mean, max, sums); outputs that are not
    asked for are None.  The outputs are pre-filled with SENTINEL, out_stride = windows + pad."""
    lib = _lib.load()
    rows, n = zd.shape
    rdt = zd.real.dtype
    ostride = windows + pad
    m = torch.full((rows, ostride), SENTINEL, dtype=rdt, device="cuda") if mean else None
    p = torch.full((rows, ostride), SENTINEL, dtype=rdt, device="cuda") if peak else None
    s = torch.full((rows, 3), SENTINEL, dtype=torch.float64, device="cuda") if sums else None
    code = (_lib.QI_F64 if rdt == torch.float64 else _lib.QI_F32) if dtype_code is None else dtype_code
    rc = lib.qi_pool_strip(code, 0, None if null_in else _lib.ptr(zd), rows, n if stride is None else stride, first, f, windows,
                           float(scale), _lib.ptr(m), _lib.ptr(p), ostride, _lib.ptr(s), _lib.stream_ptr(zd.device))
    return rc, m, p, s


# ---- 1. the kernel against the restatement ---------------------------------------------------------------------------
ROWS, STRIDE = 6, 2100
CASES = [(0, 2, 1050), (3, 7, 299), (5, 64, 32), (1, 100, 20), (13, 1031, 2), (77, 2000, 1)]  # (first, factor, windows)


@pytest.mark.parametrize("dtype", pc.DTYPES)
def test_kernel_against_restatement(dtype):
    z = pc.noise(31 + (dtype == "float64"), (ROWS, STRIDE), dtype, complex_=True)
    zd = dev(z)
    z64 = z.astype(np.complex128)
    for first, f, w in CASES:
        sl = slice(first, first + w * f)
        for scale in (0.0, 2.0):
            p64 = (scale if scale else 1.0) * (z64.real ** 2 + z64.imag ** 2)[:, sl]
            top = np.max(p64)
            plogp = p64 * np.log2(np.where(p64 > 0, p64, 1.0))
            want_sums = np.stack([p64.max(axis=1), p64.sum(axis=1), plogp.sum(axis=1)], axis=1)
            sums_scale = np.stack([p64.max(axis=1), p64.sum(axis=1), np.abs(plogp).sum(axis=1)], axis=1)
            # the power in the input precision, as the kernels form it: the existing kernel on the contiguous range
            want_max = sampling.pool_rows(zd[:, sl].contiguous(), f, "max", POWER, scale)
            for pad in (0, 5):
                where = (dtype, first, f, w, scale, pad)
                rc, m, p, s = strip(zd, first, f, w, scale, pad=pad)
                assert rc == 0, where
                assert torch.equal(p[:, :w], want_max), where
                assert np.max(np.abs(p[:, :w].cpu().numpy() - pc.pool_ref(p64, f, "max"))) <= red_tol(dtype) * top, where
                err = np.max(np.abs(m[:, :w].cpu().numpy().astype(np.float64) - pc.pool_ref(p64, f, "average"))) / top
                print("average", where, err)
                assert err <= red_tol(dtype), (where, err)
                serr = np.max(np.abs(s.cpu().numpy() - want_sums) / sums_scale)
                print("sums", where, serr)
                assert serr <= sum_tol(dtype), (where, serr)
                if pad:
                    assert bool((m[:, w:] == SENTINEL).all()) and bool((p[:, w:] == SENTINEL).all()), where
                # each output alone: the same bits
                _, m1, p1, s1 = strip(zd, first, f, w, scale, peak=False, sums=False, pad=pad)
                assert p1 is None and s1 is None and torch.equal(m1, m), where
                _, m1, p1, s1 = strip(zd, first, f, w, scale, mean=False, sums=False, pad=pad)
                assert torch.equal(p1, p), where
                _, m1, p1, s1 = strip(zd, first, f, w, scale, mean=False, peak=False, pad=pad)
                assert torch.equal(s1, s), where


@pytest.mark.parametrize("dtype", pc.DTYPES)
def test_kernel_argument_errors(dtype):
    zd = dev(pc.noise(3, (ROWS, STRIDE), dtype, complex_=True))
    assert strip(zd, 5, 64, 32, 1.0, dtype_code=7)[0] == -1  # QI_ERR_ARG: a bad dtype
    assert strip(zd, 5, 64, 32, 1.0, null_in=True)[0] == -1
    assert strip(zd, 53, 64, 32, 1.0)[0] == -1  # 53 + 32 * 64 = 2101 > 2100
    assert strip(zd, 0, 2000, 2, 1.0)[0] == -1
    assert strip(zd, 5, 64, 32, 1.0, pad=-1)[0] == -1  # out_stride < windows with an output asked for
    assert strip(zd, 5, 64, 32, 1.0, mean=False, peak=False, pad=-1)[0] == 0  # ... and with none
    assert strip(zd, 5, 1, 32, 1.0)[0] == -1
    rc, m, p, s = strip(zd, 52, 64, 32, 1.0)  # 52 + 2048 = 2100: the range ends with the row
    assert rc == 0 and torch.equal(p, sampling.pool_rows(zd[:, 52:].contiguous(), 64, "max", POWER, 1.0))
    rc, m, p, s = strip(zd, 5, 64, 0, 1.0, pad=4)  # no windows: a successful no-op
    assert rc == 0 and bool((m == SENTINEL).all()) and bool((p == SENTINEL).all()) and bool((s == SENTINEL).all())


# ---- 2. determinism --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", pc.DTYPES)
def test_strip_is_deterministic(dtype):
    zd = dev(pc.noise(5, (ROWS, STRIDE), dtype, complex_=True))
    for first, f, w in ((5, 64, 32), (13, 1031, 2)):
        a = strip(zd, first, f, w, 2.0)
        b = strip(zd, first, f, w, 2.0)
        assert a[0] == b[0] == 0
        for x, y in zip(a[1:], b[1:]):
            assert torch.equal(x, y), (dtype, first, f, w)


# ---- 3 / 4. a record stitched from the owned ranges of its chunks ------------------------------------------------------
SMALL = ("float32", 1024, 512, 5000, 24, 2)  # dtype, chunk, hop, n_total, factor, block: the small-record engine
NATIVE = {"float32": ("float32", 1 << 14, 1 << 13, 3 * (1 << 14) + 777, 100, 1),
          "float64": ("float64", 1 << 15, 1 << 14, 2 * (1 << 15) + 12345, 1000, 1)}
RECORDS = 2
METHODS = ("average", "max")


def coef_eps(dtype):
    return 1e-11 if dtype == "float64" else 2e-5


@functools.lru_cache(maxsize=None)
def host_records(dtype, n_total):
    return pc.noise(n_total, (RECORDS, n_total), dtype)


@functools.lru_cache(maxsize=None)
def stitched_oracle(case):
    """{transform: float64 power [records, B, (n_total // factor) factor]}: the float64 oracle on every chunk as the
    device sees it, each chunk's owned range cut out and the ranges put side by side."""
    dtype, chunk, hop, n_total, factor, _ = case
    x = host_records(dtype, n_total).astype(np.float64)
    starts, edges = stream.owned_windows(n_total, chunk, hop, factor)
    out = {}
    for name, fn in (("cwt", orc.cwt_fft), ("stx", orc.stx_fft)):
        parts = []
        for i, s in enumerate(starts):
            panel = np.stack([fn(ORDER, x[c, s : s + chunk], FS)[2] for c in range(RECORDS)])
            own = panel[:, :, edges[i] - s : edges[i + 1] - s]
            parts.append(own.real ** 2 + own.imag ** 2)
        out[name] = np.concatenate(parts, axis=-1)
    return out


def run_pooled(case, plan):
    dtype, chunk, hop, n_total, factor, block = case
    pipe = stream.StreamPipeline(plan, host_records(dtype, n_total), hop, block=block, pooled=factor, pooled_methods=METHODS)
    return list(pipe.run())


def check_stitched(case, plan, nb):
    dtype, chunk, hop, n_total, factor, block = case
    items = run_pooled(case, plan)
    starts, edges = stream.owned_windows(n_total, chunk, hop, factor)
    assert len(items) == (RECORDS // block) * len(starts)
    cols = n_total // factor
    e = coef_eps(dtype)
    bound = 2 * e + e * e
    tdt = torch.float64 if dtype == "float64" else torch.float32
    for name in ("cwt", "stx"):
        rec = stream.PooledRecord(RECORDS, nb, cols, METHODS, tdt, "cuda")
        for m in METHODS:
            rec.panel[m].fill_(float("nan"))
        for it in items:
            assert it.window0 == edges[it.chunk] // factor and it.windows == (edges[it.chunk + 1] - edges[it.chunk]) // factor
            res = it.cwt if name == "cwt" else it.stx
            assert res.power_time is None and set(res.pooled) == set(METHODS)
            assert tuple(res.pooled["max"].shape) == (it.channels, nb, it.windows) and res.pooled["max"].dtype == tdt
            rec.add(it, name)
        p = stitched_oracle(case)[name]
        assert p.shape == (RECORDS, nb, cols * factor)
        top = np.max(p)
        for m in METHODS:
            got = rec.panel[m].cpu().numpy()
            assert got.shape == (RECORDS, nb, cols) and not np.isnan(got).any(), (name, m)  # every column is written
            err = np.abs(got.astype(np.float64) - pc.pool_ref(p, factor, m)).reshape(RECORDS, -1).max(axis=1) / top
            print("pooled", dtype, name, m, err)
            assert np.all(err <= bound), (dtype, name, m, err)
        res = rec.result()
        berr = np.abs(res.power_band.cpu().numpy() - p.sum(axis=-1)).max(axis=1) / (top * cols * factor)
        print("band", dtype, name, berr)
        assert np.all(berr <= bound), (dtype, name, berr)
        total = res.power_band.sum(dim=1)
        assert float(((res.total_power - total).abs() / total).max()) <= 1e-12, (dtype, name)
        # the whole record's entropy and band bits come from the added sums (TfrResult's own formulas, float64)
        st = res.stats.cpu().numpy()
        want_h = np.log2(st[:, 1]) - st[:, 2] / st[:, 1]
        assert np.all(np.abs(res.entropy_bits.cpu().numpy() - want_h) <= 1e-9), (dtype, name)
        bits = res.power_per_band_bits().cpu().numpy()
        assert bits.shape == (RECORDS, nb) and np.all(bits.max(axis=1) == 0.0), (dtype, name)
    return items


def test_stitched_record_on_small_engine():
    dtype, chunk = SMALL[0], SMALL[1]
    plan, nb = styx_stx_plan(chunk, ORDER, np.dtype(dtype).type, _lib.QI_ENGINE_AUTO, SMALL[5])
    if not _knobs():
        assert plan.stage_bands("small")[STYX] == nb and plan.stage_bands("small")[STX] == nb
    check_stitched(SMALL, plan, nb)
    plan.close()


@pytest.mark.parametrize("dtype", pc.DTYPES)
def test_stitched_record_on_native_engines(dtype):
    case = NATIVE[dtype]
    plan, nb = styx_stx_plan(case[1], ORDER, np.dtype(dtype).type, _lib.QI_ENGINE_AUTO, case[5])
    for which in (STYX, STX):
        assert_native(plan, which, nb)
    items = check_stitched(case, plan, nb)
    assert sorted({it.first_channel for it in items}) == [0, 1]  # two channel blocks: first_channel placement
    plan.close()


# ---- 5. consistency with the plan's other outputs ----------------------------------------------------------------------
@pytest.mark.parametrize("dtype", pc.DTYPES)
def test_strip_consistent_with_panel(dtype):
    _, chunk, hop, n_total, factor, _ = NATIVE[dtype]
    f64 = dtype == "float64"
    rt = 1e-10 if f64 else 1e-5  # check_direct
    starts, edges = stream.owned_windows(n_total, chunk, hop, factor)
    i = len(starts) - 1  # the last chunk: flush with the record end, an offset of no particular alignment
    first, windows = int(edges[i] - starts[i]), int((edges[i + 1] - edges[i]) // factor)
    assert first % 2 == 1 and windows > 0
    plan, nb = styx_stx_plan(chunk, ORDER, np.dtype(dtype).type, _lib.QI_ENGINE_AUTO, RECORDS)
    sig = dev(host_records(dtype, n_total)[:, starts[i] : starts[i] + chunk])
    scale = 2.0
    for which, run in ((STYX, plan.cwt), (STX, plan.stx)):
        strips, band, stats = plan.pooled_strip(which, sig, factor, first, windows, METHODS, power_scale=scale)
        z = run(sig, coef=True).coef[:, :, first : first + windows * factor]
        p = scale * (z.real.double() ** 2 + z.imag.double() ** 2)
        assert band.dtype == torch.float64 and tuple(band.shape) == (RECORDS, nb) and tuple(stats.shape) == (RECORDS, 4)
        assert torch.allclose(band, p.sum(dim=2), rtol=rt, atol=rt * 1e-4 * float(band.max())), which
        plogp = p * torch.log2(torch.where(p > 0, p, torch.ones_like(p)))
        want = torch.stack([p.amax(dim=(1, 2)), p.sum(dim=(1, 2)), plogp.sum(dim=(1, 2))], dim=1)
        den = torch.stack([want[:, 0], want[:, 1], plogp.abs().sum(dim=(1, 2))], dim=1)
        serr = float(((stats[:, :3] - want).abs() / den.clamp_min(1e-300)).max())
        print("stats", dtype, which, serr)
        assert serr <= 10 * rt and bool((stats[:, 3] == 0).all()), (which, serr)
        assert torch.equal(strips["max"], sampling.pool_rows(z.contiguous(), factor, "max", POWER, scale)), which
        one = nb * chunk * (16 if f64 else 8)  # one record per tile: two tiles
        again, band1, stats1 = plan.pooled_strip(which, sig, factor, first, windows, METHODS, power_scale=scale, tile_bytes=one)
        for m in METHODS:
            assert torch.equal(again[m], strips[m]), (which, m)
        # (the order of the sums may depend on the rows of a launch: equal to the tolerance of the sums, not to the bit)
        assert torch.allclose(band1, band, rtol=rt, atol=0.0) and torch.allclose(stats1, stats, rtol=10 * rt, atol=0.0), which
    with pytest.raises(ValueError):
        plan.pooled_strip(STYX, sig, factor, first, windows + 1 + (chunk - first) // factor, METHODS)
    with pytest.raises(ValueError):
        plan.pooled_strip(STYX, sig, factor, first, windows, ("median",))
    plan.close()
    assert plan._stage is None


# ---- 6. additivity -----------------------------------------------------------------------------------------------------
def test_owned_sums_add_up_and_chunk_sums_do_not():
    case = NATIVE["float32"]
    dtype, chunk, hop, n_total, factor, block = case
    plan, nb = styx_stx_plan(chunk, ORDER, np.float32, _lib.QI_ENGINE_AUTO, block)
    items = run_pooled(case, plan)
    parent = list(stream.StreamPipeline(plan, host_records(dtype, n_total), hop, block=block).run())
    assert len(parent) == len(items)
    for name in ("cwt", "stx"):
        rec = stream.PooledRecord(RECORDS, nb, n_total // factor, METHODS, torch.float32, "cuda")
        added = torch.zeros(RECORDS, dtype=torch.float64, device="cuda")
        chunk_sums = torch.zeros(RECORDS, dtype=torch.float64, device="cuda")
        for it, old in zip(items, parent):
            rec.add(it, name)
            ch = slice(it.first_channel, it.first_channel + it.channels)
            added[ch] += (it.cwt if name == "cwt" else it.stx).stats[:, 1]
            chunk_sums[ch] += (old.cwt if name == "cwt" else old.stx).stats[:, 1]
        total = rec.result().total_power
        assert float(((added - total).abs() / total).max()) <= 1e-12, name
        ratio = (chunk_sums / total).cpu().numpy()
        print("chunk sums / record total", name, ratio)
        assert np.all(np.abs(ratio - 1.0) > 0.3), (name, ratio)  # the per-chunk sums count the overlaps twice
    plan.close()


# ---- 7. the default pipeline is unchanged ------------------------------------------------------------------------------
def test_default_pipeline_unchanged():
    dtype, chunk, hop, n_total, _, block = SMALL
    host = host_records(dtype, n_total)
    plan, _ = styx_stx_plan(chunk, ORDER, np.float32, _lib.QI_ENGINE_AUTO, block)
    items = list(stream.StreamPipeline(plan, host, hop, block=block).run())
    starts = stream.chunk_starts(n_total, chunk, hop)
    assert len(items) == len(starts)
    for it in items:
        assert it.window0 is None and it.windows is None and it.start == starts[it.chunk]
        x = dev(host[it.first_channel : it.first_channel + it.channels, it.start : it.start + chunk])
        for got, want in zip((it.cwt, it.stx), plan.cwt_stx(x, coef=False, reductions=True)):
            assert got.pooled is None
            assert torch.equal(got.power_band, want.power_band) and torch.equal(got.stats, want.stats)
            assert torch.equal(got.power_time, want.power_time)
    plan.close()
