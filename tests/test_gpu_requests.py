"""GPU tests (-m gpu) of requests the benchmark does not make, on the native engines: the atoms bank (chirped atoms,
both dictionaries), the conv back end, the spect / unit styx dictionaries, `power_scale` and `eps` on every engine path,
degenerate records (zeros, impulses at the record ends and next to a block boundary) and the plan-less reduction kernels
at multi-block shapes.  Every native case also asserts that the native engines ran the whole table (no row left to the
hipFFT engine), so that a plan change cannot quietly move the case there.

Tolerances as test_gpu_parity.TOL: float32 2e-5 of each row's own maximum; float64 1e-11 of the panel maximum and
5e-9 of each row's own maximum.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import relmax
from oracle import tfr_oracle as orc

from quantum_inferno_amd import _lib, cwt_atoms, engine, scales_dyadic, stream, tfr_info

pytestmark = pytest.mark.gpu

FS = 1000.0
ROW32, PANEL64, ROW64 = 2e-5, 1e-11, 5e-9
# switches that move bands between the engines on purpose: the engine-census assertions do not apply under them
KNOBS = ("QI_FORCE_HIPFFT", "QI_NATIVE_SPLIT", "QI_NATIVE_SPLIT64", "QI_NATIVE_Z64", "QI_NATIVE_BLOCK64", "QI_NATIVE_ZOOM",
         "QI_NATIVE_BLOCK")
STYX, ATOMS, STX = _lib.QI_BANK_STYX, _lib.QI_BANK_ATOMS, _lib.QI_TABLE_STX


def _knobs():
    return any(k in os.environ for k in KNOBS)


def assert_native(plan, which, nb):
    """The zoom, block and two-pass engines produce every row of table `which`; the hipFFT engine none."""
    if _knobs():
        return
    assert plan.stage_bands("inverse")[which] == 0, (which, plan.stage_bands("inverse"))
    assert sum(plan.stage_bands(s)[which] for s in ("zoom", "block", "pass2")) == nb, which


def spread(nb):
    return sorted({0, 1, nb // 5, (2 * nb) // 5, nb // 2, (3 * nb) // 4, nb - 2, nb - 1})


def record(n, dtype, seed, channels=1, noise=0.25):
    """Chirp + noise records up to the record ends (distinct per channel)."""
    rng = np.random.default_rng(seed)
    x = np.stack([orc.synth_chirp(n, FS, c, channels, np.float64) for c in range(channels)])
    return (x + noise * rng.standard_normal((channels, n))).astype(dtype)


def check_rows(got, want, f64, what="", panel64=PANEL64):
    """Every row of `got` [..., n] against `want`: to the row's own maximum (float32 2e-5, float64 5e-9), in float64 also
    to 1e-11 of the panel maximum.  A row whose reference is 0 must be 0."""
    dev = got.device if isinstance(got, torch.Tensor) else torch.device("cuda")
    got = torch.as_tensor(got).to(dev, torch.complex128)
    want = torch.as_tensor(want).to(dev, torch.complex128)
    err = (got - want).abs().amax(dim=-1)
    top = want.abs().amax(dim=-1)
    rel = err / top.clamp_min(1e-300)
    worst = float(rel.max())
    assert worst <= (ROW64 if f64 else ROW32), (what, np.unravel_index(int(rel.argmax()), tuple(rel.shape)), worst)
    if f64:
        assert float(err.max()) <= panel64 * float(top.max()), (what, float(err.max()) / float(top.max()))


def check_bits(bits, ref_coef, f64, what=""):
    """log2(|z| + eps) against the reference panel where the coefficient tolerance implies the bits tolerance:
    float64 1e-9 bits from 1.5e-2 of the maximum, float32 1e-3 bits from 1e-3 of the maximum."""
    mag = ref_coef.abs().double()
    floor, tol = (1.5e-2, 1e-9) if f64 else (1e-3, 1e-3)
    sel = mag >= floor * float(mag.max())
    d = (bits.double() - torch.log2(mag + orc.EPS64))[sel].abs()
    assert float(d.max()) <= tol, (what, float(d.max()))


def check_reductions(a, b, f64, what=""):
    """Fused reductions of `a` against those of `b` (the hipFFT engine)."""
    rt = 1e-9 if f64 else 1e-4
    assert torch.allclose(a.power_band, b.power_band, rtol=rt, atol=(1e-12 if f64 else 1e-9) * float(b.power_band.max())), what
    if a.power_time is not None and b.power_time is not None:
        assert torch.allclose(a.power_time.double(), b.power_time.double(), rtol=1e-8 if f64 else 1e-3,
                              atol=(1e-11 if f64 else 1e-6) * float(b.power_time.max())), what
    assert torch.allclose(a.stats[:, :3], b.stats[:, :3], rtol=rt), what


def check_direct(res, f64, what=""):
    """Fused reductions against direct sums of the stored panel (P = power_scale |z|^2)."""
    rt = 1e-10 if f64 else 1e-5
    p = res.power_scale * (res.coef.real.double() ** 2 + res.coef.imag.double() ** 2)
    assert torch.allclose(res.power_band, p.sum(dim=2), rtol=rt, atol=rt * 1e-4 * float(res.power_band.max())), what
    if res.power_time is not None:
        pt = p.sum(dim=1)
        assert torch.allclose(res.power_time.double(), pt, rtol=10 * rt, atol=10 * rt * 1e-3 * float(pt.max())), what
    plogp = p * torch.log2(torch.where(p > 0, p, torch.ones_like(p)))
    want = torch.stack([p.amax(dim=(1, 2)), p.sum(dim=(1, 2)), plogp.sum(dim=(1, 2))], dim=1)
    scale = torch.stack([want[:, 0], want[:, 1], plogp.abs().sum(dim=(1, 2))], dim=1)
    assert float(((res.stats[:, :3] - want).abs() / scale.clamp_min(1e-300)).max()) <= 10 * rt, what


def atom_tables(n, order, shift=0.0, dict_type="norm"):
    """(f_hz, (p_re, p_im, omega, amp)) of cwt_chirp_from_sig's band table (cwt_atoms.py:447-486)."""
    _, f_min = cwt_atoms.chirp_scales_from_duration(order, n / FS, shift)
    o, _, _, _, f_desc, _, _ = cwt_atoms.chirp_frequency_bands(order, f_min, FS, FS / 2.0, shift)
    f = np.flip(f_desc)
    return f, cwt_atoms._atom_tables(o, f, FS, shift, scales_dyadic.Slice.G2, dict_type)


def bank_plan(n, dtype, which, tables, eng=_lib.QI_ENGINE_AUTO, channels=1):
    f, tabs = tables
    plan = engine.TfrPlan(n, dtype, None, engine.TfrPlan.workspace_for(n, len(f), dtype, channels), eng)
    plan.set_gabor_bank(which, f, *tabs)
    return plan


def styx_stx_plan(n, order, dtype, eng=_lib.QI_ENGINE_AUTO, channels=1):
    nb = len(scales_dyadic.log_frequency_hz_from_fft_points(FS, n, order))
    plan = engine.TfrPlan(n, dtype, None, engine.TfrPlan.workspace_for(n, nb, dtype, channels), eng)
    plan.set_styx_bank(order, FS)
    plan.set_stx_bands(order, FS)
    return plan, nb


# the oracle's atoms sit on the reference's time axis x = fs (t - t[-1] / 2), whose rounding (~5e-11 samples at 2^20) moves
# the phase of the highest bands by ~1e-10: measured 9.9e-11 of the panel maximum at float64 2^20 order 12 (the hipFFT
# engine and the native engines agree to 1e-11); each row stays far inside 5e-9 of its own maximum
PANEL64_ATOM_AXIS = 2e-10


# ---- the atoms bank on the native engines -------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,log2n,order,shift,dict_type", [
    (np.float32, 20, 3, 1.0, "norm"), (np.float32, 20, 12, -1.0, "spect"), (np.float32, 21, 6, 0.0, "norm"),
    (np.float64, 20, 12, 0.0, "spect"), (np.float64, 20, 6, 1.0, "norm"), (np.float64, 21, 3, -1.0, "norm")])
def test_atoms_bank_on_native_engines(dtype, log2n, order, shift, dict_type):
    """QI_BANK_ATOMS (circular correlation, half-record roll) with chirped atoms (complex p) and both dictionaries on the
    native engines (which take that bank at 2^20 and 2^21 samples; other lengths run it on the hipFFT engine): every row,
    the bits and every fused reduction against the hipFFT engine; spread bands against the oracle; the reductions against
    direct sums of the stored panel; the public wrapper against the plan call."""
    n, f64 = 1 << log2n, dtype == np.float64
    tables = atom_tables(n, order, shift, dict_type)
    nb = len(tables[0])
    x = record(n, dtype, log2n + order)
    xt = torch.from_numpy(x).cuda()
    nat = bank_plan(n, dtype, ATOMS, tables)
    ref = bank_plan(n, dtype, ATOMS, tables, _lib.QI_ENGINE_HIPFFT)
    assert_native(nat, ATOMS, nb)
    a = nat.cwt_atoms(xt, coef=True, bits=True, reductions=True)
    b = ref.cwt_atoms(xt, coef=True, bits=True, reductions=True)
    check_rows(a.coef, b.coef, f64, "hipfft")
    check_bits(a.bits, b.coef, f64)
    check_reductions(a, b, f64)
    check_direct(a, f64)
    pick = spread(nb)
    want, _, _, f_or = orc.cwt_chirp_fft(x[0].astype(np.float64), FS, order, index_shift=shift, dict_type=dict_type, bands=pick)
    assert np.array_equal(f_or, tables[0])
    check_rows(a.coef[0, pick], want, f64, "oracle", PANEL64_ATOM_AXIS)
    ref.close()
    del b
    if (order, log2n) in ((12, 20), (6, 20)):  # the public wrapper: the same table on the same engines
        c, bits, _, fc = cwt_atoms.cwt_chirp_from_sig(xt[0], FS, order, index_shift=shift, dictionary_type=dict_type)
        assert np.array_equal(fc, tables[0])
        assert torch.equal(c, a.coef[0]) and torch.equal(bits, a.bits[0])
        engine.clear_plans()
    nat.close()


# ---- the conv back end at native lengths --------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,log2n", [(np.float32, 16), (np.float32, 20), (np.float64, 19), (np.float64, 20)])
def test_conv_back_end_at_native_lengths(dtype, log2n):
    """cwt_chirp_from_sig(cwt_type="conv") (the chirp atoms in the styx bank: linear correlation) with index_shift 0 and
    +-1 against the oracle's restatement of signal.convolve and against the hipFFT engine.  Chirped atoms are not pure
    Gaussians: float32 runs the short ones as non-analytic picks of the block engine (the band's bank row), float64
    leaves them to the short-atom table at 2^20 (k_edge_fix with its p_im phase) and to the two-pass kernels at 2^19.
    (In float64 the native engines take this table only where the two-pass kernels can run, 2^19 and 2^20 samples.)"""
    n, f64, order = 1 << log2n, dtype == np.float64, 3
    x = record(n, dtype, 40 + log2n)
    xt = torch.from_numpy(x).cuda()
    for shift in (0.0, 1.0, -1.0):
        tables = atom_tables(n, order, shift)
        nb = len(tables[0])
        c, bits, _, fc = cwt_atoms.cwt_chirp_from_sig(xt[0], FS, order, cwt_type="conv", index_shift=shift)
        assert np.array_equal(fc, tables[0])
        engine.clear_plans()
        nat = bank_plan(n, dtype, STYX, tables)  # the wrapper's plan, for its engine census
        assert_native(nat, STYX, nb)
        if shift != 0.0 and not _knobs():
            if f64:  # no chirped band on the float64 block engine (Gaussians only): short-atom table / two-pass kernels
                assert nat.stage_bands("block")[STYX] == 0 and nat.stage_bands("pass2")[STYX] > 0
            else:
                assert nat.stage_bands("block")[STYX] > 0
        mine = nat.cwt(xt, coef=True, bits=True)
        assert torch.equal(mine.coef[0], c) and torch.equal(mine.bits[0], bits)
        nat.close()
        del mine
        ref = bank_plan(n, dtype, STYX, tables, _lib.QI_ENGINE_HIPFFT)
        b = ref.cwt(xt, coef=True)
        check_rows(c, b.coef[0], f64, ("hipfft", shift))
        check_bits(bits, b.coef[0], f64, ("bits", shift))
        ref.close()
        del b
        pick = spread(nb)
        want = orc.cwt_chirp_conv(x[0].astype(np.float64), FS, order, index_shift=shift, bands=pick)[0]
        check_rows(c[pick], want, f64, ("oracle", shift), PANEL64_ATOM_AXIS)
        del c, bits


# ---- the spect / unit styx dictionaries at native lengths ---------------------------------------------------------------
@pytest.mark.parametrize("dtype,log2n,order", [(np.float32, 20, 3), (np.float64, 16, 12)])
def test_styx_dictionaries_at_native_lengths(dtype, log2n, order):
    """set_styx_bank(dictionary_type="spect" / "unit") on the native engines: spread bands against the oracle, every row
    against the "norm" row times the amplitude ratio (styx_cwt.py:139-144), reductions against the stored panel."""
    n, f64 = 1 << log2n, dtype == np.float64
    x = record(n, dtype, 60 + order)
    xt = torch.from_numpy(x).cuda()
    nb = len(scales_dyadic.log_frequency_hz_from_fft_points(FS, n, order))
    ws = engine.TfrPlan.workspace_for(n, nb, dtype, 1)
    pick = spread(nb)
    base = None
    for dict_type in ("norm", "spect", "unit"):
        plan = engine.TfrPlan(n, dtype, None, ws)
        plan.set_styx_bank(order, FS, dict_type)
        assert_native(plan, STYX, nb)
        res = plan.cwt(xt, coef=True, reductions=True)
        _, _, want = orc.cwt_fft(order, x[0].astype(np.float64), FS, dict_type=dict_type, bands=pick)
        check_rows(res.coef[0, pick], want, f64, dict_type)
        amp = engine.styx_bank_tables(order, n, FS, dict_type)[4]
        if base is None:
            base = res.coef, amp
        else:
            ratio = torch.from_numpy(amp / base[1]).cuda()
            check_rows(res.coef, base[0] * ratio[None, :, None], f64, ("ratio", dict_type))
            check_direct(res, f64, dict_type)
        plan.close()


# ---- power_scale and eps on every engine path ---------------------------------------------------------------------------
def check_scale_and_eps(call, f64):
    """`call(power_scale, eps)` -> list of TfrResult.  P = s |z|^2: for s = 2 (a power of two) every product and every
    fixed-order sum doubles exactly -- band / time powers, maximum and total bit-equal to twice the default, sum P log2 P =
    2 (sum P log2 P + sum P), entropy unchanged, panels bit-equal; for s = 0.3 the same relations to rounding.  With an
    explicit eps the bits are log2(|z| + eps) of the returned panel and the reductions bit-equal; eps = 2^-52 is the
    default spelled out."""
    rt = 1e-12 if f64 else 1e-6
    one = call(1.0, 0.0)

    def same_panels(a, b):
        for u, v in ((a.coef, b.coef), (a.bits, b.bits)):
            assert (u is None) == (v is None)
            if u is not None:
                assert torch.equal(u, v)

    def same_reductions(a, b):
        assert torch.equal(a.power_band, b.power_band) and torch.equal(a.stats, b.stats)
        assert (a.power_time is None) == (b.power_time is None)
        if a.power_time is not None:
            assert torch.equal(a.power_time, b.power_time)

    for s in (2.0, 0.3):
        got = call(s, 0.0)
        for k, (a, b) in enumerate(zip(one, got)):
            same_panels(a, b)
            assert b.power_scale == s
            a1, a2 = a.stats[:, 1], a.stats[:, 2]
            ls = float(np.log2(s))
            size = (s * (a2.abs() + abs(ls) * a1)).max()
            assert torch.allclose(b.stats[:, 2], s * (a2 + ls * a1), rtol=0.0, atol=rt * float(size)), (s, k)
            assert float((b.entropy_bits - a.entropy_bits).abs().max()) <= (1e-9 if f64 else 1e-5), (s, k)
            if s == 2.0:
                assert torch.equal(b.power_band, 2 * a.power_band), k
                assert torch.equal(b.stats[:, :2], 2 * a.stats[:, :2]), k
                if a.power_time is not None:
                    assert torch.equal(b.power_time, 2 * a.power_time), k
            else:
                assert torch.allclose(b.power_band, s * a.power_band, rtol=rt, atol=0.0), k
                assert torch.allclose(b.stats[:, :2], s * a.stats[:, :2], rtol=rt, atol=0.0), k
                if a.power_time is not None:
                    assert torch.allclose(b.power_time.double(), s * a.power_time.double(), rtol=rt,
                                          atol=rt * 1e-3 * s * float(a.power_time.max())), k
        del got
    top = max((float(a.coef.abs().max()) for a in one if a.coef is not None), default=1.0)
    eps = 1e-3 * top
    got = call(1.0, eps)
    for a, b in zip(one, got):
        same_reductions(a, b)
        if a.coef is not None:
            assert torch.equal(a.coef, b.coef)
        if b.bits is not None:
            want = torch.log2(b.coef.abs().double() + eps)
            assert float((b.bits.double() - want).abs().max()) <= (1e-12 if f64 else 1e-5)
    del got
    got = call(1.0, 2.0 ** -52)
    for a, b in zip(one, got):
        same_panels(a, b)
        same_reductions(a, b)


def test_power_scale_and_eps_float32_native():
    """float32 2^20 order 3 (zoom, block, split bands) through cwt, stx, the joint cwt_stx, reductions only,
    reductions="band"; the atoms bank."""
    n, order = 1 << 20, 3
    xt = torch.from_numpy(record(n, np.float32, 5, channels=2)).cuda()
    plan, nb = styx_stx_plan(n, order, np.float32, channels=2)
    assert_native(plan, STYX, nb)
    assert_native(plan, STX, nb)
    for name in ("cwt", "stx"):
        fn = getattr(plan, name)
        check_scale_and_eps(lambda s, e: [fn(xt, coef=True, bits=True, reductions=True, power_scale=s, eps=e)], False)
        check_scale_and_eps(lambda s, e: [fn(xt, coef=False, reductions=True, power_scale=s, eps=e)], False)
    check_scale_and_eps(lambda s, e: list(plan.cwt_stx(xt, coef=True, bits=True, reductions=True, power_scale=s, eps=e)), False)
    check_scale_and_eps(lambda s, e: list(plan.cwt_stx(xt, coef=True, reductions="band", power_scale=s, eps=e)), False)
    check_scale_and_eps(lambda s, e: list(plan.cwt_stx(xt, coef=False, reductions="band", power_scale=s, eps=e)), False)
    plan.close()
    tables = atom_tables(n, order)
    atoms = bank_plan(n, np.float32, ATOMS, tables, channels=2)
    assert_native(atoms, ATOMS, len(tables[0]))
    check_scale_and_eps(lambda s, e: [atoms.cwt_atoms(xt, coef=True, bits=True, reductions=True, power_scale=s, eps=e)], False)
    atoms.close()


def test_power_scale_and_eps_stockwell_rows_behind_the_native_run():
    """float32 2^16 order 1: the top Stockwell rows on a pass of the hipFFT engine behind the native run."""
    n, order = 1 << 16, 1
    xt = torch.from_numpy(record(n, np.float32, 11, channels=2)).cuda()
    plan, nb = styx_stx_plan(n, order, np.float32, channels=2)
    assert 0 < plan.stage_bands("inverse")[STX] < nb
    check_scale_and_eps(lambda s, e: [plan.stx(xt, coef=True, bits=True, reductions=True, power_scale=s, eps=e)], False)
    check_scale_and_eps(lambda s, e: list(plan.cwt_stx(xt, coef=True, bits=True, reductions=True, power_scale=s, eps=e)), False)
    check_scale_and_eps(lambda s, e: list(plan.cwt_stx(xt, coef=False, reductions=True, power_scale=s, eps=e)), False)
    plan.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_power_scale_and_eps_hipfft_engine_and_float64_atoms(dtype):
    """The hipFFT engine (n = 3000, both precisions) and the atoms bank on the native engines in the same precision."""
    f64 = dtype == np.float64
    m = 3000
    xm = torch.from_numpy(record(m, dtype, 12, channels=2)).cuda()
    gen, nbm = styx_stx_plan(m, 3, dtype, channels=2)
    assert gen.stage_bands("inverse")[STYX] == nbm and gen.stage_bands("inverse")[STX] == nbm
    for name in ("cwt", "stx"):
        fn = getattr(gen, name)
        check_scale_and_eps(lambda s, e: [fn(xm, coef=True, bits=True, reductions=True, power_scale=s, eps=e)], f64)
    check_scale_and_eps(lambda s, e: list(gen.cwt_stx(xm, coef=False, reductions="band", power_scale=s, eps=e)), f64)
    gen.close()
    if f64:
        n = 1 << 20
        x64 = torch.from_numpy(record(n, np.float64, 13, channels=2)).cuda()
        tables = atom_tables(n, 6, 1.0)
        atoms = bank_plan(n, np.float64, ATOMS, tables, channels=2)
        assert_native(atoms, ATOMS, len(tables[0]))
        check_scale_and_eps(lambda s, e: [atoms.cwt_atoms(x64, coef=True, bits=True, reductions=True, power_scale=s, eps=e)], True)
        atoms.close()


def test_power_scale_and_eps_float64_order12():
    """float64 2^20 order 12 x 2 records (the float64 zoom kernels with the MFMA interpolation, k_block64, k_block64_edge)
    through the joint call with and without stored panels, reductions="band" too."""
    n, order = 1 << 20, 12
    xt = torch.from_numpy(record(n, np.float64, 17, channels=2)).cuda()
    plan, nb = styx_stx_plan(n, order, np.float64, channels=2)
    assert_native(plan, STYX, nb)
    assert_native(plan, STX, nb)
    check_scale_and_eps(lambda s, e: list(plan.cwt_stx(xt, coef=True, bits=True, reductions=True, power_scale=s, eps=e)), True)
    check_scale_and_eps(lambda s, e: list(plan.cwt_stx(xt, coef=False, reductions=True, power_scale=s, eps=e)), True)
    check_scale_and_eps(lambda s, e: list(plan.cwt_stx(xt, coef=False, reductions="band", power_scale=s, eps=e)), True)
    plan.close()


@pytest.mark.parametrize("dtype,log2n,order", [(np.float32, 20, 3), (np.float64, 18, 12)])
def test_fused_call_sides_keep_their_own_scale_and_eps(dtype, log2n, order):
    """qi_cwt_stx through the C ABI with a different (power_scale, eps) on each side: each side equals its own separate
    call (joint launches against separate ones: float rounding), its bits use its own eps, its reductions its own scale."""
    n, f64 = 1 << log2n, dtype == np.float64
    xt = torch.from_numpy(record(n, dtype, 21, channels=2)).cuda()
    plan, nb = styx_stx_plan(n, order, dtype, channels=2)
    top = float(plan.cwt(xt, coef=True).coef.abs().max())
    sides = ((STYX, 2.0, 1e-3 * top), (STX, 0.25, 1e-5 * top))
    outs = [plan._outputs(which, 2, True, True, True, s, e, None, None) for which, s, e in sides]
    with torch.cuda.device(plan.device):
        _lib.check(plan._lib.qi_cwt_stx(plan._handle, STYX, _lib.ptr(xt), 2, C.byref(outs[0][1]), C.byref(outs[1][1]),
                                        plan._stream()))
    torch.cuda.synchronize()
    for (res, _), (which, s, e) in zip(outs, sides):
        sep = (plan.cwt if which == STYX else plan.stx)(xt, coef=True, bits=True, reductions=True, power_scale=s, eps=e)
        scale = float(sep.coef.abs().max())
        assert float((res.coef - sep.coef).abs().max()) <= (1e-12 if f64 else 2e-6) * scale, which
        want = torch.log2(res.coef.abs().double() + e)
        assert float((res.bits.double() - want).abs().max()) <= (1e-12 if f64 else 1e-5), which
        assert torch.allclose(res.power_band, sep.power_band, rtol=1e-11 if f64 else 1e-5), which
        assert torch.allclose(res.power_time.double(), sep.power_time.double(), rtol=1e-10 if f64 else 1e-4,
                              atol=(1e-13 if f64 else 1e-7) * float(sep.power_time.max())), which
        assert torch.allclose(res.stats[:, :3], sep.stats[:, :3], rtol=1e-11 if f64 else 1e-5), which
        check_direct(res, f64, which)
        del sep
    plan.close()


def test_stream_pipeline_power_scale_and_reused_outputs():
    """StreamPipeline(power_scale=2) yields exactly twice the default items; a result reused through out= reports the
    power_scale of the call that filled it."""
    n, hop, order = 1 << 16, 1 << 15, 3
    host = record(n + hop + 333, np.float64, 23, channels=3)
    plan, _ = styx_stx_plan(n, order, np.float64, channels=2)
    for keep_time in (True, False):
        one = list(stream.StreamPipeline(plan, host, hop, block=2, keep_time=keep_time).run())
        two = list(stream.StreamPipeline(plan, host, hop, block=2, power_scale=2.0, keep_time=keep_time).run())
        assert len(one) == len(two) == 2 * 3
        for a, b in zip(one, two):
            for ra, rb in ((a.cwt, b.cwt), (a.stx, b.stx)):
                assert rb.power_scale == 2.0
                assert torch.equal(rb.power_band, 2 * ra.power_band) and torch.equal(rb.stats[:, :2], 2 * ra.stats[:, :2])
                if keep_time:
                    assert torch.equal(rb.power_time, 2 * ra.power_time)
    xt = torch.from_numpy(host[:2, :n].copy()).cuda()
    first = plan.cwt(xt, coef=False, reductions=True, power_scale=2.0)
    want = plan.cwt(xt, coef=False, reductions=True, power_scale=0.5)
    again = plan.cwt(xt, coef=False, reductions=True, power_scale=0.5, out=first)
    assert again is first and again.power_scale == 0.5 and torch.equal(again.reduced, want.reduced)
    pair = plan.cwt_stx(xt, coef=False, reductions=True, power_scale=2.0)
    pair = plan.cwt_stx(xt, coef=False, reductions=True, power_scale=4.0, out=pair)
    assert [r.power_scale for r in pair] == [4.0, 4.0]
    plan.close()


# ---- degenerate records on the native engines ---------------------------------------------------------------------------
def degenerate_batch(n, dtype):
    """zeros; unit impulses at 0, n - 1, n / 2 and just before a block-stride boundary (3584 k); a chirp."""
    x = np.zeros((6, n))
    x[1, 0] = x[2, n - 1] = x[3, n // 2] = 1.0
    x[4, 3584 * (n // 3584 // 3) - 1] = 1.0
    x[5] = orc.synth_chirp(n, FS, 0, 1, np.float64)
    return x.astype(dtype)


def _rows(res, sl):
    return engine.TfrResult(frequency_hz=res.frequency_hz, power_band=res.power_band[sl], power_time=res.power_time[sl],
                            stats=res.stats[sl])


@pytest.mark.parametrize("dtype,log2n,order", [(np.float32, 20, 3), (np.float64, 18, 12)])
def test_degenerate_records_on_native_engines(dtype, log2n, order):
    """One batch of degenerate records through the styx CWT, the Stockwell transform and the atoms bank on the native
    engines (split-band edge items, the short-atom edge fix, the outermost blocks, the atoms' circular roll).  The
    all-zero record gives zero panels, log2(eps) bits and zero, finite reductions; every other record equals the hipFFT
    engine row by row (to each row's own maximum) and, for the impulses at the record ends, the oracle; each record
    equals its single-record run."""
    n, f64 = 1 << log2n, dtype == np.float64
    x = degenerate_batch(n, dtype)
    xt = torch.from_numpy(x).cuda()
    nat, nb = styx_stx_plan(n, order, dtype, channels=6)
    ref, _ = styx_stx_plan(n, order, dtype, _lib.QI_ENGINE_HIPFFT, channels=6)
    tables = atom_tables(n, order)
    for plan in (nat, ref):
        plan.set_gabor_bank(ATOMS, tables[0], *tables[1])
    nba = len(tables[0])
    runs = [("cwt", STYX, nb), ("stx", STX, nb)] + ([("cwt_atoms", ATOMS, nba)] if log2n >= 20 else [])  # (atoms: 2^20, 2^21)
    for _, which, count in runs:
        assert_native(nat, which, count)
    x64 = x.astype(np.float64)
    oracle = {
        "cwt": lambda c, pick: orc.cwt_fft(order, x64[c], FS, bands=pick)[2],
        "stx": lambda c, pick: orc.stx_fft(order, x64[c], FS, bands=pick)[2],
        "cwt_atoms": lambda c, pick: orc.cwt_chirp_fft(x64[c], FS, order, bands=pick)[0],
    }
    for name, _, count in runs:
        a = getattr(nat, name)(xt, coef=True, bits=True, reductions=True)
        b = getattr(ref, name)(xt, coef=True, reductions=True)
        # the all-zero record
        assert float(a.coef[0].abs().max()) == 0.0, name
        assert bool((a.bits[0] == -52.0).all()), name  # log2(0 + 2^-52)
        assert float(a.power_band[0].abs().max()) == 0.0 and float(a.power_time[0].abs().max()) == 0.0, name
        st = a.stats[0, :3]
        assert bool(torch.isfinite(st).all()) and float(st.abs().max()) == 0.0, (name, st)
        # every other record against the hipFFT engine
        check_rows(a.coef[1:], b.coef[1:], f64, name)
        check_bits(a.bits[1:], b.coef[1:], f64, name)
        check_reductions(_rows(a, slice(1, None)), _rows(b, slice(1, None)), f64, name)
        del b
        # the impulses at the record ends against the oracle
        pick = sorted({0, count // 3, count // 2, count - 1})
        for c in (1, 2):
            check_rows(a.coef[c, pick], oracle[name](c, pick), f64, (name, c), PANEL64_ATOM_AXIS)
        # each record equals its single-record run (a batch of six merges the split bands' edge items into a launch of
        # their own: float rounding, far inside the engine tolerance)
        for c in range(6):
            one = getattr(nat, name)(xt[c : c + 1], coef=True, reductions=True)
            d = (one.coef[0] - a.coef[c]).abs().amax(dim=1).double()
            worst = float((d / a.coef[c].abs().amax(dim=1).double().clamp_min(1e-300)).max())
            assert worst <= (1e-12 if f64 else 1e-6), (name, c, worst)
            assert torch.allclose(one.power_band[0], a.power_band[c], rtol=1e-12 if f64 else 1e-5, atol=0.0), (name, c)
            assert torch.allclose(one.power_time[0], a.power_time[c], rtol=1e-11 if f64 else 1e-5,
                                  atol=(1e-13 if f64 else 1e-7) * float(one.power_time.max())), (name, c)
            assert torch.allclose(one.stats[0, :3], a.stats[c, :3], rtol=1e-12 if f64 else 1e-5), (name, c)
            del one
        del a
    nat.close()
    ref.close()


# ---- plan-less kernels at multi-block shapes ----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n", [5000, 3 * 1024 + 7])
def test_panel_reductions_per_channel(dtype, n):
    """power_dynamics_scaled_bits, scale_power_bits and the three ShannonStft classes on [3, B, n] panels of distinct
    energy (several epilogue spans, a partial last one): every channel against the oracle."""
    rng = np.random.default_rng(n)
    p = np.stack([(a * rng.standard_normal((9, n)) + b) ** 2 for a, b in ((1.0, 0.0), (3.0, 0.5), (0.05, 0.02))]).astype(dtype)
    atol = 1e-9 if dtype == np.float64 else 1e-3
    red = 1e-10 if dtype == np.float64 else 1e-4
    bits, per_time, per_freq = tfr_info.power_dynamics_scaled_bits(p)
    sb = tfr_info.scale_power_bits(p)
    assert bits.shape == p.shape and per_time.shape == (3, n) and per_freq.shape == (3, 9)
    objs = (tfr_info.shannon_stft_from_tfr_power(p), tfr_info.ShannonStftPerTime(p), tfr_info.ShannonStftPerFreq(p))
    for c in range(3):
        pc = p[c].astype(np.float64)
        rb, rt, rf = orc.power_dynamics_scaled_bits(pc)
        assert np.max(np.abs(bits[c] - rb)) <= atol, c
        assert np.max(np.abs(per_time[c] - rt)) <= atol, c
        assert np.max(np.abs(per_freq[c] - rf)) <= atol, c
        assert np.max(np.abs(sb[c] - rb)) <= atol, c
        for obj, want in zip(objs, (orc.shannon_from_power(pc), orc.shannon_per_time(pc), orc.shannon_per_freq(pc))):
            assert np.max(np.abs(obj.info[c] - want.info)) <= atol, c
            assert relmax(obj.shannon_bits[c], want.shannon_bits) <= red, c
            assert np.max(np.abs(obj.isnr[c] - want.isnr)) <= atol, c
            assert relmax(obj.esnr[c], want.esnr) <= red, c
            assert obj.ref_bits == want.ref_bits


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n", [3 * 4096 + 5, 1 << 16])
def test_shannon_1d_per_channel(dtype, n):
    """ShannonTDR / ShannonFFT on three records of distinct energy at lengths of several reduction spans and several
    unwrap chunks: every channel against the oracle."""
    rng = np.random.default_rng(n + 1)
    x = np.stack([a * (orc.synth_chirp(n, FS, c, 3, np.float64) + 0.3 * rng.standard_normal(n))
                  for c, a in enumerate((1.0, 7.0, 0.05))]).astype(dtype)
    f64 = dtype == np.float64
    rel = 1e-12 if f64 else 2e-6
    tdr, fft = tfr_info.ShannonTDR(x), tfr_info.ShannonFFT(x)
    for c in range(3):
        xc = x[c].astype(np.float64)
        sig_n, marg = orc.shannon_tdr(xc)
        spec, angle, freq, fmarg = orc.shannon_fft(xc)
        np.testing.assert_allclose(tdr.sig[c], sig_n, rtol=rel, atol=rel * np.abs(sig_n).max())
        np.testing.assert_allclose(fft.sig[c], spec, rtol=0, atol=10 * rel * np.abs(spec).max())
        np.testing.assert_array_equal(fft.frequency, freq)
        if f64:
            np.testing.assert_allclose(fft.angle_rads[c], angle, rtol=0, atol=1e-8)
        else:  # modulo 2 pi the phases agree; unwrapped, no step exceeds pi (to the rounding of the largest value)
            got = fft.angle_rads[c].astype(np.float64)
            ulp = 4 * float(np.spacing(np.float32(np.abs(got).max())))
            assert np.abs(np.angle(np.exp(1j * (got - angle)))).max() <= 2e-3 + ulp
            assert np.abs(np.diff(got)).max() <= np.pi + 1e-5 + ulp and abs(got[0]) <= np.pi + 1e-6
        for obj, m in ((tdr, marg), (fft, fmarg)):
            info, ent, ref_ent, isnr, esnr = orc.shannon_1d(m)
            # (float32: the information of a bin is compared where the rounding of its marginal cannot move it)
            sel = np.ones(m.shape, bool) if f64 else m >= 1e-3 * m.max()
            np.testing.assert_allclose(obj.marginal[c], m, rtol=10 * rel, atol=rel * m.max())
            np.testing.assert_allclose(obj.info[c][sel], info[sel], rtol=0, atol=1e-9 if f64 else 2e-4)
            np.testing.assert_allclose(obj.isnr[c][sel], isnr[sel], rtol=0, atol=1e-9 if f64 else 2e-4)
            np.testing.assert_allclose(obj.entropy[c], ent, rtol=1e-9 if f64 else 1e-4, atol=rel * ent.max())
            np.testing.assert_allclose(obj.esnr[c], esnr, rtol=1e-9 if f64 else 1e-4, atol=10 * rel * esnr.max())
            assert obj.ref_entropy == ref_ent
