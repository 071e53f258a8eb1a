"""The STFT's reduced product (qi_stft_out: power marginals and entropy sums from the kernel that forms the coefficients)
against the float64 oracle panel reduced in NumPy (-m gpu).

tests/stft_reduced_cases.py holds the cases, the reference reduction and the bounds (the reduction contract: float64 1e-10,
float32 1e-4).  Which branch of qi_stft_fused.hip / qi_api_ops.hip each group is there for:

  test_plain_form_every_fused_length
      k_stft_fused<T, R, C, PLAIN, RED, no panels> at all seven shapes (float64: six) through stft_reductions_from_sig: one
      segment group of 7 - 9 segments (3 at n = seg), i.e. lanes of a group past the last segment (tiles of zeros, P = 0), the
      per-bin sum over the group's lanes (group_sum), the pair (k, M - k) walk with its single middle bin, and the last
      column, which is the one-sample segment.  The same request with both panels (<PLAIN, RED, WZ, WB>): coefficients and
      bits are stft_from_sig's bit for bit and the reductions are those without panels, at every length.
  test_several_groups_and_a_ragged_last_one
      44 and 82 segments: k_stft_reduce adds three or more partials per bin in index order, the last group is not full.
  test_general_form
      seg < nfft, hop 1 / odd hop / hop = seg, a Gaussian window, through _stft_windowed's private keyword: with `coef`
      alone the general walk <PLAIN = false, RED, WZ> (its coefficients are qi_stft's, bit for bit), with no panel the PLAIN
      walk on the same shapes.  seg96_hop96's all-zero last segment: power_time exactly 0 there, nothing NaN.
  test_hipfft_path
      nfft 300, nfft 4096 in float64, seg 8192: frames -> hipFFT -> transpose (into scratch without `coef`) -> k_epilogue ->
      k_finalize.
  test_output_options
      one fused and one hipFFT shape: panels equal to qi_stft's, reductions equal with and without them, power_scale,
      reductions="band", nothing asked for.
  test_batch_invariance, test_zero_record, test_gather_layout
"""
import ctypes as C

import numpy as np
import pytest
import torch

import stft_cases as sc
import stft_reduced_cases as rc

from quantum_inferno_amd import _lib, dist, engine, styx_fft

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
IDS = ["f64", "f32"]


def as_numpy(res):
    """(power_band, power_time or None, stats, entropy_bits) of a TfrResult as NumPy arrays."""
    pt = None if res.power_time is None else res.power_time.cpu().numpy()
    return res.power_band.cpu().numpy(), pt, res.stats.cpu().numpy(), res.entropy_bits.cpu().numpy()


def same_reductions(a, b):
    return (torch.equal(a.power_band, b.power_band) and torch.equal(a.stats, b.stats)
            and (a.power_time is None or b.power_time is None or torch.equal(a.power_time, b.power_time)))


def from_sig_reduce(case, dtype, x=None, **kw):
    order, center, octaves = sc.SEGMENT_ARGS[case.seg]
    x = sc.from_sig_record(case, dtype) if x is None else x
    return styx_fft.stft_reductions_from_sig(x, sc.FS, order, center, octaves, **kw)


def spectral_reduce(case, dtype, x=None, **options):
    """_stft_windowed(_reduce=options) with the arguments stft_complex_pow2 / gtx_complex_pow2 hand it."""
    seg, overlap, nfft = sc.spectral_geometry(case)
    x = sc.spectral_record(case, dtype) if x is None else x
    return styx_fft._stft_windowed(x, sc.FS, sc.spectral_window(case), seg, overlap, nfft, _reduce=options)


def check_with_panels(case, dtype, bare):
    """The same request with both panels: stft_from_sig's coefficients and bits, bit for bit, and the reductions of `bare`."""
    order, center, octaves = sc.SEGMENT_ARGS[case.seg]
    x = torch.from_numpy(sc.from_sig_record(case, dtype)).cuda()
    z, bits, _, _ = styx_fft.stft_from_sig(x, sc.FS, order, center, octaves)
    _, _, full = styx_fft._stft_windowed(x, sc.FS, styx_fft.tukey_window_periodic(case.seg, 1.0), case.seg, case.seg // 2, case.seg,
                                         extra_scale=2 * np.sqrt(np.pi) / case.seg, _reduce=dict(coef=True, bits=True))
    assert torch.equal(full.coef, z) and torch.equal(full.bits, bits), sc.from_sig_id(case)
    assert same_reductions(full, bare), sc.from_sig_id(case)


def plain_params():
    return [pytest.param(case, dtype, id=f"{sc.from_sig_id(case)}-{tag}")
            for dtype, tag in zip(DTYPES, IDS) for case in rc.plain_cases(dtype)]


@pytest.mark.parametrize("case,dtype", plain_params())
def test_plain_form_every_fused_length(case, dtype):
    assert sc.fused_transform(case.seg, case.seg, dtype)
    res, t, f = from_sig_reduce(case, dtype)
    ref_f, ref_t, ref_z = sc.from_sig_reference(case, dtype)
    assert np.array_equal(t, ref_t) and np.array_equal(f, ref_f) and np.array_equal(res.frequency_hz, ref_f)
    assert res.coef is None and res.bits is None and res.reduced is not None
    assert res.power_time.shape == (sc.CHANNELS, ref_z.shape[-1]) and ref_z.shape[-1] <= 16
    rc.check_reduced(*as_numpy(res), rc.from_sig_reduced(case, dtype), dtype, sc.from_sig_id(case))
    check_with_panels(case, dtype, res)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", rc.GROUP_CASES, ids=sc.from_sig_id)
def test_several_groups_and_a_ragged_last_one(case, dtype):
    res, _, _ = from_sig_reduce(case, dtype)
    n_seg = res.power_time.shape[-1]
    assert n_seg > 32 and n_seg % 16 != 0
    rc.check_reduced(*as_numpy(res), rc.from_sig_reduced(case, dtype), dtype, sc.from_sig_id(case))
    check_with_panels(case, dtype, res)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("coef", [True, False], ids=["coef", "nopanel"])
@pytest.mark.parametrize("name", rc.GENERAL_NAMES)
def test_general_form(name, coef, dtype):
    case = rc.spectral_case(name)
    seg, overlap, nfft = sc.spectral_geometry(case)
    assert sc.fused_transform(nfft, seg, dtype)
    x = torch.from_numpy(sc.spectral_record(case, dtype)).cuda()
    f, t, res = spectral_reduce(case, dtype, x, coef=coef)
    ref_f, ref_t, ref_z = sc.spectral_reference(case, dtype)
    assert np.array_equal(t, ref_t) and np.array_equal(f, ref_f)
    ref = rc.spectral_reduced(case, dtype)
    rc.check_reduced(*as_numpy(res), ref, dtype, name)
    assert torch.isfinite(res.stats).all() and torch.isfinite(res.power_time).all()
    if sc.last_segment_all_zero(case.n, seg, seg - overlap):
        assert name == "seg96_hop96" and torch.all(res.power_time[:, -1] == 0)
    else:
        assert name != "seg96_hop96"
    if coef:  # the coefficients are those of the wrappers' own call (qi_stft with Z alone: the general store loop)
        fn = styx_fft.stft_complex_pow2 if case.fn == "stft" else styx_fft.gtx_complex_pow2
        _, _, z = fn(x, sc.FS, case.seg, overlap_points=case.overlap, nfft_points=case.nfft)
        assert res.bits is None and torch.equal(res.coef, z)


def hipfft_params():
    out = [pytest.param(rc.spectral_case(name), dtype, id=f"{name}-{IDS[DTYPES.index(dtype)]}")
           for name, dtypes in rc.HIPFFT_SPECTRAL for dtype in dtypes]
    return out + [pytest.param(rc.HIPFFT_FROM_SIG, dtype, id=f"{sc.from_sig_id(rc.HIPFFT_FROM_SIG)}-{tag}")
                  for dtype, tag in zip(DTYPES, IDS)]


@pytest.mark.parametrize("case,dtype", hipfft_params())
def test_hipfft_path(case, dtype):
    if isinstance(case, sc.FromSig):
        assert not sc.fused_transform(case.seg, case.seg, dtype)
        res, _, _ = from_sig_reduce(case, dtype)
        ref, what = rc.from_sig_reduced(case, dtype), sc.from_sig_id(case)
    else:
        seg, _, nfft = sc.spectral_geometry(case)
        assert not sc.fused_transform(nfft, seg, dtype)
        _, _, res = spectral_reduce(case, dtype, coef=False)
        ref, what = rc.spectral_reduced(case, dtype), case.name
    assert res.coef is None and res.bits is None
    rc.check_reduced(*as_numpy(res), ref, dtype, what)


def run_options(dtype, fused):
    """-> run(**options) -> TfrResult with fresh tensors, (z, bits) of qi_stft, reference(power_scale)."""
    if fused:  # StftPlan at order 1: 128-sample segments
        case = sc.FromSig(128, 3 * 128 + 1)
        x = torch.from_numpy(sc.from_sig_record(case, dtype)).cuda()
        plan = styx_fft.StftPlan(case.n, sc.CHANNELS, sc.FS, 1, x.dtype)
        assert plan.seg == 128

        def run(**kw):
            res = plan.reduce(x, **kw)
            return engine.TfrResult(res.frequency_hz, *(None if v is None else v.clone() for v in
                                                        (res.coef, res.bits, res.power_band, res.power_time, res.stats)))

        z, bits = (v.clone() for v in plan.run(x))
        return run, z, bits, lambda ps: rc.from_sig_reduced(case, dtype, ps)
    case = rc.spectral_case("seg200_nfft300")
    seg, overlap, nfft = sc.spectral_geometry(case)
    x = torch.from_numpy(sc.spectral_record(case, dtype)).cuda()
    _, _, z, bits = styx_fft._stft_windowed(x, sc.FS, sc.spectral_window(case), seg, overlap, nfft, want_bits=True)
    return (lambda **kw: spectral_reduce(case, dtype, x, **kw)[2]), z, bits, lambda ps: rc.spectral_reduced(case, dtype, ps)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "hipfft"])
def test_output_options(fused, dtype):
    run, z, bits, reference = run_options(dtype, fused)
    bare = run(coef=False, bits=False)
    assert bare.coef is None and bare.bits is None
    rc.check_reduced(*as_numpy(bare), reference(1.0), dtype, "no panel")
    # both panels: qi_stft's, bit for bit; the reductions do not change with them
    full = run(coef=True, bits=True)
    assert torch.equal(full.coef, z) and torch.equal(full.bits, bits)
    assert same_reductions(full, bare)
    # the panels alone: qi_stft itself
    only = run(coef=True, bits=True, reductions=False)
    assert only.power_band is None and only.stats is None and only.power_time is None
    assert torch.equal(only.coef, z) and torch.equal(only.bits, bits)
    # power_scale = 2: against the reference, and (a factor of two is exact) twice the unscaled sums
    twice = run(coef=False, bits=False, power_scale=2.0)
    rc.check_reduced(*as_numpy(twice), reference(2.0), dtype, "power_scale 2")
    assert torch.equal(twice.power_band, 2 * bare.power_band) and torch.equal(twice.power_time, 2 * bare.power_time)
    assert torch.equal(twice.stats[:, :2], 2 * bare.stats[:, :2])
    # no per-time marginal
    band = run(coef=False, bits=False, reductions="band")
    assert band.power_time is None and same_reductions(band, bare)


def test_nothing_asked_for_is_an_error():
    lib = _lib.require_gpu()
    x = torch.zeros((1, 385), dtype=torch.float32, device="cuda")
    win = torch.ones(128, dtype=torch.float32, device="cuda")
    nbytes = int(lib.qi_stft_out_scratch_bytes(_lib.QI_F32, 1, 385, 128, 64, 128, 0, 0))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    desc = _lib.TfrOut(power_scale=1.0)
    rc_ = lib.qi_stft_out(_lib.QI_F32, x.device.index, _lib.ptr(x), 1, 385, _lib.ptr(win), 128, 64, 128, 1.0, C.byref(desc),
                          _lib.ptr(scratch), nbytes, _lib.stream_ptr(x.device))
    assert rc_ == -1 and b"nothing to produce" in lib.qi_last_error()
    # statistics without the band powers (they come together), and a scratch one byte short
    stats = torch.empty((1, 4), dtype=torch.float64, device="cuda")
    desc = _lib.TfrOut(stats=_lib.ptr(stats))
    assert lib.qi_stft_out(_lib.QI_F32, x.device.index, _lib.ptr(x), 1, 385, _lib.ptr(win), 128, 64, 128, 1.0, C.byref(desc),
                           _lib.ptr(scratch), nbytes, _lib.stream_ptr(x.device)) == -1
    band = torch.empty((1, 65), dtype=torch.float64, device="cuda")
    desc = _lib.TfrOut(power_band=_lib.ptr(band), stats=_lib.ptr(stats))
    assert lib.qi_stft_out(_lib.QI_F32, x.device.index, _lib.ptr(x), 1, 385, _lib.ptr(win), 128, 64, 128, 1.0, C.byref(desc),
                           _lib.ptr(scratch), nbytes - 1, _lib.stream_ptr(x.device)) == -1


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", ["seg64_groups", "seg512_groups", "hipfft"])
def test_batch_invariance(shape, dtype):
    """Channel 1 of the three-channel call against the same record alone.  The partials are per (record, group), so the
    record count changes nothing; what the loaders do depends on the record's ADDRESS alone (2-sample alignment picks the
    vector, pair or scalar loads, and the pair loader adds the segment mean in another order), so the 512-sample shape,
    which the pair loader takes, runs the record where it lies (a view of the batch); the others run a copy of it."""
    if shape == "hipfft":
        case = rc.spectral_case("seg200_nfft300")
        x = torch.from_numpy(sc.spectral_record(case, dtype)).cuda()
        run = lambda sig: spectral_reduce(case, dtype, sig, coef=False)[2]
    else:
        case = rc.GROUP_CASES[1 if shape == "seg64_groups" else 0]
        x = torch.from_numpy(sc.from_sig_record(case, dtype)).cuda()
        run = lambda sig: from_sig_reduce(case, dtype, sig)[0]
    batch = run(x)
    alone = run(x[1:2] if shape == "seg512_groups" else x[1:2].clone())
    assert alone.power_band.shape[0] == 1
    assert torch.equal(alone.power_band[0], batch.power_band[1]) and torch.equal(alone.power_time[0], batch.power_time[1])
    assert torch.equal(alone.stats[0], batch.stats[1])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", ["fused", "hipfft"])
def test_zero_record(shape, dtype):
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    if shape == "fused":
        x = torch.zeros((2, 40 * 64 + 1), dtype=tdt, device="cuda")
        res, _, _ = styx_fft.stft_reductions_from_sig(x, sc.FS, *sc.SEGMENT_ARGS[64])
    else:
        case = rc.spectral_case("seg200_nfft300")
        _, _, res = spectral_reduce(case, dtype, torch.zeros((2, case.n), dtype=tdt, device="cuda"), coef=False)
    for v in (res.power_band, res.power_time, res.stats):
        assert torch.isfinite(v).all() and torch.all(v == 0)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gather_layout(dtype):
    """pack_reduced of a CWT, a Stockwell and an STFT result of the same records is one buffer in the reduced_slots layout:
    unpacked with the three shapes it gives the results' own tensors back."""
    n, order = 4096, 3
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    x = torch.from_numpy(sc.record(n, [7, n], dtype)).cuda()
    bands = len(engine.scales.log_frequency_hz_from_fft_points(sc.FS, n, order))
    plan = engine.TfrPlan(n, tdt, "cuda:0", engine.TfrPlan.workspace_for(n, bands, tdt))
    plan.set_styx_bank(order, sc.FS)
    plan.set_stx_bands(order, sc.FS)
    stft_plan = styx_fft.StftPlan(n, sc.CHANNELS, sc.FS, 1, tdt)
    results = [plan.cwt(x, coef=False, reductions=True), plan.stx(x, coef=False, reductions=True), stft_plan.reduce(x)]
    stft = results[2]
    assert stft.reduced.numel() == dist.reduced_slots(sc.CHANNELS, stft_plan.n_f, stft_plan.n_seg, tdt)
    assert stft.power_band.shape == (sc.CHANNELS, stft_plan.n_f) and stft.power_time.shape == (sc.CHANNELS, stft_plan.n_seg)
    # kept between calls like the plan's other buffers
    assert stft_plan.reduce(x).reduced.data_ptr() == stft.reduced.data_ptr()
    flat = dist.pack_reduced(results)
    shapes = [(bands, n), (bands, n), (stft_plan.n_f, stft_plan.n_seg)]
    assert flat.numel() == sum(dist.reduced_slots(sc.CHANNELS, b, m, tdt) for b, m in shapes)
    for res, (band, time, stats) in zip(results, dist.unpack_reduced(flat, sc.CHANNELS, shapes, tdt)):
        assert torch.equal(band, res.power_band) and torch.equal(time, res.power_time) and torch.equal(stats, res.stats)
    # one caller-owned message for the three
    message = torch.empty(flat.numel(), dtype=torch.float64, device="cuda")
    first = sum(dist.reduced_slots(sc.CHANNELS, b, m, tdt) for b, m in shapes[:2])
    again = stft_plan.reduce(x, reduced_out=message[first:])
    assert again.reduced.data_ptr() == message[first:].data_ptr() and same_reductions(again, stft)
    plan.close()
