"""Synchrosqueezing on the device (include/qi_squeeze.h): qi_tfr_squeeze on every case of tests/squeeze_cases.py bit for bit
against the NumPy restatement in the panel's precision, on given frequency tables; qi_tfr_ifreq as wrapped phase against the
float64 restatement, its NaN mask exactly; qi_tfr_synchrosqueeze bit for bit against the two calls on the device and, away
from the bins' edges, against the float64 restatement; the header's contract (a column and its partner alone decide, a record's
place in the batch, two runs); the wrappers on the tone and the chirp; the stream-order cases of
tests/squeeze_stream_cases.py."""
import numpy as np
import pytest
import torch

import squeeze_cases as sq
import squeeze_stream_cases as ssc
import stream_order as so

from quantum_inferno_amd import _lib, engine, styx_cwt, styx_stx
from quantum_inferno_amd import scales_dyadic as scales

pytestmark = pytest.mark.gpu
REAL = {"float32": torch.float32, "float64": torch.float64}
CPLX = {"float32": torch.complex64, "float64": torch.complex128}


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()  # (a copy: the cases' arrays are read-only)


def host(t):
    return t.detach().cpu().numpy()


def call(which, z, fs=sq.FS, edges=None, carrier=None, weight=None, floor=0.0, given=None):
    """One of the three entry points on a device panel, straight through the library, every output prefilled with NaN: an
    element the call does not write stays NaN."""
    lib = _lib.require_gpu()
    C, nb, n = z.shape
    rdtype = torch.float32 if z.dtype == torch.complex64 else torch.float64
    code, device = _lib.dtype_code(rdtype), z.device
    nbin = 1 if edges is None else len(edges) - 1
    keep = [None if v is None else _lib.darr(v) for v in (carrier, edges, weight)]
    c_ptr, e_ptr, w_ptr = (None if k is None else k[1] for k in keep)
    scratch, nbytes = _lib.scratch(lib.qi_tfr_squeeze_scratch_bytes, device, code, C, nb, n, nbin)
    if which == "ifreq":
        out = torch.full((C, nb, n), 12345.0, dtype=rdtype, device=device)
        _lib.call(lib.qi_tfr_ifreq, device, code, device.index, _lib.ptr(z), C, nb, n, c_ptr, fs, floor, _lib.ptr(out), _lib.ptr(scratch), nbytes)
        assert not (out == 12345.0).any()
        return out
    out = torch.full((C, nbin, n), float("nan"), dtype=z.dtype, device=device)
    if which == "squeeze":
        _lib.call(lib.qi_tfr_squeeze, device, code, device.index, _lib.ptr(z), _lib.ptr(given), C, nb, n, e_ptr, nbin, w_ptr, _lib.ptr(out),
                  _lib.ptr(scratch), nbytes)
    else:
        _lib.call(lib.qi_tfr_synchrosqueeze, device, code, device.index, _lib.ptr(z), C, nb, n, c_ptr, fs, floor, e_ptr, nbin, w_ptr,
                  _lib.ptr(out), _lib.ptr(scratch), nbytes)
    return out


def assert_same_values(got, want, what):
    """Bit for bit, but for the payload of a NaN: the same NaN mask, and the same bits everywhere else (the sign of a zero too)."""
    assert got.dtype == want.dtype and got.shape == want.shape, what
    r = sq.real_of(got)
    g, w = np.ascontiguousarray(got).view(r), np.ascontiguousarray(want).view(r)
    nan = np.isnan(w)
    assert np.array_equal(np.isnan(g), nan), what
    bits = np.uint32 if r == np.float32 else np.uint64
    diff = g.view(bits)[~nan] != w.view(bits)[~nan]
    assert not diff.any(), f"{what}: {int(diff.sum())} of {diff.size} values differ"


# ---- qi_tfr_squeeze: exact given the frequencies -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", sq.DTYPES)
@pytest.mark.parametrize("cid", sq.ids())
def test_squeeze_is_the_restatement_bit_for_bit(cid, dtype):
    c = sq.by_id(cid)
    edges, weight = sq.case_edges(sq.bins(c, dtype)), sq.weight_of(c.nb)
    runs = [(False, kind, None) for kind in sq.TABLE_KINDS] + [(False, "random", weight), (True, "planted", None), (True, "one_bin", weight)]
    for whole, kind, w in runs:
        z = np.array(sq.panel(cid, dtype, whole))
        f = sq.given_frequencies(cid, dtype, kind)
        if kind == "planted":  # what is not moved enters nothing: NaN and Inf coefficients under the dropped frequencies
            cc, bb, tt = np.nonzero(sq.bins_of(f, edges) < 0)
            z[cc, bb, tt] = np.where(np.arange(len(cc)) % 2 == 0, np.nan, np.inf) * (1 - 1j)
        want = sq.squeeze_restated(z, f, edges, w)
        got = host(call("squeeze", dev(z), edges=edges, weight=w, given=dev(f)))
        assert np.isfinite(got.view(sq.real_of(got))).all(), (kind, whole)  # every element written, nothing poisoned
        assert_same_values(got, want, f"{cid} {dtype} {kind} whole={whole} weight={w is not None}")
        if kind == "one_bin" and not whole:
            k = sq.bins(c, dtype) // 2
            assert not np.delete(got, k, axis=1).any() and got[:, k].all()


@pytest.mark.parametrize("dtype", sq.DTYPES)
def test_a_nan_that_is_moved_poisons_its_bin_alone(dtype):
    c = sq.by_id("c3_b24_n700_k65")
    z, edges = np.array(sq.panel(c.id, dtype)), sq.case_edges(sq.bins(c, dtype))
    f = sq.given_frequencies(c.id, dtype, "random")
    k = sq.bins_of(f, edges)
    cc, bb, tt = (a[:50] for a in np.nonzero(k >= 0))
    z[cc, bb, tt] = np.nan
    got = host(call("squeeze", dev(z), edges=edges, given=dev(f)))
    want = np.zeros(got.shape, dtype=bool)
    want[cc, k[cc, bb, tt], tt] = True
    assert np.array_equal(np.isnan(got), want)


def test_wrappers_numpy_in_numpy_out_and_their_refusals():
    c = sq.by_id("c3_b24_n256_k32")
    z, edges = np.array(sq.panel(c.id, "float32")), sq.case_edges(40)
    f = engine.instantaneous_frequency(z, sq.FS, sq.carrier_of(c.nb), 0.25)
    assert isinstance(f, np.ndarray) and f.dtype == np.float32 and f.shape == z.shape and np.isnan(f).any()
    out = engine.squeeze(z, f, edges, sq.weight_of(c.nb))
    fused = engine.synchrosqueeze(z, sq.FS, edges, sq.carrier_of(c.nb), sq.weight_of(c.nb), 0.25)
    assert isinstance(out, np.ndarray) and out.dtype == np.complex64 and out.shape == (c.C, 40, c.n) and np.array_equal(out, fused)
    on_device = engine.synchrosqueeze(dev(z), sq.FS, edges, sq.carrier_of(c.nb), sq.weight_of(c.nb), 0.25)
    assert isinstance(on_device, torch.Tensor) and on_device.is_cuda and np.array_equal(host(on_device), fused)
    for bad in (lambda: engine.squeeze(z, f.astype(np.float64), edges), lambda: engine.squeeze(z, f[:, :-1], edges),
                lambda: engine.synchrosqueeze(z, sq.FS, edges[:1]), lambda: engine.synchrosqueeze(z, sq.FS, edges, carrier_hz=np.zeros(3)),
                lambda: engine.instantaneous_frequency(z.real, sq.FS)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(_lib.QiError):
        engine.synchrosqueeze(z, sq.FS, edges[::-1].copy())


# ---- qi_tfr_ifreq: a tolerance on the phase, the mask exactly -----------------------------------------------------------------------
def wrapped(f, carrier, fs):
    return np.exp(2j * np.pi * (f - carrier[None, :, None]) / fs)


@pytest.mark.parametrize("dtype", sq.DTYPES)
@pytest.mark.parametrize("cid", sq.ids())
def test_ifreq_against_the_restatement(cid, dtype):
    c = sq.by_id(cid)
    r = np.dtype(dtype).type
    carrier = sq.carrier_of(c.nb)
    car = carrier.astype(r).astype(np.float64)
    z = np.array(sq.panel(cid, dtype))
    got = host(call("ifreq", dev(z), carrier=carrier)).astype(np.float64)
    want = sq.ifreq_restated(z, sq.FS, carrier)
    assert not np.isnan(got).any() and not np.isnan(want).any()
    err = float(np.abs(wrapped(got, car, sq.FS) - wrapped(want, car, sq.FS)).max())
    print(f"squeeze ifreq {cid} {dtype}: wrapped phase within {err:.3g}")
    assert err <= sq.PHASE_TOL[dtype]
    # powers at, one ulp below and one ulp above the floor, zeros, NaN, Inf and a finite coefficient whose power overflows:
    # in a column, in its partner, and in the last two columns
    z0 = sq.COMPLEX[dtype](0.8125 - 0.34375j)
    p0 = sq.power_of(np.array([z0]))[0]
    big = r(1e25) if dtype == "float32" else r(1e200)
    specials = [z0, 0, np.nan, z0, np.inf * (1 + 0j), big, z0, -0.0]
    rng = np.random.default_rng([61, c.nb, c.n])
    for k, value in enumerate(specials):
        z[rng.integers(c.C), rng.integers(c.nb), (0, 1, c.n - 2, c.n - 1, c.n // 2, c.n // 2 + 1, c.n // 3, 2 * c.n // 3)[k] % c.n] = value
    z[0, 0, c.n - 1], z[c.C - 1, c.nb - 1, c.n - 2] = z0, z0
    for floor in (p0, np.nextafter(p0, r(np.inf)), np.nextafter(p0, r(0)), r(0)):
        got = host(call("ifreq", dev(z), carrier=carrier, floor=float(floor))).astype(np.float64)
        want = sq.ifreq_restated(z, sq.FS, carrier, float(floor))
        assert np.array_equal(np.isnan(got), np.isnan(want)), (cid, dtype, float(floor))
        ok = ~np.isnan(want)
        assert ok.any() or c.n * c.nb < 8
        assert np.abs(wrapped(got, car, sq.FS)[ok] - wrapped(want, car, sq.FS)[ok]).max(initial=0.0) <= sq.PHASE_TOL[dtype]


# ---- qi_tfr_synchrosqueeze ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", sq.DTYPES)
@pytest.mark.parametrize("cid", sq.ids())
def test_the_fused_call_is_the_composition_bit_for_bit(cid, dtype):
    c = sq.by_id(cid)
    edges, carrier, weight = sq.case_edges(sq.bins(c, dtype)), sq.carrier_of(c.nb), sq.weight_of(c.nb)
    z = sq.panel(cid, dtype)
    zd = dev(z)
    for floor in (0.0, 1.0):  # (a floor of 1: about two in five of the normal coefficients are below it)
        fused = call("fused", zd, edges=edges, carrier=carrier, weight=weight, floor=floor)
        f = call("ifreq", zd, carrier=carrier, floor=floor)
        two = call("squeeze", zd, edges=edges, weight=weight, given=f)
        assert so.same_bits(fused, two), (cid, dtype, floor)
        assert torch.isfinite(torch.view_as_real(fused)).all()  # every element written
        want, f64 = sq.synchro_restated(z, sq.FS, edges, carrier, weight, floor)
        assert np.array_equal(np.isnan(host(f)), np.isnan(f64))
        touched, share = sq.near_edges(f64, edges.astype(dtype).astype(np.float64), sq.EDGE_GUARD[dtype] * sq.FS)
        assert share <= sq.EXCLUDED_CAP
        err = float(np.abs(host(fused).astype(np.complex128) - want)[~touched].max(initial=0.0) / np.abs(want).max(initial=1e-300))
        print(f"squeeze fused {cid} {dtype} floor {floor}: within {err:.3g} of the largest modulus, {share:.4f} of the elements near an edge")
        assert err <= sq.FUSED_TOL[dtype]


# ---- the contract ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", sq.DTYPES)
@pytest.mark.parametrize("nbin", (7, 64, 568))
def test_a_column_and_its_partner_alone_decide(nbin, dtype):
    c = sq.Case("contract", 3, 24, 700, nbin)
    rng = np.random.default_rng([67, sq.bins(c, dtype)])
    z = dev((rng.standard_normal((c.C, c.nb, c.n)) + 1j * rng.standard_normal((c.C, c.nb, c.n))).astype(sq.COMPLEX[dtype]))
    edges, carrier, weight = sq.case_edges(sq.bins(c, dtype)), sq.carrier_of(c.nb), sq.weight_of(c.nb)
    kw = dict(edges=edges, carrier=carrier, weight=weight, floor=0.5)
    whole = call("fused", z, **kw)
    assert so.same_bits(call("fused", z, **kw), whole)  # two runs
    f = call("ifreq", z, carrier=carrier, floor=0.5)
    for a, b in ((100, 400), (0, 257), (255, 700), (511, 513)):  # any tile position; columns a .. b - 2 have their partner inside
        part = call("fused", z[:, :, a:b].contiguous(), **kw)
        assert so.same_bits(part[:, :, :b - a - 1].contiguous(), whole[:, :, a:b - 1].contiguous()), (a, b)
        f_part = call("ifreq", z[:, :, a:b].contiguous(), carrier=carrier, floor=0.5)
        assert so.same_bits(f_part[:, :, :b - a - 1].contiguous(), f[:, :, a:b - 1].contiguous()), (a, b)
    for record in range(c.C):  # a record alone, and at another place of the batch
        assert so.same_bits(call("fused", z[record:record + 1].contiguous(), **kw), whole[record:record + 1].contiguous())
    assert so.same_bits(call("fused", z.flip(0).contiguous(), **kw), whole.flip(0).contiguous())


# ---- the wrappers on the tone and the chirp ------------------------------------------------------------------------------------------------
def method_figures(kind, order, signal, n, dtype):
    wrapper = styx_cwt.cwt_synchrosqueezed_pow2 if kind == "cwt" else styx_stx.stx_synchrosqueezed_pow2
    plain = styx_cwt.cwt_complex_any_scale_pow2 if kind == "cwt" else styx_stx.stx_complex_any_scale_pow2
    sig, truth = (sq.tone(n), None) if signal == "tone" else sq.chirp(n)
    per = 1 if signal == "tone" else 8
    x = dev(sig.astype(dtype))
    centre, time_s, out = wrapper(order, x, sq.FS, bins_per_band=per)
    f, _, panel = plain(order, x, sq.FS)
    assert isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == CPLX[dtype] and tuple(out.shape) == (len(f) * per, n)
    assert np.array_equal(time_s, np.arange(n) / sq.FS)
    edges, w_centre = scales.squeeze_bin_edges(f, per)
    assert np.array_equal(centre, w_centre)
    carrier = None if kind == "cwt" else scales.stx_shift_indices(f, n, sq.FS) * sq.FS / n
    assert so.same_bits(engine.synchrosqueeze(panel[None], sq.FS, edges, carrier_hz=carrier)[0], out)
    return f, host(panel.abs() ** 2).astype(np.float64), edges, centre, host(out.abs() ** 2).astype(np.float64), truth


@pytest.mark.parametrize("n", (4096, 1 << 14))
@pytest.mark.parametrize("order", sq.ORDERS)
@pytest.mark.parametrize("kind", ("cwt", "stx"))
def test_wrappers_squeeze_the_tone_and_the_chirp(kind, order, n, capsys):
    cols = sq.inner(n)
    for dtype in sq.DTYPES if n == 4096 else ("float32",):
        f, raw, edges, _, power, _ = method_figures(kind, order, "tone", n, dtype)
        k = int(np.searchsorted(edges, sq.TONE_HZ)) - 1
        share, before = sq.bin_share(power, k, cols), sq.bin_share(raw, k, cols)
        f, raw, _, centre, power, truth = method_figures(kind, order, "chirp", n, dtype)
        ridge, ridge_raw = sq.ridge_error_octaves(power, centre, truth, cols), sq.ridge_error_octaves(raw, f, truth, cols)
        near = sq.share_near_truth(power, centre, truth, cols, 1 / (4 * order))
        near_raw = sq.share_near_truth(raw, f, truth, cols, 1 / (4 * order))
        print(f"squeeze wrappers {kind} order {order} n {n} {dtype}: tone {share:.4f} (raw {before:.4f}); chirp ridge {ridge:.4f} "
              f"(raw {ridge_raw:.4f}) octaves, near the truth {near:.3f} (raw {near_raw:.3f})")
        assert share >= 0.95
        assert ridge <= 0.5 * ridge_raw and near >= 1.5 * near_raw


def test_wrappers_take_batches_and_numpy():
    n = 4096
    records = np.stack([sq.tone(n), sq.chirp(n)[0]])
    centre, time_s, batch = styx_cwt.cwt_synchrosqueezed_pow2(3, records, sq.FS, bins_per_band=2, power_floor=1e-6)
    assert isinstance(batch, np.ndarray) and batch.dtype == np.complex128 and batch.shape == (2, len(centre), n)
    _, _, one = styx_cwt.cwt_synchrosqueezed_pow2(3, records[1], sq.FS, bins_per_band=2, power_floor=1e-6)
    assert one.shape == (len(centre), n) and np.array_equal(one, batch[1])
    _, _, stx = styx_stx.stx_synchrosqueezed_pow2(3, records.astype(np.float32), sq.FS)
    assert stx.dtype == np.complex128 and stx.shape == (2, len(centre) // 2, n)  # (float32 records: widened on the way out)


# ---- stream order ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ssc.TABLE.ids())
def test_ordered_behind_a_delayed_producer(cid):
    assert ssc.TABLE.by_id(cid).asynchronous
    so.ordered_behind_producer(ssc.TABLE, cid)


def teardown_module(module):
    so.clear_cases()
