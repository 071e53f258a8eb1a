"""qi_pair_lags on the device (-m gpu) against the float64 NumPy restatement of tests/lag_cases.py fed the same matrices,
upcast: only this call's arithmetic is judged.  cc and peak_value within TOL (1e-4 float32, 1e-10 float64) of the case's
largest |r|; the integer peak index equal (tests/test_lags_cpu.py holds the margins that make it well defined); the
sub-sample offset within twice the first-order propagation of the cc tolerance through the parabola, plus the rounding of
the stored lag in the output's precision; the planted delays within the parabola's own bias.  Then the edges of the window,
the tie, the impulse, exact spectra bit for bit, the contract (position, stack and run independence; NaN containment; NULL
outputs and guard regions) and two end-to-end runs beside the f-k beamformer.

Measured on an MI355X (largest deviation over the parity cases, as a fraction of the case's largest |r|): see the README row.
"""
import functools
import itertools

import numpy as np
import pytest
import torch

import beam_cases as bc
import lag_cases as lc
import window_cases as wc

pytestmark = pytest.mark.gpu

EPS = {"float32": 2.0 ** -24, "float64": 2.0 ** -53}  # half an ulp of 1


def torch_real(dtype):
    return torch.float32 if dtype == "float32" else torch.float64


def run(csd, dtype, **kw):
    """engine.pair_lags on a NumPy stack rounded to `dtype` -> (the rounded stack upcast, peak_lag, peak_value, cc) as float64
    NumPy arrays (the widening is exact)."""
    from quantum_inferno_amd import engine

    rounded = np.ascontiguousarray(csd.astype(lc.complex_of(dtype)))
    lag, value, cc = engine.pair_lags(torch.from_numpy(rounded).cuda(), want_cc=True, **kw)
    assert lag.dtype == value.dtype == cc.dtype == torch_real(dtype)
    return rounded.astype(np.complex128), lag.double().cpu().numpy(), value.double().cpu().numpy(), cc.double().cpu().numpy()


def restate_for(case_kw, upcast):
    return lc.restate(upcast, case_kw["bins"], lc.WEIGHTINGS.index(case_kw["weighting"]), case_kw["halve_interior"], case_kw["normalize"],
                      case_kw["upsample"], case_kw["max_lag"])


def judge(tag, dtype, res, lag, value, cc, upsample):
    """The parity assertions on one call's outputs; returns the measured deviations."""
    tol, scale = lc.TOL[dtype], float(np.abs(res.r).max())
    max_lag = (cc.shape[-1] - 1) // 2
    d_cc, d_value = float(np.abs(cc - res.cc).max()) / scale, float(np.abs(value - res.peak_value).max()) / scale
    index = np.argmax(cc, axis=-1) - max_lag
    offset = lag * upsample - res.index
    # twice the first-order propagation of the cc tolerance, and the rounding of the stored lag (half an ulp, in finer samples)
    bound = 2.0 * tol * scale * res.bound + EPS[dtype] * 2.0 * np.maximum(np.abs(res.peak_lag * upsample), 1.0)
    d_offset = float((np.abs(offset - res.delta) / bound).max())
    print(f"{tag} {dtype}: cc {d_cc:.3g}, peak_value {d_value:.3g} of the largest |r| (bound {tol:g}); offset at {d_offset:.3g} of its bound "
          f"(largest bound {bound.max():.3g} samples)")
    assert d_cc <= tol and d_value <= tol, tag
    assert np.array_equal(index, res.index), tag
    assert d_offset <= 1.0, tag
    return d_cc, d_value, d_offset, bound


@pytest.mark.parametrize("dtype", lc.DTYPES)
@pytest.mark.parametrize("cid", lc.ids())
def test_parity_with_the_restatement(cid, dtype):
    case = lc.by_id(cid)
    kw = lc.call_args(case)
    s, delays = lc.matrices(cid)
    upcast, lag, value, cc = run(s, dtype, **kw)
    n_pair = case.C * (case.C - 1) // 2
    assert lag.shape == value.shape == (case.nstack, n_pair) and cc.shape == (case.nstack, n_pair, 2 * case.max_lag + 1)
    res = lc.restated(cid) if dtype == "float64" else restate_for(kw, upcast)
    _, _, _, bound = judge(cid, dtype, res, lag, value, cc, case.upsample)
    rows, cols = lc.pair_table(case.C)
    planted = delays[:, cols] - delays[:, rows]
    own_bias = np.abs(res.peak_lag * case.upsample - planted)  # the parabola's, as the restatement measures it
    assert (np.abs(lag * case.upsample - planted) <= own_bias + bound).all(), cid


@pytest.mark.parametrize("dtype", lc.DTYPES)
@pytest.mark.parametrize("nfft,max_lag,delay", [(64, 5, -5), (64, 5, 5), (64, 31, 31), (64, 31, -31), (256, 9, 9)])
def test_maximum_on_the_windows_edge_and_across_the_wrap(nfft, max_lag, delay, dtype):
    """The first and the last sample of the window, and lag L / 2 - 1 whose upper neighbour is r[L / 2] = r[-L / 2]: the
    neighbours come from the whole correlation.  (nfft 256: the transform whose first pass is of radix 8.)"""
    kw = dict(bins=None, weighting="phat", halve_interior=False, normalize=True, upsample=1, max_lag=max_lag)
    upcast, lag, value, cc = run(lc.delayed_pair(nfft, delay), dtype, **kw)
    res = restate_for(kw, upcast)
    assert res.index[0, 0] == delay
    judge(f"edge nfft {nfft} delay {delay}", dtype, res, lag, value, cc, 1)
    assert abs(lag[0, 0] - delay) <= 1e-3 and abs(value[0, 0] - 1.0) <= 1e-3


@pytest.mark.parametrize("dtype", lc.DTYPES)
def test_tie_goes_to_the_smaller_lag_and_flat_phat_is_the_unit_impulse(dtype):
    s = np.zeros((1, 33, 2, 2), dtype=np.complex128)
    s[0, 0, 0, 1], s[0, 32, 0, 1] = 5, 3  # r[l] = (5 + 3 (-1)^l) / 64, exactly: every even lag ties
    _, lag, value, cc = run(s, dtype, bins=None, weighting="plain", halve_interior=False, normalize=False, upsample=1, max_lag=5)
    assert cc[0, 0].tolist() == [2 / 64, 8 / 64] * 5 + [2 / 64] and lag[0, 0] == -4.0 and value[0, 0] == 8 / 64
    flat = np.zeros((1, 33, 2, 2), dtype=np.complex128)
    flat[0, :, 0, 1] = 3.0
    _, lag, value, cc = run(flat, dtype, bins=None, weighting="phat", halve_interior=False, normalize=True, upsample=1, max_lag=None)
    want = np.zeros(63)
    want[31] = 1.0
    assert np.array_equal(cc[0, 0], want) and lag[0, 0] == 0.0 and value[0, 0] == 1.0


@pytest.mark.parametrize("dtype", lc.DTYPES)
@pytest.mark.parametrize("nfft,upsample", [(64, 1), (64, 2), (4096, 1), (4096, 2)])
def test_gaussian_integer_spectra_are_exact(nfft, upsample, dtype):
    s = lc.exact_matrices(nfft, upsample)
    for halve in (False, True):
        kw = dict(bins=None, weighting="plain", halve_interior=halve, normalize=False, upsample=upsample, max_lag=None)
        upcast, lag, value, cc = run(s, dtype, **kw)
        assert np.array_equal(upcast, s)
        res = restate_for(kw, upcast)
        assert np.array_equal(res.r, lc.exact_correlation(s, upsample, halve))
        real = np.float32 if dtype == "float32" else np.float64
        assert np.array_equal(cc, res.cc), (nfft, upsample, halve)
        assert np.array_equal(lag, res.peak_lag.astype(real).astype(np.float64)), (nfft, upsample, halve)
        assert np.array_equal(value, res.peak_value.astype(real).astype(np.float64)), (nfft, upsample, halve)


# ---- the contract -----------------------------------------------------------------------------------------------------------------------
BIG_C, BIG_STACKS, BIG_NFFT, BIG_UP, AT = 17, 3, 128, 2, (2, 3, 11)  # the pair (3, 11) of stack 2


@functools.lru_cache(maxsize=None)
def big_stack():
    rng = np.random.default_rng(20260305)
    nf = BIG_NFFT // 2 + 1
    x = rng.standard_normal((BIG_STACKS, 3, BIG_C, nf)) + 1j * rng.standard_normal((BIG_STACKS, 3, BIG_C, nf))
    s = np.einsum("kmif,kmjf->kfij", np.conj(x), x)
    s.setflags(write=False)
    return s


def bits(*arrays):
    return [a.tobytes() for a in arrays]


@pytest.mark.parametrize("dtype", lc.DTYPES)
@pytest.mark.parametrize("weighting,normalize", [("plain", True), ("plain", False), ("phat", True), ("scot", True), ("scot", False)])
def test_a_pair_does_not_depend_on_its_stack_or_the_run(weighting, normalize, dtype):
    s = big_stack()
    k, i, j = AT
    kw = dict(bins=(2, 60), weighting=weighting, halve_interior=True, normalize=normalize, upsample=BIG_UP, max_lag=40)
    _, lag, value, cc = run(s, dtype, **kw)
    _, lag2, value2, cc2 = run(s, dtype, **kw)
    assert bits(lag, value, cc) == bits(lag2, value2, cc2)
    small = s[k][:, [i, j]][:, :, [i, j]][None]
    _, lag1, value1, cc1 = run(small, dtype, **kw)
    p = lc.pair_index(BIG_C, i, j)
    assert bits(lag1[0, 0], value1[0, 0], cc1[0, 0]) == bits(lag[k, p], value[k, p], cc[k, p])
    moved = np.stack([s[k], s[0]])  # the same matrices as stack 0 of two
    _, lag0, value0, cc0 = run(moved, dtype, **kw)
    assert bits(lag0[0], value0[0], cc0[0]) == bits(lag[k], value[k], cc[k]) and bits(lag0[1], cc0[1]) == bits(lag[0], cc[0])


@pytest.mark.parametrize("dtype", lc.DTYPES)
def test_nan_stays_in_its_pair_and_outside_the_band_changes_nothing(dtype):
    s = big_stack()
    kw = dict(bins=(2, 60), weighting="phat", halve_interior=True, normalize=True, upsample=BIG_UP, max_lag=40)
    _, lag, value, cc = run(s, dtype, **kw)
    assert np.isfinite(lag).all() and np.isfinite(value).all() and np.isfinite(cc).all()
    hit = s.copy()
    hit[1, 30, 3, 11] = complex(np.nan, 0.0)
    hit[0, 59, 0, 1] = complex(1.0, np.inf)
    _, lag_h, value_h, cc_h = run(hit, dtype, **kw)
    poisoned = np.zeros(lag.shape, dtype=bool)
    poisoned[1, lc.pair_index(BIG_C, 3, 11)] = poisoned[0, 0] = True
    assert np.isnan(lag_h[poisoned]).all() and np.isnan(value_h[poisoned]).all() and np.isnan(cc_h[poisoned]).all()
    assert bits(lag_h[~poisoned], value_h[~poisoned], cc_h[~poisoned]) == bits(lag[~poisoned], value[~poisoned], cc[~poisoned])
    out = s.copy()
    out[:, :2] = np.nan  # the bins below the band, every entry
    out[:, 60:, 3, 11] = complex(np.inf, np.nan)
    out[:, 10, 11, 3] = np.nan  # below the diagonal: never read
    out[:, 10, 5, 5] = np.nan  # an auto-power PHAT does not read
    _, lag_o, value_o, cc_o = run(out, dtype, **kw)
    assert bits(lag_o, value_o, cc_o) == bits(lag, value, cc)
    # the auto-powers are read by SCOT and by the plain coefficient: record 5's pairs, in every stack, and no others
    for weighting in ("scot", "plain"):
        _, lag_a, _, _ = run(out, dtype, **{**kw, "weighting": weighting})
        with_5 = np.array([5 in pair for pair in zip(*lc.pair_table(BIG_C))])
        assert (np.isnan(lag_a) == with_5[None, :]).all(), weighting


GUARD = 64


@pytest.mark.parametrize("dtype", lc.DTYPES)
def test_null_outputs_and_guard_regions(dtype):
    from quantum_inferno_amd import _lib

    lib = _lib.require_gpu()
    s = big_stack()
    n_pair, max_lag, real = BIG_C * (BIG_C - 1) // 2, 40, torch_real(dtype)
    csd = torch.from_numpy(np.ascontiguousarray(s.astype(lc.complex_of(dtype)))).cuda()
    dev, code = csd.device, _lib.dtype_code(real)
    sizes = (BIG_STACKS * n_pair * (2 * max_lag + 1), BIG_STACKS * n_pair, BIG_STACKS * n_pair)
    full = None
    for wanted in [w for w in itertools.product((True, False), repeat=3) if any(w)]:  # (cc, peak_lag, peak_value); all three first
        bufs = [torch.full((n + GUARD,), -7.0, dtype=real, device=dev) if on else None for n, on in zip(sizes, wanted)]
        _lib.call(lib.qi_pair_lags, dev, code, dev.index, _lib.ptr(csd), BIG_STACKS, BIG_C, BIG_NFFT, 2, 60, 1, 1, 1, BIG_UP, max_lag,
                  _lib.ptr(bufs[0]), _lib.ptr(bufs[1]), _lib.ptr(bufs[2]), None, 0)
        got = [None if b is None else b.cpu().numpy() for b in bufs]
        if full is None:
            full = got
        for k, (g, n) in enumerate(zip(got, sizes)):
            if g is None:
                continue
            assert (g[n:] == -7.0).all(), (wanted, k)
            assert g[:n].tobytes() == full[k][:n].tobytes() and np.isfinite(g[:n]).all() and not (g[:n] == -7.0).all(), (wanted, k)


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
def test_plane_wave_slowness_beside_the_fk_peak():
    """The five-sensor plane wave in noise of tests/beam_cases.py: the slowness fitted to the pair delays lies within one grid
    step of the f-k peak (which is the source's grid point) -- in fact within a hundredth of a step of the source."""
    from quantum_inferno_amd import beamform, styx_fft

    x = bc.pw_records().copy()
    grid = beamform.slowness_grid(bc.PW_MAX_SLOWNESS, bc.PW_GRID_POINTS)
    edges = np.fft.rfftfreq(bc.PW_SEG, 1 / bc.PW_FS)[list(bc.PW_BANDS)]
    _, _, peak_index, _ = beamform.fk_power_pow2(x, bc.PW_FS, bc.PW_POSITIONS_M, grid, bc.PW_SEG, bc.PW_OVERLAP, band_edges_hz=edges)
    assert (peak_index == bc.pw_true_index()).all()
    step = 2 * bc.PW_MAX_SLOWNESS / (bc.PW_GRID_POINTS - 1)
    for weighting in lc.WEIGHTINGS:
        lag_s, value, pairs = styx_fft.pair_lags_pow2(x, bc.PW_FS, 1024, nfft_points=2048, band_hz=(25.0, 225.0), weighting=weighting, upsample=4)
        assert lag_s.shape == value.shape == (10,) and pairs.tolist() == [list(p) for p in zip(*lc.pair_table(5))]
        slowness, rms = beamform.slowness_from_lags(lag_s, bc.PW_POSITIONS_M, weights=value)
        fk = grid[int(peak_index[0])].numpy()
        err = np.abs(slowness.numpy() - fk).max()
        print(f"{weighting}: slowness {slowness.numpy() * 1e3} ms/m, f-k peak {fk * 1e3}, rms residual {float(rms) * 1e6:.2f} us, "
              f"largest closure {float(beamform.lag_closure(lag_s, 5).abs().max()) * 1e6:.2f} us")
        assert err <= step and err <= 0.01 * step, weighting
        assert float(rms) <= 0.1 / bc.PW_FS and float(beamform.lag_closure(lag_s, 5).abs().max()) <= 0.2 / bc.PW_FS
        want_az, want_v = bc.pw_true_azimuth_velocity()
        az, v = beamform.back_azimuth_and_velocity(slowness)
        assert abs(float(az) - want_az) <= 0.1 and abs(float(v) / want_v - 1) <= 1e-3


def test_windowed_delays_follow_the_two_sources():
    """The timeline case of tests/window_cases.py (one source in the first half of the record, another in the second): the
    fitted slowness of the windows wholly in one half lies within one grid step of that half's source."""
    from quantum_inferno_amd import beamform, styx_fft

    x = wc.timeline_records().astype(np.float32)
    lag_s, value, pairs, time_s = styx_fft.pair_lags_pow2(x, bc.PW_FS, wc.TL_SEG, nfft_points=2 * wc.TL_SEG, band_hz=(25.0, 225.0),
                                                          upsample=4, window_segments=wc.TL_WIN, window_hop_segments=wc.TL_HOP)
    assert lag_s.shape == value.shape == (14, 10) and lag_s.dtype == np.float32 and np.allclose(time_s, wc.timeline_times(), rtol=0, atol=1e-12)
    slowness, rms = beamform.slowness_from_lags(lag_s, bc.PW_POSITIONS_M)
    step = 2 * bc.PW_MAX_SLOWNESS / (bc.PW_GRID_POINTS - 1)
    for windows, point in zip((wc.TL_FIRST, wc.TL_SECOND), wc.TL_POINTS):
        err = np.abs(slowness.numpy()[list(windows)] - bc.pw_slowness()[point]).max()
        print(f"windows {list(windows)}: within {err / step:.3g} grid steps of source {point}; rms residual <= {float(rms[list(windows)].max()) * 1e6:.1f} us")
        assert err <= step
