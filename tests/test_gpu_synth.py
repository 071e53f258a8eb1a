"""Synthetic signals on the GPU.  qi_synth and qi_doppler through ctypes against their NumPy restatements (synth_cases) for every
record length, record count, parameter layout, time axis, stored type and envelope of the matrix, and 65537 records to cross
the grid limit: bit for bit where no library function is involved (the GT pulse, its derivative and integral, the sawtooth from
a given phase, the zeros of every gate), within the project's tolerances of the record's maximum everywhere else.  A record
gives the same bits alone, in row 0 and in row 64 of 65 and on a second call; refused calls write nothing; no records is a
no-op.  The reference-signature wrappers end to end against the reference's recorded results (tests/golden/synth.npz) with the
recorded noise passed in, and the doppler tutorial's six calls at its own sizes.  Every buffer is pre-filled with a sentinel
and carries a guard element.

The GT integral is compared with the restatement that forms tau^3 as the kernel does (synth_cases.cube_ref, the correctly
rounded cube); the reference's np.power is a library call that is up to one unit in the last place off it."""
import numpy as np
import pytest
import scipy.signal
import torch

import synth_cases as sc
from quantum_inferno_amd import _lib, engine
from quantum_inferno_amd.synth import benchmark_signals, blast_gt_pulse, doppler, synthetic_signals

pytestmark = pytest.mark.gpu

GUARD = 1          # elements behind each buffer that the call must leave alone
FILL = 2.0 ** 100  # (a float32 as well; no result comes near it)
MODULES = {"benchmark_signals": benchmark_signals, "synthetic_signals": synthetic_signals, "blast_gt_pulse": blast_gt_pulse,
           "doppler": doppler}


@pytest.fixture(scope="module")
def g(golden):
    return golden("synth.npz")


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def padded(rows, width):
    rows = np.asarray(rows, dtype=np.float64)
    out = np.zeros(rows.shape[:-1] + (width,))
    out[..., :rows.shape[-1]] = rows
    return out


def axis_args(ax, n):
    x = dev(ax["x"])
    return x, dict(axis=ax["axis"], value=float(ax["value"] or 0.0), x=_lib.ptr(x), xstride=n if x is not None and x.dim() == 2 else 0,
                   s0=float(ax["s0"]), s1=float(ax["s1"]))


def synth(kind, params, n, ax, records, dtype="float64", cplx=False, env=sc.ENV_NONE, alpha=0.0, tmin=0.0, tmax=0.0, k0=0, m=0, expect=0,
          override=None):
    """qi_synth -> out [C, n] (complex for cplx) on the host, after checking that every output was written and the guard was
    not.  `expect`: the status the call must return (then -> None); `override`: arguments of the C call to replace."""
    lib = _lib.require_gpu()
    p = dev(padded(params, sc.P))
    d = p.device
    x, a = axis_args(ax, n)
    width = 2 if cplx else 1
    out = torch.full((records * n * width + GUARD,), FILL, dtype=torch.float64 if dtype == "float64" else torch.float32, device=d)
    a.update(dtype=_lib.QI_F64 if dtype == "float64" else _lib.QI_F32, kind=sc.KINDS.index(kind), cplx=int(cplx), params=_lib.ptr(p),
             pstride=sc.P if p.dim() == 2 else 0, env=env, alpha=float(alpha), tmin=float(tmin), tmax=float(tmax), k0=k0, m=m, c=records,
             n=n, out=_lib.ptr(out))
    a.update(override or {})
    with torch.cuda.device(d):
        rc_ = lib.qi_synth(a["dtype"], d.index, a["kind"], a["cplx"], a["params"], a["pstride"], a["axis"], a["value"], a["x"], a["xstride"],
                           a["s0"], a["s1"], a["env"], a["alpha"], a["tmin"], a["tmax"], a["k0"], a["m"], a["c"], a["n"], a["out"],
                           _lib.stream_ptr(d))
    torch.cuda.synchronize(d)
    assert rc_ == expect, (rc_, lib.qi_last_error())
    assert out[-1].item() == FILL, "the guard was written"
    if expect != 0:
        assert (out == FILL).all(), "a refused call wrote"
        return None
    got = out[:-GUARD].view(records, n, width).cpu().numpy()
    assert not (got == FILL).any(), "an output was not written"
    return got[..., 0] + 1j * got[..., 1] if cplx else got[..., 0]


def dopp(params, n, ax, records, inverse, expect=0, override=None):
    """qi_doppler -> (time, range, omega) [C, n] on the host."""
    lib = _lib.require_gpu()
    p = dev(params)
    d = p.device
    x, a = axis_args(ax, n)
    outs = [torch.full((records * n + GUARD,), FILL, dtype=torch.float64, device=d) for _ in range(3)]
    a.update(inverse=int(inverse), params=_lib.ptr(p), pstride=sc.DP if p.dim() == 2 else 0, c=records, n=n, t=_lib.ptr(outs[0]),
             r=_lib.ptr(outs[1]), o=_lib.ptr(outs[2]))
    a.update(override or {})
    with torch.cuda.device(d):
        rc_ = lib.qi_doppler(d.index, a["inverse"], a["params"], a["pstride"], a["axis"], a["value"], a["x"], a["xstride"], a["s0"], a["s1"],
                             a["c"], a["n"], a["t"], a["r"], a["o"], _lib.stream_ptr(d))
    torch.cuda.synchronize(d)
    assert rc_ == expect, (rc_, lib.qi_last_error())
    assert all(o[-1].item() == FILL for o in outs), "a guard was written"
    if expect != 0:
        assert all((o == FILL).all() for o in outs), "a refused call wrote"
        return None
    got = [o[:-GUARD].view(records, n).cpu().numpy() for o in outs]
    assert not any((o == FILL).any() for o in got), "an output was not written"
    return got


def same(where, got, want):
    if not sc.same_bits(got, want):
        with np.errstate(all="ignore"):
            diff = np.nanmax(np.abs(got.astype(np.complex128) - want), initial=0.0) if got.shape == want.shape else np.nan
        print(f"{where}: dtypes {got.dtype} / {want.dtype}, max |difference| {diff:.3e}, "
              f"{int(np.sum(got != want)) if got.shape == want.shape else -1} of {want.size} differ (bit for bit asked)")
    assert sc.same_bits(got, want), where


def close(where, got, want, tol, worst=None):
    """Each record of got [C, n] within tol of the maximum of its record of want; a record of zeros is compared for equality;
    NaN where the restatement has NaN (a logarithm of a negative number), nowhere else."""
    assert got.shape == want.shape, where
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), where
    want0, got0 = np.where(nan, 0.0, want), np.where(nan, 0.0, got)
    scale = np.max(np.abs(want0), axis=-1)
    err = np.max(np.abs(got0 - want0), axis=-1)
    zero = scale == 0
    assert np.all(err[zero] == 0), where
    if worst is not None and np.any(~zero):
        worst[0] = max(worst[0], float(np.max(err[~zero] / scale[~zero])))
    assert np.all(err <= tol * scale), (where, float(np.max(err[~zero] / scale[~zero])) if np.any(~zero) else 0.0)


def zeros_are_plus_zero(where, got, want):
    """Exactly +0.0 wherever the restatement is +0.0, part by part."""
    parts = ((got.real, np.real(want)), (got.imag, np.imag(want))) if np.iscomplexobj(got) else ((got, np.real(want)),)
    for have, wanted in parts:
        z = (wanted == 0) & ~np.signbit(wanted)
        assert np.all(have[z] == 0) and not np.any(np.signbit(have[z])), where


def envelope_of(index, ax, n, t):
    """The envelope of combination `index`: none, a Tukey window or a gate in turn (a gate needs one axis for all records)."""
    which = index % 3
    if which == 1:
        return dict(env=sc.ENV_TUKEY, alpha=(0.25, 1.0, 0.0)[index // 3 % 3]), dict(envelope=sc.ENV_TUKEY, alpha=(0.25, 1.0, 0.0)[index // 3 % 3])
    if which == 2 and t.ndim == 1:
        alpha = (0.05, 0.6, 1.0)[index // 3 % 3]
        k0, m = sc.gate_span_ref(t, 0.0, 1.0)
        return (dict(env=sc.ENV_GATE, alpha=alpha, tmin=0.0, tmax=1.0, k0=k0, m=m),
                dict(envelope=sc.ENV_GATE, alpha=alpha, tmin=0.0, tmax=1.0))
    return {}, {}


@pytest.mark.parametrize("kind", sc.KINDS)
def test_synth_equals_the_restatement(kind):
    exact = kind in sc.EXACT_KINDS
    worst = {"float64": [0.0], "float32": [0.0]}
    index = 0
    for n in sc.LENGTHS:
        for records in sc.RECORDS:
            for name in sc.AXES:
                for per_record in (False, True):
                    index += 1
                    ax = sc.axis_case(name, n, records)
                    rows = sc.kind_rows(kind, records, salt=n)
                    params = rows if per_record else rows[0]
                    t = sc.axis_time(n, ax["axis"], ax["value"], ax["x"], ax["s0"], ax["s1"])
                    call_env, ref_env = envelope_of(index, ax, n, t)
                    want = sc.synth_ref(kind, params, n, ax["axis"], ax["value"], ax["x"], ax["s0"], ax["s1"], records=records,
                                        cube=sc.cube_ref, **ref_env)
                    where = f"{kind} n {n} records {records} {name} rows {per_record} envelope {call_env.get('env', 0)}"
                    cplx = kind == "quantum_chirp" or index % 4 == 0
                    for dtype in ("float64", "float32"):
                        got = synth(kind, params, n, ax, records, dtype, cplx, **call_env)
                        wanted = want if cplx else want.real
                        if dtype == "float32":  # the one rounding of the store (a value below float32's range is stored as 0)
                            wanted = wanted.astype(np.complex64 if np.iscomplexobj(wanted) else np.float32)
                            wanted = wanted.astype(np.complex128 if np.iscomplexobj(wanted) else np.float64)
                        if exact and call_env.get("alpha", 0.0) <= 0:  # (a window with a cosine in it is not bit for bit)
                            same(where + " " + dtype, got, wanted.astype(got.dtype))  # (exact for float32: wanted holds float32 values)
                        else:
                            zeros_are_plus_zero(where, got, wanted)
                            if cplx:
                                stacked_got = np.concatenate([got.real, got.imag], axis=-1).astype(np.float64)
                                stacked_want = np.concatenate([wanted.real, np.imag(wanted) + np.zeros_like(wanted.real)], axis=-1)
                                close(where + " " + dtype, stacked_got, stacked_want, sc.TOL[dtype], worst[dtype])
                            else:
                                close(where + " " + dtype, got.astype(np.float64), wanted, sc.TOL[dtype], worst[dtype])
    print(f"{kind}: largest deviation from the restatement, of the record's maximum: float64 {worst['float64'][0]:.3e} "
          f"(bound {sc.TOL['float64']:.0e}), float32 {worst['float32'][0]:.3e} (bound {sc.TOL['float32']:.0e})"
          + (" -- bit for bit asked and met" if exact else ""))


def test_sawtooth_from_a_phase_record_and_the_gates_zeros_bit_for_bit():
    for n in sc.LENGTHS:
        for records in (1, 3):
            r = sc.rng(11, n)
            phase = np.cumsum(r.uniform(-0.2, 0.9, (records, n)), axis=1) * 3.0  # rises, falls back, passes zero and negative values
            phase[:, 0] = 0.0
            if n > 2:
                phase[:, 1] = -2 * np.pi
                phase[:, 2] = 4 * np.pi
            ax = dict(axis=sc.AXIS_TIMESTAMPS, value=0.0, x=phase, s0=0.0, s1=0.0)
            for env in ({}, dict(env=sc.ENV_TUKEY, alpha=0.25)):
                want = sc.synth_ref("sawtooth", [1.0], n, sc.AXIS_TIMESTAMPS, x=phase,
                                    **({"envelope": sc.ENV_TUKEY, "alpha": 0.25} if env else {}))
                got = synth("sawtooth", [1.0], n, ax, records, **env)
                if not env:
                    same(f"sawtooth of a phase record n {n} records {records}", got, want)  # fmod, a subtraction and a division
                else:
                    close(f"tapered sawtooth n {n}", got, want, sc.TOL["float64"])
        # every gate's zeros: where the restatement is +0.0 the device is +0.0, for every kind
        ax = sc.axis_case("step", n, 1)
        t = sc.axis_time(n, ax["axis"], ax["value"], ax["x"], ax["s0"], ax["s1"])
        for kind in sc.KINDS:
            for tmin, tmax in ((0.0, 1.0), (0.2, 0.5), (5.0, 6.0)):
                k0, m = sc.gate_span_ref(t, tmin, tmax)
                want = sc.synth_ref(kind, sc.kind_rows(kind, 1)[0], n, ax["axis"], ax["value"], None, ax["s0"], ax["s1"], envelope=sc.ENV_GATE,
                                    alpha=0.3, tmin=tmin, tmax=tmax, cube=sc.cube_ref)
                cplx = kind == "quantum_chirp"
                got = synth(kind, sc.kind_rows(kind, 1)[0], n, ax, 1, "float64", cplx, env=sc.ENV_GATE, alpha=0.3, tmin=tmin, tmax=tmax, k0=k0, m=m)
                outside = np.logical_or(t < tmin, t > tmax)[None, :]
                assert np.all(got[outside] == 0) and not np.any(np.signbit(got[outside].real)), (kind, n, tmin)
                zeros_are_plus_zero(f"{kind} n {n} gate {tmin}", got, want if cplx else want.real)


def test_more_records_than_one_launch_takes():
    records, n = 65537, 3
    r = sc.rng(3)
    x = r.uniform(-0.1, 0.4, (records, n))
    ax = dict(axis=sc.AXIS_TIMESTAMPS, value=0.0, x=x, s0=0.0, s1=0.0)
    quarter = 0.25 / 4.0
    got = synth("gt", [quarter], n, ax, records)
    same("65537 records, timestamps per record", got, sc.kind_ref("gt", [quarter], x.ravel()).reshape(records, n))
    rows = np.tile(np.array([quarter, 0.0]), (records, 1)) * r.uniform(0.5, 2.0, (records, 1))
    ax = dict(axis=sc.AXIS_RATE, value=10.0, x=None, s0=0.05, s1=0.0)
    for dtype in ("float64", "float32"):
        got = synth("gt", rows, n, ax, records, dtype)
        t = sc.axis_time(n, sc.AXIS_RATE, 10.0, s0=0.05)
        for row in (0, 1, 65533, 65534, 65535, 65536):
            same(f"65537 records, a parameter row per record, row {row}", got[row], sc.kind_ref("gt", rows[row], t).astype(got.dtype))
        tau = t[None, :] / rows[:, :1] + 1.0  # every row at once
        away = sc.GT_A - tau
        want = np.where((0.0 <= tau) & (tau <= 1.0), 1.0 - tau, np.where((1.0 < tau) & (tau <= sc.GT_A), (1.0 / 6.0) * (1.0 - tau) * (away * away), 0.0))
        assert sc.same_bits(got, want.astype(got.dtype))
    prow = np.stack([sc.doppler_row(340., 68., 5. + (c % 7), sc.SRC0, sc.SRC1, *sc.RCV_MOVING, False) for c in range(7)])
    params = prow[np.arange(records) % 7]
    ax = dict(axis=sc.AXIS_STEP, value=0.5, x=None, s0=0.0, s1=0.0)
    got = dopp(params, n, ax, records, False)
    t = sc.axis_time(n, sc.AXIS_STEP, 0.5)
    for row in (0, 6, 65534, 65535, 65536):
        for out, want in zip(got, sc.doppler_ref(params[row], t, False)):
            close(f"doppler, 65537 records, row {row}", out[row:row + 1], want[None, :], sc.TOL["float64"])
    assert 65534 % 7 == 0 and all(np.array_equal(out[:3], out[65534:]) for out in got)  # (the rows repeat with period 7)


def test_doppler_equals_the_restatement_and_the_reference(g):
    differ, total, worst = [0, 0, 0], 0, [0.0]
    for n in sc.LENGTHS:
        for records in sc.RECORDS:
            for name in sc.AXES:
                for inverse in (False, True):
                    ax = sc.axis_case(name, n, records)
                    ax = dict(ax, s1=ax["s1"] - 3.0 if inverse else ax["s1"])  # receiver times after the first arrival
                    rows = np.stack([sc.doppler_row(340., 68., 3.0 * (c % 5), sc.SRC0 + 10.0 * c, sc.SRC1, sc.RCV_MOVING[0] - c,
                                                    sc.RCV_MOVING[1], inverse) for c in range(records)])
                    t = sc.axis_time(n, ax["axis"], ax["value"], ax["x"], ax["s0"], ax["s1"])
                    for params in (rows, rows[0]):
                        got = dopp(params, n, ax, records, inverse)
                        for c in range(records):
                            want = sc.doppler_ref(params[c] if params.ndim == 2 else params, t[c] if t.ndim == 2 else t, inverse)
                            for i in range(3):
                                close(f"doppler n {n} records {records} {name} inverse {inverse} output {i}", got[i][c:c + 1], want[i][None, :],
                                      sc.TOL["float64"], worst)
                                differ[i] += int(np.sum(got[i][c] != want[i]))
                            total += n
    print(f"qi_doppler: samples whose bits differ from the restatement: time {differ[0]}, range {differ[1]}, omega {differ[2]} of {total}; "
          f"largest deviation, of the output's maximum, {worst[0]:.3e}")
    # the reference's recorded results through the wrappers
    for key, n, inverse, geometry, times, images in sc.doppler_cases():
        c, vs, vr, s0, s1, r0, r1 = geometry
        for image in images:
            fn = getattr(doppler, ("image_" if image else "") + ("doppler_inverse" if inverse else "doppler_forward"))
            got = fn(times.copy(), c, vs, vr, 3, s0, s1, r0, r1)
            assert len(got) == 3
            for i in range(3):
                want = g[f"doppler_{key}_{int(image)}_{i}"]
                assert isinstance(got[i], np.ndarray) and got[i].dtype == np.float64 and got[i].shape == want.shape
                close(f"{key} image {image} output {i}", got[i][None, :], want[None, :], sc.TOL["float64"])


def test_a_record_gives_the_same_bits_alone_in_any_row_and_on_a_second_call():
    n = 2 * sc.T + 17
    for kind in ("tone", "synth_02", "quantum_chirp", "gt_integral", "sawtooth"):
        for name in ("rate", "rowsE"):
            ax = sc.axis_case(name, n, 65)
            rows = sc.kind_rows(kind, 65, salt=5)
            cplx = kind == "quantum_chirp"
            one_ax = dict(ax, x=ax["x"][40:41]) if name == "rowsE" else ax
            alone = synth(kind, rows[40:41], n, one_ax, 1, "float64", cplx, env=sc.ENV_TUKEY, alpha=0.25)
            for row in (0, 64):
                batch = rows.copy()
                batch[row] = rows[40]
                bax = ax
                if name == "rowsE":
                    x = ax["x"].copy()
                    x[row] = ax["x"][40]
                    bax = dict(ax, x=x)
                got = synth(kind, batch, n, bax, 65, "float64", cplx, env=sc.ENV_TUKEY, alpha=0.25)
                assert sc.same_bits(got[row], alone[0]), (kind, name, row)
                assert sc.same_bits(synth(kind, batch, n, bax, 65, "float64", cplx, env=sc.ENV_TUKEY, alpha=0.25), got), (kind, name, row)
    ax = sc.axis_case("sharedE", n, 65)
    rows = np.stack([sc.doppler_row(340., 68., 2.0 + c % 5, sc.SRC0 + c, sc.SRC1, *sc.RCV_MOVING, False) for c in range(65)])
    alone = dopp(rows[40:41], n, ax, 1, False)
    for row in (0, 64):
        batch = rows.copy()
        batch[row] = rows[40]
        got = dopp(batch, n, ax, 65, False)
        again = dopp(batch, n, ax, 65, False)
        for i in range(3):
            assert sc.same_bits(got[i][row], alone[i][0]) and sc.same_bits(again[i], got[i]), (row, i)


def test_refused_calls_write_nothing():
    lib = _lib.require_gpu()
    n = sc.T + 2
    ax = sc.axis_case("shared0", n, 2)
    rows = sc.kind_rows("tone", 2)
    for bad, word in ((dict(dtype=2), b"dtype"), (dict(kind=12), b"kind"), (dict(axis=3), b"axis"), (dict(env=3), b"envelope"),
                      (dict(cplx=2), b"complex_out"), (dict(pstride=6), b"param_stride"), (dict(xstride=sc.T), b"x_stride"),
                      (dict(x=None), b"x and x_stride"), (dict(axis=0), b"x and x_stride"), (dict(c=-1), b"record count"),
                      (dict(n=0), b"record length"), (dict(env=2, k0=0, m=n + 1), b"gate"), (dict(env=2, k0=n, m=1), b"gate"),
                      (dict(env=2, k0=-1, m=1), b"gate"), (dict(n=1 << 40), b"too large"), (dict(params=None), b"null"),
                      (dict(out=None), b"null")):
        assert synth("tone", rows, n, ax, 2, expect=-1, override=bad) is None
        assert word in lib.qi_last_error(), (bad, lib.qi_last_error())
    drows = np.stack([sc.doppler_row(340., 68., 0., sc.SRC0, sc.SRC1, sc.RCV0, sc.RCV1, False)] * 2)
    for bad, word in ((dict(inverse=2), b"inverse"), (dict(axis=3), b"axis"), (dict(pstride=9), b"param_stride"),
                      (dict(xstride=3), b"x_stride"), (dict(x=None), b"x and x_stride"), (dict(c=-1), b"record count"),
                      (dict(n=0), b"record length"), (dict(params=None), b"null"), (dict(t=None), b"null"), (dict(o=None), b"null")):
        assert dopp(drows, n, ax, 2, False, expect=-1, override=bad) is None
        assert word in lib.qi_last_error(), (bad, lib.qi_last_error())


def test_no_records_is_a_successful_no_op():
    lib = _lib.require_gpu()
    d = torch.device("cuda", torch.cuda.current_device())
    buf = torch.full((64,), FILL, dtype=torch.float64, device=d)
    p = _lib.ptr(buf)
    with torch.cuda.device(d):
        assert lib.qi_synth(_lib.QI_F64, d.index, 0, 0, p, 0, 0, 100.0, None, 0, 0.0, 0.0, 0, 0.0, 0.0, 0.0, 0, 0, 0, 8, p, _lib.stream_ptr(d)) == 0
        assert lib.qi_doppler(d.index, 0, p, 0, 0, 100.0, None, 0, 0.0, 0.0, 0, 8, p, p, p, _lib.stream_ptr(d)) == 0
    torch.cuda.synchronize(d)
    assert (buf == FILL).all()
    assert engine.synthesize("tone", np.zeros((0, 1)), 8).shape == (0, 8)
    assert all(o.shape == (0, 8) for o in engine.doppler(np.zeros((0, 12)), 8, ("rate", 10.0)))


def test_engine_calls_return_device_tensors_of_the_asked_shape_and_type():
    rows = sc.kind_rows("synth_01", 3)
    t = sc.axis_time(2000, sc.AXIS_STEP, 0.0005)
    want = sc.synth_ref("synth_01", rows, 2000, sc.AXIS_STEP, 0.0005, envelope=sc.ENV_GATE, alpha=0.05, tmin=0.0, tmax=1.0)
    got = engine.synthesize("synth_01", rows, 2000, axis=("step", 0.0005), envelope=("gate", 0.0, 1.0, 0.05))
    assert got.is_cuda and got.dtype == torch.float64 and got.shape == (3, 2000)
    close("engine.synthesize, gate", got.cpu().numpy(), want, sc.TOL["float64"])
    got = engine.synthesize("synth_01", rows[0], 2000, axis=("timestamps", t), dtype=torch.float32)
    assert got.dtype == torch.float32 and got.shape == (2000,)
    close("engine.synthesize, float32", got.cpu().numpy()[None, :].astype(np.float64), sc.synth_ref("synth_01", rows[0], 2000, sc.AXIS_STEP, 0.0005),
          sc.TOL["float32"])
    got = engine.synthesize("tone", [0.3], 16, records=5, complex_out=True, dtype=np.float32)
    assert got.dtype == torch.complex64 and got.shape == (5, 16) and float(got.imag.abs().max()) == 0.0
    got = engine.synthesize("gt", [0.0625], 100, axis=("rate", 100.0, 0.495), envelope=("tukey", 0.5))
    want = sc.synth_ref("gt", [0.0625], 100, sc.AXIS_RATE, 100.0, s0=0.495, envelope=sc.ENV_TUKEY, alpha=0.5)[0]
    close("engine.synthesize, tukey", got.cpu().numpy()[None, :], want[None, :], sc.TOL["float64"])
    rows = np.stack([doppler.geometry_row(340., 68., 4., sc.SRC0, sc.SRC1, sc.RCV_MOVING[0] + c, sc.RCV_MOVING[1]) for c in range(4)])
    outs = engine.doppler(rows, 1000, ("rate", 1000.0))
    assert all(o.is_cuda and o.dtype == torch.float64 and o.shape == (4, 1000) for o in outs)
    for c in range(4):
        for o, want in zip(outs, sc.doppler_ref(rows[c], np.arange(1000) / 1000.0, False)):
            close("engine.doppler, a row per receiver", o[c:c + 1].cpu().numpy(), want[None, :], sc.TOL["float64"])


@pytest.mark.parametrize("case", sc.WRAPPER_CASES, ids=[c[0] for c in sc.WRAPPER_CASES])
def test_reference_signature_wrappers_end_to_end(g, case, capsys):
    key, module, name, kwargs = case
    fn = getattr(MODULES[module], name)
    kw = sc.wrapper_kwargs(kwargs)
    if key in sc.NOISY:
        size = g[f"{key}_filtfilt0"].size if f"{key}_filtfilt0" in g.files else g[f"{key}_out0"].size
        kw["noise"] = sc.normal(key, size)
    capsys.readouterr()
    got = fn(**kw)
    printed = capsys.readouterr().out.splitlines()
    got = got if isinstance(got, tuple) else (got,)
    i = 0
    while f"{key}_out{i}" in g.files:
        want = g[f"{key}_out{i}"]
        part = got[i]
        where = f"{key} output {i}"
        if want.ndim == 0:
            assert type(part) is type(want.item()) or np.asarray(part).dtype == want.dtype, where
            assert part == want, where
        else:
            assert isinstance(part, np.ndarray) and part.dtype == want.dtype and part.shape == want.shape, (where, part.dtype, want.dtype)
            if np.iscomplexobj(want):
                close(where, np.concatenate([part.real, part.imag])[None, :], np.concatenate([want.real, want.imag])[None, :], sc.TOL["float64"])
            else:
                close(where, part.astype(np.float64)[None, :], want.astype(np.float64)[None, :], sc.TOL["float64"])
        i += 1
    assert i == len(got)
    assert printed == list(g[f"{key}_printed"]), key  # the reference's printed warnings
    if key == "qchirp_reset":
        assert printed == ["Omega >= 0.8*pi (AA*Nyquist), reset to pi * 2**(-1/N"]
    elif key == "tone_nominal":
        assert len(printed) == 2 and printed[0].startswith("Warning: The time duration 2.0 s") and printed[1].startswith("Warning: fft duration 0.5 s")


def test_gt_family_on_given_times_and_drawn_noise(g):
    t = sc.gt_times()
    for key, name, period in sc.GT_CASES:
        got = getattr(blast_gt_pulse, name)(t.copy(), period)
        want = g[key]
        assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == want.shape
        if sc.GT_KIND[name] in ("gt", "gt_derivative"):
            same(key, got, want)  # the reference's own bits
        else:
            close(key, got[None, :], want[None, :], sc.TOL["float64"])
        if sc.GT_KIND[name] == "gt_integral":
            quarter = period / 4.0
            zero = sc.kind_ref("gt_integral", [quarter, 0.0], t)
            tau = t / quarter + 1.0
            const = zero[np.where((0.0 <= tau) & (tau <= 1.0))[0][-1]] - zero[np.where((1.0 < tau) & (tau <= sc.GT_A))[0][0]]
            same(key + " against the kernel's cube", got, sc.kind_ref("gt_integral", [quarter, const], t, sc.cube_ref))
    # without `noise` the draw is torch.randn's: shape, type, finiteness, and equal generators give equal records
    def gen(device):
        return torch.Generator(device=device).manual_seed(1234)

    calls = ((synthetic_signals.chirp_noise_16bit, dict(duration_points=1000), np.float16, (1000,)),
             (synthetic_signals.sawtooth_noise_16bit, dict(duration_points=1000), np.float16, (1000,)),
             (synthetic_signals.sawtooth_doppler_noise_16bit, dict(phase_radians=sc.doppler_phase(1000)), np.float64, (1000,)),
             (synthetic_signals.white_noise_fbits, dict(sig=np.sin(np.arange(500.0)), std_bit_loss=3.0), np.float64, (500,)),
             (lambda **kw: synthetic_signals.chirp_linear_in_noise(3.0, 500.0, 1.0, 20.0, 100.0, 0.2, 0.3, **kw)[0], dict(), np.float64, (750,)),
             (lambda **kw: blast_gt_pulse.gt_blast_center_fast(**kw)[1], dict(), np.float64, (253,)),
             (lambda **kw: blast_gt_pulse.gt_blast_center_noise(**kw)[1], dict(duration_s=5.0), np.float64, (500,)),
             (blast_gt_pulse.gt_blast_center_noise_uneven, dict(sensor_epoch_s=sc.uneven_epoch(600)), np.float64, (600,)),
             (lambda **kw: benchmark_signals.well_tempered_tone(add_noise_taper_aa=True, time_duration_s=1.28, **kw)[0], dict(), np.float64, (1024,)))
    for fn, kw, dtype, shape in calls:
        drawn = fn(**kw)
        assert isinstance(drawn, np.ndarray) and drawn.dtype == dtype and drawn.shape == shape and np.all(np.isfinite(drawn)), fn
        for device in ("cuda", "cpu"):
            first, second = fn(generator=gen(device), **kw), fn(generator=gen(device), **kw)
            assert sc.same_bits(first, second) and first.shape == shape, (fn, device)
        assert not sc.same_bits(fn(generator=gen("cuda"), **kw), drawn)
    noise = synthetic_signals.white_noise_fbits(np.sin(np.arange(4096.0)), 3.0, generator=gen("cuda"))
    assert abs(np.std(noise) / (np.std(np.sin(np.arange(4096.0))) / 8.0) - 1.0) < 0.1 and abs(np.mean(noise)) < 0.01


def test_the_doppler_tutorial_runs_through_the_package():
    """s00_doppler_20hz: two forward and two inverse doppler calls and two sawtooth_doppler_noise_16bit calls, at its sizes."""
    src0, src1, rcv0, rcv1 = sc.SRC0, sc.SRC1, sc.RCV0, sc.RCV1
    c, vs, vr = 340., 68., 0.
    tau_n = int(doppler.range_scalar(src0, src1) / vs * 1000)
    assert tau_n == 29411
    tau = np.arange(tau_n) / 1000
    fwd = doppler.doppler_forward(tau, c, vs, vr, 3, src0, src1, rcv0, rcv1)
    img = doppler.image_doppler_forward(tau, c, vs, vr, 3, src0, src1, rcv0, rcv1)
    start, end = np.min(fwd[0]), np.max(fwd[0])
    inv_t = start + np.arange(int((end - start) * 1000.)) / 1000.
    inv = doppler.doppler_inverse(inv_t, c, vs, vr, 3, src0, src1, rcv0, rcv1)
    inv_img = doppler.image_doppler_inverse(inv_t, c, vs, vr, 3, src0, src1, rcv0, rcv1)
    for got, times, inverse, image in ((fwd, tau, False, False), (img, tau, False, True), (inv, inv_t, True, False), (inv_img, inv_t, True, True)):
        row = sc.doppler_row(c, vs, vr, src0 * sc.IMAGE if image else src0, src1 * sc.IMAGE if image else src1, rcv0, rcv1, inverse)
        for i, want in enumerate(sc.doppler_ref(row, times, inverse)):
            assert got[i].shape == times.shape and got[i].dtype == np.float64
            close(f"tutorial inverse {inverse} image {image} output {i}", got[i][None, :], want[None, :], sc.TOL["float64"])
    # the source time of the inverse problem recovers the forward problem's: the arrival of tau is heard at fwd[0]
    assert np.max(np.abs(np.interp(fwd[0][100:-100], inv_t, inv[0]) - tau[100:-100])) < 1e-4
    b, a = scipy.signal.butter(4, 0.5, btype="lowpass")
    waves = []
    for key, tau_s, rng_m in (("direct", inv[0], inv[1]), ("image", inv_img[0], inv_img[1])):
        phase = 2. * np.pi * 20. * tau_s
        z = sc.normal("tutorial " + key, len(phase))
        got = synthetic_signals.sawtooth_doppler_noise_16bit(phase, noise=z)
        saw = sc.synth_ref("sawtooth", [1.0], len(phase), sc.AXIS_TIMESTAMPS, x=phase, envelope=sc.ENV_TUKEY, alpha=0.25)[0]
        want = scipy.signal.filtfilt(b, a, saw + np.std(saw) / 2.0 ** 4.0 * z)
        assert got.dtype == np.float64 and got.shape == phase.shape
        close("tutorial sawtooth, " + key, got[None, :], want[None, :], sc.TOL["float64"])
        waves.append(got / rng_m)
    sig_wf = waves[0] + waves[1]
    sig_wf /= np.abs(np.max(sig_wf))
    assert np.all(np.isfinite(sig_wf)) and np.max(sig_wf) == 1.0
