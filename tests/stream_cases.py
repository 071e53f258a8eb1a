"""Case table of the stream-order tests (a plain helper module: imports on the CPU, builds its closures on the GPU).

One case per C-ABI function of include/qi_tfr.h that takes a `qi_stream`, one per path where a function has several.  A
case names the functions it reaches (`functions`: tests/test_stream_cases_cpu.py holds the table against the header) and
builds, on the device, a closure `op(x) -> tuple of device tensors` together with two record sets A and B of one shape,
both finite and legal for the op: the harness (tests/stream_order.py, for tests/test_gpu_streams.py) runs `op` on a buffer
that a delayed producer turns from A into B and compares with the serial result on B.  The table is a stream_table.Table.  The closures go through the Python call path of the other GPU tests:
TfrPlan methods, the engine.* record ops, the public helpers of tfr_info / sampling, and `_lib.call` for the plan-less
short-time family (whose public wrappers upload a window first, a host synchronisation of their own).  Buffers a closure
owns are filled with FILL on the current stream before the call, so an output that is read before the library's own work
has been ordered behind the caller's stream shows as a mismatch.

`asynchronous` is True wherever the header or the docstring promises no host synchronisation; every False carries its
reason.  For the ops without a record input the "records" are what the op reads from the device: timestamp rows (synth,
doppler), atom positions (qi_gabor_atoms_at) or the parameter rows themselves (qi_gabor_atoms, which waits anyway).
"""
import collections
import functools
import os

import numpy as np

from stream_table import ROOT, Built, Table

GOLDEN = os.path.join(ROOT, "tests", "golden")
FS = 1000.0
ORDER = 3
FILL = 0.3125  # finite, exactly representable, and no result of any case

# a plan case's `engine` is a key of ENGINES, PASS2_ENGINE's or the name of a plan of the case's own
TABLE = Table("qi_tfr.h")  # power "any": one output that differs between A and B gives a case power
_case = TABLE.case


def noise(seed, shape, dtype, offset=0.75):
    """Seeded normal records with a non-zero mean."""
    rng = np.random.default_rng([20251019, *(int(v) for v in np.atleast_1d(seed))])
    return (rng.standard_normal(shape) + offset).astype(dtype)


def record_pair(shape, dtype, salt):
    salt = tuple(np.atleast_1d(salt))
    return noise(salt + (1,), shape, dtype), noise(salt + (2,), shape, dtype)


def sorted_rows(records, n, salt):
    """Two sets of jittered, strictly increasing float64 timestamp rows [records, n] at a mean rate of FS."""
    out = []
    for k in (1, 2):
        rng = np.random.default_rng([20251019, 77, salt, k])
        steps = (1.0 + 0.3 * rng.uniform(-1.0, 1.0, (records, n))) / FS
        out.append(np.ascontiguousarray(np.cumsum(steps, axis=1)))
    return tuple(out)


def strip_segments(rows, windows, factor):
    """S of launch_strip (qi_pool.hip): the partial sums per row that k_strip_fold folds when S > 1."""
    gmin = 256 if factor < 64 else (4 if factor <= 1024 else 1)
    groups = max(gmin, -(-(rows * windows) // 4096))
    return -(-windows // groups)


# ---- plans, one per engine, shared by the cases and closed by close_plans() -------------------------------------------------
STYX, ATOMS, STX = 0, 1, 2
ENGINES = collections.OrderedDict([
    # key -> (dtype, n, what the build asserts of the styx and Stockwell tables)
    ("f32_n16384", ("float32", 1 << 14, "native")),
    ("f64_n32768", ("float64", 1 << 15, "side")),
    ("f32_n2048", ("float32", 1 << 11, "small")),
    ("f64_n2048", ("float64", 1 << 11, "small")),
    ("f32_n3000", ("float32", 3000, "hipfft")),
])
# The two-pass kernels run 2^20- and 2^21-point transforms only, and no constant-Q table has a band for them (at 2^14 and
# at 2^19 the order-3 plans report none): they get test_gpu_tables' one-band table at 2^20 samples, an atom cut by the record
# with no block band beside it (band_tables.single_band("split")) -- every output for one record, the band form for 1 and 8.
PASS2_ENGINE = ("f32_n1048576_one_band", ("float32", 1 << 20, "pass2"))
PASS2_FORMS = ((True, 1), (False, 1), (False, 8))  # (every output?, records)
RECORD_COUNTS = (1, 8)
_PLANS = {}


def _engine(key):
    return PASS2_ENGINE[1] if key == PASS2_ENGINE[0] else ENGINES[key]


def atom_tables(n, order):
    """(f_hz, (p_re, p_im, omega, amp)) of cwt_chirp_from_sig's band table, chirped (index_shift 1)."""
    from quantum_inferno_amd import cwt_atoms, scales_dyadic

    _, f_min = cwt_atoms.chirp_scales_from_duration(order, n / FS, 1.0)
    o, _, _, _, f_desc, _, _ = cwt_atoms.chirp_frequency_bands(order, f_min, FS, FS / 2.0, 1.0)
    f = np.flip(f_desc)
    return f, cwt_atoms._atom_tables(o, f, FS, 1.0, scales_dyadic.Slice.G2, "norm")


def _routes(plan, which, records):
    return [plan.band_route(which, j, records) for j in range(len(plan.freq[which]))]


def side_stream_runs(plan, which, records):
    """launch_block<double> forks to the plan's side stream when the table has split bands (their two-piece blocks around
    the middle of the record) beside band items of the block engine (qi_block.hip: `beside`)."""
    from quantum_inferno_amd import _lib

    routes = _routes(plan, which, records)
    return (any(st == "zoom" and fl & _lib.ROUTE_SPLIT for st, _, _, fl in routes) and any(st == "block" for st, _, _, _ in routes))


def engine_plan(key):
    """(plan, note) of ENGINES[key] with the styx bank, the atoms bank and the Stockwell table set, and the engine the key
    names asserted from the plan's own queries."""
    if key in _PLANS:
        return _PLANS[key]
    import torch

    from quantum_inferno_amd import _lib, engine, scales_dyadic

    dtype, n, expect = _engine(key)
    tdt = torch.float64 if dtype == "float64" else torch.float32
    if expect == "pass2":
        import band_tables as bt

        table = bt.single_band("split", n)
        plan = engine.TfrPlan(n, tdt, None, engine.TfrPlan.workspace_for(n, 1, tdt, max(RECORD_COUNTS)))
        plan.set_gabor_bank(STYX, np.arange(1, dtype=np.float64), table["p_re"], table["p_im"], table["omega"], table["amp"])
        route = plan.band_route(STYX, 0)
        note = f"{key}: one band, route {route}"
        assert os.environ.get("QI_FORCE_HIPFFT") or route[0] == "pass2", note
        _PLANS[key] = (plan, note)
        return _PLANS[key]
    orders = (ORDER, 6, 12, 1) if expect == "side" else (ORDER,)
    note = None
    for order in orders:
        f_atoms, tabs = atom_tables(n, order)
        nb = max(len(scales_dyadic.log_frequency_hz_from_fft_points(FS, n, order)), len(f_atoms))
        plan = engine.TfrPlan(n, tdt, None, engine.TfrPlan.workspace_for(n, nb, tdt, max(RECORD_COUNTS)))
        plan.set_styx_bank(order, FS)
        plan.set_stx_bands(order, FS)
        plan.set_gabor_bank(ATOMS, f_atoms, *tabs)
        stages = {s: plan.stage_bands(s) for s in ("zoom", "block", "pass2", "small", "inverse")}
        note = f"{key}: order {order}, bands {[len(plan.freq.get(w, ())) for w in (STYX, ATOMS, STX)]}, stage bands {stages}"
        if expect != "side":
            break
        side = {(w, r): side_stream_runs(plan, w, r) for w in (STYX, STX) for r in RECORD_COUNTS}
        note += f", side stream {side}"
        if all(side[(STYX, r)] for r in RECORD_COUNTS):
            break
        plan.close()
        plan = None
    assert plan is not None, f"no order of {orders} gives a float64 table with split bands beside block bands: {note}"
    if not os.environ.get("QI_FORCE_HIPFFT"):
        for which in (STYX, STX):
            nbw = len(plan.freq[which])
            if expect in ("native", "side"):
                assert stages["inverse"][which] == 0 and stages["zoom"][which] > 0 and stages["block"][which] > 0, note
                assert stages["zoom"][which] + stages["block"][which] + stages["pass2"][which] == nbw, note
            elif expect == "small":
                assert stages["small"][which] == nbw, note
            else:
                assert stages["inverse"][which] == nbw, note
    _PLANS[key] = (plan, note)
    return _PLANS[key]


def close_plans():
    while _PLANS:
        _, (plan, _) = _PLANS.popitem()
        plan.close()


def _result_buffers(plan, which, n_ch, full):
    """A TfrResult whose buffers hold FILL (written on the current stream): every output (`full`) or the band form."""
    import torch

    from quantum_inferno_amd import engine

    nb = len(plan.freq[which])
    res = engine.TfrResult(frequency_hz=plan.freq[which])
    if full:
        res.coef = torch.full((n_ch, nb, plan.n), FILL, dtype=engine._complex_of(plan.rdtype), device=plan.device)
        res.bits = torch.full((n_ch, nb, plan.n), FILL, dtype=plan.rdtype, device=plan.device)
    res.reduced, res.power_band, res.power_time, res.stats = engine.reduced_views(n_ch, nb, plan.n, plan.rdtype, plan.device,
                                                                                 True if full else "band")
    for t in (res.power_band, res.power_time, res.stats):
        if t is not None:
            t.fill_(FILL)
    return res


def _tensors(*results):
    return tuple(t for r in results for t in (r.coef, r.bits, r.power_band, r.power_time, r.stats) if t is not None)


TRANSFORMS = collections.OrderedDict([("cwt_styx", ("qi_cwt",)), ("cwt_atoms", ("qi_cwt",)), ("stx", ("qi_stx",)),
                                      ("cwt_stx", ("qi_cwt_stx",))])


def _build_transform(key, transform, full, records):
    plan, note = engine_plan(key)
    dtype, n, _ = _engine(key)
    a, b = record_pair((records, n), dtype, (1, n, dtype == "float64", records))
    kw = dict(coef=full, bits=full, reductions=True if full else "band")

    def op(x):
        if transform == "cwt_stx":
            out = (_result_buffers(plan, STYX, records, full), _result_buffers(plan, STX, records, full))
            return _tensors(*plan.cwt_stx(x, out=out, **kw))
        which, fn = {"cwt_styx": (STYX, plan.cwt), "cwt_atoms": (ATOMS, plan.cwt_atoms), "stx": (STX, plan.stx)}[transform]
        return _tensors(fn(x, out=_result_buffers(plan, which, records, full), **kw))

    return Built(op, a, b, note)


for _key in ENGINES:
    for _transform, _functions in TRANSFORMS.items():
        for _full in (True, False):
            for _records in RECORD_COUNTS:
                _case(f"{_transform}-{_key}-{'all' if _full else 'band'}-r{_records}", _functions,
                      functools.partial(_build_transform, _key, _transform, _full, _records), engine=_key)


for _full, _records in PASS2_FORMS:
    _case(f"cwt_styx-{PASS2_ENGINE[0]}-{'all' if _full else 'band'}-r{_records}", ("qi_cwt",),
          functools.partial(_build_transform, PASS2_ENGINE[0], "cwt_styx", _full, _records), engine=PASS2_ENGINE[0])


def _build_pooled(key, strip):
    import torch  # noqa: F401

    plan, note = engine_plan(key)
    dtype, n, _ = ENGINES[key]
    records = 2
    a, b = record_pair((records, n), dtype, (2, int(strip)))
    if not strip:
        return Built(lambda x: (plan.pooled(STYX, x, 24, "average"),), a, b, note)
    factor, first, windows = 2, 5, 1000
    segments = strip_segments(records * len(plan.freq[STYX]), windows, factor)
    assert segments > 1, (segments, len(plan.freq[STYX]))

    def op(x):
        strips, band, stats = plan.pooled_strip(STYX, x, factor, first, windows, ("average", "max"), power_scale=2.0)
        return strips["average"], strips["max"], band, stats

    return Built(op, a, b, note + f"; strip partials per row S = {segments}")


_case("pooled-average-f32_n2048", ("qi_cwt", "qi_pool_panel"), functools.partial(_build_pooled, "f32_n2048", False), engine="f32_n2048")
_case("pooled_strip-f32_n2048", ("qi_cwt", "qi_pool_strip", "qi_pool_strip_stats"), functools.partial(_build_pooled, "f32_n2048", True),
      engine="f32_n2048")


def _build_set_bank():
    import torch

    from quantum_inferno_amd import engine, scales_dyadic

    n = 1 << 11
    nb = len(scales_dyadic.log_frequency_hz_from_fft_points(FS, n, ORDER))
    plan = engine.TfrPlan(n, torch.float32, None, engine.TfrPlan.workspace_for(n, nb, torch.float32, 1))
    _PLANS["set_bank"] = (plan, "set_bank")
    a, b = record_pair((1, n), "float32", 3)

    def op(x):
        plan.set_styx_bank(ORDER, FS)  # on the current stream, then the transform that reads the new bank
        return _tensors(plan.cwt(x, coef=True, reductions=True))

    return Built(op, a, b, "")


_case("set_gabor_bank-then-cwt", ("qi_plan_set_gabor_bank", "qi_cwt"), _build_set_bank, asynchronous=False,
      reason="qi_plan_set_gabor_bank uploads the tables and ends with hipStreamSynchronize(st) (qi_api.hip: build_gabor_bank)",
      engine="set_bank")


# ---- the short-time family: _lib calls, one fused and one hipFFT shape --------------------------------------------------------
# (seg, hop, nfft, n): stft_cases' seg 256 at half overlap (fused) and its "seg200_nfft300" row (not a power of two: hipFFT)
STFT_SHAPES = collections.OrderedDict([("fused", (256, 128, 256, 3 * 256 + 1)), ("hipfft", (200, 100, 300, 601))])
SLIDING_SEGS = collections.OrderedDict([("fused", 256), ("hipfft", 24)])  # nfft 256; nfft 32: below the fused shapes
CHANNELS = 3


def _gpu():
    import torch

    from quantum_inferno_amd import _lib

    lib = _lib.require_gpu()
    return torch, _lib, lib, torch.device("cuda", torch.cuda.current_device())


def _full(torch, shape, dtype, dev):
    return torch.full(tuple(shape), FILL, dtype=dtype, device=dev)


def _scratch(torch, nbytes, dev):
    assert nbytes >= 0, nbytes
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=dev)


def _stft_window(torch, seg, dev):
    from quantum_inferno_amd import styx_fft

    win = styx_fft.tukey_window_periodic(seg, 0.25).astype(np.float32)
    return torch.from_numpy(win).to(dev), float(1.0 / np.sum(win.astype(np.float64)))


def _build_stft(shape, form):
    import ctypes as C

    torch, _lib, lib, dev = _gpu()
    seg, hop, nfft, n = STFT_SHAPES[shape]
    a, b = record_pair((CHANNELS, n), "float32", (4, seg))
    win, scale = _stft_window(torch, seg, dev)
    n_seg, n_f, code = int(lib.qi_stft_segments(n, seg, hop)), nfft // 2 + 1, _lib.QI_F32
    panel = (CHANNELS, n_f, n_seg)

    if form == "stft":
        nbytes = int(lib.qi_stft_scratch_bytes(code, CHANNELS, n, seg, hop, nfft))

        def op(x):
            z, bits, scratch = _full(torch, panel, torch.complex64, dev), _full(torch, panel, torch.float32, dev), _scratch(torch, nbytes, dev)
            _lib.call(lib.qi_stft, dev, code, dev.index, _lib.ptr(x), CHANNELS, n, _lib.ptr(win), seg, hop, nfft, scale, _lib.ptr(z),
                      _lib.ptr(bits), 2.0 ** -52, _lib.ptr(scratch), nbytes)
            return z, bits
    elif form in ("out_reduced", "out_panels"):
        panels = form == "out_panels"
        nbytes = int(lib.qi_stft_out_scratch_bytes(code, CHANNELS, n, seg, hop, nfft, int(panels), int(panels)))

        def op(x):
            z = _full(torch, panel, torch.complex64, dev) if panels else None
            bits = _full(torch, panel, torch.float32, dev) if panels else None
            band, time = _full(torch, (CHANNELS, n_f), torch.float64, dev), _full(torch, (CHANNELS, n_seg), torch.float32, dev)
            stats, scratch = _full(torch, (CHANNELS, 4), torch.float64, dev), _scratch(torch, nbytes, dev)
            desc = _lib.TfrOut(coef=_lib.ptr(z), bits=_lib.ptr(bits), power_band=_lib.ptr(band), power_time=_lib.ptr(time),
                               stats=_lib.ptr(stats), power_scale=2.0, eps=2.0 ** -52)
            _lib.call(lib.qi_stft_out, dev, code, dev.index, _lib.ptr(x), CHANNELS, n, _lib.ptr(win), seg, hop, nfft, scale,
                      C.byref(desc), _lib.ptr(scratch), nbytes)
            return tuple(t for t in (z, bits, band, time, stats) if t is not None)
    elif form == "out_range":
        from quantum_inferno_amd import styx_fft

        plan = styx_fft.StftRangePlan(n, FS, window=styx_fft.tukey_window_periodic(seg, 0.25), overlap_points=seg - hop,
                                      nfft_points=nfft, dtype=torch.float32)
        assert plan.n_seg == n_seg and n_seg % 2 == 0

        def op(x):
            res = plan.segment_range(x, 0, n_seg, 0, pooled=2, pooled_methods=("average", "max"), power_scale=2.0)
            return res.power_band, res.power_time, res.stats, res.pooled["average"], res.pooled["max"]
    else:
        assert form == "welch", form
        nbytes = int(lib.qi_welch_scratch_bytes(code, CHANNELS, n, seg, hop, nfft))

        def op(x):
            pxx, scratch = _full(torch, (CHANNELS, n_f), torch.float32, dev), _scratch(torch, nbytes, dev)
            _lib.call(lib.qi_welch, dev, code, dev.index, _lib.ptr(x), CHANNELS, n, _lib.ptr(win), seg, hop, nfft, scale,
                      _lib.ptr(pxx), _lib.ptr(scratch), nbytes)
            return (pxx,)

    return Built(op, a, b, "")


def _build_sliding(shape, inverse):
    torch, _lib, lib, dev = _gpu()
    from quantum_inferno_amd.utilities import short_time_fft as stf

    seg = SLIDING_SEGS[shape]
    obj = stf.get_stft_object_tukey(FS, 0.25, seg, 3 * seg // 4, "magnitude")
    n = 3 * seg + 1
    n_slices, first, code = obj.p_max(n) - obj.p_min, obj.p_min * obj.hop - obj.m_num_mid, _lib.QI_F32
    nbytes = int(lib.qi_sliding_scratch_bytes(code, CHANNELS, obj.mfft, n_slices))
    panel = (CHANNELS, obj.f_pts, n_slices)
    if not inverse:
        a, b = record_pair((CHANNELS, n), "float32", (5, seg))
        win = torch.from_numpy(obj.win.astype(np.float32)).to(dev)

        def op(x):
            z, mag, scratch = _full(torch, panel, torch.complex64, dev), _full(torch, panel, torch.float32, dev), _scratch(torch, nbytes, dev)
            _lib.call(lib.qi_sliding_stft, dev, code, dev.index, _lib.ptr(x), CHANNELS, n, _lib.ptr(win), obj.m_num, obj.hop, obj.mfft,
                      first, n_slices, 0, 1, obj.m_num_mid, _lib.ptr(z), _lib.ptr(mag), 1, _lib.ptr(scratch), nbytes)
            return z, mag
    else:
        a, b = ((noise((6, seg, k), panel, np.float32) + 1j * noise((7, seg, k), panel, np.float32)).astype(np.complex64) for k in (1, 2))
        dual = torch.from_numpy(obj.dual_win.astype(np.float32)).to(dev)
        k1 = (n_slices - 1) * obj.hop

        def op(x):
            out, scratch = _full(torch, (CHANNELS, k1), torch.float32, dev), _scratch(torch, nbytes, dev)
            _lib.call(lib.qi_sliding_istft, dev, code, dev.index, _lib.ptr(x), CHANNELS, _lib.ptr(dual), obj.m_num, obj.hop, obj.mfft,
                      first, n_slices, obj.m_num_mid, 0, k1, _lib.ptr(out), _lib.ptr(scratch), nbytes)
            return (out,)

    return Built(op, a, b, "")


for _shape in STFT_SHAPES:
    for _form, _fn in (("stft", "qi_stft"), ("out_reduced", "qi_stft_out"), ("out_panels", "qi_stft_out"),
                       ("out_range", "qi_stft_out_range"), ("welch", "qi_welch")):
        _case(f"{_form}-{_shape}", (_fn,), functools.partial(_build_stft, _shape, _form))
    _case(f"sliding_stft-{_shape}", ("qi_sliding_stft",), functools.partial(_build_sliding, _shape, False))
    _case(f"sliding_istft-{_shape}", ("qi_sliding_istft",), functools.partial(_build_sliding, _shape, True))


# ---- plan-less kernels: three records of 5000 samples, panels of 7 bands -------------------------------------------------------
N_OPS, BANDS = 5000, 7


def _build_panel_op(name):
    torch, _lib, lib, dev = _gpu()
    from quantum_inferno_amd import tfr_info
    from quantum_inferno_amd.utilities import sampling

    shape = (CHANNELS, BANDS, N_OPS)
    a, b = (np.abs(noise((8, k), shape, np.float32)) ** 2 + np.float32(0.01) for k in (1, 2))
    code = _lib.QI_F32
    if name == "power_marginals":
        op = lambda x: tuple(tfr_info.power_marginals(x))  # noqa: E731
    elif name == "log2_offset":
        ref = torch.from_numpy(np.array([0.5, -1.25, 3.0])).to(dev)

        def op(x):
            out = _full(torch, shape, torch.float32, dev)
            _lib.call(lib.qi_log2_offset, dev, code, dev.index, _lib.ptr(x), _lib.ptr(out), CHANNELS, BANDS * N_OPS, 2.0 ** -52, _lib.ptr(ref))
            return (out,)
    elif name == "log2_abs":
        op = lambda x: (tfr_info.log2_abs(x),)  # noqa: E731
    elif name == "widen":
        def op(x):
            out = _full(torch, shape, torch.float64, dev)
            _lib.call(lib.qi_widen, dev, dev.index, _lib.ptr(x), _lib.ptr(out), x.numel())
            return (out,)
    elif name == "shannon_panel":
        mult = torch.from_numpy(np.array([1e-4, 2e-4, 5e-5], dtype=np.float32)).to(dev)

        def op(x):
            outs = [_full(torch, shape, torch.float32, dev) for _ in range(4)]
            _lib.call(lib.qi_shannon_panel, dev, code, dev.index, _lib.ptr(x), _lib.ptr(mult), 0, CHANNELS, BANDS, N_OPS,
                      float(BANDS * N_OPS), *[_lib.ptr(o) for o in outs])
            return tuple(outs)
    else:
        assert name == "pool_panel", name
        op = lambda x: (sampling.pool_rows(x, 7, "average"), sampling.pool_rows(x, 100, "median"))  # noqa: E731
    return Built(op, a, b, "")


def _build_row_op(name):
    torch, _lib, lib, dev = _gpu()
    code, shape = _lib.QI_F32, (CHANNELS, N_OPS)
    a, b = record_pair(shape, "float32", 9)
    nbytes = int(lib.qi_shannon_scratch_bytes(code, CHANNELS, N_OPS))
    nf = N_OPS // 2 + 1
    if name == "shannon_1d":
        a, b = (np.abs(m) / np.abs(m).sum(axis=1, keepdims=True) for m in (a, b))

        def op(x):
            outs = [_full(torch, shape, torch.float32, dev) for _ in range(4)]
            _lib.call(lib.qi_shannon_1d, dev, code, dev.index, _lib.ptr(x), CHANNELS, N_OPS, *[_lib.ptr(o) for o in outs])
            return tuple(outs)
    elif name == "shannon_tdr":
        def op(x):
            sig, marginal, scratch = _full(torch, shape, torch.float32, dev), _full(torch, shape, torch.float32, dev), _scratch(torch, nbytes, dev)
            _lib.call(lib.qi_shannon_tdr, dev, code, dev.index, _lib.ptr(x), CHANNELS, N_OPS, _lib.ptr(sig), _lib.ptr(marginal),
                      _lib.ptr(scratch), nbytes)
            return sig, marginal
    else:
        assert name == "shannon_fft", name

        def op(x):
            spec = _full(torch, (CHANNELS, nf), torch.complex64, dev)
            angle, marginal = _full(torch, (CHANNELS, nf), torch.float32, dev), _full(torch, (CHANNELS, nf), torch.float32, dev)
            scratch = _scratch(torch, nbytes, dev)
            _lib.call(lib.qi_shannon_fft, dev, code, dev.index, _lib.ptr(x), CHANNELS, N_OPS, _lib.ptr(spec), _lib.ptr(angle),
                      _lib.ptr(marginal), _lib.ptr(scratch), nbytes)
            return spec, angle, marginal
    return Built(op, a, b, "")


STRIP = dict(records=2, bands=3, stride=2100, first=0, factor=2, windows=1050)  # test_gpu_stream_pool's first case: S = 5


def _build_pool_strip():
    torch, _lib, lib, dev = _gpu()
    rows, stride, first, factor, windows = STRIP["records"] * STRIP["bands"], STRIP["stride"], STRIP["first"], STRIP["factor"], STRIP["windows"]
    segments = strip_segments(rows, windows, factor)
    assert segments > 1, segments
    a, b = ((noise((10, k), (rows, stride), np.float32) + 1j * noise((11, k), (rows, stride), np.float32)).astype(np.complex64) for k in (1, 2))

    def op(x):
        mean, peak = _full(torch, (rows, windows), torch.float32, dev), _full(torch, (rows, windows), torch.float32, dev)
        sums, stats = _full(torch, (rows, 3), torch.float64, dev), _full(torch, (STRIP["records"], 4), torch.float64, dev)
        _lib.call(lib.qi_pool_strip, dev, _lib.QI_F32, dev.index, _lib.ptr(x), rows, stride, first, factor, windows, 2.0, _lib.ptr(mean),
                  _lib.ptr(peak), windows, _lib.ptr(sums))
        _lib.call(lib.qi_pool_strip_stats, dev, dev.index, _lib.ptr(sums), STRIP["records"], STRIP["bands"], _lib.ptr(stats))
        return mean, peak, sums, stats

    return Built(op, a, b, f"strip partials per row S = {segments}")


ATOM_N, ATOM_BANDS = 1031, 5


def _atom_params(k):
    rng = np.random.default_rng([20251019, 12, k])
    p_re = 0.5 / rng.uniform(8.0, 60.0, ATOM_BANDS) ** 2
    return np.stack([p_re, 0.3 * p_re, rng.uniform(0.1, 3.0, ATOM_BANDS), (2.0 * p_re / np.pi) ** 0.25])


def _build_atoms(at):
    torch, _lib, lib, dev = _gpu()
    from quantum_inferno_amd import engine

    if not at:  # no device input at all: the records are the parameter rows, read back by the closure (the call waits anyway)
        def op(x):
            rows = x.cpu().numpy()
            return (engine.gabor_atoms(ATOM_N, rows[0], rows[1], rows[2], rows[3], device=dev),)

        return Built(op, _atom_params(1), _atom_params(2), "")
    keep = [_lib.darr(row) for row in _atom_params(1)]
    a, b = (np.arange(ATOM_N) - (ATOM_N - 1) / 2.0 + noise((13, k), (ATOM_N,), np.float64, 0.0) * 0.2 for k in (1, 2))

    def op(x):
        out = _full(torch, (ATOM_BANDS, ATOM_N), torch.complex128, dev)
        _lib.call(lib.qi_gabor_atoms_at, dev, dev.index, ATOM_N, ATOM_BANDS, keep[0][1], keep[1][1], keep[2][1], keep[3][1], _lib.ptr(x),
                  _lib.ptr(out))
        return (out,)

    return Built(op, a, b, "")


for _name, _fn in (("power_marginals", "qi_power_marginals"), ("log2_offset", "qi_log2_offset"), ("log2_abs", "qi_log2_abs"),
                   ("widen", "qi_widen"), ("shannon_panel", "qi_shannon_panel"), ("pool_panel", "qi_pool_panel")):
    _case(_name, (_fn,), functools.partial(_build_panel_op, _name))
for _name in ("shannon_1d", "shannon_tdr", "shannon_fft"):
    _case(_name, ("qi_" + _name,), functools.partial(_build_row_op, _name))
_case("pool_strip-with-stats", ("qi_pool_strip", "qi_pool_strip_stats"), _build_pool_strip)
_ATOMS_WAIT = "the parameter tables go to a temporary the call frees: it ends with hipStreamSynchronize(st) (qi_api.hip: atoms_rows)"
_case("gabor_atoms", ("qi_gabor_atoms",), functools.partial(_build_atoms, False), asynchronous=False, reason=_ATOMS_WAIT)
_case("gabor_atoms_at", ("qi_gabor_atoms_at",), functools.partial(_build_atoms, True), asynchronous=False, reason=_ATOMS_WAIT)


# ---- record ops (engine.*): tables and record shapes of the existing case modules -------------------------------------------------
def _golden(name):
    return np.load(os.path.join(GOLDEN, name), allow_pickle=False)


def _build_record_op(name):
    import torch

    from quantum_inferno_amd import engine

    dev = torch.device("cuda", torch.cuda.current_device())
    n = 1031  # filter_cases' and decimate_cases' prime length: every tile ragged
    if name in ("filtfilt_ba", "filtfilt_sos"):
        import filter_cases as fc

        form, coef, zi, edge = fc.tables(_golden("filter.npz"), "lp4" if name == "filtfilt_ba" else "sos3")
        a, b = (fc.noise((14, k), fc.RECORDS, n, "float64") for k in (1, 2))
        return Built(lambda x: (engine.zero_phase_filter(x, form, coef, zi, edge),), a, b, "")
    if name == "decimate":
        import decimate_cases as dc
        import filter_cases as fc

        sos, zi, edge = dc.tables(_golden("decimate.npz"), 5, "float32")
        a, b = (fc.noise((15, k), dc.RECORDS, n, "float32") for k in (1, 2))
        return Built(lambda x: (engine.zero_phase_decimate(x, 5, sos, zi, edge),), a, b, "")
    if name == "find_peaks":
        import peak_cases as pk

        m = 3 * pk.TILE + 17
        a, b = record_pair((pk.RECORDS, m), "float32", 16)

        def op(x):
            positions, values, counts, scaled = engine.find_peaks(x, "sigmax", "below_max", 0.7, want_scaled=True)
            live = torch.arange(positions.shape[1], device=dev)[None, :] < counts[:, None]  # the other columns are not written
            return (torch.where(live, positions, torch.full_like(positions, -1)), torch.where(live, values, torch.zeros_like(values)),
                    counts, scaled)

        return Built(op, a, b, "")
    records, m = 3, 5000
    values = torch.from_numpy(noise(17, (records, m), np.float32)).to(dev)
    shared = torch.from_numpy(sorted_rows(1, m, 18)[0][0]).to(dev)
    rows_a, rows_b = sorted_rows(records, m, 19)
    value_pair = record_pair((records, m), "float32", 20)
    if name == "interp_shared":
        return Built(lambda x: (engine.interp_to_grid(x, shared, 0.01, 0.37 / FS, 9000),), *value_pair, "")
    if name == "interp_rows":
        return Built(lambda x: (engine.interp_to_grid(values, x, 0.01, 0.37 / FS, 9000),), rows_a, rows_b, "")
    if name == "resample_fft":
        a, b = record_pair((records, 1000), "float32", 21)
        return Built(lambda x: (engine.fft_resample(x, 441),), a, b, "")
    if name == "cumtrapz_dx":
        return Built(lambda x: (engine.cumulative_trapezoid(x, dx=1.0 / FS),), *value_pair, "")
    if name == "cumtrapz_rows":
        return Built(lambda x: (engine.cumulative_trapezoid(values, x),), rows_a, rows_b, "")
    if name == "gradient_h":
        return Built(lambda x: (engine.derivative(x, h=1.0 / FS, kind="gradient"),), *value_pair, "")
    if name == "difference_rows":
        return Built(lambda x: (engine.derivative(values, x, kind="difference", fill_at="start"),), rows_a, rows_b, "")
    if name == "synth_tone_tukey":
        import synth_cases as sy

        params = sy.kind_rows("tone", records)
        return Built(lambda x: (engine.synthesize("tone", params, m, ("timestamps", x, 0.5), ("tukey", 0.5), torch.float32),),
                     rows_a, rows_b, "")
    assert name == "doppler", name
    import synth_cases as sy

    params = np.stack([sy.doppler_row(340., 68., speed, sy.SRC0, sy.SRC1, *sy.RCV_MOVING, False) for speed in (0., 6., 12.)])
    return Built(lambda x: engine.doppler(params, m, ("timestamps", x)), rows_a, rows_b, "")


for _name, _fn in (("filtfilt_ba", "qi_filtfilt"), ("filtfilt_sos", "qi_filtfilt"), ("decimate", "qi_decimate"),
                   ("find_peaks", "qi_find_peaks"), ("interp_shared", "qi_interp_grid"), ("interp_rows", "qi_interp_grid"),
                   ("resample_fft", "qi_resample_fft"), ("cumtrapz_dx", "qi_cumtrapz"), ("cumtrapz_rows", "qi_cumtrapz"),
                   ("gradient_h", "qi_derivative"), ("difference_rows", "qi_derivative"), ("synth_tone_tukey", "qi_synth"),
                   ("doppler", "qi_doppler")):
    _case(_name, (_fn,), functools.partial(_build_record_op, _name))

# the plan-less ops that share process-wide state: the hipFFT handles kept per device, the strip partials kept per stream
SHARED_STATE = ("stft-hipfft", "out_panels-hipfft", "resample_fft", "shannon_fft", "sliding_stft-hipfft", "pool_strip-with-stats")
