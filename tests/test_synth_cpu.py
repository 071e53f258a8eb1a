"""Synthetic signals without a GPU: the NumPy restatements of qi_synth and qi_doppler (synth_cases) against the reference's
recorded arrays (tests/golden/synth.npz, tools/gen_golden_synth.py) bit for bit -- the waveforms it hands to decimate and to
filtfilt, the GT family, all three doppler outputs; host NumPy runs one math library, so a difference is a mistake in the order
of operations.  The C ABI declares and exports the two entry points and their constants, the argument checks answer through
ctypes without a device, the host-only functions equal the reference, the wrappers raise their errors before the device is
needed, and the package's own seeded generator is unchanged."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import synth_cases as sc
from quantum_inferno_amd import _lib, engine
from quantum_inferno_amd.synth import benchmark_signals, blast_gt_pulse, doppler, synthetic_signals
from quantum_inferno_amd.utilities import window

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODULES = {"benchmark_signals": benchmark_signals, "synthetic_signals": synthetic_signals, "blast_gt_pulse": blast_gt_pulse,
           "doppler": doppler}


@pytest.fixture(scope="module")
def g(golden):
    return golden("synth.npz")


def test_restatements_equal_the_reference_bit_for_bit(g):
    assert sc.restatement_failures(g) == []
    # the fixture holds what the tests below and on the GPU rely on
    for key, _, name, _ in sc.WRAPPER_CASES:
        assert f"{key}_out0" in g.files, key
        if name.startswith(("quantum", "synth_0")):
            assert f"{key}_decimate0" in g.files, key
    assert g["chirp16_default_out0"].dtype == np.float16 and g["saw16_default_out0"].dtype == np.float16
    assert g["saw_doppler_out0"].dtype == np.float64  # the reference drops its cast
    assert sc.same_bits(g["tone_noise_out0"], g["tone_noise_filtfilt0"])  # ... and returns the record it did not filter
    assert g["qchirp_default_out0"].dtype == np.complex128
    assert list(g["qchirp_reset_printed"]) == ["Omega >= 0.8*pi (AA*Nyquist), reset to pi * 2**(-1/N"]
    assert len(g["tone_nominal_printed"]) == 2 and len(g["tone_default_printed"]) == 0


def test_the_window_and_the_gate_are_scipys():
    for m, alpha in ((1, 0.5), (2, 0.5), (3, 0.25), (7, 1.0), (8, 1.5), (257, 0.05), (1000, 0.25), (1024, 0.1), (64, 0.0), (5, -1.0),
                     (2000, 0.05), (2, 1.0), (33, 0.999)):
        assert sc.same_bits(sc.tukey_ref(m, alpha), window.get_tukey(np.zeros(m), alpha)), (m, alpha)
    # the bisection of the wrappers finds the samples NumPy's comparison includes, with the kernel's own t(k)
    for n, axis, value in ((2000, "step", 0.0005), (2001, "rate", 1777.0), (3, "step", 0.4), (1, "rate", 10.0), (4096, "step", 1 / 4096)):
        for s0 in (0.0, 0.25):
            for tmin, tmax in ((0.0, 1.0), (0.5, 1.0), (0.0, 0.5), (0.25, 0.4), (2.0, 3.0), (-3.0, -2.0), (0.7, 0.6)):
                t = sc.axis_time(n, sc.AXIS_STEP if axis == "step" else sc.AXIS_RATE, value, s0=s0)
                assert engine.gate_span(n, (axis, value, s0), tmin, tmax) == sc.gate_span_ref(t, tmin, tmax), (n, axis, s0, tmin, tmax)
                assert engine.gate_span(n, ("timestamps", t), tmin, tmax) == sc.gate_span_ref(t, tmin, tmax)
                assert all(engine.synth_time(k, (axis, value, s0)) == t[k] for k in (0, n // 2, n - 1))


def test_the_cube_of_the_integral_is_the_correctly_rounded_one():
    """The kernel forms tau^3 of the GT integral from exact products (cube(), restated as synth_cases.cube_ref): the correctly
    rounded cube.  The reference calls np.power(tau, 3), a library function: glibc's rounds correctly on these inputs, NumPy's
    AVX-512 loop is one unit in the last place off on some of them -- never more."""
    taus = [sc.gt_times() / (period / 4.0) + 1.0 for _, name, period in sc.GT_CASES if name.endswith("integral_period_center")]
    taus.append(sc.axis_time(2 * sc.T + 17, sc.AXIS_RATE, (2 * sc.T + 16) / 1.7, s0=0.3) / (0.25 / 4.0) + 1.0)
    for tau in taus:
        tau = tau[(1.0 < tau) & (tau <= sc.GT_A)]
        assert len(tau) > 100
        exact = np.array([float(Fraction(float(v)) ** 3) for v in tau])  # (float() of a Fraction rounds correctly)
        assert sc.same_bits(sc.cube_ref(tau), exact)
        library = np.power(tau, 3)
        print(f"np.power(tau, 3) differs from the correctly rounded cube in {int(np.sum(library != exact))} of {len(tau)} samples")
        assert np.all(np.abs(library - exact) <= np.spacing(exact))


def test_header_library_and_binding_agree():
    header = open(os.path.join(ROOT, "include", "qi_tfr.h")).read()
    lib = _lib.load()
    for name in ("qi_synth", "qi_doppler"):
        assert re.search(rf"\b{name}\s*\(", header), f"{name} is not declared"
        assert hasattr(lib, name) and name in _lib.PROTOTYPES
    for macro, ours, cases in (("QI_SYNTH_TILE", _lib.SYNTH_TILE, sc.T), ("QI_SYNTH_PARAMS", _lib.SYNTH_PARAMS, sc.P),
                               ("QI_DOPPLER_PARAMS", _lib.DOPPLER_PARAMS, sc.DP)):
        assert int(re.search(rf"#define\s+{macro}\s+(\d+)", header).group(1)) == ours == cases, macro
    kinds = re.search(r"typedef enum \{([^}]*)\} qi_synth_kind;", header).group(1)
    names = [(m.group(1), int(m.group(2))) for m in re.finditer(r"QI_SYNTH_(\w+)\s*=\s*(\d+)", kinds)]
    assert [v for _, v in names] == list(range(len(names))) and names[-1] == ("KINDS", len(_lib.SYNTH_KINDS))
    assert _lib.SYNTH_KINDS == sc.KINDS and engine.SYNTH_KINDS == {k: i for i, k in enumerate(sc.KINDS)}
    assert re.search(r"QI_AXIS_RATE\s*=\s*0\s*,\s*QI_AXIS_STEP\s*=\s*1\s*,\s*QI_AXIS_TIMESTAMPS\s*=\s*2", header)
    assert re.search(r"QI_ENVELOPE_NONE\s*=\s*0\s*,\s*QI_ENVELOPE_TUKEY\s*=\s*1\s*,\s*QI_ENVELOPE_GATE\s*=\s*2", header)
    assert (_lib.QI_AXIS_RATE, _lib.QI_AXIS_STEP, _lib.QI_AXIS_TIMESTAMPS) == (sc.AXIS_RATE, sc.AXIS_STEP, sc.AXIS_TIMESTAMPS) == (0, 1, 2)
    assert (_lib.QI_ENVELOPE_NONE, _lib.QI_ENVELOPE_TUKEY, _lib.QI_ENVELOPE_GATE) == (sc.ENV_NONE, sc.ENV_TUKEY, sc.ENV_GATE) == (0, 1, 2)
    assert lib.qi_abi_version() == 1


def test_refused_arguments():
    lib = _lib.load()
    buf = np.full(64, 7.0)
    p = buf.ctypes.data_as(C.c_void_p)

    def synth(dtype=_lib.QI_F64, kind=0, cplx=0, params=p, pstride=0, axis=0, value=100.0, x=None, xstride=0, env=0, k0=0, m=0, c=1, n=8,
              out=p):
        return lib.qi_synth(dtype, 0, kind, cplx, params, pstride, axis, value, x, xstride, 0.0, 0.0, env, 0.5, 0.0, 1.0, k0, m, c, n, out, None)

    for bad, word in ((dict(dtype=2), b"dtype"), (dict(kind=12), b"kind"), (dict(kind=-1), b"kind"), (dict(axis=3), b"axis"),
                      (dict(axis=-1), b"axis"), (dict(env=3), b"envelope"), (dict(env=-1), b"envelope"), (dict(cplx=2), b"complex_out"),
                      (dict(pstride=8), b"param_stride"), (dict(pstride=-12), b"param_stride"), (dict(axis=2, x=p, xstride=4), b"x_stride"),
                      (dict(xstride=8), b"x and x_stride"), (dict(axis=2), b"x and x_stride"), (dict(x=p), b"x and x_stride"),
                      (dict(c=-1), b"record count"), (dict(n=0), b"record length"), (dict(n=-3), b"record length"),
                      (dict(value=0.0), b"rate"), (dict(env=2, k0=-1, m=2), b"gate"), (dict(env=2, k0=0, m=9), b"gate"),
                      (dict(env=2, k0=9, m=0), b"gate"), (dict(env=2, k0=4, m=5), b"gate"), (dict(env=2, k0=0, m=-1), b"gate"),
                      (dict(n=1 << 40), b"too large"), (dict(c=1 << 31), b"too large"), (dict(params=None), b"null"),
                      (dict(out=None), b"null")):
        assert synth(**bad) == -1 and word in lib.qi_last_error(), (bad, lib.qi_last_error())
    assert synth(c=0) == 0 and synth(c=0, params=None, out=None) == 0  # no records: a successful no-op

    def dopp(inverse=0, params=p, pstride=0, axis=0, value=100.0, x=None, xstride=0, c=1, n=8, t=p, r=p, o=p):
        return lib.qi_doppler(0, inverse, params, pstride, axis, value, x, xstride, 0.0, 0.0, c, n, t, r, o, None)

    for bad, word in ((dict(inverse=2), b"inverse"), (dict(axis=3), b"axis"), (dict(pstride=9), b"param_stride"),
                      (dict(axis=2, x=p, xstride=4), b"x_stride"), (dict(axis=2), b"x and x_stride"), (dict(c=-1), b"record count"),
                      (dict(n=0), b"record length"), (dict(value=0.0), b"rate"), (dict(n=1 << 40), b"too large"),
                      (dict(params=None), b"null"), (dict(t=None), b"null"), (dict(r=None), b"null"), (dict(o=None), b"null")):
        assert dopp(**bad) == -1 and word in lib.qi_last_error(), (bad, lib.qi_last_error())
    assert dopp(c=0) == 0 and dopp(c=0, params=None, t=None, r=None, o=None) == 0
    assert (buf == 7.0).all()


def test_host_only_functions_equal_the_reference(g):
    for key, module, name, args in sc.HOST_CASES:
        got = getattr(MODULES[module], name)(*[a.copy() if isinstance(a, np.ndarray) else a for a in args])
        for i, part in enumerate(got if isinstance(got, tuple) else (got,)):
            assert sc.same_bits(np.asarray(part), g[f"host_{key}_{i}"]), (key, i)
    # signal_gate on the host: in place, the reference's zeros and window
    t = benchmark_signals.oversample_time(1.0, 1e-3, 2)
    wf = np.cos(40.0 * t)
    want = sc.synth_ref("tone", [40.0], len(t), sc.AXIS_STEP, 0.0005, envelope=sc.ENV_GATE, alpha=0.3, tmin=0.1, tmax=0.8)[0]
    assert benchmark_signals.signal_gate(wf, t, 0.1, 0.8, 0.3) is wf and sc.same_bits(wf, want)
    assert (benchmark_signals.DEFAULT_TIME_SAMPLE_INTERVAL, benchmark_signals.DEFAULT_TIME_DURATION,
            benchmark_signals.DEFAULT_OVERSAMPLE_SCALE) == (1e-3, 1.0, 2)
    # a geometry row is built by the reference's expressions (the restatement's row equals the fixture's results through it)
    for key, n, inverse, geometry, times, images in sc.doppler_cases():
        c, vs, vr, s0, s1, r0, r1 = geometry
        assert sc.same_bits(doppler.geometry_row(c, vs, vr, s0, s1, r0, r1, inverse), sc.doppler_row(c, vs, vr, s0, s1, r0, r1, inverse))


def test_wrappers_refuse_bad_arguments_before_the_device():
    z = np.zeros(16)
    gen = torch.Generator()
    for call, match in (
        (lambda: engine.synthesize("square", [1.0], 8), "kind must be one of"),
        (lambda: engine.synthesize("tone", [1.0], 0), "at least one sample"),
        (lambda: engine.synthesize("tone", np.zeros(13), 8), "params must be"),
        (lambda: engine.synthesize("tone", np.zeros((2, 2, 2)), 8), "params must be"),
        (lambda: engine.synthesize("tone", [1.0], 8, axis=("period", 1.0)), "axis must be"),
        (lambda: engine.synthesize("tone", [1.0], 8, axis=("rate", 0.0)), "rate must not be 0"),
        (lambda: engine.synthesize("tone", [1.0], 8, axis=("timestamps", np.zeros(7))), "timestamps must be"),
        (lambda: engine.synthesize("tone", np.zeros((3, 1)), 8, axis=("timestamps", np.zeros((2, 8)))), "disagree on the record count"),
        (lambda: engine.synthesize("tone", np.zeros((3, 1)), 8, records=4), "disagree on the record count"),
        (lambda: engine.synthesize("tone", [1.0], 8, envelope=("hann",)), "envelope must be"),
        (lambda: engine.synthesize("tone", [1.0], 8, envelope=("gate", 0.0, 1.0)), "envelope must be"),
        (lambda: engine.synthesize("tone", [1.0], 8, axis=("timestamps", np.zeros((2, 8))), envelope=("gate", 0.0, 1.0, 0.1)), "one time axis"),
        (lambda: engine.synthesize("tone", [1.0], 8, axis=("step", -1.0), envelope=("gate", 0.0, 1.0, 0.1)), "positive rate or step"),
        (lambda: engine.doppler(np.zeros(9), 8, ("rate", 1.0)), "params must be"),
        (lambda: engine.doppler(np.zeros(12), 0, ("rate", 1.0)), "at least one sample"),
        (lambda: synthetic_signals.chirp_noise_16bit(0), "duration_points"),
        (lambda: synthetic_signals.chirp_noise_16bit(16, noise=z, generator=gen), "not both"),
        (lambda: synthetic_signals.sawtooth_noise_16bit(16, noise=z, generator=gen), "not both"),
        (lambda: synthetic_signals.sawtooth_doppler_noise_16bit(np.zeros((2, 8))), "phase_radians must be"),
        (lambda: synthetic_signals.white_noise_fbits(z, 4.0, noise=z, generator=gen), "not both"),
        (lambda: synthetic_signals.antialias_half_nyquist(np.zeros(15)), "greater than padlen"),
        (lambda: blast_gt_pulse.gt_blast_period_center(np.zeros((2, 3)), 1.0), "time_center_s must be"),
        (lambda: blast_gt_pulse.gt_blast_center_noise_uneven(np.zeros(0)), "time_center_s must be"),
        (lambda: doppler.doppler_forward(np.zeros(4), 340., 1., 0., 2, sc.SRC0, sc.SRC1, sc.RCV0, sc.RCV1), "space_dimensions"),
        (lambda: doppler.doppler_inverse(np.zeros((2, 4)), 340., 1., 0., 3, sc.SRC0, sc.SRC1, sc.RCV0, sc.RCV1), "times must be"),
        (lambda: doppler.doppler_forward(np.zeros(4), 340., 1., 0., 3, sc.SRC0[:2], sc.SRC1, sc.RCV0, sc.RCV1), "3-element"),
    ):
        with pytest.raises(ValueError, match=match):
            call()
    with pytest.raises(TypeError, match="torch.Generator"):
        synthetic_signals.chirp_noise_16bit(16, generator=np.random.default_rng(0))
    with pytest.raises(TypeError, match="unsupported dtype"):
        engine.synthesize("tone", [1.0], 8, dtype=torch.float16)
    # the reference's IndexError when a phase of the pulse holds no sample: found on the host
    for t in (np.linspace(-5.0, -4.0, 16), np.linspace(-0.2, -0.1, 16), np.linspace(0.01, 0.2, 16)):
        with pytest.raises(IndexError, match="out of bounds for axis 0 with size 0"):
            blast_gt_pulse.gt_blast_integral_period_center(t, 1.0)


def test_the_packages_own_generator_is_unchanged():
    from quantum_inferno_amd import synth

    assert synth.SEED == 20250213

    def chirp(n, fs, channel, n_channels, dtype):  # synth.log_chirp as it has been since the first round
        k = np.arange(n, dtype=np.float64)
        f0, f1 = fs * 2.0 ** -14, 0.4 * fs
        rate = np.log(f1 / f0) / (n / fs)
        phase = 2 * np.pi * f0 * (np.exp(rate * k / fs) - 1.0) / rate + 2 * np.pi * channel / n_channels
        edge = int(np.floor(0.05 * (n - 1) / 2.0))
        ramp = 0.5 * (1 + np.cos(np.pi * (-1 + 2.0 * np.arange(edge + 1) / 0.05 / (n - 1))))
        taper = np.ones(n)
        taper[: edge + 1] = ramp
        taper[n - edge - 1:] = ramp[::-1]
        x = np.sin(phase) * taper
        x = x + (2.0 ** -8) * np.std(x) * np.random.default_rng(20250213 + channel).standard_normal(n)
        return x.astype(dtype)

    for dtype in (np.float32, np.float64):
        got = synth.channels(1000, 800.0, 1, 3, 8, dtype)
        assert got.shape == (3, 1000) and got.dtype == dtype
        assert sc.same_bits(got, np.stack([chirp(1000, 800.0, c, 8, dtype) for c in (1, 2, 3)]))
    assert sc.same_bits(synth.log_chirp(512, 100.0), chirp(512, 100.0, 0, 1, np.float32))
