"""Cases of the synthetic-signal tests and NumPy restatements of qi_synth and qi_doppler (csrc/qi_synth.hip) in the kernel's
order of operations: the time axis, the Tukey window, every kind, the envelopes, the source / receiver geometry.  Shared by
tests/test_synth_cpu.py, tests/test_gpu_synth.py and tools/gen_golden_synth.py.  Inputs are rebuilt from seeds; nothing here
reads the reference."""
import numpy as np

T = 1024          # QI_SYNTH_TILE
P = 12            # QI_SYNTH_PARAMS
DP = 12           # QI_DOPPLER_PARAMS
TOL = {"float64": 1e-11, "float32": 2e-5}  # of the record's maximum (what every record op is held to)
KINDS = ("tone", "sines3", "synth_01", "synth_02", "synth_03", "quantum_chirp", "chirp_linear", "sawtooth", "gt", "gt_hilbert",
         "gt_derivative", "gt_integral")
EXACT_KINDS = ("gt", "gt_derivative", "gt_integral")  # no library function: bit for bit on the device
AXIS_RATE, AXIS_STEP, AXIS_TIMESTAMPS = 0, 1, 2
ENV_NONE, ENV_TUKEY, ENV_GATE = 0, 1, 2
LENGTHS = (1, 2, 3, T - 1, T, T + 1, 2 * T + 17)
RECORDS = (1, 3, 65)
EPOCH = 1.7e9
FS = 800.0
SQRT6 = np.sqrt(6.0)
GT_A = 1 + np.sqrt(6.0)
EPS = np.finfo(np.float64).eps


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    return a.tobytes() == b.tobytes()


# ---- the time axis -----------------------------------------------------------------------------------------------------
def axis_time(n, axis, value=None, x=None, s0=0.0, s1=0.0):
    """t = (base(k) - s0) - s1; x [n] or [C, n] for the timestamp axis -> [n] or [C, n]."""
    k = np.arange(n)
    if axis == AXIS_RATE:
        base = k / value
    elif axis == AXIS_STEP:
        base = k * float(value)
    else:
        base = np.asarray(x, dtype=np.float64)
    return (base - s0) - s1


def tukey_ref(m, alpha):
    """scipy.signal.windows.tukey(m, alpha), element by element as the kernel's tukey_at forms it."""
    if m < 1:
        return np.zeros(0)
    if m == 1 or alpha <= 0:
        return np.ones(m)
    j = np.arange(m)
    m1 = float(m - 1)
    if alpha >= 1.0:
        step = (2 * np.pi) / m1
        fac = j * step + (-np.pi)
        fac[-1] = np.pi
        return (0.0 + 0.5 * np.cos(0.0 * fac)) + 0.5 * np.cos(fac)
    width = int(np.floor(alpha * m1 / 2.0))
    w = np.ones(m)
    head = j <= width
    tail = np.logical_and(j >= m - width - 1, ~head)
    w[head] = 0.5 * (1.0 + np.cos(np.pi * (-1.0 + 2.0 * j[head] / alpha / m1)))
    w[tail] = 0.5 * (1.0 + np.cos(np.pi * ((-2.0 / alpha + 1.0) + 2.0 * j[tail] / alpha / m1)))
    return w


def gate_span_ref(t, tmin, tmax):
    include = np.logical_and(t >= tmin, t <= tmax)
    m = int(include.sum())
    return (int(np.argmax(include)) if m else 0), m


# ---- the kinds ---------------------------------------------------------------------------------------------------------
def _gate0(v, t, tmin, tmax):
    return np.where(np.logical_or(t < tmin, t > tmax), 0.0, v)


def _two_prod(a, b):
    """a * b = h + l exactly (Dekker's product with Veltkamp's split): h the rounded product, l what a fused multiply-add
    fma(a, b, -h) returns."""
    h = a * b
    a1 = a * 134217729.0
    a1 = a1 - (a1 - a)
    a2 = a - a1
    b1 = b * 134217729.0
    b1 = b1 - (b1 - b)
    b2 = b - b1
    return h, a2 * b2 - (((h - a1 * b1) - a2 * b1) - a1 * b2)


def cube_ref(x):
    """The kernel's cube(): x * x and (x * x) * x without error, one rounding of the sum of the parts -- the correctly rounded
    x^3 (test_synth_cpu checks it against exact arithmetic on the inputs of these tests)."""
    h, l = _two_prod(x, x)
    ph, pl = _two_prod(h, x)
    return ph + (pl + l * x)


def kind_ref(kind, p, t, cube=None):
    """The sample values of one record: p its parameter row [P], t its times [n] -> float64 (complex128 for the chirp).
    cube: tau -> tau^3 of the GT integral; None is np.power(tau, 3), the reference's own call -- NumPy's pow is a library
    function that need not round correctly (its AVX-512 loop does not) -- and cube_ref is the device's."""
    p = np.concatenate([np.asarray(p, dtype=np.float64), np.zeros(P)])[:P]
    if kind == "tone":
        return np.cos(p[0] * t)
    if kind == "sines3":
        g = [_gate0(np.sin(p[i] * t), t, p[3 + 2 * i], p[4 + 2 * i]) for i in range(3)]
        return (g[0] + g[1]) + g[2]
    if kind == "synth_01":
        return np.cos(p[0] * t - p[1] * t * t) + np.cos(p[3] * np.sin(p[2] * t) + p[4] * t)
    if kind == "synth_02":
        u = [np.exp(p[3 * q] * ((t - p[3 * q + 1]) * (t - p[3 * q + 1]))) * np.cos(p[3 * q + 2] * t) for q in range(4)]
        return ((u[0] + u[1]) + u[2]) + u[3]
    if kind == "synth_03":
        with np.errstate(all="ignore"):
            return np.cos(p[0] * np.log(p[1] * t + 1.0)) + np.cos(p[2] * t + p[3] * (t * t))
    if kind == "quantum_chirp":
        q = t / p[2]
        phase = p[0] * t + p[1] * (q * q)
        z = np.zeros(len(t), dtype=np.complex128)  # NumPy's complex exp of the kernel's two arguments: exp(re) (cos(im), sin(im))
        z.real = -0.5 * (q * q) if p[3] != 0.0 else 0.0
        z.imag = phase
        return np.exp(z)
    if kind == "chirp_linear":
        return np.cos((2 * np.pi) * (p[0] * t + p[1] * t * t) + 0.0)
    if kind == "sawtooth":
        r = np.fmod(p[0] * t, 2 * np.pi)
        r = np.where(r < 0.0, r + 2 * np.pi, r)
        r = np.where(r == 0.0, 0.0, r)
        return (np.pi - r) / np.pi
    tau = t / p[0] + 1.0
    with np.errstate(invalid="ignore"):
        one = np.logical_and(0.0 <= tau, tau <= 1.0)
        two = np.logical_and(1.0 < tau, tau <= GT_A)
    v = np.zeros(len(t))
    t1, t2 = tau[one], tau[two]
    if kind == "gt":
        v[one] = 1.0 - t1
        v[two] = (1.0 / 6.0) * (1.0 - t2) * ((GT_A - t2) * (GT_A - t2))
    elif kind == "gt_derivative":
        v[one] = -1.0
        v[two] = -(1.0 / 6.0) * ((3.0 + SQRT6) - 3.0 * t2) * (GT_A - t2)
    elif kind == "gt_integral":
        v[one] = (1.0 - t1 / 2.0) * t1
        t3 = np.power(t2, 3) if cube is None else cube(t2)
        v[two] = -t2 / 72.0 * (((3.0 * t3 - (4 * (3 + 2 * SQRT6)) * (t2 * t2)) + (6 * (9 + 4 * SQRT6)) * t2) - 12 * (7 + 2 * SQRT6)) + p[1]
    elif kind == "gt_hilbert":
        u = 1.0 - t1
        v[one] = (1.0 + u * np.log(t1 + EPS)) - u * np.log(u + EPS)
        a = GT_A
        h21 = ((a - 1) / 6.0) * ((((a * (2 * a + 5)) - 1.0) + 6.0 * (t2 * t2)) - 3.0 * t2 * (1 + 3 * a))
        d = a - t2
        h22 = (t2 - 1.0) * (d * d) * (np.log(d + EPS) - np.log((t2 - 1.0) + EPS))
        v[two] = (1.0 / 6.0) * (h21 + h22)
        v = v / np.pi
    else:
        raise ValueError(kind)
    return v


def _times_window(v, w):
    """v * w, the real and the imaginary part each on its own as the kernel multiplies them (the sign of a zero product)."""
    if not np.iscomplexobj(v):
        return v * w
    out = np.empty(len(v), dtype=np.complex128)
    out.real = v.real * w
    out.imag = v.imag * w
    return out


def synth_ref(kind, params, n, axis, value=None, x=None, s0=0.0, s1=0.0, envelope=ENV_NONE, alpha=0.0, tmin=0.0, tmax=0.0,
              k0=None, m=None, records=None, cube=None):
    """qi_synth restated -> float64 [C, n] (complex128 for "quantum_chirp").  params [P'] or [C, P'], x [n] or [C, n]."""
    params = np.asarray(params, dtype=np.float64)
    times = axis_time(n, axis, value, x, s0, s1)
    count = records or (params.shape[0] if params.ndim == 2 else (times.shape[0] if times.ndim == 2 else 1))
    rows = []
    for c in range(count):
        t = times[c] if times.ndim == 2 else times
        v = kind_ref(kind, params[c] if params.ndim == 2 else params, t, cube)
        if envelope == ENV_TUKEY:
            v = _times_window(v, tukey_ref(n, alpha))
        elif envelope == ENV_GATE:
            a, b = gate_span_ref(t, tmin, tmax) if k0 is None else (k0, m)
            w = tukey_ref(max(b, 1), alpha)
            inside = np.logical_and(t >= tmin, t <= tmax)
            j = np.clip(np.arange(n) - a, 0, max(b, 1) - 1)
            v = np.where(inside, _times_window(v, w[j]), v)
            v = np.where(np.logical_or(t < tmin, t > tmax), 0.0, v)
        rows.append(v)
    return np.stack(rows)


# ---- parameter rows, by the reference's own host expressions ----------------------------------------------------------------
def row_sines3(f0=100.0, f1=200.0, f2=400.0, start2=0.25, stop2=0.4):
    return np.array([2.0 * np.pi * f0, 2.0 * np.pi * f1, 2.0 * np.pi * f2, 0, 0.5, 0.5, 1.0, start2, stop2], dtype=np.float64)


def row_synth_01(a=100.0, b=20.0, f=5.0):
    return np.array([a * np.pi, b * np.pi, np.pi * f, 4.0 * np.pi, np.pi * 80.0])


def row_synth_02(t1=0.3, t2=0.7, t3=0.5, f1=45.0, f2=75.0, f3=15.0):
    return np.array([-35.0 * np.pi, t1, np.pi * f1, -35.0 * np.pi, t2, np.pi * f1, -55.0 * np.pi, t3, np.pi * f2, -45.0 * np.pi, t3, np.pi * f3])


def row_synth_03(a=30.0, b=40.0, c=150.0):
    return np.array([20.0 * np.pi, a, b * np.pi, c * np.pi])


def row_chirp(f0, t1, f1):
    beta = (float(f1) - float(f0)) / float(t1)
    return np.array([float(f0), 0.5 * beta])


# ---- doppler -------------------------------------------------------------------------------------------------------------
def dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def doppler_ref(p, t, inverse):
    """qi_doppler restated for one record: p its parameter row [DP], t its times [n] -> (time, range, omega)."""
    c, c2, denom = p[0], p[1], p[2]
    s, v, r = p[3:6], p[6:9], p[9:12]
    if inverse:
        q = [r[d] + v[d] * t for d in range(3)]
        term1 = c2 * t - dot3(s, q)
    else:
        q = [r[d] - s[d] * t for d in range(3)]
        term1 = c2 * t + dot3(v, q)
    term1 = term1 * denom
    rm = np.sqrt(dot3(q, q))
    tc = t * c
    term2 = (rm * rm - tc * tc) * denom
    root = np.sqrt(term1 * term1 + term2)
    if inverse:
        ts = term1 - root
        g = [q[d] - s[d] * ts for d in range(3)]
    else:
        ts = term1 + root
        g = [q[d] + v[d] * ts for d in range(3)]
    rt = np.sqrt(dot3(g, g))
    om = (c - dot3(g, v) / rt) / (c - dot3(g, s) / rt)
    return ts, rt, om


def velocity(speed, init, final):
    """doppler._get_velocity_mps's vector, by its expression."""
    init, final = np.asarray(init, dtype=np.float64), np.asarray(final, dtype=np.float64)
    if speed > 0:
        rv = final - init
        return speed * (rv / np.sqrt(np.sum(rv * rv)))
    return np.zeros(3)


def doppler_row(c, source_speed, receiver_speed, src_init, src_final, rcvr_init, rcvr_final, inverse):
    obj = source_speed if inverse else receiver_speed
    denom = 1. / (c**2 - obj**2)
    return np.concatenate([[c, c**2, denom], velocity(source_speed, src_init, src_final), velocity(receiver_speed, rcvr_init, rcvr_final),
                           np.asarray(rcvr_init, dtype=np.float64) - np.asarray(src_init, dtype=np.float64)])


# geometry of the tutorial s00_doppler_20hz, and a moving receiver
SRC0, SRC1 = np.array([-1000., 10., 150.]), np.array([1000., 10., 150.])
RCV0, RCV1 = np.array([0., 0., 1.]), np.array([0., 0., 1.])
RCV_MOVING = (np.array([-50., 30., 2.]), np.array([80., -20., 2.]))
IMAGE = np.array([1., 1., -1.])
DOPPLER_SPEEDS = (340., 68., 0.)  # signal, source, receiver
DOPPLER_N = (7, 1000, 4097)


def doppler_cases():
    """(name, n, inverse, geometry, times, images): the tutorial's geometry and a moving receiver, both directions, each with
    its image source; at the longest n the tutorial's direct path alone (the fixture's size)."""
    out = []
    for n in DOPPLER_N:
        t = np.arange(n) / 1000
        for inverse in (False, True):
            times = 2.9 + t if inverse else t
            out.append((f"tutorial_n{n}_{int(inverse)}", n, inverse, (340., 68., 0., SRC0, SRC1, RCV0, RCV1), times,
                        (False,) if n == DOPPLER_N[-1] else (False, True)))
            if n != DOPPLER_N[-1]:
                out.append((f"moving_n{n}_{int(inverse)}", n, inverse, (340., 68., 12., SRC0, SRC1) + RCV_MOVING, times, (False, True)))
    return out


# ---- the device matrix ------------------------------------------------------------------------------------------------------
def rng(*salt):
    return np.random.default_rng([20250213, *salt])


def kind_rows(kind, records, salt=0):
    """`records` parameter rows of a kind that differ from one another (a stride mistake shows), sized for times in about [-1, 2] s."""
    r = rng(KINDS.index(kind), salt)
    f = r.uniform(0.8, 1.25, (records, 1))
    base = {
        "tone": np.array([2.0 * np.pi * 60.0]),
        "sines3": row_sines3(),
        "synth_01": row_synth_01(),
        "synth_02": row_synth_02(),
        "synth_03": row_synth_03(),
        "quantum_chirp": np.array([40.0, 0.5 * 0.3, 0.7, 1.0]),
        "chirp_linear": row_chirp(5.0, 1.5, 100.0),
        "sawtooth": np.array([2 * np.pi * 7.0]),
        "gt": np.array([0.25 / 4.0, 0.0]),
        "gt_hilbert": np.array([0.25 / 4.0, 0.0]),
        "gt_derivative": np.array([0.25 / 4.0, 0.0]),
        "gt_integral": np.array([0.25 / 4.0, 0.125]),
    }[kind]
    rows = np.tile(base, (records, 1))
    if kind == "sines3":
        rows[:, :3] *= f
    elif kind == "synth_02":
        rows[:, 2::3] *= f
    elif kind == "quantum_chirp":
        rows[:, :1] *= f
    elif kind == "synth_03":
        rows[:, 2:] *= f
    else:
        rows[:, :1] *= f
    return rows


AXES = ("rate", "step", "shared0", "sharedE", "rowsE")


def axis_case(name, n, records):
    """-> dict(axis, value, x, s0, s1) of one of AXES.  The times run over about [-0.3, 1.4] s at 800 Hz for every n up to
    2 T + 17: "rate" and "step" from 0, the timestamp forms jittered, from 0 or from an epoch near 1.7e9 s (s0 takes it off)."""
    span = max(n - 1, 1)
    rate = span / 1.7
    if name == "rate":
        return dict(axis=AXIS_RATE, value=rate, x=None, s0=0.3, s1=0.0)
    if name == "step":
        return dict(axis=AXIS_STEP, value=1.7 / span, x=None, s0=0.0, s1=0.3)
    r = rng(99, n, AXES.index(name))
    shape = (records, n) if name == "rowsE" else (n,)
    x = (np.arange(n) + r.uniform(-0.3, 0.3, shape)) / rate
    start = EPOCH if name.endswith("E") else 0.0
    return dict(axis=AXIS_TIMESTAMPS, value=0.0, x=start + x, s0=start, s1=0.3)


# ---- the reference-signature wrappers: (key, module, function, keyword arguments); inputs and noise rebuilt from seeds -------
def normal(key, n):
    """The standard-normal variates the fixture's noise was made of, for the wrapper case `key`."""
    return rng(7, sum(key.encode())).standard_normal(n)


def uneven_epoch(n=1000):
    return EPOCH + (np.arange(n) + rng(5).uniform(-0.3, 0.3, n)) / 100.0


def doppler_phase(n=3000):
    """A phase record as the tutorial forms it: 2 pi f tau for source times that the inverse problem returns (smooth, uneven)."""
    t = np.arange(n) / 1000.0
    return 2. * np.pi * 20. * (t + 0.05 * np.sin(2 * np.pi * 0.7 * t))


WRAPPER_CASES = (
    ("qchirp_default", "benchmark_signals", "quantum_chirp", dict(omega=np.pi / 8)),
    ("qchirp_sweep", "benchmark_signals", "quantum_chirp", dict(omega=np.pi / 5, order=3.0, gamma=0.5, gauss=False)),
    ("qchirp_reset", "benchmark_signals", "quantum_chirp", dict(omega=0.9 * np.pi, order=6.0, oversample_scale=1)),  # (at 2 and more the
    # reset frequency lies in the decimator's stop band and the reference returns rounding noise)
    ("synth_00_default", "benchmark_signals", "synth_00", dict()),
    ("synth_00_small", "benchmark_signals", "synth_00", dict(frequency_0=30.0, frequency_1=55.0, frequency_2=90.0, time_start_2=0.2,
                                                             time_stop_2=0.7, time_sample_interval=2e-3, oversample_scale=3)),
    ("synth_01_default", "benchmark_signals", "synth_01", dict()),
    ("synth_01_long", "benchmark_signals", "synth_01", dict(a=80.0, b=10.0, f=3.0, time_duration=1.3)),
    ("synth_02_default", "benchmark_signals", "synth_02", dict()),
    ("synth_03_default", "benchmark_signals", "synth_03", dict()),
    ("synth_03_small", "benchmark_signals", "synth_03", dict(a=10.0, b=25.0, c=60.0, time_sample_interval=1.0 / 1024)),
    ("tone_default", "benchmark_signals", "well_tempered_tone", dict()),
    ("tone_nominal", "benchmark_signals", "well_tempered_tone", dict(frequency_sample_rate_hz=1000.0, frequency_center_hz=61.7,
                                                                     time_duration_s=2.0, time_fft_s=0.5, use_fft_frequency=False)),
    ("tone_noise", "benchmark_signals", "well_tempered_tone", dict(time_duration_s=2.56, add_noise_taper_aa=True)),
    ("chirp16_default", "synthetic_signals", "chirp_noise_16bit", dict()),
    ("chirp16_small", "synthetic_signals", "chirp_noise_16bit", dict(duration_points=1000, sample_rate_hz=200.0, noise_std_loss_bits=6.0,
                                                                     frequency_center_hz=10.0)),
    ("saw16_default", "synthetic_signals", "sawtooth_noise_16bit", dict()),
    ("saw16_small", "synthetic_signals", "sawtooth_noise_16bit", dict(duration_points=1025, sample_rate_hz=100.0, frequency_center_hz=3.0)),
    ("saw_doppler", "synthetic_signals", "sawtooth_doppler_noise_16bit", dict(phase_radians="doppler_phase")),
    ("chirp_in_noise", "synthetic_signals", "chirp_linear_in_noise", dict(snr_bits=3.0, sample_rate_hz=500.0, duration_s=2.0,
                                                                          frequency_start_hz=20.0, frequency_end_hz=120.0, intro_s=0.5,
                                                                          outro_s=1)),
    ("gt_fast", "blast_gt_pulse", "gt_blast_center_fast", dict()),
    ("gt_noise", "blast_gt_pulse", "gt_blast_center_noise", dict()),
    ("gt_noise_small", "blast_gt_pulse", "gt_blast_center_noise", dict(duration_s=10.25, frequency_peak_hz=2.0, noise_std_loss_bits=8.)),
    ("gt_uneven", "blast_gt_pulse", "gt_blast_center_noise_uneven", dict(sensor_epoch_s="uneven_epoch")),
    ("gt_uneven_fc", "blast_gt_pulse", "gt_blast_center_noise_uneven", dict(sensor_epoch_s="uneven_epoch", noise_std_loss_bits=5.,
                                                                            frequency_center_hz=0.8)),
    ("gt_calculus", "blast_gt_pulse", "gt_blast_center_integral_and_derivative", dict(frequency_peak_hz=1.3, sample_rate_hz=1000.0)),
)
NOISY = ("tone_noise", "chirp16_default", "chirp16_small", "saw16_default", "saw16_small", "saw_doppler", "chirp_in_noise", "gt_fast",
         "gt_noise", "gt_noise_small", "gt_uneven", "gt_uneven_fc")
INPUTS = {"doppler_phase": doppler_phase, "uneven_epoch": uneven_epoch}


def wrapper_kwargs(kwargs):
    return {k: (INPUTS[v]() if isinstance(v, str) else v) for k, v in kwargs.items()}


# the GT family on given centred times: (key, function, time, pseudo period)
def gt_times(n=2 * T + 17, span=3.0):
    return (np.arange(n) - (n - 1) / 2.0) * (span / n)


GT_CASES = tuple((f"{fn}_{i}", fn, period) for fn in ("gt_blast_period_center", "gt_hilbert_blast_period_center",
                                                      "gt_blast_derivative_period_center", "gt_blast_integral_period_center")
                 for i, period in enumerate((1.0, 0.37)))
GT_KIND = {"gt_blast_period_center": "gt", "gt_hilbert_blast_period_center": "gt_hilbert", "gt_blast_derivative_period_center": "gt_derivative",
           "gt_blast_integral_period_center": "gt_integral"}

# host-only functions: (key, module, function, positional arguments)
HOST_CASES = (
    ("grain", "synthetic_signals", "gabor_grain_frequencies", (3.0, 1.0, 100.0, 800.0)),
    ("algebraic", "synthetic_signals", "frequency_algebraic_nth", (np.array([1.0, 2.5, 40.0]), 6.0)),
    ("taper", "synthetic_signals", "taper_tukey", (np.zeros(257), 0.25)),
    ("oversample", "benchmark_signals", "oversample_time", (1.0, 1e-3, 2)),
    ("ft", "blast_gt_pulse", "gt_blast_ft", (6.3, np.linspace(0.5, 40.0, 64))),
    ("density", "blast_gt_pulse", "gt_blast_spectral_density", (6.3, np.linspace(0.5, 40.0, 64))),
    ("duration", "doppler", "time_duration", (np.array([3.0, -1.0, 2.5]),)),
    ("time4d", "doppler", "time_4d_mx", (np.arange(4.0), 3)),
    ("space4d", "doppler", "space_4d_mx", (np.array([1.0, 2.0, 3.0]), 4)),
    ("hadamard", "doppler", "hadamard_dot_product_mx", (np.arange(12.0).reshape(4, 3) / 7, np.arange(12.0, 24.0).reshape(4, 3) / 3)),
    ("range_vector", "doppler", "range_vector_sr", (SRC0, RCV0)),
    ("range_matrix", "doppler", "range_matrix_sr", (np.arange(12.0).reshape(4, 3), np.ones((4, 3)))),
    ("range_hadamard", "doppler", "range_hadamard", (np.arange(12.0).reshape(4, 3) / 7,)),
    ("range_scalar", "doppler", "range_scalar", (SRC0, RCV0)),
)


# ---- what the reference hands to decimate / filtfilt, or returns unfiltered, restated per wrapper case -----------------------
def _noisy(key, wf, bits):
    return wf + (0.0 + np.std(wf) / 2.0 ** bits * normal(key, wf.size))


def _defaults(kwargs, **defaults):
    return [kwargs.get(k, v) for k, v in defaults.items()]


def wrapper_restated(key, name, kwargs):
    """-> {fixture suffix: array} of the waveforms of one wrapper case that the restatements give bit for bit."""
    kw = wrapper_kwargs(kwargs)
    if name == "quantum_chirp":
        omega, order, gamma, gauss, q = _defaults(kw, omega=None, order=12.0, gamma=0.0, gauss=True, oversample_scale=2)
        if omega >= 0.8 * np.pi:
            omega = np.pi * 2 ** (-1 / order)
        chirp_scale = 3.0 / 4.0 * np.pi * order / omega * np.sqrt(1 + gamma ** 2)
        points = q * 2 ** int((np.ceil(np.log2(2.0 * np.pi * chirp_scale))))
        wf = synth_ref("quantum_chirp", [omega, 0.5 * gamma, chirp_scale, float(gauss)], points, AXIS_STEP, 1.0, s0=(points - 1) / 2)[0]
        return {"decimate0": wf.real.copy(), "decimate1": wf.imag.copy()}
    if name in ("synth_00", "synth_01", "synth_02", "synth_03"):
        dt, duration, q = _defaults(kw, time_sample_interval=1e-3, time_duration=1.0, oversample_scale=2)
        if name == "synth_00":
            kind, row = "sines3", row_sines3(*_defaults(kw, frequency_0=100.0, frequency_1=200.0, frequency_2=400.0, time_start_2=0.25, time_stop_2=0.4))
        elif name == "synth_01":
            kind, row = name, row_synth_01(*_defaults(kw, a=100.0, b=20.0, f=5.0))
        elif name == "synth_02":
            kind, row = name, row_synth_02(*_defaults(kw, t1=0.3, t2=0.7, t3=0.5, f1=45.0, f2=75.0, f3=15.0))
        else:
            kind, row = name, row_synth_03(*_defaults(kw, a=30.0, b=40.0, c=150.0))
        interval = dt / q
        gate = dict(envelope=ENV_GATE, alpha=0.05, tmin=0.0, tmax=1.0) if name != "synth_02" else {}
        return {"decimate0": synth_ref(kind, row, int(duration / interval), AXIS_STEP, interval, **gate)[0]}
    if name == "well_tempered_tone":
        rate, fc, duration, fft_s, use_fft, noisy = _defaults(kw, frequency_sample_rate_hz=800.0, frequency_center_hz=60.0, time_duration_s=10.24,
                                                              time_fft_s=0.64, use_fft_frequency=True, add_noise_taper_aa=False)
        n, nfft = 2 ** (int(np.log2(duration * rate))), 2 ** (int(np.log2(fft_s * rate)))
        bins = np.fft.rfftfreq(nfft, d=1 / rate)
        f_c = (bins[np.argmin(np.abs(bins - fc))] if use_fft else fc) / rate
        wf = synth_ref("tone", [2.0 * np.pi * f_c], n, AXIS_STEP, 1.0)[0]
        if noisy:
            wf = _noisy(key, wf, 8.0) * tukey_ref(n, 0.1)
            return {"out0": wf, "filtfilt0": wf}
        return {"out0": wf}
    if name in ("chirp_noise_16bit", "sawtooth_noise_16bit"):
        n, rate, bits, fc = _defaults(kw, duration_points=2 ** 12, sample_rate_hz=80.0, noise_std_loss_bits=4.0, frequency_center_hz=None)
        fc = fc if fc else 8.0 / (n / rate)
        if name == "chirp_noise_16bit":
            wf = synth_ref("chirp_linear", row_chirp(0.5 * fc, (n - 1) / rate, rate / 4.0), n, AXIS_RATE, rate, envelope=ENV_TUKEY, alpha=0.25)[0]
        else:
            wf = synth_ref("sawtooth", [(2 * np.pi * fc)], n, AXIS_RATE, rate, envelope=ENV_TUKEY, alpha=0.25)[0]
        return {"filtfilt0": _noisy(key, wf, bits)}
    if name == "sawtooth_doppler_noise_16bit":
        phase = kw["phase_radians"]
        wf = synth_ref("sawtooth", [1.0], len(phase), AXIS_TIMESTAMPS, x=phase, envelope=ENV_TUKEY, alpha=0.25)[0]
        return {"filtfilt0": _noisy(key, wf, kw.get("noise_std_loss_bits", 4.0))}
    if name == "chirp_linear_in_noise":
        rate, n = kw["sample_rate_hz"], int(kw["sample_rate_hz"] * kw["duration_s"])
        row = row_chirp(kw["frequency_start_hz"], (n - 1) / rate, kw["frequency_end_hz"])
        wf = synth_ref("chirp_linear", row, n, AXIS_RATE, rate, envelope=ENV_TUKEY, alpha=0.25)[0]
        sig = np.concatenate((np.zeros(int(kw["intro_s"] * rate)), wf, np.zeros(int(kw["outro_s"] * rate))))
        return {"out0": _noisy(key, sig, kw["snr_bits"])}
    if name in ("gt_blast_center_fast", "gt_blast_center_noise"):
        fpeak, rate, bits = _defaults(kw, frequency_peak_hz=6.3, sample_rate_hz=100.0, noise_std_loss_bits=16.)
        n = int(16 / fpeak * rate) if name == "gt_blast_center_fast" else int(kw.get("duration_s", 16.) * rate)
        half = ((n - 1) / rate) / 2.0
        wf = synth_ref("gt", [(1 / fpeak) / 4.0], n, AXIS_RATE, rate, s0=half)[0]
        return {"out0": axis_time(n, AXIS_RATE, rate, s0=half), "filtfilt0": _noisy(key, wf, bits)}
    if name == "gt_blast_center_noise_uneven":
        epoch, bits, fc = _defaults(kw, sensor_epoch_s=None, noise_std_loss_bits=2., frequency_center_hz=None)
        duration = epoch[-1] - epoch[0]
        wf = synth_ref("gt", [(1 / fc if fc else duration / 4.0) / 4.0], len(epoch), AXIS_TIMESTAMPS, x=epoch, s0=epoch[0], s1=duration / 2.0)[0]
        return {"filtfilt0": _noisy(key, wf, bits)}
    if name == "gt_blast_center_integral_and_derivative":
        fpeak, rate = kw["frequency_peak_hz"], kw["sample_rate_hz"]
        n = int(2 / fpeak * rate)
        axis = dict(axis=AXIS_RATE, value=rate, s0=((n - 1) / rate) / 2.0)
        quarter = (1 / fpeak) / 4.0
        gt = synth_ref("gt", [quarter], n, **axis)[0]
        zero = synth_ref("gt_integral", [quarter, 0.0], n, **axis)[0]
        tau = axis_time(n, **axis) / quarter + 1.0
        last = np.where((0.0 <= tau) & (tau <= 1.0))[0][-1]
        first = np.where((1.0 < tau) & (tau <= GT_A))[0][0]
        integral = synth_ref("gt_integral", [quarter, zero[last] - zero[first]], n, **axis)[0]
        deriv = synth_ref("gt_derivative", [quarter], n, **axis)[0]
        deriv[np.argmax(gt) - 1] = np.max(np.diff(gt)) / np.mean(np.diff(axis_time(n, **axis) / quarter))
        return {"out0": axis_time(n, **axis) / quarter, "out1": gt, "out2": integral, "out3": deriv}
    raise ValueError(name)


def gt_case_restated(name, period, t):
    quarter = period / 4.0
    kind = GT_KIND[name]
    if kind != "gt_integral":
        return kind_ref(kind, [quarter], t)
    zero = kind_ref(kind, [quarter, 0.0], t)
    tau = t / quarter + 1.0
    last = np.where((0.0 <= tau) & (tau <= 1.0))[0][-1]
    first = np.where((1.0 < tau) & (tau <= GT_A))[0][0]
    return kind_ref(kind, [quarter, zero[last] - zero[first]], t)


def restatement_failures(g):
    """Every array of the fixture `g` that a restatement should equal bit for bit and does not -> [description]."""
    bad = []

    def compare(where, got, want):
        if not same_bits(got, want):
            differ = int(np.sum(got != want)) if np.shape(got) == np.shape(want) else -1
            bad.append(f"{where}: {differ} of {np.size(want)} differ, dtypes {np.asarray(got).dtype} / {want.dtype}")

    for key, _, name, kwargs in WRAPPER_CASES:
        for suffix, got in wrapper_restated(key, name, kwargs).items():
            compare(f"{key}_{suffix}", got, g[f"{key}_{suffix}"])
    t = gt_times()
    for key, name, period in GT_CASES:
        compare(key, gt_case_restated(name, period, t), g[key])
    for key, n, inverse, geometry, times, images in doppler_cases():
        for image in images:
            c, vs, vr, s0, s1, r0, r1 = geometry
            row = doppler_row(c, vs, vr, s0 * IMAGE if image else s0, s1 * IMAGE if image else s1, r0, r1, inverse)
            for i, got in enumerate(doppler_ref(row, times, inverse)):
                compare(f"doppler_{key}_{int(image)}_{i}", got, g[f"doppler_{key}_{int(image)}_{i}"])
    return bad
