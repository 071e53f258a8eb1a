"""Hard inputs of the array factorisations (qi_csd_eigh, qi_csd_whiten) and of the forms that read them, shared by
tests/test_array_hard_cpu.py and tests/test_gpu_array_hard.py.  The restatements are those of music_cases, capon_cases,
beam_cases and steer_cases; here are only the matrices those files never draw, the grids, two closed forms and the recorded
deviations of the restatements on these matrices.

`families(C, dtype)` is a stack [len(FAMILIES), C, C], one seeded Hermitian matrix per name of FAMILIES, from
np.random.default_rng([SEED, C]): where a spectrum is prescribed the matrix is Q diag(lambda) Q^H with a seeded unitary Q,
symmetrised in complex128 and then rounded to `dtype`.  At C = 1 every family is a 1 x 1 matrix.
  repeated       1.5 I plus a part of rank k = min(2, C - 1) with eigenvalues in [50, 100]: the noise eigenvalue 1.5 is repeated
                 C - k times (white noise and k sources)
  rank_one       x x^H, x complex normal (one coherent arrival); `rank_one_vector` is x
  graded         eigenvalues 10^(-p j / (C - 1)), p = GRADE[dtype] decades (a spectrum that falls across the band)
  indefinite     eigenvalues uniform in [-100, 100] (an imaginary part of the coherence, a difference of two matrices)
  pairs          eigenvalues m and m (1 + 1e-3), m = 1, 2, ...: close pairs
  dead_sensor    eigenvalues uniform in [1, 100], then row and column C // 2 zero: the unit vector C // 2 spans the null space
  twin_sensors   the same kind, then row and column C - 1 are copies of row and column 0 (T S T^H, T the identity with its
                 last row e_0^T): Hermitian, one zero eigenvalue, the null vector (e_0 - e_{C-1}) / sqrt 2
  two_subarrays  two full blocks of sizes C // 2 (the odd sensors) and C - C // 2 (the even ones) that share nothing: in every
                 step of the solver's schedule a wave has rotations it takes beside rotations it skips
  all_equal      every entry 3: rank one with equal rows
`conditioned` and `first_bad_pivot` are further inputs of the whitener.  The closed forms of the rank-one matrix owe nothing
to LAPACK: with one source the MUSIC null spectrum is C - |x^H e|^2 / |x|^2, and for R = sigma I + x x^H, sigma = loading
|x|^2 / C (capon_cases.loaded's rule), Sherman and Morrison give e^H R^-1 e = (C - |x^H e|^2 / (sigma + |x|^2)) / sigma.
"""
import functools

import numpy as np

import beam_cases as bc
import capon_cases as cpc
import music_cases as mc

DTYPES = bc.DTYPES
TOL = bc.TOL
SEED = 53
FAMILIES = ("repeated", "rank_one", "graded", "indefinite", "pairs", "dead_sensor", "twin_sensors", "two_subarrays", "all_equal")
GRADE = {"float32": 6, "float64": 12}  # decades of the graded spectrum
CONDITION = {"float32": 1e4, "float64": 1e10}  # of `conditioned`
G = 17  # grid points of every form here
CPU_SENSORS = (2, 3, 8, 17, 48, 63, 64)  # where the CPU test runs eigh_steps on the families
WHITEN_SENSORS = (5, 17, 64)  # where `conditioned`, `first_bad_pivot` and the closed forms are run
SCALE_SENSORS = (5, 33, 64)
SWEEPS_MOST = mc.SWEEP_CAP // 2
# Exact rescales: eigh_steps(2^k S) has the eigenvectors of eigh_steps(S) bit for bit, its eigenvalues times 2^k and its sweep
# counts; whiten_steps(4^k S, loading) is 2^-k whiten_steps(S, loading) bit for bit.  The exponents are what leaves every
# entry, every product of the Cholesky and every square of the double-precision norms a normal number: float64 at 2^-500 does
# not hold (the squares underflow).
EIGH_SCALES = {"float32": (60, -60), "float64": (300, -300)}
WHITEN_SCALES = {"float32": (30, -30), "float64": (250, -250)}
# The largest deviations of the restatements in `dtype` from the float64 statements on these inputs, as NumPy gave them on the
# CPU (tests/test_array_hard_cpu.py computes every one again and holds the constant to it).  eigh_steps on every family at
# CPU_SENSORS, per matrix: the eigenvalues against eigh64's as a fraction of the matrix's largest modulus, max |U^H U - I|,
# max |S U - U w| over the largest modulus.  whiten_steps of `conditioned` without loading at WHITEN_SENSORS: max |V^H R V - I|,
# and 1 / power of the Capon form fed that V (capon32 in float32) against the form of capon_cases.whiten's, as a fraction of
# the largest 1 / power.
# Each is the measurement rounded up by a tenth: the test admits the measurement up to a quarter below its constant.
EIGH_HARD_VALUES = {"float32": 1.26e-6, "float64": 2.77e-15}  # (1.146e-06: twin_sensors, C = 64; 2.522e-15: indefinite, C = 63)
EIGH_HARD_ORTHO = {"float32": 1.85e-5, "float64": 2.54e-14}  # (1.686e-05: graded, C = 64; 2.309e-14: graded, C = 48)
EIGH_HARD_PAIRS = {"float32": 6.35e-6, "float64": 6.28e-15}  # (5.776e-06: two_subarrays, C = 64; 5.711e-15: pairs, C = 64)
WHITEN_HARD_RESIDUAL = {"float32": 5.54e-5, "float64": 2.96e-7}  # (5.036e-05: C = 17, cond 1e4; 2.688e-07: C = 5, cond 1e10)
CAPON_HARD_RECIPROCAL = {"float32": 6.33e-5, "float64": 1.71e-7}  # (5.754e-05: C = 17, cond 1e4; 1.556e-07: C = 5, cond 1e10)
RESTATEMENT_MARGIN = 16  # the project's margin between a restatement's deviation and a bound on the kernel


def index_of(name):
    return FAMILIES.index(name)


# ---- the families -----------------------------------------------------------------------------------------------------------------
def _unitary(rng, n):
    q, _ = np.linalg.qr(rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))
    return q


def _of_spectrum(q, lam):
    s = (q * np.asarray(lam, dtype=np.float64)[None, :]) @ np.conj(q.T)
    return 0.5 * (s + np.conj(s.T))


@functools.lru_cache(maxsize=None)
def _draws(C):
    """Everything random of the families of C sensors, drawn once in a fixed order."""
    rng = np.random.default_rng([SEED, C])
    k = mc.sources_of(C)
    d = {}
    q = _unitary(rng, C)
    d["repeated"] = 1.5 * np.eye(C) + _of_spectrum(q[:, C - k:], rng.uniform(50.0, 100.0, k))
    x = rng.standard_normal(C) + 1j * rng.standard_normal(C)
    d["x"] = x
    d["rank_one"] = _of_spectrum(x[:, None], [1.0])
    d["q_graded"] = _unitary(rng, C)
    d["indefinite"] = _of_spectrum(_unitary(rng, C), rng.uniform(-100.0, 100.0, C))
    m = np.arange(C) // 2 + 1.0
    d["pairs"] = _of_spectrum(_unitary(rng, C), np.where(np.arange(C) % 2 == 0, m, m * (1 + 1e-3)))
    dead = _of_spectrum(_unitary(rng, C), rng.uniform(1.0, 100.0, C))
    dead[C // 2, :] = 0
    dead[:, C // 2] = 0
    d["dead_sensor"] = dead
    twin = _of_spectrum(_unitary(rng, C), rng.uniform(1.0, 100.0, C))
    twin[C - 1, :] = twin[0, :]
    twin[:, C - 1] = twin[:, 0]  # (the corner: S[0][0])
    d["twin_sensors"] = twin
    two = np.zeros((C, C), dtype=np.complex128)
    for sensors in (np.arange(1, C, 2), np.arange(0, C, 2)):
        if sensors.size:
            two[np.ix_(sensors, sensors)] = _of_spectrum(_unitary(rng, sensors.size), rng.uniform(1.0, 100.0, sensors.size))
    d["two_subarrays"] = two
    d["all_equal"] = np.full((C, C), 3.0 + 0j)
    d["q_conditioned"] = _unitary(rng, C)
    for a in d.values():
        a.setflags(write=False)
    return d


def _powers(base, C):
    """base^(j / (C - 1)), j = 0 .. C - 1; 1 at C = 1."""
    return base ** (np.arange(C) / float(max(C - 1, 1)))


@functools.lru_cache(maxsize=None)
def _families(C, dtype):
    d = _draws(C)
    graded = _of_spectrum(d["q_graded"], _powers(10.0 ** -GRADE[dtype], C))
    out = np.stack([graded if name == "graded" else d[name] for name in FAMILIES])
    assert np.array_equal(out, np.conj(np.swapaxes(out, 1, 2)))
    out = out.astype(bc.complex_of(dtype))
    out.setflags(write=False)
    return out


def families(C, dtype):
    """[len(FAMILIES), C, C] complex of dtype, Hermitian, in the order of FAMILIES (a copy of the stack that is built once)."""
    return _families(int(C), np.dtype(dtype).name).copy()


def rank_one_vector(C):
    """x of the family rank_one, complex128."""
    return _draws(int(C))["x"]


# ---- further inputs of the whitener -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _conditioned(C, dtype, cond):
    out = _of_spectrum(_draws(C)["q_conditioned"], _powers(cond, C))[None].astype(bc.complex_of(dtype))
    out.setflags(write=False)
    return out


def conditioned(C, dtype, cond=None):
    """[1, C, C] complex of dtype, positive definite: eigenvalues cond^(j / (C - 1)), cond = CONDITION[dtype] unless given."""
    name = np.dtype(dtype).name
    return _conditioned(int(C), name, float(CONDITION[name] if cond is None else cond)).copy()


def first_bad_pivot(C, k):
    """[C, C] complex128: L D L^H, L unit lower triangular with 0.3 x complex normal below the diagonal, D = I but D[k-1] = -1:
    the first k - 1 pivots of a Cholesky factorisation are 1 and pivot k is -1 -- potrf's info is exactly k."""
    rng = np.random.default_rng([SEED, C, k])
    low = np.tril(0.3 * (rng.standard_normal((C, C)) + 1j * rng.standard_normal((C, C))), -1) + np.eye(C)
    d = np.ones(C)
    d[k - 1] = -1.0
    r = (low * d[None, :]) @ np.conj(low.T)
    return 0.5 * (r + np.conj(r.T))


def bad_pivots(C):
    return (1, 2, C // 2 + 1, C)


def definite_stack(C, nf, dtype):
    """[nf, C, C] matrices of capon_cases: the good neighbours of a flagged matrix."""
    return cpc._definite_matrices(C, nf).astype(bc.complex_of(dtype))


# ---- the grid -----------------------------------------------------------------------------------------------------------------------
def grid(C, nf):
    """(frequency_hz [nf], delays_s [G, C] float64): frequencies uniform in 1 .. 40 Hz, delays of beam_cases' range."""
    rng = np.random.default_rng([SEED + 1, C, nf])
    return rng.uniform(1.0, 40.0, nf), rng.uniform(-bc.MAX_DELAY_S, bc.MAX_DELAY_S, (G, C))


def factors(freq, tau):
    """e [nf, G, C] = exp(2 pi i reduced turns), complex128."""
    return np.exp(2j * np.pi * bc.reduced_turns(freq, tau))


# ---- the closed forms of x x^H --------------------------------------------------------------------------------------------------------
def _along(x, e):
    """|x^H e|^2 [nf, G]."""
    p = np.einsum("i,fgi->fg", np.conj(np.asarray(x, dtype=np.complex128)), e)
    return p.real ** 2 + p.imag ** 2


def music_rank_one(x, e):
    """The MUSIC null spectrum D [nf, G] of x x^H with one source: 1 / power = D / C."""
    n2 = float(np.sum(np.abs(x) ** 2))
    return float(len(x)) - _along(x, e) / n2


def capon_rank_one(x, e, loading):
    """e^H R^-1 e [nf, G] of R = x x^H + loading mean(diag x x^H) I: 1 / power."""
    n2 = float(np.sum(np.abs(x) ** 2))
    sigma = loading * n2 / float(len(x))
    return (float(len(x)) - _along(x, e) / (sigma + n2)) / sigma


# ---- deviations -----------------------------------------------------------------------------------------------------------------------
def eigen_deviations(w, u, csd):
    """Per matrix, in float64: (the eigenvalues against eigh64's over the matrix's largest modulus, max |U^H U - I|,
    max |S U - U w| over the largest modulus) -> three arrays [nf].  A matrix of zeros is measured absolutely."""
    ref = mc.eigh64(csd)[0]
    top = np.abs(ref).max(axis=1)
    top = np.where(top > 0, top, 1.0)
    values = np.abs(np.asarray(w).astype(np.float64) - ref).max(axis=1) / top
    u64, w64, s = np.asarray(u).astype(np.complex128), np.asarray(w).astype(np.float64), mc.hermitian_of_lower(csd)
    ortho = np.abs(np.conj(np.swapaxes(u64, 1, 2)) @ u64 - np.eye(u64.shape[1])).max(axis=(1, 2))
    pairs = np.abs(s @ u64 - u64 * w64[:, None, :]).max(axis=(1, 2)) / top
    return values, ortho, pairs


def projector(u, columns):
    """U_c U_c^H of the given columns, complex128 [nf, C, C] (u: [nf, C, C]) or [C, C]."""
    uc = np.asarray(u).astype(np.complex128)[..., columns]
    return uc @ np.conj(np.swapaxes(uc, -1, -2))


def subspaces(C):
    """(family, columns of the ascending eigenvectors) where a gap makes the subspace well defined."""
    k = mc.sources_of(C)
    out = [("rank_one", slice(C - 1, C)), ("all_equal", slice(C - 1, C)), ("dead_sensor", slice(0, 1)), ("twin_sensors", slice(0, 1))]
    return ([("repeated", slice(C - k, C))] if k else []) + out


def capon_in(v, freq, tau, dtype):
    """The Capon form restated in `dtype`: capon32 in float32, capon (double) in float64 -> float64."""
    if np.dtype(dtype) == np.float32:
        return cpc.capon32(v, freq, tau).astype(np.float64)
    return cpc.capon(v, freq, tau)


def whitener_deviations(C, dtype):
    """whiten_steps of `conditioned` without loading -> (info, max |V^H R V - I|, the deviation of 1 / power of the form fed
    that V from the float64 statement's, over the largest 1 / power)."""
    s = conditioned(C, dtype)
    freq, tau = grid(C, 1)
    v, info = cpc.whiten_steps(s, 0.0, dtype)
    ref = 1.0 / cpc.capon(cpc.whiten(s, 0.0), freq, tau)
    got = 1.0 / capon_in(v, freq, tau, dtype)
    return int(info[0]), cpc.residual(v, cpc.loaded(s, 0.0)), float(np.abs(got - ref).max() / np.abs(ref).max())
