"""Synthetic band tables for the native engines (a plain helper module: deterministic, parameters only).

Every band table the library's own host code makes is constant-Q: atom length and centre frequency are tied (w ~ 1 / f), so
the plan's thresholds on those two properties are only ever walked along one curve.  The tables here sweep them
independently, through the C ABI's own contract (include/qi_tfr.h: any host table).  Used by tests/test_gpu_tables.py (GPU),
tests/test_tables_cpu.py (CPU) and tests/sanitize/gen_tables.py (host sanitizer walk).

A Gabor table is a dict of float64 arrays p_re, p_im, omega, amp (qi_plan_set_gabor_bank); a Stockwell table a pair
(shift_index int64, sigma float64) (qi_plan_set_stx_bands).

The whole-table fallback (qi_plan_set_gabor_bank's `!native_len_ok(L) && !h_rows.empty()` branch, build_stx_tables): the
two-pass kernels run 2^20- and 2^21-point transforms only, and at any other length ONE row that needs them sends the whole
table to the hipFFT engine (but for up to four last Stockwell rows).  `split_gabor` / `split_stx` therefore cut a sweep in
two at those lengths: rows the zoom, block and split engines take, and the rest.  The rules they apply are derived from
qi_plan_build.hip in their docstrings; the plan itself (qi_plan_band_route) is the judge in the tests.
"""
import numpy as np

LN2 = np.log(2.0)
OMEGAS = (0.02, 0.3, 0.55, 0.97)  # centre frequencies, in units of pi
SHORT_ATOM = 1.0 / (2.0 * 2.75 ** 2)  # p_re above which an atom is shorter than 2.75 samples (no analytic block filter)


# ---- (a) Gabor sweep ----------------------------------------------------------------------------------------------------
def gabor_rows(reach, omega_pi, ratio=0.0):
    """Rows of reach `w` samples (exp(-p_re w^2) = 2^-30: the plan's own float32 measure of an atom's length) at centre
    frequency omega_pi * pi, with p_im = ratio * p_re and the unit-energy amplitude (2 p_re / pi)^(1/4)."""
    w = np.atleast_1d(np.asarray(reach, dtype=np.float64))
    p_re = 30.0 * LN2 / w ** 2
    return dict(p_re=p_re, p_im=ratio * p_re, omega=np.full(w.shape, omega_pi * np.pi), amp=(2.0 * p_re / np.pi) ** 0.25)


def concat(tables):
    return {k: np.concatenate([t[k] for t in tables]) for k in ("p_re", "p_im", "omega", "amp")}


def take(table, rows):
    rows = np.asarray(rows, dtype=np.int64)
    return {k: v[rows].copy() for k, v in table.items()}


def gabor_sweep(n, steps, ratios=(0.0,), omegas=OMEGAS, outside=True):
    """Reach geometric from 3 samples to 3 n in `steps` steps at each centre frequency and each p_im / p_re ratio (not
    sorted by frequency: omega is the outer loop), then -- `outside` -- six short atoms outside the analytic domain of the
    block engine (build_native_bank: p_im == 0, 0 < p_re <= 1 / (2 2.75^2), 0 < omega < pi): omega < 0, omega > pi and
    atoms shorter than 2.75 samples."""
    reach = np.geomspace(3.0, 3.0 * n, steps)
    parts = [gabor_rows(reach, om, r) for r in ratios for om in omegas]
    if outside:
        parts += [gabor_rows([40.0, 300.0], -0.3), gabor_rows([40.0, 300.0], 1.2),
                  dict(p_re=np.array([2.0 * SHORT_ATOM, 4.0 * SHORT_ATOM]), p_im=np.zeros(2), omega=np.array([0.3, 0.8]) * np.pi,
                       amp=np.ones(2))]
    return concat(parts)


def in_analytic_domain(table):
    return (table["p_im"] == 0.0) & (table["p_re"] <= SHORT_ATOM) & (table["omega"] > 0.0) & (table["omega"] < np.pi)


def split_gabor(table, n, f64):
    """(rows for the zoom / block / split engines, the rest) of a styx-bank table at a record length without two-pass
    kernels.  From build_native_bank, for pure Gaussians (p_im == 0):
      * reach <= 1024 samples: the block engine -- float32 any atom (a non-analytic one reads its bank row), float64
        Gaussians inside (0, pi) only (analytic 1 or 2); a float64 atom outside goes to the short-atom table, which exists
        at 2^20 / 2^21 only -> the rest;
      * longer, not cut by the record: spectrum support 2 sqrt(4 p_re bits ln 2) L / 2 pi < L / 16 bins (reach > 1024 ->
        < 3000 of 131 072 bins at 2^16), which every zoom grid from level 1 oversamples four times -> zoom;
      * cut by the record (p_re n^2 / 4 <= bits ln 2): a split band, the tapered spectrum being as narrow.
    A chirped row (p_im != 0) is wider by sqrt(1 + ratio^2) and its cut form has no compact tapered spectrum: the rest.
    float64 keeps the block rows only: the support analysis there keeps every bin above 2^-50 of the peak, and the rounding
    of the atom's own phase omega x (up to 1e5 rad at these lengths) leaves a floor of 2^-51 .. 2^-54 of the peak over the
    WHOLE row of an atom longer than the block engine's 1024 samples (NumPy, n = 2^16: reach 1200 at 0.3 pi 2^-53.7 with
    3364 bins above 2^-50 spread over the row; reach 2000 at 0.97 pi 2^-51.3; reach 20000 at 0.55 pi 2^-51.8; only the
    lowest centre frequency stays compact, 2^-56.5 at 0.02 pi) -- a constant-Q table never has such an atom (omega x stays
    a few cycles).  The plan then sees a full-row support and hands the band to the two-pass kernels, i.e. the rest."""
    pure = table["p_im"] == 0.0
    if f64:
        reach = np.ceil(np.sqrt(52.0 * LN2 / table["p_re"])) + 1.0
        ok = pure & (table["omega"] > 0.0) & (table["omega"] < np.pi) & (reach <= 1024.0)
    else:  # an atom outside the analytic domain is a block row read from the bank as long as it reaches <= 1024 samples
        reach = np.ceil(np.sqrt(30.0 * LN2 / table["p_re"])) + 1.0
        ok = pure & (in_analytic_domain(table) | (reach <= 1024.0))
    rows = np.arange(len(pure))
    return rows[ok], rows[~ok]


# ---- (b) Stockwell sweep ------------------------------------------------------------------------------------------------
def stx_shifts(n):
    return (1, 3, n // 64, n // 4, n // 2 - n // 64, n // 2 - 1)


def stx_sweep(n, widths, order="ascending", sigma_lo=1.0):
    """sigma geometric from sigma_lo to n / 4 samples in `widths` steps at each of six shift indices (windows cut at
    Nyquist and windows that reach across bin 0).  order: "ascending" (by shift index, then sigma), "shuffled" (a fixed
    permutation) or "duplicates" (ascending with rows 1 and B // 2 repeated at the end)."""
    sig = np.geomspace(sigma_lo, n / 4.0, widths)
    idx = np.repeat(np.array(stx_shifts(n), dtype=np.int64), widths)
    sigma = np.tile(sig, 6)
    if order == "shuffled":
        perm = shuffle_permutation(len(idx))
        return idx[perm], sigma[perm]
    if order == "duplicates":
        dup = [1, len(idx) // 2]
        return np.concatenate([idx, idx[dup]]), np.concatenate([sigma, sigma[dup]])
    assert order == "ascending", order
    return idx, sigma


def shuffle_permutation(count):
    return np.random.default_rng(20240607).permutation(count)


def split_stx(idx, sigma, n):
    """(rows for the zoom / block engines, the rest) at a record length without two-pass kernels.  From build_stx_tables:
    sigma >= 2.75 and reach sqrt(60 ln 2) sigma <= 1024 (float64: sqrt(104 ln 2)) -> block; a longer window has
    2 floor(sqrt(30) / coef) + 1 < n / 16 occupied bins -> zoom on some grid; sigma < 2.75 is neither (its frequency window
    has not decayed before Nyquist: more than n / 16 bins) -> two-pass, i.e. the rest."""
    rows = np.arange(len(sigma))
    ok = np.asarray(sigma) >= 2.75
    return rows[ok], rows[~ok]


# ---- (c) population tables ----------------------------------------------------------------------------------------------
def join_zoom_classes(counts):
    """upload_native_table's join rule on per-class band counts [7] -> counts after the joins: class 6 (< 6 bands) joins 5,
    class 5 (< 6) joins 0, a level (< 6) joins the next occupied level at most two up."""
    c = list(counts)
    if 0 < c[6] < 6:
        c[5], c[6] = c[5] + c[6], 0
    if 0 < c[5] < 6:
        c[0], c[5] = c[0] + c[5], 0
    for g in range(4):
        if c[g] == 0 or c[g] >= 6:
            continue
        for h in (g + 1, g + 2):
            if h < 5 and c[h] > 0:
                c[h], c[g] = c[h] + c[g], 0
                break
    return c


def join_fine_classes(counts):
    """upload_native_table's rule for the float64 zoom's fine classes of the coarsest grid, on band counts [6] (index 0:
    the 16-tap class, 1: the second grid -- untouched --, 2..5: the 12- / 10- / 8- / 6-tap classes): from the shortest
    interpolator down, a class of fewer than four bands joins the next longer one (class 2 the 16-tap class)."""
    c = list(counts)
    for q in (5, 4, 3, 2):
        if 0 < c[q] < 4:
            to = 0 if q == 2 else q - 1
            c[to], c[q] = c[to] + c[q], 0
    return c


# tfr_stx_fft's keyword sets at n_fft = 2^16 (the fixture tests/golden/stx_general_n65536.npz holds the reference's rows of each)
GENERAL_SETS = {
    "lin": dict(frequency_min=20.0, frequency_max=400.0, frequency_step=20.0),
    "geo": dict(scale_order_input=3.0, frequency_min=10.0, frequency_max=450.0, is_geometric=True),
    "inferno": dict(scale_order_input=3.0, frequency_min=8.0, frequency_max=400.0, is_geometric=True, is_inferno=True),
    "qpr": dict(frequency_min=25.0, frequency_max=300.0, frequency_step=25.0, factor_q=0.5, power_p=1.0, power_r=0.75),
    "const_width": dict(frequency_min=5.0, frequency_max=495.0, frequency_step=10.0, power_r=0.0),
    "q2p1": dict(frequency_min=2.0, frequency_max=480.0, frequency_step=6.0, factor_q=2.0, power_p=1.0),
    "short_windows": dict(scale_order_input=2.0, frequency_min=100.0, frequency_max=480.0, frequency_step=20.0),
}


def stx_two_pass_population(n, k, where, natives=24):
    """A Stockwell table of `natives` block / zoom rows (sigma >= 2.75) and k rows that need the two-pass kernels
    (sigma < 2.75), placed "last" or in the "middle"."""
    idx, sigma = stx_sweep(n, natives // 6, sigma_lo=3.0)
    hard_idx = np.array([n // 4, n // 8, n // 3, n // 2 - 5, n // 5][:k], dtype=np.int64)
    hard_sigma = np.array([1.0, 1.5, 2.0, 2.5, 1.2][:k])
    at = len(idx) if where == "last" else len(idx) // 2
    return np.insert(idx, at, hard_idx), np.insert(sigma, at, hard_sigma)


def single_band(kind, n):
    """B = 1 Gabor tables: "zoom" (a long atom inside the record), "block" (a short one), "split" (cut by the record)."""
    reach = {"zoom": n / 8.0, "block": 100.0, "split": 2.0 * n}[kind]
    return gabor_rows([reach], 0.3)


def single_stx_band(kind, n):
    """B = 1 Stockwell tables: "zoom" (a window of n / 64 samples) and "block" (20 samples) at shift index n / 4."""
    return np.array([n // 4], dtype=np.int64), np.array([{"zoom": n / 64.0, "block": 20.0}[kind]])


# ---- (d) a large linear Stockwell table ---------------------------------------------------------------------------------
def linear_stx_table(n, fs=1000.0, count=2000, order=8.0):
    """About `count` bands by tfr_stx_fft's linear rule (frequency_step), with frequency_max low enough that no window is
    shorter than 2.75 samples: sigma = (12 / 5) order / omega >= 2.75 <-> f <= fs (12 / 5) order / (2 pi 2.75)... capped
    at 0.45 fs."""
    from quantum_inferno_amd import styx_stx

    f_max = min(0.45 * fs, fs * 2.4 * order / (2 * np.pi * 2.75) * 0.98)
    f_min = 4.0 * 2.4 * order * fs / n
    f, idx, sigma, _, _ = styx_stx.stx_general_table(n, 1.0 / fs, order, f_min, f_max, (f_max - f_min) / count)
    return f, idx, sigma


# ---- single-precision restatement (the arithmetic floor of the float32 engines) -----------------------------------------
def gabor_table_fft32(sig32, table, bands=None, circular=False):
    """oracle.gabor_table_fft with the record, the atom and every transform in single precision (scipy.fft on float32 /
    complex64): what the same algorithm gives without any float64 step but the atom's formula."""
    import scipy.fft as sf

    n = len(sig32)
    x = np.arange(n, dtype=np.float64) - (n - 1) / 2.0
    spec = sf.fft(np.asarray(sig32, dtype=np.float32), n if circular else 2 * n)
    assert spec.dtype == np.complex64
    rows = range(len(table["p_re"])) if bands is None else bands
    out = np.empty((len(rows), n), dtype=np.complex64)
    start = (n - 1) // 2
    for i, j in enumerate(rows):
        atom = table["amp"][j] * np.exp(-(table["p_re"][j] + 1j * table["p_im"][j]) * x * x) * np.exp(1j * table["omega"][j] * x)
        if circular:
            raw = sf.ifft(spec * np.conj(sf.fft(atom.astype(np.complex64))))
            out[i] = np.append(raw[n // 2 :], raw[: n // 2])
        else:
            out[i] = sf.ifft(spec * sf.fft(np.conj(atom[::-1]).astype(np.complex64), 2 * n))[start : start + n]
    return out


def stx_table_fft32(sig32, idx, sigma, bands=None):
    import scipy.fft as sf

    n = len(sig32)
    spec = sf.fft(np.asarray(sig32, dtype=np.float32))
    cat = np.concatenate([spec, spec])
    om = 2 * np.pi * np.fft.fftfreq(n)
    rows = range(len(sigma)) if bands is None else bands
    out = np.empty((len(rows), n), dtype=np.complex64)
    for i, j in enumerate(rows):
        out[i] = sf.ifft(cat[idx[j] : idx[j] + n] * np.exp(-0.5 * sigma[j] ** 2 * om ** 2).astype(np.float32))
    return out


# ---- the tables the tests use, by name ----------------------------------------------------------------------------------
def gabor_cases():
    """(name, log2n, f64, bank, table, expect) of every Gabor table of the suite.  expect: "native" (no row on the hipFFT
    engine) or "fallback" (the whole table).  Steps per length keep one stored panel, the hipFFT engine's panel and bank of
    the same table and the plan's scratch (TfrPlan.workspace_for: one full-length row per band) within ~25 GB together."""
    out = []
    for log2n, steps in ((16, 60), (17, 60)):
        n = 1 << log2n
        full = gabor_sweep(n, steps)
        for f64 in (False, True):
            if f64 and log2n == 17:
                continue
            nat, rest = split_gabor(full, n, f64)
            tag = f"{'f64' if f64 else 'f32'}_2^{log2n}"
            out.append((f"styx_sweep_{tag}", log2n, f64, 0, take(full, nat), "native"))
            if len(rest):
                out.append((f"styx_sweep_rest_{tag}", log2n, f64, 0, take(full, rest), "fallback"))
        # chirped rows at a length without two-pass kernels, float32, with the pure rows of one centre frequency.  Three rows
        # of reach 1100 .. 1300 at ratio 3: past the block engine's 1024 samples, with a spectrum sqrt(10) wider than a
        # Gaussian's (L / 32 .. L / 16 bins) -- the finest zoom grid, level 4, which no pure Gaussian reaches
        chirped = concat([gabor_sweep(n, 12, ratios=(3.0, -2.0), omegas=(0.3, 0.55), outside=False),
                          gabor_rows(np.geomspace(3, 3 * n, 12), 0.3), gabor_rows([1100.0, 1200.0, 1300.0], 0.3, 3.0)])
        out.append((f"styx_chirped_f32_2^{log2n}", log2n, False, 0, chirped, "native"))
    # 2^20: the two-pass kernels exist, every table runs on the native engines -- the chirped rows belong here (ratio 3 at
    # two centre frequencies, one negative ratio); fewer steps in float64 (one stored panel and the hipFFT engine's bank
    # of the same table stay within a few GB)
    n = 1 << 20
    for f64, steps in ((False, 40), (True, 16)):
        tag = "f64" if f64 else "f32"
        for bank, name in ((0, "styx"), (1, "atoms")):
            reach = np.geomspace(3.0, 3.0 * n, steps)
            chirped = [gabor_rows(reach, 0.3, 3.0), gabor_rows(reach, 0.55, 3.0), gabor_rows(reach, 0.55, -2.0)]
            out.append((f"{name}_sweep_{tag}_2^20", 20, f64, bank, concat([gabor_sweep(n, steps)] + chirped), "native"))
    # the atoms bank at its other native length
    n = 1 << 21
    reach = np.geomspace(3.0, 3.0 * n, 10)
    out.append(("atoms_sweep_f32_2^21", 21, False, 1, concat([gabor_sweep(n, 10), gabor_rows(reach, 0.55, 3.0), gabor_rows(reach, 0.3, -2.0)]),
                "native"))
    return out


def stx_cases():
    """(name, log2n, f64, (idx, sigma), expect) of every Stockwell sweep table (ascending order)."""
    out = []
    for log2n, widths in ((16, 80), (20, 48)):
        n = 1 << log2n
        idx, sigma = stx_sweep(n, widths)
        for f64 in (False, True):
            tag = f"{'f64' if f64 else 'f32'}_2^{log2n}"
            if log2n == 20:
                out.append((f"stx_sweep_{tag}", log2n, f64, (idx, sigma), "native"))
            else:
                nat, rest = split_stx(idx, sigma, n)
                out.append((f"stx_sweep_{tag}", log2n, f64, (idx[nat], sigma[nat]), "native"))
                out.append((f"stx_sweep_rest_{tag}", log2n, f64, (idx[rest], sigma[rest]), "fallback"))
    return out
