"""Cases of the peak-picking tests and a NumPy restatement of qi_find_peaks' and qi_peaks_select_distance's semantics
(include/qi_tfr.h) without SciPy, shared by the CPU and GPU tests and by tools/gen_golden_peaks.py."""
import warnings

import numpy as np

TILE = 256  # QI_PEAKS_TILE (test_peaks_cpu checks it against the header)
RECORDS = 3
DTYPES = ("float64", "float32")
LENGTHS = (1, 2, 3, 4, TILE - 1, TILE, TILE + 1, 3 * TILE + 17)
TYPES = ("sigmax", "sigmin", "sigabs", "log2", "log2max")
SIG_TYPES = TYPES[:3]
HEIGHTS = (None, 0.3, 0.7)
BITS_SCALINGS = ("amplitude", "log2")
BITS_THRESHOLDS = (1, 3)
BITS_DISTANCES = (1, 7, 250)
SAMPLE_RATE_HZ = 1.0  # the bits cases: time_distance_seconds = distance at 1 Hz
EPS = 2.220446049250313e-16
MARGIN = 1e-6
# scale / height codes of the C ABI
SCALE = {t: i for i, t in enumerate(TYPES)}
HEIGHT_NONE, HEIGHT_ABS, HEIGHT_BELOW_MAX, HEIGHT_BELOW_RAW_MAX = 0, 1, 2, 3
# band-passed cases: (name, band in Hz, filter order) at FS_BP, on records of BP_N samples
FS_BP = 1000.0
BP_N = 3 * TILE + 17
BP_DESIGNS = {"bp7": ((100.0, 200.0), 7), "bp3": ((10.0, 400.0), 3)}
BP_HEIGHTS = (0.3, 0.7)


def tags(dtype):
    """Input sets of a dtype: one per length, and for float32 the records in which the division itself makes a plateau
    (adjacent float32 values: not for the log2* kinds, whose cases keep unequal neighbours 1e-6 bits apart)."""
    return [f"n{n}" for n in LENGTHS] + (["div"] if dtype == "float32" else [])


def types_of(tag):
    return SIG_TYPES if tag == "div" else TYPES


def has_bits(tag):
    return tag != "div"


def x_key(dtype, tag):
    return f"{dtype}_{tag}_x"


def scaled_key(dtype, tag, kind):
    return f"{dtype}_{tag}_{kind}_scaled"


def case_ids(tag):
    """The picking cases of an input set, in the order the fixture stores them: ("ext", extraction type, height) and
    ("bits", scaling type, threshold in bits, distance in samples)."""
    ids = [("ext", kind, h) for kind in types_of(tag) for h in HEIGHTS]
    if has_bits(tag):
        ids += [("bits", s, t, d) for s in BITS_SCALINGS for t in BITS_THRESHOLDS for d in BITS_DISTANCES]
    return ids


def peaks_key(dtype, tag):
    return f"{dtype}_{tag}_peaks"


def pack(rows_of_cases):
    """One int64 array of the cases' results: per case the RECORDS counts, then the records' positions end to end."""
    out = []
    for rows in rows_of_cases:
        assert len(rows) == RECORDS
        out.append(np.asarray([len(r) for r in rows], dtype=np.int64))
        out += [np.asarray(r, dtype=np.int64) for r in rows]
    return np.concatenate(out) if out else np.zeros(0, dtype=np.int64)


def unpack(packed, ids):
    """{case id: [positions of record r]} of a pack()ed array."""
    out, at = {}, 0
    for cid in ids:
        cnt = packed[at:at + RECORDS]
        at += RECORDS
        rows = []
        for c in cnt:
            rows.append(np.asarray(packed[at:at + c], dtype=np.int64))
            at += int(c)
        out[cid] = rows
    assert at == len(packed), "the fixture does not hold exactly these cases"
    return out


def bp_ids(g, dtype):
    """The band-passed cases the fixture kept for a dtype: ("bp7" | "bp3", extraction type, height)."""
    return [(n, k, float(h)) for n, k, h in (str(c).split("|") for c in g[f"{dtype}_bp_cases"])]


def scaled_type(dtype, kind):
    return np.dtype(np.float64) if kind in ("log2", "log2max") else np.dtype(dtype)


def transform_ref(x, kind):
    """u of a record: the record itself, or log2(|x| + eps) in float64."""
    if kind in ("log2", "log2max"):
        return np.log2(np.abs(x.astype(np.float64)) + EPS)
    return x


def scale_ref(x, kind):
    """The scaled record s [n] of record x [n]."""
    u = transform_ref(x, kind)
    if kind == "log2":
        return u
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        d = {"sigmax": np.nanmax, "sigmin": np.nanmin, "log2max": np.nanmax}.get(kind, lambda v: np.nanmax(np.abs(v)))(u)
        s = u / d
    assert s.dtype == u.dtype
    return s


def local_maxima_ref(s):
    """Sample i, 1 <= i <= n - 2, opens a peak when s[i-1] < s[i]; j is the first index behind i with s[j] != s[i], at
    most n - 1; a peak when s[j] < s[i], at (i + j - 1) // 2."""
    n = len(s)
    out = []
    i = 1
    while i <= n - 2:
        if s[i - 1] < s[i]:
            j = i + 1
            while j < n - 1 and not (s[j] != s[i]):
                j += 1
            if s[j] < s[i]:
                out.append((i + j - 1) // 2)
            i = j
        else:
            i += 1
    return np.asarray(out, dtype=np.int64)


def threshold_ref(x, s, height_kind, height):
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        if height_kind == HEIGHT_ABS:
            return float(height)
        if height_kind == HEIGHT_BELOW_MAX:
            return float(np.max(s) - s.dtype.type(height))
        if height_kind == HEIGHT_BELOW_RAW_MAX:
            return float(np.max(x) - x.dtype.type(height))
    return None


def peaks_ref(x, kind, height_kind=HEIGHT_NONE, height=0.0):
    """qi_find_peaks on records x [R, n]: -> (scaled [R, n], [positions of record r], [float64 values of record r])."""
    x = np.asarray(x)
    assert x.ndim == 2 and x.dtype in (np.float32, np.float64)
    scaled = np.stack([scale_ref(row, kind) for row in x])
    positions, values = [], []
    for row, s in zip(x, scaled):
        pos = local_maxima_ref(s)
        val = s[pos].astype(np.float64)
        thr = threshold_ref(row, s, height_kind, height)
        if thr is not None:
            keep = val >= thr  # (a NaN threshold keeps nothing)
            pos, val = pos[keep], val[keep]
        positions.append(pos)
        values.append(val)
    return scaled, positions, values


def bits_ref(x, scaling, threshold):
    """The candidates of find_peaks_with_bits before the distance rule."""
    if scaling == "log2":
        return peaks_ref(x, "log2", HEIGHT_BELOW_MAX, float(threshold))
    return peaks_ref(x, "log2", HEIGHT_BELOW_RAW_MAX, float(2 ** threshold))


def select_distance_ref(positions, values, distance):
    """qi_peaks_select_distance: keep mask; from the highest value down, of equal values the later first."""
    keep = np.ones(len(positions), dtype=bool)
    order = np.argsort(values, kind="stable")
    for j in order[::-1]:
        if not keep[j]:
            continue
        k = j - 1
        while k >= 0 and positions[j] - positions[k] < distance:
            keep[k] = False
            k -= 1
        k = j + 1
        while k < len(positions) and positions[k] - positions[j] < distance:
            keep[k] = False
            k += 1
    return keep


def log2_neighbours_clear(x):
    """No adjacent log2 values of records x [R, n] that are unequal but within MARGIN bits."""
    u = np.log2(np.abs(x.astype(np.float64)) + EPS)
    with np.errstate(invalid="ignore"):
        d = np.abs(np.diff(u, axis=1))
    d = d[np.isfinite(d)]
    return not np.any((d > 0) & (d <= MARGIN))


def equal_values_within(positions, values, distance):
    """Two candidates of equal value closer than `distance` samples?"""
    for a in range(len(positions)):
        for b in range(a + 1, len(positions)):
            if positions[b] - positions[a] >= distance:
                break
            if values[a] == values[b]:
                return True
    return False
