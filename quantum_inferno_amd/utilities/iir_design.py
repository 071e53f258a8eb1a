"""Butterworth design and zero-phase set-up on the host, NumPy only: what the reference takes from SciPy for
styx_fft.butter_* (styx_fft.py:60-149: signal.butter(output="ba") + signal.filtfilt) and utilities.picker.apply_bandpass
(picker.py:56-76: butter(output="sos") + sosfiltfilt), restated operation by operation so that the tables come out as
SciPy's bits: analog prototype, pre-warp, band transform and bilinear transform on (zeros, poles, gain), then the
polynomial coefficients or the second-order sections in SciPy's default pairing ("nearest").  The filter itself runs on
the device (engine.zero_phase_filter, qi_filtfilt).  The same steps from the Chebyshev type I prototype give the sections of
scipy.signal.decimate's anti-alias filter (utilities.sampling.decimate_*: cheby1_sos, decimator; engine.zero_phase_decimate,
qi_decimate), in float64 or cast to float32 as SciPy casts them for a float32 record."""
import numpy as np

BTYPES = ("lowpass", "highpass", "bandpass")


def _check_design(order, wn, btype):
    """-> (order, wn [1] or [2]) of a digital design request; wn in units of Nyquist."""
    if btype not in BTYPES:
        raise ValueError(f"btype must be one of {BTYPES}, got {btype!r}")
    if int(order) != order or order < 1:
        raise ValueError(f"filter order must be a positive integer, got {order!r}")
    order = int(order)
    wn = np.atleast_1d(np.asarray(wn, dtype=np.float64))
    if wn.ndim != 1 or wn.size != (2 if btype == "bandpass" else 1):
        raise ValueError(f"{btype}: wn must hold {2 if btype == 'bandpass' else 1} critical frequencies, got {wn!r}")
    if np.any(wn <= 0) or np.any(wn >= 1):
        raise ValueError("Digital filter critical frequencies must be 0 < Wn < 1")
    if wn.size > 1 and not wn[0] < wn[1]:
        raise ValueError("Wn[0] must be less than Wn[1]")
    return order, wn


def _butter_zpk(order, wn, btype):
    """Digital Butterworth (zeros, poles, gain); wn in units of Nyquist."""
    order, wn = _check_design(order, wn, btype)
    # analog prototype: poles on the unit circle, the middle one exactly real
    m = np.arange(-order + 1, order, 2)
    p = -np.exp(1j * np.pi * m / (2 * order))
    return _to_digital(np.array([]), p, 1, wn, btype)


def _cheby1_zpk(order, rp, wn, btype):
    """Digital Chebyshev type I (zeros, poles, gain) with rp decibels of pass-band ripple; wn in units of Nyquist."""
    order, wn = _check_design(order, wn, btype)
    # analog prototype (scipy.signal.cheb1ap): poles on an ellipse, an even order has a DC gain of -rp dB
    eps = np.sqrt(10 ** (0.1 * rp) - 1.0)
    mu = 1.0 / order * np.arcsinh(1 / eps)
    m = np.arange(-order + 1, order, 2)
    theta = np.pi * m / (2 * order)
    p = -np.sinh(mu + 1j * theta)
    k = np.prod(-p, axis=0).real
    if order % 2 == 0:
        k = k / np.sqrt(1 + eps * eps)
    return _to_digital(np.array([]), p, k, wn, btype)


def _to_digital(z, p, k, wn, btype):
    """An analog low-pass prototype (cut-off 1 rad/s) -> the digital filter of the band wn: pre-warp, band transform, bilinear."""
    fs = 2.0
    warped = 2 * fs * np.tan(np.pi * wn / fs)
    degree = len(p) - len(z)
    if btype == "lowpass":
        wo = float(warped[0])
        z, p, k = wo * z, wo * p, k * wo ** degree
    elif btype == "highpass":
        wo = float(warped[0])
        k = k * np.real(np.prod(-z) / np.prod(-p))
        z, p = np.append(wo / z, np.zeros(degree)), wo / p
    else:
        bw = float(warped[1] - warped[0])
        wo = float(np.sqrt(warped[0] * warped[1]))
        z_lp = (z * bw / 2).astype(complex)
        p_lp = (p * bw / 2).astype(complex)
        z = np.concatenate((z_lp + np.sqrt(z_lp ** 2 - wo ** 2), z_lp - np.sqrt(z_lp ** 2 - wo ** 2)))
        p = np.concatenate((p_lp + np.sqrt(p_lp ** 2 - wo ** 2), p_lp - np.sqrt(p_lp ** 2 - wo ** 2)))
        z = np.append(z, np.zeros(degree))
        k = k * bw ** degree
    # bilinear transform; the zeros at infinity move to Nyquist
    degree = len(p) - len(z)
    fs2 = 2.0 * fs
    k = k * np.real(np.prod(fs2 - z) / np.prod(fs2 - p))
    z = np.append((fs2 + z) / (fs2 - z), -np.ones(degree))
    p = (fs2 + p) / (fs2 - p)
    return z, p, k


def _real_if_conjugate(coef, roots):
    """np.poly's rule, as zpk2tf repeats it: complex coefficients of conjugate root pairs are real."""
    if issubclass(coef.dtype.type, np.complexfloating):
        roots = np.asarray(roots, complex)
        pos = np.compress(roots.imag > 0, roots)
        neg = np.conjugate(np.compress(roots.imag < 0, roots))
        if len(pos) == len(neg) and np.all(np.sort_complex(neg) == np.sort_complex(pos)):
            coef = coef.real.copy()
    return coef


def _zpk2tf(z, p, k):
    z = np.atleast_1d(z)
    k = np.atleast_1d(k)
    b = k * np.poly(z)
    a = np.atleast_1d(np.poly(p))
    return _real_if_conjugate(b, z), _real_if_conjugate(a, p)


def butter_ba(order, wn, btype):
    """(b, a) of scipy.signal.butter(order, wn, btype), wn in units of Nyquist."""
    return _zpk2tf(*_butter_zpk(order, wn, btype))


def _cplxreal(z):
    """One member (positive imaginary part) of every conjugate pair, and the real values, both sorted."""
    z = np.atleast_1d(z)
    if z.size == 0:
        return z, z
    tol = 100 * np.finfo((1.0 * z).dtype).eps
    z = z[np.lexsort((abs(z.imag), z.real))]
    real_indices = abs(z.imag) <= tol * abs(z)
    zr = z[real_indices].real
    if len(zr) == len(z):
        return np.array([]), zr
    z = z[~real_indices]
    zp = z[z.imag > 0]
    zn = z[z.imag < 0]
    if len(zp) != len(zn):
        raise ValueError("Array contains complex value with no matching conjugate.")
    same_real = np.diff(zp.real) <= tol * abs(zp[:-1])
    diffs = np.diff(np.concatenate(([0], same_real, [0])))
    run_starts = np.nonzero(diffs > 0)[0]
    run_stops = np.nonzero(diffs < 0)[0]
    for start, stop in zip(run_starts, run_stops + 1):
        for chunk in (zp[start:stop], zn[start:stop]):
            chunk[...] = chunk[np.lexsort([abs(chunk.imag)])]
    if any(abs(zp - zn.conj()) > tol * abs(zn)):
        raise ValueError("Array contains complex value with no matching conjugate.")
    return (zp + zn.conj()) / 2, zr


def _nearest(fro, to, which):
    order = np.argsort(np.abs(fro - to))
    if which == "any":
        return order[0]
    mask = np.isreal(fro[order])
    if which == "complex":
        mask = ~mask
    return order[np.nonzero(mask)[0][0]]


def _section(z, p):
    sos = np.zeros(6)
    b, a = _zpk2tf(z, p, 1)
    sos[3 - len(b):3] = b
    sos[6 - len(a):6] = a
    return sos


def _zpk2sos(z, p, k):
    """Digital second-order sections, pairing "nearest": the pole nearest the unit circle goes last, each with the zero nearest to it."""
    if len(z) == len(p) == 0:
        return np.array([[k, 0.0, 0.0, 1.0, 0.0, 0.0]])
    p = np.concatenate((p, np.zeros(max(len(z) - len(p), 0))))
    z = np.concatenate((z, np.zeros(max(len(p) - len(z), 0))))
    n_sections = (max(len(p), len(z)) + 1) // 2
    if len(p) % 2 == 1:
        p = np.concatenate((p, [0.0]))
        z = np.concatenate((z, [0.0]))
    z = np.concatenate(_cplxreal(z))
    p = np.concatenate(_cplxreal(p))
    if not np.isreal(k):
        raise ValueError("k must be real")
    k = k.real

    def idx_worst(q):
        return np.argmin(np.abs(1 - np.abs(q)))

    sos = np.zeros((n_sections, 6))
    for si in range(n_sections - 1, -1, -1):
        p1_idx = idx_worst(p)
        p1 = p[p1_idx]
        p = np.delete(p, p1_idx)
        if np.isreal(p1) and np.isreal(p).sum() == 0:  # the last real pole
            z1_idx = _nearest(z, p1, "real")
            z1 = z[z1_idx]
            z = np.delete(z, z1_idx)
            sos[si] = _section([z1, 0], [p1, 0])
        elif len(p) + 1 == len(z) and not np.isreal(p1) and np.isreal(p).sum() == 1 and np.isreal(z).sum() == 1:
            # one real pole and one real zero are left: this complex pole takes a complex zero
            z1_idx = _nearest(z, p1, "complex")
            z1 = z[z1_idx]
            z = np.delete(z, z1_idx)
            sos[si] = _section([z1, z1.conj()], [p1, p1.conj()])
        else:
            if np.isreal(p1):
                prealidx = np.flatnonzero(np.isreal(p))
                p2_idx = prealidx[idx_worst(p[prealidx])]
                p2 = p[p2_idx]
                p = np.delete(p, p2_idx)
            else:
                p2 = p1.conj()
            if len(z) > 0:
                z1_idx = _nearest(z, p1, "any")
                z1 = z[z1_idx]
                z = np.delete(z, z1_idx)
                if not np.isreal(z1):
                    sos[si] = _section([z1, z1.conj()], [p1, p2])
                elif len(z) > 0:
                    z2_idx = _nearest(z, p1, "real")
                    z2 = z[z2_idx]
                    z = np.delete(z, z2_idx)
                    sos[si] = _section([z1, z2], [p1, p2])
                else:
                    sos[si] = _section([z1], [p1, p2])
            else:
                sos[si] = _section([], [p1, p2])
    assert len(p) == len(z) == 0
    sos[0][:3] *= k
    return sos


def butter_sos(order, wn, btype):
    """scipy.signal.butter(order, wn, btype, output="sos"): [sections][6] = b0 b1 b2 1 a1 a2, wn in units of Nyquist."""
    return _zpk2sos(*_butter_zpk(order, wn, btype))


def cheby1_sos(order, rp, wn, btype="lowpass"):
    """scipy.signal.cheby1(order, rp, wn, btype, output="sos"): [sections][6] = b0 b1 b2 1 a1 a2, wn in units of Nyquist."""
    return _zpk2sos(*_cheby1_zpk(order, rp, wn, btype))


DECIMATE_ORDER, DECIMATE_RIPPLE_DB = 8, 0.05  # scipy.signal.decimate's defaults for ftype="iir", which the reference keeps


def decimator(q, dtype=np.float64):
    """(sos, zi, edge) of scipy.signal.decimate(x, q, zero_phase=True) for records of `dtype` (float32 or float64): the
    order-8 Chebyshev type I low-pass of 0.05 dB ripple at 0.8 / q of Nyquist, designed in float64 and cast to the
    records' type as SciPy casts it; zi evaluated in that type; edge = 27 samples of extension (4 sections)."""
    dtype = np.dtype(dtype)
    if dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise TypeError(f"records are filtered in float32 or float64, got {dtype}")
    sos = np.asarray(cheby1_sos(DECIMATE_ORDER, DECIMATE_RIPPLE_DB, 0.8 / q), dtype=dtype)
    return sos, sosfilt_zi(sos), sosfiltfilt_edge(sos)


def lfilter_zi(b, a):
    """Steady-state delays of the transposed direct form II for a unit step (scipy.signal.lfilter_zi)."""
    b = np.atleast_1d(b)
    a = np.atleast_1d(a)
    if b.ndim != 1 or a.ndim != 1:
        raise ValueError("b and a must be 1-D")
    while len(a) > 1 and a[0] == 0.0:
        a = a[1:]
    if a.size < 1:
        raise ValueError("There must be at least one nonzero `a` coefficient.")
    if a[0] != 1.0:
        b = b / a[0]
        a = a / a[0]
    n = max(len(a), len(b))
    if len(a) < n:
        a = np.r_[a, np.zeros(n - len(a), dtype=a.dtype)]
    elif len(b) < n:
        b = np.r_[b, np.zeros(n - len(b), dtype=b.dtype)]
    companion = np.zeros((n - 1, n - 1), dtype=np.result_type(a, b))
    companion[0] = -a[1:] / (1.0 * a[0])
    companion[list(range(1, n - 1)), list(range(0, n - 2))] = 1
    i_minus_a = np.eye(n - 1, dtype=np.result_type(a, b)) - companion.T
    return np.linalg.solve(i_minus_a, b[1:] - a[1:] * b[0])


def sosfilt_zi(sos):
    """scipy.signal.sosfilt_zi: [sections][2], in the sections' type (float32 sections give SciPy's float32 values)."""
    sos = _validate_sos(sos)
    zi = np.empty((sos.shape[0], 2), dtype=sos.dtype)
    scale = 1.0
    for section in range(sos.shape[0]):
        b = sos[section, :3]
        a = sos[section, 3:]
        zi[section] = scale * lfilter_zi(b, a)
        scale *= b.sum() / a.sum()
    return zi


def _validate_sos(sos):
    sos = np.asarray(sos)
    sos = np.atleast_2d(sos if sos.dtype == np.float32 else sos.astype(np.float64))  # float32 sections are not widened
    if sos.ndim != 2 or sos.shape[1] != 6:
        raise ValueError("sos array must be shape (n_sections, 6)")
    if not (sos[:, 3] == 1).all():
        raise ValueError("sos[:, 3] should be all ones")
    return sos


def filtfilt_edge(b, a):
    """Samples scipy.signal.filtfilt extends a record by at each end (its default padlen)."""
    return 3 * max(len(a), len(b))


def sosfiltfilt_edge(sos):
    """The same for scipy.signal.sosfiltfilt."""
    sos = _validate_sos(sos)
    return 3 * int(2 * sos.shape[0] + 1 - min((sos[:, 2] == 0).sum(), (sos[:, 5] == 0).sum()))


def check_length(n, edge):
    """A record must be longer than the extension, as SciPy requires."""
    if n <= edge:
        raise ValueError(f"The length of the input vector x must be greater than padlen, which is {edge}.")
