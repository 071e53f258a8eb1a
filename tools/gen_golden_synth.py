"""Generator of tests/golden/synth.npz -- TEST INFRASTRUCTURE, run where the reference package is installed or checked out
(QI_REFERENCE names its directory) and SciPy is.  Runs the reference's synth modules on the cases of tests/synth_cases.py and
stores only data: the arrays they return; what they hand to scipy.signal.decimate and scipy.signal.filtfilt (those two calls
are wrapped for the run); and, where noise is drawn, the result of a run in which np.random.normal(loc, scale, size) is
replaced by loc + scale * z for the seeded standard-normal z that synth_cases.normal rebuilds -- so the same z goes into the
port as `noise=`; and the lines each call prints.  Inputs are rebuilt from seeds and not stored; nothing of the reference itself is copied.

    python tools/gen_golden_synth.py

The generator asserts what the tests rely on: every restatement of tests/synth_cases.py equals the reference's arrays bit for
bit (the waveforms before decimation and before the filter, the GT family, all three doppler outputs)."""
import contextlib
import io
import os
import sys

import numpy as np
import scipy
import scipy.signal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
if os.environ.get("QI_REFERENCE"):
    sys.path.insert(0, os.environ["QI_REFERENCE"])

from quantum_inferno.synth import benchmark_signals, blast_gt_pulse, doppler, synthetic_signals  # noqa: E402

import synth_cases as sc  # noqa: E402

MODULES = {"benchmark_signals": benchmark_signals, "synthetic_signals": synthetic_signals, "blast_gt_pulse": blast_gt_pulse,
           "doppler": doppler}


@contextlib.contextmanager
def captured(key):
    """Wrap scipy.signal.decimate and filtfilt (record their input) and np.random.normal (loc + scale * seeded z)."""
    seen = {"decimate": [], "filtfilt": []}
    decimate, filtfilt, normal = scipy.signal.decimate, scipy.signal.filtfilt, np.random.normal

    def wrapped_decimate(x, q, *args, **kwargs):
        seen["decimate"].append(np.array(x))
        return decimate(x, q, *args, **kwargs)

    def wrapped_filtfilt(b, a, x, *args, **kwargs):
        seen["filtfilt"].append(np.array(x))
        return filtfilt(b, a, x, *args, **kwargs)

    def seeded_normal(loc=0.0, scale=1.0, size=None):
        return loc + scale * sc.normal(key, size)

    scipy.signal.decimate, scipy.signal.filtfilt, np.random.normal = wrapped_decimate, wrapped_filtfilt, seeded_normal
    try:
        yield seen
    finally:
        scipy.signal.decimate, scipy.signal.filtfilt, np.random.normal = decimate, filtfilt, normal


def main():
    out = {}
    np.seterr(all="ignore")
    for key, module, name, kwargs in sc.WRAPPER_CASES:
        printed = io.StringIO()
        with captured(key) as seen, contextlib.redirect_stdout(printed):
            got = getattr(MODULES[module], name)(**sc.wrapper_kwargs(kwargs))
        out[f"{key}_printed"] = np.array(printed.getvalue().splitlines(), dtype=str)
        for i, part in enumerate(got if isinstance(got, tuple) else (got,)):
            out[f"{key}_out{i}"] = np.asarray(part)
        for what, arrays in seen.items():
            for i, x in enumerate(arrays):
                out[f"{key}_{what}{i}"] = x
    t = sc.gt_times()
    for key, name, period in sc.GT_CASES:
        out[key] = getattr(blast_gt_pulse, name)(t.copy(), period)
    for key, module, name, args in sc.HOST_CASES:
        got = getattr(MODULES[module], name)(*args)
        for i, part in enumerate(got if isinstance(got, tuple) else (got,)):
            out[f"host_{key}_{i}"] = np.asarray(part)
    for key, n, inverse, geometry, times, images in sc.doppler_cases():
        fn = doppler.doppler_inverse if inverse else doppler.doppler_forward
        c, vs, vr, s0, s1, r0, r1 = geometry
        for image in images:
            f = (doppler.image_doppler_inverse if inverse else doppler.image_doppler_forward) if image else fn
            got = f(times.copy(), c, vs, vr, 3, s0, s1, r0, r1)
            for i, part in enumerate(got):
                out[f"doppler_{key}_{int(image)}_{i}"] = part
    path = os.path.join(ROOT, "tests", "golden", "synth.npz")
    np.savez_compressed(path, versions=np.array([np.__version__, scipy.__version__, "quantum-inferno 1.1.3"]), **out)
    print(f"{path}: {os.path.getsize(path) / 1e6:.3f} MB, {len(out)} arrays")
    failures = sc.restatement_failures(np.load(path, allow_pickle=False))
    assert not failures, failures
    print("every restatement equals the reference bit for bit")


if __name__ == "__main__":
    main()
