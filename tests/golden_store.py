"""Digests of the reference's outputs, committed as tests/golden/reference_digests.npz.

The file records what the reference's own CPU kernels (oracle/_ref, built where a reference
checkout is present) returned for the exhaustive sweeps, one digest per case
(tests/golden/make_golden_digests.py), so that the sweeps pin the oracle to the reference
without that build.  A digest covers the output names and every array's dtype, shape and
bytes, with NaNs made canonical and -0.0 made +0.0, so equal digests mean equal names and
``np.array_equal(a, b, equal_nan=True)`` with equal dtype and shape for every output.
"""
import hashlib
import json
import os

import numpy as np

DIGESTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_digests.npz")


def _update(h, a):
    if a is None:
        h.update(b"None")
        return
    a = np.array(a, order="C")        # a copy
    if a.dtype.kind == "f":
        a += a.dtype.type(0)          # -0.0 -> +0.0
        a[np.isnan(a)] = np.nan       # one NaN bit pattern
    h.update(("%s%s" % (a.dtype.str, a.shape)).encode())
    h.update(a.tobytes())


def digest(outputs):
    """Digest of one array, or of a dict of named arrays (None entries included)."""
    h = hashlib.sha256()
    if isinstance(outputs, dict):
        for k in sorted(outputs):
            h.update(k.encode())
            _update(h, outputs[k])
    else:
        _update(h, outputs)
    return h.hexdigest()[:24]


def save_digests(sections):
    """sections: name -> {case name -> digest string or JSON-able record}."""
    np.savez_compressed(DIGESTS, **{s: np.array([[k, v if isinstance(v, str) else json.dumps(v)]
                                                   for k, v in sorted(cases.items())])
                                     for s, cases in sections.items()})


def load_digests(section):
    with np.load(DIGESTS) as f:
        return {k: v for k, v in f[section].tolist()}
