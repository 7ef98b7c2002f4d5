"""The compiled reference's answers to the checks of test_oracle_vs_reference.py and test_reference_parser.py, stored so that those
checks run in every checkout, not only where the reference can be built (oracle/_ref).

tests/golden/reference_records.json holds JSON values: digests of the reference's arrays where a check compares bit for bit,
small values (parsed fields, flags) as they are. tests/golden/reference_arrays.npz holds the arrays a check compares with a
tolerance. Where oracle/_ref was built the reference is asked live as well, and its answer must be the stored one.
`python oracle/make_golden.py --records` rewrites both files from oracle/_ref."""
import atexit
import hashlib
import json
import os

import numpy as np
import pytest

import oracle_py as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RECORDS_JSON = os.path.join(GOLDEN, "reference_records.json")
ARRAYS_NPZ = os.path.join(GOLDEN, "reference_arrays.npz")
RECORDING = os.environ.get("DRT_RECORD_REFERENCE") == "1"  # set by oracle/make_golden.py --records

# recording starts from nothing, so that answers no check asks for any more are dropped
_records = json.load(open(RECORDS_JSON)) if os.path.exists(RECORDS_JSON) and not RECORDING else {}
_arrays = dict(np.load(ARRAYS_NPZ, allow_pickle=False)) if os.path.exists(ARRAYS_NPZ) and not RECORDING else {}


def digest(*arrays):
    """sha256 of the arrays' shapes and values. Two equal digests mean np.array_equal(a, b, equal_nan=True) for each pair:
    NaN equals NaN whatever its payload, -0 equals 0, and an int32 array equals the same numbers in int64."""
    h = hashlib.sha256()
    for a in arrays:
        a = np.asarray(a)
        if a.dtype.kind == "f":
            a = a.astype(np.float64)
            a = np.where(np.isnan(a), np.nan, a + 0.0)  # one NaN bit pattern; -0 + 0 is +0
        else:
            a = a.astype(np.int64)
        h.update(repr(a.shape).encode())
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:32]


def _missing(key):
    return "no stored reference answer for %r: python oracle/make_golden.py --records" % key


def scene_digest(bundle):
    """digest of what the host loader computed for a scene: its SPD block and its camera. Black bodies and the camera go through
    x87 expl / powl / tanl, whose last bits can differ from one CPU to another."""
    return digest(bundle.spds(), np.frombuffer(bytes(bundle.camera), dtype=np.float64))


def reference(key, live, bundle=None):
    """The reference's answer for `key`, a JSON value: live() where oracle/_ref was built (it must equal the stored answer),
    the stored answer elsewhere. With `bundle`, the answer is for that scene as the host loader built it where the answer was
    recorded: if this machine's host built other bits (scene_digest), the stored answer does not apply -- the live one is
    used where there is one, and the check is skipped where there is none."""
    scene = None if bundle is None else scene_digest(bundle)
    if scene is not None and key in _records and not RECORDING and _records[key].get("scene") != scene:
        if not O.ref_available():
            pytest.skip("the host built %r with other last bits on this CPU than where the reference's answer was recorded" % key)
        return json.loads(json.dumps(live()))
    if not O.ref_available():
        assert key in _records, _missing(key)
        return _records[key]
    got = json.loads(json.dumps(live()))
    if scene is not None:
        got["scene"] = scene
    if RECORDING:
        _records[key] = got
    else:
        assert key in _records, _missing(key)
        assert json.dumps(got, sort_keys=True) == json.dumps(_records[key], sort_keys=True), \
            "the reference's answer for %r is not the stored one: python oracle/make_golden.py --records" % key
    return got


def reference_array(key, live):
    """reference() for an array (float64), stored whole in reference_arrays.npz; live answers must equal it bit for bit."""
    if not O.ref_available():
        assert key in _arrays, _missing(key)
        return _arrays[key]
    got = np.asarray(live(), dtype=np.float64)
    if RECORDING:
        _arrays[key] = got
    else:
        assert key in _arrays, _missing(key)
        assert got.shape == _arrays[key].shape and np.array_equal(got, _arrays[key], equal_nan=True), \
            "the reference's answer for %r is not the stored one: python oracle/make_golden.py --records" % key
    return got


@atexit.register
def _write():
    if not RECORDING:
        return
    with open(RECORDS_JSON, "w") as f:
        json.dump(_records, f, indent=0, sort_keys=True)
        f.write("\n")
    np.savez_compressed(ARRAYS_NPZ, **_arrays)
