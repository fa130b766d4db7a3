"""The real reference (oracle/_ref) where it is built, and its recorded answers where it is not.

The live comparisons of the oracle's restatement with the reference's own C++ (tests/test_oracle_*.py, tests/test_pivot_ref.py) reach the reference through
ref().  Where oracle/_ref is built (that needs the reference's sources) that is the library itself.  Elsewhere the restatement
computes each call, and its answer is handed back only if it is the reference's: tests/golden/ref_live.npz
(tests/golden/make_golden_live.py) holds, for every call the tests make of the reference, a digest of the call and a digest of
the reference's answer (every array of it, or the error code it raised).  Another answer, or a call the recording does not know,
fails the test.  Digests are taken as np.array_equal(..., equal_nan=True) compares: every NaN one NaN, every -0.0 made 0.0."""
import hashlib
import numbers
import os

import numpy as np

from oracle import oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_live.npz")
DIGEST_BYTES = 8

_stored = None          # call digest -> answer digest, from GOLDEN
_recording = None       # the same, while make_golden_live.py records


def _feed(h, x):
    if isinstance(x, np.ndarray):
        a = np.ascontiguousarray(x)
        if a.dtype.kind == "f":
            a = np.where(np.isnan(a), np.nan, a) + a.dtype.type(0)
        h.update(("a%s%s:" % (a.dtype.str, a.shape)).encode() + a.tobytes())
    elif isinstance(x, (tuple, list)):
        h.update(b"(")
        for y in x:
            _feed(h, y)
        h.update(b")")
    elif isinstance(x, dict):
        _feed(h, sorted(x.items()))
    elif isinstance(x, O.OracleError):
        h.update(b"err%d" % x.code)
    elif isinstance(x, O.ML):
        _feed(h, (x.levels(), x.total_nnz(), [x.level(k) for k in range(x.levels())]))
    elif isinstance(x, O.ILUCP):
        _feed(h, (x.perm, x.L, x.U))           # (not zero_pivots: the reference does not count them)
    elif isinstance(x, O.MLParams):
        _feed(h, [(f[0], list(v) if hasattr(v, "__len__") else v) for f in x._fields_ for v in [getattr(x, f[0])]])
    elif isinstance(x, (bool, np.bool_, numbers.Integral, str)):
        h.update(("%s:%r;" % (type(x).__name__, x if isinstance(x, str) else int(x))).encode())
    elif isinstance(x, numbers.Real):
        h.update(("f" + float(x).hex()).encode())
    elif isinstance(x, bytes):
        h.update(b"y%d:" % len(x) + x)
    else:
        raise TypeError("cannot digest %r" % type(x))


def _digest(x):
    h = hashlib.sha256()
    _feed(h, x)
    return h.digest()[:DIGEST_BYTES]


def start_recording():
    global _recording
    _recording = {}


def save_recording(path=GOLDEN):
    calls = sorted(_recording)
    np.savez(path, calls=np.frombuffer(b"".join(calls), np.uint8).reshape(-1, DIGEST_BYTES),
             answers=np.frombuffer(b"".join(_recording[c] for c in calls), np.uint8).reshape(-1, DIGEST_BYTES))
    return len(calls)


def _recorded(call):
    global _stored
    if _stored is None:
        z = np.load(GOLDEN)
        _stored = {c.tobytes(): a.tobytes() for c, a in zip(z["calls"], z["answers"])}
    assert call in _stored, "no recorded answer of the reference for this call (inputs changed?): build oracle/_ref, run make_golden_live.py"
    return _stored[call]


class _Ref:
    """O.ref()'s methods, O.ILUCP(O.ref(), ...) and O.ILUTP(O.ref(), ...): answered by oracle/_ref, or by the restatement and checked"""

    def __init__(self):
        self.live = O.ref_available()
        self.lib = O.ref() if self.live else O.orc()

    def __getattr__(self, name):
        return lambda *a, **kw: self.answer((name, a, kw), lambda: getattr(self.lib, name)(*a, **kw))

    def ILUCP(self, A, **kw):
        return self.answer(("ILUCP", A, kw), lambda: O.ILUCP(self.lib, A, **kw))

    def ILUTP(self, A, **kw):
        return self.answer(("ILUTP", A, kw), lambda: O.ILUTP(self.lib, A, **kw))

    def answer(self, call, compute):
        key = _digest(call) if (not self.live or _recording is not None) else None
        try:
            res = compute()
        except O.OracleError as e:
            res = e
        if key is not None:
            got = _digest(res)
            if not self.live:
                assert got == _recorded(key), "the restatement's answer to %s is not the reference's recorded one" % call[0]
            else:
                assert _recording.setdefault(key, got) == got, "one call, two answers: %s" % call[0]
        if isinstance(res, O.OracleError):
            raise res
        return _Object(self, key, res) if isinstance(res, (O.ML, O.ILUCP)) else res


class _Object:
    """a preconditioner object of the reference: its members as built (checked with the construction), apply() checked per call"""

    def __init__(self, ref, key, obj):
        self._ref, self._key, self._obj = ref, key, obj

    def __getattr__(self, name):
        return getattr(self._obj, name)

    def apply(self, x, use=O.ID):
        return self._ref.answer(("apply", self._key, x, use), lambda: self._obj.apply(x, use))


def ref():
    """the reference for a live comparison: oracle/_ref where it is built, else the restatement checked against its recorded answers"""
    return _Ref()


def recorded_only_for_default_seeds():
    """the recording covers the default seeds; other ILUPP_FUZZ_OFFSET values need oracle/_ref itself"""
    return int(os.environ.get("ILUPP_FUZZ_OFFSET", "0")) != 0 and not O.ref_available()
