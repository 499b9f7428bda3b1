"""A search's attribute checks (hdx_passes_checks, hdx_check_encoded_device; include/hdxhash.h):
passes_attribute_checks of common/attribute_check.cc:123-237 per object and over stored objects.

Expected values come from the restatement held here (`check_one`, `expected_first_fail`): Python
`bytes` ordering for strings (unsigned, the shorter of two equal prefixes first: memcmp, then the
lengths), `struct` for the numerics with the NaN rule written out.  Slices and decode verdicts of
stored objects are the oracle's decode_value.  The restatement is pinned for the primitive datatypes:
tests/test_reference_checks.py holds `check_one`, `expected_first_fail` and `compare` to what the
reference's compiled attribute_check.cc and datatype_*::compare return
(tests/golden/reference_check_values.json).  A container, document or macaroon datatype in a
check stays as restated."""
import ctypes
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import hyperdex_amd as hdx
from hyperdex_amd import _lib, datatypes as dt, synth
from hyperdex_amd.checks import AttributeCheck, _checks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRING, INT64, FLOAT = dt.HYPERDATATYPE_STRING, dt.HYPERDATATYPE_INT64, dt.HYPERDATATYPE_FLOAT
TS_DAY, TS_SEC = dt.HYPERDATATYPE_TIMESTAMP_DAY, dt.HYPERDATATYPE_TIMESTAMP_SECOND
LIST_STRING, DOCUMENT = dt.HYPERDATATYPE_LIST_STRING, dt.HYPERDATATYPE_DOCUMENT
PRIMITIVE = (STRING,) + dt.NUMERIC
FAIL, EQ, LE, GE, CLT, REGEX, LEN_EQ, LEN_LE, LEN_GE, CONTAINS, LT, GT = range(9728, 9740)
UNKNOWN_PREDICATE = 9800
PREDICATES = list(range(9728, 9740)) + [UNKNOWN_PREDICATE]
ORDERING = (EQ, LT, LE, GE, GT)
LENGTH = (LEN_EQ, LEN_LE, LEN_GE)
COMPARING = ORDERING + LENGTH  # the eight comparing predicates
T_POOL = [STRING, INT64, FLOAT, TS_DAY, TS_SEC]
D_POOL = T_POOL + [LIST_STRING, DOCUMENT, 12345]
BADENC_FF = 0xffffffff
BADENC_BIT = 1 << _lib.HDX_E_BADENC
SCHEMA = [STRING, STRING, INT64, FLOAT, TS_DAY, STRING]


# ---- the restatement ---------------------------------------------------------------------------

def validate(t, b):
    """datatype_*::validate for the primitive types."""
    return True if t == STRING else len(b) in (0, 8)


def compare(t, k, v):
    """datatype_*::compare(k, v): the check's value on the left."""
    if t == STRING:
        return (k > v) - (k < v)
    if t == FLOAT:
        a = struct.unpack("<d", k)[0] if k else 0.0
        b = struct.unpack("<d", v)[0] if v else 0.0
        return -1 if a < b else 1 if a > b else 0  # a NaN on either side: neither holds, 0
    a = struct.unpack("<q", k)[0] if k else 0
    b = struct.unpack("<q", v)[0] if v else 0
    return -1 if a < b else 1 if a > b else 0


def check_one(T, ck, v):
    """passes_attribute_check(T, check, v), attribute_check.cc:123-207, for a primitive T."""
    assert T in PRIMITIVE
    D, k, p = ck.datatype, ck.value, ck.predicate
    if D not in dt.KNOWN:
        return False
    if D not in PRIMITIVE:
        # a container, document or macaroon D: every predicate below needs T == D, D == INT64 or
        # D == STRING, or has_contains() of a primitive: false whichever way validate(k) goes
        return False
    if not validate(T, v) or not validate(D, k):
        return False
    if p in ORDERING:
        if T != D:
            return False
        c = compare(T, k, v)
        return {EQ: k == v or c == 0, LT: c > 0, LE: c >= 0, GE: c <= 0, GT: c < 0}[p]
    if p in LENGTH or p == CLT:
        tmp = struct.unpack("<q", (k[:8] + bytes(8))[:8])[0]
        if D != INT64 or T != STRING:
            return False
        return {LEN_EQ: len(v) == tmp, LEN_LE: len(v) <= tmp, CLT: len(v) <= tmp, LEN_GE: len(v) >= tmp}[p]
    if p == REGEX:
        assert not (T == STRING and D == STRING), "out of scope: the library refuses it"
        return False
    return False  # FAIL, CONTAINS (no primitive has_contains()), anything else


def expected_first_fail(types, key, values, checks):
    """passes_attribute_checks, attribute_check.cc:209-237."""
    for i, ck in enumerate(checks):
        if ck.attr >= len(types):
            return i
        if not check_one(int(types[ck.attr]), ck, key if ck.attr == 0 else values[ck.attr - 1]):
            return i
    return len(checks)


# ---- the edge pools ----------------------------------------------------------------------------

BASE = bytes((7 * i + 33) & 0xff for i in range(41))
LONG = np.random.default_rng(1100).bytes(1100)


def _flip(b, pos):
    return b[:pos] + bytes([b[pos] ^ 0x40]) + b[pos + 1:]


DIFF_AT = (0, 3, 4, 7, 8, 15, 16, 40)
STRINGS = ([b""] + [BASE[:L] for L in range(1, 42)] + [_flip(BASE, p) for p in DIFF_AT]
           + [b"\x7f", b"\x80", b"ab\x7f", b"ab\x80", b"abcdefg\x7f", b"abcdefg\x80", b"abcdefgh\x7fx", b"abcdefgh\x80x"]
           + [LONG, _flip(LONG, 1099), LONG[:1000]])
I64 = [struct.pack("<q", x) for x in (-2 ** 63, -1, 0, 1, 2 ** 63 - 1)] + [b""]
F64 = [struct.pack("<d", x) for x in (0.0, -0.0, float("inf"), float("-inf"), 5e-324, 1.5)] + \
      [struct.pack("<Q", 0x7ff8000000000001), struct.pack("<Q", 0xfff0000000000123), b""]
MIS_SIZED = [bytes([0x11] * L) for L in (1, 2, 3, 4, 5, 6, 7, 9)]


def pool(t):
    return STRINGS if t == STRING else F64 if t == FLOAT else I64


def draw(rng, t, mis=0.12):
    """One value of type t; numerics are mis-sized now and then."""
    if t != STRING and rng.random() < mis:
        return MIS_SIZED[int(rng.integers(len(MIS_SIZED)))]
    p = pool(t)
    return p[int(rng.integers(len(p)))]


def rates(outcomes):
    """{predicate: (true fraction, false fraction)} over [(predicate, bool)]."""
    out = {}
    for p in COMPARING:
        r = [t for q, t in outcomes if q == p]
        assert r, p
        out[p] = (sum(r) / len(r), 1 - sum(r) / len(r))
    return out


def assert_rates(outcomes):
    for p, (t, f) in rates(outcomes).items():
        assert t >= 0.10 and f >= 0.10, (p, t, f)


# ---- 1. hdx_passes_checks against the restatement ------------------------------------------------

def single_check_cases():
    """(T, check, v): every predicate x T x D, the values from the pools; about a third of the
    ordering checks carry the attribute's own bytes, and the length checks sit around len(v)."""
    rng = np.random.default_rng(20)
    cases = []
    for T in T_POOL:
        for D in D_POOL:
            for p in PREDICATES:
                if p == REGEX and T == STRING and D == STRING:
                    continue  # refused: test_refusals
                for _ in range(36):
                    v = draw(rng, T)
                    if D in PRIMITIVE:
                        k = draw(rng, D)
                    else:
                        k = [b"", bytes(8), b"abc"][int(rng.integers(3))]
                    if p in ORDERING and rng.random() < 0.3:
                        k = v
                    if p in LENGTH + (CLT,) and D == INT64:
                        tmp = [len(v) - 1, len(v), len(v) + 1, 0, -1, 5, 1100, -2 ** 63][int(rng.integers(8))]
                        k = struct.pack("<q", tmp)
                        r = rng.random()
                        if r < 0.08:
                            k = k[:3]      # 3 bytes: not an INT64
                        elif r < 0.16:
                            k = k + b"\1"  # 9 bytes
                        elif r < 0.24:
                            k = b""        # tmp = 0
                    cases.append((T, AttributeCheck(1, k, D, p), v))
    # every structured string pair under every ordering predicate, both ways round
    pairs = [(BASE, _flip(BASE, p)) for p in DIFF_AT] + [(BASE[:20], BASE[:21]), (b"", b"a"), (b"\x7f", b"\x80"),
                                                         (b"abcdefgh\x7fx", b"abcdefgh\x80x"), (LONG, _flip(LONG, 1099)),
                                                         (LONG[:1000], LONG), (BASE, BASE)]
    for a, b in pairs:
        for p in ORDERING:
            cases += [(STRING, AttributeCheck(1, a, STRING, p), b), (STRING, AttributeCheck(1, b, STRING, p), a)]
    # mis-sized numerics as the stored value and as the check's value, under every predicate
    for T in (INT64, FLOAT, TS_DAY):
        for bad in MIS_SIZED:
            for p in PREDICATES:
                cases += [(T, AttributeCheck(1, pool(T)[2], T, p), bad), (T, AttributeCheck(1, bad, T, p), pool(T)[2])]
    return cases


def test_cpu_single_checks_match_the_restatement():
    cases = single_check_cases()
    want = [check_one(T, ck, v) for T, ck, v in cases]
    # the condition, on the expected values alone
    assert_rates([(ck.predicate, w) for (T, ck, v), w in zip(cases, want)
                  if (ck.predicate in ORDERING and T == ck.datatype)
                  or (ck.predicate in LENGTH and T == STRING and ck.datatype == INT64)])
    for (T, ck, v), w in zip(cases, want):
        got = hdx.passes_checks([STRING, T], b"key", [v], [ck])
        assert got == (1 if w else 0), (T, ck, v)
        # ... and the same check on the key
        got = hdx.passes_checks([T, STRING], v, [b"x"], [AttributeCheck(0, ck.value, ck.datatype, ck.predicate)])
        assert got == (1 if w else 0), ("key", T, ck, v)
    assert len(cases) > 18000


def q(x):
    return struct.pack("<q", x)


def d(x):
    return struct.pack("<d", x)


# Check lists over SCHEMA.  LADDER fails at every index and passes, on BATCH.
LADDER = [AttributeCheck(1, q(3), INT64, LEN_GE), AttributeCheck(2, q(-1), INT64, GE),
          AttributeCheck(0, BASE[:24], STRING, LT), AttributeCheck(3, d(1.5), FLOAT, LE)]
ALL_TRUE_16 = ([AttributeCheck(1, b"", STRING, GE), AttributeCheck(5, q(5000), INT64, LEN_LE),
                AttributeCheck(0, b"", STRING, GE), AttributeCheck(5, b"\xff" * 2, STRING, LT),
                AttributeCheck(1, q(2 ** 62), INT64, CLT), AttributeCheck(0, q(-1), INT64, LEN_GE)] * 3)[:16]
LISTS = {
    "none": [],
    "one": [AttributeCheck(2, q(0), INT64, EQ)],
    "ladder": LADDER,
    "sixteen": [AttributeCheck(1, q(1), INT64, LEN_GE), AttributeCheck(1, q(1100), INT64, LEN_LE),
                AttributeCheck(0, b"", STRING, GE), AttributeCheck(5, LONG[:900], STRING, LE),
                AttributeCheck(2, q(2 ** 63 - 1), INT64, LE), AttributeCheck(2, q(-2 ** 63), INT64, GE),
                AttributeCheck(3, d(float("inf")), FLOAT, LE), AttributeCheck(3, d(float("-inf")), FLOAT, GE),
                AttributeCheck(4, q(-2 ** 63), TS_DAY, GE), AttributeCheck(4, b"", TS_DAY, LE),
                AttributeCheck(1, q(41), INT64, CLT), AttributeCheck(0, q(1), INT64, LEN_GE),
                AttributeCheck(5, q(0), INT64, LEN_GE), AttributeCheck(1, b"\xff" * 9, STRING, LE),
                AttributeCheck(2, b"", INT64, LE), AttributeCheck(3, d(1.5), FLOAT, GE)],
    "all_true_16": ALL_TRUE_16,
    "repeated": [AttributeCheck(1, BASE[:8], STRING, GE), AttributeCheck(1, _flip(BASE, 40), STRING, LE),
                 AttributeCheck(1, q(12), INT64, LEN_GE), AttributeCheck(1, BASE, STRING, GT)],
    "equalities": [AttributeCheck(1, BASE, STRING, EQ)],
    "equal_numbers": [AttributeCheck(3, d(float("nan")), FLOAT, EQ), AttributeCheck(2, b"", INT64, EQ)],
    "equal_floats": [AttributeCheck(3, d(-0.0), FLOAT, EQ)],
    "lengths": [AttributeCheck(5, q(17), INT64, LEN_EQ)],
    "length_41": [AttributeCheck(1, q(41), INT64, LEN_EQ)],
    "strict": [AttributeCheck(5, BASE[:17], STRING, LT), AttributeCheck(1, BASE[:30], STRING, GT)],
    "strict_numbers": [AttributeCheck(2, q(0), INT64, GT), AttributeCheck(4, q(1), TS_DAY, LT)],
    "beyond_schema": [AttributeCheck(0, b"", STRING, GE), AttributeCheck(6, b"", STRING, EQ),
                      AttributeCheck(1, b"", STRING, GE)],
    "far_beyond_schema": [AttributeCheck(0xffffffff, b"", STRING, GE)],
    "short": [AttributeCheck(1, q(10), INT64, LEN_LE), AttributeCheck(5, q(20), INT64, LEN_LE)],
    "long": [AttributeCheck(5, q(1000), INT64, LEN_GE)],
    "longish": [AttributeCheck(1, q(30), INT64, LEN_GE)],
    "mismatched": [AttributeCheck(4, q(0), TS_SEC, LE)],                 # another granularity: false
    "containers": [AttributeCheck(1, b"", STRING, GE), AttributeCheck(1, b"", LIST_STRING, EQ)],
    "regex_elsewhere": [AttributeCheck(2, b"", STRING, REGEX)],          # on a numeric: simply false
    "long_prefix": [AttributeCheck(5, LONG[:1000], STRING, LT)],
    "long_differs_last": [AttributeCheck(5, _flip(LONG, 1099)[:1016], STRING, LE)],
    "bad_constant": [AttributeCheck(2, b"\1\2\3", INT64, LE)],
    "tail_bytes": [AttributeCheck(1, _flip(BASE, 40), STRING, LE), AttributeCheck(5, _flip(BASE, 16)[:19], STRING, GE)],
}


def make_objects(n, seed):
    """[(key, [4 attributes + 1])] under SCHEMA, drawn from the pools; BASE comes up often so that
    equalities hold for more than a tenth."""
    rng = np.random.default_rng(seed)

    def s():
        return BASE if rng.random() < 0.2 else STRINGS[int(rng.integers(len(STRINGS)))]
    return [(s(), [s(), draw(rng, INT64), draw(rng, FLOAT), draw(rng, TS_DAY), s()]) for _ in range(n)]


class Batch:
    """2 000 objects and, per list, the restatement's first_fail of each: built once, never changed."""
    _the = None

    def __init__(self):
        self.objs = make_objects(2000, 7)
        self.want = {name: np.array([expected_first_fail(SCHEMA, k, vs, cl) for k, vs in self.objs], np.uint32)
                     for name, cl in LISTS.items()}
        self._cpu = None

    @classmethod
    def get(cls):
        if cls._the is None:
            cls._the = cls()
        return cls._the

    def cpu(self):
        """hdx_passes_checks over the batch, per list."""
        if self._cpu is None:
            self._cpu = {name: np.array([hdx.passes_checks(SCHEMA, k, vs, cl) for k, vs in self.objs], np.uint32)
                         for name, cl in LISTS.items()}
        return self._cpu

    def outcomes(self):
        """(predicate, result) of every (check, object) pair a comparing predicate is applied to
        with matching types."""
        out = []
        for cl in LISTS.values():
            for ck in cl:
                if ck.attr >= len(SCHEMA):
                    continue
                T = SCHEMA[ck.attr]
                if (ck.predicate in ORDERING and T == ck.datatype) or \
                        (ck.predicate in LENGTH and T == STRING and ck.datatype == INT64):
                    out += [(ck.predicate, check_one(T, ck, k if ck.attr == 0 else vs[ck.attr - 1]))
                            for k, vs in self.objs]
        return out

    def assert_condition(self):
        assert any(len(cl) >= 3 and set(self.want[name].tolist()) == set(range(len(cl) + 1))
                   for name, cl in LISTS.items())
        assert_rates(self.outcomes())
        for name in ("none", "one", "sixteen", "all_true_16"):
            assert len(LISTS[name]) == {"none": 0, "one": 1}.get(name, 16)
        assert (self.want["all_true_16"] == 16).all() and (self.want["none"] == 0).all()


def test_cpu_lists_match_the_restatement():
    b = Batch.get()
    b.assert_condition()
    got = b.cpu()
    for name in LISTS:
        assert np.array_equal(got[name], b.want[name]), name


def test_cpu_a_key_only_schema():
    assert hdx.passes_checks([INT64], q(5), [], [AttributeCheck(0, q(5), INT64, EQ)]) == 1
    assert hdx.passes_checks([INT64], q(5), [], [AttributeCheck(0, q(5), INT64, LT)]) == 0
    assert hdx.passes_checks([INT64], q(5), [], [AttributeCheck(1, q(5), INT64, EQ)]) == 0
    assert hdx.passes_checks([INT64], q(5), [], []) == 0


# ---- 2. refusals -------------------------------------------------------------------------------

def _passes_call(types, checks, c=None, null=None):
    t = np.asarray(types, np.uint32)
    vals = (ctypes.c_char_p * 8)(*[b""] * 8)
    lens = (ctypes.c_size_t * 8)()
    ff = ctypes.c_uint32(0xabcd)
    arr = _checks(checks)
    if null == "value":
        arr[0].value, arr[0].value_len = None, 3
    a = {"types": t.ctypes.data, "key": b"", "values": vals, "lens": lens, "checks": arr, "ff": ctypes.byref(ff)}
    if null in a:
        a[null] = None
    st = hdx.lib().hdx_passes_checks(a["types"], len(t), a["key"], 3 if null == "key" else 0, a["values"], a["lens"],
                                     a["checks"], len(checks) if c is None else c, a["ff"])
    return st, ff.value


def _device_call(types, checks, c=None, null=None, n=5, match=True):
    """hdx_check_encoded_device with stand-in (never dereferenced) device pointers."""
    t = np.asarray(types, np.uint32)
    p = {k: 4096 * (i + 1) for i, k in enumerate(("keys", "key_off", "key_len", "vals", "val_off", "val_len",
                                                  "first_fail", "match", "match_count"))}
    arr = _checks(checks)
    tp = t.ctypes.data
    if null == "types":
        tp = None
    elif null == "checks":
        arr = None
    elif null == "value":
        arr[0].value, arr[0].value_len = None, 3
    elif null:
        p[null] = None
    if not match:
        p["match"] = p["match_count"] = None
    return hdx.lib().hdx_check_encoded_device(tp, len(t), p["keys"], p["key_off"], p["key_len"], p["vals"],
                                              p["val_off"], p["val_len"], n, arr, len(checks) if c is None else c,
                                              p["first_fail"], p["match"], p["match_count"], None, None)


OK_CHECKS = [AttributeCheck(1, b"abc", STRING, LE), AttributeCheck(2, q(1), INT64, GE)]


def test_refusals_bad_type():
    for bad in (LIST_STRING, DOCUMENT, dt.HYPERDATATYPE_MAP_INT64_FLOAT, dt.HYPERDATATYPE_MACAROON_SECRET, 12345):
        ck = [AttributeCheck(1, b"", STRING, EQ)]
        assert _passes_call([STRING, bad], ck) == (_lib.HDX_E_BADTYPE, 0xabcd)
        assert _device_call([STRING, bad], ck) == _lib.HDX_E_BADTYPE
        assert _passes_call([bad, STRING], [AttributeCheck(0, b"", STRING, EQ)]) == (_lib.HDX_E_BADTYPE, 0xabcd)
        assert _device_call([bad, STRING], [AttributeCheck(0, b"", STRING, EQ)]) == _lib.HDX_E_BADTYPE
        # a container no check names is nobody's business here
        assert _passes_call([STRING, bad, STRING], [AttributeCheck(2, b"", STRING, EQ)]) == (_lib.HDX_OK, 1)
    rx = [AttributeCheck(1, b"a.*", STRING, REGEX)]
    assert _passes_call([STRING, STRING], rx) == (_lib.HDX_E_BADTYPE, 0xabcd)
    assert _device_call([STRING, STRING], rx) == _lib.HDX_E_BADTYPE
    # not refused: REGEX with D != STRING, or on a numeric attribute: simply false
    for types, ck in (([STRING, STRING], AttributeCheck(1, b"a.*", INT64, REGEX)),
                      ([STRING, INT64], AttributeCheck(1, b"a.*", STRING, REGEX)),
                      ([STRING, STRING], AttributeCheck(5, b"a.*", STRING, REGEX))):
        assert _passes_call(types, [ck]) == (_lib.HDX_OK, 0)
        assert _device_call(types, [ck], null="vals") == _lib.HDX_E_INVALID  # past the type checks


def test_refusals_invalid():
    types = [STRING, STRING, INT64]
    for null in ("types", "checks", "ff", "key", "values", "lens", "value"):
        assert _passes_call(types, OK_CHECKS, null=null) == (_lib.HDX_E_INVALID, 0xabcd), null
    assert _passes_call(types, [OK_CHECKS[0]] * 17) == (_lib.HDX_E_INVALID, 0xabcd)
    assert _passes_call([], OK_CHECKS) == (_lib.HDX_E_INVALID, 0xabcd)
    assert _passes_call(types, [OK_CHECKS[0]] * 16)[0] == _lib.HDX_OK
    # the per-object form reads the values in place: no cap on their bytes
    assert _passes_call(types, [AttributeCheck(1, bytes(1025), STRING, GE)]) == (_lib.HDX_OK, 0)
    for null in ("types", "checks", "value", "keys", "key_off", "key_len", "vals", "val_off", "val_len", "first_fail",
                 "match_count"):
        assert _device_call(types, OK_CHECKS, null=null) == _lib.HDX_E_INVALID, null
    assert _device_call(types, [OK_CHECKS[0]] * 17) == _lib.HDX_E_INVALID
    assert _device_call([], OK_CHECKS) == _lib.HDX_E_INVALID
    assert _device_call(types, [AttributeCheck(1, bytes(1000), STRING, GE), AttributeCheck(2, bytes(25), INT64, GE)]) \
        == _lib.HDX_E_INVALID  # 1025 bytes, whatever the ops make of them
    if hdx.lib().hdx_device_count() == 0:  # valid arguments reach the device binding, and only then
        assert _device_call(types, OK_CHECKS) == _lib.HDX_E_DEVICE
        assert _device_call(types, OK_CHECKS, match=False) == _lib.HDX_E_DEVICE
        assert _device_call(types, [AttributeCheck(1, bytes(1016), STRING, GE), AttributeCheck(2, q(1), INT64, GE)]) \
            == _lib.HDX_E_DEVICE  # 1024 bytes
        assert _device_call(types, [], c=0) == _lib.HDX_E_DEVICE
        assert _device_call(types, [], c=0, null="checks") == _lib.HDX_E_DEVICE


def test_predicate_values_and_geometry():
    assert [dt.HYPERPREDICATE_FAIL, dt.HYPERPREDICATE_EQUALS, dt.HYPERPREDICATE_LESS_EQUAL,
            dt.HYPERPREDICATE_GREATER_EQUAL, dt.HYPERPREDICATE_CONTAINS_LESS_THAN, dt.HYPERPREDICATE_REGEX,
            dt.HYPERPREDICATE_LENGTH_EQUALS, dt.HYPERPREDICATE_LENGTH_LESS_EQUAL,
            dt.HYPERPREDICATE_LENGTH_GREATER_EQUAL, dt.HYPERPREDICATE_CONTAINS, dt.HYPERPREDICATE_LESS_THAN,
            dt.HYPERPREDICATE_GREATER_THAN] == list(range(9728, 9740))
    assert hdx.checks.check_block_objects() in (64, 128, 256, 512, 1024)


# ---- 3. a stand-alone C++ caller ---------------------------------------------------------------

@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_cpu_checks_cpp_caller(tmp_path):
    """tests/cpp/passes_checks_test.cc + hdx_cpu.cpp as one program (no Python, no device)."""
    inc = ["-I" + os.path.join(ROOT, "hyperdex_amd", "csrc"), "-I" + os.path.join(ROOT, "include")]
    exe = str(tmp_path / "passes_checks_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *inc,
                    os.path.join(ROOT, "tests", "cpp", "passes_checks_test.cc"),
                    os.path.join(ROOT, "hyperdex_amd", "csrc", "hdx_cpu.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "passes_checks_test ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---- the device: helpers -----------------------------------------------------------------------

@pytest.fixture(scope="module")
def torch_gpu():
    import torch
    return torch


def packed(objs):
    """Objects [(key, [attributes])] as a packed batch (blob, obj_base, attr_len) for synth's encoders."""
    A = 1 + len(objs[0][1])
    lens = np.array([[len(k)] + [len(x) for x in vs] for k, vs in objs], np.uint32)
    blob = np.frombuffer(b"".join(k + b"".join(vs) for k, vs in objs) + b"\0", np.uint8).copy()
    base = np.concatenate([[0], np.cumsum(lens.sum(axis=1, dtype=np.uint64))[:-1]]).astype(np.uint64)
    assert lens.shape[1] == A
    return blob, base, lens.reshape(-1)


def encode(types, objs, layout):
    blob, base, lens = packed(objs)
    t = np.asarray(types, np.uint32)
    if layout == "columns":
        return synth.encode_values_host(t, blob, base, lens, first_version=5)
    return synth.encode_store_host(t, blob, base, lens, first_version=5, layout=layout)


def to_dev(torch, enc, shift=0):
    """The six arrays on the device; the stores at data_ptr() % 16 == shift."""
    from test_device_edges import shifted
    from test_encoded import _to_dev
    dev = torch.device("cuda", 0)
    keys, key_off, key_len, vals, val_off, val_len = enc
    out = _to_dev(torch, dev, (key_off, key_len, val_off, val_len))
    dk = shifted(torch, dev, keys, shift)
    dv = dk if keys is vals else shifted(torch, dev, vals, shift)
    return [dk, out[0], out[1], dv, out[2], out[3]]


def run(torch, types, d, checks, want_match=True, stream=None):
    dev = torch.device("cuda", 0)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    ff, match = hdx.check_encoded(types, *d, checks, want_match=want_match, status=status, stream=stream)
    (stream or torch.cuda.current_stream(dev)).synchronize()
    return (ff.cpu().numpy().view(np.uint32), None if match is None else match.cpu().numpy().view(np.uint64),
            int(status.item()) & 0xffffffff)


def assert_result(got, want_ff, c, want_status=0):
    ff, match, status = got
    assert np.array_equal(ff, want_ff)
    if match is not None:
        assert np.array_equal(match, np.nonzero(want_ff == c)[0].astype(np.uint64))
    assert status == want_status


def expected_stored(oracle, types, enc, checks):
    """The restatement over stored objects: slices and verdicts from the oracle's decode_value."""
    keys, key_off, key_len, vals, val_off, val_len = enc
    A = len(types)
    out = np.zeros(len(val_off), np.uint32)
    for i in range(len(val_off)):
        vo = int(val_off[i])
        ok, _, sl = oracle.decode_value(A, vals, vo, int(val_len[i]))
        if not ok:
            out[i] = BADENC_FF
            continue
        key = bytes(keys[int(key_off[i]):int(key_off[i]) + int(key_len[i])])
        out[i] = expected_first_fail(types, key, [bytes(vals[vo + o:vo + o + L]) for o, L in sl], checks)
    return out


# ---- 4. the matrix as stored objects -----------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("layout,shift", [("keycol", 0), ("records", 0), ("columns", 0), ("keycol", 1), ("records", 7),
                                          ("columns", 13)])
def test_gpu_matrix(oracle, torch_gpu, layout, shift):
    b = Batch.get()
    b.assert_condition()
    enc = encode(SCHEMA, b.objs, layout)
    # the stored form decodes to the objects the restatement saw
    assert np.array_equal(expected_stored(oracle, SCHEMA, enc, LADDER), b.want["ladder"])
    d = to_dev(torch_gpu, enc, shift)
    cpu = b.cpu()
    for name, cl in LISTS.items():
        got = run(torch_gpu, SCHEMA, d, cl)
        assert_result(got, b.want[name], len(cl))
        assert np.array_equal(got[0], cpu[name]), name
    # without match: the same verdicts
    got = run(torch_gpu, SCHEMA, d, LADDER, want_match=False)
    assert got[1] is None
    assert_result(got, b.want["ladder"], 4)


# ---- 5. bad encodings --------------------------------------------------------------------------

@pytest.mark.gpu
def test_gpu_bad_encodings(oracle, torch_gpu):
    from test_encoded import _corrupt
    b = Batch.get()
    keys, key_off, key_len, vals, val_off, val_len = [np.array(x) for x in encode(SCHEMA, b.objs, "columns")]
    clean = (keys, key_off, key_len, vals.copy(), val_off, val_len.copy())
    rng = np.random.default_rng(4)
    damaged = set()
    for lo in range(0, 2000, 400):  # 40 of every 400: a tenth
        s = slice(lo, lo + 400)
        (_, _, _, vals, _, vl), cases = _corrupt((keys, key_off[s], key_len[s], vals, val_off[s], val_len[s]), rng)
        val_len[s] = vl
        damaged |= {lo + i for i in cases}
    enc = (keys, key_off, key_len, vals, val_off, val_len)
    want = expected_stored(oracle, SCHEMA, enc, LADDER)
    bad = want == BADENC_FF
    assert set(np.nonzero(bad)[0].tolist()) == damaged and len(damaged) == 200
    assert np.array_equal(want[~bad], b.want["ladder"][~bad])
    got = run(torch_gpu, SCHEMA, to_dev(torch_gpu, enc), LADDER)
    assert_result(got, want, 4, want_status=BADENC_BIT)
    assert not (set(got[1].tolist()) & damaged) and len(got[1]) > 0
    # c == 0: every decodable object matches, the others do not
    got = run(torch_gpu, SCHEMA, to_dev(torch_gpu, enc), [])
    assert_result(got, np.where(bad, BADENC_FF, 0).astype(np.uint32), 0, want_status=BADENC_BIT)
    # a clean batch, mis-sized stored numerics and all: no bit
    assert any(len(vs[1]) not in (0, 8) for _, vs in b.objs)
    assert_result(run(torch_gpu, SCHEMA, to_dev(torch_gpu, clean), LADDER), b.want["ladder"], 4, want_status=0)


# ---- 6. sizes ----------------------------------------------------------------------------------

def pair_batch(torch, n):
    """n objects under [STRING, INT64], 4 + 22 bytes each, built on the device: key = i (4 bytes),
    attribute 1 = i & 1.  Returns the six tensors."""
    dev = torch.device("cuda", 0)
    i = torch.arange(n, dtype=torch.int64, device=dev)
    keys = torch.stack([(i >> s) & 0xff for s in (0, 8, 16, 24)], dim=1).to(torch.uint8).reshape(-1)
    vals = torch.zeros((n, 22), dtype=torch.uint8, device=dev)
    for b_ in range(8):
        vals[:, 7 - b_] = ((i + 1) >> (8 * b_)) & 0xff   # the version, big-endian
    vals[:, 9] = 1                                       # one attribute
    vals[:, 13] = 8                                      # of 8 bytes
    vals[:, 14] = i & 1
    out = [keys, i * 4, torch.full((n,), 4, dtype=torch.int32, device=dev), vals.reshape(-1), i * 22,
           torch.full((n,), 22, dtype=torch.int32, device=dev)]
    # tensors without elements have no address: one-element stand-ins that nothing reads
    return [x if x.numel() else torch.zeros(1, dtype=x.dtype, device=dev) for x in out]


def second_level():
    """The first n at which the compaction's scan of one count per workgroup takes a second level."""
    return hdx.checks.check_block_objects() * hdx.index.SCAN_BLOCK + 1


def raw_call(torch, types, d, checks, n, match, count, ff, status):
    t = np.asarray(types, np.uint32)
    _lib.check(hdx.lib().hdx_check_encoded_device(
        t.ctypes.data, len(t), *[x.data_ptr() for x in d], n, _checks(checks), len(checks), ff.data_ptr(),
        match.data_ptr(), count.data_ptr(), status.data_ptr(), torch.cuda.current_stream().cuda_stream))


SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, "level-2", "level-1", "level"]
GUARD = -0x5a5a5a5a5a5a5a5b


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_gpu_sizes(torch_gpu, n):
    """Every second object matches; match has n elements and the guard pattern behind the
    match_count entries is intact.  Then c == 0 and 16 true checks on the same objects."""
    torch = torch_gpu
    assert hdx.checks.check_block_objects() * hdx.index.SCAN_BLOCK == 256 * 1024
    if isinstance(n, str):
        n = second_level() - {"level-2": 2, "level-1": 1, "level": 0}[n]
    dev = torch.device("cuda", 0)
    types = [STRING, INT64]
    d = pair_batch(torch, n)
    idx = torch.arange(n, dtype=torch.int64, device=dev)
    true16 = ([AttributeCheck(0, q(4), INT64, LEN_EQ), AttributeCheck(1, q(0), INT64, GE),
               AttributeCheck(0, b"", STRING, GE), AttributeCheck(1, q(1), INT64, LE)] * 4)
    for checks, want_ff, want_match in (
            ([AttributeCheck(0, q(4), INT64, LEN_EQ), AttributeCheck(1, q(0), INT64, EQ)], 1 + (1 - (idx & 1)), idx[::2]),
            ([], torch.zeros_like(idx), idx), (true16, torch.full_like(idx, 16), idx)):
        ff = torch.full((max(n, 1),), -7, dtype=torch.int32, device=dev)
        match = torch.full((max(n, 1),), GUARD, dtype=torch.int64, device=dev)
        count = torch.full((1,), GUARD, dtype=torch.int64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        raw_call(torch, types, d, checks, n, match, count, ff, status)
        torch.cuda.synchronize()
        k = int(count.item())
        assert k == want_match.numel() and int(status.item()) == 0
        assert torch.equal(ff[:n].to(torch.int64), want_ff)
        assert torch.equal(match[:k], want_match) and bool((match[k:] == GUARD).all())
        if n == 0:
            assert int(ff.item()) == -7


# ---- 7. width ----------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("A", [1, 129, 130, 300])
def test_gpu_width(oracle, torch_gpu, A):
    s10 = synth.Rule(STRING, synth.UNIFORM, 0, 10)
    if A == 1:
        rules = [s10]
        checks = [AttributeCheck(0, q(4), INT64, LEN_GE), AttributeCheck(0, b"\x80", STRING, GE)]
    else:
        rules = [s10] * (A - 2) + [synth._n(INT64), synth.Rule(STRING, synth.UNIFORM, 0, 30)]
        checks = [AttributeCheck(A - 1, q(9), INT64, LEN_GE), AttributeCheck(0, b"\x80", STRING, GE),
                  AttributeCheck(A - 2, q(0), INT64, GE), AttributeCheck(A - 1, b"\x70", STRING, LT)]
    types, blob, base, lens = synth.make_batch_host(rules, 300, seed=A)
    enc = synth.encode_values_host(types, blob, base, lens, first_version=1)
    want = expected_stored(oracle, [int(t) for t in types], enc, checks)
    assert len(set(want.tolist())) >= 3 and BADENC_FF not in want  # fails at several indices, and passes
    assert_result(run(torch_gpu, types, to_dev(torch_gpu, enc), checks), want, len(checks))


# ---- 8. a side stream, and offsets across 4 GiB --------------------------------------------------

@pytest.mark.gpu
def test_gpu_side_stream(torch_gpu):
    """One call on a side stream behind a producer on that stream, while the default stream is
    busy: launches and the read of the count run on the given stream only."""
    torch = torch_gpu
    b = Batch.get()
    dev = torch.device("cuda", 0)
    d = to_dev(torch, encode(SCHEMA, b.objs, "keycol"))
    staged = d[3].clone()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    busy = torch.empty(256 << 20, dtype=torch.uint8, device=dev)
    for _ in range(8):
        busy.fill_(1)                 # the default stream's work
    with torch.cuda.stream(side):
        d[3].zero_()                  # the producer: a launch that escapes the stream reads zeros
        d[3].copy_(staged)
    assert_result(run(torch, SCHEMA, d, LADDER, stream=side), b.want["ladder"], 4)
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_gpu_offsets_across_4gib(torch_gpu):
    """The values lie just below and just above offset 2^32 of one store."""
    from test_device_edges import TWO32, HighArena, straddles
    torch = torch_gpu
    b = Batch.get()
    dev = torch.device("cuda", 0)
    keys, key_off, key_len, vals, val_off, val_len = encode(SCHEMA, b.objs, "keycol")
    arena = HighArena(torch, dev)
    try:
        shift = arena.place(vals)
        high_off = val_off + np.uint64(shift)
        assert straddles(high_off, val_len)
        d = to_dev(torch, (keys, key_off, key_len, vals[:1], high_off, val_len))
        d[3] = arena.view
        assert_result(run(torch, SCHEMA, d, LADDER), b.want["ladder"], 4)
        assert int(high_off[0]) < TWO32 < int(high_off[-1])
    finally:
        arena.view = arena.arena = None
        torch.cuda.empty_cache()


# ---- 9. the packed constants at their largest size -------------------------------------------------

CAP_TYPES = [STRING, STRING, STRING]
CAP_STORED = bytes((11 * i + 70) & 0xff for i in range(64)) + b"\x80"  # attribute 2 of every object
CAP_LAST = bytes((5 * i + 0x41) & 0xff for i in range(49))              # check 15's constant
CAP_N = 257                                                             # two workgroups, one lane in the second


def cap_list():
    """16 STRING comparisons whose constants, of lengths = 1 (mod 8), sum to HDX_CHECK_BYTES_MAX: packed,
    each takes 7 bytes of padding, the largest block there is (1136 bytes).  Checks 0-14 compare attribute
    2 with constants that differ from CAP_STORED in the last byte only, the predicates chosen so that all
    pass: a lane reads every staged word of theirs.  Check 15: attribute 1 EQUALS CAP_LAST, whose last
    byte lies alone in the block's last word."""
    cl = []
    for i in range(15):
        above = i % 2 == 0
        k = CAP_STORED[:64] + bytes([0x80 + (1 + i if above else -1 - i)])
        cl.append(AttributeCheck(2, k, STRING, ((LT, LE) if above else (GT, GE))[i // 2 % 2]))
    return cl + [AttributeCheck(1, CAP_LAST, STRING, EQ)]


def cap_objects():
    """Attribute 1 in turn: CAP_LAST, CAP_LAST with another last byte, CAP_LAST without its last byte."""
    a1 = (CAP_LAST, CAP_LAST[:48] + bytes([CAP_LAST[48] ^ 1]), CAP_LAST[:48])
    return [(b"key%d" % i, [a1[i % 3], CAP_STORED]) for i in range(CAP_N)]


def assert_cap_outcomes(want, c):
    """first_fail is c for a third of the objects and c - 1 for the rest: each outcome over a tenth."""
    assert set(want.tolist()) == {c - 1, c}
    assert np.array_equal(want == c, np.arange(CAP_N) % 3 == 0)
    assert (want == c).mean() >= 0.10 and (want != c).mean() >= 0.10


def test_cap_list_holds_both_outcomes():
    """The condition of test_gpu_constants_at_the_cap, on the restatement alone; and the per-object form."""
    cl, objs = cap_list(), cap_objects()
    assert len(cl) == hdx.checks.HDX_MAX_CHECKS and all(len(ck.value) % 8 == 1 for ck in cl)
    assert sum(len(ck.value) for ck in cl) == hdx.checks.HDX_CHECK_BYTES_MAX
    want = np.array([expected_first_fail(CAP_TYPES, k, vs, cl) for k, vs in objs], np.uint32)
    assert_cap_outcomes(want, 16)
    assert [hdx.passes_checks(CAP_TYPES, k, vs, cl) for k, vs in objs] == want.tolist()


@pytest.mark.gpu
def test_gpu_constants_at_the_cap(torch_gpu):
    """Every word of the largest constants block reaches the workgroups: a count one word short leaves
    check 15's last byte unstaged, and the objects that equal CAP_LAST fail it."""
    cl, objs = cap_list(), cap_objects()
    want = np.array([expected_first_fail(CAP_TYPES, k, vs, cl) for k, vs in objs], np.uint32)
    d = to_dev(torch_gpu, encode(CAP_TYPES, objs, "keycol"))
    got = run(torch_gpu, CAP_TYPES, d, cl)
    assert_result(got, want, 16)
    assert int(got[1].size) == int((want == 16).sum()) == 86  # match_count: every third object of 257
