"""REGEX on STRING attributes through a compiled list of checks (hdx_regex_match, hdx_checks_compile,
hdx_checks_passes, hdx_checks_encoded_device, hdx_checks_sorted_device; include/hdxhash.h).

The pin is tests/golden/reference_regex_values.json: the reference's own regex_match (common/
regex_match.cc, compiled unmodified by tests/golden/make_reference_regex_values.py) over a hand-written
edge list and 20 000 random cases.  `py_regex` below restates the matcher as an iterative set of
positions; it equals the fixture on every case and provides the expected values of everything else.
Nothing on the GPU carries a pathological pattern: linear time is a host test, and hdx_regex.h's step is
the one both sides compile."""
import ctypes
import importlib.util
import json
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

import hyperdex_amd as hdx
from hyperdex_amd import _lib, datatypes as dt
from hyperdex_amd.checks import AttributeCheck, CompiledChecks, _checks
from hyperdex_amd.sorting import KEEP_LARGEST, KEEP_SMALLEST, SortSpec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRING, INT64, FLOAT = dt.HYPERDATATYPE_STRING, dt.HYPERDATATYPE_INT64, dt.HYPERDATATYPE_FLOAT
LIST_STRING, DOCUMENT = dt.HYPERDATATYPE_LIST_STRING, dt.HYPERDATATYPE_DOCUMENT
EQ, LE, GE, REGEX, LEN_GE, LEN_LE = 9729, 9730, 9731, 9733, 9736, 9735
BADENC_FF = 0xffffffff
BADENC_BIT = 1 << _lib.HDX_E_BADENC


def _load_generator():
    spec = importlib.util.spec_from_file_location(
        "make_reference_regex_values", os.path.join(ROOT, "tests", "golden", "make_reference_regex_values.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


gen = _load_generator()


def q(x):
    return struct.pack("<q", x)


def rx(attr, pattern, datatype=STRING):
    return AttributeCheck(attr, pattern, datatype, REGEX)


# ---- the restatement: an iterative set of positions ----------------------------------------------

def parse(p):
    """(items, anchored, end): items of ("lit" | "any" | "star" | "starany" | "dead", byte)."""
    i, anchored, end, items = 0, False, False, []
    if p[:1] == b"^":
        anchored, i = True, 1
    while i < len(p):
        ch = p[i]
        if ch == 0x5c:  # a backslash
            items.append(("lit", p[i + 1]) if i + 1 < len(p) else ("dead", 0))
            i += 2
        elif i + 1 < len(p) and p[i + 1] == 0x2a:  # x*
            items.append(("starany", 0) if ch == 0x2e else ("star", ch))
            i += 2
        elif ch == 0x24 and i + 1 == len(p):  # $ as the very last byte
            end = True
            i += 1
        else:
            items.append(("any", 0) if ch == 0x2e else ("lit", ch))
            i += 1
    return items, anchored, end


def item_count(p):
    items, _, end = parse(p)
    return len(items) + int(end)


def py_regex(p, t):
    items, anchored, end = parse(p)
    m = len(items)

    def close(s):
        out, work = set(s), list(s)
        while work:
            j = work.pop()
            if j < m and items[j][0] in ("star", "starany") and j + 1 not in out:
                out.add(j + 1)
                work.append(j + 1)
        return out

    s = close({0})
    if not end and m in s:
        return True
    for c in t:
        nxt = set()
        for j in s:
            if j == m:
                continue
            kind, b = items[j]
            if kind in ("any", "starany") or (kind in ("lit", "star") and b == c):
                nxt.add(j if kind in ("star", "starany") else j + 1)
        if not anchored:
            nxt.add(0)
        s = close(nxt)
        if not end and m in s:
            return True
        if not s:
            return False
    return m in s


_memo = {}


def expected_regex(p, t):
    k = (p, t)
    if k not in _memo:
        _memo[k] = py_regex(p, t)
    return _memo[k]


def check_one(T, ck, v):
    """test_checks.check_one with the one case it leaves out."""
    from test_checks import check_one as base
    if ck.predicate == REGEX and T == STRING and ck.datatype == STRING:
        return expected_regex(ck.value, v)
    return base(T, ck, v)


def expected_first_fail(types, key, values, checks):
    for i, ck in enumerate(checks):
        if ck.attr >= len(types):
            return i
        if not check_one(int(types[ck.attr]), ck, key if ck.attr == 0 else values[ck.attr - 1]):
            return i
    return len(checks)


# ---- 1. the fixture ------------------------------------------------------------------------------

def fixture():
    with open(gen.FIXTURE) as f:
        return json.load(f)


def fixture_cases():
    """[(pattern, text, matched)] of both groups, the inputs checked against the fixture's digests."""
    fx, out = fixture(), []
    for name, cases in (("edge", gen.edge_cases()), ("random", gen.random_cases())):
        assert fx[name]["cases"] == len(cases) and fx[name]["inputs_sha256"] == gen.inputs_sha256(cases), name
        bits = gen.unpack_bits(fx[name]["matched"], len(cases))
        out += [(p, t, bool(b)) for (p, t), b in zip(cases, bits)]
    return out


def test_fixture_holds_the_edges_and_both_outcomes():
    fx = fixture()
    assert fx["random"]["cases"] >= 20000
    bits = gen.unpack_bits(fx["random"]["matched"], fx["random"]["cases"])
    assert 0.10 <= bits.mean() <= 0.90, bits.mean()  # each outcome at least a tenth of the random cases
    pats = set(gen.EDGE_PATTERNS)
    for p in (b"", b"^", b"$", b"^$", b"a$b", b"$*", b"**", b"a^b", b"\\", b"\\\\", b"\\a*", b".*a", b"a.*", b"a.*b",
              b"a*b*c*", b"\x80", gen.LIT63, gen.LIT64):
        assert p in pats, p
    assert b"" in gen.EDGE_TEXTS and any(c >= 0x80 for t in gen.EDGE_TEXTS for c in t)
    assert item_count(gen.LIT63) == 63 and item_count(gen.LIT64) == 64 and item_count(gen.LIT63[:62] + b"$") == 63


@pytest.mark.skipif(not gen.available(), reason="needs the reference's sources and a C++ compiler")
def test_fixture_regenerates_from_the_reference():
    with open(gen.FIXTURE) as f:
        assert gen.dumps(gen.build_fixture()) == f.read()


def test_regex_match_equals_the_fixture():
    n = 0
    for p, t, want in fixture_cases():
        if item_count(p) > hdx.checks.HDX_REGEX_ITEMS_MAX:
            with pytest.raises(hdx.HdxError) as e:
                hdx.regex_match(p, t)
            assert e.value.status == _lib.HDX_E_INVALID
            n += 1
        else:
            assert hdx.regex_match(p, t) == want, (p, t)
    assert n > 0
    out = ctypes.c_int(77)
    assert hdx.lib().hdx_regex_match(gen.LIT64, 64, b"a", 1, ctypes.byref(out)) == _lib.HDX_E_INVALID
    assert hdx.lib().hdx_regex_match(None, 1, b"a", 1, ctypes.byref(out)) == _lib.HDX_E_INVALID
    assert hdx.lib().hdx_regex_match(b"a", 1, None, 1, ctypes.byref(out)) == _lib.HDX_E_INVALID
    assert hdx.lib().hdx_regex_match(b"a", 1, b"a", 1, None) == _lib.HDX_E_INVALID
    assert out.value == 77  # untouched on refusal
    assert hdx.lib().hdx_regex_match(None, 0, None, 0, ctypes.byref(out)) == _lib.HDX_OK and out.value == 1


def test_restatement_equals_the_fixture():
    for p, t, want in fixture_cases():
        assert py_regex(p, t) == want, (p, t)


LINEAR = """
import ctypes, signal, sys
L = ctypes.CDLL(sys.argv[1])
text = b"a" * 4096
out = ctypes.c_int(-1)
signal.setitimer(signal.ITIMER_REAL, 1.0)  # no handler: the alarm ends this process, inside a C call too
for p in (b"a.*a.*a.*a.*a.*b", b"^a.*a.*a.*a.*a.*$"):
    st = L.hdx_regex_match(p, ctypes.c_size_t(len(p)), text, ctypes.c_size_t(len(text)), ctypes.byref(out))
    print(st, out.value)
"""


def test_linear_time():
    """Five stars against 4096 x 'a': 4096 steps for a linear matcher, on the order of 4096^5 for a
    backtracking one.  The 1 s limit is a condition, not a measurement: a child process that sets itself an
    alarm once the library is loaded, so that the limit covers the two calls and can end them."""
    r = subprocess.run([sys.executable, "-c", LINEAR, _lib.LIB_PATH], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split() == ["0", "0", "0", "1"]


# ---- 2. hdx_checks_compile ---------------------------------------------------------------------------

def compile_call(types, checks, c=None, null=None):
    t = np.asarray(types, np.uint32)
    arr = _checks(checks)
    h = ctypes.c_void_p(0xabcd)
    a = {"types": t.ctypes.data, "checks": arr, "out": ctypes.byref(h)}
    if null == "value":
        arr[0].value, arr[0].value_len = None, 3
    elif null:
        a[null] = None
    st = hdx.lib().hdx_checks_compile(a["types"], len(t), a["checks"], len(checks) if c is None else c, a["out"])
    if st == _lib.HDX_OK:
        hdx.lib().hdx_checks_free(h)
        return st, None
    return st, h.value


def test_compile_refusals():
    types = [STRING, STRING, INT64]
    ok = [rx(1, b"a.*b"), AttributeCheck(2, q(1), INT64, GE)]
    assert compile_call(types, ok) == (_lib.HDX_OK, None)
    for null in ("types", "checks", "out", "value"):
        assert compile_call(types, ok, null=null) == (_lib.HDX_E_INVALID, 0xabcd), null
    assert compile_call(types, [], c=0, null="checks") == (_lib.HDX_OK, None)
    # the existing caps
    assert compile_call(types, [ok[1]] * 17) == (_lib.HDX_E_INVALID, 0xabcd)
    assert compile_call(types, [ok[1]] * 16) == (_lib.HDX_OK, None)
    assert compile_call([], ok) == (_lib.HDX_E_INVALID, 0xabcd)
    assert compile_call(types, [AttributeCheck(1, bytes(1000), STRING, GE), rx(1, b"." * 25)]) \
        == (_lib.HDX_E_INVALID, 0xabcd)  # 1025 bytes, the pattern's included
    assert compile_call(types, [AttributeCheck(1, bytes(1000), STRING, GE), rx(1, b"." * 24)]) == (_lib.HDX_OK, None)
    # the new ones
    assert compile_call(types, [rx(1, b"a")] * 4) == (_lib.HDX_OK, None)
    assert compile_call(types, [rx(1, b"a")] * 5) == (_lib.HDX_E_INVALID, 0xabcd)
    assert compile_call(types, [rx(1, b"a")] * 4 + [rx(2, b"a"), rx(1, b"a", INT64), rx(7, b"a")]) == (_lib.HDX_OK, None)
    assert compile_call(types, [rx(0, gen.LIT63)]) == (_lib.HDX_OK, None)
    assert compile_call(types, [rx(0, b"^" + gen.LIT63[:62] + b"$")]) == (_lib.HDX_OK, None)
    assert compile_call(types, [rx(0, gen.LIT64)]) == (_lib.HDX_E_INVALID, 0xabcd)
    assert compile_call(types, [rx(0, gen.LIT63 + b"$")]) == (_lib.HDX_E_INVALID, 0xabcd)
    assert compile_call(types, [rx(2, gen.LIT64)]) == (_lib.HDX_OK, None)  # simply false: never parsed
    # container and document attributes
    for bad in (LIST_STRING, DOCUMENT, 12345):
        assert compile_call([STRING, bad], [rx(1, b"a")]) == (_lib.HDX_E_BADTYPE, 0xabcd)
        assert compile_call([STRING, bad], [AttributeCheck(1, b"", STRING, EQ)]) == (_lib.HDX_E_BADTYPE, 0xabcd)
        assert compile_call([STRING, bad, STRING], [rx(2, b"a")]) == (_lib.HDX_OK, None)
    hdx.lib().hdx_checks_free(None)
    ff = ctypes.c_uint32(0xabcd)
    assert hdx.lib().hdx_checks_passes(None, b"", 0, None, None, ctypes.byref(ff)) == _lib.HDX_E_INVALID
    with CompiledChecks(types, ok) as cc:
        assert hdx.lib().hdx_checks_passes(cc._handle(), b"", 0, None, None, ctypes.byref(ff)) == _lib.HDX_E_INVALID
        assert hdx.lib().hdx_checks_passes(cc._handle(), b"", 0, None, None, None) == _lib.HDX_E_INVALID
        assert hdx.lib().hdx_checks_encoded_device(cc._handle(), None, 1, 1, 1, 1, 1, 5, 1, None, None, None, None) \
            == _lib.HDX_E_INVALID
        spec = SortSpec(1)._c()
        assert hdx.lib().hdx_checks_sorted_device(cc._handle(), 1, 1, 1, 1, 1, 1, 5, ctypes.byref(spec), 2000, None, 1, 1,
                                                  None, None) == _lib.HDX_E_INVALID  # the limit
        assert hdx.lib().hdx_checks_sorted_device(cc._handle(), 1, 1, 1, 1, 1, 1, 5, None, 5, None, 1, 1, None,
                                                  None) == _lib.HDX_E_INVALID
    assert ff.value == 0xabcd
    assert hdx.lib().hdx_checks_encoded_device(None, 1, 1, 1, 1, 1, 1, 5, 1, None, None, None, None) == _lib.HDX_E_INVALID


def test_regex_elsewhere_compiles_and_is_false():
    for types, ck in (([STRING, STRING], rx(1, b"a.*", INT64)), ([STRING, INT64], rx(1, b"a.*")),
                      ([STRING, STRING], rx(5, b"a.*")), ([INT64, STRING], rx(0, b""))):
        with CompiledChecks(types, [ck]) as cc:
            assert cc.passes(q(0) if types[0] == INT64 else b"aaa", [q(0) if types[1] == INT64 else b"aaa"]) == 0
    with CompiledChecks([STRING, STRING], [rx(1, b"a.*"), rx(0, b"^k")]) as cc:  # the handle copied its bytes
        assert cc.passes(b"key", [b"xa"]) == 2 and cc.passes(b"key", [b"x"]) == 0 and cc.passes(b"yek", [b"a"]) == 1


# ---- 3. hdx_checks_passes over the pools of test_checks.py ---------------------------------------------

def regex_lists():
    """Lists over test_checks.SCHEMA = [STRING, STRING, INT64, FLOAT, TS_DAY, STRING] with REGEX on the
    key and on value attributes; BASE is the pool's most common string."""
    from test_checks import BASE
    head = BASE[:4]  # no byte of BASE[:24] is special in a pattern
    assert not set(BASE[:24]) & set(b".*\\$^")
    return {
        "rx_key": [rx(0, b"^" + head)],
        "rx_value": [rx(1, BASE[8:12])],
        "rx_last": [rx(5, BASE[20:22] + b".*" + BASE[30:31])],
        "rx_end": [rx(1, BASE[39:40] + b".$")],
        "rx_two": [rx(1, b"^" + head), rx(1, BASE[9:10] + b".*" + BASE[12:13])],
        "rx_behind": [AttributeCheck(2, q(0), INT64, GE), rx(5, head)],
        "rx_range": [rx(0, head + b".*" + BASE[7:8]), AttributeCheck(1, q(3), INT64, LEN_GE)],
        "rx_four_16": [AttributeCheck(1, b"", STRING, GE), AttributeCheck(5, q(5000), INT64, LEN_LE),
                       AttributeCheck(0, b"", STRING, GE), rx(0, b"^" + head[:2]),
                       AttributeCheck(1, q(2 ** 62), INT64, LEN_LE), AttributeCheck(0, q(-1), INT64, LEN_GE),
                       AttributeCheck(5, b"\xff" * 2, STRING, LE), rx(1, b"..........*"),
                       AttributeCheck(1, b"", STRING, GE), AttributeCheck(5, q(0), INT64, LEN_GE),
                       AttributeCheck(0, b"", STRING, GE), rx(5, b"^" + head[:1] + b".*"),
                       AttributeCheck(1, b"", STRING, GE), AttributeCheck(5, q(5000), INT64, LEN_LE),
                       AttributeCheck(0, b"", STRING, GE), rx(5, BASE[5:6] + b".*" + BASE[9:10])],
        "rx_high": [rx(1, BASE[14:15] + b".*" + BASE[30:31])],  # BASE[14] = 0x83: a byte >= 0x80 in pattern and text
    }


def test_passes_matches_the_restatement_and_the_one_shot_form():
    from test_checks import LISTS, SCHEMA, Batch
    objs = Batch.get().objs[:600]
    for name, cl in regex_lists().items():
        want = [expected_first_fail(SCHEMA, k, vs, cl) for k, vs in objs]
        with CompiledChecks(SCHEMA, cl) as cc:
            assert [cc.passes(k, vs) for k, vs in objs] == want, name
        passed = sum(w == len(cl) for w in want) / len(want)
        assert 0.10 <= passed <= 0.90, (name, passed)
    # without REGEX on STRING: hdx_passes_checks case by case
    for name, cl in LISTS.items():
        with CompiledChecks(SCHEMA, cl) as cc:
            assert [cc.passes(k, vs) for k, vs in objs] == [hdx.passes_checks(SCHEMA, k, vs, cl) for k, vs in objs], name


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_host_forms_sanitized(tmp_path):
    """tests/cpp/regex_checks_test.cc + hdx_cpu.cpp as one program under -fsanitize=address,undefined (no
    Python, no device), the sanitizers' runtimes linked statically: the program needs nothing from its
    environment, which it inherits as it is."""
    inc = ["-I" + os.path.join(ROOT, "hyperdex_amd", "csrc"), "-I" + os.path.join(ROOT, "include")]
    exe = str(tmp_path / "regex_checks_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", *inc,
                    os.path.join(ROOT, "tests", "cpp", "regex_checks_test.cc"),
                    os.path.join(ROOT, "hyperdex_amd", "csrc", "hdx_cpu.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "regex_checks_test ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---- the device: a batch built by struct.pack ----------------------------------------------------------

TYPES = [STRING, STRING, INT64, STRING]
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 2049]
TEXT_LENGTHS = (0, 1, 7, 8, 9, 15, 16, 17, 41, 1100)
LENGTH_WEIGHTS = (1, 1, 2, 2, 2, 2, 2, 2, 3, 7)   # long texts often: the 63-item pattern needs them
VARIANTS = 6


def text_pool():
    """{length: VARIANTS texts} over a / b / c with a few special and high bytes; three of the 1100-byte
    texts hold LIT63 (at the start, in the middle, at the very end)."""
    rng = np.random.default_rng(63)
    alphabet = np.frombuffer(b"aaaaaabbbbbccc.*$\\^\x80\xffxy", np.uint8)
    pool = {}
    for L in TEXT_LENGTHS:
        pool[L] = [alphabet[rng.integers(0, len(alphabet), L)].tobytes() for _ in range(VARIANTS)]
    for v, at in enumerate((0, 517, 1100 - 63)):
        t = pool[1100][v]
        pool[1100][v] = t[:at] + gen.LIT63 + t[at + 63:]
    pool[1100][3] = pool[1100][3][:600] + gen.LIT63[:62] + b"#" + pool[1100][3][663:]  # all but the last item
    pool[1100][4] = pool[1100][4][:1100 - 62] + gen.LIT63[:62]                         # for LIT63[:62] + "$"
    assert all(len(t) == L for L, ts in pool.items() for t in ts)
    return pool


class Stored:
    """2049 objects under TYPES as stored keys and values, built once: values by struct.pack (u64
    version, u16 count, then u32 length and bytes per attribute, big-endian) with 0-3 bytes between
    them, so that the values, and with the varying lengths the attributes, start at every alignment."""
    _the = None

    @classmethod
    def get(cls):
        if cls._the is None:
            cls._the = cls()
        return cls._the

    def __init__(self, n=2049):
        rng = np.random.default_rng(2049)
        pool = text_pool()
        w = np.array(LENGTH_WEIGHTS, float) / sum(LENGTH_WEIGHTS)

        def text():
            return pool[TEXT_LENGTHS[int(rng.choice(len(TEXT_LENGTHS), p=w))]][int(rng.integers(VARIANTS))]
        self.objs = [(text(), [text(), q(int(rng.integers(-50, 50))), text()]) for _ in range(n)]
        keys, vals, self.key_off, self.val_off = bytearray(), bytearray(b"\xee"), [], []
        for i, (k, vs) in enumerate(self.objs):
            self.key_off.append(len(keys))
            keys += k
            vals += b"\xee" * (i % 4)
            self.val_off.append(len(vals))
            vals += struct.pack(">QH", 1000 + i, 3) + b"".join(struct.pack(">I", len(a)) + a for a in vs)
        self.keys = np.frombuffer(bytes(keys) + b"\0", np.uint8)
        self.vals = np.frombuffer(bytes(vals), np.uint8)
        self.key_off = np.array(self.key_off, np.uint64)
        self.val_off = np.array(self.val_off, np.uint64)
        self.key_len = np.array([len(k) for k, _ in self.objs], np.uint32)
        self.val_len = np.array([10 + sum(4 + len(a) for a in vs) for _, vs in self.objs], np.uint32)
        assert set((self.val_off % 4).tolist()) == {0, 1, 2, 3}
        starts = {(int(o) + 14 + len(vs[0]) + 4 + 8 + 4) % 4 for o, (_, vs) in zip(self.val_off, self.objs)}
        assert starts == {0, 1, 2, 3}  # the last attribute's text as well
        assert {len(k) for k, _ in self.objs} == set(TEXT_LENGTHS) == {len(vs[2]) for _, vs in self.objs}
        self._dev = None

    def want(self, checks, n=None):
        return np.array([expected_first_fail(TYPES, k, vs, checks) for k, vs in self.objs[:n]], np.uint32)

    def dev(self, torch, n=None, val_len=None):
        """The six tensors of the first n objects."""
        from test_encoded import _to_dev
        if self._dev is None:
            self._dev = _to_dev(torch, torch.device("cuda", 0), (self.keys, self.key_off, self.key_len, self.vals,
                                                                 self.val_off, self.val_len))
        d = list(self._dev)
        if val_len is not None:
            d[5] = _to_dev(torch, torch.device("cuda", 0), (val_len,))[0]
        if n is not None:
            d = [d[0], d[1][:n], d[2][:n], d[3], d[4][:n], d[5][:n]]
        return d


# The named cases: (checks, which first_fail values must each hold a tenth of the objects).
CASES = {
    "key": [rx(0, b"a.*b.*c")],
    "value": [rx(3, b"^a")],
    "value_end": [rx(1, b"b.$")],
    "two_on_one": [rx(1, b"a.*b"), rx(1, b"c.*a")],
    "behind": [AttributeCheck(2, q(0), INT64, GE), rx(1, b"ab")],
    "range": [rx(3, b"b.*a"), AttributeCheck(2, q(-30), INT64, GE), AttributeCheck(2, q(30), INT64, LE)],
    "bit63": [rx(3, gen.LIT63)],
    "four_16": [AttributeCheck(1, b"", STRING, GE), AttributeCheck(3, q(5000), INT64, LEN_LE),
                AttributeCheck(0, b"", STRING, GE), rx(0, b"a"),
                AttributeCheck(2, q(-50), INT64, GE), AttributeCheck(0, q(0), INT64, LEN_GE),
                AttributeCheck(3, b"\xff" * 3, STRING, LE), rx(1, b"b"),
                AttributeCheck(1, b"", STRING, GE), AttributeCheck(3, q(0), INT64, LEN_GE),
                AttributeCheck(0, b"", STRING, GE), rx(3, b"a.*a"),
                AttributeCheck(2, q(50), INT64, LE), AttributeCheck(1, q(5000), INT64, LEN_LE),
                AttributeCheck(0, b"", STRING, GE), rx(3, b"b.*b.*b")],
}
NO_REGEX = [AttributeCheck(1, q(8), INT64, LEN_GE), AttributeCheck(2, q(0), INT64, GE), AttributeCheck(0, b"b", STRING, LE)]


SIZE_CASES = ("two_on_one", "key")


def outcome_shares(want, c):
    return (want == c).mean(), (want != c).mean()


def test_device_cases_hold_both_outcomes():
    """The condition of every GPU test below, on the restatement alone: in each named case a tenth of the
    objects pass and a tenth fail (bit63: the long texts are over a quarter of the batch), the ladder cases
    fail at every index, and the edge sweep as a whole has both outcomes."""
    s = Stored.get()
    for name, cl in CASES.items():
        t, f = outcome_shares(s.want(cl), len(cl))
        assert t >= 0.10 and f >= 0.10, (name, t, f)
    assert set(s.want(CASES["behind"]).tolist()) == {0, 1, 2}
    assert set(s.want(CASES["range"]).tolist()) == {0, 1, 2, 3}
    assert {3, 7, 11, 15, 16} <= set(s.want(CASES["four_16"]).tolist())
    for n in SIZES[2:]:  # the size sweep's two lists, at every size that holds ten objects or more
        for name in SIZE_CASES:
            t, f = outcome_shares(s.want(CASES[name], n), len(CASES[name]))
            assert t >= 0.10 and f >= 0.10, (name, n, t, f)
    for attr in (0, 1, 3):  # the edge sweep, per attribute: the patterns pooled (the empty one matches everything)
        sweep = np.concatenate([s.want([rx(attr, p)], 257) for p in edge_patterns()])
        assert (sweep == 1).mean() >= 0.10 and (sweep == 0).mean() >= 0.10, attr


def edge_patterns():
    return [p for p in gen.EDGE_PATTERNS if item_count(p) <= 63]


def cap_lists():
    """test_checks.cap_list, the largest block of packed constants, and the same with a '^'-anchored REGEX
    op in place of check 0 (a list holds 16 checks at most): its table shares the workgroup's LDS with the
    staged constants, which all move down by one 72-byte slot; that block is 1 064 bytes, 72 short of the
    largest, and check 15's last byte still lies alone in its last word."""
    from test_checks import CAP_LAST, cap_list
    assert not set(CAP_LAST[:4]) & set(b".*\\$^")
    return {"cap": cap_list(), "cap_regex": [rx(1, b"^" + CAP_LAST[:4])] + cap_list()[1:]}


def cap_want(cl):
    from test_checks import CAP_TYPES, cap_objects
    return np.array([expected_first_fail(CAP_TYPES, k, vs, cl) for k, vs in cap_objects()], np.uint32)


def test_cap_lists_hold_both_outcomes():
    """The condition of test_gpu_constants_at_the_cap, on the restatement alone; and the host form."""
    from test_checks import CAP_TYPES, assert_cap_outcomes, cap_objects
    for name, cl in cap_lists().items():
        want = cap_want(cl)
        assert_cap_outcomes(want, 16)
        with CompiledChecks(CAP_TYPES, cl) as cc:
            assert [cc.passes(k, vs) for k, vs in cap_objects()] == want.tolist(), name


@pytest.fixture(scope="module")
def torch_gpu():
    import torch
    return torch


def run(torch, cc, d, want_match=True, stream=None):
    dev = torch.device("cuda", 0)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    ff, match = cc.check_encoded(*d, want_match=want_match, status=status, stream=stream)
    (stream or torch.cuda.current_stream(dev)).synchronize()
    return (ff.cpu().numpy().view(np.uint32), None if match is None else match.cpu().numpy().view(np.uint64),
            int(status.item()) & 0xffffffff)


def assert_result(got, want_ff, c, want_status=0):
    ff, match, status = got
    assert np.array_equal(ff, want_ff), np.nonzero(ff != want_ff)[0][:10]
    if match is not None:
        assert np.array_equal(match, np.nonzero(want_ff == c)[0].astype(np.uint64))
    assert status == want_status


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_gpu_cases(torch_gpu, name):
    """first_fail of every object and the match list against the restatement; without the list; twice."""
    s, cl = Stored.get(), CASES[name]
    want = s.want(cl)
    with CompiledChecks(TYPES, cl) as cc:
        first = run(torch_gpu, cc, s.dev(torch_gpu))
        assert_result(first, want, len(cl))
        again = run(torch_gpu, cc, s.dev(torch_gpu))
        assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
        got = run(torch_gpu, cc, s.dev(torch_gpu), want_match=False)
        assert got[1] is None
        assert_result(got, want, len(cl))


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_gpu_sizes(torch_gpu, n):
    s = Stored.get()
    for name in SIZE_CASES:
        cl = CASES[name]
        with CompiledChecks(TYPES, cl) as cc:
            assert_result(run(torch_gpu, cc, s.dev(torch_gpu, n)), s.want(cl, n), len(cl))


@pytest.mark.gpu
def test_gpu_edge_patterns(torch_gpu):
    """Every pattern of the fixture's edge list (up to 63 items) on the key and on both value strings."""
    s = Stored.get()
    d = s.dev(torch_gpu, 257)
    for p in edge_patterns():
        for attr in (0, 1, 3):
            with CompiledChecks(TYPES, [rx(attr, p)]) as cc:
                assert_result(run(torch_gpu, cc, d, want_match=False), s.want([rx(attr, p)], 257), 1)


@pytest.mark.gpu
def test_gpu_bad_encodings(torch_gpu):
    """Objects that do not decode: HDX_CHECK_BADENC and the status bit; the others as before."""
    s, cl = Stored.get(), CASES["two_on_one"]
    val_len = s.val_len.copy()
    bad = np.arange(5, 2049, 9)
    val_len[bad] -= 1  # the last attribute runs past the value
    want = s.want(cl)
    want[bad] = BADENC_FF
    with CompiledChecks(TYPES, cl) as cc:
        got = run(torch_gpu, cc, s.dev(torch_gpu, val_len=val_len))
    assert_result(got, want, 2, want_status=BADENC_BIT)
    assert not set(got[1].tolist()) & set(bad.tolist()) and len(got[1]) > 0


@pytest.mark.gpu
def test_gpu_constants_at_the_cap(torch_gpu):
    """test_checks.test_gpu_constants_at_the_cap through a compiled list, without and with a REGEX op ahead
    of the STRING comparisons.  One launch per list: a second one could find the first one's words still
    in LDS."""
    from test_checks import CAP_TYPES, cap_objects, encode, to_dev
    d = to_dev(torch_gpu, encode(CAP_TYPES, cap_objects(), "keycol"))
    for name, cl in cap_lists().items():
        want = cap_want(cl)
        with CompiledChecks(CAP_TYPES, cl) as cc:
            got = run(torch_gpu, cc, d)
        assert_result(got, want, 16)
        assert int(got[1].size) == int((want == 16).sum()) == 86, name


def sort_key(obj, attr):
    k, vs = obj
    if attr == 0:
        return k
    return struct.unpack("<q", vs[1])[0] if attr == 2 else vs[attr - 1]


def expected_top(objs, ff, c, spec, limit):
    """A Python sort of the matches: the kept end by (value, index), then the output's direction with
    ascending indices among ties."""
    idx = [i for i in range(len(objs)) if ff[i] == c]  # ascending
    kept = sorted(idx, key=lambda i: sort_key(objs[i], spec.attr), reverse=spec.keep == KEEP_LARGEST)[:limit]
    return sorted(sorted(kept), key=lambda i: sort_key(objs[i], spec.attr), reverse=bool(spec.descending))


@pytest.mark.gpu
def test_gpu_sorted_search(torch_gpu):
    torch = torch_gpu
    s = Stored.get()
    dev = torch.device("cuda", 0)
    for name in ("range", "two_on_one"):
        cl = CASES[name]
        want = s.want(cl)
        with CompiledChecks(TYPES, cl) as cc:
            for attr in (2, 1, 0):
                for keep in (KEEP_SMALLEST, KEEP_LARGEST):
                    for desc in (0, 1):
                        for limit in (0, 1, 100):
                            spec = SortSpec(attr, keep, desc)
                            status = torch.zeros(1, dtype=torch.int32, device=dev)
                            ff, top = cc.sorted_search(*s.dev(torch), spec, limit, status=status)
                            torch.cuda.synchronize()
                            assert np.array_equal(ff.cpu().numpy().view(np.uint32), want)
                            assert top.cpu().tolist() == expected_top(s.objs, want, len(cl), spec, limit), (spec, limit)
                            assert int(status.item()) == 0


@pytest.mark.gpu
def test_gpu_without_regex_equals_the_one_shot_forms(torch_gpu):
    torch = torch_gpu
    s = Stored.get()
    d = s.dev(torch)
    with CompiledChecks(TYPES, NO_REGEX) as cc:
        a = cc.check_encoded(*d)
        b = hdx.check_encoded(TYPES, *d, NO_REGEX)
        torch.cuda.synchronize()
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and 0 < a[1].numel() < 2049
        for spec in (SortSpec(2, KEEP_SMALLEST, 0), SortSpec(1, KEEP_LARGEST, 1)):
            a = cc.sorted_search(*d, spec, 100)
            b = hdx.sorted_search(TYPES, *d, NO_REGEX, spec, 100)
            torch.cuda.synchronize()
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[1].numel() == 100
    for cl in ([], [rx(2, b"a")], [rx(1, b"a", INT64)]):  # c == 0, and REGEX that is simply false
        with CompiledChecks(TYPES, cl) as cc:
            a = cc.check_encoded(*d)
            b = hdx.check_encoded(TYPES, *d, cl)
            torch.cuda.synchronize()
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.gpu
def test_gpu_side_stream(torch_gpu):
    """One call on a side stream behind a producer on that stream: the launches and the read of the
    count run on the given stream only."""
    torch = torch_gpu
    s, cl = Stored.get(), CASES["four_16"]
    d = [x.clone() for x in s.dev(torch)]
    staged = d[3].clone()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        d[3].zero_()  # the producer: a launch that escapes the stream reads zeros
        d[3].copy_(staged)
    with CompiledChecks(TYPES, cl) as cc:
        assert_result(run(torch, cc, d, stream=side), s.want(cl), 16)
    torch.cuda.synchronize()
