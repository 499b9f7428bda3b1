"""Inputs for the attribute-check pin, and the generator of its fixture.

tests/golden/reference_check_values.json holds what the reference's own
passes_attribute_check, passes_attribute_checks (common/attribute_check.cc) and
datatype_*::compare — compiled unmodified into oracle/_ref/libref_checks.so
(oracle/Makefile, `make ref`) — return for the inputs built here.  The fixture
is data only: a digest of the inputs, the reference's results and the counts
the tests assert.  No restatement (include/hdxhash.h's table, hdx_cpu.cpp, the
kernels, the tests' Python) takes part in producing it.

    python tests/golden/make_reference_check_values.py      # needs libref_checks.so

Three parts, each a matrix so that one device launch answers a whole row:
  single   per attribute type T, the bits of check_pool(T) x value_pool(T);
  lists    the first failing index of every list of lists() on every object of
           objects() under the ten-attribute SCHEMA;
  compare  per type, the sign of compare(a, b) over compare_pool(T) squared.

tests/test_reference_checks.py imports this module for the inputs and, where
libref_checks.so is built, regenerates the fixture and compares it with the
committed file.  Everything random comes from make_reference_hash_values.py's
counter-based splitmix64; the pools are written out by hand.
"""
import hashlib
import importlib.util
import json
import os
import struct
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "reference_check_values.json")


def _load_hash_generator():
    spec = importlib.util.spec_from_file_location("make_reference_hash_values",
                                                  os.path.join(HERE, "make_reference_hash_values.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


hgen = _load_hash_generator()

STRING, INT64, FLOAT = 9217, 9218, 9219
TIMESTAMPS = tuple(range(9473, 9479))   # second, minute, hour, day, week, month
TYPES = (STRING, INT64, FLOAT) + TIMESTAMPS
FAIL, EQ, LE, GE, CLT, REGEX, LEN_EQ, LEN_LE, LEN_GE, CONTAINS, LT, GT = range(9728, 9740)
BELOW_ENUM, ABOVE_ENUM = 9727, 9740
PREDICATES = (BELOW_ENUM,) + tuple(range(9728, 9740)) + (ABOVE_ENUM,)
ORDERING = (EQ, LT, LE, GE, GT)
LENGTH = (LEN_EQ, LEN_LE, LEN_GE)


def q(x):
    return struct.pack("<q", x)


def d(x):
    return struct.pack("<d", x)


# ---- the hand-written pools --------------------------------------------------------------------

BASE = bytes((7 * i + 33) & 0xff for i in range(41))     # test_checks.BASE; no byte is special in a pattern
LONG = hgen.rnd(301, 138).view(np.uint8)[:1100].tobytes()


def flip(b, pos):
    return b[:pos] + bytes([b[pos] ^ 0x40]) + b[pos + 1:]


PAIRS = [b"\x7f", b"\x80", b"ab\x7f", b"ab\x80", b"abcdefg\x7f", b"abcdefg\x80", b"abcdefgh\x7fx", b"abcdefgh\x80x"]
# the empty string; lengths 1..17 (every tail length of a word and of two); BASE and BASE differing at one
# byte, 7 / 8 / 15 / 16 among them; one word differing at each of its bytes; the 0x7f / 0x80 pairs; 1000
# and 1100 bytes, the latter differing at its last byte.  Lengths 8 and 41 are common on purpose: LENGTH_EQUALS
# needs lengths that a tenth of the pool shares.
V_STRING = ([b""] + [BASE[:L] for L in range(1, 18)] + [BASE] + [flip(BASE, p) for p in (0, 1, 3, 4, 7, 8, 15, 16,
                                                                                        23, 24, 31, 32, 39, 40)]
            + [flip(BASE[:8], p) for p in range(8)] + PAIRS + [LONG[:1000], LONG, flip(LONG, 1099)])
I64 = [q(x) for x in (-2 ** 63, -1, 0, 1, 2 ** 63 - 1)] + [b""]                    # test_checks.I64
NAN_POS, NAN_NEG = struct.pack("<Q", 0x7ff8000000000001), struct.pack("<Q", 0xfff0000000000123)
F64 = [d(x) for x in (0.0, -0.0, float("inf"), float("-inf"), 5e-324, 1.5)] + [NAN_POS, NAN_NEG, b""]  # test_checks.F64
MIS_SIZED = [bytes([0x11] * L) for L in (1, 2, 3, 4, 5, 6, 7, 9)]                    # test_checks.MIS_SIZED
MIS3 = MIS_SIZED[2]


def value_pool(T):
    """V_T: the stored values of the single-check matrix."""
    return V_STRING if T == STRING else (F64 if T == FLOAT else I64) + MIS_SIZED


# check values for D == T.  EQUALS: members, the classes that compare equal without equal bytes (0 and the
# empty value; 0.0, -0.0; a NaN against anything), a mis-sized one.  The other four: members, one value
# either side of a member, the empty value, a mis-sized one.  No value is longer than 1000 bytes: the
# device forms cap a list's bytes at 1024.
BELOW_16 = BASE[:15] + bytes([BASE[15] - 1])
ABOVE_16 = BASE[:16] + b"\0"
K_EQ = {STRING: [b"", BASE[:8], BASE, LONG[:1000]],
        INT64: [q(0), b"", q(1), MIS3],
        FLOAT: [d(0.0), d(-0.0), b"", NAN_POS, NAN_NEG, d(1.5), d(float("inf")), d(2.5), MIS3]}
K_ORD = {STRING: [b"", BASE[:8], BASE[:16], BELOW_16, ABOVE_16, BASE, b"\x7f", b"\x80", LONG[:1000], b"\xff\xff"],
         INT64: [q(0), b"", q(1), q(-1), q(2), q(-2), q(2 ** 63 - 1), q(-2 ** 63), MIS3],
         FLOAT: [d(0.0), d(-0.0), b"", d(1.5), d(1.25), d(2.5), d(float("inf")), d(float("-inf")), d(5e-324),
                 d(-5e-324), NAN_POS, MIS3]}
# INT64 check values of the length predicates on a STRING: around the pool's lengths; 3 bytes and 9 bytes
# (not an INT64: false, though the first bytes spell 8) and the empty value (0)
K_LEN_EQ = [q(8), q(41), b"", q(8)[:3], q(8) + b"\0"]
K_LEN = K_LEN_EQ + [q(0), q(-1), q(1), q(7), q(9), q(16), q(17), q(40), q(1000), q(1100), q(1101), q(2 ** 63 - 1)]
# patterns of make_reference_regex_values.EDGE_PATTERNS that go both ways on V_STRING
REGEX_PATTERNS = [b"", b"^$", b"..", b"^..$", b"a", b"\x80", b"^abc", b".*\x80$", b"a.*b", b"ab$", b"^a.*b$"]


def _k(table, T):
    return table[T if T in (STRING, FLOAT) else INT64]


def reachable(T, D, p):
    """The types alone let predicate p compare: attribute_check.cc's conditions on datatype(), comparable(),
    has_length() and has_regex() for the nine primitive types."""
    if p in ORDERING:
        return T == D
    if p in LENGTH or p == CLT:
        return T == STRING and D == INT64
    if p == REGEX:
        return T == STRING and D == STRING
    return False


def check_pool(T):
    """C_T: [(D, predicate, k)].  First the rows whose types let the predicate compare, with the pools
    above; then every other (predicate, D) of the fourteen predicate values and the nine datatypes with
    three values: a member of V_T (8 bytes, so it validates under any D), the empty value, 3 bytes."""
    rows = [(T, EQ, k) for k in _k(K_EQ, T)]
    rows += [(T, p, k) for p in (LT, LE, GE, GT) for k in _k(K_ORD, T)]
    if T == STRING:
        rows += [(INT64, LEN_EQ, k) for k in K_LEN_EQ]
        rows += [(INT64, p, k) for p in (LEN_LE, LEN_GE, CLT) for k in K_LEN]
        rows += [(STRING, REGEX, k) for k in REGEX_PATTERNS]
    member = BASE[:8] if T == STRING else value_pool(T)[3]
    assert len(member) == 8 and member in value_pool(T)
    for p in PREDICATES:
        for D in TYPES:
            if not reachable(T, D, p):
                rows += [(D, p, k) for k in (member, b"", MIS3)]
    assert len(set(rows)) == len(rows)
    return rows


def compare_pool(T):
    """Well-sized values only; the NaNs are in, so that the reference's 0 is on record."""
    if T == STRING:
        return V_STRING
    if T == FLOAT:
        return F64 + [d(x) for x in (-1.5, 2.5, -5e-324, 1.25)]
    return I64 + [q(x) for x in (256, -256, 1 << 32, -(1 << 32), 1 << 56)]


# ---- the lists ---------------------------------------------------------------------------------

SCHEMA = [STRING, STRING, INT64, FLOAT] + list(TIMESTAMPS)   # a STRING key and one attribute of each type
OBJECTS = 259
TS_SEC, TS_MIN, TS_HOUR, TS_DAY, TS_WEEK, TS_MONTH = TIMESTAMPS

# (attr, k, D, predicate)
HAND_LISTS = [
    [],
    [(2, q(0), INT64, EQ)],
    # a ladder: fails at every index, and passes
    [(1, q(3), INT64, LEN_GE), (2, q(-1), INT64, GE), (0, BASE[:16], STRING, LT), (3, d(1.5), FLOAT, LE),
     (6, q(1), TS_HOUR, GE), (1, b"^!(/6=D", STRING, REGEX)],
    [(0, b"", STRING, GE), (1, q(2 ** 62), INT64, CLT), (9, b"", TS_MONTH, EQ)],
    # beyond the schema: attr == attrs_sz behind a true check, and 0xffff
    [(0, b"", STRING, GE), (10, b"", STRING, EQ), (1, b"", STRING, GE)],
    [(0xffff, b"", STRING, GE)],
    # repeated attributes
    [(1, BASE[:8], STRING, GE), (1, flip(BASE, 40), STRING, LE), (1, q(8), INT64, LEN_GE), (1, BASE, STRING, GT)],
    [(0, q(1), INT64, LEN_GE), (0, q(41), INT64, LEN_LE), (0, BASE[:8], STRING, GE), (0, b"^!", STRING, REGEX)],
    # REGEX: on the key and an attribute, behind a range, four in one list, on a numeric (false)
    [(0, b"..", STRING, REGEX), (1, b"!.*6", STRING, REGEX)],
    [(2, q(0), INT64, GE), (1, b"^!(/6", STRING, REGEX)],
    [(1, b"", STRING, REGEX), (0, b".", STRING, REGEX), (1, b"^.", STRING, REGEX), (0, b"(/", STRING, REGEX),
     (2, q(2 ** 63 - 1), INT64, LE)],
    [(0, b"", STRING, GE), (2, b"", STRING, REGEX)],
    [(1, b"a", INT64, REGEX)],
    # sixteen true checks
    [(1, b"", STRING, GE), (0, q(5000), INT64, LEN_LE), (0, b"", STRING, GE), (1, b"\xff" * 2, STRING, LT),
     (1, q(2 ** 62), INT64, CLT), (0, q(-1), INT64, LEN_GE), (0, b"", STRING, REGEX), (1, q(0), INT64, LEN_GE)] * 2,
    # equal without equal bytes; another granularity; a mis-sized check value
    [(3, NAN_POS, FLOAT, EQ), (2, b"", INT64, EQ)],
    [(3, d(-0.0), FLOAT, EQ)],
    [(4, q(0), TS_MIN, LE)],
    [(4, q(0), TS_SEC, LE), (5, q(0), TS_MIN, GE), (7, b"", TS_DAY, EQ), (8, q(1), TS_WEEK, LT)],
    [(2, b"\1\2\3", INT64, LE)],
    [(1, LONG[:1000], STRING, LT), (0, flip(BASE, 16)[:19], STRING, GE)],
]
RANDOM_LISTS = 16


def _draw(r, pool):
    return pool[int(r % np.uint64(len(pool)))]


def random_lists():
    """Lists of 0..16 checks drawn from the comparing rows of check_pool(type of the attribute), short
    check values only, at most four REGEX each (the compiled form's cap)."""
    r = hgen.rnd(302, RANDOM_LISTS * 64).reshape(RANDOM_LISTS, 64)
    pools = {T: [c for c in check_pool(T) if reachable(T, c[0], c[1]) and len(c[2]) <= 41] for T in set(SCHEMA)}
    out = []
    for i in range(RANDOM_LISTS):
        n, cl, rx = int(r[i, 0] % np.uint64(17)), [], 0
        for j in range(n):
            attr = int(r[i, 1 + 3 * j] % np.uint64(len(SCHEMA)))
            if r[i, 2 + 3 * j] % np.uint64(4) == 0:
                attr = 0 if j & 1 else 1  # strings more often: their checks pass more often
            D, p, k = _draw(r[i, 3 + 3 * j], pools[SCHEMA[attr]])
            if p == REGEX:
                rx += 1
                if rx > 4:
                    continue
            cl.append((attr, k, D, p))
        out.append(cl)
    return out


# checks that hold for most well-sized values: a long list of them fails where an object's first mis-sized
# numeric is named, so the later checks of a list decide too
WIDE = {STRING: [(STRING, GE, b""), (STRING, LE, b"\xff\xff"), (INT64, LEN_GE, q(0)), (INT64, LEN_LE, q(1100)),
                 (STRING, REGEX, b""), (INT64, LEN_GE, q(1)), (INT64, CLT, q(1000))],
        INT64: [(INT64, GE, q(-2 ** 63)), (INT64, LE, q(2 ** 63 - 1)), (INT64, GE, q(-1)), (INT64, LE, q(1))],
        FLOAT: [(FLOAT, GE, d(float("-inf"))), (FLOAT, LE, d(float("inf"))), (FLOAT, EQ, NAN_NEG), (FLOAT, LE, d(1.5))]}
WIDE_LENGTHS = (16, 16, 13, 10, 7, 4)


def wide_lists():
    r = hgen.rnd(304, len(WIDE_LENGTHS) * 32).reshape(len(WIDE_LENGTHS), 32)
    out = []
    for i, n in enumerate(WIDE_LENGTHS):
        cl, rx = [], 0
        for j in range(n):
            attr = int(r[i, 2 * j] % np.uint64(len(SCHEMA)))
            T = SCHEMA[attr]
            D, p, k = _draw(r[i, 2 * j + 1], _k(WIDE, T))
            rx += p == REGEX
            if p == REGEX and rx > 4:
                D, p, k = WIDE[STRING][0]
            cl.append((attr, k, T if D == INT64 and T in TIMESTAMPS else D, p))
        out.append(cl)
    return out


def lists():
    return HAND_LISTS + random_lists() + wide_lists()


def objects():
    """[(key, [nine attributes])] under SCHEMA from the value pools; one numeric in eight is mis-sized."""
    r = hgen.rnd(303, OBJECTS * 20).reshape(OBJECTS, 20)
    short = [s for s in V_STRING if len(s) <= 41]
    out = []
    for i in range(OBJECTS):
        vals = []
        for a, T in enumerate(SCHEMA):
            if T == STRING:
                vals.append(_draw(r[i, 2 * a], V_STRING if r[i, 2 * a + 1] % np.uint64(8) == 0 else short))
            elif r[i, 2 * a + 1] % np.uint64(8) == 0:
                vals.append(_draw(r[i, 2 * a], MIS_SIZED))
            else:
                vals.append(_draw(r[i, 2 * a], F64 if T == FLOAT else I64))
        out.append((vals[0], vals[1:]))
    return out


# ---- digests and encodings -----------------------------------------------------------------------

def _h(h, b):
    h.update(len(b).to_bytes(4, "little") + b)


def single_sha256(T):
    h = hashlib.sha256()
    for v in value_pool(T):
        _h(h, v)
    for D, p, k in check_pool(T):
        h.update(struct.pack("<II", D, p))
        _h(h, k)
    return h.hexdigest()


def lists_sha256():
    h = hashlib.sha256()
    h.update(struct.pack("<%dI" % len(SCHEMA), *SCHEMA))
    for key, vals in objects():
        for v in [key] + vals:
            _h(h, v)
    for cl in lists():
        h.update(struct.pack("<I", len(cl)))
        for attr, k, D, p in cl:
            h.update(struct.pack("<III", attr, D, p))
            _h(h, k)
    return h.hexdigest()


def compare_sha256(T):
    h = hashlib.sha256()
    for v in compare_pool(T):
        _h(h, v)
    return h.hexdigest()


def pack_bits(bits):
    """One bit per case, case i at bit i % 8 of byte i // 8, as hex."""
    return np.packbits(np.asarray(bits, np.uint8).reshape(-1), bitorder="little").tobytes().hex()


def unpack_bits(text, rows, cols):
    return np.unpackbits(np.frombuffer(bytes.fromhex(text), np.uint8), bitorder="little")[:rows * cols] \
        .astype(bool).reshape(rows, cols)


FF_DIGITS = "0123456789abcdefg"   # a first failing index, 0..16
SIGNS = "<=>"                     # compare's sign, -1 / 0 / 1


# ---- the conditions, on the results alone ------------------------------------------------------------

def outcome_counts(passes):
    """{predicate or "regex": [true, cases]} over the single-check rows whose types let the predicate
    compare; passes[T] is the bit matrix of check_pool(T) x value_pool(T)."""
    out = {}
    for T in TYPES:
        for (D, p, k), row in zip(check_pool(T), passes[T]):
            if reachable(T, D, p) and p != CLT:
                c = out.setdefault(p, [0, 0])
                c[0] += int(np.sum(row))
                c[1] += len(row)
    return out


def assert_conditions(passes, first_fail, signs):
    counts = outcome_counts(passes)
    assert set(counts) == set(ORDERING + LENGTH + (REGEX,))
    for p, (t, n) in counts.items():
        assert 0.10 * n <= t <= 0.90 * n, (p, t, n)
    cls = lists()
    seen = any(len(cl) >= 3 and set(ff) == set(range(len(cl) + 1)) for cl, ff in zip(cls, first_fail))
    assert seen, "no list of three or more checks fails at every index and passes"
    for T in TYPES:
        assert set(np.unique(signs[T]).tolist()) == {-1, 0, 1}, T
    return counts


# ---- the fixture ---------------------------------------------------------------------------------

def reference_results(oracle):
    """(passes, first_fail, signs) from oracle/_ref/libref_checks.so."""
    assert oracle.ref_checks() is not None, "oracle/_ref/libref_checks.so is not built (make -C oracle ref)"
    passes, signs = {}, {}
    for T in TYPES:
        V = value_pool(T)
        passes[T] = np.array([[oracle.ref_passes_attribute_check(T, D, p, k, v) for v in V]
                              for D, p, k in check_pool(T)], bool)
        P = compare_pool(T)
        m = np.zeros((len(P), len(P)), np.int8)
        for i, a in enumerate(P):
            for j, b in enumerate(P):
                m[i, j], err = oracle.ref_compare(T, a, b)
                assert err == 0
        signs[T] = m
    objs = objects()
    first_fail = [[oracle.ref_passes_attribute_checks(SCHEMA, cl, key, vals) for key, vals in objs] for cl in lists()]
    return passes, first_fail, signs


def build_fixture(oracle) -> dict:
    passes, first_fail, signs = reference_results(oracle)
    counts = assert_conditions(passes, first_fail, signs)
    cls = lists()
    assert len(cls) >= 32 and OBJECTS >= 257 and all(len(cl) <= 16 for cl in cls)
    assert all(0 <= x <= len(cl) for cl, ff in zip(cls, first_fail) for x in ff)
    return {
        "source": "passes_attribute_check and passes_attribute_checks of the reference's common/attribute_check.cc and "
                  "compare of its common/datatype_{string,int64,float,timestamp}.cc, compiled unmodified "
                  "(oracle/Makefile: _ref/libref_checks.so); inputs from tests/golden/make_reference_check_values.py",
        "single": {str(T): {"checks": len(check_pool(T)), "values": len(value_pool(T)),
                            "inputs_sha256": single_sha256(T), "passes": pack_bits(passes[T])} for T in TYPES},
        "lists": {"lists": len(cls), "objects": OBJECTS, "inputs_sha256": lists_sha256(),
                  "first_fail": ["".join(FF_DIGITS[x] for x in ff) for ff in first_fail]},
        "compare": {str(T): {"values": len(compare_pool(T)), "inputs_sha256": compare_sha256(T),
                             "sign": "".join(SIGNS[int(s) + 1] for s in signs[T].reshape(-1))} for T in TYPES},
        "counts": {"single_cases": int(sum(m.size for m in passes.values())),
                   "list_cases": len(cls) * OBJECTS,
                   "compare_cases": int(sum(m.size for m in signs.values())),
                   "true_of_comparing_cases": {str(p): c for p, c in sorted(counts.items())}},
    }


def load(fx):
    """(passes, first_fail, signs) of a fixture dict, the inputs checked against its digests."""
    passes, signs = {}, {}
    for T in TYPES:
        s, c = fx["single"][str(T)], fx["compare"][str(T)]
        assert s["inputs_sha256"] == single_sha256(T) and c["inputs_sha256"] == compare_sha256(T), T
        assert (s["checks"], s["values"], c["values"]) == (len(check_pool(T)), len(value_pool(T)), len(compare_pool(T)))
        passes[T] = unpack_bits(s["passes"], s["checks"], s["values"])
        assert len(c["sign"]) == c["values"] ** 2
        signs[T] = np.array([SIGNS.index(ch) - 1 for ch in c["sign"]], np.int8).reshape(c["values"], c["values"])
    L = fx["lists"]
    assert L["inputs_sha256"] == lists_sha256() and (L["lists"], L["objects"]) == (len(lists()), OBJECTS)
    first_fail = [[FF_DIGITS.index(ch) for ch in row] for row in L["first_fail"]]
    assert all(len(row) == OBJECTS for row in first_fail) and len(first_fail) == L["lists"]
    return passes, first_fail, signs


def dumps(fixture: dict) -> str:
    return json.dumps(fixture, indent=0, separators=(",", ":"), sort_keys=True) + "\n"


def main(out=FIXTURE):
    sys.path.insert(0, ROOT)
    from oracle import oracle
    text = dumps(build_fixture(oracle))
    with open(out, "w") as f:
        f.write(text)
    print("wrote", out, len(text), "bytes")


if __name__ == "__main__":
    main(*sys.argv[1:])
