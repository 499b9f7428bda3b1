"""Inputs for the reference-hash pin, and the generator of its fixture.

tests/golden/reference_hash_values.json holds what the reference's own
hash(hyperdatatype, slice) — compiled unmodified into
oracle/_ref/libref_hash.so (oracle/Makefile, `make ref`) — returns for the
inputs built here.  The fixture is data only: inputs and the reference's
outputs.  No restatement (oracle/hdx_oracle.c, hdx_cpu.cpp, the kernels) takes
part in producing it.

    python tests/golden/make_reference_hash_values.py        # needs libref_hash.so

tests/test_reference_hash.py imports this module for the input lists (the
full ones of its CPU comparison and the trimmed one of the fixture) and, where
libref_hash.so is built, regenerates the fixture and compares it with the
committed file.

Everything random comes from a counter-based splitmix64 written out below, so
the lists do not depend on numpy's generators.
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "reference_hash_values.json")

STRING, INT64, FLOAT = 9217, 9218, 9219
TIMESTAMPS = tuple(range(9473, 9479))   # second, minute, hour, day, week, month
NUMERIC_TYPES = (INT64, FLOAT) + TIMESTAMPS
M64 = (1 << 64) - 1


def rnd(stream: int, n: int) -> np.ndarray:
    """n uint64 of splitmix64's finaliser over (stream, counter)."""
    k = np.arange(1, n + 1, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64((stream * 0xd1b54a32d192ed03) & M64) + k * np.uint64(0x9e3779b97f4a7c15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xbf58476d1ce4e5b9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94d049bb133111eb)
    return z ^ (z >> np.uint64(31))


def u64(values) -> np.ndarray:
    return np.array([int(v) & M64 for v in values], dtype=np.uint64)


# ---- strings -----------------------------------------------------------------------

STRING_BLOB_BYTES = 8192
FIXTURE_STRING_LENGTHS = list(range(521)) + [1023, 1024, 1025, 4096]


def string_blob(nbytes: int = STRING_BLOB_BYTES, stream: int = 1) -> np.ndarray:
    return rnd(stream, (nbytes + 7) // 8).view(np.uint8)[:nbytes].copy()


def fixture_string_cases():
    """(offset, len) into string_blob(): every length 0..520 and 1023 / 1024 /
    1025 / 4096, at offsets whose low four bits take every value."""
    cases = [((37 * i) % 4096, n) for i, n in enumerate(FIXTURE_STRING_LENGTHS)]
    assert all(off + n <= STRING_BLOB_BYTES for off, n in cases)
    assert {off % 16 for off, _ in cases} == set(range(16))
    return cases


# ---- eight-byte patterns -------------------------------------------------------------

# the specials of test_gpu_parity.py::test_float_and_int_specials
SPECIALS = [0, 1 << 63, 0x7ff0000000000000, 0xfff0000000000000, 0x7ff8000000000000,
            0xfff8000000000001, 0x7ff0000000000001, 0xfff0000000000001, 1, (1 << 63) | 1,
            0x000fffffffffffff, 0x800fffffffffffff, 0x0010000000000000, 0x8010000000000000,
            0x7fefffffffffffff, 0xffefffffffffffff, 0x3ff0000000000000, 0xbff0000000000000,
            0x7fffffffffffffff, 0xffffffffffffffff]

# 0, +-1, 2^53 +- 1, 2^63 - 1, 2^63 as int64 timestamps (two's complement)
TIMESTAMP_SPECIALS = [0, 1, M64, (1 << 53) - 1, (1 << 53) + 1, (1 << 63) - 1, 1 << 63]

# microsecond timestamps of 2014 / 2015 (tests/golden/reference_values.json) and around them
REALISTIC_TIMESTAMPS = [1420666849000000, 1389130849000000, 1420666849999999, 1420666850000000,
                        1420070400000000, 1420070399999999, 978307200000000, 4102444800000000]

RADIX = (60, 60, 24, 7, 4, 12)


def radix_boundaries() -> np.ndarray:
    """Where a digit of the timestamp hash's mixed radix 60.60.24.7.4.12 (over
    whole seconds) rolls over: 1 s and each cumulative product, in
    microseconds, and one microsecond either side."""
    out, p = [], 1
    for r in (1,) + RADIX:
        p *= r
        out += [p * 10**6 - 1, p * 10**6, p * 10**6 + 1]
    return u64(out)


def exponent_boundaries(exponents=range(2048)) -> np.ndarray:
    """Both ends of every binade of both signs: mantissa all zeros and all ones."""
    out = []
    for e in exponents:
        for sign in (0, 1 << 63):
            out += [sign | (e << 52), sign | (e << 52) | ((1 << 52) - 1)]
    return u64(out)


FIXTURE_EXPONENTS = (0, 1, 2, 1022, 1023, 1024, 1075, 1086, 2045, 2046, 2047)


def nan_payloads(n: int, stream: int = 2) -> np.ndarray:
    """Quiet and signalling NaNs of both signs with random non-zero payloads."""
    r = rnd(stream, n)
    frac = (r & np.uint64((1 << 52) - 1)) | np.uint64(1)
    quiet = np.where((np.arange(n) & 2) != 0, np.uint64(1 << 51), np.uint64(0))
    frac = (frac & np.uint64(~(1 << 51) & M64)) | quiet
    sign = np.where((np.arange(n) & 1) != 0, np.uint64(1 << 63), np.uint64(0))
    return sign | np.uint64(0x7ff << 52) | frac


def subnormals(n: int, stream: int = 3) -> np.ndarray:
    """Subnormals of both signs over every magnitude (the top set bit cycles)."""
    r = rnd(stream, n)
    shift = (12 + np.arange(n) % 52).astype(np.uint64)
    frac = (r >> shift) | np.uint64(1)
    sign = np.where((np.arange(n) & 1) != 0, np.uint64(1 << 63), np.uint64(0))
    return sign | frac


def double_quotient(t: np.ndarray) -> np.ndarray:
    """uint64_t(t / 1000000.) of datatype_timestamp.cc:198: u64 -> f64 (round to
    nearest), IEEE divide, truncation."""
    return (np.asarray(t, np.uint64).astype(np.float64) / 1000000.0).astype(np.uint64)


def integer_quotient(t: np.ndarray) -> np.ndarray:
    return np.asarray(t, np.uint64) // np.uint64(1000000)


def rounding_edge_timestamps(candidates: int = 4096, stream: int = 4) -> np.ndarray:
    """Timestamps whose double quotient differs from integer division — what an
    integer divide, or a double divide that is not correctly rounded, gets
    wrong.  Candidates are k * 10^6 - 1 with k cycling through 2^33 .. 2^44
    (t from 2^53 to past 2^63, so negative int64 too); kept where the two
    quotients differ."""
    r = rnd(stream, candidates)
    shift = (20 + np.arange(candidates) % 12).astype(np.uint64)
    k = (r >> shift) | (np.uint64(1) << (np.uint64(63) - shift))
    k = np.minimum(k, np.uint64(M64 // 10**6))
    t = k * np.uint64(10**6) - np.uint64(1)
    return t[double_quotient(t) != integer_quotient(t)]


def random_patterns(n: int, stream: int = 5) -> np.ndarray:
    return rnd(stream, n)


def full_numeric_patterns(t: int) -> np.ndarray:
    """The CPU comparison's list for numeric type t (tests/test_reference_hash.py)."""
    parts = [u64(SPECIALS), exponent_boundaries(), nan_payloads(512), subnormals(512), random_patterns(50000, 5 + t)]
    if t in TIMESTAMPS:
        parts += [u64(TIMESTAMP_SPECIALS), u64(REALISTIC_TIMESTAMPS), radix_boundaries(), rounding_edge_timestamps()]
    return np.concatenate(parts)


FIXTURE_ROUNDING_EDGES = 72
FIXTURE_RANDOM = 80


def fixture_patterns():
    """(patterns, groups): the fixture's one list of eight-byte patterns, hashed
    under each of the eight numeric types, and groups[name] = (first, count).
    Trimmed from the lists above; only the random tail may shrink."""
    parts = [("specials", u64(SPECIALS)),
             ("timestamp_specials", u64(TIMESTAMP_SPECIALS)),
             ("realistic_timestamps", u64(REALISTIC_TIMESTAMPS)),
             ("radix_boundaries", radix_boundaries()),
             ("rounding_edges", rounding_edge_timestamps()[:FIXTURE_ROUNDING_EDGES]),
             ("exponent_boundaries", exponent_boundaries(FIXTURE_EXPONENTS)),
             ("nan_payloads", nan_payloads(8)),
             ("subnormals", subnormals(8, stream=6)),
             ("random", random_patterns(FIXTURE_RANDOM))]
    groups, first = {}, 0
    for name, p in parts:
        groups[name] = [first, len(p)]
        first += len(p)
    return np.concatenate([p for _, p in parts]), groups


def pattern_bytes(patterns: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(patterns, dtype="<u8").view(np.uint8)


# ---- the fixture ---------------------------------------------------------------------------

def build_fixture(oracle) -> dict:
    """The fixture as a dict, from oracle.ref_hash_lib() (which must be built)."""
    assert oracle.ref_hash_lib() is not None, "oracle/_ref/libref_hash.so is not built (make -C oracle ref)"
    blob = string_blob()
    cases = fixture_string_cases()
    h, err = oracle.ref_hash_values(STRING, blob, [o for o, _ in cases], [n for _, n in cases])
    assert err == 0
    strings = {"blob_bytes": len(blob), "blob_sha256": hashlib.sha256(blob.tobytes()).hexdigest(),
               "cases": [[o, n, "%016x" % int(x)] for (o, n), x in zip(cases, h)]}
    patterns, groups = fixture_patterns()
    raw = pattern_bytes(patterns)
    off = np.arange(len(patterns), dtype=np.uint64) * np.uint64(8)
    hashes = {}
    for t in NUMERIC_TYPES:
        h, err = oracle.ref_hash_values(t, raw, off, np.full(len(patterns), 8, np.uint32))
        assert err == 0
        empty, err = oracle.ref_hash(t, b"")
        assert err == 0
        hashes[str(t)] = {"empty": "%016x" % empty, "values": ["%016x" % int(x) for x in h]}
    return {"source": "hyperdex::hash(hyperdatatype, e::slice) of the reference's common/hash.cc, "
                      "common/datatype_{string,int64,float,timestamp}.cc, common/ordered_encoding.cc and "
                      "cityhash/city.cc, compiled unmodified (oracle/Makefile: _ref/libref_hash.so); inputs from "
                      "tests/golden/make_reference_hash_values.py",
            "strings": strings,
            "numerics": {"patterns": ["%016x" % int(p) for p in patterns], "groups": groups, "hashes": hashes}}


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
