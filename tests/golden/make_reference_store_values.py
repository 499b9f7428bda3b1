"""Inputs for the stored-value / index-key / partition pin, and the generator of its fixture.

tests/golden/reference_store_values.json holds what the reference's own
encode_value / decode_value (daemon/datalayer_encodings.cc), numeric index
encoders (daemon/index_{int64,float,timestamp}.cc) and partition()
(admin/partition.cc) — compiled unmodified into oracle/_ref/libref_store.so —
and its hash() (oracle/_ref/libref_hash.so) return for the inputs built here.
The fixture is data only: digests of the inputs and the reference's outputs.
No restatement (oracle/hdx_oracle.c, hdx_cpu.cpp, the kernels, synth) takes
part in producing it.

    python tests/golden/make_reference_store_values.py    # needs libref_store.so, libref_hash.so

tests/test_reference_store.py imports this module for the inputs and, where
the two libraries are built, regenerates the fixture and compares it with the
committed file.

The stored values are written here by a plain struct.pack of the layout
(version, count, length-prefixed attributes) and then damaged on purpose;
build_fixture() checks every undamaged one byte for byte against the
reference's encode_value, and the fixture pins every value's bytes by SHA-256.
Everything random comes from make_reference_hash_values.py's counter-based
splitmix64.
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
FIXTURE = os.path.join(HERE, "reference_store_values.json")


def _load_hash_generator():
    spec = importlib.util.spec_from_file_location("make_reference_hash_values",
                                                  os.path.join(HERE, "make_reference_hash_values.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


hgen = _load_hash_generator()
STRING, INT64, FLOAT, TIMESTAMPS = hgen.STRING, hgen.INT64, hgen.FLOAT, hgen.TIMESTAMPS
NUMERIC_TYPES = hgen.NUMERIC_TYPES
M64 = hgen.M64

# ---- stored values ---------------------------------------------------------------------

# name -> (types, number of values, longest string); attribute 0 is the key.
# a5 = config 2's types, a17 = config 3b's, a129 cycles string / int64 / float,
# a9 holds every hashable type (timestamps: the sweep's form without NUM2).
SCHEMAS = {
    "a1": ((STRING,), 32, 64),
    "a2": ((STRING, STRING), 32, 60),
    "a5": ((STRING,) + (INT64,) * 4, 32, 64),
    "a17": ((STRING,) * 11 + (INT64,) * 3 + (FLOAT,) * 3, 32, 100),
    "a129": (tuple((STRING, INT64, FLOAT)[j % 3] for j in range(129)), 24, 24),
    "a9": ((STRING, INT64, FLOAT) + TIMESTAMPS, 16, 40),
}
# a9 exists to reach the sweep's other form: one damaged value of each sort
A9_MALFORMED = ("len9", "cut2", "mid_overrun", "count65535", "count_m2", "count_A", "last_over1", "last_over2g")

WELL_FORMED = ("ok", "ok_empty", "ok_v0", "ok_vmax", "ok_trailing")
# refused by the reference (class b); count65535's prefixes never fit in these values
REFUSED = ("len0", "len7", "len8", "len9", "cut0", "cut1", "cut2", "cut3", "mid_overrun", "count65535")
CLASS_C = ("count_m2", "count_A", "count0")
CLASS_L = ("last_over1", "last_over2g")
# the sweep hashes 7 objects per wave: in a list of 32, the malformed values sit
# at the even positions 0..28 — first (0, 14, 28), in the middle (10, 24) and
# last (6, 20) in a group of 7 — each between well-formed neighbours (a9's 16:
# the even positions 0..14, first, in the middle (10) and last in a group)
OBJECTS_PER_WAVE = 7


def malformed_kinds(A):
    """The damaged forms a schema of A attributes can hold."""
    kinds = list(REFUSED) + list(CLASS_C) + list(CLASS_L)
    if A < 3:  # no middle attribute; A - 2 is 0 (count0) or negative
        kinds.remove("mid_overrun")
        kinds.remove("count_m2")
    if A < 2:  # no attribute at all: nothing to run past the value, count 0 is right
        kinds.remove("count0")
        kinds.remove("last_over1")
        kinds.remove("last_over2g")
    return kinds


def kind_list(name):
    """The kind of each of the schema's values, in order."""
    types, n, _ = SCHEMAS[name]
    bad = list(A9_MALFORMED) if name == "a9" else malformed_kinds(len(types))
    out, b, g = [], 0, 0
    for i in range(n):
        spaced = i % 2 == 0 if n != 24 else i % 3 != 2  # 24 wide values hold 15 damaged ones: two in three
        if spaced and b < len(bad):
            out.append(bad[b])
            b += 1
        else:
            out.append(WELL_FORMED[g % len(WELL_FORMED)])
            g += 1
    assert b == len(bad) and g >= len(WELL_FORMED), (name, b, g)
    assert n == 24 or all(k in WELL_FORMED for k in out[1::2])  # well-formed neighbours
    return out


def expected_class_counts(name):
    """{"a": .., "b": .., "c": .., "d": ..} as the kinds above intend them."""
    kinds = kind_list(name)
    return {"a": sum(k in WELL_FORMED for k in kinds), "b": sum(k in REFUSED for k in kinds),
            "c": sum(k in CLASS_C for k in kinds), "d": sum(k in CLASS_L for k in kinds)}


def pack_value(attrs, version, count=None, lengths=None):
    """The stored layout: u64 version, u16 count, then a u32 length and the
    bytes of each attribute, all big-endian.  count and lengths override what
    is written into the fields."""
    count = len(attrs) if count is None else count
    lengths = [len(a) for a in attrs] if lengths is None else lengths
    return struct.pack(">QH", version, count) + b"".join(struct.pack(">I", n) + a for n, a in zip(lengths, attrs))


def schema_objects(name):
    """[(kind, key, attrs, version)] before any damage."""
    types, n, longest = SCHEMAS[name]
    A = len(types)
    sidx = sorted(SCHEMAS).index(name)
    r = hgen.rnd(40 + sidx, n * A).reshape(n, A)
    raw = hgen.string_blob(n * A * (longest + 8), stream=60 + sidx)
    pos, out = 0, []
    for i, kind in enumerate(kind_list(name)):
        parts = []
        for j, t in enumerate(types):
            if t == STRING:
                L = int(r[i, j] % np.uint64(longest + 1))
            else:
                L = 0 if int(r[i, j] % np.uint64(8)) == 0 else 8
            if kind == "ok_empty":
                L = 0
            if kind in CLASS_L and j == A - 1 and L == 0:
                L = 8  # something to run past the end with
            parts.append(raw[pos:pos + L].tobytes())
            pos += L
        version = {"ok_v0": 0, "ok_vmax": M64}.get(kind, 1000 + 17 * i)
        out.append((kind, parts[0], parts[1:], version))
    return out


def damage(kind, attrs, version, index):
    """The value's bytes for `kind`."""
    A1 = len(attrs)
    good = pack_value(attrs, version)
    mid = (A1 - 1) // 2  # a middle attribute (never the last one where there are three or more)
    mid_at = 10 + sum(4 + len(a) for a in attrs[:mid])
    if kind in ("ok", "ok_empty", "ok_v0", "ok_vmax"):
        return good
    if kind == "ok_trailing":
        return good + b"\xee" * (1 + index % 5)
    if kind.startswith("len"):
        return (good + bytes(10))[:int(kind[3:])]
    if kind.startswith("cut"):
        k = int(kind[3:])
        if A1 == 0:  # no prefix of its own: one attribute announced, k bytes of its prefix present
            return pack_value([], version, count=1) + bytes(k)
        return good[:mid_at + k]
    if kind == "mid_overrun":
        lengths = [len(a) for a in attrs]
        lengths[mid] = 0xffffffff
        return pack_value(attrs, version, lengths=lengths)
    if kind == "count65535":
        return pack_value(attrs, version, count=65535)
    if kind == "count_m2":
        return pack_value(attrs, version, count=A1 - 1)
    if kind == "count_A":
        return pack_value(attrs, version, count=A1 + 1) + bytes(4)  # one more prefix: an empty attribute
    if kind == "count0":
        return pack_value(attrs, version, count=0)
    lengths = [len(a) for a in attrs]
    lengths[-1] += {"last_over1": 1, "last_over2g": 1 << 31}[kind]
    return pack_value(attrs, version, lengths=lengths)


def schema_values(name):
    """[(kind, key bytes, value bytes)]: the schema's values as stored."""
    return [(kind, key, damage(kind, attrs, version, i))
            for i, (kind, key, attrs, version) in enumerate(schema_objects(name))]


# the window of the wave-staged sweep holds 9.5 KiB: a value that cannot lie in it
LONG_STRING_BYTES = 12001


def long_values():
    """The a2 schema with its string replaced by one of LONG_STRING_BYTES:
    well-formed, and with the last (only) attribute one byte past the value."""
    s = hgen.string_blob(LONG_STRING_BYTES, stream=90).tobytes()
    return [(kind, b"long-key-%d" % i, damage(kind, [s], 77 + i, i)) for i, kind in enumerate(("ok", "last_over1"))]


# ---- index keys -----------------------------------------------------------------------------

INDEX_TYPES = (INT64, FLOAT, TIMESTAMPS[0])


def index_inputs():
    """The hash fixture's eight-byte patterns, then the empty value."""
    patterns, _ = hgen.fixture_patterns()
    return [int(p).to_bytes(8, "little") for p in patterns] + [b""]


# ---- partition ---------------------------------------------------------------------------------

PARTITION_PAIRS = [(1, 1), (1, 3), (1, 7), (1, 64), (1, 256), (2, 49), (2, 50), (2, 256), (3, 8), (3, 27), (3, 64),
                   (3, 125), (3, 216), (3, 1000), (4, 81), (5, 32), (5, 243), (16, 64)]


def boxes_sha256(lower, upper):
    lower = np.ascontiguousarray(lower, "<u8")
    upper = np.ascontiguousarray(upper, "<u8")
    return hashlib.sha256(lower.tobytes() + upper.tobytes()).hexdigest()


LONGEST_LISTED = 32


def lower_bounds_record(lows):
    """A dimension's lower bounds in hex; a list longer than LONGEST_LISTED as
    its length, first three, last and SHA-256 (the boxes' digest holds the rest)."""
    text = ["%016x" % x for x in lows]
    if len(text) <= LONGEST_LISTED:
        return text
    return {"intervals": len(text), "first": text[:3], "last": text[-1],
            "sha256": hashlib.sha256("".join(text).encode()).hexdigest()}


def dimension_lowers(lower):
    """Per dimension, the sorted distinct lower bounds."""
    return [sorted(set(int(x) for x in lower[:, a])) for a in range(lower.shape[1])]


# ---- the fixture -------------------------------------------------------------------------------------

def classify(A, vlen, success, count, slices):
    """a / b / c / d from the reference's own output alone."""
    if not success:
        return "b"
    if count != A - 1:
        return "c"
    if slices and slices[-1][0] + slices[-1][1] > vlen:
        return "d"
    return "a"


# a value's record in the fixture is a list in this order: slices is the flat
# (offset, length, offset, length ...) list, hashes the key's hash and then each
# in-bounds slice's, 16 hex digits each
VALUE_COLUMNS = ("kind", "sha256", "bytes", "success", "version", "count", "slices", "hashes", "class")


def value_dict(rec):
    return dict(zip(VALUE_COLUMNS, rec))


def value_record(oracle, types, kind, key, value):
    A = len(types)
    buf = np.frombuffer(value + bytes(1), np.uint8)
    success, version, count, slices = oracle.ref_decode_value(buf, 0, len(value))
    assert count == len(slices)
    h, err = oracle.ref_hash(types[0], key)
    assert err == 0
    hashes = ["%016x" % h]
    if success:  # the in-bounds slices that have a type, in order
        for j, (o, n) in enumerate(slices[:A - 1]):
            if o + n <= len(value):
                h, err = oracle.ref_hash(types[j + 1], value[o:o + n])
                assert err == 0, (kind, j, n)
                hashes.append("%016x" % h)
    # a refused value's partial slice list is of no use to anyone: its count stays
    rec = {"kind": kind, "sha256": hashlib.sha256(value).hexdigest(), "bytes": len(value), "success": int(success),
           "version": "%016x" % version, "count": count, "slices": [x for s in slices for x in s] if success else [],
           "hashes": "".join(hashes), "class": classify(A, len(value), success, count, slices)}
    return [rec[c] for c in VALUE_COLUMNS]


def build_fixture(oracle) -> dict:
    """The fixture as a dict, from oracle.ref_store_lib() and oracle.ref_hash_lib() (which must be built)."""
    assert oracle.ref_store_lib() is not None and oracle.ref_hash_lib() is not None, \
        "oracle/_ref/libref_store.so / libref_hash.so are not built (make -C oracle ref)"
    stored = {}
    for name in sorted(SCHEMAS):
        types = SCHEMAS[name][0]
        for (kind, _, attrs, version), (_, _, value) in zip(schema_objects(name), schema_values(name)):
            if kind in WELL_FORMED[:4]:  # the input's own packing against the reference's encode_value
                assert oracle.ref_encode_value(attrs, version) == value, (name, kind)
        recs = [value_record(oracle, types, kind, key, value) for kind, key, value in schema_values(name)]
        counts = {c: sum(value_dict(r)["class"] == c for r in recs) for c in "abcd"}
        stored[name] = {"types": list(types), "class_counts": counts, "values": recs}
    long_recs = [value_record(oracle, SCHEMAS["a2"][0], kind, key, value) for kind, key, value in long_values()]
    keys = {}
    for t in INDEX_TYPES:
        enc, sizes = [], []
        for v in index_inputs():
            k, err = oracle.ref_index_encode(t, v)
            assert err == 0
            enc.append(k.hex())
            sizes.append(oracle.ref_index_encoded_size(t, v))
            assert sizes[-1] == len(k)
        keys[str(t)] = {"encoded_size": sorted(set(sizes)), "keys": "".join(enc)}
    parts = []
    for A, S in PARTITION_PAIRS:
        lower, upper = oracle.ref_partition(A, S)
        lists, dims = [], []
        for lows in dimension_lowers(lower):
            text = lower_bounds_record(lows)
            if text not in lists:
                lists.append(text)
            dims.append(lists.index(text))
        parts.append({"num_attrs": A, "num_servers": S, "regions": len(lower), "dimensions": dims,
                      "lower_bounds": lists, "boxes_sha256": boxes_sha256(lower, upper)})
    return {"source": "encode_value / decode_value of the reference's daemon/datalayer_encodings.cc, "
                      "index_encoding_{int64,float,timestamp}::encode / encoded_size of daemon/index_*.cc and "
                      "partition() of admin/partition.cc, compiled unmodified (oracle/Makefile: "
                      "_ref/libref_store.so), with hash() of _ref/libref_hash.so; inputs from "
                      "tests/golden/make_reference_store_values.py",
            "value_columns": list(VALUE_COLUMNS), "stored": stored, "long": long_recs, "index_keys": keys,
            "partition": parts}


def dumps(fixture: dict) -> str:
    return json.dumps(fixture, indent=None, separators=(",", ":"), sort_keys=True) + "\n"


def main(out=FIXTURE):
    sys.path.insert(0, ROOT)
    from oracle import oracle
    text = dumps(build_fixture(oracle))
    with open(out, "w") as f:
        f.write(text)
    print("wrote", out, len(text), "bytes")


if __name__ == "__main__":
    main(*sys.argv[1:])
