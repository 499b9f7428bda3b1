"""Pins the oracle, the CPU path and the kernels to the reference's compiled hash().

Every other parity test ends at oracle/hdx_oracle.c, a restatement written
from the same reading of the reference as the product.  These end at the
reference's own code instead: common/hash.cc, common/datatype_{string,int64,
float,timestamp}.cc, common/ordered_encoding.cc and cityhash/city.cc compiled
unmodified into oracle/_ref/libref_hash.so (oracle/Makefile, `make ref`).

  1. where that library is built: the oracle (hash_value / hash_batch) and the
     product's per-object C-ABI (hdx_hash_value / _key / _object, hdx_cpu.cpp)
     against it, bit for bit, on
       strings   every length 0..1100 at source alignments 0..15, and 4096,
                 65537 and 1 MiB at every alignment;
       numerics  for INT64, FLOAT and the six timestamp types: the empty value,
                 the specials of test_float_and_int_specials, both ends of
                 every binade, NaN payloads, subnormals, 50 k random patterns;
                 for timestamps also 0, +-1, 2^53 +- 1, 2^63 - 1, 2^63, every
                 digit boundary of the radix 60.60.24.7.4.12 (x 10^6, +- 1) and
                 the timestamps whose double quotient t / 1000000. differs
                 from integer division (more than 1000, counted);
       objects   cfg2, cfg3b and `mixed`, 300 each, through the reference's
                 hash(schema, key, value, hs).  The glue's lookup() knows the
                 nine hashable types only, so `mixed` goes to the reference
                 without its three container / document attributes; those
                 coordinates (0: not hashable) stay restated.
     Mis-sized numerics and unknown types make the reference assert: the glue
     refuses them, and the error paths stay with test_oracle_golden.py /
     test_cpu_per_object.py.
  2. everywhere: tests/golden/reference_hash_values.json, recorded from that
     library by tests/golden/make_reference_hash_values.py — 525 strings and
     268 eight-byte patterns (+ the empty value) under the eight numeric types
     — against the oracle, the product's per-object path and the C++ drop-in
     (tests/cpp/dropin_test values); where the library is built, the fixture
     regenerated in memory equals the committed file.
  3. on a GPU: the kernels against the fixture alone (no oracle, no _ref).
     A packed batch for a type list gives object i, attribute j the case
     (i + 7 j) mod count of its type's fixture list, n = the longest list (525
     with a string, 269 without), so every attribute column sees every case of
     its type — (i A + j) mod count, per column, skips cases whenever A and
     count share a factor (A = 5, 525 strings).  The forms, each asserted with
     hashing.kernel_for as test_device_edges.py does:
       packed  12 (strings, A = 1), 21 (key + 4 int64), 46 (string, int64,
               float and the six timestamps), 212 (config 3b's schema: NUM2
               selects), 44 at A = 129 (strings / int64 / float cycling: the
               policy's form; all nine types cycling: forced through the debug
               library, since the policy gives timestamps 46 — that row runs
               too), 300 (A = 257, all nine cycling);
       stored  the same objects in the key-column layout: the NUM2 sweep
               (config 3b's schema), the round-5 form (the schema of 46), the
               wide sweep (A = 129, all nine cycling).
     Integer work: equality, no tolerance.
"""
import ctypes
import functools
import hashlib
import importlib.util
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import hyperdex_amd as hdx
from hyperdex_amd import _lib, synth
from hyperdex_amd import datatypes as dt

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _load_generator():
    spec = importlib.util.spec_from_file_location("make_reference_hash_values",
                                                  os.path.join(GOLD, "make_reference_hash_values.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


gen = _load_generator()
STRING, INT64, FLOAT = dt.HYPERDATATYPE_STRING, dt.HYPERDATATYPE_INT64, dt.HYPERDATATYPE_FLOAT
assert (gen.STRING, gen.INT64, gen.FLOAT, gen.TIMESTAMPS) == (STRING, INT64, FLOAT, dt.TIMESTAMPS)
NUMERIC_TYPES = gen.NUMERIC_TYPES
NINE = (STRING,) + NUMERIC_TYPES


def _ref_or_skip(oracle):
    if oracle.ref_hash_lib() is None:
        pytest.skip("oracle/_ref not built (needs /root/reference at build time)")


def aligned_bytes(nbytes):
    """A zeroed uint8 array of nbytes whose address is a multiple of 16."""
    raw = np.zeros(nbytes + 16, np.uint8)
    skew = (-raw.ctypes.data) % 16
    view = raw[skew:skew + nbytes]
    assert view.ctypes.data % 16 == 0
    return view


# ---- the product's per-object C-ABI over values in place ---------------------------------

def product_values(t, blob, off, lens):
    """hdx_hash_value on blob[off[i]:off[i] + lens[i]] where it lies (the
    value's own address and alignment), one call each."""
    L, base, out = hdx.lib(), blob.ctypes.data, ctypes.c_uint64(0)
    got = np.zeros(len(off), np.uint64)
    for i, (o, n) in enumerate(zip(off.tolist(), lens.tolist())):
        _lib.check(L.hdx_hash_value(t, base + o, n, ctypes.byref(out)))
        got[i] = out.value
    return got


def product_keys(t, blob, off, lens):
    """hdx_hash_key under a schema whose key has type t."""
    L, base, out = hdx.lib(), blob.ctypes.data, ctypes.c_uint64(0)
    types = np.array([t, INT64], np.uint32)
    got = np.zeros(len(off), np.uint64)
    for i, (o, n) in enumerate(zip(off.tolist(), lens.tolist())):
        _lib.check(L.hdx_hash_key(types.ctypes.data, 2, base + o, n, ctypes.byref(out)))
        got[i] = out.value
    return got


def product_as_attributes(t, blob, off, lens, chunk=32768):
    """hdx_hash_object with the values, in place, as attributes 1.. of one wide
    object per chunk (the key: the chunk's first value once more)."""
    L, base = hdx.lib(), blob.ctypes.data
    off = np.asarray(off, np.uint64)
    lens = np.asarray(lens, np.uint64)
    got = np.zeros(len(off), np.uint64)
    for first in range(0, len(off), chunk):
        o, n = off[first:first + chunk], lens[first:first + chunk]
        types = np.full(len(o) + 1, t, np.uint32)
        ptrs = np.ascontiguousarray(o + np.uint64(base))
        sizes = np.ascontiguousarray(n)
        hs = np.zeros(len(o) + 1, np.uint64)
        _lib.check(L.hdx_hash_object(types.ctypes.data, len(types), base + int(o[0]), int(n[0]), ptrs.ctypes.data,
                                     sizes.ctypes.data, hs.ctypes.data))
        assert hs[0] == hs[1]
        got[first:first + chunk] = hs[1:]
    return got


def oracle_values(oracle, t, blob, off, lens):
    """oracle.hash_batch over one-attribute objects that start at off."""
    got, err = oracle.hash_batch([t], blob, off, lens)
    assert err == 0
    return got[:, 0]


def first_difference(got, want):
    bad = np.nonzero(np.asarray(got, np.uint64) != np.asarray(want, np.uint64))[0]
    return None if bad.size == 0 else (int(bad[0]), "%016x" % int(got[bad[0]]), "%016x" % int(want[bad[0]]), bad.size)


# ---- 1. against the compiled reference ----------------------------------------------------

def test_strings_every_length_and_alignment_vs_reference(oracle):
    _ref_or_skip(oracle)
    blob = aligned_bytes(16 + 16 * 64 + 1100)
    blob[:] = gen.string_blob(len(blob), stream=11)
    n, a = np.meshgrid(np.arange(1101, dtype=np.uint64), np.arange(16, dtype=np.uint64), indexing="ij")
    off = (a + np.uint64(16) * (n % np.uint64(64))).reshape(-1)
    lens = n.reshape(-1).astype(np.uint32)
    assert ((off + blob.ctypes.data) % 16 == a.reshape(-1)).all() and len(off) == 1101 * 16
    want, err = oracle.ref_hash_values(STRING, blob, off, lens)
    assert err == 0
    assert first_difference(oracle_values(oracle, STRING, blob, off, lens), want) is None
    assert first_difference(product_values(STRING, blob, off, lens), want) is None
    assert first_difference(product_as_attributes(STRING, blob, off, lens), want) is None
    assert first_difference(product_keys(STRING, blob, off[::7], lens[::7]), want[::7]) is None
    for i in (0, 1, 17, 16 * 600 + 5):  # the one-value forms agree with the batch form
        v = blob[int(off[i]):int(off[i]) + int(lens[i])].tobytes()
        assert oracle.ref_hash(STRING, v) == (int(want[i]), 0)
        assert oracle.hash_value(STRING, v) == (int(want[i]), 0)


def test_long_strings_at_every_alignment_vs_reference(oracle):
    _ref_or_skip(oracle)
    blob = aligned_bytes((1 << 20) + 16)
    blob[:] = gen.string_blob(len(blob), stream=12)
    off = np.tile(np.arange(16, dtype=np.uint64), 3)
    lens = np.repeat(np.array([4096, 65537, 1 << 20], np.uint32), 16)
    want, err = oracle.ref_hash_values(STRING, blob, off, lens)
    assert err == 0 and len(set(want.tolist())) == 48
    assert first_difference(oracle_values(oracle, STRING, blob, off, lens), want) is None
    assert first_difference(product_values(STRING, blob, off, lens), want) is None
    assert first_difference(product_as_attributes(STRING, blob, off, lens), want) is None


def test_rounding_edge_timestamps_exist():
    """More than 1000 timestamps whose double quotient differs from integer
    division, below and above 2^63, and at least 64 of them in the fixture's
    list: the edge an integer divide or an inexact double divide gets wrong
    cannot silently vanish from either list."""
    edges = gen.rounding_edge_timestamps()
    assert len(edges) >= 1000 and len(set(edges.tolist())) == len(edges)
    assert (gen.double_quotient(edges) != gen.integer_quotient(edges)).all()
    assert (edges < np.uint64(1 << 63)).sum() >= 500 and (edges >= np.uint64(1 << 63)).sum() >= 100
    patterns, groups = gen.fixture_patterns()
    first, count = groups["rounding_edges"]
    kept = patterns[first:first + count]
    assert count >= 64 and (gen.double_quotient(kept) != gen.integer_quotient(kept)).all()
    assert (kept < np.uint64(1 << 63)).any() and (kept >= np.uint64(1 << 63)).any()
    # the plain cases stay plain: on the radix boundaries the two quotients agree
    rb = gen.radix_boundaries()
    assert (gen.double_quotient(rb) == gen.integer_quotient(rb)).all()


@pytest.mark.parametrize("t", NUMERIC_TYPES)
def test_numeric_types_vs_reference(oracle, t):
    _ref_or_skip(oracle)
    patterns = gen.full_numeric_patterns(t)
    assert len(patterns) >= 50000 + 8192 + 20
    if t in dt.TIMESTAMPS:
        assert int((gen.double_quotient(patterns) != gen.integer_quotient(patterns)).sum()) >= 1000
    blob = aligned_bytes(8 * len(patterns) + 3)
    off = np.arange(len(patterns), dtype=np.uint64) * np.uint64(8)
    lens = np.full(len(patterns), 8, np.uint32)
    for shift in (0, 3):  # values at 8-byte-aligned and at odd addresses
        blob[shift:shift + 8 * len(patterns)] = gen.pattern_bytes(patterns)
        want, err = oracle.ref_hash_values(t, blob, off + np.uint64(shift), lens)
        assert err == 0
        assert first_difference(oracle_values(oracle, t, blob, off + np.uint64(shift), lens), want) is None
        assert first_difference(product_as_attributes(t, blob, off + np.uint64(shift), lens), want) is None
    # one call per value: every edge list (they come first, and for timestamps last too), a 13th of the random ones
    head = len(patterns) - 50000 if t not in dt.TIMESTAMPS else len(gen.full_numeric_patterns(INT64)) - 50000
    pick = np.concatenate([np.arange(head), np.arange(head, head + 50000, 13), np.arange(head + 50000, len(patterns))])
    assert first_difference(product_values(t, blob, off[pick] + np.uint64(3), lens[pick]), want[pick]) is None
    assert first_difference(product_keys(t, blob, off[pick[::5]] + np.uint64(3), lens[pick[::5]]), want[pick[::5]]) is None
    empty, err = oracle.ref_hash(t, b"")
    assert err == 0
    assert oracle.hash_value(t, b"") == (empty, 0)
    assert hdx.hash(t, b"") == empty and hdx.hash_key([t], b"") == empty
    assert hdx.hash_object([STRING, t], b"k", [b""])[1] == empty


def hashable_columns(types, blob, base, lens):
    """The packed batch without its non-hashable attributes: (kept column
    indices, types, blob, base, lens)."""
    A, n = len(types), len(base)
    keep = [j for j in range(A) if int(types[j]) in NINE]
    L = lens.reshape(n, A).astype(np.int64)
    start = base.astype(np.int64)[:, None] + np.concatenate([np.zeros((n, 1), np.int64), np.cumsum(L, axis=1)[:, :-1]],
                                                            axis=1)
    parts = [blob[start[i, j]:start[i, j] + L[i, j]] for i in range(n) for j in keep]
    new_lens = L[:, keep].astype(np.uint32)
    new_base, _ = synth.object_bases(new_lens.reshape(-1), len(keep))
    new_blob = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    return keep, np.asarray(types, np.uint32)[keep], new_blob, new_base, new_lens.reshape(-1)


@pytest.mark.parametrize("cfg", ["cfg2", "cfg3b", "mixed"])
def test_objects_vs_reference(oracle, cfg):
    """hash(schema, key, value, hs) of the reference over 300 synthetic objects
    against the oracle's batch and the product's hdx_hash_object / _key."""
    _ref_or_skip(oracle)
    n = 300
    types, blob, base, lens = synth.make_batch_host(cfg, n, seed=2024)
    A = len(types)
    keep, rtypes, rblob, rbase, rlens = hashable_columns(types, blob, base, lens)
    assert (len(keep) == A) == (cfg != "mixed") and len(keep) >= A - 3
    if cfg == "mixed":  # the glue refuses the full schema and calls nothing
        assert oracle.ref_hash_objects(types, blob, base, lens)[1] == 1
    want, err = oracle.ref_hash_objects(rtypes, rblob, rbase, rlens)
    assert err == 0
    got, err = oracle.hash_batch(types, blob, base, lens)
    assert err == 0
    assert np.array_equal(got[:, keep], want)
    drop = [j for j in range(A) if j not in keep]
    assert not got[:, drop].any()
    L = lens.reshape(n, A)
    for i in range(n):
        offs = int(base[i]) + np.concatenate([[0], np.cumsum(L[i, :-1], dtype=np.int64)])
        parts = [blob[o:o + k].tobytes() for o, k in zip(offs, L[i])]
        hs = hdx.hash_object(types, parts[0], parts[1:])
        assert [hs[j] for j in keep] == want[i].tolist() and not any(hs[j] for j in drop), (cfg, i)
        assert hdx.hash_key(types, parts[0]) == int(want[i, 0])


def test_glue_refuses_what_the_reference_asserts_on(oracle):
    """lookup() == NULL and mis-sized numerics: an error code, no call."""
    _ref_or_skip(oracle)
    for t in (dt.HYPERDATATYPE_GENERIC, dt.HYPERDATATYPE_MAP_STRING_KEYONLY, dt.HYPERDATATYPE_LIST_STRING,
              dt.HYPERDATATYPE_DOCUMENT, dt.HYPERDATATYPE_TIMESTAMP_GENERIC, dt.HYPERDATATYPE_MACAROON_SECRET, 0):
        assert oracle.ref_hash(t, b"12345678") == (0, 1)
    for t in NUMERIC_TYPES:
        assert oracle.ref_hash(t, b"1234") == (0, 2) and oracle.ref_hash(t, b"123456789") == (0, 2)
    out, err = oracle.ref_hash_values(INT64, np.zeros(16, np.uint8), [0, 8], [8, 7])
    assert err == 2 and not out.any()
    assert oracle.ref_hash_objects([STRING, INT64], np.zeros(16, np.uint8), [0, 8], [0, 8, 3, 5])[1] == 2


# ---- 2. the fixture -----------------------------------------------------------------------------

@functools.lru_cache(maxsize=1)
def fixture_text():
    with open(gen.FIXTURE) as f:
        return f.read()


@functools.lru_cache(maxsize=1)
def fixture():
    """The committed fixture as per-type case lists: cases[t] = [(value bytes,
    the reference's hash)], the empty value last for the numeric types."""
    fx = json.loads(fixture_text())
    blob = gen.string_blob(fx["strings"]["blob_bytes"])
    assert hashlib.sha256(blob.tobytes()).hexdigest() == fx["strings"]["blob_sha256"], \
        "string_blob() no longer generates the bytes the fixture was recorded from"
    cases = {STRING: [(blob[o:o + n].tobytes(), int(h, 16)) for o, n, h in fx["strings"]["cases"]]}
    patterns = [int(p, 16) for p in fx["numerics"]["patterns"]]
    for t in NUMERIC_TYPES:
        rec = fx["numerics"]["hashes"][str(t)]
        assert len(rec["values"]) == len(patterns)
        cases[t] = [(p.to_bytes(8, "little"), int(h, 16)) for p, h in zip(patterns, rec["values"])]
        cases[t].append((b"", int(rec["empty"], 16)))
    return fx, cases


def test_fixture_holds_its_edge_lists():
    """Under 96 KiB; the inputs are the generator's (so the edge lists are all
    there: only random cases may ever be trimmed)."""
    fx, cases = fixture()
    assert len(fixture_text().encode()) < 96 * 1024
    assert [(o, n) for o, n, _ in fx["strings"]["cases"]] == gen.fixture_string_cases()
    assert [n for _, n, _ in fx["strings"]["cases"]] == list(range(521)) + [1023, 1024, 1025, 4096]
    patterns, groups = gen.fixture_patterns()
    assert fx["numerics"]["patterns"] == ["%016x" % int(p) for p in patterns] and fx["numerics"]["groups"] == groups
    have = set(int(p) for p in patterns)
    for must in (gen.SPECIALS, gen.TIMESTAMP_SPECIALS, gen.radix_boundaries().tolist()):
        assert set(int(x) for x in must) <= have
    assert groups["rounding_edges"][1] >= 64 and 200 <= len(patterns) <= 300
    assert sorted(fx["numerics"]["hashes"]) == sorted(str(t) for t in NUMERIC_TYPES)
    # not a degenerate recording: the types disagree with each other on the list
    columns = {t: tuple(h for _, h in cases[t]) for t in NUMERIC_TYPES}
    assert len(set(columns.values())) == len(NUMERIC_TYPES)


def test_oracle_matches_fixture(oracle):
    _, cases = fixture()
    for t, rows in cases.items():
        for v, want in rows:
            assert oracle.hash_value(t, v) == (want, 0), (t, v[:16].hex(), len(v))


def test_product_per_object_matches_fixture():
    """hdx_hash_value / hdx_hash_key on every case; hdx_hash_object on rows of
    the nine-type schema that cycle through every case."""
    _, cases = fixture()
    for t, rows in cases.items():
        for v, want in rows:
            assert hdx.hash(t, v) == want, (t, v[:16].hex(), len(v))
            assert hdx.hash_key([t, STRING], v) == want
    n = max(len(rows) for rows in cases.values())
    for i in range(n):
        row = [cases[t][(i + 7 * j) % len(cases[t])] for j, t in enumerate(NINE)]
        assert hdx.hash_object(NINE, row[0][0], [v for v, _ in row[1:]]) == [h for _, h in row], i


def test_cpp_dropin_matches_fixture(tmp_path):
    """include/hyperdex_amd/hash.h's hash(hyperdatatype, e::slice), through
    tests/cpp/dropin_test, on every case of the fixture."""
    import test_dropin_cpp as dropin
    dropin.build(dropin.have_reference_headers())
    _, cases = fixture()
    records = [(t, v, want) for t, rows in cases.items() for v, want in rows]
    path = tmp_path / "values.bin"
    path.write_bytes(b"".join(struct.pack("<II", t, len(v)) + v for t, v, _ in records))
    r = subprocess.run([dropin.EXE, "values", str(path)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert [int(x, 16) for x in r.stdout.split()] == [want for _, _, want in records]


def test_fixture_regenerates_from_the_reference(oracle):
    _ref_or_skip(oracle)
    assert gen.dumps(gen.build_fixture(oracle)) == fixture_text()


# ---- 3. the kernels against the fixture ----------------------------------------------------------

CFG3B_TYPES = tuple(int(r.type) for r in synth.CONFIGS["cfg3b"])
SCHEMAS = {
    "strings": (STRING,),
    "key+4int64": (STRING,) + (INT64,) * 4,
    "all-nine": NINE,
    "cfg3b": CFG3B_TYPES,
    "a129-num2": tuple((STRING, STRING, INT64, STRING, FLOAT)[j % 5] for j in range(129)),
    "a129-nine": tuple(NINE[j % 9] for j in range(129)),
    "a257-nine": tuple(NINE[j % 9] for j in range(257)),
}
# (schema, debug variant or None, the form kernel_for names)
BATCH_ROWS = [("strings", None, 12), ("key+4int64", None, 21), ("all-nine", None, 46), ("cfg3b", None, 212),
              ("a129-num2", None, 44), ("a129-nine", 44, 44), ("a129-nine", None, 46), ("a257-nine", None, 300)]
# (schema, the batch policy's form for it: 212 -> the sweep's NUM2 form, 46 -> its round-5 form; more than 128
# attributes -> the wide sweep whatever the types)
SWEEP_ROWS = [("cfg3b", 212), ("all-nine", 46), ("a129-nine", 46)]


class FixtureBatch:
    pass


@functools.lru_cache(maxsize=None)
def fixture_batch(name):
    """The packed batch of SCHEMAS[name] whose object i, attribute j holds case
    (i + 7 j) mod count of its type's fixture list, n = the longest list in the
    schema; .want (n, A) comes from the fixture alone."""
    _, cases = fixture()
    types = SCHEMAS[name]
    A = len(types)
    n = max(len(cases[t]) for t in set(types))
    pick = np.array([[(i + 7 * j) % len(cases[types[j]]) for j in range(A)] for i in range(n)])
    for j, t in enumerate(types):  # coverage: every column holds every case of its type
        assert set(pick[:, j].tolist()) == set(range(len(cases[t])))
    b = FixtureBatch()
    b.name, b.n, b.A, b.types = name, n, A, np.array(types, np.uint32)
    b.lens = np.array([len(cases[types[j]][pick[i, j]][0]) for i in range(n) for j in range(A)], np.uint32)
    b.blob = np.frombuffer(b"".join(cases[types[j]][pick[i, j]][0] for i in range(n) for j in range(A)) + bytes(16),
                           np.uint8)
    b.base, total = synth.object_bases(b.lens, A)
    assert total + 16 == len(b.blob)
    b.want = np.array([[cases[types[j]][pick[i, j]][1] for j in range(A)] for i in range(n)], np.uint64)
    return b


@functools.lru_cache(maxsize=None)
def fixture_stored(name):
    """fixture_batch(name) as stored objects in the key-column layout (the
    suite's value encoder, synth.encode_store_host)."""
    b = fixture_batch(name)
    return b, [np.array(x) for x in synth.encode_store_host(b.types, b.blob, b.base, b.lens, first_version=3,
                                                            layout="keycol")]


def test_fixture_batches_cover_every_case():
    """On the CPU: the helper's n and coverage (asserted inside), and its
    expected coordinates against the product's per-object path."""
    for name, n in (("strings", 525), ("key+4int64", 525), ("all-nine", 525), ("cfg3b", 525)):
        b = fixture_batch(name)
        assert b.n == n and b.want.shape == (n, b.A)
        L = b.lens.reshape(n, b.A)
        for i in (0, 1, n // 2, n - 1):
            offs = int(b.base[i]) + np.concatenate([[0], np.cumsum(L[i, :-1], dtype=np.int64)])
            parts = [b.blob[o:o + k].tobytes() for o, k in zip(offs, L[i])]
            assert hdx.hash_object(b.types, parts[0], parts[1:]) == b.want[i].tolist()


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available()
    return torch, torch.device("cuda", 0)


def to_dev(torch, dev, a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a.copy()).to(dev)


def row_id(row):
    return "-".join(str(x) for x in row if x is not None)


def check_form(b, variant, form):
    """The policy's form outside the debug library, the forced one inside."""
    assert hdx.hashing.kernel_for(b.types, b.n)[0] == form or variant == form
    if variant is not None:
        with _lib.debug_library(variant):
            assert hdx.hashing.kernel_for(b.types, b.n)[0] == variant


@pytest.mark.gpu
@pytest.mark.parametrize("row", BATCH_ROWS, ids=row_id)
def test_kernels_match_fixture_packed(torch_dev, row):
    torch, dev = torch_dev
    name, variant, form = row
    b = fixture_batch(name)
    check_form(b, variant, form)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    args = [to_dev(torch, dev, x) for x in (b.blob, b.base, b.lens)]
    if variant is None:
        coords = hdx.hash_batch(b.types, *args, status=status)
        torch.cuda.synchronize()
    else:
        with _lib.debug_library(variant):
            coords = hdx.hash_batch(b.types, *args, status=status)
            torch.cuda.synchronize()
    got = coords.cpu().numpy().view(np.uint64)
    assert int(status.item()) == 0
    bad = np.argwhere(got != b.want)
    assert bad.size == 0, "object %d attribute %d (type %d): got %016x, the reference %016x; %d differ" % (
        bad[0][0], bad[0][1], b.types[bad[0][1]], got[tuple(bad[0])], b.want[tuple(bad[0])], len(bad))


@pytest.mark.gpu
@pytest.mark.parametrize("row", SWEEP_ROWS, ids=row_id)
def test_kernels_match_fixture_stored(torch_dev, row):
    torch, dev = torch_dev
    name, form = row
    b, enc = fixture_stored(name)
    check_form(b, None, form)
    assert (b.A > 128) == (name == "a129-nine")
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    versions = torch.zeros(b.n, dtype=torch.int64, device=dev)
    coords = hdx.hash_encoded(b.types, *[to_dev(torch, dev, x) for x in enc], versions=versions, status=status)
    torch.cuda.synchronize()
    got = coords.cpu().numpy().view(np.uint64)
    assert int(status.item()) == 0
    assert np.array_equal(versions.cpu().numpy(), 3 + np.arange(b.n))
    bad = np.argwhere(got != b.want)
    assert bad.size == 0, "object %d attribute %d (type %d): got %016x, the reference %016x; %d differ" % (
        bad[0][0], bad[0][1], b.types[bad[0][1]], got[tuple(bad[0])], b.want[tuple(bad[0])], len(bad))
