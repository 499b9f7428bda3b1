"""Pins the stored-value decoder, the index keys and the partition to the reference's compiled code.

tests/test_reference_hash.py ends the hash chain at the reference's own
hash().  These end the rest of what the sweep, index-key and region tests rest
on at the reference's own daemon/datalayer_encodings.cc (encode_value,
decode_value), daemon/index_{int64,float,timestamp}.cc and admin/partition.cc,
compiled unmodified into oracle/_ref/libref_store.so (oracle/Makefile,
`make ref`).  The region lookups (configuration.cc) stay restated: DESIGN.md
section 3 says why.

The contract for stored values.  The project's decoder (the oracle, the host
path, every sweep kernel) deliberately refuses two sorts of value that the
reference's decode_value accepts, and nothing else:

    class C  the reference says SUCCESS and its attribute count is not A - 1;
    class L  the reference says SUCCESS, the count is A - 1 and the last
             attribute ends past the value (last offset + length > the value's
             length) — the reference would go on to read past the value.

Both are recognised from the reference's own output alone.  The project's
verdict is "bad" iff the reference returns BAD_ENCODING or the value is in
class C or class L; a bad value's answer is the project's documented one
(every coordinate 0, version 0, HDX_E_BADENC in the status word).  Where both
accept, the version and every (offset, length) are equal, and the coordinates
are the reference's hash() of the key and of each slice.  No value outside C
and L may differ, and C and L values are asserted, never skipped.

  1. where that library is built (skipped otherwise): the oracle against
     ref_decode_value + ref_hash under that contract on the fixture's values,
     on 20 000 synthetic values per schema of cfg2, cfg3b and `mixed` (without
     its non-hashable attributes) and on the same values run through
     test_encoded._corrupt; synth.encode_values_host byte for byte against
     encode_value; oracle.index_encode against the reference's encoders on
     every numeric list of make_reference_hash_values.py under all eight
     types, and on lengths 1-7 and 9, which make the reference assert (the
     glue refuses them, the oracle reports its size error); oracle.partition
     against partition() for 1-16 attributes x 1-300 servers.
  2. everywhere: tests/golden/reference_store_values.json, recorded from that
     library by tests/golden/make_reference_store_values.py, against the
     oracle; where the library is built, the fixture regenerated in memory
     equals the committed file.  The number of values per class (a:
     well-formed, b: refused by the reference, c, d = L) is written by the
     generator and asserted here.
  3. on a GPU: the kernels against the fixture alone (no oracle, no _ref): the
     sweep in the columns, keycol and records layouts, the whole list in one
     launch and with every malformed value alone in its launch, under the
     product policy and the debug library's forms; a value the 9.5 KiB window
     cannot hold; the host entry point (hdx_hash_encoded_host) on the same
     values; the index keys; the device value generator.
Integer work: equality, no tolerance.
"""
import functools
import hashlib
import importlib.util
import json
import os

import numpy as np
import pytest

import hyperdex_amd as hdx
from hyperdex_amd import _lib, synth
from hyperdex_amd import datatypes as dt

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(GOLD, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


gen = _load("make_reference_store_values")
hgen = gen.hgen
STRING, INT64, FLOAT = dt.HYPERDATATYPE_STRING, dt.HYPERDATATYPE_INT64, dt.HYPERDATATYPE_FLOAT
assert (gen.STRING, gen.INT64, gen.FLOAT, gen.TIMESTAMPS) == (STRING, INT64, FLOAT, dt.TIMESTAMPS)
NUMERIC_TYPES = gen.NUMERIC_TYPES
SCHEMA_NAMES = sorted(gen.SCHEMAS)
PAD = 64  # zero bytes after the last key / value of every buffer


def _ref_or_skip(oracle):
    if oracle.ref_store_lib() is None or oracle.ref_hash_lib() is None:
        pytest.skip("oracle/_ref not built (needs the reference tree at build time)")


# ---- stored objects as arrays ------------------------------------------------------------------

def store_arrays(objects, layout="keycol"):
    """[(key bytes, value bytes)] -> (keys, key_off, key_len, vals, val_off,
    val_len) in one of synth.make_encoded_device's layouts: "columns" (each key
    in place inside a larger blob, here followed by 5 bytes of something else),
    "keycol" (keys back to back), "records" ([key][value] back to back in one
    store that is both keys and vals)."""
    key_len = np.array([len(k) for k, _ in objects], np.uint32)
    val_len = np.array([len(v) for _, v in objects], np.uint32)

    def starts(sizes):
        out = np.zeros(len(sizes), np.uint64)
        out[1:] = np.cumsum(np.asarray(sizes[:-1], np.uint64))
        return out
    if layout == "records":
        rec_off = starts(key_len.astype(np.uint64) + val_len)
        store = np.frombuffer(b"".join(k + v for k, v in objects) + bytes(PAD), np.uint8)
        return store, rec_off, key_len, store, rec_off + key_len, val_len
    vals = np.frombuffer(b"".join(v for _, v in objects) + bytes(PAD), np.uint8)
    if layout == "keycol":
        keys = np.frombuffer(b"".join(k for k, _ in objects) + bytes(PAD), np.uint8)
        return keys, starts(key_len), key_len, vals, starts(val_len), val_len
    assert layout == "columns"
    keys = np.frombuffer(b"".join(k + b"\xa5" * 5 for k, _ in objects) + bytes(PAD), np.uint8)
    return keys, starts(key_len.astype(np.uint64) + 5), key_len, vals, starts(val_len), val_len


# ---- 1. against the compiled reference ---------------------------------------------------------------

def check_contract(oracle, types, enc):
    """The oracle over the stored objects `enc` against ref_decode_value +
    ref_hash.  Returns the number of values per class."""
    types = [int(t) for t in types]
    A = len(types)
    keys, key_off, key_len, vals, val_off, val_len = [np.asarray(x) for x in enc]
    n = len(val_off)
    coords, versions, bad = oracle.hash_encoded(types, keys, key_off, key_len, vals, val_off, val_len)
    classes = dict.fromkeys("abcd", 0)
    good, offs, lens = [], np.zeros((n, max(A - 1, 1)), np.uint64), np.zeros((n, max(A - 1, 1)), np.uint32)
    for i in range(n):
        o, L = int(val_off[i]), int(val_len[i])
        success, version, count, slices = oracle.ref_decode_value(vals, o, L, max_attrs=A + 1)
        cls = gen.classify(A, L, success, count, slices)
        classes[cls] += 1
        mine = oracle.decode_value(A, vals, o, L)
        assert bool(bad[i]) == (cls != "a") == (not mine[0]), (i, cls, success, count, slices[-1:], L)
        if cls == "a":
            assert (mine[1], mine[2]) == (version, slices) and int(versions[i]) == version, i
            good.append(i)
            for k, (so, sn) in enumerate(slices):
                offs[i, k], lens[i, k] = o + so, sn
        else:  # the project's documented answer
            assert mine == (False, 0, []) and int(versions[i]) == 0 and not coords[i].any(), (i, cls)
    good = np.array(good, np.int64)
    want, err = oracle.ref_hash_values(types[0], keys, key_off[good], key_len[good])
    assert err == 0 and np.array_equal(coords[good, 0], want)
    for k in range(A - 1):
        want, err = oracle.ref_hash_values(types[k + 1], vals, offs[good, k], lens[good, k])
        assert err == 0 and np.array_equal(coords[good, k + 1], want), k
    return classes


@pytest.mark.parametrize("name", SCHEMA_NAMES)
def test_oracle_decodes_fixture_values_as_the_reference(oracle, name):
    _ref_or_skip(oracle)
    types = gen.SCHEMAS[name][0]
    objects = [(key, value) for _, key, value in gen.schema_values(name)]
    for layout in ("keycol", "records"):
        assert check_contract(oracle, types, store_arrays(objects, layout)) == gen.expected_class_counts(name)


def test_oracle_decodes_long_values_as_the_reference(oracle):
    _ref_or_skip(oracle)
    objects = [(key, value) for _, key, value in gen.long_values()]
    assert check_contract(oracle, gen.SCHEMAS["a2"][0], store_arrays(objects)) == {"a": 1, "b": 0, "c": 0, "d": 1}


def synthetic_store(cfg, n, seed):
    """A synth batch of cfg's hashable attributes as stored objects."""
    import test_reference_hash as trh
    types, blob, base, lens = synth.make_batch_host(cfg, n, seed=seed)
    keep, types, blob, base, lens = trh.hashable_columns(types, blob, base, lens)
    assert len(keep) == (11 if cfg == "mixed" else len(synth.CONFIGS[cfg]))
    blob = np.concatenate([blob, np.zeros(PAD, np.uint8)])
    return types, synth.encode_values_host(types, blob, base, lens, first_version=(1 << 40) + 5)


@pytest.mark.parametrize("cfg", ["cfg2", "cfg3b", "mixed"])
def test_oracle_decodes_synthetic_values_as_the_reference(oracle, cfg):
    """20 000 values per schema as encoded, then with test_encoded._corrupt's
    damage: the oracle differs from the reference in classes C and L only."""
    import test_encoded
    _ref_or_skip(oracle)
    n = 20000
    types, enc = synthetic_store(cfg, n, seed=77)
    assert check_contract(oracle, types, enc) == {"a": n, "b": 0, "c": 0, "d": 0}
    damaged, cases = test_encoded._corrupt(enc, np.random.default_rng(11))
    classes = check_contract(oracle, types, damaged)
    assert classes["a"] == n - len(cases) and len(cases) == 40 and sum(classes.values()) == n
    # _corrupt's five sorts, 8 each.  Three the reference refuses itself (a value under 10 bytes, a first length
    # that overruns, a cut prefix).  The count with its low bit flipped grows in all three schemas (4 -> 5,
    # 16 -> 17, 10 -> 11) and no further prefix follows, so the reference refuses it too: class C is the fixture's
    # to cover.  The value cut short by 1-4 bytes is class L, unless its last attribute is empty and the cut
    # takes its prefix.
    assert classes["c"] == 0
    assert 1 <= classes["d"] <= 8 and classes["b"] == 40 - classes["c"] - classes["d"]


@pytest.mark.parametrize("cfg,n", [("cfg2", 300), ("cfg3b", 300), ("mixed", 300), ("wide", 40), ("cfg1", 50)])
def test_host_encoder_matches_the_reference_encode_value(oracle, cfg, n):
    """synth.encode_values_host (what every sweep test is fed with) byte for byte."""
    _ref_or_skip(oracle)
    types, blob, base, lens = synth.make_batch_host(cfg, n, seed=31)
    A = len(types)
    first = (1 << 63) + 12345
    _, _, _, vals, val_off, val_len = synth.encode_values_host(types, blob, base, lens, first_version=first)
    L = lens.reshape(n, A)
    for i in range(n):
        at = int(base[i]) + np.concatenate([[0], np.cumsum(L[i], dtype=np.int64)])
        attrs = [blob[at[j]:at[j + 1]].tobytes() for j in range(1, A)]
        want = oracle.ref_encode_value(attrs, first + i)
        got = vals[int(val_off[i]):int(val_off[i]) + int(val_len[i])].tobytes()
        assert got == want, (cfg, i)
        assert want == gen.pack_value(attrs, first + i)  # the fixture generator's packing too


def test_reference_round_trips_its_own_values(oracle):
    """decode_value(encode_value(x)) on the edges of the header fields."""
    _ref_or_skip(oracle)
    for attrs, version in (([], 0), ([b""], (1 << 64) - 1), ([b"a" * 70000, b"", b"12345678"], 1 << 63)):
        v = oracle.ref_encode_value(attrs, version)
        success, ver, count, slices = oracle.ref_decode_value(np.frombuffer(v + b"\0", np.uint8), 0, len(v))
        assert (success, ver, count) == (True, version, len(attrs))
        assert [v[o:o + n] for o, n in slices] == attrs


@pytest.mark.parametrize("t", NUMERIC_TYPES)
def test_index_keys_vs_reference(oracle, t):
    """index_encoding::lookup(t)->encode on every list of the hash pin, full
    length; the FLOAT key's second half and the timestamp-to-int64 delegation
    come from the reference's own code."""
    _ref_or_skip(oracle)
    patterns = hgen.full_numeric_patterns(t)
    assert len(patterns) >= 50000 + 8192 + 20
    size = 16 if t == FLOAT else 8
    for p in patterns.tolist():
        v = p.to_bytes(8, "little")
        want, err = oracle.ref_index_encode(t, v)
        assert err == 0 and len(want) == size
        assert oracle.index_encode(t, v) == (want, 0), "%016x" % p
    want, err = oracle.ref_index_encode(t, b"")
    assert err == 0 and oracle.index_encode(t, b"") == (want, 0)
    assert oracle.ref_index_encoded_size(t, b"") == oracle.ref_index_encoded_size(t, bytes(8)) == size
    assert hdx.index.index_key_size(t) == size
    if t in dt.TIMESTAMPS:  # keyed as int64, not by the calendar hash
        assert oracle.ref_index_encode(t, bytes(range(8))) == oracle.ref_index_encode(INT64, bytes(range(8)))


def test_index_encoder_on_sizes_the_reference_asserts_on(oracle):
    """Lengths 1-7 and 9: datatype_*::hash asserts validate() under all three
    encoders (FLOAT's `validate && size == 8` only guards the second half), so
    the glue refuses them without a call; the oracle reports its size error and
    a zero key of the encoder's size.  Types without a numeric encoder: refused."""
    _ref_or_skip(oracle)
    for t in NUMERIC_TYPES:
        size = 16 if t == FLOAT else 8
        for n in (1, 2, 3, 4, 5, 6, 7, 9):
            v = bytes(range(1, n + 1))
            assert oracle.ref_index_encode(t, v) == (b"", 2)
            assert oracle.ref_index_encoded_size(t, v) == size  # the size does not look at the value
            assert oracle.index_encode(t, v) == (bytes(size), 2)
    for t in (STRING, dt.HYPERDATATYPE_LIST_STRING, dt.HYPERDATATYPE_DOCUMENT, 0):
        assert oracle.ref_index_encode(t, bytes(8)) == (b"", 1) and oracle.ref_index_encoded_size(t, bytes(8)) == -1
        assert oracle.index_encode(t, bytes(8)) == (b"", 0)


def test_partition_vs_reference(oracle):
    """Every (num_attrs, num_servers) of 1-16 x 1-300, and the fixture's pairs:
    region count, order and both boxes.  The largest (8 attributes, 256-300
    servers: 3^8 regions) stay in; nothing here reaches 4096 x 16 words twice."""
    _ref_or_skip(oracle)
    pairs = [(a, s) for a in range(1, 17) for s in range(1, 301)] + gen.PARTITION_PAIRS
    most = 0
    for a, s in pairs:
        lower, upper = oracle.ref_partition(a, s)
        got = oracle.partition(a, s)
        assert got[0].shape == lower.shape, (a, s, got[0].shape, lower.shape)
        assert np.array_equal(got[0], lower) and np.array_equal(got[1], upper), (a, s)
        most = max(most, len(lower))
    assert most == 3 ** 8
    assert oracle.ref_partition(0, 5) is None and oracle.ref_partition(3, 0) is None


# ---- 2. the fixture ----------------------------------------------------------------------------------

@functools.lru_cache(maxsize=1)
def fixture_text():
    with open(gen.FIXTURE) as f:
        return f.read()


class Stored:
    """A schema's values with what the fixture says of them: .objects [(key,
    value)], .records (dicts of gen.VALUE_COLUMNS), .bad (n,), .versions (n,),
    .coords (n, A): the contract's answer, from the fixture alone."""


def _stored(types, values, records):
    s = Stored()
    s.types, s.A, s.n = np.array(types, np.uint32), len(types), len(values)
    s.objects = [(key, value) for _, key, value in values]
    s.records = [gen.value_dict(r) for r in records]
    s.bad = np.zeros(s.n, bool)
    s.versions = np.zeros(s.n, np.uint64)
    s.coords = np.zeros((s.n, s.A), np.uint64)
    for i, ((kind, _, value), r) in enumerate(zip(values, s.records)):
        assert r["kind"] == kind and r["bytes"] == len(value), (i, kind)
        assert hashlib.sha256(value).hexdigest() == r["sha256"], \
            "value %d (%s): the generator no longer writes the bytes the fixture was recorded from" % (i, kind)
        slices = list(zip(r["slices"][0::2], r["slices"][1::2]))
        assert r["class"] == gen.classify(s.A, len(value), bool(r["success"]), r["count"], slices)
        s.bad[i] = r["class"] != "a"
        if not s.bad[i]:
            assert len(r["hashes"]) == 16 * s.A and len(slices) == s.A - 1
            s.versions[i] = int(r["version"], 16)
            s.coords[i] = [int(r["hashes"][16 * j:16 * j + 16], 16) for j in range(s.A)]
    return s


@functools.lru_cache(maxsize=None)
def stored(name):
    fx = json.loads(fixture_text())
    assert tuple(fx["value_columns"]) == gen.VALUE_COLUMNS
    if name == "long":
        return _stored(gen.SCHEMAS["a2"][0], gen.long_values(), fx["long"])
    assert tuple(fx["stored"][name]["types"]) == gen.SCHEMAS[name][0]
    return _stored(gen.SCHEMAS[name][0], gen.schema_values(name), fx["stored"][name]["values"])


def test_fixture_holds_its_cases():
    """Under 100 KB; every schema holds the classes it is meant to, in the
    numbers the generator wrote, with the malformed values where the sweep's
    groups of 7 make them matter."""
    fx = json.loads(fixture_text())
    assert len(fixture_text().encode()) <= 100 * 1000
    assert sorted(fx["stored"]) == SCHEMA_NAMES
    assert [len(gen.SCHEMAS[k][0]) for k in ("a1", "a2", "a5", "a17", "a129")] == [1, 2, 5, 17, 129]
    assert gen.SCHEMAS["a5"][0] == tuple(r.type for r in synth.CONFIGS["cfg2"])
    assert gen.SCHEMAS["a17"][0] == tuple(r.type for r in synth.CONFIGS["cfg3b"])
    for name in SCHEMA_NAMES:
        s = stored(name)
        counts = {c: sum(r["class"] == c for r in s.records) for c in "abcd"}
        assert counts == fx["stored"][name]["class_counts"] == gen.expected_class_counts(name), name
        kinds = [r["kind"] for r in s.records]
        assert kinds == gen.kind_list(name)
        for r in s.records:  # every kind lands in the class it was written for
            want = ("a" if r["kind"] in gen.WELL_FORMED else "b" if r["kind"] in gen.REFUSED
                    else "c" if r["kind"] in gen.CLASS_C else "d")
            assert r["class"] == want, (name, r["kind"], r["class"])
        assert set(gen.WELL_FORMED) <= set(kinds)
        assert set(kinds) >= set(gen.A9_MALFORMED if name == "a9" else gen.malformed_kinds(s.A))
        if s.A <= 128:  # a ragged tail, and a malformed value first, in the middle and last in a group of 7
            K = gen.OBJECTS_PER_WAVE
            assert s.n % K != 0 and s.n > 2 * K
            where = {i % K for i in np.nonzero(s.bad)[0] if i < s.n - s.n % K}
            assert {0, K // 2, K - 1} <= where
            assert not (s.bad[1:] & s.bad[:-1]).any()
    counts = {name: fx["stored"][name]["class_counts"] for name in SCHEMA_NAMES}
    assert counts["a17"] == counts["a5"] == {"a": 17, "b": 10, "c": 3, "d": 2}
    assert counts["a129"] == {"a": 9, "b": 10, "c": 3, "d": 2}
    assert counts["a2"] == {"a": 19, "b": 9, "c": 2, "d": 2} and counts["a1"] == {"a": 22, "b": 9, "c": 1, "d": 0}
    assert counts["a9"] == {"a": 8, "b": 4, "c": 2, "d": 2}
    long = stored("long")
    assert [r["class"] for r in long.records] == ["a", "d"] and min(r["bytes"] for r in long.records) > 9728
    # the header's edges are among the accepted values
    versions = {int(r["version"], 16) for r in stored("a17").records if r["class"] == "a"}
    assert {0, (1 << 64) - 1} <= versions


@pytest.mark.parametrize("name", SCHEMA_NAMES + ["long"])
def test_oracle_matches_fixture_values(oracle, name):
    """Verdicts, versions, slices and coordinates, in two layouts."""
    s = stored(name)
    for layout in ("columns", "records"):
        enc = store_arrays(s.objects, layout)
        coords, versions, bad = oracle.hash_encoded(s.types, *enc)
        assert np.array_equal(bad, s.bad) and np.array_equal(versions, s.versions)
        assert np.array_equal(coords, s.coords)
    for (_, value), r, bad in zip(s.objects, s.records, s.bad):
        got = oracle.decode_value(s.A, np.frombuffer(value + b"\0", np.uint8), 0, len(value))
        if bad:
            assert got == (False, 0, [])
        else:
            assert got == (True, int(r["version"], 16), list(zip(r["slices"][0::2], r["slices"][1::2])))
        # classes C and L: the slices the reference reports inside the value hash as the reference hashed them
        if r["success"] and bad:
            slices = list(zip(r["slices"][0::2], r["slices"][1::2]))[:s.A - 1]
            inside = [(j, o, n) for j, (o, n) in enumerate(slices) if o + n <= len(value)]
            assert len(r["hashes"]) == 16 * (1 + len(inside))
            for k, (j, o, n) in enumerate(inside):
                assert oracle.hash_value(int(s.types[j + 1]), value[o:o + n]) == \
                    (int(r["hashes"][16 * (k + 1):16 * (k + 2)], 16), 0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCHEMA_NAMES + ["long"])
def test_host_entry_point_matches_fixture_values(name):
    """hdx_hash_encoded_host (stored objects in host memory, through the host
    pipeline and the sweep) on the same values, from the fixture alone."""
    s = stored(name)
    for layout in ("keycol", "records"):
        enc = store_arrays(s.objects, layout)
        coords, versions, st, _ = hdx.hashing.hash_encoded_host_status(s.types, *enc)
        assert st == (_lib.HDX_E_BADENC if s.bad.any() else _lib.HDX_OK)
        assert np.array_equal(versions, s.versions) and np.array_equal(coords, s.coords)
    good = [o for o, b in zip(s.objects, s.bad) if not b]
    coords, versions, st, _ = hdx.hashing.hash_encoded_host_status(s.types, *store_arrays(good))
    assert st == _lib.HDX_OK and np.array_equal(coords, s.coords[~s.bad])
    assert np.array_equal(versions, s.versions[~s.bad])


@functools.lru_cache(maxsize=1)
def index_cases():
    """{type: [(value bytes, key bytes)]} from the fixture: INT64, FLOAT, and
    the one recorded timestamp type's keys under each of the six."""
    fx = json.loads(fixture_text())["index_keys"]
    inputs = gen.index_inputs()
    assert len(inputs) == 269 and inputs[-1] == b"" and sorted(fx) == sorted(str(t) for t in gen.INDEX_TYPES)
    out = {}
    for t in gen.INDEX_TYPES:
        size = 16 if t == FLOAT else 8
        rec = fx[str(t)]
        assert rec["encoded_size"] == [size] and len(rec["keys"]) == 2 * size * len(inputs)
        keys = bytes.fromhex(rec["keys"])
        out[t] = [(v, keys[size * i:size * (i + 1)]) for i, v in enumerate(inputs)]
    for t in dt.TIMESTAMPS:
        out[t] = out[gen.INDEX_TYPES[2]]
    assert out[INT64] == out[dt.TIMESTAMPS[0]]  # the delegation, as recorded
    # FLOAT: the hash, then the value's own bytes — or zeros for the empty value
    assert all(k[8:] == (v or bytes(8)) for v, k in out[FLOAT])
    return out


def test_oracle_matches_fixture_index_keys(oracle):
    for t, rows in index_cases().items():
        for v, want in rows:
            assert oracle.index_encode(t, v) == (want, 0), (t, v.hex())


# the recorded region counts for 3 attributes and 8, 27, 64, 125, 216, 1000 servers: the side starts at
# uint64_t(pow(servers, 1 / 3.)) and the growth loop starts from 3 * side (sic), so 27 servers get 4 x 4 x 4
CUBE_REGIONS = [12, 64, 64, 125, 216, 1000]


def partition_records():
    return json.loads(fixture_text())["partition"]


def test_oracle_matches_fixture_partition(oracle):
    recs = partition_records()
    assert [(r["num_attrs"], r["num_servers"]) for r in recs] == gen.PARTITION_PAIRS
    for r in recs:
        lower, upper = oracle.partition(r["num_attrs"], r["num_servers"])
        assert len(lower) == r["regions"], (r["num_attrs"], r["num_servers"], len(lower))
        lists = []
        for lows in gen.dimension_lowers(lower):
            rec = gen.lower_bounds_record(lows)
            if rec not in lists:
                lists.append(rec)
        assert lists == r["lower_bounds"], (r["num_attrs"], r["num_servers"])
        assert [lists.index(gen.lower_bounds_record(lows)) for lows in gen.dimension_lowers(lower)] == r["dimensions"]
        assert gen.boxes_sha256(lower, upper) == r["boxes_sha256"], (r["num_attrs"], r["num_servers"])
    # the quirks are in: a floor of pow() below a perfect power, and an interval that does not divide 2^64
    by_pair = {(r["num_attrs"], r["num_servers"]): r for r in recs}
    assert by_pair[(1, 3)]["lower_bounds"][0][1] == "5555555555555554"
    assert [by_pair[(3, s)]["regions"] for s in (8, 27, 64, 125, 216, 1000)] == CUBE_REGIONS


def test_fixture_regenerates_from_the_reference(oracle):
    _ref_or_skip(oracle)
    assert gen.dumps(gen.build_fixture(oracle)) == fixture_text()


# ---- 3. the kernels against the fixture ------------------------------------------------------------

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


def launches_with_malformed_alone(bad):
    """[(first, count)] covering 0..n: every bad value a launch of its own,
    the runs of good values between them one launch each."""
    out, i, n = [], 0, len(bad)
    while i < n:
        j = i + 1
        while not bad[i] and j < n and not bad[j]:
            j += 1
        out.append((i, j - i))
        i = j
    return out


def run_sweep(torch, dev, s, layout, launches):
    """hdx_hash_encoded_device over each (first, count) of `launches` on the
    same uploaded store -> (coords, versions, status word per launch)."""
    enc = store_arrays(s.objects, layout)
    d = [to_dev(torch, dev, x) for x in enc]
    if layout == "records":
        d[3] = d[0]  # one store on the device too
    keys, key_off, key_len, vals, val_off, val_len = d
    coords = torch.full((s.n, s.A), -1, dtype=torch.int64, device=dev)
    versions = torch.full((s.n,), -1, dtype=torch.int64, device=dev)
    status = torch.zeros(len(launches), dtype=torch.int32, device=dev)
    for k, (first, count) in enumerate(launches):
        sl = slice(first, first + count)
        hdx.hash_encoded(s.types, keys, key_off[sl], key_len[sl], vals, val_off[sl], val_len[sl],
                         coords=coords[sl], versions=versions[sl], status=status[k:k + 1])
    torch.cuda.synchronize()
    return coords.cpu().numpy().view(np.uint64), versions.cpu().numpy().view(np.uint64), status.cpu().numpy()


def check_sweep(torch, dev, s, layout):
    for launches in ([(0, s.n)], launches_with_malformed_alone(s.bad)):
        coords, versions, status = run_sweep(torch, dev, s, layout, launches)
        want = [(1 << _lib.HDX_E_BADENC) if s.bad[f:f + c].any() else 0 for f, c in launches]
        assert status.tolist() == want, (layout, len(launches))
        assert np.array_equal(versions, s.versions), (layout, len(launches), np.nonzero(versions != s.versions)[0][:8])
        wrong = np.argwhere(coords != s.coords)
        assert wrong.size == 0, \
            "%s, %d launches: value %d (%s) attribute %d: got %016x, the reference %016x; %d differ" % (
                layout, len(launches), wrong[0][0], s.records[wrong[0][0]]["kind"], wrong[0][1],
                coords[tuple(wrong[0])], s.coords[tuple(wrong[0])], len(wrong))
    alone = launches_with_malformed_alone(s.bad)
    assert sum(c == 1 and s.bad[f] for f, c in alone) == s.bad.sum() and sum(c for _, c in alone) == s.n


# (schema, debug variant or None): the product policy on every schema — the
# wave-staged sweep with NUM2 for a1 (keys only), a2, a5, a17, its round-5 form
# for a9 (timestamps), the wide walk + hash for a129 — and through the debug
# library the product sweep (230; a9: the round-5 form) and the gather sweep of
# hdx_encoded.hip (49), the ids test_encoded.py uses for them
SWEEP_ROWS = ([(name, None) for name in SCHEMA_NAMES] + [("a9", 230), ("a17", 230)] +
              [(name, 49) for name in SCHEMA_NAMES if name != "a129"])


def check_policy_form(s, name):
    """What can be read of the policy's choice: the wave-staged sweep's geometry
    (None: the wide sweep) and NUM2's condition (hdx_wsweep.h num2_codes: strings,
    int64 and floats only), with the batch policy's form where it tells the two
    apart (212 <-> NUM2, 46 <-> the round-5 form, as in test_reference_hash.py)."""
    g = hdx.hashing.wave_geometry(s.types, sweep=True)
    if name == "a129":
        assert g is None and s.A > 128
        return
    assert g["objects"] == gen.OBJECTS_PER_WAVE and g["window"] == 9728 < gen.LONG_STRING_BYTES
    num2 = set(s.types.tolist()) <= {STRING, INT64, FLOAT}
    assert num2 == (name != "a9")
    if name == "a17":
        assert hdx.hashing.kernel_for(s.types, s.n)[0] == 212
    if name == "a9":
        assert hdx.hashing.kernel_for(s.types, s.n)[0] == 46


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["columns", "keycol", "records"])
@pytest.mark.parametrize("row", SWEEP_ROWS, ids=lambda r: "%s-%s" % r)
def test_sweep_matches_fixture(torch_dev, row, layout):
    torch, dev = torch_dev
    name, variant = row
    s = stored(name)
    check_policy_form(s, name)
    if variant is None:
        check_sweep(torch, dev, s, layout)
    else:
        with _lib.debug_library(variant):
            check_sweep(torch, dev, s, layout)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [None, 49])
@pytest.mark.parametrize("layout", ["keycol", "records"])
def test_sweep_value_longer_than_the_window(torch_dev, layout, variant):
    """A string the 9.5 KiB window cannot hold goes through the walk and the
    hash from global memory: well-formed, and with its last byte missing (class
    L: in the records layout the next record's key lies where it would read).
    Among a2's own values, so the waves hold both sorts."""
    torch, dev = torch_dev
    a2, long = stored("a2"), stored("long")
    s = Stored()
    s.types, s.A = a2.types, a2.A
    at = [3, 9]  # odd positions: well-formed neighbours stay on both sides
    s.objects, s.records = list(a2.objects), list(a2.records)
    s.bad, s.versions, s.coords = a2.bad.copy(), a2.versions.copy(), a2.coords.copy()
    for k, where in enumerate(at):
        s.objects.insert(where, long.objects[k])
        s.records.insert(where, long.records[k])
        s.bad = np.insert(s.bad, where, long.bad[k])
        s.versions = np.insert(s.versions, where, long.versions[k])
        s.coords = np.insert(s.coords, where, long.coords[k], axis=0)
    s.n = a2.n + len(at)
    assert s.bad[at].tolist() == [False, True] and s.coords[at[0]].all() and not s.coords[at[1]].any()
    assert hdx.hashing.wave_geometry(s.types, sweep=True)["window"] < min(len(v) for _, v in long.objects)
    if variant is None:
        check_sweep(torch, dev, s, layout)
    else:
        with _lib.debug_library(variant):
            check_sweep(torch, dev, s, layout)


@pytest.mark.gpu
@pytest.mark.parametrize("t", (INT64, FLOAT) + tuple(dt.TIMESTAMPS))
def test_index_kernel_matches_fixture(torch_dev, t):
    """hdx_index_encode_device at n = 269, values back to back from an aligned
    start and from byte 3 (every value at an odd address; the empty one last)."""
    torch, dev = torch_dev
    rows = index_cases()[t]
    size = 16 if t == FLOAT else 8
    lens = np.array([len(v) for v, _ in rows], np.uint32)
    assert len(rows) == 269 and lens.tolist() == [8] * 268 + [0]
    off = np.arange(len(rows), dtype=np.uint64) * np.uint64(8)
    want = np.frombuffer(b"".join(k for _, k in rows), np.uint8).reshape(len(rows), size)
    for shift in (0, 3):
        blob = np.frombuffer(bytes(shift) + b"".join(v for v, _ in rows) + bytes(PAD), np.uint8)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        got = hdx.index.index_encode(t, to_dev(torch, dev, blob), to_dev(torch, dev, off + np.uint64(shift)),
                                     to_dev(torch, dev, lens), status=status)
        torch.cuda.synchronize()
        assert int(status.item()) == 0
        got = got.cpu().numpy()
        wrong = np.nonzero((got != want).any(axis=1))[0]
        assert wrong.size == 0, "shift %d value %d (%s): got %s, the reference %s" % (
            shift, wrong[0], rows[wrong[0]][0].hex(), got[wrong[0]].tobytes().hex(), rows[wrong[0]][1].hex())


@pytest.mark.gpu
def test_device_value_generator_writes_the_host_encoding(torch_dev):
    """synth.make_encoded_device's values for a 64-object config-3b store,
    copied back, are synth.encode_values_host's of the same objects (the two
    generators share their seed contract; the host one is pinned to the
    reference's encode_value above)."""
    torch, dev = torch_dev
    n, first = 64, 4242
    host = synth.encode_values_host(*synth.make_batch_host("cfg3b", n, seed=99, first=first), first_version=first)
    got = synth.make_encoded_device("cfg3b", n, seed=99, first=first, device=dev)
    torch.cuda.synchronize()
    assert np.array_equal(got[4].cpu().numpy()[:len(host[3])], host[3])
    assert len(host[3]) == int(host[4][-1]) + int(host[5][-1])
    for g, h in zip((got[2], got[3], got[5], got[6]), (host[1], host[2], host[4], host[5])):
        assert np.array_equal(g.cpu().numpy().view(h.dtype), h)
    assert np.array_equal(got[1].cpu().numpy()[:len(host[0])], host[0])
