"""The top-limit matches by one attribute (hdx_compare, hdx_sorted_search, hdx_sorted_search_device;
include/hdxhash.h): what search_manager::sorted_search (daemon/search_manager.cc:305-502) does with the
objects that pass a search's checks.

Two restatements live here; the pools, `compare` and `expected_first_fail` are test_checks.py's.
  R1 (`r1`)  the contract of include/hdxhash.h: sorted() on (value, index) with functools.cmp_to_key.
             Compared exactly, by index.
  R2 (`r2`)  search_manager::sorted_search as written (:355-423, :469-484): heapq over items whose
             __lt__(a, b) is the reference's operator<(b, a), popped when over `limit`, then a sort by the
             reference's operator>.  The reference's order among ties is unspecified, so R2 is compared by
             the sequence of sort values under compare == 0.
R1's `compare` is pinned to the reference's compiled datatype_*::compare by tests/test_reference_checks.py
(`sort_compare` wherever no NaN is involved; the NaN rule is the library's own).  R2 is unpinned: no
committed recipe compiles search_manager.cc, which needs the whole daemon."""
import ctypes
import functools
import heapq
import os
import struct
import subprocess

import numpy as np
import pytest

import hyperdex_amd as hdx
from hyperdex_amd import _lib
from hyperdex_amd.checks import AttributeCheck, _checks
from hyperdex_amd.sorting import KEEP_LARGEST, KEEP_SMALLEST, HDX_SORT_LIMIT_MAX, SortSpec, _Sort, sort_finish_block
from test_checks import (BADENC_BIT, BADENC_FF, BASE, DIFF_AT, F64, FLOAT, GE, I64, INT64, LE, LEN_GE, LISTS,
                         LIST_STRING, MIS_SIZED, SCHEMA, STRING, STRINGS, TS_DAY, Batch, _flip, compare, encode,
                         expected_first_fail, pair_batch, q, second_level, to_dev, torch_gpu)  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BADSIZE_BIT = 1 << _lib.HDX_E_BADSIZE
KEEPS = (KEEP_SMALLEST, KEEP_LARGEST)
USED = ("ladder", "longish", "long_prefix")  # the lists of test_checks.LISTS the pooled batch is searched with


# ---- the restatements ----------------------------------------------------------------------------

def is_nan(b):
    return len(b) == 8 and (struct.unpack("<Q", b)[0] & 0x7fffffffffffffff) > 0x7ff0000000000000


def sort_compare(t, a, b):
    """The contract's order: compare, and the library's own rule for NaN (above +inf, all tie)."""
    if t is None:
        return 0  # attr >= attrs_sz: every object ties
    if t == FLOAT and (is_nan(a) or is_nan(b)):
        return int(is_nan(a)) - int(is_nan(b))
    return compare(t, a, b)


def sort_value(objs, attr, i):
    """The key, an attribute, or nothing where attr lies beyond the schema."""
    return objs[i][0] if attr == 0 else objs[i][1][attr - 1] if attr <= len(objs[i][1]) else b""


def members(types, objs, ff, c, attr):
    """(S as indices, status bits): the matching objects whose sort value is not a mis-sized numeric."""
    t = types[attr] if attr < len(types) else None
    S, bits = [], 0
    for i in range(len(objs)):
        if ff[i] == BADENC_FF:
            bits |= BADENC_BIT
        if ff[i] != c:
            continue
        if t not in (None, STRING) and len(sort_value(objs, attr, i)) not in (0, 8):
            bits |= BADSIZE_BIT
            continue
        S.append(i)
    return S, bits


def kept_order(types, objs, S, attr, keep):
    """S ordered by (value ascending, or descending for KEEP_LARGEST; index ascending)."""
    t = types[attr] if attr < len(types) else None
    sign = -1 if keep == KEEP_LARGEST else 1

    def cmp(i, j):
        return sign * sort_compare(t, sort_value(objs, attr, i), sort_value(objs, attr, j)) or (i > j) - (i < j)
    return sorted(S, key=functools.cmp_to_key(cmp))


def output_order(types, objs, kept, attr, descending):
    t = types[attr] if attr < len(types) else None
    sign = -1 if descending else 1

    def cmp(i, j):
        return sign * sort_compare(t, sort_value(objs, attr, i), sort_value(objs, attr, j)) or (i > j) - (i < j)
    return sorted(kept, key=functools.cmp_to_key(cmp))


def r1(types, objs, ff, c, spec, limit):
    """R1: (top, status bits)."""
    S, bits = members(types, objs, ff, c, spec.attr)
    kept = kept_order(types, objs, S, spec.attr, spec.keep)[:limit]
    return output_order(types, objs, kept, spec.attr, spec.descending), bits


class RefItem:
    """_sorted_search_item with the reference's two operators (search_manager.cc:355-423)."""

    def __init__(self, t, v, maximize):
        self.t, self.v, self.maximize = t, v, maximize

    def ref_lt(self, o):
        c = compare(self.t, self.v, o.v)
        return c < 0 if self.maximize else c > 0

    def ref_gt(self, o):
        c = compare(self.t, self.v, o.v)
        return c > 0 if self.maximize else c < 0

    def __lt__(self, o):  # heapq pops its least: the reference's std::pop_heap pops its greatest under <
        return o.ref_lt(self)


def r2(t, values, limit, maximize):
    """R2: the sort values in the order the daemon sends them (:469-484)."""
    top = []
    for v in values:
        heapq.heappush(top, RefItem(t, v, maximize))
        if len(top) > limit:
            heapq.heappop(top)
    top.sort(key=functools.cmp_to_key(lambda a, b: -1 if a.ref_gt(b) else 1 if b.ref_gt(a) else 0))
    return [x.v for x in top]


# ---- helpers -------------------------------------------------------------------------------------

def host(types, enc, checks, spec, limit):
    top, bits = hdx.sorted_search_host(types, *enc, checks, spec, limit)
    return top.tolist(), bits


class Pooled:
    """test_checks.Batch's 2 000 objects, encoded once; S and the kept orders per (list, attr, keep)."""
    _the = None

    def __init__(self):
        self.b = Batch.get()
        self.objs = self.b.objs
        self.enc = encode(SCHEMA, self.objs, "keycol")
        self._kept = {}

    @classmethod
    def get(cls):
        if cls._the is None:
            cls._the = cls()
        return cls._the

    def kept(self, name, attr, keep):
        k = (name, attr, keep)
        if k not in self._kept:
            S, bits = members(SCHEMA, self.objs, self.b.want[name], len(LISTS[name]), attr)
            self._kept[k] = (kept_order(SCHEMA, self.objs, S, attr, keep), bits)
        return self._kept[k]

    def want(self, name, spec, limit):
        kept, bits = self.kept(name, spec.attr, spec.keep)
        return output_order(SCHEMA, self.objs, kept[:limit], spec.attr, spec.descending), bits

    def assert_condition(self, limits_of):
        """On the expected values alone: every list both passes and fails a tenth of the objects, and
        per sort attribute some case with 0 < limit < |S| has a tie straddling the boundary."""
        for name in USED:
            rate = float((self.b.want[name] == len(LISTS[name])).mean())
            assert 0.10 <= rate <= 0.90, (name, rate)
        for attr in range(len(SCHEMA)):
            straddles = 0
            for name in USED:
                for keep in KEEPS:
                    kept, _ = self.kept(name, attr, keep)
                    for limit in limits_of(len(kept)):
                        if 0 < limit < len(kept):
                            a, b_ = (sort_value(self.objs, attr, kept[limit - 1]), sort_value(self.objs, attr, kept[limit]))
                            straddles += sort_compare(SCHEMA[attr], a, b_) == 0
            assert straddles > 0, attr


def host_limits(size):
    return sorted({0, 1, 3, max(size - 1, 0), size, size + 1, 5000})


# ---- 1. hdx_compare ------------------------------------------------------------------------------

def test_compare_matches_the_restatement():
    for t, pool in ((STRING, STRINGS), (INT64, I64), (FLOAT, F64), (TS_DAY, I64)):
        for a in pool:
            for b in pool:
                assert hdx.compare(t, a, b) == compare(t, a, b), (t, a, b)
    cmp = ctypes.c_int(77)
    for t in (INT64, FLOAT, TS_DAY):
        for bad in MIS_SIZED:
            for a, b in ((bad, q(1)), (q(1), bad), (bad, b""), (bad, bad)):
                assert hdx.lib().hdx_compare(t, a, len(a), b, len(b), ctypes.byref(cmp)) == _lib.HDX_E_BADSIZE
    for t in (LIST_STRING, 12345, 0):
        assert hdx.lib().hdx_compare(t, b"", 0, b"", 0, ctypes.byref(cmp)) == _lib.HDX_E_BADTYPE
    assert hdx.lib().hdx_compare(STRING, b"", 0, b"", 0, None) == _lib.HDX_E_INVALID
    assert hdx.lib().hdx_compare(STRING, None, 2, b"", 0, ctypes.byref(cmp)) == _lib.HDX_E_INVALID
    assert cmp.value == 77
    assert hdx.compare(STRING, b"ab", b"ab\0") == -1 and hdx.compare(FLOAT, F64[6], F64[2]) == 0


# ---- 2. the host form against R1 -----------------------------------------------------------------

def test_host_matches_the_contract():
    p = Pooled.get()
    p.assert_condition(host_limits)
    cases = 0
    for name in USED:
        for attr in range(len(SCHEMA)):
            for keep in KEEPS:
                size = len(p.kept(name, attr, keep)[0])
                for desc in (0, 1):
                    for limit in host_limits(size):
                        spec = SortSpec(attr, keep, desc)
                        assert host(SCHEMA, p.enc, LISTS[name], spec, limit) == p.want(name, spec, limit), (name, spec, limit)
                        cases += 1
    assert cases >= 3 * 6 * 2 * 2 * 6


def plain_objects(n, seed):
    """Objects under SCHEMA whose numerics are neither NaN nor mis-sized: where R2 is defined."""
    rng = np.random.default_rng(seed)
    f64 = [x for x in F64 if not is_nan(x)]

    def pick(pool):
        return pool[int(rng.integers(len(pool)))]
    return [(pick(STRINGS), [pick(STRINGS), pick(I64), pick(f64), pick(I64), pick(STRINGS)]) for _ in range(n)]


def test_host_mappings_against_the_daemon_as_written():
    """(KEEP_SMALLEST, descending) is the daemon with maximize, (KEEP_LARGEST, ascending) without."""
    vals = [5, 1, 9, 3, 7, 2, 8]
    objs = [(b"k%d" % i, [q(v)]) for i, v in enumerate(vals)]
    enc = encode([STRING, INT64], objs, "keycol")
    for (keep, desc, maximize), known in (((KEEP_LARGEST, 0, False), [7, 8, 9]), ((KEEP_SMALLEST, 1, True), [3, 2, 1])):
        top, _ = host([STRING, INT64], enc, [], SortSpec(1, keep, desc), 3)
        assert [vals[i] for i in top] == known
        assert [struct.unpack("<q", v)[0] for v in r2(INT64, [q(v) for v in vals], 3, maximize)] == known
    objs = plain_objects(400, 31)
    checks = [AttributeCheck(1, q(12), INT64, LEN_GE)]
    ff = [expected_first_fail(SCHEMA, k, vs, checks) for k, vs in objs]
    match = [i for i in range(len(objs)) if ff[i] == 1]
    assert 0.1 * len(objs) <= len(match) <= 0.9 * len(objs)
    enc = encode(SCHEMA, objs, "keycol")
    for attr in range(len(SCHEMA)):
        t = SCHEMA[attr]
        values = [sort_value(objs, attr, i) for i in match]
        # R2 is only defined here
        assert all(not (t == FLOAT and is_nan(v)) and (t == STRING or len(v) in (0, 8)) for v in values)
        for limit in (1, 3, 50, len(match) - 1, len(match), len(match) + 1):
            for keep, desc, maximize in ((KEEP_SMALLEST, 1, True), (KEEP_LARGEST, 0, False)):
                top, bits = host(SCHEMA, enc, checks, SortSpec(attr, keep, desc), limit)
                got = [sort_value(objs, attr, i) for i in top]
                want = r2(t, values, limit, maximize)
                assert bits == 0 and len(got) == len(want) == min(limit, len(match))
                assert all(compare(t, a, b) == 0 for a, b in zip(got, want)), (attr, limit, maximize)


def special_objects():
    """Under [STRING, FLOAT, INT64]: NaNs of both signs among ordinary floats; mis-sized values in
    matching and in non-matching objects (the check: attribute 2's key length >= 2)."""
    f = [struct.pack("<d", x) for x in (1.5, float("inf"), float("-inf"), -0.0, 0.0)] + \
        [struct.pack("<Q", x) for x in (0x7ff8000000000001, 0xfff0000000000123, 0x7ff0000000000001)] + [b""]
    objs = []
    for i in range(60):
        key = b"k" if i % 5 == 0 else b"key%02d" % i          # every fifth object does not match
        fv = MIS_SIZED[i % 8] if i % 7 == 3 else f[i % len(f)]
        iv = MIS_SIZED[i % 8] if i % 11 == 5 else q(i % 4 - 2)
        objs.append((key, [fv, iv]))
    return objs


SPECIAL_TYPES = [STRING, FLOAT, INT64]
SPECIAL_CHECKS = [AttributeCheck(0, q(2), INT64, LEN_GE)]


def test_host_nan_missized_and_badenc():
    objs = special_objects()
    ff = np.array([expected_first_fail(SPECIAL_TYPES, k, vs, SPECIAL_CHECKS) for k, vs in objs], np.uint32)
    enc = encode(SPECIAL_TYPES, objs, "keycol")
    # the NaN rule: every NaN above +inf, all NaNs tie (so by index); mis-sized values left out
    top, bits = host(SPECIAL_TYPES, enc, SPECIAL_CHECKS, SortSpec(1, KEEP_LARGEST, 1), 6)
    nans = [i for i in range(60) if ff[i] == 1 and is_nan(objs[i][1][0])]
    assert len(nans) > 6 and top == nans[:6] and bits == BADSIZE_BIT
    for attr in (1, 2):
        for keep in KEEPS:
            for desc in (0, 1):
                for limit in (1, 5, 40, 60):
                    spec = SortSpec(attr, keep, desc)
                    want = r1(SPECIAL_TYPES, objs, ff, 1, spec, limit)
                    assert host(SPECIAL_TYPES, enc, SPECIAL_CHECKS, spec, limit) == want
                    assert want[1] == BADSIZE_BIT and not any(len(objs[i][1][attr - 1]) not in (0, 8) for i in want[0])
    # mis-sized values in non-matching objects only: ignored
    only = [(k if len(vs[1]) in (0, 8) else b"k", vs) for k, vs in objs]
    ff2 = np.array([expected_first_fail(SPECIAL_TYPES, k, vs, SPECIAL_CHECKS) for k, vs in only], np.uint32)
    assert any(len(vs[1]) not in (0, 8) for _, vs in only)
    got = host(SPECIAL_TYPES, encode(SPECIAL_TYPES, only, "keycol"), SPECIAL_CHECKS, SortSpec(2), 60)
    assert got == r1(SPECIAL_TYPES, only, ff2, 1, SortSpec(2), 60) and got[1] == 0
    # values that do not decode: left out, the bit set
    keys, key_off, key_len, vals, val_off, val_len = [np.array(x) for x in enc]
    val_len[[4, 17, 33]] -= 1
    ff3 = ff.copy()
    ff3[[4, 17, 33]] = BADENC_FF
    got = host(SPECIAL_TYPES, (keys, key_off, key_len, vals, val_off, val_len), SPECIAL_CHECKS, SortSpec(2), 60)
    assert got == r1(SPECIAL_TYPES, objs, ff3, 1, SortSpec(2), 60)
    assert got[1] == BADENC_BIT | BADSIZE_BIT and not {4, 17, 33} & set(got[0])


def test_host_attr_beyond_the_schema_and_key_only():
    p = Pooled.get()
    match = np.nonzero(p.b.want["ladder"] == 4)[0].tolist()
    for attr in (len(SCHEMA), 0xffffffff):
        for keep in KEEPS:
            for desc in (0, 1):
                for limit in (0, 1, 7, len(match) + 5):
                    assert host(SCHEMA, p.enc, LISTS["ladder"], SortSpec(attr, keep, desc), limit) == (match[:limit], 0)
    objs = [(q(v), []) for v in (5, 1, 9)]
    assert host([INT64], encode([INT64], objs, "keycol"), [], SortSpec(0), 2) == ([1, 0], 0)


# ---- 3. refusals ---------------------------------------------------------------------------------

def _call(device, types, checks, sort=(1, 0, 0, 0), limit=3, null=None, c=None):
    """hdx_sorted_search / _device with stand-in (never dereferenced) object pointers; returns the
    status and whether the outputs were left alone."""
    t = np.asarray(types, np.uint32)
    p = {k: 4096 * (i + 1) for i, k in enumerate(("keys", "key_off", "key_len", "vals", "val_off", "val_len"))}
    top = np.full(4, 0xabcd, np.uint64)
    count, status = ctypes.c_uint64(0xabcd), ctypes.c_uint32(0xabcd)
    spec = _Sort(*sort)
    a = {"types": t.ctypes.data, "checks": _checks(checks), "sort": ctypes.byref(spec), "top": top.ctypes.data,
         "top_count": ctypes.byref(count)}
    if null in a:
        a[null] = None
    elif null:
        p[null] = None
    obj = [p[k] for k in ("keys", "key_off", "key_len", "vals", "val_off", "val_len")]
    nc = len(checks) if c is None else c
    if device:
        st = hdx.lib().hdx_sorted_search_device(a["types"], len(t), *obj, 5, a["checks"], nc, a["sort"], limit, None,
                                                a["top"], a["top_count"], None, None)
    else:
        st = hdx.lib().hdx_sorted_search(a["types"], len(t), *obj, 0, a["checks"], nc, a["sort"], limit, a["top"],
                                         a["top_count"], ctypes.byref(status))
    assert st != _lib.HDX_OK or not device
    untouched = (top == 0xabcd).all() and count.value == 0xabcd and status.value == 0xabcd
    return st, bool(untouched)


@pytest.mark.parametrize("device", [False, True])
def test_refusals(device):
    types = [STRING, STRING, INT64, LIST_STRING]
    ok = [AttributeCheck(1, b"abc", STRING, LE)]
    bad = (_lib.HDX_E_INVALID, True)
    for null in ("types", "checks", "sort", "top", "top_count", "keys", "key_off", "key_len", "vals", "val_off", "val_len"):
        assert _call(device, types, ok, null=null) == bad, null
    for sort in ((1, 2, 0, 0), (1, 0, 2, 0), (1, 0, 0, 1)):
        assert _call(device, types, ok, sort=sort) == bad, sort
    assert _call(device, types, [ok[0]] * 17) == bad
    assert _call(device, types, ok, sort=(3, 0, 0, 0)) == (_lib.HDX_E_BADTYPE, True)        # a container sort attribute
    assert _call(device, [12345, STRING], [], sort=(0, 0, 0, 0)) == (_lib.HDX_E_BADTYPE, True)
    assert _call(device, types, [AttributeCheck(3, b"", STRING, LE)]) == (_lib.HDX_E_BADTYPE, True)  # as the checks'
    if device:
        assert _call(True, types, ok, limit=HDX_SORT_LIMIT_MAX + 1) == bad
        assert _call(True, types, [AttributeCheck(1, bytes(1025), STRING, GE)]) == bad
        if hdx.lib().hdx_device_count() == 0:  # valid arguments reach the device binding, and only then
            for limit in (0, HDX_SORT_LIMIT_MAX):
                assert _call(True, types, ok, limit=limit) == (_lib.HDX_E_DEVICE, True)
            assert _call(True, types, ok, sort=(4, 1, 1, 0)) == (_lib.HDX_E_DEVICE, True)
    else:  # n == 0 here: any limit, no cap on the checks' bytes, an empty result
        for limit in (0, 3, 1 << 40):
            assert _call(False, types, ok, limit=limit)[0] == _lib.HDX_OK
        assert _call(False, types, [AttributeCheck(1, bytes(1025), STRING, GE)])[0] == _lib.HDX_OK
        assert _call(False, types, ok, sort=(9, 1, 1, 0))[0] == _lib.HDX_OK
    assert sort_finish_block() >= HDX_SORT_LIMIT_MAX and sort_finish_block() & (sort_finish_block() - 1) == 0


# ---- 4. the host form under ASan and UBSan ---------------------------------------------------------

def test_host_form_sanitized(tmp_path):
    """tests/cpp/sorted_search_test.cc + hdx_cpu.cpp as one program under -fsanitize=address,undefined
    (no Python, no device).  The sanitizers' runtimes are linked statically, so the program needs nothing
    from its environment, which it inherits as it is.  A missing g++ fails the test."""
    inc = ["-I" + os.path.join(ROOT, "hyperdex_amd", "csrc"), "-I" + os.path.join(ROOT, "include")]
    exe = str(tmp_path / "sorted_search_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", *inc,
                    os.path.join(ROOT, "tests", "cpp", "sorted_search_test.cc"),
                    os.path.join(ROOT, "hyperdex_amd", "csrc", "hdx_cpu.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "sorted_search_test ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---- the device ----------------------------------------------------------------------------------

def run(torch, types, d, checks, spec, limit, stream=None, want_first_fail=True):
    dev = torch.device("cuda", 0)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    ff, top = hdx.sorted_search(types, *d, checks, spec, limit, want_first_fail=want_first_fail, status=status,
                                stream=stream)
    (stream or torch.cuda.current_stream(dev)).synchronize()
    return (None if ff is None else ff.cpu().numpy().view(np.uint32), top.cpu().numpy().view(np.uint64).tolist(),
            int(status.item()) & 0xffffffff)


DEVICE_LIMITS = (0, 1, 3, 64, 1024)


@pytest.mark.gpu
@pytest.mark.parametrize("name", USED)
def test_gpu_pooled(torch_gpu, name):
    """The pooled batch: every type of SCHEMA and the key, both keeps, both orders."""
    p = Pooled.get()
    p.assert_condition(lambda size: DEVICE_LIMITS)
    d = to_dev(torch_gpu, p.enc)
    for attr in range(len(SCHEMA) + 1):
        for keep in KEEPS:
            for desc in (0, 1):
                for limit in DEVICE_LIMITS:
                    spec = SortSpec(attr, keep, desc)
                    ff, top, bits = run(torch_gpu, SCHEMA, d, LISTS[name], spec, limit)
                    assert np.array_equal(ff, p.b.want[name])
                    assert (top, bits) == p.want(name, spec, limit), (spec, limit)
                    if limit in (3, 1024):
                        assert (top, bits) == host(SCHEMA, p.enc, LISTS[name], spec, limit)


@pytest.mark.gpu
@pytest.mark.parametrize("layout,shift", [("records", 0), ("records", 5), ("columns", 3), ("keycol", 9)])
def test_gpu_layouts(torch_gpu, layout, shift):
    """keys == vals records, and stores at odd addresses."""
    p = Pooled.get()
    enc = encode(SCHEMA, p.objs, layout)
    assert (enc[0] is enc[3]) == (layout == "records")
    d = to_dev(torch_gpu, enc, shift)
    for attr in range(len(SCHEMA)):
        spec = SortSpec(attr, attr & 1, (attr >> 1) & 1)
        ff, top, bits = run(torch_gpu, SCHEMA, d, LISTS["ladder"], spec, 64)
        assert (top, bits) == p.want("ladder", spec, 64), attr


@pytest.mark.gpu
def test_gpu_nan_missized_and_badenc(torch_gpu):
    objs = special_objects()
    ff = np.array([expected_first_fail(SPECIAL_TYPES, k, vs, SPECIAL_CHECKS) for k, vs in objs], np.uint32)
    enc = [np.array(x) for x in encode(SPECIAL_TYPES, objs, "keycol")]
    enc[5][[4, 17, 33]] -= 1
    ff[[4, 17, 33]] = BADENC_FF
    d = to_dev(torch_gpu, enc)
    for attr in (0, 1, 2):
        for keep in KEEPS:
            for desc in (0, 1):
                for limit in (1, 6, 60):
                    spec = SortSpec(attr, keep, desc)
                    got = run(torch_gpu, SPECIAL_TYPES, d, SPECIAL_CHECKS, spec, limit)
                    want = r1(SPECIAL_TYPES, objs, ff, 1, spec, limit)
                    assert np.array_equal(got[0], ff) and got[1:] == want, (spec, limit)
                    assert want[1] == (BADENC_BIT | BADSIZE_BIT if attr else BADENC_BIT)
                    assert got[1:] == host(SPECIAL_TYPES, enc, SPECIAL_CHECKS, spec, limit)


def int_batch(values, keys=None):
    objs = [((b"k%03d" % i) if keys is None else keys[i], [q(v)]) for i, v in enumerate(values)]
    return objs, encode([STRING, INT64], objs, "keycol")


@pytest.mark.gpu
def test_gpu_radix_passes(torch_gpu):
    """INT64 sort values 1 << b, 0 and -1: the deciding bit sits in every possible digit."""
    types = [STRING, INT64]
    values = [(1 << b) if b < 63 else -(1 << 63) for b in range(64)] + [0, -1]
    np.random.default_rng(9).shuffle(values)
    objs, enc = int_batch(values)
    d = to_dev(torch_gpu, enc)
    ff = np.zeros(len(objs), np.uint32)
    for limit in range(1, 67):
        for keep in KEEPS:
            spec = SortSpec(1, keep, limit & 1)
            assert run(torch_gpu, types, d, [], spec, limit)[1:] == r1(types, objs, ff, 0, spec, limit), (limit, keep)
    # every value equal: the index alone decides
    objs, enc = int_batch([7] * 700)
    d = to_dev(torch_gpu, enc)
    for keep in KEEPS:
        for desc in (0, 1):
            for limit in (1, 255, 256, 700, 1024):
                assert run(torch_gpu, types, d, [], SortSpec(1, keep, desc), limit)[1] == list(range(min(limit, 700)))
    # exactly `limit` objects match, fewer match, none match
    values = list(range(300, 0, -1))
    objs, enc = int_batch(values, keys=[b"kk" if i % 10 == 0 else b"k" for i in range(300)])
    d = to_dev(torch_gpu, enc)
    for checks, c in (([AttributeCheck(0, q(2), INT64, LEN_GE)], 30), ([AttributeCheck(0, q(3), INT64, LEN_GE)], 0)):
        ff = np.array([expected_first_fail(types, k, vs, checks) for k, vs in objs], np.uint32)
        assert int((ff == 1).sum()) == c
        for limit in (30, 31, 1024, 29):
            for keep in KEEPS:
                spec = SortSpec(1, keep, 0)
                assert run(torch_gpu, types, d, checks, spec, limit)[1:] == r1(types, objs, ff, 1, spec, limit)


@pytest.mark.gpu
def test_gpu_string_boundary(torch_gpu):
    """Strings that share their 8-byte rank key and differ later, or in length alone."""
    types = [STRING, STRING]
    edge = [b"ab", b"ab\0", b"ab\0\0", b"", b"\x7f" + BASE[:9], b"\x80" + BASE[:9], b"abcdefgh", b"abcdefgh\0", BASE]
    assert {7, 8, 15, 16, 40} <= set(DIFF_AT)
    edge += [_flip(BASE, p) for p in (7, 8, 15, 16, 40)] + [BASE[:8], BASE[:7], BASE[:9], BASE[:16]]
    rng = np.random.default_rng(3)
    strings = [edge[i] for i in rng.permutation(len(edge) * 3) % len(edge)]
    for as_key in (False, True):
        objs = [(s, [b"x"]) if as_key else (b"k%d" % i, [s]) for i, s in enumerate(strings)]
        ff = np.zeros(len(objs), np.uint32)
        d = to_dev(torch_gpu, encode(types, objs, "keycol"))
        for limit in range(1, len(objs) + 2):
            for keep in KEEPS:
                spec = SortSpec(0 if as_key else 1, keep, limit & 1)
                assert run(torch_gpu, types, d, [], spec, limit)[1:] == r1(types, objs, ff, 0, spec, limit), (limit, keep)
    # a group that shares 8 bytes and takes several rounds of the finishing step, the limit inside it
    F = sort_finish_block()
    group = [b"sameeight" + struct.pack(">I", int(x)) + b"tail" * int(x % 3) for x in rng.permutation(3 * F + 1)]
    strings = [b"a", b"b", b"zz"] + group[:2000] + [b"c", b"sameeigh", b"sameeight"] + group[2000:] + [b"zzz", b"d"]
    objs = [(b"k", [s]) for s in strings]
    ff = np.zeros(len(objs), np.uint32)
    enc = encode(types, objs, "keycol")
    d = to_dev(torch_gpu, enc)
    for keep in KEEPS:
        for limit, desc in ((1, 0), (5, 1), (700, 0), (1024, 1)):
            spec = SortSpec(1, keep, desc)
            got = run(torch_gpu, types, d, [], spec, limit)[1:]
            assert got == r1(types, objs, ff, 0, spec, limit), (keep, limit)
            assert got == host(types, enc, [], spec, limit)



@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 255, 256, 257, "level+257"])
def test_gpu_sizes(torch_gpu, n):
    """pair_batch: key = i as 4 little-endian bytes, attribute 1 = i & 1; every second object matches.
    The last size takes the scans' second level."""
    torch = torch_gpu
    if isinstance(n, str):
        n = second_level() - 1 + 257
        assert n == hdx.checks.check_block_objects() * hdx.index.SCAN_BLOCK + 257
    types = [STRING, INT64]
    d = pair_batch(torch, n)
    checks = [AttributeCheck(1, q(0), INT64, LE)]   # 0 >= the attribute: the even ones
    even = np.arange(0, n, 2, dtype=np.uint64)
    rank = even.astype(np.uint32).byteswap().astype(np.uint64)  # the key's bytes, big-endian
    order = even[np.lexsort((even, rank))]
    for spec, want in ((SortSpec(0, KEEP_SMALLEST, 0), order[:64]), (SortSpec(0, KEEP_LARGEST, 1), order[::-1][:64]),
                       (SortSpec(0, KEEP_LARGEST, 0), order[::-1][:64][::-1]), (SortSpec(1, KEEP_LARGEST, 1), even[:64]),
                       (SortSpec(7, KEEP_SMALLEST, 0), even[:64])):
        ff, top, bits = run(torch, types, d, checks, spec, 64)
        assert top == want.tolist() and bits == 0, spec
        assert np.array_equal(ff, (np.arange(n) & 1 == 0).astype(np.uint32))
    # the guard behind top_count entries stays
    dev = torch.device("cuda", 0)
    top = torch.full((1024,), -7, dtype=torch.int64, device=dev)
    count = torch.full((1,), -7, dtype=torch.int64, device=dev)
    t = np.asarray(types, np.uint32)
    spec = _Sort(0, 0, 0, 0)
    _lib.check(hdx.lib().hdx_sorted_search_device(
        t.ctypes.data, 2, *[x.data_ptr() for x in d], n, _checks(checks), 1, ctypes.byref(spec), 1000, None,
        top.data_ptr(), count.data_ptr(), None, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    k = int(count.item())
    assert k == min(1000, len(even)) and top[:k].tolist() == order[:k].tolist() and bool((top[k:] == -7).all())


@pytest.mark.gpu
def test_gpu_sort_value_ends_the_store(torch_gpu):
    """The sort attribute as the last bytes of vals, and the key as the last bytes of keys, at every
    alignment and with lengths 1..9."""
    cases = [([STRING, INT64], [(b"k", [q(x - 100)]) for x in (9, 200, 3, 77, 3)])]  # 8 bytes, whatever L
    for L in range(1, 10):
        tails = [bytes([65] * (L - 1) + [x]) for x in (9, 200, 3, 77, 3)]
        cases += [([STRING, STRING], [(b"key", [t]) for t in tails]), ([STRING, STRING], [(t, [b"v"]) for t in tails])]
    for types, objs in cases:
        attr = 0 if objs[0][1] == [b"v"] else 1
        enc = encode(types, objs, "keycol")
        assert int(enc[4][-1]) + int(enc[5][-1]) == len(enc[3]) and int(enc[1][-1]) + int(enc[2][-1]) == len(enc[0])
        ff = np.zeros(5, np.uint32)
        for shift in range(8):
            d = to_dev(torch_gpu, enc, shift)
            for keep in KEEPS:
                spec = SortSpec(attr, keep, keep)
                assert run(torch_gpu, types, d, [], spec, 3)[1:] == r1(types, objs, ff, 0, spec, 3), (shift, types, objs)


@pytest.mark.gpu
def test_gpu_side_stream_null_first_fail_and_twice(torch_gpu):
    torch = torch_gpu
    p = Pooled.get()
    dev = torch.device("cuda", 0)
    d = to_dev(torch, p.enc)
    spec = SortSpec(5, KEEP_LARGEST, 0)
    want = p.want("ladder", spec, 64)
    first = run(torch, SCHEMA, d, LISTS["ladder"], spec, 64)
    assert first[1:] == want
    # the same call again: nothing is left in pooled scratch between calls
    assert run(torch, SCHEMA, d, LISTS["ladder"], spec, 64)[1:] == want
    # a call in between with another shape, then again
    assert run(torch, SCHEMA, d, LISTS["longish"], SortSpec(2, KEEP_SMALLEST, 1), 1024)[1:] == \
        p.want("longish", SortSpec(2, KEEP_SMALLEST, 1), 1024)
    assert run(torch, SCHEMA, d, LISTS["ladder"], spec, 64)[1:] == want
    # first_fail == NULL: the same top
    got = run(torch, SCHEMA, d, LISTS["ladder"], spec, 64, want_first_fail=False)
    assert got[0] is None and got[1:] == want
    # a side stream behind a producer on that stream, the default stream busy
    staged = d[3].clone()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    busy = torch.empty(256 << 20, dtype=torch.uint8, device=dev)
    for _ in range(8):
        busy.fill_(1)
    with torch.cuda.stream(side):
        d[3].zero_()
        d[3].copy_(staged)
    got = run(torch, SCHEMA, d, LISTS["ladder"], spec, 64, stream=side)
    assert np.array_equal(got[0], p.b.want["ladder"]) and got[1:] == want
    torch.cuda.synchronize()
