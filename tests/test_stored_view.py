"""Stored objects as one view (StoredObjects, hdx_host_common.h; hyperdex_amd/_tensors.py): every
entry point that takes the six columns keys, key_off, key_len, vals, val_off, val_len refuses a
missing column at the same place among its other refusals, and every Python wrapper takes the same
tensors: empty batches, both store layouts, the stream argument in each of its forms, and tensors of
the wrong shape refused before anything is launched.

REFUSALS pins, per entry point, what comes back when a column is NULL together with one other fault:
the status and the text of hdx_last_error() name the fault that won.  Pointers are stand-in
addresses: a call that is refused dereferences none of them."""
import ctypes
import functools
import struct

import numpy as np
import pytest

import hyperdex_amd as hdx
from hyperdex_amd import _lib, _tensors, datatypes as dt, gather
from hyperdex_amd.checks import AttributeCheck, CompiledChecks
from hyperdex_amd.index import IndexSpec, _specs
from hyperdex_amd.sorting import SortSpec
from test_index_entries import store, to_dev

STRING, INT64 = dt.HYPERDATATYPE_STRING, dt.HYPERDATATYPE_INT64
TYPES = [STRING, STRING, INT64]
COLUMNS = ("keys", "key_off", "key_len", "vals", "val_off", "val_len")
OK, BADTYPE, DEVICE, INVALID = _lib.HDX_OK, _lib.HDX_E_BADTYPE, _lib.HDX_E_DEVICE, _lib.HDX_E_INVALID
NULL_DEV, NULL_HOST, NULL_PTR = "NULL device pointer", "NULL host pointer", "NULL pointer"
BAD_TYPE = "attribute 1: unknown hyperdatatype 1"
BAD_CHECK_TYPE = "types is NULL"
NO_LIST = "the compiled list is NULL"
NO_TABLE = "NULL table 0"
NO_SORT = "sort is NULL"
BAD_WHAT = "what=4 is not HDX_GATHER_KEYS, HDX_GATHER_VALUES or both"
LIMIT = "limit=1025 above 1024"
NO_KEYS, NO_VALS = "HDX_GATHER_KEYS without keys or key_off", "HDX_GATHER_VALUES without vals or val_off"


# ---- the entry points: argument names in order, the columns each reads, its other faults ----------

STORED = list(COLUMNS)
ENTRY_POINTS = {
    "hdx_hash_encoded_device": (["types", "attrs_sz"] + STORED + ["n", "coords", "versions", "status", "stream"],
                                COLUMNS, ("bad_type",)),
    "hdx_hash_encoded_regions_device": (["types", "attrs_sz"] + STORED + ["n", "tables", "ntables", "region_ids",
                                                                        "coords", "versions", "status", "stream"],
                                        COLUMNS, ("bad_type", "no_table")),
    "hdx_hash_encoded_host": (["types", "attrs_sz", "keys", "keys_bytes", "key_off", "key_len", "vals", "vals_bytes",
                               "val_off", "val_len", "n", "coords", "versions"], COLUMNS, ("bad_type",)),
    "hdx_index_entries_plan_device": (["types", "attrs_sz", "key_len", "vals", "val_off", "val_len", "n", "specs", "m",
                                       "attr_off", "attr_len", "entry_off", "status", "stream"],
                                      ("key_len", "vals", "val_off", "val_len"), ("bad_type", "overflow")),
    "hdx_index_entries_fill_device": (["types", "attrs_sz", "keys", "key_off", "key_len", "vals", "val_off", "n",
                                       "specs", "m", "attr_off", "attr_len", "entry_off", "entries", "entries_bytes",
                                       "status", "stream"],
                                      ("keys", "key_off", "key_len", "vals", "val_off"), ("bad_type", "overflow")),
    "hdx_check_encoded_device": (["types", "attrs_sz"] + STORED + ["n", "checks", "c", "first_fail", "match",
                                                                 "match_count", "status", "stream"],
                                 COLUMNS, ("no_types", "no_count")),
    "hdx_checks_encoded_device": (["h"] + STORED + ["n", "first_fail", "match", "match_count", "status", "stream"],
                                  COLUMNS, ("no_list", "no_count")),
    "hdx_sorted_search_device": (["types", "attrs_sz"] + STORED + ["n", "checks", "c", "sort", "limit", "first_fail",
                                                                 "top", "top_count", "status", "stream"],
                                 COLUMNS, ("no_types", "no_sort", "limit")),
    "hdx_checks_sorted_device": (["h"] + STORED + ["n", "sort", "limit", "first_fail", "top", "top_count", "status",
                                                  "stream"], COLUMNS, ("no_list", "no_sort", "limit")),
    "hdx_sorted_search": (["types", "attrs_sz"] + STORED + ["n", "checks", "c", "sort", "limit", "top", "top_count",
                                                          "status"], COLUMNS, ("no_types", "no_sort")),
    "hdx_gather_objects_plan_device": (["key_len", "val_len", "n", "idx", "count_dev", "cap", "what", "rec_off",
                                        "rec_key_len", "status", "stream"], ("key_len", "val_len"),
                                       ("bad_what", "above_2_40")),
    "hdx_gather_objects_fill_device": (STORED + ["n", "idx", "count_dev", "cap", "what", "rec_off", "out", "out_bytes",
                                                 "status", "stream"], COLUMNS, ("bad_what", "above_2_40")),
    "hdx_gather_objects": (STORED + ["n", "idx", "cap", "what", "rec_off", "rec_key_len", "out", "out_bytes", "status"],
                           COLUMNS, ("bad_what", "above_2_40")),
}
# (status, hdx_last_error()) of each entry point with `column` NULL and `fault` (None: the column
# alone), recorded from the library before its entry points were rewritten over StoredObjects.
REFUSALS = {}


def _record(entry, outcomes):
    """outcomes: {fault: outcome or {column: outcome}}; one outcome for every column unless given per column."""
    names, columns, faults = ENTRY_POINTS[entry]
    assert set(outcomes) == set(faults) | {None}
    for fault, by_column in outcomes.items():
        for col in columns:
            REFUSALS[entry, col, fault] = by_column[col] if isinstance(by_column, dict) else by_column


_record("hdx_hash_encoded_device", {"bad_type": (BADTYPE, BAD_TYPE), None: (INVALID, NULL_DEV)})
_record("hdx_hash_encoded_regions_device", {"bad_type": (BADTYPE, BAD_TYPE), "no_table": (INVALID, NO_TABLE),
                                            None: (INVALID, NULL_DEV)})
# the stores themselves may be NULL when they hold no bytes; here they hold one
_record("hdx_hash_encoded_host", {"bad_type": (BADTYPE, BAD_TYPE), None: (INVALID, NULL_HOST)})
for _entry in ("hdx_index_entries_plan_device", "hdx_index_entries_fill_device"):
    _record(_entry, {"bad_type": (BADTYPE, BAD_TYPE), "overflow": (INVALID, NULL_DEV), None: (INVALID, NULL_DEV)})
_record("hdx_check_encoded_device", {"no_types": (INVALID, BAD_CHECK_TYPE), "no_count": (INVALID, NULL_DEV),
                                     None: (INVALID, NULL_DEV)})
_record("hdx_checks_encoded_device", {"no_list": (INVALID, NO_LIST), "no_count": (INVALID, NULL_DEV),
                                      None: (INVALID, NULL_DEV)})
_record("hdx_sorted_search_device", {"no_types": (INVALID, BAD_CHECK_TYPE), "no_sort": (INVALID, NO_SORT),
                                     "limit": (INVALID, LIMIT), None: (INVALID, NULL_DEV)})
_record("hdx_checks_sorted_device", {"no_list": (INVALID, NO_LIST), "no_sort": (INVALID, NO_SORT),
                                     "limit": (INVALID, LIMIT), None: (INVALID, NULL_DEV)})
_record("hdx_sorted_search", {"no_types": (INVALID, BAD_CHECK_TYPE), "no_sort": (INVALID, NO_SORT),
                              None: (INVALID, NULL_PTR)})
_record("hdx_gather_objects_plan_device", {"bad_what": (INVALID, BAD_WHAT), "above_2_40": (INVALID, NULL_PTR),
                                           None: (INVALID, NULL_PTR)})
_BYTES = {"keys": (INVALID, NO_KEYS), "key_off": (INVALID, NO_KEYS), "key_len": (INVALID, NULL_PTR),
          "vals": (INVALID, NO_VALS), "val_off": (INVALID, NO_VALS), "val_len": (INVALID, NULL_PTR)}
for _entry in ("hdx_gather_objects_fill_device", "hdx_gather_objects"):
    _record(_entry, {"bad_what": (INVALID, BAD_WHAT), "above_2_40": _BYTES, None: _BYTES})


class _Sort(ctypes.Structure):
    _fields_ = [("attr", ctypes.c_uint32), ("keep", ctypes.c_uint32), ("descending", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


@pytest.fixture(scope="module")
def arguments():
    """Valid arguments by name (what is read before a refusal is real memory, the rest stand-in
    addresses), and each fault as the arguments it replaces."""
    types = np.array(TYPES, np.uint32)
    bad = np.array([STRING, 1, INT64], np.uint32)
    table = None  # a region table lives on a device: without one only the calls refused before it is read run
    if hdx.lib().hdx_device_count() > 0:
        table = hdx.RegionTable([0], [[0]], [[2 ** 64 - 1]], [7])
    tables = (ctypes.c_void_p * 1)(table.handle.value if table else None)
    specs = _specs([IndexSpec(1, b"i\x05")])
    compiled = CompiledChecks(TYPES, [])
    sort = _Sort(1, 0, 0, 0)
    valid = {name: 4096 * (k + 1) for k, name in enumerate(
        COLUMNS + ("coords", "versions", "region_ids", "attr_off", "attr_len", "entry_off", "entries", "first_fail",
                   "match", "match_count", "top", "top_count", "idx", "rec_off", "rec_key_len", "out"))}
    valid.update(types=types.ctypes.data, attrs_sz=3, n=5, keys_bytes=1, vals_bytes=1, tables=tables, ntables=1,
                 specs=specs, m=1, entries_bytes=1 << 20, checks=None, c=0, h=compiled._handle(),
                 sort=ctypes.addressof(sort), limit=3, count_dev=None, cap=3, what=3, out_bytes=1 << 20, status=None,
                 stream=None)
    faults = {"bad_type": {"types": bad.ctypes.data}, "no_types": {"types": None}, "no_list": {"h": None},
              "no_sort": {"sort": None}, "no_table": {"tables": (ctypes.c_void_p * 1)(None)},
              "bad_what": {"what": 4}, "overflow": {"n": 1 << 60}, "above_2_40": {"n": (1 << 40) + 1},
              "limit": {"limit": 1025}, "no_count": {"match_count": None}, None: {}}
    yield valid, faults, table is not None
    del types, bad, tables, specs, sort
    compiled.close()
    if table:
        table.close()


def _outcome(entry, valid, **over):
    lib = hdx.lib()
    st = getattr(lib, entry)(*[over.get(name, valid[name]) for name in ENTRY_POINTS[entry][0]])
    return st, (lib.hdx_last_error() or b"").decode() if st != OK else ""


@pytest.mark.parametrize("entry", list(ENTRY_POINTS))
def test_a_null_column_keeps_its_place_among_the_refusals(arguments, entry):
    valid, faults, have_table = arguments
    names, columns, others = ENTRY_POINTS[entry]
    for col in columns:
        for fault in others + (None,):
            if "tables" in names and fault is None and not have_table:
                continue  # the table list is read before the columns are looked at
            got = _outcome(entry, valid, **{col: None}, **faults[fault])
            assert got == REFUSALS[entry, col, fault], (col, fault)
    # each other fault alone is refused too, and what is not refused reaches the device binding
    for fault in others:
        assert _outcome(entry, valid, **faults[fault])[0] in (BADTYPE, INVALID), fault
    if "stream" in names and "tables" not in names and hdx.lib().hdx_device_count() == 0:
        assert _outcome(entry, valid)[0] == DEVICE


def test_the_parts_a_gather_does_not_copy_may_be_absent(arguments):
    valid = arguments[0]
    entry = "hdx_gather_objects_fill_device"
    assert _outcome(entry, valid, what=gather.KEYS, keys=None) == (INVALID, NO_KEYS)
    assert _outcome(entry, valid, what=gather.VALUES, val_off=None) == (INVALID, NO_VALS)
    if hdx.lib().hdx_device_count() == 0:
        assert _outcome(entry, valid, what=gather.VALUES, keys=None, key_off=None)[0] == DEVICE
        assert _outcome(entry, valid, what=gather.KEYS, vals=None, val_off=None)[0] == DEVICE


# ---- the wrappers on the device -------------------------------------------------------------------

SPECS = [IndexSpec(1, b"i\x05\x07"), IndexSpec(2, b"i\x02")]
CHECKS = [AttributeCheck(2, struct.pack("<q", -20), INT64, dt.HYPERPREDICATE_GREATER_EQUAL),
          AttributeCheck(1, struct.pack("<q", 9), INT64, dt.HYPERPREDICATE_LENGTH_LESS_EQUAL)]
SORT, LIMIT = SortSpec(2, descending=True), 5
BOTH = gather.KEYS | gather.VALUES
WRAPPERS = ("hash_encoded", "hash_encoded_regions", "index_entries", "check_encoded", "compiled.check_encoded",
            "sorted_search", "compiled.sorted_search", "gather_objects")


def objects(n):
    rng = np.random.default_rng(n)
    return [(rng.bytes(int(rng.integers(1, 10))),
             [rng.bytes(int(rng.integers(0, 13))), struct.pack("<q", int(rng.integers(-50, 51)))]) for _ in range(n)]


@functools.lru_cache(maxsize=None)
def host_forms(n):
    """What each wrapper returns for objects(n), from the host forms; neither store layout changes it."""
    objs = objects(n)
    e = store(objs, len(TYPES))
    coords = np.array([hdx.hash_object(TYPES, k, a) for k, a in objs], np.uint64).reshape(n, len(TYPES))
    first_fail = np.array([hdx.passes_checks(TYPES, k, a, CHECKS) for k, a in objs], np.uint32)
    with CompiledChecks(TYPES, CHECKS) as cc:
        assert [cc.passes(k, a) for k, a in objs] == first_fail.tolist()
    match = np.flatnonzero(first_fail == len(CHECKS)).astype(np.uint64)
    records, rec_off, rec_key_len, bits = hdx.gather_objects_host(*e, match, BOTH)
    assert bits == 0
    return {"coords": coords, "ids": np.where(coords[:, 0] < 2 ** 63, 5, 9).astype(np.uint64),
            "entries": [hdx.index_entry(s, TYPES[0], k, TYPES[s.attr], a[s.attr - 1]) for k, a in objs for s in SPECS],
            "first_fail": first_fail, "match": match, "top": hdx.sorted_search_host(TYPES, *e, CHECKS, SORT, LIMIT)[0],
            "records": records.tobytes(), "rec_off": rec_off, "rec_key_len": rec_key_len}


@pytest.fixture(scope="module")
def gpu():
    import torch
    dev = torch.device("cuda", 0)
    table = hdx.RegionTable([0], [[0], [2 ** 63]], [[2 ** 63 - 1], [2 ** 64 - 1]], [5, 9])
    compiled = CompiledChecks(TYPES, CHECKS)
    yield torch, dev, table, compiled
    compiled.close()
    table.close()


def call(gpu, name, d, idx=None, types=TYPES, specs=SPECS, checks=CHECKS, what=BOTH, **kw):
    """Wrapper `name` over the stored objects d (and idx, gather_objects' list)."""
    torch, dev, table, compiled = gpu
    return {"hash_encoded": lambda: hdx.hash_encoded(types, *d, **kw),
            "hash_encoded_regions": lambda: hdx.hash_encoded_regions(types, *d, [table], **kw),
            "index_entries": lambda: hdx.index_entries(types, *d, specs, **kw),
            "check_encoded": lambda: hdx.check_encoded(types, *d, checks, **kw),
            "compiled.check_encoded": lambda: compiled.check_encoded(*d, **kw),
            "sorted_search": lambda: hdx.sorted_search(types, *d, checks, SORT, LIMIT, **kw),
            "compiled.sorted_search": lambda: compiled.sorted_search(*d, SORT, LIMIT, **kw),
            "gather_objects": lambda: hdx.gather_objects(*d, idx, what=what, **kw)}[name]()


def u(t, dtype=np.uint64):
    return t.cpu().numpy().view(dtype)


@pytest.mark.gpu
def test_gpu_empty_batches(gpu):
    torch, dev, table, compiled = gpu
    d = [torch.empty(0, dtype=t, device=dev) for t in (torch.uint8, torch.int64, torch.int32) * 2]
    idx = torch.empty(0, dtype=torch.int64, device=dev)
    assert tuple(call(gpu, "hash_encoded", d).shape) == (0, len(TYPES))
    assert tuple(call(gpu, "hash_encoded_regions", d).shape) == (1, 0)
    entries, entry_off = call(gpu, "index_entries", d)
    assert entries.numel() == 0 and entry_off.cpu().tolist() == [0]
    for name in ("check_encoded", "compiled.check_encoded", "sorted_search", "compiled.sorted_search"):
        first_fail, found = call(gpu, name, d)
        assert first_fail.numel() == 0 and found.numel() == 0, name
    out, rec_off, rec_key_len = call(gpu, "gather_objects", d, idx)
    assert out.numel() == 0 and rec_off.cpu().tolist() == [0] and rec_key_len.numel() == 0
    # what does not depend on the objects is refused as on any batch
    listed = [STRING, dt.HYPERDATATYPE_LIST_STRING, INT64]
    on_a_list = [AttributeCheck(1, b"", STRING, dt.HYPERPREDICATE_EQUALS)]
    for name, bad, want in (("hash_encoded", {"types": [STRING, 1, INT64]}, BADTYPE),
                            ("hash_encoded_regions", {"types": [STRING, 1, INT64]}, BADTYPE),
                            ("index_entries", {"specs": [IndexSpec(0, b"i")]}, INVALID),
                            ("index_entries", {"types": listed}, BADTYPE),
                            ("check_encoded", {"types": listed, "checks": on_a_list}, BADTYPE),
                            ("check_encoded", {"checks": CHECKS * 9}, INVALID),
                            ("sorted_search", {"types": listed, "checks": on_a_list}, BADTYPE),
                            ("gather_objects", {"what": 4}, INVALID)):
        with pytest.raises(hdx.HdxError) as err:
            call(gpu, name, d, idx, **bad)
        assert err.value.status == want, name
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["current", "torch", "raw", "zero"])
@pytest.mark.parametrize("layout", ["keycol", "records"])
@pytest.mark.parametrize("n", [1, 257])
def test_gpu_layouts_and_streams(gpu, n, layout, how):
    """Every wrapper equals its host form: one object and one past a 256-object workgroup, keys in
    their own column and records [key][value] (vals is keys), on the current stream and on a side
    stream given as a torch stream or as its raw handle, and on raw handle 0."""
    torch, dev, table, compiled = gpu
    want = host_forms(n)
    d = to_dev(torch, dev, store(objects(n), len(TYPES), layout))
    assert (d[3] is d[0]) == (layout == "records")
    idx = torch.from_numpy(want["match"].view(np.int64)).to(dev)
    torch.cuda.synchronize()  # the inputs are in place before another stream reads them
    side = torch.cuda.Stream(dev)
    stream = {"current": None, "torch": side, "raw": side.cuda_stream, "zero": 0}[how]
    assert how in ("current", "torch") or _tensors.torch_stream(stream, dev).cuda_stream == stream
    got = {name: call(gpu, name, d, idx, stream=stream) for name in WRAPPERS}
    if how in ("torch", "raw"):
        side.synchronize()
    else:
        torch.cuda.synchronize()
    assert np.array_equal(u(got["hash_encoded"]), want["coords"])
    assert np.array_equal(u(got["hash_encoded_regions"]), want["ids"].reshape(1, n))
    entries, entry_off = got["index_entries"]
    sizes = [len(x) for x in want["entries"]]
    assert u(entry_off).tolist() == np.concatenate([[0], np.cumsum(sizes)]).tolist()
    assert u(entries, np.uint8).tobytes() == b"".join(want["entries"])
    for name in ("check_encoded", "compiled.check_encoded"):
        assert np.array_equal(u(got[name][0], np.uint32), want["first_fail"]), name
        assert np.array_equal(u(got[name][1]), want["match"]), name
    for name in ("sorted_search", "compiled.sorted_search"):
        assert np.array_equal(u(got[name][0], np.uint32), want["first_fail"]), name
        assert np.array_equal(u(got[name][1]), want["top"]), name
    out, rec_off, rec_key_len = got["gather_objects"]
    assert u(out, np.uint8).tobytes() == want["records"] and np.array_equal(u(rec_off), want["rec_off"])
    assert np.array_equal(u(rec_key_len, np.uint32), want["rec_key_len"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", WRAPPERS)
def test_gpu_tensors_of_the_wrong_shape_are_refused_before_any_launch(gpu, name):
    """key_len with 8-byte elements, and a val_off that is not contiguous: an AssertionError, and
    outputs given to the call keep their 0xA5."""
    torch, dev, table, compiled = gpu
    n = 257
    good = to_dev(torch, dev, store(objects(n), len(TYPES)))
    idx = torch.arange(n, dtype=torch.int64, device=dev)
    wide = list(good)
    wide[2] = good[2].to(torch.int64)
    strided = list(good)
    strided[4] = torch.stack([good[4], good[4]], 1)[:, 0]
    assert not strided[4].is_contiguous() and strided[4].numel() == n
    outputs = {"status": torch.full((1,), 0xA5A5A5A5 - (1 << 32), dtype=torch.int32, device=dev)}
    if name == "hash_encoded":
        outputs["coords"] = torch.full((n, len(TYPES)), 0xA5, dtype=torch.int64, device=dev)
    before = {k: v.clone() for k, v in outputs.items()}
    for d in (wide, strided):
        with pytest.raises(AssertionError):
            call(gpu, name, d, idx, **outputs)
    torch.cuda.synchronize()
    assert all(torch.equal(outputs[k], before[k]) for k in outputs)
