"""Secondary-index keys and search pruning on the GPU.

index_encode   index_encoding_{int64,timestamp,float}::encode
               (daemon/index_int64.cc:76-79, index_timestamp.cc:79-82,
               index_float.cc:75-90) over a column of values in HBM.
search_regions the region test of configuration::lookup_search
               (common/configuration.cc:736-858) for one subspace's table.
"""
import ctypes
from typing import Optional, Sequence, Tuple

import numpy as np

from ._lib import check, lib
from ._tensors import check_stored, opt_ptr, ptrs, read_back, torch_stream, types_array
from .regions import RegionTable


def index_key_size(type_id: int) -> int:
    """8 for INT64/TIMESTAMP_*, 16 for FLOAT, 0 otherwise."""
    return int(lib().hdx_index_key_size(type_id))


def index_encode(type_id: int, blob, off, length, out=None, status=None, stream=None):
    """Index keys of n values (value i = blob[off[i] : off[i] + length[i]]), all
    HIP tensors; returns a (n, key_size) uint8 tensor.  `out`, when given, must
    start at an 8-byte-aligned address (include/hdxhash.h)."""
    import torch

    size = index_key_size(type_id)
    n = off.numel()
    assert length.numel() == n and off.element_size() == 8 and length.element_size() == 4
    for x in (blob, off, length):
        assert x.is_cuda and x.is_contiguous()
    if out is None:
        out = torch.empty((n, max(size, 1)), dtype=torch.uint8, device=off.device)
    assert out.is_cuda and out.is_contiguous() and out.data_ptr() % 8 == 0, \
        "out must be a contiguous device tensor at an 8-byte-aligned address"
    check(lib().hdx_index_encode_device(type_id, blob.data_ptr(), off.data_ptr(), length.data_ptr(), n,
                                        out.data_ptr(), opt_ptr(status),
                                        torch_stream(stream, off.device).cuda_stream))
    return out


class Range(ctypes.Structure):
    """hdx_range: one range of a search after range_searches()
    (common/range.h:40-55): inclusive, start/end optional."""
    _fields_ = [("attr", ctypes.c_uint32), ("type", ctypes.c_uint32),
                ("start", ctypes.c_char_p), ("start_len", ctypes.c_uint64),
                ("end", ctypes.c_char_p), ("end_len", ctypes.c_uint64),
                ("has_start", ctypes.c_uint32), ("has_end", ctypes.c_uint32),
                ("invalid", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


def _ranges(ranges: Sequence[tuple]):
    arr = (Range * max(len(ranges), 1))()
    for k, r in enumerate(ranges):
        attr, t, start, end = r[:4]
        arr[k].attr, arr[k].type = attr, t
        arr[k].has_start, arr[k].has_end = start is not None, end is not None
        arr[k].start, arr[k].start_len = (start or b""), len(start or b"")
        arr[k].end, arr[k].end_len = (end or b""), len(end or b"")
        arr[k].invalid = bool(r[4]) if len(r) > 4 else False
    return arr


def search_regions(table: RegionTable, ranges: Sequence[tuple],
                   has_replicas=None) -> Tuple[np.ndarray, bool]:
    """ranges: [(attr, hyperdatatype, start bytes | None, end bytes | None[, invalid])].
    has_replicas: u8[R] (0 = the region has no replicas and is skipped, as
    configuration.cc:782-785 does) or None (all have).  Returns (include u8[R],
    cleared): include[r] = 0 when region r is skipped or a range rules it out;
    cleared when the reference returns an empty server list."""
    R = len(table.ids)
    include = np.zeros(max(R, 1), np.uint8)
    cleared = ctypes.c_int(0)
    arr = _ranges(ranges)
    rep = None
    if has_replicas is not None:
        rep = np.ascontiguousarray(has_replicas, np.uint8)
        assert rep.size == R, "has_replicas must hold one flag per region"
    check(lib().hdx_search_regions(table.handle, arr, len(ranges), None if rep is None else rep.ctypes.data,
                                   include.ctypes.data, ctypes.byref(cleared)))
    return include[:R], bool(cleared.value)


def search_space(tables: Sequence[RegionTable], ranges: Sequence[tuple],
                 has_replicas=None) -> Tuple[int, np.ndarray, bool]:
    """configuration::lookup_search over a space's subspaces (tables in the
    space's order; hdx_search_space).  has_replicas: None or one u8[R] array
    (or None) per table.  Returns (chosen subspace index or -1, its include
    mask u8[R], cleared)."""
    T = len(tables)
    handles = (ctypes.c_void_p * max(T, 1))(*[t.handle for t in tables])
    rmax = max([len(t.ids) for t in tables] + [1])
    include = np.zeros(rmax, np.uint8)
    reps, keep = None, []
    if has_replicas is not None:
        assert len(has_replicas) == T
        reps = (ctypes.c_void_p * max(T, 1))()
        for i, r in enumerate(has_replicas):
            if r is not None:
                a = np.ascontiguousarray(r, np.uint8)
                assert a.size == len(tables[i].ids), "has_replicas[%d] must hold one flag per region" % i
                keep.append(a)
                reps[i] = a.ctypes.data
    chosen, servers, cleared = ctypes.c_int32(-1), ctypes.c_uint32(0), ctypes.c_int(0)
    arr = _ranges(ranges)
    check(lib().hdx_search_space(handles, T, arr, len(ranges), reps, ctypes.byref(chosen), include.ctypes.data,
                                 ctypes.byref(servers), ctypes.byref(cleared)))
    c = chosen.value
    mask = include[:len(tables[c].ids)] if c >= 0 else include[:0]
    assert c < 0 or int(mask.sum()) == servers.value
    return c, mask, bool(cleared.value)


# ---- secondary-index entries of stored objects (hdx_index_entries_*) ---------

HDX_MAX_INDICES = 32
HDX_INDEX_PREFIX_MAX = 21


class _Spec(ctypes.Structure):
    """hdx_index_spec (include/hdxhash.h)."""
    _fields_ = [("attr", ctypes.c_uint16), ("prefix_len", ctypes.c_uint8),
                ("prefix", ctypes.c_uint8 * HDX_INDEX_PREFIX_MAX)]


class IndexSpec:
    """One index: the schema attribute it is on (1 .. A-1) and its entries'
    prefix 'i' ++ varint(region) ++ varint(index id), which the daemon's own
    index_entry(ri, ii, &scratch, &slice) (daemon/index_primitive.cc:209-230)
    produces; this package never encodes a varint."""

    def __init__(self, attr: int, prefix: bytes):
        self.attr, self.prefix = int(attr), bytes(prefix)

    def c(self) -> _Spec:
        """The C struct; values the struct cannot hold are passed through as
        out-of-range ones, so the library refuses them."""
        s = _Spec()
        s.attr = self.attr if 0 <= self.attr < 65536 else 0
        n = len(self.prefix)
        s.prefix_len = n if n <= HDX_INDEX_PREFIX_MAX else 255
        ctypes.memmove(s.prefix, self.prefix, min(n, HDX_INDEX_PREFIX_MAX))
        return s


def _specs(specs):
    arr = (_Spec * max(len(specs), 1))()
    for k, s in enumerate(specs):
        arr[k] = s.c()
    return arr


def scan_block() -> int:
    return int(lib().hdx_index_scan_block())


def __getattr__(name):  # SCAN_BLOCK: read from the library on first use (it may not be built at import)
    if name == "SCAN_BLOCK":
        return scan_block()
    raise AttributeError(name)


def index_entry(spec: IndexSpec, key_type: int, key: bytes, attr_type: int, value: bytes) -> bytes:
    """One object's entry under one index on the host CPU (hdx_index_entry):
    prefix ++ enc(attr_type, value) ++ enc(key_type, key) [++ u32 BE key size
    when both are STRING], index_primitive::index_entry's bytes."""
    c = spec.c()
    need = ctypes.c_size_t(0)
    cap = len(spec.prefix) + len(value) + len(key) + 40
    out = ctypes.create_string_buffer(cap)
    check(lib().hdx_index_entry(ctypes.byref(c), key_type, key, len(key), attr_type, value, len(value), out, cap,
                                ctypes.byref(need)))
    return out.raw[:need.value]


def index_entries_plan(types, key_len, vals, val_off, val_len, specs, status=None, stream=None):
    """hdx_index_entries_plan_device on torch HIP tensors: returns (attr_off
    i32[n*m], attr_len i32[n*m], entry_off i64[n*m + 1]) — u32 / u64 bit
    patterns; entry_off[-1] is the total size of the entries."""
    import torch

    t = types_array(types)
    n, dev = check_stored(None, None, key_len, vals, val_off, val_len)
    m = len(specs)
    s = torch_stream(stream, dev)
    with torch.cuda.stream(s):
        attr_off = torch.empty(max(n * m, 1), dtype=torch.int32, device=dev)
        attr_len = torch.empty(max(n * m, 1), dtype=torch.int32, device=dev)
        entry_off = torch.empty(n * m + 1, dtype=torch.int64, device=dev)
    # an empty batch is planned (and its types and specs checked) like any other
    check(lib().hdx_index_entries_plan_device(
        t.ctypes.data, len(t), *ptrs((key_len, vals, val_off, val_len), entry_off), n, _specs(specs), m,
        attr_off.data_ptr(), attr_len.data_ptr(), entry_off.data_ptr(), opt_ptr(status), s.cuda_stream))
    return attr_off[:n * m], attr_len[:n * m], entry_off


def index_entries_fill(types, keys, key_off, key_len, vals, val_off, specs, attr_off, attr_len, entry_off,
                       entries, status=None, stream=None):
    """hdx_index_entries_fill_device: writes entry e at entries[entry_off[e]:]
    (`entries` a contiguous uint8 HIP tensor, any alignment); with fewer than
    entry_off[-1] bytes nothing is written and status gets HDX_E_NOMEM's bit."""
    t = types_array(types)
    n, dev = check_stored(keys, key_off, key_len, vals, val_off, None)
    m = len(specs)
    for x in (attr_off, attr_len, entry_off, entries):
        assert x.is_cuda and x.is_contiguous()
    assert entries.element_size() == 1 and entry_off.numel() == n * m + 1
    check(lib().hdx_index_entries_fill_device(
        t.ctypes.data, len(t), *[x.data_ptr() for x in (keys, key_off, key_len, vals, val_off)], n, _specs(specs), m,
        attr_off.data_ptr(), attr_len.data_ptr(), entry_off.data_ptr(), entries.data_ptr(), entries.numel(),
        opt_ptr(status), torch_stream(stream, dev).cuda_stream))
    return entries


def index_entries(types, keys, key_off, key_len, vals, val_off, val_len, specs, status=None, stream=None):
    """Every stored object's entry under every index of `specs`, on the device:
    plan, one read of the total, the allocation, fill — launches and the read
    on `stream` only.  Returns (entries u8[total], entry_off i64[n*m + 1]):
    entry e = i*m + k is entries[entry_off[e] : entry_off[e+1]].  An object
    that does not decode, or whose key or an indexed attribute is a numeric
    of neither 0 nor 8 bytes, has empty entries (status: HDX_E_BADENC /
    HDX_E_BADSIZE bits)."""
    import torch

    n, dev = check_stored(keys, key_off, key_len, vals, val_off, val_len)
    s = torch_stream(stream, dev)
    attr_off, attr_len, entry_off = index_entries_plan(types, key_len, vals, val_off, val_len, specs, status, s)
    if n == 0:  # planned, so types and specs are checked; there is nothing to fill
        return torch.empty(0, dtype=torch.uint8, device=dev), entry_off
    total = read_back(entry_off[-1:], s)
    with torch.cuda.stream(s):
        entries = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
    index_entries_fill(types, keys, key_off, key_len, vals, val_off, specs, attr_off, attr_len, entry_off,
                       entries, status, s)
    return entries[:total], entry_off
