"""The top-limit matches of a search by one attribute (include/hdxhash.h): what
search_manager::sorted_search (daemon/search_manager.cc:305-502) does with the
objects that pass the checks.

compare             datatype_*::compare(a, b) on the host CPU (hdx_compare).
sorted_search_host  stored objects in numpy arrays, on the host CPU
                    (hdx_sorted_search), any limit.
sorted_search       stored objects in torch HIP tensors, on the GPU
                    (hdx_sorted_search_device), limit <= HDX_SORT_LIMIT_MAX.

Which end is kept and the direction of the output are two arguments, not one
`maximize` flag: the daemon as written is SortSpec(attr, KEEP_SMALLEST,
descending=True) for maximize and SortSpec(attr, KEEP_LARGEST) without it
(INTEGRATION.md).
"""
import ctypes
from typing import Sequence

import numpy as np

from ._lib import check, lib
from ._tensors import check_stored, opt_ptr, ptrs, read_back, stored_host, torch_stream, types_array
from .checks import AttributeCheck, _checks

HDX_SORT_LIMIT_MAX = 1024
KEEP_SMALLEST = 0
KEEP_LARGEST = 1


class _Sort(ctypes.Structure):
    """hdx_sort_spec (include/hdxhash.h)."""
    _fields_ = [("attr", ctypes.c_uint32), ("keep", ctypes.c_uint32), ("descending", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


class SortSpec:
    """The sort attribute (0 = the key; >= len(types): every object ties), which
    end of the order is kept, and the direction of the output."""

    def __init__(self, attr: int, keep: int = KEEP_SMALLEST, descending: bool = False):
        self.attr, self.keep, self.descending = int(attr), int(keep), int(descending)

    def __repr__(self):
        return "SortSpec(%d, %d, %d)" % (self.attr, self.keep, self.descending)

    def _c(self):
        return _Sort(self.attr, self.keep, self.descending, 0)


def sort_finish_block() -> int:
    """Candidates the device form's finishing step takes per round."""
    return int(lib().hdx_sort_finish_block())


def compare(type: int, a: bytes, b: bytes) -> int:
    """datatype_{string,int64,float,timestamp}::compare(a, b): -1, 0 or 1 (a NaN
    on either side: 0)."""
    out = ctypes.c_int(0)
    check(lib().hdx_compare(int(type), bytes(a), len(a), bytes(b), len(b), ctypes.byref(out)))
    return int(out.value)


def sorted_search_host(types, keys, key_off, key_len, vals, val_off, val_len, checks: Sequence[AttributeCheck],
                       sort: SortSpec, limit: int):
    """hdx_sorted_search on numpy arrays (stored objects as in hash_encoded_host):
    returns (top u64[count], status bits)."""
    t = types_array(types)
    *cols, n = stored_host(keys, key_off, key_len, vals, val_off, val_len)
    top = np.empty(max(min(int(limit), n), 1), np.uint64)
    count, status, spec = ctypes.c_uint64(0), ctypes.c_uint32(0), sort._c()
    # arrays without elements still need an address: nothing reads it
    ptr = [x.ctypes.data if x.size else top.ctypes.data for x in cols]
    check(lib().hdx_sorted_search(t.ctypes.data, len(t), *ptr, n, _checks(checks), len(checks), ctypes.byref(spec),
                                  int(limit), top.ctypes.data, ctypes.byref(count), ctypes.byref(status)))
    return top[:int(count.value)], int(status.value)


def sorted_search(types, keys, key_off, key_len, vals, val_off, val_len, checks: Sequence[AttributeCheck],
                  sort: SortSpec, limit: int, want_first_fail=True, status=None, stream=None):
    """hdx_sorted_search_device on torch HIP tensors (stored objects as in
    check_encoded): returns (first_fail i32[n] or None, top i64[count]).
    first_fail is check_encoded's; top holds the kept objects' indices in the
    output order.  The count is read back on `stream`, which is then waited for."""
    t = types_array(types)
    arr = _checks(checks)

    def call(ptrs, n, spec, lim, first_fail, top, count, status_ptr, stream_ptr):
        return lib().hdx_sorted_search_device(t.ctypes.data, len(t), *ptrs, n, arr, len(checks), spec, lim,
                                              first_fail, top, count, status_ptr, stream_ptr)
    return _sorted_search(call, keys, key_off, key_len, vals, val_off, val_len, sort, limit, want_first_fail, status,
                          stream)


def _sorted_search(call, keys, key_off, key_len, vals, val_off, val_len, sort, limit, want_first_fail, status, stream):
    """The tensors around one of the two device forms: call(the six pointers, n, sort, limit,
    first_fail, top, count, status, stream) -> hdx_status."""
    import torch

    n, dev = check_stored(keys, key_off, key_len, vals, val_off, val_len)
    s = torch_stream(stream, dev)
    with torch.cuda.stream(s):
        first_fail = torch.empty(max(n, 1), dtype=torch.int32, device=dev) if want_first_fail else None
        top = torch.empty(max(min(int(limit), HDX_SORT_LIMIT_MAX), 1), dtype=torch.int64, device=dev)
        count = torch.empty(1, dtype=torch.int64, device=dev)
    spec = sort._c()
    check(call(ptrs((keys, key_off, key_len, vals, val_off, val_len), count), n, ctypes.byref(spec), int(limit),
               opt_ptr(first_fail), top.data_ptr(), count.data_ptr(), opt_ptr(status), s.cuda_stream))
    return (first_fail[:n] if want_first_fail else None), top[:read_back(count, s)]
