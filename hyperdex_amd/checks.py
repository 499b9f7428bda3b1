"""A search's attribute checks (common/attribute_check.cc:123-237; the table is
restated in include/hdxhash.h).

passes_checks   one object on the host CPU (hdx_passes_checks):
                passes_attribute_checks' result, the index of the first check
                that fails or len(checks).
check_encoded   a batch of stored objects on the GPU (hdx_check_encoded_device):
                what datalayer::search_iterator::valid() does per candidate
                (daemon/datalayer_iterator.cc:792-850), plus the compacted list
                of the objects that pass.
"""
import ctypes
from typing import Sequence

from ._lib import check, lib
from ._tensors import check_stored, opt_ptr, ptrs, read_back, torch_stream, types_array

HDX_MAX_CHECKS = 16
HDX_CHECK_BYTES_MAX = 1024
HDX_CHECK_BADENC = 0xffffffff


class _Check(ctypes.Structure):
    """hdx_attribute_check (include/hdxhash.h)."""
    _fields_ = [("attr", ctypes.c_uint32), ("datatype", ctypes.c_uint32), ("predicate", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32), ("value", ctypes.c_char_p), ("value_len", ctypes.c_uint64)]


class AttributeCheck:
    """common/attribute_check.h: the schema attribute (0 = the key), the
    check's value and its hyperdatatype, and a HYPERPREDICATE_* value."""

    def __init__(self, attr: int, value: bytes, datatype: int, predicate: int):
        self.attr, self.value, self.datatype, self.predicate = int(attr), bytes(value), int(datatype), int(predicate)

    def __repr__(self):
        return "AttributeCheck(%d, %r, %d, %d)" % (self.attr, self.value, self.datatype, self.predicate)


def _checks(checks: Sequence[AttributeCheck]):
    """The C array; it refers to the checks' own bytes, which `checks` keeps alive."""
    arr = (_Check * max(len(checks), 1))()
    for k, ck in enumerate(checks):
        arr[k].attr, arr[k].datatype, arr[k].predicate = ck.attr, ck.datatype, ck.predicate
        arr[k].value, arr[k].value_len = ck.value, len(ck.value)
    return arr


def check_block_objects() -> int:
    """Objects per workgroup of the check kernel (the compaction scans one count each)."""
    return int(lib().hdx_check_block_objects())


def passes_checks(types, key: bytes, values: Sequence[bytes], checks: Sequence[AttributeCheck]) -> int:
    """passes_attribute_checks(schema, checks, key, value) for one object:
    the index of the first failing check, len(checks) when all pass."""
    t = types_array(types)
    m = len(values)
    ptrs = (ctypes.c_char_p * max(m, 1))(*[bytes(v) for v in values])
    lens = (ctypes.c_size_t * max(m, 1))(*[len(v) for v in values])
    out = ctypes.c_uint32(0)
    check(lib().hdx_passes_checks(t.ctypes.data, len(t), bytes(key), len(key), ptrs, lens, _checks(checks),
                                  len(checks), ctypes.byref(out)))
    return int(out.value)


def check_encoded(types, keys, key_off, key_len, vals, val_off, val_len, checks: Sequence[AttributeCheck],
                  want_match=True, status=None, stream=None):
    """hdx_check_encoded_device on torch HIP tensors (stored objects as in
    hash_encoded): returns (first_fail i32[n], match i64[count] or None).
    first_fail holds u32 bit patterns: 0 .. len(checks), or -1
    (HDX_CHECK_BADENC) for a value that does not decode (status: HDX_E_BADENC's
    bit).  match: the indices with first_fail == len(checks), ascending; with
    want_match the count is read back on `stream`, which is then waited for."""
    t = types_array(types)
    arr = _checks(checks)

    def call(ptrs, n, first_fail, match, count, status_ptr, stream_ptr):
        return lib().hdx_check_encoded_device(t.ctypes.data, len(t), *ptrs, n, arr, len(checks), first_fail, match,
                                              count, status_ptr, stream_ptr)
    return _check_encoded(call, keys, key_off, key_len, vals, val_off, val_len, want_match, status, stream)


def _check_encoded(call, keys, key_off, key_len, vals, val_off, val_len, want_match, status, stream):
    """The tensors around one of the two device forms: call(the six pointers, n, first_fail, match,
    count, status, stream) -> hdx_status."""
    import torch

    n, dev = check_stored(keys, key_off, key_len, vals, val_off, val_len)
    s = torch_stream(stream, dev)
    with torch.cuda.stream(s):
        first_fail = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        match = torch.empty(max(n, 1), dtype=torch.int64, device=dev) if want_match else None
        count = torch.empty(1, dtype=torch.int64, device=dev) if want_match else None
    check(call(ptrs((keys, key_off, key_len, vals, val_off, val_len), first_fail), n, first_fail.data_ptr(),
               opt_ptr(match), opt_ptr(count), opt_ptr(status), s.cuda_stream))
    if not want_match:
        return first_fail[:n], None
    return first_fail[:n], match[:read_back(count, s)]


HDX_REGEX_ITEMS_MAX = 63
HDX_MAX_REGEX_CHECKS = 4


def regex_match(regex: bytes, text: bytes) -> bool:
    """regex_match(regex, text) of common/regex_match.cc on the host CPU
    (hdx_regex_match): linear in len(text) whatever the pattern."""
    out = ctypes.c_int(0)
    check(lib().hdx_regex_match(bytes(regex), len(regex), bytes(text), len(text), ctypes.byref(out)))
    return bool(out.value)


class CompiledChecks:
    """A list of checks compiled once per search (hdx_checks_compile): the one
    form that runs REGEX on a STRING attribute.  Host memory only; usable from
    any thread and on any device.  A context manager; freed on exit, by
    close() or with the object."""

    def __init__(self, types, checks: Sequence[AttributeCheck]):
        self._h = None
        t = types_array(types)
        h = ctypes.c_void_p(None)
        check(lib().hdx_checks_compile(t.ctypes.data, len(t), _checks(checks), len(checks), ctypes.byref(h)))
        self._h = h
        self._free = lib().hdx_checks_free  # still there when __del__ runs at interpreter exit
        self.attrs_sz, self.c = len(t), len(checks)

    def close(self):
        if self._h is not None:
            self._free(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        self.close()

    def _handle(self):
        assert self._h is not None, "the compiled list was freed"
        return self._h

    def passes(self, key: bytes, values: Sequence[bytes]) -> int:
        """As passes_checks: the index of the first failing check, len(checks) when all pass."""
        m = len(values)
        assert m == self.attrs_sz - 1
        ptrs = (ctypes.c_char_p * max(m, 1))(*[bytes(v) for v in values])
        lens = (ctypes.c_size_t * max(m, 1))(*[len(v) for v in values])
        out = ctypes.c_uint32(0)
        check(lib().hdx_checks_passes(self._handle(), bytes(key), len(key), ptrs, lens, ctypes.byref(out)))
        return int(out.value)

    def check_encoded(self, keys, key_off, key_len, vals, val_off, val_len, want_match=True, status=None,
                      stream=None):
        """As check_encoded (hdx_checks_encoded_device): returns what it returns."""
        def call(ptrs, n, first_fail, match, count, status_ptr, stream_ptr):
            return lib().hdx_checks_encoded_device(self._handle(), *ptrs, n, first_fail, match, count, status_ptr,
                                                   stream_ptr)
        return _check_encoded(call, keys, key_off, key_len, vals, val_off, val_len, want_match, status, stream)

    def sorted_search(self, keys, key_off, key_len, vals, val_off, val_len, sort, limit: int, want_first_fail=True,
                      status=None, stream=None):
        """As sorted_search (hdx_checks_sorted_device): returns what it returns."""
        from .sorting import _sorted_search  # sorting imports this module

        def call(ptrs, n, spec, lim, first_fail, top, count, status_ptr, stream_ptr):
            return lib().hdx_checks_sorted_device(self._handle(), *ptrs, n, spec, lim, first_fail, top, count,
                                                  status_ptr, stream_ptr)
        return _sorted_search(call, keys, key_off, key_len, vals, val_off, val_len, sort, limit, want_first_fail,
                              status, stream)
