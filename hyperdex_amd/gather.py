"""The objects behind a match or top list, packed back to back (include/hdxhash.h,
hdx_gather_objects_*): what a search sends per item (daemon/search_manager.cc:267-281,
:484-501, :505-560), as stored objects rather than in the wire format.

gather_objects        on the GPU: plan, one read of the total, the allocation, fill.
gather_objects_host   the same contract over numpy arrays on the host CPU.

Record r = [key of idx[r] if KEYS][value of idx[r] if VALUES]; with rec_off and rec_key_len
the output is a stored-object batch again (batch_of), valid input to every *_encoded call.
"""
import numpy as np

from ._lib import HDX_E_NOMEM, check, lib
from ._tensors import check_stored, opt_ptr, ptrs, read_back, stored_host, torch_stream

KEYS = 1
VALUES = 2


def gather_tile_bytes() -> int:
    """Output bytes one wave of the fill owns per step."""
    return int(lib().hdx_gather_tile_bytes())


def gather_objects_plan(key_len, val_len, idx, count=None, what=KEYS | VALUES, status=None, stream=None):
    """hdx_gather_objects_plan_device on torch HIP tensors: idx i64[cap], count a device i64[1]
    or None (all of idx).  Returns (rec_off i64[cap + 1], rec_key_len i32[cap]); rec_off[-1] is
    the total."""
    import torch

    n, dev = check_stored(None, None, key_len, None, None, val_len)
    cap = idx.numel()
    for x in (idx,) + ((count,) if count is not None else ()):
        assert x.is_cuda and x.is_contiguous() and x.element_size() == 8 and x.device == dev
    s = torch_stream(stream, dev)
    with torch.cuda.stream(s):
        rec_off = torch.empty(cap + 1, dtype=torch.int64, device=dev)
        rec_key_len = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
    key_len, val_len, idx = ptrs((key_len, val_len, idx), rec_off)
    check(lib().hdx_gather_objects_plan_device(key_len, val_len, n, idx, opt_ptr(count), cap, what, rec_off.data_ptr(),
                                               rec_key_len.data_ptr(), opt_ptr(status), s.cuda_stream))
    return rec_off, rec_key_len[:cap]


def _fill(entry, keys, key_off, key_len, vals, val_off, val_len, idx, count, what, rec_off, out, status, stream):
    """One of the two fill forms (the product's, or the debug library's record-major baseline)."""
    n, dev = check_stored(keys, key_off, key_len, vals, val_off, val_len)
    cap = idx.numel()
    for x in (idx, rec_off, out):
        assert x.is_cuda and x.is_contiguous()
    assert out.element_size() == 1 and rec_off.numel() == cap + 1
    *cols, idx_ptr, dst = ptrs((keys, key_off, key_len, vals, val_off, val_len, idx, out), rec_off)
    check(entry(*cols, n, idx_ptr, opt_ptr(count), cap, what, rec_off.data_ptr(), dst, out.numel(), opt_ptr(status),
                torch_stream(stream, dev).cuda_stream))
    return out


def gather_objects_fill(keys, key_off, key_len, vals, val_off, val_len, idx, count, what, rec_off, out,
                        status=None, stream=None):
    """hdx_gather_objects_fill_device: writes record r at out[rec_off[r]:] (`out` a contiguous
    uint8 HIP tensor, any alignment); with fewer than rec_off[-1] bytes nothing is written and
    status gets HDX_E_NOMEM's bit."""
    return _fill(lib().hdx_gather_objects_fill_device, keys, key_off, key_len, vals, val_off, val_len, idx, count,
                 what, rec_off, out, status, stream)


def gather_objects(keys, key_off, key_len, vals, val_off, val_len, idx, count=None, what=KEYS | VALUES,
                   status=None, stream=None):
    """The objects idx names (`match` of check_encoded, `top` of sorted_search), packed on the
    device: plan, one read of the total on `stream`, the allocation, fill.  Returns (out
    u8[total], rec_off i64[cap + 1], rec_key_len i32[cap]).  An index >= n gives an empty record
    (status: HDX_E_INVALID's bit)."""
    import torch

    _, dev = check_stored(keys, key_off, key_len, vals, val_off, val_len)
    s = torch_stream(stream, dev)
    rec_off, rec_key_len = gather_objects_plan(key_len, val_len, idx, count, what, status, s)
    total = read_back(rec_off[-1:], s)
    with torch.cuda.stream(s):
        out = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
    gather_objects_fill(keys, key_off, key_len, vals, val_off, val_len, idx, count, what, rec_off, out[:total],
                        status, s)
    return out[:total], rec_off, rec_key_len


def batch_of(out, rec_off, rec_key_len):
    """The gathered records as stored objects (keys, key_off, key_len, vals, val_off, val_len)
    over `out`; torch tensors or numpy arrays."""
    key_off = rec_off[:-1]
    size = rec_off[1:] - key_off
    val_off = key_off + rec_key_len
    val_len = size - rec_key_len
    if hasattr(out, "is_cuda"):
        import torch
        return out, key_off.contiguous(), rec_key_len, out, val_off.contiguous(), val_len.to(torch.int32)
    return out, np.ascontiguousarray(key_off), rec_key_len, out, val_off.astype(np.uint64), val_len.astype(np.uint32)


def gather_objects_host(keys, key_off, key_len, vals, val_off, val_len, idx, what=KEYS | VALUES, out=None):
    """hdx_gather_objects over numpy arrays on the host CPU.  Returns (out u8[total], rec_off
    u64[count + 1], rec_key_len u32[count], status bits).  With `out` given (a uint8 array) the
    records go there; if it is too small nothing is written and the bits hold HDX_E_NOMEM's."""
    *cols, n = stored_host(keys, key_off, key_len, vals, val_off, val_len)
    idx = np.ascontiguousarray(idx, np.uint64)
    count = len(idx)
    rec_off = np.zeros(count + 1, np.uint64)
    rec_key_len = np.zeros(max(count, 1), np.uint32)
    status = np.zeros(1, np.uint32)

    def ptr(x):
        return None if x is None else x.ctypes.data

    def call(buf, room):
        return lib().hdx_gather_objects(*[ptr(x) for x in cols], n, ptr(idx), count, what, ptr(rec_off),
                                        ptr(rec_key_len), ptr(buf), room, ptr(status))
    if out is None:  # sized from the offsets a first call without room leaves
        out = np.zeros(1, np.uint8)
        st = call(out, 0)
        if st == HDX_E_NOMEM:
            status[0] = 0
            out = np.zeros(int(rec_off[-1]), np.uint8)
            st = call(out, len(out))
        check(st)
    else:
        assert out.dtype == np.uint8 and out.flags.c_contiguous
        st = call(out if len(out) else np.zeros(1, np.uint8), len(out))
        if st != HDX_E_NOMEM:
            check(st)
    total = int(rec_off[-1]) if st == 0 else 0
    return out[:total], rec_off, rec_key_len[:count], int(status[0])
