"""The tensor plumbing the binding modules share: the schema array, the stream
argument, optional pointers, and stored objects — the six columns keys, key_off,
key_len, vals, val_off, val_len of include/hdxhash.h — as torch HIP tensors and
as numpy arrays.  Private: the public functions are the binding modules'.
"""
import numpy as np

_WIDTH = (1, 8, 4, 1, 8, 4)  # bytes per element of keys, key_off, key_len, vals, val_off, val_len
_DTYPE = (np.uint8, np.uint64, np.uint32, np.uint8, np.uint64, np.uint32)
_PER_OBJECT = (1, 2, 4, 5)   # the columns with one element per object


def types_array(types):
    """A schema's hyperdatatypes as the contiguous u32 array the C calls take."""
    return np.ascontiguousarray(np.asarray(types, dtype=np.uint32))


def torch_stream(stream, device):
    """The `stream` argument of the device wrappers as a torch stream: None (torch's current
    stream on `device`), a torch stream, or a raw hipStream_t handle, which .cuda_stream hands
    back unchanged.  Handle 0 is the null stream, torch's default stream: ExternalStream(0)
    would be a new stream instead."""
    import torch
    if stream is None:
        return torch.cuda.current_stream(device)
    if hasattr(stream, "cuda_stream"):
        return stream
    if int(stream) == 0:
        return torch.cuda.default_stream(device)
    return torch.cuda.ExternalStream(int(stream), device=device)


def opt_ptr(t):
    """The address of an optional tensor (None: NULL)."""
    return t.data_ptr() if t is not None else None


def check_stored(keys, key_off, key_len, vals, val_off, val_len):
    """Stored objects on the device: u8 keys / values, u64 offsets, u32 lengths (any dtype of
    that width), contiguous, on one device, n of each per-object column.  None: a column the
    call does not read.  Returns (n, device)."""
    cols = (keys, key_off, key_len, vals, val_off, val_len)
    first = next(cols[k] for k in _PER_OBJECT if cols[k] is not None)
    n, dev = first.numel(), first.device
    for k, x in enumerate(cols):
        if x is None:
            continue
        assert x.is_cuda and x.is_contiguous() and x.device == dev, "contiguous tensors on one device"
        assert x.element_size() == _WIDTH[k], "keys / offsets / lengths must have 1 / 8 / 4-byte elements"
        assert k not in _PER_OBJECT or x.numel() == n, "one offset and one length per object"
    return n, dev


def ptrs(tensors, stand_in):
    """The tensors' addresses.  A tensor without elements has no address, so `stand_in` (an
    output of the call, never empty) stands in for it: nothing reads it then."""
    return [(x if x.numel() else stand_in).data_ptr() for x in tensors]


def read_back(count, s):
    """The one element of the device tensor `count`, read through pinned memory on the torch
    stream `s`, which is waited for."""
    import torch
    with torch.cuda.stream(s):
        host = torch.empty(1, dtype=torch.int64, pin_memory=True)
        host.copy_(count, non_blocking=True)
        s.synchronize()
    return int(host.item())


def stored_host(keys, key_off, key_len, vals, val_off, val_len):
    """Stored objects in host memory as contiguous numpy arrays of the C types, and n.  The
    same array as keys and vals (records [key][value] in one store) stays one buffer; None (a
    column the call may do without) stays None."""
    cols = [keys, key_off, key_len, vals, val_off, val_len]
    out = [None if x is None else np.ascontiguousarray(x, dtype=t) for x, t in zip(cols, _DTYPE)]
    if vals is keys:
        out[3] = out[0]
    n = len(out[5])
    assert all(out[k] is None or len(out[k]) == n for k in _PER_OBJECT), "one offset and one length per object"
    return (*out, n)
