"""Host-resident batches in any order: a chunk whose objects
do not lie back to back is packed in index order — on the device from pinned
memory (hdx_gather.hip), by a host copy per object from pageable memory —
so only the objects' own bytes cross PCIe.  Coordinates against the oracle
and the device-resident path on the same shuffled layout."""
import numpy as np
import pytest

import hyperdex_amd as hdx
from hyperdex_amd import datatypes as dt
from hyperdex_amd import synth

pytestmark = pytest.mark.gpu


def _shuffle(blob, base, lens, A, rng, max_gap=37, lead=5):
    """Every object rewritten at a shuffled position with random gaps."""
    n = len(base)
    sizes = lens.reshape(n, A).astype(np.uint64).sum(axis=1)
    gaps = rng.integers(0, max_gap + 1, n).astype(np.uint64)
    order = rng.permutation(n)
    new_base = np.zeros(n, np.uint64)
    starts = np.cumsum(np.concatenate([[lead], (gaps[order] + sizes[order])[:-1]])).astype(np.uint64)
    starts += gaps[order]
    new_base[order] = starts
    out = np.zeros(int(starts[-1] + sizes[order[-1]]) + 64, np.uint8)
    for k in range(n):  # vectorised enough for a test: one slice per object
        b, s, d = int(base[k]), int(sizes[k]), int(new_base[k])
        out[d:d + s] = blob[b:b + s]
    return out, new_base


def _pinned(torch, a):
    t = torch.empty(a.nbytes, dtype=torch.uint8, pin_memory=True)
    view = t.numpy()
    view[:] = a.view(np.uint8)
    return t, view


@pytest.mark.parametrize("pinned", [True, False])
def test_shuffled_multichunk_batch(oracle, pinned):
    """~250 MB of config-3b objects in shuffled order (two and a half 128 MiB
    chunks, every one packed): equal to the device path and the oracle."""
    import torch
    types, blob, base, lens = synth.make_batch_host("cfg3b", 230_000, seed=31)
    A = len(types)
    rng = np.random.default_rng(5)
    sblob, sbase = _shuffle(blob, base, lens, A, rng)
    keep = None
    if pinned:
        keep, sblob = _pinned(torch, sblob)
    got = hdx.hash_batch_host(types, sblob, sbase, lens)
    idx = np.sort(rng.choice(len(base), 3000, replace=False))
    want, _ = oracle.hash_batch(types, blob, base[idx], lens.reshape(len(base), A)[idx].ravel())
    assert np.array_equal(got[idx], want)
    dev = torch.device("cuda", 0)
    b = torch.from_numpy(np.ascontiguousarray(sblob).copy()).to(dev)
    o = torch.from_numpy(sbase.view(np.int64).copy()).to(dev)
    L = torch.from_numpy(lens.view(np.int32).copy()).to(dev)
    ref = hdx.hash_batch(types, b, o, L).cpu().numpy().view(np.uint64)
    assert np.array_equal(got, ref)
    del keep


@pytest.mark.parametrize("pinned", [True, False])
def test_shuffled_tiny_objects_every_alignment(oracle, pinned):
    """Objects of 0..40 bytes at every source alignment, shuffled with wide
    gaps: the gather's byte-wise edge chunks (extents shorter than a chunk,
    sharing destination chunks with their neighbours)."""
    import torch
    rng = np.random.default_rng(17)
    n = 8000
    types = [dt.HYPERDATATYPE_STRING, dt.HYPERDATATYPE_STRING]
    lens = rng.integers(0, 21, 2 * n).astype(np.uint32)
    lens[::97] = 0
    sizes = lens.reshape(n, 2).sum(axis=1).astype(np.uint64)
    base = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.uint64)
    blob = rng.integers(0, 256, int(sizes.sum()) + 64, dtype=np.uint8)
    sblob, sbase = _shuffle(blob, base, lens, 2, rng, max_gap=200, lead=3)
    keep = None
    if pinned:
        keep, sblob = _pinned(torch, sblob)
    got = hdx.hash_batch_host(types, sblob, sbase, lens)
    want, _ = oracle.hash_batch(types, blob, base, lens)
    assert np.array_equal(got, want)
    del keep


def test_ordered_batch_still_one_span(oracle):
    """Objects back to back (the common case) keep the single span copy; with
    a few gaps (< 1/8 of the payload) too — results identical either way."""
    types, blob, base, lens = synth.make_batch_host("cfg3b", 20_000, seed=2)
    want, _ = oracle.hash_batch(types, blob, base, lens)
    assert np.array_equal(hdx.hash_batch_host(types, blob, base, lens), want)


def _scatter(buf, off, ln, rng, max_gap):
    """Each extent [off, +ln) of buf rewritten at a shuffled place with gaps."""
    n = len(off)
    order = rng.permutation(n)
    gaps = rng.integers(0, max_gap + 1, n).astype(np.uint64)
    new_off = np.zeros(n, np.uint64)
    pos = np.uint64(3)
    for k in order:
        pos += gaps[k]
        new_off[k] = pos
        pos += np.uint64(ln[k])
    out = np.zeros(int(pos) + 16, np.uint8)
    for k in range(n):
        out[int(new_off[k]):int(new_off[k]) + int(ln[k])] = buf[int(off[k]):int(off[k]) + int(ln[k])]
    return out, new_off


def _pinned_np(a):
    import ctypes
    from hyperdex_amd import _lib
    lib = hdx.lib()
    p = ctypes.c_void_p()
    _lib.check(lib.hdx_alloc_pinned(max(a.nbytes, 1), ctypes.byref(p)))
    view = np.frombuffer((ctypes.c_uint8 * max(a.nbytes, 1)).from_address(p.value), dtype=a.dtype, count=a.size)
    view[:] = a
    return view, lambda: lib.hdx_free_pinned(p)


_PIN_CASES = [(kind, blob, lens, coords) for kind in ("span", "packed") for blob in (False, True)
              for lens in (False, True) for coords in (False, True)]
_PIN_CASES += [("stored", store, lens, False) for store in ("keys", "vals") for lens in (False, True)]
_pin_inputs = {}  # kind -> the shuffled inputs and the oracle's outputs, made once


def _pin_case_inputs(oracle, kind):
    if kind not in _pin_inputs:
        types, blob, base, lens = synth.make_batch_host("cfg3b", 97, seed=53)
        rng = np.random.default_rng(29)
        if kind != "stored":  # gaps of ~2 % of the payload: a span; of ~190 %: packed
            sblob, sbase = _shuffle(blob, base, lens, len(types), rng, max_gap=37 if kind == "span" else 4000)
            _pin_inputs[kind] = (types, [sblob, sbase, lens], oracle.hash_batch(types, blob, base, lens)[0])
        else:
            keys, key_off, key_len, vals, val_off, val_len = synth.encode_store_host(types, blob, base, lens,
                                                                                      first_version=11, layout="keycol")
            skeys, nkoff = _scatter(keys, key_off, key_len, rng, 200)
            svals, nvoff = _scatter(vals, val_off, val_len, rng, 3000)
            enc = [skeys, nkoff, key_len, svals, nvoff, val_len]
            want, wver, bad = oracle.hash_encoded(types, *enc)
            assert not bad.any()
            _pin_inputs[kind] = (types, enc, (want, wver))
    return _pin_inputs[kind]


@pytest.mark.parametrize("kind,main,lens,coords", _PIN_CASES,
                         ids=["%s-%s-lens%d-coords%d" % (k, m if k == "stored" else "blob%d" % m, l, c)
                              for k, m, l, c in _PIN_CASES])
def test_each_array_pinned_or_pageable(oracle, kind, main, lens, coords):
    """Which of a call's arrays are pinned, one by one (97 shuffled objects, one
    chunk): every input goes from the caller's pinned array or through pinned
    staging, every output lands in place or through staging.  A packed batch,
    as one span and as a packed chunk (on the device from a pinned blob, by the
    host from a pageable one): the blob, the lengths, the coordinates.  Stored
    objects (a key column, wide gaps: a packed chunk): the keys pinned
    and the values pageable, or the reverse — one pageable store and the host
    packs the chunk — and both length arrays; versions requested."""
    types, arrays, want = _pin_case_inputs(oracle, kind)
    arrays = list(arrays)
    closers = []

    def pin(a):
        view, close = _pinned_np(a)
        closers.append(close)
        return view

    try:
        if kind != "stored":
            if main:
                arrays[0] = pin(arrays[0])
            if lens:
                arrays[2] = pin(arrays[2])
            out = np.zeros(want.size, np.uint64)
            out = (pin(out) if coords else out).reshape(want.shape)
            got = hdx.hash_batch_host(types, *arrays, out=out)
            assert got is out and np.array_equal(got, want)
        else:
            store = 0 if main == "keys" else 3
            arrays[store] = pin(arrays[store])
            if lens:
                arrays[2], arrays[5] = pin(arrays[2]), pin(arrays[5])
            got, vers = hdx.hash_encoded_host(types, *arrays, versions=True)
            assert np.array_equal(got, want[0]) and np.array_equal(vers, want[1])
    finally:
        for c in closers:
            c()


@pytest.mark.parametrize("pinned", [True, False])
@pytest.mark.parametrize("records", [False, True])
def test_shuffled_stores(oracle, pinned, records):
    """Stored objects (the indexer's host arrays) with keys and values at
    shuffled places and wide gaps: every chunk is packed into records [key]
    [value] in index order (two gather extents per object from pinned
    stores); a corrupt value among them fails only itself (HDX_E_BADENC)."""
    from hyperdex_amd import _lib
    types, blob, base, lens = synth.make_batch_host("cfg3b", 6000, seed=41)
    keys, key_off, key_len, vals, val_off, val_len = synth.encode_store_host(types, blob, base, lens,
                                                                              first_version=7, layout="keycol")
    rng = np.random.default_rng(9)
    if records:  # one store: each record's key right before its value, records shuffled
        rec = np.zeros(int(key_len.astype(np.uint64).sum() + val_len.astype(np.uint64).sum()), np.uint8)
        roff = np.zeros(len(key_off), np.uint64)
        at = 0
        for i in range(len(key_off)):
            roff[i] = at
            rec[at:at + int(key_len[i])] = keys[int(key_off[i]):int(key_off[i] + key_len[i])]
            at += int(key_len[i])
            rec[at:at + int(val_len[i])] = vals[int(val_off[i]):int(val_off[i] + val_len[i])]
            at += int(val_len[i])
        store, noff = _scatter(rec, roff, key_len.astype(np.uint64) + val_len, rng, 3000)
        enc = [store, noff, key_len, store, noff + key_len.astype(np.uint64), val_len]
    else:
        skeys, nkoff = _scatter(keys, key_off, key_len, rng, 200)
        svals, nvoff = _scatter(vals, val_off, val_len, rng, 3000)
        enc = [skeys, nkoff, key_len, svals, nvoff, val_len]
    # a corrupt value: its first length prefix claims more than the value holds
    victim = 4321
    vbuf = enc[3]
    p = int(enc[4][victim]) + 10
    vbuf[p:p + 4] = np.frombuffer((0x7fffffff).to_bytes(4, "big"), np.uint8)
    closers = []
    if pinned:
        for idx in ((0,) if records else (0, 3)):
            view, close = _pinned_np(enc[idx])
            closers.append(close)
            enc[idx] = view
        if records:
            enc[3] = enc[0]  # one store: the same pinned buffer
    try:
        want, wver, bad = oracle.hash_encoded(types, *enc)
        assert bad[victim] and bad.sum() == 1
        with pytest.raises(hdx.HdxError) as e:
            hdx.hash_encoded_host(types, *enc, versions=True)
        assert e.value.status == _lib.HDX_E_BADENC
        coords, vers, st, _ = hdx.hash_encoded_host_status(types, *enc)
        assert st == _lib.HDX_E_BADENC
        assert np.array_equal(coords, want) and np.array_equal(vers, wver)
    finally:
        for c in closers:
            c()


@pytest.mark.parametrize("pinned", [True, False])
def test_shuffled_batch_region_ids(oracle, pinned):
    """The regions form of the host batch (hdx_hash_batch_regions_host, the
    ingest path's call) on packed chunks: a key subspace of 64 regions and a
    3-attribute subspace of 4 x 4 x 4, ids equal to the oracle's lookup of the
    oracle's coordinates, with and without coordinates returned."""
    import torch
    from hyperdex_amd import regions
    types, blob, base, lens = synth.make_batch_host("cfg3b", 40_000, seed=23)
    A = len(types)
    rng = np.random.default_rng(12)
    sblob, sbase = _shuffle(blob, base, lens, A, rng, max_gap=1500)
    keep = None
    if pinned:
        keep, sblob = _pinned(torch, sblob)
    want_c, _ = oracle.hash_batch(types, blob, base, lens)
    lo1, up1 = oracle.partition(1, 64)
    lo3, up3 = oracle.partition(3, 64)
    t1 = regions.RegionTable([0], lo1, up1, np.arange(1, len(lo1) + 1, dtype=np.uint64))
    t3 = regions.RegionTable([1, 2, 3], lo3, up3, np.arange(100, 100 + len(lo3), dtype=np.uint64))
    try:
        ids, coords = hdx.hash_batch_regions_host(types, sblob, sbase, lens, [t1, t3], coords=True)
        assert np.array_equal(coords, want_c)
        assert np.array_equal(ids[0], oracle.lookup_region([0], lo1, up1, t1.ids, want_c))
        assert np.array_equal(ids[1], oracle.lookup_region([1, 2, 3], lo3, up3, t3.ids, want_c))
        ids2 = hdx.hash_batch_regions_host(types, sblob, sbase, lens, [t1, t3])
        assert np.array_equal(ids2, ids)
    finally:
        t1.close()
        t3.close()
        del keep


def _giant_batch(rng, n=40, big=600 << 20, at=17):
    """n objects of two strings, object `at` holding a `big`-byte second
    attribute (alone in its host chunk: larger than a packed chunk), the rest
    small; objects written at shuffled places."""
    types = [dt.HYPERDATATYPE_STRING, dt.HYPERDATATYPE_STRING]
    lens = rng.integers(0, 200, 2 * n).astype(np.uint32)
    lens[2 * at + 1] = big
    sizes = lens.reshape(n, 2).sum(axis=1).astype(np.uint64)
    base = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.uint64)
    block = rng.integers(0, 256, 1 << 20, dtype=np.uint8)
    blob = np.tile(block, int(sizes.sum()) // len(block) + 2)[:int(sizes.sum()) + 64].copy()
    blob[:4096] = rng.integers(0, 256, 4096, dtype=np.uint8)
    sblob, sbase = _shuffle(blob, base, lens, 2, rng, max_gap=100)
    return types, blob, base, lens, sblob, sbase


@pytest.mark.parametrize("pinned", [True, False])
def test_giant_object_alone_in_its_chunk(oracle, pinned):
    """An object larger than a packed chunk (600 MB) among small shuffled ones:
    its chunk holds it alone and moves as one span (pinned or pageable), the
    small objects' chunks are packed; every row equal to the oracle's."""
    import torch
    rng = np.random.default_rng(77)
    types, blob, base, lens, sblob, sbase = _giant_batch(rng)
    keep = None
    if pinned:
        keep, sblob = _pinned(torch, sblob)
    got = hdx.hash_batch_host(types, sblob, sbase, lens)
    want, _ = oracle.hash_batch(types, blob, base, lens)
    assert np.array_equal(got, want)
    del keep


@pytest.mark.parametrize("pinned", [True, False])
def test_giant_value_alone_in_its_chunk(oracle, pinned):
    """A stored object whose value is 600 MB, keys in a key column apart from
    the values: its chunk holds it alone and moves as two spans."""
    rng = np.random.default_rng(78)
    types, blob, base, lens, _, _ = _giant_batch(rng)
    keys, key_off, key_len, vals, val_off, val_len = synth.encode_store_host(types, blob, base, lens,
                                                                              first_version=3, layout="keycol")
    enc = [keys, key_off, key_len, vals, val_off, val_len]
    closers = []
    if pinned:
        for idx in (0, 3):
            view, close = _pinned_np(enc[idx])
            closers.append(close)
            enc[idx] = view
    try:
        want, wver, bad = oracle.hash_encoded(types, *enc)
        assert not bad.any()
        coords, vers = hdx.hash_encoded_host(types, *enc, versions=True)
        assert np.array_equal(coords, want) and np.array_equal(vers, wver)
    finally:
        for c in closers:
            c()
