"""The memory contract between a caller and the device entry points.

The other GPU tests check what the kernels compute; these check where they
read and write, against the same CPU oracle and bit for bit:

  1. every output (coordinates, region ids, versions, index keys, the status
     word) is a view inside an arena of sentinels at the lowest alignment the
     ABI allows: a store past either end of the view lands in a sentinel;
  2. blob / keys / vals start at odd addresses (the loaders take alignment
     from absolute addresses, and only the offset part had ever varied);
  3. obj_base / val_off / key_off / off run across 2^32 inside one
     allocation of 4 GiB + 32 MiB whose surroundings hold other bytes, so an
     offset cut to 32 bits reads wrong bytes from mapped memory;
  4. the entries that issue several launches run on a side stream behind a
     long producer and are waited for on that stream alone;
  5. PointLeaders checks its status word and runs its abort check on the
     caller's stream;
  6. index keys go to an 8-byte-aligned `out`, and a misaligned one is
     rejected before any launch.

Each case asserts the kernel form it reaches (hashing.kernel_for; forms the
policy picks by size alone are forced through the debug library).  Shapes are
the smallest that leave a last wave partial and n * A odd where possible:

  hash_batch            cfg1 65 -> 12; cfg3a 65 -> 20, 25 (forced); cfg2 65 ->
                        21; mixed 65 -> 46; cfg3b 1, 7, 8, 65 -> 212 (7 objects
                        per wave); strings/int64/float at A = 129, n = 9 -> 44;
                        at A = 257, n = 9 -> 300
  hash_encoded          cfg3b x {columns, keycol, records} at 1, 7, 8, 65 -> the
                        product sweep, NUM2; mixed x {keycol, records} at 65 ->
                        its round-5 form; A = 129, n = 9 -> the wide sweep
  hash_batch_regions    cfg3a, cfg1 (policy 12 at this size), cfg2 (21), mixed
                        (46), cfg3b (212) at 65, coords NULL and given; cfg3b
                        65 under debug 235 -> hash + lookups through pool
                        scratch.  The fused form of policies 20 / 25 starts at
                        32 M slots and is not reached at these sizes.
  hash_encoded_regions  cfg3b 65 -> the gather sweep's fused form
  lookup_region         an indexed (R = 64) and a scanned (R = 300) table, 1, 65
  index_encode          INT64, FLOAT, TIMESTAMP_SECOND at 1, 255, 257
"""
import contextlib
import ctypes
import functools

import numpy as np
import pytest

import hyperdex_amd as hdx
from hyperdex_amd import RegionTable, _lib, regions, synth
from hyperdex_amd import datatypes as dt

pytestmark = pytest.mark.gpu

MiB = 1 << 20
TWO32 = 1 << 32
MARGIN = 16 * MiB      # before and after the arena's 4 GiB
MAX_BATCH = 8 * MiB    # a placed batch: a 32-bit cut of its offsets stays inside the arena
GUARD = 512            # sentinel elements on each side of a guarded view
PATTERN = {1: 0xA5, 4: 0xA5A5A5A5 - (1 << 32), 8: 0xA5A5A5A5A5A5A5A5 - (1 << 64)}
BADSIZE, BADENC = 1 << _lib.HDX_E_BADSIZE, 1 << _lib.HDX_E_BADENC
INT64, FLOAT, TS_SECOND = dt.HYPERDATATYPE_INT64, dt.HYPERDATATYPE_FLOAT, dt.TIMESTAMPS[0]


# ---- helpers -------------------------------------------------------------------

def guarded(torch, dev, numel, dtype, skew):
    """(arena, view): `view` is numel elements of a 1-D arena that holds GUARD
    sentinel elements before view[-skew] and GUARD after the view's end; skew
    picks the view's alignment (skew 1 on 8-byte elements: 8- but not
    16-byte aligned)."""
    arena = torch.empty(GUARD + skew + numel + GUARD, dtype=dtype, device=dev)
    arena.fill_(PATTERN[arena.element_size()])
    view = arena[GUARD + skew:GUARD + skew + numel]
    assert arena.data_ptr() % 16 == 0 and view.is_contiguous()
    return arena, view


def assert_guards_intact(arena, view):
    """Both sentinel bands still hold the pattern (call after synchronising);
    reports the first clobbered index relative to the view."""
    size = arena.element_size()
    first = (view.data_ptr() - arena.data_ptr()) // size
    host = arena.cpu().numpy()
    bad = np.nonzero(host != host.dtype.type(PATTERN[size]))[0]
    bad = bad[(bad < first) | (bad >= first + view.numel())]
    assert bad.size == 0, "store outside the output: first at view index %d (view holds %d elements), %d in all" % (
        int(bad[0]) - first, view.numel(), bad.size)


def shifted(torch, dev, host_bytes, shift):
    """A device uint8 view of host_bytes whose data_ptr() % 16 == shift."""
    host_bytes = np.ascontiguousarray(host_bytes, np.uint8)
    buf = torch.zeros(shift + max(len(host_bytes), 1), dtype=torch.uint8, device=dev)
    view = buf[shift:shift + max(len(host_bytes), 1)]
    if len(host_bytes):
        view[:len(host_bytes)].copy_(torch.from_numpy(host_bytes.copy()))
    assert view.data_ptr() % 16 == shift
    return view


def to_dev(torch, dev, a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    if a.size == 0:
        a = np.zeros(1, a.dtype)
    return torch.from_numpy(a.copy()).to(dev)


def u64(t):
    return t.cpu().numpy().view(np.uint64)


class HighArena:
    """One uint8 allocation of 16 MiB + 4 GiB + 16 MiB.  view = arena[16 MiB:],
    so view offset 2^32 lies 16 MiB before the arena's end.  place() copies a
    batch to view[2^32 - S // 2:]: its middle object straddles 2^32.  The
    16 MiB before the view and the view's first 16 MiB hold seeded random
    bytes: an offset cut to 32 bits (zero- or sign-extended) reads those."""

    def __init__(self, torch, dev):
        self.torch, self.dev = torch, dev
        self.arena = torch.empty(MARGIN + TWO32 + MARGIN, dtype=torch.uint8, device=dev)
        self.view = self.arena[MARGIN:]
        self.dirty = True

    def decoys(self):
        if self.dirty:
            g = self.torch.Generator(device=self.dev)
            g.manual_seed(0x5eed)
            self.arena[:2 * MARGIN].copy_(self.torch.randint(0, 256, (2 * MARGIN,), dtype=self.torch.uint8,
                                                             device=self.dev, generator=g))
            self.dirty = False

    def shift_for(self, nbytes):
        assert 0 < nbytes <= MAX_BATCH
        return TWO32 - nbytes // 2

    def place(self, host_bytes):
        """Copy the batch in (one copy) and return the offset to add to its
        compact offsets."""
        self.decoys()
        host_bytes = np.ascontiguousarray(host_bytes, np.uint8)
        shift = self.shift_for(len(host_bytes))
        self.view[shift:shift + len(host_bytes)].copy_(self.torch.from_numpy(host_bytes.copy()))
        return shift

    def behind_producer(self, stream, host_bytes, at=None):
        """On `stream`: zero the whole arena (a long producer), then copy the
        batch in (at view offset `at`, default shift_for's).  The caller
        launches on `stream` right after: a launch that escapes to another
        stream reads zeros."""
        torch = self.torch
        host_bytes = np.ascontiguousarray(host_bytes, np.uint8)
        staged = torch.from_numpy(host_bytes.copy()).to(self.dev)
        at = self.shift_for(len(host_bytes)) if at is None else at
        torch.cuda.synchronize()
        self.dirty = True
        staged.record_stream(stream)
        with torch.cuda.stream(stream):
            self.arena.fill_(0)
            self.view[at:at + len(host_bytes)].copy_(staged)


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available()
    return torch, torch.device("cuda", 0)


@pytest.fixture(scope="module")
def high_arena(torch_dev):
    torch, dev = torch_dev
    h = HighArena(torch, dev)
    yield h
    h.view = h.arena = None
    torch.cuda.empty_cache()


def straddles(start, size):
    """At least one object starts below 2^32 and ends above it, and at least
    one starts above it."""
    start = np.asarray(start, np.uint64).astype(object)
    end = start + np.asarray(size, np.uint64).astype(object)
    return bool(((start < TWO32) & (end > TWO32)).any()) and bool((start > TWO32).any())


def variant_ctx(v):
    return _lib.debug_library(v) if v is not None else contextlib.nullcontext()


# ---- the batches (built and hashed by the oracle once, then left unchanged) ------

# strings of three length ranges, int64 and float: fewer numerics than strings, so the policy takes the
# mixed-strings branch (44 above 128 attributes, the wide kernel above 256), not the numeric one (21)
WIDE_KINDS = [synth.Rule(dt.HYPERDATATYPE_STRING, synth.UNIFORM, 0, 150), synth.Rule(INT64, synth.NUMERIC, 8, 8),
              synth.Rule(dt.HYPERDATATYPE_STRING, synth.UNIFORM, 0, 40), synth.Rule(FLOAT, synth.NUMERIC, 8, 8),
              synth.Rule(dt.HYPERDATATYPE_STRING, synth.UNIFORM, 60, 200)]
RULES = {name: synth.CONFIGS[name] for name in ("cfg1", "cfg2", "cfg3a", "cfg3b", "mixed")}
RULES["a129"] = [WIDE_KINDS[j % 5] for j in range(129)]
RULES["a257"] = [WIDE_KINDS[j % 5] for j in range(257)]

_ORACLE = []


@pytest.fixture(scope="module", autouse=True)
def _the_oracle(oracle):
    _ORACLE.append(oracle)
    yield
    _ORACLE.clear()
    packed.cache_clear()
    stored.cache_clear()


class Packed:
    def __init__(self, name, n, types, blob, base, lens):
        self.name, self.n, self.A = name, n, len(types)
        self.types, self.blob, self.base, self.lens = types, blob, base, lens
        self.sizes = lens.reshape(n, self.A).astype(np.uint64).sum(axis=1)
        self.want, self.err = _ORACLE[0].hash_batch(types, blob, base, lens)


@functools.lru_cache(maxsize=None)
def packed(name, n, bad=False):
    """The packed synthetic batch `name` of n objects and the oracle's
    coordinates.  bad: the last object's middle numeric is 5 bytes long (its
    later attributes follow it 3 bytes earlier; the oracle reads the same)."""
    types, blob, base, lens = synth.make_batch_host(RULES[name], n, seed=1000 + n)
    if bad:
        A = len(types)
        numeric = [j for j in range(A) if RULES[name][j].kind == synth.NUMERIC]
        victim = (n - 1) * A + numeric[len(numeric) // 2]
        lens = lens.copy()
        lens[victim] = 5
        p = Packed(name, n, types, blob, base, lens)
        p.victim = victim
        assert p.err == _lib.HDX_E_BADSIZE and p.want.reshape(-1)[victim] == 0
        return p
    p = Packed(name, n, types, blob, base, lens)
    assert p.err == 0
    return p


class Stored:
    pass


@functools.lru_cache(maxsize=None)
def stored(name, n, layout, fault=None):
    """The same batch as stored objects (synth's three layouts) and the
    oracle's coordinates and versions.  fault "size": packed(..., bad=True);
    "corrupt": the last object's attribute count is wrong."""
    p = packed(name, n, fault == "size")
    if layout == "columns":
        enc = synth.encode_values_host(p.types, p.blob, p.base, p.lens, first_version=7)
    else:
        enc = synth.encode_store_host(p.types, p.blob, p.base, p.lens, first_version=7, layout=layout)
    keys, key_off, key_len, vals, val_off, val_len = [np.array(x) for x in enc]
    if fault == "corrupt":
        vals[int(val_off[n - 1]) + 9] ^= 1
    s = Stored()
    s.records = layout == "records"
    if s.records:
        keys = vals
    s.p, s.n, s.A, s.types = p, n, p.A, p.types
    s.enc = (keys, key_off, key_len, vals, val_off, val_len)
    if fault == "size":
        # the oracle's decoder refuses a mis-sized numeric outright; its hash_batch gives that value 0
        # and hashes the rest, which is what the sweep does with the same attributes once decoded
        s.want, s.versions, s.bad = p.want, np.uint64(7) + np.arange(n, dtype=np.uint64), np.zeros(n, bool)
    else:
        s.want, s.versions, s.bad = _ORACLE[0].hash_encoded(p.types, *s.enc)
    assert list(np.nonzero(s.bad)[0]) == ([n - 1] if fault == "corrupt" else [])
    return s


def tables_for(A, want_coords):
    """Two tables: the key grid (64 regions: indexed) and 300 random boxes over
    the last attribute and the key (scanned); (tables, ids (2, n) wanted)."""
    oracle = _ORACLE[0]
    rng = np.random.default_rng(A)
    lo1, up1 = oracle.partition(1, 64)
    a = rng.integers(0, 2**64, size=(300, 2), dtype=np.uint64)
    b = rng.integers(0, 2**64, size=(300, 2), dtype=np.uint64)
    specs = [([0], lo1, up1), ([A - 1, 0], np.minimum(a, b), np.maximum(a, b))]
    ids = [np.arange(1, len(lo) + 1, dtype=np.uint64) * 3 for _, lo, _ in specs]
    tables = [RegionTable(at, lo, up, i) for (at, lo, up), i in zip(specs, ids)]
    want = np.stack([oracle.lookup_region(at, lo, up, i, want_coords) for (at, lo, up), i in zip(specs, ids)])
    return tables, want


# ---- one runner per entry point: guarded outputs, optional side stream ------------

class Run:
    """Allocates every output inside sentinels, calls the entry point, waits
    (for `stream` alone when given) and checks the sentinels.  `before`, when
    given, is called once the outputs are ready (the device idle) and right
    before the entry: it enqueues the input's producer on `stream`."""

    def __init__(self, torch, dev, stream=None, before=None):
        self.torch, self.dev, self.stream, self.before = torch, dev, stream, before
        self.arenas = []

    def ready(self):
        if self.before is not None:
            self.torch.cuda.synchronize()
            self.before()

    def out(self, numel, dtype=None, skew=1, zero=False):
        arena, view = guarded(self.torch, self.dev, numel, dtype or self.torch.int64, skew)
        if zero:
            view.zero_()
        self.arenas.append((arena, view))
        return view

    def status(self):
        return self.out(1, self.torch.int32, 1, zero=True)

    def handle(self):
        s = self.stream if self.stream is not None else self.torch.cuda.current_stream(self.dev)
        return s.cuda_stream

    def finish(self):
        if self.stream is not None:
            self.stream.synchronize()
        else:
            self.torch.cuda.synchronize()
        for arena, view in self.arenas:
            assert_guards_intact(arena, view)

    def hash_batch(self, types, blob, base, lens):
        n, A = base.numel(), len(types)
        coords, status = self.out(n * A), self.status()
        self.ready()
        hdx.hash_batch(types, blob, base, lens, coords=coords.view(n, A), status=status, stream=self.stream)
        self.finish()
        return u64(coords).reshape(n, A), int(status.item())

    def hash_encoded(self, types, enc):
        n, A = enc[4].numel(), len(types)
        coords, versions, status = self.out(n * A), self.out(n), self.status()
        self.ready()
        hdx.hash_encoded(types, *enc, coords=coords.view(n, A), versions=versions, status=status,
                         stream=self.stream)
        self.finish()
        return u64(coords).reshape(n, A), u64(versions), int(status.item())

    def batch_regions(self, types, blob, base, lens, tables, with_coords):
        """hdx_hash_batch_regions_device through the C-ABI (the Python wrapper
        allocates the ids itself)."""
        n, A, T = base.numel(), len(types), len(tables)
        t = np.ascontiguousarray(types, np.uint32)
        ids, status = self.out(T * n), self.status()
        coords = self.out(n * A) if with_coords else None
        handles = (ctypes.c_void_p * T)(*[tb.handle.value for tb in tables])
        self.ready()
        _lib.check(hdx.lib().hdx_hash_batch_regions_device(
            t.ctypes.data, A, blob.data_ptr(), base.data_ptr(), lens.data_ptr(), n, handles, T, ids.data_ptr(),
            coords.data_ptr() if with_coords else None, status.data_ptr(), self.handle()))
        self.finish()
        return u64(ids).reshape(T, n), u64(coords).reshape(n, A) if with_coords else None, int(status.item())

    def encoded_regions(self, types, enc, tables, with_coords):
        """hdx_hash_encoded_regions_device through the C-ABI."""
        n, A, T = enc[4].numel(), len(types), len(tables)
        t = np.ascontiguousarray(types, np.uint32)
        ids, versions, status = self.out(T * n), self.out(n), self.status()
        coords = self.out(n * A) if with_coords else None
        handles = (ctypes.c_void_p * T)(*[tb.handle.value for tb in tables])
        keys, key_off, key_len, vals, val_off, val_len = enc
        self.ready()
        _lib.check(hdx.lib().hdx_hash_encoded_regions_device(
            t.ctypes.data, A, keys.data_ptr(), key_off.data_ptr(), key_len.data_ptr(), vals.data_ptr(),
            val_off.data_ptr(), val_len.data_ptr(), n, handles, T, ids.data_ptr(),
            coords.data_ptr() if with_coords else None, versions.data_ptr(), status.data_ptr(), self.handle()))
        self.finish()
        return (u64(ids).reshape(T, n), u64(coords).reshape(n, A) if with_coords else None, u64(versions),
                int(status.item()))

    def lookup(self, table, coords):
        ids = self.out(coords.shape[0])
        self.ready()
        regions.lookup_region(table, coords, out=ids, stream=self.stream)
        self.finish()
        return u64(ids)

    def index_encode(self, t, blob, off, lens):
        """Keys into a view that is 8- but not 16-byte aligned."""
        size = hdx.index_key_size(t)
        out, status = self.out(off.numel() * size, self.torch.uint8, 8), self.status()
        assert out.data_ptr() % 16 == 8
        self.ready()
        hdx.index_encode(t, blob, off, lens, out=out, status=status, stream=self.stream)
        self.finish()
        return out.cpu().numpy().tobytes(), int(status.item())


def dev_packed(torch, dev, p):
    return to_dev(torch, dev, p.blob), to_dev(torch, dev, p.base), to_dev(torch, dev, p.lens)


def dev_stored(torch, dev, s):
    d = [to_dev(torch, dev, x) for x in s.enc]
    if s.records:
        d[3] = d[0]  # one store: the product takes the records form only when keys == vals
    return d


# ---- the form matrix ---------------------------------------------------------------

# (batch, n, debug variant or None, the form kernel_for names)
BATCH_ROWS = [("cfg1", 65, None, 12), ("cfg3a", 65, 20, 20), ("cfg3a", 65, 25, 25), ("cfg2", 65, None, 21),
              ("mixed", 65, None, 46), ("cfg3b", 1, None, 212), ("cfg3b", 7, None, 212), ("cfg3b", 8, None, 212),
              ("cfg3b", 65, None, 212), ("a129", 9, None, 44), ("a257", 9, None, 300)]
# (batch, n, layout, the batch policy's form for the schema: 212 = strings + int64 / float (the sweep's
# NUM2 form), 46 = other types too (its round-5 form), 44 = more than 128 attributes (the wide sweep))
SWEEP_ROWS = ([("cfg3b", n, layout, 212) for layout in ("columns", "keycol", "records") for n in (1, 7, 8, 65)]
              + [("mixed", 65, "keycol", 46), ("mixed", 65, "records", 46), ("a129", 9, "columns", 44)])
# (batch, n, debug variant, the batch policy's form, which picks the fused form)
REGION_ROWS = [("cfg3a", 65, None, 12), ("cfg2", 65, None, 21), ("cfg1", 65, None, 12), ("mixed", 65, None, 46),
               ("cfg3b", 65, None, 212), ("cfg3b", 65, 235, 212)]
INDEX_ROWS = [(t, n) for t in (INT64, FLOAT, TS_SECOND) for n in (1, 255, 257)]


def row_id(row):
    return "-".join(str(x) for x in row if x is not None)


def check_form(p, variant, form):
    """The policy's form outside the debug library, the forced one inside."""
    assert hdx.hashing.kernel_for(p.types, p.n)[0] == form or variant == form
    if variant is not None:
        with _lib.debug_library(variant):
            assert hdx.hashing.kernel_for(p.types, p.n)[0] == variant


@functools.lru_cache(maxsize=None)
def index_column(t, n):
    """n values of type t (a few of them empty) at odd offsets with gaps:
    (blob, off, len, the oracle's keys)."""
    rng = np.random.default_rng(t * 1000 + n)
    vals = [b"" if rng.random() < 0.1 else rng.bytes(8) for _ in range(n)]
    blob, off = bytearray(), np.zeros(n, np.uint64)
    for i, v in enumerate(vals):
        blob += bytes(1 + 2 * int(rng.integers(0, 3)) if len(blob) % 2 == 0 else 2 * int(rng.integers(0, 3)))
        off[i] = len(blob)
        blob += v
    blob += bytes((-len(blob)) % 4)
    assert (off % 2 == 1).all() and len(blob) % 4 == 0
    want = b"".join(_ORACLE[0].index_encode(t, v)[0] for v in vals)
    return np.frombuffer(bytes(blob), np.uint8), off, np.array([len(v) for v in vals], np.uint32), want


def lookup_case(R, n):
    oracle = _ORACLE[0]
    rng = np.random.default_rng(R + n)
    A = 5
    if R == 64:
        attrs = [3]
        lo, up = oracle.partition(1, 64)
    else:
        attrs = [4, 1]
        a = rng.integers(0, 2**64, size=(R, 2), dtype=np.uint64)
        b = rng.integers(0, 2**64, size=(R, 2), dtype=np.uint64)
        lo, up = np.minimum(a, b), np.maximum(a, b)
    ids = rng.integers(1, 2**63, R, dtype=np.uint64)
    coords = rng.integers(0, 2**64, size=(n, A), dtype=np.uint64)
    coords[0, attrs[0]] = lo[R // 2, 0]
    return attrs, lo, up, ids, coords, oracle.lookup_region(attrs, lo, up, ids, coords)


# ---- 1. guard bands on every output ----------------------------------------------------

@pytest.mark.parametrize("row", BATCH_ROWS, ids=row_id)
def test_guards_hash_batch(torch_dev, row):
    torch, dev = torch_dev
    name, n, variant, form = row
    p = packed(name, n)
    check_form(p, variant, form)
    with variant_ctx(variant):
        got, status = Run(torch, dev).hash_batch(p.types, *dev_packed(torch, dev, p))
    assert np.array_equal(got, p.want) and status == 0


@pytest.mark.parametrize("name,form", [("cfg2", 21), ("cfg3b", 212)])
def test_guards_hash_batch_bad_size_in_the_last_object(torch_dev, name, form):
    """A 5-byte numeric in the last object: the status atomic and that slot's
    zero run next to the buffer's end; every coordinate is the oracle's."""
    torch, dev = torch_dev
    p = packed(name, 65, True)
    check_form(p, None, form)
    got, status = Run(torch, dev).hash_batch(p.types, *dev_packed(torch, dev, p))
    assert status == BADSIZE and got.reshape(-1)[p.victim] == 0
    assert np.array_equal(got, p.want)


@pytest.mark.parametrize("row", SWEEP_ROWS, ids=row_id)
def test_guards_hash_encoded(torch_dev, row):
    torch, dev = torch_dev
    name, n, layout, form = row
    s = stored(name, n, layout)
    check_form(s.p, None, form)
    got, versions, status = Run(torch, dev).hash_encoded(s.types, dev_stored(torch, dev, s))
    assert np.array_equal(got, s.want) and np.array_equal(versions, s.versions) and status == 0


@pytest.mark.parametrize("layout", ["columns", "keycol", "records"])
@pytest.mark.parametrize("fault", ["size", "corrupt"])
def test_guards_hash_encoded_faulty_last_object(torch_dev, layout, fault):
    """The last stored object holds a 5-byte numeric (that coordinate 0,
    HDX_E_BADSIZE) or does not decode (the whole object 0, version 0,
    HDX_E_BADENC): the zeros and the status atomic at the outputs' end."""
    torch, dev = torch_dev
    s = stored("cfg3b", 65, layout, fault)
    check_form(s.p, None, 212)
    got, versions, status = Run(torch, dev).hash_encoded(s.types, dev_stored(torch, dev, s))
    assert status == (BADSIZE if fault == "size" else BADENC)
    if fault == "size":
        assert got.reshape(-1)[s.p.victim] == 0
    else:
        assert not got[-1].any() and versions[-1] == 0
    assert np.array_equal(got, s.want) and np.array_equal(versions, s.versions)


@pytest.mark.parametrize("with_coords", [False, True], ids=["ids", "ids+coords"])
@pytest.mark.parametrize("row", REGION_ROWS, ids=row_id)
def test_guards_hash_batch_regions(torch_dev, row, with_coords):
    torch, dev = torch_dev
    name, n, variant, form = row
    p = packed(name, n)
    check_form(p, None, form)
    tables, want_ids = tables_for(p.A, p.want)
    try:
        with variant_ctx(variant):
            ids, coords, status = Run(torch, dev).batch_regions(p.types, *dev_packed(torch, dev, p), tables,
                                                                with_coords)
    finally:
        for t in tables:
            t.close()
    assert np.array_equal(ids, want_ids) and status == 0
    if with_coords:
        assert np.array_equal(coords, p.want)


@pytest.mark.parametrize("with_coords", [False, True], ids=["ids", "ids+coords"])
def test_guards_hash_encoded_regions(torch_dev, with_coords):
    """Below 2^20 objects the regions sweep is the gather sweep's fused form."""
    torch, dev = torch_dev
    s = stored("cfg3b", 65, "columns")
    check_form(s.p, None, 212)
    tables, want_ids = tables_for(s.A, s.want)
    try:
        ids, coords, versions, status = Run(torch, dev).encoded_regions(s.types, dev_stored(torch, dev, s), tables,
                                                                        with_coords)
    finally:
        for t in tables:
            t.close()
    assert np.array_equal(ids, want_ids) and np.array_equal(versions, s.versions) and status == 0
    if with_coords:
        assert np.array_equal(coords, s.want)


@pytest.mark.parametrize("n", [1, 65])
@pytest.mark.parametrize("R", [64, 300], ids=["indexed", "scanned"])
def test_guards_lookup_region(torch_dev, R, n):
    torch, dev = torch_dev
    attrs, lo, up, ids, coords, want = lookup_case(R, n)
    t = RegionTable(attrs, lo, up, ids)
    try:
        got = Run(torch, dev).lookup(t, to_dev(torch, dev, coords))
    finally:
        t.close()
    assert np.array_equal(got, want)


@pytest.mark.parametrize("t,n", INDEX_ROWS)
def test_guards_index_encode(torch_dev, t, n):
    torch, dev = torch_dev
    blob, off, lens, want = index_column(t, n)
    got, status = Run(torch, dev).index_encode(t, *[to_dev(torch, dev, x) for x in (blob, off, lens)])
    assert got == want and status == 0


# ---- 2. input base pointers at odd addresses ---------------------------------------------

SHIFTS = (1, 7, 13)


@pytest.mark.parametrize("row", BATCH_ROWS, ids=row_id)
def test_odd_blob_address_hash_batch(torch_dev, row):
    """blob itself at 1, 7 and 13 bytes past a 16-byte boundary, offsets
    unchanged.  The synthetic batches are back to back from byte 0 of blob,
    so the wave-staged span copy's lead comes from the pointer alone; the
    config-3b rows also run with 3 bytes before the first object."""
    torch, dev = torch_dev
    name, n, variant, form = row
    p = packed(name, n)
    check_form(p, variant, form)
    assert p.base[0] == 0 and np.array_equal(p.base[1:], np.cumsum(p.sizes)[:-1])
    base, lens = to_dev(torch, dev, p.base), to_dev(torch, dev, p.lens)
    with variant_ctx(variant):
        aligned, _ = Run(torch, dev).hash_batch(p.types, to_dev(torch, dev, p.blob), base, lens)
        for shift in SHIFTS:
            got, status = Run(torch, dev).hash_batch(p.types, shifted(torch, dev, p.blob, shift), base, lens)
            assert np.array_equal(got, p.want) and np.array_equal(got, aligned) and status == 0, shift
            if name == "cfg3b":
                lead = np.concatenate([np.full(3, 0xEE, np.uint8), p.blob])
                got, _ = Run(torch, dev).hash_batch(p.types, shifted(torch, dev, lead, shift),
                                                    to_dev(torch, dev, p.base + np.uint64(3)), lens)
                assert np.array_equal(got, p.want), (shift, "lead 3")


@pytest.mark.parametrize("row", SWEEP_ROWS, ids=row_id)
def test_odd_store_address_hash_encoded(torch_dev, row):
    """keys and vals at odd addresses (one view for records: the product takes
    the records form only when keys == vals)."""
    torch, dev = torch_dev
    name, n, layout, form = row
    s = stored(name, n, layout)
    check_form(s.p, None, form)
    d = dev_stored(torch, dev, s)
    aligned, aligned_versions, _ = Run(torch, dev).hash_encoded(s.types, d)
    for shift in SHIFTS:
        e = list(d)
        e[3] = shifted(torch, dev, s.enc[3], shift)
        e[0] = e[3] if s.records else shifted(torch, dev, s.enc[0], (3 * shift) % 16)
        got, versions, status = Run(torch, dev).hash_encoded(s.types, e)
        assert np.array_equal(got, s.want) and np.array_equal(got, aligned) and status == 0, shift
        assert np.array_equal(versions, s.versions) and np.array_equal(versions, aligned_versions), shift


@pytest.mark.parametrize("t,n", INDEX_ROWS)
def test_odd_blob_address_index_encode(torch_dev, t, n):
    torch, dev = torch_dev
    blob, off, lens, want = index_column(t, n)
    d_off, d_lens = to_dev(torch, dev, off), to_dev(torch, dev, lens)
    for shift in SHIFTS:
        got, status = Run(torch, dev).index_encode(t, shifted(torch, dev, blob, shift), d_off, d_lens)
        assert got == want and status == 0, shift


# ---- 3. offsets across 2^32 -----------------------------------------------------------------

def high_rows(rows):
    """One case per form: the row's largest n (a single object cannot both
    straddle 2^32 and start above it)."""
    best = {}
    for row in rows:
        key = (row[0],) + tuple(row[2:])
        if key not in best or row[1] > best[key][1]:
            best[key] = row
    return [r for r in rows if best[(r[0],) + tuple(r[2:])] == r]


@pytest.mark.parametrize("order", ["in order", "permuted"])
@pytest.mark.parametrize("row", high_rows(BATCH_ROWS), ids=row_id)
def test_offsets_across_4gib_hash_batch(torch_dev, high_arena, row, order):
    torch, dev = torch_dev
    name, n, variant, form = row
    p = packed(name, n)
    check_form(p, variant, form)
    perm = np.random.default_rng(n).permutation(n) if order == "permuted" else np.arange(n)
    shift = high_arena.place(p.blob)
    base = p.base[perm] + np.uint64(shift)
    assert straddles(base, p.sizes[perm])
    lens = p.lens.reshape(n, p.A)[perm].reshape(-1)
    with variant_ctx(variant):
        got, status = Run(torch, dev).hash_batch(p.types, high_arena.view, to_dev(torch, dev, base),
                                                 to_dev(torch, dev, lens))
    assert np.array_equal(got, p.want[perm]) and status == 0


@pytest.mark.parametrize("order", ["in order", "permuted"])
@pytest.mark.parametrize("row", high_rows(SWEEP_ROWS), ids=row_id)
def test_offsets_across_4gib_hash_encoded(torch_dev, high_arena, row, order):
    """keycol and columns: the value store is in the arena (val_off across
    2^32); records: the one store is (key_off and val_off)."""
    torch, dev = torch_dev
    name, n, layout, form = row
    s = stored(name, n, layout)
    check_form(s.p, None, form)
    perm = np.random.default_rng(n).permutation(n) if order == "permuted" else np.arange(n)
    keys, key_off, key_len, vals, val_off, val_len = s.enc
    shift = np.uint64(high_arena.place(vals))
    val_off = val_off[perm] + shift
    key_off = key_off[perm] + (shift if s.records else np.uint64(0))
    assert straddles(key_off if s.records else val_off,
                     val_len[perm].astype(np.uint64) + (key_len[perm] if s.records else 0))
    d_keys = high_arena.view if s.records else to_dev(torch, dev, keys)
    enc = [d_keys, to_dev(torch, dev, key_off), to_dev(torch, dev, key_len[perm]), high_arena.view,
           to_dev(torch, dev, val_off), to_dev(torch, dev, val_len[perm])]
    got, versions, status = Run(torch, dev).hash_encoded(s.types, enc)
    assert np.array_equal(got, s.want[perm]) and np.array_equal(versions, s.versions[perm]) and status == 0


@pytest.mark.parametrize("order", ["in order", "permuted"])
@pytest.mark.parametrize("row", REGION_ROWS, ids=row_id)
def test_offsets_across_4gib_hash_batch_regions(torch_dev, high_arena, row, order):
    torch, dev = torch_dev
    name, n, variant, form = row
    p = packed(name, n)
    check_form(p, None, form)
    perm = np.random.default_rng(n + 1).permutation(n) if order == "permuted" else np.arange(n)
    shift = high_arena.place(p.blob)
    base = p.base[perm] + np.uint64(shift)
    assert straddles(base, p.sizes[perm])
    lens = p.lens.reshape(n, p.A)[perm].reshape(-1)
    tables, want_ids = tables_for(p.A, p.want)
    try:
        with variant_ctx(variant):
            ids, coords, status = Run(torch, dev).batch_regions(p.types, high_arena.view, to_dev(torch, dev, base),
                                                                to_dev(torch, dev, lens), tables,
                                                                order == "permuted")
    finally:
        for t in tables:
            t.close()
    assert np.array_equal(ids, want_ids[:, perm]) and status == 0
    if coords is not None:
        assert np.array_equal(coords, p.want[perm])


@pytest.mark.parametrize("order", ["in order", "permuted"])
def test_offsets_across_4gib_hash_encoded_regions(torch_dev, high_arena, order):
    torch, dev = torch_dev
    n = 65
    s = stored("cfg3b", n, "columns")
    perm = np.random.default_rng(n + 2).permutation(n) if order == "permuted" else np.arange(n)
    keys, key_off, key_len, vals, val_off, val_len = s.enc
    val_off = val_off[perm] + np.uint64(high_arena.place(vals))
    assert straddles(val_off, val_len[perm])
    enc = [to_dev(torch, dev, keys), to_dev(torch, dev, key_off[perm]), to_dev(torch, dev, key_len[perm]),
           high_arena.view, to_dev(torch, dev, val_off), to_dev(torch, dev, val_len[perm])]
    tables, want_ids = tables_for(s.A, s.want)
    try:
        ids, coords, versions, status = Run(torch, dev).encoded_regions(s.types, enc, tables, order == "permuted")
    finally:
        for t in tables:
            t.close()
    assert np.array_equal(ids, want_ids[:, perm]) and np.array_equal(versions, s.versions[perm]) and status == 0
    if coords is not None:
        assert np.array_equal(coords, s.want[perm])


@pytest.mark.parametrize("t", [INT64, FLOAT, TS_SECOND])
def test_offsets_across_4gib_index_encode(torch_dev, high_arena, t):
    """257 values at odd offsets on both sides of 2^32."""
    torch, dev = torch_dev
    blob, off, lens, want = index_column(t, 257)
    shift = high_arena.place(blob)
    off = off + np.uint64(shift)
    assert (off % 2 == 1).all() and (off < TWO32).any() and (off > TWO32).any()
    got, status = Run(torch, dev).index_encode(t, high_arena.view, to_dev(torch, dev, off), to_dev(torch, dev, lens))
    assert got == want and status == 0


# ---- 4. side stream ------------------------------------------------------------------------------
#
# The input is produced on the side stream s right before the call (the whole
# arena zeroed — a long producer — then the batch copied in), the entry gets
# stream=s, and only s is waited for.  A launch, an allocation or a free that
# the entry puts on another stream is not ordered behind the producer: it very
# likely reads zeros instead of the batch, and the values then differ from the
# oracle's.  Likely, not certain: a wrong library could pass by luck; a correct
# one passes every time.

def test_side_stream_hash_batch(torch_dev, high_arena):
    torch, dev = torch_dev
    p = packed("cfg3b", 65)
    check_form(p, None, 212)
    s = torch.cuda.Stream(dev)
    base = to_dev(torch, dev, p.base + np.uint64(high_arena.shift_for(len(p.blob))))
    run = Run(torch, dev, s, before=lambda: high_arena.behind_producer(s, p.blob))
    got, status = run.hash_batch(p.types, high_arena.view, base, to_dev(torch, dev, p.lens))
    assert np.array_equal(got, p.want) and status == 0


@pytest.mark.parametrize("with_coords", [False, True], ids=["ids", "ids+coords"])
def test_side_stream_hash_batch_regions_by_lookup(torch_dev, high_arena, with_coords):
    """Debug 235: the hash, the pool allocation of the coordinates' scratch
    (without coords), one lookup per table and the free, all on s."""
    torch, dev = torch_dev
    p = packed("cfg3b", 65)
    check_form(p, None, 212)
    s = torch.cuda.Stream(dev)
    base = to_dev(torch, dev, p.base + np.uint64(high_arena.shift_for(len(p.blob))))
    tables, want_ids = tables_for(p.A, p.want)
    try:
        with _lib.debug_library(235):
            run = Run(torch, dev, s, before=lambda: high_arena.behind_producer(s, p.blob))
            ids, coords, status = run.batch_regions(p.types, high_arena.view, base, to_dev(torch, dev, p.lens),
                                                    tables, with_coords)
    finally:
        for t in tables:
            t.close()
    assert np.array_equal(ids, want_ids) and status == 0
    if with_coords:
        assert np.array_equal(coords, p.want)


def _wide_stored_in_arena(torch, dev, high_arena):
    s = stored("a129", 9, "columns")
    check_form(s.p, None, 44)
    keys, key_off, key_len, vals, val_off, val_len = s.enc
    enc = [to_dev(torch, dev, keys), to_dev(torch, dev, key_off), to_dev(torch, dev, key_len), high_arena.view,
           to_dev(torch, dev, val_off + np.uint64(high_arena.shift_for(len(vals)))), to_dev(torch, dev, val_len)]
    return s, vals, enc


def test_side_stream_hash_encoded_wide(torch_dev, high_arena):
    """A = 129: the wide sweep's walk, then its hash, on s."""
    torch, dev = torch_dev
    s, vals, enc = _wide_stored_in_arena(torch, dev, high_arena)
    st = torch.cuda.Stream(dev)
    run = Run(torch, dev, st, before=lambda: high_arena.behind_producer(st, vals))
    got, versions, status = run.hash_encoded(s.types, enc)
    assert np.array_equal(got, s.want) and np.array_equal(versions, s.versions) and status == 0


@pytest.mark.parametrize("with_coords", [False, True], ids=["ids", "ids+coords"])
def test_side_stream_hash_encoded_regions_wide(torch_dev, high_arena, with_coords):
    """A = 129: walk, hash, the scratch's allocation and free (without
    coords) and one lookup per table, on s."""
    torch, dev = torch_dev
    s, vals, enc = _wide_stored_in_arena(torch, dev, high_arena)
    st = torch.cuda.Stream(dev)
    tables, want_ids = tables_for(s.A, s.want)
    try:
        run = Run(torch, dev, st, before=lambda: high_arena.behind_producer(st, vals))
        ids, coords, versions, status = run.encoded_regions(s.types, enc, tables, with_coords)
    finally:
        for t in tables:
            t.close()
    assert np.array_equal(ids, want_ids) and np.array_equal(versions, s.versions) and status == 0
    if with_coords:
        assert np.array_equal(coords, s.want)


@pytest.mark.parametrize("R", [64, 300], ids=["indexed", "scanned"])
def test_side_stream_lookup_region(torch_dev, high_arena, R):
    """The coordinates themselves are produced on s (in the arena, at 2^32)."""
    torch, dev = torch_dev
    n = 65
    attrs, lo, up, ids, coords, want = lookup_case(R, n)
    s = torch.cuda.Stream(dev)
    d_coords = high_arena.view[TWO32:TWO32 + coords.nbytes].view(torch.int64).view(n, coords.shape[1])
    t = RegionTable(attrs, lo, up, ids)
    try:
        run = Run(torch, dev, s, before=lambda: high_arena.behind_producer(s, coords.view(np.uint8).reshape(-1),
                                                                            at=TWO32))
        got = run.lookup(t, d_coords)
    finally:
        t.close()
    assert np.array_equal(got, want)


# ---- 5. PointLeaders -------------------------------------------------------------------------------

def _pack_keys(keys):
    lens = np.array([len(k) for k in keys], np.uint32)
    base = np.zeros(len(keys), np.uint64)
    base[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    return np.frombuffer(b"".join(keys) + bytes(16), np.uint8), base, lens


def test_point_leaders_mis_sized_key_raises(torch_dev):
    """A 5-byte INT64 key: the reference asserts; HdxError(HDX_E_BADSIZE), not
    the leader of coordinate 0."""
    torch, dev = torch_dev
    oracle = _ORACLE[0]
    rng = np.random.default_rng(5)
    keys = [rng.bytes(8) for _ in range(65)]
    keys[40] = rng.bytes(5)
    lo, up = oracle.partition(1, 16)
    pl = regions.PointLeaders(lo[:, 0], up[:, 0], np.arange(100, 116, dtype=np.uint64), np.ones(16, bool))
    try:
        with pytest.raises(hdx.HdxError) as e:
            pl.leaders(INT64, *[to_dev(torch, dev, x) for x in _pack_keys(keys)])
        assert e.value.status == _lib.HDX_E_BADSIZE
        with pytest.raises(hdx.HdxError) as e:
            pl.leaders(INT64, *[to_dev(torch, dev, x) for x in _pack_keys(keys)], check=False)
        assert e.value.status == _lib.HDX_E_BADSIZE
    finally:
        pl.close()


def _leader_keys():
    """65 string keys, a 16-region key grid, and the grid without one region
    that holds some of the keys but not key 0."""
    oracle = _ORACLE[0]
    rng = np.random.default_rng(11)
    keys = [rng.bytes(int(rng.integers(1, 60))) for _ in range(65)]
    lo, up = oracle.partition(1, 16)
    vsi = np.arange(100, 116, dtype=np.uint64)
    h = np.array([oracle.cityhash64(k) for k in keys], np.uint64)
    where = np.array([int(np.nonzero((lo[:, 0] <= x) & (x <= up[:, 0]))[0][0]) for x in h])
    hole = where[np.nonzero(where != where[0])[0][0]]
    return keys, lo[:, 0], up[:, 0], vsi, np.arange(16) != hole


def test_point_leaders_abort_on_a_side_stream(torch_dev, high_arena):
    """The keys are produced on s and the current stream is left alone: the
    abort check has to run behind the launch on s to see the key in the hole
    (the first one: ids read early are not the launch's)."""
    torch, dev = torch_dev
    keys, lo, up, vsi, keep = _leader_keys()
    blob, base, lens = _pack_keys(keys)
    want, aborted = _ORACLE[0].point_leader(dt.HYPERDATATYPE_STRING, keys, lo[keep], up[keep], vsi[keep],
                                            np.ones(15, bool))
    first = int(np.nonzero(aborted)[0][0])
    assert first > 0
    s = torch.cuda.Stream(dev)
    d_base = to_dev(torch, dev, base + np.uint64(high_arena.shift_for(len(blob))))
    d_lens = to_dev(torch, dev, lens)
    pl = regions.PointLeaders(lo[keep], up[keep], vsi[keep], np.ones(15, bool))
    try:
        high_arena.behind_producer(s, blob)
        with pytest.raises(regions.PointLeaderAbort, match=r"^key %d:" % first):
            pl.leaders(dt.HYPERDATATYPE_STRING, high_arena.view, d_base, d_lens, stream=s)
        s.synchronize()
    finally:
        pl.close()


@pytest.mark.parametrize("side", [True, False], ids=["side stream", "current stream"])
def test_point_leaders_match_oracle_on_either_stream(torch_dev, high_arena, side):
    torch, dev = torch_dev
    keys, lo, up, vsi, _ = _leader_keys()
    blob, base, lens = _pack_keys(keys)
    has = np.arange(16) % 5 != 2
    want, aborted = _ORACLE[0].point_leader(dt.HYPERDATATYPE_STRING, keys, lo, up, vsi, has)
    assert not aborted.any() and (want == 0).any()
    d_base = to_dev(torch, dev, base + np.uint64(high_arena.shift_for(len(blob))))
    d_lens = to_dev(torch, dev, lens)
    pl = regions.PointLeaders(lo, up, vsi, has)
    try:
        if side:
            s = torch.cuda.Stream(dev)
            high_arena.behind_producer(s, blob)
            leader, where = pl.leaders(dt.HYPERDATATYPE_STRING, high_arena.view, d_base, d_lens, stream=s)
            s.synchronize()
        else:
            high_arena.place(blob)
            leader, where = pl.leaders(dt.HYPERDATATYPE_STRING, high_arena.view, d_base, d_lens)
            torch.cuda.synchronize()
        assert np.array_equal(u64(leader), want)
        assert (u64(where) != 0).all()
    finally:
        pl.close()


# ---- 6. index key output alignment --------------------------------------------------------------------

def test_index_float_keys_into_an_8_aligned_view(torch_dev):
    """FLOAT's 16-byte keys into a uint64_t-aligned array that is not 16-byte
    aligned (include/hdxhash.h asks for 8)."""
    torch, dev = torch_dev
    blob, off, lens, want = index_column(FLOAT, 257)
    arena, out = guarded(torch, dev, 257 * 16, torch.uint8, 8)
    assert out.data_ptr() % 16 == 8
    got = hdx.index_encode(FLOAT, *[to_dev(torch, dev, x) for x in (blob, off, lens)], out=out)
    torch.cuda.synchronize()
    assert got.cpu().numpy().tobytes() == want
    assert_guards_intact(arena, out)


@pytest.mark.parametrize("t", [INT64, FLOAT])
@pytest.mark.parametrize("skew", [1, 4, 13])
def test_index_out_at_a_misaligned_address_is_rejected(torch_dev, t, skew):
    """HDX_E_INVALID before any launch: the view and its sentinels untouched."""
    torch, dev = torch_dev
    blob, off, lens, _ = index_column(t, 257)
    d = [to_dev(torch, dev, x) for x in (blob, off, lens)]
    arena, out = guarded(torch, dev, 257 * hdx.index_key_size(t), torch.uint8, skew)
    assert out.data_ptr() % 8 == skew % 8
    st = hdx.lib().hdx_index_encode_device(t, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), 257, out.data_ptr(),
                                           None, torch.cuda.current_stream(dev).cuda_stream)
    assert st == _lib.HDX_E_INVALID
    with pytest.raises(AssertionError):
        hdx.index_encode(t, *d, out=out)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0xA5).all()
    assert_guards_intact(arena, out)
