"""Every consumer of a region table (the plain lookup kernels, the fused gather
and wave-staged forms over packed batches, the stored-object sweep, the
batcher's multi-table kernel and its host lookup) over every kind of table
the lookup code tells apart, against the oracle's lookup_region over the
oracle's coordinates.

The kinds (_kinds; index sizes in u64 words, hdx_region_index.h's layout,
asserted by test_region_kinds_sizes_and_expected_answers):
  grid1   partition(1, 64) on [0]: R 64, W 1, index 195 words (1.5 KiB).
  grid3   partition(3, 64) on [1, 2, 3]: R 64, D 3, W 1, index 225 words.
  w2      R 100, D 1 on [0], boxes of width 2^58 at random positions: W 2,
          index 668 words (5.2 KiB).  With grid1 before it, it still fits the
          fused gather forms' 16 KiB of LDS table copies.
  w4      R 256, D 1 on [0], the same way: W 4, index 2630 words (20.5 KiB) —
          over the fused forms' 16 KiB budget (read from global memory there),
          under the plain kernels' 48 KiB (staged in LDS there).
  scan    R 300, D 2 on [A - 1, 0], random wide boxes: more than 256 regions,
          so no index; every lookup scans the boxes.
  bigidx  R 256, D 3 on [A - 1, 0, 2], overlapping random boxes: W 4, index
          7890 words (61.6 KiB) — over the plain kernels' 48 KiB too, read
          from global memory.  Plain and multi-table consumers only.
A lookup that always answered from the first mask word, or never with "no
region", would pass on grids alone: the expected answers themselves are
checked (_check_expected) to hold positions >= 64 for w2, a position in each
64-block and 0 for w4, and more than one id for scan."""
import contextlib

import numpy as np
import pytest

from hyperdex_amd import synth
from test_regions import _coords

SETS = {"indexed": ("grid1", "w2", "w4", "grid3"), "scan": ("grid1", "w4", "scan", "grid3")}
BATCHER_TYPES = [9217, 9218, 9219, 9217, 9474]
_FIRST_ID = {"grid1": 1001, "grid3": 2001, "w2": 3001, "w4": 4001, "scan": 5001, "bigidx": 6001}


def _kinds(oracle, A):
    """name -> (attrs, lower, upper, ids); ids[r] = _FIRST_ID[name] + r."""
    rng = np.random.default_rng(8)

    def narrow(R):
        lo = rng.integers(0, 2**64 - 2**58, size=(R, 1), dtype=np.uint64)
        return lo, lo + np.uint64(2**58 - 1)

    def wide(R, D):
        a = rng.integers(0, 2**64, size=(R, D), dtype=np.uint64)
        b = rng.integers(0, 2**64, size=(R, D), dtype=np.uint64)
        return np.minimum(a, b), np.maximum(a, b)

    boxes = {"grid1": ([0],) + tuple(oracle.partition(1, 64)),
             "grid3": ([1, 2, 3],) + tuple(oracle.partition(3, 64)),
             "w2": ([0],) + narrow(100), "w4": ([0],) + narrow(256),
             "scan": ([A - 1, 0],) + wide(300, 2), "bigidx": ([A - 1, 0, 2],) + wide(256, 3)}
    return {k: (at, lo, up, np.arange(len(lo), dtype=np.uint64) + np.uint64(_FIRST_ID[k]))
            for k, (at, lo, up) in boxes.items()}


def _index_words(lo, up):
    """u64 words of region_index_build's index (0: none)."""
    R, D = lo.shape
    if R > 256:
        return 0
    words = D
    for d in range(D):
        pts = set(lo[:, d].tolist()) | {int(u) + 1 for u in up[:, d].tolist() if int(u) != 2**64 - 1}
        words += 65 + len(pts) + (len(pts) + 1) * ((R + 63) // 64)
    return words


def _check_expected(kind, want):
    pos = want[want != 0].astype(np.int64) - _FIRST_ID[kind]
    if kind == "w2":
        assert (pos >= 64).any()
    if kind == "w4":
        assert set((pos // 64).tolist()) == {0, 1, 2, 3} and (want == 0).any()
    if kind == "scan":
        assert len(np.unique(want)) >= 2


def _expected(oracle, specs, kinds, coords):
    want = {k: oracle.lookup_region(*specs[k], coords) for k in kinds}
    for k in kinds:
        _check_expected(k, want[k])
    return want


_INPUTS = {}


def _packed(oracle, cfg, n):
    """(types, blob, base, lens, the oracle's coordinates), computed once."""
    if (cfg, n) not in _INPUTS:
        types, blob, base, lens = synth.make_batch_host(cfg, n, seed=n)
        _INPUTS[cfg, n] = (types, blob, base, lens, oracle.hash_batch(types, blob, base, lens)[0])
    return _INPUTS[cfg, n]


def _stored(oracle, cfg, n):
    if ("stored", cfg, n) not in _INPUTS:
        types, blob, base, lens, _ = _packed(oracle, cfg, n)
        enc = synth.encode_values_host(types, blob, base, lens, first_version=2)
        _INPUTS["stored", cfg, n] = (types, enc, oracle.hash_encoded(types, *enc)[0])
    return _INPUTS["stored", cfg, n]


def _batcher_objects(oracle):
    if "batcher" not in _INPUTS:
        rng = np.random.default_rng(12)
        objs = []
        for _ in range(300):
            key = rng.bytes(int(rng.integers(0, 120)))
            objs.append((key, [rng.bytes(8), rng.bytes(8), rng.bytes(int(rng.integers(0, 70))), rng.bytes(8)]))
        coords = np.array([[oracle.hash_value(t, v)[0] for t, v in zip(BATCHER_TYPES, [k] + vs)] for k, vs in objs],
                          np.uint64)
        _INPUTS["batcher"] = (objs, coords)
    return _INPUTS["batcher"]


def _library(variant):
    from hyperdex_amd import _lib
    return _lib.debug_library(variant) if variant is not None else contextlib.nullcontext()


def _to_dev(torch, arrs):
    views = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}
    return [torch.from_numpy(np.ascontiguousarray(a).view(views.get(a.dtype, a.dtype))).to(torch.device("cuda", 0))
            for a in arrs]


def test_region_kinds_sizes_and_expected_answers(oracle):
    """On the CPU, with the oracle alone: the tables have the index sizes the
    module docstring gives and fall on the intended side of the 16 KiB and
    48 KiB budgets, and the expected answers of every GPU test below hold the
    cases that tell the lookup paths apart (_check_expected)."""
    specs = _kinds(oracle, 6)
    words = {k: _index_words(lo, up) for k, (_, lo, up, _) in specs.items()}
    assert words == {"grid1": 195, "grid3": 225, "w2": 668, "w4": 2630, "scan": 0, "bigidx": 7890}
    staged = {k: 8 * (words[k] + len(specs[k][1])) for k in specs}  # index + ids, bytes
    assert staged["grid1"] + staged["w2"] <= 16384 < staged["w4"] <= 48 * 1024 < staged["bigidx"]
    assert staged["grid1"] + staged["grid3"] <= 16384
    # the batcher's multi-table kernel: five tables fit its 48 KiB of LDS, six do not
    boxes = 8 * (2 * 300 * 2 + 300)
    five = sum(staged[k] for k in ("grid1", "w2", "w4", "grid3")) + boxes
    assert five <= 48 * 1024 < five + staged["bigidx"]
    rng = np.random.default_rng(3)
    for k, (at, lo, up, ids) in specs.items():
        _check_expected(k, oracle.lookup_region(at, lo, up, ids, _coords(rng, 4000, 6, lo, up, at)))
    for kinds in SETS.values():
        for cfg, n in (("cfg2", 1537), ("cfg3b", 777)):
            types, _, _, _, coords = _packed(oracle, cfg, n)
            _expected(oracle, _kinds(oracle, len(types)), kinds, coords)
        types, _, coords = _stored(oracle, "cfg3b", 777)
        _expected(oracle, _kinds(oracle, len(types)), kinds, coords)
    _expected(oracle, _kinds(oracle, 5), list(_FIRST_ID), _batcher_objects(oracle)[1])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(_FIRST_ID))
def test_gpu_plain_lookup_every_kind(oracle, kind):
    """regions.lookup_region, each kind on its own: 4000 rows, a quarter of
    them on box edges."""
    import torch

    from hyperdex_amd import regions
    A = 6
    at, lo, up, ids = _kinds(oracle, A)[kind]
    coords = _coords(np.random.default_rng(3), 4000, A, lo, up, at)
    want = oracle.lookup_region(at, lo, up, ids, coords)
    _check_expected(kind, want)
    t = regions.RegionTable(at, lo, up, ids)
    got = regions.lookup_region(t, _to_dev(torch, [coords])[0])
    torch.cuda.synchronize()
    t.close()
    assert np.array_equal(got.cpu().numpy().view(np.uint64), want)


def _batch_regions(oracle, cfg, n, kinds, variant):
    import torch

    import hyperdex_amd as hdx
    types, blob, base, lens, want_coords = _packed(oracle, cfg, n)
    specs = _kinds(oracle, len(types))
    want = _expected(oracle, specs, kinds, want_coords)
    d = _to_dev(torch, [blob, base, lens])
    with _library(variant):
        tables = [hdx.RegionTable(*specs[k]) for k in kinds]
        for with_coords in (False, True):
            out = hdx.hash_batch_regions(types, *d, tables, coords=with_coords)
            torch.cuda.synchronize()
            ids, coords = out if with_coords else (out, None)
            for j, k in enumerate(kinds):
                assert np.array_equal(ids[j].cpu().numpy().view(np.uint64), want[k]), (k, with_coords)
            if with_coords:
                assert np.array_equal(coords.cpu().numpy().view(np.uint64), want_coords)
        for t in tables:
            t.close()


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [None, 100, 101, 104])
@pytest.mark.parametrize("tables", list(SETS))
def test_gpu_fused_gather_form_every_kind(oracle, tables, variant):
    """hash_batch_regions on cfg2, 1537 objects, with and without coordinates:
    the product library, a lane per (table, object) pair (100), the
    wave-uniform table loop (101), the tables in global memory (104).  grid1,
    w2 and grid3 are looked up in their LDS copies, w4 through its index in
    global memory, scan by the scan."""
    _batch_regions(oracle, "cfg2", 1537, SETS[tables], variant)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [None, 217])
@pytest.mark.parametrize("tables", list(SETS))
def test_gpu_fused_wave_staged_form_every_kind(oracle, tables, variant):
    """hash_batch_regions on cfg3b, 777 objects: the wave-staged form (the
    product library, and forced, 217).  Its 7 objects per wave times the 6
    table dimensions are at most 64 searches, so the all-indexed set takes
    lookup_tables_wave's parallel arm; with scan in the set it takes the
    table-by-table arm."""
    _batch_regions(oracle, "cfg3b", 777, SETS[tables], variant)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [None, 233, 234, 235])
@pytest.mark.parametrize("tables", list(SETS))
def test_gpu_stored_objects_every_kind(oracle, tables, variant):
    """hash_encoded_regions on cfg3b, 777 stored objects, key-column layout:
    the product library (the gather sweep's fused form at this size), the
    wave-staged sweep with the lookup fused (233), the gather sweep's fused
    form forced (234), the sweep and one lookup launch per table (235)."""
    import torch

    import hyperdex_amd as hdx
    kinds = SETS[tables]
    types, enc, want_coords = _stored(oracle, "cfg3b", 777)
    specs = _kinds(oracle, len(types))
    want = _expected(oracle, specs, kinds, want_coords)
    d = _to_dev(torch, enc)
    with _library(variant):
        tabs = [hdx.RegionTable(*specs[k]) for k in kinds]
        for with_coords in (False, True):
            out = hdx.hash_encoded_regions(types, *d, tabs, coords=with_coords)
            torch.cuda.synchronize()
            ids, coords = out if with_coords else (out, None)
            for j, k in enumerate(kinds):
                assert np.array_equal(ids[j].cpu().numpy().view(np.uint64), want[k]), (k, with_coords)
            if with_coords:
                assert np.array_equal(coords.cpu().numpy().view(np.uint64), want_coords)
        for t in tabs:
            t.close()


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["device_six_tables", "device_five_tables", "host"])
def test_gpu_batcher_every_kind(oracle, path):
    """hdx.Batcher over 300 objects with more tables than the fused kernel
    takes, so the device batches run the multi-table lookup kernel — which no
    other test reaches (the other batcher tests use one or two tables): all
    six kinds (bigidx pushes the tables past 48 KiB: walked in global memory),
    the five without bigidx (staged in LDS), and every object on the calling
    thread (region_lookup_host over the host arrays)."""
    import hyperdex_amd as hdx
    kinds = [k for k in _FIRST_ID if k != "bigidx" or path != "device_five_tables"]
    objs, coords = _batcher_objects(oracle)
    specs = _kinds(oracle, len(BATCHER_TYPES))
    want = _expected(oracle, specs, kinds, coords)
    tables = [hdx.RegionTable(*specs[k]) for k in kinds]
    bad = []
    with hdx.Batcher(BATCHER_TYPES, tables=tables, max_delay_us=100, device_only=path != "host") as b:
        for i, (key, vals) in enumerate(objs):
            hs, rid = b.hash_object(key, vals)
            if hs != coords[i].tolist() or rid != [int(want[k][i]) for k in kinds]:
                bad.append(i)
        st = b.stats()
    for t in tables:
        t.close()
    assert not bad, bad[:5]
    assert st["objects"] == len(objs)
    assert (st["host"] == len(objs) and st["batches"] == 0) if path == "host" else (st["host"] == 0 and st["batches"] >= 1)
