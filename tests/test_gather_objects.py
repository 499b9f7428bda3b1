"""The objects behind a list of indices, packed (hdx_gather_objects, hdx_gather_objects_plan_device /
_fill_device; include/hdxhash.h): record r = [key of idx[r] if KEYS][value of idx[r] if VALUES].

The expected bytes are slices of the host arrays (`expect`); nothing is decoded, so keys and values
here are mostly raw random bytes.  The device output must equal the host form and the slices, with
the status bits compared."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import hyperdex_amd as hdx
from hyperdex_amd import _lib, datatypes as dt, gather
from hyperdex_amd.checks import AttributeCheck
from hyperdex_amd.sorting import SortSpec
from test_index_entries import synth_store, to_dev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS, VALUES, BOTH = gather.KEYS, gather.VALUES, gather.KEYS | gather.VALUES
INVALID, NOMEM = 1 << _lib.HDX_E_INVALID, 1 << _lib.HDX_E_NOMEM
LAYOUTS = ["keycol", "records", "columns", "scatter"]


# ---- stores of raw (key, value) pairs and the expected records ------------------------------------

def excl(x):
    return np.concatenate([[0], np.cumsum(np.asarray(x, np.uint64))[:-1]]).astype(np.uint64)


def raw_store(pairs, layout="keycol", seed=0):
    """(key bytes, value bytes) pairs as (keys, key_off, key_len, vals, val_off, val_len): keys and
    values back to back (keycol), records [key][value] in one store, keys with gaps between them
    (columns), or both moved to a shuffled order with gaps (scatter)."""
    from test_encoded import _scatter
    rng = np.random.default_rng(seed)
    key_len = np.array([len(k) for k, _ in pairs], np.uint32)
    val_len = np.array([len(v) for _, v in pairs], np.uint32)
    if layout == "records":
        rec = np.frombuffer(b"".join(k + v for k, v in pairs) + b"\0", np.uint8)
        ro = excl(key_len.astype(np.uint64) + val_len)
        return rec, ro, key_len, rec, ro + key_len, val_len
    vals = np.frombuffer(b"".join(v for _, v in pairs) + b"\0", np.uint8)
    if layout == "columns":
        gaps = [bytes(int(g)) for g in rng.integers(0, 23, len(pairs))]
        keys = np.frombuffer(b"".join(g + k for g, (k, _) in zip(gaps, pairs)) + b"\0", np.uint8)
        key_off = excl([len(g) + len(k) for g, (k, _) in zip(gaps, pairs)]) + np.array([len(g) for g in gaps], np.uint64)
        return keys, key_off, key_len, vals, excl(val_len), val_len
    e = (np.frombuffer(b"".join(k for k, _ in pairs) + b"\0", np.uint8), excl(key_len), key_len, vals, excl(val_len),
         val_len)
    return _scatter(e, rng) if layout == "scatter" else e


def rand_pairs(rng, n, klo, khi, vlo, vhi):
    return [(rng.bytes(int(rng.integers(klo, khi + 1))), rng.bytes(int(rng.integers(vlo, vhi + 1)))) for _ in range(n)]


def sized_values(rng, sizes):
    return [(rng.bytes(int(rng.integers(0, 9))), rng.bytes(int(s))) for s in sizes]


def expect(e, idx, what, count=None):
    """(bytes, rec_off u64[cap + 1], rec_key_len u32[cap], status bits) by slicing."""
    keys, key_off, key_len, vals, val_off, val_len = e
    n, cap = len(val_len), len(idx)
    count = cap if count is None else min(count, cap)
    recs, kls, bits = [], [], 0
    for r in range(cap):
        k = v = b""
        i = int(idx[r])
        if r < count and i >= n:
            bits |= INVALID
        elif r < count:
            if what & KEYS:
                k = bytes(keys[int(key_off[i]):int(key_off[i]) + int(key_len[i])])
            if what & VALUES:
                v = bytes(vals[int(val_off[i]):int(val_off[i]) + int(val_len[i])])
        recs.append(k + v)
        kls.append(len(k))
    rec_off = np.concatenate([[0], np.cumsum([len(x) for x in recs], dtype=np.uint64)]).astype(np.uint64)
    return b"".join(recs), rec_off, np.array(kls, np.uint32), bits


def orders(rng, n):
    return {"ascending": np.arange(n, dtype=np.uint64), "descending": np.arange(n, dtype=np.uint64)[::-1].copy(),
            "shuffled": rng.integers(0, n, n + n // 2).astype(np.uint64)}


# ---- the host form --------------------------------------------------------------------------------

@pytest.mark.parametrize("what", [KEYS, VALUES, BOTH])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_host_form(layout, what):
    rng = np.random.default_rng(LAYOUTS.index(layout) * 3 + what)
    pairs = rand_pairs(rng, 300, 0, 20, 0, 60)
    pairs[0], pairs[7], pairs[299] = (b"", b""), (b"", rng.bytes(5)), (rng.bytes(3), b"")
    e = raw_store(pairs, layout, seed=what)
    for name, idx in orders(rng, len(pairs)).items():
        want, rec_off, kl, bits = expect(e, idx, what)
        out, got_off, got_kl, status = hdx.gather_objects_host(*e, idx, what)
        assert out.tobytes() == want and status == bits == 0, name
        assert np.array_equal(got_off, rec_off) and np.array_equal(got_kl, kl), name
        if name != "shuffled":  # object 0 is empty: an empty record among them
            assert 0 in np.diff(rec_off.astype(np.int64)).tolist()


def test_host_form_bad_index_and_short_buffer():
    rng = np.random.default_rng(5)
    e = raw_store(rand_pairs(rng, 50, 0, 9, 0, 30))
    idx = np.array([3, 50, 4, 2 ** 63, 49, 3], np.uint64)
    want, rec_off, kl, bits = expect(e, idx, BOTH)
    out, got_off, got_kl, status = hdx.gather_objects_host(*e, idx, BOTH)
    assert bits == INVALID == status and out.tobytes() == want
    assert np.array_equal(got_off, rec_off) and np.array_equal(got_kl, kl)
    assert rec_off[2] == rec_off[1] and rec_off[4] == rec_off[3]  # size 0
    # one byte short: HDX_E_NOMEM, offsets filled, nothing written
    buf = np.full(len(want) + 8, 0xA5, np.uint8)
    out, got_off, got_kl, status = hdx.gather_objects_host(*e, idx, BOTH, out=buf[:len(want) - 1])
    assert status == INVALID | NOMEM and len(out) == 0 and np.array_equal(got_off, rec_off)
    assert buf.tobytes() == b"\xa5" * len(buf)
    out, _, _, status = hdx.gather_objects_host(*e, idx, BOTH, out=buf[:len(want)])
    assert status == INVALID and buf.tobytes() == want + b"\xa5" * 8
    # no records at all
    out, got_off, got_kl, status = hdx.gather_objects_host(*e, np.zeros(0, np.uint64), BOTH)
    assert len(out) == 0 and got_off.tolist() == [0] and len(got_kl) == 0 and status == 0


# ---- refusals before any device -------------------------------------------------------------------

PLAN_ARGS = ["key_len", "val_len", "n", "idx", "count_dev", "cap", "what", "rec_off", "rec_key_len", "status_dev",
             "stream"]
FILL_ARGS = ["keys", "key_off", "key_len", "vals", "val_off", "val_len", "n", "idx", "count_dev", "cap", "what",
             "rec_off", "out", "out_bytes", "status_dev", "stream"]
HOST_ARGS = ["keys", "key_off", "key_len", "vals", "val_off", "val_len", "n", "idx", "count", "what", "rec_off",
             "rec_key_len", "out", "out_bytes", "status"]
SCALARS = {"n": 5, "cap": 3, "count": 0, "what": BOTH, "out_bytes": 1 << 20}
MAY_BE_NULL = {"count_dev", "rec_key_len", "status_dev", "status", "stream"}


def _call(entry, names, **over):
    """The entry point with stand-in (never dereferenced) pointers; `over` replaces arguments."""
    args = []
    for k, name in enumerate(names):
        v = SCALARS.get(name, None if name in MAY_BE_NULL else 4096 * (k + 1))
        args.append(over.get(name, v))
    return entry(*args)


@pytest.mark.parametrize("form", ["plan", "fill", "host"])
def test_entry_points_refuse_bad_arguments(form):
    lib = hdx.lib()
    entry, names = {"plan": (lib.hdx_gather_objects_plan_device, PLAN_ARGS),
                    "fill": (lib.hdx_gather_objects_fill_device, FILL_ARGS),
                    "host": (lib.hdx_gather_objects, HOST_ARGS)}[form]
    cap = "count" if form == "host" else "cap"
    for name in names:
        if name not in SCALARS and name not in MAY_BE_NULL:
            assert _call(entry, names, **{name: None}) == _lib.HDX_E_INVALID, name
    for what in (0, 4, 5, 8, 0xffffffff):
        assert _call(entry, names, what=what) == _lib.HDX_E_INVALID, what
    assert _call(entry, names, **{cap: (1 << 40) + 1}) == _lib.HDX_E_INVALID
    assert _call(entry, names, n=(1 << 40) + 1) == _lib.HDX_E_INVALID
    if form != "plan":  # the parts asked for need their bytes; the other part's may be absent
        assert _call(entry, names, what=KEYS, keys=None) == _lib.HDX_E_INVALID
        assert _call(entry, names, what=KEYS, key_off=None) == _lib.HDX_E_INVALID
        assert _call(entry, names, what=VALUES, vals=None) == _lib.HDX_E_INVALID
        assert _call(entry, names, what=VALUES, val_off=None) == _lib.HDX_E_INVALID
    if form == "host":  # count == 0: nothing is dereferenced but rec_off[0]
        rec_off = np.full(1, 7, np.uint64)
        assert _call(entry, names, rec_off=rec_off.ctypes.data, what=KEYS, vals=None, val_off=None) == _lib.HDX_OK
        assert rec_off[0] == 0
    elif lib.hdx_device_count() == 0:  # valid arguments reach the device binding, and only then
        assert _call(entry, names) == _lib.HDX_E_DEVICE
        assert _call(entry, names, what=VALUES, keys=None, key_off=None) == _lib.HDX_E_DEVICE


def test_tile_bytes_is_exported():
    T = hdx.lib().hdx_gather_tile_bytes()
    assert T == hdx.gather_tile_bytes() and T >= 64 and T & (T - 1) == 0


def test_debug_baseline_is_in_the_debug_library_only():
    assert hasattr(_lib.debug_lib(), "hdxdbg_gather_objects_fill_by_extents")
    with pytest.raises(AttributeError):
        hdx.lib().hdxdbg_gather_objects_fill_by_extents


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_host_form_under_asan_ubsan(tmp_path):
    """tests/cpp/gather_objects_test.cc + hdx_cpu.cpp as one sanitized program (no Python in it)."""
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
    inc = ["-I" + os.path.join(ROOT, "hyperdex_amd", "csrc"), "-I" + os.path.join(ROOT, "include")]
    exe = str(tmp_path / "gather_objects_test")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *san, *inc,
                    os.path.join(ROOT, "tests", "cpp", "gather_objects_test.cc"),
                    os.path.join(ROOT, "hyperdex_amd", "csrc", "hdx_cpu.cpp"), "-o", exe], check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "gather_objects_test ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---- the device: helpers --------------------------------------------------------------------------

@pytest.fixture(scope="module")
def torch_gpu():
    import torch
    return torch


def dev_idx(torch, dev, idx):
    return torch.from_numpy(np.asarray(idx, np.uint64).view(np.int64).copy()).to(dev)


def baseline_fill(torch, d, idx_d, count_d, what, rec_off, out, status):
    """The debug library's record-major fill into `out`."""
    gather._fill(_lib.debug_lib().hdxdbg_gather_objects_fill_by_extents, *d, idx_d, count_d, what, rec_off, out,
                 status, None)


def check_device(torch, e, idx, what, count=None, stream=None, baseline=False):
    """gather_objects on the device == the host form == the slices; returns the expected bytes."""
    dev = torch.device("cuda", 0)
    d = to_dev(torch, dev, e)
    idx_d = dev_idx(torch, dev, idx)
    count_d = None if count is None else torch.tensor([count], dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()  # the inputs are in place before another stream reads them
    out, rec_off, rec_kl = hdx.gather_objects(*d, idx_d, count_d, what, status=status, stream=stream)
    (stream or torch.cuda.current_stream(dev)).synchronize()
    want, want_off, want_kl, bits = expect(e, idx, what, count)
    assert np.array_equal(rec_off.cpu().numpy().view(np.uint64), want_off)
    assert np.array_equal(rec_kl.cpu().numpy().view(np.uint32), want_kl)
    assert out.cpu().numpy().tobytes() == want
    assert int(status.item()) == bits
    live = len(idx) if count is None else min(count, len(idx))
    h_out, h_off, h_kl, h_bits = hdx.gather_objects_host(*e, np.asarray(idx, np.uint64)[:live], what)
    assert h_out.tobytes() == want and h_bits == bits
    assert np.array_equal(h_off, want_off[:live + 1]) and np.array_equal(h_kl, want_kl[:live])
    assert (want_off[live:] == want_off[-1]).all() and not want_kl[live:].any()
    if baseline:
        buf = torch.full((len(want) + 32,), 0xA5, dtype=torch.uint8, device=dev)
        status.zero_()
        baseline_fill(torch, d, idx_d, count_d, what, rec_off, buf[:len(want)], status)
        torch.cuda.synchronize()
        assert buf.cpu().numpy().tobytes() == want + b"\xa5" * 32 and int(status.item()) == 0
    return want


# ---- the device: tests ----------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("cap", [0, 1, 63, 64, 65, 255, 256, 257])
def test_gpu_record_counts(torch_gpu, cap):
    rng = np.random.default_rng(cap)
    e = raw_store(rand_pairs(rng, 300, 0, 20, 0, 90))
    check_device(torch_gpu, e, rng.integers(0, 300, cap).astype(np.uint64), BOTH)


@pytest.mark.gpu
@pytest.mark.parametrize("count", [0, 37, 100, 101, 5000])
def test_gpu_count_on_the_device(torch_gpu, count):
    """count_dev below, at and above cap = 100: the tail of rec_off is the total, rec_key_len's is 0."""
    rng = np.random.default_rng(count)
    e = raw_store(rand_pairs(rng, 200, 1, 20, 0, 90))
    torch = torch_gpu
    idx = rng.integers(0, 200, 100).astype(np.uint64)
    want = check_device(torch, e, idx, BOTH, count=count)
    # more room than the total: `out` beyond the total is untouched
    dev = torch.device("cuda", 0)
    d, idx_d = to_dev(torch, dev, e), dev_idx(torch, dev, idx)
    count_d = torch.tensor([count], dtype=torch.int64, device=dev)
    rec_off, _ = hdx.gather_objects_plan(d[2], d[5], idx_d, count_d, BOTH)
    buf = torch.full((len(want) + 5000,), 0xA5, dtype=torch.uint8, device=dev)
    hdx.gather_objects_fill(*d, idx_d, count_d, BOTH, rec_off, buf)
    torch.cuda.synchronize()
    assert buf.cpu().numpy().tobytes() == want + b"\xa5" * 5000


def _sizes_to(rng, total, hi=300):
    sizes = []
    while sum(sizes) < total:
        sizes.append(int(rng.integers(0, hi + 1)))
    sizes[-1] -= sum(sizes) - total
    return sizes


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["T-1", "T", "T+1", "2T-1", "2T+1", "long", "ends_on_tile", "empty_run"])
def test_gpu_tile_edges(torch_gpu, case):
    """VALUES only, record sizes chosen so that the total or a record's end falls around a tile
    boundary (the output is allocated, so its base is aligned and tiles start at multiples of T)."""
    T = hdx.gather_tile_bytes()
    rng = np.random.default_rng(len(case))
    totals = {"T-1": T - 1, "T": T, "T+1": T + 1, "2T-1": 2 * T - 1, "2T+1": 2 * T + 1}
    if case in totals:
        sizes = _sizes_to(rng, totals[case])
    elif case == "long":  # one record of 3T + 5 bytes among small ones
        sizes = _sizes_to(rng, 700, 40) + [3 * T + 5] + _sizes_to(rng, 900, 40)
    elif case == "ends_on_tile":  # a record ends exactly at T, and one at 2T
        sizes = _sizes_to(rng, T) + _sizes_to(rng, T) + _sizes_to(rng, 333)
    else:  # 200 empty records between the last byte of a tile and the first of the next
        sizes = _sizes_to(rng, T) + [0] * 200 + _sizes_to(rng, 500)
    e = raw_store(sized_values(rng, sizes))
    want = check_device(torch_gpu, e, np.arange(len(sizes), dtype=np.uint64), VALUES, baseline=True)
    assert len(want) == sum(sizes)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["int64_keys", "sizes_0_40", "both_parts"])
def test_gpu_small_records(torch_gpu, case):
    rng = np.random.default_rng(len(case))
    if case == "int64_keys":  # KEYS only, 8-byte keys: two records per 16-byte chunk
        pairs, what = [(rng.bytes(8), rng.bytes(int(rng.integers(10, 40)))) for _ in range(3000)], KEYS
    elif case == "sizes_0_40":
        sizes = list(range(41)) * 30
        rng.shuffle(sizes)
        pairs, what = sized_values(rng, sizes), VALUES
    else:
        pairs, what = rand_pairs(rng, 3000, 0, 17, 10, 27), BOTH
    e = raw_store(pairs)
    idx = rng.permutation(len(pairs)).astype(np.uint64)
    _, rec_off, _, _ = expect(e, idx, what)
    if case == "sizes_0_40":
        assert set(np.diff(rec_off.astype(np.int64)).tolist()) == set(range(41))
    check_device(torch_gpu, e, idx, what, baseline=True)


@pytest.mark.gpu
@pytest.mark.parametrize("short", [0, 1])
@pytest.mark.parametrize("lead", [0, 1, 2, 3, 5, 16])
def test_gpu_alignment_and_ownership(torch_gpu, lead, short):
    """Keys and values at every address mod 16, `out` at `lead` inside a larger buffer of 0xA5: with
    room for exactly the total the canaries on both sides stay; one byte short nothing is written
    and HDX_E_NOMEM's bit is set."""
    torch = torch_gpu
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(lead)
    e = raw_store(rand_pairs(rng, 1200, 0, 33, 0, 70))
    nonempty_k, nonempty_v = e[2] > 0, e[5] > 0
    assert set((e[1][nonempty_k] % 16).tolist()) == set(range(16))
    assert set((e[4][nonempty_v] % 16).tolist()) == set(range(16))
    idx = rng.integers(0, 1200, 900).astype(np.uint64)
    want, want_off, _, _ = expect(e, idx, BOTH)
    d = to_dev(torch, dev, e)
    assert d[0].data_ptr() % 16 == 0 and d[3].data_ptr() % 16 == 0
    idx_d = dev_idx(torch, dev, idx)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    rec_off, _ = hdx.gather_objects_plan(d[2], d[5], idx_d, None, BOTH, status=status)
    buf = torch.full((lead + len(want) + 37,), 0xA5, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 16 == 0
    hdx.gather_objects_fill(*d, idx_d, None, BOTH, rec_off, buf[lead:lead + len(want) - short], status=status)
    torch.cuda.synchronize()
    got = buf.cpu().numpy().tobytes()
    assert np.array_equal(rec_off.cpu().numpy().view(np.uint64), want_off)
    if short:
        assert got == b"\xa5" * len(got) and int(status.item()) == NOMEM
    else:
        assert got == b"\xa5" * lead + want + b"\xa5" * 37 and int(status.item()) == 0


@pytest.mark.gpu
def test_gpu_bad_indices_among_good_ones(torch_gpu):
    rng = np.random.default_rng(9)
    e = raw_store(rand_pairs(rng, 500, 0, 20, 0, 90))
    idx = rng.integers(0, 500, 700).astype(np.uint64)
    idx[[0, 63, 64, 300, 699]] = [500, 2 ** 63, 501, 2 ** 40, 2 ** 64 - 1]
    check_device(torch_gpu, e, idx, BOTH, baseline=True)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_gpu_layouts_in_top_order(torch_gpu, layout):
    from test_encoded import _scatter
    types, e = synth_store("cfg3b", 700, seed=50, layout="columns" if layout == "scatter" else layout)
    rng = np.random.default_rng(8)
    if layout == "scatter":
        e = _scatter(e, rng)
    idx = rng.integers(0, 700, 400).astype(np.uint64)  # no order, duplicates
    assert len(set(idx.tolist())) < 400
    for what in (BOTH, KEYS, VALUES):
        check_device(torch_gpu, e, idx, what)


@pytest.mark.gpu
def test_gpu_side_stream(torch_gpu):
    """Launches and the read of the total run on the given stream only."""
    torch = torch_gpu
    types, e = synth_store("cfg3b", 500, seed=70)
    torch.cuda.synchronize()
    check_device(torch, e, np.arange(500, dtype=np.uint64)[::-1].copy(), BOTH, stream=torch.cuda.Stream())


@pytest.mark.gpu
@pytest.mark.parametrize("delta", [-1, 0, 1, "square"])
def test_gpu_scan_levels(torch_gpu, delta):
    """cap at SCAN_BLOCK - 1, SCAN_BLOCK, SCAN_BLOCK + 1 and SCAN_BLOCK^2 + 1025 (every level of the
    reduce-then-scan), KEYS only over 8-byte keys: the output is the keys as int64, indexed."""
    torch = torch_gpu
    dev = torch.device("cuda", 0)
    SB = hdx.index.SCAN_BLOCK
    cap = SB * SB + 1025 if delta == "square" else SB + delta
    n = 5000
    g = torch.Generator(device="cpu").manual_seed(cap)
    keys64 = torch.randint(-2 ** 62, 2 ** 62, (n,), dtype=torch.int64, generator=g).to(dev)
    keys = keys64.view(torch.uint8)
    key_off = torch.arange(n, dtype=torch.int64, device=dev) * 8
    key_len = torch.full((n,), 8, dtype=torch.int32, device=dev)
    val_len = torch.full((n,), 11, dtype=torch.int32, device=dev)
    idx = torch.randint(0, n, (cap,), dtype=torch.int64, generator=g).to(dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    out, rec_off, rec_kl = hdx.gather_objects(keys, key_off, key_len, keys, key_off, val_len, idx, None, KEYS,
                                              status=status)
    torch.cuda.synchronize()
    assert torch.equal(rec_off, torch.arange(cap + 1, dtype=torch.int64, device=dev) * 8)
    assert bool((rec_kl == 8).all()) and int(status.item()) == 0
    assert out.numel() == 8 * cap and torch.equal(out.view(torch.int64), keys64[idx])


@pytest.mark.gpu
def test_gpu_offsets_beyond_32_bits(torch_gpu):
    """Plan only (no bytes are read): seven records whose values sum past 4 GiB."""
    torch = torch_gpu
    dev = torch.device("cuda", 0)
    vl = np.array([0xfffffff0, 5, 0x80000000, 0, 0xffffffff, 123, 0x7fffffff], np.uint32)
    kl = np.array([3, 0, 9, 7, 0, 1, 2], np.uint32)
    idx = np.array([4, 0, 0, 6, 2, 3, 7, 1, 5], np.uint64)  # 7: a bad index
    val_len, key_len = [torch.from_numpy(x.view(np.int32).copy()).to(dev) for x in (vl, kl)]
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    rec_off, rec_kl = hdx.gather_objects_plan(key_len, val_len, dev_idx(torch, dev, idx), None, BOTH, status=status)
    torch.cuda.synchronize()
    sizes = [0 if i == 7 else int(vl[i]) + int(kl[i]) for i in idx.tolist()]
    want = np.concatenate([[0], np.cumsum(sizes, dtype=np.uint64)]).astype(np.uint64)
    assert int(want[-1]) > 1 << 32
    assert np.array_equal(rec_off.cpu().numpy().view(np.uint64), want) and int(status.item()) == INVALID
    assert rec_kl.cpu().tolist() == [0 if i == 7 else int(kl[i]) for i in idx.tolist()]


HALF = AttributeCheck(2, b"\x80", dt.HYPERDATATYPE_STRING, dt.HYPERPREDICATE_LESS_EQUAL)


@pytest.mark.gpu
def test_gpu_closure_with_check_encoded(torch_gpu):
    """match -> gather -> the same checks over the gathered batch: every object passes."""
    torch = torch_gpu
    dev = torch.device("cuda", 0)
    types, e = synth_store("cfg3b", 3000, seed=81)
    d = to_dev(torch, dev, e)
    first_fail, match = hdx.check_encoded(types, *d, [HALF])
    assert 900 < match.numel() < 2100
    out, rec_off, rec_kl = hdx.gather_objects(*d, match)
    batch = gather.batch_of(out, rec_off, rec_kl)
    ff2, match2 = hdx.check_encoded(types, *batch, [HALF])
    torch.cuda.synchronize()
    assert ff2.numel() == match.numel() and bool((ff2 == 1).all())
    assert torch.equal(match2, torch.arange(match.numel(), dtype=torch.int64, device=dev))
    want, _, _, _ = expect(e, match.cpu().numpy().view(np.uint64), BOTH)
    assert out.cpu().numpy().tobytes() == want


@pytest.mark.gpu
def test_gpu_closure_with_sorted_search(oracle, torch_gpu):
    """top -> gather: attribute 11 (INT64) read out of the gathered values ascends."""
    torch = torch_gpu
    dev = torch.device("cuda", 0)
    types, e = synth_store("cfg3b", 3000, seed=82)
    d = to_dev(torch, dev, e)
    _, top = hdx.sorted_search(types, *d, [HALF], SortSpec(11), 100)
    assert top.numel() == 100
    out, rec_off, rec_kl = hdx.gather_objects(*d, top)
    torch.cuda.synchronize()
    _, _, _, vals, val_off, val_len = [x.cpu().numpy() for x in gather.batch_of(out, rec_off, rec_kl)]
    got = []
    for r in range(100):
        ok, _, sl = oracle.decode_value(len(types), vals, int(val_off[r]), int(val_len[r]))
        assert ok
        o, L = sl[10]
        assert L == 8
        got.append(struct.unpack("<q", bytes(vals[int(val_off[r]) + o:int(val_off[r]) + o + 8]))[0])
    assert got == sorted(got)
    want, _, _, _ = expect(e, top.cpu().numpy().view(np.uint64), BOTH)
    assert out.cpu().numpy().tobytes() == want
