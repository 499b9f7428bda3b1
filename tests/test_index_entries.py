"""Secondary-index entries of stored objects (hdx_index_entry, hdx_index_entries_plan_device /
_fill_device; include/hdxhash.h): what datalayer::indexer_thread Puts per object and index
(daemon/index_primitive.cc:291-329).

The expected bytes are composed here (`compose`): prefix ++ enc(attribute) ++ enc(key) ++ a
u32 BE key size only for STRING x STRING.  Numeric encodings come from oracle.index_encode
(pinned to the reference's compiled encoders where they are built and to
tests/golden/reference_store_values.json); one GPU test takes them from that fixture alone.
Strings are raw.  Decode verdicts are the oracle's decode_value."""
import ctypes
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import hyperdex_amd as hdx
from hyperdex_amd import _lib, datatypes as dt, synth
from hyperdex_amd.index import IndexSpec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRING, INT64, FLOAT = dt.HYPERDATATYPE_STRING, dt.HYPERDATATYPE_INT64, dt.HYPERDATATYPE_FLOAT
TS = dt.TIMESTAMPS[3]
P1, P3, P21 = b"i", b"i\x05\x07", b"i" + bytes(range(0x81, 0x8b)) + bytes(range(0x91, 0x9b))
BADENC, BADSIZE, NOMEM = 1 << _lib.HDX_E_BADENC, 1 << _lib.HDX_E_BADSIZE, 1 << _lib.HDX_E_NOMEM


def enc(oracle, t, v):
    """enc(type, value) of the header's table; None for a numeric the reference asserts on."""
    if t == STRING:
        return bytes(v)
    k, err = oracle.index_encode(t, bytes(v))
    return None if err else k


def compose(oracle, prefix, key_type, key, attr_type, value):
    v, k = enc(oracle, attr_type, value), enc(oracle, key_type, key)
    if v is None or k is None:
        return None
    e = prefix + v + k
    if key_type == STRING and attr_type == STRING:
        e += struct.pack(">I", len(k))
    return e


# ---- the CPU form ------------------------------------------------------------------------

def _values(t, rng):
    if t == STRING:
        return [rng.bytes(L) for L in list(range(41)) + [1100]]
    return [b"", bytes(8), struct.pack("<q", -2), struct.pack("<d", 1.5), struct.pack("<d", float("-inf")),
            rng.bytes(8), b"\xff" * 8]


@pytest.mark.parametrize("key_type", [STRING, INT64, FLOAT, TS])
@pytest.mark.parametrize("attr_type", [STRING, INT64, FLOAT, TS])
def test_cpu_entry_matches_composition(oracle, key_type, attr_type):
    rng = np.random.default_rng(key_type * 7 + attr_type)
    count = 0
    for prefix in (P1, P3, P21):
        for key in _values(key_type, rng):
            for value in _values(attr_type, rng):
                want = compose(oracle, prefix, key_type, key, attr_type, value)
                got = hdx.index_entry(IndexSpec(2, prefix), key_type, key, attr_type, value)
                assert got == want, (prefix, key, value)
                fixed = (8 if key_type != STRING else len(key)) + (0 if attr_type != FLOAT else 8) \
                    + (8 if attr_type != STRING else len(value)) + (8 if key_type == FLOAT else 0)
                # the u32 suffix only when neither encoding is fixed
                assert len(got) == len(prefix) + fixed + (4 if key_type == attr_type == STRING else 0)
                count += 1
    assert count >= 3 * 7 * 7


def _raw_entry(spec, key_type, key, attr_type, value, cap):
    c = spec.c()
    out = ctypes.create_string_buffer(b"\xa5" * (cap + 8), cap + 8)
    need = ctypes.c_size_t(12345)
    st = hdx.lib().hdx_index_entry(ctypes.byref(c), key_type, key, len(key), attr_type, value, len(value), out, cap,
                                   ctypes.byref(need))
    return st, need.value, out.raw


def test_cpu_entry_one_byte_short(oracle):
    for key_type, key, attr_type, value in ((STRING, b"key", STRING, b"value"), (INT64, bytes(8), FLOAT, b""),
                                            (STRING, b"", STRING, b"")):
        want = compose(oracle, P3, key_type, key, attr_type, value)
        st, need, raw = _raw_entry(IndexSpec(1, P3), key_type, key, attr_type, value, len(want) - 1)
        assert st == _lib.HDX_E_NOMEM and need == len(want) and raw == b"\xa5" * (len(want) + 7)
        st, need, raw = _raw_entry(IndexSpec(1, P3), key_type, key, attr_type, value, len(want))
        assert st == _lib.HDX_OK and need == len(want) and raw == want + b"\xa5" * 8


@pytest.mark.parametrize("size", [1, 2, 3, 4, 5, 6, 7, 9])
def test_cpu_entry_bad_numeric_size(size):
    """HDX_E_BADSIZE, nothing written, and *out_len still the entry's size: a numeric's
    encoded size does not depend on its value."""
    for t in (INT64, FLOAT, TS):
        ksz = 16 if t == FLOAT else 8
        st, need, raw = _raw_entry(IndexSpec(1, P1), STRING, b"k", t, bytes(size), 64)
        assert (st, need, raw) == (_lib.HDX_E_BADSIZE, 1 + ksz + 1, b"\xa5" * 72)
        st, need, raw = _raw_entry(IndexSpec(1, P1), t, bytes(size), STRING, b"v", 64)
        assert (st, need, raw) == (_lib.HDX_E_BADSIZE, 1 + 1 + ksz, b"\xa5" * 72)


def test_cpu_entry_bad_type_and_spec():
    for t in (dt.HYPERDATATYPE_LIST_STRING, dt.HYPERDATATYPE_DOCUMENT, dt.HYPERDATATYPE_MAP_INT64_FLOAT, 12345):
        assert _raw_entry(IndexSpec(1, P1), t, b"", STRING, b"", 64)[:2] == (_lib.HDX_E_BADTYPE, 0)
        assert _raw_entry(IndexSpec(1, P1), STRING, b"", t, b"", 64)[:2] == (_lib.HDX_E_BADTYPE, 0)
    assert _raw_entry(IndexSpec(0, P1), STRING, b"", STRING, b"", 64)[0] == _lib.HDX_E_INVALID
    assert _raw_entry(IndexSpec(1, b""), STRING, b"", STRING, b"", 64)[0] == _lib.HDX_E_INVALID
    assert _raw_entry(IndexSpec(1, b"i" * 22), STRING, b"", STRING, b"", 64)[0] == _lib.HDX_E_INVALID


# ---- the device entry points' argument checks: before the device is touched ---------------

def _plan_call(types, specs, m=None, null=None, n=5):
    """hdx_index_entries_plan_device with stand-in (never dereferenced) device pointers."""
    t = np.asarray(types, np.uint32)
    p = {k: 4096 * (i + 1) for i, k in enumerate(("key_len", "vals", "val_off", "val_len", "attr_off", "attr_len",
                                                  "entry_off"))}
    sp = hdx.index._specs(specs) if specs is not None else None
    tp = t.ctypes.data
    if null == "types":
        tp = None
    elif null == "specs":
        sp = None
    elif null:
        p[null] = None
    return hdx.lib().hdx_index_entries_plan_device(tp, len(t), p["key_len"], p["vals"], p["val_off"], p["val_len"], n,
                                                   sp, len(specs) if m is None else m, p["attr_off"], p["attr_len"],
                                                   p["entry_off"], None, None)


def _fill_call(types, specs, m=None, null=None, n=5):
    t = np.asarray(types, np.uint32)
    p = {k: 4096 * (i + 1) for i, k in enumerate(("keys", "key_off", "key_len", "vals", "val_off", "attr_off",
                                                  "attr_len", "entry_off", "entries"))}
    sp = hdx.index._specs(specs) if specs is not None else None
    tp = t.ctypes.data
    if null == "types":
        tp = None
    elif null == "specs":
        sp = None
    elif null:
        p[null] = None
    return hdx.lib().hdx_index_entries_fill_device(tp, len(t), p["keys"], p["key_off"], p["key_len"], p["vals"],
                                                   p["val_off"], n, sp, len(specs) if m is None else m, p["attr_off"],
                                                   p["attr_len"], p["entry_off"], p["entries"], 1 << 20, None, None)


@pytest.mark.parametrize("call", [_plan_call, _fill_call])
def test_device_entry_points_refuse_bad_arguments(call):
    types = [STRING, STRING, INT64]
    ok = [IndexSpec(1, P3), IndexSpec(2, P21)]
    assert call(types, ok, m=0) == _lib.HDX_E_INVALID
    assert call(types, [IndexSpec(1, P1)] * 33) == _lib.HDX_E_INVALID
    assert call(types, [IndexSpec(0, P1)]) == _lib.HDX_E_INVALID          # the key is no index
    assert call(types, [IndexSpec(3, P1)]) == _lib.HDX_E_INVALID          # attr >= attrs_sz
    assert call(types, [IndexSpec(1, b"")]) == _lib.HDX_E_INVALID
    assert call(types, [IndexSpec(1, b"i" * 22)]) == _lib.HDX_E_INVALID
    assert call([], ok) == _lib.HDX_E_INVALID
    for bad in (dt.HYPERDATATYPE_LIST_INT64, dt.HYPERDATATYPE_DOCUMENT, dt.HYPERDATATYPE_MAP_STRING_STRING):
        assert call([STRING, bad, INT64], [IndexSpec(1, P1)]) == _lib.HDX_E_BADTYPE   # an indexed container
        assert call([bad, STRING, INT64], [IndexSpec(1, P1)]) == _lib.HDX_E_BADTYPE   # a container key
        # a container no index names is the sweep's business only
        assert call([STRING, bad, INT64], [IndexSpec(1, P1)], null="vals") == _lib.HDX_E_BADTYPE
        assert call([STRING, bad, INT64], [IndexSpec(2, P1)], null="vals") == _lib.HDX_E_INVALID
    assert call([STRING, 12345], [IndexSpec(1, P1)]) == _lib.HDX_E_BADTYPE
    names = ["types", "specs", "key_len", "vals", "val_off", "attr_off", "attr_len", "entry_off"]
    names += ["val_len"] if call is _plan_call else ["keys", "key_off", "entries"]
    for name in names:
        assert call(types, ok, null=name) == _lib.HDX_E_INVALID, name
    if hdx.lib().hdx_device_count() == 0:  # valid arguments reach the device binding, and only then
        assert call(types, ok) == _lib.HDX_E_DEVICE


def test_scan_block_is_exported():
    assert hdx.index.SCAN_BLOCK == hdx.lib().hdx_index_scan_block() and hdx.index.SCAN_BLOCK >= 64


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_cpu_entry_under_asan_ubsan(tmp_path):
    """tests/cpp/index_entry_test.cc + hdx_cpu.cpp as one sanitized program (no Python in it)."""
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
    inc = ["-I" + os.path.join(ROOT, "hyperdex_amd", "csrc"), "-I" + os.path.join(ROOT, "include")]
    exe = str(tmp_path / "index_entry_test")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *san, *inc,
                    os.path.join(ROOT, "tests", "cpp", "index_entry_test.cc"),
                    os.path.join(ROOT, "hyperdex_amd", "csrc", "hdx_cpu.cpp"), "-o", exe], check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "index_entry_test ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---- the device: helpers -------------------------------------------------------------------

def store(objs, A, layout="keycol", first_version=1):
    """Stored objects [(key, [attribute bytes] * (A - 1))] as (keys, key_off, key_len, vals, val_off, val_len)."""
    keys = [k for k, _ in objs]
    vals = [struct.pack(">QH", first_version + i, A - 1) + b"".join(struct.pack(">I", len(x)) + x for x in attrs)
            for i, (_, attrs) in enumerate(objs)]
    key_len = np.array([len(k) for k in keys], np.uint32)
    val_len = np.array([len(v) for v in vals], np.uint32)

    def excl(x):
        return np.concatenate([[0], np.cumsum(x.astype(np.uint64))[:-1]]).astype(np.uint64)
    if layout == "records":
        rec = np.frombuffer(b"".join(k + v for k, v in zip(keys, vals)) + b"\0", np.uint8)
        ro = excl(key_len.astype(np.uint64) + val_len)
        return rec, ro, key_len, rec, ro + key_len, val_len
    return (np.frombuffer(b"".join(keys) + b"\0", np.uint8), excl(key_len), key_len,
            np.frombuffer(b"".join(vals) + b"\0", np.uint8), excl(val_len), val_len)


def expected(oracle, types, enc_arrays, specs):
    """Per object: the list of its m entries, or None where it is refused (the oracle's decode
    verdict, or a mis-sized numeric key / indexed attribute); and the descriptors."""
    keys, key_off, key_len, vals, val_off, val_len = enc_arrays
    A, n, m = len(types), len(val_off), len(specs)
    out, desc = [], np.zeros((n, m, 2), np.uint32)
    badenc = np.zeros(n, bool)
    for i in range(n):
        vo = int(val_off[i])
        ok, _, sl = oracle.decode_value(A, vals, vo, int(val_len[i]))
        badenc[i] = not ok
        ents = None
        if ok:
            key = bytes(keys[int(key_off[i]):int(key_off[i]) + int(key_len[i])])
            ents = []
            for s in specs:
                o, L = sl[s.attr - 1]
                e = compose(oracle, s.prefix, int(types[0]), key, int(types[s.attr]), bytes(vals[vo + o:vo + o + L]))
                if e is None:
                    ents = None
                    break
                ents.append(e)
            if ents is not None:
                desc[i] = [sl[s.attr - 1] for s in specs]
        out.append(ents)
    return out, desc, badenc


def to_dev(torch, dev, arrs):
    from test_encoded import _to_dev
    out = _to_dev(torch, dev, arrs)
    if arrs[0] is arrs[3]:  # records: one store
        out[3] = out[0]
    return out


def run_device(torch, types, enc_arrays, specs, stream=None):
    dev = torch.device("cuda", 0)
    d = to_dev(torch, dev, enc_arrays)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    keys, key_off, key_len, vals, val_off, val_len = d
    torch.cuda.synchronize()  # the inputs are in place before another stream reads them
    plan = hdx.index_entries_plan(types, key_len, vals, val_off, val_len, specs, status=status, stream=stream)
    entries, entry_off = hdx.index_entries(types, *d, specs, status=status, stream=stream)
    (stream or torch.cuda.current_stream(dev)).synchronize()
    assert torch.equal(plan[2], entry_off)
    n, m = len(enc_arrays[4]), len(specs)
    return (entries.cpu().numpy().tobytes(), entry_off.cpu().numpy().view(np.uint64),
            plan[0].cpu().numpy().view(np.uint32).reshape(n, m), plan[1].cpu().numpy().view(np.uint32).reshape(n, m),
            int(status.item()) & 0xffffffff)


def check_device(torch, oracle, types, enc_arrays, specs, want_status=0, stream=None):
    want, desc, badenc = expected(oracle, types, enc_arrays, specs)
    m = len(specs)
    sizes = np.array([len(e) for ents in want for e in (ents if ents is not None else [b""] * m)], np.uint64)
    blob, entry_off, attr_off, attr_len, status = run_device(torch, types, enc_arrays, specs, stream)
    assert np.array_equal(entry_off, np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64))
    assert blob == b"".join(e for ents in want if ents is not None for e in ents)
    assert np.array_equal(attr_off, desc[:, :, 0]) and np.array_equal(attr_len, desc[:, :, 1])
    assert status == want_status
    return want, badenc


def synth_store(cfg_or_rules, n, seed, layout="keycol"):
    types, blob, base, lens = synth.make_batch_host(cfg_or_rules, n, seed=seed)
    if layout == "columns":
        return types, synth.encode_values_host(types, blob, base, lens, first_version=3)
    return types, synth.encode_store_host(types, blob, base, lens, first_version=3, layout=layout)


@pytest.fixture(scope="module")
def torch_gpu():
    import torch
    return torch


SMALL = [synth.Rule(STRING, synth.UNIFORM, 0, 9), synth.Rule(STRING, synth.UNIFORM, 0, 12), synth._n(INT64)]


# ---- the device: tests ---------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_gpu_lane_wave_block_edges(oracle, torch_gpu, n):
    types, e = synth_store(SMALL, n, seed=n)
    check_device(torch_gpu, oracle, types, e, [IndexSpec(1, P3), IndexSpec(2, P21)])


@pytest.mark.gpu
@pytest.mark.parametrize("delta", [-1, 0, 1, "square"])
def test_gpu_scan_block_boundaries(oracle, torch_gpu, delta):
    """n*m at SCAN_BLOCK - 1, SCAN_BLOCK, SCAN_BLOCK + 1 and SCAN_BLOCK^2 + 1 (every level of the
    reduce-then-scan): entry_off against a vectorised cumsum, bytes on samples."""
    torch = torch_gpu
    SB = hdx.index.SCAN_BLOCK
    n = SB * SB + 1 if delta == "square" else SB + delta
    rules = [synth.Rule(STRING, synth.UNIFORM, 0, 3), synth.Rule(STRING, synth.UNIFORM, 0, 5)]
    dev = torch.device("cuda", 0)
    types, keys, key_off, key_len, vals, val_off, val_len = synth.make_encoded_device(rules, n, seed=77, device=dev,
                                                                                     layout="keycol")
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    entries, entry_off = hdx.index_entries(types, keys, key_off, key_len, vals, val_off, val_len, [IndexSpec(1, P3)],
                                           status=status)
    torch.cuda.synchronize()
    sizes = len(P3) + (val_len.to(torch.int64) - 14) + key_len.to(torch.int64) + 4
    want_off = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(sizes, 0)])
    assert torch.equal(entry_off, want_off) and int(status.item()) == 0
    assert entries.numel() == int(want_off[-1].item())
    hk, hko, hkl = keys.cpu().numpy(), key_off.cpu().numpy(), key_len.cpu().numpy()
    hv, hvo, hvl = vals.cpu().numpy(), val_off.cpu().numpy(), val_len.cpu().numpy()
    he, ho = entries.cpu().numpy(), entry_off.cpu().numpy()
    rng = np.random.default_rng(5)
    for i in [0, n - 1] + rng.integers(0, n, 2000).tolist():
        key = bytes(hk[hko[i]:hko[i] + hkl[i]])
        value = bytes(hv[hvo[i] + 14:hvo[i] + hvl[i]])
        assert bytes(he[ho[i]:ho[i + 1]]) == compose(oracle, P3, STRING, key, STRING, value), i


@pytest.mark.gpu
def test_gpu_alignment_coverage(oracle, torch_gpu):
    """STRING key 0-33 B, STRING attribute 0-40 B and an INT64; prefixes of 3 and 21 bytes: entries
    start at every offset mod 16, keys and attributes at every address mod 16."""
    rng = np.random.default_rng(11)
    objs = [(rng.bytes(int(rng.integers(0, 34))),
             [rng.bytes(int(rng.integers(0, 41))), rng.bytes(8) if rng.random() < 0.9 else b""]) for _ in range(1500)]
    types = [STRING, STRING, INT64]
    specs = [IndexSpec(1, P3), IndexSpec(2, P21), IndexSpec(1, P21)]
    e = store(objs, 3)
    want, _ = check_device(torch_gpu, oracle, types, e, specs)
    starts = np.concatenate([[0], np.cumsum([len(x) for ents in want for x in ents])])[:-1].reshape(-1, 3)
    for k in range(3):
        assert set((starts[:, k] % 16).tolist()) == set(range(16)), k
    nonempty = e[2] > 0
    assert set((e[1][nonempty] % 16).tolist()) == set(range(16))          # keys
    attr1 = e[4] + np.uint64(14)
    assert set((attr1 % 16).tolist()) == set(range(16))                   # the string attribute
    attr2 = attr1 + np.array([len(o[1][0]) for o in objs], np.uint64) + np.uint64(4)
    assert set((attr2 % 16).tolist()) == set(range(16))                   # the numeric


@pytest.mark.gpu
def test_gpu_schema_cfg3b(oracle, torch_gpu):
    types, e = synth_store("cfg3b", 3000, seed=31)
    check_device(torch_gpu, oracle, types, e, [IndexSpec(2, P3), IndexSpec(12, P21), IndexSpec(15, P1)])


@pytest.mark.gpu
def test_gpu_schema_mixed(oracle, torch_gpu):
    types, e = synth_store("mixed", 2000, seed=32)
    specs = [IndexSpec(1, P3)] + [IndexSpec(4 + g, b"i\x02" + bytes([g + 1])) for g in range(6)]
    assert [int(types[s.attr]) for s in specs[1:]] == list(dt.TIMESTAMPS)
    check_device(torch_gpu, oracle, types, e, specs)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["A2", "A130_last", "twice", "descending", "int64_key", "float_key", "m32"])
def test_gpu_schema_shapes(oracle, torch_gpu, case):
    s10 = synth.Rule(STRING, synth.UNIFORM, 0, 10)
    if case == "A2":
        rules, specs = [synth._s(5), s10], [IndexSpec(1, P3)]
    elif case == "A130_last":
        rules = [s10] * 127 + [synth._n(INT64), synth._n(FLOAT), synth.Rule(STRING, synth.UNIFORM, 0, 30)]
        specs = [IndexSpec(129, P3)]
    elif case == "twice":
        rules, specs = SMALL, [IndexSpec(1, P3), IndexSpec(1, P21), IndexSpec(2, P3), IndexSpec(2, P1)]
    elif case == "descending":
        rules = [s10, s10, synth._n(INT64), synth._n(FLOAT), s10]
        specs = [IndexSpec(4, P3), IndexSpec(3, P3), IndexSpec(2, P21), IndexSpec(1, P1)]
    elif case == "int64_key":
        rules, specs = [synth._n(INT64), s10, synth._n(FLOAT)], [IndexSpec(1, P3), IndexSpec(2, P3)]
    elif case == "float_key":
        rules, specs = [synth._n(FLOAT), s10, synth._n(TS)], [IndexSpec(1, P21), IndexSpec(2, P3)]
    else:  # the most indices a call takes (the plan's 128-object workgroups)
        rules = [s10, s10, synth._n(INT64)]
        specs = [IndexSpec(1 + k % 2, b"i" + bytes([k + 1])) for k in range(32)]
    types, e = synth_store(rules, 300, seed=40)
    want, _ = check_device(torch_gpu, oracle, types, e, specs)
    if case in ("int64_key", "float_key"):  # a fixed key encoding: no suffix
        ksz = 8 if case == "int64_key" else 16
        _, desc, _ = expected(oracle, types, e, specs)
        assert all(len(ents[0]) == len(specs[0].prefix) + int(desc[i, 0, 1]) + ksz for i, ents in enumerate(want))


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["keycol", "records", "columns", "scatter"])
def test_gpu_layouts(oracle, torch_gpu, layout):
    from test_encoded import _scatter
    types, e = synth_store("cfg3b", 700, seed=50, layout="columns" if layout == "scatter" else layout)
    if layout == "scatter":
        e = _scatter(e, np.random.default_rng(8))
    check_device(torch_gpu, oracle, types, e, [IndexSpec(2, P3), IndexSpec(12, P21)])


CORRUPT_SEED = 2


def _corrupt_case(oracle):
    from test_encoded import _corrupt
    types, blob, base, lens = synth.make_batch_host("cfg3b", 100, seed=9)
    e, cases = _corrupt(synth.encode_values_host(types, blob, base, lens, first_version=1),
                        np.random.default_rng(CORRUPT_SEED))
    _, _, bad = oracle.hash_encoded(types, *e)
    return types, e, cases, bad


def test_corrupt_case_on_the_oracle(oracle):
    """The damage test's premise, on the CPU: the oracle refuses exactly the damaged values, and at
    least a third of the objects still yield entries."""
    types, e, cases, bad = _corrupt_case(oracle)
    assert set(np.nonzero(bad)[0].tolist()) == set(cases) and len(cases) == 40
    want, _, badenc = expected(oracle, types, e, [IndexSpec(2, P3), IndexSpec(12, P21)])
    assert np.array_equal(badenc, bad)
    assert sum(w is not None for w in want) * 3 >= len(want)


@pytest.mark.gpu
def test_gpu_damaged_values(oracle, torch_gpu):
    torch = torch_gpu
    types, e, cases, bad = _corrupt_case(oracle)
    want, badenc = check_device(torch, oracle, types, e, [IndexSpec(2, P3), IndexSpec(12, P21), IndexSpec(15, P1)],
                                want_status=BADENC)
    refused = np.array([w is None for w in want])
    assert np.array_equal(refused, bad) and refused.sum() == bad.sum() == len(cases)
    assert (~refused).sum() * 3 >= len(want)
    # ... and the sweep's verdict (version 0) on the same values
    dev = torch.device("cuda", 0)
    versions = torch.zeros(len(want), dtype=torch.int64, device=dev)
    hdx.hash_encoded(types, *to_dev(torch, dev, e), versions=versions)
    torch.cuda.synchronize()
    assert np.array_equal(versions.cpu().numpy() == 0, refused)


@pytest.mark.gpu
def test_gpu_bad_numeric_sizes(oracle, torch_gpu):
    rng = np.random.default_rng(3)
    types = [STRING, STRING, INT64, INT64]
    objs = [(rng.bytes(7), [rng.bytes(int(rng.integers(0, 20))), rng.bytes(8), rng.bytes(8)]) for _ in range(200)]
    objs[17][1][1] = rng.bytes(5)
    objs[130][1][1] = rng.bytes(5)
    e = store(objs, 4)
    # attribute 2 indexed: objects 17 and 130 are empty, HDX_E_BADSIZE
    want, _ = check_device(torch_gpu, oracle, types, e, [IndexSpec(1, P3), IndexSpec(2, P21)], want_status=BADSIZE)
    assert [i for i, w in enumerate(want) if w is None] == [17, 130]
    # attribute 2 not named by any index: nothing is refused, no bit
    want, _ = check_device(torch_gpu, oracle, types, e, [IndexSpec(1, P3), IndexSpec(3, P21)], want_status=0)
    assert all(w is not None for w in want)
    # a mis-sized numeric key refuses the object too
    objs2 = [(rng.bytes(8 if i != 5 else 3), [b"abc"]) for i in range(70)]
    want, _ = check_device(torch_gpu, oracle, [INT64, STRING], store(objs2, 2), [IndexSpec(1, P3)], want_status=BADSIZE)
    assert [i for i, w in enumerate(want) if w is None] == [5]


@pytest.mark.gpu
@pytest.mark.parametrize("lead", [0, 1, 2, 3, 5, 16])
def test_gpu_ownership_canaries(oracle, torch_gpu, lead):
    """entries inside a larger buffer of 0xA5: with capacity exactly the total the canaries on both
    sides stay; with total - 1 nothing is written and HDX_E_NOMEM is set."""
    torch = torch_gpu
    dev = torch.device("cuda", 0)
    types, e = synth_store(SMALL, 130, seed=60 + lead)
    specs = [IndexSpec(1, P3), IndexSpec(2, P1)]
    want, _, _ = expected(oracle, types, e, specs)
    blob = b"".join(x for ents in want for x in ents)
    d = to_dev(torch, dev, e)
    keys, key_off, key_len, vals, val_off, val_len = d
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    plan = hdx.index_entries_plan(types, key_len, vals, val_off, val_len, specs, status=status)
    for short in (0, 1):
        buf = torch.full((lead + len(blob) + 37,), 0xA5, dtype=torch.uint8, device=dev)
        status.zero_()
        hdx.index_entries_fill(types, keys, key_off, key_len, vals, val_off, specs, *plan,
                               buf[lead:lead + len(blob) - short], status=status)
        torch.cuda.synchronize()
        got = buf.cpu().numpy().tobytes()
        if short:
            assert got == b"\xa5" * len(got) and int(status.item()) == NOMEM
        else:
            assert got == b"\xa5" * lead + blob + b"\xa5" * 37 and int(status.item()) == 0


@pytest.mark.gpu
def test_gpu_entry_offsets_beyond_32_bits(torch_gpu):
    """Plan only: the total passes 2^32 bytes; entry_off is the cumsum of the closed form."""
    torch = torch_gpu
    dev = torch.device("cuda", 0)
    rules = [synth._s(8), synth.Rule(STRING, synth.UNIFORM, 200, 4000)]
    n = 2_100_000
    types, keys, key_off, key_len, vals, val_off, val_len = synth.make_encoded_device(rules, n, seed=4, device=dev,
                                                                                     layout="keycol")
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    attr_off, attr_len, entry_off = hdx.index_entries_plan(types, key_len, vals, val_off, val_len, [IndexSpec(1, P3)],
                                                           status=status)
    torch.cuda.synchronize()
    sizes = len(P3) + (val_len.to(torch.int64) - 14) + key_len.to(torch.int64) + 4
    want = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(sizes, 0)])
    assert int(want[-1].item()) > 1 << 32
    assert torch.equal(entry_off, want) and int(status.item()) == 0
    assert bool((attr_off == 14).all()) and torch.equal(attr_len, val_len - 14)


@pytest.mark.gpu
def test_gpu_empty_batch_is_checked_like_any_other(torch_gpu):
    """n == 0: no entries and entry_off == [0]; bad specs and types are refused as on any batch."""
    torch = torch_gpu
    dev = torch.device("cuda", 0)
    e = [torch.empty(0, dtype=d, device=dev) for d in (torch.uint8, torch.int64, torch.int32, torch.uint8,
                                                        torch.int64, torch.int32)]
    types = [STRING, STRING, INT64]
    entries, entry_off = hdx.index_entries(types, *e, [IndexSpec(1, P3), IndexSpec(2, P21)])
    torch.cuda.synchronize()
    assert entries.numel() == 0 and entry_off.cpu().tolist() == [0]
    for bad_types, specs, want in ((types, [IndexSpec(0, P3)], _lib.HDX_E_INVALID), (types, [], _lib.HDX_E_INVALID),
                                   (types, [IndexSpec(1, b"")], _lib.HDX_E_INVALID),
                                   ([STRING, dt.HYPERDATATYPE_LIST_STRING], [IndexSpec(1, P3)], _lib.HDX_E_BADTYPE)):
        with pytest.raises(hdx.HdxError) as err:
            hdx.index_entries(bad_types, *e, specs)
        assert err.value.status == want


@pytest.mark.gpu
def test_gpu_side_stream(oracle, torch_gpu):
    """Launches and the read of the total run on the given stream only: results are right with
    only that stream waited for."""
    torch = torch_gpu
    types, e = synth_store("cfg3b", 500, seed=70)
    torch.cuda.synchronize()
    check_device(torch, oracle, types, e, [IndexSpec(2, P3), IndexSpec(12, P21)], stream=torch.cuda.Stream())


@pytest.mark.gpu
def test_gpu_equals_cpu_form(torch_gpu):
    """The device's entries equal hdx_index_entry's on 500 objects (no oracle in between)."""
    types, e = synth_store("cfg3b", 500, seed=71)
    specs = [IndexSpec(2, P3), IndexSpec(12, P21), IndexSpec(15, P1)]
    blob, entry_off, attr_off, attr_len, status = run_device(torch_gpu, types, e, specs)
    keys, key_off, key_len, vals, val_off, val_len = e
    assert status == 0
    for i in range(500):
        key = bytes(keys[int(key_off[i]):int(key_off[i]) + int(key_len[i])])
        for k, s in enumerate(specs):
            o = int(val_off[i]) + int(attr_off[i, k])
            want = hdx.index_entry(s, int(types[0]), key, int(types[s.attr]), bytes(vals[o:o + int(attr_len[i, k])]))
            assert blob[int(entry_off[i * 3 + k]):int(entry_off[i * 3 + k + 1])] == want, (i, k)


@pytest.mark.gpu
def test_gpu_numeric_keys_from_the_fixture_alone(torch_gpu):
    """Expected bytes from tests/golden/reference_store_values.json only (no oracle): the 269 recorded
    values of INT64, FLOAT and the timestamp as attributes 1-3 of 269 objects, and as keys."""
    from test_reference_store import index_cases
    cases = index_cases()
    rows = list(zip(cases[INT64], cases[FLOAT], cases[TS]))
    types = [STRING, INT64, FLOAT, TS]
    objs = [(b"key%03d" % i + b"x" * (i % 5), [r[0][0], r[1][0], r[2][0]]) for i, r in enumerate(rows)]
    specs = [IndexSpec(1, P3), IndexSpec(2, P21), IndexSpec(3, P1)]
    blob, entry_off, _, _, status = run_device(torch_gpu, types, store(objs, 4), specs)
    want = b"".join(s.prefix + r[k][1] + objs[i][0] for i, r in enumerate(rows) for k, s in enumerate(specs))
    assert blob == want and status == 0 and int(entry_off[-1]) == len(want)
    # the same values as keys: FLOAT key, STRING attribute -> prefix ++ string ++ 16-byte key, no suffix
    objs = [(r[1][0], [b"v" * (i % 7)]) for i, r in enumerate(rows)]
    blob, entry_off, _, _, status = run_device(torch_gpu, [FLOAT, STRING], store(objs, 2), [IndexSpec(1, P3)])
    assert blob == b"".join(P3 + b"v" * (i % 7) + r[1][1] for i, r in enumerate(rows)) and status == 0
