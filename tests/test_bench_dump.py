"""bench.py's plain run and --dump-outputs: the rows a dump holds are fixed by
(n, A) alone and fit the 64 MB a dump may take; the files give every
coordinate back exactly; a plain run measures the headline only, honours
--steps, and dumps the coordinates the oracle computes for the same batch."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

EXTRAS = ("secondary", "regions", "regions_entry_point", "host_path", "config4", "config4_device_set",
          "cpu_baseline", "cpu_per_object", "allgather")


def test_full_and_dump_are_off_by_default():
    import bench
    args = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert args.full is False and args.dump_outputs is None and args.steps == 7 and args.warmup == 2
    args = bench.parse_args(["--full", "--dump-outputs", "d"])
    assert args.full is True and args.dump_outputs == "d"


@pytest.mark.parametrize("n,A", [(1, 17), (5000, 17), (10_000_000, 17), (50_000_000, 17), (200_000, 1001)])
def test_dump_rows_are_fixed_and_fit(n, A):
    import bench
    rows = bench.dump_rows(n, A)
    assert rows.dtype == np.int64 and np.array_equal(rows, bench.dump_rows(n, A))
    assert np.all(np.diff(rows) > 0) and rows[0] == 0 and rows[-1] == n - 1
    # <name>.npy float64, <name>_bytes.npy 8 x float32, <name>_rows.npy float64
    assert len(rows) * (8 + A * (8 + 32)) <= 64 * 10**6
    if n * (8 + A * 40) <= bench.DUMP_BUDGET_BYTES:
        assert len(rows) == n
    else:  # a sample uses the budget: not a token handful of rows
        assert len(rows) * (8 + A * 40) > bench.DUMP_BUDGET_BYTES // 2


def test_written_outputs_are_exact(tmp_path):
    import bench
    rng = np.random.default_rng(3)
    v = rng.integers(0, 2**64, size=(300, 5), dtype=np.uint64)
    v[0, 0], v[0, 1], v[0, 2] = 0, 2**64 - 1, 2**53 + 1  # 2^53 + 1: not a float64
    rows = np.arange(300, dtype=np.int64) * 7
    bench.write_outputs(str(tmp_path / "d"), "coords", rows, v)
    assert sorted(os.listdir(tmp_path / "d")) == ["coords.npy", "coords_bytes.npy", "coords_rows.npy"]
    f = np.load(tmp_path / "d" / "coords.npy")
    b = np.load(tmp_path / "d" / "coords_bytes.npy")
    r = np.load(tmp_path / "d" / "coords_rows.npy")
    assert f.dtype == np.float64 and b.dtype == np.float32 and r.dtype == np.float64
    assert f.shape == (300, 5) and b.shape == (300, 5, 8)
    assert np.array_equal(f, v.astype(np.float64)) and np.array_equal(r, rows)
    back = np.zeros(v.shape, np.uint64)
    for k in range(8):  # most significant byte first
        back = (back << np.uint64(8)) | b[:, :, k].astype(np.uint64)
    assert np.array_equal(back, v)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg,n", [("cfg3a", 4099), ("cfg3b", 80_011)])
def test_plain_run_dumps_the_oracles_coordinates(oracle, tmp_path, capsys, cfg, n):
    """One plain run in this process: the line's headline keys, none of the
    --full extras, `steps` timed steps; the dump equals the oracle's coordinates
    of the same seeded batch (all rows at 4099 objects, a sample at 80 011)."""
    import torch

    import bench
    from hyperdex_amd import synth
    out = str(tmp_path / "dump")
    args = bench.parse_args(["--gpus", "1", "--steps", "3", "--warmup", "1", "--warmup-ms", "0",
                             "--config", cfg, "--objects", str(n), "--dump-outputs", out])
    assert bench.run_rank(args) == 0
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    res = json.loads(lines[0])
    assert res["steps"] == 3 and res["warmup"] == 1 and res["unit"] == "GiB/s" and res["dtype"] == "u8"
    assert res["higher_is_better"] is True and res["value"] > 0 and res["ms_per_step"] > 0
    assert res["metric"].startswith("hashed GiB/s")
    assert not [k for k in EXTRAS if k in res] and "stream_probe" not in res["roofline"]
    # value is the payload over ms_per_step
    assert res["value"] == pytest.approx(
        res["config"]["payload_bytes_per_gpu"] / (res["ms_per_step"] / 1e3) / 2**30,
        rel=1e-3 + 5e-5 / res["ms_per_step"])  # both figures are rounded in the line

    dev = torch.device("cuda", 0)
    types, blob, base, lens = synth.make_batch_device(cfg, n, device=dev)
    want, err = oracle.hash_batch(types, blob.cpu().numpy(), base.cpu().numpy().view(np.uint64),
                                  lens.cpu().numpy().view(np.uint32))
    assert err == 0
    want = want.reshape(n, len(types))
    rows = np.load(os.path.join(out, "coords_rows.npy")).astype(np.int64)
    assert np.array_equal(rows, bench.dump_rows(n, len(types)))
    assert (len(rows) == n) == (n == 4099)
    b = np.load(os.path.join(out, "coords_bytes.npy")).astype(np.uint64)
    got = np.zeros(b.shape[:2], np.uint64)
    for k in range(8):
        got = (got << np.uint64(8)) | b[:, :, k]
    assert np.array_equal(got, want[rows])
    assert np.array_equal(np.load(os.path.join(out, "coords.npy")), want[rows].astype(np.float64))
