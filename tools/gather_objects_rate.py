#!/usr/bin/env python3
"""Rate of the object gather (hdx_gather_objects_plan_device / _fill_device) on one MI355X, with
three yardsticks timed on the same buffers in the same process.  Needs a gfx950 device; there is no
CPU substitute.

Shapes (key column):
  cfg3b_match   config 3b, the match of attribute 2 <= "\\x80" (check_encoded_rate.py's list c, about
                half of the objects), keys and values;
  cfg3b_top     the same store, `top` of a sorted search by attribute 11 with limit 1024;
  cfg2_keys     config 2, the match of attribute 1 >= 0, KEYS only (64-byte records).
Steps per shape:
  plan          hdx_gather_objects_plan_device (sizes, scan);
  fill          hdx_gather_objects_fill_device, the tile-owned kernel;
  by_extents    yardstick 1: hdxdbg_gather_objects_fill_by_extents (debug library), the record-major
                copy kernel over the same plan;
  d2d           yardstick 2: a device-to-device copy of as many bytes, the floor;
  check_match   yardstick 3: hdx_check_encoded_device with match, the call that makes the list.
Every repetition runs all steps once, in rotation (interleaved), each between two device events;
the medians and ranges go to profiles/r11/gather_objects.jsonl, one JSON object per line.  Before
anything is timed the two fills' outputs are compared byte for byte.
"""
import argparse
import json
import os
import statistics
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "r11", "gather_objects.jsonl")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--objects", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--no-write", action="store_true")
    args = ap.parse_args()

    import torch

    import hyperdex_amd as hdx
    from hyperdex_amd import _lib, datatypes as dt, gather, synth
    from hyperdex_amd._lib import check, lib
    from hyperdex_amd.checks import AttributeCheck, _checks
    from hyperdex_amd.sorting import SortSpec

    if not torch.cuda.is_available():
        raise SystemExit("gather_objects_rate: needs a gfx950 device (nothing is measured without one)")
    dev = torch.device("cuda", 0)
    n = args.objects
    stream = torch.cuda.current_stream(dev)
    S, I = dt.HYPERDATATYPE_STRING, dt.HYPERDATATYPE_INT64
    dbg_fill = _lib.debug_lib().hdxdbg_gather_objects_fill_by_extents
    rows = []

    def shape(name, cfg, checks, what, limit=None):
        types, keys, key_off, key_len, vals, val_off, val_len = synth.make_encoded_device(cfg, n, device=dev,
                                                                                         layout="keycol")
        store = (keys, key_off, key_len, vals, val_off, val_len)
        t32, A = types.astype("uint32"), len(types)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        if limit is None:
            _, idx = hdx.check_encoded(types, *store, checks, status=status)
        else:
            _, idx = hdx.sorted_search(types, *store, checks, SortSpec(11), limit, want_first_fail=False,
                                       status=status)
        idx = idx.contiguous()
        cap = idx.numel()
        count = torch.tensor([cap], dtype=torch.int64, device=dev)
        rec_off, _ = hdx.gather_objects_plan(key_len, val_len, idx, count, what, status=status)
        torch.cuda.synchronize()
        total = int(rec_off[-1].item())
        out = torch.empty(total, dtype=torch.uint8, device=dev)
        other = torch.empty(total, dtype=torch.uint8, device=dev)
        rec_key_len = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
        first_fail = torch.empty(n, dtype=torch.int32, device=dev)
        match = torch.empty(n, dtype=torch.int64, device=dev)
        match_count = torch.zeros(1, dtype=torch.int64, device=dev)
        arr = _checks(checks)

        def plan():
            check(lib().hdx_gather_objects_plan_device(key_len.data_ptr(), val_len.data_ptr(), n, idx.data_ptr(),
                                                       count.data_ptr(), cap, what, rec_off.data_ptr(),
                                                       rec_key_len.data_ptr(), status.data_ptr(), stream.cuda_stream))

        def fill():
            gather.gather_objects_fill(*store, idx, count, what, rec_off, out, status=status)

        def by_extents():
            gather._fill(dbg_fill, *store, idx, count, what, rec_off, other, status, None)

        def d2d():
            other.copy_(out)

        def check_match():
            check(lib().hdx_check_encoded_device(
                t32.ctypes.data, A, keys.data_ptr(), key_off.data_ptr(), key_len.data_ptr(), vals.data_ptr(),
                val_off.data_ptr(), val_len.data_ptr(), n, arr, len(checks), first_fail.data_ptr(), match.data_ptr(),
                match_count.data_ptr(), status.data_ptr(), stream.cuda_stream))

        fill()
        by_extents()
        torch.cuda.synchronize()
        assert torch.equal(out, other), "%s: the two fills differ" % name
        steps = [("plan", plan), ("fill", fill), ("by_extents", by_extents), ("d2d", d2d),
                 ("check_match", check_match)]
        times = {s: [] for s, _ in steps}
        for rep in range(args.warmup + args.reps):
            order = steps[rep % len(steps):] + steps[:rep % len(steps)]  # rotate: no step always follows the same one
            marks = []
            for s, fn in order:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                marks.append((s, a, b))
            torch.cuda.synchronize()
            if rep >= args.warmup:
                for s, a, b in marks:
                    times[s].append(a.elapsed_time(b))
        assert int(status.item()) == 0, "status %#x" % int(status.item())
        med = {s: statistics.median(ts) for s, ts in times.items()}
        for s, _ in steps:
            ts = times[s]
            row = {"shape": name, "step": s, "what": "call" if s in ("plan", "fill") else "yardstick", "objects": n,
                   "records": cap, "bytes": total, "reps": args.reps, "median_ms": med[s], "min_ms": min(ts),
                   "max_ms": max(ts)}
            if s in ("fill", "by_extents", "d2d"):
                row["gb_per_s_out"] = total / med[s] / 1e6
                row["vs_by_extents"] = med[s] / med["by_extents"]
                row["vs_d2d"] = med[s] / med["d2d"]
            rows.append(row)
            print(json.dumps(row, sort_keys=True), flush=True)

    half = AttributeCheck(2, b"\x80", S, dt.HYPERPREDICATE_LESS_EQUAL)
    shape("cfg3b_match", "cfg3b", [half], gather.KEYS | gather.VALUES)
    torch.cuda.empty_cache()
    shape("cfg3b_top", "cfg3b", [half], gather.KEYS | gather.VALUES, limit=1024)
    torch.cuda.empty_cache()
    shape("cfg2_keys", "cfg2", [AttributeCheck(1, struct.pack("<q", 0), I, dt.HYPERPREDICATE_GREATER_EQUAL)],
          gather.KEYS)
    if not args.no_write:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
