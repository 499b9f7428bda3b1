#!/usr/bin/env python3
"""Rate of the device attribute checks (hdx_check_encoded_device) on one MI355X: config 3b, key
column, with the index-entry plan call (hdx_index_entries_plan_device, m = 2: the parent commit's
code doing the same walk) and the reindex sweep (hdx_hash_encoded_device) timed on the same buffers
in the same process as yardsticks.  Needs a gfx950 device; there is no CPU substitute.

Check lists (config 3b: attribute 0 the 64-byte key, 1-10 strings of 0-195 random bytes, 11-13
INT64, 14-16 FLOAT):
  a   two numeric checks: attribute 11 >= 0 and attribute 14 >= 0.0;
  b   attribute 2 <= "\\x80" (about half of the objects pass it), then the key EQUALS object 0's
      key (random keys: one object passes the list);
  c   b's first check alone: about half of the objects match, the compaction's full load.
Each is timed without match (the check kernel alone) and with match (plus the counts' scan and
the compaction).  Every repetition runs all of them once, in rotation (interleaved), each between
two device events; the medians go to profiles/r8/check_encoded.jsonl, one JSON object per line.
"""
import argparse
import json
import os
import statistics
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "r8", "check_encoded.jsonl")


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
    from hyperdex_amd import datatypes as dt, synth
    from hyperdex_amd._lib import check, lib
    from hyperdex_amd.checks import AttributeCheck, _checks
    from hyperdex_amd.index import IndexSpec, _specs

    if not torch.cuda.is_available():
        raise SystemExit("check_encoded_rate: needs a gfx950 device (nothing is measured without one)")
    dev = torch.device("cuda", 0)
    n = args.objects
    types, keys, key_off, key_len, vals, val_off, val_len = synth.make_encoded_device("cfg3b", n, device=dev,
                                                                                     layout="keycol")
    A = len(types)
    t32 = types.astype("uint32")
    stream = torch.cuda.current_stream(dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    coords = torch.empty((n, A), dtype=torch.int64, device=dev)
    key_bytes, val_bytes = int(key_len.sum().item()), int(val_len.to(torch.int64).sum().item())
    key0 = bytes(keys[:int(key_len[0].item())].cpu().numpy().tobytes())

    S, I, F = dt.HYPERDATATYPE_STRING, dt.HYPERDATATYPE_INT64, dt.HYPERDATATYPE_FLOAT
    GE, LE, EQ = dt.HYPERPREDICATE_GREATER_EQUAL, dt.HYPERPREDICATE_LESS_EQUAL, dt.HYPERPREDICATE_EQUALS
    half = AttributeCheck(2, b"\x80", S, LE)
    lists = {"a": [AttributeCheck(11, struct.pack("<q", 0), I, GE), AttributeCheck(14, struct.pack("<d", 0.0), F, GE)],
             "b": [half, AttributeCheck(0, key0, S, EQ)],
             "c": [half]}
    first_fail = torch.empty(n, dtype=torch.int32, device=dev)
    match = torch.empty(n, dtype=torch.int64, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    specs = [IndexSpec(a, b"i\x07" + bytes([k + 1])) for k, a in enumerate([2, 12])]
    cspecs, m = _specs(specs), len(specs)
    attr_off = torch.empty(n * m, dtype=torch.int32, device=dev)
    attr_len = torch.empty(n * m, dtype=torch.int32, device=dev)
    entry_off = torch.empty(n * m + 1, dtype=torch.int64, device=dev)

    def checks_call(name, with_match):
        cl = lists[name]
        arr = _checks(cl)

        def run():
            check(lib().hdx_check_encoded_device(
                t32.ctypes.data, A, keys.data_ptr(), key_off.data_ptr(), key_len.data_ptr(), vals.data_ptr(),
                val_off.data_ptr(), val_len.data_ptr(), n, arr, len(cl), first_fail.data_ptr(),
                match.data_ptr() if with_match else None, count.data_ptr() if with_match else None,
                status.data_ptr(), stream.cuda_stream))
        return run

    def plan():
        check(lib().hdx_index_entries_plan_device(t32.ctypes.data, A, key_len.data_ptr(), vals.data_ptr(),
                                                  val_off.data_ptr(), val_len.data_ptr(), n, cspecs, m,
                                                  attr_off.data_ptr(), attr_len.data_ptr(), entry_off.data_ptr(),
                                                  status.data_ptr(), stream.cuda_stream))

    def sweep():
        hdx.hash_encoded(types, keys, key_off, key_len, vals, val_off, val_len, coords=coords, status=status)

    steps = [("check_%s%s" % (name, "_match" if wm else ""), checks_call(name, wm))
             for name in ("a", "b", "c") for wm in (False, True)] + [("plan_m2", plan), ("sweep", sweep)]
    passing = {}
    for name in lists:  # what passes each list
        checks_call(name, True)()
        torch.cuda.synchronize()
        passing[name] = int(count.item())
    times = {name: [] for name, _ in steps}
    for rep in range(args.warmup + args.reps):
        order = steps[rep % len(steps):] + steps[:rep % len(steps)]  # rotate: no step always follows the same one
        marks = []
        for name, fn in order:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            marks.append((name, a, b))
        torch.cuda.synchronize()
        if rep >= args.warmup:
            for name, a, b in marks:
                times[name].append(a.elapsed_time(b))
    assert int(status.item()) == 0, "status %#x" % int(status.item())

    plan_ms = statistics.median(times["plan_m2"])
    rows = []
    for name, _ in steps:
        ts = times[name]
        med = statistics.median(ts)
        row = {"what": "yardstick" if name in ("plan_m2", "sweep") else "call", "phase": name, "objects": n,
               "reps": args.reps, "median_ms": med, "min_ms": min(ts), "max_ms": max(ts),
               "objects_per_s": n / med * 1e3, "vs_plan": med / plan_ms, "key_bytes": key_bytes,
               "value_bytes": val_bytes}
        if name.startswith("check_"):
            row["matching"] = passing[name[6]]
        rows.append(row)
    for r in rows:
        print(json.dumps(r, sort_keys=True))
    if not args.no_write:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
