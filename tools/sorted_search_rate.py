#!/usr/bin/env python3
"""Rate of the device sorted search (hdx_sorted_search_device) on one MI355X: config 3b, key column,
10 M objects, with hdx_check_encoded_device with match (the parent commit's code doing the same walk)
timed on the same buffers in the same process as the yardstick.  Needs a gfx950 device; there is no
CPU substitute.

The checks are case (c) of tools/check_encoded_rate.py (attribute 2 <= "\\x80": about half of the
objects match).  The matches are sorted by an INT64 attribute (11) and by a STRING attribute (3: 0-195
random bytes), with limit 100 and 1024 and both keeps.  Every repetition runs all of them once, in
rotation (interleaved), each between two device events; the medians go to
profiles/r9/sorted_search.jsonl, one JSON object per line.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "r9", "sorted_search.jsonl")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--objects", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--no-write", action="store_true")
    args = ap.parse_args()

    import torch

    from hyperdex_amd import datatypes as dt, synth
    from hyperdex_amd._lib import check, lib
    from hyperdex_amd.checks import AttributeCheck, _checks
    from hyperdex_amd.sorting import KEEP_LARGEST, KEEP_SMALLEST, SortSpec

    if not torch.cuda.is_available():
        raise SystemExit("sorted_search_rate: needs a gfx950 device (nothing is measured without one)")
    dev = torch.device("cuda", 0)
    n = args.objects
    types, keys, key_off, key_len, vals, val_off, val_len = synth.make_encoded_device("cfg3b", n, device=dev,
                                                                                     layout="keycol")
    A = len(types)
    t32 = types.astype("uint32")
    stream = torch.cuda.current_stream(dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    key_bytes, val_bytes = int(key_len.sum().item()), int(val_len.to(torch.int64).sum().item())
    cl = [AttributeCheck(2, b"\x80", dt.HYPERDATATYPE_STRING, dt.HYPERPREDICATE_LESS_EQUAL)]
    arr = _checks(cl)
    first_fail = torch.empty(n, dtype=torch.int32, device=dev)
    match = torch.empty(n, dtype=torch.int64, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    top = torch.empty(1024, dtype=torch.int64, device=dev)
    top_count = torch.zeros(1, dtype=torch.int64, device=dev)
    objects = (keys.data_ptr(), key_off.data_ptr(), key_len.data_ptr(), vals.data_ptr(), val_off.data_ptr(),
               val_len.data_ptr())

    def yardstick():
        check(lib().hdx_check_encoded_device(t32.ctypes.data, A, *objects, n, arr, len(cl), first_fail.data_ptr(),
                                             match.data_ptr(), count.data_ptr(), status.data_ptr(), stream.cuda_stream))

    def sorted_call(attr, keep, limit):
        spec = SortSpec(attr, keep, 0)._c()

        def run():
            check(lib().hdx_sorted_search_device(t32.ctypes.data, A, *objects, n, arr, len(cl), ctypes.byref(spec),
                                                 limit, first_fail.data_ptr(), top.data_ptr(), top_count.data_ptr(),
                                                 status.data_ptr(), stream.cuda_stream))
        return run

    steps = [("check_c_match", yardstick)]
    for kind, attr in (("int64", 11), ("string", 3)):
        for keep, kname in ((KEEP_SMALLEST, "smallest"), (KEEP_LARGEST, "largest")):
            for limit in (100, 1024):
                steps.append(("sorted_%s_%s_%d" % (kind, kname, limit), sorted_call(attr, keep, limit)))
    kept = {}
    for name, fn in steps:  # what each call keeps
        fn()
        torch.cuda.synchronize()
        kept[name] = int(count.item()) if name == "check_c_match" else int(top_count.item())
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

    yard_ms = statistics.median(times["check_c_match"])
    rows = []
    for name, _ in steps:
        ts = times[name]
        med = statistics.median(ts)
        rows.append({"what": "yardstick" if name == "check_c_match" else "call", "phase": name, "objects": n,
                     "reps": args.reps, "median_ms": med, "min_ms": min(ts), "max_ms": max(ts),
                     "objects_per_s": n / med * 1e3, "vs_check_match": med / yard_ms, "key_bytes": key_bytes,
                     "value_bytes": val_bytes, "matching": kept["check_c_match"],
                     "kept": kept[name] if name != "check_c_match" else None})
    for r in rows:
        print(json.dumps(r, sort_keys=True))
    if not args.no_write:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
