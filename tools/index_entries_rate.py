#!/usr/bin/env python3
"""Rate of the device index-entry builder (hdx_index_entries_plan_device / _fill_device) on one
MI355X: config 3b, key column, m = 2 (attributes 2 and 12) and m = 6, with the reindex sweep
(hdx_hash_encoded_device, the parent commit's kernel over the same input bytes) timed in the same
process as a yardstick.  Needs a gfx950 device; there is no CPU substitute.

Every repetition runs plan(m=2), fill(m=2), plan(m=6), fill(m=6) and the sweep once, in rotation
(interleaved), each between two device events; the medians go to profiles/r7/index_entries.jsonl,
one JSON object per line.  "plan" is the whole plan call: the walk and the prefix sum.  Their split
comes from a kernel trace taken in a run of its own:

    python tools/index_entries_rate.py                                   # the timed run
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/index_entries_rate.py --reps 3 --no-write
    python tools/index_entries_rate.py --kernel-stats DIR                # appends the per-kernel rows

Bytes are what the algorithm needs, computed from the shapes (not counters):
  plan  reads  the offsets and lengths (16 B per object) and each value's header and length
               prefixes (10 + 4 (A - 1) B; the 64 B lines they lie in span most of the value, so the
               values' total is reported beside it as bytes_spanned);
        writes 16 B of descriptors and size per entry;
  scan  reads  the sizes twice, writes them once (reduce-then-scan): 24 B per entry;
  fill  reads  the offsets, descriptors and lengths (16 B per entry + 28 B per object) and the source
               bytes of every entry (its key and its attribute);
        writes the entries.
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "r7", "index_entries.jsonl")
KERNELS = {"walk": "index_plan_kernel", "scan_sums": "index_scan_sums_kernel", "scan_block": "index_scan_block_kernel",
           "fill": "index_fill_kernel"}


def kernel_rows(directory, n):
    """Per-kernel average times of the index-entry kernels from rocprofv3's *kernel_stats.csv."""
    paths = glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True)
    if not paths:
        raise SystemExit("no *kernel_stats.csv under %s" % directory)
    rows = []
    for path in sorted(paths):
        for r in csv.DictReader(open(path)):
            for phase, sym in KERNELS.items():
                if sym in r["Name"]:
                    rows.append({"what": "kernel_trace", "phase": phase, "kernel": r["Name"], "calls": int(r["Calls"]),
                                 "avg_ms": float(r["AverageNs"]) / 1e6, "min_ms": float(r["MinNs"]) / 1e6,
                                 "max_ms": float(r["MaxNs"]) / 1e6, "objects": n,
                                 "note": "averaged over the m = 2 and m = 6 calls of the traced run",
                                 "source": os.path.relpath(path, directory)})
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--objects", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--no-write", action="store_true")
    ap.add_argument("--kernel-stats", metavar="DIR", help="append per-kernel rows from a rocprofv3 --stats run")
    args = ap.parse_args()
    if args.kernel_stats:
        rows = kernel_rows(args.kernel_stats, args.objects)
        with open(args.out, "a") as f:
            for r in rows:
                f.write(json.dumps(r, sort_keys=True) + "\n")
                print(json.dumps(r, sort_keys=True))
        return

    import torch

    import hyperdex_amd as hdx
    from hyperdex_amd import synth
    from hyperdex_amd._lib import check, lib
    from hyperdex_amd.index import IndexSpec, _specs

    if not torch.cuda.is_available():
        raise SystemExit("index_entries_rate: needs a gfx950 device (nothing is measured without one)")
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

    cases = {}
    for name, attrs in (("m2", [2, 12]), ("m6", [2, 3, 12, 13, 15, 16])):
        specs = [IndexSpec(a, b"i\x07" + bytes([k + 1])) for k, a in enumerate(attrs)]
        m = len(specs)
        c = {"specs": specs, "cspecs": _specs(specs), "m": m,
             "attr_off": torch.empty(n * m, dtype=torch.int32, device=dev),
             "attr_len": torch.empty(n * m, dtype=torch.int32, device=dev),
             "entry_off": torch.empty(n * m + 1, dtype=torch.int64, device=dev)}
        cases[name] = c

    def plan(c):
        check(lib().hdx_index_entries_plan_device(t32.ctypes.data, A, key_len.data_ptr(), vals.data_ptr(),
                                                  val_off.data_ptr(), val_len.data_ptr(), n, c["cspecs"], c["m"],
                                                  c["attr_off"].data_ptr(), c["attr_len"].data_ptr(),
                                                  c["entry_off"].data_ptr(), status.data_ptr(), stream.cuda_stream))

    def fill(c):
        hdx.index_entries_fill(types, keys, key_off, key_len, vals, val_off, c["specs"], c["attr_off"], c["attr_len"],
                               c["entry_off"], c["entries"], status=status)

    def sweep(_):
        hdx.hash_encoded(types, keys, key_off, key_len, vals, val_off, val_len, coords=coords, status=status)

    for c in cases.values():  # the first plan sizes the output; it stays allocated
        plan(c)
        torch.cuda.synchronize()
        c["total"] = int(c["entry_off"][-1].item())
        c["entries"] = torch.empty(c["total"], dtype=torch.uint8, device=dev)
        c["src"] = int(c["attr_len"].to(torch.int64).sum().item()) + c["m"] * key_bytes
    steps = [("m2", "plan", plan), ("m2", "fill", fill), ("m6", "plan", plan), ("m6", "fill", fill),
             ("-", "sweep", sweep)]
    times = {(cn, ph): [] for cn, ph, _ in steps}
    for rep in range(args.warmup + args.reps):
        order = steps[rep % len(steps):] + steps[:rep % len(steps)]  # rotate: no phase always follows the same one
        marks = []
        for cn, ph, fn in order:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn(cases.get(cn))
            b.record()
            marks.append((cn, ph, a, b))
        torch.cuda.synchronize()
        if rep >= args.warmup:
            for cn, ph, a, b in marks:
                times[(cn, ph)].append(a.elapsed_time(b))
    assert int(status.item()) == 0, "status %#x" % int(status.item())

    rows = []
    sweep_ms = statistics.median(times[("-", "sweep")])
    sweep_read = 20 * n + key_bytes + val_bytes
    rows.append({"what": "yardstick", "phase": "hdx_hash_encoded_device", "objects": n, "reps": args.reps,
                 "median_ms": sweep_ms, "min_ms": min(times[("-", "sweep")]), "max_ms": max(times[("-", "sweep")]),
                 "read_bytes": sweep_read, "write_bytes": 8 * n * A,
                 "tb_per_s": (sweep_read + 8 * n * A) / sweep_ms / 1e9})
    for cn in ("m2", "m6"):
        c = cases[cn]
        m, E = c["m"], n * c["m"]
        acct = {"plan": (16 * n + n * (10 + 4 * (A - 1)) + 16 * E, 16 * E + 8 * E),  # walk + scan (reads, writes)
                "fill": (16 * E + 28 * n + c["src"], c["total"])}
        for ph in ("plan", "fill"):
            ts = times[(cn, ph)]
            rd, wr = acct[ph]
            med = statistics.median(ts)
            row = {"what": "call", "phase": ph, "m": m, "objects": n, "reps": args.reps, "median_ms": med,
                   "min_ms": min(ts), "max_ms": max(ts), "read_bytes": rd, "write_bytes": wr,
                   "tb_per_s": (rd + wr) / med / 1e9, "entries_bytes": c["total"],
                   "vs_sweep": med / sweep_ms}
            if ph == "plan":
                row["bytes_spanned"] = val_bytes + 16 * n
                row["tb_per_s_spanned"] = (val_bytes + 16 * n + wr) / med / 1e9
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
