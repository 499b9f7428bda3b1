#!/usr/bin/env python3
"""Rate of REGEX checks through a compiled list (hdx_checks_encoded_device) on one MI355X: config 3b,
key column, 10 M stored objects, one REGEX check on attribute 2 (a string of 0-195 random bytes).
Needs a gfx950 device; there is no CPU substitute.

Timed, each without and with the match list:
  abc        an unanchored literal: every start position stays alive, the whole text is scanned;
  ^abc       an anchored prefix: a lane leaves at the first byte that is not 'a';
  a.*b.*c$   two stars and END: scans to the text's end;
  equals     the baseline, existing code: the same batch through hdx_check_encoded_device with one
             EQUALS check on the same attribute (object 0's value).
Every repetition runs all of them once, in rotation (interleaved), each between two device events.
`scanned_bytes_per_object` is the matcher's own count of text bytes stepped over (early accept and
dead anchored states end a scan), worked out on the host over the first --sample objects with the
item grammar restated below; `text_bytes_per_object` is the attribute's mean length over the batch.
The medians go to profiles/r10/regex_check.jsonl, one JSON object per line.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "r10", "regex_check.jsonl")
ATTR = 2
PATTERNS = {"abc": b"abc", "^abc": b"^abc", "a.*b.*c$": b"a.*b.*c$"}


def scanned(pattern, text):
    """(bytes stepped over, matched) of the set-of-positions matcher (include/hdxhash.h's grammar)."""
    anchored, end, items = pattern[:1] == b"^", False, []
    i = 1 if anchored else 0
    while i < len(pattern):
        ch = pattern[i]
        if ch == 0x5c:
            items.append(("lit", pattern[i + 1]) if i + 1 < len(pattern) else ("dead", 0))
            i += 2
        elif i + 1 < len(pattern) and pattern[i + 1] == 0x2a:
            items.append(("starany", 0) if ch == 0x2e else ("star", ch))
            i += 2
        elif ch == 0x24 and i + 1 == len(pattern):
            end, i = True, i + 1
        else:
            items.append(("any", 0) if ch == 0x2e else ("lit", ch))
            i += 1
    m = len(items)
    star = sum(1 << j for j, (k, _) in enumerate(items) if k.startswith("star"))
    cls = [sum(1 << j for j, (k, b) in enumerate(items) if k in ("any", "starany") or (k != "dead" and b == c))
           for c in range(256)]

    def close(s):
        return s | (((s & star) + star) ^ star)
    s = close(1)
    if not end and s >> m & 1:
        return 0, True
    for n, c in enumerate(text):
        adv = s & cls[c]
        s = close(((adv & ~star) << 1) | (adv & star) | (0 if anchored else 1))
        if not end and s >> m & 1:
            return n + 1, True
        if not s:
            return n + 1, False
    return len(text), bool(s >> m & 1)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--objects", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sample", type=int, default=4096)
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--no-write", action="store_true")
    args = ap.parse_args()

    import torch

    from hyperdex_amd import datatypes as dt, synth
    from hyperdex_amd._lib import check, lib
    from hyperdex_amd.checks import AttributeCheck, CompiledChecks, _checks
    from hyperdex_amd.index import IndexSpec, _specs

    if not torch.cuda.is_available():
        raise SystemExit("regex_check_rate: needs a gfx950 device (nothing is measured without one)")
    dev = torch.device("cuda", 0)
    n = args.objects
    types, keys, key_off, key_len, vals, val_off, val_len = synth.make_encoded_device("cfg3b", n, device=dev,
                                                                                     layout="keycol")
    A = len(types)
    t32 = types.astype("uint32")
    stream = torch.cuda.current_stream(dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    first_fail = torch.empty(n, dtype=torch.int32, device=dev)
    match = torch.empty(n, dtype=torch.int64, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    objs = [x.data_ptr() for x in (keys, key_off, key_len, vals, val_off, val_len)]

    # where attribute ATTR lies in each value: the index-entry plan's walk
    cspecs = _specs([IndexSpec(ATTR, b"i")])
    attr_off = torch.empty(n, dtype=torch.int32, device=dev)
    attr_len = torch.empty(n, dtype=torch.int32, device=dev)
    entry_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    check(lib().hdx_index_entries_plan_device(t32.ctypes.data, A, key_len.data_ptr(), vals.data_ptr(), val_off.data_ptr(),
                                              val_len.data_ptr(), n, cspecs, 1, attr_off.data_ptr(), attr_len.data_ptr(),
                                              entry_off.data_ptr(), status.data_ptr(), stream.cuda_stream))
    torch.cuda.synchronize()
    text_bytes = float(attr_len.to(torch.int64).sum().item()) / n
    k = min(args.sample, n)
    lo, hi = int(val_off[0].item()), int(val_off[k - 1].item()) + int(val_len[k - 1].item())
    blob = vals[lo:hi].cpu().numpy().tobytes()
    vo, ao, al = (x[:k].cpu().numpy() for x in (val_off, attr_off, attr_len))
    texts = [blob[int(vo[i]) - lo + int(ao[i]):int(vo[i]) - lo + int(ao[i]) + int(al[i])] for i in range(k)]
    del attr_off, attr_len, entry_off

    S = dt.HYPERDATATYPE_STRING
    compiled = {name: CompiledChecks(types, [AttributeCheck(ATTR, p, S, dt.HYPERPREDICATE_REGEX)])
                for name, p in PATTERNS.items()}
    equals = _checks([AttributeCheck(ATTR, texts[0], S, dt.HYPERPREDICATE_EQUALS)])

    def regex_call(name, with_match):
        h = compiled[name]._handle()

        def run():
            check(lib().hdx_checks_encoded_device(h, *objs, n, first_fail.data_ptr(),
                                                  match.data_ptr() if with_match else None,
                                                  count.data_ptr() if with_match else None, status.data_ptr(),
                                                  stream.cuda_stream))
        return run

    def equals_call(with_match):
        def run():
            check(lib().hdx_check_encoded_device(t32.ctypes.data, A, *objs, n, equals, 1, first_fail.data_ptr(),
                                                 match.data_ptr() if with_match else None,
                                                 count.data_ptr() if with_match else None, status.data_ptr(),
                                                 stream.cuda_stream))
        return run

    steps = [("%s%s" % (name, "_match" if wm else ""), name, regex_call(name, wm))
             for name in PATTERNS for wm in (False, True)]
    steps += [("equals%s" % ("_match" if wm else ""), "equals", equals_call(wm)) for wm in (False, True)]
    passing = {}
    for phase, name, fn in steps:
        if phase.endswith("_match"):
            fn()
            torch.cuda.synchronize()
            passing[name] = int(count.item())
    times = {phase: [] for phase, _, _ in steps}
    for rep in range(args.warmup + args.reps):
        order = steps[rep % len(steps):] + steps[:rep % len(steps)]  # rotate: no step always follows the same one
        marks = []
        for phase, _, fn in order:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            marks.append((phase, a, b))
        torch.cuda.synchronize()
        if rep >= args.warmup:
            for phase, a, b in marks:
                times[phase].append(a.elapsed_time(b))
    assert int(status.item()) == 0, "status %#x" % int(status.item())

    base = {wm: statistics.median(times["equals%s" % ("_match" if wm else "")]) for wm in (False, True)}
    rows = []
    for phase, name, _ in steps:
        ts = times[phase]
        med = statistics.median(ts)
        row = {"what": "baseline" if name == "equals" else "call", "phase": phase, "objects": n, "reps": args.reps,
               "median_ms": med, "min_ms": min(ts), "max_ms": max(ts), "objects_per_s": n / med * 1e3,
               "vs_equals": med / base[phase.endswith("_match")], "matching": passing[name],
               "text_bytes_per_object": text_bytes}
        if name in PATTERNS:
            sc = [scanned(PATTERNS[name], t) for t in texts]
            row["scanned_bytes_per_object"] = sum(x for x, _ in sc) / k
            row["sample"] = k
            row["sample_matching"] = sum(m for _, m in sc)
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
