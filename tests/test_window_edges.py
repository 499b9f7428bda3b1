"""The window decisions of the two wave-staged kernels, pinned at their edges.

hash_wstage_kernel (hdx_wstage.h) and hash_sweep_wstage_kernel (hdx_wsweep.h)
decide per wave whether a group of objects is hashed from an LDS window or
from global memory, by exact comparisons against the window geometry.  The
other tests draw object sizes from synth's random rules, where a group whose
span ends on the window's last byte turns up by luck.  Here every comparison
gets groups built to land on both of its sides.

Three parts:

  * builders (BatchChain, SweepChain) that lay groups out one after another
    in one blob, each group's sizes computed from the absolute address it
    lands on (the device buffers start at data_ptr() % 16 == SHIFT), and from
    the geometry hashing.wave_geometry reports: no window size, object count
    or pad is written here;
  * a decision model (model_batch, model_sweep): the kernels' comparisons
    restated in plain Python.  It is the reference for WHICH PATH a group
    takes; the CPU tests assert with it that the case lists hold a group on
    each side of every boundary, so a case list that stops covering one
    fails there and not silently on the GPU;
  * the GPU tests: every launch compared bit for bit with the oracle
    (coordinates, versions, status), on the product batch form, its non-NUM2
    instantiation (debug 212 on a schema with a timestamp and a non-hashable
    attribute), the fused regions form, and the sweep's NUM2 / non-NUM2 forms.

A launch over a prefix of a chain makes any group the launch's last one, so
the "last group" cases cost a launch each but no blob of their own.
"""
import contextlib
import functools

import numpy as np
import pytest

import hyperdex_amd as hdx
from hyperdex_amd import _lib, synth
from hyperdex_amd import datatypes as dt

S, I, F = dt.HYPERDATATYPE_STRING, dt.HYPERDATATYPE_INT64, dt.HYPERDATATYPE_FLOAT
TS, LST = dt.TIMESTAMPS[0], dt.HYPERDATATYPE_LIST_STRING
FIXED8 = (I, F) + tuple(dt.TIMESTAMPS)
BADENC = 1 << _lib.HDX_E_BADENC

SHIFT = 5            # data_ptr() % 16 of every device byte buffer (asserted on allocation)
SHIFT_V = 11         # ... of the values' buffer when keys and values are two buffers
DELTAS = (-17, -16, -15, -1, 0, 1, 15, 16, 17)
LEADS = (0, 1, 15)
# a length in every CityHash regime and on each side of their borders
REGIMES = (0, 1, 3, 4, 7, 8, 16, 17, 32, 33, 64, 65, 128, 129, 193)
FIT = sorted({(l, d) for l in LEADS for d in DELTAS} | {(l, d) for l in range(16) for d in (0, 1)})


# ---- schemas -----------------------------------------------------------------------

def schema17(ends=S, num2=True):
    """17 attributes, mostly strings (the policy's wave-staged form): `ends`
    is the type of the first and the last; not num2: one timestamp and one
    non-hashable attribute, which the NUM2 instantiations do not take."""
    t = [S] * 17
    t[5], t[9] = I, F
    t[0] = t[16] = ends
    if not num2:
        t[6], t[7] = TS, LST
    return t


def schema_mixed(A, num2=True):
    """Strings, strings, int64, float, ...: fewer numerics than strings; not
    num2: with a timestamp (and, where there is room, a non-hashable attribute)."""
    t = [(S, S, I, F)[j % 4] for j in range(A)] if A > 2 else [S, I][:A]
    if not num2 and A == 2:
        t[1] = TS
    elif not num2:
        t[6], t[7] = TS, LST
    return t


def geometry(types, sweep=False, forced=False):
    with (_lib.debug_library(212) if forced else contextlib.nullcontext()):
        g = hdx.hashing.wave_geometry(types, sweep)
    assert g is not None, "the schema takes no wave-staged form"
    return g


# ---- the decision models -----------------------------------------------------------

def model_batch(base, sizes, K, WB, addr0):
    """describe_group's decisions for a launch over objects base[] / sizes[]
    whose blob starts at an address = addr0 mod 16: one dict per group."""
    n, out = len(base), []
    for o0 in range(0, n, K):
        nobj = min(K, n - o0)
        has_next = o0 + K < n
        b0 = int(base[o0])
        bnext = int(base[o0 + nobj]) if has_next else 0
        lead = (addr0 + b0) & 15
        early = has_next and bnext > b0 and lead + (bnext - b0) <= WB
        ends = [int(base[o0 + i]) + int(sizes[o0 + i]) for i in range(nobj)]
        nexts = [int(base[o0 + i + 1]) for i in range(nobj - 1)] + ([bnext] if has_next else [])
        breaks = [i for i, nb in enumerate(nexts) if ends[i] != nb]
        runs = not breaks
        bend = ends[-1]
        staged = runs and bend >= b0 and lead + (bend - b0) <= WB
        units = None
        if early:
            units = (lead + (bnext - b0) + 15) >> 4
        elif staged:
            units = (lead + (bend - b0) + 15) >> 4
        out.append(dict(o0=o0, nobj=nobj, has_next=has_next, b0=b0, bnext=bnext, bend=bend, lead=lead, early=early,
                        runs=runs, staged=staged, late=staged and not early, units=units, breaks=breaks,
                        gaps=[nexts[i] - ends[i] for i in breaks]))
    return out


def decodes(val, A):
    """decode_value: (ok, version) of one stored value."""
    if len(val) < 10 or int.from_bytes(val[8:10], "big") != A - 1:
        return False, 0
    pos = 10
    for _ in range(A - 1):
        if len(val) - pos < 4:
            return False, 0
        ln = int.from_bytes(val[pos:pos + 4], "big")
        pos += 4
        if ln > len(val) - pos:
            return False, 0
        pos += ln
    return True, int.from_bytes(val[:8], "big")


def model_sweep(koff, klen, voff, vlen, K, WB, KR, kaddr0, vaddr0, records):
    """hash_sweep_wstage_kernel's decisions: one dict per group; keys: "span"
    (one DMA), "units", "dwords" (the two gathers) or "global"; vin[i]: object
    i's value is walked and hashed from the window."""
    n, out = len(koff), []
    for o0 in range(0, n, K):
        nobj = min(K, n - o0)
        has_next = o0 + nobj < n
        ko = [int(x) for x in koff[o0:o0 + nobj]]
        kl = [int(x) for x in klen[o0:o0 + nobj]]
        vo = [int(x) for x in voff[o0:o0 + nobj]]
        vl = [int(x) for x in vlen[o0:o0 + nobj]]
        k0, v0 = ko[0], vo[0]
        klead = (kaddr0 + k0) & 15
        vlead = (vaddr0 + v0) & 15
        g = dict(o0=o0, nobj=nobj, has_next=has_next, klead=klead, rspan=False, rtotal=None, kU=0, td=None, ktotal=None)
        if records and all(vo[i] == ko[i] + kl[i] and (i + 1 >= nobj or ko[i + 1] == vo[i] + vl[i]) for i in range(nobj)):
            rend = vo[-1] + vl[-1]
            g["rtotal"] = rend - k0 + klead
            g["rspan"] = g["rtotal"] <= WB
        if g["rspan"]:
            keys, kreg = "span", 0
            vlead = klead + (v0 - k0)
            vheld = klead + (rend - k0)
        else:
            keys, kreg = None, 0
            if all(ko[i] + kl[i] == ko[i + 1] for i in range(nobj - 1)):
                kend = ko[-1] + kl[-1]
                g["ktotal"] = kend - k0 + klead
                if g["ktotal"] <= KR:
                    keys, kreg = "span", (klead + (kend - k0) + 15) & ~15
            if keys is None:
                ku = [(((kaddr0 + ko[i]) & 15) + kl[i] + 15) >> 4 for i in range(nobj)]
                g["kU"] = kU = max(ku)
                g["reach"] = [((kaddr0 + ko[i]) & 15) + kl[i] for i in range(nobj)]
                g["last_key_units"] = ku[-1]
                if kU and nobj * kU <= 64 and 16 * nobj * kU <= KR:
                    keys, kreg = "units", 16 * nobj * kU
            if keys is None:
                g["td"] = td = sum((((kaddr0 + ko[i]) & 3) + kl[i] + 3) >> 2 for i in range(nobj))
                g["kmod4"] = sorted({(kaddr0 + ko[i]) & 3 for i in range(nobj)})
                keys, kreg = ("dwords", (4 * td + 15) & ~15) if 4 * td <= KR else ("global", 0)
            vend = int(voff[o0 + nobj]) if has_next else 0
            g["vbefore"] = has_next and vend < v0
            vheld = min(vlead + (vend - v0), WB - kreg) if has_next and vend >= v0 else 0
        g.update(keys=keys, kreg=kreg, vlead=vlead, vheld=vheld, room=WB - kreg)
        g["vlen0"] = vl[0]
        g["vend"] = [vlead + (vo[i] - v0) + vl[i] for i in range(nobj)]
        g["vin"] = [vo[i] >= v0 and g["vend"][i] <= vheld for i in range(nobj)]
        out.append(g)
    return out


# ---- object sizes ------------------------------------------------------------------

def nonzero_bytes(rng, n):
    return rng.integers(1, 256, int(n), dtype=np.uint8).tobytes()


def group_lens(types, nobj, total, rng, first=None, last=None, empty=(), big=None):
    """Attribute lengths (nobj, A) that sum to `total`: numerics 8 bytes,
    strings of mixed regimes, one filler string in the middle taking the
    rest.  first / last: the length of the first object's first and the last
    object's last attribute (strings); empty: objects with every attribute
    empty; big = (object, bytes): that object's own size (total None)."""
    A = len(types)
    L = np.zeros((nobj, A), np.int64)
    for j, t in enumerate(types):
        if t in FIXED8:
            L[:, j] = 8
    for o in empty:
        L[o, :] = 0
    free = [(o, j) for o in range(nobj) for j in range(A) if types[j] not in FIXED8 and o not in empty]
    pinned = []
    if first is not None and types[0] not in FIXED8:
        L[0, 0] = first
        pinned.append((0, 0))
    if last is not None and types[-1] not in FIXED8:
        L[nobj - 1, A - 1] = last
        pinned.append((nobj - 1, A - 1))
    free = [s for s in free if s not in pinned]
    assert free, "no string to take the remainder"
    if big is not None:
        rows = [s for s in free if s[0] == big[0]]
        filler = rows[len(rows) // 2]
        others = [s for s in free if s != filler]
        for s in others:
            L[s] = rng.integers(0, 40)
        L[filler] = big[1] - L[big[0]].sum()
        assert L[filler] >= 0 and total is None
        return L
    filler = free[len(free) // 2]
    others = [s for s in free if s != filler]
    budget = total - int(L.sum())
    assert budget >= 0, "target %d too small for this group" % total
    hi = min(195, budget // (len(others) + 1))
    for s in others:
        L[s] = rng.integers(0, hi + 1)
    L[filler] = total - int(L.sum())
    assert L[filler] >= 0 and int(L.sum()) == total
    return L


def object_bytes(types, row, rng):
    return [nonzero_bytes(rng, n) for n in row]


# ---- the packed batch: groups laid out in one blob ----------------------------------

class BatchChain:
    """Logical objects (base, lens) over one blob.  Every logical group holds
    K objects; launches = [(first object, end object)], all starting on a
    group boundary."""

    def __init__(self, types, geom, seed):
        self.types, self.A, self.K, self.WB = list(types), len(types), geom["objects"], geom["window"]
        self.rng = np.random.default_rng(seed)
        self.blob = bytearray()
        self.base, self.lens, self.attrs = [], [], []
        self.launches = []
        self.first_len, self.last_len = {}, {}   # logical group -> the pinned end lengths

    def lead(self):
        return (SHIFT + len(self.blob)) & 15

    def gap(self, n):
        self.blob += nonzero_bytes(self.rng, n)

    def put(self, row):
        """One object's bytes at the blob's end: (base, lens, attrs)."""
        at = object_bytes(self.types, row, self.rng)
        b = len(self.blob)
        for a in at:
            self.blob += a
        return b, [int(x) for x in row], at

    def name(self, objs):
        for b, row, at in objs:
            self.base.append(b)
            self.lens.append(row)
            self.attrs.append(at)

    def add(self, L, gaps=None):
        """New objects, back to back but for gaps = {object: bytes after it}."""
        assert len(self.base) % self.K == 0
        g = len(self.base) // self.K
        objs = []
        for o, row in enumerate(L):
            objs.append(self.put(row))
            if gaps and o in gaps:
                self.gap(gaps[o])
        self.name(objs)
        return g

    def filler(self, next_lead):
        """A staged group of about half a window that ends at next_lead."""
        span = self.WB // 2
        span += (next_lead - self.lead() - span) % 16
        return self.add(group_lens(self.types, self.K, span, self.rng))

    def launch_to(self, g, nobj=None):
        """A launch whose last group is g (its first nobj objects)."""
        self.launches.append((max(0, g - 2) * self.K, g * self.K + (nobj or self.K)))

    def fit(self, lead, delta, role="mid", **kw):
        """A group with lead + span == WB + delta; role "last": also a launch
        ending with it; "part": its first K - 1 objects carry the span and end
        a launch."""
        self.filler(lead)
        assert self.lead() == lead
        if role == "part":
            L = group_lens(self.types, self.K - 1, self.WB + delta - lead, self.rng, **kw)
            L = np.vstack([L, group_lens(self.types, 1, 200, self.rng)])
        else:
            L = group_lens(self.types, self.K, self.WB + delta - lead, self.rng, **kw)
        g = self.add(L)
        if role != "mid":
            self.launch_to(g, self.K - 1 if role == "part" else None)
        if "first" in kw:
            self.first_len[g] = kw["first"]
        if "last" in kw:
            self.last_len[g] = kw["last"]
        return g

    def finish(self):
        self.filler(0)
        self.blob += nonzero_bytes(self.rng, 64)
        self.n = len(self.base)
        self.launches.insert(0, (0, self.n))
        self.base = np.array(self.base, np.uint64)
        self.lens = np.array(self.lens, np.uint32).reshape(-1)
        self.sizes = self.lens.reshape(self.n, self.A).sum(axis=1)
        self.blob = np.frombuffer(bytes(self.blob), np.uint8)
        return self

    def model(self, s, e):
        return model_batch(self.base[s:e], self.sizes[s:e], self.K, self.WB, SHIFT)

    def repacked(self):
        """The same objects back to back in logical order."""
        blob = b"".join(b"".join(at) for at in self.attrs)
        return synth.object_bases(self.lens, self.A)[0], np.frombuffer(blob, np.uint8)


def fit_cases(c, roles):
    for role in roles:
        for lead, delta in FIT:
            c.fit(lead, delta, role)


@functools.lru_cache(maxsize=None)
def batch_chain(name, num2=True):
    """"full": every batch case at 17 attributes; "int" / "float": the window
    ends with a numeric in the first and last slot; "a2" / "a65": the fit
    boundary at 63 objects and at one object per wave."""
    types = {"full": schema17(S, num2), "int": schema17(I, num2), "float": schema17(F, num2),
             "a2": schema_mixed(2, num2), "a65": schema_mixed(65, num2)}[name]
    c = BatchChain(types, geometry(types, forced=not num2), seed=len(name) * 1000 + 17 * num2)
    K, WB, rng = c.K, c.WB, c.rng
    if name in ("a2", "a65"):
        fit_cases(c, ("mid", "last") + (("part",) if K > 1 else ()))
        return c.finish()
    if name in ("int", "float"):
        for role in ("mid", "last"):
            c.fit(0, 0, role)
            c.fit(15, 0, role)
            c.fit(1, 1, role)
        return c.finish()
    fit_cases(c, ("mid", "last", "part"))
    # the window's two ends in every regime: the first and the last staged string
    for role in ("mid", "last"):
        for k, n in enumerate(REGIMES):
            c.fit((0, 1, 15)[k % 3], 0, role, first=n, last=n)
    # not back to back
    for gap in (1, 16):
        for after in (0, K - 2):
            c.filler(3)
            c.add(group_lens(types, K, WB // 2, rng), gaps={after: gap})
        # ... between the group's last object and the next group's first: the early copy goes out
        # (the next base is within the window) or not, and the group is hashed from global memory
        c.filler(2)
        c.add(group_lens(types, K, WB - 2 - gap, rng), gaps={K - 1: gap})
        c.filler(2)
        c.add(group_lens(types, K, WB - 2 - gap + 1, rng), gaps={K - 1: gap})
    # order: the next group's first object below b0 (the next group lies before this one) ...
    c.filler(4)
    y = [c.put(row) for row in group_lens(types, K, WB // 2, rng)]
    c.add(group_lens(types, K, WB // 2, rng))
    c.name(y)
    # ... equal to b0 (the same K objects named twice) ...
    c.filler(6)
    g = c.add(group_lens(types, K, WB // 2, rng))
    c.name([(c.base[g * K + i], c.lens[g * K + i], c.attrs[g * K + i]) for i in range(K)])
    # ... and inside this group's span (the next group starts at this one's object 3)
    c.filler(7)
    g = c.add(group_lens(types, K, WB // 2, rng))
    tail = [(c.base[g * K + i], c.lens[g * K + i], c.attrs[g * K + i]) for i in range(3, K)]
    c.name(tail + [c.put(row) for row in group_lens(types, 3, 500, rng)])
    # empty: a whole group of span 0, in the middle and last; single empty objects in a full group
    for lead in (0, 9):
        c.filler(lead)
        g = c.add(np.zeros((K, c.A), np.int64))
        c.launch_to(g)
    c.filler(5)
    c.add(group_lens(types, K, WB // 2, rng, empty=(0, 3, K - 1)))
    # oversized: one object alone larger than the window
    for o in (0, K // 2, K - 1):
        c.filler(8)
        c.add(group_lens(types, K, None, rng, big=(o, WB + 100)))
    return c.finish()


def batch_features(c):
    """What the model says the chain's launches reach, as a set of tags."""
    K, WB, feats = c.K, c.WB, set()
    for s, e in c.launches:
        for g in c.model(s, e):
            role = "mid" if g["has_next"] else "last" if g["nobj"] == K else "part"
            span = g["bend"] - g["b0"]
            gi = (s + g["o0"]) // K
            sizes = c.sizes[s + g["o0"]:s + g["o0"] + g["nobj"]]
            if g["runs"] and g["bend"] >= g["b0"]:
                delta = g["lead"] + span - WB
                assert g["staged"] == (delta <= 0)
                if g["has_next"]:
                    assert g["early"] == (delta <= 0 and span > 0) and g["bnext"] == g["bend"]
                feats.add(("fit", role, g["lead"], delta))
                if g["staged"]:
                    assert g["units"] == (g["lead"] + span + 15) // 16 and 16 * g["units"] <= WB
                    feats.add(("copy", "early" if g["early"] else "late"))
                if delta == 0 and g["nobj"] == K:
                    feats.add(("front", role, c.first_len.get(gi, "-")))
                    feats.add(("back", role, c.last_len.get(gi, "-")))
                if span == 0:
                    feats.add(("empty group", role))
                elif (sizes == 0).any():
                    feats.add(("empty object",))
            for i, gap in zip(g["breaks"], g["gaps"]):
                if len(g["breaks"]) == 1 and gap in (1, 16):
                    where = "first" if i == 0 else "last" if i == g["nobj"] - 1 else "last but one" if i == K - 2 else "-"
                    feats.add(("gap", gap, where) + ((("early",) if g["early"] else ("no copy",)) if where == "last" else ()))
            if g["has_next"] and g["nobj"] == K:
                if g["bnext"] < g["b0"]:
                    feats.add(("next", "below b0"))
                elif g["bnext"] == g["b0"] and span > 0:
                    feats.add(("next", "at b0"))
                elif g["bnext"] < g["bend"]:
                    feats.add(("next", "inside", "early" if g["early"] else "no copy"))
            for o in np.nonzero(sizes > WB)[0]:
                feats.add(("oversized", "first" if o == 0 else "last" if o == K - 1 else "middle"))
    return feats


def batch_required(name, K):
    roles = ("mid", "last") + (("part",) if K > 1 else ())
    if name in ("int", "float"):
        return {("fit", r, l, d) for r in ("mid", "last") for l, d in ((0, 0), (15, 0), (1, 1))} | {
            ("front", "mid", "-"), ("back", "last", "-")}
    need = {("fit", r, l, d) for r in roles for l, d in FIT} | {("copy", "early"), ("copy", "late")}
    if name != "full":
        return need
    need |= {(end, r, n) for end in ("front", "back") for r in ("mid", "last") for n in REGIMES}
    for gap in (1, 16):
        need |= {("gap", gap, "first"), ("gap", gap, "last but one"), ("gap", gap, "last", "early"),
                 ("gap", gap, "last", "no copy")}
    need |= {("next", "below b0"), ("next", "at b0"), ("next", "inside", "early")}
    need |= {("empty group", "mid"), ("empty group", "last"), ("empty object",)}
    need |= {("oversized", w) for w in ("first", "middle", "last")}
    return need


BATCH_CHAINS = [("full", True), ("int", True), ("float", True), ("a2", True), ("a65", True),
                ("full", False), ("int", False), ("float", False), ("a2", False), ("a65", False)]


# ---- stored objects: keys and values laid out in one or two buffers -----------------

def be(n, size):
    return int(n).to_bytes(size, "big")


class SweepChain:
    """Stored objects over a key buffer and a value buffer ("columns"), or one
    store of [key][value] records.  Every logical group holds K objects."""

    def __init__(self, types, geom, records, seed):
        self.types, self.A = list(types), len(types)
        self.K, self.WB, self.KR = geom["objects"], geom["window"], geom["key_region"]
        self.records = records
        self.rng = np.random.default_rng(seed)
        self.keys = bytearray()
        self.vals = self.keys if records else bytearray()
        self.kaddr0, self.vaddr0 = SHIFT, SHIFT if records else SHIFT_V
        self.koff, self.klen, self.voff, self.vlen, self.attrs, self.raw, self.kind = [], [], [], [], [], [], []
        self.launches = []
        self.version = 1000   # the next object's
        self.tags = {}   # logical group -> what the case pins (regime lengths)

    def lead(self):
        return (self.kaddr0 + len(self.keys)) & 15

    def encode(self, L):
        """The group's objects through synth.encode_values_host: [(key, value, attrs)]."""
        L = np.asarray(L, np.int64)
        at = [object_bytes(self.types, row, self.rng) for row in L]
        blob = np.frombuffer(b"".join(b"".join(a) for a in at) + b"\0", np.uint8)
        lens = L.reshape(-1).astype(np.uint32)
        base = synth.object_bases(lens, self.A)[0]
        _, ko, kl, vals, vo, vl = synth.encode_values_host(self.types, blob, base, lens,
                                                           first_version=self.version)
        self.version += len(L)
        out = []
        for i in range(len(L)):
            v = bytes(vals[int(vo[i]):int(vo[i]) + int(vl[i])])
            assert bytes(blob[int(ko[i]):int(ko[i]) + int(kl[i])]) == at[i][0]
            out.append([at[i][0], v, at[i], None])
        return out

    def place(self, objs, key_at=None, key_gaps=None, val_gaps=None):
        """Objects [(key, value, attrs)] at the buffers' ends: records back to
        back, or keys in the key buffer (key_at[i]: at the next address with
        those low 4 bits; key_gaps[i] bytes after key i) and values in theirs."""
        rows = []
        for i, (k, v, at, kind) in enumerate(objs):
            if key_at and key_at[i] is not None:
                self.keys += nonzero_bytes(self.rng, (key_at[i] - self.lead()) % 16)
            ko = len(self.keys)
            self.keys += k
            if key_gaps and i in key_gaps:
                self.keys += nonzero_bytes(self.rng, key_gaps[i])
            vo = len(self.vals)
            self.vals += v
            if kind == "9 bytes":   # the bytes stay, the length says 9: what follows keeps its place
                v = v[:9]
            if val_gaps and i in val_gaps:
                self.vals += nonzero_bytes(self.rng, val_gaps[i])
            rows.append((ko, len(k), vo, len(v), at, v, kind))
        return rows

    def name(self, rows):
        assert len(self.koff) % self.K == 0 and len(rows) == self.K
        for ko, kl, vo, vl, at, v, kind in rows:
            self.koff.append(ko)
            self.klen.append(kl)
            self.voff.append(vo)
            self.vlen.append(vl)
            self.attrs.append(at)
            self.raw.append(v)
            self.kind.append(kind)
        return len(self.koff) // self.K - 1

    def overhead(self, nobj):
        return nobj * (10 + 4 * (self.A - 1))

    def launch_to(self, g, nobj=None):
        self.launches.append((max(0, g - 2) * self.K, g * self.K + (nobj or self.K)))

    def finish(self):
        pad = nonzero_bytes(self.rng, 64)
        self.keys += pad
        if not self.records:
            self.vals += pad
        self.n = len(self.koff)
        self.launches.insert(0, (0, self.n))
        self.koff, self.voff = np.array(self.koff, np.uint64), np.array(self.voff, np.uint64)
        self.klen, self.vlen = np.array(self.klen, np.uint32), np.array(self.vlen, np.uint32)
        self.keys = np.frombuffer(bytes(self.keys), np.uint8)
        self.vals = self.keys if self.records else np.frombuffer(bytes(self.vals), np.uint8)
        self.good = np.array([decodes(v, self.A)[0] for v in self.raw])
        return self

    def enc(self):
        return self.keys, self.koff, self.klen, self.vals, self.voff, self.vlen


def corrupt(v, A, how):
    """A stored value whose last length field, or attribute count, is wrong."""
    assert how in BAD_KINDS
    v = bytearray(v)
    pos = 10
    for _ in range(A - 2):
        pos += 4 + int.from_bytes(v[pos:pos + 4], "big")
    if how == "len+1":      # one more than what remains
        v[pos:pos + 4] = be(len(v) - pos - 4 + 1, 4)
    elif how == "len max":
        v[pos:pos + 4] = b"\xff" * 4
    elif how == "count+1":
        v[8:10] = be(A, 2)
    elif how == "count-1":
        v[8:10] = be(A - 2, 2)
    return bytes(v)   # "9 bytes": SweepChain.place cuts the length


BAD_KINDS = ("len+1", "len max", "count+1", "count-1", "9 bytes")


def model_sweep_prefix(c, s, e):
    """model_sweep over a launch [s, e) of the chain (the launch sees no
    object past e)."""
    return model_sweep(c.koff[s:e], c.klen[s:e], c.voff[s:e], c.vlen[s:e], c.K, c.WB, c.KR, c.kaddr0, c.vaddr0,
                       c.records)


@functools.lru_cache(maxsize=None)
def records_chain(num2=True, ends=S, A=17):
    """One store of records: the record span against the window (other
    attribute counts: that boundary alone)."""
    types = schema17(ends, num2) if A == 17 else schema_mixed(A, num2)
    c = SweepChain(types, geometry(types, sweep=True), True, seed=31 + num2)
    K, WB, rng = c.K, c.WB, c.rng

    def filler(next_lead):
        span = WB // 2
        span += (next_lead - c.lead() - span) % 16
        c.name(c.place(c.encode(group_lens(types, K, span - c.overhead(K), rng))))

    def fit(lead, delta, bad=(), **kw):
        filler(lead)
        assert c.lead() == lead
        objs = c.encode(group_lens(types, K, WB + delta - lead - c.overhead(K), rng, **kw))
        for o, how in bad:   # same length: the span stays what it was
            objs[o][1], objs[o][3] = corrupt(objs[o][1], c.A, how), how
        g = c.name(c.place(objs))
        c.tags[g] = kw
        return g

    if ends != S:
        for lead, delta in ((0, 0), (15, 0), (1, 1)):
            c.launch_to(fit(lead, delta))
        filler(0)
        return c.finish()
    for lead, delta in FIT:
        g = fit(lead, delta)
        if (lead, delta) in ((0, 0), (15, 0), (0, 1)):
            c.launch_to(g)
            if K > 1:
                c.launch_to(g, K - 1)
    if A != 17:
        filler(0)
        return c.finish()
    for k, n in enumerate(REGIMES):   # the span's first key and its last attribute in every regime
        fit((0, 1, 15)[k % 3], 0, first=n, last=n)
    # undecodable values inside a staged span and inside one walked from global memory
    for delta in (0, 1):
        fit(3, delta, bad=[(0, "len+1"), (2, "len max"), (3, "count+1"), (K - 1, "count-1")])
    # a gap inside the group: no record span; the keys are gathered, the values held in part
    filler(2)
    c.name(c.place(c.encode(group_lens(types, K, WB // 2, rng)), key_gaps={2: 1}))
    filler(0)
    return c.finish()


@functools.lru_cache(maxsize=None)
def columns_chain(num2=True, ends=S):
    """Keys in a buffer of their own: the key column against the key region,
    the two gathers of scattered keys, and how much of the values is held."""
    types = schema17(ends, num2)
    c = SweepChain(types, geometry(types, sweep=True), False, seed=57 + num2)
    K, WB, KR, rng, A = c.K, c.WB, c.KR, c.rng, c.A
    VOH = 10 + 4 * (A - 1)   # a value's header and length fields

    def keys_of(plan):
        """(key lengths, key_at, key_gaps) of a group's K keys."""
        kind = plan[0]
        if kind == "column":       # back to back: kend - k0 + klead == KR + delta
            total = KR + plan[1] - c.lead()
            first = plan[2] if len(plan) > 2 else None
            if types[0] in FIXED8:
                return None, None, None
            rest = rng.integers(0, (total - (first or 0)) // K, K)
            if first is not None:
                rest[0] = first
            rest[K // 2] += total - rest.sum()
            assert rest[K // 2] >= 0
            return [int(x) for x in rest], None, None
        if kind == "units":        # scattered, the longest reaching plan[2] bytes from its unit's start
            nobj, reach = plan[1], plan[2]
            at = [int(rng.integers(0, 16)) for _ in range(K)]
            kl = [int(rng.integers(0, reach - 16 - a)) for a in at]
            for i in range(nobj):   # every key of the group reaches into the last unit: each lane's copy counts
                kl[i] = reach - int(rng.integers(0, 15)) * (i != nobj - 1) - at[i]
            return kl, at, {i: 1 + int(rng.integers(0, 40)) for i in range(K)}
        assert kind == "dwords"    # scattered, long: 4 * td == plan[1]
        mods = [0, 1, 3, 2, 1, 3, 0][:K] + [0] * max(0, K - 7)
        at = [4 * int(rng.integers(0, 4)) + m for m in mods]
        d = [plan[1] // 4 // K] * K
        d[0] += plan[1] // 4 - sum(d)
        kl = [4 * d[i] - mods[i] - int(rng.integers(0, 4)) * (i % 2) for i in range(K)]
        return kl, at, {i: 5 + int(rng.integers(0, 40)) for i in range(K)}

    def group(kplan, vplan, bad=(), tag=None):
        kl, key_at, key_gaps = keys_of(kplan)
        L = group_lens(types, K, K * 60 + 8 * sum(t in FIXED8 for t in types) * K, rng)
        if kl is None:   # a numeric key column: 8 bytes each
            kl = [8] * K
        L[:, 0] = kl
        # where the keys will lie, so the model can say how much room the values get
        k_at = len(c.keys)
        ko = []
        for i in range(K):
            if key_at:
                k_at += (key_at[i] - (c.kaddr0 + k_at)) % 16
            ko.append(k_at)
            k_at += kl[i] + (key_gaps or {}).get(i, 0)
        v_at = len(c.vals)
        probe = model_sweep(ko, kl, [v_at] * K, [0] * K, K, WB, KR, c.kaddr0, c.vaddr0, False)[0]
        room, vlead = WB - probe["kreg"], (c.vaddr0 + v_at) & 15
        strings = [j for j in range(1, A) if types[j] not in FIXED8]
        fixed = VOH + 8 * sum(types[j] in FIXED8 for j in range(1, A))

        def value_row(total, last=None):
            """Lengths of attributes 1.. for a value of `total` bytes."""
            row = np.zeros(A, np.int64)
            for j in range(1, A):
                row[j] = 8 if types[j] in FIXED8 else 0
            budget = total - fixed
            free = list(strings)
            if last is not None and types[-1] not in FIXED8:
                row[A - 1] = last
                budget -= last
                free.remove(A - 1)
            assert budget >= 0 and free
            hi = min(195, budget // len(free))
            for j in free[1:]:
                row[j] = rng.integers(0, hi + 1)
            row[free[0]] = total - VOH - row[1:].sum()
            assert row[free[0]] >= 0 and VOH + row[1:].sum() == total
            return row

        kind = vplan[0]
        small = fixed + 13 * len(strings)
        if kind == "fit":
            totals = [small + int(rng.integers(0, 300)) for _ in range(K)]
            lasts = {}
        elif kind == "edge":       # object i ends `extra` bytes past what the window holds
            i, extra = vplan[1], vplan[2]
            head = room - vlead + extra
            each = head // (i + 1)
            totals = [each] * i + [head - each * i] + [small + 200] * (K - 1 - i)
            lasts = {i: vplan[3]} if len(vplan) > 3 else {}
        else:
            assert kind == "first big"
            totals = [room + 1] + [small + 100] * (K - 1)
            lasts = {}
        for i in range(K):
            L[i, 1:] = value_row(totals[i], lasts.get(i))[1:]
        objs = c.encode(L)
        for o, how in bad:
            objs[o][1], objs[o][3] = corrupt(objs[o][1], A, how), how
        assert all(len(objs[i][1]) == totals[i] for i in range(K))
        rows = c.place(objs, key_at, key_gaps)
        assert [r[0] for r in rows] == ko
        g = c.name(rows)
        c.tags[g] = tag or {}
        return g

    def tail():
        return group(("column", -40), ("fit",))

    if ends != S:
        # a numeric key column; the last in-window value ends on the window's last byte with a numeric
        c.launch_to(group(("column", 0), ("edge", K - 3, 0)))
        c.launch_to(group(("column", 0), ("edge", K - 3, 1)))
        tail()
        return c.finish()
    # the key column at the key region's edge, each with the value cases
    for delta in (-1, 0, 1):
        group(("column", delta), ("fit",))
        group(("column", delta), ("edge", K - 3, 0))       # object K - 3 ends exactly at vheld
        group(("column", delta), ("edge", K - 3, 1))       # ... one byte past it
        group(("column", delta), ("edge", 0, 1))           # no value fits
        group(("column", delta), ("first big",))
        c.launch_to(group(("column", delta), ("fit",)))     # the launch's last group holds no values
        # the next group's first value before this group's: named in the other order
        x = c.place(c.encode(group_lens(types, K, K * 300, rng)))
        y = c.place(c.encode(group_lens(types, K, K * 300, rng)))
        c.name(y)
        c.name(x)
    # scattered keys as 16-byte units: nobj * kU on both sides of the wave's 64 lanes (7 objects: 9 and
    # 10 units); the longest key ends on its last unit's last byte, or one byte into another unit
    full = 64 // K
    c.launch_to(group(("units", K, 16 * full), ("fit",)))
    group(("units", K, 16 * full), ("edge", 3, 1))
    c.launch_to(group(("units", K, 16 * full + 1), ("edge", 3, 0)))    # gathered as dwords
    for nobj, units in ((4, 16), (4, 17), (5, 13), (5, 12)):
        g = group(("units", nobj, 16 * units), ("edge", 2, 1))
        c.launch_to(g, nobj)
    # ... as dwords: all of the key region, and one dword more (hashed from global memory)
    for extra in (0, 4):
        group(("dwords", KR + extra), ("fit",))
        c.launch_to(group(("dwords", KR + extra), ("edge", K - 3, 0)))
    # decode edges on both walks: objects 0..2 in the window, 3.. walked from global memory
    for pair in (("len+1", "len max"), ("count+1", "count-1"), ("9 bytes", "len+1")):
        group(("column", -8), ("edge", 2, 0), bad=[(1, pair[0]), (4, pair[0]), (2, pair[1]), (K - 1, pair[1])])
    # the window's ends in every regime: the key that starts the key region, and the last
    # attribute of the last value the window holds
    for n in REGIMES:
        group(("column", 0, n), ("edge", K - 3, 0, n), tag=dict(first=n, last=n))
    tail()
    return c.finish()


@functools.lru_cache(maxsize=None)
def keyonly_chain(key_type=S):
    """One attribute: the value is its 10-byte header alone."""
    types = [key_type]
    c = SweepChain(types, geometry(types, sweep=True), False, seed=77)
    K, rng = c.K, c.rng
    for bad in ((), [(1, "9 bytes"), (K - 1, "count+1")]):
        L = np.array([[8 if key_type in FIXED8 else int(rng.integers(0, 100))] for _ in range(K)])
        objs = c.encode(L)
        assert all(len(o[1]) == 10 for o in objs)
        for o, how in bad:
            objs[o][1], objs[o][3] = corrupt(objs[o][1], 1, how), how
        c.launch_to(c.name(c.place(objs)))
    c.name(c.place(c.encode(np.array([[8 if key_type in FIXED8 else 20]] * K))))
    return c.finish()


def sweep_features(c):
    K, WB, KR, feats = c.K, c.WB, c.KR, set()
    for s, e in c.launches:
        for g in model_sweep_prefix(c, s, e):
            gi = (s + g["o0"]) // K
            tag = c.tags.get(gi, {})
            good = c.good[s + g["o0"]:s + g["o0"] + g["nobj"]]
            if g["rtotal"] is not None:
                feats.add(("records", g["klead"], g["rtotal"] - WB))
                if g["rtotal"] == WB and g["nobj"] == K:
                    feats.add(("record ends", tag.get("first", "-"), tag.get("last", "-")))
                if not good.all():
                    feats.add(("records bad", "window" if g["rspan"] else "global"))
                if not g["has_next"]:
                    feats.add(("records last", g["nobj"] == K, g["rspan"]))
                continue
            if g["ktotal"] is not None:
                feats.add(("key column", g["ktotal"] - KR, g["keys"]))
            if g["kU"]:
                feats.add(("key units", g["nobj"], g["kU"], g["keys"]))
                if g["last_key_units"] == g["kU"]:   # the group's last unit holds key bytes
                    feats.add(("last key's last unit", g["nobj"], g["kU"]))
                feats.update(("key reach", r) for r in g["reach"] if r and r % 16 in (0, 1))
            if g["td"] is not None and g["ktotal"] is None:
                feats.add(("key dwords", 4 * g["td"] - KR, g["keys"]) + tuple(g["kmod4"]))
            if g["vbefore"]:
                feats.add(("next value before v0",))
            if not g["has_next"]:
                feats.add(("last group",))
            held = [i for i in range(g["nobj"]) if g["vin"][i]]
            if g["vheld"] == g["room"] and g["has_next"]:
                over = [v - g["vheld"] for v in g["vend"]]
                if 0 in over:
                    assert g["vin"][over.index(0)] and not any(g["vin"][over.index(0) + 1:])
                    feats.add(("value ends at vheld", g["keys"]))
                    feats.add(("window ends", tag.get("first", "-"), tag.get("last", "-")))
                if 1 in over:
                    assert not any(g["vin"][over.index(1):])
                    feats.add(("value one past vheld", g["keys"]))
                if over[0] > 0:
                    feats.add(("first value too long", g["keys"], g["vlen0"] > g["room"]))
            if held and len(held) < g["nobj"]:
                feats.add(("both walks",))
            for i in range(g["nobj"]):
                if not good[i]:
                    feats.add(("bad", c.kind[s + g["o0"] + i], "window" if g["vin"][i] else "global"))
    return feats


def records_required():
    need = {("records", l, d) for l, d in FIT}
    need |= {("record ends", n, n) for n in REGIMES}
    need |= {("records bad", "window"), ("records bad", "global")}
    need |= {("records last", True, True), ("records last", False, True), ("records last", True, False)}
    return need


def columns_required(K):
    need = {("key column", -1, "span"), ("key column", 0, "span"), ("key column", 1, "global")}
    full = 64 // K   # units per key at which K keys fill the wave's lanes
    need |= {("key units", K, full, "units"), ("key units", K, full + 1, "dwords"), ("key units", 4, 16, "units"),
             ("key units", 4, 17, "dwords"), ("key units", 5, 13, "dwords"), ("key units", 5, 12, "units")}
    need |= {("last key's last unit", n, u) for n, u in ((K, full), (K, full + 1), (4, 16), (4, 17), (5, 13), (5, 12))}
    need |= {("key reach", 16 * full), ("key reach", 16 * full + 1)}
    need |= {("key dwords", 0, "dwords", 0, 1, 2, 3), ("key dwords", 4, "global", 0, 1, 2, 3)}
    need |= {("value ends at vheld", k) for k in ("span", "global", "dwords")}
    need |= {("value one past vheld", k) for k in ("span", "global", "units")}
    need |= {("first value too long", "span", False), ("first value too long", "span", True)}
    need |= {("next value before v0",), ("last group",), ("both walks",)}
    need |= {("bad", what, where) for what in BAD_KINDS for where in ("window", "global")}
    need |= {("window ends", n, n) for n in REGIMES}
    return need


# ---- CPU self-checks ---------------------------------------------------------------

def test_geometry_follows_the_launch_formula():
    """K = min(64 * NCH / A, cap) for every attribute count, in both libraries."""
    for A in range(1, 129):
        types = schema_mixed(A)
        for sweep in (False, True):
            g = geometry(types, sweep, forced=not sweep)   # A = 1 is not the policy's batch form: forced
            assert g["objects"] == min(64 * g["passes"] // A, g["object_cap"]) >= 1, (A, sweep, g)
            assert g["objects"] * A <= 64 * g["passes"] and g["window"] % 16 == 0
            assert g["front_pad"] >= 32 and g["back_pad"] >= 36, "hash_slot_window's reads around a short string"
            if sweep:
                assert 0 < g["key_region"] < g["window"] and g["key_region"] % 16 == 0
            else:
                assert g["objects"] <= 63, "lane K holds the next group's first base"
                if A > 1:
                    assert hdx.hashing.kernel_for(types, 1000)[0] == 212 and geometry(types) == g
                with _lib.debug_library(212):   # the debug library's sweep: the same form
                    assert hdx.hashing.wave_geometry(types, True) == geometry(types, True)


def test_geometry_refuses_other_forms():
    wg = hdx.hashing.wave_geometry
    assert wg([S]) is None and wg([S, I, I]) is None and wg(schema17(S, num2=False)) is None
    assert wg(schema_mixed(129)) is None and wg(schema_mixed(129), True) is None
    assert wg(schema17(S, num2=False), True) is not None
    with _lib.debug_library(212):
        assert wg(schema17(S, num2=False))["objects"] == wg(schema17())["objects"]
        assert wg(schema_mixed(129)) is None
    with _lib.debug_library(44):
        assert wg(schema17()) is None and wg(schema17(), True) is None
    with pytest.raises(hdx.HdxError):
        wg([S, 12345])


@pytest.mark.parametrize("name,num2", BATCH_CHAINS)
def test_batch_cases_cover_every_boundary(name, num2):
    c = batch_chain(name, num2)
    assert c.K == geometry(c.types, forced=not num2)["objects"]
    assert c.K == {"a2": geometry(c.types, forced=not num2)["object_cap"], "a65": 1}.get(name, c.K), "the lane-63 edge / one object per wave"
    missing = batch_required(name, c.K) - batch_features(c)
    assert not missing, sorted(missing, key=str)


def test_sweep_cases_cover_every_boundary():
    for num2 in (True, False):
        r, c = records_chain(num2), columns_chain(num2)
        missing = records_required() - sweep_features(r)
        assert not missing, sorted(missing, key=str)
        missing = columns_required(c.K) - sweep_features(c)
        assert not missing, sorted(missing, key=str)
        for A in (2, 65):
            missing = {("records", l, d) for l, d in FIT} - sweep_features(records_chain(num2, A=A))
            assert not missing, sorted(missing, key=str)
        # a numeric as the span's first key and last attribute, as the key region's first key and
        # as the last attribute of the last value the window holds
        for ends in (I, F):
            f = sweep_features(records_chain(num2, ends))
            assert {("records", 0, 0), ("records", 15, 0), ("records", 1, 1)} <= f
            f = sweep_features(columns_chain(num2, ends))
            assert {("value ends at vheld", "span"), ("value one past vheld", "span")} <= f
            assert any(t[0] == "key column" and t[2] == "span" for t in f), "the 8-byte keys copied as one span"
    for key_type in (S, TS):
        f = sweep_features(keyonly_chain(key_type))
        need = {("bad", how, where) for how in ("9 bytes", "count+1") for where in ("window", "global")}
        missing = (need | {("last group",)}) - f
        assert not missing, sorted(missing, key=str)


@pytest.mark.parametrize("name,num2", BATCH_CHAINS)
def test_oracle_ignores_batch_placement(oracle, name, num2):
    """The same objects back to back give the chain's coordinates: the
    builders name each object's bytes whatever its lead, gaps and order."""
    c = batch_chain(name, num2)
    want, err = batch_want(oracle, c)
    base, blob = c.repacked()
    again, err2 = oracle.hash_batch(c.types, blob, base, c.lens)
    assert err == 0 and err2 == 0 and np.array_equal(want, again)
    assert int((c.base + c.sizes).max()) <= len(c.blob)


def sweep_chains():
    return ([records_chain(n) for n in (True, False)] + [columns_chain(n) for n in (True, False)]
            + [chain(n, e) for chain in (records_chain, columns_chain) for n in (True, False) for e in (I, F)]
            + [records_chain(n, A=A) for n in (True, False) for A in (2, 65)] + [keyonly_chain(S), keyonly_chain(TS)])


def test_oracle_ignores_sweep_placement(oracle):
    """Decodable objects hash as the packed objects they were encoded from,
    with the version they were given; the model and the oracle agree on
    which values do not decode."""
    for c in sweep_chains():
        want, versions, bad = sweep_want(oracle, c)
        assert np.array_equal(~bad, c.good)
        assert (want[bad] == 0).all() and (versions[bad] == 0).all()
        lens = np.array([[len(a) for a in at] for at in c.attrs], np.uint32).reshape(-1)
        blob = np.frombuffer(b"".join(b"".join(at) for at in c.attrs) + b"\0", np.uint8)
        packed, err = oracle.hash_batch(c.types, blob, synth.object_bases(lens, c.A)[0], lens)
        assert err == 0 and np.array_equal(want[c.good], packed[c.good])
        assert [decodes(v, c.A)[1] for v in c.raw] == [int(x) for x in versions]
        assert (versions[c.good] >= 1000).all() and len(set(versions[c.good])) == int(c.good.sum())
        assert int((c.voff + c.vlen).max()) <= len(c.vals) and int((c.koff + c.klen).max()) <= len(c.keys)


# ---- the GPU runs ------------------------------------------------------------------

_WANT = {}


def batch_want(oracle, c):
    if id(c) not in _WANT:
        _WANT[id(c)] = oracle.hash_batch(c.types, c.blob, c.base, c.lens)
    return _WANT[id(c)]


def sweep_want(oracle, c):
    if id(c) not in _WANT:
        _WANT[id(c)] = oracle.hash_encoded(c.types, *c.enc())
    return _WANT[id(c)]


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available()
    return torch, torch.device("cuda", 0)


def on_device(torch, dev, host_bytes, shift):
    """test_device_edges.shifted: a device view with data_ptr() % 16 == shift."""
    buf = torch.zeros(shift + len(host_bytes), dtype=torch.uint8, device=dev)
    view = buf[shift:]
    view.copy_(torch.from_numpy(np.array(host_bytes)))
    assert view.data_ptr() % 16 == shift
    return view


def ints(torch, dev, a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64 if a.dtype == np.uint64 else np.int32).copy()).to(dev)


def u64(t):
    return t.cpu().numpy().view(np.uint64)


def run_batch_chain(torch, dev, oracle, c, forced=False, tables=None, want_ids=None):
    """Every launch of the chain; forced: through debug variant 212; tables:
    through hdx_hash_batch_regions_device."""
    want, err = batch_want(oracle, c)
    assert err == 0
    A = c.A
    blob, base, lens = on_device(torch, dev, c.blob, SHIFT), ints(torch, dev, c.base), ints(torch, dev, c.lens)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    with (_lib.debug_library(212) if forced else contextlib.nullcontext()):
        assert hdx.hashing.kernel_for(c.types, c.n)[0] == 212
        for s, e in c.launches:
            if tables is None:
                got = hdx.hash_batch(c.types, blob, base[s:e], lens[s * A:e * A], status=status)
            else:
                ids, got = hdx.hash_batch_regions(c.types, blob, base[s:e], lens[s * A:e * A], tables, coords=True,
                                                  status=status)
                assert np.array_equal(u64(ids), want_ids[:, s:e]), "region ids, launch [%d, %d)" % (s, e)
            got = u64(got)
            if not np.array_equal(got, want[s:e]):
                o, j = np.argwhere(got != want[s:e])[0]
                g = c.model(s, e)[o // c.K]
                raise AssertionError("launch [%d, %d): object %d attribute %d (length %d) differs; its group: %r"
                                     % (s, e, s + o, j, c.lens[(s + o) * A + j], g))
        assert int(status.item()) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name,num2", BATCH_CHAINS)
def test_batch_window_edges(oracle, torch_dev, name, num2):
    """The product batch form (NUM2), and its other instantiation forced on a
    schema with a timestamp and a non-hashable attribute."""
    torch, dev = torch_dev
    c = batch_chain(name, num2)
    if num2:
        assert hdx.hashing.kernel_for(c.types, c.n)[0] == 212
    else:
        assert hdx.hashing.kernel_for(c.types, c.n)[0] != 212
    run_batch_chain(torch, dev, oracle, c, forced=not num2)


def region_tables(oracle, A, want_coords):
    """The two tables of test_device_edges.tables_for: the key grid (64
    regions: indexed) and 300 random boxes over the last attribute and the key
    (scanned); (tables, the oracle's ids (2, n))."""
    rng = np.random.default_rng(A)
    lo1, up1 = oracle.partition(1, 64)
    a = rng.integers(0, 2**64, size=(300, 2), dtype=np.uint64)
    b = rng.integers(0, 2**64, size=(300, 2), dtype=np.uint64)
    specs = [([0], lo1, up1), ([A - 1, 0], np.minimum(a, b), np.maximum(a, b))]
    ids = [np.arange(1, len(lo) + 1, dtype=np.uint64) * 3 for _, lo, _ in specs]
    tables = [hdx.RegionTable(at, lo, up, i) for (at, lo, up), i in zip(specs, ids)]
    want = np.stack([oracle.lookup_region(at, lo, up, i, want_coords) for (at, lo, up), i in zip(specs, ids)])
    return tables, want


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["full", "int", "float", "a2", "a65"])
def test_batch_regions_window_edges(oracle, torch_dev, name):
    """hdx_hash_batch_regions_device: the wave-staged kernel with the fused lookups."""
    torch, dev = torch_dev
    c = batch_chain(name)
    want, _ = batch_want(oracle, c)
    tables, want_ids = region_tables(oracle, c.A, want)
    run_batch_chain(torch, dev, oracle, c, tables=tables, want_ids=want_ids)


def run_sweep_chain(torch, dev, oracle, c):
    want, versions, bad = sweep_want(oracle, c)
    keys = on_device(torch, dev, c.keys, c.kaddr0)
    vals = keys if c.records else on_device(torch, dev, c.vals, c.vaddr0)
    koff, klen, voff, vlen = (ints(torch, dev, x) for x in (c.koff, c.klen, c.voff, c.vlen))
    for s, e in c.launches:
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        vers = torch.empty(e - s, dtype=torch.int64, device=dev)
        got = u64(hdx.hash_encoded(c.types, keys, koff[s:e], klen[s:e], vals, voff[s:e], vlen[s:e], versions=vers,
                                   status=status))
        if not np.array_equal(got, want[s:e]):
            o, j = np.argwhere(got != want[s:e])[0]
            g = model_sweep_prefix(c, s, e)[o // c.K]
            raise AssertionError("launch [%d, %d): object %d attribute %d differs; its group: %r" % (s, e, s + o, j, g))
        assert np.array_equal(u64(vers), versions[s:e]), "versions, launch [%d, %d)" % (s, e)
        assert int(status.item()) == (BADENC if bad[s:e].any() else 0), "status, launch [%d, %d)" % (s, e)


@pytest.mark.gpu
@pytest.mark.parametrize("num2", [True, False], ids=["num2", "other types"])
@pytest.mark.parametrize("layout", ["records", "columns"])
def test_sweep_window_edges(oracle, torch_dev, layout, num2):
    torch, dev = torch_dev
    run_sweep_chain(torch, dev, oracle, (records_chain if layout == "records" else columns_chain)(num2))


@pytest.mark.gpu
@pytest.mark.parametrize("num2", [True, False], ids=["num2", "other types"])
@pytest.mark.parametrize("A", [2, 65])
def test_sweep_record_fit_other_attribute_counts(oracle, torch_dev, A, num2):
    torch, dev = torch_dev
    run_sweep_chain(torch, dev, oracle, records_chain(num2, A=A))


@pytest.mark.gpu
@pytest.mark.parametrize("num2", [True, False], ids=["num2", "other types"])
@pytest.mark.parametrize("ends", [I, F], ids=["int64", "float"])
def test_sweep_window_ends_numeric(oracle, torch_dev, ends, num2):
    """An int64 / a float in the first and the last slot, on both sweep forms."""
    torch, dev = torch_dev
    run_sweep_chain(torch, dev, oracle, records_chain(num2, ends))
    run_sweep_chain(torch, dev, oracle, columns_chain(num2, ends))


@pytest.mark.gpu
@pytest.mark.parametrize("key_type", [S, TS], ids=["string", "timestamp"])
def test_sweep_ten_byte_values(oracle, torch_dev, key_type):
    torch, dev = torch_dev
    run_sweep_chain(torch, dev, oracle, keyonly_chain(key_type))


# ---- every attribute count -----------------------------------------------------------

KINDS = [synth.Rule(S, synth.UNIFORM, 0, 150), synth.Rule(I, synth.NUMERIC, 8, 8), synth.Rule(F, synth.NUMERIC, 8, 8)]


@pytest.mark.gpu
@pytest.mark.parametrize("A", range(1, 129))
def test_every_attribute_count(oracle, torch_dev, A):
    """2K + 1 objects (a full middle group, a full later one, a last group of
    one) as a packed batch and as stored objects, through the policy and,
    where that picks another batch kernel, forced through the wave-staged one."""
    torch, dev = torch_dev
    rules = [KINDS[j % 3] for j in range(A)]
    types = [r.type for r in rules]
    K = geometry(types, forced=True)["objects"]
    _, blob, base, lens = synth.make_batch_host(rules, 2 * K + 1, seed=4000 + A)
    want, err = oracle.hash_batch(types, blob, base, lens)
    assert err == 0
    d = on_device(torch, dev, np.concatenate([blob, np.zeros(16, np.uint8)]), SHIFT), ints(torch, dev, base), \
        ints(torch, dev, lens)
    policy = hdx.hashing.kernel_for(types, len(base))[0]
    assert np.array_equal(u64(hdx.hash_batch(types, *d)), want), "policy form %d" % policy
    if policy != 212:
        with _lib.debug_library(212):
            assert hdx.hashing.kernel_for(types, len(base))[0] == 212
            assert np.array_equal(u64(hdx.hash_batch(types, *d)), want), "forced 212"
    K = geometry(types, sweep=True)["objects"]
    n = 2 * K + 1
    for layout in ("columns", "records"):
        if layout == "columns":
            enc = synth.encode_values_host(types, blob, base[:n], lens[:n * A], first_version=9)
        else:
            enc = synth.encode_store_host(types, blob, base[:n], lens[:n * A], first_version=9, layout="records")
        w, v, bad = oracle.hash_encoded(types, *enc)
        assert not bad.any() and np.array_equal(w, want[:n])
        keys = on_device(torch, dev, np.concatenate([enc[0], np.zeros(16, np.uint8)]), SHIFT)
        vals = keys if layout == "records" else on_device(torch, dev, np.concatenate([enc[3], np.zeros(16, np.uint8)]),
                                                          SHIFT_V)
        vers = torch.empty(n, dtype=torch.int64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        got = hdx.hash_encoded(types, keys, ints(torch, dev, enc[1]), ints(torch, dev, enc[2]), vals,
                               ints(torch, dev, enc[4]), ints(torch, dev, enc[5]), versions=vers, status=status)
        assert np.array_equal(u64(got), w), layout
        assert np.array_equal(u64(vers), v) and int(status.item()) == 0, layout
