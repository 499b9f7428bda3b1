"""The attribute checks and the sort order against the reference's compiled code.

The pin is tests/golden/reference_check_values.json: what the reference's own passes_attribute_check,
passes_attribute_checks (common/attribute_check.cc) and datatype_*::compare return, compiled unmodified
into oracle/_ref/libref_checks.so (oracle/Makefile), for the inputs of
tests/golden/make_reference_check_values.py.  Held to it here: hdx_passes_checks, hdx_checks_passes and
hdx_compare on the host; check_kernel (one-shot and compiled, REGEX included) and sorted_rank_kernel with
its finishing step on the device; and the restatements the other tests take their expected values from
(test_checks.check_one / expected_first_fail / compare, test_regex_checks' versions with REGEX,
test_sorted_search.sort_compare), which turns their matrices into pinned ones.

The GPU tests read the fixture and the generator's inputs only.  Container, document and macaroon
datatypes are outside the pin (the recipe's lookup() knows the nine primitive types), and so is
search_manager.cc (R2 of test_sorted_search.py)."""
import functools
import importlib.util
import json
import os

import numpy as np
import pytest

import hyperdex_amd as hdx
from hyperdex_amd.checks import AttributeCheck, CompiledChecks
from hyperdex_amd.sorting import KEEP_LARGEST, KEEP_SMALLEST, SortSpec
from test_checks import encode, to_dev, torch_gpu  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load_generator():
    spec = importlib.util.spec_from_file_location(
        "make_reference_check_values", os.path.join(ROOT, "tests", "golden", "make_reference_check_values.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


gen = _load_generator()
STRING, INT64, FLOAT, REGEX = gen.STRING, gen.INT64, gen.FLOAT, gen.REGEX


def _ref():
    from oracle import oracle
    return oracle if oracle.ref_checks() is not None else None


needs_ref = pytest.mark.skipif(_ref() is None, reason="needs oracle/_ref/libref_checks.so (make -C oracle ref)")


class Pin:
    """The fixture, read once: passes[T] (bool, checks x values), first_fail (lists x objects), signs[T]."""
    _the = None

    def __init__(self):
        with open(gen.FIXTURE) as f:
            self.text = f.read()
        self.fx = json.loads(self.text)
        self.passes, ff, self.signs = gen.load(self.fx)
        self.first_fail = np.array(ff, np.uint32)
        self.lists = gen.lists()
        self.objs = gen.objects()

    @classmethod
    def get(cls):
        if cls._the is None:
            cls._the = cls()
        return cls._the


def is_string_regex(T, D, p):
    return p == REGEX and T == STRING and D == STRING


def list_has_string_regex(cl):
    return any(a < len(gen.SCHEMA) and is_string_regex(gen.SCHEMA[a], D, p) for a, k, D, p in cl)


def as_checks(cl):
    return [AttributeCheck(a, k, D, p) for a, k, D, p in cl]


# ---- 1. the fixture ------------------------------------------------------------------------------

def test_fixture_meets_its_conditions():
    """On the fixture and the generator's inputs alone: per comparing predicate and for REGEX each outcome
    is a tenth of the cases whose types let it compare; some list of three or more checks fails at every
    index and passes; each sign occurs per type; the pools hold the edges."""
    from test_checks import F64, I64, MIS_SIZED, STRINGS
    pin = Pin.get()
    assert len(pin.text) <= 95326  # no larger than reference_store_values.json
    counts = gen.assert_conditions(pin.passes, pin.first_fail.tolist(), pin.signs)
    assert pin.fx["counts"]["true_of_comparing_cases"] == {str(p): c for p, c in sorted(counts.items())}
    assert pin.fx["counts"]["single_cases"] == sum(m.size for m in pin.passes.values())
    # the pools
    V = gen.V_STRING
    assert {len(s) for s in V} >= set(range(18)) and max(len(s) for s in V) >= 1000
    for pos in (7, 8, 15, 16):
        assert gen.BASE in V and gen.flip(gen.BASE, pos) in V
    assert {b"\x7f", b"\x80", b"ab\x7f", b"ab\x80"} <= set(V)
    assert all(s in STRINGS for s in V if len(s) <= 41 and s not in [gen.flip(gen.BASE[:8], p) for p in range(8)]
               and s not in [gen.flip(gen.BASE, p) for p in (1, 23, 24, 31, 32, 39)])
    assert gen.I64 == I64 and gen.F64 == F64 and gen.MIS_SIZED == MIS_SIZED
    for T in gen.TYPES:
        pool, vals = gen.check_pool(T), gen.value_pool(T)
        assert {p for _, p, _ in pool} == set(gen.PREDICATES) and len(gen.PREDICATES) == 14
        assert {D for D, _, _ in pool} == set(gen.TYPES)
        own = [k for D, p, k in pool if D == T and p in gen.ORDERING]
        assert any(k in vals for k in own) and b"" in own and (T == STRING or gen.MIS3 in own)
        if T != STRING:
            assert set(gen.MIS_SIZED) <= set(vals) and b"" in vals
    lens = [k for D, p, k in gen.check_pool(STRING) if D == INT64 and p in gen.LENGTH]
    assert {0, 3, 8, 9} <= {len(k) for k in lens}
    assert sum(1 for D, p, k in gen.check_pool(STRING) if is_string_regex(STRING, D, p)) >= 5
    # the lists
    assert len(gen.SCHEMA) == 10 and gen.SCHEMA[0] == STRING and set(gen.SCHEMA) == set(gen.TYPES)
    assert len(pin.objs) >= 257 and len(pin.lists) >= 32
    assert {len(cl) for cl in pin.lists} >= {0, 1, 16}
    attrs = [a for cl in pin.lists for a, _, _, _ in cl]
    assert 0 in attrs and len(gen.SCHEMA) in attrs and 0xffff in attrs
    assert any(len(cl) > len({a for a, _, _, _ in cl}) for cl in pin.lists)
    assert sum(list_has_string_regex(cl) for cl in pin.lists) >= 3
    # compare: a group of strings that shares its first eight bytes
    assert sum(s[:8] == gen.BASE[:8] for s in gen.compare_pool(STRING)) >= 10


@needs_ref
def test_fixture_regenerates_from_the_reference():
    assert gen.dumps(gen.build_fixture(_ref())) == Pin.get().text


# ---- 2. the host library against the fixture -----------------------------------------------------------

def test_cpu_single_checks_equal_the_fixture():
    """hdx_passes_checks on attribute 1 and on the key; REGEX on a STRING through the compiled form."""
    pin = Pin.get()
    n = 0
    for T in gen.TYPES:
        vals = gen.value_pool(T)
        for (D, p, k), row in zip(gen.check_pool(T), pin.passes[T]):
            on_attr, on_key = AttributeCheck(1, k, D, p), AttributeCheck(0, k, D, p)
            if is_string_regex(T, D, p):
                with CompiledChecks([STRING, T], [on_attr]) as a, CompiledChecks([T, STRING], [on_key]) as b:
                    got = [(a.passes(b"key", [v]), b.passes(v, [b"x"])) for v in vals]
            else:
                got = [(hdx.passes_checks([STRING, T], b"key", [v], [on_attr]),
                        hdx.passes_checks([T, STRING], v, [b"x"], [on_key])) for v in vals]
            assert got == [(int(w), int(w)) for w in row], (T, D, p, k)
            n += len(vals)
    assert n == pin.fx["counts"]["single_cases"]


def test_cpu_lists_equal_the_fixture():
    pin = Pin.get()
    for cl, want in zip(pin.lists, pin.first_fail):
        checks = as_checks(cl)
        with CompiledChecks(gen.SCHEMA, checks) as cc:
            assert [cc.passes(key, vals) for key, vals in pin.objs] == want.tolist(), cl
        if not list_has_string_regex(cl):
            assert [hdx.passes_checks(gen.SCHEMA, key, vals, checks) for key, vals in pin.objs] == want.tolist(), cl


def test_cpu_compare_equals_the_fixture():
    """hdx_compare against the sign matrix, and test_sorted_search.sort_compare wherever no NaN is involved."""
    from test_sorted_search import is_nan, sort_compare
    pin = Pin.get()
    for T in gen.TYPES:
        pool = gen.compare_pool(T)
        for i, a in enumerate(pool):
            for j, b in enumerate(pool):
                assert hdx.compare(T, a, b) == pin.signs[T][i, j], (T, a, b)
                if not (T == FLOAT and (is_nan(a) or is_nan(b))):
                    assert sort_compare(T, a, b) == pin.signs[T][i, j], (T, a, b)


# ---- 3. the restatements against the fixture -----------------------------------------------------------

def test_restatements_equal_the_fixture():
    """test_checks.check_one, expected_first_fail and compare, and test_regex_checks' versions of the first
    two (REGEX on a STRING): the expected values of those modules' matrices."""
    import test_checks
    import test_regex_checks
    pin = Pin.get()
    for T in gen.TYPES:
        vals = gen.value_pool(T)
        for (D, p, k), row in zip(gen.check_pool(T), pin.passes[T]):
            ck = AttributeCheck(1, k, D, p)
            assert [test_regex_checks.check_one(T, ck, v) for v in vals] == row.tolist(), (T, D, p, k)
            if not is_string_regex(T, D, p):
                assert [test_checks.check_one(T, ck, v) for v in vals] == row.tolist(), (T, D, p, k)
        pool = gen.compare_pool(T)
        got = [[test_checks.compare(T, a, b) for b in pool] for a in pool]
        assert np.array_equal(np.array(got), pin.signs[T]), T
    for cl, want in zip(pin.lists, pin.first_fail):
        checks = as_checks(cl)
        got = [test_regex_checks.expected_first_fail(gen.SCHEMA, key, vals, checks) for key, vals in pin.objs]
        assert got == want.tolist(), cl
        if not list_has_string_regex(cl):
            got = [test_checks.expected_first_fail(gen.SCHEMA, key, vals, checks) for key, vals in pin.objs]
            assert got == want.tolist(), cl


@needs_ref
def test_reference_on_the_single_check_cases():
    """The reference's passes_attribute_check itself on test_checks.single_check_cases() with a primitive
    check datatype, against check_one."""
    import test_checks
    oracle = _ref()
    n = 0
    for T, ck, v in test_checks.single_check_cases():
        if ck.datatype in test_checks.PRIMITIVE:
            want = oracle.ref_passes_attribute_check(T, ck.datatype, ck.predicate, ck.value, v)
            assert test_checks.check_one(T, ck, v) == want, (T, ck, v)
            n += 1
    assert n > 12000
    assert oracle.ref_compare(INT64, b"abc", b"")[1] == 2 and oracle.ref_compare(12345, b"", b"")[1] == 1


# ---- the device ----------------------------------------------------------------------------------------

LAYOUTS = [("keycol", 0), ("records", 7)]
SINGLE_OBJECTS = 257   # two workgroups of the check kernel, the second with one lane
SORTED_EVERY = 11      # every eleventh row also goes through the sorted search


def stacked(torch, tensors):
    return torch.stack(tensors).cpu().numpy().view(np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("T", gen.TYPES)
def test_gpu_single_checks(torch_gpu, T):
    """V_T as 257 stored objects under [T, T] (key = attribute = v_i, the pool cycled): one launch per row
    of C_T, on attribute 1 and on the key in turn, through hdx_check_encoded_device and
    hdx_checks_encoded_device; a sample of the rows through hdx_sorted_search_device."""
    torch = torch_gpu
    pin = Pin.get()
    assert hdx.checks.check_block_objects() == 256
    vals, pool = gen.value_pool(T), gen.check_pool(T)
    idx = np.arange(SINGLE_OBJECTS) % len(vals)
    objs = [(vals[i], [vals[i]]) for i in idx]
    want = pin.passes[T][:, idx].astype(np.uint32)
    types = [T, T]
    dev = torch.device("cuda", 0)
    for layout, shift in LAYOUTS:
        d = to_dev(torch, encode(types, objs, layout), shift)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        one_shot, compiled, sorted_rows, sorted_ff, rows = [], [], [], [], []
        for r, (D, p, k) in enumerate(pool):
            checks = [AttributeCheck(1 - (r & 1), k, D, p)]
            rx = is_string_regex(T, D, p)
            if not rx:
                one_shot.append(hdx.check_encoded(types, *d, checks, want_match=False, status=status)[0])
                rows.append(r)
            with CompiledChecks(types, checks) as cc:
                compiled.append(cc.check_encoded(*d, want_match=False, status=status)[0])
                if r % SORTED_EVERY == 0 or rx:
                    spec = SortSpec(r & 1, KEEP_LARGEST if r & 2 else KEEP_SMALLEST, (r >> 2) & 1)
                    if rx:
                        sorted_ff.append(cc.sorted_search(*d, spec, 5)[0])
                    else:
                        sorted_ff.append(hdx.sorted_search(types, *d, checks, spec, 5)[0])
                    sorted_rows.append(r)
        got = stacked(torch, compiled)
        assert np.array_equal(got, want), (layout, "compiled", [pool[r] for r in np.nonzero((got != want).any(1))[0][:5]])
        got = stacked(torch, one_shot)
        assert np.array_equal(got, want[rows]), (layout, [pool[rows[r]] for r in
                                                          np.nonzero((got != want[rows]).any(1))[0][:5]])
        got = stacked(torch, sorted_ff)
        assert np.array_equal(got, want[sorted_rows]), (layout, "sorted", [pool[sorted_rows[r]] for r in np.nonzero(
            (got != want[sorted_rows]).any(1))[0][:5]])
        assert int(status.item()) == 0 and len(sorted_rows) >= len(pool) // SORTED_EVERY


@pytest.mark.gpu
@pytest.mark.parametrize("layout,shift", LAYOUTS)
def test_gpu_lists(torch_gpu, layout, shift):
    """The 259 objects under the ten-attribute schema, every list, through both check entry points."""
    torch = torch_gpu
    pin = Pin.get()
    dev = torch.device("cuda", 0)
    d = to_dev(torch, encode(gen.SCHEMA, pin.objs, layout), shift)
    for cl, want in zip(pin.lists, pin.first_fail):
        checks = as_checks(cl)
        forms = []
        with CompiledChecks(gen.SCHEMA, checks) as cc:
            status = torch.zeros(1, dtype=torch.int32, device=dev)
            forms.append(cc.check_encoded(*d, status=status) + (status,))
            if not list_has_string_regex(cl):
                status = torch.zeros(1, dtype=torch.int32, device=dev)
                forms.append(hdx.check_encoded(gen.SCHEMA, *d, checks, status=status) + (status,))
            torch.cuda.synchronize()
        for ff, match, status in forms:
            assert np.array_equal(ff.cpu().numpy().view(np.uint32), want), cl
            assert np.array_equal(match.cpu().numpy().view(np.uint64), np.nonzero(want == len(cl))[0].astype(np.uint64)), cl
            assert int(status.item()) == 0


def expected_top(signs, members, keep, descending, limit):
    """sorted() over the fixture's sign matrix: the kept end by (value, index), then the output's direction
    with ascending indices among ties.  members[i] is object i's row of the matrix."""
    def order(idx, sign):
        def cmp(i, j):
            return sign * int(signs[members[i], members[j]]) or (i > j) - (i < j)
        return sorted(idx, key=functools.cmp_to_key(cmp))
    kept = order(range(len(members)), -1 if keep == KEEP_LARGEST else 1)[:limit]
    return order(kept, -1 if descending else 1)


@pytest.mark.gpu
@pytest.mark.parametrize("T", gen.TYPES)
def test_gpu_sort_order(torch_gpu, T):
    """The compare pool (FLOAT: without the NaNs, whose place is the library's own rule) as objects under
    [T, T], sorted by the key and by the attribute with no checks: both keeps, both directions, limits 1,
    |pool| - 1 and |pool| + 1.  The expected top comes from the fixture's signs alone."""
    from test_sorted_search import is_nan
    torch = torch_gpu
    pin = Pin.get()
    pool = gen.compare_pool(T)
    members = [i for i, v in enumerate(pool) if not (T == FLOAT and is_nan(v))]
    members = members[3:] + members[:3]  # not in the pool's own order
    if T == STRING:
        assert sum(pool[i][:8] == gen.BASE[:8] and len(pool[i]) > 8 for i in members) >= 10  # compare_stored decides
    objs = [(pool[i], [pool[i]]) for i in members]
    types = [T, T]
    dev = torch.device("cuda", 0)
    d = to_dev(torch, encode(types, objs, "keycol"))
    n = len(members)
    for attr in (0, 1):
        for keep in (KEEP_SMALLEST, KEEP_LARGEST):
            for desc in (0, 1):
                for limit in (1, n - 1, n + 1):
                    status = torch.zeros(1, dtype=torch.int32, device=dev)
                    ff, top = hdx.sorted_search(types, *d, [], SortSpec(attr, keep, desc), limit, status=status)
                    torch.cuda.synchronize()
                    assert top.cpu().tolist() == expected_top(pin.signs[T], members, keep, desc, limit), \
                        (attr, keep, desc, limit)
                    assert int(status.item()) == 0 and not ff.cpu().numpy().any()
