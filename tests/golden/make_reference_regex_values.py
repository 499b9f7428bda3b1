"""Inputs for the regex_match pin, and the generator of its fixture.

tests/golden/reference_regex_values.json holds what the reference's own
regex_match (common/regex_match.cc) returns for the (pattern, text) pairs built
here.  The generator compiles that file where it lies, unmodified, together
with a few-line C-linkage driver written below, into a temporary directory
outside the tree, and records one result bit per case.  The fixture is data
only: a digest of the inputs and the result bits.  No restatement (hdx_regex.h,
the tests' Python matcher) takes part in producing it.

    python tests/golden/make_reference_regex_values.py    # needs the reference (REF, as oracle/Makefile) and a C++ compiler

tests/test_regex_checks.py imports this module for the inputs and, where the
reference and a compiler are present, regenerates the fixture and compares it
with the committed file.  Everything random comes from
make_reference_hash_values.py's counter-based splitmix64.
"""
import ctypes
import hashlib
import importlib.util
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "reference_regex_values.json")
REF = os.environ.get("REF", "/root/reference")  # oracle/Makefile's default

DRIVER = """\
#include <stddef.h>
#include <stdint.h>
#include "common/regex_match.h"
extern "C" int ref_regex_match(const uint8_t* regex, size_t regex_sz, const uint8_t* text, size_t text_sz)
{
    return hyperdex::regex_match(regex, regex_sz, text, text_sz) ? 1 : 0;
}
"""


def _load_hash_generator():
    spec = importlib.util.spec_from_file_location("make_reference_hash_values",
                                                  os.path.join(HERE, "make_reference_hash_values.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


hgen = _load_hash_generator()

# ---- the hand-written edges --------------------------------------------------------------------

LIT63 = bytes(97 + j % 26 for j in range(63))          # 63 items, no END: the match needs bit 63
LIT64 = LIT63 + b"l"                                   # 64 items
EDGE_PATTERNS = [
    b"", b"^", b"$", b"^$", b"a$b", b"$a", b"a$", b"^a$", b"$*", b"$*a", b"a$*", b"**", b"**a", b"a**", b"*", b"*a",
    b"a^", b"a^b", b"^^", b"^*", b"^^*a", b"^*a", b"\\", b"a\\", b"^\\", b"\\\\", b"\\\\a", b"a\\\\", b"\\a*",
    b"\\a*b", b"\\.*", b"\\**", b"\\*", b"\\.", b"\\$", b"a\\$", b"\\^a", b".*", b".*a", b".*ab", b"a.*", b"ab.*",
    b"a.*b", b"^a.*b", b"a.*b$", b"^a.*b$", b"^.*$", b".*$", b"a*b*c*", b"a*b*c*d", b"^a*b*c*$", b"xa*b*c*y",
    b"a*.*b*", b"a*a*a*a", b"^a*a*a*$", b".", b"..", b"^..$", b"a.b", b"\x80", b"\x80*", b"^\x80*$", b"\x80.\xff",
    b"a\xffb", b".*\x80$", b"a", b"ab", b"^ab", b"ab$", b"abc", b"^abc", b"a.*b.*c$", b"b*", b"^b*$", b"b*$",
    LIT63, b"^" + LIT63, LIT63[:62] + b"$", b"^" + LIT63[:62] + b"$", LIT63[:62] + b"z*", LIT64, LIT63 + b"$",
    b"^" + LIT64, b"a*" * 32,
]  # nothing here makes the reference backtrack for long: these run through its recursion
EDGE_TEXTS = [
    b"", b"a", b"b", b"ab", b"ba", b"aa", b"abc", b"aab", b"abb", b"aabbcc", b"xaabbccy", b"xy", b"$", b"a$", b"a$b",
    b"*", b"**", b"*a", b"a*", b"^", b"a^", b"a^b", b"^a", b"\\", b"\\a", b"a\\", b"\\\\", b".", b"a.b", b"axb", b"acb",
    b"\x80", b"\x80\x80", b"\x80a\xff", b"a\xffb", b"a\x7fb", b"ab\x80", b"abcabc", b"xxabcxx", b"abxc", b"a-b-c",
    b"a-b-c-", b"bbb", b"bbba", b"aaaa", b"aaaaaaab", b"\x00", b"a\x00b", LIT63, b"x" + LIT63, LIT63 + b"x",
    LIT63[:62], LIT63[:62] + b"zzz", LIT63[:62] + b"y", LIT64, b"a" * 40, b"a" * 40 + b"b",
]


def edge_cases():
    return [(p, t) for p in EDGE_PATTERNS for t in EDGE_TEXTS]


# ---- the random cases --------------------------------------------------------------------------

RANDOM_CASES = 20000
PATTERN_ALPHABET = b"ab.*\\^$\x80"
TEXT_ALPHABET = b"aaaabbbb\x80.*$\\^ab"    # biased to a / b


def random_cases(n=RANDOM_CASES):
    """Patterns of length 0-8 over PATTERN_ALPHABET, texts of length 0-12 over TEXT_ALPHABET."""
    r = hgen.rnd(201, n * 24).reshape(n, 24)
    out = []
    for i in range(n):
        pl, tl = int(r[i, 0] % np.uint64(9)), int(r[i, 1] % np.uint64(13))
        p = bytes(PATTERN_ALPHABET[int(r[i, 2 + k] % np.uint64(len(PATTERN_ALPHABET)))] for k in range(pl))
        t = bytes(TEXT_ALPHABET[int(r[i, 10 + k] % np.uint64(len(TEXT_ALPHABET)))] for k in range(tl))
        out.append((p, t))
    return out


def inputs_sha256(cases):
    h = hashlib.sha256()
    for p, t in cases:
        h.update(len(p).to_bytes(4, "little") + p + len(t).to_bytes(4, "little") + t)
    return h.hexdigest()


def pack_bits(bits):
    """One bit per case, case i at bit i % 8 of byte i // 8, as hex."""
    return np.packbits(np.asarray(bits, np.uint8), bitorder="little").tobytes().hex()


def unpack_bits(text, n):
    return np.unpackbits(np.frombuffer(bytes.fromhex(text), np.uint8), bitorder="little")[:n].astype(bool)


# ---- the reference -----------------------------------------------------------------------------

def compiler():
    return shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")


def available():
    return os.path.exists(os.path.join(REF, "common", "regex_match.cc")) and compiler() is not None


def reference_results(groups):
    """[[0 / 1 per case] per group] from the reference's regex_match, compiled in a temporary directory."""
    with tempfile.TemporaryDirectory(prefix="ref_regex_") as tmp:
        drv, lib = os.path.join(tmp, "ref_regex_driver.cc"), os.path.join(tmp, "libref_regex.so")
        with open(drv, "w") as f:
            f.write(DRIVER)
        subprocess.run([compiler(), "-O2", "-std=c++11", "-fPIC", "-shared", "-I" + REF, "-I" + os.path.join(REF, "include"),
                        "-o", lib, drv, os.path.join(REF, "common", "regex_match.cc")], check=True, timeout=300)
        fn = ctypes.CDLL(lib).ref_regex_match
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t]
        return [[int(fn(p, len(p), t, len(t))) for p, t in cases] for cases in groups]


def build_fixture() -> dict:
    edges, rand = edge_cases(), random_cases()
    e_bits, r_bits = reference_results([edges, rand])
    true = sum(r_bits) / len(r_bits)
    assert 0.10 <= true <= 0.90, true  # each outcome at least a tenth of the random cases
    return {"source": "regex_match of the reference's common/regex_match.cc, compiled unmodified with a C-linkage "
                      "driver; inputs from tests/golden/make_reference_regex_values.py",
            "edge": {"cases": len(edges), "inputs_sha256": inputs_sha256(edges), "matched": pack_bits(e_bits)},
            "random": {"cases": len(rand), "inputs_sha256": inputs_sha256(rand), "matched": pack_bits(r_bits),
                       "true_fraction": round(true, 4)}}


def dumps(fixture: dict) -> str:
    return json.dumps(fixture, indent=None, separators=(",", ":"), sort_keys=True) + "\n"


def main(out=FIXTURE):
    text = dumps(build_fixture())
    with open(out, "w") as f:
        f.write(text)
    print("wrote", out, len(text), "bytes")


if __name__ == "__main__":
    main(*sys.argv[1:])
