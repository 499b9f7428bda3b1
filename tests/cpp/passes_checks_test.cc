// passes_checks_test.cc — hdx_passes_checks (hyperdex_amd/csrc/hdx_cpu.cpp) from
// a stand-alone C++ caller: built by tests/test_checks.py together with
// hdx_cpu.cpp, run as a program; no device, no Python.  Every key, value and
// check constant lives in a heap buffer of exactly its size.  The expected
// results are worked by hand from common/attribute_check.cc:123-237.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#include "hdx_host_common.h"
#include "hdxhash.h"

namespace hdx {
hdx_status fail(hdx_status s, const char*, ...) { return s; }
}  // namespace hdx

#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            exit(1);                                               \
        }                                                          \
    } while (0)

static const uint32_t STRING = 9217, INT64 = 9218, FLOAT = 9219, TS_DAY = 9476, TS_HOUR = 9475, LIST_STRING = 9281;
enum : uint32_t { P_FAIL = 9728, P_EQ = 9729, P_LE = 9730, P_GE = 9731, P_CLT = 9732, P_REGEX = 9733, P_LEN_EQ = 9734,
                  P_LEN_LE = 9735, P_LEN_GE = 9736, P_CONTAINS = 9737, P_LT = 9738, P_GT = 9739 };

static std::unique_ptr<uint8_t[]> exact(const std::string& s) {
    std::unique_ptr<uint8_t[]> p(new uint8_t[s.size() ? s.size() : 1]);
    if (!s.empty()) memcpy(p.get(), s.data(), s.size());
    return p;
}
static std::string le64(uint64_t v) {
    std::string s;
    for (int i = 0; i < 8; ++i) s.push_back((char)(v >> (8 * i)));
    return s;
}
static std::string f64(double d) {
    uint64_t b;
    memcpy(&b, &d, 8);
    return le64(b);
}

struct Ck {
    uint32_t attr, datatype, predicate;
    std::string value;
};

// schema [STRING key, STRING, INT64, FLOAT, TS_DAY]
static const uint32_t kTypes[5] = {STRING, STRING, INT64, FLOAT, TS_DAY};

static uint32_t run(const std::string& key, const std::vector<std::string>& attrs, const std::vector<Ck>& cks,
                    hdx_status want = HDX_OK) {
    std::vector<std::unique_ptr<uint8_t[]>> hold;
    std::vector<const uint8_t*> values;
    std::vector<size_t> lens;
    for (const std::string& a : attrs) {
        hold.push_back(exact(a));
        values.push_back(hold.back().get());
        lens.push_back(a.size());
    }
    std::vector<hdx_attribute_check> c(cks.size() ? cks.size() : 1);
    for (size_t i = 0; i < cks.size(); ++i) {
        hold.push_back(exact(cks[i].value));
        c[i] = hdx_attribute_check{cks[i].attr, cks[i].datatype, cks[i].predicate, 0, hold.back().get(),
                                   cks[i].value.size()};
    }
    auto k = exact(key);
    uint32_t ff = 0xabcd;
    CHECK(hdx_passes_checks(kTypes, 5, k.get(), key.size(), values.data(), lens.data(), c.data(), (uint32_t)cks.size(),
                            &ff) == want);
    return ff;
}

int main() {
    const std::string nan = le64(0x7ff8000000000000ULL);
    const std::vector<std::string> obj = {"hello world", le64((uint64_t)-5), f64(-0.0), ""};
    size_t cases = 0;
    auto one = [&](const Ck& c, bool want) {
        CHECK(run("key\x80", obj, {c}) == (want ? 1u : 0u));
        ++cases;
    };
    // strings: the check's value on the left; unsigned bytes; the shorter of equal prefixes first
    one({1, STRING, P_EQ, "hello world"}, true);
    one({1, STRING, P_EQ, "hello worle"}, false);
    one({1, STRING, P_LT, "hello worle"}, true);    // v < k
    one({1, STRING, P_LT, "hello world"}, false);
    one({1, STRING, P_LE, "hello world"}, true);
    one({1, STRING, P_GT, "hello"}, true);          // v > its proper prefix
    one({1, STRING, P_GE, "hello world!"}, false);
    one({0, STRING, P_GT, "key\x7f"}, true);        // 0x80 > 0x7f
    one({0, STRING, P_LT, "key\x7f"}, false);
    one({1, STRING, P_GE, ""}, true);
    // lengths: D == INT64, T == STRING
    one({1, INT64, P_LEN_EQ, le64(11)}, true);
    one({1, INT64, P_LEN_LE, le64(10)}, false);
    one({1, INT64, P_CLT, le64(11)}, true);         // shares LENGTH_LESS_EQUAL's code
    one({1, INT64, P_LEN_GE, le64((uint64_t)-1)}, true);
    one({1, INT64, P_LEN_GE, ""}, true);            // tmp = 0
    one({1, INT64, P_LEN_EQ, le64(11).substr(0, 3)}, false);  // 3 bytes: not an INT64
    one({1, INT64, P_LEN_EQ, le64(11) + "x"}, false);
    one({1, STRING, P_LEN_EQ, le64(11)}, false);    // D != INT64
    one({2, INT64, P_LEN_EQ, le64(8)}, false);      // an INT64 has no length
    // numerics: signed; empty = 0; exact type match
    one({2, INT64, P_EQ, le64((uint64_t)-5)}, true);
    one({2, INT64, P_GT, le64((uint64_t)-6)}, true);
    one({2, INT64, P_GT, ""}, false);               // -5 > 0
    one({2, INT64, P_LT, ""}, true);
    one({2, INT64, P_LE, le64(1).substr(0, 7)}, false);
    one({4, TS_DAY, P_EQ, le64(0)}, true);          // the empty value is 0
    one({4, TS_HOUR, P_EQ, le64(0)}, false);        // another granularity
    one({4, INT64, P_EQ, le64(0)}, false);
    one({3, FLOAT, P_EQ, f64(0.0)}, true);          // -0.0 equals 0.0
    one({3, FLOAT, P_EQ, nan}, true);               // a NaN compares 0 with everything
    one({3, FLOAT, P_LE, nan}, true);
    one({3, FLOAT, P_LT, nan}, false);
    one({3, FLOAT, P_GT, f64(-1.5)}, true);
    // the rest is false
    one({1, STRING, P_FAIL, "hello world"}, false);
    one({1, STRING, P_CONTAINS, "hello"}, false);
    one({1, STRING, 9800, "hello world"}, false);
    one({1, LIST_STRING, P_EQ, ""}, false);
    one({1, 12345, P_EQ, "hello world"}, false);
    one({1, INT64, P_REGEX, "h.*"}, false);
    one({2, STRING, P_REGEX, "h.*"}, false);
    one({5, STRING, P_EQ, ""}, false);              // attr >= attrs_sz
    // a mis-sized stored numeric fails every check on it, without an error
    std::vector<std::string> bad = obj;
    bad[1] = "12345";
    for (uint32_t p = P_FAIL; p <= P_GT; ++p) CHECK(run("k", bad, {{2, INT64, p, le64(0)}}) == 0);
    // lists: the first failing index, c when all pass, c == 0
    const std::vector<Ck> all = {{1, STRING, P_GE, "h"}, {0, STRING, P_EQ, "key\x80"}, {2, INT64, P_LE, le64(0)},
                                 {1, INT64, P_LEN_GE, le64(11)}, {3, FLOAT, P_GE, f64(0.0)}};
    CHECK(run("key\x80", obj, all) == 5);
    for (size_t f = 0; f < all.size(); ++f) {
        std::vector<Ck> l = all;
        l[f].predicate = P_FAIL;
        CHECK(run("key\x80", obj, l) == f);
    }
    CHECK(run("key\x80", obj, {}) == 0);
    CHECK(run("key\x80", obj, std::vector<Ck>(16, all[0])) == 16);
    // a 1100-byte constant against a 1100-byte attribute that differs in the last byte
    std::string big(1100, 'q'), big2 = big;
    big2[1099] = 'r';
    std::vector<std::string> o2 = obj;
    o2[0] = big;
    CHECK(run("k", o2, {{1, STRING, P_LT, big2}}) == 1);
    CHECK(run("k", o2, {{1, STRING, P_EQ, big2}}) == 0);
    CHECK(run("k", o2, {{1, STRING, P_EQ, big}}) == 1);
    // refusals leave *first_fail alone
    CHECK(run("k", obj, std::vector<Ck>(17, all[0]), HDX_E_INVALID) == 0xabcd);
    CHECK(run("k", obj, {{1, STRING, P_REGEX, "h.*"}}, HDX_E_BADTYPE) == 0xabcd);
    const uint32_t doc_types[2] = {STRING, 9223};
    const uint8_t* vals[1] = {nullptr};
    const size_t lens[1] = {0};
    const hdx_attribute_check c1 = {1, STRING, P_EQ, 0, nullptr, 0};
    uint32_t ff = 7;
    CHECK(hdx_passes_checks(doc_types, 2, nullptr, 0, vals, lens, &c1, 1, &ff) == HDX_E_BADTYPE && ff == 7);
    CHECK(hdx_passes_checks(nullptr, 2, nullptr, 0, vals, lens, &c1, 1, &ff) == HDX_E_INVALID && ff == 7);
    CHECK(hdx_passes_checks(kTypes, 2, nullptr, 0, vals, lens, &c1, 1, nullptr) == HDX_E_INVALID);
    CHECK(hdx_passes_checks(kTypes, 2, nullptr, 0, vals, lens, nullptr, 1, &ff) == HDX_E_INVALID && ff == 7);
    CHECK(hdx_passes_checks(kTypes, 2, nullptr, 0, vals, lens, nullptr, 0, &ff) == HDX_OK && ff == 0);
    printf("passes_checks_test ok: %zu single checks\n", cases);
    return 0;
}
