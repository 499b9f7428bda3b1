// regex_checks_test.cc — hdx_regex_match and the compiled list of checks
// (hdx_checks_compile / _passes / _free; hyperdex_amd/csrc/hdx_cpu.cpp) from a
// stand-alone C++ caller: built by tests/test_regex_checks.py together with
// hdx_cpu.cpp under -fsanitize=address,undefined, run as a program; no device,
// no Python.  Patterns, texts, types and check values live in heap buffers of
// exactly their size and are freed as soon as the contract allows, so a read
// past any of them, or of memory the handle should have copied, is reported.
// The expected results are worked by hand from the grammar of include/hdxhash.h.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

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

static const uint32_t STRING = 9217, INT64 = 9218, LIST_STRING = 9281;
static const uint32_t P_REGEX = 9733, P_GE = 9731;

// The bytes of s in a heap buffer of exactly s.size() bytes (NULL when empty).
static uint8_t* exact(const std::string& s) {
    if (s.empty()) return nullptr;
    uint8_t* p = (uint8_t*)malloc(s.size());
    memcpy(p, s.data(), s.size());
    return p;
}

// regex_match(re, text), both at the end of exactly-sized heap buffers.
static int match(const std::string& re, const std::string& text) {
    uint8_t *r = exact(re), *t = exact(text);
    int m = -1;
    CHECK(hdx_regex_match(r, re.size(), t, text.size(), &m) == HDX_OK);
    free(r);
    free(t);
    return m;
}

int main() {
    // texts of 0, 1, 7, 8, 9 bytes
    const std::string texts[] = {"", "a", "aaaaaab", "aaaaaaab", "aaaaaaaab"};
    for (const std::string& t : texts) {
        CHECK(match("", t) == 1);
        CHECK(match("$", t) == 1);
        CHECK(match("^$", t) == (t.empty() ? 1 : 0));
        CHECK(match("a", t) == (t.empty() ? 0 : 1));
        CHECK(match("b$", t) == (t.size() >= 7 ? 1 : 0));
        CHECK(match("^a*b$", t) == (t.size() >= 7 ? 1 : 0));
        CHECK(match("^a*$", t) == (t.size() <= 1 ? 1 : 0));
        CHECK(match("a.*b", t) == (t.size() >= 7 ? 1 : 0));
        CHECK(match("^.......$", t) == (t.size() == 7 ? 1 : 0));
        CHECK(match("........", t) == (t.size() >= 8 ? 1 : 0));
        CHECK(match("\\", t) == 0);
        CHECK(match("b\\", t) == 0);
        CHECK(match("\\a", t) == (t.empty() ? 0 : 1));
        CHECK(match("x*", t) == 1);
        CHECK(match("^x*y*z*b", t) == 0);
        CHECK(match("a$b", t) == 0);
    }
    CHECK(match("a**", "a*") == 1 && match("^a**$", "a*") == 1 && match("^a**$", "a") == 0);
    CHECK(match("$*a", "$$a") == 1 && match("^$*a", "b") == 0);
    CHECK(match("\x80.\xff", "a\x80z\xff") == 1 && match("\x80.\xff", "a\x80\xff") == 0);
    std::string lit63;
    for (int j = 0; j < 63; ++j) lit63.push_back((char)('a' + j % 26));
    CHECK(match(lit63, "zz" + lit63) == 1 && match(lit63, lit63.substr(0, 62)) == 0);
    CHECK(match("^" + lit63.substr(0, 62) + "$", lit63.substr(0, 62)) == 1);
    int m = 5;
    CHECK(hdx_regex_match((const uint8_t*)(lit63 + "a").data(), 64, (const uint8_t*)"a", 1, &m) == HDX_E_INVALID);
    CHECK(hdx_regex_match((const uint8_t*)(lit63 + "$").data(), 64, (const uint8_t*)"a", 1, &m) == HDX_E_INVALID);
    CHECK(hdx_regex_match(nullptr, 1, (const uint8_t*)"a", 1, &m) == HDX_E_INVALID && m == 5);
    // linear time: five stars against 4096 x 'a'
    const std::string as(4096, 'a');
    CHECK(match("a.*a.*a.*a.*a.*b", as) == 0 && match("^a.*a.*a.*a.*a.*$", as) == 1);

    // compile: the handle copies types and the checks' bytes
    {
        uint32_t* types = (uint32_t*)malloc(3 * sizeof(uint32_t));
        types[0] = STRING, types[1] = STRING, types[2] = INT64;
        const std::string p0 = "^k.*y$", p1 = "b.*a";
        uint8_t *v0 = exact(p0), *v1 = exact(p1), *v2 = exact(std::string(8, '\0'));
        hdx_attribute_check* cks = (hdx_attribute_check*)malloc(3 * sizeof(hdx_attribute_check));
        cks[0] = hdx_attribute_check{0, STRING, P_REGEX, 0, v0, p0.size()};
        cks[1] = hdx_attribute_check{1, STRING, P_REGEX, 0, v1, p1.size()};
        cks[2] = hdx_attribute_check{2, INT64, P_GE, 0, v2, 8};  // value >= 0
        hdx_checks h = nullptr;
        CHECK(hdx_checks_compile(types, 3, cks, 3, &h) == HDX_OK && h);
        free(types);
        free(v0);
        free(v1);
        free(v2);
        free(cks);
        struct Obj {
            std::string key, s;
            int64_t n;
            uint32_t want;
        };
        const Obj objs[] = {{"key", "xbxa", 5, 3},  {"key", "xbxa", -1, 2}, {"key", "ab", 5, 1},  {"kay", "", 5, 1},
                            {"keys", "ba", 5, 0},   {"", "ba", 5, 0},       {"ky", "ba", 0, 3}};
        for (const Obj& o : objs) {
            uint8_t *k = exact(o.key), *s = exact(o.s);
            uint8_t* nb = (uint8_t*)malloc(8);
            memcpy(nb, &o.n, 8);
            const uint8_t* values[2] = {s, nb};
            const size_t lens[2] = {o.s.size(), 8};
            uint32_t ff = 99;
            CHECK(hdx_checks_passes(h, k, o.key.size(), values, lens, &ff) == HDX_OK);
            CHECK(ff == o.want);
            free(k);
            free(s);
            free(nb);
        }
        uint32_t ff = 99;
        CHECK(hdx_checks_passes(h, nullptr, 0, nullptr, nullptr, &ff) == HDX_E_INVALID && ff == 99);
        hdx_checks_free(h);
    }
    // refusals leave *out alone
    {
        const uint32_t types[2] = {STRING, STRING}, bad[2] = {STRING, LIST_STRING};
        const uint8_t re[] = {'a'};
        hdx_attribute_check five[5];
        for (auto& c : five) c = hdx_attribute_check{1, STRING, P_REGEX, 0, re, 1};
        hdx_checks h = (hdx_checks)(uintptr_t)0x10;
        CHECK(hdx_checks_compile(types, 2, five, 5, &h) == HDX_E_INVALID && h == (hdx_checks)(uintptr_t)0x10);
        CHECK(hdx_checks_compile(bad, 2, five, 1, &h) == HDX_E_BADTYPE && h == (hdx_checks)(uintptr_t)0x10);
        CHECK(hdx_checks_compile(types, 2, five, 4, nullptr) == HDX_E_INVALID);
        const std::string long_re = lit63 + "a";
        hdx_attribute_check big{1, STRING, P_REGEX, 0, (const uint8_t*)long_re.data(), long_re.size()};
        CHECK(hdx_checks_compile(types, 2, &big, 1, &h) == HDX_E_INVALID && h == (hdx_checks)(uintptr_t)0x10);
        CHECK(hdx_checks_compile(types, 2, five, 4, &h) == HDX_OK);
        hdx_checks_free(h);
        CHECK(hdx_checks_compile(types, 2, nullptr, 0, &h) == HDX_OK);  // c == 0
        uint32_t ff = 99;
        const uint8_t* values[1] = {nullptr};
        const size_t lens[1] = {0};
        CHECK(hdx_checks_passes(h, nullptr, 0, values, lens, &ff) == HDX_OK && ff == 0);
        hdx_checks_free(h);
        hdx_checks_free(nullptr);
    }
    printf("regex_checks_test ok\n");
    return 0;
}
