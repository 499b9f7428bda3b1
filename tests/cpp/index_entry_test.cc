// index_entry_test.cc — hdx_index_entry (hyperdex_amd/csrc/hdx_cpu.cpp) under
// AddressSanitizer + UndefinedBehaviorSanitizer: built by
// tests/test_index_entries.py together with hdx_cpu.cpp, run as a program.
// Every key, value and output lives in a heap buffer of exactly its size, so
// a read or write one byte outside any of them is reported.  The expected
// bytes are composed here from the table of include/hdxhash.h; the numeric
// encodings are worked by hand from common/ordered_encoding.cc:43-49,114-161.
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

static const uint32_t STRING = 9217, INT64 = 9218, FLOAT = 9219, TS_DAY = 9476, LIST_STRING = 9281;

static std::unique_ptr<uint8_t[]> exact(const std::string& s) {
    std::unique_ptr<uint8_t[]> p(new uint8_t[s.size() ? s.size() : 1]);
    if (!s.empty()) memcpy(p.get(), s.data(), s.size());
    return p;
}

static std::string be(uint64_t v, int bytes) {
    std::string s;
    for (int i = bytes - 1; i >= 0; --i) s.push_back((char)(v >> (8 * i)));
    return s;
}
static std::string le64(uint64_t v) {
    std::string s;
    for (int i = 0; i < 8; ++i) s.push_back((char)(v >> (8 * i)));
    return s;
}

// enc(type, value) for the values used below
static std::string enc(uint32_t type, const std::string& v, uint64_t ordered) {
    if (type == STRING) return v;
    if (type == FLOAT) return be(ordered, 8) + (v.empty() ? le64(0) : v);
    return be(ordered, 8);
}

static hdx_index_spec spec_of(uint16_t attr, const std::string& prefix) {
    hdx_index_spec s;
    memset(&s, 0, sizeof s);
    s.attr = attr;
    s.prefix_len = (uint8_t)prefix.size();
    memcpy(s.prefix, prefix.data(), prefix.size() < sizeof s.prefix ? prefix.size() : sizeof s.prefix);
    return s;
}

struct Val {
    uint32_t type;
    std::string bytes;
    uint64_t ordered;  // the ordered encoding of a numeric
};

int main() {
    const uint64_t one = 1, minus_two = (uint64_t)-2;
    const uint64_t d_one = 0x3ff0000000000000ULL;  // 1.0
    std::vector<Val> vals = {
        {STRING, "", 0},
        {STRING, "a", 0},
        {STRING, std::string(40, 'x') + "tail", 0},
        {STRING, std::string(1100, 'q'), 0},
        {INT64, "", 0x8000000000000000ULL},
        {INT64, le64(one), 0x8000000000000001ULL},
        {INT64, le64(minus_two), 0x7ffffffffffffffeULL},
        {TS_DAY, le64(one), 0x8000000000000001ULL},  // the int64 encoding, not the calendar hash
        {FLOAT, "", 0x8000000000000001ULL},          // 0.0
        {FLOAT, le64(d_one), (d_one | 0x8000000000000000ULL) + 2},
    };
    const std::string prefixes[] = {"i", "i\x05\x07", std::string("i") + std::string(20, '\x81')};
    size_t cases = 0;
    for (const std::string& prefix : prefixes)
        for (const Val& k : vals)
            for (const Val& v : vals) {
                const hdx_index_spec s = spec_of(3, prefix);
                std::string want = prefix + enc(v.type, v.bytes, v.ordered) + enc(k.type, k.bytes, k.ordered);
                if (k.type == STRING && v.type == STRING) want += be(k.bytes.size(), 4);
                auto kb = exact(k.bytes), vb = exact(v.bytes);
                size_t len = 0;
                // one byte short: the size is reported, nothing is written
                if (want.size() > 1) {
                    std::unique_ptr<uint8_t[]> small(new uint8_t[want.size() - 1]);
                    memset(small.get(), 0xA5, want.size() - 1);
                    CHECK(hdx_index_entry(&s, k.type, kb.get(), k.bytes.size(), v.type, vb.get(), v.bytes.size(),
                                          small.get(), want.size() - 1, &len) == HDX_E_NOMEM);
                    CHECK(len == want.size());
                    for (size_t b = 0; b + 1 < want.size(); ++b) CHECK(small[b] == 0xA5);
                }
                std::unique_ptr<uint8_t[]> out(new uint8_t[want.size()]);
                len = 0;
                CHECK(hdx_index_entry(&s, k.type, kb.get(), k.bytes.size(), v.type, vb.get(), v.bytes.size(),
                                      out.get(), want.size(), &len) == HDX_OK);
                CHECK(len == want.size());
                CHECK(memcmp(out.get(), want.data(), want.size()) == 0);
                ++cases;
            }
    // refusals
    uint8_t out[64];
    size_t len = 99;
    const hdx_index_spec s = spec_of(1, "i\x01\x02");
    for (size_t bad : {1, 2, 3, 4, 5, 6, 7, 9}) {
        auto b = exact(std::string(bad, 'z'));
        // the size is still reported: a numeric's encoded size does not depend on its value
        CHECK(hdx_index_entry(&s, STRING, b.get(), 0, INT64, b.get(), bad, out, sizeof out, &len) == HDX_E_BADSIZE);
        CHECK(len == 3 + 8 + 0);
        CHECK(hdx_index_entry(&s, FLOAT, b.get(), bad, STRING, b.get(), 0, out, sizeof out, &len) == HDX_E_BADSIZE);
        CHECK(len == 3 + 0 + 16);
    }
    CHECK(hdx_index_entry(&s, LIST_STRING, out, 0, STRING, out, 0, out, sizeof out, &len) == HDX_E_BADTYPE);
    CHECK(hdx_index_entry(&s, STRING, out, 0, LIST_STRING, out, 0, out, sizeof out, &len) == HDX_E_BADTYPE);
    CHECK(hdx_index_entry(&s, STRING, out, 0, 12345, out, 0, out, sizeof out, &len) == HDX_E_BADTYPE);
    CHECK(len == 0);  // no size exists
    hdx_index_spec z = spec_of(0, "i");
    CHECK(hdx_index_entry(&z, STRING, out, 0, STRING, out, 0, out, sizeof out, &len) == HDX_E_INVALID);
    z = spec_of(1, "");
    CHECK(hdx_index_entry(&z, STRING, out, 0, STRING, out, 0, out, sizeof out, &len) == HDX_E_INVALID);
    z = spec_of(1, "i");
    z.prefix_len = HDX_INDEX_PREFIX_MAX + 1;
    CHECK(hdx_index_entry(&z, STRING, out, 0, STRING, out, 0, out, sizeof out, &len) == HDX_E_INVALID);
    CHECK(hdx_index_entry(nullptr, STRING, out, 0, STRING, out, 0, out, sizeof out, &len) == HDX_E_INVALID);
    CHECK(hdx_index_entry(&s, STRING, out, 0, STRING, out, 0, out, sizeof out, nullptr) == HDX_E_INVALID);
    printf("index_entry_test ok: %zu entries\n", cases);
    return 0;
}
