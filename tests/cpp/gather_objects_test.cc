// gather_objects_test.cc — hdx_gather_objects (hyperdex_amd/csrc/hdx_cpu.cpp)
// under AddressSanitizer + UndefinedBehaviorSanitizer: built by
// tests/test_gather_objects.py together with hdx_cpu.cpp, run as a program.
// The stores, the index list, rec_off, rec_key_len and the output live in heap
// buffers of exactly their sizes, so a read or write one byte outside any of
// them is reported.  The expected bytes are composed here by slicing.
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

template <typename T>
static std::unique_ptr<T[]> exact(const std::vector<T>& v) {
    std::unique_ptr<T[]> p(new T[v.size() ? v.size() : 1]);
    for (size_t i = 0; i < v.size(); ++i) p[i] = v[i];
    return p;
}

static uint32_t g_rng = 12345;
static uint32_t rnd() { return g_rng = g_rng * 1664525u + 1013904223u; }
static std::string bytes(size_t n) {
    std::string s;
    for (size_t i = 0; i < n; ++i) s.push_back((char)(rnd() >> 24));
    return s;
}

struct Store {
    std::vector<std::string> key, val;
    std::vector<uint8_t> keys, vals;
    std::vector<uint64_t> key_off, val_off;
    std::vector<uint32_t> key_len, val_len;
};

// records: keys and values in one store, [key][value] back to back
static Store make(const std::vector<size_t>& klens, const std::vector<size_t>& vlens, bool records) {
    Store s;
    for (size_t i = 0; i < klens.size(); ++i) {
        s.key.push_back(bytes(klens[i]));
        s.val.push_back(bytes(vlens[i]));
        std::vector<uint8_t>& kb = s.keys;
        std::vector<uint8_t>& vb = records ? s.keys : s.vals;
        s.key_off.push_back(kb.size());
        kb.insert(kb.end(), s.key[i].begin(), s.key[i].end());
        s.val_off.push_back(vb.size());
        vb.insert(vb.end(), s.val[i].begin(), s.val[i].end());
        s.key_len.push_back((uint32_t)klens[i]);
        s.val_len.push_back((uint32_t)vlens[i]);
    }
    if (records) s.vals = s.keys;
    return s;
}

static size_t run(const Store& s, const std::vector<uint64_t>& idx, uint32_t what) {
    const uint64_t n = s.key.size(), count = idx.size();
    std::string want;
    std::vector<uint64_t> off{0};
    std::vector<uint32_t> kls;
    uint32_t bits = 0;
    for (uint64_t i : idx) {
        uint32_t kl = 0;
        if (i >= n) {
            bits |= 1u << HDX_E_INVALID;
        } else {
            if (what & HDX_GATHER_KEYS) want += s.key[i], kl = (uint32_t)s.key[i].size();
            if (what & HDX_GATHER_VALUES) want += s.val[i];
        }
        kls.push_back(kl);
        off.push_back(want.size());
    }
    auto keys = exact(s.keys), vals = exact(s.vals);
    auto key_off = exact(s.key_off), val_off = exact(s.val_off);
    auto key_len = exact(s.key_len), val_len = exact(s.val_len);
    auto ix = exact(idx);
    // a part that is not asked for may be absent
    const uint8_t* kp = (what & HDX_GATHER_KEYS) ? keys.get() : nullptr;
    const uint64_t* kop = (what & HDX_GATHER_KEYS) ? key_off.get() : nullptr;
    const uint8_t* vp = (what & HDX_GATHER_VALUES) ? vals.get() : nullptr;
    const uint64_t* vop = (what & HDX_GATHER_VALUES) ? val_off.get() : nullptr;
    std::unique_ptr<uint64_t[]> rec_off(new uint64_t[count + 1]);
    std::unique_ptr<uint32_t[]> rec_kl(new uint32_t[count ? count : 1]);
    if (!want.empty()) {  // one byte short: the offsets are filled, nothing is written
        std::unique_ptr<uint8_t[]> small(new uint8_t[want.size() - 1 ? want.size() - 1 : 1]);
        memset(small.get(), 0xA5, want.size() - 1);
        uint32_t status = 0;
        CHECK(hdx_gather_objects(kp, kop, key_len.get(), vp, vop, val_len.get(), n, ix.get(), count, what,
                                 rec_off.get(), rec_kl.get(), small.get(), want.size() - 1, &status) == HDX_E_NOMEM);
        CHECK(status == (bits | (1u << HDX_E_NOMEM)));
        for (uint64_t r = 0; r <= count; ++r) CHECK(rec_off[r] == off[r]);
        for (size_t b = 0; b + 1 < want.size(); ++b) CHECK(small[b] == 0xA5);
    }
    std::unique_ptr<uint8_t[]> out(new uint8_t[want.size() ? want.size() : 1]);
    uint32_t status = 0;
    CHECK(hdx_gather_objects(kp, kop, key_len.get(), vp, vop, val_len.get(), n, ix.get(), count, what, rec_off.get(),
                             rec_kl.get(), out.get(), want.size(), &status) == HDX_OK);
    CHECK(status == bits);
    for (uint64_t r = 0; r <= count; ++r) CHECK(rec_off[r] == off[r]);
    for (uint64_t r = 0; r < count; ++r) CHECK(rec_kl[r] == kls[r]);
    CHECK(memcmp(out.get(), want.data(), want.size()) == 0);
    // rec_key_len and status may be NULL
    CHECK(hdx_gather_objects(kp, kop, key_len.get(), vp, vop, val_len.get(), n, ix.get(), count, what, rec_off.get(),
                             nullptr, out.get(), want.size(), nullptr) == HDX_OK);
    CHECK(memcmp(out.get(), want.data(), want.size()) == 0);
    return want.size();
}

int main() {
    const uint32_t K = HDX_GATHER_KEYS, V = HDX_GATHER_VALUES;
    size_t total = 0, cases = 0;
    for (int records = 0; records < 2; ++records) {
        // the edge records of the device tests: empty keys and values, 8-byte keys, sizes 0..40, one long record
        std::vector<size_t> kl, vl;
        for (size_t i = 0; i < 41; ++i) kl.push_back(i % 18), vl.push_back(i);
        kl.push_back(0), vl.push_back(0);
        kl.push_back(8), vl.push_back(0);
        kl.push_back(0), vl.push_back(3 * 4096 + 5);
        kl.push_back(64), vl.push_back(1100);
        const Store s = make(kl, vl, records != 0);
        const uint64_t n = kl.size();
        std::vector<uint64_t> asc, desc, dup, bad, none;
        for (uint64_t i = 0; i < n; ++i) asc.push_back(i), desc.push_back(n - 1 - i);
        for (uint64_t i = 0; i < 2 * n; ++i) dup.push_back(rnd() % n);
        bad = dup;
        bad[0] = n, bad[5] = UINT64_MAX, bad[bad.size() - 1] = 1ull << 40;
        for (uint32_t what : {K, V, K | V})
            for (const std::vector<uint64_t>* idx : {&asc, &desc, &dup, &bad, &none}) {
                total += run(s, *idx, what);
                ++cases;
            }
    }
    // refusals: nothing is dereferenced
    uint8_t b[8];
    uint64_t o[2] = {0, 0};
    uint32_t l[1] = {0};
    CHECK(hdx_gather_objects(b, o, l, b, o, l, 1, o, 1, 0, o, l, b, 8, nullptr) == HDX_E_INVALID);
    CHECK(hdx_gather_objects(b, o, l, b, o, l, 1, o, 1, 4, o, l, b, 8, nullptr) == HDX_E_INVALID);
    CHECK(hdx_gather_objects(nullptr, o, l, b, o, l, 1, o, 1, K, o, l, b, 8, nullptr) == HDX_E_INVALID);
    CHECK(hdx_gather_objects(b, o, l, nullptr, o, l, 1, o, 1, V, o, l, b, 8, nullptr) == HDX_E_INVALID);
    CHECK(hdx_gather_objects(b, o, l, b, o, l, 1, nullptr, 1, K, o, l, b, 8, nullptr) == HDX_E_INVALID);
    CHECK(hdx_gather_objects(b, o, l, b, o, l, 1, o, 1, K, nullptr, l, b, 8, nullptr) == HDX_E_INVALID);
    CHECK(hdx_gather_objects(b, o, l, b, o, l, 1, o, 1, K, o, l, nullptr, 8, nullptr) == HDX_E_INVALID);
    CHECK(hdx_gather_objects(b, o, l, b, o, l, 1, o, (1ull << 40) + 1, K, o, l, b, 8, nullptr) == HDX_E_INVALID);
    CHECK(hdx_gather_objects(b, o, l, b, o, l, (1ull << 40) + 1, o, 1, K, o, l, b, 8, nullptr) == HDX_E_INVALID);
    printf("gather_objects_test ok: %zu cases, %zu bytes\n", cases, total);
    return 0;
}
