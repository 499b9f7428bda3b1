// sorted_search_test.cc — hdx_sorted_search and hdx_compare (hyperdex_amd/csrc/
// hdx_cpu.cpp) from a stand-alone C++ caller: built by tests/
// test_sorted_search.py together with hdx_cpu.cpp under -fsanitize=address,
// undefined, run as a program; no device, no Python.  The stores, offsets,
// check constants and outputs live in heap buffers of exactly their size, so
// a read or write past any of them is reported.  The expected results are
// worked by hand from the contract of include/hdxhash.h.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

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

static const uint32_t STRING = 9217, INT64 = 9218, FLOAT = 9219, LIST_STRING = 9281;
static const uint32_t P_LEN_GE = 9736;

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
static std::string be32(uint32_t v) {
    std::string s;
    for (int i = 3; i >= 0; --i) s.push_back((char)(v >> (8 * i)));
    return s;
}

// A stored value: version, count, then [u32 BE length][bytes] per attribute.
static std::string value_of(const std::vector<std::string>& attrs) {
    std::string s(8, '\0');
    s.push_back((char)(attrs.size() >> 8));
    s.push_back((char)attrs.size());
    for (const std::string& a : attrs) s += be32((uint32_t)a.size()) + a;
    return s;
}

template <typename T>
static T* exact(const std::vector<T>& v) {
    T* p = (T*)malloc(v.size() ? v.size() * sizeof(T) : 1);
    if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
}

struct Store {
    uint8_t *keys, *vals;
    uint64_t *key_off, *val_off;
    uint32_t *key_len, *val_len;
    uint64_t n;
    Store(const std::vector<std::string>& k, const std::vector<std::string>& v) : n(k.size()) {
        std::vector<uint8_t> kb, vb;
        std::vector<uint64_t> ko, vo;
        std::vector<uint32_t> kl, vl;
        for (uint64_t i = 0; i < n; ++i) {
            ko.push_back(kb.size());
            kl.push_back((uint32_t)k[i].size());
            kb.insert(kb.end(), k[i].begin(), k[i].end());
            vo.push_back(vb.size());
            vl.push_back((uint32_t)v[i].size());
            vb.insert(vb.end(), v[i].begin(), v[i].end());
        }
        keys = exact(kb), vals = exact(vb), key_off = exact(ko), val_off = exact(vo), key_len = exact(kl),
        val_len = exact(vl);
    }
    ~Store() {
        free(keys), free(vals), free(key_off), free(val_off), free(key_len), free(val_len);
    }
};

static std::vector<uint64_t> search(const uint32_t* types, uint32_t A, const Store& s, const hdx_attribute_check* ck,
                                    uint32_t c, hdx_sort_spec sort, uint64_t limit, uint32_t* status) {
    const uint64_t cap = limit < s.n ? limit : s.n;
    uint64_t* top = (uint64_t*)malloc(cap ? cap * 8 : 1);  // exactly min(limit, n) indices
    uint64_t count = 99;
    *status = 0;
    CHECK(hdx_sorted_search(types, A, s.keys, s.key_off, s.key_len, s.vals, s.val_off, s.val_len, s.n, ck, c, &sort,
                            limit, top, &count, status) == HDX_OK);
    CHECK(count <= cap);
    std::vector<uint64_t> out(top, top + count);
    free(top);
    return out;
}

typedef std::vector<uint64_t> V;

int main() {
    const uint32_t types[3] = {STRING, INT64, FLOAT};
    const uint64_t nan1 = 0x7ff8000000000001ull, nan2 = 0xfff0000000000123ull;
    // index:                        0     1     2     3     4     5       6      7     8
    const int64_t iv[9] = {5, 1, 9, 3, 7, 2, 8, 3, 3};
    const std::string fv[9] = {f64(1.5), le64(nan1), f64(-0.0), f64(0.0), le64(nan2), f64(-1e300), f64(1e300), "", f64(1.5)};
    std::vector<std::string> keys, vals;
    for (int i = 0; i < 9; ++i) {
        keys.push_back(i == 4 ? "k" : "key" + std::to_string(i));  // object 4 fails the check
        vals.push_back(value_of({i == 7 ? std::string("\1\2\3") : le64((uint64_t)iv[i]), fv[i]}));
    }
    vals[6] = vals[6].substr(0, vals[6].size() - 1);  // object 6 does not decode
    const Store s(keys, vals);
    // the check's constant in a buffer of exactly its size
    const std::string two = le64(2);
    uint8_t* konst = (uint8_t*)malloc(8);
    memcpy(konst, two.data(), 8);
    const hdx_attribute_check ck[1] = {{0, INT64, P_LEN_GE, 0, konst, 8}};
    uint32_t st;
    // INT64: object 7 is mis-sized (left out, its bit), 6 undecodable, 4 does not match: S = {0, 1, 2, 3, 5, 8}
    const uint32_t both = (1u << HDX_E_BADSIZE) | (1u << HDX_E_BADENC);
    CHECK(search(types, 3, s, ck, 1, {1, HDX_KEEP_SMALLEST, 0, 0}, 3, &st) == (V{1, 5, 3}) && st == both);
    CHECK(search(types, 3, s, ck, 1, {1, HDX_KEEP_SMALLEST, 1, 0}, 4, &st) == (V{3, 8, 5, 1}));  // 3, 3, 2, 1
    CHECK(search(types, 3, s, ck, 1, {1, HDX_KEEP_LARGEST, 0, 0}, 3, &st) == (V{3, 0, 2}));      // the tie at 3: index 3
    CHECK(search(types, 3, s, ck, 1, {1, HDX_KEEP_LARGEST, 1, 0}, 100, &st) == (V{2, 0, 3, 8, 5, 1}));
    CHECK(search(types, 3, s, ck, 1, {1, HDX_KEEP_LARGEST, 1, 0}, 0, &st).empty() && st == both);
    // FLOAT: S = {0, 1, 2, 3, 5, 7, 8}; NaN above everything, -0.0 == 0.0 == empty
    CHECK(search(types, 3, s, ck, 1, {2, HDX_KEEP_SMALLEST, 0, 0}, 9, &st) == (V{5, 2, 3, 7, 0, 8, 1}));
    CHECK(st == (1u << HDX_E_BADENC));
    CHECK(search(types, 3, s, ck, 1, {2, HDX_KEEP_LARGEST, 1, 0}, 2, &st) == (V{1, 0}));
    // the key, and beyond the schema
    CHECK(search(types, 3, s, ck, 1, {0, HDX_KEEP_LARGEST, 0, 0}, 2, &st) == (V{7, 8}));
    CHECK(search(types, 3, s, ck, 1, {3, HDX_KEEP_LARGEST, 1, 0}, 4, &st) == (V{0, 1, 2, 3}));
    CHECK(search(types, 3, s, nullptr, 0, {77, HDX_KEEP_SMALLEST, 0, 0}, 1u << 20, &st) == (V{0, 1, 2, 3, 4, 5, 7, 8}));
    // refusals leave the outputs alone
    uint64_t top[1] = {42}, count = 42;
    hdx_sort_spec bad = {1, 2, 0, 0};
    CHECK(hdx_sorted_search(types, 3, s.keys, s.key_off, s.key_len, s.vals, s.val_off, s.val_len, s.n, ck, 1, &bad, 1,
                            top, &count, nullptr) == HDX_E_INVALID);
    const uint32_t lists[2] = {STRING, LIST_STRING};
    hdx_sort_spec on_list = {1, 0, 0, 0};
    CHECK(hdx_sorted_search(lists, 2, s.keys, s.key_off, s.key_len, s.vals, s.val_off, s.val_len, s.n, nullptr, 0,
                            &on_list, 1, top, &count, nullptr) == HDX_E_BADTYPE);
    CHECK(top[0] == 42 && count == 42);
    // hdx_compare on operands of exactly their size
    int cmp = 7;
    uint8_t* a = (uint8_t*)malloc(2);
    uint8_t* b = (uint8_t*)malloc(3);
    memcpy(a, "ab", 2);
    memcpy(b, "ab\0", 3);
    CHECK(hdx_compare(STRING, a, 2, b, 3, &cmp) == HDX_OK && cmp == -1);
    CHECK(hdx_compare(STRING, b, 3, a, 2, &cmp) == HDX_OK && cmp == 1);
    CHECK(hdx_compare(STRING, a, 0, b, 0, &cmp) == HDX_OK && cmp == 0);
    CHECK(hdx_compare(INT64, konst, 8, nullptr, 0, &cmp) == HDX_OK && cmp == 1);
    CHECK(hdx_compare(FLOAT, (const uint8_t*)&nan1, 8, konst, 8, &cmp) == HDX_OK && cmp == 0);
    cmp = 7;
    CHECK(hdx_compare(INT64, a, 2, konst, 8, &cmp) == HDX_E_BADSIZE && cmp == 7);
    CHECK(hdx_compare(LIST_STRING, a, 2, b, 3, &cmp) == HDX_E_BADTYPE && cmp == 7);
    free(a), free(b), free(konst);
    printf("sorted_search_test ok\n");
    return 0;
}
