// hdx_cpu.cpp — the per-object entry points of libhdxhash.so on the host CPU.
//
// The reference's hash() is an in-process CPU leaf (common/hash.cc:34-68),
// reached per object from the client library (client/client.cc:1240 ->
// configuration::point_leader, common/configuration.cc:438,475), from
// configuration::lookup_search (:819,833,843) and from the daemon's
// key_state::hash_objects (daemon/key_state.cc:1477-1517) — on hosts with or
// without an MI355X, one object per call, from every network thread at once.
// A GPU round trip per object would cost tens of microseconds against a
// fraction of one on a core, so these signatures are served here, by design:
//
//   hdx_hash_value   hash(hyperdatatype, const e::slice&)      common/hash.cc:34-46
//   hdx_hash_key     hash(const schema&, key, uint64_t* h)     common/hash.cc:48-54
//   hdx_hash_object  hash(const schema&, key, value, hs)       common/hash.cc:56-68
//
// The same goes for one object's index entry, one object's attribute checks
// and the reference's compare (hdx_index_entry, hdx_passes_checks,
// hdx_compare), and for the sorted search over host-resident stored objects
// (hdx_sorted_search: the daemon's own loop for what the device form leaves
// to it; the one entry point here that allocates).
// Every batch entry point (hdx_hash_batch_*, the sweep, the fused lookups, the
// batcher) runs the gfx950 kernels only; nothing here is a fallback for them.
// Pure, reentrant, lock-free, no allocation, no HIP call: works on a host with
// no GPU.  Bit-exact with the kernels (hdx_device_hash.h) and the reference:
//   CityHash64 v1.1         cityhash/city.cc:255-397, city.h:100-109
//   ordered_encode_int64    common/ordered_encoding.cc:43-49
//   ordered_encode_double   common/ordered_encoding.cc:114-161
//   timestamp calendar hash common/datatype_timestamp.cc:117-219
// Built without -ffast-math: the timestamp hash needs an IEEE division.
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <new>

#include "hdx_cpu.h"
#include "hdx_host_common.h"

namespace hdx {
namespace cpu {
namespace {

constexpr uint64_t kK0 = 0xc3a5c85c97cb3127ULL;
constexpr uint64_t kK1 = 0xb492b66fbe98f273ULL;
constexpr uint64_t kK2 = 0x9ae16a3b2f90404fULL;
constexpr uint64_t kMul128 = 0x9ddfea08eb382d69ULL;  // Hash128to64, city.h:100-109

// Little-endian loads at any alignment (Fetch64/Fetch32, city.cc:107-113 on x86/arm64 LE)
inline uint64_t le64(const uint8_t* p) {
    uint64_t v;
    memcpy(&v, p, 8);
    return v;
}
inline uint32_t le32(const uint8_t* p) {
    uint32_t v;
    memcpy(&v, p, 4);
    return v;
}
inline uint64_t rotr(uint64_t v, unsigned r) { return (v >> r) | (v << ((64 - r) & 63)); }
inline uint64_t fold47(uint64_t v) { return v ^ (v >> 47); }

// HashLen16(u, v, mul) (city.cc:268-276); with kMul128 it is Hash128to64(u, v)
inline uint64_t murmur2x64(uint64_t u, uint64_t v, uint64_t mul) {
    const uint64_t a = fold47((u ^ v) * mul);
    return fold47((v ^ a) * mul) * mul;
}

// city.cc:278-301
inline uint64_t len_upto16(const uint8_t* s, uint64_t n) {
    if (n >= 8) {
        const uint64_t mul = kK2 + 2 * n;
        const uint64_t a = le64(s) + kK2;
        const uint64_t b = le64(s + n - 8);
        return murmur2x64(rotr(b, 37) * mul + a, (rotr(a, 25) + b) * mul, mul);
    }
    if (n >= 4) {
        const uint64_t mul = kK2 + 2 * n;
        return murmur2x64(n + ((uint64_t)le32(s) << 3), le32(s + n - 4), mul);
    }
    if (n == 0) return kK2;
    const uint32_t lo = (uint32_t)s[0] | ((uint32_t)s[n >> 1] << 8);  // unsigned bytes (:293-297)
    const uint32_t hi = (uint32_t)n + ((uint32_t)s[n - 1] << 2);
    return fold47((uint64_t)lo * kK2 ^ (uint64_t)hi * kK0) * kK2;
}

// city.cc:305-313
inline uint64_t len_17to32(const uint8_t* s, uint64_t n) {
    const uint64_t mul = kK2 + 2 * n;
    const uint64_t a = le64(s) * kK1, b = le64(s + 8);
    const uint64_t c = le64(s + n - 8) * mul, d = le64(s + n - 16) * kK2;
    return murmur2x64(rotr(a + b, 43) + rotr(c, 30) + d, a + rotr(b + kK2, 18) + c, mul);
}

// city.cc:340-359
inline uint64_t len_33to64(const uint8_t* s, uint64_t n) {
    const uint64_t mul = kK2 + 2 * n;
    uint64_t a = le64(s) * kK2;
    uint64_t b = le64(s + 8);
    const uint64_t c = le64(s + n - 24), d = le64(s + n - 32);
    const uint64_t e = le64(s + 16) * kK2, f = le64(s + 24) * 9;
    const uint64_t g = le64(s + n - 8), h = le64(s + n - 16) * mul;
    const uint64_t u = rotr(a + g, 43) + (rotr(b, 30) + c) * 9;
    const uint64_t v = ((a + g) ^ d) + f + 1;
    const uint64_t w = __builtin_bswap64((u + v) * mul) + h;
    const uint64_t x = rotr(e + f, 42) + c;
    const uint64_t y = (__builtin_bswap64((v + w) * mul) + g) * mul;
    const uint64_t z = e + f + c;
    a = __builtin_bswap64((x + z) * mul + y) + b;
    b = fold47((z + a) * mul + d + h) * mul;
    return b + x;
}

// WeakHashLen32WithSeeds on the 32 bytes at s (city.cc:317-337)
struct Pair {
    uint64_t first, second;
};
inline Pair weak_seeded32(const uint8_t* s, uint64_t a, uint64_t b) {
    const uint64_t w = le64(s), x = le64(s + 8), y = le64(s + 16), z = le64(s + 24);
    a += w;
    b = rotr(b + a + z, 21);
    const uint64_t c = a;
    a += x + y;
    b += rotr(a, 44);
    return Pair{a + z, b + c};
}

}  // namespace

// CityHash64 v1.1, city.cc:361-397
uint64_t cityhash64(const uint8_t* s, uint64_t n) {
    if (n <= 16) return len_upto16(s, n);
    if (n <= 32) return len_17to32(s, n);
    if (n <= 64) return len_33to64(s, n);
    uint64_t x = le64(s + n - 40);
    uint64_t y = le64(s + n - 16) + le64(s + n - 56);
    uint64_t z = murmur2x64(le64(s + n - 48) + n, le64(s + n - 24), kMul128);
    Pair v = weak_seeded32(s + n - 64, n, z);
    Pair w = weak_seeded32(s + n - 32, y + kK1, x);
    x = x * kK1 + le64(s);
    for (uint64_t blocks = (n - 1) >> 6; blocks; --blocks, s += 64) {
        x = rotr(x + y + v.first + le64(s + 8), 37) * kK1;
        y = rotr(y + v.second + le64(s + 48), 42) * kK1;
        x ^= w.second;
        y += v.first + le64(s + 40);
        z = rotr(z + w.first, 33) * kK1;
        v = weak_seeded32(s, v.second * kK1, x + w.first);
        w = weak_seeded32(s + 32, z + w.second, y + le64(s + 16));
        const uint64_t t = z;
        z = x;
        x = t;
    }
    return murmur2x64(murmur2x64(v.first, w.first, kMul128) + fold47(y) * kK1 + z,
                      murmur2x64(v.second, w.second, kMul128) + x, kMul128);
}

// ordered_encoding.cc:43-49: (u64)x + (x >= 0 ? 2^63 : INT64_MIN) == x ^ 2^63
uint64_t ordered_int64(uint64_t bits) { return bits ^ 0x8000000000000000ULL; }

// ordered_encoding.cc:114-161, tested on the bit pattern in the reference's
// order: inf, NaN, zero (either sign -> the same code), then finite values
// (subnormals keep their fraction).
uint64_t ordered_double(uint64_t bits) {
    const uint64_t exp = (bits >> 52) & 0x7ff, frac = bits & 0x000fffffffffffffULL;
    if (exp == 0x7ff) return frac ? 0xfff0000000000003ULL : (bits >> 63) ? 0ULL : 0xfff0000000000002ULL;
    if ((bits << 1) == 0) return 0x8000000000000001ULL;
    if (bits >> 63) return (~bits & 0x7fffffffffffffffULL) + 1;
    return (bits | 0x8000000000000000ULL) + 2;
}

// datatype_timestamp.cc:138-219; g = 0..5 for second..month.  The digit
// visiting order TABLE_* (:131-136) is g, g-1, .., 0, then g+1 .. 6.
uint64_t timestamp_hash(unsigned g, uint64_t t) {
    static const uint64_t kIntervals[6] = {60, 60, 24, 7, 4, 12};  // :117-129
    uint64_t x = (uint64_t)((double)t / 1000000.);                 // :198 (u64 -> f64, IEEE divide)
    uint64_t digit[7];
    for (int i = 0; i < 6; ++i) {
        digit[i] = x % kIntervals[i];
        x /= kIntervals[i];
    }
    digit[6] = x;
    uint64_t y = ~0ULL, h = 0;
    for (unsigned i = 0; i < 6; ++i) {
        const unsigned k = i <= g ? g - i : i;
        y /= kIntervals[k];
        h += digit[k] * y;
    }
    return h + digit[6];
}

// hash(hyperdatatype, slice), hash.cc:34-46, on a dispatch code (type_code)
hdx_status hash_code(int code, const uint8_t* p, uint64_t n, uint64_t* out) {
    switch (code) {
        case CODE_STRING:
            *out = cityhash64(p, n);
            return HDX_OK;
        case CODE_ZERO:  // hashable() == false (datatype_info.cc:169-180)
            *out = 0;
            return HDX_OK;
        default:
            break;
    }
    // int64 / float / timestamp: 8 bytes LE, empty = 0 (datatype_int64.cc:46-59,
    // datatype_float.cc:44-57, datatype_timestamp.cc:43-56); other sizes assert
    if (n != 0 && n != 8) return HDX_E_BADSIZE;
    const uint64_t bits = n ? le64(p) : 0;
    if (code == CODE_INT64) *out = ordered_int64(bits);
    else if (code == CODE_FLOAT) *out = ordered_double(bits);
    else *out = timestamp_hash((unsigned)(code - CODE_TS_SECOND), bits);
    return HDX_OK;
}

}  // namespace cpu
}  // namespace hdx

using namespace hdx;

HDX_EXPORT hdx_status hdx_hash_value(uint32_t type, const uint8_t* data, size_t len, uint64_t* out) {
    const int code = type_code(type);
    if (code < 0) return fail(HDX_E_BADTYPE, "unknown hyperdatatype %u", type);
    if (!out || (!data && len)) return fail(HDX_E_INVALID, "NULL pointer");
    const hdx_status st = cpu::hash_code(code, data, len, out);
    if (st != HDX_OK) return fail(st, "hyperdatatype %u: numeric value of %zu bytes", type, len);
    return HDX_OK;
}

HDX_EXPORT hdx_status hdx_hash_key(const uint32_t* types, uint32_t attrs_sz, const uint8_t* key,
                                   size_t key_len, uint64_t* h) {
    if (!types || attrs_sz == 0) return fail(HDX_E_INVALID, "empty schema");
    return hdx_hash_value(types[0], key, key_len, h);
}

HDX_EXPORT hdx_status hdx_hash_object(const uint32_t* types, uint32_t attrs_sz, const uint8_t* key,
                                      size_t key_len, const uint8_t* const* values, const size_t* value_lens,
                                      uint64_t* hs) {
    if (!types) return fail(HDX_E_INVALID, "types is NULL");
    if (attrs_sz == 0 || attrs_sz > HDX_MAX_ATTRS)
        return fail(HDX_E_INVALID, "attrs_sz=%u outside [1, %d]", attrs_sz, HDX_MAX_ATTRS);
    if (!hs || (!key && key_len) || (attrs_sz > 1 && (!values || !value_lens)))
        return fail(HDX_E_INVALID, "NULL pointer");
    // the reference asserts on the first bad attribute (hash.cc:38, :233/:204);
    // here nothing is written unless the whole object hashes
    for (uint32_t j = 0; j < attrs_sz; ++j) {
        const int code = type_code(types[j]);
        if (code < 0) return fail(HDX_E_BADTYPE, "attribute %u: unknown hyperdatatype %u", j, types[j]);
        const size_t n = j ? value_lens[j - 1] : key_len;
        if (code >= (int)CODE_INT64 && n != 0 && n != 8) {
            if (j) return fail(HDX_E_BADSIZE, "attribute %u: numeric value of %zu bytes", j, n);
            return fail(HDX_E_BADSIZE, "key: numeric value of %zu bytes", n);
        }
        if (j > 0 && !values[j - 1] && n) return fail(HDX_E_INVALID, "value %u is NULL", j - 1);
    }
    (void)cpu::hash_code(type_code(types[0]), key, key_len, &hs[0]);
    for (uint32_t j = 1; j < attrs_sz; ++j)
        (void)cpu::hash_code(type_code(types[j]), values[j - 1], value_lens[j - 1], &hs[j]);
    return HDX_OK;
}

// ---- one object's secondary-index entry (include/hdxhash.h) ----------------

namespace {

// enc(type, value) written at out (ENC_*, hdx_host_common.h)
uint8_t* entry_encode(uint32_t enc, const uint8_t* p, size_t len, uint8_t* out) {
    if (enc == ENC_STRING) {
        if (len) memcpy(out, p, len);
        return out + len;
    }
    const uint64_t bits = len ? cpu::le64(p) : 0;
    const uint64_t be = __builtin_bswap64(enc == ENC_INT64 ? cpu::ordered_int64(bits) : cpu::ordered_double(bits));
    memcpy(out, &be, 8);
    if (enc == ENC_INT64) return out + 8;
    memcpy(out + 8, &bits, 8);  // packdoublele(number): 0.0 when empty
    return out + 16;
}

}  // namespace

// index_primitive::index_entry(ri, ii, key_ie, key, value, ..), daemon/index_primitive.cc:291-329,
// with the caller's prefix standing for 'i' ++ varint(ri) ++ varint(ii)
HDX_EXPORT hdx_status hdx_index_entry(const hdx_index_spec* spec, uint32_t key_type, const uint8_t* key,
                                      size_t key_len, uint32_t attr_type, const uint8_t* value, size_t value_len,
                                      uint8_t* out, size_t out_cap, size_t* out_len) {
    if (out_len) *out_len = 0;
    if (!spec || !out_len || (!key && key_len) || (!value && value_len) || (!out && out_cap))
        return fail(HDX_E_INVALID, "NULL pointer");
    if (spec->attr == 0) return fail(HDX_E_INVALID, "an index names attribute 0 (the key)");
    if (spec->prefix_len == 0 || spec->prefix_len > HDX_INDEX_PREFIX_MAX)
        return fail(HDX_E_INVALID, "prefix_len %u outside [1, %d]", spec->prefix_len, HDX_INDEX_PREFIX_MAX);
    const uint32_t kenc = entry_encoder(key_type), venc = entry_encoder(attr_type);
    if (!kenc) return fail(HDX_E_BADTYPE, "key: hyperdatatype %u has no primitive index encoding", key_type);
    if (!venc) return fail(HDX_E_BADTYPE, "hyperdatatype %u has no primitive index encoding", attr_type);
    // encoded_size() of a numeric does not look at the value (index_int64.cc, index_float.cc): the
    // entry's size is known, and reported, even where encode() would assert
    const size_t key_sz = entry_encoded_size(kenc, key_len), val_sz = entry_encoded_size(venc, value_len);
    const bool variable = kenc == ENC_STRING && venc == ENC_STRING;  // !encoding_fixed() for both (:302)
    const size_t sz = spec->prefix_len + val_sz + key_sz + (variable ? 4 : 0);
    *out_len = sz;
    if (kenc != ENC_STRING && key_len != 0 && key_len != 8)
        return fail(HDX_E_BADSIZE, "key: numeric value of %zu bytes", key_len);
    if (venc != ENC_STRING && value_len != 0 && value_len != 8)
        return fail(HDX_E_BADSIZE, "numeric value of %zu bytes", value_len);
    if (out_cap < sz) return fail(HDX_E_NOMEM, "entry of %zu bytes, room for %zu", sz, out_cap);
    memcpy(out, spec->prefix, spec->prefix_len);
    uint8_t* p = entry_encode(venc, value, value_len, out + spec->prefix_len);
    p = entry_encode(kenc, key, key_len, p);
    if (variable) {
        const uint32_t be = __builtin_bswap32((uint32_t)key_sz);  // pack32be(key_sz), :322-325
        memcpy(p, &be, 4);
    }
    return HDX_OK;
}

// ---- one object against a search's attribute checks (include/hdxhash.h) ----

namespace {

// passes_attribute_check (common/attribute_check.cc:141-199) past what
// compile_checks decided: validate(v), then the comparison.  k: the check's
// own bytes (a STRING comparison reads them in place).
bool check_passes(const CheckOp& o, const uint8_t* k, const uint8_t* v, size_t len) {
    if (o.op == OP_NEVER || o.op > OP_LEN_GE) return false;  // OP_REGEX has its own path (object_first_fail)
    if (o.op >= OP_LEN_EQ) {  // :178-199, T == STRING: length(v) = its size
        const int64_t L = (int64_t)len, tmp = (int64_t)o.imm;
        return o.op == OP_LEN_EQ ? L == tmp : o.op == OP_LEN_LE ? L <= tmp : L >= tmp;
    }
    int cmp;
    if (o.family == FAM_STRING) {  // datatype_string.cc:263-285; memcmp compares unsigned bytes
        const size_t m = o.klen < len ? o.klen : len;
        cmp = m ? memcmp(k, v, m) : 0;
        if (cmp == 0) cmp = o.klen < len ? -1 : o.klen > len ? 1 : 0;
    } else {
        if (len != 0 && len != 8) return false;  // :141 validate(v): fails every check on it
        const uint64_t vb = len ? cpu::le64(v) : 0;  // an empty value is 0 / 0.0
        if (o.family == FAM_INT64) {  // datatype_int64.cc, datatype_timestamp.cc:268-285
            const int64_t a = (int64_t)o.imm, b = (int64_t)vb;
            cmp = a < b ? -1 : a > b ? 1 : 0;
        } else {  // datatype_float.cc:256-273: a NaN on either side gives 0
            double a, b;
            memcpy(&a, &o.imm, 8);
            memcpy(&b, &vb, 8);
            cmp = a < b ? -1 : a > b ? 1 : 0;
        }
    }
    return check_relation(o.op, cmp);
}

// passes_attribute_checks (common/attribute_check.cc:209-237) over compiled ops, for both per-object
// forms: the pointer checks, then the ops in order up to the first false one.  progs / table: the
// compiled form's regex programs and byte classes (op k's at ops[k].koff), NULL for the one-shot form,
// whose compile step makes no OP_REGEX.
hdx_status object_first_fail(const CheckOp* ops, const hdx_attribute_check* checks, uint32_t c, uint32_t attrs_sz,
                             const RegexProg* progs, const uint64_t (*table)[256], const uint8_t* key,
                             size_t key_len, const uint8_t* const* values, const size_t* value_lens,
                             uint32_t* first_fail) {
    if (!first_fail || (!key && key_len) || (attrs_sz > 1 && (!values || !value_lens)))
        return fail(HDX_E_INVALID, "NULL pointer");
    for (uint32_t i = 0; i < c; ++i)
        if (ops[i].op != OP_NEVER && ops[i].attr && !values[ops[i].attr - 1] && value_lens[ops[i].attr - 1])
            return fail(HDX_E_INVALID, "value %u is NULL", ops[i].attr - 1);
    uint32_t i = 0;
    for (; i < c; ++i) {
        const CheckOp& o = ops[i];
        const bool on_key = o.attr == 0;
        const uint8_t* v = on_key ? key : values[o.attr - 1];
        const size_t len = on_key ? key_len : value_lens[o.attr - 1];
        if (!(o.op == OP_REGEX && progs ? regex_run_host(progs[o.koff], table[o.koff], v, len)
                                        : check_passes(o, checks[i].value, v, len)))
            break;
    }
    *first_fail = i;
    return HDX_OK;
}

}  // namespace

// passes_attribute_checks, common/attribute_check.cc:209-237
HDX_EXPORT hdx_status hdx_passes_checks(const uint32_t* types, uint32_t attrs_sz, const uint8_t* key,
                                        size_t key_len, const uint8_t* const* values, const size_t* value_lens,
                                        const hdx_attribute_check* checks, uint32_t c, uint32_t* first_fail) {
    CheckOp ops[HDX_MAX_CHECKS];
    const hdx_status st = compile_checks(types, attrs_sz, checks, c, UINT64_MAX, ops);
    if (st != HDX_OK) return st;
    return object_first_fail(ops, checks, c, attrs_sz, nullptr, nullptr, key, key_len, values, value_lens, first_fail);
}

// ---- a list of checks compiled once per search (include/hdxhash.h) ---------

HDX_EXPORT hdx_status hdx_regex_match(const uint8_t* regex, size_t regex_len, const uint8_t* text, size_t text_len,
                                      int* matched) {
    if (!matched || (!regex && regex_len) || (!text && text_len)) return fail(HDX_E_INVALID, "NULL pointer");
    RegexProg g;
    if (!regex_parse(regex, regex_len, &g))
        return fail(HDX_E_INVALID, "a pattern of more than %d items", HDX_REGEX_ITEMS_MAX);
    *matched = regex_run_host(g, nullptr, text, text_len) ? 1 : 0;
    return HDX_OK;
}

HDX_EXPORT hdx_status hdx_checks_compile(const uint32_t* types, uint32_t attrs_sz, const hdx_attribute_check* checks,
                                         uint32_t c, hdx_checks* out) {
    CheckOp ops[HDX_MAX_CHECKS];
    RegexProg progs[HDX_MAX_REGEX_CHECKS];
    uint32_t nrx = 0;
    const hdx_status st = compile_checks(types, attrs_sz, checks, c, HDX_CHECK_BYTES_MAX, ops, progs, &nrx);
    if (st != HDX_OK) return st;
    if (!out) return fail(HDX_E_INVALID, "out is NULL");
    size_t bytes = 0;
    for (uint32_t i = 0; i < c; ++i) bytes += checks[i].value_len;
    const size_t types_at = sizeof(hdx_checks_s), bytes_at = types_at + (size_t)attrs_sz * 4;
    void* block = ::operator new(bytes_at + bytes, std::nothrow);
    if (!block) return fail(HDX_E_NOMEM, "a compiled list of %zu bytes", bytes_at + bytes);
    hdx_checks_s* h = new (block) hdx_checks_s{};
    uint8_t* base = static_cast<uint8_t*>(block);
    memcpy(base + types_at, types, (size_t)attrs_sz * 4);
    h->types = reinterpret_cast<const uint32_t*>(base + types_at);
    h->attrs_sz = attrs_sz;
    h->c = c;
    h->nrx = nrx;
    uint8_t* at = base + bytes_at;
    for (uint32_t i = 0; i < c; ++i) {
        h->checks[i] = checks[i];
        h->ops[i] = ops[i];
        if (checks[i].value_len) memcpy(at, checks[i].value, checks[i].value_len);
        h->checks[i].value = at;
        at += checks[i].value_len;
    }
    for (uint32_t r = 0; r < nrx; ++r) {
        h->progs[r] = progs[r];
        for (uint32_t b = 0; b < 256; ++b) h->table[r][b] = regex_class(progs[r], b);
    }
    *out = h;
    return HDX_OK;
}

HDX_EXPORT void hdx_checks_free(hdx_checks h) { ::operator delete(h); }

HDX_EXPORT hdx_status hdx_checks_passes(hdx_checks h, const uint8_t* key, size_t key_len,
                                        const uint8_t* const* values, const size_t* value_lens,
                                        uint32_t* first_fail) {
    if (!h) return fail(HDX_E_INVALID, "the compiled list is NULL");
    return object_first_fail(h->ops, h->checks, h->c, h->attrs_sz, h->progs, h->table, key, key_len, values,
                             value_lens, first_fail);
}

// ---- the top-limit matches by one attribute (include/hdxhash.h) ------------

namespace {

// datatype_{string,int64,float,timestamp}::compare(a, b) on validated operands
// (numerics of 0 or 8 bytes): datatype_string.cc:263-285, datatype_int64.cc,
// datatype_float.cc:256-273 (a NaN on either side gives 0).
int compare_values(int fam, const uint8_t* a, size_t al, const uint8_t* b, size_t bl) {
    if (fam == (int)FAM_STRING) {
        const size_t m = al < bl ? al : bl;
        const int c = m ? memcmp(a, b, m) : 0;
        return c ? (c < 0 ? -1 : 1) : al < bl ? -1 : al > bl ? 1 : 0;
    }
    const uint64_t x = al ? cpu::le64(a) : 0, y = bl ? cpu::le64(b) : 0;  // an empty value is 0 / 0.0
    if (fam == (int)FAM_INT64) return (int64_t)x < (int64_t)y ? -1 : (int64_t)x > (int64_t)y ? 1 : 0;
    double p, q;
    memcpy(&p, &x, 8);
    memcpy(&q, &y, 8);
    return p < q ? -1 : p > q ? 1 : 0;
}

// A sort value: the library's order is compare's, with its own rule for NaN
// (every NaN above +inf, all NaNs tie).
struct SortValue {
    const uint8_t* p;
    uint32_t len;
    uint64_t idx;
};
bool is_nan(const SortValue& v) {
    return v.len == 8 && (cpu::le64(v.p) & 0x7fffffffffffffffULL) > 0x7ff0000000000000ULL;
}
int sort_compare(int fam, const SortValue& a, const SortValue& b) {
    if (fam < 0) return 0;  // attr >= attrs_sz: every object ties (search_manager.cc:361)
    if (fam == (int)FAM_FLOAT) {
        const bool na = is_nan(a), nb = is_nan(b);
        if (na || nb) return na == nb ? 0 : na ? 1 : -1;
    }
    return compare_values(fam, a.p, a.len, b.p, b.len);
}

// a comes before b in the kept order: (value ascending, or descending with
// largest; then index ascending)
struct KeptOrder {
    int fam;
    bool largest;
    bool operator()(const SortValue& a, const SortValue& b) const {
        int c = sort_compare(fam, a, b);
        if (largest) c = -c;
        return c ? c < 0 : a.idx < b.idx;
    }
};

// decode_value under the sweep's contract (value_walk, hdx_value_walk.h): attribute j's bytes at
// v + pos[j - 1], len[j - 1] for the attributes named in want[0 .. w); false where the value is refused.
bool walk_value(const uint8_t* v, uint32_t vlen, uint32_t A, const uint32_t* want, uint32_t w, uint32_t* pos,
                uint32_t* len) {
    if (vlen < 10) return false;
    if ((((uint32_t)v[8] << 8) | v[9]) != ((A - 1) & 0xffffu) || A - 1 > 0xffffu) return false;
    uint32_t at = 10;
    for (uint32_t j = 1; j < A; ++j) {
        if (vlen - at < 4) return false;
        const uint32_t L = __builtin_bswap32(cpu::le32(v + at));
        at += 4;
        if (L > vlen - at) return false;
        for (uint32_t k = 0; k < w; ++k)
            if (want[k] == j) {
                pos[k] = at;
                len[k] = L;
            }
        at += L;
    }
    return true;
}

}  // namespace

HDX_EXPORT hdx_status hdx_compare(uint32_t type, const uint8_t* a, size_t a_len, const uint8_t* b, size_t b_len,
                                  int* cmp) {
    const int fam = check_family(type);
    if (fam < 0) return fail(HDX_E_BADTYPE, "hyperdatatype %u (only STRING, INT64, FLOAT, TIMESTAMP_*)", type);
    if (!cmp || (!a && a_len) || (!b && b_len)) return fail(HDX_E_INVALID, "NULL pointer");
    if (fam != (int)FAM_STRING && ((a_len != 0 && a_len != 8) || (b_len != 0 && b_len != 8)))
        return fail(HDX_E_BADSIZE, "numeric values of %zu and %zu bytes", a_len, b_len);
    *cmp = compare_values(fam, a, a_len, b, b_len);
    return HDX_OK;
}

HDX_EXPORT hdx_status hdx_sorted_search(const uint32_t* types, uint32_t attrs_sz, const uint8_t* keys,
                                        const uint64_t* key_off, const uint32_t* key_len, const uint8_t* vals,
                                        const uint64_t* val_off, const uint32_t* val_len, uint64_t n,
                                        const hdx_attribute_check* checks, uint32_t c, const hdx_sort_spec* sort,
                                        uint64_t limit, uint64_t* top, uint64_t* top_count, uint32_t* status) {
    const StoredObjects so{keys, key_off, key_len, vals, val_off, val_len};
    CheckOp ops[HDX_MAX_CHECKS];
    hdx_status st = compile_checks(types, attrs_sz, checks, c, UINT64_MAX, ops);
    if (st != HDX_OK) return st;
    int fam;
    if ((st = sort_args(types, attrs_sz, sort, &fam)) != HDX_OK) return st;
    if (!has_columns(so, SO_ALL) || !top || !top_count) return fail(HDX_E_INVALID, "NULL pointer");
    // the attributes the walk reports: the ops' and, last, the sort attribute
    uint32_t want[HDX_MAX_CHECKS + 1], pos[HDX_MAX_CHECKS + 1], len[HDX_MAX_CHECKS + 1];
    for (uint32_t k = 0; k < c; ++k) want[k] = ops[k].op != OP_NEVER ? ops[k].attr : 0;  // 0: never reported
    want[c] = fam >= 0 ? sort->attr : 0;
    // top[0 .. kept) is a heap with the worst of the kept on top; the values stand beside it
    const KeptOrder order{fam, sort->keep == HDX_KEEP_LARGEST};
    SortValue* heap = nullptr;
    const uint64_t cap = limit < n ? limit : n;
    if (cap) {
        heap = new (std::nothrow) SortValue[cap];
        if (!heap) return fail(HDX_E_NOMEM, "%llu kept values", (unsigned long long)cap);
    }
    uint64_t kept = 0;
    uint32_t bits = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const uint8_t* v = vals + val_off[i];
        memset(pos, 0, sizeof pos);
        memset(len, 0, sizeof len);
        if (!walk_value(v, val_len[i], attrs_sz, want, c + 1, pos, len)) {
            bits |= 1u << HDX_E_BADENC;
            continue;
        }
        const uint8_t* key = keys + key_off[i];
        uint32_t k = 0;
        for (; k < c; ++k) {
            const bool on_key = ops[k].attr == 0;
            if (!check_passes(ops[k], checks[k].value, on_key ? key : v + pos[k], on_key ? key_len[i] : len[k])) break;
        }
        if (k < c) continue;
        SortValue x{nullptr, 0, i};
        if (fam >= 0) {
            x.p = sort->attr == 0 ? key : v + pos[c];
            x.len = sort->attr == 0 ? key_len[i] : len[c];
            if (fam != (int)FAM_STRING && x.len != 0 && x.len != 8) {  // the reference's unpack asserts
                bits |= 1u << HDX_E_BADSIZE;
                continue;
            }
        }
        if (kept < cap) {
            heap[kept++] = x;
            std::push_heap(heap, heap + kept, order);
        } else if (cap && order(x, heap[0])) {
            std::pop_heap(heap, heap + kept, order);
            heap[kept - 1] = x;
            std::push_heap(heap, heap + kept, order);
        }
    }
    // the output: value ascending or descending, the index ascending among ties either way
    const bool desc = sort->descending != 0;
    std::sort(heap, heap + kept, [&](const SortValue& a, const SortValue& b) {
        int cmp = sort_compare(fam, a, b);
        if (desc) cmp = -cmp;
        return cmp ? cmp < 0 : a.idx < b.idx;
    });
    for (uint64_t k = 0; k < kept; ++k) top[k] = heap[k].idx;
    delete[] heap;
    *top_count = kept;
    if (status) *status |= bits;
    return HDX_OK;
}

// The objects behind a list of indices, packed (the host form of
// hdx_gather_objects_plan_device / _fill_device): the offsets first, since
// nothing may be written when they do not fit, then the bytes.
HDX_EXPORT hdx_status hdx_gather_objects(const uint8_t* keys, const uint64_t* key_off, const uint32_t* key_len,
                                         const uint8_t* vals, const uint64_t* val_off, const uint32_t* val_len,
                                         uint64_t n, const uint64_t* idx, uint64_t count, uint32_t what,
                                         uint64_t* rec_off, uint32_t* rec_key_len, uint8_t* out, uint64_t out_bytes,
                                         uint32_t* status) {
    const StoredObjects so{keys, key_off, key_len, vals, val_off, val_len};
    const hdx_status st = gather_objects_check(so, idx && rec_off && out, true, n, count, what);
    if (st != HDX_OK) return st;
    uint32_t bits = 0;
    uint64_t at = 0;
    for (uint64_t r = 0; r < count; ++r) {
        const uint64_t i = idx[r];
        uint32_t kl = 0;
        uint64_t size = 0;
        if (i < n) {
            if (what & HDX_GATHER_KEYS) kl = key_len[i];
            size = (uint64_t)kl + ((what & HDX_GATHER_VALUES) ? val_len[i] : 0u);
        } else {
            bits |= 1u << HDX_E_INVALID;
        }
        rec_off[r] = at;
        if (rec_key_len) rec_key_len[r] = kl;
        at += size;
    }
    rec_off[count] = at;
    if (at > out_bytes) {
        if (status) *status |= bits | (1u << HDX_E_NOMEM);
        return fail(HDX_E_NOMEM, "records of %llu bytes, room for %llu", (unsigned long long)at,
                    (unsigned long long)out_bytes);
    }
    for (uint64_t r = 0; r < count; ++r) {
        const uint64_t size = rec_off[r + 1] - rec_off[r];
        if (size == 0) continue;  // an index >= n among them
        const uint64_t i = idx[r];
        uint8_t* d = out + rec_off[r];
        const uint32_t kl = (what & HDX_GATHER_KEYS) ? key_len[i] : 0;
        if (kl) memcpy(d, keys + key_off[i], kl);
        if (size > kl) memcpy(d + kl, vals + val_off[i], size - kl);
    }
    if (status) *status |= bits;
    return HDX_OK;
}
