// hdx_host_common.h — declarations the host translation units share that need
// no HIP header (the CPU per-object path, hdx_cpu.cpp, includes only this).
#pragma once

#include <stdint.h>

#include "../../include/hdxhash.h"
#include "hdx_regex.h"

#define HDX_EXPORT extern "C" __attribute__((visibility("default")))

namespace hdx {

// Attribute classes the kernels and the CPU path dispatch on (the host maps
// hyperdatatype -> code, type_code).
enum : uint32_t {
    CODE_ZERO = 0,     // not hashable: document/list/set/map/macaroon -> 0
    CODE_STRING = 1,
    CODE_INT64 = 2,
    CODE_FLOAT = 3,
    CODE_TS_SECOND = 4,  // .. CODE_TS_MONTH = 9, in hyperdatatype order
    CODE_TS_MONTH = 9,
};

// hyperdatatype -> CODE_* (-1: the reference's datatype_info::lookup returns
// NULL); include/hyperdex.h:53-102, datatype_info.cc:72-141.  Inline: the
// per-object CPU entry points call it once per attribute.
inline int type_code(uint32_t t) {
    switch (t) {
        case 9217: return CODE_STRING;
        case 9218: return CODE_INT64;
        case 9219: return CODE_FLOAT;
        case 9473: case 9474: case 9475: case 9476: case 9477: case 9478:
            return CODE_TS_SECOND + (int)(t - 9473);
        // lookup() returns a datatype whose hashable() is false (hash.cc:40-43)
        case 9223:                                   // document
        case 9281: case 9282: case 9283:             // list string/int64/float
        case 9345: case 9346: case 9347:             // set string/int64/float
        case 9417: case 9418: case 9419:             // map string->*
        case 9425: case 9426: case 9427:             // map int64->*
        case 9433: case 9434: case 9435:             // map float->*
        case 9664:                                   // macaroon secret
            return CODE_ZERO;
        default:  // generic, *_GENERIC, *_KEYONLY, garbage, anything else: lookup() == NULL
            return -1;
    }
}
// The index encoder of a key or an indexed attribute in a secondary-index
// entry (daemon/index_info.cc:77-118), shared by the per-object CPU form
// (hdx_cpu.cpp) and the device entry points (hdx_capi_index.cpp,
// hdx_index_entries.hip): the bytes themselves (index_string.cc:62-79), the
// 8-byte ordered int64 (index_int64.cc:76-79; the timestamps delegate to it,
// index_timestamp.cc:79-82), the 16-byte float key (index_float.cc:69-90).
enum : uint8_t { ENC_NONE = 0, ENC_STRING = 1, ENC_INT64 = 2, ENC_FLOAT = 3 };
// ENC_NONE: unknown types and the container, document and macaroon types,
// whose indices write one entry per element or none.
inline uint8_t entry_encoder(uint32_t type) {
    const int c = type_code(type);
    if (c == (int)CODE_STRING) return ENC_STRING;
    if (c == (int)CODE_INT64) return ENC_INT64;
    if (c == (int)CODE_FLOAT) return ENC_FLOAT;
    if (c >= (int)CODE_TS_SECOND && c <= (int)CODE_TS_MONTH) return ENC_INT64;
    return ENC_NONE;
}
// Bytes of enc(type, value) for a value of len bytes.
inline uint64_t entry_encoded_size(uint32_t enc, uint64_t len) {
    return enc == ENC_STRING ? len : enc == ENC_INT64 ? 8 : 16;
}

// Sets the calling thread's hdx_last_error() text and returns s.
hdx_status fail(hdx_status s, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

// n stored objects: object i's key is key_len[i] bytes at keys + key_off[i], its value val_len[i]
// bytes at vals + val_off[i]; keys == vals for records [key][value] in one store.  Every
// extern "C" entry point after the hash builds one from its parameters; the host layers below it
// pass the view on, and the kernel argument structs that read stored objects derive from it
// (hdx_internal.h), so a new stored-object call is one construction, one has_columns with its row
// of the table, and one assignment into its arguments.  The columns each stage reads (the others
// may be NULL):
//   sweep, checks, sorted search   all
//   entries plan                   key_len, vals, val_off, val_len
//   entries fill                   keys, key_off, key_len, vals, val_off
//   gather plan                    key_len, val_len
//   gather fill                    key_len, val_len; keys, key_off with KEYS; vals, val_off with VALUES
struct StoredObjects {
    const uint8_t* keys;  const uint64_t* key_off;  const uint32_t* key_len;
    const uint8_t* vals;  const uint64_t* val_off;  const uint32_t* val_len;
};
enum : uint32_t {
    SO_KEYS = 1, SO_KEY_OFF = 2, SO_KEY_LEN = 4, SO_VALS = 8, SO_VAL_OFF = 16, SO_VAL_LEN = 32,
    SO_ALL = 63,
};
// True when none of the columns in mask is NULL.
inline bool has_columns(const StoredObjects& so, uint32_t mask) {
    const uint32_t have = (so.keys ? SO_KEYS : 0u) | (so.key_off ? SO_KEY_OFF : 0u) | (so.key_len ? SO_KEY_LEN : 0u) |
                          (so.vals ? SO_VALS : 0u) | (so.val_off ? SO_VAL_OFF : 0u) | (so.val_len ? SO_VAL_LEN : 0u);
    return (mask & ~have) == 0;
}

// What hdx_gather_objects and its two device calls refuse before anything is
// read (include/hdxhash.h): `others` is the form's other pointers ANDed
// together; keys and key_off matter only with KEYS, vals and val_off only
// with VALUES (with_bytes: the forms that copy; the plan reads lengths only).
constexpr uint64_t kGatherMaxRecords = 1ull << 40;
inline hdx_status gather_objects_check(const StoredObjects& so, bool others, bool with_bytes, uint64_t n,
                                       uint64_t cap, uint32_t what) {
    if (what == 0 || (what & ~(HDX_GATHER_KEYS | HDX_GATHER_VALUES)))
        return fail(HDX_E_INVALID, "what=%u is not HDX_GATHER_KEYS, HDX_GATHER_VALUES or both", what);
    if (!has_columns(so, SO_KEY_LEN | SO_VAL_LEN) || !others) return fail(HDX_E_INVALID, "NULL pointer");
    if (with_bytes && (what & HDX_GATHER_KEYS) && !has_columns(so, SO_KEYS | SO_KEY_OFF))
        return fail(HDX_E_INVALID, "HDX_GATHER_KEYS without keys or key_off");
    if (with_bytes && (what & HDX_GATHER_VALUES) && !has_columns(so, SO_VALS | SO_VAL_OFF))
        return fail(HDX_E_INVALID, "HDX_GATHER_VALUES without vals or val_off");
    if (n > kGatherMaxRecords || cap > kGatherMaxRecords)
        return fail(HDX_E_INVALID, "n=%llu or cap=%llu above 2^40", (unsigned long long)n, (unsigned long long)cap);
    return HDX_OK;
}

// ---- a search's attribute checks (common/attribute_check.cc:123-237) --------
//
// One compiled form for the per-object CPU path (hdx_cpu.cpp) and the device
// launcher (hdx_capi_index.cpp, hdx_checks.hip): op k stands for checks[k].
// Everything of passes_attribute_check that does not depend on the object is
// decided by compile_checks; what is left per object is the attribute's own
// validate() (:141) and one comparison.
// OP_REGEX (regex_match(k, v), :174-177) comes only out of the compiled form (hdx_checks_compile).
enum : uint8_t { OP_NEVER = 0, OP_EQ, OP_LT, OP_LE, OP_GE, OP_GT, OP_LEN_EQ, OP_LEN_LE, OP_LEN_GE, OP_REGEX };
enum : uint8_t { FAM_STRING = 0, FAM_INT64 = 1, FAM_FLOAT = 2 };
struct CheckOp {
    uint16_t attr;   // 0: the key; 0 also with OP_NEVER, which reads nothing
    uint8_t op, family;
    uint32_t klen;   // FAM_STRING comparisons: the constant's length
    uint32_t koff;   // ... and its 8-byte-aligned offset in the packed constants (pack_check_constants);
                     // OP_REGEX: the index of its program
    uint32_t pad_;
    uint64_t imm;    // numeric comparisons: k's little-endian bits (empty: 0); OP_LEN_*: tmp
};
// Room for the packed STRING constants: each starts 8-byte aligned and is zero-padded to 8.
constexpr uint32_t kCheckConstBytes = HDX_CHECK_BYTES_MAX + 8 * HDX_MAX_CHECKS;

// FAM_* of an attribute type the checks are built for, -1 for every other
// type (document_check, container length / contains: out of scope).
inline int check_family(uint32_t type) {
    const int c = type_code(type);
    if (c == (int)CODE_STRING) return FAM_STRING;
    if (c == (int)CODE_INT64) return FAM_INT64;
    if (c == (int)CODE_FLOAT) return FAM_FLOAT;
    if (c >= (int)CODE_TS_SECOND && c <= (int)CODE_TS_MONTH) return FAM_INT64;  // datatype_timestamp.cc:268-285
    return -1;
}

// The argument checks of both forms, then ops[0..c).  max_bytes: the cap on
// the sum of the checks' value_len (the device form's HDX_CHECK_BYTES_MAX: its
// constants travel in the kernel arguments; the CPU form reads them in place
// and has none).  progs: NULL for the one-shot entry points, which refuse REGEX
// on a STRING attribute; the compiled form's HDX_MAX_REGEX_CHECKS programs,
// *nprogs of them used, op k's at ops[k].koff.
inline hdx_status compile_checks(const uint32_t* types, uint32_t attrs_sz, const hdx_attribute_check* checks,
                                 uint32_t c, uint64_t max_bytes, CheckOp* ops, RegexProg* progs = nullptr,
                                 uint32_t* nprogs = nullptr) {
    if (!types) return fail(HDX_E_INVALID, "types is NULL");
    if (attrs_sz == 0 || attrs_sz > HDX_MAX_ATTRS)
        return fail(HDX_E_INVALID, "attrs_sz=%u outside [1, %d]", attrs_sz, HDX_MAX_ATTRS);
    if (c > HDX_MAX_CHECKS) return fail(HDX_E_INVALID, "c=%u above %d", c, HDX_MAX_CHECKS);
    if (c && !checks) return fail(HDX_E_INVALID, "checks is NULL");
    uint64_t bytes = 0;
    for (uint32_t i = 0; i < c; ++i) {
        if (!checks[i].value && checks[i].value_len) return fail(HDX_E_INVALID, "check %u: value is NULL", i);
        if (checks[i].value_len > max_bytes - bytes)
            return fail(HDX_E_INVALID, "the checks' values exceed %llu bytes", (unsigned long long)max_bytes);
        bytes += checks[i].value_len;
    }
    uint32_t koff = 0;
    if (nprogs) *nprogs = 0;
    for (uint32_t i = 0; i < c; ++i) {
        const hdx_attribute_check& ck = checks[i];
        CheckOp& o = ops[i];
        o = CheckOp{};
        if (ck.attr >= attrs_sz) continue;  // :217-220: fails at i
        const uint32_t T = types[ck.attr], D = ck.datatype;
        const int fam = check_family(T);
        if (fam < 0)
            return fail(HDX_E_BADTYPE, "check %u: attribute %u of hyperdatatype %u (only STRING, INT64, FLOAT, TIMESTAMP_*)",
                        i, ck.attr, T);
        if (ck.predicate == 9733 && T == 9217 && D == 9217) {  // :174-177, the one case that runs regex_match
            if (!progs)
                return fail(HDX_E_BADTYPE, "check %u: REGEX on a STRING attribute needs the compiled form", i);
            if (*nprogs == HDX_MAX_REGEX_CHECKS)
                return fail(HDX_E_INVALID, "more than %d REGEX checks on STRING attributes", HDX_MAX_REGEX_CHECKS);
            if (!regex_parse(ck.value, ck.value_len, &progs[*nprogs]))
                return fail(HDX_E_INVALID, "check %u: a pattern of more than %d items", i, HDX_REGEX_ITEMS_MAX);
            o.attr = (uint16_t)ck.attr;
            o.op = OP_REGEX;
            o.family = FAM_STRING;
            o.klen = (uint32_t)ck.value_len;
            o.koff = (*nprogs)++;
            continue;
        }
        // :128-134 lookup(D) == NULL -> false.  A container, document or macaroon D is false too,
        // whichever way its validate(k) goes: T is primitive here, so T == D (:155-173) fails, the
        // LENGTH forms want D == INT64 (:182-199), REGEX wants D == STRING (:175), and a primitive
        // has_contains() is false (:201).  So nothing of those types is implemented.
        const int dfam = check_family(D);
        if (dfam < 0) continue;
        // :142 validate(k) under D
        if (dfam != (int)FAM_STRING && ck.value_len != 0 && ck.value_len != 8) continue;
        uint8_t op = OP_NEVER;
        switch (ck.predicate) {
            case 9729: op = OP_EQ; break;
            case 9738: op = OP_LT; break;
            case 9730: op = OP_LE; break;
            case 9731: op = OP_GE; break;
            case 9739: op = OP_GT; break;
            case 9734: op = OP_LEN_EQ; break;
            case 9732:  // CONTAINS_LESS_THAN shares LENGTH_LESS_EQUAL's code (:185-192)
            case 9735: op = OP_LEN_LE; break;
            case 9736: op = OP_LEN_GE; break;
            default: break;  // FAIL, CONTAINS (no primitive has_contains()), REGEX left over, unknown values
        }
        if (op == OP_NEVER) continue;
        if (op >= OP_LEN_EQ) {
            // :179-184: D == INT64 exactly, has_length() (of these types only STRING)
            if (D != 9218 || fam != (int)FAM_STRING) continue;
            uint64_t tmp = 0;  // the first min(len(k), 8) bytes, little-endian, zero-padded
            for (uint64_t b = 0; b < ck.value_len && b < 8; ++b) tmp |= (uint64_t)ck.value[b] << (8 * b);
            o.imm = tmp;
        } else {
            if (T != D) continue;  // an exact type match: two timestamp granularities differ
            if (fam == (int)FAM_STRING) {
                o.klen = (uint32_t)ck.value_len;
                o.koff = koff;
                koff += ((uint32_t)ck.value_len + 7u) & ~7u;
            } else {
                for (uint64_t b = 0; b < ck.value_len; ++b) o.imm |= (uint64_t)ck.value[b] << (8 * b);
            }
        }
        o.attr = (uint16_t)ck.attr;
        o.op = op;
        o.family = (uint8_t)fam;
    }
    return HDX_OK;
}

// What both forms of the sorted search (hdx_sorted_search, _device) refuse in their sort
// argument before anything runs; *fam: the sort attribute's FAM_*, -1 where sort->attr >=
// attrs_sz and every object ties (search_manager.cc:361).  After compile_checks: types is set.
inline hdx_status sort_args(const uint32_t* types, uint32_t attrs_sz, const hdx_sort_spec* sort, int* fam) {
    if (!sort) return fail(HDX_E_INVALID, "sort is NULL");
    if (sort->keep > 1 || sort->descending > 1 || sort->reserved != 0)
        return fail(HDX_E_INVALID, "sort: keep=%u descending=%u reserved=%u", sort->keep, sort->descending,
                    sort->reserved);
    *fam = -1;
    if (sort->attr < attrs_sz && (*fam = check_family(types[sort->attr])) < 0)
        return fail(HDX_E_BADTYPE, "sort attribute %u of hyperdatatype %u (only STRING, INT64, FLOAT, TIMESTAMP_*)",
                    sort->attr, types[sort->attr]);
    return HDX_OK;
}

// The relation a comparing op asks of cmp = compare(k, v), the check's value on the left (:154-173).
// Host and device: the kernel applies the same table.
#ifdef __HIPCC__
__host__ __device__
#endif
inline bool check_relation(uint8_t op, int cmp) {
    switch (op) {
        case OP_EQ: return cmp == 0;  // k == v bytewise implies compare == 0 in every family
        case OP_LT: return cmp > 0;
        case OP_LE: return cmp >= 0;
        case OP_GE: return cmp <= 0;
        default: return cmp < 0;      // OP_GT
    }
}

// regex_match(k, v) on the host with k's program; table: its byte classes
// (regex_class of every byte), or NULL to work them out per byte of v.
inline bool regex_run_host(const RegexProg& g, const uint64_t* table, const uint8_t* v, uint64_t len) {
    uint64_t s = regex_start(g);
    if (regex_accepted(g, s)) return true;
    for (uint64_t i = 0; i < len; ++i) {
        s = regex_step(g, s, table ? table[v[i]] : regex_class(g, v[i]));
        if (regex_accepted(g, s)) return true;
        if (!s) return false;  // anchored, and every position has died
    }
    return regex_at_end(g, s);
}

}  // namespace hdx

// A compiled list of checks (hdx_checks_compile, hdx_cpu.cpp): one heap block,
// host memory only, never written after compile — any thread, any device.
struct hdx_checks_s {
    uint32_t attrs_sz, c, nrx, pad_;
    const uint32_t* types;                        // [attrs_sz], behind the struct
    hdx_attribute_check checks[HDX_MAX_CHECKS];   // value: into the block
    hdx::CheckOp ops[HDX_MAX_CHECKS];
    hdx::RegexProg progs[HDX_MAX_REGEX_CHECKS];   // op k's: progs[ops[k].koff]
    uint64_t table[HDX_MAX_REGEX_CHECKS][256];    // the host form's byte classes
};
