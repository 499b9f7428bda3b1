// ref_hash_glue.cc — TEST INFRASTRUCTURE ONLY.
//
// Links the reference's own hash chain — common/hash.cc,
// common/datatype_{string,int64,float,timestamp}.cc, common/ordered_encoding.cc,
// common/regex_match.cc and cityhash/city.cc, compiled unmodified from the
// reference tree by oracle/Makefile — into oracle/_ref/libref_hash.so and
// exports hyperdex::hash under C linkage (the reference's namespace has hidden
// visibility, namespace.h).
//
// This file stands in for common/datatype_info.cc, common/schema.cc and
// common/attribute.cc, which pull in the container, document and macaroon
// types and their libraries.  It holds no hashing logic: the base class's
// do-nothing defaults, constructors, and a lookup() over the nine hashable
// types.  lookup() returns NULL for every other type, on which the reference
// asserts, and the numeric types assert on a value that is neither empty nor 8
// bytes: the exported functions refuse both with an error code and never call
// into the reference with them.
#include <stdint.h>
#include <stdlib.h>

#include <vector>

#include "common/attribute.h"
#include "common/datatype_float.h"
#include "common/datatype_info.h"
#include "common/datatype_int64.h"
#include "common/datatype_string.h"
#include "common/datatype_timestamp.h"
#include "common/hash.h"
#include "common/schema.h"

using hyperdex::attribute;
using hyperdex::datatype_info;
using hyperdex::schema;

// ---- stand-in for common/datatype_info.cc ------------------------------------

namespace {
hyperdex::datatype_string d_string;
hyperdex::datatype_int64 d_int64;
hyperdex::datatype_float d_float;
hyperdex::datatype_timestamp d_ts_second(HYPERDATATYPE_TIMESTAMP_SECOND);
hyperdex::datatype_timestamp d_ts_minute(HYPERDATATYPE_TIMESTAMP_MINUTE);
hyperdex::datatype_timestamp d_ts_hour(HYPERDATATYPE_TIMESTAMP_HOUR);
hyperdex::datatype_timestamp d_ts_day(HYPERDATATYPE_TIMESTAMP_DAY);
hyperdex::datatype_timestamp d_ts_week(HYPERDATATYPE_TIMESTAMP_WEEK);
hyperdex::datatype_timestamp d_ts_month(HYPERDATATYPE_TIMESTAMP_MONTH);
}  // namespace

datatype_info* datatype_info::lookup(hyperdatatype t) {
    switch (static_cast<uint32_t>(t)) {
        case HYPERDATATYPE_STRING: return &d_string;
        case HYPERDATATYPE_INT64: return &d_int64;
        case HYPERDATATYPE_FLOAT: return &d_float;
        case HYPERDATATYPE_TIMESTAMP_SECOND: return &d_ts_second;
        case HYPERDATATYPE_TIMESTAMP_MINUTE: return &d_ts_minute;
        case HYPERDATATYPE_TIMESTAMP_HOUR: return &d_ts_hour;
        case HYPERDATATYPE_TIMESTAMP_DAY: return &d_ts_day;
        case HYPERDATATYPE_TIMESTAMP_WEEK: return &d_ts_week;
        case HYPERDATATYPE_TIMESTAMP_MONTH: return &d_ts_month;
        default: return NULL;
    }
}

datatype_info::datatype_info() {}
datatype_info::~datatype_info() throw() {}

// Defaults of the optional capabilities: "not supported".  The nine types
// above override everything the hash path reaches, so none of these runs in
// a test; the ones that have no sensible answer abort.
bool datatype_info::client_to_server(const e::slice&, e::arena*, e::slice*) const { abort(); }
bool datatype_info::server_to_client(const e::slice&, e::arena*, e::slice*) const { abort(); }
bool datatype_info::hashable() const { return false; }
uint64_t datatype_info::hash(const e::slice&) const { abort(); }
bool datatype_info::indexable() const { return false; }
bool datatype_info::has_length() const { return false; }
uint64_t datatype_info::length(const e::slice&) const { abort(); }
bool datatype_info::has_regex() const { return false; }
bool datatype_info::regex(const e::slice&, const e::slice&) const { abort(); }
bool datatype_info::has_contains() const { return false; }
hyperdatatype datatype_info::contains_datatype() const { abort(); }
bool datatype_info::contains(const e::slice&, const e::slice&) const { abort(); }
bool datatype_info::containable() const { return false; }
bool datatype_info::step(const uint8_t**, const uint8_t*, e::slice*) const { abort(); }
uint64_t datatype_info::write_sz(const e::slice&) const { abort(); }
uint8_t* datatype_info::write(const e::slice&, uint8_t*) const { abort(); }
bool datatype_info::comparable() const { return false; }
int datatype_info::compare(const e::slice&, const e::slice&) const { abort(); }
datatype_info::compares_less datatype_info::compare_less() const { abort(); }
bool datatype_info::document() const { return false; }
bool datatype_info::document_check(const hyperdex::attribute_check&, const e::slice&) const { abort(); }

// ---- stand-ins for common/attribute.cc and common/schema.cc (constructors only) --

attribute::attribute() : name(""), type(HYPERDATATYPE_GARBAGE) {}
schema::schema() : attrs_sz(0), attrs(NULL), authorization(false) {}

// ---- the exports ------------------------------------------------------------------

#define REF_EXPORT extern "C" __attribute__((visibility("default")))

enum { REF_OK = 0, REF_E_BADTYPE = 1, REF_E_BADSIZE = 2, REF_E_INVALID = 4 };

// 0 when hyperdex::hash(type, value of len bytes) can be called: one of the
// nine types, and for the numeric ones an empty or 8-byte value.
static int ref_refuses(uint32_t type, uint64_t len) {
    if (datatype_info::lookup(static_cast<hyperdatatype>(type)) == NULL) return REF_E_BADTYPE;
    if (type != HYPERDATATYPE_STRING && len != 0 && len != 8) return REF_E_BADSIZE;
    return REF_OK;
}

// hyperdex::hash(hyperdatatype, e::slice)
REF_EXPORT int ref_hash(uint32_t type, const uint8_t* ptr, size_t len, uint64_t* out) {
    const int e = ref_refuses(type, len);
    if (e != REF_OK) return e;
    *out = hyperdex::hash(static_cast<hyperdatatype>(type), e::slice(ptr, len));
    return REF_OK;
}

// out[i] = hyperdex::hash(type, blob[off[i] .. off[i] + len[i])) for i < n.
// Every value is checked before the first one is hashed.
REF_EXPORT int ref_hash_batch(uint32_t type, const uint8_t* blob, const uint64_t* off, const uint32_t* len,
                              uint64_t n, uint64_t* out) {
    for (uint64_t i = 0; i < n; ++i) {
        const int e = ref_refuses(type, len[i]);
        if (e != REF_OK) return e;
    }
    for (uint64_t i = 0; i < n; ++i)
        out[i] = hyperdex::hash(static_cast<hyperdatatype>(type), e::slice(blob + off[i], len[i]));
    return REF_OK;
}

// hyperdex::hash(schema, key, value, hs) over n objects of the packed layout:
// object i's attributes lie back to back from blob + obj_base[i], attribute j
// attr_len[i * attrs_sz + j] bytes long (attribute 0 is the key);
// out[i * attrs_sz + j] = hs[j].  The schema is built from `types`.
REF_EXPORT int ref_hash_object(const uint32_t* types, uint32_t attrs_sz, const uint8_t* blob,
                               const uint64_t* obj_base, const uint32_t* attr_len, uint64_t n, uint64_t* out) {
    if (attrs_sz == 0 || attrs_sz > 65535) return REF_E_INVALID;
    for (uint32_t j = 0; j < attrs_sz; ++j)
        if (datatype_info::lookup(static_cast<hyperdatatype>(types[j])) == NULL) return REF_E_BADTYPE;
    for (uint64_t i = 0; i < n; ++i)
        for (uint32_t j = 0; j < attrs_sz; ++j) {
            const int e = ref_refuses(types[j], attr_len[i * attrs_sz + j]);
            if (e != REF_OK) return e;
        }
    attribute* attrs = new attribute[attrs_sz];  // filled member by member: the copy operations are not linked
    for (uint32_t j = 0; j < attrs_sz; ++j) {
        attrs[j].name = "a";
        attrs[j].type = static_cast<hyperdatatype>(types[j]);
    }
    schema sc;
    sc.attrs_sz = static_cast<uint16_t>(attrs_sz);
    sc.attrs = attrs;
    std::vector<e::slice> value(attrs_sz - 1);
    for (uint64_t i = 0; i < n; ++i) {
        const uint32_t* len = attr_len + i * attrs_sz;
        const uint8_t* p = blob + obj_base[i];
        const e::slice key(p, len[0]);
        p += len[0];
        for (uint32_t j = 1; j < attrs_sz; ++j) {
            value[j - 1] = e::slice(p, len[j]);
            p += len[j];
        }
        hyperdex::hash(sc, key, value, out + i * attrs_sz);
    }
    delete[] attrs;
    return REF_OK;
}
