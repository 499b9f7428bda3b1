// ref_checks_glue.cc — TEST INFRASTRUCTURE ONLY.
//
// Links the reference's own attribute checks — common/attribute_check.cc,
// compiled unmodified from the reference tree by oracle/Makefile, with the hash
// chain of libref_hash.so and ref_hash_glue.cc beside it (the datatypes'
// validate, compare, length and regex live in common/datatype_{string,int64,
// float,timestamp}.cc and common/regex_match.cc) — into
// oracle/_ref/libref_checks.so and exports them under C linkage (the
// reference's namespace has hidden visibility).
//
// This file stands in for common/serialization.cc, which pulls in libe's
// packers: the hyperdatatype / hyperpredicate serialization operators, every
// one an abort().  It holds no predicate logic, no compare and no validate.
// The libe stand-ins this target adds are in ref_stub_checks/ (complete packer
// types whose operators abort, and e::slice's equality).
//
// ref_hash_glue.cc's lookup() knows the nine hashable types only: a container,
// document or macaroon datatype on either side of a check returns false at the
// reference's NULL check and pins nothing.  The numeric compare()s unpack with
// an assert on the size: ref_compare refuses an operand that is neither empty
// nor 8 bytes with an error code and never calls into the reference with one.
// passes_attribute_check validates both values before it compares.
#include <stdint.h>
#include <stdlib.h>

#include <vector>

#include "common/attribute.h"
#include "common/attribute_check.h"
#include "common/datatype_info.h"
#include "common/schema.h"
#include "common/serialization.h"

using hyperdex::attribute;
using hyperdex::attribute_check;
using hyperdex::datatype_info;
using hyperdex::schema;

// ---- stand-in for common/serialization.cc (linked, never called) ---------------------

e::packer hyperdex::operator<<(e::packer, const hyperdatatype&) { abort(); }
e::unpacker hyperdex::operator>>(e::unpacker, hyperdatatype&) { abort(); }
size_t hyperdex::pack_size(const hyperdatatype&) { abort(); }
e::packer hyperdex::operator<<(e::packer, const hyperpredicate&) { abort(); }
e::unpacker hyperdex::operator>>(e::unpacker, hyperpredicate&) { abort(); }
size_t hyperdex::pack_size(const hyperpredicate&) { abort(); }

// ---- the exports ------------------------------------------------------------------

#define REF_EXPORT extern "C" __attribute__((visibility("default")))

enum { REF_OK = 0, REF_E_BADTYPE = 1, REF_E_BADSIZE = 2, REF_E_INVALID = 4 };

// hyperdex::passes_attribute_check(T, {datatype D, predicate, value k}, v) -> 0 / 1
REF_EXPORT int ref_passes_attribute_check(uint32_t T, uint32_t D, uint32_t predicate, const uint8_t* k, size_t klen,
                                          const uint8_t* v, size_t vlen) {
    attribute_check c;
    c.attr = 0;
    c.value = e::slice(k, klen);
    c.datatype = static_cast<hyperdatatype>(D);
    c.predicate = static_cast<hyperpredicate>(predicate);
    return hyperdex::passes_attribute_check(static_cast<hyperdatatype>(T), c, e::slice(v, vlen)) ? 1 : 0;
}

// hyperdex::passes_attribute_checks(schema, checks, key, value) -> the
// reference's size_t.  The schema is built from `types` member by member;
// check i is (ck_attr[i], ck_type[i], ck_pred[i], ck_val[i] of ck_len[i]
// bytes); value[j - 1] = vals[j - 1] of val_len[j - 1] bytes for 1 <= j < attrs_sz.
REF_EXPORT uint64_t ref_passes_attribute_checks(const uint32_t* types, uint32_t attrs_sz, const uint16_t* ck_attr,
                                                const uint32_t* ck_type, const uint32_t* ck_pred,
                                                const uint8_t* const* ck_val, const uint64_t* ck_len, uint32_t nchecks,
                                                const uint8_t* key, uint64_t key_len, const uint8_t* const* vals,
                                                const uint64_t* val_len) {
    if (attrs_sz == 0 || attrs_sz > 65535) abort();
    attribute* attrs = new attribute[attrs_sz];  // filled member by member: the copy operations are not linked
    for (uint32_t j = 0; j < attrs_sz; ++j) {
        attrs[j].name = "a";
        attrs[j].type = static_cast<hyperdatatype>(types[j]);
    }
    schema sc;
    sc.attrs_sz = static_cast<uint16_t>(attrs_sz);
    sc.attrs = attrs;
    std::vector<attribute_check> checks(nchecks);
    for (uint32_t i = 0; i < nchecks; ++i) {
        checks[i].attr = ck_attr[i];
        checks[i].value = e::slice(ck_val[i], ck_len[i]);
        checks[i].datatype = static_cast<hyperdatatype>(ck_type[i]);
        checks[i].predicate = static_cast<hyperpredicate>(ck_pred[i]);
    }
    std::vector<e::slice> value(attrs_sz - 1);
    for (uint32_t j = 1; j < attrs_sz; ++j) value[j - 1] = e::slice(vals[j - 1], val_len[j - 1]);
    const size_t r = hyperdex::passes_attribute_checks(sc, checks, e::slice(key, key_len), value);
    delete[] attrs;
    return r;
}

// *sign = the sign of datatype_info::lookup(type)->compare(a, b)
REF_EXPORT int ref_compare(uint32_t type, const uint8_t* a, size_t alen, const uint8_t* b, size_t blen, int* sign) {
    datatype_info* di = datatype_info::lookup(static_cast<hyperdatatype>(type));
    if (di == NULL || !di->comparable()) return REF_E_BADTYPE;
    if (type != HYPERDATATYPE_STRING && ((alen != 0 && alen != 8) || (blen != 0 && blen != 8))) return REF_E_BADSIZE;
    const int c = di->compare(e::slice(a, alen), e::slice(b, blen));
    *sign = (c > 0) - (c < 0);
    return REF_OK;
}

// datatype_info::lookup(type)->validate(v) -> 0 / 1, or -1 for a type lookup() does not know
REF_EXPORT int ref_validate(uint32_t type, const uint8_t* v, size_t len) {
    datatype_info* di = datatype_info::lookup(static_cast<hyperdatatype>(type));
    if (di == NULL) return -1;
    return di->validate(e::slice(v, len)) ? 1 : 0;
}
