// ref_store_glue.cc — TEST INFRASTRUCTURE ONLY.
//
// Links the reference's own stored-value coder, numeric index encoders and
// partitioner — daemon/datalayer_encodings.cc, daemon/index_{int64,float,
// timestamp}.cc and admin/partition.cc, compiled unmodified from the reference
// tree by oracle/Makefile, with the hash chain of libref_hash.so and
// ref_hash_glue.cc beside them — into oracle/_ref/libref_store.so and exports
// them under C linkage (the reference's namespace has hidden visibility).
//
// This file stands in for daemon/index_info.cc, daemon/index_primitive.cc,
// common/hyperspace.cc and libe's varint functions, which pull in LevelDB, the
// container and document indices and libe's packers.  It holds no decoding,
// encoding or partition logic: a lookup() over the three numeric encoders,
// base-class constructors and destructors, member-wise special members of
// region and replica, and abort() for every other symbol the link wants, so
// that reaching one fails loudly.
//
// The numeric encoders call datatype_*::hash, which asserts on a value that is
// neither empty nor 8 bytes; partition() asserts on zero attributes and divides
// by zero servers.  The exports refuse those inputs with an error code and
// never call into the reference with them.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "admin/partition.h"
#include "common/hyperspace.h"
#include "daemon/datalayer_encodings.h"
#include "daemon/index_float.h"
#include "daemon/index_info.h"
#include "daemon/index_int64.h"
#include "daemon/index_primitive.h"
#include "daemon/index_timestamp.h"

using hyperdex::datalayer;
using hyperdex::index_encoding;
using hyperdex::index_info;
using hyperdex::index_primitive;
using hyperdex::region;
using hyperdex::replica;

// ---- stand-in for daemon/index_info.cc -------------------------------------------

namespace {
hyperdex::index_encoding_int64 e_int64;
hyperdex::index_encoding_float e_float;
hyperdex::index_encoding_timestamp e_timestamp;
}  // namespace

const index_encoding* index_encoding::lookup(hyperdatatype t) {
    switch (static_cast<uint32_t>(t)) {
        case HYPERDATATYPE_INT64: return &e_int64;
        case HYPERDATATYPE_FLOAT: return &e_float;
        case HYPERDATATYPE_TIMESTAMP_SECOND:
        case HYPERDATATYPE_TIMESTAMP_MINUTE:
        case HYPERDATATYPE_TIMESTAMP_HOUR:
        case HYPERDATATYPE_TIMESTAMP_DAY:
        case HYPERDATATYPE_TIMESTAMP_WEEK:
        case HYPERDATATYPE_TIMESTAMP_MONTH: return &e_timestamp;
        default: return NULL;
    }
}

index_encoding::index_encoding() {}
index_encoding::~index_encoding() throw() {}

const index_info* index_info::lookup(hyperdatatype) { abort(); }
index_info::index_info() {}
index_info::~index_info() throw() {}
datalayer::index_iterator* index_info::iterator_for_keys(hyperdex::leveldb_snapshot_ptr,
                                                         const hyperdex::region_id&) const { abort(); }
datalayer::index_iterator* index_info::iterator_from_range(hyperdex::leveldb_snapshot_ptr, const hyperdex::region_id&,
                                                           const hyperdex::index_id&, const hyperdex::range&,
                                                           const index_encoding*) const { abort(); }
datalayer::index_iterator* index_info::iterator_from_check(hyperdex::leveldb_snapshot_ptr, const hyperdex::region_id&,
                                                           const hyperdex::index_id&, const hyperdex::attribute_check&,
                                                           const index_encoding*) const { abort(); }

// ---- stand-in for daemon/index_primitive.cc (the index classes are linked, never built) --

index_primitive::index_primitive(const index_encoding* ie) : m_ie(ie) {}
index_primitive::~index_primitive() throw() {}
void index_primitive::index_changes(const hyperdex::index*, const hyperdex::region_id&, const index_encoding*,
                                    const e::slice&, const e::slice*, const e::slice*,
                                    leveldb::WriteBatch*) const { abort(); }
datalayer::index_iterator* index_primitive::iterator_for_keys(hyperdex::leveldb_snapshot_ptr,
                                                              const hyperdex::region_id&) const { abort(); }
datalayer::index_iterator* index_primitive::iterator_from_range(hyperdex::leveldb_snapshot_ptr,
                                                                const hyperdex::region_id&, const hyperdex::index_id&,
                                                                const hyperdex::range&,
                                                                const index_encoding*) const { abort(); }

// ---- stand-in for common/hyperspace.cc: region and replica, member-wise --------------

region::region() : id(), lower_coord(), upper_coord(), replicas() {}
region::region(const region& o)
    : id(o.id), lower_coord(o.lower_coord), upper_coord(o.upper_coord), replicas(o.replicas) {}
region::~region() throw() {}
region& region::operator=(const region& o) {
    id = o.id;
    lower_coord = o.lower_coord;
    upper_coord = o.upper_coord;
    replicas = o.replicas;
    return *this;
}

replica::replica() : si(), vsi() {}
replica::replica(const replica& o) : si(o.si), vsi(o.vsi) {}
replica::~replica() throw() {}
replica& replica::operator=(const replica& o) {
    si = o.si;
    vsi = o.vsi;
    return *this;
}

// ---- stand-in for libe's varint functions (key prefixes only; no test reaches them) ---

namespace e {
size_t varint_length(uint64_t) { abort(); }
char* packvarint64(uint64_t, char*) { abort(); }
const char* varint64_decode(const char*, const char*, uint64_t*) { abort(); }
}  // namespace e

// ---- the exports ------------------------------------------------------------------

#define REF_EXPORT extern "C" __attribute__((visibility("default")))

enum { REF_OK = 0, REF_E_BADTYPE = 1, REF_E_BADSIZE = 2, REF_E_INVALID = 4 };

// hyperdex::decode_value(e::slice(val, len), &attrs, &version).  *rc is the
// datalayer::returncode as the reference numbers it, *count is attrs.size()
// whatever the return code, and the first min(*count, max_attrs) slices are
// reported as (offset of slice.data() from val, slice.size()).  No slice is
// ever dereferenced: the last one may end past the value.
REF_EXPORT int ref_decode_value(const uint8_t* val, uint64_t len, uint64_t max_attrs, int32_t* rc, uint64_t* version,
                                uint64_t* count, uint64_t* off, uint64_t* n) {
    std::vector<e::slice> attrs;
    *version = 0;
    *rc = static_cast<int32_t>(hyperdex::decode_value(e::slice(val, len), &attrs, version));
    *count = attrs.size();
    for (uint64_t i = 0; i < attrs.size() && i < max_attrs; ++i) {
        off[i] = static_cast<uint64_t>(reinterpret_cast<uintptr_t>(attrs[i].data()) -
                                       reinterpret_cast<uintptr_t>(val));
        n[i] = attrs[i].size();
    }
    return REF_OK;
}

// the numbering *rc uses
REF_EXPORT int32_t ref_rc_success() { return static_cast<int32_t>(datalayer::SUCCESS); }
REF_EXPORT int32_t ref_rc_bad_encoding() { return static_cast<int32_t>(datalayer::BAD_ENCODING); }

// hyperdex::encode_value over attribute i = blob[off[i] .. off[i] + len[i]);
// returns the encoded size and copies it to out where out_cap holds it.
REF_EXPORT uint64_t ref_encode_value(const uint8_t* blob, const uint64_t* off, const uint32_t* len, uint32_t nattrs,
                                     uint64_t version, uint8_t* out, uint64_t out_cap) {
    if (nattrs > 65535) return 0;
    std::vector<e::slice> attrs(nattrs);
    for (uint32_t i = 0; i < nattrs; ++i) attrs[i] = e::slice(blob + off[i], len[i]);
    std::vector<char> backing;
    leveldb::Slice s;
    hyperdex::encode_value(attrs, version, &backing, &s);
    if (s.size() <= out_cap) memcpy(out, s.data(), s.size());
    return s.size();
}

static int index_refuses(uint32_t type, uint64_t len) {
    if (index_encoding::lookup(static_cast<hyperdatatype>(type)) == NULL) return REF_E_BADTYPE;
    if (len != 0 && len != 8) return REF_E_BADSIZE;
    return REF_OK;
}

// index_encoding::lookup(type)->encoded_size(value), or -1 for a type without a numeric encoder
REF_EXPORT int64_t ref_index_encoded_size(uint32_t type, const uint8_t* data, uint64_t len) {
    const index_encoding* ie = index_encoding::lookup(static_cast<hyperdatatype>(type));
    if (ie == NULL) return -1;
    return static_cast<int64_t>(ie->encoded_size(e::slice(data, len)));
}

// index_encoding::lookup(type)->encode(value, out); out holds 16 bytes,
// *written is how far encode() advanced.
REF_EXPORT int ref_index_encode(uint32_t type, const uint8_t* data, uint64_t len, uint8_t* out, uint64_t* written) {
    const int e = index_refuses(type, len);
    if (e != REF_OK) return e;
    const index_encoding* ie = index_encoding::lookup(static_cast<hyperdatatype>(type));
    char* begin = reinterpret_cast<char*>(out);
    *written = static_cast<uint64_t>(ie->encode(e::slice(data, len), begin) - begin);
    return REF_OK;
}

// hyperdex::partition(num_attrs, num_servers, &regions): the region count in
// *count, and where cap holds them the boxes, region-major.
REF_EXPORT int ref_partition(uint32_t num_attrs, uint32_t num_servers, uint64_t* count, uint64_t* lower,
                             uint64_t* upper, uint64_t cap) {
    if (num_attrs == 0 || num_attrs > 65535 || num_servers == 0) return REF_E_INVALID;
    std::vector<region> regions;
    hyperdex::partition(static_cast<uint16_t>(num_attrs), num_servers, &regions);
    *count = regions.size();
    if (regions.size() > cap) return REF_OK;
    for (size_t r = 0; r < regions.size(); ++r) {
        if (regions[r].lower_coord.size() != num_attrs || regions[r].upper_coord.size() != num_attrs)
            return REF_E_INVALID;
        for (uint32_t a = 0; a < num_attrs; ++a) {
            lower[r * num_attrs + a] = regions[r].lower_coord[a];
            upper[r * num_attrs + a] = regions[r].upper_coord[a];
        }
    }
    return REF_OK;
}
