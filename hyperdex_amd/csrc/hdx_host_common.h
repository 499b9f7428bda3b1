// hdx_host_common.h — declarations the host translation units share that need
// no HIP header (the CPU per-object path, hdx_cpu.cpp, includes only this).
#pragma once

#include <stdint.h>

#include "../../include/hdxhash.h"

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

}  // namespace hdx
