// hdx_value_walk.h — one lane's walk over a stored value's [u32 BE len] chain:
// decode_value (daemon/datalayer_encodings.cc:174-213) under the sweep's
// contract — the 10-byte header, count == A - 1, every length prefix and
// every attribute inside the value — so its verdict is the sweep's at any A.
// Shared by the kernels that give a lane per object (index_plan_kernel,
// hdx_index_entries.hip; check_kernel, hdx_checks.hip;
// sorted_rank_kernel, hdx_sorted.hip).  hdx_wide.hip keeps
// its own walk: it stores descriptors 16 at a time.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hdx_wave.h"

namespace hdx {

// Calls on_attr(j, pos, L) for attribute j = 1 .. A-1 in order: L bytes at
// v + pos, lying inside the value.  Returns false where the value is refused
// (attributes reported before the refusal are then to be ignored).  Reads
// unaligned dwords lying wholly inside the value.
template <typename F>
__device__ __forceinline__ bool value_walk(const uint8_t* v, uint32_t vlen, uint32_t A, F&& on_attr) {
    if (vlen < 10) return false;
    if ((__builtin_bswap32(*(gu32_ptr)(v + 6)) & 0xffffu) != A - 1) return false;  // the u16 at bytes 8..9
    uint32_t pos = 10;  // pos <= vlen throughout
    for (uint32_t j = 1; j < A; ++j) {
        if (vlen - pos < 4) return false;
        const uint32_t L = __builtin_bswap32(*(gu32_ptr)(v + pos));
        pos += 4;
        if (L > vlen - pos) return false;
        on_attr(j, pos, L);
        pos += L;
    }
    return true;
}

// Attribute attr (1 .. A-1) of a value value_walk accepts: the walk up to it
// and no further, L bytes at v + pos.
__device__ __forceinline__ void value_attr(const uint8_t* v, uint32_t attr, uint32_t* pos_out, uint32_t* len_out) {
    uint32_t pos = 10, L;
    for (uint32_t j = 1;; ++j) {
        L = __builtin_bswap32(*(gu32_ptr)(v + pos));
        pos += 4;
        if (j == attr) break;
        pos += L;
    }
    *pos_out = pos;
    *len_out = L;
}

}  // namespace hdx
