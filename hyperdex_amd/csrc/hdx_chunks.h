// hdx_chunks.h — the chunk rule of the host-resident pipelines
// (hdx_hostpath.cpp): which objects of a call travel together, and whether as
// the byte span(s) that hold them or packed in index order.  It reads offsets
// and lengths only, never the objects' bytes.  Host-only, no HIP:
// tests/cpp/sanitize_test.cc builds it under ASan/UBSan.
#pragma once

#include <stdint.h>

#include "hdx_host_common.h"

namespace hdx {

constexpr uint64_t kChunkBytes = 128ull << 20;  // payload bytes per in-flight chunk
// A chunk packed on the device (hdx_gather.hip) grows to this: its two slots'
// kernels share one hardware queue, so each chunk pays ~0.5 ms of queue
// turnaround between its gather and the next (profiles/r6/host_order_trace.txt);
// larger chunks amortise it (device staging only: no pinned copy)
constexpr uint64_t kPackChunkBytes = 512ull << 20;
// A call's first chunk: small, so the first copy starts after a few
// milliseconds less of host-side validation (later chunks are validated while
// the previous ones move)
constexpr uint64_t kFirstChunkBytes = 16ull << 20;

// A chunk whose objects' byte span is no more than this much over their
// payload goes as one span copy (no gather); otherwise its objects are packed
// in index order (hdx_gather.hip for pinned sources, a host copy per object
// for pageable ones), so a batch in any order moves only its own bytes.
inline bool span_pays(uint64_t span, uint64_t payload) {
    return span <= kChunkBytes && span <= payload + payload / 8 + (64u << 10);
}

// A call's objects lie in one or two stores (byte arrays): a packed batch's
// blob; stored objects' records (keys == vals); a key column beside the
// values.  An object is one or two extents, and has one in every store.
constexpr uint32_t kMaxStores = 2;
struct Extent {
    uint32_t store;
    uint64_t off, len;
};
struct ObjectExtents {
    uint32_t count = 0;
    Extent ext[2] = {};
    uint64_t bytes() const { return ext[0].len + (count > 1 ? ext[1].len : 0); }
};

// Objects [first, first + cnt) of a call, moved together.
struct Chunk {
    uint64_t first = 0, cnt = 0;  // cnt 0: the call has no further chunk
    bool span = false;            // moved as each store's [lo, hi); else packed in index order
    uint32_t stores = 0;
    uint64_t lo[kMaxStores] = {UINT64_MAX, UINT64_MAX}, hi[kMaxStores] = {0, 0};
    uint64_t payload = 0;  // the objects' own bytes

    uint64_t span_bytes() const {
        uint64_t b = 0;
        for (uint32_t s = 0; s < stores; ++s) b += hi[s] - lo[s];
        return b;
    }
    uint64_t moved() const { return span ? span_bytes() : payload; }  // bytes that cross to the device
    void add(const ObjectExtents& o) {
        for (uint32_t x = 0; x < o.count; ++x) {
            const Extent& e = o.ext[x];
            widen(e.store ? 1 : 0, e.off, e.off + e.len);
            payload += e.len;
        }
    }

private:
    // constant indices on both sides of the branch: a chunk being grown stays in registers
    void widen(int s, uint64_t from, uint64_t to) {
        if (s == 0) {
            if (from < lo[0]) lo[0] = from;
            if (to > hi[0]) hi[0] = to;
        } else {
            if (from < lo[1]) lo[1] = from;
            if (to > hi[1]) hi[1] = to;
        }
    }
};

// Where a call's planning stands: the next chunk's first object, and that
// object's extents when it was validated as the one that did not fit the chunk
// before (every object is validated once).
struct ChunkCursor {
    uint64_t next = 0;
    bool held = false;
    ObjectExtents ahead;
};

// The next chunk of a call's n objects.  Source:
//   uint32_t stores() const;
//   hdx_status object(uint64_t i, ObjectExtents& o);  // validates object i; its extents
// A chunk starts with object cur.next, whatever its size, and grows by payload
// to kFirstChunkBytes (a call's first) or kChunkBytes; one that the device
// would pack (device_packs: every store has a device view) grows on to
// kPackChunkBytes.  An object that fails validation ends planning with the
// source's status: the chunk being grown is not produced.
// Not inlined: its loop runs once per object of the call with the chunk and
// the object in hand in registers; inlined into the driver they spill to the
// stack, which cost a shuffled 2 M-object call 0.8 ms of 50.
template <typename Source>
__attribute__((noinline)) hdx_status next_chunk(Source& src, uint64_t n, bool device_packs, ChunkCursor& cur, Chunk& c) {
    c = Chunk{};
    if (cur.next >= n) return HDX_OK;
    // the chunk and the object in hand are locals, stored to c and cur once
    // per chunk, and src.object has one call site (inlined)
    Chunk g;
    g.first = cur.next;
    g.stores = src.stores();
    uint64_t limit = g.first == 0 ? kFirstChunkBytes : kChunkBytes;
    uint64_t e = g.first;
    if (cur.held) {  // validated as the object that did not fit the chunk before
        g.add(cur.ahead);
        cur.held = false;
        ++e;
    }
    ObjectExtents o;
    for (; e < n; ++e) {
        const hdx_status st = src.object(e, o);
        if (st != HDX_OK) return st;
        const uint64_t size = o.bytes();
        if (e > g.first && g.payload + size > limit) {  // the first object joins whatever its size
            // a chunk the device will pack grows further
            if (limit == kChunkBytes && device_packs && !span_pays(g.span_bytes(), g.payload)) limit = kPackChunkBytes;
            if (g.payload + size > limit) {
                cur.held = true;  // starts the next chunk
                cur.ahead = o;
                break;
            }
        }
        g.add(o);
    }
    g.cnt = e - g.first;
    // one object whose spans hold nothing else moves as spans, however large
    g.span = span_pays(g.span_bytes(), g.payload) || (g.cnt == 1 && g.span_bytes() == g.payload);
    cur.next = e;
    c = g;
    return HDX_OK;
}

}  // namespace hdx
