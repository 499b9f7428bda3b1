// hdx_gather_objects.hip — the objects behind a list of indices, packed back
// to back on gfx950: what a search sends per item (daemon/search_manager.cc:
// 267-281, :484-501, :505-560), as stored objects rather than in the wire
// format (the contract is in include/hdxhash.h).  Record r = [key of idx[r] if
// KEYS][value of idx[r] if VALUES] at out + rec_off[r].
//
//   plan  gather_plan_kernel: a lane per record stores its size (0 past the
//         count and for an index >= n) and its key length; then scan_exclusive
//         (hdx_scratch.hip) over the cap + 1 sizes, the last one 0, so
//         rec_off[cap] is the total.
//   fill  gather_fill_kernel, tile-owned: the output is cut into tiles of
//         kGatherTileBytes from its 16-byte-aligned base, a wave per tile, so
//         the lanes are busy whatever the record sizes (a wave per record
//         idles most lanes below ~1 KiB and on 8-byte keys).  The wave finds
//         the first record that touches its tile by one search of rec_off in
//         which each round the 64 lanes probe 64 points (first_record: 4
//         rounds for 10^6 records), then keeps a window of 64 records in LDS:
//         their 65 offsets and, for the records with bytes in the tile, where
//         the key and the value lie.  A step is 64 lanes x one destination-
//         aligned 16-byte chunk; when a step runs past the window the wave
//         loads the next one.  A lane finds its record in the window by a
//         search of the LDS offsets and assembles its chunk:
//           - 16 bytes inside one key or value: one unaligned 16-byte load
//             (all 16 bytes are the object's);
//           - else piece by piece along the records the chunk crosses (8-byte
//             keys put two in a chunk, empty records any number): an
//             unaligned 8- or 4-byte load lying wholly inside the key or
//             value, or, for 1-3 bytes, the one or two aligned dwords that
//             hold the bytes taken (tail_bytes, hdx_wave.h: each holds a
//             byte of the object, so it lies in the object's pages).  No
//             dword without a byte of the object is read.
//         Whole chunks are stored as 16 aligned bytes; the chunks at the
//         output's two ends, shared with the caller's memory, byte by byte,
//         only the output's own bytes, never read (index_fill_kernel's rule).
//         Tiles end on chunk boundaries, so no two waves share a chunk.
//
// No kernel waits on another workgroup and no atomic hands out positions.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdint.h>

#include "hdx_internal.h"
#include "hdx_wave.h"

namespace hdx {

namespace {

constexpr uint32_t kChunk = 16;                        // bytes a lane stores per step
constexpr uint32_t kStepBytes = 64 * kChunk;           // a wave's step
constexpr uint32_t kSteps = kGatherTileBytes / kStepBytes;
constexpr uint32_t kWindow = 64;                       // records of a window: one lane loads one
static_assert(kSteps * kStepBytes == kGatherTileBytes && (kGatherTileBytes & (kGatherTileBytes - 1)) == 0, "tile");

// ---- plan -----------------------------------------------------------------

__global__ void __launch_bounds__(256) gather_plan_kernel(const GatherObjectsArgs a) {
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    uint64_t count = a.cap;
    if (a.count) {
        const uint64_t given = *a.count;
        if (given < count) count = given;
    }
    bool bad = false;
    if (r < a.cap) {
        uint64_t size = 0;
        uint32_t kl = 0;
        if (r < count) {
            const uint64_t i = a.idx[r];
            if (i < a.n) {
                if (a.what & HDX_GATHER_KEYS) kl = a.key_len[i];
                size = (uint64_t)kl + ((a.what & HDX_GATHER_VALUES) ? a.val_len[i] : 0u);
            } else {
                bad = true;
            }
        }
        a.rec_off[r] = size;
        if (a.rec_key_len) a.rec_key_len[r] = kl;
    }
    wave_status_or(a.status, bad, kStatusInvalid);
    if (r == 0) a.rec_off[a.cap] = 0;  // the scan's last element: the total lands here
}

// ---- fill -----------------------------------------------------------------

// What a wave keeps in LDS of kWindow consecutive records from record r on:
// ro[j] = rec_off[min(r + j, cap)], and of each record with bytes in the
// wave's tile the addresses of its key and value and its key length.
struct GatherWindow {
    uint64_t ro[kWindow + 1];
    uint64_t ksrc[kWindow], vsrc[kWindow];
    uint32_t klen[kWindow];
};

// The record that holds output position p: the last r in [lo, cap) with
// rec_off[r] <= p, given rec_off[lo] <= p < rec_off[cap] (empty records are
// stepped over: rec_off[r + 1] > p).  Wave-uniform; each round the lanes probe
// 64 points of the span left and a ballot keeps one 64th of it.
__device__ __forceinline__ uint64_t first_record(const uint64_t* rec_off, uint64_t cap, uint64_t p, uint64_t lo,
                                                 uint32_t lane) {
    uint64_t hi = cap;
    while (hi - lo > 1) {
        const uint64_t span = hi - lo, step = (span + 63) / 64;
        const uint64_t probe = lo + std::min<uint64_t>((uint64_t)(lane + 1) * step, span);
        const bool le = probe < hi && rec_off[probe] <= p;  // rec_off[hi] > p
        const uint32_t c = (uint32_t)__popcll(__ballot(le));  // rec_off ascends: the lanes that hold form a prefix, c <= 63
        hi = lo + std::min<uint64_t>((uint64_t)(c + 1) * step, span);
        lo += (uint64_t)c * step;
    }
    return lo;
}

// Loads the window from record r on.  A record's descriptor is read only when
// it has bytes (so r + lane < count and its index is < n: the plan gave every
// other record size 0) and starts before tile_end.
__device__ __forceinline__ void stage_window(GatherWindow& g, const GatherObjectsArgs& a, uint64_t r,
                                             uint64_t tile_end, uint32_t lane) {
    wave_fence();  // the previous window is done with
    const uint64_t j = r + lane;
    const uint64_t o0 = a.rec_off[std::min<uint64_t>(j, a.cap)];
    const uint64_t o1 = a.rec_off[std::min<uint64_t>(j + 1, a.cap)];
    g.ro[lane] = o0;
    if (lane == kWindow - 1) g.ro[kWindow] = o1;
    if (o1 > o0 && o0 < tile_end) {
        const uint64_t i = a.idx[j];
        uint32_t kl = 0;
        uint64_t ks = 0, vs = 0;
        if (a.what & HDX_GATHER_KEYS) {
            kl = a.key_len[i];
            ks = (uint64_t)(uintptr_t)(a.keys + a.key_off[i]);
        }
        if (a.what & HDX_GATHER_VALUES) vs = (uint64_t)(uintptr_t)(a.vals + a.val_off[i]);
        g.klen[lane] = kl;
        g.ksrc[lane] = ks;
        g.vsrc[lane] = vs;
    }
    wave_fence();
}

// v into dword w of the chunk (no indexed register array)
__device__ __forceinline__ void put_dword(u32x4& o, uint32_t w, uint32_t v) {
    o.x |= w == 0 ? v : 0u;
    o.y |= w == 1 ? v : 0u;
    o.z |= w == 2 ? v : 0u;
    o.w |= w == 3 ? v : 0u;
}

// The lane's chunk holds output positions [cpos, cpos + 16) (cpos may be
// "negative" for the output's first chunk: wrapped, only differences are
// used).  Adds the bytes of positions [p, lim) to o from the window's records
// and returns lim; g.ro[0] <= p < lim <= g.ro[kWindow].
__device__ __forceinline__ uint64_t chunk_bytes(const GatherWindow& g, uint64_t cpos, uint64_t p, uint64_t lim,
                                                u32x4& o) {
    uint32_t t = 0;  // the record that holds p: the last t with ro[t] <= p
#pragma unroll
    for (uint32_t step = kWindow / 2; step; step >>= 1)
        if (g.ro[t + step] <= p) t += step;
    while (p < lim) {
        while (g.ro[t + 1] <= p) ++t;  // p < ro[kWindow], so t < kWindow
        const uint64_t off = p - g.ro[t];
        const uint32_t kl = g.klen[t];
        const uint8_t* src;
        uint64_t rem;  // bytes left of the key or of the value
        if (off < kl) {
            src = (const uint8_t*)(uintptr_t)g.ksrc[t] + off;
            rem = kl - off;
        } else {
            src = (const uint8_t*)(uintptr_t)g.vsrc[t] + (off - kl);
            rem = g.ro[t + 1] - p;
        }
        const uint32_t b = (uint32_t)(p - cpos);  // the byte of the chunk p is
        const uint64_t room = std::min<uint64_t>(rem, lim - p);
        if (b == 0 && room >= kChunk) {
            o = *(gu128_ptr)src;
            p += kChunk;
        } else if ((b & 3) == 0 && room >= 8) {  // b <= 8
            const uint64_t v = *(gu64_ptr)src;
            put_dword(o, b >> 2, (uint32_t)v);
            put_dword(o, (b >> 2) + 1, (uint32_t)(v >> 32));
            p += 8;
        } else {  // up to the end of the chunk's dword
            const uint32_t take = (uint32_t)std::min<uint64_t>(room, 4 - (b & 3));
            put_dword(o, b >> 2, tail_bytes(src, take) << (8 * (b & 3)));
            p += take;
        }
    }
    return p;
}

__global__ void __launch_bounds__(256) gather_fill_kernel(const GatherObjectsArgs a) {
    __shared__ GatherWindow s_window[4];
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint64_t total = a.rec_off[a.cap];
    if (total > a.out_bytes) {  // the caller's buffer is too small: nothing is written
        if (blockIdx.x == 0 && threadIdx.x == 0 && a.status) atomicOr(a.status, kStatusNoMem);
        return;
    }
    if (total == 0) return;
    GatherWindow& g = s_window[w];
    const uintptr_t dst = (uintptr_t)a.out;
    const uint32_t lead = (uint32_t)(dst & (kChunk - 1));
    uint8_t* const base = a.out - lead;  // 16-byte aligned; aligned offset x holds output position x - lead
    const uint64_t end = lead + total;   // aligned offset of the output's end
    const uint64_t tiles = (end + kGatherTileBytes - 1) / kGatherTileBytes, nwaves = (uint64_t)gridDim.x * 4;
    for (uint64_t tile = (uint64_t)blockIdx.x * 4 + w; tile < tiles; tile += nwaves) {
        const uint64_t x0 = tile * kGatherTileBytes;
        const uint64_t p0 = x0 > lead ? x0 - lead : 0;                         // the tile's positions [p0, p1)
        const uint64_t p1 = std::min<uint64_t>(x0 + kGatherTileBytes, end) - lead;  // p0 < p1 <= total
        uint64_t r = first_record(a.rec_off, a.cap, p0, 0, lane);
        stage_window(g, a, r, p1, lane);
        for (uint32_t s = 0; s < kSteps; ++s) {
            const uint64_t xs = x0 + (uint64_t)s * kStepBytes;
            if (xs >= end) break;  // wave-uniform
            const uint64_t s1 = std::min<uint64_t>(xs + kStepBytes, end) - lead;  // the step's last position + 1
            const uint64_t x = xs + (uint64_t)lane * kChunk;                      // the lane's chunk
            const uint64_t cpos = x - lead;                                       // wraps for the first chunk
            const uint64_t lo = x > lead ? x - lead : 0;
            const uint64_t hi = std::min<uint64_t>(x + kChunk, end) - lead;       // may be <= lo: no bytes
            u32x4 o = {0u, 0u, 0u, 0u};
            uint64_t p = lo;
            for (;;) {  // wave-uniform: the windows the step runs through
                const uint64_t wbeg = g.ro[0], wend = g.ro[kWindow];
                if (p < hi && p < wend) p = chunk_bytes(g, cpos, p, std::min(hi, wend), o);
                if (wend >= s1) break;  // the last window ends at the total
                // 64 empty records: search on from them instead of walking the run
                r = wend > wbeg ? r + kWindow : first_record(a.rec_off, a.cap, wend, r + kWindow, lane);
                stage_window(g, a, r, p1, lane);
            }
            if (lo >= hi) continue;
            if (hi - lo == kChunk) {
                *reinterpret_cast<u32x4*>(base + x) = o;
            } else {  // a chunk shared with the caller's memory: only the output's bytes, no read
                const uint32_t b0 = (uint32_t)(lo - cpos), b1 = (uint32_t)(hi - cpos);
                const uint32_t ob[4] = {o.x, o.y, o.z, o.w};
#pragma unroll
                for (uint32_t q = 0; q < kChunk; ++q)
                    if (q >= b0 && q < b1) base[x + q] = (uint8_t)(ob[q >> 2] >> (8 * (q & 3)));
            }
        }
    }
}

}  // namespace

hipError_t launch_gather_objects_plan(const GatherObjectsArgs& a, hipStream_t stream, bool* no_scratch) {
    *no_scratch = false;
    const uint64_t N = a.cap + 1;
    const uint64_t blocks = std::max<uint64_t>((a.cap + 255) / 256, 1);
    if (blocks > 0x7fffffffULL) return hipErrorInvalidValue;
    const uint64_t words = scan_scratch_words(N);
    PoolScratch sums;
    if (words && !sums.acquire(words * 8, stream, no_scratch)) return hipSuccess;
    hipLaunchKernelGGL(gather_plan_kernel, dim3((uint32_t)blocks), dim3(256), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = scan_exclusive(a.rec_off, N, static_cast<uint64_t*>(sums.p), stream);
    return sums.release(e);
}

hipError_t launch_gather_objects_fill(const GatherObjectsArgs& a, hipStream_t stream) {
    // the total is on the device: a wave per tile of the room given, grid-stride above 1 GiB
    const uint64_t tiles = (a.out_bytes + kChunk - 1 + kGatherTileBytes - 1) / kGatherTileBytes;
    const uint64_t blocks = std::min<uint64_t>(std::max<uint64_t>((tiles + 3) / 4, 1), 1ull << 16);
    hipLaunchKernelGGL(gather_fill_kernel, dim3((uint32_t)blocks), dim3(256), 0, stream, a);
    return hipGetLastError();
}

#if HDX_DEBUG_BUILD
namespace {

// Record r as extents 2r (its key) and 2r + 1 (its value): absolute source
// addresses, so the copy's source base is 0.
__global__ void __launch_bounds__(256) gather_extents_plan_kernel(const GatherObjectsArgs a, uint64_t* src_off,
                                                                   uint32_t* len, uint64_t* dst_off) {
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const bool fits = a.rec_off[a.cap] <= a.out_bytes;
    if (r == 0 && !fits && a.status) atomicOr(a.status, kStatusNoMem);
    if (r >= a.cap) return;
    const uint64_t at = a.rec_off[r], size = a.rec_off[r + 1] - at;
    uint32_t kl = 0, vl = 0;
    uint64_t ks = 0, vs = 0;
    if (fits && size) {
        const uint64_t i = a.idx[r];
        if (a.what & HDX_GATHER_KEYS) {
            kl = a.key_len[i];
            ks = (uint64_t)(uintptr_t)(a.keys + a.key_off[i]);
        }
        if (a.what & HDX_GATHER_VALUES) {
            vl = (uint32_t)(size - kl);
            vs = (uint64_t)(uintptr_t)(a.vals + a.val_off[i]);
        }
    }
    src_off[2 * r] = ks;
    len[2 * r] = kl;
    dst_off[2 * r] = at;
    src_off[2 * r + 1] = vs;
    len[2 * r + 1] = vl;
    dst_off[2 * r + 1] = at + kl;
}

}  // namespace

hipError_t launch_gather_objects_by_extents(const GatherObjectsArgs& a, hipStream_t stream, bool* no_scratch) {
    *no_scratch = false;
    const uint64_t E = 2 * a.cap, blocks = std::max<uint64_t>((a.cap + 255) / 256, 1);
    if (blocks > 0x7fffffffULL) return hipErrorInvalidValue;
    PoolScratch scratch;
    if (!scratch.acquire(std::max<uint64_t>(E, 1) * 20, stream, no_scratch)) return hipSuccess;
    uint64_t* src_off = static_cast<uint64_t*>(scratch.p);
    uint64_t* dst_off = src_off + E;
    uint32_t* len = reinterpret_cast<uint32_t*>(dst_off + E);
    hipLaunchKernelGGL(gather_extents_plan_kernel, dim3((uint32_t)blocks), dim3(256), 0, stream, a, src_off, len,
                       dst_off);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = launch_gather_extents(nullptr, src_off, len, dst_off, a.out, E, stream);
    return scratch.release(e);
}
#endif

}  // namespace hdx
