// hdx_index_entries.hip — the secondary-index entries of stored objects on
// gfx950: what datalayer::indexer_thread Puts per object and index
// (daemon/datalayer_indexer_thread.cc:361-399 -> create_index_changes,
// daemon/datalayer_encodings.cc:283-318 -> index_primitive::index_entry,
// daemon/index_primitive.cc:291-329; the composition is restated in
// include/hdxhash.h).  Entry e = i*m + k, object-major.
//
//   plan  index_plan_kernel: a lane per object walks its value's [u32 BE len]
//         chain (value_walk, hdx_value_walk.h: the full walk, as
//         sweep_wide_walk_kernel's, so its verdict is the sweep's), keeps the
//         descriptors of the indexed attributes in LDS, and the workgroup then
//         stores attr_off, attr_len and the entry sizes of its objects
//         coalesced.
//   scan  scan_exclusive (hdx_scratch.hip): the exclusive prefix sum of the
//         n*m + 1 sizes (the last one is 0, so entry_off[n*m] is the total).
//   fill  index_fill_kernel: a wave per group of up to 16 consecutive objects
//         (at most 64 entries).  Object-major order makes the group's entries
//         one contiguous span of the output, which the wave owns; it loads the
//         group's offsets and descriptors into LDS in one step, then each lane
//         takes one destination-aligned dword of the span at a time, finds the
//         entry and segment (prefix, value, key, suffix) its bytes come from,
//         and stores the dword; the dwords at the span's two ends that other
//         waves (or the caller's memory) share are written byte by byte,
//         only the span's own bytes, never read.  Source bytes are read as
//         unaligned dwords / 8-byte values lying wholly inside a key or an
//         attribute, or as the aligned dwords that hold the bytes taken
//         (tail_dwords, hdx_wave.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdint.h>

#include "hdx_device_hash.h"
#include "hdx_internal.h"
#include "hdx_value_walk.h"

namespace hdx {

namespace {

constexpr uint32_t kRefused = 0xffffffffu;

__device__ __forceinline__ uint32_t enc_size(uint32_t enc, uint32_t len) {
    return enc == ENC_STRING ? len : enc == ENC_INT64 ? 8u : 16u;
}

// ---- plan -----------------------------------------------------------------

// blockDim.x objects per workgroup.  Dynamic LDS: off[B*m] | len[B*m] |
// key_size[B] (kRefused: the object is refused) | enc[32] plen[32] as bytes.
__global__ void __launch_bounds__(256) index_plan_kernel(const IndexEntriesArgs a) {
    extern __shared__ uint32_t plan_lds[];
    const uint32_t B = blockDim.x, m = a.m, tid = threadIdx.x;
    uint32_t* s_off = plan_lds;
    uint32_t* s_len = s_off + B * m;
    uint32_t* s_key = s_len + B * m;
    uint8_t* s_enc = reinterpret_cast<uint8_t*>(s_key + B);
    uint8_t* s_plen = s_enc + HDX_MAX_INDICES;
    if (tid < m) {
        s_enc[tid] = a.enc[tid];
        s_plen[tid] = a.plen[tid];
    }
    const uint64_t first = (uint64_t)blockIdx.x * B;
    const uint64_t i = first + tid;
    bool badenc = false, badsize = false;
    for (uint32_t k = 0; k < m; ++k) {
        s_off[tid * m + k] = 0;
        s_len[tid * m + k] = 0;
    }
    if (i < a.n) {
        const uint32_t A = a.A;
        const uint8_t* v = a.vals + a.val_off[i];
        const uint32_t vlen = a.val_len[i];
        // decode_value under the sweep's contract (hdx_value_walk.h)
        const bool ok = value_walk(v, vlen, A, [&](uint32_t j, uint32_t pos, uint32_t L) {
            for (uint32_t k = 0; k < m; ++k)  // uniform: the specs are kernel arguments
                if (a.attr[k] == j) {
                    s_off[tid * m + k] = pos;
                    s_len[tid * m + k] = L;
                    if (a.enc[k] != ENC_STRING && L != 0 && L != 8) badsize = true;
                }
        });
        badenc = !ok;
        const uint32_t kl = a.key_len[i];
        if (a.key_enc != ENC_STRING && kl != 0 && kl != 8) badsize = true;
        badsize = badsize && ok;
        s_key[tid] = (badenc || badsize) ? kRefused : enc_size(a.key_enc, kl);
    }
    wave_status_or(a.status, badenc, kStatusBadEnc);  // one atomic per wave and bit
    wave_status_or(a.status, badsize, kStatusBadSize);
    __syncthreads();
    const uint64_t left = a.n - first;  // > 0: the grid covers n exactly
    const uint32_t cnt = (uint32_t)std::min<uint64_t>(B, left) * m;
    const uint64_t e0 = first * m;
    for (uint32_t t = tid; t < cnt; t += B) {
        const uint32_t o = t / m, k = t - o * m;
        const uint32_t ks = s_key[o];
        uint32_t off = 0, len = 0;
        uint64_t size = 0;
        if (ks != kRefused) {
            off = s_off[t];
            len = s_len[t];
            const uint32_t enc = s_enc[k];
            size = (uint64_t)s_plen[k] + enc_size(enc, len) + ks +
                   ((enc == ENC_STRING && a.key_enc == ENC_STRING) ? 4u : 0u);
        }
        a.attr_off[e0 + t] = off;
        a.attr_len[e0 + t] = len;
        a.entry_off[e0 + t] = size;
    }
    if (blockIdx.x == 0 && tid == 0) a.entry_off[a.n * m] = 0;  // the scan's last element: the total lands here
}

// ---- fill -----------------------------------------------------------------

// The bytes of one segment of an entry, from offset r on: `rem` of them.
// src != NULL: raw bytes of a key or an attribute at src; else the immediate
// lo | hi (little-endian memory order), or, with lds_prefix, the prefix table.
struct Seg {
    const uint8_t* src;
    const uint8_t* lds_prefix;
    uint64_t lo, hi;
    uint32_t r, rem;
};

// Up to four bytes of the segment from offset s.r on, in the low bytes of the
// result (the bytes past `take` are unspecified: the caller masks them).
// Raw bytes: by the load rule of hdx_wave.h (tail_bytes without its mask).
__device__ __forceinline__ uint32_t seg_bytes(const Seg& s, uint32_t take) {
    if (s.src) {
        const uint8_t* p = s.src + s.r;
        if (take == 4) return *(gu32_ptr)p;
        return tail_dwords(p, take);
    }
    if (s.lds_prefix) {  // dwords of the prefix table (padded by one dword)
        const uint32_t* w = reinterpret_cast<const uint32_t*>(s.lds_prefix) + (s.r >> 2);
        return __builtin_amdgcn_alignbyte(w[1], w[0], s.r & 3);
    }
    const uint32_t r = s.r;
    uint64_t v = r < 8 ? s.lo >> (8 * r) : s.hi >> (8 * (r - 8));
    if (r > 4 && r < 8) v |= s.hi << (8 * (8 - r));
    return (uint32_t)v;
}

// enc(type, value) from offset r on (index_{string,int64,float}.cc)
__device__ __forceinline__ void seg_encoded(Seg& s, uint32_t enc, const uint8_t* p, uint32_t len, uint32_t r) {
    s.r = r;
    if (enc == ENC_STRING) {
        s.src = p;
        s.rem = len - r;
        return;
    }
    const uint64_t bits = len == 8 ? *(gu64_ptr)p : 0;  // the plan admits only 0 and 8
    if (enc == ENC_INT64) {
        s.lo = __builtin_bswap64(encode_int64(bits));
        s.rem = 8 - r;
    } else {
        s.lo = __builtin_bswap64(encode_double(bits));
        s.hi = bits;  // packdoublele(number): the value's own bytes, 0.0 when empty
        s.rem = 16 - r;
    }
}

// What a wave keeps in LDS of its group of objects: the G * m + 1 entry
// offsets, each entry's descriptor and object, each object's key and value.
constexpr uint32_t kFillEntries = 64;  // entries per wave and step: one lane loads one
constexpr uint32_t kFillObjects = 16;
struct FillGroup {
    uint64_t eo[kFillEntries + 1];
    uint64_t koff[kFillObjects], voff[kFillObjects];
    uint32_t aoff[kFillEntries], alen[kFillEntries];
    uint32_t klen[kFillObjects];
    uint8_t obj[kFillEntries];
};

// G = fill_group_objects(m) consecutive objects per wave and step: their G * m
// entries are one contiguous span of the output, which the wave owns.
__host__ __device__ inline uint32_t fill_group_objects(uint32_t m) {
    return std::min(kFillObjects, kFillEntries / m);  // m <= 32: at least 2
}

__global__ void __launch_bounds__(256) index_fill_kernel(const IndexEntriesArgs a) {
    __shared__ uint32_t s_prefix32[HDX_MAX_INDICES * kIndexPrefixStride / 4 + 1];
    __shared__ uint8_t s_enc[HDX_MAX_INDICES], s_plen[HDX_MAX_INDICES];
    __shared__ FillGroup s_group[4];
    uint8_t* s_prefix = reinterpret_cast<uint8_t*>(s_prefix32);
    const uint32_t m = a.m, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (uint32_t t = threadIdx.x; t < m * kIndexPrefixStride; t += blockDim.x) s_prefix[t] = a.prefix[t];
    if (threadIdx.x == 0) s_prefix32[HDX_MAX_INDICES * kIndexPrefixStride / 4] = 0;
    if (threadIdx.x < m) {
        s_enc[threadIdx.x] = a.enc[threadIdx.x];
        s_plen[threadIdx.x] = a.plen[threadIdx.x];
    }
    __syncthreads();
    if (a.entry_off[a.n * m] > a.entries_bytes) {  // the caller's buffer is too small: nothing is written
        if (blockIdx.x == 0 && threadIdx.x == 0 && a.status) atomicOr(a.status, kStatusNoMem);
        return;
    }
    FillGroup& g = s_group[w];
    const uint32_t G = fill_group_objects(m);
    const uint64_t groups = (a.n + G - 1) / G, nwaves = (uint64_t)gridDim.x * 4;
    const uintptr_t dst = (uintptr_t)a.entries;
    for (uint64_t gi = (uint64_t)blockIdx.x * 4 + w; gi < groups; gi += nwaves) {
        const uint64_t i0 = gi * G;
        const uint32_t objs = (uint32_t)std::min<uint64_t>(G, a.n - i0), E = objs * m;  // E <= 64
        wave_fence();  // the previous group's tables are done with
        if (lane < E) {
            g.eo[lane] = a.entry_off[i0 * m + lane];
            g.aoff[lane] = a.attr_off[i0 * m + lane];
            g.alen[lane] = a.attr_len[i0 * m + lane];
            g.obj[lane] = (uint8_t)(lane / m);
        }
        if (lane == 0) g.eo[E] = a.entry_off[i0 * m + E];
        if (lane < objs) {
            g.koff[lane] = a.key_off[i0 + lane];
            g.klen[lane] = a.key_len[i0 + lane];
            g.voff[lane] = a.val_off[i0 + lane];
        }
        wave_fence();
        const uint64_t s = g.eo[0], e = g.eo[E];
        if (s == e) continue;  // every object of the group is refused
        // the aligned dwords that hold bytes [dst + s, dst + e)
        const uintptr_t d0 = (dst + s) & ~(uintptr_t)3, d1 = (dst + e + 3) & ~(uintptr_t)3;
        uint32_t t = 0;  // the lane's entry: its positions only grow, so t only advances
        bool searched = false;
        for (uintptr_t addr = d0 + 4 * lane; addr < d1; addr += 256) {
            // output positions of the dword's bytes: [addr - dst, +4) clipped to [s, e)
            const uint64_t lo = addr < dst + s ? s : (uint64_t)(addr - dst);
            const uint64_t hi = std::min<uint64_t>((uint64_t)(addr + 4 - dst), e);
            const uint32_t b0 = (uint32_t)(dst + lo - addr), b1 = (uint32_t)(dst + hi - addr);  // byte lanes [b0, b1)
            if (!searched) {
                // the entry that holds the lane's first position: the last t with eo[t] <= lo
                // (s <= lo < e, so 0 <= t < E; the empty entries of refused objects are stepped over)
                for (uint32_t step = kFillEntries / 2; step; step >>= 1)
                    if (t + step < E && g.eo[t + step] <= lo) t += step;
                searched = true;
            }
            uint32_t word = 0;
            uint64_t p = lo;
            uint32_t b = b0;
            while (b < b1) {
                while (g.eo[t + 1] <= p) ++t;  // p < e = eo[E], so t < E
                const uint32_t o = g.obj[t], k = t - o * m;
                uint32_t r = (uint32_t)(p - g.eo[t]);
                const uint32_t enc = s_enc[k], plen = s_plen[k];
                const uint32_t alen = g.alen[t], klen = g.klen[o];
                const uint32_t vsz = enc_size(enc, alen), ksz = enc_size(a.key_enc, klen);
                Seg sg{};
                if (r < plen) {
                    sg.lds_prefix = s_prefix + k * kIndexPrefixStride;
                    sg.r = r;
                    sg.rem = plen - r;
                } else if ((r -= plen) < vsz) {
                    seg_encoded(sg, enc, a.vals + g.voff[o] + g.aoff[t], alen, r);
                } else if ((r -= vsz) < ksz) {
                    seg_encoded(sg, a.key_enc, a.keys + g.koff[o], klen, r);
                } else {  // pack32be(key_sz), index_primitive.cc:322-325
                    r -= ksz;
                    sg.lo = __builtin_bswap32(ksz);
                    sg.r = r;
                    sg.rem = 4 - r;
                }
                const uint32_t take = std::min(sg.rem, b1 - b);
                const uint32_t got = seg_bytes(sg, take);
                word |= (take == 4 ? got : got & ((1u << (8 * take)) - 1)) << (8 * b);
                b += take;
                p += take;
            }
            if (b0 == 0 && b1 == 4) {
                *reinterpret_cast<uint32_t*>(addr) = word;
            } else {  // a dword shared with a neighbour: only this span's bytes, no read
                for (uint32_t q = b0; q < b1; ++q) reinterpret_cast<uint8_t*>(addr)[q] = (uint8_t)(word >> (8 * q));
            }
        }
    }
}

}  // namespace

hipError_t launch_index_entries_plan(const IndexEntriesArgs& a, hipStream_t stream, bool* no_scratch) {
    *no_scratch = false;
    const uint64_t N = a.n * a.m + 1;
    const uint32_t B = a.m > 16 ? 128 : 256;  // the descriptors' LDS stays within 33 KiB
    const uint64_t blocks = (a.n + B - 1) / B;
    if (blocks > 0x7fffffffULL || (N + kIndexScanBlock - 1) / kIndexScanBlock > 0x7fffffffULL)
        return hipErrorInvalidValue;
    const uint64_t words = scan_scratch_words(N);
    PoolScratch sums;
    if (words && !sums.acquire(words * 8, stream, no_scratch)) return hipSuccess;
    hipError_t e = hipSuccess;
    if (a.n) {
        const size_t lds = (size_t)B * a.m * 8 + (size_t)B * 4 + 2 * HDX_MAX_INDICES;
        hipLaunchKernelGGL(index_plan_kernel, dim3((uint32_t)blocks), dim3(B), lds, stream, a);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = scan_exclusive(a.entry_off, N, static_cast<uint64_t*>(sums.p), stream);
    return sums.release(e);
}

hipError_t launch_index_entries_fill(const IndexEntriesArgs& a, hipStream_t stream) {
    if (a.n == 0) return hipSuccess;
    const uint64_t groups = (a.n + fill_group_objects(a.m) - 1) / fill_group_objects(a.m);
    const uint64_t blocks = std::min<uint64_t>((groups + 3) / 4, 1ull << 20);  // 4 groups per block, grid-stride
    hipLaunchKernelGGL(index_fill_kernel, dim3((uint32_t)blocks), dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace hdx
