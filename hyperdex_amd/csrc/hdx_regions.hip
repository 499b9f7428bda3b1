// hdx_regions.hip — coordinates -> region ids on gfx950.
//
// configuration::lookup_region (common/configuration.cc:698-735): the first
// region r of a subspace whose box holds the object's coordinates,
//   lower[r][a] <= hs[attrs[a]] <= upper[r][a]   for every subspace dimension a,
// else region_id() (0).  point_leader (:427-497) is the same lookup on subspace
// 0 (attrs = {0}).  One lane per object; the region table is staged in LDS
// once per workgroup and every lane walks it in the reference's order, so the
// table reads are LDS broadcasts.  The region boxes come from
// admin/partition.cc and are taken as input (coordinator-assigned ids,
// coordinator/coordinator.cc:586-596), never recomputed here.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "hdx_internal.h"
#include "hdx_region_lookup.h"

#ifndef HDX_DEBUG_BUILD
#define HDX_DEBUG_BUILD 0
#endif

namespace hdx {

// The interval index (region_index_build) is built on the host: hdx_region_index.h.

template <bool IN_LDS, bool INDEX = false>
__global__ void __launch_bounds__(256)
lookup_region_kernel(const RegionArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint64_t smem[];
    const RegionView& t = a.t;
    const uint64_t* lower = t.lower;
    const uint64_t* upper = t.upper;
    const uint64_t* ids = t.ids;
    const uint64_t* index = t.index;
    if (IN_LDS) {  // an indexed table stages its index and ids, a scanned one its boxes and ids
        if (INDEX) {
            for (uint32_t k = threadIdx.x; k < t.index_words; k += blockDim.x) smem[k] = t.index[k];
            for (uint32_t k = threadIdx.x; k < t.R; k += blockDim.x) smem[t.index_words + k] = t.ids[k];
            index = smem;
            ids = smem + t.index_words;
        } else {
            const uint32_t box = t.R * t.D;
            for (uint32_t k = threadIdx.x; k < box; k += blockDim.x) {
                smem[k] = t.lower[k];
                smem[box + k] = t.upper[k];
            }
            for (uint32_t k = threadIdx.x; k < t.R; k += blockDim.x) smem[2 * box + k] = t.ids[k];
            lower = smem;
            upper = smem + box;
            ids = smem + 2 * box;
        }
        __syncthreads();
    }
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    uint64_t h[kMaxLookupDims];
    const uint64_t* row = a.coords + i * a.A;
#pragma unroll
    for (uint32_t d = 0; d < kMaxLookupDims; ++d)
        if (d < t.D) h[d] = row[t.attrs[d]];
    a.out[i] = INDEX ? lookup_indexed(index, t.W, t.D, h, ids) : lookup_scan(lower, upper, ids, t.R, t.D, h);
}

hipError_t launch_lookup_region(const RegionArgs& a, hipStream_t stream) {
    if (a.n == 0) return hipSuccess;
    const uint64_t blocks = (a.n + 255) / 256;
    if (blocks > 0x7fffffffULL) return hipErrorInvalidValue;
    const RegionView& t = a.t;
    if (t.index) {
        const size_t lds = ((size_t)t.index_words + t.R) * 8;
        if (lds <= 48 * 1024)
            hipLaunchKernelGGL((lookup_region_kernel<true, true>), dim3((uint32_t)blocks), dim3(256), lds, stream, a);
        else
            hipLaunchKernelGGL((lookup_region_kernel<false, true>), dim3((uint32_t)blocks), dim3(256), 0, stream, a);
        return hipGetLastError();
    }
    const size_t lds = (size_t)t.R * t.D * 16 + (size_t)t.R * 8;
    if (lds <= 48 * 1024) {
        hipLaunchKernelGGL(lookup_region_kernel<true>, dim3((uint32_t)blocks), dim3(256), lds, stream, a);
    } else {
        hipLaunchKernelGGL(lookup_region_kernel<false>, dim3((uint32_t)blocks), dim3(256), 0, stream, a);
    }
    return hipGetLastError();
}

bool regions_by_lookup_pays(uint64_t n) {
#if HDX_DEBUG_BUILD
    if (hash_variant() == 235 || hash_variant() == 247) return true;
#endif
    return n >= kRegionLookupMinObjects;
}

uint64_t regions_chunk_objects(uint64_t n, uint32_t A) {
    uint64_t bytes = kRegionChunkBytes;
#if HDX_DEBUG_BUILD
    if (hash_variant() == 235 || hash_variant() == 247) bytes = 64ull << 20;  // tests: several chunks at small n
#endif
    return std::min<uint64_t>(n, std::max<uint64_t>(1, bytes / (8ull * A)));
}

// The coordinate chunks are scratch from the library's pool (PoolScratch,
// hdx_scratch.hip).
hipError_t regions_by_lookup(uint64_t n, uint32_t A, const SweepTable* t, uint32_t T, uint64_t* coords,
                             const RegionHashFn& hash, hipStream_t stream, bool* no_scratch) {
    *no_scratch = false;
    if (n == 0) return hipSuccess;
    const uint64_t chunk = coords ? n : regions_chunk_objects(n, A);
    PoolScratch scratch;
    if (!coords) {
        // on failure nothing is launched yet: the caller runs its fused form,
        // which needs no scratch (no new out-of-memory failure)
        bool have = scratch.acquire(chunk * A * 8, stream, no_scratch);
#if HDX_DEBUG_BUILD
        if (have && hash_variant() == 247) {  // tests: the allocation "fails"
            (void)scratch.release(hipSuccess);
            *no_scratch = true;
            have = false;
        }
#endif
        if (!have) return hipSuccess;
    }
    hipError_t e = hipSuccess;
    for (uint64_t first = 0; first < n && e == hipSuccess; first += chunk) {
        const uint64_t count = std::min(chunk, n - first);
        uint64_t* c = coords ? coords + first * A : static_cast<uint64_t*>(scratch.p);
        if ((e = hash(first, count, c)) != hipSuccess) break;
        for (uint32_t k = 0; k < T && e == hipSuccess; ++k) {
            e = launch_lookup_region(RegionArgs{t[k], c, t[k].out + first, count, A}, stream);
        }
    }
    return scratch.release(e);
}

// One lane per (table, object): small batches from the daemon shim, where a
// launch per table would cost more than the lookups.  Every table's boxes
// and ids are staged in LDS per workgroup (the walk is then LDS broadcasts,
// as in lookup_region_kernel); tables too large for that are walked in global
// memory.
// A table with an interval index stages the index (in the lower slot) and its
// ids; one without stages its boxes and ids.
struct MultiLayout {
    uint32_t lower[kMaxMultiTables], upper[kMaxMultiTables], ids[kMaxMultiTables];  // u64 offsets
    uint32_t words;
};

__host__ __device__ inline MultiLayout multi_layout(const MultiRegionArgs& a) {
    MultiLayout l{};
    uint32_t w = 0;
    for (uint32_t t = 0; t < a.T; ++t) {
        const uint32_t box = a.t[t].index ? a.t[t].index_words : a.t[t].R * a.t[t].D;
        l.lower[t] = w;
        l.upper[t] = w + box;
        l.ids[t] = a.t[t].index ? w + box : w + 2 * box;
        w = l.ids[t] + a.t[t].R;
    }
    l.words = w;
    return l;
}

template <bool IN_LDS>
__global__ void __launch_bounds__(256) lookup_regions_multi_kernel(const MultiRegionArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint64_t smem[];
    const MultiLayout l = multi_layout(a);
    if (IN_LDS) {
        for (uint32_t t = 0; t < a.T; ++t) {
            if (a.t[t].index) {
                for (uint32_t k = threadIdx.x; k < a.t[t].index_words; k += blockDim.x)
                    smem[l.lower[t] + k] = a.t[t].index[k];
            } else {
                const uint32_t box = a.t[t].R * a.t[t].D;
                for (uint32_t k = threadIdx.x; k < box; k += blockDim.x) {
                    smem[l.lower[t] + k] = a.t[t].lower[k];
                    smem[l.upper[t] + k] = a.t[t].upper[k];
                }
            }
            for (uint32_t k = threadIdx.x; k < a.t[t].R; k += blockDim.x) smem[l.ids[t] + k] = a.t[t].ids[k];
        }
        __syncthreads();
    }
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t t = g / a.n, i = g - t * a.n;
    if (t >= a.T) return;
    const RegionView& tb = a.t[t];
    const uint64_t* lower = IN_LDS ? smem + l.lower[t] : tb.lower;
    const uint64_t* upper = IN_LDS ? smem + l.upper[t] : tb.upper;
    const uint64_t* ids = IN_LDS ? smem + l.ids[t] : tb.ids;
    const uint64_t* row = a.coords + i * a.A;
    uint64_t h[kMaxLookupDims];
#pragma unroll
    for (uint32_t d = 0; d < kMaxLookupDims; ++d)
        if (d < tb.D) h[d] = row[tb.attrs[d]];
    if (tb.index) {
        a.out[t * a.out_stride + i] = lookup_indexed(IN_LDS ? smem + l.lower[t] : tb.index, tb.W, tb.D, h, ids);
        return;
    }
    a.out[t * a.out_stride + i] = lookup_scan(lower, upper, ids, tb.R, tb.D, h);
}

hipError_t launch_lookup_regions_multi(const MultiRegionArgs& a, hipStream_t stream) {
    const uint64_t work = a.n * a.T;
    if (work == 0) return hipSuccess;
    const uint64_t blocks = (work + 255) / 256;
    if (blocks > 0x7fffffffULL) return hipErrorInvalidValue;
    const size_t lds = (size_t)multi_layout(a).words * 8;
    if (lds <= 48 * 1024)
        hipLaunchKernelGGL(lookup_regions_multi_kernel<true>, dim3((uint32_t)blocks), dim3(256), lds, stream, a);
    else
        hipLaunchKernelGGL(lookup_regions_multi_kernel<false>, dim3((uint32_t)blocks), dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace hdx
