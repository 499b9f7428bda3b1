// hdx_region_lookup.h — configuration::lookup_region's first-match test
// (common/configuration.cc:698-735) as device functions, one copy of each step
// for every kernel that looks regions up (hdx_regions.hip, hdx_regroup.h,
// hdx_encoded.hip, hdx_wstage.h, hdx_wsweep.h): the indexed lookup (over
// index_interval, hdx_region_index.h), the scan, the choice between them for
// one table (lookup_table), a wave's tables at once (lookup_tables_wave), and
// the LDS copies of indexed tables that the fused gather forms keep per
// workgroup (place_tables on the host, stage_tables on the device).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hdx_internal.h"
#include "hdx_region_index.h"

namespace hdx {

// Region id of coordinates hd(0..D) through the interval index idx (hd reads
// one coordinate, so a caller holding them in LDS need not copy them out).
template <class HD>
__device__ __forceinline__ uint64_t lookup_indexed_fn(const uint64_t* idx, uint32_t W, uint32_t D, HD hd,
                                                      const uint64_t* ids) {
    uint64_t acc[4] = {~0ull, ~0ull, ~0ull, ~0ull};
#pragma unroll
    for (uint32_t d = 0; d < kMaxLookupDims; ++d) {
        if (d >= D) break;
        const uint64_t* mask = index_interval(idx, W, d, hd(d));
#pragma unroll
        for (uint32_t w = 0; w < 4; ++w)
            if (w < W) acc[w] &= mask[w];
    }
#pragma unroll
    for (uint32_t w = 0; w < 4; ++w)
        if (w < W && acc[w]) return ids[64 * w + __builtin_ctzll(acc[w])];
    return 0;  // region_id()
}

__device__ __forceinline__ uint64_t lookup_indexed(const uint64_t* idx, uint32_t W, uint32_t D, const uint64_t* h,
                                                   const uint64_t* ids) {
    return lookup_indexed_fn(idx, W, D, [h](uint32_t d) { return h[d]; }, ids);
}

// The reference's scan: the first region whose box holds h on every dimension.
__device__ __forceinline__ uint64_t lookup_scan(const uint64_t* lower, const uint64_t* upper, const uint64_t* ids,
                                                uint32_t R, uint32_t D, const uint64_t (&h)[kMaxLookupDims]) {
    uint64_t rid = 0;  // region_id()
    for (uint32_t r = 0; r < R; ++r) {
        bool match = true;
#pragma unroll
        for (uint32_t d = 0; d < kMaxLookupDims; ++d)
            if (d < D) match &= lower[r * D + d] <= h[d] && h[d] <= upper[r * D + d];
        if (match) {
            rid = ids[r];
            break;
        }
    }
    return rid;
}

// ---- indexed tables copied into LDS, once per workgroup ---------------------
// place_tables (host) gives each indexed table of tabs[0..T) a place (lds_index
// / lds_ids, u64 offsets) while `stage` holds and index + ids of all placed
// tables fit in kStagedTableBytes, else kNotStaged; it returns the u64 words
// of dynamic LDS the launch adds for them.  stage_tables (the whole workgroup,
// before any wave may leave: it ends in the kernel's only barrier) copies them
// to tbl, that LDS area (the stored-object sweep; the packed batches' fused
// kernel keeps the same loop written out, hdx_regroup.h says why).
constexpr uint32_t kNotStaged = 0xffffffffu;
constexpr uint32_t kStagedTableBytes = 16384;

inline uint32_t place_tables(SweepTable* tabs, uint32_t T, bool stage) {
    uint32_t words = 0;
    for (uint32_t t = 0; t < T; ++t) {
        SweepTable& tb = tabs[t];
        tb.lds_index = tb.lds_ids = kNotStaged;
        const uint32_t need = tb.index_words + tb.R;
        if (stage && tb.index && (words + need) * 8 <= kStagedTableBytes) {
            tb.lds_index = words;
            tb.lds_ids = words + tb.index_words;
            words += (need + 1) & ~1u;  // keep 16-byte alignment
        }
    }
    return words;
}

__device__ __forceinline__ void stage_tables(const SweepTable* tabs, uint32_t T, uint64_t* tbl) {
    for (uint32_t t = 0; t < T; ++t) {
        // the table's fields by value: read once, not again after every store
        const uint32_t at_index = tabs[t].lds_index, at_ids = tabs[t].lds_ids;
        const uint32_t words = tabs[t].index_words, R = tabs[t].R;
        const uint64_t* index = tabs[t].index;
        const uint64_t* ids = tabs[t].ids;
        if (at_index == kNotStaged) continue;
        for (uint32_t k = threadIdx.x; k < words; k += blockDim.x) tbl[at_index + k] = index[k];
        for (uint32_t k = threadIdx.x; k < R; k += blockDim.x) tbl[at_ids + k] = ids[k];
    }
    __syncthreads();
}

// Table tb's region id of the coordinates hd(0..D): through its index's LDS
// copy when tbl (stage_tables' area) holds one, else through the index in
// global memory, else the scan.  STAGED false: a launch that staged nothing
// and never ran place_tables — tbl and lds_index are then not read.  Not
// __forceinline__: the fused gather kernels compile to the hand-written
// choice's code only when the inliner places it in its own order.
template <bool STAGED, class HD>
__device__ inline uint64_t lookup_table(const SweepTable& tb, const uint64_t* tbl, HD hd) {
    if (STAGED && tb.lds_index != kNotStaged)
        return lookup_indexed_fn(tbl + tb.lds_index, tb.W, tb.D, hd, tbl + tb.lds_ids);
    if (tb.index) return lookup_indexed_fn(tb.index, tb.W, tb.D, hd, tb.ids);
    uint64_t h[kMaxLookupDims];
#pragma unroll
    for (uint32_t d = 0; d < kMaxLookupDims; ++d)
        if (d < tb.D) h[d] = hd(d);
    return lookup_scan(tb.lower, tb.upper, tb.ids, tb.R, tb.D, h);
}

// configuration::lookup_region for a wave's nobj objects whose coordinates are
// parked in LDS (coords[o * A + j]), every table of tabs[0..T): indexed tables
// with one lane per (object, table dimension) — each searches its interval
// and parks the mask words in the scratch (LDS, nobj * sum(D) * 32 bytes) —
// then one lane per (object, table) ANDs them: a few dependent round trips
// for all the tables instead of ~3 per dimension one after another.  Scanned
// tables, or more than 64 searches: lane = object, table by table.  Region
// ids go to tabs[t].out[o0 + o].  The whole wave calls it.  Its callers (the
// wave-staged forms) never place tables in LDS and leave lds_index unset, so
// the table-by-table arm calls lookup_table<false>: no staging area is read.
template <class FENCE>
__device__ __forceinline__ void lookup_tables_wave(const SweepTable* tabs, uint32_t T, const uint64_t* coords,
                                                   uint32_t A, uint32_t nobj, uint64_t o0, uint64_t* scratch,
                                                   FENCE fence) {
    const uint32_t lane = threadIdx.x & 63;
    uint32_t P = 0;
    bool all_indexed = true;
    for (uint32_t t = 0; t < T; ++t) {
        P += tabs[t].D;
        all_indexed &= tabs[t].index != nullptr;
    }
    if (all_indexed && nobj * P <= 64) {
        if (lane < nobj * P) {
            const uint32_t o = lane / P, p = lane - o * P;
            uint32_t t = 0, d = p;
            while (d >= tabs[t].D) d -= tabs[t++].D;
            const SweepTable& tb = tabs[t];
            const uint64_t* mask = index_interval(tb.index, tb.W, d, coords[o * A + tb.attrs[d]]);
#pragma unroll
            for (uint32_t w = 0; w < 4; ++w) scratch[(o * P + p) * 4 + w] = w < tb.W ? mask[w] : 0;
        }
        fence();
        if (lane < nobj * T) {
            const uint32_t o = lane / T, t = lane - o * T;
            uint32_t p0 = 0;
            for (uint32_t u = 0; u < t; ++u) p0 += tabs[u].D;
            const SweepTable& tb = tabs[t];
            uint64_t acc[4] = {~0ull, ~0ull, ~0ull, ~0ull};
            for (uint32_t d = 0; d < tb.D; ++d)
#pragma unroll
                for (uint32_t w = 0; w < 4; ++w) acc[w] &= scratch[(o * P + p0 + d) * 4 + w];
            uint64_t r = 0;
#pragma unroll
            for (int w = 3; w >= 0; --w)  // descending: the lowest word with a bit wins (first match)
                if ((uint32_t)w < tb.W && acc[w]) r = tb.ids[64 * w + __builtin_ctzll(acc[w])];
            tb.out[o0 + o] = r;
        }
    } else if (lane < nobj) {
        const uint64_t* po = coords + lane * A;
        for (uint32_t t = 0; t < T; ++t) {
            const SweepTable& tb = tabs[t];
            tb.out[o0 + lane] = lookup_table<false>(tb, nullptr, [&](uint32_t d) { return po[tb.attrs[d]]; });
        }
    }
}

}  // namespace hdx
