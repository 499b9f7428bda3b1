// hdx_kernels_dbg.hip — the debug library's variant selection, built into
// libhdxhash_dbg.so only (Makefile SRCS_DBG): the process-wide forced id
// (hdxdbg_set_kernel_variant / HDX_KERNEL_VARIANT), the lookup of that id in
// each entry point's table (hdx_variants.h), the list of ids that switch a
// policy instead of a kernel, and the rows of the kernels instantiated here —
// the regroup / chunk kernels' other template forms, their debug shapes and
// the fused hash + lookup forms.  Every form writes the
// reference's coordinates (except the named debug shapes) and is
// parity-tested in tests/; none is reachable from the product library.
// Round 5 removed the retired experiments no A/B still used (occupancy caps,
// quad loads, late heads, register descriptors, grid striding, the column /
// typed / workgroup-sorted / LDS-staged / streamed kernels: variants 60-99,
// 140-191, 220-227); their results are in DESIGN.md Appendix A and
// profiles/r1-r3.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/hdxhash_debug.h"
#include "hdx_regroup.h"
#include "hdx_variants.h"

namespace hdx {

namespace {

// a kernel of the automatic policy, forced (launch_hash_batch_variant)
template <int V>
hipError_t product(const BatchArgs& args, hipStream_t stream) {
    return launch_hash_batch_variant(args, stream, V);
}

const BatchRow kBatchRows[] = {
    {12, product<12>, "the policy's chunk kernel"},
    {20, product<20>, "the policy's regroup kernel, 8 chunks unsorted"},
    {21, product<21>, "the policy's regroup kernel, 4 chunks unsorted, one wave per workgroup"},
    {25, product<25>, "the policy's regroup kernel, 16 chunks unsorted, burst stores"},
    {44, product<44>, "the policy's regroup kernel, 2 chunks class-sorted, A4 loads, ORDER 1"},
    {46, product<46>, "the policy's regroup kernel, 8 chunks class-sorted, ORDER 1, one wave per workgroup"},
    {212, product<212>, "the policy's wave-staged kernel (hdx_wstage.hip)"},
    {300, product<300>, "the wide kernel (hdx_wide.hip), at any A"},
    // alternatives for interleaved A/B (scripts/ab_variants.py), bit-exact
    {18, launch_regroup<4, true>, "regroup, 4 chunks class-sorted"},
    {19, launch_regroup<8, true>, "regroup, 8 chunks class-sorted"},
    {26, launch_regroup<2, true>, "regroup, 2 chunks class-sorted"},
    {30, launch_chunk<true, true>, "12 with the next block of the > 64-byte loop in flight (PIPE)"},
    {31, launch_chunk<true, false, 0, true>, "12 with dword-aligned loads (A4)"},
    {35, launch_regroup<2, true, true, true, true>, "26 with dword-aligned loads (A4)"},
    {37, launch_regroup<2, true, true, true, true, true>, "35 with PIPE"},
    {38, launch_regroup<2, true, true, true, true, false, true>, "35 with the class sort by LDS fetch-add (ASORT): 44 in ORDER 0"},
    {39, launch_regroup<8, true, true, true, false, false, true>, "19 with ASORT: 46 in ORDER 0, four waves per workgroup"},
    {45, launch_regroup<2, true, true, true, true, false, true, 2>, "44 in ORDER 2"},
    // one wave per workgroup (round 5)
    {260, launch_regroup<4, true, false, true, false, false, false, 0, 1>, "= 21"},
    {261, launch_regroup<16, true, false, false, false, false, false, 0, 1>, "25 with one wave per workgroup"},
    {262, launch_chunk<true, false, 0, false, 1>, "12 with one wave per workgroup"},
    {263, launch_regroup<8, true, false, true, false, false, false, 0, 1>, "20 with one wave per workgroup"},
    {264, launch_regroup<8, true, true, true, false, false, true, 1, 1>, "= 46"},
    {265, launch_regroup<2, true, true, true, true, false, true, 1, 1>, "44 with one wave per workgroup"},
    // deferred strings (round 5, hash_regroup_defer_kernel)
    {280, launch_regroup_defer<4, true, false, 1>, "21 with the string slots deferred to passes of their own, first"},
    {281, launch_regroup_defer<4, false, false, 1>, "280 with cached stores"},
    {282, launch_regroup_defer<4, true, false, 2>, "280 with the strings last"},
    {283, launch_regroup_defer<8, true, false, 1>, "280 with 8 chunks"},
    {284, launch_regroup_defer<4, true, true, 1>, "280 with A4 loads"},
    {285, launch_regroup_defer<4, false, false, 2>, "282 with cached stores"},
    {286, launch_regroup_defer<8, false, false, 1>, "283 with cached stores"},
    // debug shapes: WRONG coordinates
    {40, launch_chunk<true, false, 1>, "debug shape of 12: loads only (WRONG coordinates)"},
    {41, launch_chunk<true, false, 2>, "debug shape of 12: arithmetic only (WRONG coordinates)"},
};

// hash + lookup_region in one launch (hdx_hash_batch_regions_device, A <= 128):
// launch_regroup_regions' C chunks, SORT, A4, ASORT, ORDER, UNI (the tables
// looked up in a wave-uniform loop, else a lane per (table, object) pair);
// LDS off: the tables stay in global memory
template <int C, bool SORT, bool A4, bool ASORT, int ORDER, bool UNI, bool LDS = true>
hipError_t fused(const BatchArgs& args, hipStream_t stream) {
    return launch_regroup_regions<C, SORT, A4, ASORT, ORDER, UNI>(args, stream, LDS);
}
const BatchRow kBatchRegionsRows[] = {
    {100, fused<4, false, false, false, 0, false>, "4 chunks unsorted, a lane per pair"},
    {101, fused<4, false, false, false, 0, true>, "100 with UNI"},
    {102, fused<2, false, false, false, 0, true>, "101 with 2 chunks"},
    {103, fused<8, false, false, false, 0, true>, "101 with 8 chunks"},
    {104, fused<4, false, false, false, 0, true, false>, "101 with the tables in global memory"},
    {105, fused<3, true, true, true, 1, false>, "3 chunks class-sorted (ORDER 1), A4 loads, a lane per pair"},
    {106, fused<3, true, true, true, 1, true>, "105 with UNI"},
    {107, fused<2, true, true, true, 1, true>, "106 with 2 chunks"},
    {108, fused<8, false, false, false, 0, false>, "100 with 8 chunks"},
    {109, fused<8, false, false, false, 0, true>, "101 with 8 chunks (= 103)"},
    {110, fused<1, false, false, false, 0, true>, "101 with 1 chunk"},
    {111, fused<4, true, true, true, 1, true>, "106 with 4 chunks"},
    {217, launch_hash_wstage_regions, "the wave-staged kernel with the fused region lookup, at any n"},
};

// Ids that switch a policy where hash_variant() is compared with them, and
// select no kernel of their own.
struct PolicyRow {
    int id;
    const char* note;
};
const PolicyRow kPolicyVariants[] = {
    {-1, "the automatic policy everywhere"},
    {47, "with region tables: the gather sweep's fused form with 64 objects per wave (hdx_encoded.hip)"},
    {233, "stored objects + regions: the wave-staged sweep with the lookup fused (hdx_encoded.hip)"},
    {234, "stored objects + regions: the gather sweep's fused form at any n (hdx_encoded.hip)"},
    {235, "regions by hash + separate lookups at any n, 64 MiB chunks (hdx_regions.hip)"},
    {247, "235 with the scratch allocation failing: the fused fallback (hdx_regions.hip)"},
    {300, "the wide kernel at any A: the classes also in device memory (set_codes, hdx_capi.cpp)"},
    {301, "the wide sweep at any A (hdx_encoded.hip; set_codes, hdx_capi.cpp)"},
};

template <class Args>
const VariantRow<Args>* find_in(int id, VariantRows<Args> a, VariantRows<Args> b) {
    const VariantRow<Args>* r = a.find(id);
    return r ? r : b.find(id);
}

}  // namespace

VariantRows<BatchArgs> regroup_variant_rows() { return kBatchRows; }
VariantRows<BatchArgs> batch_regions_variant_rows() { return kBatchRegionsRows; }

const BatchRow* batch_variant(int id) { return find_in(id, regroup_variant_rows(), wstage_variant_rows()); }
const BatchRow* batch_regions_variant(int id) { return batch_regions_variant_rows().find(id); }
const SweepRow* sweep_variant(int id) { return find_in(id, gather_sweep_variant_rows(), wsweep_variant_rows()); }
const SweepRow* wide_sweep_variant(int id) { return find_in(id, wide_two_variant_rows(), wide_sweep_variant_rows()); }

// Where the id selects something (hdxdbg_variant_entries); -2: nowhere, unknown.
int variant_entries(int id) {
    int mask = 0;
    if (batch_variant(id)) mask |= HDXDBG_ENTRY_BATCH;
    if (batch_regions_variant(id)) mask |= HDXDBG_ENTRY_BATCH_REGIONS;
    if (sweep_variant(id)) mask |= HDXDBG_ENTRY_SWEEP;
    if (wide_sweep_variant(id)) mask |= HDXDBG_ENTRY_WIDE_SWEEP;
    for (const PolicyRow& p : kPolicyVariants)
        if (p.id == id) mask |= HDXDBG_ENTRY_POLICY;
    return mask ? mask : -2;
}

static int g_variant = [] {
    const char* e = getenv("HDX_KERNEL_VARIANT");
    return e && *e && variant_entries(atoi(e)) != -2 ? atoi(e) : -1;
}();

int hash_variant() { return __atomic_load_n(&g_variant, __ATOMIC_RELAXED); }

int set_hash_variant(int v) {
    if (variant_entries(v) == -2) return -2;
    return __atomic_exchange_n(&g_variant, v, __ATOMIC_RELAXED);
}

}  // namespace hdx
