// hdx_variants.h — the debug library's kernel-variant tables (libhdxhash_dbg.so
// only; the product library has no kernel selection).  A forced id
// (hdxdbg_set_kernel_variant / HDX_KERNEL_VARIANT) selects a kernel at each
// entry point whose table has a row for it — id, launcher, note — and leaves
// the others' automatic policy alone; one id may have rows at several (270:
// the batch kernel and the sweep in the XCD-aware block order).  A table is
// the rows of the files that instantiate its kernels.  Ids that switch a
// policy instead are kPolicyVariants (hdx_kernels_dbg.hip).
#pragma once

#include <stddef.h>

#include "hdx_internal.h"

namespace hdx {

template <class Args>
struct VariantRow {
    int id;
    hipError_t (*launch)(const Args&, hipStream_t);
    const char* note;
};
template <class Args>
struct VariantRows {
    const VariantRow<Args>* rows;
    size_t n;
    template <size_t N>
    constexpr VariantRows(const VariantRow<Args> (&r)[N]) : rows(r), n(N) {}
    const VariantRow<Args>* find(int id) const {
        for (size_t i = 0; i < n; ++i)
            if (rows[i].id == id) return &rows[i];
        return nullptr;
    }
};
using BatchRow = VariantRow<BatchArgs>;
using SweepRow = VariantRow<EncodedArgs>;

VariantRows<BatchArgs> regroup_variant_rows();        // hdx_kernels_dbg.hip: batch hash
VariantRows<BatchArgs> wstage_variant_rows();         // hdx_wstage_dbg.hip: batch hash
VariantRows<BatchArgs> batch_regions_variant_rows();  // hdx_kernels_dbg.hip: batch hash + regions
VariantRows<EncodedArgs> gather_sweep_variant_rows(); // hdx_encoded.hip: stored-object sweep
VariantRows<EncodedArgs> wsweep_variant_rows();       // hdx_wsweep_dbg.hip: stored-object sweep
VariantRows<EncodedArgs> wide_two_variant_rows();     // hdx_wide.hip: wide sweep
VariantRows<EncodedArgs> wide_sweep_variant_rows();   // hdx_wide_dbg.hip: wide sweep

// The forced id's row at an entry point, or NULL (hdx_kernels_dbg.hip); the
// HDXDBG_ENTRY_* mask of where it has one (include/hdxhash_debug.h), -2 if unknown.
const BatchRow* batch_variant(int id);
const BatchRow* batch_regions_variant(int id);
const SweepRow* sweep_variant(int id);
const SweepRow* wide_sweep_variant(int id);
int variant_entries(int id);

}  // namespace hdx
