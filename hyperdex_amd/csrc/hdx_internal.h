// hdx_internal.h — declarations shared by the kernels and the C-ABI layer.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <functional>
#include <vector>

#include "../../include/hdxhash.h"
#include "hdx_host_common.h"
#include "hdx_region_index.h"

namespace hdx {


// Kernel arguments, passed by value (kernarg segment).  codes[] holds the
// per-attribute dispatch class (hdx_device_hash.h CODE_*) for schemas of up
// to kKernargCodes attributes; wider schemas (up to HDX_MAX_ATTRS, the
// reference's u16 attrs_sz) run the wide kernels (hdx_wide.hip), which read
// the classes from codes_dev, a device copy (device_codes, hdx_capi.cpp).
constexpr uint32_t kKernargCodes = 256;
constexpr uint32_t kMaxSweepTables = 4;
constexpr uint32_t kWavePlanSlots = 128;  // BatchArgs::plan: two 64-slot passes
// A table of a fused launch: the view (RegionView, hdx_region_index.h), where
// its region ids go, and where the workgroup's LDS copy of an indexed table
// lies (place_tables, hdx_region_lookup.h; only the gather forms set them).
struct SweepTable : RegionView {
    uint64_t* out;
    uint32_t lds_index, lds_ids;  // u64 offsets, kNotStaged: none
};
static_assert(sizeof(RegionView) == 80 && sizeof(SweepTable) == 96, "kernel argument layout");

struct BatchArgs {
    const uint8_t* blob;
    const uint64_t* obj_base;
    const uint32_t* attr_len;
    uint64_t* coords;
    uint32_t* status;
    uint64_t n;
    uint32_t A;
    uint32_t uniform_code;  // the code every attribute shares, or 0xff if mixed
    double inv_A;           // 1.0 / A                       (finalize_args)
    uint32_t a_magic;       // ceil(2^31 / A): t / A == (t * a_magic) >> 31 for t * A < 2^31
    uint32_t pad_;
    const uint8_t* codes_dev;  // A > 128: the classes in device memory (the wide kernels)
    uint8_t codes[kKernargCodes];
    // fused region lookup (hash_regroup_regions_kernel): T tables, K whole
    // objects per wave, lds_tables u64 words of LDS table copies per workgroup
    uint32_t T, K, lds_tables;
    SweepTable t[kMaxSweepTables];
    // The wave-staged kernel's slot plan (hdx_wstage.h, PLAN; filled by its
    // launcher): every wave holds K objects of the same schema, so slot s of
    // any wave is attribute s % A of object s / A — j | o << 8 | code << 16,
    // code CODE_ZERO past the K objects.  Replaces per-slot division and the
    // code-table shuffle on the device.
    uint32_t plan[kWavePlanSlots];
};
static_assert(sizeof(BatchArgs) == 1248, "kernel argument layout");

hipError_t launch_hash_batch(const BatchArgs& args, hipStream_t stream);
// Wave-staged hash (hdx_wstage.hip): K whole objects per wave copied into an
// LDS window by DMA and hashed from LDS.  The product form: two passes per
// wave, head/tail hashing; A <= 128 (else hipErrorInvalidValue).
hipError_t launch_hash_wstage_product(const BatchArgs& args, hipStream_t stream);
hipError_t launch_hash_wstage_regions(const BatchArgs& args, hipStream_t stream);  // + args.T tables
// What a wave of the product's wave-staged forms holds for a schema of A
// attributes (hdxdbg_wave_geometry, include/hdxhash_debug.h): from the
// constants their launches use (hdx_wstage.hip, hdx_wsweep.hip).
struct WaveGeometry {
    uint32_t objects, window, key_region, front_pad, back_pad, passes, object_cap;
};
void wstage_product_geometry(uint32_t A, WaveGeometry& g);
void wsweep_product_geometry(uint32_t A, WaveGeometry& g);
// hash + lookup_region (args.T tables in args.t): one fused launch for A <=
// 128 below kRegionLookupMinObjects, else the hash and one lookup launch per
// table (hipErrorOutOfMemory when A > 128, coords is NULL and no scratch can
// be allocated)
hipError_t launch_hash_batch_regions(const BatchArgs& args, hipStream_t stream);
// The wide kernels (hdx_wide.hip): any A (args.codes_dev set).  Packed
// batches (the policy takes them for A > kKernargCodes) and stored objects
// (A > kWsweepMaxAttrs; coords != NULL).
hipError_t launch_hash_wide(const BatchArgs& args, hipStream_t stream);
struct EncodedArgs;
hipError_t launch_hash_sweep_wide(const EncodedArgs& a, hipStream_t stream);
// Fills args.uniform_code from args.codes[0..A), and inv_A / a_magic from A.
void finalize_args(BatchArgs& args);
// The automatic policy's kernels by variant id (hdx_kernels.hip,
// variant_kernel_name); any other id is hipErrorInvalidValue.
hipError_t launch_hash_batch_variant(const BatchArgs& args, hipStream_t stream, int variant);
// The forced variant: -1 (the automatic policy) in the product library;
// libhdxhash_dbg.so (HDX_DEBUG_BUILD) adds a process-wide selection, looked up
// in each entry point's variant table (hdx_variants.h).
int hash_variant();
int set_hash_variant(int v);  // debug build only: -2 if unknown, else the previous selection
// The variant launch_hash_batch would run for args, and its kernel's symbol.
int chosen_variant(const BatchArgs& args);
const char* variant_kernel_name(int v);

// Region lookup (hdx_regions.hip) of n coordinate rows in one table: t's
// arrays are device memory owned by an hdx_region_table handle (region_view,
// hdx_host.h).
struct RegionArgs {
    RegionView t;
    const uint64_t* coords;  // [n*A]
    uint64_t* out;           // [n]
    uint64_t n;
    uint32_t A;
};

hipError_t launch_lookup_region(const RegionArgs& a, hipStream_t stream);

// Region ids by hash + one lookup launch per table instead of a fused kernel
// (hdx_regions.hip), for the VALU-bound hash kernels whose fused epilogue
// costs more than the coordinates' round trip through HBM — from
// kRegionLookupMinObjects objects (below, the one launch of the fused form
// wins: the daemon shim's batches).  hash(first, count, c) hashes objects
// [first, first + count) into c.  With coords, all n objects are hashed there
// first; without, chunks of at most kRegionChunkBytes of coordinates go
// through a stream-ordered scratch buffer (hipMallocAsync; each chunk pays a
// launch tail of ~0.01 ms: config 3b 4.59 / 3.72 / 3.52 ms with 16 / 64 /
// 256 MiB chunks, 3.47 unchunked, profiles/r3/ab_regions_by_lookup.jsonl).
// If that scratch cannot be allocated nothing is launched and *no_scratch is
// set: the caller then runs its fused form, which needs none.
// Debug variant 235: by lookup at any n, 64 MiB chunks (tests); 247: the
// same with the scratch allocation failing (the fallback).
using RegionHashFn = std::function<hipError_t(uint64_t first, uint64_t count, uint64_t* coords)>;
constexpr uint64_t kRegionChunkBytes = 2ull << 30;
constexpr uint64_t kRegionLookupMinObjects = 1ull << 20;
bool regions_by_lookup_pays(uint64_t n);
uint64_t regions_chunk_objects(uint64_t n, uint32_t A);
hipError_t regions_by_lookup(uint64_t n, uint32_t A, const SweepTable* t, uint32_t T, uint64_t* coords,
                             const RegionHashFn& hash, hipStream_t stream, bool* no_scratch);

// Several subspaces at once (the batcher's prev/this/next lookups): table t's
// region ids for object i go to out[t * out_stride + i].
constexpr uint32_t kMaxMultiTables = 16;
struct MultiRegionArgs {
    const uint64_t* coords;  // [n*A]
    uint64_t* out;
    uint64_t n, out_stride;
    uint32_t A, T;
    RegionView t[kMaxMultiTables];
};

hipError_t launch_lookup_regions_multi(const MultiRegionArgs& a, hipStream_t stream);

// Host: the interval index of a region table, hdx_region_index.h.

// The stored-object stages' arguments begin with the objects themselves (StoredObjects,
// hdx_host_common.h, which also says which columns each stage reads); the host sets them
// with one assignment, static_cast<StoredObjects&>(a) = so.
//
// Stored-object sweep (hdx_encoded.hip): device arrays.  T region tables
// (hdx_hash_encoded_regions_device): table t's region id of object i goes to
// t[t].out[i]; coords may then be NULL.
struct EncodedArgs : StoredObjects {
    uint64_t* coords;
    uint64_t* versions;  // may be NULL
    uint32_t* status;    // may be NULL
    uint64_t n;
    uint32_t A;
    uint32_t a_magic;  // ceil(2^31 / A) (launch_hash_encoded fills it)
    uint32_t T, lds_tables;  // lds_tables: u64 words of the workgroup's table copies
    SweepTable t[kMaxSweepTables];
    const uint8_t* codes_dev;  // A > 128: the classes in device memory (the wide sweep)
    uint8_t codes[kKernargCodes];
    // numeric walk (launch_hash_encoded fills them): the attributes left to the
    // hash passes — the key and every STRING value attribute — in order
    uint8_t p2[kKernargCodes];
    uint32_t S, s_magic;  // how many; ceil(2^31 / S)
};
static_assert(sizeof(EncodedArgs) == 1008, "kernel argument layout");

hipError_t launch_hash_encoded(const EncodedArgs& a, hipStream_t stream);
// hdx_gather.hip: n extents [src + src_off[i], +len[i]) written back to back at
// dst + dst_off[i] (src: device view of pinned host memory, or device memory;
// destination extents must not overlap).
hipError_t launch_gather_extents(const uint8_t* src, const uint64_t* src_off, const uint32_t* len,
                                 const uint64_t* dst_off, uint8_t* dst, uint64_t n, hipStream_t stream);
// hdx_gather.hip: up to 8 contiguous copies of whole dwords (src: device
// views of pinned host memory, or device memory) by a kernel on `stream`.
hipError_t launch_copy_linear(const void* const* src, void* const* dst, const uint64_t* bytes, uint32_t count,
                              hipStream_t stream);
// The wave-staged sweep (hdx_wsweep.h): K objects per wave, keys and values
// copied into LDS by DMA, the walk and the hashing from LDS; coords != NULL,
// A <= 64 * passes (else hipErrorInvalidValue).  The product form.
constexpr uint32_t kWsweepMaxAttrs = 128;
hipError_t launch_hash_wsweep_product(const EncodedArgs& a, hipStream_t stream);
// HBM streaming probe (hdx_synth.hip): read `bytes` (write = 1: plus one
// 8-byte store per 64 bytes read into sink[bytes / 64]).
hipError_t launch_stream_probe(const uint8_t* src, uint64_t bytes, uint64_t* sink, int write, hipStream_t s);

// Index-key encoding (hdx_index.hip): n values of one INT64 / FLOAT /
// TIMESTAMP_* attribute at blob + off[i], len[i] bytes; out holds n entries
// of 8 B (16 B for CODE_FLOAT).
struct IndexArgs {
    const uint8_t* blob;
    const uint64_t* off;
    const uint32_t* len;
    uint8_t* out;
    uint32_t* status;  // may be NULL
    uint64_t n;
    uint32_t code;     // CODE_INT64 or CODE_FLOAT (timestamps encode as int64)
};

hipError_t launch_index_encode(const IndexArgs& a, hipStream_t stream);

// Stream-ordered scratch and the prefix sum (hdx_scratch.hip).
// A buffer from the library's per-device memory pool (the regions' coordinate
// chunks, the scan's block sums, the stored-object stages' arrays), on the
// calling thread's current device.  acquire before the first launch: on
// failure HIP's last error is cleared, *no_scratch is set and false comes back
// — nothing may be launched.  release(e): frees it behind the work on the
// stream (nothing to free: no call) and returns e, or the free's error where e
// is hipSuccess.
struct PoolScratch {
    void* p = nullptr;
    hipStream_t stream = nullptr;
    bool acquire(uint64_t bytes, hipStream_t s, bool* no_scratch);
    hipError_t release(hipError_t e);
};
void trim_scratch_pools();  // release the pools' cached memory
// The exclusive prefix sum of data[0..N) in place, reduce-then-scan over
// separate launches; scratch holds scan_scratch_words(N) u64 of block sums
// (none up to kIndexScanBlock).
constexpr uint32_t kIndexScanBlock = 1024;  // elements per workgroup of the prefix sum
hipError_t scan_exclusive(uint64_t* data, uint64_t N, uint64_t* scratch, hipStream_t stream);
uint64_t scan_scratch_words(uint64_t N);

// Secondary-index entries of stored objects (hdx_index_entries.hip): m
// indices over n stored objects, entry e = i*m + k.  enc[] / key_enc hold the
// index encoder of each indexed attribute and of the key (ENC_*,
// hdx_host_common.h).
constexpr uint32_t kIndexPrefixStride = 24; // >= HDX_INDEX_PREFIX_MAX
struct IndexEntriesArgs : StoredObjects {
    uint32_t* attr_off;       // [n*m] plan writes, fill reads
    uint32_t* attr_len;       // [n*m]
    uint64_t* entry_off;      // [n*m + 1]
    uint8_t* entries;         // fill only
    uint64_t entries_bytes;
    uint32_t* status;         // may be NULL
    uint64_t n;
    uint32_t A, m;
    uint32_t key_enc;
    uint16_t attr[HDX_MAX_INDICES];
    uint8_t enc[HDX_MAX_INDICES];
    uint8_t plen[HDX_MAX_INDICES];
    uint8_t prefix[HDX_MAX_INDICES * kIndexPrefixStride];
};
static_assert(sizeof(IndexEntriesArgs) == 1016, "kernel argument layout");
// The walk (a lane per object), then scan_exclusive over the n*m + 1 entry
// sizes.  Its block sums come from the library's stream-ordered pool
// (PoolScratch); if that allocation fails nothing is launched and *no_scratch
// is set.
hipError_t launch_index_entries_plan(const IndexEntriesArgs& a, hipStream_t stream, bool* no_scratch);
hipError_t launch_index_entries_fill(const IndexEntriesArgs& a, hipStream_t stream);

// The objects behind a list of indices, packed (hdx_gather_objects.hip):
// record r = [key of idx[r] if KEYS][value of idx[r] if VALUES] at out +
// rec_off[r], r < min(*count, cap).
constexpr uint32_t kGatherTileBytes = 4096;  // output bytes a wave of the fill owns per step
struct GatherObjectsArgs : StoredObjects {
    const uint64_t* idx;      // [cap]
    const uint64_t* count;    // one u64, or NULL: cap
    uint64_t* rec_off;        // [cap + 1] plan writes, fill reads
    uint32_t* rec_key_len;    // [cap] plan only, may be NULL
    uint8_t* out;             // fill only
    uint64_t out_bytes;
    uint32_t* status;         // may be NULL
    uint64_t n, cap;
    uint32_t what;            // HDX_GATHER_KEYS | HDX_GATHER_VALUES
};
static_assert(sizeof(GatherObjectsArgs) == 128, "kernel argument layout");
// A lane per record stores its size, then scan_exclusive over cap + 1
// elements; block sums from the pool, *no_scratch as above.
hipError_t launch_gather_objects_plan(const GatherObjectsArgs& a, hipStream_t stream, bool* no_scratch);
// Tile-owned: a wave per kGatherTileBytes of the output.
hipError_t launch_gather_objects_fill(const GatherObjectsArgs& a, hipStream_t stream);
// Debug library only: the plan as two extents per record, then
// launch_gather_extents (the record-major A/B baseline).
hipError_t launch_gather_objects_by_extents(const GatherObjectsArgs& a, hipStream_t stream, bool* no_scratch);

// A search's attribute checks over stored objects (hdx_checks.hip): the ops
// of compile_checks (hdx_host_common.h) and their STRING constants, packed
// at op[k].koff, travel by value.
constexpr uint32_t kCheckBlock = 256;  // objects per workgroup of both kernels
struct CheckArgs : StoredObjects {
    uint32_t* first_fail;  // [n]
    uint64_t* match;       // [n] or NULL: no compaction
    uint64_t* match_count;
    uint32_t* status;      // may be NULL
    uint64_t n;
    uint32_t A, c;
    CheckOp op[HDX_MAX_CHECKS];
    uint64_t konst[kCheckConstBytes / 8];
};
static_assert(sizeof(CheckArgs) == 1632, "kernel argument layout");
// The programs of a compiled list's OP_REGEX ops (op k's: prog[op[k].koff]):
// a further, last kernel argument of the kernels that run them, so the kernels
// the one-shot entry points launch keep their arguments.  Their byte-class tables
// are built in LDS by each workgroup (hdx_check_eval.h).
struct RegexArgs {
    uint32_t count, pad_;
    RegexProg prog[HDX_MAX_REGEX_CHECKS];
};
// check_kernel (the walk and the ops, a lane per object); with a.match also
// one pass count per workgroup, their scan (scan_exclusive) and
// check_compact_kernel.  The counts come from the library's stream-ordered
// pool; if that allocation fails nothing is launched and *no_scratch is set.
// rx: NULL, or a list with OP_REGEX ops (check_kernel<RegexArgs>).
hipError_t launch_check_encoded(const CheckArgs& a, hipStream_t stream, bool* no_scratch,
                                const RegexArgs* rx = nullptr);
// The top-limit matches by one attribute (hdx_sorted.hip): the checks as
// above (ck.first_fail may be NULL; ck.match is not used), then a 64-bit rank
// key per matching object, a radix select of the limit-th key, the compacted
// candidates and one workgroup's finishing sort.
constexpr uint32_t kSortFinishBlock = 1024;  // candidates per round of the finishing step
enum : uint32_t { SORT_TIE = 0, SORT_STRING = 1, SORT_INT64 = 2, SORT_FLOAT = 3 };
struct SortedArgs {
    CheckArgs ck;
    uint64_t* top;        // [limit]
    uint64_t* top_count;
    uint64_t limit;       // <= HDX_SORT_LIMIT_MAX
    uint32_t attr;        // the sort attribute, 0 = the key (unused with SORT_TIE)
    uint32_t kind;        // SORT_*: SORT_TIE where attr >= attrs_sz, every object ties
    uint32_t keep, descending;
};
static_assert(sizeof(SortedArgs) == 1672, "kernel argument layout");
// Device scratch of sorted_scratch_bytes(n) from the library's stream-ordered
// pool; if that allocation fails nothing is launched and *no_scratch is set.
uint64_t sorted_scratch_bytes(uint64_t n);
hipError_t launch_sorted_search(const SortedArgs& a, hipStream_t stream, bool* no_scratch,
                                const RegexArgs* rx = nullptr);
static_assert(sizeof(SortedArgs) + sizeof(RegexArgs) + 64 <= 3072, "kernel arguments: well under the 4 KiB limit");

// Search pruning (hdx_index.hip) over one subspace's region table: m ranges
// that name a subspace attribute, in the order lookup_search visits them.
enum : uint8_t { SEARCH_NONE = 0, SEARCH_STRING_EQ = 1, SEARCH_ORDERED = 2 };
constexpr uint32_t kMaxSearchRanges = 16;  // one range per subspace dimension
struct SearchArgs {
    RegionView t;            // the table: its boxes (lower, upper, R, D) are read
    const uint64_t* hashes;  // [2*m]: hash of start, hash of end
    const uint8_t* replicas; // [R] 0 = region without replicas (skipped), or NULL = all have
    uint8_t* include;        // [R]
    uint32_t* cleared;       // set when the reference would clear the server list
    uint32_t m;
    uint8_t dim[kMaxSearchRanges];
    uint8_t kind[kMaxSearchRanges];
    uint8_t flags[kMaxSearchRanges];  // bit 0 has_start, bit 1 has_end
};

hipError_t launch_search_regions(const SearchArgs& a, hipStream_t stream);

struct SynthArgs {
    uint64_t seed;
    uint64_t first;
    uint64_t n;
    uint32_t A;
    uint32_t pad_;
    hdx_synth_rule rules[64];
};

hipError_t launch_synth_lengths(const SynthArgs& a, uint32_t* attr_len, hipStream_t s);
hipError_t launch_synth_fill(const SynthArgs& a, const uint64_t* obj_base, const uint32_t* attr_len,
                             uint8_t* blob, uint64_t bytes, hipStream_t s);

// keys (may be NULL): each key is also copied to keys + key_off[i]
hipError_t launch_synth_encode(const uint8_t* blob, const uint64_t* obj_base, const uint32_t* attr_len,
                               uint32_t A, uint64_t n, uint64_t first_version, const uint64_t* val_off,
                               uint8_t* vals, hipStream_t s, const uint64_t* key_off = nullptr,
                               uint8_t* keys = nullptr);

}  // namespace hdx
