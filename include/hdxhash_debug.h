/*
 * hdxhash_debug.h — measurement and tuning hooks (not part of the drop-in
 * boundary).
 *
 * Both libraries: hdxdbg_kernel_for (which kernel the automatic policy runs),
 * hdxdbg_stream_probe (bench.py's practical HBM ceiling),
 * hdxdbg_region_chunk_objects (tests/test_scale.py's chunk edges) and
 * hdxdbg_wave_geometry (tests/test_window_edges.py's window boundaries).
 * libhdxhash_dbg.so only (HDX_DEBUG_BUILD, hyperdex_amd/csrc/Makefile):
 * hdxdbg_set_kernel_variant / hdxdbg_kernel_variant / hdxdbg_variant_entries,
 * used by scripts/ab_variants.py and the variant parity tests, and
 * hdxdbg_gather_objects_fill_by_extents, the object gather's record-major
 * baseline.  The product library
 * has no kernel selection and no environment switches.
 */
#ifndef HDXHASH_DEBUG_H
#define HDXHASH_DEBUG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* [debug library only] Select the hash kernel variant for subsequent launches in this process
 * (see hyperdex_amd/csrc/hdx_kernels.hip; -1 = automatic per schema);
 * returns the previous selection, or -2 for an unknown variant (nothing
 * changed). */
int hdxdbg_set_kernel_variant(int variant);
int hdxdbg_kernel_variant(void);
/* [debug library only] Where a variant id selects something: a mask of the
 * entry points at which it has a row in the variant table (the other entry
 * points keep their automatic policy under it), HDXDBG_ENTRY_POLICY for an id
 * that switches a policy instead of a kernel; -2 for an unknown id. */
#define HDXDBG_ENTRY_BATCH 1          /* hdx_hash_batch_device */
#define HDXDBG_ENTRY_BATCH_REGIONS 2  /* hdx_hash_batch_regions_device, A <= 128 */
#define HDXDBG_ENTRY_SWEEP 4          /* hdx_hash_encoded_device, A <= 128 */
#define HDXDBG_ENTRY_WIDE_SWEEP 8     /* hdx_hash_encoded_device, wide schemas */
#define HDXDBG_ENTRY_POLICY 16
int hdxdbg_variant_entries(int variant);
/* The variant hdx_hash_batch_device would launch for this schema and object
 * count (under the current selection), and the kernel's symbol as rocprofv3
 * reports it (*name; static string).  Returns -2 on a bad schema. */
int hdxdbg_kernel_for(const uint32_t* types, uint32_t attrs_sz, uint64_t n, const char** name);
/* HBM streaming probe: read `bytes` (a multiple of 4096) of device memory at
 * src in the hash kernels' access shape; write != 0 also stores one 8-byte
 * word per 64 bytes read into sink[bytes / 64] (the 1:8 write mix of the
 * 64-byte-attribute configs).  Asynchronous on `stream`.  bench.py reports the
 * rate as the practical ceiling beside the HBM3E spec. */
int hdxdbg_stream_probe(const void* src, uint64_t bytes, uint64_t* sink, int write, void* stream);
/* [debug library only] The device set of hdx_init_mask from an explicit list
 * of HIP ordinals, repeats allowed (world 2+ on one GPU: host batches and
 * ungathered shards; a gather over a repeated device returns HDX_E_INVALID). */
int hdxdbg_init_devices(const int* devices, int n);
/* Objects per scratch chunk of the regions entry points when the caller
 * wants no coordinates (n objects of attrs_sz attributes; hdx_regions.hip). */
uint64_t hdxdbg_region_chunk_objects(uint64_t n, uint32_t attrs_sz);
/* What one wave of the wave-staged form holds for this schema: sweep == 0 the
 * batch kernel hdx_hash_batch_device launches (hdx_wstage.hip; under the
 * current selection, when that is the product's form), sweep != 0 the
 * stored-object sweep of hdx_hash_encoded_device (hdx_wsweep.hip).  Fills
 * out[HDXDBG_WAVE_GEOMETRY_WORDS]: objects per wave K; window bytes WB; the
 * bytes of the window that keys copied apart from their values may take (0
 * for the batch kernel); the bytes kept readable before and after the window
 * (hash_slot_window's reads around a short string); passes of 64 slots per
 * wave NCH and the cap on K, so that K = min(64 * NCH / attrs_sz, cap).
 * tests/test_window_edges.py builds its boundary cases from these.  Returns
 * 0, -2 on a bad schema, -1 when the schema takes another form.
 * It answers for the product's two forms only.  In the debug library, with a
 * variant selected: 212 (the batch product's own id, which leaves the sweep's
 * policy alone) answers as the automatic policy does, for any schema of up to
 * 128 attributes; every other selection returns -1 for both kernels, the
 * other wave-staged A/B variants (213..216, 258, 273, ...: windows and
 * object counts of their own) and the ones that would leave the sweep alone
 * included. */
#define HDXDBG_WAVE_GEOMETRY_WORDS 7
int hdxdbg_wave_geometry(const uint32_t* types, uint32_t attrs_sz, int sweep, uint32_t* out);
/* [debug library only] hdx_gather_objects_fill_device's arguments and output
 * by the record-major form: a kernel turns the plan into two extents per
 * record (source address, length, destination offset), then the host
 * pipelines' extent copy (hdx_gather.hip), a wave per extent, moves them.
 * The A/B baseline of tools/gather_objects_rate.py and a second opinion for
 * the tests.  The extents, 40 bytes per record, come from the library's
 * stream-ordered pool (HDX_E_NOMEM, nothing launched, if that fails). */
int hdxdbg_gather_objects_fill_by_extents(const uint8_t* keys, const uint64_t* key_off, const uint32_t* key_len,
                                          const uint8_t* vals, const uint64_t* val_off, const uint32_t* val_len,
                                          uint64_t n, const uint64_t* idx, const uint64_t* count_dev, uint64_t cap,
                                          uint32_t what, const uint64_t* rec_off, uint8_t* out, uint64_t out_bytes,
                                          uint32_t* status_dev, void* stream);

#ifdef __cplusplus
}
#endif

#endif
