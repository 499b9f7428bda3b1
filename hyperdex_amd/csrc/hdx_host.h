// hdx_host.h — host-side helpers shared by the C-ABI translation units
// (argument checking, error text, device binding, staging growth).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <functional>
#include <mutex>
#include <vector>

#include "hdx_internal.h"

namespace hdx {

hdx_status hip_fail(hipError_t e, const char* what);

#define HIP_TRY(expr)                                     \
    do {                                                  \
        hipError_t e_ = (expr);                           \
        if (e_ != hipSuccess) return hip_fail(e_, #expr); \
    } while (0)

template <typename T>
inline hdx_status grow_dev(T** p, size_t* cap, size_t need) {
    if (need <= *cap) return HDX_OK;
    size_t n = std::max(need, *cap * 3 / 2);
    (void)hipFree(*p);
    *p = nullptr;
    *cap = 0;
    if (hipMalloc((void**)p, n * sizeof(T)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(HDX_E_NOMEM, "hipMalloc(%zu) failed", n * sizeof(T));
    }
    *cap = n;
    return HDX_OK;
}

template <typename T>
inline hdx_status grow_pinned(T** p, size_t* cap, size_t need) {
    if (need <= *cap) return HDX_OK;
    size_t n = std::max(need, *cap * 3 / 2);
    (void)hipHostFree(*p);
    *p = nullptr;
    *cap = 0;
    if (hipHostMalloc((void**)p, n * sizeof(T), hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        return fail(HDX_E_NOMEM, "hipHostMalloc(%zu) failed", n * sizeof(T));
    }
    *cap = n;
    return HDX_OK;
}

// Validates a schema and fills codes_out[A] (may be NULL).
hdx_status check_schema(const uint32_t* types, uint32_t A, uint8_t* codes_out);
// The kernels' code table from codes[0..A): the kernarg copy, and for wide
// schemas (the wide kernels, hdx_wide.hip) a device copy on the calling
// thread's current device.
hdx_status set_codes(BatchArgs& args, const uint8_t* codes, uint32_t A);
hdx_status set_codes(EncodedArgs& a, const uint8_t* codes, uint32_t A);
// Region tables of a call: at most kMaxSweepTables, none NULL, every
// subspace attribute < A; region_ids non-NULL when there are tables.
hdx_status check_tables(const hdx_region_table* tables, uint32_t ntables, uint32_t A, const uint64_t* region_ids);
// the table list alone (count, NULLs, subspace attributes < A): no output pointer
hdx_status check_table_list(const hdx_region_table* tables, uint32_t ntables, uint32_t A);
// A packed batch's kernel arguments on device `dev` (the calling thread's
// current device): codes, arrays, and T tables whose ids go to ids + t *
// ids_stride.
hdx_status batch_args(BatchArgs& args, const uint8_t* codes, uint32_t A, const uint8_t* blob,
                      const uint64_t* obj_base, const uint32_t* attr_len, uint64_t n, uint64_t* coords,
                      uint32_t* status, const hdx_region_table* tables, uint32_t T, uint64_t* ids,
                      uint64_t ids_stride, int dev);
// The same for stored objects (the sweep).
hdx_status encoded_args(EncodedArgs& a, const uint8_t* codes, uint32_t A, const StoredObjects& so, uint64_t n,
                        uint64_t* coords, uint64_t* versions, uint32_t* status, const hdx_region_table* tables,
                        uint32_t T, uint64_t* ids, uint64_t ids_stride, int dev);
// Device scratch owned by the library (per-thread staging and streams),
// registered so hdx_shutdown can free every thread's (track_scratch /
// untrack_scratch; release() must leave the object reusable).
struct Scratch {
    virtual void release() = 0;
    virtual ~Scratch() = default;
};
void track_scratch(Scratch* s);
void untrack_scratch(Scratch* s);
// Binds the calling thread to `want` (-1: its current device) after checking it is gfx950.
hdx_status bind_device(int want);
// Frees the calling thread's library scratch now (streams, staging) and
// unregisters it: a thread the library owns calls it as its last job, so no
// HIP call runs in its thread-local destructors at exit (rocprofv3, among
// others, has torn down its per-thread state by then).
void release_thread_scratch();
// Hands the frees of an exiting thread's scratch to the library: a
// thread-local destructor makes no HIP call itself (the runtime or a
// profiler's per-thread state may be gone at thread exit); hdx_shutdown or
// the next thread binding a device runs them.
void park_orphan(std::function<void()> free_fn);
// The calling thread's library stream (created on first use).
hdx_status thread_stream(hipStream_t* out);
// The device the calling thread is bound to (-1: none yet).
int thread_device();
// True for page-locked host memory (hipHostMalloc / registered).
bool is_pinned(const void* p);

// One of a thread's two host-pipeline slots (hdx_hostpath.cpp): a stream,
// device staging and pinned staging, grown on demand, freed with the thread's
// scratch (hdx_capi.cpp).
template <typename T>
struct DevBuf {  // hipMalloc'd
    T* p = nullptr;
    size_t cap = 0;
    hdx_status need(size_t n) { return grow_dev(&p, &cap, n); }
    void release() {
        (void)hipFree(p);
        *this = DevBuf{};
    }
};
template <typename T>
struct PinBuf {  // hipHostMalloc'd
    T* p = nullptr;
    size_t cap = 0;
    hdx_status need(size_t n) { return grow_pinned(&p, &cap, n); }
    void release() {
        (void)hipHostFree(p);
        *this = PinBuf{};
    }
};
// A slot's buffers, each declared here once: X(type, name) is a device buffer
// d_<name> and a pinned one h_<name> (inputs: filled only when the caller's
// array is pageable or the chunk is rebased or packed; outputs: only for
// pageable destinations).  The packed and the stored pipeline never hold a
// slot at the same time and share the buffers of one role.
#define HDX_SLOT_BUFFERS(X)                                                                    \
    X(uint8_t, blob)    /* packed blob; stored values, records, or packed records */          \
    X(uint8_t, keys)    /* the key column's span */                                            \
    X(uint64_t, off)    /* the chunk's object bases / key offsets */                           \
    X(uint64_t, voff)   /* value offsets */                                                    \
    X(uint32_t, len)    /* attribute lengths / key lengths */                                  \
    X(uint32_t, vlen)   /* value lengths */                                                    \
    X(uint64_t, coords) /* outputs */                                                          \
    X(uint64_t, ids)                                                                           \
    X(uint64_t, ver)                                                                           \
    X(uint32_t, status) /* the sweep's status word */                                          \
    X(uint64_t, src)    /* packed chunks (objects out of address order): the extents' */      \
    X(uint32_t, sz)     /* sources, lengths and destination offsets for the gather */         \
    X(uint64_t, dst)    /* kernel (hdx_gather.hip) */
struct HostSlot {
    hipStream_t s = nullptr;
#define HDX_SLOT_DECLARE(T, name) \
    DevBuf<T> d_##name;           \
    PinBuf<T> h_##name;
    HDX_SLOT_BUFFERS(HDX_SLOT_DECLARE)
#undef HDX_SLOT_DECLARE
    void release_buffers() {
#define HDX_SLOT_RELEASE(T, name) \
    d_##name.release();           \
    h_##name.release();
        HDX_SLOT_BUFFERS(HDX_SLOT_RELEASE)
#undef HDX_SLOT_RELEASE
    }
};
// The device view of pinned host memory p (for a kernel to read it), or NULL
// when p is not pinned.
const uint8_t* device_view(const uint8_t* p);
// Waits for the slot's stream, frees everything, destroys the stream (on the
// current device, which must be the slot's).
void free_host_slot(HostSlot& s);
// The calling thread's two slots (binds the thread; streams created).
hdx_status thread_slots(HostSlot** out);

// Region outputs of a host-resident call: table t's id of the call's object
// i goes to ids[t * stride + i].
struct HostRegions {
    const hdx_region_table* tables;
    uint32_t T;
    uint64_t* ids;
    uint64_t stride;
};

// The single-device host-resident pipelines (hdx_hostpath.cpp) on the calling
// thread's device; codes validated, n > 0.  coords may be NULL when R has
// tables; R may be NULL.
hdx_status hash_host(const uint8_t* codes, uint32_t A, const uint8_t* blob, uint64_t blob_bytes,
                     const uint64_t* obj_base, const uint32_t* attr_len, uint64_t n, uint64_t* coords,
                     const HostRegions* R);
// Stored objects in host memory: the columns and the sizes of the two stores, which every
// object's extents are checked against.
struct StoredHost {
    StoredObjects o;
    uint64_t keys_bytes, vals_bytes;
    // objects [first, ...): the per-object columns advance, the stores stay
    StoredHost from(uint64_t first) const {
        return {{o.keys, o.key_off + first, o.key_len + first, o.vals, o.val_off + first, o.val_len + first},
                keys_bytes, vals_bytes};
    }
};
// Stored objects: *status_bits receives the OR of the device status words
// (1 << HDX_E_BADENC, 1 << HDX_E_BADSIZE); versions may be NULL.
hdx_status hash_encoded_host(const uint8_t* codes, uint32_t A, const StoredHost& h, uint64_t n, uint64_t* coords,
                             uint64_t* versions, const HostRegions* R, uint32_t* status_bits);

// The device set of hdx_init_mask (hdx_multi.cpp): create (replacing a set
// of another mask), tear down (waits for calls in progress, joins its
// workers), and the host-resident calls split over it (the calling thread's
// device alone without a set).
hdx_status device_set_create(uint64_t mask, const std::vector<int>& devs);
void device_set_teardown();
hdx_status hash_host_any(const uint8_t* codes, uint32_t A, const uint8_t* blob, uint64_t blob_bytes,
                         const uint64_t* obj_base, const uint32_t* attr_len, uint64_t n, uint64_t* coords,
                         const HostRegions* R);
hdx_status hash_encoded_host_any(const uint8_t* codes, uint32_t A, const StoredHost& h, uint64_t n, uint64_t* coords,
                                 uint64_t* versions, const HostRegions* R);

}  // namespace hdx

// One subspace's region table (include/hdxhash.h): its host arrays and a copy
// of them on every device it has been used on.
struct hdx_region_table_s {
    // The arrays on one device; index NULL: the table has none (lookups scan
    // the boxes).  lower, upper and ids carry 8 bytes of padding.
    struct Copy {
        int device;
        uint64_t *lower, *upper, *ids, *index;
    };
    // The copy on the device the table was created on.  home.device is the
    // struct's first int and is compared with the calling device on every
    // call (region_view); tests rewrite it to force the replica path.
    Copy home;
    uint32_t D, R, W, index_words;
    uint16_t attrs[16];
    // host copies (the batcher's calling-thread lookups, the replicas below);
    // h_index empty: no index
    std::vector<uint64_t> h_lower, h_upper, h_ids, h_index;
    // copies on the other devices a call has used the table on (the device
    // set's entry points), made on first use under rep_mu, freed with the table
    std::mutex rep_mu;
    std::vector<Copy> replicas;
};

namespace hdx {
// Table t as a launch on device `dev` (the calling thread's current device)
// sees it: the home copy on the device the table was created on, else a
// replica there, uploaded on first use (HDX_E_NOMEM if that fails).  The one
// way from a handle to kernel arguments.
hdx_status region_view(hdx_region_table_s* t, int dev, RegionView& v);
// A fused launch's table: the view, and its id output at `out`.
inline hdx_status fill_sweep_table(SweepTable& st, hdx_region_table_s* t, int dev, uint64_t* out) {
    st = SweepTable{};
    st.out = out;
    return region_view(t, dev, st);
}
}  // namespace hdx

// configuration::lookup_region (common/configuration.cc:698-735) on the host
// (hdx_region_index.h) over the table's host arrays: through its interval
// index when it has one, else the reference's scan.
inline uint64_t region_lookup_host(const hdx_region_table_s* t, const uint64_t* hs) {
    return hdx::region_lookup_arrays(t->D, t->R, t->W, t->attrs, t->h_lower.data(), t->h_upper.data(), t->h_ids.data(),
                                     t->h_index.empty() ? nullptr : t->h_index.data(), hs);
}

