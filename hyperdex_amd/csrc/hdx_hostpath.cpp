// hdx_hostpath.cpp — the host-resident entry points (include/hdxhash.h):
// batches and stored objects that arrive in host memory and whose outputs go
// back to host memory, as in the daemon: objects come from network buffers
// (daemon/key_state.cc:1455-1543 -> hyperdex::hash) and the reindex sweep
// reads LevelDB values on the host (daemon/datalayer_indexer_thread.cc:
// 161-176 -> datalayer::get_from_iterator -> decode_value,
// daemon/datalayer.cc:853-882).
//
// One device's pipeline (hash_host, hash_encoded_host) streams the call
// through its two slots in chunks (hdx_chunks.h): host validation of the
// chunk, H2D of its span(s) and rebased offsets, the kernel(s), D2H of the
// outputs — the two slots' streams overlap one chunk's copies with the
// other's kernel.  One driver (run_chunks) owns the slots and the chunks in
// flight; a source per kind of input (PackedSource, StoredSource) validates
// the objects, uploads a chunk and launches its kernel.  hdx_multi.cpp splits
// a call over the device set and runs one pipeline per device (hash_host_any /
// hash_encoded_host_any).  Stored objects travel through all of it as one
// StoredHost (hdx_host.h): the columns and the two stores' sizes; a device's
// range and a chunk are h.from(first).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "hdx_chunks.h"
#include "hdx_host.h"

namespace hdx {

void free_host_slot(HostSlot& s) {
    if (s.s) (void)hipStreamSynchronize(s.s);
    s.release_buffers();
    if (s.s) (void)hipStreamDestroy(s.s);
    s = HostSlot{};
}

static bool is_numeric_code(uint8_t c) { return c >= CODE_INT64; }

const uint8_t* device_view(const uint8_t* p) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    if (a.type != hipMemoryTypeHost || !a.devicePointer || !a.hostPointer) return nullptr;
    return (const uint8_t*)a.devicePointer + (p - (const uint8_t*)a.hostPointer);
}

namespace {

// The host source of an H2D copy of p[0, count): the caller's array when it
// is pinned, else a copy of it in pinned staging.
template <typename T>
hdx_status pinned_or_staged(const T* p, bool pinned, PinBuf<T>& buf, uint64_t count, const T** src) {
    *src = p;
    if (pinned) return HDX_OK;
    const hdx_status st = buf.need(std::max<uint64_t>(count, 1));
    if (st != HDX_OK) return st;
    std::memcpy(buf.p, p, count * sizeof(T));
    *src = buf.p;
    return HDX_OK;
}

// A chunk's small arrays (offsets, lengths, gather extents), host to device.
// by_kernel (a chunk the device packs): one copy kernel through the sources'
// device views when each has one, so that every input of the chunk is moved by
// the compute queue and the gather waits on no SDMA copy; else a copy each.
struct SmallCopy {
    const void* src;
    void* dst;
    uint64_t bytes;
};
hdx_status copy_small(const SmallCopy* c, uint32_t count, bool by_kernel, hipStream_t s) {
    const void* src[8];
    void* dst[8];
    uint64_t bytes[8];
    for (uint32_t x = 0; by_kernel && x < count; ++x) {
        src[x] = device_view((const uint8_t*)c[x].src);
        dst[x] = c[x].dst;
        bytes[x] = c[x].bytes;
        by_kernel = src[x] != nullptr;
    }
    if (by_kernel) {
        HIP_TRY(launch_copy_linear(src, dst, bytes, count, s));
        return HDX_OK;
    }
    for (uint32_t x = 0; x < count; ++x) HIP_TRY(hipMemcpyAsync(c[x].dst, c[x].src, c[x].bytes, hipMemcpyHostToDevice, s));
    return HDX_OK;
}

// One chunk in flight on a slot: where its outputs go once it lands.
struct Pending {
    bool live = false;
    uint64_t first = 0, cnt = 0;
};

// The outputs common to both pipelines: coordinates, region ids (staged
// through pinned memory when the caller's arrays are pageable).
struct Outputs {
    uint32_t A;
    uint64_t* coords;  // may be NULL
    bool coords_pinned;
    const HostRegions* R;  // may be NULL
    bool ids_pinned;
    uint64_t* versions = nullptr;  // stored objects only
    bool versions_pinned = false;

    Outputs(uint32_t A_, uint64_t* coords_, const HostRegions* R_, uint64_t* versions_ = nullptr)
        : A(A_), coords(coords_), coords_pinned(coords_ && is_pinned(coords_)), R(R_),
          ids_pinned(R_ && R_->T && is_pinned(R_->ids)), versions(versions_),
          versions_pinned(versions_ && is_pinned(versions_)) {}

    uint32_t T() const { return R ? R->T : 0; }
    // D2H of a chunk's outputs on the slot's stream
    hdx_status copy_back(HostSlot& sl, uint64_t i, uint64_t cnt) const {
        hdx_status st;
        if (coords) {
            uint64_t* dst = coords + i * A;
            if (!coords_pinned) {
                if ((st = sl.h_coords.need(cnt * A)) != HDX_OK) return st;
                dst = sl.h_coords.p;
            }
            HIP_TRY(hipMemcpyAsync(dst, sl.d_coords.p, cnt * A * 8, hipMemcpyDeviceToHost, sl.s));
        }
        if (T()) {
            if (!ids_pinned && (st = sl.h_ids.need(cnt * T())) != HDX_OK) return st;
            for (uint32_t t = 0; t < T(); ++t) {
                uint64_t* dst = ids_pinned ? R->ids + t * R->stride + i : sl.h_ids.p + t * cnt;
                HIP_TRY(hipMemcpyAsync(dst, sl.d_ids.p + t * cnt, cnt * 8, hipMemcpyDeviceToHost, sl.s));
            }
        }
        if (versions) {
            uint64_t* dst = versions + i;
            if (!versions_pinned) {
                if ((st = sl.h_ver.need(cnt)) != HDX_OK) return st;
                dst = sl.h_ver.p;
            }
            HIP_TRY(hipMemcpyAsync(dst, sl.d_ver.p, cnt * 8, hipMemcpyDeviceToHost, sl.s));
        }
        return HDX_OK;
    }
    // after the slot's stream synchronised: the staged outputs into place
    void land(HostSlot& sl, uint64_t i, uint64_t cnt) const {
        if (coords && !coords_pinned) std::memcpy(coords + i * A, sl.h_coords.p, cnt * A * 8);
        if (T() && !ids_pinned)
            for (uint32_t t = 0; t < T(); ++t) std::memcpy(R->ids + t * R->stride + i, sl.h_ids.p + t * cnt, cnt * 8);
        if (versions && !versions_pinned) std::memcpy(versions + i, sl.h_ver.p, cnt * 8);
    }
};

// The pipeline of one call on the calling thread's two slots (thread_slots,
// taken before the source is built: it binds the thread).  Per chunk:
// wait for the slot's previous chunk and land its outputs, then the source's
// upload (grow the slot's buffers, host-side staging, H2D) and launch (the
// kernel into d_coords / d_ids / d_ver), then the outputs' D2H.  Host
// validation of the next chunk (next_chunk -> src.object) runs while both
// slots' chunks move.  status_bits (stored objects; else NULL) receives the OR
// of the chunks' device status words, d_status -> h_status.  Any failure lets
// every copy in flight land before it returns.
template <typename Source>
hdx_status run_chunks(HostSlot* slots, Source& src, uint64_t n, const Outputs& out, uint32_t* status_bits) {
    hdx_status st;
    Pending pend[2];
    auto finish = [&](int k) -> hdx_status {
        if (!pend[k].live) return HDX_OK;
        pend[k].live = false;
        HIP_TRY(hipStreamSynchronize(slots[k].s));
        out.land(slots[k], pend[k].first, pend[k].cnt);
        if (status_bits) *status_bits |= *slots[k].h_status.p;
        return HDX_OK;
    };
    auto drain = [&](hdx_status err) {
        for (int q = 0; q < 2; ++q) {
            (void)finish(q);
            (void)hipStreamSynchronize(slots[q].s);
        }
        return err;
    };
    auto status_back = [&](HostSlot& sl) -> hdx_status {
        if (status_bits) HIP_TRY(hipMemcpyAsync(sl.h_status.p, sl.d_status.p, 4, hipMemcpyDeviceToHost, sl.s));
        return HDX_OK;
    };
    ChunkCursor cur;
    Chunk c;
    int k = 0;
    for (;; k ^= 1) {
        if ((st = next_chunk(src, n, src.device_packs(), cur, c)) != HDX_OK) return drain(st);
        if (c.cnt == 0) break;
        HostSlot& sl = slots[k];
        if ((st = finish(k)) != HDX_OK || (st = src.upload(sl, c)) != HDX_OK || (st = src.launch(sl, c)) != HDX_OK ||
            (st = out.copy_back(sl, c.first, c.cnt)) != HDX_OK || (st = status_back(sl)) != HDX_OK)
            return drain(st);
        pend[k] = {true, c.first, c.cnt};
    }
    if ((st = finish(k)) != HDX_OK) return drain(st);
    return finish(k ^ 1);
}

// ---- packed batches ---------------------------------------------------------------

struct PackedSource {
    const uint8_t* codes;
    uint32_t A;
    const uint8_t* blob;
    uint64_t blob_bytes;
    const uint64_t* obj_base;
    const uint32_t* attr_len;
    const HostRegions* R;  // may be NULL
    const bool blob_pinned = is_pinned(blob), len_pinned = is_pinned(attr_len);
    const uint8_t* const blob_dev = blob_pinned ? device_view(blob) : nullptr;  // the gather kernel's view
    const int dev = thread_device();
    std::vector<uint32_t> sizes;  // of the objects validated and not yet uploaded, in order

    uint32_t stores() const { return 1; }
    bool device_packs() const { return blob_dev != nullptr; }

    // Host-side validation (the reference asserts here) and the object's byte
    // extent, done chunk by chunk as the pipeline reaches each object, so the
    // first copies start after one chunk's validation, not the batch's.
    hdx_status object(uint64_t i, ObjectExtents& o) {
        uint64_t s = 0;
        for (uint32_t j = 0; j < A; ++j) {
            const uint32_t L = attr_len[i * A + j];
            if (is_numeric_code(codes[j]) && L != 0 && L != 8)
                return fail(HDX_E_BADSIZE, "object %llu attribute %u: numeric value of %u bytes",
                            (unsigned long long)i, j, L);
            s += L;
        }
        if (s >= (1ull << 32))
            return fail(HDX_E_INVALID, "object %llu is %llu bytes (limit 4 GiB)", (unsigned long long)i,
                        (unsigned long long)s);
        if (obj_base[i] > blob_bytes || s > blob_bytes - obj_base[i])
            return fail(HDX_E_INVALID, "object %llu [%llu,+%llu) outside blob of %llu bytes", (unsigned long long)i,
                        (unsigned long long)obj_base[i], (unsigned long long)s, (unsigned long long)blob_bytes);
        sizes.push_back((uint32_t)s);
        o.count = 1;
        o.ext[0] = {0, obj_base[i], s};
        return HDX_OK;
    }

    // The chunk as one span when its objects lie (nearly) back to back, else
    // packed in index order.
    hdx_status upload(HostSlot& sl, const Chunk& c) {
        const uint64_t i = c.first, cnt = c.cnt, lo = c.lo[0], bytes = c.moved();
        const uint32_t T = R ? R->T : 0;
        hdx_status st;
        if ((st = sl.d_blob.need(std::max<uint64_t>(bytes, 1))) != HDX_OK || (st = sl.d_off.need(cnt)) != HDX_OK ||
            (st = sl.d_len.need(cnt * A)) != HDX_OK || (st = sl.d_coords.need(cnt * A)) != HDX_OK ||
            (T && (st = sl.d_ids.need(cnt * T)) != HDX_OK) || (st = sl.h_off.need(cnt)) != HDX_OK)
            return st;
        const bool gather = !c.span && blob_dev;  // pinned objects out of order: packed on the device
        const uint8_t* src_blob = nullptr;
        if (c.span) {
            for (uint64_t t = 0; t < cnt; ++t) sl.h_off.p[t] = obj_base[i + t] - lo;
            if ((st = pinned_or_staged(blob + lo, blob_pinned, sl.h_blob, bytes, &src_blob)) != HDX_OK) return st;
        } else {
            uint64_t at = 0;  // packed offsets, index order
            for (uint64_t t = 0; t < cnt; ++t) {
                sl.h_off.p[t] = at;
                at += sizes[t];
            }
            if (gather) {
                if ((st = sl.h_src.need(cnt)) != HDX_OK || (st = sl.h_sz.need(cnt)) != HDX_OK ||
                    (st = sl.d_src.need(cnt)) != HDX_OK || (st = sl.d_sz.need(cnt)) != HDX_OK)
                    return st;
                std::memcpy(sl.h_src.p, obj_base + i, cnt * 8);
                std::memcpy(sl.h_sz.p, sizes.data(), cnt * 4);
            } else {  // pageable: each object copied into the pinned staging
                if ((st = sl.h_blob.need(std::max<uint64_t>(bytes, 1))) != HDX_OK) return st;
                for (uint64_t t = 0; t < cnt; ++t) std::memcpy(sl.h_blob.p + sl.h_off.p[t], blob + obj_base[i + t], sizes[t]);
                src_blob = sl.h_blob.p;
            }
        }
        sizes.erase(sizes.begin(), sizes.begin() + cnt);  // at most the next chunk's first object stays
        const uint32_t* src_len;
        if ((st = pinned_or_staged(attr_len + i * A, len_pinned, sl.h_len, cnt * A, &src_len)) != HDX_OK) return st;
        const SmallCopy off{sl.h_off.p, sl.d_off.p, cnt * 8}, len{src_len, sl.d_len.p, cnt * A * 4};
        if (gather) {
            const SmallCopy small[] = {off, {sl.h_src.p, sl.d_src.p, cnt * 8}, {sl.h_sz.p, sl.d_sz.p, cnt * 4}, len};
            if ((st = copy_small(small, 4, true, sl.s)) != HDX_OK) return st;
            HIP_TRY(launch_gather_extents(blob_dev, sl.d_src.p, sl.d_sz.p, sl.d_off.p, sl.d_blob.p, cnt, sl.s));
        } else {
            const SmallCopy small[] = {off, len};
            if ((st = copy_small(small, 2, false, sl.s)) != HDX_OK) return st;
            HIP_TRY(hipMemcpyAsync(sl.d_blob.p, src_blob, bytes, hipMemcpyHostToDevice, sl.s));
        }
        return HDX_OK;
    }

    hdx_status launch(HostSlot& sl, const Chunk& c) {
        const uint32_t T = R ? R->T : 0;
        BatchArgs args;
        // status: none (sizes validated above); the coordinates always land in
        // device staging, so the regions form needs no scratch of its own
        const hdx_status st = batch_args(args, codes, A, sl.d_blob.p, sl.d_off.p, sl.d_len.p, c.cnt, sl.d_coords.p,
                                         nullptr, R ? R->tables : nullptr, T, sl.d_ids.p, c.cnt, dev);
        if (st != HDX_OK) return st;
        if (T) {
            HIP_TRY(launch_hash_batch_regions(args, sl.s));
        } else {
            HIP_TRY(launch_hash_batch(args, sl.s));
        }
        return HDX_OK;
    }
};

// ---- stored objects (the reindex sweep from host memory) ----------------------------

struct StoredSource {
    const uint8_t* codes;
    uint32_t A;
    StoredHost h;
    const HostRegions* R;  // may be NULL
    // records [key][value] in one store (keys == vals, a LevelDB block's
    // adjacency): one span per chunk, and the kernel sees keys == vals
    const bool records = h.o.keys == h.o.vals;
    const uint32_t vstore = records ? 0 : 1;  // the values' store (hdx_chunks.h)
    const bool keys_pinned = is_pinned(h.o.keys), vals_pinned = is_pinned(h.o.vals);
    const bool klen_pinned = is_pinned(h.o.key_len), vlen_pinned = is_pinned(h.o.val_len);
    // keys and values out of order: packed as records [key][value] in index
    // order (hdx_gather.hip from pinned stores, a host copy per object from
    // pageable ones), so the kernel sees the record layout
    const uint8_t* const keys_dev = keys_pinned ? device_view(h.o.keys) : nullptr;
    const uint8_t* const vals_dev = vals_pinned ? device_view(h.o.vals) : nullptr;
    const int dev = thread_device();

    uint32_t stores() const { return records ? 1 : 2; }
    bool device_packs() const { return keys_dev && vals_dev; }

    hdx_status object(uint64_t i, ObjectExtents& o) const {
        const uint32_t kl = h.o.key_len[i], vl = h.o.val_len[i];
        const uint64_t ko = h.o.key_off[i], vo = h.o.val_off[i];
        if (is_numeric_code(codes[0]) && kl != 0 && kl != 8)
            return fail(HDX_E_BADSIZE, "object %llu: numeric key of %u bytes", (unsigned long long)i, kl);
        if (ko > h.keys_bytes || kl > h.keys_bytes - ko)
            return fail(HDX_E_INVALID, "object %llu: key [%llu,+%u) outside keys of %llu bytes", (unsigned long long)i,
                        (unsigned long long)ko, kl, (unsigned long long)h.keys_bytes);
        if (vo > h.vals_bytes || vl > h.vals_bytes - vo)
            return fail(HDX_E_INVALID, "object %llu: value [%llu,+%u) outside values of %llu bytes",
                        (unsigned long long)i, (unsigned long long)vo, vl, (unsigned long long)h.vals_bytes);
        o.count = 2;
        o.ext[0] = {0, ko, kl};
        o.ext[1] = {vstore, vo, vl};
        return HDX_OK;
    }

    hdx_status upload(HostSlot& sl, const Chunk& c) {
        const StoredObjects so = h.from(c.first).o;  // the chunk's objects: t = 0 .. cnt
        const uint64_t cnt = c.cnt, bytes = c.span ? c.hi[vstore] - c.lo[vstore] : c.payload;
        const uint64_t klo = c.lo[0], vlo = c.lo[vstore], key_bytes = c.hi[0] - klo;
        const uint32_t T = R ? R->T : 0;
        const bool key_span = c.span && !records;  // the key column's span beside the values'
        const bool gather = !c.span && device_packs();
        hdx_status st;
        if ((st = sl.d_blob.need(std::max<uint64_t>(bytes, 1))) != HDX_OK ||
            (key_span && (st = sl.d_keys.need(std::max<uint64_t>(key_bytes, 1))) != HDX_OK) ||
            (st = sl.d_off.need(cnt)) != HDX_OK || (st = sl.d_voff.need(cnt)) != HDX_OK ||
            (st = sl.d_len.need(cnt)) != HDX_OK || (st = sl.d_vlen.need(cnt)) != HDX_OK ||
            (st = sl.d_coords.need(cnt * A)) != HDX_OK || (st = sl.d_ver.need(cnt)) != HDX_OK ||
            (st = sl.d_status.need(1)) != HDX_OK || (st = sl.h_status.need(1)) != HDX_OK ||
            (T && (st = sl.d_ids.need(cnt * T)) != HDX_OK) || (st = sl.h_off.need(cnt)) != HDX_OK ||
            (st = sl.h_voff.need(cnt)) != HDX_OK)
            return st;
        const uint8_t *src_vals = nullptr, *src_keys = nullptr;
        if (c.span) {
            for (uint64_t t = 0; t < cnt; ++t) {
                sl.h_off.p[t] = so.key_off[t] - klo;
                sl.h_voff.p[t] = so.val_off[t] - vlo;
            }
            if ((st = pinned_or_staged(so.vals + vlo, vals_pinned, sl.h_blob, bytes, &src_vals)) != HDX_OK) return st;
            if (key_span &&
                (st = pinned_or_staged(so.keys + klo, keys_pinned, sl.h_keys, key_bytes, &src_keys)) != HDX_OK)
                return st;
        } else {
            uint64_t at = 0;  // record t: its key at h_off, its value right after
            for (uint64_t t = 0; t < cnt; ++t) {
                sl.h_off.p[t] = at;
                sl.h_voff.p[t] = at + so.key_len[t];
                at += (uint64_t)so.key_len[t] + so.val_len[t];
            }
            if (gather) {  // 2 extents per object, absolute device-view sources
                if ((st = sl.h_src.need(2 * cnt)) != HDX_OK || (st = sl.h_sz.need(2 * cnt)) != HDX_OK ||
                    (st = sl.h_dst.need(2 * cnt)) != HDX_OK || (st = sl.d_src.need(2 * cnt)) != HDX_OK ||
                    (st = sl.d_sz.need(2 * cnt)) != HDX_OK || (st = sl.d_dst.need(2 * cnt)) != HDX_OK)
                    return st;
                for (uint64_t t = 0; t < cnt; ++t) {
                    sl.h_src.p[2 * t] = (uint64_t)(uintptr_t)keys_dev + so.key_off[t];
                    sl.h_sz.p[2 * t] = so.key_len[t];
                    sl.h_dst.p[2 * t] = sl.h_off.p[t];
                    sl.h_src.p[2 * t + 1] = (uint64_t)(uintptr_t)vals_dev + so.val_off[t];
                    sl.h_sz.p[2 * t + 1] = so.val_len[t];
                    sl.h_dst.p[2 * t + 1] = sl.h_voff.p[t];
                }
            } else {  // pageable: each key and value copied into the pinned staging
                if ((st = sl.h_blob.need(std::max<uint64_t>(bytes, 1))) != HDX_OK) return st;
                for (uint64_t t = 0; t < cnt; ++t) {
                    std::memcpy(sl.h_blob.p + sl.h_off.p[t], so.keys + so.key_off[t], so.key_len[t]);
                    std::memcpy(sl.h_blob.p + sl.h_voff.p[t], so.vals + so.val_off[t], so.val_len[t]);
                }
                src_vals = sl.h_blob.p;
            }
        }
        const uint32_t *src_klen, *src_vlen;
        if ((st = pinned_or_staged(so.key_len, klen_pinned, sl.h_len, cnt, &src_klen)) != HDX_OK ||
            (st = pinned_or_staged(so.val_len, vlen_pinned, sl.h_vlen, cnt, &src_vlen)) != HDX_OK)
            return st;
        const SmallCopy small[] = {{sl.h_off.p, sl.d_off.p, cnt * 8},          {sl.h_voff.p, sl.d_voff.p, cnt * 8},
                                   {src_klen, sl.d_len.p, cnt * 4},            {src_vlen, sl.d_vlen.p, cnt * 4},
                                   {sl.h_src.p, sl.d_src.p, 2 * cnt * 8},      {sl.h_sz.p, sl.d_sz.p, 2 * cnt * 4},
                                   {sl.h_dst.p, sl.d_dst.p, 2 * cnt * 8}};  // the last three: a gather's extents
        if ((st = copy_small(small, gather ? 7 : 4, gather, sl.s)) != HDX_OK) return st;
        if (gather) {
            HIP_TRY(launch_gather_extents(nullptr, sl.d_src.p, sl.d_sz.p, sl.d_dst.p, sl.d_blob.p, 2 * cnt, sl.s));
        } else {
            HIP_TRY(hipMemcpyAsync(sl.d_blob.p, src_vals, bytes, hipMemcpyHostToDevice, sl.s));
            if (key_span) HIP_TRY(hipMemcpyAsync(sl.d_keys.p, src_keys, key_bytes, hipMemcpyHostToDevice, sl.s));
        }
        return HDX_OK;
    }

    hdx_status launch(HostSlot& sl, const Chunk& c) {
        HIP_TRY(hipMemsetAsync(sl.d_status.p, 0, 4, sl.s));
        // a packed chunk's device layout is records; the coordinates are
        // always staged, so the regions form needs no scratch
        const uint8_t* d_keys = records || !c.span ? sl.d_blob.p : sl.d_keys.p;
        const StoredObjects staged{d_keys, sl.d_off.p, sl.d_len.p, sl.d_blob.p, sl.d_voff.p, sl.d_vlen.p};
        EncodedArgs a;
        const hdx_status st = encoded_args(a, codes, A, staged, c.cnt, sl.d_coords.p, sl.d_ver.p, sl.d_status.p,
                                           R ? R->tables : nullptr, R ? R->T : 0, sl.d_ids.p, c.cnt, dev);
        if (st != HDX_OK) return st;
        HIP_TRY(launch_hash_encoded(a, sl.s));
        return HDX_OK;
    }
};

}  // namespace

hdx_status hash_host(const uint8_t* codes, uint32_t A, const uint8_t* blob, uint64_t blob_bytes,
                     const uint64_t* obj_base, const uint32_t* attr_len, uint64_t n, uint64_t* coords,
                     const HostRegions* R) {
    HostSlot* slots;
    const hdx_status st = thread_slots(&slots);
    if (st != HDX_OK) return st;
    PackedSource src{codes, A, blob, blob_bytes, obj_base, attr_len, R};
    return run_chunks(slots, src, n, Outputs(A, coords, R), nullptr);
}

hdx_status hash_encoded_host(const uint8_t* codes, uint32_t A, const StoredHost& h, uint64_t n, uint64_t* coords,
                             uint64_t* versions, const HostRegions* R, uint32_t* status_bits) {
    *status_bits = 0;
    HostSlot* slots;
    const hdx_status st = thread_slots(&slots);
    if (st != HDX_OK) return st;
    StoredSource src{codes, A, h, R};
    return run_chunks(slots, src, n, Outputs(A, coords, R, versions), status_bits);
}

}  // namespace hdx

using namespace hdx;

// ---- exported -----------------------------------------------------------------------

static const uint8_t g_empty = 0;  // a blob / store of 0 bytes

HDX_EXPORT hdx_status hdx_hash_batch_host(const uint32_t* types, uint32_t attrs_sz, const uint8_t* blob,
                                          uint64_t blob_bytes, const uint64_t* obj_base, const uint32_t* attr_len,
                                          uint64_t n, uint64_t* coords) {
    std::vector<uint8_t> codes(attrs_sz ? attrs_sz : 1);
    hdx_status st = check_schema(types, attrs_sz, codes.data());
    if (st != HDX_OK) return st;
    if (n == 0) return HDX_OK;
    if (!obj_base || !attr_len || !coords || (!blob && blob_bytes)) return fail(HDX_E_INVALID, "NULL host pointer");
    return hash_host_any(codes.data(), attrs_sz, blob ? blob : &g_empty, blob_bytes, obj_base, attr_len, n, coords,
                         nullptr);
}

HDX_EXPORT hdx_status hdx_hash_batch_regions_host(const uint32_t* types, uint32_t attrs_sz, const uint8_t* blob,
                                                  uint64_t blob_bytes, const uint64_t* obj_base,
                                                  const uint32_t* attr_len, uint64_t n, const hdx_region_table* tables,
                                                  uint32_t ntables, uint64_t* region_ids, uint64_t* coords) {
    if (ntables == 0) return fail(HDX_E_INVALID, "no region tables");
    std::vector<uint8_t> codes(attrs_sz ? attrs_sz : 1);
    hdx_status st = check_schema(types, attrs_sz, codes.data());
    if (st != HDX_OK) return st;
    if ((st = check_tables(tables, ntables, attrs_sz, region_ids)) != HDX_OK) return st;
    if (n == 0) return HDX_OK;
    if (!obj_base || !attr_len || (!blob && blob_bytes)) return fail(HDX_E_INVALID, "NULL host pointer");
    const HostRegions R{tables, ntables, region_ids, n};
    return hash_host_any(codes.data(), attrs_sz, blob ? blob : &g_empty, blob_bytes, obj_base, attr_len, n, coords,
                         &R);
}

static hdx_status encoded_host(const uint32_t* types, uint32_t attrs_sz, StoredHost h, uint64_t n,
                               const hdx_region_table* tables, uint32_t ntables, uint64_t* region_ids,
                               uint64_t* coords, uint64_t* versions) {
    std::vector<uint8_t> codes(attrs_sz ? attrs_sz : 1);
    hdx_status st = check_schema(types, attrs_sz, codes.data());
    if (st != HDX_OK) return st;
    if ((st = check_tables(tables, ntables, attrs_sz, region_ids)) != HDX_OK) return st;
    if (n == 0) return HDX_OK;
    if (!has_columns(h.o, SO_ALL & ~(SO_KEYS | SO_VALS)) || (!coords && !ntables) || (!h.o.keys && h.keys_bytes) ||
        (!h.o.vals && h.vals_bytes))
        return fail(HDX_E_INVALID, "NULL host pointer");
    if (!h.o.keys) h.o.keys = &g_empty;  // a store of 0 bytes
    if (!h.o.vals) h.o.vals = &g_empty;
    const HostRegions R{tables, ntables, region_ids, n};
    return hash_encoded_host_any(codes.data(), attrs_sz, h, n, coords, versions, ntables ? &R : nullptr);
}

HDX_EXPORT hdx_status hdx_hash_encoded_host(const uint32_t* types, uint32_t attrs_sz, const uint8_t* keys,
                                            uint64_t keys_bytes, const uint64_t* key_off, const uint32_t* key_len,
                                            const uint8_t* vals, uint64_t vals_bytes, const uint64_t* val_off,
                                            const uint32_t* val_len, uint64_t n, uint64_t* coords,
                                            uint64_t* versions) {
    const StoredObjects so{keys, key_off, key_len, vals, val_off, val_len};
    return encoded_host(types, attrs_sz, {so, keys_bytes, vals_bytes}, n, nullptr, 0, nullptr, coords, versions);
}

HDX_EXPORT hdx_status hdx_hash_encoded_regions_host(const uint32_t* types, uint32_t attrs_sz, const uint8_t* keys,
                                                    uint64_t keys_bytes, const uint64_t* key_off,
                                                    const uint32_t* key_len, const uint8_t* vals, uint64_t vals_bytes,
                                                    const uint64_t* val_off, const uint32_t* val_len, uint64_t n,
                                                    const hdx_region_table* tables, uint32_t ntables,
                                                    uint64_t* region_ids, uint64_t* coords, uint64_t* versions) {
    if (ntables == 0) return fail(HDX_E_INVALID, "no region tables");
    const StoredObjects so{keys, key_off, key_len, vals, val_off, val_len};
    return encoded_host(types, attrs_sz, {so, keys_bytes, vals_bytes}, n, tables, ntables, region_ids, coords, versions);
}
