// hdx_checks.hip — a search's attribute checks over stored objects on gfx950:
// what datalayer::search_iterator::valid() does per candidate object
// (daemon/datalayer_iterator.cc:792-850: decode_value, then
// passes_attribute_checks, common/attribute_check.cc:209-237; the table is
// restated in include/hdxhash.h).  The ops are compile_checks' (hdx_host_common.h):
// everything that does not depend on the object is decided on the host.
//
//   check    check_kernel: a lane per object walks its value (value_walk, the
//            full walk: the verdict is the sweep's at any A), keeps {offset,
//            length} of the attributes the ops name in LDS, then evaluates the
//            ops in order up to the first false one and stores first_fail.
//            With compaction it also stores how many of its workgroup's
//            objects pass.
//   scan     scan_exclusive (hdx_index_entries.hip) over those counts.
//   compact  check_compact_kernel: the same workgroups re-read first_fail,
//            rank the passing objects inside the workgroup (ballots) and
//            store their indices at the workgroup's scanned base; the last
//            workgroup stores the total.  No kernel waits on another
//            workgroup, no atomic hands out positions: match is ascending.
//
// Loads: numerics as one unaligned 8-byte value lying wholly inside the key
// or attribute; strings in 8-byte steps the same way, and the last 1..7 bytes
// as the aligned dwords that hold them (as seg_bytes of hdx_index_entries.hip
// reads a segment's end) — never a dword that holds no byte of the attribute.
// Not -ffast-math (Makefile): the FLOAT comparison's NaN behaviour is IEEE's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdint.h>

#include "hdx_internal.h"
#include "hdx_value_walk.h"

namespace hdx {

namespace {

typedef uint32_t __attribute__((aligned(1))) ck_u32_u;
typedef uint64_t __attribute__((aligned(1))) ck_u64_u;
typedef const __attribute__((address_space(1))) ck_u32_u* ck_gu32_ptr;
typedef const __attribute__((address_space(1))) ck_u64_u* ck_gu64_ptr;
typedef const __attribute__((address_space(1))) uint32_t* ck_g32_ptr;

constexpr uint32_t kKonstWords = kCheckConstBytes / 8;

// The `take` (1..4) bytes at p in the low bytes of the result, the rest zero.
__device__ __forceinline__ uint32_t tail_bytes(const uint8_t* p, uint32_t take) {
    if (take == 4) return *(ck_gu32_ptr)p;
    const uint32_t sh = (uint32_t)(uintptr_t)p & 3;
    const uint8_t* q = p - sh;  // the aligned dword that holds p[0]
    const uint32_t d0 = *(ck_g32_ptr)q;
    const uint32_t d1 = sh + take > 4 ? *(ck_g32_ptr)(q + 4) : 0u;
    return __builtin_amdgcn_alignbyte(d1, d0, sh) & ((1u << (8 * take)) - 1);
}

// compare(k, v) of datatype_string.cc:263-285, k in LDS at 8-byte-aligned kw
// (zero-padded to 8): memcmp over the shorter length as big-endian unsigned
// words, ending at the first differing one, then the lengths.
__device__ __forceinline__ int compare_string(const uint64_t* kw, uint32_t klen, const uint8_t* v, uint32_t vlen) {
    const uint32_t m = std::min(klen, vlen);
    for (uint32_t w = 0; w < m; w += 8) {
        const uint32_t r = m - w;
        uint64_t a = kw[w >> 3], b;
        if (r >= 8) {
            b = *(ck_gu64_ptr)(v + w);
        } else {
            a &= (1ull << (8 * r)) - 1;  // k may go on past the shorter length
            b = tail_bytes(v + w, std::min(r, 4u));
            if (r > 4) b |= (uint64_t)tail_bytes(v + w + 4, r - 4) << 32;
        }
        if (a != b) return __builtin_bswap64(a) < __builtin_bswap64(b) ? -1 : 1;
    }
    return klen < vlen ? -1 : klen > vlen ? 1 : 0;
}

// One op on the attribute (or key) of len bytes at p: passes_attribute_check
// :141-199 past what compile_checks decided.
__device__ __forceinline__ bool eval_op(const CheckOp& o, const uint64_t* s_konst, const uint8_t* p, uint32_t len) {
    if (o.op >= OP_LEN_EQ) {  // :178-199, T == STRING: length(v) = its size
        const int64_t L = (int64_t)len, tmp = (int64_t)o.imm;
        return o.op == OP_LEN_EQ ? L == tmp : o.op == OP_LEN_LE ? L <= tmp : L >= tmp;
    }
    int cmp;
    if (o.family == FAM_STRING) {
        if (o.op == OP_EQ && len != o.klen) return false;  // compare == 0 needs equal lengths
        cmp = compare_string(s_konst + (o.koff >> 3), o.klen, p, len);
    } else {
        if (len != 0 && len != 8) return false;  // :141 validate(v): fails every check, no status bit
        const uint64_t vb = len ? *(ck_gu64_ptr)p : 0;  // an empty value is 0 / 0.0
        if (o.family == FAM_INT64) {
            const int64_t k = (int64_t)o.imm, v = (int64_t)vb;
            cmp = k < v ? -1 : k > v ? 1 : 0;
        } else {  // datatype_float.cc:256-273: a NaN on either side gives 0
            const double k = __longlong_as_double((long long)o.imm), v = __longlong_as_double((long long)vb);
            cmp = k < v ? -1 : k > v ? 1 : 0;
        }
    }
    return check_relation(o.op, cmp);
}

// Dynamic LDS, in this order: the constants (u64[kKonstWords]), off[c][B],
// len[c][B] (lane-minor: no bank conflicts), then the waves' pass counts.
__global__ void __launch_bounds__(kCheckBlock) check_kernel(const CheckArgs a, uint64_t* block_pass) {
    extern __shared__ __attribute__((aligned(16))) uint64_t check_lds[];
    constexpr uint32_t B = kCheckBlock;
    const uint32_t c = a.c, tid = threadIdx.x;
    uint64_t* s_konst = check_lds;
    uint32_t* s_off = reinterpret_cast<uint32_t*>(s_konst + kKonstWords);
    uint32_t* s_len = s_off + B * c;
    uint32_t* s_cnt = s_len + B * c;
    uint32_t konst_words = 0;  // what the ops use
    for (uint32_t k = 0; k < c; ++k)
        if (a.op[k].op != OP_NEVER && a.op[k].op < OP_LEN_EQ && a.op[k].family == FAM_STRING)
            konst_words = std::max(konst_words, (a.op[k].koff + a.op[k].klen + 7) >> 3);
    for (uint32_t t = tid; t < konst_words; t += B) s_konst[t] = a.konst[t];
    for (uint32_t k = 0; k < c; ++k) {
        s_off[k * B + tid] = 0;
        s_len[k * B + tid] = 0;
    }
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * B + tid;
    bool badenc = false, pass = false;
    if (i < a.n) {
        const uint8_t* v = a.vals + a.val_off[i];
        const bool ok = value_walk(v, a.val_len[i], a.A, [&](uint32_t j, uint32_t pos, uint32_t L) {
            for (uint32_t k = 0; k < c; ++k)  // uniform: the ops are kernel arguments
                if (a.op[k].attr == j) {      // attr 0 (the key, OP_NEVER) never equals j >= 1
                    s_off[k * B + tid] = pos;
                    s_len[k * B + tid] = L;
                }
        });
        badenc = !ok;
        uint32_t ff = HDX_CHECK_BADENC;
        if (ok) {
            ff = c;
            const uint8_t* key = a.keys + a.key_off[i];
            const uint32_t kl = a.key_len[i];
            for (uint32_t k = 0; k < c; ++k) {  // uniform; lanes leave at their first false op
                const CheckOp& o = a.op[k];
                bool t = false;
                if (o.op != OP_NEVER) {
                    const bool on_key = o.attr == 0;
                    t = eval_op(o, s_konst, on_key ? key : v + s_off[k * B + tid], on_key ? kl : s_len[k * B + tid]);
                }
                if (!t) {
                    ff = k;
                    break;
                }
            }
            pass = ff == c;
        }
        a.first_fail[i] = ff;
    }
    if (a.status && __any(badenc) && (tid & 63) == 0) atomicOr(a.status, 1u << 6 /* HDX_E_BADENC */);
    if (block_pass) {
        const uint32_t cnt = (uint32_t)__popcll(__ballot(pass));
        if ((tid & 63) == 0) s_cnt[tid >> 6] = cnt;
        __syncthreads();
        if (tid == 0) {
            uint32_t all = 0;
            for (uint32_t w = 0; w < B / 64; ++w) all += s_cnt[w];
            block_pass[blockIdx.x] = all;
        }
    }
}

// block_base: the workgroups' pass counts, scanned (exclusive).
__global__ void __launch_bounds__(kCheckBlock) check_compact_kernel(const CheckArgs a, const uint64_t* block_base) {
    __shared__ uint32_t s_cnt[kCheckBlock / 64];
    constexpr uint32_t B = kCheckBlock;
    const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const uint64_t i = (uint64_t)blockIdx.x * B + tid;
    const bool pass = i < a.n && a.first_fail[i] == a.c;
    const uint64_t mask = __ballot(pass);
    if (lane == 0) s_cnt[w] = (uint32_t)__popcll(mask);
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (uint32_t u = 0; u < B / 64; ++u) {
        const uint32_t s = s_cnt[u];
        if (u < w) before += s;
        all += s;
    }
    const uint64_t base = block_base[blockIdx.x];
    if (pass) a.match[base + before + (uint32_t)__popcll(mask & ((1ull << lane) - 1))] = i;
    if (blockIdx.x == gridDim.x - 1 && tid == 0) *a.match_count = base + all;
}

}  // namespace

hipError_t launch_check_encoded(const CheckArgs& a, hipStream_t stream, bool* no_scratch) {
    *no_scratch = false;
    const uint64_t blocks = (a.n + kCheckBlock - 1) / kCheckBlock;
    if (blocks > 0x7fffffffULL) return hipErrorInvalidValue;
    if (a.n == 0) return a.match ? hipMemsetAsync(a.match_count, 0, sizeof(uint64_t), stream) : hipSuccess;
    uint64_t* counts = nullptr;  // [blocks] | the scan's block sums
    if (a.match) {
        hipMemPool_t pool = nullptr;
        hipError_t e = scratch_pool(&pool);
        if (e == hipSuccess)
            e = hipMallocFromPoolAsync((void**)&counts, (blocks + scan_scratch_words(blocks)) * 8, pool, stream);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            *no_scratch = true;
            return hipSuccess;
        }
    }
    const size_t lds = kCheckConstBytes + (size_t)kCheckBlock * a.c * 8 + (kCheckBlock / 64) * 4;
    hipLaunchKernelGGL(check_kernel, dim3((uint32_t)blocks), dim3(kCheckBlock), lds, stream, a, counts);
    hipError_t e = hipGetLastError();
    if (counts) {
        if (e == hipSuccess) e = scan_exclusive(counts, blocks, counts + blocks, stream);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(check_compact_kernel, dim3((uint32_t)blocks), dim3(kCheckBlock), 0, stream, a,
                               (const uint64_t*)counts);
            e = hipGetLastError();
        }
        const hipError_t f = hipFreeAsync(counts, stream);
        if (e == hipSuccess) e = f;
    }
    return e;
}

}  // namespace hdx
