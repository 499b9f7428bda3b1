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
//   scan     scan_exclusive (hdx_scratch.hip) over those counts.
//   compact  check_compact_kernel: the same workgroups re-read first_fail,
//            rank the passing objects inside the workgroup (block_ranks) and
//            store their indices at the workgroup's scanned base; the last
//            workgroup stores the total.  No kernel waits on another
//            workgroup, no atomic hands out positions: match is ascending.
//
// The per-object step and its loads are hdx_check_eval.h's, shared with
// sorted_rank_kernel (hdx_sorted.hip).
// Not -ffast-math (Makefile): the FLOAT comparison's NaN behaviour is IEEE's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdint.h>

#include "hdx_check_eval.h"
#include "hdx_internal.h"

namespace hdx {

namespace {

// Dynamic LDS: the checks' (check_lds_carve, hdx_check_eval.h), for a list
// with OP_REGEX ops their byte-class tables (regex_lds_bytes), then the waves'
// pass counts.  RXA: nothing — the one-shot entry points' kernel, and a
// compiled list's without OP_REGEX ops — or RegexArgs, a third kernel argument.
template <typename... RXA>
__global__ void __launch_bounds__(kCheckBlock) check_kernel(const CheckArgs a, uint64_t* block_pass, const RXA... rx) {
    extern __shared__ __attribute__((aligned(16))) uint64_t check_lds[];
    constexpr uint32_t B = kCheckBlock;
    constexpr bool RX = sizeof...(RXA) != 0;
    const uint32_t c = a.c, tid = threadIdx.x;
    uint32_t* s_cnt;
    const CheckLds s = check_lds_carve<B>(check_lds, c, &s_cnt);
    RegexLds rl{};
    check_lds_init<B>(a, s);
    if constexpr (RX) s_cnt = regex_lds_init<B>(rl, rx..., s_cnt);
    const uint64_t i = (uint64_t)blockIdx.x * B + tid;
    bool badenc = false, pass = false;
    if (i < a.n) {
        const uint32_t ff = check_object<B, RX>(a, s, rl, i, [](uint32_t, uint32_t, uint32_t) {});
        badenc = ff == HDX_CHECK_BADENC;
        pass = ff == c;
        a.first_fail[i] = ff;
    }
    wave_status_or(a.status, badenc, kStatusBadEnc);
    if (block_pass) {
        uint32_t rank[1], all[1];
        block_ranks<B, 1>({pass}, s_cnt, rank, all);
        if (tid == 0) block_pass[blockIdx.x] = all[0];
    }
}

// block_base: the workgroups' pass counts, scanned (exclusive).
__global__ void __launch_bounds__(kCheckBlock) check_compact_kernel(const CheckArgs a, const uint64_t* block_base) {
    __shared__ uint32_t s_cnt[kCheckBlock / 64];
    constexpr uint32_t B = kCheckBlock;
    const uint32_t tid = threadIdx.x;
    const uint64_t i = (uint64_t)blockIdx.x * B + tid;
    const bool pass = i < a.n && a.first_fail[i] == a.c;
    uint32_t rank[1], all[1];
    block_ranks<B, 1>({pass}, s_cnt, rank, all);
    const uint64_t base = block_base[blockIdx.x];
    if (pass) a.match[base + rank[0]] = i;
    if (blockIdx.x == gridDim.x - 1 && tid == 0) *a.match_count = base + all[0];
}

}  // namespace

hipError_t launch_check_encoded(const CheckArgs& a, hipStream_t stream, bool* no_scratch, const RegexArgs* rx) {
    static_assert(check_lds_bytes(kCheckBlock, HDX_MAX_CHECKS) + regex_lds_bytes(HDX_MAX_REGEX_CHECKS) +
                          (kCheckBlock / 64) * 4 < (64 << 10),
                  "dynamic LDS at c = 16 with every regex op");
    *no_scratch = false;
    const uint64_t blocks = (a.n + kCheckBlock - 1) / kCheckBlock;
    if (blocks > 0x7fffffffULL) return hipErrorInvalidValue;
    if (a.n == 0) return a.match ? hipMemsetAsync(a.match_count, 0, sizeof(uint64_t), stream) : hipSuccess;
    PoolScratch scratch;  // [blocks] | the scan's block sums
    if (a.match && !scratch.acquire((blocks + scan_scratch_words(blocks)) * 8, stream, no_scratch)) return hipSuccess;
    uint64_t* counts = static_cast<uint64_t*>(scratch.p);
    const size_t lds = check_lds_bytes(kCheckBlock, a.c) + (kCheckBlock / 64) * 4;
    if (rx && rx->count)
        hipLaunchKernelGGL(check_kernel<RegexArgs>, dim3((uint32_t)blocks), dim3(kCheckBlock),
                           lds + regex_lds_bytes(rx->count), stream, a, counts, *rx);
    else
        hipLaunchKernelGGL(check_kernel<>, dim3((uint32_t)blocks), dim3(kCheckBlock), lds, stream, a, counts);
    hipError_t e = hipGetLastError();
    if (counts) {
        if (e == hipSuccess) e = scan_exclusive(counts, blocks, counts + blocks, stream);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(check_compact_kernel, dim3((uint32_t)blocks), dim3(kCheckBlock), 0, stream, a,
                               (const uint64_t*)counts);
            e = hipGetLastError();
        }
    }
    return scratch.release(e);
}

}  // namespace hdx
