// hdx_sorted.hip — the top-limit matching objects by one attribute on gfx950:
// what search_manager::sorted_search (daemon/search_manager.cc:305-502) does
// with the objects datalayer::search_iterator::valid() lets through, under
// the contract of include/hdxhash.h (hdx_sorted_search_device): which end is
// kept and the output's direction are two arguments, ties go by index.
//
//   rank     sorted_rank_kernel: check_kernel's per-object step (check_object,
//            hdx_check_eval.h; one walk), then for a matching object a 64-bit
//            rank key that is monotone in datatype_*::compare — INT64 and
//            TIMESTAMP_* x ^ 2^63; FLOAT the sign transform after -0.0 -> +0.0,
//            NaN -> all ones; STRING the first 8 bytes big-endian, zero-padded;
//            0 where every object ties — and a member byte.  A matching object
//            whose numeric sort value has neither 0 nor 8 bytes is no member.
//   select   eight rounds of sorted_hist_kernel (the members whose key agrees
//            with the running prefix, counted by the next 8 bits: LDS atomics,
//            then one global add per non-empty bin and workgroup) and
//            sorted_pick_kernel (one workgroup finds the bin that holds the
//            k-th key, k = min(limit, members), and leaves prefix, members
//            strictly before it and the rest still needed in device memory).
//            KEEP_LARGEST selects on the complemented key.  Integer adds only:
//            the bins do not depend on the order of arrival.
//   compact  sorted_count_kernel, scan_exclusive over the workgroups' {before,
//            equal} counts, sorted_compact_kernel: the candidates' indices in
//            index order — every key strictly before the threshold, and of the
//            equal ones the first `needed` by index (numeric keys: equal keys
//            are true ties) or all of them (STRING: equal keys share 8 bytes
//            and nothing more).
//   finish   sorted_finish_kernel, one workgroup: rounds of kSortFinishBlock
//            candidates merged with the best so far by a bitonic sort on (key,
//            for STRING compare of the stored strings, index) — a round none
//            of whose candidates enters the best `limit` is skipped; a last sort
//            where the output runs against the kept order; top, top_count.
//
// No kernel waits on another workgroup and no atomic hands out positions, so
// the result never varies.  Loads follow hdx_check_eval.h's rule.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdint.h>

#include "hdx_check_eval.h"
#include "hdx_internal.h"

namespace hdx {

namespace {

constexpr uint32_t kBins = 256, kPasses = 8;
constexpr uint32_t kHistBlocks = 1024;  // the grid of a histogram pass: at most this many adds per bin
constexpr uint64_t kEmpty = ~0ull;      // no candidate in this slot of the finishing sort

// What the select leaves for the kernels behind it (zeroed per call).
struct SortState {
    uint64_t prefix;   // the threshold's bits found so far (select space)
    uint64_t need;     // of the keys that agree with prefix, how many are still to be kept
    uint64_t inside;   // members strictly before the prefix
    uint64_t kept;     // min(limit, members)
    uint64_t ncand;    // candidates the compaction wrote
    uint64_t pad_[3];
};
struct SortScratch {
    uint64_t* bins;    // [kPasses][kBins]
    SortState* state;
    uint64_t* rank;    // [n]
    uint64_t* cand;    // [n]
    uint64_t* counts;  // [2 * blocks] | the scan's block sums
    uint8_t* member;   // [n]
};
constexpr uint64_t kHeadWords = kPasses * kBins + sizeof(SortState) / 8;

__device__ __forceinline__ uint64_t rank_float(uint64_t bits) {
    if ((bits & 0x7fffffffffffffffull) > 0x7ff0000000000000ull) return ~0ull;  // every NaN: above +inf
    if ((bits << 1) == 0) bits = 0;                                            // -0.0 ties with 0.0
    return (bits >> 63) ? ~bits : bits | 0x8000000000000000ull;
}

// Dynamic LDS: the checks' (check_lds_carve), for a list with OP_REGEX ops
// their byte-class tables (regex_lds_bytes).  RXA: nothing — the one-shot
// entry point's kernel, and a compiled list's without OP_REGEX ops — or
// RegexArgs, a fourth kernel argument.
template <typename... RXA>
__global__ void __launch_bounds__(kCheckBlock) sorted_rank_kernel(const SortedArgs a, uint64_t* rank, uint8_t* member,
                                                                  const RXA... rx) {
    extern __shared__ __attribute__((aligned(16))) uint64_t rank_lds[];
    constexpr uint32_t B = kCheckBlock;
    constexpr bool RX = sizeof...(RXA) != 0;
    const CheckArgs& ck = a.ck;
    const uint32_t tid = threadIdx.x;
    uint32_t* end;
    const CheckLds s = check_lds_carve<B>(rank_lds, ck.c, &end);
    RegexLds rl{};
    check_lds_init<B>(ck, s);
    if constexpr (RX) regex_lds_init<B>(rl, rx..., end);
    const uint64_t i = (uint64_t)blockIdx.x * B + tid;
    bool badenc = false, badsize = false;
    if (i < ck.n) {
        uint32_t spos = 0, slen = 0;
        const uint32_t sattr = a.attr;
        const uint32_t ff = check_object<B, RX>(ck, s, rl, i, [&](uint32_t j, uint32_t pos, uint32_t L) {
            if (j == sattr) {
                spos = pos;
                slen = L;
            }
        });
        badenc = ff == HDX_CHECK_BADENC;
        if (ck.first_fail) ck.first_fail[i] = ff;
        bool in = ff == ck.c;
        uint64_t r = 0;
        if (in && a.kind != SORT_TIE) {
            const uint8_t* p;
            if (sattr == 0) {
                p = ck.keys + ck.key_off[i];
                slen = ck.key_len[i];
            } else {
                p = ck.vals + ck.val_off[i] + spos;
            }
            if (a.kind == SORT_STRING) {
                if (slen) r = __builtin_bswap64(word_bytes(p, std::min(slen, 8u)));
            } else if (slen != 0 && slen != 8) {  // the reference's unpack asserts
                in = false;
                badsize = true;
            } else {
                const uint64_t bits = slen ? *(gu64_ptr)p : 0;  // an empty value is 0 / 0.0
                r = a.kind == SORT_INT64 ? bits ^ 0x8000000000000000ull : rank_float(bits);
            }
        }
        rank[i] = r;
        member[i] = in ? 1 : 0;
    }
    wave_status_or(ck.status, (__any(badenc) ? kStatusBadEnc : 0) | (__any(badsize) ? kStatusBadSize : 0));
}

// Pass p counts the members that agree with state->prefix above bit 64 - 8p
// by their next 8 bits.
__global__ void __launch_bounds__(256) sorted_hist_kernel(const uint64_t* rank, const uint8_t* member, uint64_t n,
                                                          uint64_t flip, uint32_t pass, const SortState* state,
                                                          uint64_t* bins) {
    __shared__ uint32_t s_hist[kBins];
    const uint32_t tid = threadIdx.x;
    s_hist[tid] = 0;
    __syncthreads();
    if (pass == 0 || state->kept != 0) {
        const uint64_t prefix = state->prefix;
        const uint32_t shift = 56 - 8 * pass;
        const uint64_t stride = (uint64_t)gridDim.x * 256;
        for (uint64_t i = (uint64_t)blockIdx.x * 256 + tid; i < n; i += stride) {
            const uint64_t k = rank[i] ^ flip;
            const bool on = member[i] != 0 && (pass == 0 || ((k ^ prefix) >> (shift + 8)) == 0);
            if (on) {
                const uint32_t d = (uint32_t)(k >> shift) & 0xff;
                // a wave whose lanes all count the same bin (clustered keys) adds once
                const uint64_t act = __ballot(1);
                const uint32_t d0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)d);
                if (__ballot(d == d0) == act) {
                    if ((uint32_t)__popcll(act & ((1ull << (tid & 63)) - 1)) == 0)
                        atomicAdd(&s_hist[d0], (uint32_t)__popcll(act));
                } else {
                    atomicAdd(&s_hist[d], 1u);
                }
            }
        }
    }
    __syncthreads();
    const uint32_t h = s_hist[tid];
    if (h) atomicAdd((unsigned long long*)&bins[pass * kBins + tid], (unsigned long long)h);
}

__global__ void __launch_bounds__(kBins) sorted_pick_kernel(const uint64_t* bins, uint32_t pass, uint64_t limit,
                                                            SortState* state) {
    __shared__ uint64_t s_bin[kBins];
    s_bin[threadIdx.x] = bins[pass * kBins + threadIdx.x];
    __syncthreads();
    if (threadIdx.x != 0) return;
    uint64_t need = state->need;
    if (pass == 0) {
        uint64_t total = 0;
        for (uint32_t d = 0; d < kBins; ++d) total += s_bin[d];
        need = std::min(limit, total);
        state->kept = need;
    }
    if (state->kept == 0) return;
    // 1 <= need <= the keys that agree with the prefix: the loop ends inside the bins
    uint64_t before = 0;
    uint32_t d = 0;
    for (; d < kBins - 1; ++d) {
        if (before + s_bin[d] >= need) break;
        before += s_bin[d];
    }
    state->prefix |= (uint64_t)d << (56 - 8 * pass);
    state->inside += before;
    state->need = need - before;
}

// flag[kBefore] / flag[kEqual]: member i's key lies strictly before the
// threshold / on it.  Ranked as two flags behind one barrier (block_ranks).
enum : uint32_t { kBefore = 0, kEqual = 1 };
__device__ __forceinline__ void candidate_flags(const uint64_t* rank, const uint8_t* member, uint64_t n, uint64_t i,
                                                uint64_t flip, const SortState* state, bool (&flag)[2]) {
    flag[kBefore] = flag[kEqual] = false;
    if (i < n && state->kept != 0 && member[i]) {
        const uint64_t k = rank[i] ^ flip, T = state->prefix;
        flag[kBefore] = k < T;
        flag[kEqual] = k == T;
    }
}

// counts[b] = workgroup b's keys before the threshold, counts[blocks + b] = its keys on it.
__global__ void __launch_bounds__(kCheckBlock) sorted_count_kernel(const uint64_t* rank, const uint8_t* member,
                                                                   uint64_t n, uint64_t flip, const SortState* state,
                                                                   uint64_t* counts) {
    __shared__ uint32_t s_cnt[2 * kCheckBlock / 64];
    bool flag[2];
    candidate_flags(rank, member, n, (uint64_t)blockIdx.x * kCheckBlock + threadIdx.x, flip, state, flag);
    uint32_t r[2], all[2];
    block_ranks<kCheckBlock, 2>(flag, s_cnt, r, all);
    if (threadIdx.x == 0) {
        counts[blockIdx.x] = all[kBefore];
        counts[gridDim.x + blockIdx.x] = all[kEqual];
    }
}

// base: the counts, scanned (exclusive) as one array of 2 * blocks elements:
// base[blocks] is the number of keys before the threshold.  all_equal: STRING.
__global__ void __launch_bounds__(kCheckBlock) sorted_compact_kernel(const uint64_t* rank, const uint8_t* member,
                                                                     uint64_t n, uint64_t flip, uint32_t all_equal,
                                                                     SortState* state, const uint64_t* base,
                                                                     uint64_t* cand) {
    const uint64_t i = (uint64_t)blockIdx.x * kCheckBlock + threadIdx.x;
    __shared__ uint32_t s_cnt[2 * kCheckBlock / 64];
    bool flag[2];
    candidate_flags(rank, member, n, i, flip, state, flag);
    uint32_t r[2], all[2];
    block_ranks<kCheckBlock, 2>(flag, s_cnt, r, all);
    const uint64_t take = all_equal ? ~0ull : state->need;  // of the equal keys, in index order
    const uint64_t b0 = base[blockIdx.x], e0 = base[gridDim.x + blockIdx.x] - base[gridDim.x];
    const uint64_t eq_before = e0 + r[kEqual];
    // positions: every candidate with a smaller index comes first; at most n in all
    if (flag[kBefore] || (flag[kEqual] && eq_before < take)) cand[b0 + r[kBefore] + std::min(eq_before, take)] = i;
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0)
        state->ncand = b0 + all[kBefore] + std::min(e0 + all[kEqual], take);
}

// ---- finish ------------------------------------------------------------------

constexpr uint32_t kSlots = 2 * kSortFinishBlock;

struct FinishLds {
    uint64_t key[kSlots];  // select space
    uint64_t idx[kSlots];  // kEmpty: no candidate
    uint64_t off[kSlots];  // STRING: the sort value's offset in keys / vals
    uint32_t len[kSlots];
};

// compare(x, y) of datatype_string.cc:263-285 for two stored strings whose
// first 8 bytes, zero-padded, are equal.
__device__ __forceinline__ int compare_stored(const uint8_t* p, uint32_t pl, const uint8_t* q, uint32_t ql) {
    const uint32_t m = std::min(pl, ql);
    for (uint32_t w = 8; w < m; w += 8) {
        const uint32_t r = std::min(m - w, 8u);
        const uint64_t x = word_bytes(p + w, r), y = word_bytes(q + w, r);
        if (x != y) return __builtin_bswap64(x) < __builtin_bswap64(y) ? -1 : 1;
    }
    return pl < ql ? -1 : pl > ql ? 1 : 0;
}

// Slot x sorts before slot y: empty slots last; the value in the kept order
// (rev: against it); then the index, ascending either way.
__device__ __forceinline__ bool slot_before(const FinishLds& s, uint32_t x, uint32_t y, const uint8_t* strings,
                                            bool largest, bool rev) {
    const uint64_t ix = s.idx[x], iy = s.idx[y];
    if (ix == kEmpty || iy == kEmpty) return ix != kEmpty;
    const uint64_t kx = s.key[x], ky = s.key[y];
    int c = kx < ky ? -1 : kx > ky ? 1 : 0;
    if (c == 0 && strings) {
        c = compare_stored(strings + s.off[x], s.len[x], strings + s.off[y], s.len[y]);
        if (largest) c = -c;
    }
    if (rev) c = -c;
    return c ? c < 0 : ix < iy;
}

// A bitonic sort of slots [0, N), N a power of two <= kSlots, by every thread of the workgroup.
__device__ __forceinline__ void bitonic(FinishLds& s, uint32_t N, const uint8_t* strings, bool largest, bool rev) {
    const uint32_t t = threadIdx.x;
    for (uint32_t k = 2; k <= N; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            if (t < N / 2) {
                const uint32_t lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
                const bool up = (lo & k) == 0;
                if (slot_before(s, hi, lo, strings, largest, rev) == up) {
                    const uint64_t a = s.key[lo], b = s.idx[lo], c = s.off[lo];
                    const uint32_t d = s.len[lo];
                    s.key[lo] = s.key[hi];
                    s.idx[lo] = s.idx[hi];
                    s.off[lo] = s.off[hi];
                    s.len[lo] = s.len[hi];
                    s.key[hi] = a;
                    s.idx[hi] = b;
                    s.off[hi] = c;
                    s.len[hi] = d;
                }
            }
            __syncthreads();
        }
}

__global__ void __launch_bounds__(kSortFinishBlock) sorted_finish_kernel(const SortedArgs a, const uint64_t* rank,
                                                                         const uint64_t* cand, const SortState* state,
                                                                         uint64_t flip) {
    __shared__ FinishLds s;
    const CheckArgs& ck = a.ck;
    const uint32_t t = threadIdx.x;
    const bool largest = a.keep == HDX_KEEP_LARGEST;
    const uint8_t* strings = a.kind != SORT_STRING ? nullptr : a.attr == 0 ? ck.keys : ck.vals;
    const uint64_t ncand = state->ncand, kept = state->kept;  // kept <= limit <= kSortFinishBlock
    s.idx[t] = kEmpty;
    for (uint64_t first = 0; first < ncand; first += kSortFinishBlock) {
        const uint32_t slot = kSortFinishBlock + t;
        uint64_t i = kEmpty;
        if (first + t < ncand) {
            i = cand[first + t];
            s.key[slot] = rank[i] ^ flip;
            if (strings) {
                if (a.attr == 0) {
                    s.off[slot] = ck.key_off[i];
                    s.len[slot] = ck.key_len[i];
                } else {  // a member: its value decodes
                    uint32_t spos, slen;
                    value_attr(ck.vals + ck.val_off[i], a.attr, &spos, &slen);
                    s.off[slot] = ck.val_off[i] + spos;
                    s.len[slot] = slen;
                }
            }
        }
        s.idx[slot] = i;
        __syncthreads();
        // a round none of whose candidates comes before the last of the best `limit` changes nothing
        // (limit >= 1 here: there are candidates)
        const bool enters = i != kEmpty && slot_before(s, slot, (uint32_t)a.limit - 1, strings, largest, false);
        if (__syncthreads_or(enters)) bitonic(s, kSlots, strings, largest, false);
    }
    // the kept ones, in the kept order, lie in front; the output may run against it
    if (t >= kept) s.idx[t] = kEmpty;
    __syncthreads();
    if (largest != (a.descending != 0)) bitonic(s, kSortFinishBlock, strings, largest, true);
    if (t < kept) a.top[t] = s.idx[t];
    if (t == 0) *a.top_count = kept;
}

}  // namespace

// bins, state | rank | cand | counts and the scan's sums | member
static uint64_t scratch_words(uint64_t n, uint64_t blocks) {
    return kHeadWords + 2 * n + 2 * blocks + scan_scratch_words(2 * blocks) + (n + 7) / 8;
}

uint64_t sorted_scratch_bytes(uint64_t n) { return scratch_words(n, (n + kCheckBlock - 1) / kCheckBlock) * 8; }

hipError_t launch_sorted_search(const SortedArgs& a, hipStream_t stream, bool* no_scratch, const RegexArgs* rx) {
    static_assert(HDX_SORT_LIMIT_MAX <= kSortFinishBlock, "the best so far fill half of the finishing sort's slots");
    static_assert(kHeadWords * 8 % 16 == 0, "the zeroed head");
    *no_scratch = false;
    const uint64_t n = a.ck.n;
    const uint64_t blocks = (n + kCheckBlock - 1) / kCheckBlock;
    if (blocks > 0x3fffffffULL || a.limit > HDX_SORT_LIMIT_MAX) return hipErrorInvalidValue;
    if (n == 0) return hipMemsetAsync(a.top_count, 0, sizeof(uint64_t), stream);
    PoolScratch scratch;
    if (!scratch.acquire(sorted_scratch_bytes(n), stream, no_scratch)) return hipSuccess;
    uint64_t* base = static_cast<uint64_t*>(scratch.p);
    SortScratch s;
    s.bins = base;
    s.state = reinterpret_cast<SortState*>(base + kPasses * kBins);
    s.rank = base + kHeadWords;
    s.cand = s.rank + n;
    s.counts = s.cand + n;
    s.member = reinterpret_cast<uint8_t*>(s.counts + 2 * blocks + scan_scratch_words(2 * blocks));
    const uint64_t flip = a.keep == HDX_KEEP_LARGEST ? ~0ull : 0;
    const uint32_t grid = (uint32_t)blocks, hist_grid = (uint32_t)std::min<uint64_t>(blocks, kHistBlocks);
    hipError_t e = hipMemsetAsync(base, 0, kHeadWords * 8, stream);
    if (e == hipSuccess) {
        const size_t lds = check_lds_bytes(kCheckBlock, a.ck.c);
        if (rx && rx->count)
            hipLaunchKernelGGL(sorted_rank_kernel<RegexArgs>, dim3(grid), dim3(kCheckBlock),
                               lds + regex_lds_bytes(rx->count), stream, a, s.rank, s.member, *rx);
        else
            hipLaunchKernelGGL(sorted_rank_kernel<>, dim3(grid), dim3(kCheckBlock), lds, stream, a, s.rank, s.member);
        e = hipGetLastError();
    }
    for (uint32_t p = 0; p < kPasses && e == hipSuccess; ++p) {
        hipLaunchKernelGGL(sorted_hist_kernel, dim3(hist_grid), dim3(256), 0, stream, (const uint64_t*)s.rank,
                           (const uint8_t*)s.member, n, flip, p, (const SortState*)s.state, s.bins);
        hipLaunchKernelGGL(sorted_pick_kernel, dim3(1), dim3(kBins), 0, stream, (const uint64_t*)s.bins, p, a.limit,
                           s.state);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL(sorted_count_kernel, dim3(grid), dim3(kCheckBlock), 0, stream, (const uint64_t*)s.rank,
                           (const uint8_t*)s.member, n, flip, (const SortState*)s.state, s.counts);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = scan_exclusive(s.counts, 2 * blocks, s.counts + 2 * blocks, stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(sorted_compact_kernel, dim3(grid), dim3(kCheckBlock), 0, stream, (const uint64_t*)s.rank,
                           (const uint8_t*)s.member, n, flip, a.kind == SORT_STRING ? 1u : 0u, s.state,
                           (const uint64_t*)s.counts, s.cand);
        hipLaunchKernelGGL(sorted_finish_kernel, dim3(1), dim3(kSortFinishBlock), 0, stream, a,
                           (const uint64_t*)s.rank, (const uint64_t*)s.cand, (const SortState*)s.state, flip);
        e = hipGetLastError();
    }
    return scratch.release(e);
}

}  // namespace hdx
