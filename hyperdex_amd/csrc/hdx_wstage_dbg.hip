// hdx_wstage_dbg.hip — the wave-staged kernel's A/B forms (debug library
// only, libhdxhash_dbg.so): each a named variation of another form
// (WstageForm, hdx_wstage.h), the class sort over the workgroup
// (hash_wgstage_kernel), debug shapes, and their rows of the batch hash's
// variant table (hdx_variants.h).  Results: DESIGN.md §4.5 (round 3),
// profiles/r3/ab_wstage_*.jsonl and the later rounds' profiles.
#include "hdx_variants.h"
#include "hdx_wstage.h"

namespace hdx {

template <int NCH, uint32_t WB>
__global__ void __launch_bounds__(256)
hash_wgstage_kernel(const BatchArgs args) {
    static_assert(NCH >= 1 && NCH <= 2 && WB % 16 == 0, "slot ids are 9 bits");
    constexpr uint32_t SL = NCH * 64;  // slots per wave
    __shared__ __attribute__((aligned(16))) uint8_t win_all[4][WB + 64];
    __shared__ uint64_t desc_all[4 * SL];  // {absolute window offset, length}; then the parked coordinate
    __shared__ uint16_t perm[4 * SL];      // workgroup slot | code << 9, in class order
    __shared__ uint32_t wcnt[4][kClasses]; // per wave: staged slots per class
    const int lane = threadIdx.x & 63;
    const int w = threadIdx.x >> 6;
    uint64_t* desc = desc_all + w * SL;
    const ldsw_t lw_all = as_ldsw(&win_all[0][0]);
    const uint32_t win_off = (uint32_t)w * (WB + 64);

    const uint64_t o0 = ((uint64_t)blockIdx.x * 4 + w) * args.K;
    const bool live = o0 < args.n;  // (every wave reaches every barrier)
    Group<NCH> g{};
    if (live) g = describe_group<NCH, WB, 0>(args, o0, win_all[w], win_off, desc);
    const bool sorted = live && g.staged;
    bool bad = false;
    if (live && !g.staged) {  // hashed here, from global memory, in slot order
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const uint32_t s = (uint32_t)(c * 64 + lane);
            desc[s] = hash_slot<0>(args, lw_all, false, g.mybase, s, g.code[c], desc[s], bad);
        }
    }
    // per-class counts of this wave's staged slots
    uint32_t mine[kClasses];
#pragma unroll
    for (int k = 0; k < kClasses; ++k) {
        uint32_t n = 0;
#pragma unroll
        for (int c = 0; c < NCH; ++c)
            n += (uint32_t)__popcll(__ballot(sorted && (uint32_t)(c * 64 + lane) < g.ns && g.cls[c] == (uint32_t)k));
        mine[k] = n;
    }
    if (lane < kClasses) {
        uint32_t v = 0;
#pragma unroll
        for (int k = 0; k < kClasses; ++k) v = lane == k ? mine[k] : v;
        wcnt[w][lane] = v;
    }
    __syncthreads();  // (1) counts published, descriptors written

    // class bases over the workgroup, and this wave's offset inside each class
    uint32_t tot = 0, before = 0;  // lane k < kClasses: class k's total, waves < w's share
    if (lane < kClasses) {
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const uint32_t x = wcnt[v][lane];
            tot += x;
            before += v < w ? x : 0u;
        }
    }
    const uint32_t cbase = wave_scan_dpp(tot) - tot;  // lanes >= kClasses add 0
    const uint32_t T = __builtin_amdgcn_readlane(cbase + tot, kClasses - 1);
    const uint32_t start = cbase + before;  // lane k: this wave's first position in class k
    uint32_t seen[kClasses];  // per class: this wave's next position (read with every lane active:
#pragma unroll                // a ds_bpermute from an inactive lane returns 0)
    for (int k = 0; k < kClasses; ++k) seen[k] = (uint32_t)__shfl((int)start, k, 64);
    if (sorted) {
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const uint32_t s = (uint32_t)(c * 64 + lane);
            const bool in = s < g.ns;
#pragma unroll
            for (int k = 0; k < kClasses; ++k) {
                const uint64_t m = __ballot(in && g.cls[c] == (uint32_t)k);
                if (in && g.cls[c] == (uint32_t)k) {
                    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32),
                                              __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                    const uint32_t pos = seen[k] + rank;
                    perm[pos] = (uint16_t)((uint32_t)(w * SL + s) | (g.code[c] << 9));
                }
                seen[k] += (uint32_t)__popcll(m);
            }
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's window has landed
    __syncthreads();  // (2) permutation complete, every window landed

    // passes of 64 class-sorted slots of the workgroup: wave w takes w, w+4, ...
    const uint32_t passes = (T + 63) / 64;
    for (uint32_t p = (uint32_t)w; p < passes; p += 4) {
        const uint32_t idx = p * 64 + (uint32_t)lane;
        if (idx < T) {
            const uint32_t e = perm[idx];
            const uint32_t gs = e & 0x1ffu, cd = e >> 9;
            desc_all[gs] = hash_slot<0>(args, lw_all, true, 0, gs, cd, desc_all[gs], bad);
        }
    }
    __syncthreads();  // (3) every parked coordinate written

    if (live) {
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const uint32_t s = (uint32_t)(c * 64 + lane);
            if (s < g.ns) __builtin_nontemporal_store(desc[s], args.coords + g.q0 + s);
        }
    }
    if (bad && args.status) atomicOr(args.status, 1u << 2 /* HDX_E_BADSIZE */);
}


template <int NCH, uint32_t WB>
static hipError_t launch_wgstage_t(BatchArgs args, hipStream_t stream) {
    args.K = std::min<uint32_t>((uint32_t)(64 * NCH) / args.A, 63u);
    if (args.K == 0) return hipErrorInvalidValue;
    const uint64_t waves = (args.n + args.K - 1) / args.K;
    const uint64_t blocks = (waves + 3) / 4;
    if (blocks == 0) return hipSuccess;
    if (blocks > 0x7fffffffULL) return hipErrorInvalidValue;
    hipLaunchKernelGGL((hash_wgstage_kernel<NCH, WB>), dim3((uint32_t)blocks), dim3(256), 0, stream, args);
    return hipGetLastError();
}


namespace {

// The forms, named by variant id.  Each says what it changes against the form
// it derives from; WstageForm and WstageProduct are in hdx_wstage.h.
// Round 3's first forms: the slots hashed as from global memory (HT 0), four
// waves per workgroup; passes per wave and window bytes.
struct V200 : WstageForm { static constexpr uint32_t WB = 10240; };
struct V201 : WstageForm { static constexpr int NCH = 3; static constexpr uint32_t WB = 14336; };
struct V202 : WstageForm { static constexpr uint32_t WB = 8192; };
struct V203 : WstageForm { static constexpr int NCH = 1; static constexpr uint32_t WB = 5120; };
struct V204 : WstageForm { static constexpr int NCH = 4; static constexpr uint32_t WB = 18432; };
using V205 = WstageForm;
struct V206 : V205 { static constexpr uint32_t KCAP = 6; };
struct V207 : V205 { static constexpr int SHAPE = 1; };
struct V208 : V205 { static constexpr int SHAPE = 2; };
struct V209 : V205 { static constexpr uint32_t KCAP = 3; };
// head/tail window hashing (hash_slot_window)
struct HeadTail : WstageForm { static constexpr int HT = 1; };
struct V213 : HeadTail { static constexpr uint32_t KCAP = 3; };
struct V214 : HeadTail { static constexpr int NCH = 3; static constexpr uint32_t WB = 14336; };
struct V215 : HeadTail { static constexpr int ORDER = 3; };
struct V216 : HeadTail { static constexpr int W128 = 1; };
struct V218 : HeadTail { static constexpr int SHAPE = 1; };
struct V219 : WstageForm { static constexpr int HT = 2; };
struct V240 : V219 { static constexpr bool GAP = true; };
struct V241 : V240 { static constexpr bool ADMA = true; static constexpr int SHAPE = 1; };
// back from the product, round by round
struct V287 : WstageProduct { static constexpr int HT = 5; };  // before LOOP 4: round 5's product
struct V279 : V287 { static constexpr int PRIO = 0; };
struct V278 : V279 { static constexpr int W128 = 1; };
struct V270 : V279 { static constexpr bool NT = false; };
struct V273 : V270 { static constexpr int NCH = 3; static constexpr uint32_t WB = 14336; };
struct V274 : V270 { static constexpr int NCH = 3; static constexpr uint32_t WB = 13312, KCAP = 10; };
struct V275 : V270 { static constexpr bool RD = true; };
struct V276 : V275 { static constexpr uint32_t WB = 8704; };
struct V256 : V270 { static constexpr bool XS = false; };
struct V257 : V256 { static constexpr int WPB = 2; };
struct V258 : V256 { static constexpr uint32_t WB = 7680, KCAP = 6; };
struct V259 : V256 { static constexpr int WPB = 4; };  // round 4's product
struct V255 : V259 { static constexpr bool DL = true; };
struct V248 : V259 { static constexpr int W128 = 2; };
struct V249 : V259 { static constexpr int W128 = 3; };
struct V245 : V259 { static constexpr int ORDER = 1; };
struct V242 : V259 { static constexpr int HT = 3; };
struct V239 : V259 { static constexpr int HT = 1; };
struct V246 : V259 { static constexpr int HT = 2; };
struct V244 : V246 { static constexpr bool PU = false; };
// round 6: the slot plan (PLAN), numerics by selects (NUM2), the class table (ORDER 5)
struct V293 : WstageProductNum2 { static constexpr int HT = 5; };
struct V294 : V287 { static constexpr bool PLAN = true; };
struct V295 : V287 { static constexpr bool NUM2 = true; };
struct V296 : V287 { static constexpr int ORDER = 5; };
struct V297 : V293 { static constexpr int SHAPE = 1; };

// A wider schema than the form's passes hold (K = 0), or one NUM2 does not
// take, runs the gather kernel 44 instead.
template <auto LAUNCH>
hipError_t or_44(const BatchArgs& args, hipStream_t stream) {
    if (args.n == 0) return hipSuccess;
    const hipError_t e = LAUNCH(args, stream);
    return e == hipErrorInvalidValue ? launch_hash_batch_variant(args, stream, 44) : e;
}
template <class F>
constexpr auto form = or_44<launch_wstage_t<F>>;

const BatchRow kRows[] = {
    {200, form<V200>, "2 passes, 10 KiB windows"},
    {201, form<V201>, "3 passes, 14 KiB windows"},
    {202, form<V202>, "2 passes, 8 KiB windows"},
    {203, form<V203>, "1 pass, 5 KiB windows"},
    {204, form<V204>, "4 passes, 18 KiB windows"},
    {205, form<V205>, "2 passes, 8832-byte windows (four workgroups per CU)"},
    {206, form<V206>, "205 with <= 6 objects per wave"},
    {207, form<V207>, "debug shape of 205: no hash (WRONG coordinates)"},
    {208, form<V208>, "debug shape of 205: no DMA (WRONG coordinates)"},
    {209, form<V209>, "205 with <= 3 objects per wave (per-regime VALU on uniform batches)"},
    {210, or_44<launch_wgstage_t<2, 8832>>, "the slots class-sorted over the workgroup, 2 passes"},
    {211, or_44<launch_wgstage_t<1, 4352>>, "... 1 pass, 4352-byte windows"},
    {213, form<V213>, "head/tail window hashing with <= 3 objects per wave (per-regime costs)"},
    {214, form<V214>, "head/tail window hashing, 3 passes, 14 KiB windows"},
    {215, form<V215>, "head/tail window hashing in class order 3"},
    {216, form<V216>, "head/tail window hashing with b128 window reads"},
    {218, form<V218>, "debug shape of head/tail window hashing: no hash (WRONG coordinates)"},
    {219, form<V219>, "round 3's product without the pass-boundary gap (class_sort)"},
    {239, form<V239>, "259 with the one-block > 64-byte loop (city_gt64_lds LOOP 1)"},
    {240, form<V240>, "round 3's product with the DMA as the builtin (describe_group ADMA off)"},
    {241, form<V241>, "debug shape of round 3's product: no hash (WRONG coordinates)"},
    {242, form<V242>, "259 with one final mix16 for the > 64 and 8..32-byte regimes (LOOP 3)"},
    {244, form<V244>, "246 with the pass loop not unrolled"},
    {245, form<V245>, "259 with the branchy work class (ORDER 1)"},
    {246, form<V246>, "259 without TNUM (numerics read apart from the strings' tail)"},
    {248, form<V248>, "debug shape of 259: its LDS reads at conflict-free addresses (WRONG coordinates)"},
    {249, form<V249>, "debug shape of 259: no funnel shifts on its LDS reads (WRONG coordinates)"},
    {255, form<V255>, "259 with round 3's per-KiB span copy"},
    {256, form<V256>, "259 with one wave per workgroup"},
    {257, form<V257>, "259 with two waves per workgroup"},
    {258, form<V258>, "256 with <= 6 objects and 7.5 KiB windows: 18 waves per CU"},
    {259, form<V259>, "round 4's product: four waves per workgroup"},
    {270, form<V270>, "256 with the XCD-aware block order"},
    {273, form<V273>, "270 with 3 passes, 11 objects per wave, 14 KiB windows"},
    {274, form<V274>, "270 with 3 passes, 10 objects per wave, 13 KiB windows"},
    {275, form<V275>, "270 with its descriptors in registers (17 waves per CU)"},
    {276, form<V276>, "275 with 8.5 KiB windows (18 waves per CU)"},
    {278, form<V278>, "279 with dword-aligned ds_read_b128 window reads (W128 1)"},
    {279, form<V279>, "270 with non-temporal loads (lengths, bases, span)"},
    {287, form<V287>, "279 with wave priorities, loads high: round 5's product, the product before LOOP 4"},
    {293, form<V293>, "287 with the slot plan, select numerics and the class table"},
    {294, form<V294>, "287 with the slot plan alone"},
    {295, form<V295>, "287 with select numerics (NUM2) alone"},
    {296, form<V296>, "287 with the class table alone"},
    {297, form<V297>, "debug shape of 293: no hash (WRONG coordinates)"},
    {298, form<V293>, "the product as before LOOP 4 (two head reads, separate mix16s; = 293)"},
};

}  // namespace

VariantRows<BatchArgs> wstage_variant_rows() { return kRows; }

}  // namespace hdx
