// hdx_check_eval.h — one lane's share of a search's attribute checks over a
// stored object: the loads, the comparisons and the walk-then-evaluate step
// that check_kernel (hdx_checks.hip) and sorted_rank_kernel (hdx_sorted.hip)
// both run.  One copy: the two kernels give the same first_fail.
//
// Loads: numerics as one unaligned 8-byte value lying wholly inside the key
// or attribute; strings in 8-byte steps the same way, and the last 1..7 bytes
// as the aligned dwords that hold them (word_bytes, hdx_wave.h) — never a
// dword that holds no byte of the attribute.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdint.h>

#include "hdx_internal.h"
#include "hdx_value_walk.h"
#include "hdx_wave.h"

namespace hdx {

constexpr uint32_t kKonstWords = kCheckConstBytes / 8;

// compare(k, v) of datatype_string.cc:263-285, k in LDS at 8-byte-aligned kw
// (zero-padded to 8): memcmp over the shorter length as big-endian unsigned
// words, ending at the first differing one, then the lengths.
__device__ __forceinline__ int compare_string(const uint64_t* kw, uint32_t klen, const uint8_t* v, uint32_t vlen) {
    const uint32_t m = std::min(klen, vlen);
    for (uint32_t w = 0; w < m; w += 8) {
        const uint32_t r = m - w;
        uint64_t a = kw[w >> 3], b;
        if (r >= 8) {
            b = *(gu64_ptr)(v + w);
        } else {
            a &= (1ull << (8 * r)) - 1;  // k may go on past the shorter length
            b = word_bytes(v + w, r);
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
        const uint64_t vb = len ? *(gu64_ptr)p : 0;  // an empty value is 0 / 0.0
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

// The workgroup's LDS for the checks, carved from base in this order: the
// constants (u64[kKonstWords]), off[c][B], len[c][B] (lane-minor: no bank
// conflicts); *end: the first byte behind them.
struct CheckLds {
    uint64_t* konst;
    uint32_t *off, *len;
};
template <uint32_t B>
__device__ __forceinline__ CheckLds check_lds_carve(uint64_t* base, uint32_t c, uint32_t** end) {
    CheckLds s;
    s.konst = base;
    s.off = reinterpret_cast<uint32_t*>(base + kKonstWords);
    s.len = s.off + B * c;
    *end = s.len + B * c;
    return s;
}
constexpr size_t check_lds_bytes(uint32_t B, uint32_t c) { return kCheckConstBytes + (size_t)B * c * 8; }

// Every thread of the workgroup: stage the constants the ops use and clear
// this lane's descriptors; ends with a barrier.
// As compiled for gfx950 this stages far more than konst_words, and only the
// LDS behind this function's barrier may be relied on.  The loop over the ops
// became a pointer at op[k].op (kernel arguments + 0x62 + 24 k) and
// `s_load_dwordx2 ..., 0x2` for klen and koff; a gfx950 scalar load drops the
// low two bits of its base and of its offset separately (measured: base + 0x62
// with offset 2 returns the dwords at + 0x60 and + 0x64), so the loop reads
// {attr | op << 16 | family << 24, klen}.  For any STRING comparison the count
// comes out at 8192 words or more: the staging loop reads that far behind the
// kernel arguments and writes over all of the workgroup's LDS (the hardware
// drops what lies past the allocation).  The results do not depend on it: the
// constants' own words are right, and off / len are cleared afterwards.
// Reading the ops as aligned dwords, or taking the count from the host,
// removes it but is slower than this form: the overrun keeps part of the waves
// off the walk, which then fetches fewer lines twice, so it
// stays until the walk's rate no longer depends on it.
template <uint32_t B>
__device__ __forceinline__ void check_lds_init(const CheckArgs& a, const CheckLds& s) {
    const uint32_t c = a.c, tid = threadIdx.x;
    uint32_t konst_words = 0;  // what the ops use
    for (uint32_t k = 0; k < c; ++k)
        if (a.op[k].op != OP_NEVER && a.op[k].op < OP_LEN_EQ && a.op[k].family == FAM_STRING)
            konst_words = std::max(konst_words, (a.op[k].koff + a.op[k].klen + 7) >> 3);
    for (uint32_t t = tid; t < konst_words; t += B) s.konst[t] = a.konst[t];
    for (uint32_t k = 0; k < c; ++k) {
        s.off[k * B + tid] = 0;
        s.len[k * B + tid] = 0;
    }
    __syncthreads();
}

// ---- OP_REGEX: a compiled list's regex_match ops (hdx_regex.h) --------------
//
// A lane keeps one 64-bit state word; per text byte one read of the op's
// byte-class table (256 x 8 B in LDS, built by the workgroup from the kernel
// arguments: no device allocation, no upload) and regex_step.  The text comes
// by the loads above.  The trip count is the text's length at most: a lane
// leaves at accept, or once every position has died (anchored patterns).
// The table reads are random 8-byte LDS reads per lane (ds_read_b64: two
// groups of 32 lanes, bank (address / 4) mod 64): lanes of a group reading
// the same byte share one read, different bytes congruent mod 32 take turns.
struct RegexLds {
    const RegexArgs* rx;
    const uint64_t* table;  // [rx->count][256]
};
constexpr size_t regex_lds_bytes(uint32_t count) { return (size_t)count * 256 * 8; }

// Every thread of the workgroup, behind check_lds_init's barrier (as compiled,
// its staging loop writes past the carve: see there): the tables at `at`
// (8-byte aligned: the carve is whole u64s); returns the first byte behind
// them.  Ends with a barrier.
template <uint32_t B>
__device__ __forceinline__ uint32_t* regex_lds_init(RegexLds& rl, const RegexArgs& rx, uint32_t* at) {
    uint64_t* table = reinterpret_cast<uint64_t*>(at);
    for (uint32_t r = 0; r < rx.count; ++r)
        for (uint32_t b = threadIdx.x; b < 256; b += B) table[r * 256 + b] = regex_class(rx.prog[r], b);
    rl.rx = &rx;
    rl.table = table;
    __syncthreads();
    return reinterpret_cast<uint32_t*>(table + rx.count * 256);
}

__device__ __forceinline__ bool regex_run(const RegexProg& g, const uint64_t* table, const uint8_t* p, uint32_t len) {
    uint64_t s = regex_start(g);
    if (regex_accepted(g, s)) return true;
    for (uint32_t w = 0; w < len; w += 8) {
        const uint32_t r = std::min(len - w, 8u);
        uint64_t word = word_bytes(p + w, r);
        for (uint32_t b = 0; b < r; ++b, word >>= 8) {
            s = regex_step(g, s, table[word & 0xff]);
            if (regex_accepted(g, s)) return true;
            if (!s) return false;
        }
    }
    return regex_at_end(g, s);
}

// Object i (< a.n): the walk (value_walk, the full walk: the verdict is the
// sweep's at any A), {offset, length} of the attributes the ops name kept in
// LDS, then the ops in order up to the first false one.  Returns first_fail:
// HDX_CHECK_BADENC where the value does not decode.  also(j, pos, L) sees
// every attribute of the walk as well.  RX: the list may hold OP_REGEX ops
// (rx is theirs); the one-shot entry points' kernels are built without.
template <uint32_t B, bool RX, typename F>
__device__ __forceinline__ uint32_t check_object(const CheckArgs& a, const CheckLds& s, const RegexLds& rx, uint64_t i,
                                                 F&& also) {
    const uint32_t c = a.c, tid = threadIdx.x;
    const uint8_t* v = a.vals + a.val_off[i];
    const bool ok = value_walk(v, a.val_len[i], a.A, [&](uint32_t j, uint32_t pos, uint32_t L) {
        for (uint32_t k = 0; k < c; ++k)  // uniform: the ops are kernel arguments
            if (a.op[k].attr == j) {      // attr 0 (the key, OP_NEVER) never equals j >= 1
                s.off[k * B + tid] = pos;
                s.len[k * B + tid] = L;
            }
        also(j, pos, L);
    });
    if (!ok) return HDX_CHECK_BADENC;
    const uint8_t* key = a.keys + a.key_off[i];
    const uint32_t kl = a.key_len[i];
    for (uint32_t k = 0; k < c; ++k) {  // uniform; lanes leave at their first false op
        const CheckOp& o = a.op[k];
        bool t = false;
        if (o.op != OP_NEVER) {
            const bool on_key = o.attr == 0;
            if constexpr (RX) {
                if (o.op == OP_REGEX) {
                    if (!regex_run(rx.rx->prog[o.koff], rx.table + o.koff * 256, on_key ? key : v + s.off[k * B + tid],
                                   on_key ? kl : s.len[k * B + tid]))
                        return k;
                    continue;
                }
            }
            t = eval_op(o, s.konst, on_key ? key : v + s.off[k * B + tid], on_key ? kl : s.len[k * B + tid]);
        }
        if (!t) return k;
    }
    return c;
}

}  // namespace hdx
