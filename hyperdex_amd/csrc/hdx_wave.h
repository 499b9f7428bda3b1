// hdx_wave.h — device helpers that more than one kernel file uses: the wave's
// LDS fence, global-memory pointer types, the partial-dword read, the ballot
// rank inside a workgroup and the status write.  One copy of each.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdint.h>

#include "../../include/hdxhash.h"

namespace hdx {

// the wave's LDS accesses ordered (the class sort's phases, a window's reuse)
__device__ __forceinline__ void wave_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Values at any byte address, and pointers to them (gu*) and to aligned
// dwords (ga32) in global memory.
typedef uint16_t __attribute__((aligned(1))) u16_u;
typedef uint32_t __attribute__((aligned(1))) u32_u;
typedef uint64_t __attribute__((aligned(1))) u64_u;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 __attribute__((aligned(1))) u32x4_u;
typedef const __attribute__((address_space(1))) u16_u* gu16_ptr;
typedef const __attribute__((address_space(1))) u32_u* gu32_ptr;
typedef const __attribute__((address_space(1))) u64_u* gu64_ptr;
typedef const __attribute__((address_space(1))) u32x4_u* gu128_ptr;
typedef const __attribute__((address_space(1))) uint32_t* ga32_ptr;

// The load rule of the kernels over stored objects: bytes of a key or an
// attribute are read as unaligned 4- / 8- / 16-byte values lying wholly inside
// it, and what is left at its end as the aligned dwords that hold the bytes
// taken.  Each holds a byte of the object, so it lies in the object's pages:
// no dword is read that holds no byte of the object.

// The `take` (1..3) bytes at p in the low bytes of the result, the bytes past
// them unspecified: for a caller that masks a whole dword anyway.
__device__ __forceinline__ uint32_t tail_dwords(const uint8_t* p, uint32_t take) {
    const uint32_t sh = (uint32_t)(uintptr_t)p & 3;
    const uint8_t* q = p - sh;  // the aligned dword that holds p[0]
    const uint32_t d0 = *(ga32_ptr)q;
    const uint32_t d1 = sh + take > 4 ? *(ga32_ptr)(q + 4) : 0u;
    return __builtin_amdgcn_alignbyte(d1, d0, sh);
}

// The `take` (1..4) bytes at p in the low bytes of the result, the rest zero.
__device__ __forceinline__ uint32_t tail_bytes(const uint8_t* p, uint32_t take) {
    if (take == 4) return *(gu32_ptr)p;
    return tail_dwords(p, take) & ((1u << (8 * take)) - 1);
}

// The r (1..8) bytes at p as a little-endian word, zero-padded.
__device__ __forceinline__ uint64_t word_bytes(const uint8_t* p, uint32_t r) {
    if (r >= 8) return *(gu64_ptr)p;
    uint64_t b = tail_bytes(p, std::min(r, 4u));
    if (r > 4) b |= (uint64_t)tail_bytes(p + 4, r - 4) << 32;
    return b;
}

// Every thread of a workgroup of B: the rank of this lane's flag k among the
// workgroup's set flags k (those of lower threads) and their number, for K
// flags behind one barrier.  s_cnt: K * (B / 64) words of LDS.
template <uint32_t B, uint32_t K>
__device__ __forceinline__ void block_ranks(const bool (&flag)[K], uint32_t* s_cnt, uint32_t (&rank)[K],
                                            uint32_t (&total)[K]) {
    constexpr uint32_t W = B / 64;
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint64_t mask[K];
#pragma unroll
    for (uint32_t k = 0; k < K; ++k) mask[k] = __ballot(flag[k]);
    if (lane == 0) {
#pragma unroll
        for (uint32_t k = 0; k < K; ++k) s_cnt[k * W + w] = (uint32_t)__popcll(mask[k]);
    }
    __syncthreads();
    const uint64_t below = (1ull << lane) - 1;
#pragma unroll
    for (uint32_t k = 0; k < K; ++k) {
        uint32_t before = 0, all = 0;
#pragma unroll
        for (uint32_t u = 0; u < W; ++u) {
            const uint32_t s = s_cnt[k * W + u];
            if (u < w) before += s;
            all += s;
        }
        rank[k] = before + (uint32_t)__popcll(mask[k] & below);
        total[k] = all;
    }
}

// The bits of a device status word (hdx_status, include/hdxhash.h).
constexpr uint32_t kStatusBadSize = 1u << HDX_E_BADSIZE, kStatusInvalid = 1u << HDX_E_INVALID,
                   kStatusNoMem = 1u << HDX_E_NOMEM, kStatusBadEnc = 1u << HDX_E_BADENC;

// One status atomic per wave: mask is wave-uniform; status may be NULL.
__device__ __forceinline__ void wave_status_or(uint32_t* status, uint32_t mask) {
    if (status && mask && (threadIdx.x & 63) == 0) atomicOr(status, mask);
}
// `bit` where cond holds on any lane of the wave.
__device__ __forceinline__ void wave_status_or(uint32_t* status, bool cond, uint32_t bit) {
    if (status && __any(cond) && (threadIdx.x & 63) == 0) atomicOr(status, bit);
}

}  // namespace hdx
