// hdx_scratch.hip — the library's stream-ordered scratch and the prefix sum
// that the stages over stored objects share (index entries, checks, sorted
// search, object gather): scan_exclusive's block sums, and most of what those
// stages keep between their launches, are such scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>

#include "hdx_internal.h"

namespace hdx {

// Stream-ordered scratch of the library — the regions' coordinate chunks
// (hdx_regions.hip), the block sums of the prefix sum below and the stages'
// own arrays — comes from a memory pool of the library's own per device that
// keeps up to one region chunk cached between calls (the device's default
// pool returns freed memory at every synchronisation, so each call would map
// its scratch afresh); the pools are trimmed at hdx_shutdown.
static std::mutex g_pool_mu;
static hipMemPool_t g_pool[64];

static hipError_t scratch_pool(hipMemPool_t* out) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= 64) return hipErrorInvalidDevice;
    std::lock_guard<std::mutex> lk(g_pool_mu);
    if (!g_pool[dev]) {
        hipMemPoolProps props{};
        props.allocType = hipMemAllocationTypePinned;
        props.location.type = hipMemLocationTypeDevice;
        props.location.id = dev;
        if ((e = hipMemPoolCreate(&g_pool[dev], &props)) != hipSuccess) {
            g_pool[dev] = nullptr;
            return e;
        }
        uint64_t keep = kRegionChunkBytes;
        (void)hipMemPoolSetAttribute(g_pool[dev], hipMemPoolAttrReleaseThreshold, &keep);
    }
    *out = g_pool[dev];
    return hipSuccess;
}

void trim_scratch_pools() {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    for (hipMemPool_t p : g_pool)
        if (p) (void)hipMemPoolTrimTo(p, 0);
}

bool PoolScratch::acquire(uint64_t bytes, hipStream_t s, bool* no_scratch) {
    hipMemPool_t pool = nullptr;
    hipError_t e = scratch_pool(&pool);
    if (e == hipSuccess) e = hipMallocFromPoolAsync(&p, bytes, pool, s);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        p = nullptr;
        *no_scratch = true;
        return false;
    }
    stream = s;
    return true;
}

hipError_t PoolScratch::release(hipError_t e) {
    if (!p) return e;
    const hipError_t f = hipFreeAsync(p, stream);
    p = nullptr;
    return e == hipSuccess ? f : e;
}

// ---- scan -----------------------------------------------------------------
//
// The exclusive prefix sum of N u64 in place, reduce-then-scan over separate
// launches: index_scan_sums_kernel (one sum per kIndexScanBlock elements), the
// same scan over those sums (recursively: a further level per factor of
// kIndexScanBlock), index_scan_block_kernel (each workgroup scans its elements
// and adds its sum's prefix).  No kernel waits on another workgroup: the order
// is the stream's.  (The kernels keep the names of the stage they were written
// for, the index entries' plan.)

namespace {

constexpr uint32_t kScanThreads = 256;
constexpr uint32_t kScanItems = kIndexScanBlock / kScanThreads;
static_assert(kScanItems * kScanThreads == kIndexScanBlock, "scan block");

// exclusive prefix of x over the workgroup's threads; *total = the sum
__device__ __forceinline__ uint64_t block_exclusive(uint64_t x, uint64_t* total) {
    __shared__ uint64_t wave_sum[kScanThreads / 64];
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint64_t incl = x;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint64_t y = (uint64_t)__shfl_up((unsigned long long)incl, d, 64);
        if (lane >= d) incl += y;
    }
    if (lane == 63) wave_sum[w] = incl;
    __syncthreads();
    uint64_t before = 0, all = 0;
#pragma unroll
    for (uint32_t u = 0; u < kScanThreads / 64; ++u) {
        const uint64_t s = wave_sum[u];
        if (u < w) before += s;
        all += s;
    }
    *total = all;
    return before + incl - x;
}

__global__ void __launch_bounds__(kScanThreads) index_scan_sums_kernel(const uint64_t* data, uint64_t N,
                                                                        uint64_t* sums) {
    const uint64_t base = (uint64_t)blockIdx.x * kIndexScanBlock + (uint64_t)threadIdx.x * kScanItems;
    uint64_t x = 0;
#pragma unroll
    for (uint32_t q = 0; q < kScanItems; ++q)
        if (base + q < N) x += data[base + q];
    uint64_t total;
    (void)block_exclusive(x, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// sums: this level's block sums already scanned (exclusive), or NULL for a
// level of one workgroup
__global__ void __launch_bounds__(kScanThreads) index_scan_block_kernel(uint64_t* data, uint64_t N,
                                                                         const uint64_t* sums) {
    const uint64_t base = (uint64_t)blockIdx.x * kIndexScanBlock + (uint64_t)threadIdx.x * kScanItems;
    uint64_t v[kScanItems];
    uint64_t x = 0;
#pragma unroll
    for (uint32_t q = 0; q < kScanItems; ++q) {
        v[q] = base + q < N ? data[base + q] : 0;
        x += v[q];
    }
    uint64_t total;
    uint64_t run = block_exclusive(x, &total) + (sums ? sums[blockIdx.x] : 0);
#pragma unroll
    for (uint32_t q = 0; q < kScanItems; ++q) {
        if (base + q < N) data[base + q] = run;
        run += v[q];
    }
}

}  // namespace

hipError_t scan_exclusive(uint64_t* data, uint64_t N, uint64_t* scratch, hipStream_t stream) {
    const uint64_t blocks = (N + kIndexScanBlock - 1) / kIndexScanBlock;
    if (blocks > 0x7fffffffULL) return hipErrorInvalidValue;
    if (blocks <= 1) {
        hipLaunchKernelGGL(index_scan_block_kernel, dim3(1), dim3(kScanThreads), 0, stream, data, N,
                           (const uint64_t*)nullptr);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(index_scan_sums_kernel, dim3((uint32_t)blocks), dim3(kScanThreads), 0, stream, data, N,
                       scratch);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if ((e = scan_exclusive(scratch, blocks, scratch + blocks, stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(index_scan_block_kernel, dim3((uint32_t)blocks), dim3(kScanThreads), 0, stream, data, N,
                       (const uint64_t*)scratch);
    return hipGetLastError();
}

// u64 words of block sums over every level of a scan of N elements
uint64_t scan_scratch_words(uint64_t N) {
    uint64_t words = 0;
    while (N > kIndexScanBlock) {
        N = (N + kIndexScanBlock - 1) / kIndexScanBlock;
        words += N;
    }
    return words;
}

}  // namespace hdx
