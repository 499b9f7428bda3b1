// hdx_multi.cpp — the device set of hdx_init_mask and the entry points that
// span it (include/hdxhash.h, "multi-device").
//
// HyperDex hashes objects from N daemon::loop threads of one process
// (daemon/daemon.cc:345-351 -> key_state::hash_objects, daemon/key_state.cc:
// 1455-1543 -> hyperdex::hash, common/hash.cc:56-68).  Objects are
// independent, so a batch splits into contiguous object ranges, one per
// device, balanced by payload bytes — the rule of
// hyperdex_amd/dist.py:shard_ranges, restated here so a C++ daemon gets it
// without Python or torch:
//   * the host-resident batch (hdx_hash_batch_host): one worker thread per
//     device pipelines its range's H2D -> kernel -> D2H straight into the
//     caller's coordinate rows (the single-device pipeline of hdx_capi.cpp,
//     run on each worker's own streams and staging);
//   * device-resident shards (hdx_hash_batch_device_multi): each device
//     hashes its shard into its rows of its own full coordinate matrix, then
//     one in-process RCCL all-gather over xGMI (ncclCommInitAll over the
//     mask) fills the rest in place.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cmath>
#include <condition_variable>
#include <cstring>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "hdx_cuts.h"
#include "hdx_exchange.h"
#include "hdx_host.h"

namespace hdx {

// ---- byte-balanced cuts: hdx_cuts.h ------------------------------------------

// ---- worker threads ---------------------------------------------------------

// One device's worker threads: a queue served by up to kWorkersPerDevice
// threads, each with its own pipeline (the per-thread slots of hdx_capi.cpp),
// spawned when a job arrives and every thread is busy.  Concurrent callers
// (N daemon::loop threads, daemon/daemon.cc:345-351) that each post a share
// for this device then run side by side instead of queueing on one thread
// (VERDICT r5 #5).  A thread releases its scratch as it exits.
constexpr size_t kWorkersPerDevice = 4;

class Worker {
public:
    Worker() = default;
    Worker(const Worker&) = delete;
    Worker& operator=(const Worker&) = delete;
    // false once join() has begun: the job will never run
    bool post(std::function<void()> job) {
        {
            std::lock_guard<std::mutex> lk(mu_);
            if (stop_) return false;
            q_.push_back(std::move(job));
            if (idle_ == 0 && th_.size() < kWorkersPerDevice) th_.emplace_back([this] { run(); });
        }
        cv_.notify_one();
        return true;
    }
    void join() {
        std::vector<std::thread> th;
        {
            std::lock_guard<std::mutex> lk(mu_);
            stop_ = true;
            th.swap(th_);
        }
        cv_.notify_all();
        for (auto& t : th)
            if (t.joinable()) t.join();
    }
    // a set dropped without destroy_set (a failed create) still ends its
    // threads: a joinable std::thread's destructor would std::terminate
    ~Worker() { join(); }

private:
    void run() {
        std::unique_lock<std::mutex> lk(mu_);
        for (;;) {
            ++idle_;
            cv_.wait(lk, [&] { return stop_ || !q_.empty(); });
            --idle_;
            if (q_.empty()) break;  // stopping, nothing left
            std::function<void()> job = std::move(q_.front());
            q_.pop_front();
            lk.unlock();
            job();
            lk.lock();
        }
        lk.unlock();
        release_thread_scratch();  // this thread's streams and staging, before hdx_shutdown walks the registry
    }
    std::mutex mu_;
    std::condition_variable cv_;
    std::deque<std::function<void()>> q_;
    size_t idle_ = 0;
    bool stop_ = false;
    std::vector<std::thread> th_;
};

// Waits for `count` posted jobs.
class Latch {
public:
    explicit Latch(size_t count) : left_(count) {}
    void done() {
        std::lock_guard<std::mutex> lk(mu_);
        if (--left_ == 0) cv_.notify_all();
    }
    void wait() {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return left_ == 0; });
    }

private:
    std::mutex mu_;
    std::condition_variable cv_;
    size_t left_;
};

// ---- the device set -----------------------------------------------------------

struct DeviceSet {
    uint64_t mask = 0;
    std::vector<int> devs;                        // ascending HIP ordinals (debug: any list)
    std::vector<std::unique_ptr<Worker>> workers;  // one pool per device: the host path
    std::vector<hipStream_t> streams;             // one per device: device-resident shards
    std::vector<ncclComm_t> comms;                // created on the first gather
    std::mutex call_mu;                           // one device-resident multi call at a time
    // calls in progress (SetRef): teardown waits for them, so hdx_init_mask /
    // hdx_shutdown from another thread never frees a set in use
    std::mutex ref_mu;
    std::condition_variable ref_cv;
    uint64_t inflight = 0;
};

static std::mutex g_set_mu;
static std::shared_ptr<DeviceSet> g_set;
// Serialises hdx_init_mask / hdx_shutdown (create and teardown) as whole
// operations: two creates cannot both build a set, and one
// cannot tear down the set another is installing.  Never taken by a call
// that uses the set.
static std::mutex g_lifecycle_mu;

// A call's hold on the set (empty without one).
class SetRef {
public:
    SetRef() = default;
    explicit SetRef(std::shared_ptr<DeviceSet> d) : ds_(std::move(d)) {
        if (ds_) {
            std::lock_guard<std::mutex> lk(ds_->ref_mu);
            ++ds_->inflight;
        }
    }
    SetRef(const SetRef&) = delete;
    SetRef& operator=(const SetRef&) = delete;
    ~SetRef() {
        if (!ds_) return;
        std::lock_guard<std::mutex> lk(ds_->ref_mu);
        if (--ds_->inflight == 0) ds_->ref_cv.notify_all();
    }
    DeviceSet* get() const { return ds_.get(); }
    DeviceSet* operator->() const { return ds_.get(); }
    explicit operator bool() const { return (bool)ds_; }

private:
    std::shared_ptr<DeviceSet> ds_;
};

static std::unique_ptr<SetRef> acquire_set() {
    std::lock_guard<std::mutex> lk(g_set_mu);  // the count is taken before teardown can see the set go
    return std::unique_ptr<SetRef>(new SetRef(g_set));
}

static void destroy_set(DeviceSet* ds) {
    if (!ds) return;
    // workers first: each thread frees its scratch as it exits (not in a
    // thread-local destructor) before hdx_shutdown walks the scratch registry
    for (auto& w : ds->workers) w->join();
    ds->workers.clear();
    for (size_t k = 0; k < ds->comms.size(); ++k) {
        (void)hipSetDevice(ds->devs[k]);
        (void)ncclCommDestroy(ds->comms[k]);
    }
    ds->comms.clear();
    for (size_t k = 0; k < ds->streams.size(); ++k) {
        if (!ds->streams[k]) continue;
        (void)hipSetDevice(ds->devs[k]);
        (void)hipStreamSynchronize(ds->streams[k]);
        (void)hipStreamDestroy(ds->streams[k]);
    }
    ds->streams.clear();
}

static void teardown_locked() {
    std::shared_ptr<DeviceSet> ds;
    {
        std::lock_guard<std::mutex> lk(g_set_mu);
        ds.swap(g_set);
    }
    if (!ds) return;
    {
        std::unique_lock<std::mutex> lk(ds->ref_mu);
        ds->ref_cv.wait(lk, [&] { return ds->inflight == 0; });
    }
    destroy_set(ds.get());
}

void device_set_teardown() {
    std::lock_guard<std::mutex> life(g_lifecycle_mu);
    teardown_locked();
}

hdx_status device_set_create(uint64_t mask, const std::vector<int>& devs) {
    std::lock_guard<std::mutex> life(g_lifecycle_mu);
    {
        std::lock_guard<std::mutex> lk(g_set_mu);
        if (g_set && g_set->mask == mask && g_set->devs == devs) return HDX_OK;
    }
    teardown_locked();  // a different mask replaces the set (after the calls in progress)
    int cur = -1;
    const bool had = hipGetDevice(&cur) == hipSuccess;
    auto ds = std::make_shared<DeviceSet>();
    ds->mask = mask;
    ds->devs = devs;
    ds->streams.assign(devs.size(), nullptr);
    for (size_t k = 0; k < devs.size(); ++k) {
        if (hipSetDevice(devs[k]) != hipSuccess ||
            hipStreamCreateWithFlags(&ds->streams[k], hipStreamNonBlocking) != hipSuccess) {
            const hipError_t e = hipGetLastError();
            destroy_set(ds.get());
            if (had) (void)hipSetDevice(cur);
            return fail(HDX_E_DEVICE, "device %d: stream creation failed: %s", devs[k], hipGetErrorString(e));
        }
    }
    for (size_t k = 0; k < devs.size(); ++k) ds->workers.emplace_back(new Worker());
    if (had) (void)hipSetDevice(cur);
    std::lock_guard<std::mutex> lk(g_set_mu);
    g_set = ds;
    return HDX_OK;
}

// Restores the caller's HIP device on scope exit.
struct DeviceGuard {
    int dev = -1;
    DeviceGuard() {
        if (hipGetDevice(&dev) != hipSuccess) dev = -1;
    }
    ~DeviceGuard() {
        if (dev >= 0) (void)hipSetDevice(dev);
    }
};

// ---- host-resident calls over the set ---------------------------------------------

// The set index whose device the calling thread is bound to (or, unbound,
// would bind to: its current HIP device), else -1.
static int caller_slot(const DeviceSet* ds) {
    int d = thread_device();
    if (d < 0 && hipGetDevice(&d) != hipSuccess) {
        (void)hipGetLastError();
        return -1;
    }
    for (size_t k = 0; k < ds->devs.size(); ++k)
        if (ds->devs[k] == d) return (int)k;
    return -1;
}

// Runs job(k) for every device of the set: the calling thread runs its own
// device's share itself (no hand-off, and concurrent callers keep
// their own pipelines), the workers the others.  Returns the first failing
// device's status (in device order) with that device named.
static hdx_status run_on_set(DeviceSet* ds, const std::function<hdx_status(size_t k)>& job) {
    const size_t nd = ds->devs.size();
    std::vector<hdx_status> st(nd, HDX_OK);
    std::vector<std::string> msg(nd);
    const int mine = caller_slot(ds);
    Latch latch(nd - (mine >= 0 ? 1 : 0));
    for (size_t k = 0; k < nd; ++k) {
        if ((int)k == mine) continue;
        const bool posted = ds->workers[k]->post([&, k] {
            st[k] = job(k);
            if (st[k] != HDX_OK) msg[k] = hdx_last_error();
            latch.done();
        });
        if (!posted) {
            st[k] = HDX_E_DEVICE;
            msg[k] = "the device set is being torn down";
            latch.done();
        }
    }
    if (mine >= 0) {
        DeviceGuard guard;
        st[mine] = job((size_t)mine);
        if (st[mine] != HDX_OK) msg[mine] = hdx_last_error();
    }
    latch.wait();
    for (size_t k = 0; k < nd; ++k)
        if (st[k] != HDX_OK) return fail(st[k], "device %d: %s", ds->devs[k], msg[k].c_str());
    return HDX_OK;
}

// Byte-balanced cuts of n objects over the set (hdx_cuts.h), the block sums
// of the prefix computed by the set's threads in parallel.
template <typename Sizes>
static hdx_status set_cuts(DeviceSet* ds, const Sizes& size, uint64_t n, std::vector<uint64_t>& first) {
    const uint32_t world = (uint32_t)ds->devs.size();
    first.assign(world + 1, 0);
    first[world] = n;
    if (world == 1) return HDX_OK;
    PrefixOf<Sizes> p{size, n, {}};
    const uint64_t blocks = (n + kCutBlock - 1) / kCutBlock;
    std::vector<uint64_t> bsum(blocks);
    hdx_status st = run_on_set(ds, [&](size_t k) {
        for (uint64_t b = blocks * k / world; b < blocks * (k + 1) / world; ++b) bsum[b] = block_bytes(size, n, b);
        return HDX_OK;
    });
    if (st != HDX_OK) return st;
    p.bprefix.assign(blocks + 1, 0);
    for (uint64_t b = 0; b < blocks; ++b) p.bprefix[b + 1] = p.bprefix[b] + bsum[b];
    cuts_from_prefix(p, world, 0.0, first.data());
    return HDX_OK;
}

static HostRegions range_regions(const HostRegions* R, uint64_t f) {
    return R ? HostRegions{R->tables, R->T, R->ids + f, R->stride} : HostRegions{nullptr, 0, nullptr, 0};
}

hdx_status hash_host_any(const uint8_t* codes, uint32_t A, const uint8_t* blob, uint64_t blob_bytes,
                         const uint64_t* obj_base, const uint32_t* attr_len, uint64_t n, uint64_t* coords,
                         const HostRegions* R) {
    std::unique_ptr<SetRef> ref = acquire_set();
    DeviceSet* ds = ref->get();
    if (!ds) return hash_host(codes, A, blob, blob_bytes, obj_base, attr_len, n, coords, R);
    std::vector<uint64_t> first;
    hdx_status st = set_cuts(ds, PackedSizes{attr_len, A}, n, first);
    if (st != HDX_OK) return st;
    return run_on_set(ds, [&](size_t k) -> hdx_status {
        const uint64_t f = first[k], cnt = first[k + 1] - first[k];
        if (cnt == 0) return HDX_OK;
        hdx_status s = bind_device(ds->devs[k]);
        if (s != HDX_OK) return s;
        const HostRegions Rk = range_regions(R, f);
        return hash_host(codes, A, blob, blob_bytes, obj_base + f, attr_len + f * A, cnt,
                         coords ? coords + f * A : nullptr, R ? &Rk : nullptr);
    });
}

// One range of stored objects: the pipeline, then its status words as a
// status (a mis-sized numeric before an undecodable value: the reference
// asserts on the former).
static hdx_status encoded_range(const uint8_t* codes, uint32_t A, const StoredHost& h, uint64_t f, uint64_t cnt,
                                uint64_t* coords, uint64_t* versions, const HostRegions* R) {
    uint32_t bits = 0;
    const HostRegions Rk = range_regions(R, f);
    hdx_status st = hash_encoded_host(codes, A, h.from(f), cnt, coords ? coords + f * A : nullptr,
                                      versions ? versions + f : nullptr, R ? &Rk : nullptr, &bits);
    if (st != HDX_OK) return st;
    if (bits & (1u << HDX_E_BADSIZE))
        return fail(HDX_E_BADSIZE, "objects [%llu, %llu): a numeric value of neither 0 nor 8 bytes (coordinate 0)",
                    (unsigned long long)f, (unsigned long long)(f + cnt));
    if (bits & (1u << HDX_E_BADENC))
        return fail(HDX_E_BADENC, "objects [%llu, %llu): a value does not decode (zero coordinates, version 0)",
                    (unsigned long long)f, (unsigned long long)(f + cnt));
    return HDX_OK;
}

hdx_status hash_encoded_host_any(const uint8_t* codes, uint32_t A, const StoredHost& h, uint64_t n, uint64_t* coords,
                                 uint64_t* versions, const HostRegions* R) {
    std::unique_ptr<SetRef> ref = acquire_set();
    DeviceSet* ds = ref->get();
    if (!ds) return encoded_range(codes, A, h, 0, n, coords, versions, R);
    std::vector<uint64_t> first;
    hdx_status st = set_cuts(ds, StoredSizes{h.o.key_len, h.o.val_len}, n, first);
    if (st != HDX_OK) return st;
    return run_on_set(ds, [&](size_t k) -> hdx_status {
        const uint64_t f = first[k], cnt = first[k + 1] - first[k];
        if (cnt == 0) return HDX_OK;
        hdx_status s = bind_device(ds->devs[k]);
        if (s != HDX_OK) return s;
        return encoded_range(codes, A, h, f, cnt, coords, versions, R);
    });
}

}  // namespace hdx

using namespace hdx;

// ---- exported -------------------------------------------------------------------

HDX_EXPORT hdx_status hdx_shard_ranges(const uint32_t* attr_len, uint32_t attrs_sz, uint64_t n, uint32_t world,
                                       double equal_count_tol, uint64_t* first) {
    if (!first || world == 0) return fail(HDX_E_INVALID, "first is NULL or world == 0");
    if (attr_len && (attrs_sz == 0 || attrs_sz > HDX_MAX_ATTRS))
        return fail(HDX_E_INVALID, "attrs_sz=%u outside [1, %d]", attrs_sz, HDX_MAX_ATTRS);
    shard_cuts(attr_len, attrs_sz, n, world, equal_count_tol, first);  // no sizes: counts differ by at most one
    return HDX_OK;
}

HDX_EXPORT int hdx_device_set(int* devices, int max_devices) {
    std::unique_ptr<SetRef> ref = acquire_set();
    DeviceSet* ds = ref->get();
    if (!ds) return 0;
    const int nd = (int)ds->devs.size();
    for (int k = 0; k < nd && k < max_devices && devices; ++k) devices[k] = ds->devs[k];
    return nd;
}

static const char* nccl_text(ncclResult_t r) { return ncclGetErrorString(r); }

// A device pointer must live on the device its shard runs on (a kernel on
// another device would read through the fabric or fault).  Host (pinned)
// pointers are accepted.
static hdx_status check_on_device(const void* p, int dev, uint32_t k, const char* what) {
    if (!p) return HDX_OK;
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return HDX_OK;  // unregistered host memory: the kernel would fault, but the caller may map it
    }
    if (a.type == hipMemoryTypeDevice && a.device != dev)
        return fail(HDX_E_INVALID, "shard %u: %s is memory of device %d, the shard runs on device %d", k, what,
                    a.device, dev);
    return HDX_OK;
}

namespace {
// One device's shard as the core below takes it (hdx_shard / hdx_region_shard).
struct MultiShard {
    const uint8_t* blob;
    const uint64_t* obj_base;
    const uint32_t* attr_len;
    uint64_t n;
    uint64_t* coords;  // the gathered matrix (T == 0, gather) or this shard's rows; may be NULL when T > 0
    uint64_t* ids;     // T > 0: T sections of N (gather) or of n region ids
    uint32_t* status;
};
}  // namespace

// hdx_hash_batch_device_multi (T == 0) and hdx_hash_batch_regions_device_multi:
// every argument validated, the communicator created and the kernel
// arguments (replicas, code tables) prepared before the first launch; after
// it, any failure waits for every device's stream before returning (ADVICE
// r4), so no kernel or collective still writes the caller's memory.
static hdx_status device_multi(const uint32_t* types, uint32_t A, const std::vector<MultiShard>& sh,
                               const hdx_region_table* tables, uint32_t T, int gather) {
    std::vector<uint8_t> codes(A ? A : 1);
    hdx_status st = check_schema(types, A, codes.data());
    if (st != HDX_OK) return st;
    // the tables (each shard's region_ids pointer is checked with the shard)
    if ((st = check_table_list(tables, T, A)) != HDX_OK) return st;
    std::unique_ptr<SetRef> ref = acquire_set();
    DeviceSet* ds = ref->get();
    if (!ds) return fail(HDX_E_INVALID, "no device set: call hdx_init_mask first");
    const uint32_t world = (uint32_t)ds->devs.size();
    if (sh.size() != world) return fail(HDX_E_INVALID, "%zu shards for a device set of %u devices", sh.size(), world);
    uint64_t total = 0;
    std::vector<uint64_t> counts(world);
    for (uint32_t k = 0; k < world; ++k) total += counts[k] = sh[k].n;
    if (total == 0) return HDX_OK;
    for (uint32_t k = 0; k < world; ++k) {
        const MultiShard& s = sh[k];
        if (s.n && (!s.blob || !s.obj_base || !s.attr_len || (!T && !s.coords) || (T && !s.ids)))
            return fail(HDX_E_INVALID, "shard %u: NULL device pointer", k);
        if (gather && !(T ? s.ids : s.coords)) return fail(HDX_E_INVALID, "shard %u: NULL %s", k, T ? "region_ids" : "coords");
        const int dev = ds->devs[k];
        if ((st = check_on_device(s.blob, dev, k, "blob")) != HDX_OK ||
            (st = check_on_device(s.obj_base, dev, k, "obj_base")) != HDX_OK ||
            (st = check_on_device(s.attr_len, dev, k, "attr_len")) != HDX_OK ||
            (st = check_on_device(s.coords, dev, k, "coords")) != HDX_OK ||
            (st = check_on_device(s.ids, dev, k, "region_ids")) != HDX_OK ||
            (st = check_on_device(s.status, dev, k, "status_dev")) != HDX_OK)
            return st;
    }
    if (gather)
        for (uint32_t k = 1; k < world; ++k)
            for (uint32_t j = 0; j < k; ++j)
                if (ds->devs[j] == ds->devs[k])  // hdxdbg_init_devices: no communicator over one GPU twice
                    return fail(HDX_E_INVALID, "device %d twice in the set: no RCCL gather", ds->devs[k]);
    DeviceGuard guard;
    std::lock_guard<std::mutex> call(ds->call_mu);
    if (gather && ds->comms.empty()) {
        ds->comms.resize(world);
        const ncclResult_t r = ncclCommInitAll(ds->comms.data(), (int)world, ds->devs.data());
        if (r != ncclSuccess) {
            ds->comms.clear();
            return fail(HDX_E_DEVICE, "ncclCommInitAll over %u devices: %s", world, nccl_text(r));
        }
    }
    // kernel arguments: shard k's rows [first_k, first_k + n_k) of its
    // device's matrix (gather), else its own rows
    std::vector<BatchArgs> args(world);
    uint64_t row = 0;
    for (uint32_t k = 0; k < world; ++k) {
        const MultiShard& s = sh[k];
        if (s.n) {
            if (hipSetDevice(ds->devs[k]) != hipSuccess) return hip_fail(hipGetLastError(), "hipSetDevice");
            uint64_t* coords = s.coords ? s.coords + (gather && !T ? row * A : 0) : nullptr;
            uint64_t* ids = T ? s.ids + (gather ? row : 0) : nullptr;
            if ((st = batch_args(args[k], codes.data(), A, s.blob, s.obj_base, s.attr_len, s.n, coords, s.status,
                                 tables, T, ids, gather ? total : s.n, ds->devs[k])) != HDX_OK)
                return st;
        }
        row += s.n;
    }
    auto sync_all = [&]() {
        hipError_t first_err = hipSuccess;
        for (uint32_t k = 0; k < world; ++k) {
            const hipError_t e = hipSetDevice(ds->devs[k]) == hipSuccess ? hipStreamSynchronize(ds->streams[k])
                                                                         : hipGetLastError();
            if (first_err == hipSuccess) first_err = e;
        }
        return first_err;
    };
    for (uint32_t k = 0; k < world; ++k) {
        if (!sh[k].n) continue;
        hipError_t e = hipSetDevice(ds->devs[k]);
        if (e == hipSuccess)
            e = T ? launch_hash_batch_regions(args[k], ds->streams[k]) : launch_hash_batch(args[k], ds->streams[k]);
        if (e != hipSuccess) {
            (void)sync_all();
            return hip_fail(e, T ? "launch_hash_batch_regions" : "launch_hash_batch");
        }
    }
    if (gather) {
        // the exchange (hdx_exchange.h): coordinates are one section of N * A
        // elements, region ids one section of N per table
        const std::vector<ExchangeOp> plan =
            T ? exchange_plan(counts.data(), world, 1, T, total) : exchange_plan(counts.data(), world, A, 1, total * A);
        ncclResult_t r = ncclGroupStart();
        const ncclResult_t r0 = r;
        for (const ExchangeOp& op : plan) {
            for (uint32_t k = 0; k < world && r == ncclSuccess; ++k) {
                uint64_t* m = (T ? sh[k].ids : sh[k].coords) + op.offset;
                r = op.kind == ExchangeOp::kAllGather
                        ? ncclAllGather(m + (size_t)k * op.count, m, op.count, ncclUint64, ds->comms[k], ds->streams[k])
                        : ncclBroadcast(m, m, op.count, ncclUint64, (int)op.root, ds->comms[k], ds->streams[k]);
            }
        }
        const ncclResult_t e = r0 == ncclSuccess ? ncclGroupEnd() : r0;  // the group is closed whatever happened in it
        if (r != ncclSuccess || e != ncclSuccess) {
            (void)sync_all();
            return fail(HDX_E_DEVICE, "RCCL gather: %s", nccl_text(r != ncclSuccess ? r : e));
        }
    }
    const hipError_t e = sync_all();
    if (e != hipSuccess) return hip_fail(e, "hipStreamSynchronize");
    return HDX_OK;
}

HDX_EXPORT hdx_status hdx_hash_batch_device_multi(const uint32_t* types, uint32_t attrs_sz, const hdx_shard* shards,
                                                  uint32_t nshards, int gather) {
    if (!shards && nshards) return fail(HDX_E_INVALID, "shards is NULL");
    std::vector<MultiShard> sh(nshards);
    for (uint32_t k = 0; k < nshards; ++k)
        sh[k] = {shards[k].blob, shards[k].obj_base, shards[k].attr_len, shards[k].n, shards[k].coords, nullptr,
                 shards[k].status_dev};
    return device_multi(types, attrs_sz, sh, nullptr, 0, gather);
}

HDX_EXPORT hdx_status hdx_hash_batch_regions_device_multi(const uint32_t* types, uint32_t attrs_sz,
                                                          const hdx_region_shard* shards, uint32_t nshards,
                                                          const hdx_region_table* tables, uint32_t ntables,
                                                          int gather) {
    if (ntables == 0) return fail(HDX_E_INVALID, "no region tables");
    if (!shards && nshards) return fail(HDX_E_INVALID, "shards is NULL");
    std::vector<MultiShard> sh(nshards);
    for (uint32_t k = 0; k < nshards; ++k)
        sh[k] = {shards[k].blob, shards[k].obj_base, shards[k].attr_len, shards[k].n, shards[k].coords,
                 shards[k].region_ids, shards[k].status_dev};
    return device_multi(types, attrs_sz, sh, tables, ntables, gather);
}

#if HDX_DEBUG_BUILD
// Debug library only (include/hdxhash_debug.h): a device set of explicit
// ordinals, repeats allowed, so the multi-device host path and ungathered
// shards run at world 2, 3, ... on a one-GPU box (tests/test_multi.py).
HDX_EXPORT hdx_status hdxdbg_init_devices(const int* devices, int n) {
    if (!devices || n <= 0 || n > 64) return fail(HDX_E_INVALID, "1 <= n <= 64 devices");
    const int nd = hdx_device_count();
    std::vector<int> devs(devices, devices + n);
    for (int d : devs)
        if (d < 0 || d >= nd) return fail(HDX_E_INVALID, "device %d (count %d)", d, nd);
    hdx_status st = bind_device(devs[0]);
    if (st != HDX_OK) return st;
    return device_set_create(1ull << 63, devs);  // mask bit 63: an explicit list
}
#endif
