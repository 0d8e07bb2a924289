// ohgpu_api.hip -- the core of the C ABI of include/ohgpu.h: errors, the context, memory, streams and events, the device-block cache,
// host staging, the planning pool, and the batch calls no family owns (destroy, info, paths).  The families: api_*.hip (api_common.h).
// No exception crosses this boundary; every failure is a negative code plus ohgpu_last_error().
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <pthread.h>
#include <sched.h>

#include <atomic>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <vector>

#include "api_common.h"

namespace ohgpu {

static thread_local char g_err[512] = "";
static int g_plan_threads = 0;
int plan_thread_cap() { return g_plan_threads; }

// ---- the planning pool: up to 15 helper threads, started on first use, one job at a time (callers queue on a mutex) ----
// The pool is a heap object that is never destroyed: its helpers are detached and sleep in `wake` between jobs, and a mutex or a
// condition variable must not be destroyed under a sleeper (glibc's pthread_cond_destroy waits for them) -- least of all in a forked
// child's exit(), whose copy of the object still counts the parent's sleepers but has none of its threads.  A child gets a pool of
// its own (pthread_atfork): the parent's is left where it lies.
namespace {
struct PlanPool {
    // A job is n_ranges independent ranges; the caller and whichever helpers are awake CLAIM them one at a time (an atomic counter), so
    // a helper that wakes late -- sixteen sleepers behind one mutex do not all start at once -- costs the job nothing but its share:
    // with a fixed range per thread the pass lasted as long as its last waker (0.63-0.99 ms for the same 0.5 ms of work, round 5).
    std::mutex one_job;                       // a job owns the pool from start to finish
    std::mutex m;
    std::condition_variable wake, done;
    unsigned n_helpers = 0;
    void (*job)(void*, unsigned) = nullptr;
    void* arg = nullptr;
    unsigned n_ranges = 0;
    bool job_open = false;                    // (under m) the job and its argument are alive: a helper may join
    unsigned active = 0;                      // (under m) helpers that have joined and not yet left
    uint64_t generation = 0;
    std::atomic<unsigned> next{0}, finished{0};
    void helper()
    {
        uint64_t seen = 0;
        std::unique_lock<std::mutex> lk(m);
        for (;;) {
            wake.wait(lk, [&] { return generation != seen; });
            seen = generation;
            if (!job_open) continue;          // (woke after the job it was woken for had finished)
            void (*j)(void*, unsigned) = job;
            void* a = arg;
            const unsigned nr = n_ranges;
            active++;
            lk.unlock();
            for (unsigned t; (t = next.fetch_add(1, std::memory_order_relaxed)) < nr;) { j(a, t); finished.fetch_add(1, std::memory_order_release); }
            lk.lock();
            if (--active == 0) done.notify_one();
        }
    }
    void run(unsigned nr, unsigned threads, void (*j)(void*, unsigned), void* a)
    {
        std::lock_guard<std::mutex> hold(one_job);
        {
            std::unique_lock<std::mutex> lk(m);
            while (n_helpers + 1 < threads) { ++n_helpers; std::thread([this] { helper(); }).detach(); }
            job = j; arg = a; n_ranges = nr;
            next.store(0, std::memory_order_relaxed); finished.store(0, std::memory_order_relaxed);
            job_open = true;
            generation++;
        }
        // (as many sleepers as the job may use: a helper beyond `threads` started by an earlier, wider job stays asleep)
        if (threads - 1 >= n_helpers) wake.notify_all();
        else for (unsigned k = 1; k < threads; k++) wake.notify_one();
        for (unsigned t; (t = next.fetch_add(1, std::memory_order_relaxed)) < nr;) { j(a, t); finished.fetch_add(1, std::memory_order_release); }
        std::unique_lock<std::mutex> lk(m);
        job_open = false;                     // (no range is left to claim: whoever has not joined yet need not)
        done.wait(lk, [&] { return active == 0; });
        // (every claimed range was run by the caller or by a helper that has left: finished == nr)
    }
};
std::atomic<PlanPool*> g_pool{nullptr};
std::once_flag g_pool_once;
PlanPool& pool()
{
    std::call_once(g_pool_once, [] {
        g_pool.store(new PlanPool());
        // (a fork taken while a job runs leaves the child a locked copy: it is abandoned with the rest)
        (void)pthread_atfork(nullptr, nullptr, [] { g_pool.store(new PlanPool()); });
    });
    return *g_pool.load();
}
}  // namespace

void run_on_pool(unsigned n_ranges, unsigned threads, void (*job)(void* arg, unsigned t), void* arg)
{
    if (threads > n_ranges) threads = n_ranges;
    if (threads > 16) threads = 16;
    if (threads <= 1) { for (unsigned t = 0; t < n_ranges; t++) job(arg, t); return; }
    pool().run(n_ranges, threads, job, arg);
}

// The CPUs this process may keep busy: the affinity mask's, capped by the container's CPU quota (cgroup v2 cpu.max; v1
// cpu.cfs_quota_us / cpu.cfs_period_us) -- a box of 256 logical CPUs whose container is granted sixteen runs sixteen planner threads'
// worth of work however many are started.  Callers that share the grant (one rank per GPU on one host) divide it themselves:
// ohgpu_set_plan_threads.
unsigned usable_cpus()
{
    static const unsigned cached = [] {
        unsigned n = std::thread::hardware_concurrency();
        cpu_set_t set;
        if (sched_getaffinity(0, sizeof(set), &set) == 0 && CPU_COUNT(&set) > 0) n = (unsigned)CPU_COUNT(&set);
        double quota = 0.0;
        if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
            char a[64] = "";
            long long period = 0;
            if (fscanf(f, "%63s %lld", a, &period) == 2 && strcmp(a, "max") != 0 && period > 0) quota = atof(a) / (double)period;
            fclose(f);
        } else {
            long long q = -1, per = 0;
            if (FILE* g = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) { if (fscanf(g, "%lld", &q) != 1) q = -1; fclose(g); }
            if (FILE* g = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) { if (fscanf(g, "%lld", &per) != 1) per = 0; fclose(g); }
            if (q > 0 && per > 0) quota = (double)q / (double)per;
        }
        if (quota >= 1.0 && (unsigned)(quota + 0.5) < n) n = (unsigned)(quota + 0.5);
        return n ? n : 1u;
    }();
    return cached;
}

int set_error(int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

hipError_t ctx_dev_alloc(ohgpu_ctx* ctx, void** p, size_t bytes)
{
    *p = nullptr;
    int c = 0;
    while (c < DevCache::kClasses && ((size_t)256 << c) < bytes) c++;
    DevCache& k = ctx->cache;
    std::lock_guard<std::mutex> hold(k.m);
    // (an idle block of the request's class, or of one of the two above it: a caller whose batches straddle a class boundary from one
    // period to the next -- a plan of 60 KB, then one of 70 -- is served by what the larger of them left behind)
    for (int q = c; q < DevCache::kClasses && q <= c + 2; q++) {
        if (k.idle[q].empty()) continue;
        *p = k.idle[q].back();
        k.idle[q].pop_back();
        return hipSuccess;
    }
    const hipError_t e = hipMalloc(p, c < DevCache::kClasses ? ((size_t)256 << c) : bytes);
    if (e != hipSuccess) { *p = nullptr; return e; }
    k.device_allocs++;
    k.cls[*p] = c < DevCache::kClasses ? c : -1;
    return hipSuccess;
}

void ctx_dev_free(ohgpu_ctx* ctx, void* p)
{
    if (!p) return;
    DevCache& k = ctx->cache;
    std::lock_guard<std::mutex> hold(k.m);
    const auto it = k.cls.find(p);
    if (it != k.cls.end() && it->second >= 0 && k.idle[it->second].size() < 64) {      // (at most 64 idle blocks per class)
        k.idle[it->second].push_back(p);
        return;
    }
    if (it != k.cls.end()) k.cls.erase(it);
    (void)hipFree(p);
}

// one of HostStage's buffers, at least `bytes` long: kept while it is, replaced by one half as large again when it is not
static int stage_reserve(ohgpu_ctx* ctx, void** p, size_t* cap, size_t bytes, bool pinned_host)
{
    if (*cap >= bytes && *p) return OHGPU_OK;
    if (*p) {
        (void)hipStreamSynchronize(ctx->stream);
        (void)(pinned_host ? hipHostFree(*p) : hipFree(*p));
        *p = nullptr; *cap = 0;
    }
    size_t want = bytes + bytes / 2;
    if (want < (64u << 10)) want = 64u << 10;
    want = (want + 4095) & ~(size_t)4095;
    const hipError_t e = pinned_host ? hipHostMalloc(p, want, hipHostMallocDefault) : hipMalloc(p, want);
    if (e != hipSuccess) {
        *p = nullptr;
        return set_error(hip_code(e), "host-buffer staging (%zu bytes): %s", want, hipGetErrorString(e));
    }
    *cap = want;
    if (!pinned_host) { std::lock_guard<std::mutex> hold(ctx->cache.m); ctx->cache.device_allocs++; }
    return OHGPU_OK;
}

int host_stage_in(ohgpu_ctx* ctx, const void* src_host, uint64_t src_bytes, uint64_t dst_bytes)
{
    HostStage& st = ctx->stage;
    st.calls++;
    int err = stage_reserve(ctx, &st.d_src, &st.src_cap, src_bytes ? src_bytes : 1, false);
    if (err == OHGPU_OK) err = stage_reserve(ctx, &st.d_dst, &st.dst_cap, dst_bytes ? dst_bytes : 1, false);
    if (err != OHGPU_OK || src_bytes == 0) return err;
    OHGPU_HIP_TRY(hipMemcpyAsync(st.d_src, src_host, src_bytes, hipMemcpyHostToDevice, ctx->stream));
    st.h2d_bytes += src_bytes;
    return OHGPU_OK;
}

int host_roundtrip(ohgpu_ctx* ctx, const void* src_host, uint64_t src_bytes, void* dst_host, uint64_t dst_bytes,
                   std::vector<std::pair<uint64_t, uint64_t>>& ranges, const std::function<int(const void*, void*)>& run)
{
    HostStage& st = ctx->stage;
    int err = host_stage_in(ctx, src_host, src_bytes, dst_bytes);
    if (err != OHGPU_OK) return err;
    hipStream_t s = ctx->stream;
    // the covered runs of the destination, merged where they touch or overlap
    std::sort(ranges.begin(), ranges.end());
    std::vector<std::pair<uint64_t, uint64_t>> runs;                  // [lo, hi)
    for (const auto& r : ranges) {
        if (r.second == 0) continue;
        if (!runs.empty() && r.first <= runs.back().second) runs.back().second = std::max(runs.back().second, r.first + r.second);
        else runs.emplace_back(r.first, r.first + r.second);
    }
    err = run(st.d_src, st.d_dst);
    if (err != OHGPU_OK) { (void)hipStreamSynchronize(s); return err; }
    if (runs.empty()) { OHGPU_HIP_TRY(hipStreamSynchronize(s)); return OHGPU_OK; }
    const uint64_t lo = runs.front().first, hi = runs.back().second;
    if (runs.size() == 1) {                                           // the outputs tile [lo, hi): one copy, straight home
        OHGPU_HIP_TRY(hipMemcpyAsync((uint8_t*)dst_host + lo, (const uint8_t*)st.d_dst + lo, hi - lo, hipMemcpyDeviceToHost, s));
        st.d2h_bytes += hi - lo;
        OHGPU_HIP_TRY(hipStreamSynchronize(s));
        return OHGPU_OK;
    }
    // holes between the outputs: the span comes back to the bounce buffer in one copy, the covered runs go home from there
    err = stage_reserve(ctx, &st.h_bounce, &st.bounce_cap, hi - lo, true);
    if (err != OHGPU_OK) { (void)hipStreamSynchronize(s); return err; }
    OHGPU_HIP_TRY(hipMemcpyAsync(st.h_bounce, (const uint8_t*)st.d_dst + lo, hi - lo, hipMemcpyDeviceToHost, s));
    st.d2h_bytes += hi - lo;
    OHGPU_HIP_TRY(hipStreamSynchronize(s));
    for (const auto& r : runs) memcpy((uint8_t*)dst_host + r.first, (const uint8_t*)st.h_bounce + (r.first - lo), r.second - r.first);
    return OHGPU_OK;
}

int upload_batch(ohgpu_ctx* ctx, ohgpu_batch* b, const void* host_descs, size_t bytes)
{
    if (bytes == 0) return OHGPU_OK;
    hipError_t e = ctx_dev_alloc(ctx, &b->d_descs, bytes);
    if (e == hipErrorOutOfMemory) return set_error(OHGPU_ERR_NOMEM, "descriptor upload: out of device memory");
    OHGPU_HIP_TRY(e);
    e = hipMemcpy(b->d_descs, host_descs, bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        ctx_dev_free(ctx, b->d_descs);
        b->d_descs = nullptr;
        return set_error(OHGPU_ERR_DEVICE, "descriptor upload: %s", hipGetErrorString(e));
    }
    return OHGPU_OK;
}

int claim_single_launch(const ohgpu_batch* b, hipStream_t s, const char* who)
{
    if (batch_busy_on_another_stream(b, s))
        return set_error(OHGPU_ERR_INVALID, "%s: the batch is still running on another stream (its unit counters / workspace serve one "
                         "launch at a time: wait for it, use the same stream, or create a second batch)", who);
    if (b->last_done == nullptr && hipEventCreate(&b->last_done) != hipSuccess) {       // (it rides on a dispatch as its stop event: src_batch_run)
        b->last_done = nullptr;
        return set_error(OHGPU_ERR_DEVICE, "%s: hipEventCreate failed", who);
    }
    b->last_stream = s;
    return OHGPU_OK;
}

int batch_begin(ohgpu_ctx* ctx, const char* who, BatchKind kind, bool args_ok, size_t n, uint64_t n_cap,
                uint64_t src_arena_bytes, uint64_t dst_arena_bytes, ohgpu_batch** out, BatchPtr* b)
{
    if (!out || !args_ok) return set_error(OHGPU_ERR_INVALID, "%s: null argument", who);
    *out = nullptr;
    if (n > n_cap) return set_error(OHGPU_ERR_INVALID, "%s: too many descriptors", who);
    *b = BatchPtr(new (std::nothrow) ohgpu_batch(), BatchDeleter{ctx});
    if (!*b) return set_error(OHGPU_ERR_NOMEM, "%s: out of host memory", who);
    (*b)->kind = kind; (*b)->n = n; (*b)->src_arena_bytes = src_arena_bytes; (*b)->dst_arena_bytes = dst_arena_bytes;
    return OHGPU_OK;
}

// One row per BatchKind: the noun, with its article, of "<who>: not a <noun> batch"; what gives back everything the family's plan
// holds (it takes a partly built batch: a failed create comes through here too); whether the device is drained first even without
// d_descs.  A new
// family is one row here, one api_*.hip, and a state that derives from RunState: its plan names each device block once (dev_array),
// its release is free_state of the batch's pointer to it (state_free, api_common.h: state_release and a delete).
template <auto State> static void free_state(ohgpu_ctx* ctx, ohgpu_batch* b) { state_free(ctx, b->*State); }
template <auto State> static void free_protected(ohgpu_ctx* ctx, ohgpu_batch* b) { protected_free(ctx, b->*State); }   // (clears the key schedules first)
static void free_fmt(ohgpu_ctx* ctx, ohgpu_batch* b) { free_fmt_line(ctx, b); free_pcm_line(ctx, b); }
static void free_pull(ohgpu_ctx* ctx, ohgpu_batch* b) { if (b->d_pull_tiles) ctx_dev_free(ctx, b->d_pull_tiles); }
static const struct { const char* noun; void (*release)(ohgpu_ctx*, ohgpu_batch*); bool drain; } kKinds[] = {
    {nullptr, nullptr, false},
    {"a pcm", free_pcm_line, true},                 // kBatchPcm
    {"a src", free_src_fast, false},                // kBatchSrc (waits for the batch's last launch: before its event goes)
    {"a fmt", free_fmt, true},                      // kBatchFmt
    {"a flywheel", free_flywheel, true},            // kBatchFlywheel
    {"a Songcast frame", free_ohm, false},          // kBatchOhm
    {"a pulled", free_pull, false},                 // kBatchSrcPull
    {"a DSD", free_dsd_line, true},                 // kBatchDsd
    {"a FLAC", free_state<&ohgpu_batch::flac>, false},   // kBatchFlac
    {"a DSD to PCM", free_dsd_pcm, true},           // kBatchDsdPcm
    {"a lossless-packet (ALAC)", free_state<&ohgpu_batch::alac>, false},   // kBatchAlac
    {"a RAOP", raop_free, false},                   // kBatchRaop
    {"a Songcast receiver", free_state<&ohgpu_batch::ohmrx>, false},   // kBatchOhmRx
    {"a Ogg", free_state<&ohgpu_batch::ogg>, false},   // kBatchOgg
    {"an MPEG-4", free_state<&ohgpu_batch::mp4>, false},   // kBatchMp4
    {"a PCM file", free_state<&ohgpu_batch::file>, false},   // kBatchIff
    {"a DSD file", free_state<&ohgpu_batch::file>, false},   // kBatchDsdFile
    {"a fragmented MPEG-4", free_state<&ohgpu_batch::mp4f>, false},   // kBatchMp4f
    {"a protected MPEG-4", free_protected<&ohgpu_batch::cenc>, false},   // kBatchCenc
    {"a RAOP receiver", free_state<&ohgpu_batch::raoprx>, false},   // kBatchRaopRx
    {"a transport stream", free_state<&ohgpu_batch::ts>, false},   // kBatchTs
    {"an ADTS", free_state<&ohgpu_batch::adts>, false},   // kBatchAdts
    {"a Vorbis", free_state<&ohgpu_batch::vorbis>, false},   // kBatchVorbis
    {"a cbcs-protected MPEG-4", free_protected<&ohgpu_batch::cbcs>, false},   // kBatchCbcs
};
static_assert(sizeof(kKinds) / sizeof(kKinds[0]) == kBatchCbcs + 1, "a row per BatchKind");

int run_guard(ohgpu_ctx* ctx, const char* who, const ohgpu_batch* batch, BatchKind kind, bool empty, bool null_src_ok,
              const void* src_base, const void* dst_base, bool needs_dst)
{
    CTX_GUARD(who);
    if (!batch || batch->kind != kind) return set_error(OHGPU_ERR_INVALID, "%s: not %s batch", who, kKinds[kind].noun);
    if (empty) return 0;
    if ((needs_dst && !dst_base) || (!src_base && !(null_src_ok && batch->src_bytes_touched == 0))) return set_error(OHGPU_ERR_INVALID, "%s: null arena pointer", who);
    return 1;
}

}  // namespace ohgpu

using namespace ohgpu;

extern "C" {

int ohgpu_abi_version(void) { return OHGPU_ABI_VERSION; }

const char* ohgpu_last_error(void) { return g_err; }

int ohgpu_device_count(void)
{
    int n = 0;
    const hipError_t e = hipGetDeviceCount(&n);
    if (e == hipErrorNoDevice) return 0;
    if (e != hipSuccess) return set_error(OHGPU_ERR_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e));
    return n;
}

int ohgpu_init(int device, ohgpu_ctx** out)
{
    if (!out) return set_error(OHGPU_ERR_INVALID, "ohgpu_init: null out pointer");
    *out = nullptr;
    const int n = ohgpu_device_count();
    if (n < 0) return n;
    if (n == 0) return set_error(OHGPU_ERR_NO_DEVICE, "ohgpu_init: no HIP device visible (this library has no CPU fallback)");
    if (device < 0 || device >= n) return set_error(OHGPU_ERR_INVALID, "ohgpu_init: device %d out of range [0,%d)", device, n);
    OHGPU_HIP_TRY(hipSetDevice(device));
    ohgpu_ctx* ctx = new (std::nothrow) ohgpu_ctx();
    if (!ctx) return set_error(OHGPU_ERR_NOMEM, "ohgpu_init: out of host memory");
    ctx->device = device;
    ctx->variant = 0;
    hipDeviceProp_t prop;
    hipError_t e = hipGetDeviceProperties(&prop, device);
    if (e == hipSuccess) {
        snprintf(ctx->name, sizeof(ctx->name), "%s (%s)", prop.name, prop.gcnArchName);
        ctx->num_cus = prop.multiProcessorCount;
    } else {
        snprintf(ctx->name, sizeof(ctx->name), "unknown");
        ctx->num_cus = 256;
    }
    e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete ctx; return set_error(OHGPU_ERR_DEVICE, "hipStreamCreate: %s", hipGetErrorString(e)); }
    uint16_t table[512];
    build_ramp_table(table);
    e = hipMalloc((void**)&ctx->d_ramp_table, sizeof(table));
    if (e == hipSuccess) e = hipMemcpy(ctx->d_ramp_table, table, sizeof(table), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        hipStreamDestroy(ctx->stream);
        delete ctx;
        return set_error(OHGPU_ERR_DEVICE, "ramp table upload: %s", hipGetErrorString(e));
    }
    // (the planner's own device pass -- the ramp planes' kernel -- is loaded here, not inside the first batch's creation)
    (void)load_ramp_plane_kernel();
    *out = ctx;
    return OHGPU_OK;
}

int ohgpu_shutdown(ohgpu_ctx* ctx)
{
    if (!ctx) return OHGPU_OK;
    hipSetDevice(ctx->device);
    hipStreamSynchronize(ctx->stream);
    hipFree(ctx->d_ramp_table);
    for (auto& list : ctx->cache.idle) for (void* p : list) (void)hipFree(p);
    if (ctx->stage.d_src) (void)hipFree(ctx->stage.d_src);
    if (ctx->stage.d_dst) (void)hipFree(ctx->stage.d_dst);
    if (ctx->stage.h_bounce) (void)hipHostFree(ctx->stage.h_bounce);
    hipStreamDestroy(ctx->stream);
    delete ctx;
    return OHGPU_OK;
}

int ohgpu_device_name(ohgpu_ctx* ctx, char* buf, size_t buf_bytes)
{
    if (!ctx || !buf || buf_bytes == 0) return set_error(OHGPU_ERR_INVALID, "ohgpu_device_name: bad argument");
    snprintf(buf, buf_bytes, "%s", ctx->name);
    return OHGPU_OK;
}

int ohgpu_device_pci_bus_id(ohgpu_ctx* ctx, char* buf, size_t buf_bytes)
{
    if (!ctx || !buf || buf_bytes < 16) return set_error(OHGPU_ERR_INVALID, "ohgpu_device_pci_bus_id: bad argument");
    OHGPU_HIP_TRY(hipDeviceGetPCIBusId(buf, (int)buf_bytes, ctx->device));
    for (char* c = buf; *c; c++) if (*c >= 'A' && *c <= 'F') *c = (char)(*c - 'A' + 'a');     // (sysfs spells it in lower case)
    return OHGPU_OK;
}

int ohgpu_set_kernel_variant(ohgpu_ctx* ctx, int variant)
{
    if (!ctx || variant < 0 || variant > 5) return set_error(OHGPU_ERR_INVALID, "ohgpu_set_kernel_variant: bad argument");
    ctx->variant = kernel_variant_alias(variant);
    return OHGPU_OK;
}

int ohgpu_malloc(ohgpu_ctx* ctx, size_t bytes, void** dptr)
{
    CTX_GUARD("ohgpu_malloc");
    if (!dptr) return set_error(OHGPU_ERR_INVALID, "ohgpu_malloc: null out pointer");
    *dptr = nullptr;
    const hipError_t e = hipMalloc(dptr, bytes ? bytes : 1);
    if (e == hipErrorOutOfMemory) return set_error(OHGPU_ERR_NOMEM, "hipMalloc(%zu): out of device memory", bytes);
    OHGPU_HIP_TRY(e);
    return OHGPU_OK;
}

int ohgpu_free(ohgpu_ctx* ctx, void* dptr)
{
    CTX_GUARD("ohgpu_free");
    if (dptr) OHGPU_HIP_TRY(hipFree(dptr));
    return OHGPU_OK;
}

int ohgpu_malloc_host(ohgpu_ctx* ctx, size_t bytes, void** hptr)
{
    CTX_GUARD("ohgpu_malloc_host");
    if (!hptr) return set_error(OHGPU_ERR_INVALID, "ohgpu_malloc_host: null out pointer");
    OHGPU_HIP_TRY(hipHostMalloc(hptr, bytes ? bytes : 1, hipHostMallocDefault));
    return OHGPU_OK;
}

int ohgpu_free_host(ohgpu_ctx* ctx, void* hptr)
{
    CTX_GUARD("ohgpu_free_host");
    if (hptr) OHGPU_HIP_TRY(hipHostFree(hptr));
    return OHGPU_OK;
}

int ohgpu_memcpy_h2d(ohgpu_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes, void* stream)
{
    CTX_GUARD("ohgpu_memcpy_h2d");
    if (bytes) OHGPU_HIP_TRY(hipMemcpyAsync(dst_dev, src_host, bytes, hipMemcpyHostToDevice, pick_stream(ctx, stream)));
    return OHGPU_OK;
}

int ohgpu_memcpy_d2h(ohgpu_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes, void* stream)
{
    CTX_GUARD("ohgpu_memcpy_d2h");
    if (bytes) OHGPU_HIP_TRY(hipMemcpyAsync(dst_host, src_dev, bytes, hipMemcpyDeviceToHost, pick_stream(ctx, stream)));
    return OHGPU_OK;
}

int ohgpu_memset(ohgpu_ctx* ctx, void* dptr, int value, size_t bytes, void* stream)
{
    CTX_GUARD("ohgpu_memset");
    if (bytes) OHGPU_HIP_TRY(hipMemsetAsync(dptr, value, bytes, pick_stream(ctx, stream)));
    return OHGPU_OK;
}

int ohgpu_stream_create(ohgpu_ctx* ctx, void** stream)
{
    CTX_GUARD("ohgpu_stream_create");
    if (!stream) return set_error(OHGPU_ERR_INVALID, "ohgpu_stream_create: null out pointer");
    hipStream_t s;
    OHGPU_HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    *stream = (void*)s;
    return OHGPU_OK;
}

int ohgpu_stream_destroy(ohgpu_ctx* ctx, void* stream)
{
    CTX_GUARD("ohgpu_stream_destroy");
    if (stream) OHGPU_HIP_TRY(hipStreamDestroy((hipStream_t)stream));
    return OHGPU_OK;
}

int ohgpu_stream_sync(ohgpu_ctx* ctx, void* stream)
{
    CTX_GUARD("ohgpu_stream_sync");
    OHGPU_HIP_TRY(hipStreamSynchronize(pick_stream(ctx, stream)));
    return OHGPU_OK;
}

int ohgpu_event_create(ohgpu_ctx* ctx, void** event)
{
    CTX_GUARD("ohgpu_event_create");
    if (!event) return set_error(OHGPU_ERR_INVALID, "ohgpu_event_create: null out pointer");
    hipEvent_t ev;
    OHGPU_HIP_TRY(hipEventCreate(&ev));
    *event = (void*)ev;
    return OHGPU_OK;
}

int ohgpu_event_destroy(ohgpu_ctx* ctx, void* event)
{
    CTX_GUARD("ohgpu_event_destroy");
    if (event) OHGPU_HIP_TRY(hipEventDestroy((hipEvent_t)event));
    return OHGPU_OK;
}

int ohgpu_event_record(ohgpu_ctx* ctx, void* event, void* stream)
{
    CTX_GUARD("ohgpu_event_record");
    OHGPU_HIP_TRY(hipEventRecord((hipEvent_t)event, pick_stream(ctx, stream)));
    return OHGPU_OK;
}

int ohgpu_stream_wait_event(ohgpu_ctx* ctx, void* stream, void* event)
{
    CTX_GUARD("ohgpu_stream_wait_event");
    if (!event) return set_error(OHGPU_ERR_INVALID, "ohgpu_stream_wait_event: null event");
    OHGPU_HIP_TRY(hipStreamWaitEvent(pick_stream(ctx, stream), (hipEvent_t)event, 0));
    return OHGPU_OK;
}

int ohgpu_event_elapsed_ms(ohgpu_ctx* ctx, void* start, void* stop, float* ms)
{
    CTX_GUARD("ohgpu_event_elapsed_ms");
    if (!ms) return set_error(OHGPU_ERR_INVALID, "ohgpu_event_elapsed_ms: null out pointer");
    OHGPU_HIP_TRY(hipEventSynchronize((hipEvent_t)stop));
    OHGPU_HIP_TRY(hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)stop));
    return OHGPU_OK;
}

int ohgpu_ramp_table(uint16_t out[512])
{
    if (!out) return set_error(OHGPU_ERR_INVALID, "ohgpu_ramp_table: null out pointer");
    build_ramp_table(out);
    return OHGPU_OK;
}

int ohgpu_device_allocations(ohgpu_ctx* ctx, uint64_t* count)
{
    CTX_GUARD("ohgpu_device_allocations");
    if (!count) return set_error(OHGPU_ERR_INVALID, "ohgpu_device_allocations: null result");
    std::lock_guard<std::mutex> hold(ctx->cache.m);
    *count = ctx->cache.device_allocs;
    return OHGPU_OK;
}

int ohgpu_batch_destroy(ohgpu_ctx* ctx, ohgpu_batch* batch)
{
    CTX_GUARD("ohgpu_batch_destroy");
    if (!batch) return OHGPU_OK;
    for (ohgpu_batch* part : batch->parts) ohgpu_batch_destroy(ctx, part);
    const auto& row = kKinds[batch->kind];
    // (its blocks go back to the context's cache, for the next batch to write into: nothing of this one may still be running --
    // what hipFree used to see to by itself)
    if (batch->d_descs || row.drain) (void)hipDeviceSynchronize();
    row.release(ctx, batch);
    if (batch->last_done) hipEventDestroy(batch->last_done);
    if (batch->d_descs) ctx_dev_free(ctx, batch->d_descs);
    delete batch;
    return OHGPU_OK;
}

int ohgpu_batch_info(const ohgpu_batch* b, uint64_t* n_msgs, uint64_t* in_frames, uint64_t* out_frames,
                     uint64_t* src_bytes_touched, uint64_t* dst_bytes_written)
{
    if (!b) return set_error(OHGPU_ERR_INVALID, "ohgpu_batch_info: null batch");
    if (n_msgs) *n_msgs = b->n;
    if (in_frames) *in_frames = b->in_frames;
    if (out_frames) *out_frames = b->out_frames;
    if (src_bytes_touched) *src_bytes_touched = b->src_bytes_touched;
    if (dst_bytes_written) *dst_bytes_written = b->dst_bytes_written;
    return OHGPU_OK;
}

static void add_line_paths(const PcmLinePlan& line, ohgpu_batch_paths* out)
{
    if (!line.enabled) return;
    out->line_planned = 1;
    for (uint32_t k = 0; k < kLineLists; k++) out->launches += line.list_count[k] != 0;
    out->staged_chunks += line.n_staged; out->group_chunks += line.n_group; out->heavy_chunks += line.n_heavy;
    out->prefixed_chunks += line.prefixed ? line.n_prefixed : 0;
}


int ohgpu_batch_paths_info(const ohgpu_batch* b, ohgpu_batch_paths* out)
{
    if (!b || !out) return set_error(OHGPU_ERR_INVALID, "ohgpu_batch_paths_info: null argument");
    memset(out, 0, sizeof(*out));
    if (b->kind == kBatchPcm) {
        add_line_paths(b->line, out);
        return OHGPU_OK;
    }
    if (b->kind == kBatchFmt) {
        const FmtLinePlan& f = b->fmtline;
        switch (fmt_route(b)) {
        case kFmtRoutePcmLine: add_line_paths(b->line, out); break;
        case kFmtRouteWide: out->fmt_wide_records = f.n_wide; break;
        case kFmtRouteStereo:
            out->fmt_stereo_records = f.n_chunks;
            out->fmt_stereo_kind = f.group_kind;
            out->fmt_stereo_bytes = f.group_bytes;
            break;
        case kFmtRouteStaged: out->fmt_staged_chunks = f.n_chunks; break;
        case kFmtRouteGeneric: break;
        }
        return OHGPU_OK;
    }
    if (b->kind == kBatchAlac || b->kind == kBatchRaop) {
        out->alac_route = b->alac && b->alac->plain ? 2u : 1u;
        return OHGPU_OK;
    }
    if (b->kind == kBatchMp4) {
        out->mp4_route = b->mp4 && b->mp4->plain ? 2u : 1u;
        return OHGPU_OK;
    }
    if (b->kind == kBatchIff) {
        out->iff_route = b->file && b->file->plain ? 2u : 1u;
        return OHGPU_OK;
    }
    if (b->kind == kBatchDsdFile) {
        out->dsd_file_route = b->file && b->file->plain ? 2u : 1u;
        return OHGPU_OK;
    }
    if (b->kind == kBatchVorbis) {
        out->vorbis_route = b->vorbis && b->vorbis->plain ? 2u : 1u;
        return OHGPU_OK;
    }
    if (b->kind == kBatchRaopRx) {
        out->raop_rx_route = b->raoprx && b->raoprx->plain ? 2u : 1u;
        return OHGPU_OK;
    }
    if (b->kind != kBatchOhm) return set_error(OHGPU_ERR_INVALID, "ohgpu_batch_paths_info: not a pcm, Songcast frame, fmt, Apple Lossless, MPEG-4, PCM file or DSD file batch");
    const OhmPlan& p = b->ohm;
    if (p.direct) add_line_paths(p.direct->line, out);
    out->ohm_wide_fragments = p.n_selr;
    out->ohm_staged_fragments = p.stage ? (uint32_t)p.stage->n : 0;
    out->ohm_headers_fused = p.n_unfolded_generic - p.n_unfolded;
    out->ohm_headers_separate = p.n_unfolded;
    return OHGPU_OK;
}

int ohgpu_set_plan_threads(int threads)
{
    if (threads < 0 || threads > 256) return set_error(OHGPU_ERR_INVALID, "ohgpu_set_plan_threads: %d", threads);
    g_plan_threads = threads;
    return OHGPU_OK;
}

// ohgpu_measure_shader_clock: every wave runs a chain of dependent integer multiply-adds (about 0.2 ms at 2.4 GHz); wave 0 of every
// workgroup reports the shader cycles and the 100 MHz reference ticks its chain took.
__global__ __launch_bounds__(256) void clock_probe_kernel(uint64_t* __restrict__ out, uint32_t iters)
{
    uint32_t x = threadIdx.x + 1u;
    const uint64_t c0 = __builtin_readcyclecounter();
    const uint64_t r0 = __builtin_amdgcn_s_memrealtime();
    for (uint32_t i = 0; i < iters; i++) x = x * 1664525u + 1013904223u;
    asm volatile("" : "+v"(x));
    const uint64_t c1 = __builtin_readcyclecounter();
    const uint64_t r1 = __builtin_amdgcn_s_memrealtime();
    if (threadIdx.x == 0) {
        out[2 * blockIdx.x] = c1 - c0;
        out[2 * blockIdx.x + 1] = (r1 - r0) + (x == 0x12345u ? 1u : 0u);      // (x is used)
    }
}

int ohgpu_measure_shader_clock(ohgpu_ctx* ctx, void* stream, double* mhz)
{
    CTX_GUARD("ohgpu_measure_shader_clock");
    if (!mhz) return set_error(OHGPU_ERR_INVALID, "ohgpu_measure_shader_clock: null result");
    hipStream_t s = pick_stream(ctx, stream);
    const uint32_t groups = ctx->num_cus > 0 ? (uint32_t)ctx->num_cus : 256u;
    uint64_t* d = nullptr;
    OHGPU_HIP_TRY(hipMalloc((void**)&d, groups * 2 * sizeof(uint64_t)));
    hipLaunchKernelGGL(clock_probe_kernel, dim3(groups), dim3(256), 0, s, d, 60000u);
    std::vector<uint64_t> h(groups * 2);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(h.data(), d, h.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(d);
    if (e != hipSuccess) return set_error(OHGPU_ERR_DEVICE, "ohgpu_measure_shader_clock: %s", hipGetErrorString(e));
    double cyc = 0.0, ref = 0.0;
    for (uint32_t i = 0; i < groups; i++) { cyc += (double)h[2 * i]; ref += (double)h[2 * i + 1]; }
    if (ref <= 0.0) return set_error(OHGPU_ERR_DEVICE, "ohgpu_measure_shader_clock: the reference counter did not advance");
    *mhz = cyc / ref * 100.0;
    return OHGPU_OK;
}

int ohgpu_host_transfer_stats(ohgpu_ctx* ctx, uint64_t* calls, uint64_t* src_calls, uint64_t* h2d_bytes, uint64_t* d2h_bytes)
{
    if (!ctx) return set_error(OHGPU_ERR_INVALID, "ohgpu_host_transfer_stats: null context");
    if (calls) *calls = ctx->stage.calls;
    if (src_calls) *src_calls = ctx->stage.src_calls;
    if (h2d_bytes) *h2d_bytes = ctx->stage.h2d_bytes;
    if (d2h_bytes) *d2h_bytes = ctx->stage.d2h_bytes;
    return OHGPU_OK;
}

}  // extern "C"
