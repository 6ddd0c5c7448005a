// runtime.hip -- what one process of libmalstroem_hip.so shares: the error text, the development-knob gate, the spinning stream
// synchronisation, the caching device pool, the upload / download helpers of the entry points, and the extern "C" calls about the
// process and its devices.  There is no CPU fallback: without a HIP device every compute call returns MHIP_ENODEV.
#include <cstdarg>
#include <chrono>
#include <map>
#include <mutex>

#include "common.hpp"

namespace mh {

static thread_local char g_err[512] = "";

void set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
const char *get_error() { return g_err; }
const char *dev_env(const char *name)
{
    static const bool on = [] { const char *e = getenv("MHIP_DEVELOPER"); return e && e[0] == '1'; }();
    return on ? getenv(name) : nullptr;
}

hipError_t stream_sync(hipStream_t s)
{
    static const long spin_us = [] { const char *e = getenv("MALSTROEM_HIP_SPIN_US"); return e ? atol(e) : 3000L; }();
    if (spin_us > 0) {
        const auto t0 = std::chrono::steady_clock::now();
        for (;;) {
            const hipError_t e = hipStreamQuery(s);
            if (e != hipErrorNotReady) return e;
            if (std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count() > spin_us) break;
        }
    }
    return hipStreamSynchronize(s);
}

// ---- caching device allocator -------------------------------------------------------------------
// Freed blocks are kept per (device, rounded size) and handed out again; callers only release a block after
// synchronising the stream that used it, so reuse needs no further ordering.
namespace {
std::mutex g_pool_mu;
std::multimap<std::pair<int, size_t>, void *> g_pool;
size_t g_pool_bytes = 0;
constexpr size_t POOL_CAP = 96ull << 30;  // MI355X has 288 GB of HBM3E; keep at most a third cached
size_t round_size(size_t n) { return n < (1u << 20) ? ((n + 255) & ~size_t(255)) : ((n + (1u << 20) - 1) & ~size_t((1u << 20) - 1)); }
// Under MHIP_DEVELOPER=1 (every test sets it) a block leaves the pool filled with 0xA5 bytes, fresh or recycled: a kernel that
// reads what nobody wrote then sees the same garbage in a fresh process as after a long session (round 3's H = 62k+2 border
// cells only showed with stale pool contents).  MHIP_POOL_POISON=0 keeps the blocks as they are (A/B timing runs).
bool pool_poison()
{
    static const bool on = [] {
        const char *d = getenv("MHIP_DEVELOPER");
        if (!(d && d[0] == '1')) return false;
        const char *e = getenv("MHIP_POOL_POISON");
        return !(e && e[0] == '0');
    }();
    return on;
}
int poison_block(void *p, size_t rs)
{
    // the block's last user synchronised before releasing it; the fill is ordered before anything the caller queues by the sync
    MH_HIP(hipMemsetAsync(p, 0xA5, rs, 0));
    MH_HIP(hipStreamSynchronize(0));
    return MHIP_OK;
}
}  // namespace

int pool_alloc(void **p, size_t bytes)
{
    int dev = 0;
    (void)hipGetDevice(&dev);
    const size_t rs = round_size(bytes);
    {
        std::unique_lock<std::mutex> lk(g_pool_mu);
        auto it = g_pool.find({dev, rs});
        if (it != g_pool.end()) {
            *p = it->second;
            g_pool.erase(it);
            g_pool_bytes -= rs;
            lk.unlock();
            return pool_poison() ? poison_block(*p, rs) : MHIP_OK;
        }
    }
    hipError_t e = hipMalloc(p, rs);
    if (e != hipSuccess) {  // drop the cache and retry once
        (void)hipGetLastError();
        {
            std::lock_guard<std::mutex> lk(g_pool_mu);
            for (auto &kv : g_pool) (void)hipFree(kv.second);
            g_pool.clear();
            g_pool_bytes = 0;
        }
        e = hipMalloc(p, rs);
    }
    if (e != hipSuccess) {
        *p = nullptr;
        set_error("hipMalloc(%zu) failed: %s", rs, hipGetErrorString(e));
        return MHIP_EHIP;
    }
    return pool_poison() ? poison_block(*p, rs) : MHIP_OK;
}

void pool_free(void *p, size_t bytes)
{
    int dev = 0;
    (void)hipGetDevice(&dev);
    const size_t rs = round_size(bytes);
    std::lock_guard<std::mutex> lk(g_pool_mu);
    if (g_pool_bytes + rs > POOL_CAP) {
        (void)hipFree(p);
        return;
    }
    g_pool.emplace(std::make_pair(dev, rs), p);
    g_pool_bytes += rs;
}

int require_device()
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n < 1) {
        (void)hipGetLastError();
        set_error("no HIP device available (libmalstroem_hip has no CPU fallback)");
        return MHIP_ENODEV;
    }
    return MHIP_OK;
}

int upload(DevBuf &b, const void *host, size_t bytes, hipStream_t s)
{
    MH_TRY(b.alloc(bytes));
    MH_HIP(hipMemcpyAsync(b.p, host, bytes, hipMemcpyHostToDevice, s));
    return MHIP_OK;
}
int download(void *host, const DevBuf &b, size_t bytes, hipStream_t s)
{
    MH_HIP(hipMemcpyAsync(host, b.p, bytes, hipMemcpyDeviceToHost, s));
    MH_HIP(stream_sync(s));
    return MHIP_OK;
}

// rank LUT of label.keep_labels + second connected_components (bluespots.py:167-170):
// rank = cumsum(keep) * keep with keep[0] forced False
int64_t build_rank_lut(const uint8_t *keep, int64_t nlab, std::vector<int32_t> &lut)
{
    lut.assign((size_t)nlab + 1, 0);
    int32_t run = 0;
    for (int64_t l = 1; l <= nlab; ++l)
        if (!keep || keep[l]) lut[(size_t)l] = ++run;
    return run;
}

}  // namespace mh

using namespace mh;

extern "C" {

const char *mhip_last_error(void) { return get_error(); }
const char *mhip_version(void) { return "malstroem_hip 0.1 (gfx950)"; }

int mhip_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

int mhip_set_device(int device)
{
    MH_TRY(require_device());
    MH_HIP(hipSetDevice(device));
    return MHIP_OK;
}

int mhip_read_bandwidth(int64_t bytes, int32_t reps, double *gbs)
{
    MH_ARG(bytes >= (1 << 20) && reps >= 1 && gbs, "read_bandwidth(bytes >= 1 MiB, reps >= 1, gbs)");
    MH_TRY(require_device());
    return read_bandwidth_dev((size_t)bytes & ~size_t(15), reps, gbs, 0);
}

int mhip_copy_bandwidth(int64_t bytes, int32_t reps, double *gbs)
{
    MH_ARG(bytes >= (1 << 20) && reps >= 1 && gbs, "copy_bandwidth(bytes >= 1 MiB, reps >= 1, gbs)");
    MH_TRY(require_device());
    return copy_bandwidth_dev((size_t)bytes & ~size_t(15), reps, gbs, 0);
}

}  // extern "C"
