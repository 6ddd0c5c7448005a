// api.hip -- extern "C" boundary of libmalstroem_hip.so (declared in include/malstroem_hip.h).
//
// Two layers over the device-pointer stage implementations (fill.hip, d8.hip, accum.hip, ccl.hip,
// label_ops.hip, watershed.hip):
//   * host-raster entry points: upload -> stage -> download, one per malstroem.algorithms stage function;
//   * mhip_ctx: device-resident DemTool/BluespotTool pipeline (reference dem.py:53-93, bluespots.py:138-216)
//     with HIP-event timing per stage.
// There is no CPU fallback anywhere in this file: without a HIP device every compute call returns MHIP_ENODEV.
#include <cstdarg>
#include <chrono>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "common.hpp"
#include <condition_variable>
#include <functional>
#include <atomic>
#include <future>
#include <thread>

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

static int require_device()
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n < 1) {
        (void)hipGetLastError();
        set_error("no HIP device available (libmalstroem_hip has no CPU fallback)");
        return MHIP_ENODEV;
    }
    return MHIP_OK;
}

static int upload(DevBuf &b, const void *host, size_t bytes, hipStream_t s)
{
    MH_TRY(b.alloc(bytes));
    MH_HIP(hipMemcpyAsync(b.p, host, bytes, hipMemcpyHostToDevice, s));
    return MHIP_OK;
}
static int download(void *host, const DevBuf &b, size_t bytes, hipStream_t s)
{
    MH_HIP(hipMemcpyAsync(host, b.p, bytes, hipMemcpyDeviceToHost, s));
    MH_HIP(stream_sync(s));
    return MHIP_OK;
}

// rank LUT of label.keep_labels + second connected_components (bluespots.py:167-170):
// rank = cumsum(keep) * keep with keep[0] forced False
static int64_t build_rank_lut(const uint8_t *keep, int64_t nlab, std::vector<int32_t> &lut)
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

int mhip_fill_f32(const float *dem, float *out, int64_t H, int64_t W, int32_t *out_rounds)
{
    MH_ARG(dem && out && H >= 1 && W >= 1, "fill_f32(dem, out, H>=1, W>=1)");
    MH_TRY(require_device());
    hipStream_t s = 0;
    const size_t n = (size_t)(H * W);
    DevBuf d_dem, d_out;
    MH_TRY(upload(d_dem, dem, n * 4, s));
    MH_TRY(d_out.alloc(n * 4));
    FillStats st;
    MH_TRY(fill_plain_dev(d_dem.as<float>(), d_out.as<float>(), H, W, s, &st));
    if (out_rounds) *out_rounds = st.rounds;
    return download(out, d_out, n * 4, s);
}

int mhip_fill_noflat_f64(const float *dem, double *out, int64_t H, int64_t W, double short_, double diag,
                         int32_t *out_rounds)
{
    MH_ARG(dem && out && H >= 1 && W >= 1, "fill_noflat_f64(dem, out, H>=1, W>=1)");
    MH_TRY(require_device());
    hipStream_t s = 0;
    const size_t n = (size_t)(H * W);
    DevBuf d_dem, d_out;
    MH_TRY(upload(d_dem, dem, n * 4, s));
    MH_TRY(d_out.alloc(n * 8));
    // plain fill first: it seeds the no-flats iteration with a rigorous upper bound (see fill_noflat_dev)
    DevBuf d_filled;
    MH_TRY(d_filled.alloc(n * 4));
    FillStats st0, st;
    MH_TRY(fill_plain_dev(d_dem.as<float>(), d_filled.as<float>(), H, W, s, &st0));
    MH_TRY(fill_noflat_dev(d_dem.as<float>(), d_out.as<double>(), H, W, short_, diag, s, &st, d_filled.as<float>()));
    if (out_rounds) *out_rounds = st.rounds + st0.rounds;
    return download(out, d_out, n * 8, s);
}

int mhip_short_diag(const float *dem, int64_t n, double *short_, double *diag)
{
    MH_ARG(dem && short_ && diag && n >= 1, "short_diag(dem, n>=1, short, diag)");
    MH_TRY(require_device());
    hipStream_t s = 0;
    DevBuf d_dem;
    MH_TRY(upload(d_dem, dem, (size_t)n * 4, s));
    return short_diag_dev(d_dem.as<float>(), n, short_, diag, s);
}

int mhip_depths_f32(const float *filled, const float *dem, float *out, int64_t n)
{
    MH_ARG(filled && dem && out && n >= 1, "depths_f32(filled, dem, out, n>=1)");
    MH_TRY(require_device());
    hipStream_t s = 0;
    DevBuf a, b, o;
    MH_TRY(upload(a, filled, (size_t)n * 4, s));
    MH_TRY(upload(b, dem, (size_t)n * 4, s));
    MH_TRY(o.alloc((size_t)n * 4));
    MH_TRY(depths_dev(a.as<float>(), b.as<float>(), o.as<float>(), n, s));
    return download(out, o, (size_t)n * 4, s);
}

int mhip_d8_f64(const double *z, uint8_t *out, int64_t H, int64_t W, int edges_outward)
{
    MH_ARG(z && out && H >= 1 && W >= 1, "d8_f64(z, out, H>=1, W>=1)");
    MH_TRY(require_device());
    hipStream_t s = 0;
    const size_t n = (size_t)(H * W);
    DevBuf d_z, d_o;
    MH_TRY(upload(d_z, z, n * 8, s));
    MH_TRY(d_o.alloc(n));
    MH_TRY(d8_dev(d_z.as<double>(), d_o.as<uint8_t>(), H, W, edges_outward, s));
    return download(out, d_o, n, s);
}

int mhip_accum(const uint8_t *flowdir, double *out, int64_t H, int64_t W)
{
    MH_ARG(flowdir && out && H >= 1 && W >= 1, "accum(flowdir, out, H>=1, W>=1)");
    MH_TRY(require_device());
    hipStream_t s = 0;
    const size_t n = (size_t)(H * W);
    DevBuf d_fd, d_o;
    MH_TRY(upload(d_fd, flowdir, n, s));
    MH_TRY(d_o.alloc(n * 8));
    MH_TRY(accum_dev(d_fd.as<uint8_t>(), d_o.as<double>(), H, W, s));
    return download(out, d_o, n * 8, s);
}

int mhip_ccl8_f32(const float *data, int32_t *labels, int64_t H, int64_t W, int64_t *nlabels)
{
    MH_ARG(data && labels && nlabels && H >= 1 && W >= 1, "ccl8_f32(data, labels, H>=1, W>=1, nlabels)");
    MH_TRY(require_device());
    hipStream_t s = 0;
    const size_t n = (size_t)(H * W);
    DevBuf d_d, d_l, d_t;
    MH_TRY(upload(d_d, data, n * 4, s));
    MH_TRY(d_l.alloc(n * 4));
    MH_TRY(d_t.alloc(n * 4));
    MH_TRY(ccl8_f32_dev(d_d.as<float>(), d_l.as<int32_t>(), d_t.as<int32_t>(), H, W, nlabels, s));
    return download(labels, d_l, n * 4, s);
}

int mhip_ccl8_u8(const uint8_t *data, int32_t *labels, int64_t H, int64_t W, int64_t *nlabels)
{
    MH_ARG(data && labels && nlabels && H >= 1 && W >= 1, "ccl8_u8(data, labels, H>=1, W>=1, nlabels)");
    MH_TRY(require_device());
    hipStream_t s = 0;
    const size_t n = (size_t)(H * W);
    DevBuf d_d, d_l, d_t;
    MH_TRY(upload(d_d, data, n, s));
    MH_TRY(d_l.alloc(n * 4));
    MH_TRY(d_t.alloc(n * 4));
    MH_TRY(ccl8_u8_dev(d_d.as<uint8_t>(), d_l.as<int32_t>(), d_t.as<int32_t>(), H, W, nlabels, s));
    return download(labels, d_l, n * 4, s);
}

int mhip_relabel_keep(int32_t *labels, const uint8_t *keep, int64_t nlab, int64_t n, int64_t *nkept)
{
    MH_ARG(labels && keep && nlab >= 0 && n >= 1, "relabel_keep(labels, keep, nlab>=0, n>=1)");
    MH_TRY(require_device());
    hipStream_t s = 0;
    std::vector<int32_t> lut;
    const int64_t kept = build_rank_lut(keep, nlab, lut);
    DevBuf d_l, d_lut;
    MH_TRY(upload(d_l, labels, (size_t)n * 4, s));
    MH_TRY(upload(d_lut, lut.data(), lut.size() * 4, s));
    MH_TRY(relabel_lut_dev(d_l.as<int32_t>(), d_lut.as<int32_t>(), nlab, n, s));
    if (nkept) *nkept = kept;
    return download(labels, d_l, (size_t)n * 4, s);
}

int mhip_keep_mask(const int32_t *labels, const uint8_t *keep, int64_t nlab, int64_t n, uint8_t *mask)
{
    MH_ARG(labels && keep && mask && nlab >= 0 && n >= 1, "keep_mask(labels, keep, nlab>=0, n>=1, mask)");
    MH_TRY(require_device());
    hipStream_t s = 0;
    DevBuf d_l, d_k, d_m;
    MH_TRY(upload(d_l, labels, (size_t)n * 4, s));
    MH_TRY(upload(d_k, keep, (size_t)nlab + 1, s));
    MH_TRY(d_m.alloc((size_t)n));
    MH_TRY(keep_mask_dev(d_l.as<int32_t>(), d_k.as<uint8_t>(), nlab, n, d_m.as<uint8_t>(), s));
    return download(mask, d_m, (size_t)n, s);
}

int mhip_label_stats_f32(const float *data, const int32_t *labels, int64_t n, int64_t nlab, mhip_stat_record *records)
{
    MH_ARG(data && labels && records && n >= 1 && nlab >= 0, "label_stats_f32(data, labels, n>=1, nlab>=0, records)");
    MH_TRY(require_device());
    hipStream_t s = 0;
    DevBuf d_d, d_l, d_r;
    MH_TRY(upload(d_d, data, (size_t)n * 4, s));
    MH_TRY(upload(d_l, labels, (size_t)n * 4, s));
    MH_TRY(d_r.alloc(sizeof(mhip_stat_record) * (size_t)(nlab + 1)));
    MH_TRY(label_stats_dev(d_d.as<float>(), d_l.as<int32_t>(), n, nlab, d_r.as<mhip_stat_record>(), s));
    MH_TRY(label_stats_zero_sign_dev(d_d.as<float>(), d_l.as<int32_t>(), n, nlab, d_r.as<mhip_stat_record>(), s));
    return download(records, d_r, sizeof(mhip_stat_record) * (size_t)(nlab + 1), s);
}

int mhip_label_stats_f64(const double *data, const int32_t *labels, int64_t n, int64_t nlab, mhip_stat_record *records)
{
    MH_ARG(data && labels && records && n >= 1 && nlab >= 0, "label_stats_f64(data, labels, n>=1, nlab>=0, records)");
    MH_TRY(require_device());
    hipStream_t s = 0;
    DevBuf d_d, d_l, d_r;
    MH_TRY(upload(d_d, data, (size_t)n * 8, s));
    MH_TRY(upload(d_l, labels, (size_t)n * 4, s));
    MH_TRY(d_r.alloc(sizeof(mhip_stat_record) * (size_t)(nlab + 1)));
    MH_TRY(label_stats64_dev(d_d.as<double>(), d_l.as<int32_t>(), n, nlab, d_r.as<mhip_stat_record>(), s));
    MH_TRY(label_stats_zero_sign_dev(d_d.as<double>(), d_l.as<int32_t>(), n, nlab, d_r.as<mhip_stat_record>(), s));
    return download(records, d_r, sizeof(mhip_stat_record) * (size_t)(nlab + 1), s);
}

static int label_arg_host(const double *data, const int32_t *labels, int64_t H, int64_t W, int64_t nlab, bool is_max,
                          mhip_index_record *records)
{
    MH_ARG(data && labels && records && H >= 1 && W >= 1 && nlab >= 0, "label_arg(data, labels, H>=1, W>=1, nlab>=0, records)");
    MH_TRY(require_device());
    hipStream_t s = 0;
    const size_t n = (size_t)(H * W);
    DevBuf d_d, d_l, d_r;
    MH_TRY(upload(d_d, data, n * 8, s));
    MH_TRY(upload(d_l, labels, n * 4, s));
    MH_TRY(d_r.alloc(sizeof(mhip_index_record) * (size_t)(nlab + 1)));
    MH_TRY(label_arg_dev(d_d.as<double>(), d_l.as<int32_t>(), H, W, nlab, is_max, d_r.as<mhip_index_record>(), s));
    return download(records, d_r, sizeof(mhip_index_record) * (size_t)(nlab + 1), s);
}

int mhip_label_argmin_f64(const double *data, const int32_t *labels, int64_t H, int64_t W, int64_t nlab,
                          mhip_index_record *records)
{
    return label_arg_host(data, labels, H, W, nlab, false, records);
}
int mhip_label_argmax_f64(const double *data, const int32_t *labels, int64_t H, int64_t W, int64_t nlab,
                          mhip_index_record *records)
{
    return label_arg_host(data, labels, H, W, nlab, true, records);
}

int mhip_label_count(const int32_t *labels, int64_t n, int64_t nlab, int64_t *counts)
{
    MH_ARG(labels && counts && n >= 1 && nlab >= 0, "label_count(labels, n>=1, nlab>=0, counts)");
    MH_TRY(require_device());
    hipStream_t s = 0;
    DevBuf d_l, d_c;
    MH_TRY(upload(d_l, labels, (size_t)n * 4, s));
    MH_TRY(d_c.alloc(8 * (size_t)(nlab + 1)));
    MH_TRY(label_count_dev(d_l.as<int32_t>(), n, nlab, d_c.as<int64_t>(), s));
    return download(counts, d_c, 8 * (size_t)(nlab + 1), s);
}

int mhip_label_max(const int32_t *labels, int64_t n, int32_t *out_max)
{
    MH_ARG(labels && out_max && n >= 1, "label_max(labels, n>=1, out)");
    MH_TRY(require_device());
    hipStream_t s = 0;
    DevBuf d_l;
    MH_TRY(upload(d_l, labels, (size_t)n * 4, s));
    return label_max_dev(d_l.as<int32_t>(), n, out_max, s);
}

/* ---- hypsometry tables, water levels, final depths on host arrays (hyps.hip; the context entry points launch the same kernels) ---- */
static bool hyps_res_ok(double res) { return res > 0.0 && res <= 1.7976931348623157e308; }   // (false for NaN)

// offsets[0 .. nlab + 1] as mhip_label_hyps_layout makes them: 0, 0, then strictly increasing, at most HYPS_MAX_BINS in all
static int hyps_check_offsets(const int64_t *offsets, int64_t nlab, int64_t *total)
{
    bool ok = offsets[0] == 0 && offsets[1] == 0;
    for (int64_t l = 1; ok && l <= nlab; ++l) ok = offsets[l + 1] > offsets[l];
    if (!ok || offsets[nlab + 1] > HYPS_MAX_BINS) {
        set_error("offsets are no hypsometry layout of %lld labels (0, 0, then strictly increasing, at most 2**30 bins)", (long long)nlab);
        return MHIP_EINVAL;
    }
    *total = offsets[nlab + 1];
    return MHIP_OK;
}

int mhip_label_hyps_layout(const double *dmax, int64_t nlab, double res, int64_t *offsets, int64_t *total)
{
    MH_ARG(dmax && offsets && total && nlab >= 0 && hyps_res_ok(res), "label_hyps_layout(dmax, nlab>=0, 0 < res < inf, offsets, total)");
    MH_TRY(require_device());
    hipStream_t s = 0;
    DevBuf d_m, d_o;
    MH_TRY(upload(d_m, dmax, 8 * (size_t)(nlab + 1), s));
    MH_TRY(d_o.alloc(8 * (size_t)(nlab + 2)));
    MH_TRY(hyps_layout_dev(d_m.as<double>(), 1, nlab, res, d_o.as<int64_t>(), total, s));
    return download(offsets, d_o, 8 * (size_t)(nlab + 2), s);
}

int mhip_label_hyps_f32(const float *data, const int32_t *labels, int64_t n, int64_t W, int64_t nlab, double res, const int64_t *offsets,
                        int64_t *counts, double *sums, int64_t *lds_spills)
{
    MH_ARG(data && labels && offsets && counts && sums && n >= 1 && W >= 0 && nlab >= 0 && hyps_res_ok(res),
           "label_hyps_f32(data, labels, n>=1, W>=0, nlab>=0, 0 < res < inf, offsets, counts, sums)");
    int64_t total = 0;
    MH_TRY(hyps_check_offsets(offsets, nlab, &total));
    MH_TRY(require_device());
    hipStream_t s = 0;
    DevBuf d_d, d_l, d_o, d_c, d_s;
    MH_TRY(upload(d_d, data, (size_t)n * 4, s));
    MH_TRY(upload(d_l, labels, (size_t)n * 4, s));
    MH_TRY(upload(d_o, offsets, 8 * (size_t)(nlab + 2), s));
    MH_TRY(d_c.alloc(4 * (size_t)total));
    MH_TRY(d_s.alloc(8 * (size_t)total));
    MH_TRY(hyps_table_dev(d_d.as<float>(), d_l.as<int32_t>(), n, W, nlab, res, d_o.as<int64_t>(), total, d_c.as<uint32_t>(), d_s.as<double>(),
                          lds_spills, s));
    if (total == 0) return MHIP_OK;
    std::vector<uint32_t> c32((size_t)total);
    MH_HIP(hipMemcpyAsync(c32.data(), d_c.p, 4 * (size_t)total, hipMemcpyDeviceToHost, s));
    MH_TRY(download(sums, d_s, 8 * (size_t)total, s));
    for (int64_t k = 0; k < total; ++k) counts[k] = (int64_t)c32[(size_t)k];
    return MHIP_OK;
}

int mhip_hyps_levels(int64_t nlab, const int64_t *offsets, const int64_t *counts, const double *sums, const double *dmax, const double *q,
                     mhip_final_record *records)
{
    MH_ARG(offsets && counts && sums && dmax && q && records && nlab >= 0, "hyps_levels(nlab>=0, offsets, counts, sums, dmax, q, records)");
    int64_t total = 0;
    MH_TRY(hyps_check_offsets(offsets, nlab, &total));
    std::vector<uint32_t> c32((size_t)total + 1);
    for (int64_t k = 0; k < total; ++k) {
        MH_ARG(counts[k] >= 0 && counts[k] < ((int64_t)1 << 31), "hyps_levels: a count outside [0, 2**31)");
        c32[(size_t)k] = (uint32_t)counts[k];
    }
    MH_TRY(require_device());
    hipStream_t s = 0;
    DevBuf d_o, d_c, d_s, d_m, d_q, d_r;
    MH_TRY(upload(d_o, offsets, 8 * (size_t)(nlab + 2), s));
    MH_TRY(upload(d_c, c32.data(), 4 * ((size_t)total + 1), s));
    MH_TRY(d_s.alloc(8 * (size_t)total));
    if (total) MH_HIP(hipMemcpyAsync(d_s.p, sums, 8 * (size_t)total, hipMemcpyHostToDevice, s));
    MH_TRY(upload(d_m, dmax, 8 * (size_t)(nlab + 1), s));
    MH_TRY(upload(d_q, q, 8 * (size_t)(nlab + 1), s));
    MH_TRY(d_r.alloc(sizeof(mhip_final_record) * (size_t)(nlab + 1)));
    MH_TRY(hyps_levels_dev(nlab, d_o.as<int64_t>(), d_c.as<uint32_t>(), d_s.as<double>(), d_m.as<double>(), 1, d_q.as<double>(),
                           d_r.as<mhip_final_record>(), s));
    return download(records, d_r, sizeof(mhip_final_record) * (size_t)(nlab + 1), s);
}

int mhip_final_depths_f32(const float *data, const int32_t *labels, int64_t n, int64_t W, int64_t nlab, mhip_final_record *records, float *out)
{
    MH_ARG(data && labels && records && out && n >= 1 && W >= 0 && nlab >= 0, "final_depths_f32(data, labels, n>=1, W>=0, nlab>=0, records, out)");
    MH_TRY(require_device());
    hipStream_t s = 0;
    std::vector<mhip_final_record> rec(records, records + nlab + 1);
    for (auto &r : rec) r.wet_cells = 0;
    DevBuf d_d, d_l, d_r, d_out;
    MH_TRY(upload(d_d, data, (size_t)n * 4, s));
    MH_TRY(upload(d_l, labels, (size_t)n * 4, s));
    MH_TRY(upload(d_r, rec.data(), sizeof(mhip_final_record) * (size_t)(nlab + 1), s));
    MH_TRY(d_out.alloc((size_t)n * 4));
    MH_TRY(final_depths_dev(d_d.as<float>(), d_l.as<int32_t>(), n, W, nlab, d_r.as<mhip_final_record>(), d_out.as<float>(), s));
    MH_HIP(hipMemcpyAsync(records, d_r.p, sizeof(mhip_final_record) * (size_t)(nlab + 1), hipMemcpyDeviceToHost, s));
    return download(out, d_out, (size_t)n * 4, s);
}

int mhip_watersheds_i32(const uint8_t *flowdir, int32_t *labels, int64_t H, int64_t W, int32_t unassigned)
{
    MH_ARG(flowdir && labels && H >= 1 && W >= 1, "watersheds_i32(flowdir, labels, H>=1, W>=1)");
    MH_TRY(require_device());
    hipStream_t s = 0;
    const size_t n = (size_t)(H * W);
    DevBuf d_fd, d_l;
    MH_TRY(upload(d_fd, flowdir, n, s));
    MH_TRY(upload(d_l, labels, n * 4, s));
    MH_TRY(watersheds_dev(d_fd.as<uint8_t>(), d_l.as<int32_t>(), H, W, unassigned, s));
    return download(labels, d_l, n * 4, s);
}

/* net.next_downstream_label for a batch of cells (reference net.py:142-169): labels / found flags / path lengths, and -- when
 * offsets (n + 1 prefix sums of the lengths of an earlier call) and out_cells are given -- the cells of every path as linear
 * indices row * W + col.  The two rasters are host arrays here; mhip_ctx_trace_downstream walks the resident ones. */
static int trace_on_device(const uint8_t *d_fd, const int32_t *d_lab, int64_t H, int64_t W, const int64_t *cells_rc, int64_t n, int use_bg,
                           int32_t bg, int32_t *out_label, int32_t *out_found, int64_t *out_len, const int64_t *offsets, int64_t *out_cells,
                           hipStream_t s)
{
    DevBuf d_c, d_l, d_f, d_n, d_o, d_p;
    MH_TRY(upload(d_c, cells_rc, (size_t)n * 16, s));
    MH_TRY(d_l.alloc((size_t)n * 4));
    MH_TRY(d_f.alloc((size_t)n * 4));
    MH_TRY(d_n.alloc((size_t)n * 8));
    int64_t total = 0;
    if (offsets && out_cells) {
        total = offsets[n];
        MH_ARG(total >= 0, "trace: offsets[n] must be the total path length");
        MH_TRY(upload(d_o, offsets, (size_t)(n + 1) * 8, s));
        MH_TRY(d_p.alloc((size_t)(total > 0 ? total : 1) * 8));
    }
    MH_TRY(trace_downstream_dev(d_fd, d_lab, H, W, d_c.as<int64_t>(), n, use_bg, bg, d_l.as<int32_t>(), d_f.as<int32_t>(), d_n.as<int64_t>(),
                                total ? d_o.as<int64_t>() : nullptr, total ? d_p.as<int64_t>() : nullptr, s));
    if (out_label) MH_HIP(hipMemcpyAsync(out_label, d_l.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    if (out_found) MH_HIP(hipMemcpyAsync(out_found, d_f.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    if (out_len) MH_HIP(hipMemcpyAsync(out_len, d_n.p, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    if (total) MH_HIP(hipMemcpyAsync(out_cells, d_p.p, (size_t)total * 8, hipMemcpyDeviceToHost, s));
    MH_HIP(stream_sync(s));
    return MHIP_OK;
}

int mhip_trace_downstream_i32(const uint8_t *flowdir, const int32_t *labels, int64_t H, int64_t W, const int64_t *cells_rc, int64_t n,
                              int use_background, int32_t background, int32_t *out_label, int32_t *out_found, int64_t *out_len,
                              const int64_t *offsets, int64_t *out_cells)
{
    MH_ARG(flowdir && labels && H >= 1 && W >= 1 && n >= 0 && (n == 0 || cells_rc), "trace_downstream_i32(flowdir, labels, H, W, cells, n, ...)");
    MH_TRY(require_device());
    if (n == 0) return MHIP_OK;
    hipStream_t s = 0;
    const size_t nc = (size_t)(H * W);
    DevBuf d_fd, d_lab;
    MH_TRY(upload(d_fd, flowdir, nc, s));
    MH_TRY(upload(d_lab, labels, nc * 4, s));
    return trace_on_device(d_fd.as<uint8_t>(), d_lab.as<int32_t>(), H, W, cells_rc, n, use_background, background, out_label, out_found, out_len,
                           offsets, out_cells, s);
}

/* ================================================================================================
 * device-resident pipeline
 * ================================================================================================ */

// One helper thread per context, started with the first request that overlaps its two branches and parked on a condition variable in
// between: mhip_ctx_run used to create (and join) a std::thread per call.
class SideThread {
    std::thread th_;
    std::mutex mu_;
    std::condition_variable cv_;
    std::function<void()> task_;
    bool busy_ = false, stop_ = false;

public:
    ~SideThread()
    {
        {
            std::lock_guard<std::mutex> lk(mu_);
            stop_ = true;
        }
        cv_.notify_all();
        if (th_.joinable()) th_.join();
    }
    void run(std::function<void()> f)      // the caller must wait() before the objects `f` refers to go away
    {
        std::unique_lock<std::mutex> lk(mu_);
        if (!th_.joinable())
            th_ = std::thread([this] {
                std::unique_lock<std::mutex> l2(mu_);
                for (;;) {
                    cv_.wait(l2, [this] { return stop_ || (busy_ && task_); });
                    if (stop_) return;
                    std::function<void()> f2 = std::move(task_);
                    task_ = nullptr;
                    l2.unlock();
                    f2();
                    l2.lock();
                    busy_ = false;
                    cv_.notify_all();
                }
            });
        task_ = std::move(f);
        busy_ = true;
        cv_.notify_all();
    }
    void wait()
    {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [this] { return !busy_; });
    }
};

struct mhip_ctx {
    SideThread side;        // drives the label branch of mhip_ctx_run
    int64_t H = 0, W = 0;   // local raster: owned rows + halo rows
    int64_t H_global = 0, row0 = 0, H_owned = 0;
    int ht = 0, hb = 0;     // 1 if a halo row (copy of the neighbouring band's edge row) sits above / below the owned rows
    FillRun *run[2] = {nullptr, nullptr};   // resumable fill (plain, no-flats) in band mode
    GeoRun *geo = nullptr;                  // ... and the geodesic no-flats fill
    PfRun *pf = nullptr;                    // ... and the tiled priority-flood (plain fill)
    bool pf_done = false;                   // the flood's raster is written and proven (mhip_ctx_fill_certify); run[0] may follow it
    DevBuf nodir_cnt;                       // interior NODIR cells of FLOWDIR, counted by the D8 kernel (the watersheds' fast-path test)
    bool nodir_valid = false;
    int device = 0, rank = 0, nranks = 1;
    hipStream_t stream = nullptr;
    DevBuf r[MHIP_R_COUNT_];
    bool have[MHIP_R_COUNT_] = {};
    DevBuf tmp_i32;         // CCL parent scratch
    CclKeep ccl_keep;       // a row band's labelling between its two halves (mhip_ctx_band_ccl_begin / _finish)
    bool ccl_pending = false;
    bool pf_depths = false;  // the band flood's last pass (mhip_ctx_fill_certify) wrote the depths of the owned rows
    DevBuf raw_stats, stats, ws_counts, pour;
    AccumKeep acc_keep;     // row band: the perimeter graph of mhip_ctx_band_accum_boundary, for the ACCUM run that follows the exchange
    int accum_algorithm = 0;   // 0: full accumulation, 1: the band's second pass as a delta over the kept graph
    DevBuf pp_mask0, pp_list, pp_tiles, pp_misc, pp_key;    // pour-point candidates on their way from the watersheds to the accumulation (PourLink)
    hipEvent_t ev_cand = nullptr;
    int pour_algorithm = 0;
    int64_t nlabels_raw = -1, nlabels = -1;
    bool labels_components = false;   // LABELS came from the library's own labelling (not uploaded): 8-connected components
    bool labels_filtered = false;
    bool stats_valid = false;         // `stats` are the label_stats of the resident DEPTHS by the resident LABELS
    // hypsometry of the resident labels (mhip_ctx_hyps): layout, table, and the records of the last mhip_ctx_final_depths
    DevBuf hyps_off, hyps_cnt, hyps_sum, hyps_rec;
    int64_t hyps_total = -1, hyps_spills = 0;     // -1: no table of the resident depths and labels
    double sh = 0, dg = 0;
    int32_t fill_rounds = 0, noflat_rounds = 0;
    FillStats fill_st, noflat_st;
    std::map<int, std::pair<hipEvent_t, hipEvent_t>> ev;
    std::map<int, bool> ev_valid;
    void *comm = nullptr;   // RCCL communicator over all bands (comm.hip); nullptr: the launcher moves the rows
    void *comm_b = nullptr; // a second one for the thread between mhip_ctx_side_begin / _end (two threads never share a communicator)
    DevBuf comm_stage, comm_word, comm_flags, comm_stage_b;
    // second stream + fork/join events of the stage DAG (mhip_ctx_run)
    hipStream_t stream_b = nullptr, stream_c = nullptr;
    hipEvent_t ev_fork = nullptr, ev_flowdir = nullptr, ev_join = nullptr, ev_label = nullptr, ev_tail = nullptr;
};

static size_t raster_elem(int which)
{
    switch (which) {
    case MHIP_R_DEM: case MHIP_R_FILLED: case MHIP_R_DEPTHS: case MHIP_R_LABELS: case MHIP_R_WATERSHEDS: case MHIP_R_NGDIST:
    case MHIP_R_FINALDEPTHS: return 4;
    case MHIP_R_NOFLAT: case MHIP_R_ACCUM: return 8;
    case MHIP_R_FLOWDIR: return 1;
    default: return 0;
    }
}

static int ctx_raster(mhip_ctx *c, int which)
{
    if (!c->r[which].p) MH_TRY(c->r[which].alloc(raster_elem(which) * (size_t)(c->H * c->W)));
    return MHIP_OK;
}

constexpr int HYPS_KERNEL_SLOT = 1 << 29, FINAL_KERNEL_SLOT = 1 << 28;      // event pairs of single kernels (mhip_ctx_kernel_ms)
static int ctx_events(mhip_ctx *c, int stage, hipEvent_t **a, hipEvent_t **b)
{
    auto it = c->ev.find(stage);
    if (it == c->ev.end()) {
        hipEvent_t e0, e1;
        MH_HIP(hipEventCreate(&e0));
        MH_HIP(hipEventCreate(&e1));
        it = c->ev.emplace(stage, std::make_pair(e0, e1)).first;
    }
    *a = &it->second.first;
    *b = &it->second.second;
    return MHIP_OK;
}

int mhip_comm_available(void) { return comm_available(); }

int mhip_comm_unique_id(void *id128)
{
    MH_ARG(id128, "comm_unique_id(id128)");
    MH_TRY(require_device());
    return comm_unique_id(id128);
}

int mhip_ctx_create_band(mhip_ctx **out, int64_t H_global, int64_t W, int64_t row0, int64_t H_local, int device, int rank,
                         int nranks, const void *nccl_unique_id)
{
    MH_ARG(out && H_global >= 1 && W >= 1 && H_local >= 1 && row0 >= 0 && row0 + H_local <= H_global, "ctx_create_band geometry");
    MH_ARG(rank >= 0 && nranks >= 1 && rank < nranks, "ctx_create_band(rank, nranks)");
    MH_TRY(require_device());
    MH_HIP(hipSetDevice(device));
    void *comm = nullptr;
    if (nccl_unique_id) MH_TRY(comm_create(&comm, nccl_unique_id, rank, nranks));   // collective over all bands
    mhip_ctx *c = new mhip_ctx();
    c->comm = comm;
    c->ht = row0 > 0 ? 1 : 0;
    c->hb = row0 + H_local < H_global ? 1 : 0;
    c->H_owned = H_local;
    c->H = H_local + c->ht + c->hb;
    c->W = W; c->H_global = H_global; c->row0 = row0;
    c->device = device; c->rank = rank; c->nranks = nranks;
    // the main stream carries the critical path (fill -> no-flats -> D8 -> accumulation): highest priority; the label / watershed
    // branch of mhip_ctx_run fills the gaps on streams of the lowest
    int prio_least = 0, prio_greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
    if (hipStreamCreateWithPriority(&c->stream, hipStreamDefault, prio_greatest) != hipSuccess) {
        comm_destroy(c->comm);
        delete c;
        set_error("hipStreamCreate failed");
        return MHIP_EHIP;
    }
    *out = c;
    return MHIP_OK;
}

int mhip_ctx_create(mhip_ctx **out, int64_t H, int64_t W, int device)
{
    return mhip_ctx_create_band(out, H, W, 0, H, device, 0, 1, nullptr);
}

int mhip_ctx_destroy(mhip_ctx *c)
{
    if (!c) return MHIP_OK;
    (void)hipSetDevice(c->device);
    (void)stream_sync(c->stream);
    for (auto &kv : c->ev) {
        (void)hipEventDestroy(kv.second.first);
        (void)hipEventDestroy(kv.second.second);
    }
    (void)hipStreamDestroy(c->stream);
    for (hipStream_t st : {c->stream_b, c->stream_c}) {
        if (st) {
            (void)stream_sync(st);
            (void)hipStreamDestroy(st);
        }
    }
    for (hipEvent_t e : {c->ev_fork, c->ev_flowdir, c->ev_join, c->ev_label, c->ev_tail, c->ev_cand})
        if (e) (void)hipEventDestroy(e);
    delete c->geo;
    delete c->pf;
    delete c->run[0];
    delete c->run[1];
    comm_destroy(c->comm);
    comm_destroy(c->comm_b);
    delete c;
    return MHIP_OK;
}

// Band launcher with two host threads (distributed.BandPipeline.run_chain): the thread that drives the labelling branch
// brackets its calls with mhip_ctx_side_begin / _end; in between, the data-movement and band entry points it calls run on
// the context's side stream, next to the fills the main thread keeps launching on the main stream.
static thread_local mhip_ctx *t_side_ctx = nullptr;
static hipStream_t cs(mhip_ctx *c) { return (t_side_ctx == c && c->stream_b) ? c->stream_b : c->stream; }
// ... and every RCCL call of that thread goes over the context's SECOND communicator (mhip_ctx_comm_add_side): the order of the
// operations on one communicator must be the same on every rank, which two threads sharing one cannot promise
static bool on_side(mhip_ctx *c) { return t_side_ctx == c; }

int mhip_ctx_comm_add_side(mhip_ctx *c, const void *nccl_unique_id)
{
    MH_ARG(c && nccl_unique_id && c->comm && !c->comm_b, "ctx_comm_add_side(ctx, id) needs a band context with a communicator and no side communicator yet");
    MH_HIP(hipSetDevice(c->device));
    return comm_create(&c->comm_b, nccl_unique_id, c->rank, c->nranks);     // collective over all bands
}

int mhip_ctx_side_begin(mhip_ctx *c)
{
    MH_ARG(c, "ctx");
    MH_HIP(hipSetDevice(c->device));
    if (!c->stream_b) MH_HIP(hipStreamCreateWithFlags(&c->stream_b, hipStreamNonBlocking));      // (a higher or lower priority moves nothing: measured in round 4)
    if (!c->ev_fork) {
        MH_HIP(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
        MH_HIP(hipEventCreateWithFlags(&c->ev_flowdir, hipEventDisableTiming));
        MH_HIP(hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming));
        MH_HIP(hipEventCreateWithFlags(&c->ev_label, hipEventDisableTiming));
        MH_HIP(hipEventCreateWithFlags(&c->ev_tail, hipEventDisableTiming));
    }
    MH_HIP(hipEventRecord(c->ev_fork, c->stream));          // everything the main stream has been given so far ...
    MH_HIP(hipStreamWaitEvent(c->stream_b, c->ev_fork, 0));  // ... is visible to the side stream
    t_side_ctx = c;
    return MHIP_OK;
}

int mhip_ctx_side_end(mhip_ctx *c)
{
    MH_ARG(c && t_side_ctx == c, "ctx_side_end without ctx_side_begin on this thread");
    MH_HIP(hipSetDevice(c->device));
    MH_HIP(stream_sync(c->stream_b));
    t_side_ctx = nullptr;
    return MHIP_OK;
}

int mhip_ctx_upload(mhip_ctx *c, int which, const void *host)
{
    MH_ARG(c && host && which >= 0 && which < MHIP_R_COUNT_, "ctx_upload(ctx, which, host)");
    MH_HIP(hipSetDevice(c->device));
    MH_TRY(ctx_raster(c, which));
    const size_t rowb = raster_elem(which) * (size_t)c->W;
    MH_HIP(hipMemcpyAsync(c->r[which].as<char>() + rowb * c->ht, host, rowb * (size_t)c->H_owned, hipMemcpyHostToDevice, cs(c)));
    MH_HIP(stream_sync(cs(c)));
    c->have[which] = true;
    if (which == MHIP_R_DEM) {  // a new DEM invalidates everything derived from the previous one
        for (int k = 0; k < MHIP_R_COUNT_; ++k)
            if (k != MHIP_R_DEM) c->have[k] = false;
        c->fill_st.have_minmax = false;      // (the extremes the last flood folded were the old DEM's)
    }
    if (which == MHIP_R_FILLED) c->fill_st.have_minmax = false;      // (an uploaded surface: no flood of this context saw its DEM)
    if (which == MHIP_R_LABELS) { c->nlabels = -1; c->nlabels_raw = -1; c->labels_filtered = true; c->labels_components = false; }
    if (which == MHIP_R_FLOWDIR) c->nodir_valid = false;
    if (which == MHIP_R_FLOWDIR || which == MHIP_R_DEM || which == MHIP_R_ACCUM) c->acc_keep.valid = false;
    if (which == MHIP_R_DEM || which == MHIP_R_DEPTHS || which == MHIP_R_LABELS) { c->stats_valid = false; c->hyps_total = -1; }
    return MHIP_OK;
}

int mhip_ctx_upload_dem(mhip_ctx *c, const float *dem) { return mhip_ctx_upload(c, MHIP_R_DEM, dem); }

/* Windowed transfers (reference io.py:21-159 moves whole rasters through the host): rows [row0, row0 + nrows) of the OWNED
 * raster.  A raster counts as present once its last row has been uploaded; uploading DEM rows invalidates what was derived
 * from the previous DEM.  The host side needs one window, whatever the raster's size. */
int mhip_ctx_upload_rows(mhip_ctx *c, int which, int64_t row0, int64_t nrows, const void *host)
{
    MH_ARG(c && host && which >= 0 && which < MHIP_R_COUNT_ && row0 >= 0 && nrows >= 1 && row0 + nrows <= c->H_owned,
           "ctx_upload_rows(ctx, which, row0, nrows, host)");
    MH_HIP(hipSetDevice(c->device));
    MH_TRY(ctx_raster(c, which));
    const size_t rowb = raster_elem(which) * (size_t)c->W;
    if (which == MHIP_R_DEM)
        for (int k = 0; k < MHIP_R_COUNT_; ++k) c->have[k] = false;
    if (which == MHIP_R_DEM || which == MHIP_R_FILLED) c->fill_st.have_minmax = false;
    if (which == MHIP_R_FLOWDIR) c->nodir_valid = false;
    if (which == MHIP_R_DEM || which == MHIP_R_DEPTHS || which == MHIP_R_LABELS) { c->stats_valid = false; c->hyps_total = -1; }
    MH_HIP(hipMemcpyAsync(c->r[which].as<char>() + rowb * (size_t)(c->ht + row0), host, rowb * (size_t)nrows, hipMemcpyHostToDevice, cs(c)));
    MH_HIP(stream_sync(cs(c)));      // the caller reuses its window buffer
    if (row0 + nrows == c->H_owned) {
        c->have[which] = true;
        if (which == MHIP_R_LABELS) { c->nlabels = -1; c->nlabels_raw = -1; c->labels_filtered = true; c->labels_components = false; }
    }
    return MHIP_OK;
}

int mhip_ctx_download_rows(mhip_ctx *c, int which, int64_t row0, int64_t nrows, void *host)
{
    MH_ARG(c && host && which >= 0 && which < MHIP_R_COUNT_ && row0 >= 0 && nrows >= 1 && row0 + nrows <= c->H_owned,
           "ctx_download_rows(ctx, which, row0, nrows, host)");
    MH_ARG(c->have[which], "raster has not been computed or uploaded");
    MH_HIP(hipSetDevice(c->device));
    const size_t rowb = raster_elem(which) * (size_t)c->W;
    MH_HIP(hipMemcpyAsync(host, c->r[which].as<char>() + rowb * (size_t)(c->ht + row0), rowb * (size_t)nrows, hipMemcpyDeviceToHost, cs(c)));
    MH_HIP(stream_sync(cs(c)));
    return MHIP_OK;
}

int mhip_ctx_download(mhip_ctx *c, int which, void *host)
{
    MH_ARG(c && host && which >= 0 && which < MHIP_R_COUNT_, "ctx_download(ctx, which, host)");
    MH_ARG(c->have[which], "raster has not been computed or uploaded");
    MH_HIP(hipSetDevice(c->device));
    const size_t rowb = raster_elem(which) * (size_t)c->W;
    MH_HIP(hipMemcpyAsync(host, c->r[which].as<char>() + rowb * c->ht, rowb * (size_t)c->H_owned, hipMemcpyDeviceToHost, cs(c)));
    MH_HIP(stream_sync(cs(c)));
    return MHIP_OK;
}

/* ---- row-band helpers: the host launcher moves edge rows between neighbouring bands -------------------------- */

int mhip_ctx_band_info(mhip_ctx *c, int64_t *row_off, int64_t *rows_local, int32_t *halo_top, int32_t *halo_bottom)
{
    MH_ARG(c, "ctx");
    if (row_off) *row_off = c->row0 - c->ht;
    if (rows_local) *rows_local = c->H;
    if (halo_top) *halo_top = c->ht;
    if (halo_bottom) *halo_bottom = c->hb;
    return MHIP_OK;
}

int mhip_ctx_get_edge_row(mhip_ctx *c, int which, int side, void *host)
{
    MH_ARG(c && host && which >= 0 && which < MHIP_R_COUNT_ && side >= 0 && side <= 3, "ctx_get_edge_row(ctx, which, side, host)");
    MH_ARG(c->r[which].p, "raster has not been computed or uploaded");
    MH_ARG(side < 2 || (side == 2 ? c->ht : c->hb), "this band has no halo row on that side");
    MH_HIP(hipSetDevice(c->device));
    const size_t rowb = raster_elem(which) * (size_t)c->W;
    const int64_t row = side == 0 ? c->ht : side == 1 ? c->ht + c->H_owned - 1 : side == 2 ? 0 : c->H - 1;
    MH_HIP(hipMemcpyAsync(host, c->r[which].as<char>() + rowb * row, rowb, hipMemcpyDeviceToHost, cs(c)));
    MH_HIP(stream_sync(cs(c)));
    return MHIP_OK;
}

int mhip_ctx_set_halo_row(mhip_ctx *c, int which, int side, const void *host, int32_t *changed)
{
    MH_ARG(c && host && which >= 0 && which < MHIP_R_COUNT_ && (side == 0 || side == 1), "ctx_set_halo_row(ctx, which, side, host)");
    MH_ARG(side == 0 ? c->ht : c->hb, "this band has no halo row on that side");
    MH_HIP(hipSetDevice(c->device));
    MH_TRY(ctx_raster(c, which));
    const size_t rowb = raster_elem(which) * (size_t)c->W;
    const int64_t row = side == 0 ? 0 : c->H - 1;
    DevBuf tmp;
    MH_TRY(tmp.alloc(rowb));
    MH_HIP(hipMemcpyAsync(tmp.p, host, rowb, hipMemcpyHostToDevice, cs(c)));
    int ch = 0;
    MH_TRY(row_update_dev(c->r[which].as<char>() + rowb * row, tmp.p, (int64_t)rowb, &ch, cs(c)));
    if (changed) *changed = ch;
    return MHIP_OK;
}

// the same two calls for a transport that moves DEVICE buffers (RCCL send/recv on tensors of the launcher)
int mhip_ctx_get_edge_row_dev(mhip_ctx *c, int which, int side, void *dev_dst)
{
    MH_ARG(c && dev_dst && which >= 0 && which < MHIP_R_COUNT_ && side >= 0 && side <= 3, "ctx_get_edge_row_dev(ctx, which, side, dev)");
    MH_ARG(c->r[which].p, "raster has not been computed or uploaded");
    MH_ARG(side < 2 || (side == 2 ? c->ht : c->hb), "this band has no halo row on that side");
    MH_HIP(hipSetDevice(c->device));
    const size_t rowb = raster_elem(which) * (size_t)c->W;
    const int64_t row = side == 0 ? c->ht : side == 1 ? c->ht + c->H_owned - 1 : side == 2 ? 0 : c->H - 1;
    MH_HIP(hipMemcpyAsync(dev_dst, c->r[which].as<char>() + rowb * row, rowb, hipMemcpyDeviceToDevice, cs(c)));
    MH_HIP(stream_sync(cs(c)));   // the transport reads the buffer on its own stream
    return MHIP_OK;
}

int mhip_ctx_set_halo_row_dev(mhip_ctx *c, int which, int side, const void *dev_src, int32_t *changed)
{
    MH_ARG(c && dev_src && which >= 0 && which < MHIP_R_COUNT_ && (side == 0 || side == 1), "ctx_set_halo_row_dev(ctx, which, side, dev)");
    MH_ARG(side == 0 ? c->ht : c->hb, "this band has no halo row on that side");
    MH_HIP(hipSetDevice(c->device));
    MH_TRY(ctx_raster(c, which));
    const size_t rowb = raster_elem(which) * (size_t)c->W;
    const int64_t row = side == 0 ? 0 : c->H - 1;
    int ch = 0;
    MH_TRY(row_update_dev(c->r[which].as<char>() + rowb * row, dev_src, (int64_t)rowb, &ch, cs(c)));
    if (changed) *changed = ch;
    return MHIP_OK;
}

/* The host transport's two halves of a halo exchange with ONE synchronisation each (mhip_ctx_get_edge_row / _set_halo_row: one per
 * row -- four host round trips per exchange, and the flood's and the no-flats fill's loops exchange 7 to 24 times per step).
 * get: the first / last owned row into host buffers (NULL: not wanted).  set: the neighbours' rows (NULL where there is none) are
 * compared with / stored into the halo rows; changed[0 / 1] = the top / bottom halo row changed. */
int mhip_ctx_get_edge_rows(mhip_ctx *c, int which, void *host_first, void *host_last)
{
    MH_ARG(c && which >= 0 && which < MHIP_R_COUNT_, "ctx_get_edge_rows(ctx, which, first, last)");
    MH_ARG(c->r[which].p, "raster has not been computed or uploaded");
    if (!host_first && !host_last) return MHIP_OK;
    MH_HIP(hipSetDevice(c->device));
    hipStream_t s = cs(c);
    const size_t rowb = raster_elem(which) * (size_t)c->W;
    const char *base = c->r[which].as<char>();
    if (host_first) MH_HIP(hipMemcpyAsync(host_first, base + rowb * c->ht, rowb, hipMemcpyDeviceToHost, s));
    if (host_last) MH_HIP(hipMemcpyAsync(host_last, base + rowb * (c->ht + c->H_owned - 1), rowb, hipMemcpyDeviceToHost, s));
    MH_HIP(stream_sync(s));
    return MHIP_OK;
}

int mhip_ctx_set_halo_rows(mhip_ctx *c, int which, const void *host_top, const void *host_bottom, int32_t *changed)
{
    MH_ARG(c && changed && which >= 0 && which < MHIP_R_COUNT_, "ctx_set_halo_rows(ctx, which, top, bottom, changed[2])");
    MH_ARG((!host_top || c->ht) && (!host_bottom || c->hb), "this band has no halo row on that side");
    changed[0] = changed[1] = 0;
    if (!host_top && !host_bottom) return MHIP_OK;
    MH_HIP(hipSetDevice(c->device));
    MH_TRY(ctx_raster(c, which));
    hipStream_t s = cs(c);
    const size_t rowb = raster_elem(which) * (size_t)c->W;
    DevBuf &stage = on_side(c) ? c->comm_stage_b : c->comm_stage;
    DevBuf flags;
    MH_TRY(stage.alloc(2 * rowb));
    MH_TRY(flags.alloc(8));
    MH_HIP(hipMemsetAsync(flags.p, 0, 8, s));
    char *base = c->r[which].as<char>();
    if (host_top) {
        MH_HIP(hipMemcpyAsync(stage.p, host_top, rowb, hipMemcpyHostToDevice, s));
        MH_TRY(row_update_async(base, stage.p, (int64_t)rowb, flags.as<int>(), s));
    }
    if (host_bottom) {
        MH_HIP(hipMemcpyAsync(stage.as<char>() + rowb, host_bottom, rowb, hipMemcpyHostToDevice, s));
        MH_TRY(row_update_async(base + rowb * (c->H - 1), stage.as<char>() + rowb, (int64_t)rowb, flags.as<int>() + 1, s));
    }
    int h[2] = {0, 0};
    MH_HIP(hipMemcpyAsync(h, flags.p, 8, hipMemcpyDeviceToHost, s));
    MH_HIP(stream_sync(s));
    changed[0] = h[0];
    changed[1] = h[1];
    return MHIP_OK;
}

/* RCCL transport (band contexts created with an ncclUniqueId): neighbours trade the edge rows of raster `which` GPU -> GPU
 * on the context's stream; the received rows are compared with / stored into the halo rows; changed[0 / 1] = top / bottom
 * halo row changed.  One host synchronisation (the two flags). */
int mhip_ctx_exchange_halo(mhip_ctx *c, int which, int32_t *changed)
{
    MH_ARG(c && changed && which >= 0 && which < MHIP_R_COUNT_, "ctx_exchange_halo(ctx, which, changed[2])");
    MH_ARG(c->comm || c->nranks == 1, "this band context has no RCCL communicator (created without an ncclUniqueId)");
    changed[0] = changed[1] = 0;
    if (!c->ht && !c->hb) return MHIP_OK;
    MH_ARG(c->r[which].p, "raster has not been computed or uploaded");
    MH_HIP(hipSetDevice(c->device));
    hipStream_t s = cs(c);
    const size_t rowb = raster_elem(which) * (size_t)c->W;
    MH_TRY(c->comm_stage.alloc(2 * rowb));
    MH_TRY(c->comm_flags.alloc(8));
    MH_HIP(hipMemsetAsync(c->comm_flags.p, 0, 8, s));
    char *base = c->r[which].as<char>();
    MH_TRY(comm_exchange_rows(c->comm, c->rank, c->nranks, base + rowb * c->ht, base + rowb * (c->ht + c->H_owned - 1), c->comm_stage.p, rowb, s));
    if (c->ht) MH_TRY(row_update_async(base, c->comm_stage.p, (int64_t)rowb, c->comm_flags.as<int>(), s));
    if (c->hb) MH_TRY(row_update_async(base + rowb * (c->H - 1), c->comm_stage.as<char>() + rowb, (int64_t)rowb, c->comm_flags.as<int>() + 1, s));
    int h[2] = {0, 0};
    MH_HIP(hipMemcpyAsync(h, c->comm_flags.p, 8, hipMemcpyDeviceToHost, s));
    MH_HIP(stream_sync(s));
    changed[0] = h[0];
    changed[1] = h[1];
    return MHIP_OK;
}

/* The same exchange WITHOUT touching the halo rows: the neighbours' edge rows of raster `which` arrive in host buffers (W elements
 * each; NULL where there is no neighbour).  The boundary systems of labelling, accumulation and watersheds compare a neighbour's
 * edge row with this band's own halo row: neighbour-to-neighbour traffic over RCCL instead of an all-gather of every band's rows. */
int mhip_ctx_exchange_edge_rows(mhip_ctx *c, int which, void *host_from_up, void *host_from_down)
{
    MH_ARG(c && which >= 0 && which < MHIP_R_COUNT_, "ctx_exchange_edge_rows(ctx, which, from_up, from_down)");
    void *comm = on_side(c) ? c->comm_b : c->comm;
    MH_ARG(comm || c->nranks == 1, on_side(c) ? "this band context has no side communicator (mhip_ctx_comm_add_side)"
                                              : "this band context has no RCCL communicator (created without an ncclUniqueId)");
    if (!c->ht && !c->hb) return MHIP_OK;
    MH_ARG(c->r[which].p, "raster has not been computed or uploaded");
    MH_ARG((!c->ht || host_from_up) && (!c->hb || host_from_down), "ctx_exchange_edge_rows: a buffer per neighbour");
    MH_HIP(hipSetDevice(c->device));
    hipStream_t s = cs(c);
    const size_t rowb = raster_elem(which) * (size_t)c->W;
    DevBuf &stage = on_side(c) ? c->comm_stage_b : c->comm_stage;
    MH_TRY(stage.alloc(2 * rowb));
    char *base = c->r[which].as<char>();
    MH_TRY(comm_exchange_rows(comm, c->rank, c->nranks, base + rowb * c->ht, base + rowb * (c->ht + c->H_owned - 1), stage.p, rowb, s));
    if (c->ht) MH_HIP(hipMemcpyAsync(host_from_up, stage.p, rowb, hipMemcpyDeviceToHost, s));
    if (c->hb) MH_HIP(hipMemcpyAsync(host_from_down, stage.as<char>() + rowb, rowb, hipMemcpyDeviceToHost, s));
    MH_HIP(stream_sync(s));
    return MHIP_OK;
}

/* max of `value` over all bands (ends the fill / accumulation loops: "is anybody still active") */
int mhip_ctx_allreduce_max(mhip_ctx *c, double value, double *out)
{
    MH_ARG(c && out, "ctx_allreduce_max(ctx, value, out)");
    if (c->nranks == 1 && !c->comm) {
        *out = value;
        return MHIP_OK;
    }
    MH_ARG(c->comm, "this band context has no RCCL communicator (created without an ncclUniqueId)");
    MH_HIP(hipSetDevice(c->device));
    hipStream_t s = cs(c);
    MH_TRY(c->comm_word.alloc(8));
    MH_HIP(hipMemcpyAsync(c->comm_word.p, &value, 8, hipMemcpyHostToDevice, s));
    MH_TRY(comm_allreduce_max(c->comm, c->comm_word.as<double>(), s));
    MH_HIP(hipMemcpyAsync(out, c->comm_word.p, 8, hipMemcpyDeviceToHost, s));
    MH_HIP(stream_sync(s));
    return MHIP_OK;
}

int mhip_ctx_has_comm(mhip_ctx *c) { return (c && c->comm) ? ((c->comm_b) ? 2 : 1) : 0; }

int mhip_ctx_zero_raster(mhip_ctx *c, int which)
{
    MH_ARG(c && which >= 0 && which < MHIP_R_COUNT_, "ctx_zero_raster(ctx, which)");
    MH_HIP(hipSetDevice(c->device));
    MH_TRY(ctx_raster(c, which));
    MH_HIP(hipMemsetAsync(c->r[which].p, 0, raster_elem(which) * (size_t)(c->H * c->W), cs(c)));
    return MHIP_OK;
}

/* accumulation on a band, boundary pass: the band's OWN contribution (halo rows = sources of no flux) into ACCUM, and for
 * every halo cell the cell of the first / last owned row through which its flux leaves the band again (see accum.hip) */
int mhip_ctx_band_accum_boundary(mhip_ctx *c, int32_t *exit_map)
{
    MH_ARG(c && exit_map && c->have[MHIP_R_FLOWDIR], "ctx_band_accum_boundary(ctx, exit_map[2 * W]) needs flow directions");
    MH_HIP(hipSetDevice(c->device));
    MH_TRY(ctx_raster(c, MHIP_R_ACCUM));
    DevBuf d_map;
    MH_TRY(d_map.alloc(8 * (size_t)c->W));
    MH_TRY(accum_dev(c->r[MHIP_R_FLOWDIR].as<uint8_t>(), c->r[MHIP_R_ACCUM].as<double>(), c->H, c->W, cs(c), c->ht, c->hb, 1,
                     d_map.as<int32_t>(), nullptr, &c->acc_keep));
    MH_HIP(hipMemcpyAsync(exit_map, d_map.p, 8 * (size_t)c->W, hipMemcpyDeviceToHost, cs(c)));
    MH_HIP(stream_sync(cs(c)));
    return MHIP_OK;
}

/* connected components of the band's LOCAL raster (owned + halo rows) in a band-local label space 1..nlocal */
int mhip_ctx_band_ccl_local(mhip_ctx *c, int64_t *nlocal)
{
    MH_ARG(c && nlocal && c->have[MHIP_R_DEPTHS], "ctx_band_ccl_local needs bluespot depths");
    MH_HIP(hipSetDevice(c->device));
    MH_TRY(ctx_raster(c, MHIP_R_LABELS));
    if (!c->tmp_i32.p) MH_TRY(c->tmp_i32.alloc(4 * (size_t)(c->H * c->W)));
    MH_TRY(ccl8_f32_dev(c->r[MHIP_R_DEPTHS].as<float>(), c->r[MHIP_R_LABELS].as<int32_t>(), c->tmp_i32.as<int32_t>(), c->H, c->W,
                        nlocal, cs(c)));
    c->nlabels_raw = *nlocal;
    c->have[MHIP_R_LABELS] = true;
    c->labels_components = true;     // (the relabelling calls of the band protocol join components across bands and drop components)
    c->labels_filtered = false;
    return MHIP_OK;
}

/* band-local labels -> global labels through a host-built LUT (nlocal + 1 entries, lut[0] == 0) */
int mhip_ctx_band_relabel(mhip_ctx *c, const int32_t *lut, int64_t nlocal, int64_t nlabels_global)
{
    MH_ARG(c && lut && nlocal >= 0 && c->have[MHIP_R_LABELS], "ctx_band_relabel(ctx, lut, nlocal, nglobal)");
    MH_HIP(hipSetDevice(c->device));
    DevBuf d_lut;
    MH_TRY(d_lut.alloc(4 * (size_t)(nlocal + 1)));
    MH_HIP(hipMemcpyAsync(d_lut.p, lut, 4 * (size_t)(nlocal + 1), hipMemcpyHostToDevice, cs(c)));
    MH_TRY(relabel_lut_dev(c->r[MHIP_R_LABELS].as<int32_t>(), d_lut.as<int32_t>(), nlocal, c->H * c->W, cs(c)));
    c->nlabels = c->nlabels_raw = nlabels_global;
    c->labels_filtered = true;
    return MHIP_OK;
}

/* the same without a dense LUT: local label l -> offset + l - #(dropped labels < l); dropped[k] (sorted, the local labels that
 * are numbered by another band or own no cell here) -> target[k] */
int mhip_ctx_band_relabel_sparse(mhip_ctx *c, int64_t nlocal, int64_t offset, const int32_t *dropped, const int32_t *target,
                                 int64_t ndropped, int64_t nlabels_global)
{
    MH_ARG(c && nlocal >= 0 && ndropped >= 0 && (ndropped == 0 || (dropped && target)) && c->have[MHIP_R_LABELS] &&
               offset + nlocal < (int64_t)INT32_MAX, "ctx_band_relabel_sparse");
    for (int64_t k = 1; k < ndropped; ++k) MH_ARG(dropped[k - 1] < dropped[k], "ctx_band_relabel_sparse: dropped labels must be sorted and unique");
    MH_HIP(hipSetDevice(c->device));
    DevBuf d_d, d_t;
    MH_TRY(d_d.alloc(4 * (size_t)(ndropped + 1)));
    MH_TRY(d_t.alloc(4 * (size_t)(ndropped + 1)));
    if (ndropped) {
        MH_HIP(hipMemcpyAsync(d_d.p, dropped, 4 * (size_t)ndropped, hipMemcpyHostToDevice, cs(c)));
        MH_HIP(hipMemcpyAsync(d_t.p, target, 4 * (size_t)ndropped, hipMemcpyHostToDevice, cs(c)));
    }
    MH_TRY(relabel_sparse_dev(c->r[MHIP_R_LABELS].as<int32_t>(), c->H * c->W, nlocal, (int32_t)offset, d_d.as<int32_t>(), d_t.as<int32_t>(),
                              (int32_t)ndropped, cs(c)));
    c->nlabels = c->nlabels_raw = nlabels_global;
    c->labels_filtered = true;
    return MHIP_OK;
}

/* The two calls above as two HALVES of one labelling, without the two passes over the label raster that lie between them (the
 * emit pass that writes band-local labels everywhere, and the relabelling pass that reads them back): `begin` stops before the emit
 * pass -- *nlocal band-local labels, and of the labels raster only the two top and the two bottom rows (band-local labels: what
 * mhip_ctx_get_edge_row / mhip_ctx_exchange_edge_rows hand to the seam merge) are written; `finish` writes the GLOBAL label of every
 * cell in one pass (local l -> offset + l - #(dropped labels < l), dropped[k] -> target[k], as mhip_ctx_band_relabel_sparse).
 * with_stats != 0: label_stats of the depths over the OWNED rows by global label ride on that pass -- what mhip_ctx_band_records(ctx, 0)
 * computes; mhip_ctx_band_fetch / _gather(which = 0) read them.  Between the two calls the labels raster is not a raster of labels. */
int mhip_ctx_band_ccl_begin(mhip_ctx *c, int64_t *nlocal)
{
    MH_ARG(c && nlocal && c->have[MHIP_R_DEPTHS], "ctx_band_ccl_begin needs bluespot depths");
    MH_HIP(hipSetDevice(c->device));
    MH_TRY(ctx_raster(c, MHIP_R_LABELS));
    c->have[MHIP_R_LABELS] = false;
    if (!c->tmp_i32.p) MH_TRY(c->tmp_i32.alloc(4 * (size_t)(c->H * c->W)));
    MH_TRY(ccl8_f32_begin_dev(c->r[MHIP_R_DEPTHS].as<float>(), c->r[MHIP_R_LABELS].as<int32_t>(), c->tmp_i32.as<int32_t>(), c->H, c->W,
                              nlocal, cs(c), &c->ccl_keep));
    c->ccl_keep.nlocal = *nlocal;
    c->ccl_pending = true;
    return MHIP_OK;
}

int mhip_ctx_band_ccl_finish(mhip_ctx *c, int64_t offset, const int32_t *dropped, const int32_t *target, int64_t ndropped, int64_t nlabels_global,
                             int with_stats)
{
    MH_ARG(c && c->ccl_pending && ndropped >= 0 && (ndropped == 0 || (dropped && target)) && nlabels_global >= 0 &&
               offset >= 0 && offset + c->ccl_keep.nlocal < (int64_t)INT32_MAX && nlabels_global < (int64_t)INT32_MAX,
           "ctx_band_ccl_finish(ctx, offset, dropped, target, ndropped, nlabels_global, with_stats) follows ctx_band_ccl_begin");
    for (int64_t k = 1; k < ndropped; ++k) MH_ARG(dropped[k - 1] < dropped[k], "ctx_band_ccl_finish: dropped labels must be sorted and unique");
    MH_ARG(!with_stats || c->have[MHIP_R_DEPTHS], "ctx_band_ccl_finish: the statistics need the depths");
    MH_HIP(hipSetDevice(c->device));
    const int64_t nlocal = c->ccl_keep.nlocal;
    DevBuf d_d, d_t;
    MH_TRY(d_d.alloc(4 * (size_t)(ndropped + 1)));
    MH_TRY(d_t.alloc(4 * (size_t)(ndropped + 1)));
    if (ndropped) {
        MH_HIP(hipMemcpyAsync(d_d.p, dropped, 4 * (size_t)ndropped, hipMemcpyHostToDevice, cs(c)));
        MH_HIP(hipMemcpyAsync(d_t.p, target, 4 * (size_t)ndropped, hipMemcpyHostToDevice, cs(c)));
    }
    c->ccl_pending = false;
    if (with_stats) MH_TRY(c->stats.alloc(sizeof(mhip_stat_record) * (size_t)(nlabels_global + 1)));
    if (c->ccl_keep.valid) {
        MH_TRY(label_emit_sparse_dev(c->tmp_i32.as<int32_t>(), c->ccl_keep.bits.as<unsigned long long>(), c->ccl_keep.wprefix.as<uint32_t>(),
                                     c->r[MHIP_R_DEPTHS].as<float>(), c->r[MHIP_R_LABELS].as<int32_t>(), c->H, c->W, c->ht, c->H_owned, nlocal,
                                     (int32_t)offset, d_d.as<int32_t>(), d_t.as<int32_t>(), (int32_t)ndropped, nlabels_global,
                                     with_stats ? c->stats.as<mhip_stat_record>() : nullptr, cs(c)));
        c->ccl_keep.bits.release();
        c->ccl_keep.wprefix.release();
        c->ccl_keep.valid = false;
    } else {
        // (a labelling schedule that keeps no tables -- MHIP_CCL=global -- has written band-local labels everywhere)
        MH_TRY(relabel_sparse_dev(c->r[MHIP_R_LABELS].as<int32_t>(), c->H * c->W, nlocal, (int32_t)offset, d_d.as<int32_t>(), d_t.as<int32_t>(),
                                  (int32_t)ndropped, cs(c)));
        if (with_stats) {
            const int64_t off = c->W * c->ht;
            MH_TRY(label_stats_dev(c->r[MHIP_R_DEPTHS].as<float>() + off, c->r[MHIP_R_LABELS].as<int32_t>() + off, c->H_owned * c->W, nlabels_global,
                                   c->stats.as<mhip_stat_record>(), cs(c), c->W, true));
        }
        MH_HIP(stream_sync(cs(c)));
    }
    c->nlabels = c->nlabels_raw = nlabels_global;
    c->have[MHIP_R_LABELS] = true;
    c->labels_components = true;
    c->labels_filtered = true;
    return MHIP_OK;
}

/* the bluespot filter on a band (reference bluespots.py:165-172 == a rank relabel): labels in [lo, hi] (numbered by this band) ->
 * lut[l - lo] (0 = dropped); a label numbered by another band -> fnew[k] where fid[k] == l (fid sorted); nlabels_new = the global count */
int mhip_ctx_band_relabel_range(mhip_ctx *c, int64_t lo, int64_t hi, const int32_t *lut, const int32_t *fid, const int32_t *fnew, int64_t nf,
                                int64_t nlabels_new)
{
    MH_ARG(c && c->have[MHIP_R_LABELS] && lo >= 1 && hi >= lo - 1 && hi < (int64_t)INT32_MAX && nf >= 0 && (hi < lo || lut) && (nf == 0 || (fid && fnew)) &&
               nlabels_new >= 0, "ctx_band_relabel_range(ctx, lo, hi, lut, fid, fnew, nf, nlabels_new)");
    for (int64_t k = 1; k < nf; ++k) MH_ARG(fid[k - 1] < fid[k], "ctx_band_relabel_range: foreign labels must be sorted and unique");
    MH_HIP(hipSetDevice(c->device));
    DevBuf d_lut, d_fid, d_fnew;
    const size_t nl = (size_t)(hi - lo + 1);
    MH_TRY(d_lut.alloc(4 * (nl + 1)));
    MH_TRY(d_fid.alloc(4 * (size_t)(nf + 1)));
    MH_TRY(d_fnew.alloc(4 * (size_t)(nf + 1)));
    if (nl) MH_HIP(hipMemcpyAsync(d_lut.p, lut, 4 * nl, hipMemcpyHostToDevice, cs(c)));
    if (nf) {
        MH_HIP(hipMemcpyAsync(d_fid.p, fid, 4 * (size_t)nf, hipMemcpyHostToDevice, cs(c)));
        MH_HIP(hipMemcpyAsync(d_fnew.p, fnew, 4 * (size_t)nf, hipMemcpyHostToDevice, cs(c)));
    }
    MH_TRY(relabel_range_dev(c->r[MHIP_R_LABELS].as<int32_t>(), c->H * c->W, (int32_t)lo, (int32_t)hi, d_lut.as<int32_t>(), d_fid.as<int32_t>(),
                             d_fnew.as<int32_t>(), (int32_t)nf, cs(c)));
    MH_HIP(stream_sync(cs(c)));
    c->nlabels = c->nlabels_raw = nlabels_new;
    c->labels_filtered = true;
    return MHIP_OK;
}

/* one leg of the stream walk on a band (trace.hip: band_trace_kernel).  cells_rc: GLOBAL (row, col) of n walkers that stand on
 * owned rows of this band; src_label[i] >= 0: the walker's source label (it came from another band), -1: its start cell's label.
 * out_status: 0 ended without a label, 1 found out_label, 2 stepped onto a neighbour's row at out_exit_rc (GLOBAL).  Geometry
 * (global linear indices) in two passes like mhip_ctx_trace_downstream: lengths first, then offsets + out_cells. */
int mhip_ctx_band_trace(mhip_ctx *c, const int64_t *cells_rc, const int32_t *src_label, int64_t n, int use_background, int32_t background,
                        int32_t *out_label, int32_t *out_status, int32_t *out_src, int64_t *out_exit_rc, int64_t *out_len, const int64_t *offsets,
                        int64_t *out_cells)
{
    MH_ARG(c && n >= 0 && (n == 0 || cells_rc), "ctx_band_trace(ctx, cells, src, n, ...)");
    MH_ARG(c->have[MHIP_R_FLOWDIR] && c->have[MHIP_R_LABELS], "ctx_band_trace needs flow directions and labels");
    if (n == 0) return MHIP_OK;
    MH_HIP(hipSetDevice(c->device));
    hipStream_t s = cs(c);
    DevBuf d_c, d_s, d_l, d_f, d_so, d_e, d_n, d_o, d_p;
    MH_TRY(upload(d_c, cells_rc, (size_t)n * 16, s));
    if (src_label) MH_TRY(upload(d_s, src_label, (size_t)n * 4, s));
    MH_TRY(d_l.alloc((size_t)n * 4));
    MH_TRY(d_f.alloc((size_t)n * 4));
    MH_TRY(d_so.alloc((size_t)n * 4));
    MH_TRY(d_e.alloc((size_t)n * 16));
    MH_TRY(d_n.alloc((size_t)n * 8));
    int64_t total = 0;
    if (offsets && out_cells) {
        total = offsets[n];
        MH_ARG(total >= 0, "band_trace: offsets[n] must be the total path length");
        MH_TRY(upload(d_o, offsets, (size_t)(n + 1) * 8, s));
        MH_TRY(d_p.alloc((size_t)(total > 0 ? total : 1) * 8));
    }
    MH_TRY(band_trace_dev(c->r[MHIP_R_FLOWDIR].as<uint8_t>(), c->r[MHIP_R_LABELS].as<int32_t>(), c->H, c->W, c->row0 - c->ht, c->ht, c->ht + c->H_owned,
                          c->H_global, d_c.as<int64_t>(), src_label ? d_s.as<int32_t>() : nullptr, n, use_background, background, d_l.as<int32_t>(),
                          d_f.as<int32_t>(), d_so.as<int32_t>(), d_e.as<int64_t>(), d_n.as<int64_t>(), total ? d_o.as<int64_t>() : nullptr,
                          total ? d_p.as<int64_t>() : nullptr, s));
    if (out_label) MH_HIP(hipMemcpyAsync(out_label, d_l.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    if (out_status) MH_HIP(hipMemcpyAsync(out_status, d_f.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    if (out_src) MH_HIP(hipMemcpyAsync(out_src, d_so.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    if (out_exit_rc) MH_HIP(hipMemcpyAsync(out_exit_rc, d_e.p, (size_t)n * 16, hipMemcpyDeviceToHost, s));
    if (out_len) MH_HIP(hipMemcpyAsync(out_len, d_n.p, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    if (total) MH_HIP(hipMemcpyAsync(out_cells, d_p.p, (size_t)total * 8, hipMemcpyDeviceToHost, s));
    MH_HIP(stream_sync(s));
    return MHIP_OK;
}

/* watersheds inside the band: halo rows are terminals carrying pseudo labels -(1+col) (top) / -(1+W+col) (bottom) */
int mhip_ctx_band_watershed_local(mhip_ctx *c)
{
    MH_ARG(c && c->have[MHIP_R_LABELS] && c->have[MHIP_R_FLOWDIR], "ctx_band_watershed_local needs labels and flow directions");
    MH_HIP(hipSetDevice(c->device));
    MH_TRY(ctx_raster(c, MHIP_R_WATERSHEDS));
    // Out of place, like one context: the watersheds read the labels where they are and write every cell of their own raster (a copy of
    // the label raster first -- 8 B per cell -- and the in-place passes behind it were what the band did until round 4).  The pseudo
    // labels of the halo rows have to be IN the raster the passes read: the labels' two halo rows are put aside, overwritten and
    // restored (nobody else reads them meanwhile: the pour points on the main thread look at owned rows only).
    hipStream_t s = cs(c);
    const size_t rowb = 4 * (size_t)c->W;
    int32_t *lab = c->r[MHIP_R_LABELS].as<int32_t>();
    DevBuf keep;
    MH_TRY(keep.alloc(2 * rowb));
    if (c->ht) MH_HIP(hipMemcpyAsync(keep.p, lab, rowb, hipMemcpyDeviceToDevice, s));
    if (c->hb) MH_HIP(hipMemcpyAsync(keep.as<char>() + rowb, lab + (c->H - 1) * c->W, rowb, hipMemcpyDeviceToDevice, s));
    int rc = band_pseudo_labels_dev(lab, c->H, c->W, c->ht, c->hb, s);
    if (rc == MHIP_OK)
        rc = watersheds_dev(c->r[MHIP_R_FLOWDIR].as<uint8_t>(), c->r[MHIP_R_WATERSHEDS].as<int32_t>(), c->H, c->W, 0, s, true, nullptr, lab, nullptr);
    // (whatever happened: the labels get their halo rows back)
    hipError_t e1 = hipSuccess, e2 = hipSuccess;
    if (c->ht) e1 = hipMemcpyAsync(lab, keep.p, rowb, hipMemcpyDeviceToDevice, s);
    if (c->hb) e2 = hipMemcpyAsync(lab + (c->H - 1) * c->W, keep.as<char>() + rowb, rowb, hipMemcpyDeviceToDevice, s);
    const hipError_t e3 = stream_sync(s);
    MH_TRY(rc);
    MH_HIP(e1);
    MH_HIP(e2);
    MH_HIP(e3);
    c->have[MHIP_R_WATERSHEDS] = true;
    return MHIP_OK;
}

/* raster[i] = lut[-raster[i]-1] wherever raster[i] < 0 (resolves the pseudo labels once the boundary system is solved) */
int mhip_ctx_band_apply_neg_lut(mhip_ctx *c, int which, const int32_t *lut, int64_t n)
{
    MH_ARG(c && lut && n >= 1 && (which == MHIP_R_WATERSHEDS || which == MHIP_R_LABELS) && c->r[which].p, "ctx_band_apply_neg_lut");
    MH_HIP(hipSetDevice(c->device));
    DevBuf d_lut;
    MH_TRY(d_lut.alloc(4 * (size_t)n));
    MH_HIP(hipMemcpyAsync(d_lut.p, lut, 4 * (size_t)n, hipMemcpyHostToDevice, cs(c)));
    MH_TRY(negative_lut_dev(c->r[which].as<int32_t>(), c->H * c->W, d_lut.as<int32_t>(), n, cs(c)));
    MH_HIP(stream_sync(cs(c)));
    return MHIP_OK;
}

/* per-label records over the OWNED rows of a band, indexed by GLOBAL label (after mhip_ctx_band_relabel).  They stay on
 * the device (nlabels_global + 1 entries: too many to ship per band); the launcher fetches the slice of the labels this
 * band numbered, the few labels that cross a band boundary, and the sparse foreign watershed counts, and merges those
 * (distributed.BandPipeline).  which: 0 = label_stats of the depths, 1 = bincount of the watersheds, 2 = first arg-max of
 * the accumulated flow (rows are GLOBAL raster rows, -1 when the label has no cell in this band) */
namespace {
__global__ void global_rows_kernel(mhip_index_record *rec, int64_t n, int64_t row0)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && rec[i].row >= 0) rec[i].row += row0;
}
__global__ void gather_bytes_kernel(const char *src, const int64_t *ids, int64_t nids, int elem, char *dst)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nids * elem) return;
    dst[i] = src[ids[i / elem] * elem + i % elem];
}
// (id, count) pairs with count > 0 and id outside [lo, hi], id != 0
__global__ void foreign_counts_kernel(const int64_t *cnt, int64_t n, int64_t lo, int64_t hi, int64_t cap, int64_t *ids, int64_t *vals,
                                      unsigned long long *nout)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= 0 || i >= n || (i >= lo && i <= hi)) return;
    const int64_t v = cnt[i];
    if (v <= 0) return;
    const unsigned long long k = atomicAdd(nout, 1ull);
    if ((int64_t)k < cap) {
        ids[k] = i;
        vals[k] = v;
    }
}
}  // namespace

static size_t band_record_size(int which) { return which == 0 ? sizeof(mhip_stat_record) : which == 1 ? 8 : sizeof(mhip_index_record); }
static DevBuf &band_record_buf(mhip_ctx *c, int which) { return which == 0 ? c->stats : which == 1 ? c->ws_counts : c->pour; }   // (2 and 3 share a buffer)

int mhip_ctx_band_records(mhip_ctx *c, int which)
{
    MH_ARG(c && which >= 0 && which <= 3 && c->have[MHIP_R_LABELS] && c->nlabels >= 0, "ctx_band_records(ctx, which) needs global labels");
    MH_HIP(hipSetDevice(c->device));
    const int64_t off = c->W * c->ht, n = c->H_owned * c->W, nrec = c->nlabels + 1;
    DevBuf &buf = band_record_buf(c, which);
    MH_TRY(buf.alloc(band_record_size(which) * (size_t)nrec));
    if (which == 0) {
        MH_ARG(c->have[MHIP_R_DEPTHS], "label_stats needs the depths");
        MH_TRY(label_stats_dev(c->r[MHIP_R_DEPTHS].as<float>() + off, c->r[MHIP_R_LABELS].as<int32_t>() + off, n, c->nlabels,
                               buf.as<mhip_stat_record>(), cs(c), c->W, c->labels_components));
    } else if (which == 1) {
        MH_ARG(c->have[MHIP_R_WATERSHEDS], "watershed counts need the watersheds");
        MH_TRY(label_count_dev(c->r[MHIP_R_WATERSHEDS].as<int32_t>() + off, n, c->nlabels, buf.as<int64_t>(), cs(c), c->W));
    } else {
        // bluespots.py:195-206: the first arg-max of the accumulated flow (2), or the first arg-min of the no-flats surface (3)
        const int src = which == 2 ? MHIP_R_ACCUM : MHIP_R_NOFLAT;
        MH_ARG(c->have[src], which == 2 ? "pour points need the accumulated flow" : "pour points need the no-flats surface");
        MH_TRY(label_arg_dev(c->r[src].as<double>() + off, c->r[MHIP_R_LABELS].as<int32_t>() + off, c->H_owned, c->W, c->nlabels,
                             which == 2, buf.as<mhip_index_record>(), cs(c), c->labels_components));
        hipLaunchKernelGGL(global_rows_kernel, dim3((unsigned)cdiv(nrec, 256)), dim3(256), 0, cs(c), buf.as<mhip_index_record>(), nrec,
                           c->row0);
        MH_HIP(hipGetLastError());
    }
    return MHIP_OK;
}

/* records [first, first + count) of the last mhip_ctx_band_records(which) */
int mhip_ctx_band_fetch(mhip_ctx *c, int which, int64_t first, int64_t count, void *out)
{
    MH_ARG(c && which >= 0 && which <= 3 && band_record_buf(c, which).p && first >= 0 && count >= 0 && first + count <= c->nlabels + 1 &&
               (out || count == 0), "ctx_band_fetch(ctx, which, first, count, out)");
    if (count == 0) return MHIP_OK;
    MH_HIP(hipSetDevice(c->device));
    const size_t e = band_record_size(which);
    MH_HIP(hipMemcpyAsync(out, band_record_buf(c, which).as<char>() + e * (size_t)first, e * (size_t)count, hipMemcpyDeviceToHost, cs(c)));
    MH_HIP(stream_sync(cs(c)));
    return MHIP_OK;
}

/* records at the given labels (any order) */
int mhip_ctx_band_gather(mhip_ctx *c, int which, const int64_t *ids, int64_t nids, void *out)
{
    MH_ARG(c && which >= 0 && which <= 3 && band_record_buf(c, which).p && nids >= 0 && ((ids && out) || nids == 0), "ctx_band_gather");
    if (nids == 0) return MHIP_OK;
    for (int64_t k = 0; k < nids; ++k) MH_ARG(ids[k] >= 0 && ids[k] <= c->nlabels, "ctx_band_gather: label outside [0, nlabels]");
    MH_HIP(hipSetDevice(c->device));
    const int e = (int)band_record_size(which);
    DevBuf d_ids, d_out;
    MH_TRY(d_ids.alloc(8 * (size_t)nids));
    MH_TRY(d_out.alloc((size_t)e * (size_t)nids));
    MH_HIP(hipMemcpyAsync(d_ids.p, ids, 8 * (size_t)nids, hipMemcpyHostToDevice, cs(c)));
    hipLaunchKernelGGL(gather_bytes_kernel, dim3((unsigned)cdiv(nids * e, 256)), dim3(256), 0, cs(c), band_record_buf(c, which).as<char>(),
                       d_ids.as<int64_t>(), nids, e, d_out.as<char>());
    MH_HIP(hipGetLastError());
    MH_HIP(hipMemcpyAsync(out, d_out.p, (size_t)e * (size_t)nids, hipMemcpyDeviceToHost, cs(c)));
    MH_HIP(stream_sync(cs(c)));
    return MHIP_OK;
}

/* watershed counts of labels OUTSIDE [lo, hi] (and != 0) that are non-zero in this band: up to `cap` (id, count) pairs,
 * *nfound = how many there are (call again with a larger cap if it exceeds cap) */
int mhip_ctx_band_foreign_counts(mhip_ctx *c, int64_t lo, int64_t hi, int64_t cap, int64_t *ids, int64_t *counts, int64_t *nfound)
{
    MH_ARG(c && c->ws_counts.p && cap >= 0 && nfound && ((ids && counts) || cap == 0), "ctx_band_foreign_counts");
    MH_HIP(hipSetDevice(c->device));
    DevBuf d_ids, d_vals, d_n;
    MH_TRY(d_ids.alloc(8 * (size_t)(cap + 1)));
    MH_TRY(d_vals.alloc(8 * (size_t)(cap + 1)));
    MH_TRY(d_n.alloc(8));
    MH_HIP(hipMemsetAsync(d_n.p, 0, 8, cs(c)));
    const int64_t nrec = c->nlabels + 1;
    hipLaunchKernelGGL(foreign_counts_kernel, dim3((unsigned)cdiv(nrec, 256)), dim3(256), 0, cs(c), c->ws_counts.as<int64_t>(), nrec, lo, hi,
                       cap, d_ids.as<int64_t>(), d_vals.as<int64_t>(), d_n.as<unsigned long long>());
    MH_HIP(hipGetLastError());
    unsigned long long k = 0;
    MH_HIP(hipMemcpyAsync(&k, d_n.p, 8, hipMemcpyDeviceToHost, cs(c)));
    MH_HIP(stream_sync(cs(c)));
    *nfound = (int64_t)k;
    const int64_t take = (int64_t)k < cap ? (int64_t)k : cap;
    if (take > 0) {
        MH_HIP(hipMemcpyAsync(ids, d_ids.p, 8 * (size_t)take, hipMemcpyDeviceToHost, cs(c)));
        MH_HIP(hipMemcpyAsync(counts, d_vals.p, 8 * (size_t)take, hipMemcpyDeviceToHost, cs(c)));
        MH_HIP(stream_sync(cs(c)));
    }
    return MHIP_OK;
}

int mhip_ctx_dem_minmax(mhip_ctx *c, float *mn, float *mx, int32_t *has_nan)
{
    MH_ARG(c && mn && mx && has_nan && c->have[MHIP_R_DEM], "ctx_dem_minmax needs the DEM");
    MH_HIP(hipSetDevice(c->device));
    if (c->have[MHIP_R_FILLED] && c->fill_st.have_minmax) {
        // the flood that has just run over this DEM folded the extremes of its tiles (pf_minmax_kernel) -- over the band's LOCAL rows,
        // halo rows included: cells of the same global raster, and the global extremes are what the callers fold these into
        *mn = c->fill_st.dem_min;
        *mx = c->fill_st.dem_max;
        *has_nan = c->fill_st.dem_nan ? 1 : 0;
        return MHIP_OK;
    }
    int hn = 0;
    MH_TRY(minmax_dev(c->r[MHIP_R_DEM].as<float>() + c->W * c->ht, c->H_owned * c->W, mn, mx, &hn, cs(c)));
    *has_nan = hn;
    return MHIP_OK;
}

/* resumable fill: kind 0 = fill_terrain (needs DEM incl. halo rows), kind 1 = fill_terrain_no_flats (needs DEM and the
 * converged plain fill incl. halo rows; short/diag from the GLOBAL |dem| maximum). */
int mhip_ctx_fill_begin(mhip_ctx *c, int kind, double short_, double diag, int32_t *active)
{
    MH_ARG(c && active && (kind == 0 || kind == 1) && c->have[MHIP_R_DEM], "ctx_fill_begin(ctx, kind, short, diag, active)");
    MH_HIP(hipSetDevice(c->device));
    const int which = kind ? MHIP_R_NOFLAT : MHIP_R_FILLED;
    MH_TRY(ctx_raster(c, which));
    if (kind == 0) {
        // the tiled priority-flood first: the band's whole local solve happens here, the loop that follows only trades edge rows
        const bool force_iter = [] { const char *e = dev_env("MHIP_FILL"); return e && std::string(e) == "iterative"; }();   // (development: engine selection for A/B runs and tests)
        delete c->pf;
        c->pf = nullptr;
        c->pf_done = false;
        c->pf_depths = false;
        if (!force_iter) {
            PfRun *p = new PfRun();
            p->dem = c->r[MHIP_R_DEM].as<float>();
            p->out = c->r[MHIP_R_FILLED].as<float>();
            p->H = c->H; p->W = c->W;
            p->fixed_top = c->ht; p->fixed_bot = c->hb;
            const int rc = p->begin(c->stream);
            if (rc == MHIP_OK) {
                c->pf = p;
                *active = 0;
                return MHIP_OK;
            }
            delete p;
            if (rc != MHIP_ELIMIT) return rc;
        }
    }
    delete c->run[kind];
    if (kind) {   // a geodesic run that was abandoned (another band found it not applicable)
        delete c->geo;
        c->geo = nullptr;
    }
    FillRun *f = c->run[kind] = new FillRun();
    f->noflat = kind != 0;
    f->dem = c->r[MHIP_R_DEM].as<float>();
    f->out = c->r[which].p;
    f->H = c->H; f->W = c->W;
    f->fixed_top = c->ht; f->fixed_bot = c->hb;
    f->rounds_per_batch = 16;   // a band pays a halo exchange + an all-reduce per batch: fewer, longer batches
    if (kind) {
        MH_ARG(c->have[MHIP_R_FILLED], "the no-flats fill of a band starts from the converged plain fill");
        f->sh = short_; f->dg = diag;
        c->sh = short_; c->dg = diag;
        noflat_seed(*f, c->r[MHIP_R_FILLED].as<float>(), short_, diag, c->H_global * c->W);
    }
    bool a = false;
    MH_TRY(f->begin(c->stream, &a));
    *active = a;
    return MHIP_OK;
}

/* like mhip_ctx_fill_begin, but the raster (MHIP_R_NOFLAT / MHIP_R_FILLED) already holds an upper bound of the fixed point: no
 * initialising round; mhip_ctx_fill_certify finds the tiles that can still move */
int mhip_ctx_fill_attach(mhip_ctx *c, int kind, double short_, double diag)
{
    MH_ARG(c && (kind == 0 || kind == 1) && c->have[MHIP_R_DEM], "ctx_fill_attach(ctx, kind, short, diag)");
    const int which = kind ? MHIP_R_NOFLAT : MHIP_R_FILLED;
    MH_ARG(c->r[which].p, "ctx_fill_attach: the raster to start from does not exist");
    MH_HIP(hipSetDevice(c->device));
    if (kind == 0) {
        delete c->pf;
        c->pf = nullptr;
    }
    delete c->run[kind];
    FillRun *f = c->run[kind] = new FillRun();
    f->noflat = kind != 0;
    f->dem = c->r[MHIP_R_DEM].as<float>();
    f->out = c->r[which].p;
    f->H = c->H; f->W = c->W;
    f->fixed_top = c->ht; f->fixed_bot = c->hb;
    f->rounds_per_batch = 16;
    if (kind) {
        f->sh = short_; f->dg = diag;
        c->sh = short_; c->dg = diag;
    }
    return f->attach(c->stream);
}

int mhip_ctx_noflat_verify(mhip_ctx *c, int32_t *ok)
{
    MH_ARG(c && ok && c->have[MHIP_R_NOFLAT] && c->have[MHIP_R_DEM], "ctx_noflat_verify(ctx, ok) needs the no-flats surface");
    MH_HIP(hipSetDevice(c->device));
    bool good = false;
    MH_TRY(noflat_verify_dev(c->r[MHIP_R_DEM].as<float>(), c->r[MHIP_R_NOFLAT].as<double>(), c->H, c->W, c->sh, c->dg, c->stream, &good, c->ht, c->hb));
    *ok = good ? 1 : 0;
    return MHIP_OK;
}

// the plain fill of a band continues on the iterative schedule from the surface it has (an upper bound of the result)
static int ctx_attach_iterative_fill(mhip_ctx *c)
{
    FillRun *f = c->run[0] = new FillRun();
    f->noflat = false;
    f->dem = c->r[MHIP_R_DEM].as<float>();
    f->out = c->r[MHIP_R_FILLED].p;
    f->H = c->H; f->W = c->W;
    f->fixed_top = c->ht; f->fixed_bot = c->hb;
    f->rounds_per_batch = 16;
    return f->attach(c->stream);
}

int mhip_ctx_fill_batch(mhip_ctx *c, int kind, int32_t *active)
{
    MH_ARG(c && active && (kind == 0 || kind == 1) && (c->run[kind] || (kind == 0 && (c->pf || c->pf_done))), "ctx_fill_batch needs ctx_fill_begin");
    MH_HIP(hipSetDevice(c->device));
    if (kind == 0 && !c->pf && !c->run[0]) {   // flood finished and proven: nothing to do
        *active = 0;
        return MHIP_OK;
    }
    if (kind == 0 && c->pf) {
        const int rc = c->pf->batch(c->stream);
        *active = 0;
        if (rc != MHIP_ELIMIT) return rc;
        // a capacity gave out while the halo links were rebuilt: start the iterative schedule instead (its edge rows are upper
        // bounds of the final surface like the ones published so far: the neighbours' state stays valid)
        delete c->pf;
        c->pf = nullptr;
        FillRun *f = c->run[0] = new FillRun();
        f->noflat = false;
        f->dem = c->r[MHIP_R_DEM].as<float>();
        f->out = c->r[MHIP_R_FILLED].p;
        f->H = c->H; f->W = c->W;
        f->fixed_top = c->ht; f->fixed_bot = c->hb;
        f->rounds_per_batch = 16;
        bool a0 = false;
        MH_TRY(f->begin(c->stream, &a0));
        *active = a0;
        return MHIP_OK;
    }
    bool a = false;
    MH_TRY(c->run[kind]->batch(c->stream, &a));
    *active = a;
    return MHIP_OK;
}

int mhip_ctx_fill_certify(mhip_ctx *c, int kind, int32_t *changed)
{
    MH_ARG(c && changed && (kind == 0 || kind == 1) && (c->run[kind] || (kind == 0 && (c->pf || c->pf_done))), "ctx_fill_certify needs ctx_fill_begin");
    MH_HIP(hipSetDevice(c->device));
    if (kind == 0 && c->pf) {
        // The flood is quiescent on every band (the caller voted): write the raster and prove it (check.hip) -- K3 is a worklist
        // schedule too.  A band whose surface fails the proof continues with the iterative schedule from that surface (an upper
        // bound of the result); its neighbours follow when their halo rows move (mhip_ctx_fill_halo_changed below).
        bool violated = false;
        FillStats st;
        MH_TRY(ctx_raster(c, MHIP_R_DEPTHS));      // the bluespot depths of the owned rows ride on the pass that writes the raster, as in one context
        MH_TRY(c->pf->finish(c->stream, c->r[MHIP_R_DEPTHS].as<float>(), &st, &violated));
        delete c->pf;
        c->pf = nullptr;
        c->fill_st = st;
        c->fill_rounds = st.rounds;
        c->pf_done = true;
        c->pf_depths = true;
        *changed = 0;
        if (violated) {
            MH_TRY(ctx_attach_iterative_fill(c));
            *changed = 1;
        }
        return MHIP_OK;
    }
    if (kind == 0 && c->pf_done && !c->run[0]) {   // proven, and nothing has touched the halo rows since
        *changed = 0;
        return MHIP_OK;
    }
    bool ch = false;
    MH_TRY(c->run[kind]->certify(c->stream, &ch));
    *changed = ch ? 1 : 0;
    return MHIP_OK;
}

int mhip_ctx_fill_halo_changed(mhip_ctx *c, int kind, int side)
{
    MH_ARG(c && (kind == 0 || kind == 1) && (c->run[kind] || (kind == 0 && (c->pf || c->pf_done))) && (side == 0 || side == 1), "ctx_fill_halo_changed needs ctx_fill_begin");
    MH_HIP(hipSetDevice(c->device));
    if (kind == 0 && c->pf) return c->pf->halo_changed(side, c->stream);
    // a neighbour repaired its surface after this band's flood was finished: follow on the iterative schedule
    if (kind == 0 && !c->run[0]) MH_TRY(ctx_attach_iterative_fill(c));
    return c->run[kind]->activate_row(side, c->stream);
}

int mhip_ctx_fill_end(mhip_ctx *c, int kind)
{
    MH_ARG(c && (kind == 0 || kind == 1) && (c->run[kind] || (kind == 0 && (c->pf || c->pf_done))), "ctx_fill_end needs ctx_fill_begin");
    MH_HIP(hipSetDevice(c->device));
    FillStats st;
    bool depths_written = false;       // (of the owned rows: the flood's last pass leaves the halo rows to the neighbour)
    if (kind == 0 && c->pf) {          // (a caller that skipped the certification: no proof either)
        MH_TRY(ctx_raster(c, MHIP_R_DEPTHS));
        MH_TRY(c->pf->finish(c->stream, c->r[MHIP_R_DEPTHS].as<float>(), &st));
        delete c->pf;
        c->pf = nullptr;
        depths_written = true;
    } else if (kind == 0 && !c->run[0]) {
        st = c->fill_st;               // finished and proven by mhip_ctx_fill_certify
        depths_written = c->pf_depths;
    } else {
        MH_TRY(c->run[kind]->finish(c->stream, &st));
        delete c->run[kind];
        c->run[kind] = nullptr;
        if (kind == 0 && c->pf_done) {   // flood + repair
            st.rounds += c->fill_st.rounds;
            st.visits += c->fill_st.visits;
            st.algorithm = 4;
        }
    }
    if (kind == 0) c->pf_done = false;
    if (kind) { c->noflat_rounds = st.rounds; c->noflat_st = st; c->have[MHIP_R_NOFLAT] = true; }
    else {
        c->fill_rounds = st.rounds; c->fill_st = st; c->have[MHIP_R_FILLED] = true;
        c->pf_depths = false;
        MH_TRY(ctx_raster(c, MHIP_R_DEPTHS));
        const float *f = c->r[MHIP_R_FILLED].as<float>(), *d = c->r[MHIP_R_DEM].as<float>();
        float *o = c->r[MHIP_R_DEPTHS].as<float>();
        if (!depths_written) {
            MH_TRY(depths_dev(f, d, o, c->H * c->W, c->stream));
        } else {                       // the halo rows: the neighbour's surface over the neighbour's terrain
            if (c->ht) MH_TRY(depths_dev(f, d, o, c->ht * c->W, c->stream));
            const int64_t below = (c->ht + c->H_owned) * c->W;
            if (c->hb) MH_TRY(depths_dev(f + below, d + below, o + below, c->hb * c->W, c->stream));
        }
        c->have[MHIP_R_DEPTHS] = true;
    }
    return MHIP_OK;
}

/* the no-flats fill of a band as an integer geodesic distance transform (noflat_geo.hip) */
int mhip_ctx_geo_begin(mhip_ctx *c, double short_, double diag, int32_t *applicable, int32_t *active)
{
    MH_ARG(c && applicable && active && c->have[MHIP_R_DEM] && c->have[MHIP_R_FILLED], "ctx_geo_begin(ctx, short, diag, applicable, active) needs the plain fill");
    MH_HIP(hipSetDevice(c->device));
    MH_TRY(ctx_raster(c, MHIP_R_NOFLAT));
    MH_TRY(ctx_raster(c, MHIP_R_NGDIST));
    delete c->geo;
    GeoRun *g = c->geo = new GeoRun();
    g->dem = c->r[MHIP_R_DEM].as<float>();
    g->filled = c->r[MHIP_R_FILLED].as<float>();
    g->out = c->r[MHIP_R_NOFLAT].as<double>();
    g->dist = c->r[MHIP_R_NGDIST].as<uint32_t>();
    g->H = c->H; g->W = c->W; g->sh = short_; g->dg = diag;
    g->fixed_top = c->ht; g->fixed_bot = c->hb;
    g->allow_partial = true;                                   // the launcher votes on what happens with a partial surface
    g->seed_add = 1.01 * (double)(c->H_global * c->W) * diag;  // see noflat_seed()
    c->sh = short_; c->dg = diag;
    bool ap = false, ac = false;
    MH_TRY(g->begin(c->stream, &ap, &ac));
    *applicable = ap ? 1 : 0;
    *active = ac ? 1 : 0;
    if (!ap) {
        delete c->geo;
        c->geo = nullptr;
    }
    c->have[MHIP_R_NGDIST] = ap;
    return MHIP_OK;
}

int mhip_ctx_geo_batch(mhip_ctx *c, int32_t *active)
{
    MH_ARG(c && active && c->geo, "ctx_geo_batch needs ctx_geo_begin");
    MH_HIP(hipSetDevice(c->device));
    bool a = false;
    MH_TRY(c->geo->batch(c->stream, &a));
    *active = a ? 1 : 0;
    return MHIP_OK;
}

int mhip_ctx_geo_halo_changed(mhip_ctx *c, int side)
{
    MH_ARG(c && c->geo && (side == 0 || side == 1), "ctx_geo_halo_changed needs ctx_geo_begin");
    MH_HIP(hipSetDevice(c->device));
    return c->geo->halo_changed(side, c->stream);
}

int mhip_ctx_geo_end(mhip_ctx *c, int32_t *ok, int32_t *partial)
{
    MH_ARG(c && ok && partial && c->geo, "ctx_geo_end needs ctx_geo_begin");
    MH_HIP(hipSetDevice(c->device));
    FillStats st;
    bool good = false;
    MH_TRY(c->geo->end(c->stream, &good, &st));
    *partial = c->geo->partial ? 1 : 0;
    delete c->geo;
    c->geo = nullptr;
    *ok = good ? 1 : 0;
    if (good) {
        c->noflat_rounds = st.rounds;
        c->noflat_st = st;
        c->have[MHIP_R_NOFLAT] = true;
    }
    return MHIP_OK;
}

/* the same walk over the context's resident flow directions and (filtered) bluespot labels: no raster leaves the device */
int mhip_ctx_trace_downstream(mhip_ctx *c, const int64_t *cells_rc, int64_t n, int use_background, int32_t background, int32_t *out_label,
                              int32_t *out_found, int64_t *out_len, const int64_t *offsets, int64_t *out_cells)
{
    MH_ARG(c && n >= 0 && (n == 0 || cells_rc), "ctx_trace_downstream(ctx, cells, n, ...)");
    MH_ARG(c->have[MHIP_R_FLOWDIR] && c->have[MHIP_R_LABELS], "ctx_trace_downstream needs flow directions and labels");
    MH_ARG(!c->ht && !c->hb, "stream tracing runs on an undivided raster");
    if (n == 0) return MHIP_OK;
    MH_HIP(hipSetDevice(c->device));
    return trace_on_device(c->r[MHIP_R_FLOWDIR].as<uint8_t>(), c->r[MHIP_R_LABELS].as<int32_t>(), c->H, c->W, cells_rc, n, use_background,
                           background, out_label, out_found, out_len, offsets, out_cells, c->stream);
}

int mhip_ctx_sync(mhip_ctx *c)
{
    MH_ARG(c, "ctx");
    MH_HIP(stream_sync(c->stream));
    return MHIP_OK;
}

static int ctx_apply_keep_on(mhip_ctx *c, const uint8_t *keep, hipStream_t s);

static int ctx_ensure_labels_final(mhip_ctx *c, hipStream_t s)
{
    if (!c->labels_filtered) return ctx_apply_keep_on(c, nullptr, s);
    return MHIP_OK;
}

static int ctx_label_max(mhip_ctx *c, hipStream_t s)
{
    if (c->nlabels < 0) {
        int32_t m = 0;
        MH_TRY(label_max_dev(c->r[MHIP_R_LABELS].as<int32_t>(), c->H * c->W, &m, s));
        c->nlabels = m < 0 ? 0 : m;
    }
    return MHIP_OK;
}

// ---- the stages; each runs on the stream it is given and brackets itself with its pair of events ----------------
static int stage_begin(mhip_ctx *c, int stage, hipStream_t s, hipEvent_t **e1)
{
    hipEvent_t *e0;
    MH_TRY(ctx_events(c, stage, &e0, e1));
    MH_HIP(hipEventRecord(*e0, s));
    return MHIP_OK;
}

static int stage_depths(mhip_ctx *c, hipStream_t s)
{
    MH_ARG(c->have[MHIP_R_FILLED] && c->have[MHIP_R_DEM], "depths need the filled surface");
    MH_TRY(ctx_raster(c, MHIP_R_DEPTHS));
    MH_TRY(depths_dev(c->r[MHIP_R_FILLED].as<float>(), c->r[MHIP_R_DEM].as<float>(), c->r[MHIP_R_DEPTHS].as<float>(), c->H * c->W, s));
    c->have[MHIP_R_DEPTHS] = true;
    c->stats_valid = false;
    c->hyps_total = -1;
    return MHIP_OK;
}

// with_depths == false: the caller computes the bluespot depths on another stream (stage DAG)
static int stage_fill(mhip_ctx *c, hipStream_t s, bool with_depths = true)
{
    const int64_t H = c->H, W = c->W;
    MH_ARG(c->have[MHIP_R_DEM], "FILL needs the DEM");
    MH_TRY(ctx_raster(c, MHIP_R_FILLED));
    MH_TRY(ctx_raster(c, MHIP_R_DEPTHS));
    hipEvent_t *e1;
    MH_TRY(stage_begin(c, MHIP_STAGE_FILL, s, &e1));
    FillStats st;
    bool depths_done = false;   // the priority-flood's last pass writes filled - dem next to the filled surface
    MH_TRY(fill_plain_dev(c->r[MHIP_R_DEM].as<float>(), c->r[MHIP_R_FILLED].as<float>(), H, W, s, &st, c->r[MHIP_R_DEPTHS].as<float>(),
                          &depths_done));
    c->have[MHIP_R_FILLED] = true;
    c->have[MHIP_R_DEPTHS] = depths_done;
    if (with_depths && !depths_done) MH_TRY(stage_depths(c, s));
    MH_HIP(hipEventRecord(*e1, s));
    c->ev_valid[MHIP_STAGE_FILL] = true;
    c->fill_rounds = st.rounds;
    c->fill_st = st;
    return MHIP_OK;
}

// shdg_done: minimum_safe_short_and_diag of the current DEM is already in c->sh / c->dg (computed next to the fill)
// with_flowdir: FLOWDIR is part of the same request -- the geodesic transform's finishing pass writes the directions as well when
// it can (one context, regular surface); *flowdir_done then tells the caller that stage_flowdir has nothing left to do
static int stage_noflat(mhip_ctx *c, hipStream_t s, bool shdg_done = false, StageHook *tail_hook = nullptr, bool with_flowdir = false,
                        bool *flowdir_done = nullptr)
{
    const int64_t H = c->H, W = c->W, n = H * W;
    MH_ARG(c->have[MHIP_R_DEM], "NOFLAT needs the DEM");
    MH_TRY(ctx_raster(c, MHIP_R_NOFLAT));
    hipEvent_t *e1;
    MH_TRY(stage_begin(c, MHIP_STAGE_NOFLAT, s, &e1));
    if (!shdg_done) {
        // (the flood of THIS DEM has folded its extremes on the way: a request without the bluespot branch -- BASELINE configs[1] -- used
        // to run the reduction over the DEM all the same, 0.38 ms of its 2.15 ms step)
        if (c->have[MHIP_R_FILLED] && c->fill_st.have_minmax) short_diag_from_minmax(c->fill_st.dem_min, c->fill_st.dem_max, c->fill_st.dem_nan, &c->sh, &c->dg);
        else MH_TRY(short_diag_dev(c->r[MHIP_R_DEM].as<float>(), n, &c->sh, &c->dg, s));
    }
    FillStats st;
    if (!c->have[MHIP_R_FILLED]) {  // the plain fill seeds the no-flats iteration (fill_noflat_dev)
        MH_TRY(ctx_raster(c, MHIP_R_FILLED));
        FillStats st0;
        MH_TRY(fill_plain_dev(c->r[MHIP_R_DEM].as<float>(), c->r[MHIP_R_FILLED].as<float>(), H, W, s, &st0));
        c->have[MHIP_R_FILLED] = true;
    }
    D8Sink d8;
    static const bool fuse_d8 = [] { const char *e = dev_env("MHIP_D8_FUSE"); return !(e && e[0] == '0'); }();   // (development: 0 = D8 as a pass of its own)
    if (with_flowdir && fuse_d8 && !c->ht && !c->hb) {
        MH_TRY(ctx_raster(c, MHIP_R_FLOWDIR));
        MH_TRY(c->nodir_cnt.alloc(4));
        MH_HIP(hipMemsetAsync(c->nodir_cnt.p, 0, 4, s));
        d8.flowdir = c->r[MHIP_R_FLOWDIR].as<uint8_t>();
        d8.nodir = c->nodir_cnt.as<unsigned int>();
    }
    MH_TRY(fill_noflat_dev(c->r[MHIP_R_DEM].as<float>(), c->r[MHIP_R_NOFLAT].as<double>(), H, W, c->sh, c->dg, s, &st,
                           c->r[MHIP_R_FILLED].as<float>(), tail_hook, d8.flowdir ? &d8 : nullptr));
    if (flowdir_done) *flowdir_done = d8.done;
    MH_HIP(hipEventRecord(*e1, s));
    c->ev_valid[MHIP_STAGE_NOFLAT] = true;
    c->noflat_rounds = st.rounds;
    c->noflat_st = st;
    c->have[MHIP_R_NOFLAT] = true;
    return MHIP_OK;
}

static int stage_flowdir(mhip_ctx *c, hipStream_t s)
{
    MH_ARG(c->have[MHIP_R_NOFLAT], "FLOWDIR needs the no-flats surface");
    MH_TRY(ctx_raster(c, MHIP_R_FLOWDIR));
    hipEvent_t *e1;
    MH_TRY(stage_begin(c, MHIP_STAGE_FLOWDIR, s, &e1));
    c->acc_keep.valid = false;
    MH_TRY(c->nodir_cnt.alloc(4));
    MH_HIP(hipMemsetAsync(c->nodir_cnt.p, 0, 4, s));
    MH_TRY(d8_dev(c->r[MHIP_R_NOFLAT].as<double>(), c->r[MHIP_R_FLOWDIR].as<uint8_t>(), c->H, c->W, 1, s, c->row0 - c->ht,
                  c->H_global, c->nodir_cnt.as<unsigned int>()));
    MH_HIP(hipEventRecord(*e1, s));
    c->ev_valid[MHIP_STAGE_FLOWDIR] = true;
    c->have[MHIP_R_FLOWDIR] = true;
    c->nodir_valid = !c->ht && !c->hb;     // (a band's halo rows are computed from clamped data: their codes do not count)
    return MHIP_OK;
}

// the no-flats fill's finishing pass wrote the flow directions (stage_noflat: with_flowdir): the stage is an empty interval
static int stage_flowdir_fused(mhip_ctx *c, hipStream_t s)
{
    hipEvent_t *e1;
    MH_TRY(stage_begin(c, MHIP_STAGE_FLOWDIR, s, &e1));
    MH_HIP(hipEventRecord(*e1, s));
    c->ev_valid[MHIP_STAGE_FLOWDIR] = true;
    c->have[MHIP_R_FLOWDIR] = true;
    c->nodir_valid = true;
    return MHIP_OK;
}

static int stage_accum(mhip_ctx *c, hipStream_t s, PourLink *pour = nullptr)
{
    MH_ARG(c->have[MHIP_R_FLOWDIR], "ACCUM needs flow directions");
    MH_TRY(ctx_raster(c, MHIP_R_ACCUM));
    hipEvent_t *e1;
    MH_TRY(stage_begin(c, MHIP_STAGE_ACCUM, s, &e1));
    bool delta_done = false;
    // a row band right behind its boundary pass (own contributions in ACCUM, the neighbours' values in the halo rows by now): only
    // the flux that enters at the seams is added, along the paths the kept perimeter graph says it takes (accum.hip)
    if ((c->ht || c->hb) && c->acc_keep.valid)
        MH_TRY(accum_band_delta_dev(c->r[MHIP_R_FLOWDIR].as<uint8_t>(), c->r[MHIP_R_ACCUM].as<double>(), c->H, c->W, s, c->ht, c->hb, &c->acc_keep, &delta_done));
    c->accum_algorithm = delta_done ? 1 : 0;
    c->acc_keep.valid = false;
    if (!delta_done)
        MH_TRY(accum_dev(c->r[MHIP_R_FLOWDIR].as<uint8_t>(), c->r[MHIP_R_ACCUM].as<double>(), c->H, c->W, s, c->ht, c->hb, 0, nullptr, pour));
    MH_HIP(hipEventRecord(*e1, s));
    c->ev_valid[MHIP_STAGE_ACCUM] = true;
    c->have[MHIP_R_ACCUM] = true;
    return MHIP_OK;
}

static int stage_label(mhip_ctx *c, hipStream_t s)
{
    const int64_t H = c->H, W = c->W, n = H * W;
    MH_ARG(c->have[MHIP_R_DEPTHS] || c->have[MHIP_R_FILLED], "LABEL needs bluespot depths");
    MH_TRY(ctx_raster(c, MHIP_R_LABELS));
    if (!c->tmp_i32.p) MH_TRY(c->tmp_i32.alloc(4 * (size_t)n));
    hipEvent_t *e1;
    MH_TRY(stage_begin(c, MHIP_STAGE_LABEL, s, &e1));
    if (!c->have[MHIP_R_DEPTHS]) MH_TRY(stage_depths(c, s));   // stage DAG: the fill left them to this branch
    // (label_stats of the raw labels rides on the labelling's last pass: as two passes 21.8 -> 22.2 ms a step, and with the statistics
    // behind the stage's event -- beside the watersheds, off the critical path -- 22.3: round 4)
    MH_TRY(ccl8_f32_dev(c->r[MHIP_R_DEPTHS].as<float>(), c->r[MHIP_R_LABELS].as<int32_t>(), c->tmp_i32.as<int32_t>(), H, W,
                        &c->nlabels_raw, s, &c->raw_stats));
    MH_HIP(hipEventRecord(*e1, s));
    c->ev_valid[MHIP_STAGE_LABEL] = true;
    c->have[MHIP_R_LABELS] = true;
    c->labels_components = true;
    c->labels_filtered = false;
    c->nlabels = c->nlabels_raw;
    c->stats_valid = false;
    c->hyps_total = -1;
    return MHIP_OK;
}

// the buffers of a PourLink for this context's raster and labels; zeroed on `s` (the stream of the watersheds' tile pass)
static int pour_link_buffers(mhip_ctx *c, PourLink *pl, hipStream_t s)
{
    const int64_t H = c->H, W = c->W;
    const int64_t ntiles = cdiv(H, 64) * cdiv(W, 64);
    MH_TRY(c->pp_mask0.alloc(2 * 256 * (size_t)ntiles));
    MH_TRY(c->pp_list.alloc(8 * (size_t)POUR_TILE_CAP * (size_t)ntiles));
    MH_TRY(c->pp_tiles.alloc(12 * (size_t)ntiles));
    MH_TRY(c->pp_misc.alloc(16));
    MH_TRY(c->pp_key.alloc(8 * (size_t)(c->nlabels + 1)));
    MH_HIP(hipMemsetAsync(c->pp_misc.p, 0, 16, s));
    MH_HIP(hipMemsetAsync(c->pp_key.p, 0, 8 * (size_t)(c->nlabels + 1), s));
    pl->dev.mask0 = c->pp_mask0.as<uint16_t>();
    pl->dev.list = c->pp_list.as<uint2>();
    pl->dev.tile_key0 = c->pp_tiles.as<unsigned long long>();
    pl->dev.tile_cnt = reinterpret_cast<uint32_t *>(c->pp_tiles.as<unsigned long long>() + ntiles);
    pl->dev.flags = c->pp_misc.as<uint32_t>() + 1;
    pl->dev.components = c->labels_components ? 1 : 0;
    pl->dev.key = c->pp_key.as<unsigned long long>();
    pl->dev.nlab = (uint32_t)c->nlabels;
    pl->ev = c->ev_cand;
    return MHIP_OK;
}

static int stage_watershed(mhip_ctx *c, hipStream_t s, PourLink *pour = nullptr)
{
    const int64_t H = c->H, W = c->W, n = H * W;
    MH_ARG(c->have[MHIP_R_LABELS] && c->have[MHIP_R_FLOWDIR], "WATERSHED needs labels and flow directions");
    MH_TRY(ctx_ensure_labels_final(c, s));
    MH_TRY(ctx_label_max(c, s));
    MH_TRY(ctx_raster(c, MHIP_R_WATERSHEDS));
    hipEvent_t *e1;
    MH_TRY(stage_begin(c, MHIP_STAGE_WATERSHED, s, &e1));
    if (pour) MH_TRY(pour_link_buffers(c, pour, s));
    // (out of place: the watersheds start from the label raster without a copy of it)
    MH_TRY(watersheds_dev(c->r[MHIP_R_FLOWDIR].as<uint8_t>(), c->r[MHIP_R_WATERSHEDS].as<int32_t>(), H, W, 0, s, false,
                          c->nodir_valid ? c->nodir_cnt.as<unsigned int>() : nullptr, c->r[MHIP_R_LABELS].as<int32_t>(), pour));
    MH_TRY(c->ws_counts.alloc(8 * (size_t)(c->nlabels + 1)));
    MH_TRY(label_count_dev(c->r[MHIP_R_WATERSHEDS].as<int32_t>(), n, c->nlabels, c->ws_counts.as<int64_t>(), s, W));
    MH_HIP(hipEventRecord(*e1, s));
    c->ev_valid[MHIP_STAGE_WATERSHED] = true;
    c->have[MHIP_R_WATERSHEDS] = true;
    return MHIP_OK;
}

static int stage_pourpoints(mhip_ctx *c, hipStream_t s, PourLink *pour = nullptr)
{
    const int64_t H = c->H, W = c->W;
    MH_ARG(c->have[MHIP_R_LABELS] && (c->have[MHIP_R_ACCUM] || c->have[MHIP_R_NOFLAT]),
           "POURPOINTS needs labels and accumulated flow or the no-flats surface");
    MH_TRY(ctx_ensure_labels_final(c, s));
    MH_TRY(ctx_label_max(c, s));
    MH_TRY(c->pour.alloc(sizeof(mhip_index_record) * (size_t)(c->nlabels + 1)));
    hipEvent_t *e1;
    MH_TRY(stage_begin(c, MHIP_STAGE_POURPOINTS, s, &e1));
    // bluespots.py:195-206: max accumulated flow if available, else min of the no-flats surface
    bool from_keys = false;
    if (pour && pour->consumed && c->have[MHIP_R_ACCUM]) {
        // the accumulation's final pass has left one key per label (common.hpp: PourLink) -- unless the candidate list overflowed
        // or a cell stayed unresolved (a flow cycle): then the general pass below
        // (the records are queued before the flags are known: one host round trip instead of two at the end of a request)
        uint32_t h[3] = {0, 1, 1};
        MH_HIP(hipMemcpyAsync(h, c->pp_misc.p, 12, hipMemcpyDeviceToHost, s));
        MH_TRY(pour_finish_dev(c->pp_key.as<unsigned long long>(), c->pp_tiles.as<unsigned long long>(), cdiv(H, 64) * cdiv(W, 64), c->nlabels, W,
                               c->pour.as<mhip_index_record>(), s));
        MH_HIP(stream_sync(s));
        from_keys = !h[1] && !h[2];
    }
    c->pour_algorithm = from_keys ? 1 : 0;
    if (from_keys) {
    } else if (c->have[MHIP_R_ACCUM])
        MH_TRY(label_arg_dev(c->r[MHIP_R_ACCUM].as<double>(), c->r[MHIP_R_LABELS].as<int32_t>(), H, W, c->nlabels, true,
                             c->pour.as<mhip_index_record>(), s, c->labels_components));
    else
        MH_TRY(label_arg_dev(c->r[MHIP_R_NOFLAT].as<double>(), c->r[MHIP_R_LABELS].as<int32_t>(), H, W, c->nlabels, false,
                             c->pour.as<mhip_index_record>(), s));
    MH_HIP(hipEventRecord(*e1, s));
    c->ev_valid[MHIP_STAGE_POURPOINTS] = true;
    return MHIP_OK;
}

// Stage DAG:  FILL -> NOFLAT -> FLOWDIR -> ACCUM ------.
//                \-> LABEL ----------\-> WATERSHED ----+-> POURPOINTS
// A request that holds both sides runs the bluespot branch (LABEL, WATERSHED) on a second stream driven by a
// second host thread (both branches read back small results between launches), so the latency-bound rounds of the
// no-flats fill and the walks of the accumulation share the GPU with the labelling instead of queueing behind each
// other.  MHIP_SERIAL=1 in the environment keeps everything on the context's stream.
int mhip_ctx_run(mhip_ctx *c, int mask)
{
    MH_ARG(c, "ctx");
    MH_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    if (c->nranks > 1 || c->ht || c->hb) {
        // row-band mode: the fills run through mhip_ctx_fill_begin/batch (halo refreshes in between); stages whose
        // cross-band protocol is not built yet are refused instead of silently computing band-local results
        MH_ARG((mask & ~(MHIP_STAGE_FLOWDIR | MHIP_STAGE_ACCUM)) == 0,
               "this stage runs through the band entry points on a row band (mhip_ctx_fill_*, mhip_ctx_band_*)");
    }
    static const bool serial_env = [] { const char *e = dev_env("MHIP_SERIAL"); return e && e[0] == '1'; }();
    const int side_a = mask & (MHIP_STAGE_NOFLAT | MHIP_STAGE_FLOWDIR | MHIP_STAGE_ACCUM);
    const int side_b = mask & (MHIP_STAGE_LABEL | MHIP_STAGE_WATERSHED);
    const bool overlap = side_a && side_b && !serial_env;

    if (!overlap) {
        if (mask & MHIP_STAGE_FILL) MH_TRY(stage_fill(c, s));
        bool fd_done = false;
        if (mask & MHIP_STAGE_NOFLAT) MH_TRY(stage_noflat(c, s, false, nullptr, (mask & MHIP_STAGE_FLOWDIR) != 0, &fd_done));
        if (mask & MHIP_STAGE_FLOWDIR) MH_TRY(fd_done ? stage_flowdir_fused(c, s) : stage_flowdir(c, s));
        if (mask & MHIP_STAGE_ACCUM) MH_TRY(stage_accum(c, s));
        if (mask & MHIP_STAGE_LABEL) MH_TRY(stage_label(c, s));
        if (mask & MHIP_STAGE_WATERSHED) MH_TRY(stage_watershed(c, s));
        if (mask & MHIP_STAGE_POURPOINTS) MH_TRY(stage_pourpoints(c, s));
        return MHIP_OK;
    }

    // events and the side streams are created here, on the calling thread: the maps are not touched concurrently
    hipEvent_t *ea, *eb;
    for (int st : {MHIP_STAGE_FILL, MHIP_STAGE_NOFLAT, MHIP_STAGE_FLOWDIR, MHIP_STAGE_ACCUM, MHIP_STAGE_LABEL, MHIP_STAGE_WATERSHED,
                   MHIP_STAGE_POURPOINTS}) {
        if (mask & st) {
            MH_TRY(ctx_events(c, st, &ea, &eb));
            c->ev_valid[st];   // creates the key
        }
    }
    // (measured and settled in rounds 3 / 4, the knobs are gone: the priorities the other way round, and a CU mask that keeps the side
    // streams off part of the chip so that the label branch could run next to the no-flats fill's latency-bound rounds -- neither
    // moved the step)
    auto side_stream = [&](hipStream_t *st) -> int {
        int least = 0, greatest = 0;
        MH_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
        MH_HIP(hipStreamCreateWithPriority(st, hipStreamNonBlocking, least));
        return MHIP_OK;
    };
    // LABEL only has to finish before the no-flats fill does: lowest priority; WATERSHED is on the critical path
    if (!c->stream_b) MH_TRY(side_stream(&c->stream_b));
    if (!c->stream_c) MH_TRY(side_stream(&c->stream_c));
    if (!c->ev_fork) {
        MH_HIP(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
        MH_HIP(hipEventCreateWithFlags(&c->ev_flowdir, hipEventDisableTiming));
        MH_HIP(hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming));
        MH_HIP(hipEventCreateWithFlags(&c->ev_label, hipEventDisableTiming));
        MH_HIP(hipEventCreateWithFlags(&c->ev_tail, hipEventDisableTiming));
    }
    if (!c->ev_cand) MH_HIP(hipEventCreateWithFlags(&c->ev_cand, hipEventDisableTiming));
    hipStream_t sb = c->stream_b;
    const bool do_fill = (mask & MHIP_STAGE_FILL) != 0;
    MH_ARG(c->have[MHIP_R_DEM] || !(mask & (MHIP_STAGE_FILL | MHIP_STAGE_NOFLAT)), "FILL / NOFLAT need the DEM");

    // hand-overs between the two host threads (each value is an error code)
    std::promise<int> fill_done, shdg_done, flowdir_ready, label_ready, tail_reached;
    std::future<int> fill_fut = fill_done.get_future(), shdg_fut = shdg_done.get_future(), tail_fut = tail_reached.get_future();
    // The label branch does not start with the no-flats fill but behind it (ev_tail).  Measured at 16384^2 (ms per step): label
    // next to the whole no-flats fill 38.0 (the fill's rounds 14.6 instead of 9.8: every one of its ~85 small launches queues behind
    // the labelling's long workgroups), from the fill's latency-bound tail rounds on 37.4, behind the fill 36.7 -- then labelling and
    // watersheds run next to D8 + accumulation.  MHIP_LABEL_START = 0 / 1 / 2 selects (development knob).
    struct TailCtx {
        mhip_ctx *c;
        std::promise<int> *p;
    } tail_ctx{c, &tail_reached};
    StageHook tail_hook;
    tail_hook.arg = &tail_ctx;
    tail_hook.fn = [](void *arg, hipStream_t st) {
        TailCtx *t = static_cast<TailCtx *>(arg);
        t->p->set_value(hipEventRecord(t->c->ev_tail, st) == hipSuccess ? MHIP_OK : MHIP_EHIP);
    };
    std::future<int> flowdir_fut = flowdir_ready.get_future(), label_fut = label_ready.get_future();
    // Pour points out of the accumulation's final pass (common.hpp: PourLink): the watersheds' tile pass on the other thread lists
    // the candidate cells, the accumulation's final pass on this one waits for them.  MHIP_POUR=pass (development): the pass
    // over accumulation + labels at the end of the request instead.
    struct CandHand {
        std::promise<int> p;
        std::future<int> f;
        std::atomic<bool> set{false};
    } cand_hand;
    cand_hand.f = cand_hand.p.get_future();
    PourLink pour_link;
    pour_link.arg = &cand_hand;
    pour_link.notify = [](void *a, int v) {
        CandHand *h = static_cast<CandHand *>(a);
        if (!h->set.exchange(true)) h->p.set_value(v);
    };
    pour_link.wait = [](void *a) { return static_cast<CandHand *>(a)->f.get(); };
    static const bool pour_pass = [] { const char *e = dev_env("MHIP_POUR"); return e && std::string(e) == "pass"; }();
    PourLink *const pour = ((mask & MHIP_STAGE_ACCUM) && (mask & MHIP_STAGE_WATERSHED) && (mask & MHIP_STAGE_POURPOINTS) && !pour_pass) ? &pour_link : nullptr;
    const bool ws_needs_new_flowdir = (mask & MHIP_STAGE_WATERSHED) && (mask & MHIP_STAGE_FLOWDIR);
    int rc_b = MHIP_OK;
    char err_b[512] = "";
    bool shdg_set = false, label_set = false;   // whatever happens on the side thread, the main thread is never left waiting
    c->side.run([&] {
        rc_b = [&]() -> int {
            MH_HIP(hipSetDevice(c->device));
            // the epsilon of the no-flats fill only needs the DEM: computed while the plain fill runs
            int rc_e = MHIP_OK;
            // (with the plain fill in the same request its first kernel delivers the DEM's extremes: see below)
            if ((mask & MHIP_STAGE_NOFLAT) && !do_fill) rc_e = short_diag_dev(c->r[MHIP_R_DEM].as<float>(), c->H * c->W, &c->sh, &c->dg, sb);
            if (rc_e != MHIP_OK) snprintf(err_b, sizeof(err_b), "%s", get_error());
            shdg_done.set_value(rc_e);
            shdg_set = true;
            int rc_l = rc_e == MHIP_OK ? fill_fut.get() : rc_e;   // ev_fork has been recorded on the main stream
            if (rc_l == MHIP_OK) rc_l = tail_fut.get();           // ... and ev_tail behind it (or at the same place)
            if (rc_l == MHIP_OK && hipStreamWaitEvent(sb, c->ev_tail, 0) != hipSuccess) rc_l = MHIP_EHIP;
            if (rc_l == MHIP_OK && (mask & MHIP_STAGE_LABEL)) rc_l = stage_label(c, sb);   // incl. the bluespot depths
            else if (rc_l == MHIP_OK && do_fill && !c->have[MHIP_R_DEPTHS]) rc_l = stage_depths(c, sb);
            // both consumers (WATERSHED here, POURPOINTS on the main thread) want the final labels: settle them once
            if (rc_l == MHIP_OK && (mask & (MHIP_STAGE_WATERSHED | MHIP_STAGE_POURPOINTS)) && c->have[MHIP_R_LABELS]) {
                rc_l = ctx_ensure_labels_final(c, sb);
                if (rc_l == MHIP_OK) rc_l = ctx_label_max(c, sb);
            }
            if (rc_l == MHIP_OK && hipEventRecord(c->ev_label, sb) != hipSuccess) rc_l = MHIP_EHIP;
            if (rc_l != MHIP_OK && !err_b[0]) snprintf(err_b, sizeof(err_b), "%s", get_error());
            label_ready.set_value(rc_l);
            label_set = true;
            MH_TRY(rc_l);
            hipStream_t sw = sb;
            if (mask & MHIP_STAGE_WATERSHED) {
                sw = c->stream_c;
                MH_HIP(hipStreamWaitEvent(sw, c->ev_label, 0));
                if (ws_needs_new_flowdir) {
                    MH_TRY(flowdir_fut.get());
                    MH_HIP(hipStreamWaitEvent(sw, c->ev_flowdir, 0));
                }
                MH_TRY(stage_watershed(c, sw, pour));
            }
            MH_HIP(hipEventRecord(c->ev_join, sw));
            return MHIP_OK;
        }();
        if (rc_b != MHIP_OK && !err_b[0]) snprintf(err_b, sizeof(err_b), "%s", get_error());
        if (!shdg_set) shdg_done.set_value(rc_b);
        if (!label_set) label_ready.set_value(rc_b);
        pour_link.notify(pour_link.arg, 0);       // (no candidates if the watersheds never got that far: nobody is left waiting)
    });
    int rc_a = MHIP_OK;
    if (do_fill) rc_a = stage_fill(c, s, /*with_depths=*/false);
    if (rc_a == MHIP_OK && hipEventRecord(c->ev_fork, s) != hipSuccess) rc_a = MHIP_EHIP;
    fill_done.set_value(rc_a);            // releases the other thread in either case
    const int rc_e = shdg_fut.get();
    if (rc_a == MHIP_OK) rc_a = [&]() -> int {
        MH_TRY(rc_e);
        if (do_fill && (mask & MHIP_STAGE_NOFLAT)) {
            // minimum_safe_short_and_diag: from the extremes the priority-flood's tile kernel found on its way through the DEM; the
            // iterative schedule (fall-back) has none: one pass over the DEM
            if (c->fill_st.have_minmax) short_diag_from_minmax(c->fill_st.dem_min, c->fill_st.dem_max, c->fill_st.dem_nan, &c->sh, &c->dg);
            else MH_TRY(short_diag_dev(c->r[MHIP_R_DEM].as<float>(), c->H * c->W, &c->sh, &c->dg, s));
        }
        static const int label_start = [] { const char *e = dev_env("MHIP_LABEL_START"); return e ? atoi(e) : 2; }();   // 0: with the no-flats fill, 1: at its tail, 2: after it
        if (label_start == 0) tail_hook.fire(s);
        bool fd_done = false;
        if (mask & MHIP_STAGE_NOFLAT)
            MH_TRY(stage_noflat(c, s, /*shdg_done=*/true, label_start == 1 ? &tail_hook : nullptr, (mask & MHIP_STAGE_FLOWDIR) != 0, &fd_done));
        if (mask & MHIP_STAGE_FLOWDIR) {
            MH_TRY(fd_done ? stage_flowdir_fused(c, s) : stage_flowdir(c, s));
            MH_HIP(hipEventRecord(c->ev_flowdir, s));
        }
        return MHIP_OK;
    }();
    tail_hook.fire(s);                    // (no NOFLAT in the mask, or it failed early: the other thread is never left waiting)
    flowdir_ready.set_value(rc_a);
    if (rc_a == MHIP_OK && (mask & MHIP_STAGE_ACCUM)) rc_a = stage_accum(c, s, pour);
    // POURPOINTS needs the final labels and the accumulation, not the watersheds: it runs next to them
    const int rc_l = label_fut.get();
    if (rc_a == MHIP_OK && rc_l == MHIP_OK && (mask & MHIP_STAGE_POURPOINTS)) {
        rc_a = hipStreamWaitEvent(s, c->ev_label, 0) == hipSuccess ? stage_pourpoints(c, s, pour) : MHIP_EHIP;
    }
    c->side.wait();
    if (rc_a != MHIP_OK) return rc_a;
    if (rc_b != MHIP_OK) {
        set_error("%s", err_b);
        return rc_b;
    }
    MH_HIP(hipStreamWaitEvent(s, c->ev_join, 0));
    return MHIP_OK;
}

int mhip_ctx_stage_ms(mhip_ctx *c, int stage, float *ms)
{
    MH_ARG(c && ms, "ctx_stage_ms(ctx, stage, ms)");
    auto it = c->ev.find(stage);
    MH_ARG(it != c->ev.end() && c->ev_valid[stage], "stage has not been run");
    MH_HIP(hipEventSynchronize(it->second.second));
    MH_HIP(hipEventElapsedTime(ms, it->second.first, it->second.second));
    return MHIP_OK;
}

int mhip_ctx_kernel_ms(mhip_ctx *c, const char *kernel, float *ms_total, int32_t *launches)
{
    MH_ARG(c && kernel && ms_total && launches, "ctx_kernel_ms(ctx, kernel, ms, launches)");
    const std::string k(kernel);
    if (k == "d8") {
        *launches = 1;
        return mhip_ctx_stage_ms(c, MHIP_STAGE_FLOWDIR, ms_total);
    }
    if (k == "d8_steady") {
        // steady-state throughput of the D8 stencil: 16 launches back to back between ONE pair of events on the context's stream
        // (a pair of events around a single 0.43 ms launch adds ~30 us of bracket to it); the resident surface and directions
        MH_ARG(c->have[MHIP_R_NOFLAT] && !c->ht && !c->hb, "d8_steady needs the no-flats surface on an undivided context");
        MH_HIP(hipSetDevice(c->device));
        MH_TRY(ctx_raster(c, MHIP_R_FLOWDIR));
        MH_TRY(c->nodir_cnt.alloc(4));
        constexpr int REPS = 16;
        hipEvent_t *e0, *e1;
        MH_TRY(ctx_events(c, 1 << 30, &e0, &e1));
        hipStream_t s = c->stream;
        MH_HIP(hipMemsetAsync(c->nodir_cnt.p, 0, 4, s));
        for (int i = 0; i < REPS + 2; ++i) {
            if (i == 2) MH_HIP(hipEventRecord(*e0, s));      // (two untimed launches first)
            MH_TRY(d8_dev(c->r[MHIP_R_NOFLAT].as<double>(), c->r[MHIP_R_FLOWDIR].as<uint8_t>(), c->H, c->W, 1, s, 0, c->H_global,
                          c->nodir_cnt.as<unsigned int>()));
        }
        MH_HIP(hipEventRecord(*e1, s));
        MH_HIP(hipEventSynchronize(*e1));
        MH_HIP(hipEventElapsedTime(ms_total, *e0, *e1));
        c->have[MHIP_R_FLOWDIR] = true;
        c->nodir_valid = true;
        *launches = REPS;
        return MHIP_OK;
    }
    if (k == "hyps_table" || k == "final_depths") {      // events around the one kernel inside mhip_ctx_hyps / mhip_ctx_final_depths
        *launches = 1;
        return mhip_ctx_stage_ms(c, k == "hyps_table" ? HYPS_KERNEL_SLOT : FINAL_KERNEL_SLOT, ms_total);
    }
    if (k == "fill_round") {
        *launches = c->fill_rounds;
        return mhip_ctx_stage_ms(c, MHIP_STAGE_FILL, ms_total);
    }
    if (k == "noflat_round") {
        *launches = c->noflat_rounds;
        return mhip_ctx_stage_ms(c, MHIP_STAGE_NOFLAT, ms_total);
    }
    set_error("unknown kernel family '%s'", kernel);
    return MHIP_EINVAL;
}

int mhip_ctx_get_i64(mhip_ctx *c, const char *key, int64_t *value)
{
    MH_ARG(c && key && value, "ctx_get_i64(ctx, key, value)");
    const std::string k(key);
    if (k == "nlabels_raw") *value = c->nlabels_raw;
    else if (k == "nlabels") {
        if (c->nlabels < 0 && c->have[MHIP_R_LABELS]) {   // labels came in by upload: their count is max(labelled), like the reference takes it
            MH_HIP(hipSetDevice(c->device));
            MH_TRY(ctx_label_max(c, c->stream));
        }
        *value = c->nlabels;
    }
    else if (k == "fill_rounds") *value = c->fill_rounds;
    else if (k == "noflat_rounds") *value = c->noflat_rounds;
    else if (k == "fill_visits") *value = c->fill_st.visits;
    else if (k == "fill_cycles") *value = c->fill_st.cycles;
    else if (k == "fill_tiles") *value = c->fill_st.tiles;
    else if (k == "fill_algorithm") *value = c->fill_st.algorithm;   // 0 iterative tile schedule, 1 tiled priority-flood
    else if (k == "fill_launches") *value = c->fill_st.rounds;
    else if (k == "fill_hot_launches") *value = c->fill_st.hot_launches;
    else if (k == "noflat_hot_launches") *value = c->noflat_st.hot_launches;
    else if (k == "accum_algorithm") *value = c->accum_algorithm;   // 0 full accumulation, 1 a row band's second pass as a delta over the boundary pass's graph
    else if (k == "pour_algorithm") *value = c->pour_algorithm;   // 0 a pass over values + labels (label_ops.hip), 1 keys out of the accumulation's final pass (PourLink)
    else if (k == "noflat_algorithm") *value = c->noflat_st.algorithm;   // 0 float64 relaxation (fill.hip), 2 integer geodesic transform (noflat_geo.hip)
    else if (k == "noflat_visits") *value = c->noflat_st.visits;
    else if (k == "noflat_reject") *value = c->noflat_st.geo_reject;            // diagnostics: FillStats::geo_reject and its counts
    else if (k == "noflat_reject_irregular") *value = c->noflat_st.geo_irregular;
    else if (k == "noflat_reject_unreached") *value = c->noflat_st.geo_unreached;
    else if (k == "noflat_reject_mismatch") *value = c->noflat_st.geo_mismatch;
    else if (k == "noflat_cycles") *value = c->noflat_st.cycles;
    else if (k == "hyps_bins") *value = c->hyps_total;               // -1: no table (mhip_ctx_hyps)
    else if (k == "hyps_lds_spills") *value = c->hyps_spills;        // runs that found no slot in their tile's LDS table
    else if (k == "H") *value = c->H;
    else if (k == "W") *value = c->W;
    else {
        set_error("unknown key '%s'", key);
        return MHIP_EINVAL;
    }
    return MHIP_OK;
}

int mhip_ctx_get_f64(mhip_ctx *c, const char *key, double *value)
{
    MH_ARG(c && key && value, "ctx_get_f64(ctx, key, value)");
    const std::string k(key);
    if (k == "short") *value = c->sh;
    else if (k == "diag") *value = c->dg;
    else if (k == "fill_hot_ms") *value = c->fill_st.hot_ms;          // pf_tile_kernel, HIP events around its launch
    else if (k == "noflat_hot_ms") *value = c->noflat_st.hot_ms;      // the ng_round_kernel launches (span of the round loop)
    else {
        set_error("unknown key '%s'", key);
        return MHIP_EINVAL;
    }
    return MHIP_OK;
}

int mhip_ctx_raw_stats(mhip_ctx *c, mhip_stat_record *records)
{
    MH_ARG(c && records && c->raw_stats.p && c->nlabels_raw >= 0, "ctx_raw_stats needs a LABEL run");
    MH_HIP(hipMemcpyAsync(records, c->raw_stats.p, sizeof(mhip_stat_record) * (size_t)(c->nlabels_raw + 1), hipMemcpyDeviceToHost,
                          c->stream));
    MH_HIP(stream_sync(c->stream));
    return MHIP_OK;
}

int mhip_ctx_apply_keep(mhip_ctx *c, const uint8_t *keep)
{
    MH_ARG(c, "ctx");
    MH_HIP(hipSetDevice(c->device));
    return ctx_apply_keep_on(c, keep, c->stream);
}

static int ctx_apply_keep_on(mhip_ctx *c, const uint8_t *keep, hipStream_t s)
{
    MH_ARG(c && c->have[MHIP_R_LABELS] && c->nlabels_raw >= 0 && !c->labels_filtered, "ctx_apply_keep needs a fresh LABEL run");
    const int64_t n = c->H * c->W;
    if (keep) {
        std::vector<int32_t> lut;
        c->nlabels = build_rank_lut(keep, c->nlabels_raw, lut);
        DevBuf d_lut;
        MH_TRY(d_lut.alloc(lut.size() * 4));
        MH_HIP(hipMemcpyAsync(d_lut.p, lut.data(), lut.size() * 4, hipMemcpyHostToDevice, s));
        MH_TRY(relabel_lut_dev(c->r[MHIP_R_LABELS].as<int32_t>(), d_lut.as<int32_t>(), c->nlabels_raw, n, s));
        MH_TRY(c->stats.alloc(sizeof(mhip_stat_record) * (size_t)(c->nlabels + 1)));
        MH_TRY(label_stats_dev(c->r[MHIP_R_DEPTHS].as<float>(), c->r[MHIP_R_LABELS].as<int32_t>(), n, c->nlabels,
                               c->stats.as<mhip_stat_record>(), s, c->W, c->labels_components));   // (kept components stay components)
    } else {
        // keep everything (background excluded by construction): labels and stats are the raw ones
        c->nlabels = c->nlabels_raw;
        MH_TRY(c->stats.alloc(sizeof(mhip_stat_record) * (size_t)(c->nlabels + 1)));
        MH_HIP(hipMemcpyAsync(c->stats.p, c->raw_stats.p, sizeof(mhip_stat_record) * (size_t)(c->nlabels + 1),
                              hipMemcpyDeviceToDevice, s));
    }
    c->labels_filtered = true;
    c->stats_valid = true;
    c->hyps_total = -1;
    return MHIP_OK;
}

int mhip_ctx_stats(mhip_ctx *c, mhip_stat_record *records)
{
    MH_ARG(c && records && c->stats.p && c->labels_filtered, "ctx_stats needs LABEL + apply_keep");
    MH_HIP(hipMemcpyAsync(records, c->stats.p, sizeof(mhip_stat_record) * (size_t)(c->nlabels + 1), hipMemcpyDeviceToHost, c->stream));
    MH_HIP(stream_sync(c->stream));
    return MHIP_OK;
}

int mhip_ctx_watershed_counts(mhip_ctx *c, int64_t *counts)
{
    MH_ARG(c && counts && c->ws_counts.p, "ctx_watershed_counts needs a WATERSHED run");
    MH_HIP(hipMemcpyAsync(counts, c->ws_counts.p, 8 * (size_t)(c->nlabels + 1), hipMemcpyDeviceToHost, c->stream));
    MH_HIP(stream_sync(c->stream));
    return MHIP_OK;
}

int mhip_ctx_pourpoints(mhip_ctx *c, mhip_index_record *records)
{
    MH_ARG(c && records && c->pour.p, "ctx_pourpoints needs a POURPOINTS run");
    MH_HIP(hipMemcpyAsync(records, c->pour.p, sizeof(mhip_index_record) * (size_t)(c->nlabels + 1), hipMemcpyDeviceToHost, c->stream));
    MH_HIP(stream_sync(c->stream));
    return MHIP_OK;
}

/* ---- final state of the bluespots on the resident rasters (hyps.hip) ------------------------------------------------------ */
int mhip_ctx_hyps(mhip_ctx *c, double res, int64_t *total)
{
    MH_ARG(c && total && hyps_res_ok(res), "ctx_hyps(ctx, 0 < res < inf, total)");
    MH_ARG(!(c->nranks > 1 || c->ht || c->hb), "hypsometry on a row band is not built (the tables of the bands add up: a later step); use an undivided context");
    MH_ARG(c->have[MHIP_R_DEPTHS] && c->have[MHIP_R_LABELS] && !c->ccl_pending, "ctx_hyps needs the DEPTHS and LABELS rasters");
    MH_ARG(c->labels_filtered, "ctx_hyps needs mhip_ctx_apply_keep after the LABEL run");
    MH_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const int64_t n = c->H * c->W;
    c->hyps_total = -1;
    if (!c->stats_valid) {       // uploaded rasters: the labels' largest depths first
        MH_TRY(ctx_label_max(c, s));
        MH_TRY(c->stats.alloc(sizeof(mhip_stat_record) * (size_t)(c->nlabels + 1)));
        MH_TRY(label_stats_dev(c->r[MHIP_R_DEPTHS].as<float>(), c->r[MHIP_R_LABELS].as<int32_t>(), n, c->nlabels, c->stats.as<mhip_stat_record>(), s,
                               c->W, c->labels_components));
        c->stats_valid = true;
    }
    const int64_t nlab = c->nlabels;
    MH_TRY(c->hyps_off.alloc(8 * (size_t)(nlab + 2)));
    hipEvent_t *e1, *k0, *k1;
    MH_TRY(ctx_events(c, HYPS_KERNEL_SLOT, &k0, &k1));
    MH_TRY(stage_begin(c, MHIP_STAGE_HYPS, s, &e1));
    int64_t tot = 0;
    MH_TRY(hyps_layout_dev(c->stats.as<double>() + 1, 4, nlab, res, c->hyps_off.as<int64_t>(), &tot, s));     // (`max` of mhip_stat_record)
    MH_TRY(c->hyps_cnt.alloc(4 * (size_t)tot));
    MH_TRY(c->hyps_sum.alloc(8 * (size_t)tot));
    MH_TRY(hyps_table_dev(c->r[MHIP_R_DEPTHS].as<float>(), c->r[MHIP_R_LABELS].as<int32_t>(), n, c->W, nlab, res, c->hyps_off.as<int64_t>(), tot,
                          c->hyps_cnt.as<uint32_t>(), c->hyps_sum.as<double>(), &c->hyps_spills, s, *k0, *k1));
    MH_HIP(hipEventRecord(*e1, s));
    c->ev_valid[MHIP_STAGE_HYPS] = true;
    c->ev_valid[HYPS_KERNEL_SLOT] = true;
    c->hyps_total = tot;
    *total = tot;
    return MHIP_OK;
}

int mhip_ctx_hyps_fetch(mhip_ctx *c, int64_t *offsets, int64_t *counts, double *sums)
{
    MH_ARG(c && offsets && counts && sums, "ctx_hyps_fetch(ctx, offsets, counts, sums)");
    MH_ARG(c->hyps_total >= 0, "ctx_hyps_fetch needs mhip_ctx_hyps on the resident depths and labels");
    MH_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const size_t tot = (size_t)c->hyps_total;
    std::vector<uint32_t> c32(tot + 1);
    MH_HIP(hipMemcpyAsync(offsets, c->hyps_off.p, 8 * (size_t)(c->nlabels + 2), hipMemcpyDeviceToHost, s));
    if (tot) {
        MH_HIP(hipMemcpyAsync(c32.data(), c->hyps_cnt.p, 4 * tot, hipMemcpyDeviceToHost, s));
        MH_HIP(hipMemcpyAsync(sums, c->hyps_sum.p, 8 * tot, hipMemcpyDeviceToHost, s));
    }
    MH_HIP(stream_sync(s));
    for (size_t k = 0; k < tot; ++k) counts[k] = (int64_t)c32[k];
    return MHIP_OK;
}

int mhip_ctx_final_depths(mhip_ctx *c, const double *q, mhip_final_record *records)
{
    MH_ARG(c && q && records, "ctx_final_depths(ctx, q, records)");
    MH_ARG(c->hyps_total >= 0 && c->stats_valid, "ctx_final_depths needs mhip_ctx_hyps on the resident depths and labels");
    MH_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const int64_t nlab = c->nlabels, n = c->H * c->W;
    DevBuf d_q;
    MH_TRY(upload(d_q, q, 8 * (size_t)(nlab + 1), s));
    MH_TRY(c->hyps_rec.alloc(sizeof(mhip_final_record) * (size_t)(nlab + 1)));
    MH_TRY(ctx_raster(c, MHIP_R_FINALDEPTHS));
    c->have[MHIP_R_FINALDEPTHS] = false;
    hipEvent_t *e1, *k0, *k1;
    MH_TRY(ctx_events(c, FINAL_KERNEL_SLOT, &k0, &k1));
    MH_TRY(stage_begin(c, MHIP_STAGE_FINALDEPTHS, s, &e1));
    MH_TRY(hyps_levels_dev(nlab, c->hyps_off.as<int64_t>(), c->hyps_cnt.as<uint32_t>(), c->hyps_sum.as<double>(), c->stats.as<double>() + 1, 4,
                           d_q.as<double>(), c->hyps_rec.as<mhip_final_record>(), s));
    MH_TRY(final_depths_dev(c->r[MHIP_R_DEPTHS].as<float>(), c->r[MHIP_R_LABELS].as<int32_t>(), n, c->W, nlab, c->hyps_rec.as<mhip_final_record>(),
                            c->r[MHIP_R_FINALDEPTHS].as<float>(), s, *k0, *k1));      // (synchronises: d_q goes back to the pool)
    MH_HIP(hipEventRecord(*e1, s));
    c->ev_valid[MHIP_STAGE_FINALDEPTHS] = true;
    c->ev_valid[FINAL_KERNEL_SLOT] = true;
    c->have[MHIP_R_FINALDEPTHS] = true;
    MH_HIP(hipMemcpyAsync(records, c->hyps_rec.p, sizeof(mhip_final_record) * (size_t)(nlab + 1), hipMemcpyDeviceToHost, s));
    MH_HIP(stream_sync(s));
    return MHIP_OK;
}

}  // extern "C"
