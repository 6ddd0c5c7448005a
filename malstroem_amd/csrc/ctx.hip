// ctx.hip -- the device-resident context (ctx.hpp): create / destroy, the side-thread bracket, whole and windowed transfers, the
// getters, the per-label records, the label filter, hypsometry and final depths, the DEM adaptations, the outlines, the flow paths, and
// the held products -- wet_at, flow distance, travel time, hand, reach catchments and their flood depths, object zones, the sea flood --
// with their one record each, one lock and one drop (held_begin / held_commit / held_drop; what each is made from is
// held_rules.hpp).  The one rule for what a write of a resident raster invalidates (ctx_wrote) and the one test for a raster held
// outside mhip_raster (ctx_held, over the HELD table) are here.  The stages are ctx_run.hip, the row-band protocol ctx_band.hip.
#include <limits>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "ctx.hpp"

namespace mh {

static void drop_hyps(mhip_ctx *c)
{
    c->hyps_total = -1;
    c->have[MHIP_R_FINALDEPTHS] = false;
}

// ---- the held products (held_rules.hpp) ---------------------------------------------------------------------------------------------
// The one drop, with held_mu held: the product goes, its buffers go back to the pool (the call that filled them has synchronised:
// nothing on the device still uses them), and so does every product that was made from it
static void held_drop(mhip_ctx *c, int product)
{
    c->held[product].state = -1;
    for (DevBuf &b : c->held[product].buf) b.release();
    for (int p = 0; p < HP_COUNT_; ++p)
        if (held_goes_with(p) & held_bit(product)) held_drop(c, p);
    uint32_t live = 0;
    for (const mhip_ctx::Held &h : c->held)
        if (h.state >= 0) live |= h.made_from;
    c->held_mask = live;
}

// a making call begins: what its last call left goes, and what was made from that; the call fills the buffers of the record ...
static mhip_ctx::Held &held_begin(mhip_ctx *c, int product)
{
    std::lock_guard<std::mutex> lk(c->held_mu);
    held_drop(c, product);
    return c->held[product];
}

// ... and has succeeded: `state` (>= 0) is what mhip_ctx_get_i64 reports, `variant` what the rule of the product looks at
static void held_commit(mhip_ctx *c, int product, int64_t state, int variant = 0)
{
    std::lock_guard<std::mutex> lk(c->held_mu);
    c->held[product].made_from = held_made_from(product, variant);
    c->held[product].state = state;
    c->held_mask |= c->held[product].made_from;
}

void ctx_wrote(mhip_ctx *c, int which, bool uploaded)
{
    // (with no product held that was made from `which` no lock is taken: all the stages' writes see of this)
    if (const uint32_t w = held_write_mask(which); w & c->held_mask) {
        std::lock_guard<std::mutex> lk(c->held_mu);
        for (int p = 0; p < HP_COUNT_; ++p)
            if (c->held[p].state >= 0 && (c->held[p].made_from & w)) held_drop(c, p);
    }
    switch (which) {
    case MHIP_R_DEM:    // a new DEM invalidates everything derived from the previous one
        c->noflat_pending = false;      // (a surface nobody has asked for goes with have[NOFLAT])
        for (int k = 0; k < MHIP_R_COUNT_; ++k) {
            if (k == MHIP_R_DEM) continue;
            c->have[k] = false;
            ctx_wrote(c, k, true);
        }
        break;
    case MHIP_R_FILLED:
        if (uploaded) c->fill_st.have_minmax = false;      // (no flood of this context saw its DEM; the context's own fill sets the extremes)
        break;
    case MHIP_R_DEPTHS:
        c->stats_valid = false;
        c->raw_stats_valid = false;      // (the labelling's statistics describe the depths it read)
        drop_hyps(c);
        break;
    case MHIP_R_NOFLAT:
        c->pour_valid = false;
        break;
    case MHIP_R_FLOWDIR:
        c->nodir_valid = false;
        c->flowdir_own = false;
        c->acc_keep.valid = false;
        break;
    case MHIP_R_ACCUM:
        c->acc_keep.valid = false;
        c->pour_valid = false;
        break;
    case MHIP_R_LABELS:
        c->nlabels = c->nlabels_raw = -1;
        c->labels_components = false;
        c->stats_valid = false;
        c->raw_stats_valid = false;
        c->ws_counts_valid = false;
        c->pour_valid = false;
        drop_hyps(c);
        break;
    case MHIP_R_WATERSHEDS:
        c->ws_counts_valid = false;
        break;
    default:
        break;
    }
}

int ctx_copy_rows(mhip_ctx *c, void *dev_base, size_t elem_bytes, int64_t row0, int64_t nrows, void *host, hipMemcpyKind kind)
{
    MH_HIP(hipSetDevice(c->device));
    const size_t rowb = elem_bytes * (size_t)c->W;
    char *dev = (char *)dev_base + rowb * (size_t)(c->ht + row0);
    const bool up = kind == hipMemcpyHostToDevice;
    MH_HIP(hipMemcpyAsync(up ? (void *)dev : host, up ? host : (void *)dev, rowb * (size_t)nrows, kind, cs(c)));
    MH_HIP(stream_sync(cs(c)));      // (an upload's caller reuses its window buffer)
    return MHIP_OK;
}

// every raster held outside mhip_raster, in the order of HeldRaster: its product and which of the product's buffers it is (0: the
// raster, 1: a second raster or the records, 2: the table); the key of mhip_ctx_get_i64 that reports the product's state (once per
// product); what mhip_ctx_zone_stats / mhip_ctx_polygonize call it as a source (-1: no source of that call); the message of its getter
static const struct HeldRow { int product, buf; const char *key; int zsrc, psrc; const char *needs; } HELD[HELD_COUNT_] = {
    {HP_WETAT, 0, "wet_at_events", MHIP_ZSRC_WETAT, -1, "ctx_wet_at_rows needs mhip_ctx_wet_at on the resident depths and labels"},
    {HP_FLOWDIST, 0, "flow_distance_unresolved", MHIP_ZSRC_FLOWDIST, -1, "ctx_flow_distance_rows needs mhip_ctx_flow_distance on the resident flow directions and labels"},
    {HP_HAND, 0, "hand_undrained", MHIP_ZSRC_HAND, -1, "ctx_hand_rows needs mhip_ctx_hand on the resident rasters"},
    {HP_HAND, 1, nullptr, MHIP_ZSRC_DRAINDIST, -1, "ctx_hand_rows needs mhip_ctx_hand on the resident rasters"},
    {HP_REACHCATCH, 0, "reach_catchments", -1, MHIP_PSRC_REACHCATCH, "ctx_reach_catchments_rows needs mhip_ctx_reach_catchments on the resident rasters"},
    {HP_INUNDATION, 0, "inundation", MHIP_ZSRC_INUNDATION, -1, "ctx_inundation_rows needs mhip_ctx_inundate on the held hand and reach catchments"},
    {HP_ZONES, 0, "zones", -1, -1, "ctx_zones_rows needs mhip_ctx_rasterize_zones"},
    {HP_TRAVELTIME, 0, "travel_time_unresolved", MHIP_ZSRC_TRAVELTIME, -1, "ctx_travel_time_rows needs mhip_ctx_travel_time on the resident rasters"},
    {HP_SEALEVEL, 0, "sea_flood", MHIP_ZSRC_SEALEVEL, -1, "ctx_sea_flood_rows needs mhip_ctx_sea_flood on the resident DEM"},
    {HP_SEADEPTH, 0, "sea_depths", MHIP_ZSRC_SEADEPTH, -1, "ctx_sea_flood_rows needs mhip_ctx_sea_depths on the held sea levels"},
    {HP_SEACLASS, 0, "sea_classes", -1, MHIP_PSRC_SEACLASSES, "ctx_sea_classes_rows needs mhip_ctx_sea_classes on the held sea levels"},
};

static int held_source(int HeldRow::*column, int source)      // the raster that zone_stats (zsrc) / polygonize (psrc) calls `source`, or -1
{
    for (int id = 0; id < HELD_COUNT_; ++id)
        if (source >= 0 && HELD[id].*column == source) return id;
    return -1;
}

int ctx_held(mhip_ctx *c, int id, void **ptr, size_t *elem_bytes)
{
    const mhip_ctx::Held &h = c->held[HELD[id].product];
    MH_ARG(h.state >= 0 && h.buf[HELD[id].buf].p, HELD[id].needs);
    *ptr = h.buf[HELD[id].buf].p;
    if (elem_bytes) *elem_bytes = 4;      // (float32 or int32, every one)
    return MHIP_OK;
}

// every mhip_ctx_*_rows getter of a held raster: the window check (`sig` names the call), the validity test, the copy
static int held_rows(mhip_ctx *c, int id, int64_t row0, int64_t nrows, void *dst, const char *sig)
{
    MH_ARG(c && dst && id >= 0 && row0 >= 0 && nrows >= 1 && row0 + nrows <= c->H_owned, sig);
    void *p = nullptr;
    size_t eb = 0;
    MH_TRY(ctx_held(c, id, &p, &eb));
    return ctx_copy_rows(c, p, eb, row0, nrows, dst, hipMemcpyDeviceToHost);
}

int ctx_noflat(mhip_ctx *c, double **g)
{
    if (c->noflat_pending) {
        MH_HIP(hipSetDevice(c->device));
        // (no cell of an accepted surface takes the seed: the finishing pass counted none)
        MH_TRY(noflat_assemble_dev(c->r[MHIP_R_FILLED].as<float>(), c->r[MHIP_R_NGDIST].as<uint32_t>(), c->r[MHIP_R_NOFLAT].as<double>(), c->H * c->W, 0.0,
                                   c->stream));
        c->noflat_pending = false;
        if (cs(c) != c->stream) MH_HIP(stream_sync(c->stream));
    }
    if (g) *g = c->r[MHIP_R_NOFLAT].as<double>();
    return MHIP_OK;
}

int ctx_fetch(mhip_ctx *c, const DevBuf &buf, size_t bytes, void *host)
{
    MH_HIP(hipSetDevice(c->device));
    return download(host, buf, bytes, c->stream);
}

int ctx_fork_join_events(mhip_ctx *c)
{
    if (c->ev_fork) return MHIP_OK;
    for (hipEvent_t *e : {&c->ev_flowdir, &c->ev_join, &c->ev_label, &c->ev_tail, &c->ev_fork}) MH_HIP(hipEventCreateWithFlags(e, hipEventDisableTiming));
    return MHIP_OK;
}

int ctx_ensure_labels_final(mhip_ctx *c, hipStream_t s)
{
    if (!c->labels_filtered) return ctx_apply_keep_on(c, nullptr, s);
    return MHIP_OK;
}

int ctx_label_max(mhip_ctx *c, hipStream_t s)
{
    if (c->nlabels < 0) {
        int32_t m = 0;
        MH_TRY(label_max_dev(c->r[MHIP_R_LABELS].as<int32_t>(), c->H * c->W, &m, s));
        c->nlabels = m < 0 ? 0 : m;
    }
    return MHIP_OK;
}

int ctx_apply_keep_on(mhip_ctx *c, const uint8_t *keep, hipStream_t s)
{
    MH_ARG(c && c->have[MHIP_R_LABELS] && c->nlabels_raw >= 0 && !c->labels_filtered, "ctx_apply_keep needs a fresh LABEL run");
    // (a filter's statistics are a pass over the depths: a raster whose last window has not arrived is none; refused with the labels as they were)
    MH_ARG(!keep || c->have[MHIP_R_DEPTHS], "ctx_apply_keep with a filter needs the DEPTHS raster");
    const int64_t n = c->H * c->W;
    // a write of LABELS that renumbers them: the raw count stays known, kept components stay components, and the raw statistics
    // still describe the resident depths if they did
    const int64_t nraw = c->nlabels_raw;
    const bool components = c->labels_components;
    const bool raw_valid = c->raw_stats_valid;
    ctx_wrote(c, MHIP_R_LABELS);
    c->nlabels_raw = nraw;
    c->labels_components = components;
    c->raw_stats_valid = raw_valid;
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
        c->labels_filtered = true;
        c->stats_valid = true;
        return MHIP_OK;
    }
    // keep everything (background excluded by construction): the labels are the raw ones, and so are the statistics while the depths
    // are the ones the labelling read (the chain: a copy, no kernel).  Depths written since: a pass over the resident ones; none
    // resident: the labels are final without statistics, and mhip_ctx_hyps computes them when it finds depths
    c->nlabels = c->nlabels_raw;
    c->labels_filtered = true;
    if (!raw_valid && !c->have[MHIP_R_DEPTHS]) return MHIP_OK;
    MH_TRY(c->stats.alloc(sizeof(mhip_stat_record) * (size_t)(c->nlabels + 1)));
    if (raw_valid)
        MH_HIP(hipMemcpyAsync(c->stats.p, c->raw_stats.p, sizeof(mhip_stat_record) * (size_t)(c->nlabels + 1), hipMemcpyDeviceToDevice, s));
    else
        MH_TRY(label_stats_dev(c->r[MHIP_R_DEPTHS].as<float>(), c->r[MHIP_R_LABELS].as<int32_t>(), n, c->nlabels, c->stats.as<mhip_stat_record>(), s,
                               c->W, c->labels_components));
    c->stats_valid = true;
    return MHIP_OK;
}

}  // namespace mh

using namespace mh;

extern "C" {

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
    for (StageTimer &t : c->timers)
        for (hipEvent_t e : {t.a, t.b})
            if (e) (void)hipEventDestroy(e);
    (void)hipStreamDestroy(c->stream);
    for (hipStream_t st : {c->stream_b, c->stream_c}) {
        if (st) {
            (void)stream_sync(st);
            (void)hipStreamDestroy(st);
        }
    }
    for (hipEvent_t e : {c->ev_fork, c->ev_flowdir, c->ev_join, c->ev_label, c->ev_tail, c->ev_cand, c->ev_prep})
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
    MH_TRY(ctx_fork_join_events(c));
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
    return mhip_ctx_upload_rows(c, which, 0, c->H_owned, host);
}

int mhip_ctx_upload_dem(mhip_ctx *c, const float *dem) { return mhip_ctx_upload(c, MHIP_R_DEM, dem); }

/* Windowed transfers (reference io.py:21-159 moves whole rasters through the host): rows [row0, row0 + nrows) of the OWNED
 * raster.  Every window is a write of the raster (ctx_wrote, as mhip_ctx_upload); the raster counts as absent from the first
 * window on and as present once its last row has been uploaded.  The host side needs one window, whatever the raster's size. */
int mhip_ctx_upload_rows(mhip_ctx *c, int which, int64_t row0, int64_t nrows, const void *host)
{
    MH_ARG(c && host && which >= 0 && which < MHIP_R_COUNT_ && row0 >= 0 && nrows >= 1 && row0 + nrows <= c->H_owned,
           "ctx_upload_rows(ctx, which, row0, nrows, host)");
    MH_HIP(hipSetDevice(c->device));
    MH_TRY(ctx_raster(c, which));
    MH_TRY(ctx_settle(c, which, /*write=*/true));     // (a foreign FILLED leaves the surface of the old one behind, as ever)
    ctx_wrote(c, which, /*uploaded=*/true);
    c->have[which] = false;
    MH_TRY(ctx_copy_rows(c, c->r[which].p, raster_elem(which), row0, nrows, const_cast<void *>(host), hipMemcpyHostToDevice));
    if (row0 + nrows == c->H_owned) {
        c->have[which] = true;
        if (which == MHIP_R_LABELS) c->labels_filtered = true;      // (uploaded labels are final: their count is max(labels), taken when asked for)
    }
    return MHIP_OK;
}

int mhip_ctx_download_rows(mhip_ctx *c, int which, int64_t row0, int64_t nrows, void *host)
{
    MH_ARG(c && host && which >= 0 && which < MHIP_R_COUNT_ && row0 >= 0 && nrows >= 1 && row0 + nrows <= c->H_owned,
           "ctx_download_rows(ctx, which, row0, nrows, host)");
    MH_ARG(c->have[which], "raster has not been computed or uploaded");
    MH_TRY(ctx_settle(c, which, /*write=*/false));
    return ctx_copy_rows(c, c->r[which].p, raster_elem(which), row0, nrows, host, hipMemcpyDeviceToHost);
}

int mhip_ctx_download(mhip_ctx *c, int which, void *host)
{
    MH_ARG(c && host && which >= 0 && which < MHIP_R_COUNT_, "ctx_download(ctx, which, host)");
    return mhip_ctx_download_rows(c, which, 0, c->H_owned, host);
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

int mhip_ctx_stage_ms(mhip_ctx *c, int stage, float *ms)
{
    MH_ARG(c && ms, "ctx_stage_ms(ctx, stage, ms)");
    const int k = timer_slot(stage);
    MH_ARG(k >= 0 && c->timers[k].valid, "stage has not been run");
    MH_HIP(hipEventSynchronize(c->timers[k].b));
    MH_HIP(hipEventElapsedTime(ms, c->timers[k].a, c->timers[k].b));
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
        double *g = nullptr;
        MH_TRY(ctx_noflat(c, &g));      // (in front of the events: the launches below are the stencil and nothing else)
        MH_TRY(ctx_raster(c, MHIP_R_FLOWDIR));
        MH_TRY(c->nodir_cnt.alloc(4));
        constexpr int REPS = 16;
        StageTimer *t;
        MH_TRY(ctx_timer(c, D8_STEADY_SLOT, &t));
        hipStream_t s = c->stream;
        ctx_wrote(c, MHIP_R_FLOWDIR);
        MH_HIP(hipMemsetAsync(c->nodir_cnt.p, 0, 4, s));
        for (int i = 0; i < REPS + 2; ++i) {
            if (i == 2) MH_HIP(hipEventRecord(t->a, s));      // (two untimed launches first)
            MH_TRY(d8_dev(g, c->r[MHIP_R_FLOWDIR].as<uint8_t>(), c->H, c->W, 1, s, 0, c->H_global, c->nodir_cnt.as<unsigned int>()));
        }
        MH_HIP(hipEventRecord(t->b, s));
        MH_HIP(hipEventSynchronize(t->b));
        MH_HIP(hipEventElapsedTime(ms_total, t->a, t->b));
        c->have[MHIP_R_FLOWDIR] = true;
        c->nodir_valid = true;
        c->flowdir_own = true;
        *launches = REPS;
        return MHIP_OK;
    }
    if (k == "hyps_table" || k == "final_depths") {      // events around the one kernel inside mhip_ctx_hyps / mhip_ctx_final_depths
        *launches = 1;
        return mhip_ctx_stage_ms(c, k == "hyps_table" ? HYPS_KERNEL_SLOT : FINAL_KERNEL_SLOT, ms_total);
    }
    if (k == "wet_at") {      // ... and around the raster pass of the last mhip_ctx_wet_at
        *launches = 1;
        return mhip_ctx_stage_ms(c, WETAT_KERNEL_SLOT, ms_total);
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
    else if (k == "fill_handover") *value = c->fill_handover;       // 1 the last request wrote FILLED / DEPTHS in the no-flats fill's first visit (ng_handover_kernel)
    else if (k == "wetbits_used") *value = (c->wet_pass_used ? 1 : 0) | (c->wet_label_used ? 2 : 0);         // bit 0: ng_finish_kernel, bit 1: ccl_tile_kernel took the wet bits of the last request's hand-over (ctx_run.hip)
    else if (k == "fill_handover_rechecks") *value = c->fill_handover_rechecks;   // diagnostics: see ctx.hpp
    else if (k == "fill_overflow") *value = c->fill_st.overflow;     // the flood's capacities that gave out (0: it ran through / was not tried)
    else if (k == "fill_launches") *value = c->fill_st.rounds;
    else if (k == "fill_hot_launches") *value = c->fill_st.hot_launches;
    else if (k == "noflat_hot_launches") *value = c->noflat_st.hot_launches;
    else if (k == "accum_algorithm") *value = c->accum_algorithm;   // 0 full accumulation, 1 a row band's second pass as a delta over the boundary pass's graph
    else if (k == "flowdir_computed") *value = (c->have[MHIP_R_FLOWDIR] && c->flowdir_own) ? 1 : 0;   // 1 the library's D8 wrote FLOWDIR, 0 it was uploaded
    else if (k == "pour_algorithm") *value = c->pour_algorithm;   // 0 a pass over values + labels (label_ops.hip), 1 keys out of the accumulation's final pass (PourLink)
    else if (k == "noflat_algorithm") *value = c->noflat_st.algorithm;   // 0 float64 relaxation (fill.hip), 2 integer geodesic transform (noflat_geo.hip)
    else if (k == "noflat_pending") *value = c->noflat_pending ? 1 : 0;   // 1 NOFLAT is resident but not written yet: the next reader's call writes it (ctx_noflat)
    else if (k == "noflat_visits") *value = c->noflat_st.visits;
    else if (k == "noflat_reject") *value = c->noflat_st.geo_reject;            // diagnostics: FillStats::geo_reject and its counts
    else if (k == "noflat_reject_irregular") *value = c->noflat_st.geo_irregular;
    else if (k == "noflat_reject_unreached") *value = c->noflat_st.geo_unreached;
    else if (k == "noflat_reject_mismatch") *value = c->noflat_st.geo_mismatch;
    else if (k == "noflat_cycles") *value = c->noflat_st.cycles;
    else if (k == "noflat_rowstore") *value = c->noflat_st.rowstore;        // what the last request's rounds stored per visit (noflat_geo.hip: MHIP_NG_ROWSTORE)
    else if (k == "noflat_rows_stored") *value = c->noflat_st.rows_stored;  // ... and the rows of distances that came to
    else if (k == "hyps_bins") *value = c->hyps_total;               // -1: no table (mhip_ctx_hyps)
    else if (k == "hyps_lds_spills") *value = c->hyps_spills;        // runs that found no slot in their tile's LDS table
    else if (k == "travel_time_saturated") *value = c->held[HP_TRAVELTIME].state >= 0 ? c->tt_saturated : -1;   // the cells whose cost was clipped to the cap
    else if (k == "travel_time_bins") *value = c->held[HP_TRAVELTIME].state >= 0 ? c->tt_bins : -1;             // the bins of the table held, 0: no table
    else if (k == "seaflood_rounds") *value = c->sea_st.rounds;      // of the last mhip_ctx_sea_flood: launches that found work,
    else if (k == "seaflood_visits") *value = c->sea_st.visits;      // ... tile visits,
    else if (k == "seaflood_rechecks") *value = c->sea_st.rechecks;  // ... tiles its proof sent back (0 unless something is broken)
    else if (k == "H") *value = c->H;
    else if (k == "W") *value = c->W;
    else {      // the state of a held product (HELD: key), -1: none
        for (const HeldRow &row : HELD)
            if (row.key && k == row.key) {
                *value = c->held[row.product].state;
                return MHIP_OK;
            }
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
    MH_ARG(c && records && c->raw_stats.p && c->nlabels_raw >= 0 && c->raw_stats_valid, "ctx_raw_stats needs a LABEL run on the resident depths");
    return ctx_fetch(c, c->raw_stats, sizeof(mhip_stat_record) * (size_t)(c->nlabels_raw + 1), records);
}

int mhip_ctx_apply_keep(mhip_ctx *c, const uint8_t *keep)
{
    MH_ARG(c, "ctx");
    MH_HIP(hipSetDevice(c->device));
    return ctx_apply_keep_on(c, keep, c->stream);
}

int mhip_ctx_stats(mhip_ctx *c, mhip_stat_record *records)
{
    MH_ARG(c && records && c->stats_valid && c->labels_filtered, "ctx_stats needs LABEL + apply_keep (or mhip_ctx_hyps) on the resident depths and labels");
    return ctx_fetch(c, c->stats, sizeof(mhip_stat_record) * (size_t)(c->nlabels + 1), records);
}

int mhip_ctx_watershed_counts(mhip_ctx *c, int64_t *counts)
{
    MH_ARG(c && counts && c->ws_counts_valid, "ctx_watershed_counts needs a WATERSHED run on the resident labels");
    return ctx_fetch(c, c->ws_counts, 8 * (size_t)(c->nlabels + 1), counts);
}

int mhip_ctx_pourpoints(mhip_ctx *c, mhip_index_record *records)
{
    MH_ARG(c && records && c->pour_valid, "ctx_pourpoints needs a POURPOINTS run on the resident labels and accumulated flow");
    return ctx_fetch(c, c->pour, sizeof(mhip_index_record) * (size_t)(c->nlabels + 1), records);
}

/* ---- final state of the bluespots on the resident rasters (hyps.hip) ------------------------------------------------------ */
int mhip_ctx_hyps(mhip_ctx *c, double res, int64_t *total)
{
    MH_ARG(c && total && hyps_res_ok(res), "ctx_hyps(ctx, 0 < res < inf, total)");
    MH_ARG(undivided(c), "hypsometry on a row band is not built (the tables of the bands add up: a later step); use an undivided context");
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
    StageTimer *k;
    MH_TRY(ctx_timer(c, HYPS_KERNEL_SLOT, &k));
    MH_TRY(stage_begin(c, MHIP_STAGE_HYPS, s));
    int64_t tot = 0;
    MH_TRY(hyps_layout_dev(c->stats.as<double>() + 1, 4, nlab, res, c->hyps_off.as<int64_t>(), &tot, s));     // (`max` of mhip_stat_record)
    MH_TRY(c->hyps_cnt.alloc(4 * (size_t)tot));
    MH_TRY(c->hyps_sum.alloc(8 * (size_t)tot));
    MH_TRY(hyps_table_dev(c->r[MHIP_R_DEPTHS].as<float>(), c->r[MHIP_R_LABELS].as<int32_t>(), n, c->W, nlab, res, c->hyps_off.as<int64_t>(), tot,
                          c->hyps_cnt.as<uint32_t>(), c->hyps_sum.as<double>(), &c->hyps_spills, s, k->a, k->b));
    MH_TRY(stage_end(c, MHIP_STAGE_HYPS, s));
    k->valid = true;
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
    StageTimer *k;
    MH_TRY(ctx_timer(c, FINAL_KERNEL_SLOT, &k));
    MH_TRY(stage_begin(c, MHIP_STAGE_FINALDEPTHS, s));
    MH_TRY(hyps_levels_dev(nlab, c->hyps_off.as<int64_t>(), c->hyps_cnt.as<uint32_t>(), c->hyps_sum.as<double>(), c->stats.as<double>() + 1, 4,
                           d_q.as<double>(), c->hyps_rec.as<mhip_final_record>(), s));
    MH_TRY(final_depths_dev(c->r[MHIP_R_DEPTHS].as<float>(), c->r[MHIP_R_LABELS].as<int32_t>(), n, c->W, nlab, c->hyps_rec.as<mhip_final_record>(),
                            c->r[MHIP_R_FINALDEPTHS].as<float>(), s, k->a, k->b));      // (synchronises: d_q goes back to the pool)
    MH_TRY(stage_end(c, MHIP_STAGE_FINALDEPTHS, s));
    k->valid = true;
    c->have[MHIP_R_FINALDEPTHS] = true;
    return ctx_fetch(c, c->hyps_rec, sizeof(mhip_final_record) * (size_t)(nlab + 1), records);
}

/* ---- the rain at which every cell gets wet (wetat.hip): K levels, one pass over the resident rasters ------------------------- */
int mhip_ctx_wet_at(mhip_ctx *c, int32_t K, const double *q, const float *values, mhip_final_record *records)
{
    MH_ARG(c && q && values && records, "ctx_wet_at(ctx, K, q, values, records)");
    MH_ARG(wet_at_events_ok(K, values), "ctx_wet_at: 1 to 16 events whose values are finite, > 0 and strictly increasing");
    MH_ARG(undivided(c), "wet_at on a row band is not built (it needs the bands' hypsometry tables: a later step); use an undivided context");
    MH_ARG(c->hyps_total >= 0 && c->stats_valid, "ctx_wet_at needs mhip_ctx_hyps on the resident depths and labels");
    MH_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const int64_t nlab = c->nlabels, n = c->H * c->W;
    const size_t nt = (size_t)K * (size_t)(nlab + 1);
    DevBuf d_q, d_rec;
    MH_TRY(upload(d_q, q, 8 * nt, s));
    MH_TRY(d_rec.alloc(sizeof(mhip_final_record) * nt));
    DevBuf &out = held_begin(c, HP_WETAT).buf[0];
    MH_TRY(out.alloc(4 * (size_t)n));
    StageTimer *k;
    MH_TRY(ctx_timer(c, WETAT_KERNEL_SLOT, &k));
    for (int32_t e = 0; e < K; ++e)
        MH_TRY(hyps_levels_dev(nlab, c->hyps_off.as<int64_t>(), c->hyps_cnt.as<uint32_t>(), c->hyps_sum.as<double>(), c->stats.as<double>() + 1, 4,
                               d_q.as<double>() + (size_t)e * (size_t)(nlab + 1), d_rec.as<mhip_final_record>() + (size_t)e * (size_t)(nlab + 1), s));
    // the draw-downs out of the records' first field, the wet cells into their last (the levels left 0 there)
    MH_TRY(wet_at_dev(c->r[MHIP_R_DEPTHS].as<float>(), c->r[MHIP_R_LABELS].as<int32_t>(), n, c->W, nlab, K, d_rec.as<double>(), 4, values,
                      out.as<float>(), d_rec.as<int64_t>() + 3, 4, s, k->a, k->b));      // (synchronises)
    k->valid = true;
    held_commit(c, HP_WETAT, K);
    return ctx_fetch(c, d_rec, sizeof(mhip_final_record) * nt, records);
}

int mhip_ctx_wet_at_rows(mhip_ctx *c, int64_t row0, int64_t nrows, float *dst)
{
    return held_rows(c, HELD_WETAT, row0, nrows, dst, "ctx_wet_at_rows(ctx, row0, nrows, dst)");
}

/* ---- flow distance to the receiving bluespot, longest flow path per watershed (flowdist.hip) ------------------------------------ */
int mhip_ctx_flow_distance(mhip_ctx *c, double scale, int64_t *unresolved)
{
    MH_ARG(c && unresolved, "ctx_flow_distance(ctx, scale, unresolved)");
    MH_ARG(flow_distance_scale_ok(scale), "ctx_flow_distance: the scale must be finite and > 0");
    MH_ARG(undivided(c), "flow distance on a row band is not built (a path crosses the seams: a later step); use an undivided context");
    MH_ARG(c->have[MHIP_R_FLOWDIR] && c->have[MHIP_R_LABELS] && !c->ccl_pending, "ctx_flow_distance needs the FLOWDIR and LABELS rasters");
    MH_ARG(c->labels_filtered, "ctx_flow_distance needs mhip_ctx_apply_keep after the LABEL run");
    MH_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    MH_TRY(ctx_label_max(c, s));
    const int64_t nlab = c->nlabels, n = c->H * c->W;
    mhip_ctx::Held &h = held_begin(c, HP_FLOWDIST);
    DevBuf &out = h.buf[0], &rec = h.buf[1];
    MH_TRY(out.alloc(4 * (size_t)n));
    MH_TRY(rec.alloc(sizeof(mhip_index_record) * (size_t)(nlab + 1)));
    int64_t u = 0;
    MH_TRY(flow_distance_dev(c->r[MHIP_R_FLOWDIR].as<uint8_t>(), c->r[MHIP_R_LABELS].as<int32_t>(), c->H, c->W, scale, nlab, out.as<float>(),
                             rec.as<mhip_index_record>(), &u, s));      // (synchronises)
    held_commit(c, HP_FLOWDIST, u);
    *unresolved = u;
    return MHIP_OK;
}

int mhip_ctx_flow_distance_rows(mhip_ctx *c, int64_t row0, int64_t nrows, float *dst)
{
    return held_rows(c, HELD_FLOWDIST, row0, nrows, dst, "ctx_flow_distance_rows(ctx, row0, nrows, dst)");
}

int mhip_ctx_flow_distance_records(mhip_ctx *c, mhip_index_record *records)
{
    MH_ARG(c && records, "ctx_flow_distance_records(ctx, records)");
    const mhip_ctx::Held &h = c->held[HP_FLOWDIST];
    MH_ARG(h.state >= 0 && h.buf[1].p, "ctx_flow_distance_records needs mhip_ctx_flow_distance on the resident flow directions and labels");
    return ctx_fetch(c, h.buf[1], sizeof(mhip_index_record) * (size_t)(c->nlabels + 1), records);
}

/* ---- travel time to the receiving bluespot, time of concentration and time-area table per watershed (traveltime.hip) ------------- */
int mhip_ctx_travel_time(mhip_ctx *c, double cellsize, const mhip_traveltime_params *params, int64_t nbins, uint64_t bin_ticks, int64_t *unresolved)
{
    MH_ARG(c && unresolved, "ctx_travel_time(ctx, cellsize, params, nbins, bin_ticks, unresolved)");
    MH_TRY(travel_time_check(cellsize, params));
    MH_TRY(travel_time_walk_check(params->tick, nbins, bin_ticks, nbins != 0));
    MH_ARG(undivided(c), "travel time on a row band is not built (a path crosses the seams: a later step); use an undivided context");
    MH_ARG(c->have[MHIP_R_FLOWDIR] && c->have[MHIP_R_LABELS] && !c->ccl_pending, "ctx_travel_time needs the FLOWDIR and LABELS rasters");
    MH_ARG(c->have[MHIP_R_FILLED], "ctx_travel_time needs the FILLED raster");
    const bool classes = params->channel_threshold <= 1.7976931348623157e308;      // (finite: two classes are live)
    MH_ARG(!classes || c->have[MHIP_R_ACCUM], "ctx_travel_time with a finite channel_threshold needs the ACCUM raster");
    MH_ARG(c->labels_filtered, "ctx_travel_time needs mhip_ctx_apply_keep after the LABEL run");
    MH_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    MH_TRY(ctx_label_max(c, s));
    const int64_t nlab = c->nlabels, n = c->H * c->W;
    mhip_ctx::Held &h = held_begin(c, HP_TRAVELTIME);
    DevBuf &out = h.buf[0], &rec = h.buf[1], &hist = h.buf[2];
    DevBuf cost;      // (scratch of this call)
    MH_TRY(cost.alloc(4 * (size_t)n));
    int64_t sat = 0, u = 0;
    MH_TRY(step_cost_dev(c->r[MHIP_R_FLOWDIR].as<uint8_t>(), c->r[MHIP_R_FILLED].as<float>(), classes ? c->r[MHIP_R_ACCUM].as<double>() : nullptr, c->H, c->W,
                         cellsize, *params, cost.as<uint32_t>(), &sat, s));
    MH_TRY(out.alloc(4 * (size_t)n));
    MH_TRY(rec.alloc(sizeof(mhip_index_record) * (size_t)(nlab + 1)));
    if (nbins) MH_TRY(hist.alloc(4 * (size_t)(nlab + 1) * (size_t)nbins));
    MH_TRY(flow_cost_distance_dev(c->r[MHIP_R_FLOWDIR].as<uint8_t>(), c->r[MHIP_R_LABELS].as<int32_t>(), cost.as<uint32_t>(), c->H, c->W, params->tick, nlab,
                                  out.as<float>(), rec.as<mhip_index_record>(), nbins, bin_ticks, nbins ? hist.as<uint32_t>() : nullptr, &u, s));      // (synchronises)
    c->tt_saturated = sat;
    c->tt_bins = nbins;
    held_commit(c, HP_TRAVELTIME, u);
    *unresolved = u;
    return MHIP_OK;
}

int mhip_ctx_travel_time_rows(mhip_ctx *c, int64_t row0, int64_t nrows, float *dst)
{
    return held_rows(c, HELD_TRAVELTIME, row0, nrows, dst, "ctx_travel_time_rows(ctx, row0, nrows, dst)");
}

int mhip_ctx_travel_time_records(mhip_ctx *c, mhip_index_record *records)
{
    MH_ARG(c && records, "ctx_travel_time_records(ctx, records)");
    const mhip_ctx::Held &h = c->held[HP_TRAVELTIME];
    MH_ARG(h.state >= 0 && h.buf[1].p, "ctx_travel_time_records needs mhip_ctx_travel_time on the resident rasters");
    return ctx_fetch(c, h.buf[1], sizeof(mhip_index_record) * (size_t)(c->nlabels + 1), records);
}

int mhip_ctx_travel_time_hist(mhip_ctx *c, int64_t nbins, uint32_t *hist)
{
    MH_ARG(c && hist, "ctx_travel_time_hist(ctx, nbins, hist)");
    const mhip_ctx::Held &h = c->held[HP_TRAVELTIME];
    MH_ARG(h.state >= 0 && c->tt_bins > 0 && h.buf[2].p, "ctx_travel_time_hist needs mhip_ctx_travel_time with a table on the resident rasters");
    MH_ARG(nbins == c->tt_bins, "ctx_travel_time_hist: nbins is not the held table's");
    return ctx_fetch(c, h.buf[2], 4 * (size_t)(c->nlabels + 1) * (size_t)nbins, hist);
}

/* ---- height above the nearest drainage and the distance to it (hand.hip) ---------------------------------------------------------- */
int mhip_ctx_hand(mhip_ctx *c, int32_t elev_source, double threshold, int32_t stop_at_labels, double scale, float nodata, int64_t *undrained)
{
    MH_ARG(c && undrained, "ctx_hand(ctx, elev_source, threshold, stop_at_labels, scale, nodata, undrained)");
    MH_ARG(elev_source == MHIP_R_FILLED || elev_source == MHIP_R_DEM, "ctx_hand: the elevation source is MHIP_R_FILLED or MHIP_R_DEM");
    MH_TRY(hand_check(threshold, scale));
    MH_ARG(undivided(c), "hand on a row band is not built (a path crosses the seams: a later step); use an undivided context");
    MH_ARG(c->have[MHIP_R_FLOWDIR] && c->have[MHIP_R_ACCUM] && c->have[elev_source], "ctx_hand needs the FLOWDIR and ACCUM rasters and the elevation source");
    if (stop_at_labels) {
        MH_ARG(c->have[MHIP_R_LABELS] && !c->ccl_pending, "ctx_hand with stop_at_labels needs the LABELS raster");
        MH_ARG(c->labels_filtered, "ctx_hand needs mhip_ctx_apply_keep after the LABEL run");
    }
    MH_HIP(hipSetDevice(c->device));
    const int64_t n = c->H * c->W;
    mhip_ctx::Held &h = held_begin(c, HP_HAND);
    DevBuf &out = h.buf[0], &dist = h.buf[1];      // (made and dropped together: one is there, both are)
    MH_TRY(out.alloc(4 * (size_t)n));
    MH_TRY(dist.alloc(4 * (size_t)n));
    int64_t u = 0;
    MH_TRY(hand_dev(c->r[MHIP_R_FLOWDIR].as<uint8_t>(), c->r[MHIP_R_ACCUM].as<double>(), c->r[elev_source].as<float>(),
                    stop_at_labels ? c->r[MHIP_R_LABELS].as<int32_t>() : nullptr, c->H, c->W, threshold, scale, nodata, out.as<float>(), dist.as<float>(), &u,
                    c->stream));      // (synchronises)
    c->hand_labels = stop_at_labels != 0;
    c->hand_thr = threshold;
    c->hand_nodata = nodata;
    held_commit(c, HP_HAND, u, held_variant(elev_source, c->hand_labels));
    *undrained = u;
    return MHIP_OK;
}

int mhip_ctx_hand_rows(mhip_ctx *c, int32_t which, int64_t row0, int64_t nrows, float *dst)
{
    return held_rows(c, which == 0 ? HELD_HAND : which == 1 ? HELD_DRAINDIST : -1, row0, nrows, dst, "ctx_hand_rows(ctx, which, row0, nrows, dst)");
}

/* ---- DEM adaptations: culvert and dike lines into the resident DEM (burn.hip) ---------------------------------------------------- */
int mhip_ctx_burn_lines(mhip_ctx *c, int64_t nseg, const mhip_burn_segment *segments, int64_t nline, const mhip_burn_line *lines, double nodata,
                        mhip_burn_result *results)
{
    MH_ARG(c, "ctx_burn_lines(ctx, nseg, segments, nline, lines, nodata, results)");
    MH_ARG(undivided(c), "DEM adaptations on a row band are not built (a line crosses the seams: a later step); use an undivided context");
    MH_ARG(c->have[MHIP_R_DEM], "ctx_burn_lines needs the DEM raster");
    MH_TRY(burn_check(nseg, segments, nline, lines, results));
    if (nseg == 0) return burn_lines_dev(nullptr, c->H, c->W, 0, segments, nline, lines, nodata, results, nullptr);      // (the records; the context stays as it is)
    MH_HIP(hipSetDevice(c->device));
    ctx_wrote(c, MHIP_R_DEM, /*uploaded=*/true);
    return burn_lines_dev(c->r[MHIP_R_DEM].as<float>(), c->H, c->W, nseg, segments, nline, lines, nodata, results, c->stream);
}

/* ---- object exposure: polygons to a zone raster of the context, statistics of a resident raster per zone (zones.hip) -------------- */
int mhip_ctx_rasterize_zones(mhip_ctx *c, int64_t nvert, const double *xy, int64_t nring, const int64_t *ring_offsets, const int32_t *ring_zone,
                             int64_t nzone, int32_t grow)
{
    MH_ARG(c, "ctx_rasterize_zones(ctx, nvert, xy, nring, ring_offsets, ring_zone, nzone, grow)");
    MH_ARG(undivided(c), "zones on a row band are not built (an object crosses the seams: a later step); use an undivided context");
    MH_TRY(zones_check(c->H, c->W, nvert, xy, nring, ring_offsets, ring_zone, nzone, grow));
    MH_HIP(hipSetDevice(c->device));
    DevBuf &zones = held_begin(c, HP_ZONES).buf[0];
    MH_TRY(zones.alloc(4 * (size_t)(c->H * c->W)));
    if (nring == 0) {
        MH_HIP(hipMemsetAsync(zones.p, 0, 4 * (size_t)(c->H * c->W), c->stream));
        MH_HIP(stream_sync(c->stream));
    } else {
        MH_TRY(zones_rasterize_dev(zones.as<int32_t>(), c->H, c->W, nvert, xy, nring, ring_offsets, ring_zone, nzone, grow, c->stream));      // (synchronises)
    }
    held_commit(c, HP_ZONES, nzone);
    return MHIP_OK;
}

int mhip_ctx_zones_rows(mhip_ctx *c, int64_t row0, int64_t nrows, int32_t *dst)
{
    return held_rows(c, HELD_ZONES, row0, nrows, dst, "ctx_zones_rows(ctx, row0, nrows, dst)");
}

int mhip_ctx_zone_stats(mhip_ctx *c, int32_t source, mhip_zone_record *records)
{
    MH_ARG(c && records, "ctx_zone_stats(ctx, source, records)");
    MH_ARG(undivided(c), "zones on a row band are not built (an object crosses the seams: a later step); use an undivided context");
    const bool member = source == MHIP_R_DEM || source == MHIP_R_FILLED || source == MHIP_R_DEPTHS || source == MHIP_R_FINALDEPTHS;
    const int id = held_source(&HeldRow::zsrc, source);
    MH_ARG(member || id >= 0, "ctx_zone_stats: the source is no float32 raster of the context");
    void *src = member ? c->r[source].p : nullptr, *zones = nullptr;
    if (member) MH_ARG(c->have[source], "raster has not been computed or uploaded");
    else MH_TRY(ctx_held(c, id, &src));
    MH_ARG(ctx_held(c, HELD_ZONES, &zones) == MHIP_OK, "ctx_zone_stats needs mhip_ctx_rasterize_zones");
    const int64_t nzone = c->held[HP_ZONES].state;
    MH_HIP(hipSetDevice(c->device));
    DevBuf d_rec;
    MH_TRY(d_rec.alloc(sizeof(mhip_zone_record) * (size_t)(nzone + 1)));
    MH_TRY(zone_stats_dev((const float *)src, (const int32_t *)zones, c->H * c->W, c->W, nzone, d_rec.as<mhip_zone_record>(), c->stream));
    return ctx_fetch(c, d_rec, sizeof(mhip_zone_record) * (size_t)(nzone + 1), records);
}

/* ---- the outlines of the resident labels or watersheds (polygonize.hip): a snapshot in buffers of the handle, no raster leaves the device */
int mhip_ctx_polygonize(mhip_ctx *c, int32_t source, mhip_polygons **out)
{
    MH_ARG(c && out, "ctx_polygonize(ctx, source, out)");
    const int id = held_source(&HeldRow::psrc, source);
    MH_ARG(source == MHIP_R_LABELS || source == MHIP_R_WATERSHEDS || id >= 0,
           "ctx_polygonize: the source is MHIP_R_LABELS or MHIP_R_WATERSHEDS, MHIP_PSRC_REACHCATCH for the reach catchments or MHIP_PSRC_SEACLASSES for the sea flood's classes");
    MH_ARG(undivided(c), "outlines on a row band are not built (a ring crosses the seams: a later step); use an undivided context");
    void *held = nullptr;
    if (id >= 0) MH_TRY(ctx_held(c, id, &held));
    else MH_ARG(c->have[source], "raster has not been computed or uploaded");
    if (source == MHIP_R_LABELS) MH_ARG(c->labels_filtered && !c->ccl_pending, "ctx_polygonize needs mhip_ctx_apply_keep after the LABEL run");
    MH_TRY(polygonize_check(c->H, c->W));
    MH_HIP(hipSetDevice(c->device));
    mhip_polygons *p = new (std::nothrow) mhip_polygons();
    if (!p) {
        set_error("ctx_polygonize: out of host memory");
        return MHIP_EHIP;
    }
    p->device = c->device;
    const int32_t *d_src = held ? (const int32_t *)held : c->r[source].as<int32_t>();
    const int rc = polygonize_dev(d_src, c->H, c->W, p->xy, p->ring_offsets, p->ring_label, &p->nring, &p->nvert, c->stream);      // (synchronises)
    if (rc != MHIP_OK) {
        delete p;
        return rc;
    }
    *out = p;
    return MHIP_OK;
}

/* ---- the flow paths of the resident flow directions and accumulation (flowpaths.hip): a snapshot in buffers of the handle */
int mhip_ctx_flowpaths(mhip_ctx *c, double threshold, int32_t stop_at_labels, mhip_flowpaths **out)
{
    MH_ARG(c && out, "ctx_flowpaths(ctx, threshold, stop_at_labels, out)");
    MH_TRY(flowpaths_check(c->H, c->W, threshold));
    MH_ARG(undivided(c), "flow paths on a row band are not built (a reach crosses the seams: a later step); use an undivided context");
    MH_ARG(c->have[MHIP_R_FLOWDIR] && c->have[MHIP_R_ACCUM], "raster has not been computed or uploaded");
    if (stop_at_labels) {
        MH_ARG(c->have[MHIP_R_LABELS], "raster has not been computed or uploaded");
        MH_ARG(c->labels_filtered && !c->ccl_pending, "ctx_flowpaths needs mhip_ctx_apply_keep after the LABEL run");
    }
    MH_HIP(hipSetDevice(c->device));
    mhip_flowpaths *p = new (std::nothrow) mhip_flowpaths();
    if (!p) {
        set_error("ctx_flowpaths: out of host memory");
        return MHIP_EHIP;
    }
    p->device = c->device;
    const int rc = flowpaths_dev(c->r[MHIP_R_FLOWDIR].as<uint8_t>(), c->r[MHIP_R_ACCUM].as<double>(), stop_at_labels ? c->r[MHIP_R_LABELS].as<int32_t>() : nullptr,
                                 c->H, c->W, threshold, p, c->stream);      // (synchronises)
    if (rc != MHIP_OK) {
        delete p;
        return rc;
    }
    *out = p;
    return MHIP_OK;
}

/* ---- runoff-weighted accumulation down the resident flow directions (wacc.hip): a snapshot in buffers of the handle, no held product */
int mhip_ctx_weighted_accum(mhip_ctx *c, const uint32_t *weight, int32_t use_watersheds, mhip_wacc **out)
{
    MH_ARG(c && weight && out, "ctx_weighted_accum(ctx, weight, use_watersheds, out)");
    MH_ARG(undivided(c), "weighted accumulation on a row band is not built (a path crosses the seams: a later step); use an undivided context");
    MH_ARG(c->have[MHIP_R_FLOWDIR], "ctx_weighted_accum needs the FLOWDIR raster");
    if (use_watersheds) MH_ARG(c->have[MHIP_R_WATERSHEDS] && c->nlabels >= 0, "ctx_weighted_accum with use_watersheds needs the WATERSHEDS raster and its labels");
    MH_TRY(wacc_check(c->H, c->W, c->nlabels, use_watersheds != 0));
    MH_HIP(hipSetDevice(c->device));
    mhip_wacc *p = new (std::nothrow) mhip_wacc();
    if (!p) {
        set_error("ctx_weighted_accum: out of host memory");
        return MHIP_EHIP;
    }
    p->device = c->device;
    p->H = c->H;
    p->W = c->W;
    p->nzone = use_watersheds ? c->nlabels : -1;
    const size_t n = (size_t)(c->H * c->W);
    DevBuf d_w;
    int rc = upload(d_w, weight, 4 * n, c->stream);
    if (rc == MHIP_OK) rc = p->acc.alloc(8 * n);
    if (rc == MHIP_OK && use_watersheds) rc = p->sums.alloc(8 * (size_t)(c->nlabels + 1));
    if (rc == MHIP_OK)
        rc = wacc_dev(c->r[MHIP_R_FLOWDIR].as<uint8_t>(), d_w.as<uint32_t>(), use_watersheds ? c->r[MHIP_R_WATERSHEDS].as<int32_t>() : nullptr, c->H, c->W,
                      c->nlabels, p->acc.as<unsigned long long>(), use_watersheds ? p->sums.as<unsigned long long>() : nullptr, &p->unresolved,
                      c->stream);      // (synchronises)
    else
        (void)stream_sync(c->stream);  // (the upload may still read the caller's array)
    if (rc != MHIP_OK) {
        delete p;
        return rc;
    }
    *out = p;
    return MHIP_OK;
}

/* ---- multiple-flow-direction accumulation down the resident no-flats surface (mfd.hip): a snapshot in an mhip_wacc handle ------------ */
int mhip_ctx_mfd_accum(mhip_ctx *c, int32_t exponent, const uint32_t *weight, mhip_wacc **out)
{
    MH_ARG(c && out, "ctx_mfd_accum(ctx, exponent, weight_or_NULL, out)");
    MH_ARG(undivided(c), "mfd accumulation on a row band is not built (the flow crosses the seams: a later step); use an undivided context");
    MH_ARG(c->have[MHIP_R_NOFLAT], "ctx_mfd_accum needs the NOFLAT raster");
    MH_ARG(exponent >= 1 && exponent <= 8, "ctx_mfd_accum: exponent in [1, 8]");
    MH_TRY(mfd_check(c->H, c->W));
    MH_HIP(hipSetDevice(c->device));
    double *g = nullptr;
    MH_TRY(ctx_noflat(c, &g));      // (a pending surface is written first, as for every other reader)
    mhip_wacc *p = new (std::nothrow) mhip_wacc();
    if (!p) {
        set_error("ctx_mfd_accum: out of host memory");
        return MHIP_EHIP;
    }
    p->device = c->device;
    p->H = c->H;
    p->W = c->W;
    p->nzone = -1;
    const size_t n = (size_t)(c->H * c->W);
    DevBuf d_w, d_fr;
    int rc = weight ? upload(d_w, weight, 4 * n, c->stream) : MHIP_OK;
    if (rc == MHIP_OK) rc = d_fr.alloc(16 * n);
    if (rc == MHIP_OK) rc = p->acc.alloc(8 * n);
    if (rc == MHIP_OK) rc = mfd_fractions_dev(g, c->H, c->W, exponent, d_fr.as<uint16_t>(), c->stream);
    MfdStats st;
    if (rc == MHIP_OK)
        rc = mfd_accum_dev(d_fr.as<uint16_t>(), weight ? d_w.as<uint32_t>() : nullptr, MHIP_WACC_UNIT, c->H, c->W, p->acc.as<unsigned long long>(), &p->unresolved,
                           &st, c->stream);      // (synchronises)
    p->rounds = st.rounds;
    p->visits = st.visits;
    p->tiles = st.tiles;
    if (rc != MHIP_OK) {
        (void)stream_sync(c->stream);      // (the upload may still read the caller's array)
        delete p;
        return rc;
    }
    *out = p;
    return MHIP_OK;
}

/* ---- reach catchments and flood depths from a stage per reach (hand.hip, flowpaths.hip, reachcatch.hip) ---------------------------- */
int mhip_ctx_reach_catchments(mhip_ctx *c, double threshold, int32_t stop_at_labels, mhip_flowpaths **out, int64_t *assigned)
{
    MH_ARG(c && out && assigned, "ctx_reach_catchments(ctx, threshold, stop_at_labels, out_reaches, assigned)");
    MH_TRY(flowpaths_check(c->H, c->W, threshold));
    MH_ARG(undivided(c), "reach catchments on a row band are not built (a path crosses the seams: a later step); use an undivided context");
    MH_ARG(c->have[MHIP_R_FLOWDIR] && c->have[MHIP_R_ACCUM], "ctx_reach_catchments needs the FLOWDIR and ACCUM rasters");
    if (stop_at_labels) {
        MH_ARG(c->have[MHIP_R_LABELS] && !c->ccl_pending, "ctx_reach_catchments with stop_at_labels needs the LABELS raster");
        MH_ARG(c->labels_filtered, "ctx_reach_catchments needs mhip_ctx_apply_keep after the LABEL run");
    }
    MH_HIP(hipSetDevice(c->device));
    mhip_flowpaths *p = new (std::nothrow) mhip_flowpaths();
    if (!p) {
        set_error("ctx_reach_catchments: out of host memory");
        return MHIP_EHIP;
    }
    p->device = c->device;
    DevBuf &catchments = held_begin(c, HP_REACHCATCH).buf[0];      // (the depths of mhip_ctx_inundate go with it)
    int64_t a = 0;
    int rc = catchments.alloc(4 * (size_t)(c->H * c->W));
    if (rc == MHIP_OK)
        rc = reach_catchments_dev(c->r[MHIP_R_FLOWDIR].as<uint8_t>(), c->r[MHIP_R_ACCUM].as<double>(),
                                  stop_at_labels ? c->r[MHIP_R_LABELS].as<int32_t>() : nullptr, c->H, c->W, threshold, catchments.as<int32_t>(), p, &a,
                                  c->stream);      // (synchronises)
    if (rc != MHIP_OK) {
        delete p;
        catchments.release();
        return rc;
    }
    c->rcatch_thr = threshold;
    c->rcatch_labels = stop_at_labels != 0;
    held_commit(c, HP_REACHCATCH, p->nreach, held_variant(0, c->rcatch_labels));
    *assigned = a;
    *out = p;
    return MHIP_OK;
}

int mhip_ctx_reach_catchments_rows(mhip_ctx *c, int64_t row0, int64_t nrows, int32_t *dst)
{
    return held_rows(c, HELD_REACHCATCH, row0, nrows, dst, "ctx_reach_catchments_rows(ctx, row0, nrows, dst)");
}

int mhip_ctx_inundate(mhip_ctx *c, int64_t nreach, const float *stage, mhip_zone_record *records)
{
    MH_ARG(c && stage, "ctx_inundate(ctx, nreach, stage, records)");
    MH_ARG(undivided(c), "inundation on a row band is not built (a path crosses the seams: a later step); use an undivided context");
    void *hand = nullptr, *rcatch = nullptr;
    MH_ARG(ctx_held(c, HELD_HAND, &hand) == MHIP_OK, "ctx_inundate needs mhip_ctx_hand on the resident rasters");
    MH_ARG(ctx_held(c, HELD_REACHCATCH, &rcatch) == MHIP_OK, "ctx_inundate needs mhip_ctx_reach_catchments on the resident rasters");
    MH_ARG(c->hand_thr == c->rcatch_thr, "ctx_inundate: the hand and the reach catchments were made with different thresholds");
    MH_ARG(c->hand_labels == c->rcatch_labels, "ctx_inundate: the hand and the reach catchments were made with different stop_at_labels");
    MH_ARG(nreach == c->held[HP_REACHCATCH].state, "ctx_inundate: nreach is not the number of reaches of the catchments held");
    MH_HIP(hipSetDevice(c->device));
    DevBuf &out = held_begin(c, HP_INUNDATION).buf[0];
    const int64_t n = c->H * c->W;
    DevBuf d_stage, d_rec;
    MH_TRY(upload(d_stage, stage, 4 * ((size_t)nreach + 1), c->stream));
    if (records) MH_TRY(d_rec.alloc(sizeof(mhip_zone_record) * (size_t)(nreach + 1)));
    MH_TRY(out.alloc(4 * (size_t)n));
    const int rc = inundate_dev((const float *)hand, (const int32_t *)rcatch, n, c->W, nreach, d_stage.as<float>(), c->hand_nodata, out.as<float>(),
                                records ? d_rec.as<mhip_zone_record>() : nullptr, c->stream);      // (synchronises)
    if (rc != MHIP_OK) {
        out.release();
        return rc;
    }
    held_commit(c, HP_INUNDATION, 1);
    if (records) return ctx_fetch(c, d_rec, sizeof(mhip_zone_record) * (size_t)(nreach + 1), records);
    return MHIP_OK;
}

int mhip_ctx_inundation_rows(mhip_ctx *c, int64_t row0, int64_t nrows, float *dst)
{
    return held_rows(c, HELD_INUNDATION, row0, nrows, dst, "ctx_inundation_rows(ctx, row0, nrows, dst)");
}

/* ---- flooding from sources at a water level, and what follows from the level raster (seaflood.hip) --------------------------------- */
int mhip_ctx_sea_flood(mhip_ctx *c, const float *stage, const float *zone_stage, int64_t nzone, float max_level, float nodata, int64_t *reached)
{
    MH_ARG(c && reached, "ctx_sea_flood(ctx, stage_or_NULL, zone_stage_or_NULL, nzone, max_level, nodata, reached)");
    MH_ARG((stage != nullptr) != (zone_stage != nullptr), "ctx_sea_flood takes exactly one source form: a stage raster, or a stage per zone");
    MH_TRY(sea_flood_check(max_level, nodata));
    MH_ARG(undivided(c), "sea flooding on a row band is not built (the water crosses the seams: a later step); use an undivided context");
    MH_ARG(c->have[MHIP_R_DEM], "ctx_sea_flood needs the DEM raster");
    void *zones = nullptr;
    if (zone_stage) {
        MH_ARG(ctx_held(c, HELD_ZONES, &zones) == MHIP_OK, "ctx_sea_flood with a stage per zone needs mhip_ctx_rasterize_zones");
        MH_ARG(nzone == c->held[HP_ZONES].state, "ctx_sea_flood: nzone is not the number of zones of the zone raster held");
    }
    MH_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const int64_t n = c->H * c->W;
    DevBuf &level = held_begin(c, HP_SEALEVEL).buf[0];      // (the depths and the classes go with it)
    DevBuf d_stage;
    if (stage) {
        MH_TRY(upload(d_stage, stage, 4 * (size_t)n, s));
    } else {      // (entry 0 is no zone: a NaN, whatever the caller left there)
        std::vector<float> zs(zone_stage, zone_stage + nzone + 1);
        zs[0] = std::numeric_limits<float>::quiet_NaN();
        MH_TRY(upload(d_stage, zs.data(), 4 * zs.size(), s));
        MH_HIP(stream_sync(s));      // (zs goes away)
    }
    MH_TRY(level.alloc(4 * (size_t)n));
    int64_t r = 0;
    const int rc = sea_flood_dev(c->r[MHIP_R_DEM].as<float>(), stage ? d_stage.as<float>() : nullptr, (const int32_t *)zones, stage ? nullptr : d_stage.as<float>(),
                                 stage ? 0 : nzone, c->H, c->W, max_level, nodata, level.as<float>(), &r, &c->sea_st, s);      // (synchronises)
    if (rc != MHIP_OK) {
        MH_HIP(stream_sync(s));      // (an error may have left launches behind: the buffers go back to the pool)
        level.release();
        return rc;
    }
    c->sea_max_level = max_level;
    c->sea_nodata = nodata;
    held_commit(c, HP_SEALEVEL, r);
    *reached = r;
    return MHIP_OK;
}

int mhip_ctx_sea_flood_rows(mhip_ctx *c, int32_t which, int64_t row0, int64_t nrows, float *dst)
{
    return held_rows(c, which == 0 ? HELD_SEALEVEL : which == 1 ? HELD_SEADEPTH : -1, row0, nrows, dst, "ctx_sea_flood_rows(ctx, which, row0, nrows, dst)");
}

int mhip_ctx_sea_levels(mhip_ctx *c, int32_t K, const float *levels, mhip_sea_record *records)
{
    MH_ARG(c && levels && records, "ctx_sea_levels(ctx, K, levels, records)");
    void *lev = nullptr;
    MH_ARG(ctx_held(c, HELD_SEALEVEL, &lev) == MHIP_OK, "ctx_sea_levels needs mhip_ctx_sea_flood on the resident DEM");
    MH_TRY(sea_levels_check(K, levels, c->sea_max_level));
    MH_HIP(hipSetDevice(c->device));
    return sea_levels_dev((const float *)lev, c->r[MHIP_R_DEM].as<float>(), c->H * c->W, c->sea_nodata, K, levels, records, c->stream);
}

int mhip_ctx_sea_depths(mhip_ctx *c, float z)
{
    MH_ARG(c, "ctx_sea_depths(ctx, z)");
    void *lev = nullptr;
    MH_ARG(ctx_held(c, HELD_SEALEVEL, &lev) == MHIP_OK, "ctx_sea_depths needs mhip_ctx_sea_flood on the resident DEM");
    MH_TRY(sea_levels_check(1, &z, c->sea_max_level));
    MH_HIP(hipSetDevice(c->device));
    DevBuf &out = held_begin(c, HP_SEADEPTH).buf[0];
    MH_TRY(out.alloc(4 * (size_t)(c->H * c->W)));
    MH_TRY(sea_depths_dev((const float *)lev, c->r[MHIP_R_DEM].as<float>(), c->H * c->W, c->sea_nodata, z, out.as<float>(), c->stream));
    held_commit(c, HP_SEADEPTH, 1);
    return MHIP_OK;
}

int mhip_ctx_sea_classes(mhip_ctx *c, int32_t K, const float *levels)
{
    MH_ARG(c && levels, "ctx_sea_classes(ctx, K, levels)");
    void *lev = nullptr;
    MH_ARG(ctx_held(c, HELD_SEALEVEL, &lev) == MHIP_OK, "ctx_sea_classes needs mhip_ctx_sea_flood on the resident DEM");
    MH_TRY(sea_levels_check(K, levels, c->sea_max_level));
    MH_HIP(hipSetDevice(c->device));
    DevBuf &out = held_begin(c, HP_SEACLASS).buf[0];
    MH_TRY(out.alloc(4 * (size_t)(c->H * c->W)));
    MH_TRY(sea_classes_dev((const float *)lev, c->H * c->W, c->sea_nodata, K, levels, out.as<int32_t>(), c->stream));
    held_commit(c, HP_SEACLASS, 1);
    return MHIP_OK;
}

int mhip_ctx_sea_classes_rows(mhip_ctx *c, int64_t row0, int64_t nrows, int32_t *dst)
{
    return held_rows(c, HELD_SEACLASS, row0, nrows, dst, "ctx_sea_classes_rows(ctx, row0, nrows, dst)");
}

}  // extern "C"
