// ctx_run.hip -- the stages of the device-resident pipeline and their DAG (mhip_ctx_run): one host thread per branch, two or three
// streams, HIP-event timing per stage.  Every stage that writes a resident raster says so with ctx_wrote (ctx.hpp).
#include <atomic>
#include <cmath>
#include <future>
#include <string>

#include "ctx.hpp"
#include "handover_addr.hpp"

using namespace mh;

constexpr int LABEL_START_DEFAULT = 3;      // chosen by measurement: DESIGN 4.5
constexpr int FILL_HANDOVER_DEFAULT = 1;    // chosen by measurement: DESIGN 7
constexpr int NOFLAT_LAZY_DEFAULT = 1;      // chosen by measurement: DESIGN 7
constexpr int WETBITS_DEFAULT = 1;          // chosen by measurement: DESIGN 7

// MHIP_FILL_HANDOVER = 0 | 1 (development knob, read per request): may a request that holds FILL and NOFLAT leave the flood's
// last pass and its proof to the first visit of the no-flats fill?
static bool fill_handover_env()
{
    const char *e = dev_env("MHIP_FILL_HANDOVER");
    return e ? e[0] != '0' : FILL_HANDOVER_DEFAULT != 0;
}

// MHIP_NOFLAT_LAZY = 0 | 1 (development knob, read per request): may a request that holds NOFLAT and FLOWDIR leave the no-flats
// surface unwritten where its finishing pass has derived the directions from it (ctx.hpp: noflat_pending)?
static bool noflat_lazy_env()
{
    const char *e = dev_env("MHIP_NOFLAT_LAZY");
    return e ? e[0] != '0' : NOFLAT_LAZY_DEFAULT != 0;
}

// MHIP_WETBITS = 0 | 1 (development knob, read per request): may the finishing pass and the labelling of a request whose flood
// handed over to the no-flats fill read that visit's proof bits "filled > dem" instead of the DEM and the depths?
static bool wetbits_env()
{
    const char *e = dev_env("MHIP_WETBITS");
    return e ? e[0] != '0' : WETBITS_DEFAULT != 0;
}

static int stage_depths(mhip_ctx *c, hipStream_t s)
{
    MH_ARG(c->have[MHIP_R_FILLED] && c->have[MHIP_R_DEM], "depths need the filled surface");
    MH_TRY(ctx_raster(c, MHIP_R_DEPTHS));
    MH_TRY(depths_dev(c->r[MHIP_R_FILLED].as<float>(), c->r[MHIP_R_DEM].as<float>(), c->r[MHIP_R_DEPTHS].as<float>(), c->H * c->W, s));
    ctx_wrote(c, MHIP_R_DEPTHS);
    c->have[MHIP_R_DEPTHS] = true;
    return MHIP_OK;
}

// with_depths == false: the caller computes the bluespot depths on another stream (stage DAG)
// ho: the flood may leave FILLED and DEPTHS to the no-flats stage of the same request (ho->pending on return; neither raster is
// marked resident before that stage has queued the pass that writes them); the stage's time then ends behind pf_final_kernel
static int stage_fill(mhip_ctx *c, hipStream_t s, bool with_depths = true, FillHandover *ho = nullptr)
{
    const int64_t H = c->H, W = c->W;
    MH_ARG(c->have[MHIP_R_DEM], "FILL needs the DEM");
    MH_TRY(ctx_raster(c, MHIP_R_FILLED));
    MH_TRY(ctx_raster(c, MHIP_R_DEPTHS));
    MH_TRY(stage_begin(c, MHIP_STAGE_FILL, s));
    FillStats st;
    bool depths_done = false;   // the priority-flood's last pass writes filled - dem next to the filled surface
    MH_TRY(fill_plain_dev(c->r[MHIP_R_DEM].as<float>(), c->r[MHIP_R_FILLED].as<float>(), H, W, s, &st, c->r[MHIP_R_DEPTHS].as<float>(),
                          &depths_done, ho));
    ctx_wrote(c, MHIP_R_FILLED);
    ctx_wrote(c, MHIP_R_DEPTHS);
    const bool owed = ho && ho->pending;
    c->have[MHIP_R_FILLED] = !owed;
    c->have[MHIP_R_DEPTHS] = depths_done && !owed;
    if (with_depths && !depths_done) MH_TRY(stage_depths(c, s));
    MH_TRY(stage_end(c, MHIP_STAGE_FILL, s));
    c->fill_rounds = st.rounds;
    c->fill_st = st;
    return MHIP_OK;
}

// shdg_done: minimum_safe_short_and_diag of the current DEM is already in c->sh / c->dg (computed next to the fill)
// with_flowdir: FLOWDIR is part of the same request -- the geodesic transform's finishing pass writes the directions as well when
// it can (one context, regular surface); *flowdir_done then tells the caller that stage_flowdir has nothing left to do
// ho (pending): FILLED and DEPTHS are still owed by the flood of this request; they become resident when the pass that writes
// them has been queued (ctx_handover_settled: from the hook that starts the label branch, and behind the stage)
static void ctx_handover_settled(mhip_ctx *c, FillHandover *ho)
{
    if (!ho || ho->pending || c->have[MHIP_R_FILLED]) return;
    c->have[MHIP_R_FILLED] = true;
    c->have[MHIP_R_DEPTHS] = true;
    c->fill_handover = ho->queued ? 1 : 0;
    if (ho->suspect) ++c->fill_handover_rechecks;
    if (ho->repaired) {      // the proof failed in the fused visit: flood + repair (fill_plain_dev reports the same)
        c->fill_st.algorithm = 4;
        c->fill_st.rounds += ho->st_repair.rounds;
        c->fill_st.visits += ho->st_repair.visits;
        c->fill_st.cycles += ho->st_repair.cycles;
        c->fill_rounds = c->fill_st.rounds;
    }
}

static int stage_noflat(mhip_ctx *c, hipStream_t s, bool shdg_done = false, StageHook *tail_hook = nullptr, bool with_flowdir = false,
                        bool *flowdir_done = nullptr, FillHandover *ho = nullptr)
{
    const int64_t H = c->H, W = c->W, n = H * W;
    MH_ARG(c->have[MHIP_R_DEM], "NOFLAT needs the DEM");
    MH_TRY(ctx_raster(c, MHIP_R_NOFLAT));      // (allocated whoever writes it: the relaxation needs it, and no later reader runs out of memory)
    c->noflat_pending = false;                 // a new surface replaces one that nobody has asked for
    MH_TRY(stage_begin(c, MHIP_STAGE_NOFLAT, s));
    if (!shdg_done) {
        // (the flood of THIS DEM has folded its extremes on the way: a request without the bluespot branch -- BASELINE configs[1] -- used
        // to run the reduction over the DEM all the same, 0.38 ms of its 2.15 ms step)
        if ((c->have[MHIP_R_FILLED] || (ho && ho->pending)) && c->fill_st.have_minmax) short_diag_from_minmax(c->fill_st.dem_min, c->fill_st.dem_max, c->fill_st.dem_nan, &c->sh, &c->dg);
        else MH_TRY(short_diag_dev(c->r[MHIP_R_DEM].as<float>(), n, &c->sh, &c->dg, s));
    }
    FillStats st;
    if (!c->have[MHIP_R_FILLED] && !(ho && ho->pending)) {  // the plain fill seeds the no-flats iteration (fill_noflat_dev)
        MH_TRY(ctx_raster(c, MHIP_R_FILLED));
        FillStats st0;
        MH_TRY(fill_plain_dev(c->r[MHIP_R_DEM].as<float>(), c->r[MHIP_R_FILLED].as<float>(), H, W, s, &st0));
        ctx_wrote(c, MHIP_R_FILLED);
        c->have[MHIP_R_FILLED] = true;
    }
    // the wet bits stand for floats only where "filled > dem" is "filled - dem != 0": no NaN, no infinity in the DEM -- which the
    // flood of this request has told (a DEM it did not fold: no bits)
    if (ho && ho->wet && !(c->fill_st.have_minmax && !c->fill_st.dem_nan && std::isfinite(c->fill_st.dem_min) && std::isfinite(c->fill_st.dem_max)))
        ho->wet = nullptr;
    D8Sink d8;
    static const bool fuse_d8 = [] { const char *e = dev_env("MHIP_D8_FUSE"); return !(e && e[0] == '0'); }();   // (development: 0 = D8 as a pass of its own)
    if (with_flowdir && fuse_d8 && !c->ht && !c->hb) {
        MH_TRY(ctx_raster(c, MHIP_R_FLOWDIR));
        MH_TRY(c->nodir_cnt.alloc(4));
        MH_HIP(hipMemsetAsync(c->nodir_cnt.p, 0, 4, s));
        d8.flowdir = c->r[MHIP_R_FLOWDIR].as<uint8_t>();
        d8.nodir = c->nodir_cnt.as<unsigned int>();
        // nobody reads the surface in this request but the pass that writes the directions: it may stay F and the distances, which
        // then live in a raster of the context's (they outlive the stage's workspace), until somebody asks (ctx_noflat)
        if (c->nranks == 1 && noflat_lazy_env()) {
            MH_TRY(ctx_raster(c, MHIP_R_NGDIST));
            d8.dist = c->r[MHIP_R_NGDIST].as<uint32_t>();
            d8.defer = true;
        }
    }
    const int rc_nf = fill_noflat_dev(c->r[MHIP_R_DEM].as<float>(), c->r[MHIP_R_NOFLAT].as<double>(), H, W, c->sh, c->dg, s, &st,
                                      c->r[MHIP_R_FILLED].as<float>(), tail_hook, d8.flowdir ? &d8 : nullptr, ho);
    ctx_handover_settled(c, ho);
    if (ho && ho->wet_pass) c->wet_pass_used = 1;
    MH_TRY(rc_nf);
    if (flowdir_done) *flowdir_done = d8.done;
    MH_TRY(stage_end(c, MHIP_STAGE_NOFLAT, s));
    c->noflat_rounds = st.rounds;
    c->noflat_st = st;
    ctx_wrote(c, MHIP_R_NOFLAT);
    c->have[MHIP_R_NOFLAT] = true;
    c->noflat_pending = d8.deferred;
    return MHIP_OK;
}

static int stage_flowdir(mhip_ctx *c, hipStream_t s)
{
    MH_ARG(c->have[MHIP_R_NOFLAT], "FLOWDIR needs the no-flats surface");
    double *g = nullptr;
    MH_TRY(ctx_noflat(c, &g));      // (in front of the stage's events)
    MH_TRY(ctx_raster(c, MHIP_R_FLOWDIR));
    MH_TRY(stage_begin(c, MHIP_STAGE_FLOWDIR, s));
    ctx_wrote(c, MHIP_R_FLOWDIR);
    MH_TRY(c->nodir_cnt.alloc(4));
    MH_HIP(hipMemsetAsync(c->nodir_cnt.p, 0, 4, s));
    MH_TRY(d8_dev(g, c->r[MHIP_R_FLOWDIR].as<uint8_t>(), c->H, c->W, 1, s, c->row0 - c->ht, c->H_global, c->nodir_cnt.as<unsigned int>()));
    MH_TRY(stage_end(c, MHIP_STAGE_FLOWDIR, s));
    c->have[MHIP_R_FLOWDIR] = true;
    c->flowdir_own = true;
    c->nodir_valid = !c->ht && !c->hb;     // (a band's halo rows are computed from clamped data: their codes do not count)
    return MHIP_OK;
}

// the no-flats fill's finishing pass wrote the flow directions (stage_noflat: with_flowdir): the stage is an empty interval
static int stage_flowdir_fused(mhip_ctx *c, hipStream_t s)
{
    MH_TRY(stage_begin(c, MHIP_STAGE_FLOWDIR, s));
    MH_TRY(stage_end(c, MHIP_STAGE_FLOWDIR, s));
    ctx_wrote(c, MHIP_R_FLOWDIR);
    c->have[MHIP_R_FLOWDIR] = true;
    c->nodir_valid = true;
    c->flowdir_own = true;
    return MHIP_OK;
}

// prep: the node buffer, cleared ahead of the stage (mhip_ctx_run)
static int stage_accum(mhip_ctx *c, hipStream_t s, PourLink *pour = nullptr, AccumPrep *prep = nullptr)
{
    MH_ARG(c->have[MHIP_R_FLOWDIR], "ACCUM needs flow directions");
    MH_TRY(ctx_raster(c, MHIP_R_ACCUM));
    MH_TRY(stage_begin(c, MHIP_STAGE_ACCUM, s));
    bool delta_done = false;
    // a row band right behind its boundary pass (own contributions in ACCUM, the neighbours' values in the halo rows by now): only
    // the flux that enters at the seams is added, along the paths the kept perimeter graph says it takes (accum.hip)
    if ((c->ht || c->hb) && c->acc_keep.valid)
        MH_TRY(accum_band_delta_dev(c->r[MHIP_R_FLOWDIR].as<uint8_t>(), c->r[MHIP_R_ACCUM].as<double>(), c->H, c->W, s, c->ht, c->hb, &c->acc_keep, &delta_done));
    c->accum_algorithm = delta_done ? 1 : 0;
    ctx_wrote(c, MHIP_R_ACCUM);
    if (!delta_done)
        MH_TRY(accum_dev(c->r[MHIP_R_FLOWDIR].as<uint8_t>(), c->r[MHIP_R_ACCUM].as<double>(), c->H, c->W, s, c->ht, c->hb, 0, nullptr, pour, nullptr,
                         prep));
    MH_TRY(stage_end(c, MHIP_STAGE_ACCUM, s));
    c->have[MHIP_R_ACCUM] = true;
    return MHIP_OK;
}

// ho: the hand-over of this request, if any -- its wet bits are the foreground of the depths its first visit wrote (wet_ok)
static int stage_label(mhip_ctx *c, hipStream_t s, const FillHandover *ho = nullptr)
{
    const int64_t H = c->H, W = c->W, n = H * W;
    MH_ARG(c->have[MHIP_R_DEPTHS] || c->have[MHIP_R_FILLED], "LABEL needs bluespot depths");
    MH_TRY(ctx_raster(c, MHIP_R_LABELS));
    if (!c->tmp_i32.p) MH_TRY(c->tmp_i32.alloc(4 * (size_t)n));
    MH_TRY(stage_begin(c, MHIP_STAGE_LABEL, s));
    if (!c->have[MHIP_R_DEPTHS]) MH_TRY(stage_depths(c, s));   // stage DAG: the fill left them to this branch
    // (label_stats of the raw labels rides on the labelling's last pass: as two passes 21.8 -> 22.2 ms a step, and with the statistics
    // behind the stage's event -- beside the watersheds, off the critical path -- 22.3: round 4)
    ctx_wrote(c, MHIP_R_LABELS);
    const unsigned long long *wet = ho && ho->wet_ok && c->have[MHIP_R_DEPTHS] ? ho->wet : nullptr;
    bool wet_used = false;
    MH_TRY(ccl8_f32_dev(c->r[MHIP_R_DEPTHS].as<float>(), c->r[MHIP_R_LABELS].as<int32_t>(), c->tmp_i32.as<int32_t>(), H, W,
                        &c->nlabels_raw, s, &c->raw_stats, wet, &wet_used));
    if (wet_used) c->wet_label_used = 1;
    MH_TRY(stage_end(c, MHIP_STAGE_LABEL, s));
    c->have[MHIP_R_LABELS] = true;
    c->labels_components = true;
    c->labels_filtered = false;
    c->nlabels = c->nlabels_raw;
    c->raw_stats_valid = true;      // (of the depths just read: a later write of DEPTHS clears it)
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
    MH_TRY(stage_begin(c, MHIP_STAGE_WATERSHED, s));
    ctx_wrote(c, MHIP_R_WATERSHEDS);
    if (pour) MH_TRY(pour_link_buffers(c, pour, s));
    // (out of place: the watersheds start from the label raster without a copy of it)
    MH_TRY(watersheds_dev(c->r[MHIP_R_FLOWDIR].as<uint8_t>(), c->r[MHIP_R_WATERSHEDS].as<int32_t>(), H, W, 0, s, false,
                          c->nodir_valid ? c->nodir_cnt.as<unsigned int>() : nullptr, c->r[MHIP_R_LABELS].as<int32_t>(), pour));
    MH_TRY(c->ws_counts.alloc(8 * (size_t)(c->nlabels + 1)));
    MH_TRY(label_count_dev(c->r[MHIP_R_WATERSHEDS].as<int32_t>(), n, c->nlabels, c->ws_counts.as<int64_t>(), s, W));
    MH_TRY(stage_end(c, MHIP_STAGE_WATERSHED, s));
    c->have[MHIP_R_WATERSHEDS] = true;
    c->ws_counts_valid = true;
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
    double *g = nullptr;
    if (!c->have[MHIP_R_ACCUM]) MH_TRY(ctx_noflat(c, &g));      // (the arg-min below reads the surface; in front of the stage's events)
    MH_TRY(stage_begin(c, MHIP_STAGE_POURPOINTS, s));
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
        MH_TRY(label_arg_dev(g, c->r[MHIP_R_LABELS].as<int32_t>(), H, W, c->nlabels, false, c->pour.as<mhip_index_record>(), s));
    MH_TRY(stage_end(c, MHIP_STAGE_POURPOINTS, s));
    c->pour_valid = true;
    return MHIP_OK;
}

// where the label branch of a request starts.  0: with the no-flats fill, 1: at its tail rounds, 2: after it, 3: at its finishing pass
static int label_start_env()
{
    const char *e = dev_env("MHIP_LABEL_START");
    const int v = e ? atoi(e) : LABEL_START_DEFAULT;
    return v >= 0 && v <= 3 ? v : LABEL_START_DEFAULT;
}

// Stage DAG:  FILL -> NOFLAT -> FLOWDIR -> ACCUM ------.
//                \-> LABEL ----------\-> WATERSHED ----+-> POURPOINTS
// A request that holds both sides runs the bluespot branch (LABEL, WATERSHED) on a second stream driven by a
// second host thread (both branches read back small results between launches), so the latency-bound rounds of the
// no-flats fill and the walks of the accumulation share the GPU with the labelling instead of queueing behind each
// other.  MHIP_SERIAL=1 in the environment keeps everything on the context's stream.
extern "C" int mhip_ctx_run(mhip_ctx *c, int mask)
{
    MH_ARG(c, "ctx");
    MH_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    if (!undivided(c)) {
        // row-band mode: the fills run through mhip_ctx_fill_begin/batch (halo refreshes in between); stages whose
        // cross-band protocol is not built yet are refused instead of silently computing band-local results
        MH_ARG((mask & ~(MHIP_STAGE_FLOWDIR | MHIP_STAGE_ACCUM)) == 0,
               "this stage runs through the band entry points on a row band (mhip_ctx_fill_*, mhip_ctx_band_*)");
    }
    // (development knobs are read per request: a test switches them between two requests of one process)
    const bool serial_env = [] { const char *e = dev_env("MHIP_SERIAL"); return e && e[0] == '1'; }();
    const int side_a = mask & (MHIP_STAGE_NOFLAT | MHIP_STAGE_FLOWDIR | MHIP_STAGE_ACCUM);
    const int side_b = mask & (MHIP_STAGE_LABEL | MHIP_STAGE_WATERSHED);
    const bool overlap = side_a && side_b && !serial_env;
    // FILL and NOFLAT in one request on one undivided raster: the flood may stop behind its final levels and leave the raster, the
    // depths and its proof to the first visit of the no-flats fill (common.hpp: FillHandover).  Whether that visit runs at all is
    // known only in the stage itself (the epsilons, the engine knobs): a hand-over nobody takes is completed there by the flood's
    // own last pass.
    FillHandover handover;
    FillHandover *const ho =
        ((mask & MHIP_STAGE_FILL) && (mask & MHIP_STAGE_NOFLAT) && undivided(c) && fill_handover_env()) ? &handover : nullptr;
    c->fill_handover = 0;
    // the wet bits of the hand-over (handover_addr.hpp): a buffer of this request -- from the pool, back with the request; the stages
    // that may read them run on this context, in this call, behind the visit that writes them
    c->wet_pass_used = c->wet_label_used = 0;
    DevBuf wetbuf;
    if (ho && wetbits_env() && c->H >= 3 && c->W >= 3) {
        MH_TRY(wetbuf.alloc(8 * (size_t)ho::wet_words(c->W, (int)((c->H - 2 + ho::TI - 1) / ho::TI))));
        handover.wet = wetbuf.as<unsigned long long>();
    }

    if (!overlap) {
        if (mask & MHIP_STAGE_FILL) MH_TRY(stage_fill(c, s, true, ho));
        bool fd_done = false;
        if (mask & MHIP_STAGE_NOFLAT) MH_TRY(stage_noflat(c, s, false, nullptr, (mask & MHIP_STAGE_FLOWDIR) != 0, &fd_done, ho));
        if (mask & MHIP_STAGE_FLOWDIR) MH_TRY(fd_done ? stage_flowdir_fused(c, s) : stage_flowdir(c, s));
        if (mask & MHIP_STAGE_ACCUM) MH_TRY(stage_accum(c, s));
        if (mask & MHIP_STAGE_LABEL) MH_TRY(stage_label(c, s, ho));
        if (mask & MHIP_STAGE_WATERSHED) MH_TRY(stage_watershed(c, s));
        if (mask & MHIP_STAGE_POURPOINTS) MH_TRY(stage_pourpoints(c, s));
        return MHIP_OK;
    }

    // events and the side streams are created here, on the calling thread, before the side thread starts
    StageTimer *t;
    for (int st : {MHIP_STAGE_FILL, MHIP_STAGE_NOFLAT, MHIP_STAGE_FLOWDIR, MHIP_STAGE_ACCUM, MHIP_STAGE_LABEL, MHIP_STAGE_WATERSHED,
                   MHIP_STAGE_POURPOINTS})
        if (mask & st) MH_TRY(ctx_timer(c, st, &t));
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
    MH_TRY(ctx_fork_join_events(c));
    if (!c->ev_cand) MH_HIP(hipEventCreateWithFlags(&c->ev_cand, hipEventDisableTiming));
    if (!c->ev_prep) MH_HIP(hipEventCreateWithFlags(&c->ev_prep, hipEventDisableTiming));
    hipStream_t sb = c->stream_b;
    const bool do_fill = (mask & MHIP_STAGE_FILL) != 0;
    MH_ARG(c->have[MHIP_R_DEM] || !(mask & (MHIP_STAGE_FILL | MHIP_STAGE_NOFLAT)), "FILL / NOFLAT need the DEM");

    // hand-overs between the two host threads (each value is an error code)
    std::promise<int> fill_done, shdg_done, flowdir_ready, label_ready, tail_reached;
    std::future<int> fill_fut = fill_done.get_future(), shdg_fut = shdg_done.get_future(), tail_fut = tail_reached.get_future();
    // The label branch does not start with the no-flats fill but at its end (ev_tail).  Measured at 16384^2 (ms per step): label
    // next to the whole no-flats fill 38.0 (the fill's rounds 14.6 instead of 9.8: every one of its ~85 small launches queues behind
    // the labelling's long workgroups), from the fill's latency-bound tail rounds on 37.4, behind the fill 36.7 -- then labelling and
    // watersheds run next to D8 + accumulation.  MHIP_LABEL_START = 0 / 1 / 2 / 3 selects (development knob).  3: at the fill's
    // finishing pass (GeoRun::end) -- one launch, no LDS: the default since round 5 (21.87 -> 21.51 ms per step; DESIGN 4.5 has the
    // table, and the terrain on which 2 is the better choice).  Engines without such a pass fire behind the stage, like 2.
    struct TailCtx {
        mhip_ctx *c;
        std::promise<int> *p;
        FillHandover *ho;
    } tail_ctx{c, &tail_reached, ho};
    StageHook tail_hook;
    tail_hook.arg = &tail_ctx;
    tail_hook.fn = [](void *arg, hipStream_t st) {
        TailCtx *t = static_cast<TailCtx *>(arg);
        ctx_handover_settled(t->c, t->ho);      // (the other thread reads have[DEPTHS] behind this event)
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
    // The accumulation's node buffer and its clears depend on the raster's shape alone.  Behind the finishing pass they sat between
    // its read-back and accum_tile_kernel, on the critical branch of the tail (0.2 ms at 16384^2); queued when the main thread turns
    // to the no-flats stage, on the stream the watersheds will use much later, the clear is through before the stage's first visit
    // starts (29 us: DESIGN 7.0000).  A request that never reaches the accumulation hands the buffer back when `acc_prep` goes.
    AccumPrep acc_prep;
    const bool prep_accum = (mask & MHIP_STAGE_ACCUM) && (mask & (MHIP_STAGE_NOFLAT | MHIP_STAGE_FLOWDIR)) && !c->ht && !c->hb;
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
            if (rc_l == MHIP_OK && (mask & MHIP_STAGE_LABEL)) rc_l = stage_label(c, sb, ho);   // incl. the bluespot depths
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
    if (do_fill) rc_a = stage_fill(c, s, /*with_depths=*/false, ho);
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
        if (prep_accum) MH_TRY(accum_prepare_dev(&acc_prep, c->H, c->W, c->stream_c, c->ev_prep));
        const int label_start = label_start_env();
        // (0 with a hand-over pending: the depths the label branch reads are written by the stage's first visit -- the hook fires behind it)
        const bool owed = ho && ho->pending;
        if (label_start == 0 && !owed) tail_hook.fire(s);
        tail_hook.at = label_start;
        const bool armed = label_start == StageHook::TAIL_ROUNDS || label_start == StageHook::FINISH || (label_start == StageHook::FIRST_VISIT && owed);
        bool fd_done = false;
        if (mask & MHIP_STAGE_NOFLAT)
            MH_TRY(stage_noflat(c, s, /*shdg_done=*/true, armed ? &tail_hook : nullptr, (mask & MHIP_STAGE_FLOWDIR) != 0, &fd_done, ho));
        if (mask & MHIP_STAGE_FLOWDIR) {
            MH_TRY(fd_done ? stage_flowdir_fused(c, s) : stage_flowdir(c, s));
            MH_HIP(hipEventRecord(c->ev_flowdir, s));
        }
        return MHIP_OK;
    }();
    tail_hook.fire(s);                    // (no NOFLAT in the mask, or it failed early: the other thread is never left waiting)
    flowdir_ready.set_value(rc_a);
    if (rc_a == MHIP_OK && (mask & MHIP_STAGE_ACCUM)) rc_a = stage_accum(c, s, pour, &acc_prep);
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
