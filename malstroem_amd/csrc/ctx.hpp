// ctx.hpp -- the device-resident context behind the mhip_ctx_* entry points (DemTool / BluespotTool pipeline, reference dem.py:53-93,
// bluespots.py:138-216), shared by ctx.hip (life cycle, transfers, getters, records, hypsometry), ctx_run.hip (the stage DAG of
// mhip_ctx_run) and ctx_band.hip (the row-band protocol).
//   ctx_wrote   ctx.hip   what a write of a resident raster invalidates: every writer calls it
//   ctx_held    ctx.hip   whether a raster held outside mhip_raster is valid, and where it is: every reader calls it
// What each held product is made from is held_rules.hpp; the context keeps one record per product, one lock and one drop (ctx.hip).
#pragma once
#include <atomic>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>

#include "common.hpp"
#include "held_rules.hpp"

namespace mh {

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

// HIP-event pair around a stage (or around one kernel: mhip_ctx_kernel_ms).  One per slot, the events created on first use; the two
// host threads of mhip_ctx_run touch different slots.
struct StageTimer {
    hipEvent_t a = nullptr, b = nullptr;
    bool valid = false;     // the pair brackets a run that has been queued
};
constexpr int N_STAGE_BITS = 9;                                                           // MHIP_STAGE_FILL .. MHIP_STAGE_FINALDEPTHS
constexpr int WETAT_KERNEL_SLOT = 1 << 27, FINAL_KERNEL_SLOT = 1 << 28, HYPS_KERNEL_SLOT = 1 << 29, D8_STEADY_SLOT = 1 << 30;     // event pairs of single kernels
constexpr int N_TIMERS = N_STAGE_BITS + 4;

}  // namespace mh

struct mhip_ctx {
    mh::SideThread side;    // drives the label branch of mhip_ctx_run
    int64_t H = 0, W = 0;   // local raster: owned rows + halo rows
    int64_t H_global = 0, row0 = 0, H_owned = 0;
    int ht = 0, hb = 0;     // 1 if a halo row (copy of the neighbouring band's edge row) sits above / below the owned rows
    mh::FillRun *run[2] = {nullptr, nullptr};   // resumable fill (plain, no-flats) in band mode
    mh::GeoRun *geo = nullptr;                  // ... and the geodesic no-flats fill
    uint32_t pf_overflow = 0;                   // the capacities that sent this band's flood to the iterative schedule (fill_begin / fill_batch)
    mh::PfRun *pf = nullptr;                    // ... and the tiled priority-flood (plain fill)
    bool pf_done = false;                   // the flood's raster is written and proven (mhip_ctx_fill_certify); run[0] may follow it
    mh::DevBuf nodir_cnt;                   // interior NODIR cells of FLOWDIR, counted by the D8 kernel (the watersheds' fast-path test)
    bool nodir_valid = false;
    bool flowdir_own = false;               // FLOWDIR is the library's own D8 (edges outward, no cycles, no sinks), not an upload: ctx_get_i64 "flowdir_computed"
    int device = 0, rank = 0, nranks = 1;
    hipStream_t stream = nullptr;
    mh::DevBuf r[MHIP_R_COUNT_];
    bool have[MHIP_R_COUNT_] = {};
    // NOFLAT is resident (have[] says so) but not written: it is noflat_assemble_dev(FILLED, NGDIST), the surface the finishing pass
    // of the last chain request checked and did not store (ctx_run.hip: stage_noflat).  ctx_noflat() is the only
    // way to the raster's memory
    bool noflat_pending = false;
    mh::DevBuf tmp_i32;     // CCL parent scratch
    mh::CclKeep ccl_keep;   // a row band's labelling between its two halves (mhip_ctx_band_ccl_begin / _finish)
    bool ccl_pending = false;
    bool pf_depths = false;  // the band flood's last pass (mhip_ctx_fill_certify) wrote the depths of the owned rows
    mh::DevBuf raw_stats, stats, ws_counts, pour;
    mh::AccumKeep acc_keep; // row band: the perimeter graph of mhip_ctx_band_accum_boundary, for the ACCUM run that follows the exchange
    int accum_algorithm = 0;   // 0: full accumulation, 1: the band's second pass as a delta over the kept graph
    mh::DevBuf pp_mask0, pp_list, pp_tiles, pp_misc, pp_key;    // pour-point candidates on their way from the watersheds to the accumulation (PourLink)
    hipEvent_t ev_cand = nullptr;
    hipEvent_t ev_prep = nullptr;   // behind the clears of the accumulation's node buffer, queued ahead of the stage (mhip_ctx_run: AccumPrep)
    int pour_algorithm = 0;
    int64_t nlabels_raw = -1, nlabels = -1;
    bool labels_components = false;   // LABELS came from the library's own labelling (not uploaded): 8-connected components
    bool labels_filtered = false;
    // The three record sets describe the resident rasters they were computed from: set by the code that computes them, cleared by
    // ctx_wrote, tested by every reader.  (Atomic: both host threads of a request clear `pour_valid`, one for ACCUM, one for LABELS.)
    std::atomic<bool> stats_valid{false};       // `stats`: label_stats of DEPTHS by LABELS
    std::atomic<bool> raw_stats_valid{false};   // `raw_stats`: label_stats of DEPTHS by the raw labels, set by the LABEL stage; a relabelling (mhip_ctx_apply_keep) keeps it
    std::atomic<bool> ws_counts_valid{false};   // `ws_counts`: label_count of WATERSHEDS
    std::atomic<bool> pour_valid{false};        // `pour`: arg-max of ACCUM (arg-min of NOFLAT) by LABELS
    // hypsometry of the resident labels (mhip_ctx_hyps): layout, table, and the records of the last mhip_ctx_final_depths
    mh::DevBuf hyps_off, hyps_cnt, hyps_sum, hyps_rec;
    int64_t hyps_total = -1, hyps_spills = 0;     // -1: no table of the resident depths and labels
    // the held products (held_rules.hpp: what each is made from), indexed by mh::HeldProduct.  state: -1 none, >= 0 held -- the value
    // mhip_ctx_get_i64 reports: the events of wet_at, the unresolved cells of the flow distance and the travel time, the undrained cells
    // of hand, the reaches, the zones, the cells the sea reached, 1 for the inundation and the sea's depths and classes.  made_from: the
    // rasters whose write drops it, set by the call that made it.  buf: its rasters (H x W, 4 bytes a cell; no members of
    // mhip_raster), records and table, as ctx.hip's HELD table and the entry points name them.  The two host threads of a request may
    // write rasters at the same time: every change of a state and every release happens under held_mu, and held_mask -- the union of
    // the live products' made_from -- lets a write that meets none of them pass without the lock
    struct Held {
        std::atomic<int64_t> state{-1};
        uint32_t made_from = 0;
        mh::DevBuf buf[3];
    } held[mh::HP_COUNT_];
    std::mutex held_mu;
    std::atomic<uint32_t> held_mask{0};
    // what a later call needs from the one that made a product: the travel time's clipped cells and the bins of its table (0: no table);
    // what mhip_ctx_inundate compares and uses of the hand and the reach catchments; the sea flood's max_level, nodata and counters
    int64_t tt_saturated = -1, tt_bins = 0;
    double hand_thr = 0, rcatch_thr = 0;
    bool hand_labels = false, rcatch_labels = false;
    float hand_nodata = 0;
    float sea_max_level = 0, sea_nodata = 0;
    mh::SeaStats sea_st;
    double sh = 0, dg = 0;
    int32_t fill_rounds = 0, noflat_rounds = 0;
    int64_t fill_handover_rechecks = 0;   // requests of this context whose fused visit failed the proof and went through the flood's own last pass
    int32_t fill_handover = 0;      // the last request's no-flats fill took the flood's last pass and proof into its first visit (ctx_run.hip)
    // the last request read that visit's wet bits instead of floats: the finishing pass (the DEM), the labelling (the depths) -- a
    // word each: the two are set by the two host threads of a request
    int32_t wet_pass_used = 0, wet_label_used = 0;
    mh::FillStats fill_st, noflat_st;
    mh::StageTimer timers[mh::N_TIMERS];
    void *comm = nullptr;   // RCCL communicator over all bands (comm.hip); nullptr: the launcher moves the rows
    void *comm_b = nullptr; // a second one for the thread between mhip_ctx_side_begin / _end (two threads never share a communicator)
    mh::DevBuf comm_stage, comm_word, comm_flags, comm_stage_b;
    // second stream + fork/join events of the stage DAG (mhip_ctx_run)
    hipStream_t stream_b = nullptr, stream_c = nullptr;
    hipEvent_t ev_fork = nullptr, ev_flowdir = nullptr, ev_join = nullptr, ev_label = nullptr, ev_tail = nullptr;
};

namespace mh {

// no row band: no halo row, and not one of several ranks (a rank may own every row and still be one of several)
inline bool undivided(const mhip_ctx *c) { return !(c->nranks > 1 || c->ht || c->hb); }

inline size_t raster_elem(int which)
{
    switch (which) {
    case MHIP_R_DEM: case MHIP_R_FILLED: case MHIP_R_DEPTHS: case MHIP_R_LABELS: case MHIP_R_WATERSHEDS: case MHIP_R_NGDIST:
    case MHIP_R_FINALDEPTHS: return 4;
    case MHIP_R_NOFLAT: case MHIP_R_ACCUM: return 8;
    case MHIP_R_FLOWDIR: return 1;
    default: return 0;
    }
}

inline int ctx_raster(mhip_ctx *c, int which)
{
    if (!c->r[which].p) MH_TRY(c->r[which].alloc(raster_elem(which) * (size_t)(c->H * c->W)));
    return MHIP_OK;
}

// ---- stage timers ----------------------------------------------------------------------------------------------------------
inline int timer_slot(int stage)      // -1: neither one stage bit nor a single-kernel slot
{
    for (int b = 0; b < N_STAGE_BITS; ++b)
        if (stage == 1 << b) return b;
    return stage == FINAL_KERNEL_SLOT ? N_STAGE_BITS : stage == HYPS_KERNEL_SLOT ? N_STAGE_BITS + 1 : stage == D8_STEADY_SLOT ? N_STAGE_BITS + 2 :
           stage == WETAT_KERNEL_SLOT ? N_STAGE_BITS + 3 : -1;
}
inline int ctx_timer(mhip_ctx *c, int stage, StageTimer **t)
{
    const int k = timer_slot(stage);
    MH_ARG(k >= 0, "not a stage");
    *t = &c->timers[k];
    if (!(*t)->a) {
        hipEvent_t e0, e1;
        MH_HIP(hipEventCreate(&e0));
        MH_HIP(hipEventCreate(&e1));
        (*t)->a = e0;
        (*t)->b = e1;
    }
    return MHIP_OK;
}
// each stage runs on the stream it is given and brackets itself with its pair of events
inline int stage_begin(mhip_ctx *c, int stage, hipStream_t s)
{
    StageTimer *t;
    MH_TRY(ctx_timer(c, stage, &t));
    MH_HIP(hipEventRecord(t->a, s));
    return MHIP_OK;
}
inline int stage_end(mhip_ctx *c, int stage, hipStream_t s)      // follows stage_begin
{
    StageTimer &t = c->timers[timer_slot(stage)];
    MH_HIP(hipEventRecord(t.b, s));
    t.valid = true;
    return MHIP_OK;
}

// Band launcher with two host threads (distributed.BandPipeline.run_chain): the thread that drives the labelling branch
// brackets its calls with mhip_ctx_side_begin / _end; in between, the data-movement and band entry points it calls run on
// the context's side stream, next to the fills the main thread keeps launching on the main stream.
inline thread_local mhip_ctx *t_side_ctx = nullptr;
static inline hipStream_t cs(mhip_ctx *c) { return (t_side_ctx == c && c->stream_b) ? c->stream_b : c->stream; }
// ... and every RCCL call of that thread goes over the context's SECOND communicator (mhip_ctx_comm_add_side): the order of the
// operations on one communicator must be the same on every rank, which two threads sharing one cannot promise
static inline bool on_side(mhip_ctx *c) { return t_side_ctx == c; }

// ---- "raster `which` was (re)written" (ctx.hip; the table is DESIGN.md 4.5a) ---------------------------------------------------
// Every writer of a resident raster calls this BEFORE it records what it knows about the new content: it clears everything that
// was derived from the old content.  Host-only flag work.  uploaded: the content comes from outside (an uploaded FILLED surface
// has no flood of this context behind it).
void ctx_wrote(mhip_ctx *c, int which, bool uploaded = false);
// ---- the no-flats surface, wherever it is read (ctx.hip) --------------------------------------------------------------------------
// The one way to c->r[MHIP_R_NOFLAT]: a surface that is pending is written first, on the context's stream (a caller on another
// stream finds it complete), and is pending no more.  Call it before a stage's event bracket opens.
int ctx_noflat(mhip_ctx *c, double **g = nullptr);
// ... and in front of whatever touches raster `which` from outside the stages: a read of NOFLAT, or a write (`write`) of NOFLAT or of
// the two rasters a pending surface is made of -- FILLED and NGDIST -- other than the context's own fill of the same DEM
inline int ctx_settle(mhip_ctx *c, int which, bool write)
{
    if (which == MHIP_R_NOFLAT || (write && (which == MHIP_R_FILLED || which == MHIP_R_NGDIST))) return ctx_noflat(c);
    return MHIP_OK;
}
// ---- the two ways data crosses between the host and a context (ctx.hip) -----------------------------------------------------------
// Rows [row0, row0 + nrows) of the OWNED rows of `dev_base`, a device array of the local raster's full-width rows (halo rows
// included) of `elem_bytes` per cell, to or from `host` by `kind`: one copy on cs(c), then one synchronisation.  The caller has
// checked the window against H_owned.  Every whole-raster and windowed transfer of ctx.hip is this call.
int ctx_copy_rows(mhip_ctx *c, void *dev_base, size_t elem_bytes, int64_t row0, int64_t nrows, void *host, hipMemcpyKind kind);
// ---- the rasters a context holds outside mhip_raster, wherever they are read (ctx.hip) ------------------------------------------
// wet_at, flow distance, hand and the distance to the drainage, reach catchments, inundation depths, zones, travel time, the sea flood's
// levels, depths and classes: each is a buffer of a held product (mhip_ctx::held), valid while the product's state says so.  ctx_held
// is the one test "is it held, and where": MHIP_EINVAL with the message of that raster's mhip_ctx_*_rows getter, or the device
// pointer and (optional) the bytes of an element.
enum HeldRaster { HELD_WETAT, HELD_FLOWDIST, HELD_HAND, HELD_DRAINDIST, HELD_REACHCATCH, HELD_INUNDATION, HELD_ZONES, HELD_TRAVELTIME, HELD_SEALEVEL, HELD_SEADEPTH,
                  HELD_SEACLASS, HELD_COUNT_ };
int ctx_held(mhip_ctx *c, int id, void **ptr, size_t *elem_bytes = nullptr);
// `bytes` of a record buffer to `host` on the main stream, synchronised: every record getter after its validity test
int ctx_fetch(mhip_ctx *c, const DevBuf &buf, size_t bytes, void *host);
// the fork / join events of the two branches (mhip_ctx_side_begin, mhip_ctx_run), created once
int ctx_fork_join_events(mhip_ctx *c);
// the label filter and what follows a LABELS write lazily (mhip_ctx_apply_keep; the stages that want final labels)
int ctx_apply_keep_on(mhip_ctx *c, const uint8_t *keep, hipStream_t s);
int ctx_ensure_labels_final(mhip_ctx *c, hipStream_t s);
int ctx_label_max(mhip_ctx *c, hipStream_t s);

}  // namespace mh
