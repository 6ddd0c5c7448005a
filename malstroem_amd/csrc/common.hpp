// common.hpp -- shared host/device helpers of libmalstroem_hip (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/malstroem_hip.h"

struct mhip_polygons;
struct mhip_flowpaths;
struct mhip_wacc;

namespace mh {

// ---- error plumbing --------------------------------------------------------------------------
void set_error(const char *fmt, ...);
const char *get_error();
// Development knobs and test hooks (engine selection for A/B runs, debug prints, fault injection for the liveness tests of the
// run-time checks) are read ONLY when MHIP_DEVELOPER=1 is set: a stray variable in a user's environment never steers the product.
const char *dev_env(const char *name);
// hipStreamSynchronize with a short busy wait first: the round loops of the fills read a few words back every 16-32 launches and
// the device idles while a sleeping host thread is woken (30-50 us per read-back; MALSTROEM_HIP_SPIN_US=0 turns the busy wait off)
hipError_t stream_sync(hipStream_t s);
int require_device();   // MHIP_ENODEV without a HIP device: there is no CPU fallback

#define MH_HIP(expr)                                                                             \
    do {                                                                                         \
        hipError_t _e = (expr);                                                                  \
        if (_e != hipSuccess) {                                                                  \
            mh::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return MHIP_EHIP;                                                                    \
        }                                                                                        \
    } while (0)

#define MH_TRY(expr)                \
    do {                            \
        int _rc = (expr);           \
        if (_rc != MHIP_OK) return _rc; \
    } while (0)

#define MH_ARG(cond, msg)                   \
    do {                                    \
        if (!(cond)) {                      \
            mh::set_error("invalid argument: %s", msg); \
            return MHIP_EINVAL;             \
        }                                   \
    } while (0)

// ---- device scratch buffer (RAII, stream-ordered free is not needed: all work is on one stream and
//      we synchronise before releasing) ------------------------------------------------------------
// Blocks come from a small caching pool (runtime.hip) so that the iterative stages and repeated pipeline runs do
// not pay hipMalloc/hipFree (the latter synchronises the device) inside the hot path.
int pool_alloc(void **p, size_t bytes);
void pool_free(void *p, size_t bytes);

struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    int alloc(size_t n)
    {
        if (n == 0) n = 16;
        if (p && bytes >= n && bytes <= 2 * n + 4096) return MHIP_OK;  // reuse what we already hold
        release();
        MH_TRY(pool_alloc(&p, n));
        bytes = n;
        return MHIP_OK;
    }
    void release()
    {
        if (p) pool_free(p, bytes);
        p = nullptr;
        bytes = 0;
    }
    template <typename T> T *as() const { return reinterpret_cast<T *>(p); }
};

// ---- host-layer helpers shared by the entry points (runtime.hip, api.hip, ctx*.hip) -------------------------------------
int upload(DevBuf &b, const void *host, size_t bytes, hipStream_t s);           // alloc + asynchronous copy
int download(void *host, const DevBuf &b, size_t bytes, hipStream_t s);         // copy + synchronise
int64_t build_rank_lut(const uint8_t *keep, int64_t nlab, std::vector<int32_t> &lut);
inline bool hyps_res_ok(double res) { return res > 0.0 && res <= 1.7976931348623157e308; }   // (false for NaN)
// api.hip: the stream walk for a batch of cells over two rasters on the device (mhip_trace_downstream_i32, mhip_ctx_trace_downstream)
int trace_on_device(const uint8_t *d_fd, const int32_t *d_lab, int64_t H, int64_t W, const int64_t *cells_rc, int64_t n, int use_bg,
                    int32_t bg, int32_t *out_label, int32_t *out_found, int64_t *out_len, const int64_t *offsets, int64_t *out_cells,
                    hipStream_t s);

// ---- AGNPS direction codes (reference flow.py:30-38, deltas _flow.pyx:36-46) -------------------
// code k: U 0, UR 1, R 2, DR 3, D 4, DL 5, L 6, UL 7, NODIR 8
__host__ __device__ inline int dir_dr(int k) { return (k == 0 || k == 1 || k == 7) ? -1 : (k >= 3 && k <= 5) ? 1 : 0; }
__host__ __device__ inline int dir_dc(int k) { return (k >= 1 && k <= 3) ? 1 : (k >= 5 && k <= 7) ? -1 : 0; }

// ---- D8 of one cell (d8.hip; noflat_geo.hip: ng_finish_kernel) ------------------------------------------------------------
__device__ __forceinline__ unsigned d8_code(double z, double u, double ur, double r, double dr, double d, double dl,
                                            double l, double ul)
{
    const double INV_SQRT2 = 0.7071067811865475;  // 1 / 2**0.5, _flow.pyx:93-94
    // `if dz > dzmax: dzmax = dz; i = k` in the reference's order.  The running maximum is a v_max_f64 (same value as the
    // conditional move: it only changes when dz > dzmax; NaN drops are ignored by both), the index a 32-bit select.
    unsigned i = 8;
    double dzmax = 0.0, dz;
#define MH_D8_STEP(expr, k)          \
    dz = (expr);                     \
    i = dz > dzmax ? (k) : i;        \
    dzmax = fmax(dzmax, dz);
    MH_D8_STEP(__dsub_rn(z, u), 0u)
    MH_D8_STEP(__dmul_rn(__dsub_rn(z, ur), INV_SQRT2), 1u)
    MH_D8_STEP(__dsub_rn(z, r), 2u)
    MH_D8_STEP(__dmul_rn(__dsub_rn(z, dr), INV_SQRT2), 3u)
    MH_D8_STEP(__dsub_rn(z, d), 4u)
    MH_D8_STEP(__dmul_rn(__dsub_rn(z, dl), INV_SQRT2), 5u)
    MH_D8_STEP(__dsub_rn(z, l), 6u)
    MH_D8_STEP(__dmul_rn(__dsub_rn(z, ul), INV_SQRT2), 7u)
#undef MH_D8_STEP
    return i;
}

// flow.py:130-139: rows first, then columns overwrite, corners last (same order => same result on 1-wide rasters)
__device__ __forceinline__ unsigned edge_code(int64_t r, int64_t c, int64_t maxr, int64_t maxc)
{
    unsigned code = 8;
    if (r == 0) code = 0;
    if (r == maxr) code = 4;
    if (c == 0) code = 6;
    if (c == maxc) code = 2;
    if (r == 0 && c == 0) code = 7;
    if (r == 0 && c == maxc) code = 1;
    if (r == maxr && c == 0) code = 5;
    if (r == maxr && c == maxc) code = 3;
    return code;
}

// monotone float/double <-> unsigned keys (for atomicMin/Max); NaN must be filtered by the caller
__host__ __device__ inline uint32_t f32_key(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ inline float key_f32(uint32_t k)
{
    uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    float f;
    memcpy(&f, &u, 4);
    return f;
}
// the flood's key of an elevation (pflood.hip; the fused first visit of noflat_geo.hip computes the same surface from it)
__device__ __forceinline__ uint32_t dem_key(float v)
{
    if (v != v) return f32_key(__builtin_inff());   // a NaN cell never wins a comparison (_fill.pyx:22): like +inf
    return f32_key(v + 0.0f);                        // -0.0 -> +0.0: the two compare equal in the reference
}
__host__ __device__ inline uint64_t f64_key(double f)
{
    uint64_t u;
    memcpy(&u, &f, 8);
    return (u & 0x8000000000000000ull) ? ~u : (u | 0x8000000000000000ull);
}
__host__ __device__ inline double key_f64(uint64_t k)
{
    uint64_t u = (k & 0x8000000000000000ull) ? (k & 0x7fffffffffffffffull) : ~k;
    double f;
    memcpy(&f, &u, 8);
    return f;
}

// ---- device-pointer stage implementations (one translation unit per stage) --------------------
struct FillStats {
    int32_t rounds = 0;   // kernel launches (tile rounds)
    int64_t visits = 0;   // tile visits over all rounds
    int64_t cycles = 0;   // local (down, up, right, left) cycles over all visits
    int64_t tiles = 0;    // tiles in the raster
    float hot_ms = 0;     // device time of the stage's dominant kernel, HIP events around its launches: pf_tile_kernel (one launch) /
    int32_t hot_launches = 0;   // the ng_round_kernel launches (the span of the round loop: compaction launches and gaps included)
    int32_t algorithm = 0;  // 0: iterative tile schedule (fill.hip), 1: tiled priority-flood (pflood.hip; rounds = kernel launches),
                            // 2: integer geodesic transform (noflat_geo.hip)
    uint32_t overflow = 0;  // plain fill: the capacities that gave out in the last attempt of the priority-flood (pflood.hip: PF_OV_*); 0: it
                            // ran through, or was not tried
    // the priority-flood reads every DEM cell anyway: smallest / largest elevation of the local raster and "holds a NaN" ride along
    bool have_minmax = false, dem_nan = false;
    float dem_min = 0.0f, dem_max = 0.0f;
    // why the integer geodesic transform handed a raster back to the float64 relaxation (diagnostics: ctx_get_int "noflat_reject*"):
    // 0 it did not, 1 not applicable (irregular levels / NaN cells / epsilons without weights), 2 its final check failed
    int32_t geo_reject = 0;
    int64_t geo_irregular = 0, geo_unreached = 0, geo_mismatch = 0;
    // the geodesic transform's rounds: what a visit stored (0 every row of its tile, 1 the six-row blocks in which a cell moved) and
    // the rows of distances that came to, over all visits behind the first
    int32_t rowstore = 0;
    int64_t rows_stored = 0;
};

// fill.hip
// Resumable fill run (row-band mode interleaves halo refreshes between batches of rounds).
struct FillRun {
    bool noflat = false;
    const float *dem = nullptr;
    void *out = nullptr;            // float* (plain) or double* (no-flats)
    int64_t H = 0, W = 0;           // local raster (band + halo rows)
    double sh = 0, dg = 0;
    const float *seed = nullptr;    // plain-filled surface: no-flats upper-bound start (see fill_noflat_dev)
    double seed_add = 0;
    int fixed_top = 0, fixed_bot = 0;  // local row 0 / H-1 is a halo row owned by the neighbouring band
    int rounds_per_batch = 8;          // rounds launched between two host checks (a band exchanges its halo rows after each batch)
    bool attach_only = false;          // (internal: attach() is begin() without the initialising round)
    struct Impl;
    Impl *impl;
    FillRun();
    ~FillRun();
    FillRun(const FillRun &) = delete;
    FillRun &operator=(const FillRun &) = delete;
    int begin(hipStream_t s, bool *active);      // initialising round over every tile
    int batch(hipStream_t s, bool *active);      // a batch of rounds; *active == false: locally converged
    int activate_row(int side, hipStream_t s);   // halo row `side` (0 top, 1 bottom) changed: revisit its tile row
    int attach(hipStream_t s);                   // instead of begin(): `out` already holds an upper bound of the fixed point
    int certify(hipStream_t s, bool *changed);   // one sweep over EVERY tile, iterated to local convergence; *changed: a tile moved
    int finish(hipStream_t s, FillStats *st);
};
void noflat_seed(FillRun &f, const float *d_filled, double sh, double dg, int64_t ncells_global);
// The hand-over of the flood's last pass to the no-flats fill's first visit (one request holds both: mhip_ctx_run).  The flood
// stops behind pf_final_kernel and keeps its workspace: `pending`.  The geodesic transform's first visit (noflat_geo.hip:
// ng_handover_kernel) then computes F of every window from dem + basin slots + final levels, writes `filled` and `depths` and
// evaluates the flood's proof on the way: `queued`; the workspace goes back to the pool behind the stream sync of GeoRun::begin,
// which reads the proof flag with its own counters.  A failed proof there (`suspect`) keeps the workspace: like a transform that
// does not run at all it leaves `pending` set, and fill_handover_complete() -- the flood's own last pass and proof, late -- writes
// and decides; a surface that fails there too (`violated`) is an upper bound: fill_handover_repair().
struct PfRun;
struct FillHandover {
    PfRun *run = nullptr;               // owns the flood's workspace while pending
    const float *dem = nullptr;
    float *filled = nullptr, *depths = nullptr;
    int64_t H = 0, W = 0;
    const uint16_t *bslot = nullptr;    // device pointers into the flood's workspace
    const uint32_t *tabV = nullptr;
    int ntr = 0, ntc = 0;
    bool pending = false, queued = false, violated = false, repaired = false;
    bool suspect = false;               // the proof failed in the fused visit: the flood's own last pass decides (and is what ran last)
    // The wet bits (handover_addr.hpp: wet_index): the caller's buffer of wet_words() words, or null.  The fused visit writes its
    // proof bits "filled > dem" there; `wet_ok` once that visit's proof has passed: for the rest of THIS request the bits stand for
    // the comparison at every cell (a finite DEM: the caller's business), and for "depths != 0"
    unsigned long long *wet = nullptr;
    bool wet_ok = false;
    bool wet_pass = false;              // the no-flats fill's finishing pass read them instead of the DEM
    FillStats st_repair;                // the relaxation that repaired a surface whose proof failed
    FillHandover() = default;
    FillHandover(const FillHandover &) = delete;
    FillHandover &operator=(const FillHandover &) = delete;
    ~FillHandover();
    void release();                     // the flood's workspace goes back to the pool (the stream has been synchronised)
};
int fill_handover_complete(FillHandover *ho, hipStream_t s);   // pflood.hip + fill.hip: K4 and the proof as PfRun::finish runs them; repairs
int fill_handover_repair(FillHandover *ho, hipStream_t s);     // fill.hip: FillRun::attach + certify on `filled`, then the depths
// ho (optional): the flood may stop behind pf_final_kernel (ho->pending; *depths_done is set: the pass that writes them is owed)
int fill_plain_dev(const float *d_dem, float *d_out, int64_t H, int64_t W, hipStream_t s, FillStats *st, float *d_depths = nullptr,
                   bool *depths_done = nullptr, FillHandover *ho = nullptr);
// check.hip: *d_flag (zeroed by the caller) = 1 when `filled` is not a fixed point of the plain fill with border == dem
int fill_check_f32_dev(const float *d_dem, const float *d_filled, int64_t H, int64_t W, int fixed_top, int fixed_bot, hipStream_t s,
                       unsigned int *d_flag);
// pflood.hip
int fill_plain_pflood_dev(const float *d_dem, float *d_out, float *d_depths, int64_t H, int64_t W, hipStream_t s, FillStats *st, bool *violated = nullptr,
                          uint32_t *overflow = nullptr, FillHandover *ho = nullptr);
// pflood.hip: the exact tiled priority-flood, resumable for row bands (whose halo rows of `out` carry the neighbours' current
// estimates of their filled edge rows; this band's own edge rows in `out` are kept current for them)
struct PfRun {
    const float *dem = nullptr;
    float *out = nullptr;            // the filled surface
    int64_t H = 0, W = 0;
    int fixed_top = 0, fixed_bot = 0;
    uint32_t overflow = 0;           // the capacities that gave out (the flags word as the last solve read it); begin / batch then return MHIP_ELIMIT
    struct Impl;
    Impl *impl;
    PfRun();
    ~PfRun();
    PfRun(const PfRun &) = delete;
    PfRun &operator=(const PfRun &) = delete;
    int begin(hipStream_t s);                     // MHIP_ELIMIT: not applicable (capacity, band alignment): run the iterative schedule
    int halo_changed(int side, hipStream_t s);
    int batch(hipStream_t s);                     // MHIP_ELIMIT as above
    // writes the raster, then proves it (check.hip); *violated: the surface is not the fixed point (it still is an upper bound of
    // it): the caller lets the iterative schedule finish the job (FillRun::attach + certify)
    // ho: the deferred form -- pf_final_kernel only, the workspace is kept and *ho points into it (ho->pending); finish_late() is
    // the rest of finish() for a hand-over nobody took
    int finish(hipStream_t s, float *d_depths, FillStats *st, bool *violated = nullptr, FillHandover *ho = nullptr);
    int finish_late(hipStream_t s, float *d_depths, bool *violated);
    int proof_flag(hipStream_t s, unsigned int *h_flag);      // reads the proof's flag back (synchronises)
    int solve(hipStream_t s);
    int pack(hipStream_t s, int row0, int nrows);
    int publish_edges(hipStream_t s);
};
// a call-back fired once, on the stage's stream, at a chosen point of a stage (mhip_ctx_run starts the label branch when the
// no-flats fill has left its throughput-bound first rounds: see ctx_run.hip)
struct StageHook {
    enum Point { FIRST_VISIT = 0, TAIL_ROUNDS = 1, FINISH = 3 };      // (the values of MHIP_LABEL_START that arm a hook; 0 only with a hand-over: behind the visit that writes the depths)
    void (*fn)(void *, hipStream_t) = nullptr;
    void *arg = nullptr;
    bool fired = false;
    int at = TAIL_ROUNDS;           // the point of the no-flats fill the hook is armed for
    void fire(hipStream_t s)
    {
        if (fn && !fired) {
            fired = true;
            fn(arg, s);
        }
    }
    void fire_at(int point, hipStream_t s)      // from inside a stage: only the point the hook was armed for fires it
    {
        if (point == at) fire(s);
    }
};

// noflat_geo.hip: the no-flats fill as an integer geodesic distance transform; resumable for row bands
struct GeoRun {
    const float *dem = nullptr, *filled = nullptr;   // local raster incl. halo rows; `filled` = the converged plain fill
    double *out = nullptr;                            // the no-flats surface (written by end())
    uint32_t *dist = nullptr;                         // distances, H * W (nullptr: kept in the run's own workspace)
    int64_t H = 0, W = 0;
    double sh = 0, dg = 0;
    int fixed_top = 0, fixed_bot = 0;
    bool allow_partial = false;                       // flats of irregular levels: leave them to the caller (else: not applicable)
    double seed_add = 0;                              // ... with the upper bound F + seed_add in `out`
    bool partial = false;                             // set by end(): `out` still needs the float64 relaxation on those flats
    StageHook *tail_hook = nullptr;                   // fired where it is armed for: behind the first batch of rounds (batch), or in front of the finishing pass (end)
    uint8_t *d8_out = nullptr;                        // optional: end() also writes the flow directions of the surface (one context, no halo rows)
    unsigned int *d8_nodir = nullptr;                 // ... and sets this word when an interior cell has none
    bool d8_done = false;                             // set by end(): d8_out holds the directions of the verified surface
    bool defer_out = false;                           // with d8_out and an external `dist`: end() may leave `out` unwritten ...
    bool out_deferred = false;                        // ... set by end(): it did -- `out` is noflat_assemble_dev(filled, dist) whenever somebody wants it
    FillHandover *handover = nullptr;                 // pending: begin() computes, writes and proves `filled` (and the depths) in its first visit
    bool wet_used = false;                            // set by end(): its pass took the DEM from the hand-over's wet bits
    struct Impl;
    Impl *impl;
    GeoRun();
    ~GeoRun();
    GeoRun(const GeoRun &) = delete;
    GeoRun &operator=(const GeoRun &) = delete;
    int begin(hipStream_t s, bool *applicable, bool *active);
    int batch(hipStream_t s, bool *active);
    int halo_changed(int side, hipStream_t s);
    int end(hipStream_t s, bool *ok, FillStats *st);
    int launch_rounds(hipStream_t s, int nb);
};
// noflat_geo.hip: MHIP_ELIMIT = not applicable, run the float64 relaxation
// D8Sink: the caller wants the flow directions of the surface too; when the geodesic transform's finishing pass could write them
// (`done`) the D8 pass over the surface is not needed
struct D8Sink {
    uint8_t *flowdir = nullptr;
    unsigned int *nodir = nullptr;     // zeroed by the caller; set when an interior cell has no downslope neighbour
    bool done = false;
    // The caller reads the surface from nowhere but these directions (a chain request): with `dist`, a raster of its own
    // for the distances, and `defer`, a finishing pass that is the last word on the surface does not store it -- `deferred`: d_out is
    // unwritten, and noflat_assemble_dev(d_filled, dist, d_out) writes it at any later time.  Every other outcome stores as ever.
    uint32_t *dist = nullptr;
    bool defer = false, deferred = false;
};
int noflat_assemble_dev(const float *d_filled, const uint32_t *d_dist, double *d_out, int64_t n, double seed_add, hipStream_t s);
int fill_noflat_geodesic_dev(const float *d_dem, const float *d_filled, double *d_out, int64_t H, int64_t W, double sh, double dg, double seed_add,
                             hipStream_t s, FillStats *st, bool *partial, StageHook *tail_hook = nullptr, D8Sink *d8 = nullptr, FillHandover *ho = nullptr);
int noflat_verify_dev(const float *d_dem, const double *d_out, int64_t H, int64_t W, double sh, double dg, hipStream_t s, bool *ok, int fixed_top = 0,
                      int fixed_bot = 0);
// ho (optional, pending): d_filled is still owed by the flood -- whatever engine runs, it holds the plain fill before it is read
int fill_noflat_dev(const float *d_dem, double *d_out, int64_t H, int64_t W, double sh, double dg, hipStream_t s,
                    FillStats *st = nullptr, const float *d_filled = nullptr, StageHook *tail_hook = nullptr, D8Sink *d8 = nullptr,
                    FillHandover *ho = nullptr);
int short_diag_dev(const float *d_dem, int64_t n, double *sh, double *dg, hipStream_t s);
int depths_dev(const float *d_filled, const float *d_dem, float *d_out, int64_t n, hipStream_t s);
// d8.hip
int d8_dev(const double *d_z, uint8_t *d_out, int64_t H, int64_t W, int edges_outward, hipStream_t s, int64_t row_off = 0,
           int64_t Hg = 0, unsigned int *d_interior_nodir = nullptr);   // d_interior_nodir (edges_outward only): left != 0 when an interior cell got NODIR (pre-zeroed by the caller)
void short_diag_from_minmax(float mn, float mx, bool has_nan, double *sh, double *dg);   // fill.py:235-250
int minmax_dev(const float *d_x, int64_t n, float *mn, float *mx, int *has_nan, hipStream_t s);
int row_update_dev(void *d_dst, const void *d_src, int64_t nbytes, int *changed, hipStream_t s);
int copy_bandwidth_dev(size_t bytes, int reps, double *gbs, hipStream_t s);
int read_bandwidth_dev(size_t bytes, int reps, double *gbs, hipStream_t s);
int row_update_async(void *d_dst, const void *d_src, int64_t nbytes, int *d_changed, hipStream_t s);
// trace.hip
int trace_downstream_dev(const uint8_t *d_fd, const int32_t *d_lab, int64_t H, int64_t W, const int64_t *d_cells, int64_t n, int use_bg,
                         int32_t bg, int32_t *d_label, int32_t *d_found, int64_t *d_len, const int64_t *d_offsets, int64_t *d_out_cells,
                         hipStream_t s);
// comm.hip (RCCL, opened at run time)
int comm_unique_id(void *id128);
int comm_available();
int comm_create(void **comm, const void *id128, int rank, int nranks);
void comm_destroy(void *comm);
int comm_exchange_rows(void *comm, int rank, int nranks, const void *first_row, const void *last_row, void *stage, size_t rowbytes,
                       hipStream_t s);
int comm_allreduce_max(void *comm, double *d_value, hipStream_t s);
// Pour points out of the accumulation's final pass (bluespots.py:195-206: the cell of the largest accumulated flow of every label,
// the first in raster order among equals).  Accumulated flow grows strictly along a flow path, so the largest value of a label
// sits on a cell whose downstream cell is NOT of that label -- a CANDIDATE: 3 % of the labelled cells, a fifth of the unlabelled
// ones.  The watersheds' tile pass (labels + flow directions of a 64 x 64 tile in one place) lists the candidates; the
// accumulation's final pass (the final sums of the same tile in LDS) turns them into one packed key per label,
// (value << 32) | (0xffffffff - cell), by atomicMax -- and the pass over accumulation + labels that the pour points were
// (12.6 B/cell at the end of a step) goes.  Exact unless a cell stays unresolved (a flow cycle: the value 0 does not grow along
// the path) or the list overflows: both raise a flag and the caller runs the general pass.
struct PourCandDev {             // device side, tile = 64 x 64 cells as in accum.hip / watershed.hip, thread t <-> row t >> 2, columns (t & 3) * 16 ..
    uint16_t *mask0 = nullptr;   // [ntiles * 256] unlabelled candidates: bit k of word t = column (t & 3) * 16 + k of row t >> 2
    uint2 *list = nullptr;       // [ntiles * POUR_TILE_CAP] labelled candidates: (cell, label); a tile's entries start at tile * POUR_TILE_CAP
    uint32_t *tile_cnt = nullptr;          // [ntiles]   (no global counters: 65 536 atomics on one address cost a millisecond)
    unsigned long long *tile_key0 = nullptr;   // [ntiles] the best key among the tile's unlabelled candidates (label 0: reduced by pour_finish_dev)
    uint32_t *flags = nullptr;   // [0] a tile's list overflowed, [1] an unresolved cell
    int components = 0;          // the labels are 8-connected components: two neighbouring labelled cells share their label
    unsigned long long *key = nullptr;   // [nlabels + 1], zeroed
    uint32_t nlab = 0;           // a candidate with a label outside [0, nlab] (uploaded labels) raises flags[1]: the general pass reports it
};
constexpr uint32_t POUR_TILE_CAP = 512;
struct PourLink {                // host side: hand-over between the thread of the watersheds and the thread of the accumulation
    PourCandDev dev;
    hipEvent_t ev = nullptr;                       // recorded behind the tile pass that wrote the candidates
    void (*notify)(void *, int) = nullptr;         // watersheds_dev: candidates recorded (1) / there will be none (0)
    int (*wait)(void *) = nullptr;                 // accum_dev, before its final pass: blocks; 1: the candidates exist (wait for `ev`)
    void *arg = nullptr;
    bool consumed = false;                         // the final pass has written the keys
};
// accum.hip
struct AccumKeep {               // the perimeter graph of a row band's boundary pass, kept for the delta pass that follows it
    DevBuf nodes;
    size_t o[9] = {};
    int64_t H = 0, W = 0;
    int fixed_top = 0, fixed_bot = 0;
    bool valid = false;
};
// accum_dev's node buffer, allocated and cleared ahead of the call on a stream of the caller's choice: neither depends on the flow
// directions, and a request that computes them first has time for both (mhip_ctx_run).  A buffer nobody takes goes back to the pool
// when the object goes, behind its clears.
struct AccumPrep {
    DevBuf nodes;
    int64_t H = 0, W = 0;
    hipEvent_t ready = nullptr;      // (the caller's) recorded behind the clears
    bool valid = false;
    ~AccumPrep();
};
int accum_prepare_dev(AccumPrep *prep, int64_t H, int64_t W, hipStream_t s, hipEvent_t ready);
// prep (optional): a buffer of accum_prepare_dev for this raster is taken over; without one, for a row band's passes (exit map,
// keep) or another raster the call allocates and clears its own, as ever
int accum_dev(const uint8_t *d_fd, double *d_out, int64_t H, int64_t W, hipStream_t s, int fixed_top = 0, int fixed_bot = 0, int halo_zero = 0,
              int32_t *d_exit_map = nullptr, PourLink *pour = nullptr, AccumKeep *keep = nullptr, AccumPrep *prep = nullptr);
int accum_band_delta_dev(const uint8_t *d_fd, double *d_out, int64_t H, int64_t W, hipStream_t s, int fixed_top, int fixed_bot, AccumKeep *keep, bool *done);
// ccl.hip   (d_tmp: H*W int32 scratch)
// stats_out: the labelling's last pass also reduces label_stats(d_data, labels) into *stats_out (allocated here: nlabels + 1 records)
// wet: "d_data != 0" of every cell as the wet bits of a hand-over (FillHandover::wet with wet_ok) -- the tile pass reads them and not
// d_data (*wet_used); the emit / statistics pass keeps reading the values
int ccl8_f32_dev(const float *d_data, int32_t *d_labels, int32_t *d_tmp, int64_t H, int64_t W, int64_t *nlabels,
                 hipStream_t s, DevBuf *stats_out = nullptr, const unsigned long long *wet = nullptr, bool *wet_used = nullptr);
int label_emit_stats_dev(const int32_t *d_parent, const unsigned long long *d_rootbits, const uint32_t *d_wordprefix, const float *d_data,
                         int32_t *d_labels, int64_t H, int64_t W, int64_t nlab, mhip_stat_record *d_rec, hipStream_t s);
int ccl8_u8_dev(const uint8_t *d_data, int32_t *d_labels, int32_t *d_tmp, int64_t H, int64_t W, int64_t *nlabels,
                hipStream_t s);
// a row band labels in two halves: ccl8_f32_begin_dev stops before the emit pass -- the labels raster gets its two top and two bottom
// rows only (band-local ranks: what the seam merge on the host compares), parent (d_tmp) / root bits / word prefixes stay in `keep`
// -- and label_emit_sparse_dev writes the GLOBAL labels once the merge has numbered them (label_ops.hip)
struct CclKeep {
    DevBuf bits, wprefix;
    int64_t H = 0, W = 0, nlocal = 0;
    bool valid = false;       // false: the labels raster holds band-local labels everywhere (a schedule without the kept tables)
};
int ccl8_f32_begin_dev(const float *d_data, int32_t *d_labels, int32_t *d_tmp, int64_t H, int64_t W, int64_t *nlabels, hipStream_t s, CclKeep *keep);
int ccl_emit_rows_dev(const int32_t *d_parent, const unsigned long long *d_rootbits, const uint32_t *d_wordprefix, int32_t *d_labels, int64_t base,
                      int64_t count, hipStream_t s);
int label_emit_sparse_dev(const int32_t *d_parent, const unsigned long long *d_rootbits, const uint32_t *d_wordprefix, const float *d_data,
                          int32_t *d_labels, int64_t H, int64_t W, int ht, int64_t H_owned, int64_t nlocal, int32_t offset,
                          const int32_t *d_dropped, const int32_t *d_target, int32_t ndropped, int64_t nlab_global, mhip_stat_record *d_rec,
                          hipStream_t s);
// label_ops.hip
int relabel_lut_dev(int32_t *d_labels, const int32_t *d_lut, int64_t nlab, int64_t n, hipStream_t s);
int relabel_range_dev(int32_t *d_labels, int64_t n, int32_t lo, int32_t hi, const int32_t *d_lut, const int32_t *d_fid, const int32_t *d_fnew, int32_t nf,
                      hipStream_t s);
int band_trace_dev(const uint8_t *d_fd, const int32_t *d_lab, int64_t Hl, int64_t W, int64_t row_lo, int64_t own0, int64_t own1, int64_t Hg,
                   const int64_t *d_cells, const int32_t *d_src, int64_t n, int use_bg, int32_t bg, int32_t *d_label, int32_t *d_status,
                   int32_t *d_src_out, int64_t *d_exit, int64_t *d_len, const int64_t *d_offsets, int64_t *d_out_cells, hipStream_t s);
int relabel_sparse_dev(int32_t *d_labels, int64_t n, int64_t nlocal, int32_t offset, const int32_t *d_dropped, const int32_t *d_target,
                       int32_t ndropped, hipStream_t s);
int keep_mask_dev(const int32_t *d_labels, const uint8_t *d_keep, int64_t nlab, int64_t n, uint8_t *d_mask,
                  hipStream_t s);
// W: raster width if the caller knows it (2-D tiles combine a label's rows before the global atomics), 0 = flat array
// components: the labels are the 8-connected components of a raster of which these n cells (rows of W) are a row range
int label_stats_dev(const float *d_data, const int32_t *d_labels, int64_t n, int64_t nlab, mhip_stat_record *d_rec,
                    hipStream_t s, int64_t W = 0, bool components = false);
int label_stats64_dev(const double *d_data, const int32_t *d_labels, int64_t n, int64_t nlab, mhip_stat_record *d_rec, hipStream_t s);
// the reference keeps the FIRST of equal values: a record whose min / max is a zero gets the sign of its label's first zero cell
// (the reductions above order -0.0 below +0.0); the standalone label_stats only, see DESIGN.md
int label_stats_zero_sign_dev(const float *d_data, const int32_t *d_labels, int64_t n, int64_t nlab, mhip_stat_record *d_rec, hipStream_t s);
int label_stats_zero_sign_dev(const double *d_data, const int32_t *d_labels, int64_t n, int64_t nlab, mhip_stat_record *d_rec, hipStream_t s);
int label_arg_dev(const double *d_data, const int32_t *d_labels, int64_t H, int64_t W, int64_t nlab, bool is_max,
                  mhip_index_record *d_rec, hipStream_t s, bool components = false);
int label_count_dev(const int32_t *d_labels, int64_t n, int64_t nlab, int64_t *d_counts, hipStream_t s, int64_t W = 0);
int label_max_dev(const int32_t *d_labels, int64_t n, int32_t *out_max, hipStream_t s);
// hyps.hip: hypsometry tables of the labels, water levels for given amounts, final-state depths.
// Bins of label l are the table entries [offsets[l], offsets[l + 1]); MHIP_HYPS_MAX_BINS bounds offsets[nlab + 1].
constexpr int64_t HYPS_MAX_BINS = (int64_t)1 << 30;   // keys of the tile tables are int32; counts + sums: 12 bytes a bin
// dmax[l * stride]: the labels' largest depths (stride in doubles: 4 walks the `max` field of mhip_stat_record)
int hyps_layout_dev(const double *d_dmax, int64_t stride, int64_t nlab, double res, int64_t *d_offsets, int64_t *total, hipStream_t s);
// ev0 / ev1 (optional): recorded around the table kernel alone; *lds_spills: runs that found no slot in their tile's table
int hyps_table_dev(const float *d_data, const int32_t *d_labels, int64_t n, int64_t W, int64_t nlab, double res, const int64_t *d_offsets,
                   int64_t total, uint32_t *d_counts, double *d_sums, int64_t *lds_spills, hipStream_t s, hipEvent_t ev0 = nullptr,
                   hipEvent_t ev1 = nullptr);
int hyps_levels_dev(int64_t nlab, const int64_t *d_offsets, const uint32_t *d_counts, const double *d_sums, const double *d_dmax, int64_t stride,
                    const double *d_q, mhip_final_record *d_rec, hipStream_t s);
int final_depths_dev(const float *d_data, const int32_t *d_labels, int64_t n, int64_t W, int64_t nlab, mhip_final_record *d_rec, float *d_out,
                     hipStream_t s, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);
// wetat.hip: the first event of a rain series that wets each cell.  d_drawdown[(k * (nlab + 1) + l) * stride]: the
// draw-down of label l in event k (stride 4 walks the `drawdown` field of K * (nlab + 1) mhip_final_records); values: HOST, the
// rains; d_wet (optional) receives the wet cells per (event, label) at d_wet[(k * (nlab + 1) + l) * wet_stride].  Synchronises.
bool wet_at_events_ok(int64_t K, const float *values);      // 1 <= K <= MHIP_WETAT_MAX_EVENTS; finite, > 0, strictly increasing
int wet_at_dev(const float *d_data, const int32_t *d_labels, int64_t n, int64_t W, int64_t nlab, int K, const double *d_drawdown, int64_t stride,
               const float *values, float *d_out, int64_t *d_wet, int64_t wet_stride, hipStream_t s, hipEvent_t ev0 = nullptr,
               hipEvent_t ev1 = nullptr);
// flowdist.hip: flow distance to the receiving terminal (float32 raster, -1 where a walk never ends) and, with d_rec (nlab + 1
// records), the head of the longest flow path per label of the terminal.  d_lab may be nullptr: no cell is labelled.
// Synchronises.  MHIP_EINVAL: with d_rec, a label outside [0, nlab].
bool flow_distance_scale_ok(double scale);      // finite and > 0
int flow_distance_dev(const uint8_t *d_fd, const int32_t *d_lab, int64_t H, int64_t W, double scale, int64_t nlab, float *d_out, mhip_index_record *d_rec,
                      int64_t *unresolved, hipStream_t s);
// The walk down the D8 forest of one call (flowdist.hip owns it; flow_distance_dev, hand_dev and reach_catchments_dev run it): the
// scratch words of the tile pass and, in `cur`, the node array a final pass reads behind the jumps.
struct FlowWalk {
    struct Misc {
        unsigned int open[2];         // the jumps' `open` words of two launches
        unsigned int bad, pad;        // the flow distance's "a label out of range"
        unsigned long long count;     // the count of the final pass
    };
    DevBuf S, NA, NB, misc;
    uint4 *cur = nullptr;
    int64_t ntc = 0;
    unsigned int *bad() { return &misc.as<Misc>()->bad; }
    unsigned long long *count() { return &misc.as<Misc>()->count; }
};
bool flow_walk_fits(int64_t n);      // the int32 index domain of the scratch word
// The limit check (MHIP_ELIMIT, `who` in the message), the buffers, `misc` cleared, the tile pass and the jumps.  An END of a walk is
// a cell with d_acc >= threshold (d_acc != nullptr; float64, a NaN is none) or, with d_lab, a label != 0; without d_acc also a cell
// that steps nowhere (flowdist.hip: walk_tile_kernel).  Synchronises.
int flow_walk_dev(const uint8_t *d_fd, const double *d_acc, const int32_t *d_lab, int64_t H, int64_t W, double threshold, const char *who, FlowWalk &w,
                  hipStream_t s);
// the count and the `bad` word of the final pass, once the stream is idle (the scratch and the nodes go back to the pool with `w`)
int flow_walk_count(FlowWalk &w, int64_t *count, bool *bad, hipStream_t s);
// traveltime.hip: travel time along the flow paths.  travel_time_check / travel_time_walk_check: the argument rules
// of the two calls (MHIP_EINVAL; no device work) -- cellsize and every parameter finite and > 0 (channel_threshold may be +inf); tick
// finite and > 0, and with a table nbins in [1, 256] and bin_ticks >= 1, without one nbins == 0.  step_cost_dev: the cost raster
// (d_acc may be nullptr) and the cells clipped to the cap.  flow_cost_distance_dev: flow_distance_dev with the cost summed down the
// path; d_rec (nlab + 1 records) and d_hist (uint32 [nlab + 1][nbins]) are optional.  MHIP_EINVAL: a cost above the cap; with d_rec
// or d_hist, a label outside [0, nlab].  Both synchronise.
int travel_time_check(double cellsize, const mhip_traveltime_params *p);
int travel_time_walk_check(double tick, int64_t nbins, uint64_t bin_ticks, bool table);
int step_cost_dev(const uint8_t *d_fd, const float *d_z, const double *d_acc, int64_t H, int64_t W, double cellsize, const mhip_traveltime_params &p,
                  uint32_t *d_cost, int64_t *saturated, hipStream_t s);
int flow_cost_distance_dev(const uint8_t *d_fd, const int32_t *d_lab, const uint32_t *d_cost, int64_t H, int64_t W, double tick, int64_t nlab, float *d_out,
                           mhip_index_record *d_rec, int64_t nbins, uint64_t bin_ticks, uint32_t *d_hist, int64_t *unresolved, hipStream_t s);
// hand.hip: height above the nearest drainage and the distance to it along the flow path.  A drainage cell:
// d_acc >= threshold (float64; a NaN is none) or, with d_lab, a label != 0.  d_hand = elev[c] - elev[D(c)] (a NaN result is the
// canonical quiet NaN), `nodata` for a cell whose walk ends without drainage; d_dist (optional) as flow_distance_dev's raster, -1
// there.  Synchronises.  hand_check: the argument rules (MHIP_EINVAL; no device work): threshold finite and >= 1, scale finite and > 0.
int hand_check(double threshold, double scale);
int hand_dev(const uint8_t *d_fd, const double *d_acc, const float *d_elev, const int32_t *d_lab, int64_t H, int64_t W, double threshold, double scale,
             float nodata, float *d_hand, float *d_dist, int64_t *undrained, hipStream_t s);
// reach_catchments_dev (hand.hip): the reaches of flowpaths_dev into `p` and, per cell, the reach (k + 1) of the drainage
// cell D(c) its walk ends at into the int32 raster d_catch -- 0 where the cell is undrained, where D(c) is labelled, and where D(c)
// lies on a cycle of the stream mask that nothing flows into; *assigned: the cells that hold a reach.  Every cell is written.
// Synchronises.  MHIP_ELIMIT as hand_dev and flowpaths_dev, MHIP_EINVAL: a negative label.
int reach_catchments_dev(const uint8_t *d_fd, const double *d_acc, const int32_t *d_lab, int64_t H, int64_t W, double threshold, int32_t *d_catch,
                         mhip_flowpaths *p, int64_t *assigned, hipStream_t s);
// reachcatch.hip: d_depth = stage[catch] - hand where catch > 0, hand is not `nodata` and stage[catch] > hand, +0.0
// elsewhere; d_stage: nreach + 1 float32 on the device; d_rec (optional): nreach + 1 records of d_depth over d_catch by
// zone_stats_dev.  Synchronises.  MHIP_EINVAL: a catchment id outside [0, nreach].
int inundate_dev(const float *d_hand, const int32_t *d_catch, int64_t n, int64_t W, int64_t nreach, const float *d_stage, float nodata, float *d_depth,
                 mhip_zone_record *d_rec, hipStream_t s);
// seaflood.hip (tests/_seaflood.py): the lowest water level at the sources at which a cell is connected to them by water,
// into d_out -- `nodata` where no level below max_level does it; *reached: the other cells.  The sources are d_stage (float32 raster,
// NaN: no source) or, with d_stage == nullptr, the cells of the zones of d_zones whose entry of d_zone_stage (nzone + 1 float32 on the
// device, entry 0 a NaN) is no NaN.  Every result is proven by a pass over both equations before it is returned.  Synchronises.
// MHIP_EINVAL: a source stage that is not finite; MHIP_ENOTCONV: the round cap.  sea_flood_check / sea_levels_check: the argument
// rules (MHIP_EINVAL; no device work).
struct SeaStats {
    int64_t rounds = 0, visits = 0, rechecks = 0;      // launches that found work, tile visits, tiles the proof sent back
};
int sea_flood_check(float max_level, float nodata);
int sea_levels_check(int64_t K, const float *levels, float max_level);
int sea_flood_dev(const float *d_dem, const float *d_stage, const int32_t *d_zones, const float *d_zone_stage, int64_t nzone, int64_t H, int64_t W,
                  float max_level, float nodata, float *d_out, int64_t *reached, SeaStats *st, hipStream_t s);
// ... and what follows from that raster for K checked levels (host array): the records (host), the depths of one level, the classes
int sea_levels_dev(const float *d_level, const float *d_dem, int64_t n, float nodata, int K, const float *levels, mhip_sea_record *records, hipStream_t s);
int sea_depths_dev(const float *d_level, const float *d_dem, int64_t n, float nodata, float z, float *d_out, hipStream_t s);
int sea_classes_dev(const float *d_level, int64_t n, float nodata, int K, const float *levels, int32_t *d_out, hipStream_t s);
// burn.hip: DEM adaptations.  burn_check: the argument rules of mhip_burn_lines_f32 on the host arrays (MHIP_EINVAL; no
// device work).  burn_lines_dev: the checked lines into the float32 raster d_dem in place, the per-line records to `results` (host).
// Synchronises.  nseg == 0 writes the records on the host and touches no device.
int burn_check(int64_t nseg, const mhip_burn_segment *segs, int64_t nline, const mhip_burn_line *lines, const mhip_burn_result *results);
int burn_lines_dev(float *d_dem, int64_t H, int64_t W, int64_t nseg, const mhip_burn_segment *segs, int64_t nline, const mhip_burn_line *lines,
                   double nodata, mhip_burn_result *results, hipStream_t s);
// zones.hip: object exposure.  zones_check: the argument rules of mhip_rasterize_zones_i32 on the host arrays
// (MHIP_EINVAL; no device work).  zones_rasterize_dev: the checked polygons into the int32 raster d_out (every cell is written);
// MHIP_ELIMIT: too many crossings.  zone_stats_dev: nzone + 1 records of d_data over d_zones; MHIP_EINVAL: a zone outside
// [0, nzone].  Both synchronise.
int zones_check(int64_t H, int64_t W, int64_t nvert, const double *xy, int64_t nring, const int64_t *ring_offsets, const int32_t *ring_zone,
                int64_t nzone, int grow);
int zones_rasterize_dev(int32_t *d_out, int64_t H, int64_t W, int64_t nvert, const double *xy, int64_t nring, const int64_t *ring_offsets,
                        const int32_t *ring_zone, int64_t nzone, int grow, hipStream_t s);
int zone_stats_dev(const float *d_data, const int32_t *d_zones, int64_t n, int64_t W, int64_t nzone, mhip_zone_record *d_rec, hipStream_t s);
// polygonize.hip: the outlines of the regions of an int32 label raster.  polygonize_check: the argument rules on the
// shape (MHIP_EINVAL; no device work).  polygonize_dev: the rings of d_lab into three buffers it allocates -- xy int32 [nvert][2],
// ring_offsets int64 [nring + 1], ring_label int32 [nring].  Synchronises.  MHIP_EINVAL: a negative label; MHIP_ELIMIT: more than
// 2**32 - 1 edges.  The handle of the C-ABI keeps the three buffers; polygons_fetch_dev copies them to the caller's arrays.
int polygonize_check(int64_t H, int64_t W);
int polygons_fetch_dev(const mhip_polygons *p, int32_t *xy, int64_t *ring_offsets, int32_t *ring_label);
int polygonize_dev(const int32_t *d_lab, int64_t H, int64_t W, DevBuf &d_xy, DevBuf &d_off, DevBuf &d_rl, int64_t *nring, int64_t *nvert, hipStream_t s);
// flowpaths.hip: the stream network above an accumulation threshold as lines.  flowpaths_check: the argument rules
// (MHIP_EINVAL; no device work).  flowpaths_dev: the reaches of d_fd / d_acc / d_lab (nullptr: no labels) into the buffers of the
// handle, which it allocates -- xy int32 [nvert][2], reach_offsets int64 [nreach + 1], records [nreach] without their orders.
// Synchronises.  MHIP_EINVAL: a negative label; MHIP_ELIMIT: more than 2**31 - 1 stream cells.  flowpaths_fetch_dev copies the three
// buffers to the caller's arrays and computes the Strahler orders there.
int flowpaths_check(int64_t H, int64_t W, double threshold);
// d_rc (optional): an int32 raster that receives the reach of every cell -- k + 1 for the cells of reach k, 0 for every
// other cell; every cell is written.  Without it the call launches what it launches without the parameter.
int flowpaths_dev(const uint8_t *d_fd, const double *d_acc, const int32_t *d_lab, int64_t H, int64_t W, double threshold, mhip_flowpaths *p, hipStream_t s,
                  int32_t *d_rc = nullptr);
int flowpaths_fetch_dev(const mhip_flowpaths *p, int32_t *xy, int64_t *reach_offsets, mhip_reach_record *records);
// watershed.hip
int watersheds_dev(const uint8_t *d_fd, int32_t *d_labels, int64_t H, int64_t W, int32_t unassigned, hipStream_t s,
                   bool band_mode = false, const unsigned int *d_known_interior_nodir = nullptr, const int32_t *d_src = nullptr, PourLink *pour = nullptr);
int pour_finish_dev(unsigned long long *d_key, const unsigned long long *d_tile_key0, int64_t ntiles, int64_t nlab, int64_t W, mhip_index_record *d_rec,
                    hipStream_t s);
int band_pseudo_labels_dev(int32_t *d_ws, int64_t H, int64_t W, int top, int bottom, hipStream_t s);
int negative_lut_dev(int32_t *d_lab, int64_t n, const int32_t *d_lut, int64_t nlut, hipStream_t s);
// the rootedness passes of a band's watersheds (watershed.hip; mhip_ctx_band_watershed_rooted)
constexpr int32_t BAND_ROOT = 1, BAND_ROOTLESS = 0x7fffffff;
int band_root_labels_dev(int32_t *d_out, int64_t H, int64_t W, int64_t row_off, int64_t Hg, hipStream_t s);
int band_hide_rootless_dev(const int32_t *d_lab, const int32_t *d_rooted, int32_t *d_out, int64_t n, hipStream_t s);
int band_show_rootless_dev(int32_t *d_ws, const int32_t *d_lab, int64_t n, hipStream_t s);

__host__ __device__ inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// ---- tile geometry shared by the LDS-table kernels (label_ops.hip, hyps.hip) --------------------------------------
// The raster (width W, n cells; a flat array is treated as 256 columns wide) is cut into tiles of TR rows x 256 columns;
// a block owns a tile, its four wavefronts the four 64-column strips of every row.
constexpr int TR = 32;
struct TileGeom {
    int64_t n, W;
    int64_t ntr, ntc;
};
__host__ __device__ inline TileGeom tile_geom(int64_t n, int64_t W)
{
    TileGeom g;
    g.n = n;
    g.W = (W > 0 && n % W == 0) ? W : 256;
    const int64_t H = cdiv(n, g.W);
    g.ntr = cdiv(H, TR);
    g.ntc = cdiv(g.W, 256);
    return g;
}
// one block per tile up to 256 CUs x 8 blocks, then tile-stride
inline unsigned tile_grid(const TileGeom &g)
{
    const int64_t nt = g.ntr * g.ntc;
    return (unsigned)(nt < 2048 ? (nt > 0 ? nt : 1) : 2048);
}

#ifdef __HIPCC__
// ---- the D8 forest in 64 x 64 tiles, shared by the watersheds and the flow distance (watershed.hip, flowdist.hip) -------------
// the cell downstream of cell i, -1 when it has no direction (a code > 7) or the step leaves the raster
__device__ __forceinline__ int64_t downstream(const uint8_t *fd, int64_t i, int64_t H, int64_t W)
{
    const unsigned code = fd[i];
    if (code > 7u) return -1;
    const int64_t r = i / W, c = i - r * W;
    const int64_t nr = r + dir_dr((int)code), nc = c + dir_dc((int)code);
    if (nr < 0 || nr >= H || nc < 0 || nc >= W) return -1;
    return nr * W + nc;
}
constexpr int WS_TILE = 64;
// The perimeter cells of the tiles -- the only cells a path can ENTER a tile at -- also live in a compact array, 256 slots per tile
// (1 KB: the jumps over the entry cells gather there instead of in the raster, where a tile's left / right columns cost a
// sector per cell: 8.7 B per raster cell for 6 % of the cells).  slot: top row, bottom row, left column, right column.
__device__ __forceinline__ int ws_perim_slot(int lr, int lc)
{
    if (lr == 0) return lc;
    if (lr == WS_TILE - 1) return WS_TILE + lc;
    if (lc == 0) return 2 * WS_TILE + (lr - 1);
    if (lc == WS_TILE - 1) return 2 * WS_TILE + (WS_TILE - 2) + (lr - 1);
    return -1;
}
// the node of an entry cell; -1 for a cell inside its tile (a pointer caught in a flow cycle: it never resolves)
__device__ __forceinline__ int64_t ws_node_of(int32_t cell, uint32_t W, int ntc)
{
    const uint32_t r = (uint32_t)cell / W, c = (uint32_t)cell - r * W;
    const int slot = ws_perim_slot((int)(r & 63u), (int)(c & 63u));
    return slot < 0 ? -1 : (int64_t)((r >> 6) * (uint32_t)ntc + (c >> 6)) * 256 + slot;
}

// ---- the scratch word, the node and the step pair of the walk (written by flowdist.hip: walk_tile_kernel, fdist_jump_kernel; read
//      by the final passes of flowdist.hip and hand.hip) ---------------------------------------------------------------------------
constexpr int32_t FD_NONE = 0x7fffffff;              // unresolved
constexpr int32_t FD_DONE = (int32_t)0x80000000;     // | the global index of the terminal; without it: an entry cell (>= 0)
constexpr double FD_SQRT2 = 1.4142135623730951;
// a step as a packed tile-local pair: orthogonal steps in the low, diagonal steps in the high 16 bits (a tile-local path has at
// most 4095 steps and one more out of the tile: neither field ever carries into the other)
__device__ __forceinline__ uint32_t fd_step(unsigned code) { return (code & 1u) ? 0x10000u : 1u; }
// the exact pair and the terminal of a cell from its scratch word and, for a path that leaves its tile, the node of its entry cell;
// false: unresolved (a cycle inside the tile, or a node still open after the jumps: a cycle across tiles)
__device__ __forceinline__ bool fd_resolve(uint2 s, const uint4 *__restrict__ Nn, uint32_t W, int ntc, uint32_t &no, uint32_t &nd, int32_t &T)
{
    int32_t t = (int32_t)s.x;
    no = s.y & 0xffffu;
    nd = s.y >> 16;
    if (t >= 0 && t != FD_NONE) {      // an entry cell: what its node has been resolved to
        const int64_t node = ws_node_of(t, W, ntc);
        uint4 m = make_uint4((uint32_t)FD_NONE, 0u, 0u, 0u);
        if (node >= 0) m = Nn[node];
        t = (int32_t)m.x;
        no += m.y;
        nd += m.z;
    }
    T = t & ~FD_DONE;      // (meaningless where the result is false)
    return t < 0;          // FD_NONE and an entry cell are >= 0
}
__device__ __forceinline__ double fd_u(uint32_t no, uint32_t nd) { return __dadd_rn((double)no, __dmul_rn((double)nd, FD_SQRT2)); }
template <int V> __device__ __forceinline__ void fd_load(const uint2 *__restrict__ S, int64_t i0, uint2 (&s)[V])
{
    if constexpr (V == 4) {
        const uint4 a = *reinterpret_cast<const uint4 *>(S + i0), b = *reinterpret_cast<const uint4 *>(S + i0 + 2);
        s[0] = make_uint2(a.x, a.y); s[1] = make_uint2(a.z, a.w); s[2] = make_uint2(b.x, b.y); s[3] = make_uint2(b.z, b.w);
    } else {
        s[0] = S[i0];
    }
}
// the count tail of a final pass: the wavefront's sum of `cnt`, one atomic per wavefront that counted anything
__device__ __forceinline__ void fd_count_add(unsigned int cnt, unsigned long long *total)
{
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) cnt += __shfl_xor(cnt, w);
    if (cnt && (threadIdx.x & 63) == 0) atomicAdd(total, (unsigned long long)cnt);
}
// the instantiation of a final-pass kernel for a launch: four cells a thread where the rasters allow 16-byte accesses, else one
template <typename K> inline K pick_v(bool vec, K k4, K k1) { return vec ? k4 : k1; }

// open-addressing slot of `key` in an LDS table of TS (power of two) slots, -1 when the probe limit is hit (the caller
// then falls back to the global atomics); keys[] holds -1 for an empty slot
template <int TS> __device__ __forceinline__ int table_slot(int *keys, int key)
{
    unsigned h = ((unsigned)key * 2654435761u) >> 7;
#pragma unroll 1
    for (int probe = 0; probe < 16; ++probe) {
        h &= (unsigned)(TS - 1);
        const int prev = atomicCAS(&keys[h], -1, key);
        if (prev == -1 || prev == key) return (int)h;
        ++h;
    }
    return -1;
}

// "Does any thread of the workgroup say yes?" with ONE barrier per call.  The library's __syncthreads_or is a reduction through 256
// bytes of LDS of its own with two barriers; the loops that end on such a vote (pointer doubling, label-correcting sweeps) are
// bound by exactly these barriers.  Three LDS words take turns: call n raises w[n % 3] in front of its barrier and reads it behind;
// thread 0 clears the word of call n + 2 there (its last readers left before call n's barrier, its next writers come behind call
// n + 1's).  The caller zeroes the three words in front of a barrier; every call must be reached by all threads of the workgroup.
struct WgVote {
    int *w;
    int turn;
    __device__ __forceinline__ explicit WgVote(int *lds3) : w(lds3), turn(0) {}
    __device__ __forceinline__ bool any(bool p)
    {
        if (__any(p) && (threadIdx.x & 63u) == 0u) w[turn] = 1;
        __syncthreads();
        const bool r = w[turn] != 0;
        if (threadIdx.x == 0) w[turn == 0 ? 2 : turn - 1] = 0;
        turn = turn == 2 ? 0 : turn + 1;
        return r;
    }
};
#endif

}  // namespace mh

struct mhip_polygons {      // a result of mhip_polygonize_i32 / mhip_ctx_polygonize: a snapshot in buffers of its own on `device`
    mh::DevBuf xy, ring_offsets, ring_label;      // (none for a raster without a label: nring == 0 and no device was asked for)
    int64_t nring = 0, nvert = 0;
    int device = -1;
};

struct mhip_flowpaths {     // a result of mhip_flowpaths_f64 / mhip_ctx_flowpaths: a snapshot in buffers of its own on `device`
    mh::DevBuf xy, reach_offsets, records;        // (none without a reach)
    int64_t nreach = 0, nvert = 0, unresolved = 0;
    int device = -1;
};

struct mhip_wacc {          // a result of mhip_ctx_weighted_accum: a snapshot in buffers of its own on `device`
    mh::DevBuf acc, sums;                         // uint64 [H][W]; uint64 [nzone + 1] (none without zones: nzone == -1)
    int64_t H = 0, W = 0, nzone = -1, unresolved = 0;
    int64_t rounds = 0, visits = 0, tiles = 0;    // of mhip_ctx_mfd_accum: launches of the tile schedule, tile visits, tiles (else 0)
    int device = -1;
};

namespace mh {
// wacc.hip: the accumulation of a uint32 weight down the D8 forest in exact uint64 sums, and the weight's sums per label (DESIGN.md
// 20; the definition is tests/_wacc.py).  wacc_check: the argument rules on the shape (MHIP_EINVAL, MHIP_ELIMIT; no device work).
// wacc_dev: d_out (uint64, H x W) and the number of unresolved cells; with d_zones (labels in [0, nzone]) also d_sums (uint64,
// nzone + 1).  Synchronises.  MHIP_EINVAL: a label outside [0, nzone].  wacc_rows_f64_dev: rows of a handle as
// (float64(sum) / div) * mul, `nodata` where the cell is unresolved, into the caller's array.
int wacc_check(int64_t H, int64_t W, int64_t nzone, bool zones);
int wacc_dev(const uint8_t *d_fd, const uint32_t *d_w, const int32_t *d_zones, int64_t H, int64_t W, int64_t nzone, unsigned long long *d_out,
             unsigned long long *d_sums, int64_t *unresolved, hipStream_t s);
int wacc_rows_f64_dev(const mhip_wacc *p, int64_t row0, int64_t nrows, double div, double mul, double nodata, double *dst);

// mfd.hip: multiple-flow-direction accumulation (the definition is tests/_mfd.py).  mfd_check: the argument rules on the
// shape (MHIP_EINVAL, MHIP_ELIMIT; no device work).  mfd_fractions_dev: the uint16 fractions [H][W][8] of a float64 surface; queues one
// launch and does not synchronise.  mfd_accum_dev: the sums of d_w -- or, with d_w null, of `wconst` on every cell -- down the fractions
// into d_out (uint64, H x W) and the number of unresolved cells.  Synchronises.  MHIP_EINVAL: fractions that sum to neither 0 nor ONE.
struct MfdStats {
    int64_t rounds = 0, visits = 0, tiles = 0;
};
int mfd_check(int64_t H, int64_t W);
int mfd_fractions_dev(const double *d_z, int64_t H, int64_t W, int exponent, uint16_t *d_out, hipStream_t s);
int mfd_accum_dev(const uint16_t *d_fr, const uint32_t *d_w, uint32_t wconst, int64_t H, int64_t W, unsigned long long *d_out, int64_t *unresolved,
                  MfdStats *stats, hipStream_t s);
}  // namespace mh
