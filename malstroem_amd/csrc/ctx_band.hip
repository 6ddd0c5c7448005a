// ctx_band.hip -- a context as one row band of a larger raster (ctx.hpp): edge and halo rows, the RCCL exchange, the band halves of
// labelling, accumulation and watersheds with their per-label records, and the resumable fills (mhip_ctx_fill_* / mhip_ctx_geo_*)
// whose rounds alternate with halo exchanges.  The launcher is distributed.BandPipeline.
#include <string>

#include "ctx.hpp"

using namespace mh;

// ---- addressing of the rows the bands trade -----------------------------------------------------------------------------------
static size_t row_bytes(mhip_ctx *c, int which) { return raster_elem(which) * (size_t)c->W; }
// side 0 / 1: the first / last owned row, 2 / 3: the halo row above / below
static char *row_ptr(mhip_ctx *c, int which, int side)
{
    const int64_t row = side == 0 ? c->ht : side == 1 ? c->ht + c->H_owned - 1 : side == 2 ? 0 : c->H - 1;
    return c->r[which].as<char>() + row_bytes(c, which) * (size_t)row;
}

// the device rows `top` / `bottom` (nullptr: none) are compared with / stored into the halo rows of raster `which`;
// changed[0 / 1] = the top / bottom halo row changed.  One host synchronisation (the two flags).
static int update_halo_rows(mhip_ctx *c, int which, const void *top, const void *bottom, int *d_flags, int32_t *changed, hipStream_t s)
{
    const int64_t rowb = (int64_t)row_bytes(c, which);
    MH_HIP(hipMemsetAsync(d_flags, 0, 8, s));
    if (top) MH_TRY(row_update_async(row_ptr(c, which, 2), top, rowb, d_flags, s));
    if (bottom) MH_TRY(row_update_async(row_ptr(c, which, 3), bottom, rowb, d_flags + 1, s));
    int h[2] = {0, 0};
    MH_HIP(hipMemcpyAsync(h, d_flags, 8, hipMemcpyDeviceToHost, s));
    MH_HIP(stream_sync(s));
    changed[0] = h[0];
    changed[1] = h[1];
    return MHIP_OK;
}

// the edge-row getters: rows side0 / side1 of raster `which` into dst0 / dst1 (nullptr: not wanted), host or device memory by
// `kind`.  One synchronisation: a transport reads a device destination on its own stream.
static int copy_edge_rows(mhip_ctx *c, int which, int side0, void *dst0, int side1, void *dst1, hipMemcpyKind kind, const char *usage)
{
    MH_ARG(c && which >= 0 && which < MHIP_R_COUNT_, usage);
    MH_ARG(c->r[which].p, "raster has not been computed or uploaded");
    MH_TRY(ctx_settle(c, which, /*write=*/false));
    const int side[2] = {side0, side1};
    void *const dst[2] = {dst0, dst1};
    for (int k = 0; k < 2; ++k) MH_ARG(!dst[k] || side[k] < 2 || (side[k] == 2 ? c->ht : c->hb), "this band has no halo row on that side");
    if (!dst0 && !dst1) return MHIP_OK;
    MH_HIP(hipSetDevice(c->device));
    hipStream_t s = cs(c);
    for (int k = 0; k < 2; ++k)
        if (dst[k]) MH_HIP(hipMemcpyAsync(dst[k], row_ptr(c, which, side[k]), row_bytes(c, which), kind, s));
    MH_HIP(stream_sync(s));
    return MHIP_OK;
}

// a relabelling of the resident labels: new numbers on the same cells (components stay components), `nlabels` of them over all bands
static void labels_renumbered(mhip_ctx *c, int64_t nlabels)
{
    const bool components = c->labels_components;
    ctx_wrote(c, MHIP_R_LABELS);
    c->labels_components = components;
    c->nlabels = c->nlabels_raw = nlabels;
    c->labels_filtered = true;
}

// ---- the resumable fills ----------------------------------------------------------------------------------------------------
// a fresh iterative fill (kind 0 plain, 1 no-flats) over the band's local raster, in place of the run of that kind
static FillRun *new_fill_run(mhip_ctx *c, int kind)
{
    delete c->run[kind];
    FillRun *f = c->run[kind] = new FillRun();
    f->noflat = kind != 0;
    f->dem = c->r[MHIP_R_DEM].as<float>();
    f->out = c->r[kind ? MHIP_R_NOFLAT : MHIP_R_FILLED].p;
    f->H = c->H; f->W = c->W;
    f->fixed_top = c->ht; f->fixed_bot = c->hb;
    f->rounds_per_batch = 16;   // a band pays a halo exchange + an all-reduce per batch: fewer, longer batches
    return f;
}
// mhip_ctx_fill_begin / _attach has been called for this kind (the plain fill may be a flood, running or proven)
static bool fill_begun(mhip_ctx *c, int kind) { return c->run[kind] || (kind == 0 && (c->pf || c->pf_done)); }

extern "C" {

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
    static const char *const usage = "ctx_get_edge_row(ctx, which, side, host)";
    MH_ARG(host && side >= 0 && side <= 3, usage);
    return copy_edge_rows(c, which, side, host, 0, nullptr, hipMemcpyDeviceToHost, usage);
}

int mhip_ctx_set_halo_row(mhip_ctx *c, int which, int side, const void *host, int32_t *changed)
{
    MH_ARG(c && host && which >= 0 && which < MHIP_R_COUNT_ && (side == 0 || side == 1), "ctx_set_halo_row(ctx, which, side, host)");
    MH_ARG(side == 0 ? c->ht : c->hb, "this band has no halo row on that side");
    int32_t ch[2];
    MH_TRY(mhip_ctx_set_halo_rows(c, which, side == 0 ? host : nullptr, side == 1 ? host : nullptr, ch));
    if (changed) *changed = ch[side];
    return MHIP_OK;
}

// the same two calls for a transport that moves DEVICE buffers (RCCL send/recv on tensors of the launcher)
int mhip_ctx_get_edge_row_dev(mhip_ctx *c, int which, int side, void *dev_dst)
{
    static const char *const usage = "ctx_get_edge_row_dev(ctx, which, side, dev)";
    MH_ARG(dev_dst && side >= 0 && side <= 3, usage);
    return copy_edge_rows(c, which, side, dev_dst, 0, nullptr, hipMemcpyDeviceToDevice, usage);
}

int mhip_ctx_set_halo_row_dev(mhip_ctx *c, int which, int side, const void *dev_src, int32_t *changed)
{
    MH_ARG(c && dev_src && which >= 0 && which < MHIP_R_COUNT_ && (side == 0 || side == 1), "ctx_set_halo_row_dev(ctx, which, side, dev)");
    MH_ARG(side == 0 ? c->ht : c->hb, "this band has no halo row on that side");
    MH_HIP(hipSetDevice(c->device));
    MH_TRY(ctx_raster(c, which));
    MH_TRY(ctx_settle(c, which, /*write=*/true));
    int ch = 0;
    MH_TRY(row_update_dev(row_ptr(c, which, 2 + side), dev_src, (int64_t)row_bytes(c, which), &ch, cs(c)));
    if (changed) *changed = ch;
    return MHIP_OK;
}

/* The host transport's two halves of a halo exchange with ONE synchronisation each (mhip_ctx_get_edge_row / _set_halo_row: one per
 * row -- four host round trips per exchange, and the flood's and the no-flats fill's loops exchange 7 to 24 times per step).
 * get: the first / last owned row into host buffers (NULL: not wanted).  set: the neighbours' rows (NULL where there is none) are
 * compared with / stored into the halo rows; changed[0 / 1] = the top / bottom halo row changed. */
int mhip_ctx_get_edge_rows(mhip_ctx *c, int which, void *host_first, void *host_last)
{
    return copy_edge_rows(c, which, 0, host_first, 1, host_last, hipMemcpyDeviceToHost, "ctx_get_edge_rows(ctx, which, first, last)");
}

int mhip_ctx_set_halo_rows(mhip_ctx *c, int which, const void *host_top, const void *host_bottom, int32_t *changed)
{
    MH_ARG(c && changed && which >= 0 && which < MHIP_R_COUNT_, "ctx_set_halo_rows(ctx, which, top, bottom, changed[2])");
    MH_ARG((!host_top || c->ht) && (!host_bottom || c->hb), "this band has no halo row on that side");
    changed[0] = changed[1] = 0;
    if (!host_top && !host_bottom) return MHIP_OK;
    MH_HIP(hipSetDevice(c->device));
    MH_TRY(ctx_raster(c, which));
    MH_TRY(ctx_settle(c, which, /*write=*/true));
    hipStream_t s = cs(c);
    const size_t rowb = row_bytes(c, which);
    DevBuf &stage = on_side(c) ? c->comm_stage_b : c->comm_stage;
    DevBuf flags;
    MH_TRY(stage.alloc(2 * rowb));
    MH_TRY(flags.alloc(8));
    char *top = stage.as<char>(), *bottom = top + rowb;
    if (host_top) MH_HIP(hipMemcpyAsync(top, host_top, rowb, hipMemcpyHostToDevice, s));
    if (host_bottom) MH_HIP(hipMemcpyAsync(bottom, host_bottom, rowb, hipMemcpyHostToDevice, s));
    return update_halo_rows(c, which, host_top ? top : nullptr, host_bottom ? bottom : nullptr, flags.as<int>(), changed, s);
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
    MH_TRY(ctx_settle(c, which, /*write=*/true));
    hipStream_t s = cs(c);
    const size_t rowb = row_bytes(c, which);
    MH_TRY(c->comm_stage.alloc(2 * rowb));
    MH_TRY(c->comm_flags.alloc(8));
    char *from_up = c->comm_stage.as<char>(), *from_down = from_up + rowb;
    MH_TRY(comm_exchange_rows(c->comm, c->rank, c->nranks, row_ptr(c, which, 0), row_ptr(c, which, 1), from_up, rowb, s));
    return update_halo_rows(c, which, c->ht ? from_up : nullptr, c->hb ? from_down : nullptr, c->comm_flags.as<int>(), changed, s);
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
    MH_TRY(ctx_settle(c, which, /*write=*/false));
    hipStream_t s = cs(c);
    const size_t rowb = row_bytes(c, which);
    DevBuf &stage = on_side(c) ? c->comm_stage_b : c->comm_stage;
    MH_TRY(stage.alloc(2 * rowb));
    MH_TRY(comm_exchange_rows(comm, c->rank, c->nranks, row_ptr(c, which, 0), row_ptr(c, which, 1), stage.p, rowb, s));
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
    MH_TRY(ctx_settle(c, which, /*write=*/true));
    ctx_wrote(c, which);
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
    ctx_wrote(c, MHIP_R_ACCUM);
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
    ctx_wrote(c, MHIP_R_LABELS);
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
    labels_renumbered(c, nlabels_global);
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
    labels_renumbered(c, nlabels_global);
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
    ctx_wrote(c, MHIP_R_LABELS);
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
    ctx_wrote(c, MHIP_R_LABELS);
    c->nlabels = c->nlabels_raw = nlabels_global;
    c->have[MHIP_R_LABELS] = true;
    c->labels_components = true;
    c->labels_filtered = true;
    c->stats_valid = with_stats != 0;
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
    labels_renumbered(c, nlabels_new);
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
    ctx_wrote(c, MHIP_R_WATERSHEDS);
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

/* The band watersheds for flow directions of ANY origin (see include/malstroem_hip.h), in three steps around two seam resolutions:
 * 1: "does my path meet a raster edge cell" as a local pass over a label raster that holds BAND_ROOT on the raster's edge cells;
 * 2: the local pass over the labels with the rootless ones hidden behind BAND_ROOTLESS (WATERSHEDS holds step 1's resolved answer);
 * 3: BAND_ROOTLESS -> the cell's own label (0: none).  The local passes run the plain rule "first label downstream" -- a path that
 * ends in a sink or a cycle inside the band takes nothing -- whatever the field holds: they vouch for "no interior NODIR" themselves. */
int mhip_ctx_band_watershed_rooted(mhip_ctx *c, int step)
{
    MH_ARG(c && step >= 1 && step <= 3 && c->have[MHIP_R_LABELS] && c->have[MHIP_R_FLOWDIR],
           "ctx_band_watershed_rooted(ctx, step 1..3) needs labels and flow directions");
    MH_ARG(step == 1 || c->r[MHIP_R_WATERSHEDS].p, "ctx_band_watershed_rooted: step 1 first");
    MH_HIP(hipSetDevice(c->device));
    MH_TRY(ctx_raster(c, MHIP_R_WATERSHEDS));
    ctx_wrote(c, MHIP_R_WATERSHEDS);
    hipStream_t s = cs(c);
    const int64_t n = c->H * c->W;
    int32_t *ws = c->r[MHIP_R_WATERSHEDS].as<int32_t>();
    const int32_t *lab = c->r[MHIP_R_LABELS].as<int32_t>();
    if (step == 3) {
        MH_TRY(band_show_rootless_dev(ws, lab, n, s));
        MH_HIP(stream_sync(s));
        c->have[MHIP_R_WATERSHEDS] = true;
        return MHIP_OK;
    }
    c->have[MHIP_R_WATERSHEDS] = false;
    DevBuf tmp, zero;
    MH_TRY(tmp.alloc(4 * (size_t)n));
    MH_TRY(zero.alloc(4));
    MH_HIP(hipMemsetAsync(zero.p, 0, 4, s));
    if (step == 1) MH_TRY(band_root_labels_dev(tmp.as<int32_t>(), c->H, c->W, c->row0 - c->ht, c->H_global, s));
    else MH_TRY(band_hide_rootless_dev(lab, ws, tmp.as<int32_t>(), n, s));
    MH_TRY(band_pseudo_labels_dev(tmp.as<int32_t>(), c->H, c->W, c->ht, c->hb, s));
    MH_TRY(watersheds_dev(c->r[MHIP_R_FLOWDIR].as<uint8_t>(), ws, c->H, c->W, 0, s, true, zero.as<unsigned int>(), tmp.as<int32_t>(), nullptr));
    MH_HIP(stream_sync(s));
    return MHIP_OK;
}

/* raster[i] = lut[-raster[i]-1] wherever raster[i] < 0 (resolves the pseudo labels once the boundary system is solved) */
int mhip_ctx_band_apply_neg_lut(mhip_ctx *c, int which, const int32_t *lut, int64_t n)
{
    MH_ARG(c && lut && n >= 1 && (which == MHIP_R_WATERSHEDS || which == MHIP_R_LABELS) && c->r[which].p, "ctx_band_apply_neg_lut");
    MH_HIP(hipSetDevice(c->device));
    if (which == MHIP_R_LABELS) labels_renumbered(c, c->nlabels);      // (pseudo labels resolve into the numbering the raster has)
    else ctx_wrote(c, which);
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
static std::atomic<bool> &band_record_valid(mhip_ctx *c, int which) { return which == 0 ? c->stats_valid : which == 1 ? c->ws_counts_valid : c->pour_valid; }
static const char *const BAND_RECORDS_MISSING = "the record set needs mhip_ctx_band_records(which) on the resident rasters (which 0: or mhip_ctx_band_ccl_finish with statistics)";

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
        // labels that were uploaded may hold cells of depth +0.0 and -0.0 (a bluespot of the library's own labelling has depth > 0):
        // which zero a record reports is the label's first one in raster order, like the standalone label_stats
        if (!c->labels_components)
            MH_TRY(label_stats_zero_sign_dev(c->r[MHIP_R_DEPTHS].as<float>() + off, c->r[MHIP_R_LABELS].as<int32_t>() + off, n, c->nlabels,
                                             buf.as<mhip_stat_record>(), cs(c)));
    } else if (which == 1) {
        MH_ARG(c->have[MHIP_R_WATERSHEDS], "watershed counts need the watersheds");
        MH_TRY(label_count_dev(c->r[MHIP_R_WATERSHEDS].as<int32_t>() + off, n, c->nlabels, buf.as<int64_t>(), cs(c), c->W));
    } else {
        // bluespots.py:195-206: the first arg-max of the accumulated flow (2), or the first arg-min of the no-flats surface (3)
        const int src = which == 2 ? MHIP_R_ACCUM : MHIP_R_NOFLAT;
        MH_ARG(c->have[src], which == 2 ? "pour points need the accumulated flow" : "pour points need the no-flats surface");
        MH_TRY(ctx_settle(c, src, /*write=*/false));
        MH_TRY(label_arg_dev(c->r[src].as<double>() + off, c->r[MHIP_R_LABELS].as<int32_t>() + off, c->H_owned, c->W, c->nlabels,
                             which == 2, buf.as<mhip_index_record>(), cs(c), c->labels_components));
        hipLaunchKernelGGL(global_rows_kernel, dim3((unsigned)cdiv(nrec, 256)), dim3(256), 0, cs(c), buf.as<mhip_index_record>(), nrec,
                           c->row0);
        MH_HIP(hipGetLastError());
    }
    band_record_valid(c, which) = true;
    return MHIP_OK;
}

/* records [first, first + count) of the last mhip_ctx_band_records(which) */
int mhip_ctx_band_fetch(mhip_ctx *c, int which, int64_t first, int64_t count, void *out)
{
    MH_ARG(c && which >= 0 && which <= 3 && first >= 0 && count >= 0 && (out || count == 0), "ctx_band_fetch(ctx, which, first, count, out)");
    MH_ARG(band_record_valid(c, which), BAND_RECORDS_MISSING);
    MH_ARG(first + count <= c->nlabels + 1, "ctx_band_fetch: records outside [0, nlabels]");
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
    MH_ARG(c && which >= 0 && which <= 3 && nids >= 0 && ((ids && out) || nids == 0), "ctx_band_gather");
    MH_ARG(band_record_valid(c, which), BAND_RECORDS_MISSING);
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
    MH_ARG(c && cap >= 0 && nfound && ((ids && counts) || cap == 0), "ctx_band_foreign_counts");
    MH_ARG(c->ws_counts_valid, BAND_RECORDS_MISSING);
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
    MH_TRY(ctx_settle(c, which, /*write=*/true));      // (this fill's raster is in flux between the calls of its loop)
    ctx_wrote(c, which);
    if (kind == 0) {
        // the tiled priority-flood first: the band's whole local solve happens here, the loop that follows only trades edge rows
        const bool force_iter = [] { const char *e = dev_env("MHIP_FILL"); return e && std::string(e) == "iterative"; }();   // (development: engine selection for A/B runs and tests)
        delete c->pf;
        c->pf = nullptr;
        c->pf_done = false;
        c->pf_depths = false;
        c->pf_overflow = 0;
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
            c->pf_overflow = p->overflow;
            delete p;
            if (rc != MHIP_ELIMIT) return rc;
        }
    }
    if (kind) {   // a geodesic run that was abandoned (another band found it not applicable)
        delete c->geo;
        c->geo = nullptr;
    }
    FillRun *f = new_fill_run(c, kind);
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
    MH_TRY(ctx_settle(c, which, /*write=*/true));      // (kind 1 starts from the surface that is there)
    ctx_wrote(c, which);
    if (kind == 0) {
        delete c->pf;
        c->pf = nullptr;
    }
    FillRun *f = new_fill_run(c, kind);
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
    double *g = nullptr;
    MH_TRY(ctx_noflat(c, &g));
    MH_TRY(noflat_verify_dev(c->r[MHIP_R_DEM].as<float>(), g, c->H, c->W, c->sh, c->dg, c->stream, &good, c->ht, c->hb));
    *ok = good ? 1 : 0;
    return MHIP_OK;
}

// the plain fill of a band continues on the iterative schedule from the surface it has (an upper bound of the result)
static int ctx_attach_iterative_fill(mhip_ctx *c) { return new_fill_run(c, 0)->attach(c->stream); }

int mhip_ctx_fill_batch(mhip_ctx *c, int kind, int32_t *active)
{
    MH_ARG(c && active && (kind == 0 || kind == 1) && fill_begun(c, kind), "ctx_fill_batch needs ctx_fill_begin");
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
        c->pf_overflow = c->pf->overflow;
        delete c->pf;
        c->pf = nullptr;
        bool a0 = false;
        MH_TRY(new_fill_run(c, 0)->begin(c->stream, &a0));
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
    MH_ARG(c && changed && (kind == 0 || kind == 1) && fill_begun(c, kind), "ctx_fill_certify needs ctx_fill_begin");
    MH_HIP(hipSetDevice(c->device));
    if (kind == 0 && c->pf) {
        // The flood is quiescent on every band (the caller voted): write the raster and prove it (check.hip) -- K3 is a worklist
        // schedule too.  A band whose surface fails the proof continues with the iterative schedule from that surface (an upper
        // bound of the result); its neighbours follow when their halo rows move (mhip_ctx_fill_halo_changed below).
        bool violated = false;
        FillStats st;
        MH_TRY(ctx_raster(c, MHIP_R_DEPTHS));      // the bluespot depths of the owned rows ride on the pass that writes the raster, as in one context
        ctx_wrote(c, MHIP_R_DEPTHS);
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
    MH_ARG(c && (kind == 0 || kind == 1) && fill_begun(c, kind) && (side == 0 || side == 1), "ctx_fill_halo_changed needs ctx_fill_begin");
    MH_HIP(hipSetDevice(c->device));
    if (kind == 0 && c->pf) return c->pf->halo_changed(side, c->stream);
    // a neighbour repaired its surface after this band's flood was finished: follow on the iterative schedule
    if (kind == 0 && !c->run[0]) MH_TRY(ctx_attach_iterative_fill(c));
    return c->run[kind]->activate_row(side, c->stream);
}

int mhip_ctx_fill_end(mhip_ctx *c, int kind)
{
    MH_ARG(c && (kind == 0 || kind == 1) && fill_begun(c, kind), "ctx_fill_end needs ctx_fill_begin");
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
    if (kind == 0) {
        c->pf_done = false;
        st.overflow = c->pf_overflow;
    }
    if (kind) { c->noflat_rounds = st.rounds; c->noflat_st = st; ctx_wrote(c, MHIP_R_NOFLAT); c->have[MHIP_R_NOFLAT] = true; }
    else {
        c->fill_rounds = st.rounds; c->fill_st = st; c->have[MHIP_R_FILLED] = true;
        ctx_wrote(c, MHIP_R_DEPTHS);
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
    MH_TRY(ctx_noflat(c));      // (the distances of a pending surface are about to be overwritten)
    ctx_wrote(c, MHIP_R_NOFLAT);
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
        ctx_wrote(c, MHIP_R_NOFLAT);
        c->have[MHIP_R_NOFLAT] = true;
    }
    return MHIP_OK;
}

}  // extern "C"
