// api.hip -- the host-raster entry points of libmalstroem_hip.so (declared in include/malstroem_hip.h): upload -> stage -> download,
// one per malstroem.algorithms stage function, over the device-pointer stage implementations (fill.hip, d8.hip, accum.hip, ccl.hip,
// label_ops.hip, hyps.hip, watershed.hip, flowdist.hip, burn.hip, zones.hip, polygonize.hip, flowpaths.hip, reachcatch.hip, trace.hip).  They keep no state; the device-resident pipeline is ctx.hip.
#include <new>
#include <vector>

#include "common.hpp"

namespace mh {

/* net.next_downstream_label for a batch of cells (reference net.py:142-169): labels / found flags / path lengths, and -- when
 * offsets (n + 1 prefix sums of the lengths of an earlier call) and out_cells are given -- the cells of every path as linear
 * indices row * W + col.  The two rasters are on the device: uploaded host arrays for mhip_trace_downstream_i32, the resident
 * ones for mhip_ctx_trace_downstream. */
int trace_on_device(const uint8_t *d_fd, const int32_t *d_lab, int64_t H, int64_t W, const int64_t *cells_rc, int64_t n, int use_bg,
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

}  // namespace mh

using namespace mh;

extern "C" {

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

int mhip_label_wet_at_f32(const float *data, const int32_t *labels, int64_t n, int64_t W, int64_t nlab, int32_t K, const double *drawdown,
                          const float *values, float *out, int64_t *wet)
{
    MH_ARG(data && labels && drawdown && values && out && n >= 1 && W >= 0 && nlab >= 0,
           "label_wet_at_f32(data, labels, n>=1, W>=0, nlab>=0, K, drawdown, values, out, wet)");
    MH_ARG(wet_at_events_ok(K, values), "label_wet_at_f32: 1 to 16 events whose values are finite, > 0 and strictly increasing");
    MH_TRY(require_device());
    hipStream_t s = 0;
    const size_t nt = (size_t)K * (size_t)(nlab + 1);
    DevBuf d_d, d_l, d_t, d_out, d_w;
    MH_TRY(upload(d_d, data, (size_t)n * 4, s));
    MH_TRY(upload(d_l, labels, (size_t)n * 4, s));
    MH_TRY(upload(d_t, drawdown, 8 * nt, s));
    MH_TRY(d_out.alloc((size_t)n * 4));
    if (wet) MH_TRY(d_w.alloc(8 * nt));
    MH_TRY(wet_at_dev(d_d.as<float>(), d_l.as<int32_t>(), n, W, nlab, K, d_t.as<double>(), 1, values, d_out.as<float>(),
                      wet ? d_w.as<int64_t>() : nullptr, 1, s));
    if (wet) MH_HIP(hipMemcpyAsync(wet, d_w.p, 8 * nt, hipMemcpyDeviceToHost, s));
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

int mhip_flow_distance(const uint8_t *flowdir, const int32_t *labels, int64_t H, int64_t W, double scale, int64_t nlab, float *out_dist,
                       mhip_index_record *records, int64_t *unresolved)
{
    MH_ARG(flowdir && out_dist && H >= 1 && W >= 1 && nlab >= 0, "flow_distance(flowdir, labels, H>=1, W>=1, scale, nlab>=0, out, records, unresolved)");
    MH_ARG(flow_distance_scale_ok(scale), "flow_distance: the scale must be finite and > 0");
    MH_TRY(require_device());
    hipStream_t s = 0;
    const size_t n = (size_t)(H * W);
    DevBuf d_fd, d_l, d_out, d_rec;
    MH_TRY(upload(d_fd, flowdir, n, s));
    if (labels) MH_TRY(upload(d_l, labels, n * 4, s));
    MH_TRY(d_out.alloc(n * 4));
    if (records) MH_TRY(d_rec.alloc(sizeof(mhip_index_record) * (size_t)(nlab + 1)));
    MH_TRY(flow_distance_dev(d_fd.as<uint8_t>(), labels ? d_l.as<int32_t>() : nullptr, H, W, scale, nlab, d_out.as<float>(),
                             records ? d_rec.as<mhip_index_record>() : nullptr, unresolved, s));
    if (records) MH_HIP(hipMemcpyAsync(records, d_rec.p, sizeof(mhip_index_record) * (size_t)(nlab + 1), hipMemcpyDeviceToHost, s));
    return download(out_dist, d_out, n * 4, s);
}

int mhip_step_cost(const uint8_t *flowdir, const float *z, const double *accum, int64_t H, int64_t W, double cellsize,
                   const mhip_traveltime_params *params, uint32_t *cost, int64_t *saturated)
{
    MH_ARG(flowdir && z && cost && H >= 1 && W >= 1, "step_cost(flowdir, z, accum, H>=1, W>=1, cellsize, params, cost, saturated)");
    MH_TRY(travel_time_check(cellsize, params));
    MH_TRY(require_device());
    hipStream_t s = 0;
    const size_t n = (size_t)(H * W);
    DevBuf d_fd, d_z, d_a, d_c;
    MH_TRY(upload(d_fd, flowdir, n, s));
    MH_TRY(upload(d_z, z, n * 4, s));
    if (accum) MH_TRY(upload(d_a, accum, n * 8, s));
    MH_TRY(d_c.alloc(n * 4));
    MH_TRY(step_cost_dev(d_fd.as<uint8_t>(), d_z.as<float>(), accum ? d_a.as<double>() : nullptr, H, W, cellsize, *params, d_c.as<uint32_t>(), saturated, s));
    return download(cost, d_c, n * 4, s);
}

int mhip_flow_cost_distance(const uint8_t *flowdir, const int32_t *labels, const uint32_t *cost, int64_t H, int64_t W, double tick, int64_t nlab,
                            float *out, mhip_index_record *records, int64_t nbins, uint64_t bin_ticks, uint32_t *hist, int64_t *unresolved)
{
    MH_ARG(flowdir && cost && out && H >= 1 && W >= 1 && nlab >= 0,
           "flow_cost_distance(flowdir, labels, cost, H>=1, W>=1, tick, nlab>=0, out, records, nbins, bin_ticks, hist, unresolved)");
    MH_TRY(travel_time_walk_check(tick, nbins, bin_ticks, hist != nullptr));
    MH_TRY(require_device());
    hipStream_t s = 0;
    const size_t n = (size_t)(H * W), nrec = (size_t)(nlab + 1), hbytes = 4 * nrec * (size_t)nbins;
    DevBuf d_fd, d_l, d_c, d_out, d_rec, d_h;
    MH_TRY(upload(d_fd, flowdir, n, s));
    if (labels) MH_TRY(upload(d_l, labels, n * 4, s));
    MH_TRY(upload(d_c, cost, n * 4, s));
    MH_TRY(d_out.alloc(n * 4));
    if (records) MH_TRY(d_rec.alloc(sizeof(mhip_index_record) * nrec));
    if (hist) MH_TRY(d_h.alloc(hbytes));
    MH_TRY(flow_cost_distance_dev(d_fd.as<uint8_t>(), labels ? d_l.as<int32_t>() : nullptr, d_c.as<uint32_t>(), H, W, tick, nlab, d_out.as<float>(),
                                  records ? d_rec.as<mhip_index_record>() : nullptr, nbins, bin_ticks, hist ? d_h.as<uint32_t>() : nullptr, unresolved, s));
    if (records) MH_HIP(hipMemcpyAsync(records, d_rec.p, sizeof(mhip_index_record) * nrec, hipMemcpyDeviceToHost, s));
    if (hist) MH_HIP(hipMemcpyAsync(hist, d_h.p, hbytes, hipMemcpyDeviceToHost, s));
    return download(out, d_out, n * 4, s);
}

int mhip_hand_f32(const uint8_t *flowdir, const double *accum, const float *elev, const int32_t *labels, int64_t H, int64_t W, double threshold,
                  double scale, float nodata, float *out_hand, float *out_dist, int64_t *undrained)
{
    MH_ARG(flowdir && accum && elev && out_hand && H >= 1 && W >= 1,
           "hand_f32(flowdir, accum, elev, labels, H>=1, W>=1, threshold, scale, nodata, out_hand, out_dist, undrained)");
    MH_TRY(hand_check(threshold, scale));
    MH_TRY(require_device());
    hipStream_t s = 0;
    const size_t n = (size_t)(H * W);
    DevBuf d_fd, d_a, d_z, d_l, d_h, d_d;
    MH_TRY(upload(d_fd, flowdir, n, s));
    MH_TRY(upload(d_a, accum, n * 8, s));
    MH_TRY(upload(d_z, elev, n * 4, s));
    if (labels) MH_TRY(upload(d_l, labels, n * 4, s));
    MH_TRY(d_h.alloc(n * 4));
    if (out_dist) MH_TRY(d_d.alloc(n * 4));
    MH_TRY(hand_dev(d_fd.as<uint8_t>(), d_a.as<double>(), d_z.as<float>(), labels ? d_l.as<int32_t>() : nullptr, H, W, threshold, scale, nodata,
                    d_h.as<float>(), out_dist ? d_d.as<float>() : nullptr, undrained, s));
    if (out_dist) MH_HIP(hipMemcpyAsync(out_dist, d_d.p, n * 4, hipMemcpyDeviceToHost, s));
    return download(out_hand, d_h, n * 4, s);
}

int mhip_sea_flood_f32(const float *dem, const float *stage, int64_t H, int64_t W, float max_level, float nodata, float *out_level, int64_t *reached)
{
    MH_ARG(dem && stage && out_level && H >= 1 && W >= 1, "sea_flood_f32(dem, stage, H>=1, W>=1, max_level, nodata, out_level, reached)");
    MH_TRY(sea_flood_check(max_level, nodata));
    MH_TRY(require_device());
    hipStream_t s = 0;
    const size_t n = (size_t)(H * W);
    DevBuf d_dem, d_stage, d_out;
    MH_TRY(upload(d_dem, dem, n * 4, s));
    MH_TRY(upload(d_stage, stage, n * 4, s));
    MH_TRY(d_out.alloc(n * 4));
    MH_TRY(sea_flood_dev(d_dem.as<float>(), d_stage.as<float>(), nullptr, nullptr, 0, H, W, max_level, nodata, d_out.as<float>(), reached, nullptr, s));
    return download(out_level, d_out, n * 4, s);
}

int mhip_burn_lines_f32(float *dem, int64_t H, int64_t W, int64_t nseg, const mhip_burn_segment *segments, int64_t nline,
                        const mhip_burn_line *lines, double nodata, mhip_burn_result *results)
{
    MH_ARG(dem && H >= 1 && W >= 1, "burn_lines_f32(dem, H>=1, W>=1, nseg, segments, nline, lines, nodata, results)");
    MH_TRY(burn_check(nseg, segments, nline, lines, results));
    if (nseg == 0) return burn_lines_dev(nullptr, H, W, 0, segments, nline, lines, nodata, results, 0);
    MH_TRY(require_device());
    hipStream_t s = 0;
    const size_t n = (size_t)(H * W);
    DevBuf d_dem;
    MH_TRY(upload(d_dem, dem, n * 4, s));
    MH_TRY(burn_lines_dev(d_dem.as<float>(), H, W, nseg, segments, nline, lines, nodata, results, s));
    return download(dem, d_dem, n * 4, s);
}

int mhip_rasterize_zones_i32(int64_t H, int64_t W, int64_t nvert, const double *xy, int64_t nring, const int64_t *ring_offsets,
                             const int32_t *ring_zone, int64_t nzone, int32_t grow, int32_t *out_zones)
{
    MH_ARG(out_zones, "rasterize_zones_i32(H, W, nvert, xy, nring, ring_offsets, ring_zone, nzone, grow, out)");
    MH_TRY(zones_check(H, W, nvert, xy, nring, ring_offsets, ring_zone, nzone, grow));
    const size_t n = (size_t)(H * W);
    if (nring == 0) {
        std::memset(out_zones, 0, 4 * n);
        return MHIP_OK;
    }
    MH_TRY(require_device());
    hipStream_t s = 0;
    DevBuf d_out;
    MH_TRY(d_out.alloc(4 * n));
    MH_TRY(zones_rasterize_dev(d_out.as<int32_t>(), H, W, nvert, xy, nring, ring_offsets, ring_zone, nzone, grow, s));
    return download(out_zones, d_out, 4 * n, s);
}

int mhip_zone_stats_f32(const float *data, const int32_t *zones, int64_t n, int64_t W, int64_t nzone, mhip_zone_record *records)
{
    MH_ARG(data && zones && records && n >= 1 && W >= 0 && nzone >= 0 && nzone <= 0x7fffffff, "zone_stats_f32(data, zones, n>=1, W>=0, 0<=nzone<2**31, records)");
    MH_TRY(require_device());
    hipStream_t s = 0;
    DevBuf d_d, d_z, d_r;
    MH_TRY(upload(d_d, data, (size_t)n * 4, s));
    MH_TRY(upload(d_z, zones, (size_t)n * 4, s));
    MH_TRY(d_r.alloc(sizeof(mhip_zone_record) * (size_t)(nzone + 1)));
    MH_TRY(zone_stats_dev(d_d.as<float>(), d_z.as<int32_t>(), n, W, nzone, d_r.as<mhip_zone_record>(), s));
    return download(records, d_r, sizeof(mhip_zone_record) * (size_t)(nzone + 1), s);
}

int mhip_polygonize_i32(const int32_t *labels, int64_t H, int64_t W, mhip_polygons **out)
{
    MH_ARG(labels && out, "polygonize_i32(labels, H, W, out)");
    MH_TRY(polygonize_check(H, W));
    const size_t n = (size_t)(H * W);
    size_t first = 0;      // (a raster without a label: no ring, no device)
    while (first < n && labels[first] == 0) ++first;
    if (first < n) MH_TRY(require_device());
    mhip_polygons *p = new (std::nothrow) mhip_polygons();
    if (!p) {
        set_error("polygonize: out of host memory");
        return MHIP_EHIP;
    }
    if (first < n) {
        hipStream_t s = 0;
        DevBuf d_lab;
        int rc = hipGetDevice(&p->device) == hipSuccess ? MHIP_OK : MHIP_EHIP;
        if (rc == MHIP_OK) rc = upload(d_lab, labels, 4 * n, s);
        if (rc == MHIP_OK) rc = polygonize_dev(d_lab.as<int32_t>(), H, W, p->xy, p->ring_offsets, p->ring_label, &p->nring, &p->nvert, s);
        if (rc != MHIP_OK) {
            delete p;
            return rc;
        }
    }
    *out = p;
    return MHIP_OK;
}

int mhip_polygons_sizes(const mhip_polygons *p, int64_t *nring, int64_t *nvert)
{
    MH_ARG(p && nring && nvert, "polygons_sizes(polygons, nring, nvert)");
    *nring = p->nring;
    *nvert = p->nvert;
    return MHIP_OK;
}

int mhip_polygons_fetch(const mhip_polygons *p, int32_t *xy, int64_t *ring_offsets, int32_t *ring_label)
{
    MH_ARG(p && ring_offsets && (xy || p->nvert == 0) && (ring_label || p->nring == 0), "polygons_fetch(polygons, xy, ring_offsets, ring_label)");
    return polygons_fetch_dev(p, xy, ring_offsets, ring_label);
}

void mhip_polygons_free(mhip_polygons *p)
{
    if (p && p->device >= 0) (void)hipSetDevice(p->device);
    delete p;
}

int mhip_flowpaths_f64(const uint8_t *flowdir, const double *accum, const int32_t *labels, int64_t H, int64_t W, double threshold, mhip_flowpaths **out)
{
    MH_ARG(flowdir && accum && out, "flowpaths_f64(flowdir, accum, labels, H, W, threshold, out)");
    MH_TRY(flowpaths_check(H, W, threshold));
    MH_TRY(require_device());
    mhip_flowpaths *p = new (std::nothrow) mhip_flowpaths();
    if (!p) {
        set_error("flowpaths: out of host memory");
        return MHIP_EHIP;
    }
    const size_t n = (size_t)(H * W);
    hipStream_t s = 0;
    DevBuf d_fd, d_acc, d_lab;
    int rc = hipGetDevice(&p->device) == hipSuccess ? MHIP_OK : MHIP_EHIP;
    if (rc == MHIP_OK) rc = upload(d_fd, flowdir, n, s);
    if (rc == MHIP_OK) rc = upload(d_acc, accum, 8 * n, s);
    if (rc == MHIP_OK && labels) rc = upload(d_lab, labels, 4 * n, s);
    if (rc == MHIP_OK) rc = flowpaths_dev(d_fd.as<uint8_t>(), d_acc.as<double>(), labels ? d_lab.as<int32_t>() : nullptr, H, W, threshold, p, s);
    if (rc != MHIP_OK) {
        delete p;
        return rc;
    }
    *out = p;
    return MHIP_OK;
}

int mhip_flowpaths_sizes(const mhip_flowpaths *p, int64_t *nreach, int64_t *nvert, int64_t *unresolved)
{
    MH_ARG(p && nreach && nvert && unresolved, "flowpaths_sizes(flowpaths, nreach, nvert, unresolved)");
    *nreach = p->nreach;
    *nvert = p->nvert;
    *unresolved = p->unresolved;
    return MHIP_OK;
}

int mhip_flowpaths_fetch(const mhip_flowpaths *p, int32_t *xy, int64_t *reach_offsets, mhip_reach_record *records)
{
    MH_ARG(p && reach_offsets && (xy || p->nvert == 0) && (records || p->nreach == 0), "flowpaths_fetch(flowpaths, xy, reach_offsets, records)");
    return flowpaths_fetch_dev(p, xy, reach_offsets, records);
}

void mhip_flowpaths_free(mhip_flowpaths *p)
{
    if (p && p->device >= 0) (void)hipSetDevice(p->device);
    delete p;
}

int mhip_reach_catchments_i32(const uint8_t *flowdir, const double *accum, const int32_t *labels, int64_t H, int64_t W, double threshold,
                              int32_t *out_catch, mhip_flowpaths **out_reaches, int64_t *assigned)
{
    MH_ARG(flowdir && accum && out_catch && out_reaches, "reach_catchments_i32(flowdir, accum, labels, H, W, threshold, out_catch, out_reaches, assigned)");
    MH_TRY(flowpaths_check(H, W, threshold));
    MH_TRY(require_device());
    mhip_flowpaths *p = new (std::nothrow) mhip_flowpaths();
    if (!p) {
        set_error("reach_catchments: out of host memory");
        return MHIP_EHIP;
    }
    const size_t n = (size_t)(H * W);
    hipStream_t s = 0;
    DevBuf d_fd, d_acc, d_lab, d_catch;
    int rc = hipGetDevice(&p->device) == hipSuccess ? MHIP_OK : MHIP_EHIP;
    if (rc == MHIP_OK) rc = upload(d_fd, flowdir, n, s);
    if (rc == MHIP_OK) rc = upload(d_acc, accum, 8 * n, s);
    if (rc == MHIP_OK && labels) rc = upload(d_lab, labels, 4 * n, s);
    if (rc == MHIP_OK) rc = d_catch.alloc(4 * n);
    if (rc == MHIP_OK)
        rc = reach_catchments_dev(d_fd.as<uint8_t>(), d_acc.as<double>(), labels ? d_lab.as<int32_t>() : nullptr, H, W, threshold, d_catch.as<int32_t>(), p,
                                  assigned, s);
    if (rc == MHIP_OK) rc = download(out_catch, d_catch, 4 * n, s);
    if (rc != MHIP_OK) {
        delete p;
        return rc;
    }
    *out_reaches = p;
    return MHIP_OK;
}

int mhip_inundate_f32(const float *hand, const int32_t *catch_, int64_t n, int64_t W, int64_t nreach, const float *stage, float nodata, float *out_depth,
                      mhip_zone_record *records)
{
    MH_ARG(hand && catch_ && stage && out_depth && n >= 1 && W >= 0 && nreach >= 0 && nreach < 0x7fffffff,
           "inundate_f32(hand, catch, n>=1, W>=0, 0<=nreach<2**31-1, stage, nodata, out_depth, records)");
    MH_TRY(require_device());
    hipStream_t s = 0;
    DevBuf d_h, d_c, d_s, d_d, d_r;
    MH_TRY(upload(d_h, hand, (size_t)n * 4, s));
    MH_TRY(upload(d_c, catch_, (size_t)n * 4, s));
    MH_TRY(upload(d_s, stage, ((size_t)nreach + 1) * 4, s));
    MH_TRY(d_d.alloc((size_t)n * 4));
    if (records) MH_TRY(d_r.alloc(sizeof(mhip_zone_record) * (size_t)(nreach + 1)));
    MH_TRY(inundate_dev(d_h.as<float>(), d_c.as<int32_t>(), n, W, nreach, d_s.as<float>(), nodata, d_d.as<float>(),
                        records ? d_r.as<mhip_zone_record>() : nullptr, s));
    if (records) MH_HIP(hipMemcpyAsync(records, d_r.p, sizeof(mhip_zone_record) * (size_t)(nreach + 1), hipMemcpyDeviceToHost, s));
    return download(out_depth, d_d, (size_t)n * 4, s);
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

/* ---- runoff-weighted flow accumulation (wacc.hip): the stand-alone call and the readers of a context's snapshot ------------------- */
int mhip_weighted_accum_u32(const uint8_t *flowdir, const uint32_t *weight, const int32_t *zones, int64_t H, int64_t W, int64_t nzone, uint64_t *out,
                            uint64_t *zone_sums, int64_t *unresolved)
{
    MH_ARG(flowdir && weight && out && unresolved && (zones != nullptr) == (zone_sums != nullptr),
           "weighted_accum_u32(flowdir, weight, zones, H, W, nzone, out, zone_sums, unresolved): zones and zone_sums go together");
    MH_TRY(wacc_check(H, W, nzone, zones != nullptr));
    MH_TRY(require_device());
    const size_t n = (size_t)(H * W);
    hipStream_t s = 0;
    DevBuf d_fd, d_w, d_z, d_out, d_sums;
    MH_TRY(upload(d_fd, flowdir, n, s));
    MH_TRY(upload(d_w, weight, 4 * n, s));
    if (zones) {
        MH_TRY(upload(d_z, zones, 4 * n, s));
        MH_TRY(d_sums.alloc(8 * (size_t)(nzone + 1)));
    }
    MH_TRY(d_out.alloc(8 * n));
    MH_TRY(wacc_dev(d_fd.as<uint8_t>(), d_w.as<uint32_t>(), zones ? d_z.as<int32_t>() : nullptr, H, W, nzone, d_out.as<unsigned long long>(),
                    zones ? d_sums.as<unsigned long long>() : nullptr, unresolved, s));
    if (zones) MH_HIP(hipMemcpyAsync(zone_sums, d_sums.p, 8 * (size_t)(nzone + 1), hipMemcpyDeviceToHost, s));
    return download(out, d_out, 8 * n, s);
}

int mhip_wacc_info(const mhip_wacc *p, int64_t *H, int64_t *W, int64_t *nzone, int64_t *unresolved)
{
    MH_ARG(p && H && W && nzone && unresolved, "wacc_info(wacc, H, W, nzone, unresolved)");
    *H = p->H;
    *W = p->W;
    *nzone = p->nzone;
    *unresolved = p->unresolved;
    return MHIP_OK;
}

int mhip_wacc_rows_u64(const mhip_wacc *p, int64_t row0, int64_t nrows, uint64_t *dst)
{
    MH_ARG(p && dst && row0 >= 0 && nrows >= 1 && row0 <= p->H - nrows, "wacc_rows_u64(wacc, row0, nrows, dst): rows inside the raster");
    MH_HIP(hipSetDevice(p->device));
    hipStream_t s = 0;      // (raw rows: a copy, no kernel)
    MH_HIP(hipMemcpyAsync(dst, p->acc.as<uint64_t>() + row0 * p->W, 8 * (size_t)(nrows * p->W), hipMemcpyDeviceToHost, s));
    MH_HIP(stream_sync(s));
    return MHIP_OK;
}

int mhip_wacc_rows_f64(const mhip_wacc *p, int64_t row0, int64_t nrows, double div, double mul, double nodata, double *dst)
{
    MH_ARG(p && dst && row0 >= 0 && nrows >= 1 && row0 <= p->H - nrows, "wacc_rows_f64(wacc, row0, nrows, div, mul, nodata, dst): rows inside the raster");
    MH_ARG(div != 0.0 && div == div, "wacc_rows_f64: div must not be 0 or NaN");
    return wacc_rows_f64_dev(p, row0, nrows, div, mul, nodata, dst);
}

int mhip_wacc_zone_sums(const mhip_wacc *p, uint64_t *dst)
{
    MH_ARG(p && dst, "wacc_zone_sums(wacc, dst)");
    MH_ARG(p->nzone >= 0, "wacc_zone_sums: the result was made without zones");
    MH_HIP(hipSetDevice(p->device));
    hipStream_t s = 0;
    MH_HIP(hipMemcpyAsync(dst, p->sums.p, 8 * (size_t)(p->nzone + 1), hipMemcpyDeviceToHost, s));
    MH_HIP(stream_sync(s));
    return MHIP_OK;
}

int mhip_wacc_work(const mhip_wacc *p, int64_t *rounds, int64_t *visits, int64_t *tiles)
{
    MH_ARG(p && rounds && visits && tiles, "wacc_work(wacc, rounds, visits, tiles)");
    *rounds = p->rounds;
    *visits = p->visits;
    *tiles = p->tiles;
    return MHIP_OK;
}

void mhip_wacc_free(mhip_wacc *p)
{
    if (p && p->device >= 0) (void)hipSetDevice(p->device);
    delete p;
}

/* ---- multiple-flow-direction accumulation (mfd.hip): the two stand-alone calls --------------------------------------------------- */
int mhip_mfd_fractions_f64(const double *z, int64_t H, int64_t W, int32_t exponent, uint16_t *out)
{
    MH_ARG(z && out, "mfd_fractions_f64(z, H, W, exponent, out)");
    MH_ARG(exponent >= 1 && exponent <= 8, "mfd_fractions_f64: exponent in [1, 8]");
    MH_TRY(mfd_check(H, W));
    MH_TRY(require_device());
    const size_t n = (size_t)(H * W);
    hipStream_t s = 0;
    DevBuf d_z, d_out;
    MH_TRY(upload(d_z, z, 8 * n, s));
    MH_TRY(d_out.alloc(16 * n));
    MH_TRY(mfd_fractions_dev(d_z.as<double>(), H, W, exponent, d_out.as<uint16_t>(), s));
    return download(out, d_out, 16 * n, s);
}

int mhip_mfd_accum_u32(const uint16_t *fractions, const uint32_t *weight, int64_t H, int64_t W, uint64_t *out, int64_t *unresolved)
{
    MH_ARG(fractions && weight && out && unresolved, "mfd_accum_u32(fractions, weight, H, W, out, unresolved)");
    MH_TRY(mfd_check(H, W));
    MH_TRY(require_device());
    const size_t n = (size_t)(H * W);
    hipStream_t s = 0;
    DevBuf d_fr, d_w, d_out;
    MH_TRY(upload(d_fr, fractions, 16 * n, s));
    MH_TRY(upload(d_w, weight, 4 * n, s));
    MH_TRY(d_out.alloc(8 * n));
    const int rc = mfd_accum_dev(d_fr.as<uint16_t>(), d_w.as<uint32_t>(), 0u, H, W, d_out.as<unsigned long long>(), unresolved, nullptr, s);
    if (rc != MHIP_OK) {
        (void)stream_sync(s);      // (the uploads may still read the caller's arrays)
        return rc;
    }
    return download(out, d_out, 8 * n, s);
}

}  // extern "C"
