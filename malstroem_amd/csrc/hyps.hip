// hyps.hip -- final state of the bluespots: hypsometry tables, water levels, final depth raster (gfx950).
//
// No reference counterpart (the reference ends with the rain events, rain.py:48-87); semantics, the bound of the table's
// model volume and its proof are in DESIGN.md 9.  In short, for labelled depths d >= 0 and a vertical resolution res:
//   layout  label l >= 1 owns nbins[l] = floor(max(dmax[l], 0) / res) + 1 table entries, [offsets[l], offsets[l + 1])
//   table   cell d of label l -> entry offsets[l] + clamp(floor(double(d) / res), 0, nbins[l] - 1): count, sum of double(d)
//   level   draw-down t below the spill level at which the table's volume sum count_k * max(0, sum_k / count_k - t) equals q
//   final   out = float(max(0, double(d) - t[label])), wet cells counted per label
// The table kernel is label_ops.hip's stats_kernel with a finer key: a thread follows its column down a 32 x 256 tile and keeps
// the vertical run of equal (label, bin) it is in in registers, finished runs go to the tile's LDS table, the table leaves as one
// pair of atomics per (entry, tile); a run that finds no slot goes to the global atomics itself and is counted.
// -ffp-contract=off (Makefile): the divisions, sums and differences below are the IEEE operations the tests' NumPy model performs.
#include "common.hpp"

namespace mh {
namespace {

// number of table entries of a label whose largest depth is dmax: floor(dmax / res) + 1; a label without cells (dmax = -inf),
// a negative or NaN dmax: one entry; 2**31 entries (beyond HYPS_MAX_BINS: the caller refuses) for a quotient that leaves int32
__device__ __forceinline__ int64_t hyps_nbins(double dmax, double res)
{
    const double x = dmax / res;
    if (!(x >= 0.0)) return 1;
    if (x >= 2147483648.0) return (int64_t)1 << 31;
    return (int64_t)x + 1;
}

// offsets[0] = offsets[1] = 0, offsets[l + 1] = offsets[l] + nbins[l] in three launches: the sums of blocks of 4096 labels (a thread 16
// labels in a row), their exclusive scan by one workgroup, and the offsets from a block's prefix and the scan of its threads' sums.
// (One workgroup over all labels was 14 ms for the 4.6 M bluespots of the 16384^2 benchmark DEM.)
constexpr int LAY_PER_THREAD = 16, LAY_PER_BLOCK = 256 * LAY_PER_THREAD;
__device__ __forceinline__ int64_t layout_thread_sum(const double *__restrict__ dmax, int64_t stride, int64_t nlab, double res, int64_t lo)
{
    int64_t sum = 0;
    for (int64_t l = lo; l < lo + LAY_PER_THREAD && l <= nlab; ++l) sum += hyps_nbins(dmax[l * stride], res);
    return sum;
}
__global__ __launch_bounds__(256) void hyps_layout_sums_kernel(const double *__restrict__ dmax, int64_t stride, int64_t nlab, double res,
                                                              int64_t *__restrict__ blocksum)
{
    __shared__ int64_t part[4];
    int64_t sum = layout_thread_sum(dmax, stride, nlab, res, 1 + (int64_t)blockIdx.x * LAY_PER_BLOCK + (int64_t)threadIdx.x * LAY_PER_THREAD);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) blocksum[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}
// x[0 .. n) -> its exclusive prefix sums in place, the total to *total: one workgroup, every thread a contiguous range
__global__ __launch_bounds__(1024) void hyps_scan_kernel(int64_t *x, int64_t n, int64_t *total)
{
    __shared__ int64_t part[1024];
    const int64_t per = cdiv(n, 1024);
    const int64_t lo = (int64_t)threadIdx.x * per;
    const int64_t hi = lo + per < n ? lo + per : n;
    int64_t sum = 0;
    for (int64_t i = lo; i < hi; ++i) sum += x[i];
    part[threadIdx.x] = sum;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {      // inclusive scan of the threads' sums
        const int64_t add = (int)threadIdx.x >= o ? part[threadIdx.x - o] : 0;
        __syncthreads();
        part[threadIdx.x] += add;
        __syncthreads();
    }
    int64_t run = part[threadIdx.x] - sum;
    for (int64_t i = lo; i < hi; ++i) {
        const int64_t v = x[i];
        x[i] = run;
        run += v;
    }
    if (threadIdx.x == 0) *total = part[1023];
}
__global__ __launch_bounds__(256) void hyps_layout_offsets_kernel(const double *__restrict__ dmax, int64_t stride, int64_t nlab, double res,
                                                                 const int64_t *__restrict__ blockprefix, int64_t *__restrict__ offsets)
{
    __shared__ int64_t part[256];
    const int64_t lo = 1 + (int64_t)blockIdx.x * LAY_PER_BLOCK + (int64_t)threadIdx.x * LAY_PER_THREAD;
    const int64_t sum = layout_thread_sum(dmax, stride, nlab, res, lo);
    part[threadIdx.x] = sum;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        const int64_t add = (int)threadIdx.x >= o ? part[threadIdx.x - o] : 0;
        __syncthreads();
        part[threadIdx.x] += add;
        __syncthreads();
    }
    int64_t run = blockprefix[blockIdx.x] + part[threadIdx.x] - sum;
    for (int64_t l = lo; l < lo + LAY_PER_THREAD && l <= nlab; ++l) {
        offsets[l] = run;
        run += hyps_nbins(dmax[l * stride], res);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) offsets[0] = 0;
}

__global__ __launch_bounds__(256) void hyps_init_kernel(uint32_t *counts, double *sums, int64_t total, unsigned int *bad, unsigned long long *spills)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        counts[i] = 0u;
        sums[i] = 0.0;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        *bad = 0u;
        *spills = 0ull;
    }
}

// ---- the table ----------------------------------------------------------------------------------------------------------------
// 1024 slots = 16 KB: ten workgroups' worth of LDS per CU, the registers decide.  A tile of a deep lake at res = 0.05 m holds more
// entries than that (8192 cells, a bin per 5 cm of depth and label); what finds no slot within table_slot's 16 probes goes to the
// global atomics run by run -- correct, slower, and counted in *spills.
constexpr int HYPS_TS = 1024;
__global__ __launch_bounds__(256) void hyps_table_kernel(const float *__restrict__ data, const int32_t *__restrict__ lab, TileGeom g, int64_t nlab,
                                                        double res, const int64_t *__restrict__ offsets, int64_t total, uint32_t *counts,
                                                        double *sums, unsigned int *bad, unsigned long long *spills)
{
    __shared__ int keys[HYPS_TS];
    __shared__ unsigned int tcnt[HYPS_TS];
    __shared__ double tsum[HYPS_TS];
    unsigned int nspill = 0, any_bad = 0;
    const int64_t ntiles = g.ntr * g.ntc;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        for (int k = threadIdx.x; k < HYPS_TS; k += 256) {
            keys[k] = -1;
            tcnt[k] = 0u;
            tsum[k] = 0.0;
        }
        __syncthreads();
        const int64_t tr = tile / g.ntc, tc = tile - tr * g.ntc;
        const int64_t col = tc * 256 + threadIdx.x;
        // the run this thread is in: table entry (< 0: none), sum, count
        int ckey = -1;
        double csum = 0.0;
        unsigned int ccnt = 0;
        auto end_run = [&]() {
            const int h = table_slot<HYPS_TS>(keys, ckey);
            if (h >= 0) {
                atomicAdd(&tsum[h], csum);
                atomicAdd(&tcnt[h], ccnt);
            } else {
                atomicAdd(&sums[ckey], csum);
                atomicAdd(&counts[ckey], ccnt);
                ++nspill;
            }
        };
        static_assert(TR % 4 == 0, "rows in batches of four");
        for (int r4 = 0; r4 < TR; r4 += 4) {
            int32_t lq[4];           // four rows' loads in flight
            float dq[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int64_t i = (tr * TR + r4 + u) * g.W + col;
                const bool valid = col < g.W && i < g.n;
                lq[u] = valid ? lab[i] : 0;
                dq[u] = valid ? data[i] : 0.0f;
                if (lq[u] < 0 || lq[u] > nlab) {
                    any_bad = 1;
                    lq[u] = 0;
                }
            }
            // ... and the four rows' table ranges (background: offsets[0] = offsets[1] = 0): eight gathers in flight instead of one inside the
            // branch where a label changes (2.41 -> 2.37 ms at 16384^2: not where this kernel's time is)
            int64_t o0[4], o1[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                o0[u] = offsets[lq[u]];
                o1[u] = offsets[lq[u] + 1];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int32_t l = lq[u];
                const double v = (double)dq[u];
                int key = -1;
                if (l > 0) {
                    const int64_t coff = o0[u], nb = o1[u] - coff;
                    const int cnb = (nb >= 1 && nb <= ((int64_t)1 << 31) - 1 && coff >= 0 && coff + nb <= total) ? (int)nb : 0;
                    if (!cnb) any_bad = 1;       // (offsets that are no layout of these labels: nothing is written)
                    if (cnb) {
                        const double x = v / res;
                        // floor of a quotient >= 0 is its truncation; below 1 (negative and NaN too): the first entry
                        const int k = x >= 1.0 ? (x < (double)cnb ? (int)x : cnb - 1) : 0;
                        key = (int)coff + k;
                    }
                }
                if (key != ckey) {
                    if (ckey >= 0) end_run();
                    ckey = key;
                    csum = 0.0;
                    ccnt = 0;
                }
                if (key >= 0) {
                    csum += v;
                    ++ccnt;
                }
            }
        }
        if (ckey >= 0) end_run();
        __syncthreads();
        for (int k = threadIdx.x; k < HYPS_TS; k += 256) {
            const int key = keys[k];
            if (key < 0) continue;
            atomicAdd(&sums[key], tsum[k]);
            atomicAdd(&counts[key], tcnt[k]);
        }
        __syncthreads();
    }
    if (any_bad) atomicOr(bad, 1u);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nspill += __shfl_xor(nspill, o);
    if ((threadIdx.x & 63) == 0 && nspill) atomicAdd(spills, (unsigned long long)nspill);
}

// ---- the levels ---------------------------------------------------------------------------------------------------------------
// One thread per label.  The order of every sum is part of the contract: entries from the deepest down.
__global__ __launch_bounds__(256) void hyps_levels_kernel(int64_t nlab, const int64_t *__restrict__ offsets, const uint32_t *__restrict__ counts,
                                                         const double *__restrict__ sums, const double *__restrict__ dmax, int64_t stride,
                                                         const double *__restrict__ q, mhip_final_record *__restrict__ rec)
{
    const int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (l > nlab) return;
    mhip_final_record r;
    r.drawdown = 0.0;
    r.dmax_final = 0.0;
    r.qmodel = 0.0;
    r.wet_cells = 0;
    if (l >= 1) {
        const int64_t lo = offsets[l], hi = offsets[l + 1];
        double dm = dmax[l * stride];
        if (!(dm > 0.0)) dm = 0.0;
        double full = 0.0;
        for (int64_t k = hi - 1; k >= lo; --k) full += sums[k];
        const double ql = q[l];
        double t;
        if (ql >= full) {
            t = 0.0;
        } else if (!(ql > 0.0)) {
            t = dm;
        } else {
            // entries >= k stand above the level while it lies between the mean depths of k and of the next entry with cells below
            // it: there the table holds S - C * t
            double C = 0.0, S = 0.0;
            bool have = false, found = false;
            t = 0.0;
            for (int64_t k = hi - 1; k >= lo; --k) {
                const uint32_t c = counts[k];
                if (!c) continue;
                if (have) {
                    const double lower = sums[k] / (double)c;
                    const double cand = (S - ql) / C;
                    if (cand >= lower) {
                        t = cand;
                        found = true;
                        break;
                    }
                }
                C += (double)c;
                S += sums[k];
                have = true;
            }
            if (!found) t = (S - ql) / C;      // below the shallowest entry with cells the segment ends at 0
        }
        double acc = 0.0;
        for (int64_t k = hi - 1; k >= lo; --k) {
            const uint32_t c = counts[k];
            if (!c) continue;
            const double x = sums[k] / (double)c - t;
            if (x > 0.0) acc += (double)c * x;
        }
        const double left = dm - t;
        r.drawdown = t;
        r.dmax_final = left > 0.0 ? left : 0.0;
        r.qmodel = acc;
    }
    rec[l] = r;
}

// ---- the final depths -----------------------------------------------------------------------------------------------------------
// The same tiles; a thread owns V consecutive columns (V = 4: 16-byte loads and stores, rows of a multiple of four cells) of every
// V-th row of the tile and counts the wet cells of the run of equal labels it is in; runs go to the tile's LDS table of counts,
// the table leaves as one atomic per (label, tile).
constexpr int FIN_TS = 512;
template <int V>      // 4 or 1
__global__ __launch_bounds__(256) void final_depths_kernel(const float *__restrict__ data, const int32_t *__restrict__ lab, TileGeom g, int64_t nlab,
                                                          mhip_final_record *rec, float *__restrict__ out, unsigned int *bad)
{
    __shared__ int keys[FIN_TS];
    __shared__ unsigned int tcnt[FIN_TS];
    constexpr int TPR = 256 / V;      // threads per tile row; V rows per pass of the workgroup
    const int tx = threadIdx.x % TPR, ty = threadIdx.x / TPR;
    unsigned int any_bad = 0;
    const int64_t ntiles = g.ntr * g.ntc;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        for (int k = threadIdx.x; k < FIN_TS; k += 256) {
            keys[k] = -1;
            tcnt[k] = 0u;
        }
        __syncthreads();
        const int64_t tr = tile / g.ntc, tc = tile - tr * g.ntc;
        const int64_t col = tc * 256 + (int64_t)tx * V;
        int32_t cl = 0;          // the label of the run, its draw-down, the run's wet cells
        double ct = 0.0;
        unsigned int cw = 0;
        auto end_run = [&]() {
            if (!cw) return;
            const int h = table_slot<FIN_TS>(keys, cl);
            if (h >= 0) atomicAdd(&tcnt[h], cw);
            else atomicAdd(reinterpret_cast<unsigned long long *>(&rec[cl].wet_cells), (unsigned long long)cw);
        };
        for (int r = ty; r < TR; r += V) {
            const int64_t i = (tr * TR + r) * g.W + col;
            if (!(col < g.W && i < g.n)) continue;       // (V = 4: W is a multiple of four, the whole vector is inside)
            int32_t lv[V];
            float dv[V], ov[V];
            if constexpr (V == 4) {
                const int4 l4 = *reinterpret_cast<const int4 *>(lab + i);
                const float4 d4 = *reinterpret_cast<const float4 *>(data + i);
                lv[0] = l4.x; lv[1] = l4.y; lv[2] = l4.z; lv[3] = l4.w;
                dv[0] = d4.x; dv[1] = d4.y; dv[2] = d4.z; dv[3] = d4.w;
            } else {
                lv[0] = lab[i];
                dv[0] = data[i];
            }
#pragma unroll
            for (int e = 0; e < V; ++e) {
                int32_t l = lv[e];
                if (l < 0 || l > nlab) {
                    any_bad = 1;
                    l = 0;
                }
                float o = 0.0f;
                if (l > 0) {
                    if (l != cl) {
                        end_run();
                        cl = l;
                        ct = rec[l].drawdown;
                        cw = 0;
                    }
                    const double x = (double)dv[e] - ct;
                    o = x > 0.0 ? (float)x : 0.0f;
                    cw += o > 0.0f ? 1u : 0u;
                }
                ov[e] = o;
            }
            if constexpr (V == 4) *reinterpret_cast<float4 *>(out + i) = make_float4(ov[0], ov[1], ov[2], ov[3]);
            else out[i] = ov[0];
        }
        end_run();
        __syncthreads();
        for (int k = threadIdx.x; k < FIN_TS; k += 256)
            if (keys[k] >= 0 && tcnt[k]) atomicAdd(reinterpret_cast<unsigned long long *>(&rec[keys[k]].wet_cells), (unsigned long long)tcnt[k]);
        __syncthreads();
    }
    if (any_bad) atomicOr(bad, 1u);
}

__global__ void word_zero_kernel(unsigned int *w) { *w = 0u; }

int hyps_check_bad(DevBuf &bad, hipStream_t s, const char *what)
{
    unsigned int h = 0;
    MH_HIP(hipMemcpyAsync(&h, bad.p, sizeof(h), hipMemcpyDeviceToHost, s));
    MH_HIP(stream_sync(s));
    if (h) {
        set_error("%s: label outside [0, nlabels], or offsets that are no layout of these labels", what);
        return MHIP_EINVAL;
    }
    return MHIP_OK;
}

}  // namespace

int hyps_layout_dev(const double *d_dmax, int64_t stride, int64_t nlab, double res, int64_t *d_offsets, int64_t *total, hipStream_t s)
{
    const int64_t nblocks = cdiv(nlab, LAY_PER_BLOCK) > 0 ? cdiv(nlab, LAY_PER_BLOCK) : 1;
    DevBuf bs;
    MH_TRY(bs.alloc(8 * (size_t)nblocks));
    hipLaunchKernelGGL(hyps_layout_sums_kernel, dim3((unsigned)nblocks), dim3(256), 0, s, d_dmax, stride, nlab, res, bs.as<int64_t>());
    hipLaunchKernelGGL(hyps_scan_kernel, dim3(1), dim3(1024), 0, s, bs.as<int64_t>(), nblocks, d_offsets + nlab + 1);
    hipLaunchKernelGGL(hyps_layout_offsets_kernel, dim3((unsigned)nblocks), dim3(256), 0, s, d_dmax, stride, nlab, res, (const int64_t *)bs.p, d_offsets);
    MH_HIP(hipGetLastError());
    int64_t t = 0;
    MH_HIP(hipMemcpyAsync(&t, d_offsets + nlab + 1, 8, hipMemcpyDeviceToHost, s));
    MH_HIP(stream_sync(s));
    if (t > HYPS_MAX_BINS) {
        set_error("hypsometry: %lld table entries at this resolution, the limit is %lld (2**30: 12 bytes each on the device) -- "
                  "or an infinite depth", (long long)t, (long long)HYPS_MAX_BINS);
        return MHIP_ELIMIT;
    }
    *total = t;
    return MHIP_OK;
}

int hyps_table_dev(const float *d_data, const int32_t *d_labels, int64_t n, int64_t W, int64_t nlab, double res, const int64_t *d_offsets,
                   int64_t total, uint32_t *d_counts, double *d_sums, int64_t *lds_spills, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1)
{
    DevBuf bad, spills;
    MH_TRY(bad.alloc(4));
    MH_TRY(spills.alloc(8));
    const unsigned gi = (unsigned)(cdiv(total, 256) < 2048 ? (total > 0 ? cdiv(total, 256) : 1) : 2048);
    hipLaunchKernelGGL(hyps_init_kernel, dim3(gi), dim3(256), 0, s, d_counts, d_sums, total, bad.as<unsigned int>(), spills.as<unsigned long long>());
    const TileGeom g = tile_geom(n, W);
    if (ev0) MH_HIP(hipEventRecord(ev0, s));
    hipLaunchKernelGGL(hyps_table_kernel, dim3(tile_grid(g)), dim3(256), 0, s, d_data, d_labels, g, nlab, res, d_offsets, total, d_counts, d_sums,
                       bad.as<unsigned int>(), spills.as<unsigned long long>());
    if (ev1) MH_HIP(hipEventRecord(ev1, s));
    MH_HIP(hipGetLastError());
    unsigned long long h = 0;
    MH_HIP(hipMemcpyAsync(&h, spills.p, 8, hipMemcpyDeviceToHost, s));
    MH_TRY(hyps_check_bad(bad, s, "label_hypsometry"));      // synchronises the stream
    if (lds_spills) *lds_spills = (int64_t)h;
    return MHIP_OK;
}

int hyps_levels_dev(int64_t nlab, const int64_t *d_offsets, const uint32_t *d_counts, const double *d_sums, const double *d_dmax, int64_t stride,
                    const double *d_q, mhip_final_record *d_rec, hipStream_t s)
{
    hipLaunchKernelGGL(hyps_levels_kernel, dim3((unsigned)cdiv(nlab + 1, 256)), dim3(256), 0, s, nlab, d_offsets, d_counts, d_sums, d_dmax, stride,
                       d_q, d_rec);
    MH_HIP(hipGetLastError());
    return MHIP_OK;
}

int final_depths_dev(const float *d_data, const int32_t *d_labels, int64_t n, int64_t W, int64_t nlab, mhip_final_record *d_rec, float *d_out,
                     hipStream_t s, hipEvent_t ev0, hipEvent_t ev1)
{
    DevBuf bad;
    MH_TRY(bad.alloc(4));
    hipLaunchKernelGGL(word_zero_kernel, dim3(1), dim3(1), 0, s, bad.as<unsigned int>());
    const TileGeom g = tile_geom(n, W);
    const bool vec = W > 0 && n % W == 0 && W % 4 == 0 && ((uintptr_t)d_data | (uintptr_t)d_labels | (uintptr_t)d_out) % 16 == 0;
    if (ev0) MH_HIP(hipEventRecord(ev0, s));
    if (vec)
        hipLaunchKernelGGL(final_depths_kernel<4>, dim3(tile_grid(g)), dim3(256), 0, s, d_data, d_labels, g, nlab, d_rec, d_out, bad.as<unsigned int>());
    else
        hipLaunchKernelGGL(final_depths_kernel<1>, dim3(tile_grid(g)), dim3(256), 0, s, d_data, d_labels, g, nlab, d_rec, d_out, bad.as<unsigned int>());
    if (ev1) MH_HIP(hipEventRecord(ev1, s));
    MH_HIP(hipGetLastError());
    return hyps_check_bad(bad, s, "final_depths");
}

}  // namespace mh
