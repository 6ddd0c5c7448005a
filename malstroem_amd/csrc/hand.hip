// hand.hip -- height above the nearest drainage and the distance to it along the flow path (gfx950).
//
// No reference counterpart.  A cell is a DRAINAGE cell when accum >= threshold (float64; a NaN is none) or, with labels, its label is
// != 0.  D(c): the first drainage cell on the downstream walk from c, c included, after no(c) orthogonal / nd(c) diagonal steps.  A
// cell whose walk ends before it meets one -- at a code > 7, at a step out of the raster, on a flow cycle -- is UNDRAINED.
//   hand   elev[c] - elev[D(c)] as one float32 subtraction (a NaN result is the canonical quiet NaN); `nodata` where undrained
//   dist   float32((float64(no) + float64(nd) * 1.4142135623730951) * scale); -1 where undrained
// The walk is flowdist.hip's (flow_walk_dev, common.hpp) with the drainage test: its tile pass ends a walk at a drainage cell, and a walk
// that ends at anything else leaves the tile's cells as FD_NONE, which is what a flow cycle leaves.  The final pass here fetches the
// elevation of the cell the walk ended at.
//
// The reach catchments (tests/_reachcatch.py) run the same walk and end in a sibling of the final pass,
// catch_final_kernel, which fetches the reach of that cell from the raster flowpaths.hip's fp_reachcell_kernel wrote.
#include <algorithm>
#include <cmath>

#include "common.hpp"

namespace mh {
namespace {

constexpr int64_t CATCH_MAX_BLOCKS = 4096;      // of catch_final_kernel: 16 workgroups of 256 a CU

// ---- final pass ------------------------------------------------------------------------------------------------------------------
// V cells a thread (V = 4: n is a multiple of four, 16-byte accesses): 8 B scratch + 4 B elevation in, one gather of the elevation at
// the end of the walk, 4 B (8 B with `dist`) out.  Every value is computed and then selected (DESIGN.md 11's miscompile note); the
// gather of an undrained cell goes to the cell itself, so that no index is ever out of the raster.
template <int V>
__global__ __launch_bounds__(256) void hand_final_kernel(const uint2 *__restrict__ S, const uint4 *__restrict__ Nn, const float *__restrict__ elev,
                                                        int64_t n, int64_t W, int ntc, double scale, float nodata, float *__restrict__ hand,
                                                        float *__restrict__ dist, unsigned long long *undrained)
{
    const int64_t i0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * V;
    unsigned int cnt = 0;
    if (i0 < n) {
        uint2 s[V];
        fd_load<V>(S, i0, s);
        float z[V];
        if constexpr (V == 4) {
            const float4 zv = *reinterpret_cast<const float4 *>(elev + i0);
            z[0] = zv.x; z[1] = zv.y; z[2] = zv.z; z[3] = zv.w;
        } else {
            z[0] = elev[i0];
        }
        float oh[V], od[V];
#pragma unroll
        for (int e = 0; e < V; ++e) {
            uint32_t no, nd;
            int32_t T;
            const bool ok = fd_resolve(s[e], Nn, (uint32_t)W, ntc, no, nd, T);
            const int64_t at = ok ? (int64_t)T : i0 + e;
            const float h = __fsub_rn(z[e], elev[at]);
            const float hc = h != h ? __int_as_float(0x7fc00000) : h;
            const float v = (float)__dmul_rn(fd_u(no, nd), scale);
            oh[e] = ok ? hc : nodata;
            od[e] = ok ? v : -1.0f;
            cnt += ok ? 0u : 1u;
        }
        if constexpr (V == 4) {
            *reinterpret_cast<float4 *>(hand + i0) = make_float4(oh[0], oh[1], oh[2], oh[3]);
            if (dist) *reinterpret_cast<float4 *>(dist + i0) = make_float4(od[0], od[1], od[2], od[3]);
        } else {
            hand[i0] = oh[0];
            if (dist) dist[i0] = od[0];
        }
    }
    fd_count_add(cnt, undrained);
}

// ---- final pass of the reach catchments ---------------------------------------------------------------------------
// hand_final_kernel's sibling: 8 B scratch in, one gather of the reach rc[D(c)] at the end of the walk, 4 B out; no elevation and no
// distance.  Every value is computed and then selected; the gather of an undrained cell goes to the cell itself.  `assigned`: the
// cells that hold a reach, one atomic per wavefront -- and so that this is a few thousand atomics on the one word and not one per 256
// cells where most cells are assigned (without labels nearly all are), the grid is bounded and a thread strides over the raster.
template <int V>
__global__ __launch_bounds__(256) void catch_final_kernel(const uint2 *__restrict__ S, const uint4 *__restrict__ Nn, const int32_t *__restrict__ rc,
                                                         int64_t n, int64_t W, int ntc, int32_t *__restrict__ out, unsigned long long *assigned)
{
    const int64_t step = (int64_t)gridDim.x * blockDim.x * V;
    unsigned int cnt = 0;      // (a thread sees fewer than 2**32 cells)
    for (int64_t i0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * V; i0 < n; i0 += step) {
        uint2 s[V];
        fd_load<V>(S, i0, s);
        int32_t o[V];
#pragma unroll
        for (int e = 0; e < V; ++e) {
            uint32_t no, nd;
            int32_t T;
            const bool ok = fd_resolve(s[e], Nn, (uint32_t)W, ntc, no, nd, T);
            const int64_t at = ok ? (int64_t)T : i0 + e;
            const int32_t k = rc[at];
            o[e] = ok ? k : 0;
            cnt += (ok && k > 0) ? 1u : 0u;
        }
        if constexpr (V == 4) *reinterpret_cast<int4 *>(out + i0) = make_int4(o[0], o[1], o[2], o[3]);
        else out[i0] = o[0];
    }
    fd_count_add(cnt, assigned);
}

}  // namespace

int hand_check(double threshold, double scale)
{
    MH_ARG(threshold >= 1.0 && threshold <= 1.7976931348623157e308, "hand: the threshold must be finite and >= 1");      // (false for NaN)
    MH_ARG(flow_distance_scale_ok(scale), "hand: the scale must be finite and > 0");
    return MHIP_OK;
}

int hand_dev(const uint8_t *d_fd, const double *d_acc, const float *d_elev, const int32_t *d_lab, int64_t H, int64_t W, double threshold, double scale,
             float nodata, float *d_hand, float *d_dist, int64_t *undrained, hipStream_t s)
{
    const int64_t n = H * W;
    FlowWalk w;
    MH_TRY(flow_walk_dev(d_fd, d_acc, d_lab, H, W, threshold, "hand", w, s));
    const bool vec = W % 4 == 0 && ((uintptr_t)d_hand | (uintptr_t)d_dist | (uintptr_t)d_elev | (uintptr_t)w.S.p) % 16 == 0;
    const dim3 grid((unsigned)cdiv(cdiv(n, vec ? 4 : 1), 256)), block(256);
    hipLaunchKernelGGL(pick_v(vec, hand_final_kernel<4>, hand_final_kernel<1>), grid, block, 0, s, w.S.as<uint2>(), w.cur, d_elev, n, W, (int)w.ntc, scale,
                       nodata, d_hand, d_dist, w.count());
    return flow_walk_count(w, undrained, nullptr, s);
}

// The reach catchments: the reaches and the reach of every stream cell by flowpaths_dev, the walk to D(c), one gather.
// The drainage cells of the walk and the stream cells of the reaches come from one threshold and one label raster, so the two masks
// agree by construction: a drainage cell that is no stream cell is a labelled one, and holds 0.
int reach_catchments_dev(const uint8_t *d_fd, const double *d_acc, const int32_t *d_lab, int64_t H, int64_t W, double threshold, int32_t *d_catch,
                         mhip_flowpaths *p, int64_t *assigned, hipStream_t s)
{
    const int64_t n = H * W;
    if (!flow_walk_fits(n)) {      // (before any device work: the limit of both engines)
        set_error("reach_catchments: %lld cells exceed the int32 index domain", (long long)n);
        return MHIP_ELIMIT;
    }
    DevBuf d_rc;
    MH_TRY(d_rc.alloc(4 * (size_t)n));
    MH_TRY(flowpaths_dev(d_fd, d_acc, d_lab, H, W, threshold, p, s, d_rc.as<int32_t>()));
    if (p->nreach == 0) {      // an empty mask, or cycles of the mask only: no walk ends in a reach
        MH_HIP(hipMemsetAsync(d_catch, 0, 4 * (size_t)n, s));
        MH_HIP(stream_sync(s));
        if (assigned) *assigned = 0;
        return MHIP_OK;
    }
    FlowWalk w;
    MH_TRY(flow_walk_dev(d_fd, d_acc, d_lab, H, W, threshold, "reach_catchments", w, s));
    const bool vec = W % 4 == 0 && ((uintptr_t)d_catch | (uintptr_t)d_rc.p | (uintptr_t)w.S.p) % 16 == 0;
    const dim3 grid((unsigned)std::min<int64_t>(cdiv(cdiv(n, vec ? 4 : 1), 256), CATCH_MAX_BLOCKS)), block(256);
    hipLaunchKernelGGL(pick_v(vec, catch_final_kernel<4>, catch_final_kernel<1>), grid, block, 0, s, w.S.as<uint2>(), w.cur, d_rc.as<int32_t>(), n, W,
                       (int)w.ntc, d_catch, w.count());
    return flow_walk_count(w, assigned, nullptr, s);
}

}  // namespace mh
