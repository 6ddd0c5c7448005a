// hand.hip -- height above the nearest drainage and the distance to it along the flow path (gfx950).
//
// No reference counterpart.  A cell is a DRAINAGE cell when accum >= threshold (float64; a NaN is none) or, with labels, its label is
// != 0.  D(c): the first drainage cell on the downstream walk from c, c included, after no(c) orthogonal / nd(c) diagonal steps.  A
// cell whose walk ends before it meets one -- at a code > 7, at a step out of the raster, on a flow cycle -- is UNDRAINED.
//   hand   elev[c] - elev[D(c)] as one float32 subtraction (a NaN result is the canonical quiet NaN); `nodata` where undrained
//   dist   float32((float64(no) + float64(nd) * 1.4142135623730951) * scale); -1 where undrained
// The engine is the flow distance's (flowdist.hip): its scratch word, its nodes, its perimeter jumps (fdist_jumps_dev) and its
// decoding (fd_resolve, common.hpp).  The tile pass and the final pass are siblings of that file's: the tile pass ends a walk at a
// drainage cell, and a walk that ends at anything else leaves the tile's cells as FD_NONE, which is what a flow cycle leaves -- the
// jumps and the decoding need no third kind of end.  The final pass fetches the elevation of the cell the walk ended at.
//
// The reach catchments (tests/_reachcatch.py) run the same tile pass and jumps (hand_walk) and end in a sibling of the final
// pass, catch_final_kernel, which fetches the reach of that cell from the raster flowpaths.hip's fp_reachcell_kernel wrote.
#include <algorithm>
#include <cmath>

#include "common.hpp"

namespace mh {
namespace {

constexpr int WT = WS_TILE;
constexpr int64_t CATCH_MAX_BLOCKS = 4096;      // of catch_final_kernel: 16 workgroups of 256 a CU

// ---- tile pass ---------------------------------------------------------------------------------------------------------------
// fdist_tile_kernel with the drainage test: one workgroup per 64 x 64 tile, a thread owns 16 consecutive cells of a tile row at the
// global ends, pull-only pointer doubling on (pointer, pair) in between.  LDS: ptr 8 KB + val 4 KB + pairs 16 KB = 28 KB.
__global__ __launch_bounds__(256) void hand_tile_kernel(const uint8_t *__restrict__ fd, const double *__restrict__ acc, const int32_t *__restrict__ lab,
                                                       double thr, uint2 *__restrict__ S, int64_t H, int64_t W, int ntc, uint4 *__restrict__ Nn)
{
    __shared__ uint16_t ptr[WT * WT];
    // V_DRAIN a drainage cell, V_DEAD a cell that is none and steps nowhere (no direction, or out of the raster), 0..7 the direction in
    // which the path leaves the tile here, V_MOVE a cell that steps on inside the tile
    __shared__ uint8_t val[WT * WT];
    __shared__ uint32_t pr[WT * WT];
    constexpr uint8_t V_DRAIN = 8, V_MOVE = 9, V_DEAD = 10;
    const int ti = blockIdx.x / ntc, tj = blockIdx.x - ti * ntc;
    const int64_t r0 = (int64_t)ti * WT, c0 = (int64_t)tj * WT;
    const int lr = threadIdx.x >> 2, lc0 = (threadIdx.x & 3) * 16;
    const int64_t r = r0 + lr, cbase = c0 + lc0;
    const bool vec = (W & 15) == 0 && r < H && cbase + 16 <= W;     // whole, 16-byte aligned group
    uint8_t code[16];
    uint32_t dmask = 0;      // my drainage cells
    if (vec) {
        const uint4 cv = *reinterpret_cast<const uint4 *>(fd + r * W + cbase);
        memcpy(code, &cv, 16);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const double2 av = *reinterpret_cast<const double2 *>(acc + r * W + cbase + 2 * q);
            dmask |= (av.x >= thr ? 1u : 0u) << (2 * q) | (av.y >= thr ? 2u : 0u) << (2 * q);
        }
        if (lab) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int4 lv = *reinterpret_cast<const int4 *>(lab + r * W + cbase + 4 * q);
                dmask |= (lv.x != 0 ? 1u : 0u) << (4 * q) | (lv.y != 0 ? 2u : 0u) << (4 * q) | (lv.z != 0 ? 4u : 0u) << (4 * q) |
                         (lv.w != 0 ? 8u : 0u) << (4 * q);
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const bool in = r < H && cbase + k < W;
            code[k] = in ? fd[r * W + cbase + k] : (uint8_t)8;
            if (in && (acc[r * W + cbase + k] >= thr || (lab && lab[r * W + cbase + k] != 0))) dmask |= 1u << k;
        }
    }
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int li = lr * WT + lc0 + k;
        uint16_t p = (uint16_t)li;
        uint8_t v = ((dmask >> k) & 1u) ? V_DRAIN : V_DEAD;      // (a cell outside the raster: V_DEAD, and nothing points at it)
        uint32_t a = 0;
        if (r < H && cbase + k < W && v == V_DEAD && code[k] <= 7u) {
            const int lr2 = lr + dir_dr((int)code[k]), lc2 = lc0 + k + dir_dc((int)code[k]);
            const int64_t nr = r0 + lr2, nc = c0 + lc2;
            if (nr >= 0 && nr < H && nc >= 0 && nc < W) {      // (else: the step leaves the raster, the walk ends undrained)
                if (lr2 >= 0 && lr2 < WT && lc2 >= 0 && lc2 < WT) {
                    p = (uint16_t)(lr2 * WT + lc2);
                    v = V_MOVE;
                    a = fd_step(code[k]);
                } else {
                    v = code[k];      // leaves the tile: the path continues at that entry cell
                }
            }
        }
        ptr[li] = p;
        val[li] = v;
        pr[li] = a;
    }
    __syncthreads();
    for (int round = 0; round < 12; ++round) {
        uint16_t np[16];
        uint32_t na[16];
        bool ch = false;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int li = k * 256 + (int)threadIdx.x;
            const uint16_t p = ptr[li], q = ptr[p];
            np[k] = q;
            na[k] = pr[p];      // (0 at a fixed point)
            ch |= q != p;
        }
        if (!__syncthreads_or(ch)) break;      // (every read of the round is behind this barrier)
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int li = k * 256 + (int)threadIdx.x;
            ptr[li] = np[k];
            pr[li] += na[k];
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < 16; k += 2) {
        uint2 o[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int li = lr * WT + lc0 + k + e;
            const int t = ptr[li];
            const unsigned vb = val[t];
            const int64_t tr = r0 + (t >> 6), tc = c0 + (t & 63);
            const bool leaves = vb <= 7u;      // (V_MOVE: a flow cycle inside the tile; V_DEAD: an end without drainage)
            const int32_t entry = (int32_t)((tr + dir_dr((int)(vb & 7u))) * W + tc + dir_dc((int)(vb & 7u)));
            const int32_t tgt = vb == V_DRAIN ? ((int32_t)(tr * W + tc) | FD_DONE) : leaves ? entry : FD_NONE;
            const uint32_t a = vb == V_DRAIN ? pr[li] : leaves ? pr[li] + fd_step(vb) : 0u;
            o[e] = make_uint2((uint32_t)tgt, a);
            const int slot = ws_perim_slot(lr, lc0 + k + e);
            if (slot >= 0) {
                const bool in = r < H && cbase + k + e < W;
                Nn[(int64_t)blockIdx.x * 256 + slot] = in ? make_uint4((uint32_t)tgt, a & 0xffffu, a >> 16, 0u) : make_uint4((uint32_t)FD_NONE, 0u, 0u, 0u);
            }
        }
        if (vec) {
            *reinterpret_cast<uint4 *>(S + r * W + cbase + k) = make_uint4(o[0].x, o[0].y, o[1].x, o[1].y);
        } else {
#pragma unroll
            for (int e = 0; e < 2; ++e)
                if (r < H && cbase + k + e < W) S[r * W + cbase + k + e] = o[e];
        }
    }
}

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
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) cnt += __shfl_xor(cnt, w);
    if (cnt && (threadIdx.x & 63) == 0) atomicAdd(undrained, (unsigned long long)cnt);
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
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) cnt += __shfl_xor(cnt, w);
    if (cnt && (threadIdx.x & 63) == 0) atomicAdd(assigned, (unsigned long long)cnt);
}

}  // namespace

int hand_check(double threshold, double scale)
{
    MH_ARG(threshold >= 1.0 && threshold <= 1.7976931348623157e308, "hand: the threshold must be finite and >= 1");      // (false for NaN)
    MH_ARG(flow_distance_scale_ok(scale), "hand: the scale must be finite and > 0");
    return MHIP_OK;
}

namespace {

// the tile pass and the perimeter jumps of one call: the scratch words and, in `cur`, the node array a final pass reads
struct HandWalk {
    DevBuf S, NA, NB, misc;      // misc: [0], [1] the `open` words of two launches, [2..3] the count of the final pass (64 bits)
    uint4 *cur = nullptr;
    int64_t ntc = 0;
    unsigned long long *count() { return misc.as<unsigned long long>() + 1; }
};

int hand_walk(const uint8_t *d_fd, const double *d_acc, const int32_t *d_lab, int64_t H, int64_t W, double threshold, const char *who, HandWalk &w,
              hipStream_t s)
{
    const int64_t n = H * W;
    if (n >= (int64_t)FD_NONE - 1) {
        set_error("%s: %lld cells exceed the int32 index domain", who, (long long)n);
        return MHIP_ELIMIT;
    }
    const int64_t ntr = cdiv(H, WT), ntc = cdiv(W, WT), ntiles = ntr * ntc, nnodes = ntiles * 256;
    MH_TRY(w.S.alloc(8 * (size_t)n));
    MH_TRY(w.NA.alloc(16 * (size_t)nnodes));
    MH_TRY(w.NB.alloc(16 * (size_t)nnodes));
    MH_TRY(w.misc.alloc(16));
    MH_HIP(hipMemsetAsync(w.misc.p, 0, 16, s));
    hipLaunchKernelGGL(hand_tile_kernel, dim3((unsigned)ntiles), dim3(256), 0, s, d_fd, d_acc, d_lab, threshold, w.S.as<uint2>(), H, W, (int)ntc, w.NA.as<uint4>());
    uint4 *nxt = w.NB.as<uint4>();
    w.cur = w.NA.as<uint4>();
    w.ntc = ntc;
    return fdist_jumps_dev(w.cur, nxt, W, ntc, ntiles, w.misc.as<unsigned int>(), s);
}

// the count of the final pass, once the stream is idle (the scratch and the nodes go back to the pool with `w`)
int hand_count(HandWalk &w, int64_t *count, hipStream_t s)
{
    MH_HIP(hipGetLastError());
    unsigned long long hm[2] = {0, 0};
    MH_HIP(hipMemcpyAsync(hm, w.misc.p, 16, hipMemcpyDeviceToHost, s));
    MH_HIP(stream_sync(s));
    if (count) *count = (int64_t)hm[1];
    return MHIP_OK;
}

}  // namespace

int hand_dev(const uint8_t *d_fd, const double *d_acc, const float *d_elev, const int32_t *d_lab, int64_t H, int64_t W, double threshold, double scale,
             float nodata, float *d_hand, float *d_dist, int64_t *undrained, hipStream_t s)
{
    const int64_t n = H * W;
    HandWalk w;
    MH_TRY(hand_walk(d_fd, d_acc, d_lab, H, W, threshold, "hand", w, s));
    const bool vec = W % 4 == 0 && ((uintptr_t)d_hand | (uintptr_t)d_dist | (uintptr_t)d_elev | (uintptr_t)w.S.p) % 16 == 0;
    const int V = vec ? 4 : 1;
    const dim3 grid((unsigned)cdiv(cdiv(n, V), 256)), block(256);
    if (vec) hipLaunchKernelGGL(hand_final_kernel<4>, grid, block, 0, s, w.S.as<uint2>(), w.cur, d_elev, n, W, (int)w.ntc, scale, nodata, d_hand, d_dist, w.count());
    else hipLaunchKernelGGL(hand_final_kernel<1>, grid, block, 0, s, w.S.as<uint2>(), w.cur, d_elev, n, W, (int)w.ntc, scale, nodata, d_hand, d_dist, w.count());
    return hand_count(w, undrained, s);
}

// The reach catchments: the reaches and the reach of every stream cell by flowpaths_dev, the walk to D(c) by the tile
// pass and the jumps above, one gather.  The drainage cells of the walk and the stream cells of the reaches come from one threshold
// and one label raster, so the two masks agree by construction: a drainage cell that is no stream cell is a labelled one, and holds 0.
int reach_catchments_dev(const uint8_t *d_fd, const double *d_acc, const int32_t *d_lab, int64_t H, int64_t W, double threshold, int32_t *d_catch,
                         mhip_flowpaths *p, int64_t *assigned, hipStream_t s)
{
    const int64_t n = H * W;
    if (n >= (int64_t)FD_NONE - 1) {      // (before any device work: the limit of both engines)
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
    HandWalk w;
    MH_TRY(hand_walk(d_fd, d_acc, d_lab, H, W, threshold, "reach_catchments", w, s));
    const bool vec = W % 4 == 0 && ((uintptr_t)d_catch | (uintptr_t)d_rc.p | (uintptr_t)w.S.p) % 16 == 0;
    const int V = vec ? 4 : 1;
    const dim3 grid((unsigned)std::min<int64_t>(cdiv(cdiv(n, V), 256), CATCH_MAX_BLOCKS)), block(256);
    if (vec) hipLaunchKernelGGL(catch_final_kernel<4>, grid, block, 0, s, w.S.as<uint2>(), w.cur, d_rc.as<int32_t>(), n, W, (int)w.ntc, d_catch, w.count());
    else hipLaunchKernelGGL(catch_final_kernel<1>, grid, block, 0, s, w.S.as<uint2>(), w.cur, d_rc.as<int32_t>(), n, W, (int)w.ntc, d_catch, w.count());
    return hand_count(w, assigned, s);
}

}  // namespace mh
