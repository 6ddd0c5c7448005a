// flowdist.hip -- flow distance to the receiving terminal and the longest flow path per label (gfx950).
//
// No reference counterpart.  A cell is a TERMINAL when it is labelled (label != 0), has no direction (a code > 7) or its downstream
// neighbour lies outside the raster; every other cell steps downstream until it meets one.  no(c) / nd(c): the orthogonal / diagonal
// steps on the way; a cell whose walk never ends (a flow cycle, or a path into one) is UNRESOLVED.
//   raster   float32((float64(no) + float64(nd) * 1.4142135623730951) * scale), -1 where unresolved
//   records  per label l the cell of the largest u = float64(no) + float64(nd) * sqrt2 among the cells whose terminal carries l
//            (l = 0: an unlabelled terminal), the first in raster order among equals; value = u * scale
// The engine is the watersheds' fast path (watershed.hip) with a payload: a tile pass resolves the 64 x 64 tiles in LDS, the tiles'
// perimeter cells -- the only cells a path enters a tile at -- are jumped on their compact array, a final pass takes the last hop.
// The same kernels take flow directions of any origin: a no-direction cell is a terminal, a cycle is what never reaches one.
// This file owns the walk -- the tile pass, the jumps and their setup (FlowWalk, flow_walk_dev: common.hpp); hand.hip runs it with the
// drainage test and ends it in final passes of its own.
#include <algorithm>
#include <cmath>

#include "common.hpp"

namespace mh {
namespace {

constexpr int WT = WS_TILE;
constexpr int FD_HOPS = 5;      // (FD_NONE, FD_DONE, the step pair and the decoding of a scratch word: common.hpp, shared with hand.hip's final passes)

// ---- tile pass ---------------------------------------------------------------------------------------------------------------
// One workgroup per 64 x 64 tile; pull-only pointer doubling on 16-bit tile-local indices as in ws_tile_kernel, and every cell
// carries the pair of its pointer: pair[c] += pair[ptr[c]]; ptr[c] = ptr[ptr[c]].  Unlike the bare pointers the (pointer, pair) of a
// cell must be read as one state, so a round reads, meets at the vote's barrier, then writes.  12 rounds cover 4096 steps: a
// pointer that is not at an end or an exit after them is caught in a cycle of the tile.
// The ends of a walk, in both instantiations (the flow distance runs <false>; hand and the reach catchments run <true>):
//   END    a cell whose mask bit is set -- DRAIN: accum >= thr or, with `lab`, a label != 0; !DRAIN: with `lab`, a label != 0 --
//          and, !DRAIN only, a cell without the bit that steps nowhere (a code > 7, or a step out of the raster)
//   dead   DRAIN only: a cell without the bit that steps nowhere
//   entry  the cell of the neighbouring tile at which a path that leaves this tile continues
// Scratch S, 8 bytes a cell: x = END | FD_DONE (an END of this tile), the entry cell (>= 0), or FD_NONE (the walk reaches a dead
// cell, or still moves after the rounds: a flow cycle); y = the packed pair up to there, 0 with FD_NONE.  The perimeter cells also go
// to their nodes (x, no, nd, 0): the jumps and the decoding know no third kind of end.
// LDS: ptr 8 KB + val 4 KB + pairs 16 KB = 28 KB: five workgroups a CU.
template <bool DRAIN>
__global__ __launch_bounds__(256) void walk_tile_kernel(const uint8_t *__restrict__ fd, const double *__restrict__ acc, const int32_t *__restrict__ lab,
                                                       double thr, uint2 *__restrict__ S, int64_t H, int64_t W, int ntc, uint4 *__restrict__ Nn)
{
    __shared__ uint16_t ptr[WT * WT];
    // V_END, V_DEAD: above; 0..7 the direction in which the path leaves the tile here, V_MOVE a cell that steps on inside the tile.  (A
    // pointer on a cycle whose length divides 2**round points at its own cell: only `val` tells that cell from a fixed point.)
    __shared__ uint8_t val[WT * WT];
    __shared__ uint32_t pr[WT * WT];
    constexpr uint8_t V_END = 8, V_MOVE = 9, V_DEAD = 10;
    const int ti = blockIdx.x / ntc, tj = blockIdx.x - ti * ntc;
    const int64_t r0 = (int64_t)ti * WT, c0 = (int64_t)tj * WT;
    // global I/O: a thread owns 16 consecutive cells of a tile row
    const int lr = threadIdx.x >> 2, lc0 = (threadIdx.x & 3) * 16;
    const int64_t r = r0 + lr, cbase = c0 + lc0;
    const bool vec = (W & 15) == 0 && r < H && cbase + 16 <= W;     // whole, 16-byte aligned group
    uint8_t code[16];
    uint32_t mask = 0;      // my cells whose bit is set
    if (vec) {
        const uint4 cv = *reinterpret_cast<const uint4 *>(fd + r * W + cbase);
        memcpy(code, &cv, 16);
        if constexpr (DRAIN) {
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const double2 av = *reinterpret_cast<const double2 *>(acc + r * W + cbase + 2 * q);
                mask |= (av.x >= thr ? 1u : 0u) << (2 * q) | (av.y >= thr ? 2u : 0u) << (2 * q);
            }
        }
        if (lab) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int4 lv = *reinterpret_cast<const int4 *>(lab + r * W + cbase + 4 * q);
                mask |= (lv.x != 0 ? 1u : 0u) << (4 * q) | (lv.y != 0 ? 2u : 0u) << (4 * q) | (lv.z != 0 ? 4u : 0u) << (4 * q) |
                        (lv.w != 0 ? 8u : 0u) << (4 * q);
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const bool in = r < H && cbase + k < W;
            code[k] = in ? fd[r * W + cbase + k] : (uint8_t)8;
            bool bit = in && lab && lab[r * W + cbase + k] != 0;
            if constexpr (DRAIN) bit = bit || (in && acc[r * W + cbase + k] >= thr);
            if (bit) mask |= 1u << k;
        }
    }
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int li = lr * WT + lc0 + k;
        const bool bit = (mask >> k) & 1u;
        uint16_t p = (uint16_t)li;
        uint8_t v = (bit || !DRAIN) ? V_END : V_DEAD;      // (a cell outside the raster: nothing points at it)
        uint32_t a = 0;
        if (r < H && cbase + k < W && !bit && code[k] <= 7u) {
            const int lr2 = lr + dir_dr((int)code[k]), lc2 = lc0 + k + dir_dc((int)code[k]);
            const int64_t nr = r0 + lr2, nc = c0 + lc2;
            if (nr >= 0 && nr < H && nc >= 0 && nc < W) {      // (else: the step leaves the raster, the cell steps nowhere)
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
    // (every value is computed and then selected, not set in the arms of a branch: fdist_final_kernel's note on the compiler)
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
            const int32_t tgt = vb == V_END ? ((int32_t)(tr * W + tc) | FD_DONE) : leaves ? entry : FD_NONE;
            const uint32_t a = vb == V_END ? pr[li] : leaves ? pr[li] + fd_step(vb) : 0u;
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

// ---- perimeter jumps -------------------------------------------------------------------------------------------------------------
// A node that still points at an entry cell takes over what that entry's node points at, and adds its pair (two uint32: below 2**31
// on any path; on a cycle they wrap, and the result is discarded).  A node and its pair are one state: a launch reads array A and
// writes every node of array B, up to FD_HOPS hops along A's pointers (the span of a node grows sixfold a launch).
__global__ __launch_bounds__(256) void fdist_jump_kernel(const uint4 *__restrict__ A, uint4 *__restrict__ B, int64_t W, int ntc, int64_t nnodes,
                                                        unsigned int *open)
{
    const int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= nnodes || (x & 255) >= 4 * WT - 4) return;
    uint4 n = A[x];
    int32_t t = (int32_t)n.x;
    if (t >= 0 && t != FD_NONE) {
#pragma unroll
        for (int h = 0; h < FD_HOPS; ++h) {
            const int64_t nd = ws_node_of(t, (uint32_t)W, ntc);
            if (nd < 0) {      // (the tile pass names perimeter cells only)
                t = FD_NONE;
                break;
            }
            const uint4 m = A[nd];
            n.y += m.y;
            n.z += m.z;
            t = (int32_t)m.x;
            if (t < 0 || t == FD_NONE) break;
        }
        n.x = (uint32_t)t;
        if (t >= 0 && t != FD_NONE) *open = 1u;
    }
    B[x] = n;
}

// ---- final pass ------------------------------------------------------------------------------------------------------------------
// (fd_resolve: the exact pair and the terminal of a cell from its scratch word and the node of its entry cell -- common.hpp)
// u >= 0: doubles order as their bit patterns; + 1 keeps 0 for "no cell"
__device__ __forceinline__ unsigned long long fd_key(double u) { return (unsigned long long)__double_as_longlong(u) + 1ull; }

// the raster alone: V cells a thread (V = 4: n is a multiple of four, 16-byte stores), 12 bytes a cell
template <int V>
__global__ __launch_bounds__(256) void fdist_final_kernel(const uint2 *__restrict__ S, const uint4 *__restrict__ Nn, int64_t n, int64_t W, int ntc,
                                                         double scale, float *__restrict__ out, unsigned long long *unres)
{
    const int64_t i0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * V;
    unsigned int cnt = 0;
    if (i0 < n) {
        uint2 s[V];
        fd_load<V>(S, i0, s);
        float o[V];
#pragma unroll
        for (int e = 0; e < V; ++e) {
            uint32_t no, nd;
            int32_t T;
            const bool ok = fd_resolve(s[e], Nn, (uint32_t)W, ntc, no, nd, T);
            // (value and count by select, not in the two arms of a branch: the compiler of ROCm 7.2 kept the -1 of the other arm in
            // the register it then used for `nd` -- an unresolved cell behind an entry cell came out as the bits of its diagonal steps)
            const float v = (float)__dmul_rn(fd_u(no, nd), scale);
            o[e] = ok ? v : -1.0f;
            cnt += ok ? 0u : 1u;
        }
        if constexpr (V == 4) *reinterpret_cast<float4 *>(out + i0) = make_float4(o[0], o[1], o[2], o[3]);
        else out[i0] = o[0];
    }
    fd_count_add(cnt, unres);
}

// The raster and the largest key per label of the terminal.  The pair is exact in registers here, so u is compared in float64
// without a float64 raster.  The traversal and the tile table are the ones of label_ops.hip / wetat.hip: TileGeom tiles of 32 x 256,
// a thread owns V consecutive columns of every V-th row and folds the run of cells that share their terminal's label in registers;
// a finished run goes to the tile's LDS table (1024 slots: label, key; a 64-bit LDS maximum), the table leaves as one look at the
// global key and, where it has to rise, one vector atomic per (label, tile); a run that finds no slot goes there itself.
// (Cell by cell on the global keys this pass took 8.9 ms at 16384^2, 8.2 ms folded per wavefront; the raster alone takes 0.6.)
constexpr int FD_SLOTS = 1024;
template <int V>
__global__ __launch_bounds__(256) void fdist_final_rec_kernel(const uint2 *__restrict__ S, const uint4 *__restrict__ Nn, const int32_t *__restrict__ lab,
                                                             TileGeom g, int ntc, double scale, int64_t nlab, float *__restrict__ out,
                                                             unsigned long long *key, unsigned long long *unres, unsigned int *bad)
{
    __shared__ int keys[FD_SLOTS];
    __shared__ unsigned long long tkey[FD_SLOTS];
    constexpr int TPR = 256 / V;      // threads per tile row; V rows per pass of the workgroup
    const int tx = threadIdx.x % TPR, ty = threadIdx.x / TPR;
    unsigned int cnt = 0, any_bad = 0;
    auto raise = [&](int32_t l, unsigned long long k) {
        if (k > __hip_atomic_load(&key[l], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&key[l], k);
    };
    const int64_t ntiles = g.ntr * g.ntc;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        for (int k = threadIdx.x; k < FD_SLOTS; k += 256) {
            keys[k] = -1;
            tkey[k] = 0ull;
        }
        __syncthreads();
        const int64_t tr = tile / g.ntc, tc = tile - tr * g.ntc;
        const int64_t col = tc * 256 + (int64_t)tx * V;
        int32_t cl = -1;      // the label of the run and its largest key
        unsigned long long ck = 0ull;
        auto end_run = [&]() {
            if (cl < 0) return;
            const int h = table_slot<FD_SLOTS>(keys, cl);
            if (h >= 0) atomicMax(&tkey[h], ck);
            else raise(cl, ck);
        };
        for (int r = ty; r < TR; r += V) {
            const int64_t i = (tr * TR + r) * g.W + col;
            if (!(col < g.W && i < g.n)) continue;       // (V = 4: W is a multiple of four, the whole vector is inside)
            uint2 s[V];
            fd_load<V>(S, i, s);
            float o[V];
#pragma unroll
            for (int e = 0; e < V; ++e) {
                uint32_t no, nd;
                int32_t T;
                const bool ok = fd_resolve(s[e], Nn, (uint32_t)g.W, ntc, no, nd, T);
                const double u = fd_u(no, nd);
                const float v = (float)__dmul_rn(u, scale);
                o[e] = ok ? v : -1.0f;      // (by select: see fdist_final_kernel)
                cnt += ok ? 0u : 1u;
                if (ok) {
                    const int32_t l = lab ? lab[T] : 0;
                    if (l < 0 || l > nlab) any_bad = 1;
                    else {
                        const unsigned long long k = fd_key(u);
                        if (l != cl) {
                            end_run();
                            cl = l;
                            ck = k;
                        } else {
                            ck = k > ck ? k : ck;
                        }
                    }
                }
            }
            if constexpr (V == 4) *reinterpret_cast<float4 *>(out + i) = make_float4(o[0], o[1], o[2], o[3]);
            else out[i] = o[0];
        }
        end_run();
        __syncthreads();
        for (int sl = threadIdx.x; sl < FD_SLOTS; sl += 256) {
            const int l = keys[sl];
            if (l >= 0) raise(l, tkey[sl]);
        }
        __syncthreads();
    }
    fd_count_add(cnt, unres);
    if (any_bad) atomicOr(bad, 1u);
}

// among the cells that hold their label's largest key, the first in raster order
template <int V>
__global__ __launch_bounds__(256) void fdist_head_kernel(const uint2 *__restrict__ S, const uint4 *__restrict__ Nn, const int32_t *__restrict__ lab, int64_t n,
                                                        int64_t W, int ntc, int64_t nlab, const unsigned long long *__restrict__ key, uint32_t *head)
{
    const int64_t i0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * V;
    if (i0 >= n) return;
    uint2 s[V];
    fd_load<V>(S, i0, s);
#pragma unroll
    for (int e = 0; e < V; ++e) {
        uint32_t no, nd;
        int32_t T;
        if (!fd_resolve(s[e], Nn, (uint32_t)W, ntc, no, nd, T)) continue;
        const int32_t l = lab ? lab[T] : 0;
        if (l < 0 || l > nlab) continue;
        if (fd_key(fd_u(no, nd)) == key[l]) atomicMin(&head[l], (uint32_t)(i0 + e));
    }
}

__global__ __launch_bounds__(256) void fdist_records_kernel(const unsigned long long *__restrict__ key, const uint32_t *__restrict__ head, int64_t nrec,
                                                           int64_t W, double scale, mhip_index_record *rec)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nrec) return;
    mhip_index_record r;
    const unsigned long long k = key[i];
    if (k == 0) {      // nothing competed: label_max_index's initial record
        r.value = -__builtin_inf();
        r.row = -1;
        r.col = -1;
    } else {
        const int64_t p = (int64_t)head[i];
        r.value = __dmul_rn(__longlong_as_double((long long)(k - 1ull)), scale);
        r.row = p / W;
        r.col = p - r.row * W;
    }
    rec[i] = r;
}

}  // namespace

bool flow_distance_scale_ok(double scale) { return std::isfinite(scale) && scale > 0.0; }

// the perimeter jumps on two node arrays of ntiles * 256 slots (`cur` written by the tile pass, `nxt` scratch); d_open: two zeroable
// words.  Afterwards `cur` is the array the final pass reads.  Synchronises.
static int fdist_jumps_dev(uint4 *&cur, uint4 *&nxt, int64_t W, int64_t ntc, int64_t ntiles, unsigned int *d_open, hipStream_t s)
{
    constexpr int MAX_ROUNDS = 40;      // the watersheds' cap; nodes on a cycle across tiles are still open then
    for (int round = 0; round < MAX_ROUNDS;) {
        const int k = round == 0 ? 2 : 1;
        MH_HIP(hipMemsetAsync(d_open, 0, 8, s));
        for (int j = 0; j < k; ++j) {
            hipLaunchKernelGGL(fdist_jump_kernel, dim3((unsigned)ntiles), dim3(256), 0, s, cur, nxt, W, (int)ntc, ntiles * 256, d_open + j);
            std::swap(cur, nxt);
        }
        unsigned int h[2] = {0, 0};
        MH_HIP(hipMemcpyAsync(h, d_open, 8, hipMemcpyDeviceToHost, s));
        MH_HIP(stream_sync(s));
        round += k;
        if (!h[k - 1]) break;
    }
    return MHIP_OK;
}

bool flow_walk_fits(int64_t n) { return n < (int64_t)FD_NONE - 1; }

int flow_walk_dev(const uint8_t *d_fd, const double *d_acc, const int32_t *d_lab, int64_t H, int64_t W, double threshold, const char *who, FlowWalk &w,
                  hipStream_t s)
{
    const int64_t n = H * W;
    if (!flow_walk_fits(n)) {
        set_error("%s: %lld cells exceed the int32 index domain", who, (long long)n);
        return MHIP_ELIMIT;
    }
    const int64_t ntr = cdiv(H, WT), ntc = cdiv(W, WT), ntiles = ntr * ntc, nnodes = ntiles * 256;
    MH_TRY(w.S.alloc(8 * (size_t)n));
    MH_TRY(w.NA.alloc(16 * (size_t)nnodes));
    MH_TRY(w.NB.alloc(16 * (size_t)nnodes));
    MH_TRY(w.misc.alloc(sizeof(FlowWalk::Misc)));
    MH_HIP(hipMemsetAsync(w.misc.p, 0, sizeof(FlowWalk::Misc), s));
    hipLaunchKernelGGL(d_acc ? walk_tile_kernel<true> : walk_tile_kernel<false>, dim3((unsigned)ntiles), dim3(256), 0, s, d_fd, d_acc, d_lab, threshold,
                       w.S.as<uint2>(), H, W, (int)ntc, w.NA.as<uint4>());
    uint4 *nxt = w.NB.as<uint4>();
    w.cur = w.NA.as<uint4>();
    w.ntc = ntc;
    return fdist_jumps_dev(w.cur, nxt, W, ntc, ntiles, w.misc.as<FlowWalk::Misc>()->open, s);
}

int flow_walk_count(FlowWalk &w, int64_t *count, bool *bad, hipStream_t s)
{
    MH_HIP(hipGetLastError());
    FlowWalk::Misc h = {};
    MH_HIP(hipMemcpyAsync(&h, w.misc.p, sizeof(h), hipMemcpyDeviceToHost, s));
    MH_HIP(stream_sync(s));
    if (count) *count = (int64_t)h.count;
    if (bad) *bad = h.bad != 0;
    return MHIP_OK;
}

int flow_distance_dev(const uint8_t *d_fd, const int32_t *d_lab, int64_t H, int64_t W, double scale, int64_t nlab, float *d_out, mhip_index_record *d_rec,
                      int64_t *unresolved, hipStream_t s)
{
    const int64_t n = H * W;
    FlowWalk w;
    MH_TRY(flow_walk_dev(d_fd, nullptr, d_lab, H, W, 0.0, "flow_distance", w, s));
    const uint2 *S = w.S.as<uint2>();
    const int ntc = (int)w.ntc;
    const bool vec = W % 4 == 0 && ((uintptr_t)d_out | (uintptr_t)w.S.p) % 16 == 0;
    const dim3 grid((unsigned)cdiv(cdiv(n, vec ? 4 : 1), 256)), block(256);
    DevBuf key, head;
    if (d_rec) {
        MH_TRY(key.alloc(8 * (size_t)(nlab + 1)));
        MH_TRY(head.alloc(4 * (size_t)(nlab + 1)));
        MH_HIP(hipMemsetAsync(key.p, 0, 8 * (size_t)(nlab + 1), s));
        MH_HIP(hipMemsetAsync(head.p, 0xff, 4 * (size_t)(nlab + 1), s));
        unsigned long long *d_key = key.as<unsigned long long>();
        const TileGeom g = tile_geom(n, W);
        hipLaunchKernelGGL(pick_v(vec, fdist_final_rec_kernel<4>, fdist_final_rec_kernel<1>), dim3(tile_grid(g)), block, 0, s, S, w.cur, d_lab, g, ntc, scale,
                           nlab, d_out, d_key, w.count(), w.bad());
        hipLaunchKernelGGL(pick_v(vec, fdist_head_kernel<4>, fdist_head_kernel<1>), grid, block, 0, s, S, w.cur, d_lab, n, W, ntc, nlab, d_key, head.as<uint32_t>());
        hipLaunchKernelGGL(fdist_records_kernel, dim3((unsigned)cdiv(nlab + 1, 256)), dim3(256), 0, s, d_key, head.as<uint32_t>(), nlab + 1, W, scale, d_rec);
    } else {
        hipLaunchKernelGGL(pick_v(vec, fdist_final_kernel<4>, fdist_final_kernel<1>), grid, block, 0, s, S, w.cur, n, W, ntc, scale, d_out, w.count());
    }
    bool bad = false;
    int64_t u = 0;
    MH_TRY(flow_walk_count(w, &u, &bad, s));      // (synchronises: the scratch, the nodes and the keys go back to the pool)
    if (bad) {
        set_error("flow_distance: label outside [0, nlabels]");
        return MHIP_EINVAL;
    }
    if (unresolved) *unresolved = u;
    return MHIP_OK;
}

}  // namespace mh
