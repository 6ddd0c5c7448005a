// traveltime.hip -- travel time along the flow paths: a step cost per cell, and that cost summed down the D8 forest (gfx950).
//
// No reference counterpart; the definition is tests/_traveltime.py.
//   step cost  uint32 ticks of the step that leaves a cell, v = k * sqrt(s) (NRCS TR-55): a stencil pass, float64, every operation
//              one IEEE rounding (tt_cost_kernel)
//   walk       ticks(c) = the sum of `cost` over the cells of the path from c up to, not including, its terminal T(c) -- the
//              terminals and the unresolved cells are flowdist.hip's in its !DRAIN form -- exact in 64 bits
//     raster   float32(float64(ticks) * tick), -1 where unresolved
//     records  per label l of the terminal the cell of the largest ticks, compared as integers, the first in raster order among equals
//     table    per label l of the terminal the cells per bin min(ticks / bin_ticks, nbins - 1)
// The engine has flowdist.hip's shape with kernels of its own: a cost is capped at 2**20 - 1, so the sum of a tile-local path --
// 4095 steps and the step out of the tile -- stays in one uint32 and the tile pass keeps that file's LDS plan; the nodes and
// everything behind the tile pass carry 64 bits, (next, lo, hi, 0) in the 16-byte node.
#include <algorithm>
#include <cmath>

#include "common.hpp"

namespace mh {
namespace {

constexpr int WT = WS_TILE;
constexpr int TT_HOPS = 5;
constexpr uint32_t TT_COST_MAX = MHIP_TRAVELTIME_COST_MAX;
constexpr unsigned int TT_BAD_LABEL = 1u, TT_BAD_COST = 2u;

// the words of one call on the device
struct TtMisc {
    unsigned int open[2];         // the jumps' `open` words of two launches
    unsigned int bad, pad;        // TT_BAD_LABEL | TT_BAD_COST
    unsigned long long count;     // the count of the final pass / of the cost pass
};

// ---- step cost -------------------------------------------------------------------------------------------------------------------
// One cell a thread: 1 B code + 4 B z + (a neighbour's z: the same sectors, a row apart) + 8 B acc read, 4 B cost written.  The
// operations and their order are the model's; -ffp-contract=off, and the intrinsics say the rounding.  (All values are computed
// and then selected: a cell that steps nowhere reads its own z as the neighbour's.)
__global__ __launch_bounds__(256) void tt_cost_kernel(const uint8_t *__restrict__ fd, const float *__restrict__ z, const double *__restrict__ acc, int64_t H,
                                                      int64_t W, double cellsize, mhip_traveltime_params p, uint32_t *__restrict__ cost,
                                                      unsigned long long *sat)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned int clipped = 0;
    if (i < H * W) {
        const unsigned code = fd[i];
        const int64_t d = downstream(fd, i, H, W);
        const bool moves = d >= 0;
        const double len = (code & 1u) ? __dmul_rn(cellsize, 1.4142135623730951) : cellsize;
        const double drop = __dsub_rn((double)z[i], (double)z[moves ? d : i]);
        double s = __ddiv_rn(drop, len);
        s = s >= p.smin ? s : p.smin;      // (false for a NaN)
        const bool channel = acc ? acc[i] >= p.channel_threshold : false;
        const double k = channel ? p.k_channel : p.k_overland;
        double v = __dmul_rn(k, __dsqrt_rn(s));
        v = v > p.vmax ? p.vmax : v;
        const double q = rint(__ddiv_rn(__ddiv_rn(len, v), p.tick));
        const bool clip = q > (double)TT_COST_MAX;
        const uint32_t c = clip ? TT_COST_MAX : (uint32_t)q;
        cost[i] = moves ? c : 0u;
        clipped = (moves && clip) ? 1u : 0u;
    }
    fd_count_add(clipped, sat);
}

// ---- tile pass -------------------------------------------------------------------------------------------------------------------
// walk_tile_kernel<false>'s pass (flowdist.hip) with the cell's cost in the place of its step pair: sum[c] += sum[ptr[c]];
// ptr[c] = ptr[ptr[c]], a round reading every (pointer, sum), meeting at the vote's barrier, then writing.  The doubling needs the
// sum of a fixed point to read 0, so the cost of the step that LEAVES the tile cannot stand in `sum` of its exit cell while the
// rounds run.  It is read from global memory again behind them: the owner of an exit cell -- a perimeter cell, at most 252 of a
// tile's 4096, and a line this workgroup has just read -- puts it into the cell's `sum`, which is final by then, and the epilogue adds
// sum[exit cell] to every path that leaves there.  (A side array of the 256 perimeter slots in LDS, read through ws_perim_slot of the
// exit cell, cost the epilogue 24 VGPRs -- 98 in all, four workgroups a CU; held in registers over the rounds the costs are 16 more.)
// LDS: ptr 8 KB + val 4 KB + sums 16 KB = 28 KB, flowdist.hip's plan: five workgroups a CU.
// Scratch S, 8 bytes a cell: x as in flowdist.hip (END | FD_DONE, the entry cell, or FD_NONE); y = the ticks up to there (below
// 2**32: 4096 costs of at most 2**20 - 1), 0 with FD_NONE.  The perimeter cells also go to their nodes (x, y, 0, 0).
// A cost above the cap sets TT_BAD_COST in *flag: the host refuses the call and nothing that was summed is used.
__global__ __launch_bounds__(256) void tt_tile_kernel(const uint8_t *__restrict__ fd, const int32_t *__restrict__ lab, const uint32_t *__restrict__ cost,
                                                      uint2 *__restrict__ S, int64_t H, int64_t W, int ntc, uint4 *__restrict__ Nn, unsigned int *flag)
{
    __shared__ uint16_t ptr[WT * WT];
    __shared__ uint8_t val[WT * WT];      // V_END; 0..7 the direction in which the path leaves the tile here; V_MOVE a cell that steps on inside the tile
    __shared__ uint32_t sum[WT * WT];
    constexpr uint8_t V_END = 8, V_MOVE = 9;
    const int ti = blockIdx.x / ntc, tj = blockIdx.x - ti * ntc;
    const int64_t r0 = (int64_t)ti * WT, c0 = (int64_t)tj * WT;
    // global I/O: a thread owns 16 consecutive cells of a tile row
    const int lr = threadIdx.x >> 2, lc0 = (threadIdx.x & 3) * 16;
    const int64_t r = r0 + lr, cbase = c0 + lc0;
    const bool vec = (W & 15) == 0 && r < H && cbase + 16 <= W;     // whole, 16-byte aligned group
    uint8_t code[16];
    uint32_t mask = 0;      // my labelled cells
    if (vec) {
        const uint4 cv = *reinterpret_cast<const uint4 *>(fd + r * W + cbase);
        memcpy(code, &cv, 16);
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
            if (in && lab && lab[r * W + cbase + k] != 0) mask |= 1u << k;
        }
    }
    uint32_t over = 0, cq[4] = {0u, 0u, 0u, 0u};
    // (the costs come in four at a time, next to their use: sixteen of them held over the loop cost the fifth workgroup its registers)
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int li = lr * WT + lc0 + k;
        const bool bit = (mask >> k) & 1u;
        if ((k & 3) == 0) {
            if (vec) {
                const uint4 kv = *reinterpret_cast<const uint4 *>(cost + r * W + cbase + k);
                cq[0] = kv.x; cq[1] = kv.y; cq[2] = kv.z; cq[3] = kv.w;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) cq[e] = (r < H && cbase + k + e < W) ? cost[r * W + cbase + k + e] : 0u;
            }
        }
        const uint32_t ck = cq[k & 3];
        over |= ck > TT_COST_MAX ? 1u : 0u;
        uint16_t p = (uint16_t)li;
        uint8_t v = V_END;      // (a cell outside the raster: nothing points at it)
        uint32_t a = 0;
        if (r < H && cbase + k < W && !bit && code[k] <= 7u) {
            const int lr2 = lr + dir_dr((int)code[k]), lc2 = lc0 + k + dir_dc((int)code[k]);
            const int64_t nr = r0 + lr2, nc = c0 + lc2;
            if (nr >= 0 && nr < H && nc >= 0 && nc < W) {      // (else: the step leaves the raster, the cell is a terminal)
                if (lr2 >= 0 && lr2 < WT && lc2 >= 0 && lc2 < WT) {
                    p = (uint16_t)(lr2 * WT + lc2);
                    v = V_MOVE;
                    a = ck;
                } else {
                    v = code[k];      // leaves the tile: the path continues at that entry cell
                }
            }
        }
        ptr[li] = p;
        val[li] = v;
        sum[li] = a;
    }
    if (over) atomicOr(flag, TT_BAD_COST);
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
            na[k] = sum[p];      // (0 at a fixed point)
            ch |= q != p;
        }
        if (!__syncthreads_or(ch)) break;      // (every read of the round is behind this barrier)
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int li = k * 256 + (int)threadIdx.x;
            ptr[li] = np[k];
            sum[li] += na[k];
        }
        __syncthreads();
    }
    // the exit cells take the cost of their step out of the tile (their sums are 0: fixed points; every sum is final)
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int li = lr * WT + lc0 + k;
        if (val[li] <= 7u) sum[li] = cost[r * W + cbase + k];      // (an exit cell lies inside the raster)
    }
    __syncthreads();
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
            const bool leaves = vb <= 7u;      // (V_MOVE: a flow cycle inside the tile)
            const uint32_t out_cost = t == li ? 0u : sum[t];      // (the exit cell's own sum is that cost already)
            const int32_t entry = (int32_t)((tr + dir_dr((int)(vb & 7u))) * W + tc + dir_dc((int)(vb & 7u)));
            const int32_t tgt = vb == V_END ? ((int32_t)(tr * W + tc) | FD_DONE) : leaves ? entry : FD_NONE;
            const uint32_t a = vb == V_END ? sum[li] : leaves ? sum[li] + out_cost : 0u;
            o[e] = make_uint2((uint32_t)tgt, a);
            const int slot = ws_perim_slot(lr, lc0 + k + e);
            if (slot >= 0) {
                const bool in = r < H && cbase + k + e < W;
                Nn[(int64_t)blockIdx.x * 256 + slot] = in ? make_uint4((uint32_t)tgt, a, 0u, 0u) : make_uint4((uint32_t)FD_NONE, 0u, 0u, 0u);
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
// fdist_jump_kernel's launch with one 64-bit sum (y: low, z: high word) in the place of the two counts.  A sum stays below 2**51 on
// any path; on a cycle it wraps, and the result is discarded.
__device__ __forceinline__ unsigned long long tt_sum(uint4 n) { return (unsigned long long)n.y | (unsigned long long)n.z << 32; }

__global__ __launch_bounds__(256) void tt_jump_kernel(const uint4 *__restrict__ A, uint4 *__restrict__ B, int64_t W, int ntc, int64_t nnodes,
                                                      unsigned int *open)
{
    const int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= nnodes || (x & 255) >= 4 * WT - 4) return;
    uint4 n = A[x];
    int32_t t = (int32_t)n.x;
    if (t >= 0 && t != FD_NONE) {
        unsigned long long a = tt_sum(n);
#pragma unroll
        for (int h = 0; h < TT_HOPS; ++h) {
            const int64_t nd = ws_node_of(t, (uint32_t)W, ntc);
            if (nd < 0) {      // (the tile pass names perimeter cells only)
                t = FD_NONE;
                break;
            }
            const uint4 m = A[nd];
            a += tt_sum(m);
            t = (int32_t)m.x;
            if (t < 0 || t == FD_NONE) break;
        }
        n.x = (uint32_t)t;
        n.y = (uint32_t)a;
        n.z = (uint32_t)(a >> 32);
        if (t >= 0 && t != FD_NONE) *open = 1u;
    }
    B[x] = n;
}

// ---- final passes ----------------------------------------------------------------------------------------------------------------
// the exact ticks and the terminal of a cell from its scratch word and, for a path that leaves its tile, the node of its entry cell;
// false: unresolved (fd_resolve with one 64-bit sum)
__device__ __forceinline__ bool tt_resolve(uint2 s, const uint4 *__restrict__ Nn, uint32_t W, int ntc, unsigned long long &ticks, int32_t &T)
{
    int32_t t = (int32_t)s.x;
    ticks = s.y;
    if (t >= 0 && t != FD_NONE) {
        const int64_t node = ws_node_of(t, W, ntc);
        uint4 m = make_uint4((uint32_t)FD_NONE, 0u, 0u, 0u);
        if (node >= 0) m = Nn[node];
        t = (int32_t)m.x;
        ticks += tt_sum(m);
    }
    T = t & ~FD_DONE;
    return t < 0;
}
// (ticks < 2**51: the conversion is exact, the product one rounding, the narrowing another)
__device__ __forceinline__ float tt_seconds(unsigned long long ticks, double tick) { return (float)__dmul_rn((double)ticks, tick); }

// the raster alone: V cells a thread
template <int V>
__global__ __launch_bounds__(256) void tt_final_kernel(const uint2 *__restrict__ S, const uint4 *__restrict__ Nn, int64_t n, int64_t W, int ntc,
                                                       double tick, float *__restrict__ out, unsigned long long *unres)
{
    const int64_t i0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * V;
    unsigned int cnt = 0;
    if (i0 < n) {
        uint2 s[V];
        fd_load<V>(S, i0, s);
        float o[V];
#pragma unroll
        for (int e = 0; e < V; ++e) {
            unsigned long long ticks;
            int32_t T;
            const bool ok = tt_resolve(s[e], Nn, (uint32_t)W, ntc, ticks, T);
            const float v = tt_seconds(ticks, tick);
            o[e] = ok ? v : -1.0f;      // (by select: fdist_final_kernel's note)
            cnt += ok ? 0u : 1u;
        }
        if constexpr (V == 4) *reinterpret_cast<float4 *>(out + i0) = make_float4(o[0], o[1], o[2], o[3]);
        else out[i0] = o[0];
    }
    fd_count_add(cnt, unres);
}

// The raster, the largest key (ticks + 1; 0: no cell) per label of the terminal and, with `hist`, the time-area table.  The
// traversal and the tile's key table are fdist_final_rec_kernel's: a thread owns V consecutive columns of every V-th row of a
// 32 x 256 tile and folds the run of cells that share their terminal's label in registers; a finished run goes to the tile's LDS
// table, the table leaves as one look at the global key and, where it has to rise, one atomic per (label, tile).  The table's counts
// fold the run of equal (label, bin) in registers as well and go to the global table with one atomicAdd a run.
constexpr int TT_SLOTS = 1024;
template <int V>
__global__ __launch_bounds__(256) void tt_final_rec_kernel(const uint2 *__restrict__ S, const uint4 *__restrict__ Nn, const int32_t *__restrict__ lab,
                                                           TileGeom g, int ntc, double tick, int64_t nlab, int nbins, unsigned long long bin_ticks,
                                                           float *__restrict__ out, unsigned long long *key, uint32_t *hist,
                                                           unsigned long long *unres, unsigned int *bad)
{
    __shared__ int keys[TT_SLOTS];
    __shared__ unsigned long long tkey[TT_SLOTS];
    constexpr int TPR = 256 / V;      // threads per tile row; V rows per pass of the workgroup
    const int tx = threadIdx.x % TPR, ty = threadIdx.x / TPR;
    unsigned int cnt = 0, any_bad = 0;
    auto raise = [&](int32_t l, unsigned long long k) {
        if (k > __hip_atomic_load(&key[l], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&key[l], k);
    };
    const int64_t ntiles = g.ntr * g.ntc;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        for (int k = threadIdx.x; k < TT_SLOTS; k += 256) {
            keys[k] = -1;
            tkey[k] = 0ull;
        }
        __syncthreads();
        const int64_t tr = tile / g.ntc, tc = tile - tr * g.ntc;
        const int64_t col = tc * 256 + (int64_t)tx * V;
        int32_t cl = -1;      // the label of the run and its largest key
        unsigned long long ck = 0ull;
        int64_t hb = -1;      // the table word of the run of equal (label, bin) and its cells
        uint32_t hn = 0;
        auto end_run = [&]() {
            if (cl < 0) return;
            const int h = table_slot<TT_SLOTS>(keys, cl);
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
                unsigned long long ticks;
                int32_t T;
                const bool ok = tt_resolve(s[e], Nn, (uint32_t)g.W, ntc, ticks, T);
                const float v = tt_seconds(ticks, tick);
                o[e] = ok ? v : -1.0f;      // (by select: fdist_final_kernel's note)
                cnt += ok ? 0u : 1u;
                if (ok) {
                    const int32_t l = lab ? lab[T] : 0;
                    if (l < 0 || l > nlab) any_bad = 1;
                    else {
                        const unsigned long long k = ticks + 1ull;
                        if (l != cl) {
                            end_run();
                            cl = l;
                            ck = k;
                        } else {
                            ck = k > ck ? k : ck;
                        }
                        if (hist) {
                            const unsigned long long b = ticks / bin_ticks;
                            const int64_t w = (int64_t)l * nbins + (int64_t)(b < (unsigned long long)(nbins - 1) ? b : (unsigned long long)(nbins - 1));
                            if (w != hb) {
                                if (hn) atomicAdd(&hist[hb], hn);
                                hb = w;
                                hn = 1;
                            } else {
                                ++hn;
                            }
                        }
                    }
                }
            }
            if constexpr (V == 4) *reinterpret_cast<float4 *>(out + i) = make_float4(o[0], o[1], o[2], o[3]);
            else out[i] = o[0];
        }
        end_run();
        if (hn) atomicAdd(&hist[hb], hn);
        __syncthreads();
        for (int sl = threadIdx.x; sl < TT_SLOTS; sl += 256) {
            const int l = keys[sl];
            if (l >= 0) raise(l, tkey[sl]);
        }
        __syncthreads();
    }
    fd_count_add(cnt, unres);
    if (any_bad) atomicOr(bad, TT_BAD_LABEL);
}

// among the cells that hold their label's largest key, the first in raster order
template <int V>
__global__ __launch_bounds__(256) void tt_head_kernel(const uint2 *__restrict__ S, const uint4 *__restrict__ Nn, const int32_t *__restrict__ lab, int64_t n,
                                                      int64_t W, int ntc, int64_t nlab, const unsigned long long *__restrict__ key, uint32_t *head)
{
    const int64_t i0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * V;
    if (i0 >= n) return;
    uint2 s[V];
    fd_load<V>(S, i0, s);
#pragma unroll
    for (int e = 0; e < V; ++e) {
        unsigned long long ticks;
        int32_t T;
        if (!tt_resolve(s[e], Nn, (uint32_t)W, ntc, ticks, T)) continue;
        const int32_t l = lab ? lab[T] : 0;
        if (l < 0 || l > nlab) continue;
        if (ticks + 1ull == key[l]) atomicMin(&head[l], (uint32_t)(i0 + e));
    }
}

__global__ __launch_bounds__(256) void tt_records_kernel(const unsigned long long *__restrict__ key, const uint32_t *__restrict__ head, int64_t nrec,
                                                         int64_t W, double tick, mhip_index_record *rec)
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
        r.value = __dmul_rn((double)(k - 1ull), tick);
        r.row = p / W;
        r.col = p - r.row * W;
    }
    rec[i] = r;
}

bool positive_finite(double v) { return std::isfinite(v) && v > 0.0; }

}  // namespace

int travel_time_check(double cellsize, const mhip_traveltime_params *p)
{
    MH_ARG(p, "travel time: the parameters are missing");
    MH_ARG(positive_finite(cellsize), "travel time: cellsize must be finite and > 0");
    MH_ARG(positive_finite(p->k_overland), "travel time: k_overland must be finite and > 0");
    MH_ARG(positive_finite(p->k_channel), "travel time: k_channel must be finite and > 0");
    MH_ARG(p->channel_threshold > 0.0, "travel time: channel_threshold must be > 0 (+inf: one class)");      // (false for a NaN)
    MH_ARG(positive_finite(p->smin), "travel time: smin must be finite and > 0");
    MH_ARG(positive_finite(p->vmax), "travel time: vmax must be finite and > 0");
    MH_ARG(positive_finite(p->tick), "travel time: tick must be finite and > 0");
    return MHIP_OK;
}

int travel_time_walk_check(double tick, int64_t nbins, uint64_t bin_ticks, bool table)
{
    MH_ARG(positive_finite(tick), "travel time: tick must be finite and > 0");
    if (table) {
        MH_ARG(nbins >= 1 && nbins <= MHIP_TRAVELTIME_MAX_BINS, "travel time: nbins must lie in [1, 256]");
        MH_ARG(bin_ticks >= 1, "travel time: bin_ticks must be >= 1");
    } else {
        MH_ARG(nbins == 0, "travel time: nbins without a table must be 0");
    }
    return MHIP_OK;
}

int step_cost_dev(const uint8_t *d_fd, const float *d_z, const double *d_acc, int64_t H, int64_t W, double cellsize, const mhip_traveltime_params &p,
                  uint32_t *d_cost, int64_t *saturated, hipStream_t s)
{
    const int64_t n = H * W;
    DevBuf misc;
    MH_TRY(misc.alloc(sizeof(TtMisc)));
    MH_HIP(hipMemsetAsync(misc.p, 0, sizeof(TtMisc), s));
    hipLaunchKernelGGL(tt_cost_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, s, d_fd, d_z, d_acc, H, W, cellsize, p, d_cost,
                       &misc.as<TtMisc>()->count);
    MH_HIP(hipGetLastError());
    TtMisc h = {};
    MH_HIP(hipMemcpyAsync(&h, misc.p, sizeof(h), hipMemcpyDeviceToHost, s));
    MH_HIP(stream_sync(s));
    if (saturated) *saturated = (int64_t)h.count;
    return MHIP_OK;
}

int flow_cost_distance_dev(const uint8_t *d_fd, const int32_t *d_lab, const uint32_t *d_cost, int64_t H, int64_t W, double tick, int64_t nlab, float *d_out,
                           mhip_index_record *d_rec, int64_t nbins, uint64_t bin_ticks, uint32_t *d_hist, int64_t *unresolved, hipStream_t s)
{
    const int64_t n = H * W;
    if (!flow_walk_fits(n)) {
        set_error("flow_cost_distance: %lld cells exceed the int32 index domain", (long long)n);
        return MHIP_ELIMIT;
    }
    const int64_t ntr = cdiv(H, WT), ntc = cdiv(W, WT), ntiles = ntr * ntc, nnodes = ntiles * 256;
    DevBuf S, NA, NB, misc, key, head;
    MH_TRY(S.alloc(8 * (size_t)n));
    MH_TRY(NA.alloc(16 * (size_t)nnodes));
    MH_TRY(NB.alloc(16 * (size_t)nnodes));
    MH_TRY(misc.alloc(sizeof(TtMisc)));
    TtMisc *d_misc = misc.as<TtMisc>();
    MH_HIP(hipMemsetAsync(misc.p, 0, sizeof(TtMisc), s));
    hipLaunchKernelGGL(tt_tile_kernel, dim3((unsigned)ntiles), dim3(256), 0, s, d_fd, d_lab, d_cost, S.as<uint2>(), H, W, (int)ntc, NA.as<uint4>(),
                       &d_misc->bad);
    // the jumps (fdist_jumps_dev's schedule); the first read-back also brings the tile pass's verdict on the costs
    uint4 *cur = NA.as<uint4>(), *nxt = NB.as<uint4>();
    constexpr int MAX_ROUNDS = 40;      // the watersheds' cap; nodes on a cycle across tiles are still open then
    for (int round = 0; round < MAX_ROUNDS;) {
        const int k = round == 0 ? 2 : 1;
        MH_HIP(hipMemsetAsync(d_misc->open, 0, 8, s));
        for (int j = 0; j < k; ++j) {
            hipLaunchKernelGGL(tt_jump_kernel, dim3((unsigned)ntiles), dim3(256), 0, s, cur, nxt, W, (int)ntc, nnodes, d_misc->open + j);
            std::swap(cur, nxt);
        }
        TtMisc h = {};
        MH_HIP(hipMemcpyAsync(&h, misc.p, 16, hipMemcpyDeviceToHost, s));
        MH_HIP(stream_sync(s));
        if (h.bad & TT_BAD_COST) {
            set_error("flow_cost_distance: a cost above %u", TT_COST_MAX);
            return MHIP_EINVAL;
        }
        round += k;
        if (!h.open[k - 1]) break;
    }
    const bool vec = W % 4 == 0 && ((uintptr_t)d_out | (uintptr_t)S.p) % 16 == 0;
    const dim3 grid((unsigned)cdiv(cdiv(n, vec ? 4 : 1), 256)), block(256);
    if (d_rec || d_hist) {
        MH_TRY(key.alloc(8 * (size_t)(nlab + 1)));
        MH_HIP(hipMemsetAsync(key.p, 0, 8 * (size_t)(nlab + 1), s));
        if (d_hist) MH_HIP(hipMemsetAsync(d_hist, 0, 4 * (size_t)(nlab + 1) * (size_t)nbins, s));
        unsigned long long *d_key = key.as<unsigned long long>();
        const TileGeom g = tile_geom(n, W);
        hipLaunchKernelGGL(pick_v(vec, tt_final_rec_kernel<4>, tt_final_rec_kernel<1>), dim3(tile_grid(g)), block, 0, s, S.as<uint2>(), cur, d_lab, g, (int)ntc,
                           tick, nlab, (int)nbins, (unsigned long long)(d_hist ? bin_ticks : 1), d_out, d_key, d_hist, &d_misc->count, &d_misc->bad);
        if (d_rec) {
            MH_TRY(head.alloc(4 * (size_t)(nlab + 1)));
            MH_HIP(hipMemsetAsync(head.p, 0xff, 4 * (size_t)(nlab + 1), s));
            hipLaunchKernelGGL(pick_v(vec, tt_head_kernel<4>, tt_head_kernel<1>), grid, block, 0, s, S.as<uint2>(), cur, d_lab, n, W, (int)ntc, nlab, d_key,
                               head.as<uint32_t>());
            hipLaunchKernelGGL(tt_records_kernel, dim3((unsigned)cdiv(nlab + 1, 256)), dim3(256), 0, s, d_key, head.as<uint32_t>(), nlab + 1, W, tick, d_rec);
        }
    } else {
        hipLaunchKernelGGL(pick_v(vec, tt_final_kernel<4>, tt_final_kernel<1>), grid, block, 0, s, S.as<uint2>(), cur, n, W, (int)ntc, tick, d_out,
                           &d_misc->count);
    }
    MH_HIP(hipGetLastError());
    TtMisc h = {};
    MH_HIP(hipMemcpyAsync(&h, misc.p, sizeof(h), hipMemcpyDeviceToHost, s));
    MH_HIP(stream_sync(s));      // (the scratch, the nodes and the keys go back to the pool)
    if (h.bad & TT_BAD_LABEL) {
        set_error("flow_cost_distance: label outside [0, nlabels]");
        return MHIP_EINVAL;
    }
    if (unresolved) *unresolved = (int64_t)h.count;
    return MHIP_OK;
}

}  // namespace mh
