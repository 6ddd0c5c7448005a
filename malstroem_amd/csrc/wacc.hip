// wacc.hip -- runoff-weighted D8 flow accumulation: uint32 weights, exact uint64 sums (gfx950).
//
// No reference counterpart; tests/_wacc.py is the definition.  wacc[c] = weight[c] + sum(wacc[n]) over the in-raster neighbours n whose
// flow direction points at c, in uint64.  A cell without a direction (a code > 7) receives and does not forward, a cell whose step
// leaves the raster keeps its sum: the rules of accum.hip.  A cell on a flow cycle is UNRESOLVED and holds MHIP_WACC_UNRESOLVED
// (every cell has one downstream cell, so nothing but the cycle itself lies downstream of a cycle); the call counts these cells.
// They are the cells accum.hip leaves 0; a weight of 0 is legal here, so 0 cannot be the sentinel.  With a label raster the call
// also sums the weights per label.  The arithmetic is integer: every summation order gives the same bits.
//
// The engine is the one of accum.hip's header comment with 64-bit sums (its packed 38- and 44-bit fields hold cell counts only):
//   phase 1  wacc_tile_kernel<false>, a workgroup per 64 x 64 tile, in LDS: pointer doubling on the in-tile forest.  With A_k[w] the
//            2**k-th downstream cell of w (SENT once the path has left the tile or ended) and S_k[v] the sum over the cells at most
//            2**k - 1 steps upstream of v:   S_{k+1}[A_k[w]] += S_k[w],  A_{k+1}[w] = A_k[A_k[w]].  A round reads S[w], A[w] and
//            A[A[w]] into registers, meets at a barrier, then pushes with non-returning 64-bit LDS adds and writes the new pointer;
//            the vote that ends the loop is the second barrier (common.hpp: WgVote).  At most 12 rounds (2**12 = the cells of a tile).
//            A pointer still moving then lies on a cycle inside the tile: the cell it points at is tainted (bit 63 of its sum; a
//            context holds fewer than 2**31 cells, so a resolved sum stays below 2**63).  The pointer word also carries R, the last
//            in-tile cell reached so far: for a perimeter cell, the cell through which its tile-local path leaves the tile.
//            Published per perimeter cell (the NODES, 256 slots per tile): its local sum, whether it is an EXIT (flows into a raster
//            cell of another tile) and into which node, and the exit of its own tile-local path.  An exit adds one to the external
//            in-degree of the node it flows into; a node with an external in-degree is an ENTRY.
//   phase 2  the perimeter graph, ~4 % of the cells: exit x forwards F(x) = local(x) + the flux routed through x to its entry cell e
//            and on to the exit of e's path.  A node holds its sum in a 64-bit word and its pending count in a word of its own: add
//            to the target, fence, decrement `pend` with a returning atomic; the last arriver reads the sum and continues.  A path
//            may leave a tile and enter it again any number of times, and an entry may be its own exit: both are just nodes.  Nodes
//            whose count never reaches 0 lie on a cycle across tiles; their entries never see all of their deliveries.
//   phase 3  wacc_tile_kernel<true>: the doubling again with every entry pre-loaded with its inflow -- or tainted when a delivery is
//            missing; the taint travels downstream with the sums, never upstream --, each cell written once as uint64.
// LDS of a tile pass: 32 KB of sums + 16 KB of pointer words (A | R << 13) + 4 KB of direction codes (phase 1) or 3 KB of node
// words (phase 3) = 52 / 51 KB: three workgroups per CU of 160 KB.  (16-bit pointers in phase 3 would make it 43 KB: still three.)
// Traffic per cell and tile pass: 1 B of directions + 4 B of weights read; phase 3 writes 8 B.
#include "common.hpp"

namespace mh {
namespace {

constexpr int WT = 64;                    // tile edge
constexpr int W_PERIM = 4 * WT - 4;       // perimeter cells of a tile
constexpr int W_STRIDE = 256;             // node slots per tile
constexpr int WTN = 256;                  // threads per tile
constexpr int W_CPT = WT * WT / WTN;      // cells per thread
static_assert(WTN == W_STRIDE, "a thread per node slot");
constexpr int W_ROUNDS = 12;              // 2**12 = cells of a tile >= any simple path
constexpr unsigned long long W_TAINT = 1ull << 63;
constexpr uint32_t W_AMASK = 0x1fffu, W_SENT = W_AMASK, W_RMASK = 0xfffu;
constexpr int W_RSHIFT = 13;
constexpr uint16_t W_NOEXIT = 0xffffu;
constexpr uint32_t W_DEXT_ONE = 1u << 16, W_ARRIVED = 0xffffu;     // `arrived`: deliveries of phase 2 | external in-degree << 16
enum : uint8_t { WF_EXIT = 1, WF_SRC = 2 };

struct WNodes {           // index = tile * W_STRIDE + slot
    unsigned long long *sum;     // per EXIT: local sum, + the flux routed through it (phase 2)
    unsigned long long *inflow;  // per ENTRY: the delivered flux
    uint32_t *pend;       // per EXIT: exits that feed it and have not fired yet
    uint32_t *arrived;    // per ENTRY
    int32_t *next;        // per EXIT: the exit its flux continues to (-1: none)
    int32_t *dst;         // per EXIT: the entry it flows into
    uint16_t *exit_of;    // per perimeter cell: slot of the exit of its tile-local path (W_NOEXIT: ends inside / leaves the raster)
    uint8_t *flags;
};

__device__ __forceinline__ int w_perim_slot(int r, int c)
{
    if (r == 0) return c;
    if (r == WT - 1) return WT + c;
    if (c == 0) return 2 * WT + (r - 1);
    if (c == WT - 1) return 2 * WT + (WT - 2) + (r - 1);
    return -1;
}
__device__ __forceinline__ void w_perim_cell(int p, int &r, int &c)
{
    if (p < WT) { r = 0; c = p; }
    else if (p < 2 * WT) { r = WT - 1; c = p - WT; }
    else if (p < 2 * WT + (WT - 2)) { r = p - 2 * WT + 1; c = 0; }
    else { r = p - 2 * WT - (WT - 2) + 1; c = WT - 1; }
}

// ---- the tile pass (phase 1: FINAL == false, phase 3: FINAL == true) ------------------------------------------------------------
template <bool FINAL>
__global__ __launch_bounds__(WTN) void wacc_tile_kernel(const uint8_t *__restrict__ fd, const uint32_t *__restrict__ wt, unsigned long long *__restrict__ out,
                                                        int64_t H, int64_t W, int ntc, WNodes nd, unsigned long long *unresolved)
{
    __shared__ unsigned long long S[WT * WT];
    __shared__ uint32_t P[WT * WT];                         // A | R << 13
    __shared__ uint8_t code_l[FINAL ? 1 : WT * WT];         // phase 1 looks up the direction of the cell a path ends at
    __shared__ unsigned long long inflow_l[FINAL ? W_STRIDE : 1];
    __shared__ uint32_t arrived_l[FINAL ? W_STRIDE : 1];
    __shared__ int vote_w[3];
    const int tile = blockIdx.x;
    const int ti = tile / ntc, tj = tile - ti * ntc;
    const int64_t r0 = (int64_t)ti * WT, c0 = (int64_t)tj * WT;
    const int tid = threadIdx.x;
    if (tid < 3) vote_w[tid] = 0;
    if (FINAL) {      // what phase 2 delivered to my perimeter cells (WTN == W_STRIDE)
        inflow_l[tid] = nd.inflow[(int64_t)tile * W_STRIDE + tid];
        arrived_l[tid] = nd.arrived[(int64_t)tile * W_STRIDE + tid];
        __syncthreads();
    }
    // my W_CPT cells: i = tid + WTN j (a wavefront takes one row of the tile per step)
    uint32_t wreg[W_CPT];
    uint8_t creg[W_CPT];
#pragma unroll
    for (int j = 0; j < W_CPT; ++j) {
        const int i = tid + WTN * j;
        const int r = i / WT, c = i - r * WT;
        const bool inside = (r0 + r) < H && (c0 + c) < W;
        creg[j] = inside ? fd[(r0 + r) * W + c0 + c] : (uint8_t)8;
        wreg[j] = inside ? wt[(r0 + r) * W + c0 + c] : 0u;
    }
#pragma unroll
    for (int j = 0; j < W_CPT; ++j) {
        const int i = tid + WTN * j;
        const int r = i / WT, c = i - r * WT;
        const bool inside = (r0 + r) < H && (c0 + c) < W;
        unsigned long long v = wreg[j];      // (not a raster cell: 0, no pointer, and nobody points at it)
        if (FINAL && inside) {
            const int slot = w_perim_slot(r, c);
            if (slot >= 0) {
                const uint32_t ar = arrived_l[slot], dext = ar >> 16;
                if (dext) {
                    if ((ar & W_ARRIVED) == dext) v += inflow_l[slot];
                    else v |= W_TAINT;      // a delivery never comes: this entry lies on a flow cycle across tiles
                }
            }
        }
        const unsigned code = creg[j];
        uint32_t nx = W_SENT;
        if (inside && code <= 7u) {
            const int nr = r + dir_dr((int)code), nc = c + dir_dc((int)code);
            if (nr >= 0 && nr < WT && nc >= 0 && nc < WT && (r0 + nr) < H && (c0 + nc) < W) nx = (uint32_t)(nr * WT + nc);
        }
        S[i] = v;
        P[i] = nx | ((uint32_t)i << W_RSHIFT);
        if (!FINAL) code_l[i] = (uint8_t)code;
    }
    __syncthreads();

    WgVote vote(vote_w);
    bool more = true;
    for (int round = 0; round < W_ROUNDS && more; ++round) {
        unsigned long long s[W_CPT];
        uint32_t a[W_CPT], aa[W_CPT];
#pragma unroll
        for (int j = 0; j < W_CPT; ++j) {
            const int i = tid + WTN * j;
            a[j] = P[i] & W_AMASK;
            s[j] = 0;
            aa[j] = W_SENT;
            if (a[j] != W_SENT) {
                s[j] = S[i];
                aa[j] = P[a[j]];
            }
        }
        __syncthreads();      // every read of S_k and A_k is done
        bool mine = false;
#pragma unroll
        for (int j = 0; j < W_CPT; ++j) {
            const int i = tid + WTN * j;
            if (a[j] != W_SENT) {
                atomicAdd(&S[a[j]], s[j] & ~W_TAINT);
                if (s[j] & W_TAINT) atomicOr(&S[a[j]], W_TAINT);
                P[i] = aa[j];      // A_{k+1} | R_{k+1}
                mine |= (aa[j] & W_AMASK) != W_SENT;
            }
        }
        more = vote.any(mine);     // (its barrier ends the round)
    }
    if (more) {
        // still walking after 2**12 steps: the path has entered a flow cycle, and A is a cell ON it; over all such paths these cells
        // cover the cycle (a rotation of the cycle is onto).  The sums of its cells are meaningless -- and flow nowhere else
#pragma unroll
        for (int j = 0; j < W_CPT; ++j) {
            const uint32_t a = P[tid + WTN * j] & W_AMASK;
            if (a != W_SENT) atomicOr(&S[a], W_TAINT);
        }
        __syncthreads();
    }

    if (FINAL) {
        unsigned int cnt = 0;
#pragma unroll
        for (int j = 0; j < W_CPT; ++j) {
            const int i = tid + WTN * j;
            const int r = i / WT, c = i - r * WT;
            if ((r0 + r) < H && (c0 + c) < W) {
                const unsigned long long v = S[i];
                const bool t = (v & W_TAINT) != 0;
                cnt += t ? 1u : 0u;
                out[(r0 + r) * W + c0 + c] = t ? MHIP_WACC_UNRESOLVED : v;
            }
        }
        fd_count_add(cnt, unresolved);
        return;
    }

    // phase 1: publish the perimeter
    if (tid < W_PERIM) {
        int r, c;
        w_perim_cell(tid, r, c);
        const int64_t node = (int64_t)tile * W_STRIDE + tid;
        const bool inside = (r0 + r) < H && (c0 + c) < W;
        const uint32_t pw = P[r * WT + c];
        const unsigned code = code_l[r * WT + c];
        uint8_t fl = 0;
        int32_t dst = -1;
        if (inside && code <= 7u) {
            const int nr = r + dir_dr((int)code), nc = c + dir_dc((int)code);
            const int64_t gr = r0 + nr, gc = c0 + nc;
            if ((nr < 0 || nr >= WT || nc < 0 || nc >= WT) && gr >= 0 && gr < H && gc >= 0 && gc < W) {
                fl = WF_EXIT;
                dst = ((int)(gr / WT) * ntc + (int)(gc / WT)) * W_STRIDE + w_perim_slot((int)(gr % WT), (int)(gc % WT));
            }
        }
        // where my tile-local path leaves the tile: through its last cell, iff that cell flows into a raster cell of another tile.  A
        // path that ends in a sink, leaves the raster or runs into a flow cycle has no exit
        uint16_t ex = W_NOEXIT;
        if (inside && (pw & W_AMASK) == W_SENT) {
            const int last = (int)((pw >> W_RSHIFT) & W_RMASK);
            const int pr = last / WT, pc = last - pr * WT;
            const unsigned cd = code_l[last];
            if (cd <= 7u) {
                const int nr = pr + dir_dr((int)cd), nc = pc + dir_dc((int)cd);
                const int64_t gr = r0 + nr, gc = c0 + nc;
                if ((nr < 0 || nr >= WT || nc < 0 || nc >= WT) && gr >= 0 && gr < H && gc >= 0 && gc < W) ex = (uint16_t)w_perim_slot(pr, pc);
            }
        }
        nd.flags[node] = fl;
        nd.dst[node] = dst;
        nd.exit_of[node] = ex;
        nd.sum[node] = S[r * WT + c] & ~W_TAINT;      // (an exit is never tainted here: a cycle inside the tile does not leave it)
        nd.next[node] = -1;
        if (dst >= 0) atomicAdd(&nd.arrived[dst], W_DEXT_ONE);      // (pend / inflow / arrived: zeroed by the host before this launch)
    }
}

// ---- phase 2: the perimeter graph -----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void wacc_link_kernel(WNodes nd, int64_t nnodes)
{
    const int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= nnodes || (x % W_STRIDE) >= W_PERIM) return;
    if (!(nd.flags[x] & WF_EXIT)) return;
    const int32_t e = nd.dst[x];
    const uint16_t ex = nd.exit_of[e];
    if (ex == W_NOEXIT) return;
    const int32_t nx = (e / W_STRIDE) * W_STRIDE + ex;
    nd.next[x] = nx;
    atomicAdd(&nd.pend[nx], 1u);
}

// the sources, fixed before the walk starts (a count that the walk brings to 0 belongs to its last arriver alone)
__global__ __launch_bounds__(256) void wacc_mark_kernel(WNodes nd, int64_t nnodes)
{
    const int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= nnodes || (x % W_STRIDE) >= W_PERIM) return;
    if ((nd.flags[x] & WF_EXIT) && nd.pend[x] == 0u) nd.flags[x] |= WF_SRC;
}

__global__ __launch_bounds__(256) void wacc_graph_walk_kernel(WNodes nd, int64_t nnodes)
{
    int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= nnodes || (x % W_STRIDE) >= W_PERIM) return;
    if (!(nd.flags[x] & WF_SRC)) return;
    unsigned long long total = nd.sum[x];
    int32_t e = nd.dst[x], nx = nd.next[x];
    for (;;) {      // (every step takes one pending count away: the walk ends, cycles or not)
        atomicAdd(&nd.inflow[e], total);
        atomicAdd(&nd.arrived[e], 1u);
        if (nx < 0) break;
        atomicAdd(&nd.sum[nx], total);
        __threadfence();                                    // my add is out before my decrement can be seen
        if (atomicSub(&nd.pend[nx], 1u) != 1u) break;       // somebody else arrives later and takes it from here
        __threadfence();
        total = atomicAdd(&nd.sum[nx], 0ull);               // the last arriver: every add is in
        e = nd.dst[nx];
        nx = nd.next[nx];
    }
}

// ---- the sums of a uint32 raster per label ----------------------------------------------------------------------------------------
// A thread folds the runs of equal label of 8 consecutive cells in registers, a workgroup folds the runs of a chunk of 2048 cells in
// an LDS table (64-bit LDS adds) and sends one global atomic per label of the chunk; a run without a slot goes to the global atomics
// itself.  A label outside [0, nzone] raises `bad` and is not summed.
constexpr int ZS_SLOTS = 256, ZS_RUN = 8;
__global__ __launch_bounds__(256) void wacc_zone_sum_kernel(const uint32_t *__restrict__ wt, const int32_t *__restrict__ zones, int64_t n, int64_t nzone,
                                                           unsigned long long *sums, unsigned int *bad)
{
    __shared__ int keys[ZS_SLOTS];
    __shared__ unsigned long long vals[ZS_SLOTS];
    auto push = [&](int32_t lab, unsigned long long v) {
        if (lab < 0 || (int64_t)lab > nzone) {
            *bad = 1u;
            return;
        }
        const int h = table_slot<ZS_SLOTS>(keys, (int)lab);
        if (h >= 0) atomicAdd(&vals[h], v);
        else atomicAdd(&sums[lab], v);
    };
    const int64_t chunk = (int64_t)256 * ZS_RUN;
    for (int64_t base = (int64_t)blockIdx.x * chunk; base < n; base += (int64_t)gridDim.x * chunk) {      // (block-uniform)
        // a table per chunk of 2048 consecutive cells, as the tables per tile of zones.hip: the labels of a chunk are few, those of
        // all the chunks of a block are not
        for (int h = threadIdx.x; h < ZS_SLOTS; h += 256) {
            keys[h] = -1;
            vals[h] = 0ull;
        }
        __syncthreads();
        const int64_t i0 = base + (int64_t)threadIdx.x * ZS_RUN;
        if (i0 < n) {
        uint32_t w[ZS_RUN];
        int32_t z[ZS_RUN];
        if (i0 + ZS_RUN <= n) {      // (i0 is a multiple of 8: 32-byte aligned in both rasters)
            const uint4 wa = *reinterpret_cast<const uint4 *>(wt + i0), wb = *reinterpret_cast<const uint4 *>(wt + i0 + 4);
            const int4 za = *reinterpret_cast<const int4 *>(zones + i0), zb = *reinterpret_cast<const int4 *>(zones + i0 + 4);
            w[0] = wa.x; w[1] = wa.y; w[2] = wa.z; w[3] = wa.w; w[4] = wb.x; w[5] = wb.y; w[6] = wb.z; w[7] = wb.w;
            z[0] = za.x; z[1] = za.y; z[2] = za.z; z[3] = za.w; z[4] = zb.x; z[5] = zb.y; z[6] = zb.z; z[7] = zb.w;
        } else {
#pragma unroll
            for (int t = 0; t < ZS_RUN; ++t) {
                const bool in = i0 + t < n;
                w[t] = in ? wt[i0 + t] : 0u;
                z[t] = in ? zones[i0 + t] : zones[i0];      // (the tail joins the run in front of it with nothing)
            }
        }
        int32_t lab = z[0];
        unsigned long long acc = w[0];
#pragma unroll
        for (int t = 1; t < ZS_RUN; ++t) {
            if (z[t] != lab) {
                push(lab, acc);
                lab = z[t];
                acc = 0ull;
            }
            acc += w[t];
        }
        push(lab, acc);
        }
        __syncthreads();
        for (int h = threadIdx.x; h < ZS_SLOTS; h += 256)
            if (keys[h] >= 0 && vals[h]) atomicAdd(&sums[keys[h]], vals[h]);
        __syncthreads();
    }
}

// ---- the float view of rows of a result: (float64(sum) / div) * mul, every operation rounded on its own ---------------------------
__global__ __launch_bounds__(256) void wacc_view_kernel(const unsigned long long *__restrict__ acc, int64_t n, double div, double mul, double nodata,
                                                       double *__restrict__ dst)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned long long v = acc[i];
    dst[i] = v == MHIP_WACC_UNRESOLVED ? nodata : __dmul_rn(__ddiv_rn(__ull2double_rn(v), div), mul);
}

}  // namespace

int wacc_check(int64_t H, int64_t W, int64_t nzone, bool zones)
{
    MH_ARG(H >= 1 && W >= 1 && H <= 0x7fffffff && W <= 0x7fffffff, "weighted_accum: H, W in [1, 2**31 - 1]");
    if (H * W >= (1ll << 31)) {      // (bit 63 of a sum is the kernels' taint flag)
        set_error("weighted_accum: %lld x %lld cells: a raster holds fewer than 2**31 cells", (long long)H, (long long)W);
        return MHIP_ELIMIT;
    }
    if (zones) MH_ARG(nzone >= 0 && nzone < 0x7fffffff, "weighted_accum: nzone in [0, 2**31 - 2]");
    return MHIP_OK;
}

// The accumulation of d_w down d_fd into d_out (uint64, H x W), the number of unresolved cells into *unresolved and, with d_zones, the
// sums of d_w per label into d_sums (uint64, nzone + 1).  Synchronises.  MHIP_EINVAL: a label outside [0, nzone].
int wacc_dev(const uint8_t *d_fd, const uint32_t *d_w, const int32_t *d_zones, int64_t H, int64_t W, int64_t nzone, unsigned long long *d_out,
             unsigned long long *d_sums, int64_t *unresolved, hipStream_t s)
{
    MH_TRY(wacc_check(H, W, nzone, d_zones != nullptr));
    const int ntr = (int)cdiv(H, WT), ntc = (int)cdiv(W, WT);
    const int64_t ntiles = (int64_t)ntr * ntc, nnodes = ntiles * W_STRIDE;
    if (nnodes >= (int64_t)INT32_MAX) {      // (a raster a few cells high or wide: every cell is a perimeter cell)
        set_error("weighted_accum: raster too large for the int32 perimeter-node domain");
        return MHIP_ELIMIT;
    }
    auto align = [](size_t x) { return (x + 255) & ~size_t(255); };
    const size_t o_sum = 0, o_inflow = align(o_sum + 8 * (size_t)nnodes), o_pend = align(o_inflow + 8 * (size_t)nnodes),
                 o_arrived = align(o_pend + 4 * (size_t)nnodes), o_next = align(o_arrived + 4 * (size_t)nnodes),
                 o_dst = align(o_next + 4 * (size_t)nnodes), o_exit = align(o_dst + 4 * (size_t)nnodes), o_flags = align(o_exit + 2 * (size_t)nnodes),
                 o_cnt = align(o_flags + (size_t)nnodes), bytes = o_cnt + 256;
    DevBuf buf;
    MH_TRY(buf.alloc(bytes));
    char *b = buf.as<char>();
    WNodes nd;
    nd.sum = reinterpret_cast<unsigned long long *>(b + o_sum);
    nd.inflow = reinterpret_cast<unsigned long long *>(b + o_inflow);
    nd.pend = reinterpret_cast<uint32_t *>(b + o_pend);
    nd.arrived = reinterpret_cast<uint32_t *>(b + o_arrived);
    nd.next = reinterpret_cast<int32_t *>(b + o_next);
    nd.dst = reinterpret_cast<int32_t *>(b + o_dst);
    nd.exit_of = reinterpret_cast<uint16_t *>(b + o_exit);
    nd.flags = reinterpret_cast<uint8_t *>(b + o_flags);
    unsigned long long *d_cnt = reinterpret_cast<unsigned long long *>(b + o_cnt);      // [0]: unresolved cells, [1] (as 32 bits): a bad label
    MH_HIP(hipMemsetAsync(b, 0, bytes, s));      // (the four unused slots of every tile stay no exit, no entry)
    const unsigned gn = (unsigned)cdiv(nnodes, 256);
    hipLaunchKernelGGL((wacc_tile_kernel<false>), dim3((unsigned)ntiles), dim3(WTN), 0, s, d_fd, d_w, d_out, H, W, ntc, nd, d_cnt);
    hipLaunchKernelGGL(wacc_link_kernel, dim3(gn), dim3(256), 0, s, nd, nnodes);
    hipLaunchKernelGGL(wacc_mark_kernel, dim3(gn), dim3(256), 0, s, nd, nnodes);
    hipLaunchKernelGGL(wacc_graph_walk_kernel, dim3(gn), dim3(256), 0, s, nd, nnodes);
    hipLaunchKernelGGL((wacc_tile_kernel<true>), dim3((unsigned)ntiles), dim3(WTN), 0, s, d_fd, d_w, d_out, H, W, ntc, nd, d_cnt);
    if (d_zones) {
        const int64_t n = H * W;
        const int64_t nb = cdiv(n, (int64_t)256 * ZS_RUN);
        MH_HIP(hipMemsetAsync(d_sums, 0, 8 * (size_t)(nzone + 1), s));
        hipLaunchKernelGGL(wacc_zone_sum_kernel, dim3((unsigned)(nb < 2048 ? nb : 2048)), dim3(256), 0, s, d_w, d_zones, n, nzone, d_sums,
                           reinterpret_cast<unsigned int *>(d_cnt + 1));
    }
    MH_HIP(hipGetLastError());
    unsigned long long h_cnt[2] = {0, 0};
    MH_HIP(hipMemcpyAsync(h_cnt, d_cnt, 16, hipMemcpyDeviceToHost, s));
    MH_HIP(stream_sync(s));      // (the node buffer goes back to the pool)
    if (h_cnt[1]) {
        set_error("invalid argument: weighted_accum: a label outside [0, %lld]", (long long)nzone);
        return MHIP_EINVAL;
    }
    *unresolved = (int64_t)h_cnt[0];
    return MHIP_OK;
}

// the float view of rows [row0, row0 + nrows) of a result into the caller's array
int wacc_rows_f64_dev(const mhip_wacc *p, int64_t row0, int64_t nrows, double div, double mul, double nodata, double *dst)
{
    MH_HIP(hipSetDevice(p->device));
    hipStream_t s = 0;
    const int64_t n = nrows * p->W;
    DevBuf view;
    MH_TRY(view.alloc(8 * (size_t)n));
    hipLaunchKernelGGL(wacc_view_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, s, p->acc.as<unsigned long long>() + row0 * p->W, n, div, mul, nodata,
                       view.as<double>());
    MH_HIP(hipGetLastError());
    return download(dst, view, 8 * (size_t)n, s);
}

}  // namespace mh
