// polygonize.hip -- the outlines of the regions of an int32 label raster as rings of lattice vertices (gfx950).
//
// The reference hands this step to GDAL (vector.py:70-74, 8CONNECTED=8); tests/_polygonize.py is the definition.  Vertex (x, y), x in
// [0, W], y in [0, H]; cell (r, c) has the corners (c, r) .. (c + 1, r + 1).  Every side of a cell of label l != 0 whose neighbour
// across it has another value, or lies outside, is a directed unit EDGE of l with the cell on its right: heading 0 right (the top
// side), 1 down (the right side), 2 left (the bottom side), 3 up (the left side).  The SUCCESSOR of an edge is the first that exists
// among the edges of l that start at its end vertex, in the order left turn, straight on, right turn; every edge has exactly one
// successor and one predecessor, so the rings are the cycles of a permutation.  A ring keeps the start vertices of its edges whose
// predecessor has another heading (CORNERS), begins at its smallest vertex by (y, x) and is not closed; rings are ordered by that
// vertex, then by the heading of their first edge.
//
// An edge is named by (start vertex, heading), and the edges are numbered in the order of that key: the smallest edge of a ring is
// the one that starts at the ring's smallest vertex, and the order of the rings is the order of their smallest edges.
//   pg_count_kernel       one thread per vertex: the headings that start there (four cells), counted; a sum per block of 1024
//   pg_scan_kernel        the exclusive prefix over the block sums, one workgroup (as ccl.hip's scan_blocks_kernel)
//   pg_base_kernel        the number of the first edge of every vertex: block offset + prefix inside the block
//   pg_edges_kernel       one thread per vertex, per edge: its successor's number, its start vertex and label; it tells the successor
//                         whether it is a corner
//   pg_init_kernel        the state of the window [e, e + 1) of every edge e
//   pg_jump_kernel        pointer doubling, one launch per round, from one state array into the other: the window of 2^k edges behind
//                         e becomes the window of 2^(k+1): its smallest edge m, the corners in front of m's first occurrence, the
//                         corners of the window, and the edge behind the window.  An edge whose window and the window behind
//                         it hold the same m is done -- the two hold its whole ring, m is the ring's first edge and the count the
//                         corners from e to it -- and points at itself from then on.  A round that moves no m was the last.
//                         log2(longest ring) + 2 rounds; the host reads one word every fourth round
//   pg_ring_count_kernel  an edge with m == e starts a ring; the corners of its ring are those from its successor to it, + 1.  (rings,
//                         vertices) per block, packed into 64 bits, scanned by pg_scan_kernel
//   pg_ring_emit_kernel   the prefix inside the block: a ring's number and the offset of its vertices, written where its first edge
//                         is, and ring_offsets / ring_label
//   pg_vertex_emit_kernel one thread per edge: a corner goes to slot offset + (corners of the ring - corners from e to the first edge)
// No thread walks a ring; the cost is vertices + edges * (log2(longest ring) + 1); the host does no work per edge.
#include "common.hpp"

namespace mh {
namespace {

constexpr int PB = 1024;                     // vertices / edges per block of the counting and prefix kernels
constexpr int PG_MAX_ROUNDS = 40;            // 2**32 edges need 33
constexpr int PG_CHECK_EVERY = 4;            // rounds between two looks of the host

struct PgGeom {
    int64_t H, W, W1, NV;      // W1 = W + 1, NV = (H + 1) * (W + 1)
};

__device__ __forceinline__ int32_t pg_cell(const int32_t *__restrict__ lab, const PgGeom &g, int64_t r, int64_t c)
{
    return (r < 0 || r >= g.H || c < 0 || c >= g.W) ? 0 : lab[r * g.W + c];
}

// the headings that start at vertex (x, y) as a mask of four bits; own[d]: the label of heading d's cell
__device__ __forceinline__ unsigned pg_mask(const int32_t *__restrict__ lab, const PgGeom &g, int64_t x, int64_t y, int32_t own[4])
{
    const int32_t nw = pg_cell(lab, g, y - 1, x - 1), ne = pg_cell(lab, g, y - 1, x), sw = pg_cell(lab, g, y, x - 1), se = pg_cell(lab, g, y, x);
    own[0] = se; own[1] = sw; own[2] = nw; own[3] = ne;      // right: top side of SE, down: right side of SW, left: bottom side of NW, up: left side of NE
    return (se != 0 && se != ne ? 1u : 0u) | (sw != 0 && sw != se ? 2u : 0u) | (nw != 0 && nw != sw ? 4u : 0u) | (ne != 0 && ne != nw ? 8u : 0u);
}

__device__ __forceinline__ int pg_dx(int d) { return d == 0 ? 1 : d == 2 ? -1 : 0; }
__device__ __forceinline__ int pg_dy(int d) { return d == 1 ? 1 : d == 3 ? -1 : 0; }

// the sum of v over the block of PB threads, valid in thread 0
template <typename T> __device__ __forceinline__ T pg_block_sum(T v, T *wsum)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
    __syncthreads();
    T t = 0;
    if (threadIdx.x == 0)
        for (int k = 0; k < PB / 64; ++k) t += wsum[k];
    return t;
}

// the sum of v over the threads of the block in front of this one
template <typename T> __device__ __forceinline__ T pg_block_prefix(T v, T *wsum)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T u = __shfl_up(incl, o);
        if (lane >= o) incl += u;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    T woff = 0;
    for (int k = 0; k < wave; ++k) woff += wsum[k];
    return woff + incl - v;
}

__global__ __launch_bounds__(PB) void pg_count_kernel(const int32_t *__restrict__ lab, PgGeom g, uint32_t *__restrict__ block_counts, unsigned int *bad)
{
    __shared__ uint32_t wsum[PB / 64];
    const int64_t v = (int64_t)blockIdx.x * PB + threadIdx.x;
    uint32_t cnt = 0;
    if (v < g.NV) {
        const int64_t y = v / g.W1, x = v - y * g.W1;
        int32_t own[4];
        cnt = (uint32_t)__popc(pg_mask(lab, g, x, y, own));
        if (own[0] < 0) atomicOr(bad, 1u);      // (SE: every cell is the SE cell of one vertex)
    }
    const uint32_t t = pg_block_sum(cnt, wsum);
    if (threadIdx.x == 0) block_counts[blockIdx.x] = t;
}

// exclusive prefix over nb block sums in place, the total to *total: one workgroup, thread t the t-th run of blocks
template <typename T> __global__ __launch_bounds__(1024) void pg_scan_kernel(T *block_counts, int64_t nb, unsigned long long *total)
{
    __shared__ unsigned long long part[1024];
    const int64_t per = (nb + 1023) / 1024;
    const int64_t b0 = (int64_t)threadIdx.x * per < nb ? (int64_t)threadIdx.x * per : nb, b1 = b0 + per < nb ? b0 + per : nb;
    unsigned long long s = 0;
    for (int64_t b = b0; b < b1; ++b) s += block_counts[b];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long run = 0;
        for (int t = 0; t < 1024; ++t) {
            const unsigned long long v = part[t];
            part[t] = run;
            run += v;
        }
        *total = run;
    }
    __syncthreads();
    unsigned long long run = part[threadIdx.x];
    for (int64_t b = b0; b < b1; ++b) {
        const T v = block_counts[b];
        block_counts[b] = (T)run;
        run += v;
    }
}

__global__ __launch_bounds__(PB) void pg_base_kernel(const int32_t *__restrict__ lab, PgGeom g, const uint32_t *__restrict__ block_offsets,
                                                    uint32_t *__restrict__ vbase)
{
    __shared__ uint32_t wsum[PB / 64];
    const int64_t v = (int64_t)blockIdx.x * PB + threadIdx.x;
    uint32_t cnt = 0;
    if (v < g.NV) {
        const int64_t y = v / g.W1, x = v - y * g.W1;
        int32_t own[4];
        cnt = (uint32_t)__popc(pg_mask(lab, g, x, y, own));
    }
    const uint32_t before = pg_block_prefix(cnt, wsum);
    if (v < g.NV) vbase[v] = block_offsets[blockIdx.x] + before;
}

__global__ __launch_bounds__(PB) void pg_edges_kernel(const int32_t *__restrict__ lab, PgGeom g, const uint32_t *__restrict__ vbase,
                                                      uint32_t nedge, uint32_t *__restrict__ succ, int2 *__restrict__ evert,
                                                      int32_t *__restrict__ elab, uint8_t *corner)
{
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= g.NV) return;
    const int64_t y = v / g.W1, x = v - y * g.W1;
    int32_t own[4];
    const unsigned mask = pg_mask(lab, g, x, y, own);
    if (!mask) return;
    const uint32_t base = vbase[v];
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        if (!(mask & (1u << d))) continue;
        const uint32_t e = base + (uint32_t)__popc(mask & ((1u << d) - 1u));
        if (e >= nedge) continue;               // (it is not: the prefix ends at nedge)
        const int32_t l = own[d];
        // the edge's cell, the cell ahead of it on the right of the line (AR) and the one ahead on the left (AL)
        const int64_t r = y - (d == 2 || d == 3 ? 1 : 0), c = x - (d == 1 || d == 2 ? 1 : 0);
        const int dl = (d + 3) & 3;
        const int64_t ar_r = r + pg_dy(d), ar_c = c + pg_dx(d);
        const int32_t ar = pg_cell(lab, g, ar_r, ar_c), al = pg_cell(lab, g, ar_r + pg_dy(dl), ar_c + pg_dx(dl));
        const int nd = al == l ? dl : ar == l ? d : (d + 1) & 3;      // left turn, straight on, right turn
        const int64_t x2 = x + pg_dx(d), y2 = y + pg_dy(d);           // (inside the lattice: the edge is a side of a cell)
        int32_t own2[4];
        const unsigned mask2 = pg_mask(lab, g, x2, y2, own2);
        uint32_t se = vbase[y2 * g.W1 + x2] + (uint32_t)__popc(mask2 & ((1u << nd) - 1u));
        se = se < nedge ? se : nedge - 1u;      // (it is: the successor exists)
        succ[e] = se;
        evert[e] = make_int2((int)x, (int)y);
        elab[e] = l;
        corner[se] = nd != d ? 1 : 0;      // (every edge is the successor of exactly one edge: every byte is written once)
    }
}

// state of the window behind edge e: x the edge behind the window, y its smallest edge m, z the corners in front of the first
// occurrence of m, w the corners of the window (modulo 2**32 once the window is longer than its ring; not read from then on)
__global__ __launch_bounds__(256) void pg_init_kernel(const uint32_t *__restrict__ succ, const uint8_t *__restrict__ corner, uint32_t nedge,
                                                     uint4 *__restrict__ st)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nedge) return;
    st[e] = make_uint4(succ[e], (uint32_t)e, 0u, corner[e]);
}

__global__ __launch_bounds__(256) void pg_jump_kernel(const uint4 *__restrict__ in, uint4 *__restrict__ out, uint32_t nedge, unsigned int *moved)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool mv = false;
    if (e < nedge) {
        const uint4 a = in[e];
        const uint4 b = in[a.x];
        mv = b.y < a.y;
        // equal: both windows hold the ring's first edge, the first occurrence is the one in `a`, and e is done: m and the count
        // stay, and it points at itself from now on (its look at the window behind becomes a look at its own line; an edge that
        // still reaches it reads m and the count, and is done with that)
        out[e] = make_uint4(b.y == a.y ? (uint32_t)e : b.x, mv ? b.y : a.y, mv ? a.w + b.z : a.z, a.w + b.w);
    }
    if (__any(mv) && (threadIdx.x & 63u) == 0u) *moved = 1u;
}

// (rings << 32) | vertices that start at edge e
__device__ __forceinline__ unsigned long long pg_ring_weight(const uint4 *__restrict__ st, const uint32_t *__restrict__ succ, int64_t e, uint32_t nedge)
{
    if (e >= nedge || st[e].y != (uint32_t)e) return 0ull;
    return (1ull << 32) | (unsigned long long)(st[succ[e]].z + 1u);
}

__global__ __launch_bounds__(PB) void pg_ring_count_kernel(const uint4 *__restrict__ st, const uint32_t *__restrict__ succ, uint32_t nedge,
                                                          unsigned long long *__restrict__ block_sums)
{
    __shared__ unsigned long long wsum[PB / 64];
    const int64_t e = (int64_t)blockIdx.x * PB + threadIdx.x;
    const unsigned long long t = pg_block_sum(pg_ring_weight(st, succ, e, nedge), wsum);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = t;
}

__global__ __launch_bounds__(PB) void pg_ring_emit_kernel(const uint4 *__restrict__ st, const uint32_t *__restrict__ succ, const int32_t *__restrict__ elab,
                                                         uint32_t nedge, const unsigned long long *__restrict__ block_offsets, int64_t nring,
                                                         int64_t nvert, uint2 *__restrict__ rinfo, int64_t *__restrict__ ring_offsets,
                                                         int32_t *__restrict__ ring_label)
{
    __shared__ unsigned long long wsum[PB / 64];
    const int64_t e = (int64_t)blockIdx.x * PB + threadIdx.x;
    const unsigned long long w = pg_ring_weight(st, succ, e, nedge);
    const unsigned long long at = block_offsets[blockIdx.x] + pg_block_prefix(w, wsum);
    if (w) {
        const uint32_t k = (uint32_t)(at >> 32), vo = (uint32_t)at;
        rinfo[e] = make_uint2(vo, (uint32_t)w);
        if ((int64_t)k < nring) {
            ring_offsets[k] = (int64_t)vo;
            ring_label[k] = elab[e];
        }
    }
    if (e == 0) ring_offsets[nring] = nvert;
}

__global__ __launch_bounds__(256) void pg_vertex_emit_kernel(const uint4 *__restrict__ st, const uint8_t *__restrict__ corner, const int2 *__restrict__ evert,
                                                            const uint2 *__restrict__ rinfo, uint32_t nedge, int64_t nvert, int2 *__restrict__ xy)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nedge || !corner[e]) return;
    const uint4 t = st[e];
    const uint2 ring = rinfo[t.y];                                      // x: the offset of the ring's vertices, y: how many
    const uint32_t pos = t.z ? ring.y - t.z : 0u;                       // (t.z: the corners from e to the ring's first edge, e's own among them)
    const int64_t at = (int64_t)ring.x + pos;
    if (at < nvert) xy[at] = evert[e];
}

}  // namespace

int polygonize_check(int64_t H, int64_t W)
{
    MH_ARG(H >= 1 && W >= 1 && W <= 0x7fffffff && H <= 0x7fffffff, "polygonize: H, W in [1, 2**31 - 1]");
    return MHIP_OK;
}

int polygonize_dev(const int32_t *d_lab, int64_t H, int64_t W, DevBuf &d_xy, DevBuf &d_off, DevBuf &d_rl, int64_t *nring, int64_t *nvert, hipStream_t s)
{
    PgGeom g;
    g.H = H; g.W = W; g.W1 = W + 1; g.NV = (H + 1) * (W + 1);
    const int64_t nb = cdiv(g.NV, PB);
    if (nb > 0x7fffffff) {
        set_error("polygonize: %lld vertices exceed the launch grid", (long long)g.NV);
        return MHIP_ELIMIT;
    }
    // words the host reads: [0] the edges, [1] (rings << 32) | vertices, [2] a negative label, [3 ..] "round k moved a window"
    struct Words {
        unsigned long long edges, rings;
        unsigned int bad, pad, moved[PG_MAX_ROUNDS];
    } h;
    DevBuf d_words, d_bc, d_vbase;
    MH_TRY(d_words.alloc(sizeof(Words)));
    MH_HIP(hipMemsetAsync(d_words.p, 0, sizeof(Words), s));
    Words *dw = d_words.as<Words>();
    MH_TRY(d_bc.alloc(4 * (size_t)nb));
    hipLaunchKernelGGL(pg_count_kernel, dim3((unsigned)nb), dim3(PB), 0, s, d_lab, g, d_bc.as<uint32_t>(), &dw->bad);
    hipLaunchKernelGGL(pg_scan_kernel<uint32_t>, dim3(1), dim3(1024), 0, s, d_bc.as<uint32_t>(), nb, &dw->edges);
    MH_HIP(hipGetLastError());
    MH_HIP(hipMemcpyAsync(&h, d_words.p, sizeof(Words), hipMemcpyDeviceToHost, s));
    MH_HIP(stream_sync(s));
    if (h.bad) {
        set_error("invalid argument: polygonize: a negative label");
        return MHIP_EINVAL;
    }
    if (h.edges > 0xffffffffull) {
        set_error("polygonize: %llu boundary edges exceed 2**32 - 1", h.edges);
        return MHIP_ELIMIT;
    }
    *nring = *nvert = 0;
    const uint32_t nedge = (uint32_t)h.edges;
    if (nedge == 0) return MHIP_OK;      // no cell has a label: no ring, and the fetch writes the one offset itself
    const int64_t neb = cdiv((int64_t)nedge, PB);
    const unsigned ge = (unsigned)cdiv((int64_t)nedge, 256);      // (at most 2**24)
    DevBuf d_succ, d_evert, d_elab, d_corner, d_st[2], d_bs, d_rinfo;
    MH_TRY(d_vbase.alloc(4 * (size_t)g.NV));
    MH_TRY(d_succ.alloc(4 * (size_t)nedge));
    MH_TRY(d_evert.alloc(8 * (size_t)nedge));
    MH_TRY(d_elab.alloc(4 * (size_t)nedge));
    MH_TRY(d_corner.alloc((size_t)nedge));
    MH_TRY(d_st[0].alloc(16 * (size_t)nedge));
    MH_TRY(d_st[1].alloc(16 * (size_t)nedge));
    hipLaunchKernelGGL(pg_base_kernel, dim3((unsigned)nb), dim3(PB), 0, s, d_lab, g, d_bc.as<uint32_t>(), d_vbase.as<uint32_t>());
    hipLaunchKernelGGL(pg_edges_kernel, dim3((unsigned)nb), dim3(PB), 0, s, d_lab, g, d_vbase.as<uint32_t>(), nedge, d_succ.as<uint32_t>(), d_evert.as<int2>(),
                       d_elab.as<int32_t>(), d_corner.as<uint8_t>());
    hipLaunchKernelGGL(pg_init_kernel, dim3(ge), dim3(256), 0, s, d_succ.as<uint32_t>(), d_corner.as<uint8_t>(), nedge, d_st[0].as<uint4>());
    int cur = 0, round = 0;
    for (;;) {
        if (round + PG_CHECK_EVERY > PG_MAX_ROUNDS) {
            set_error("polygonize: the rings did not close within %d rounds", PG_MAX_ROUNDS);
            return MHIP_ENOTCONV;
        }
        for (int k = 0; k < PG_CHECK_EVERY; ++k, ++round, cur ^= 1)
            hipLaunchKernelGGL(pg_jump_kernel, dim3(ge), dim3(256), 0, s, d_st[cur].as<uint4>(), d_st[cur ^ 1].as<uint4>(), nedge, &dw->moved[round]);
        MH_HIP(hipGetLastError());
        unsigned int moved = 0;
        MH_HIP(hipMemcpyAsync(&moved, &dw->moved[round - 1], 4, hipMemcpyDeviceToHost, s));
        MH_HIP(stream_sync(s));
        if (!moved) break;
    }
    const uint4 *st = d_st[cur].as<uint4>();
    MH_TRY(d_bs.alloc(8 * (size_t)neb));
    hipLaunchKernelGGL(pg_ring_count_kernel, dim3((unsigned)neb), dim3(PB), 0, s, st, d_succ.as<uint32_t>(), nedge, d_bs.as<unsigned long long>());
    hipLaunchKernelGGL(pg_scan_kernel<unsigned long long>, dim3(1), dim3(1024), 0, s, d_bs.as<unsigned long long>(), neb, &dw->rings);
    MH_HIP(hipGetLastError());
    MH_HIP(hipMemcpyAsync(&h.rings, &dw->rings, 8, hipMemcpyDeviceToHost, s));
    MH_HIP(stream_sync(s));
    const int64_t nr = (int64_t)(h.rings >> 32), nv = (int64_t)(h.rings & 0xffffffffull);
    MH_TRY(d_rinfo.alloc(8 * (size_t)nedge));
    MH_TRY(d_xy.alloc(8 * (size_t)nv));
    MH_TRY(d_off.alloc(8 * (size_t)(nr + 1)));
    MH_TRY(d_rl.alloc(4 * (size_t)nr));
    hipLaunchKernelGGL(pg_ring_emit_kernel, dim3((unsigned)neb), dim3(PB), 0, s, st, d_succ.as<uint32_t>(), d_elab.as<int32_t>(), nedge,
                       d_bs.as<unsigned long long>(), nr, nv, d_rinfo.as<uint2>(), d_off.as<int64_t>(), d_rl.as<int32_t>());
    hipLaunchKernelGGL(pg_vertex_emit_kernel, dim3(ge), dim3(256), 0, s, st, d_corner.as<uint8_t>(), d_evert.as<int2>(), d_rinfo.as<uint2>(), nedge,
                       nv, d_xy.as<int2>());
    MH_HIP(hipGetLastError());
    MH_HIP(stream_sync(s));      // (the work buffers may go)
    *nring = nr;
    *nvert = nv;
    return MHIP_OK;
}

// the three buffers of a handle to the caller's arrays: copies on the null stream of the handle's device, one synchronisation
int polygons_fetch_dev(const mhip_polygons *p, int32_t *xy, int64_t *ring_offsets, int32_t *ring_label)
{
    if (p->nring == 0) {
        ring_offsets[0] = 0;
        return MHIP_OK;
    }
    MH_HIP(hipSetDevice(p->device));
    hipStream_t s = 0;
    MH_HIP(hipMemcpyAsync(xy, p->xy.p, 8 * (size_t)p->nvert, hipMemcpyDeviceToHost, s));
    MH_HIP(hipMemcpyAsync(ring_offsets, p->ring_offsets.p, 8 * ((size_t)p->nring + 1), hipMemcpyDeviceToHost, s));
    MH_HIP(hipMemcpyAsync(ring_label, p->ring_label.p, 4 * (size_t)p->nring, hipMemcpyDeviceToHost, s));
    MH_HIP(stream_sync(s));
    return MHIP_OK;
}

}  // namespace mh
