// flowpaths.hip -- the stream network above an accumulation threshold as lines with the upstream area on them (gfx950).
//
// tests/_flowpaths.py is the definition.  A cell is a STREAM CELL when accum >= threshold and its label is 0; down(c) is the neighbour
// its AGNPS code points at (none: a code > 7, or outside); indeg(c) counts the stream cells that step to c.  A stream cell is FIRST
// when indeg != 1 (a head or a confluence) and LAST when down(c) is none, no stream cell or a confluence.  The SUCCESSOR of a stream
// cell that is not last is down(c); every stream cell that is not first has exactly one predecessor.  So the mask falls apart into
// chains from a first to a last cell -- the REACHES -- and into cycles that nothing flows into.  A reach keeps its first cell, its
// last point and every point where the step changes; the reaches are ordered by their first cell.
//
// The stream cells are numbered in raster order (their COMPACT index) by a popcount prefix over one bit per cell:
//   fp_class_kernel        one thread per cell, a 3 x 3 stencil for a stream cell only: one class byte (stream, indeg clipped to 2,
//                          "the predecessor's code differs", the code), one bit per cell in 64-cell words, the `bad` word
//   fp_wcount_kernel       the stream cells of every block of 1024 words
//   fp_scan_kernel         the exclusive prefix over the block sums, one workgroup (as polygonize.hip's pg_scan_kernel)
//   fp_wbase_kernel        the compact index of the first cell of every word
//   fp_compact_kernel      one thread per cell: a stream cell reads the class byte of down(c) and fills the compact arrays -- its cell,
//                          its flags (first, last, kept, "e is appended", the end kind) and the state of the window [c, down(c))
//   fp_jump_kernel         pointer doubling, one launch per round, from one state array into the other: the window [c, p) becomes
//                          [c, p'), p' the end of p's window: the pointer, the orthogonal and the diagonal steps to it and the kept
//                          cells in the window.  A last cell points at itself with an empty window.  ceil(log2(stream cells)) + 1
//                          rounds at most; the host reads one "a pointer moved" word every fourth round.  What does not point at a
//                          last cell after that lies on a cycle that nothing flows into
//   fp_reach_count_kernel  a first cell starts a reach: (1 << 32) + its vertices per block, and the unresolved cells
//   fp_reach_emit_kernel   the prefix inside the block: the reach's number, the offset of its vertices and the kept cells in front of
//                          its last cell, written where its LAST cell is; reach_offsets
//   fp_vertex_kernel       one thread per stream cell: a kept cell goes to slot offset + (kept cells of the reach - kept cells from it
//                          on); a last cell appends e = down(c)
//   fp_record_kernel       one thread per stream cell: a first cell writes the record of its reach; to_reach is the number held where
//                          the reach of end_cell ends
//   fp_reachcell_kernel    (only with a reach raster) one thread per cell: a stream cell writes the number of its reach
//                          + 1 -- rinfo where its pointer rests -- or 0 when that is no last cell; every other cell writes 0
// No thread walks a reach.  The Strahler orders are one pass of Kahn's algorithm over to_reach on the host (flowpaths_fetch_dev).
#include <new>
#include <vector>

#include "common.hpp"

namespace mh {
namespace {

constexpr int FB = 1024;                     // cells / words / stream cells per block of the counting and prefix kernels
constexpr int FP_MAX_ROUNDS = 40;            // 2**31 stream cells need 32
constexpr int FP_CHECK_EVERY = 4;            // rounds between two looks of the host

// class byte of a cell (0: no stream cell)
constexpr unsigned CL_STREAM = 1u, CL_INDEG_SHIFT = 1u, CL_PREDDIFF = 8u, CL_CODE_SHIFT = 4u;
// flags of a stream cell; bits 4 .. 6 the end kind of a last cell
constexpr unsigned FL_FIRST = 1u, FL_LAST = 2u, FL_KEEP = 4u, FL_APP = 8u, FL_KIND_SHIFT = 4u;

struct FpGeom {
    int64_t H, W, N;
};

// the cell that code k points at from cell c, -1: none
__device__ __forceinline__ int64_t fp_down(const FpGeom &g, int64_t c, unsigned k)
{
    if (k > 7u) return -1;
    const int64_t r = c / g.W, col = c - r * g.W;
    const int64_t rr = r + dir_dr((int)k), cc = col + dir_dc((int)k);
    return (rr < 0 || rr >= g.H || cc < 0 || cc >= g.W) ? -1 : rr * g.W + cc;
}

// the compact index of stream cell c
__device__ __forceinline__ uint32_t fp_rank(const unsigned long long *__restrict__ bits, const uint32_t *__restrict__ wbase, int64_t c)
{
    return wbase[c >> 6] + (uint32_t)__popcll(bits[c >> 6] & ((1ull << (c & 63)) - 1ull));
}

// the sum of v over the block of FB threads, valid in thread 0
template <typename T> __device__ __forceinline__ T fp_block_sum(T v, T *wsum)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
    __syncthreads();
    T t = 0;
    if (threadIdx.x == 0)
        for (int k = 0; k < FB / 64; ++k) t += wsum[k];
    return t;
}

// the sum of v over the threads of the block in front of this one
template <typename T> __device__ __forceinline__ T fp_block_prefix(T v, T *wsum)
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

__global__ __launch_bounds__(FB) void fp_class_kernel(const uint8_t *__restrict__ fd, const double *__restrict__ acc, const int32_t *__restrict__ lab,
                                                     FpGeom g, double thr, uint8_t *__restrict__ cls, unsigned long long *__restrict__ bits,
                                                     unsigned int *bad)
{
    const int64_t c = (int64_t)blockIdx.x * FB + threadIdx.x;
    bool stream = false;
    if (c < g.N) {
        const int32_t l = lab ? lab[c] : 0;
        if (l < 0) atomicOr(bad, 1u);
        stream = acc[c] >= thr && l == 0;      // (NaN compares false)
        unsigned cl = 0;
        if (stream) {
            const unsigned code = fd[c] > 8 ? 8u : (unsigned)fd[c];
            const int64_t r = c / g.W, col = c - r * g.W;
            unsigned indeg = 0, pcode = 8;
#pragma unroll
            for (int k = 0; k < 8; ++k) {      // the neighbour in direction k steps to c with the opposite code
                const int64_t rr = r + dir_dr(k), cc = col + dir_dc(k);
                if (rr < 0 || rr >= g.H || cc < 0 || cc >= g.W) continue;
                const int64_t nb = rr * g.W + cc;
                if (fd[nb] != (uint8_t)((k + 4) & 7)) continue;
                if (acc[nb] >= thr && (!lab || lab[nb] == 0)) {
                    ++indeg;
                    pcode = (unsigned)((k + 4) & 7);
                }
            }
            cl = CL_STREAM | ((indeg > 2u ? 2u : indeg) << CL_INDEG_SHIFT) | (indeg == 1u && pcode != code ? CL_PREDDIFF : 0u) | (code << CL_CODE_SHIFT);
        }
        cls[c] = (uint8_t)cl;
    }
    const unsigned long long m = __ballot(stream);      // (a wave is the 64 cells of one word: FB is a multiple of 64)
    if ((threadIdx.x & 63) == 0 && c < g.N) bits[c >> 6] = m;
}

__global__ __launch_bounds__(FB) void fp_wcount_kernel(const unsigned long long *__restrict__ bits, int64_t nw, uint32_t *__restrict__ block_counts)
{
    __shared__ uint32_t wsum[FB / 64];
    const int64_t w = (int64_t)blockIdx.x * FB + threadIdx.x;
    const uint32_t t = fp_block_sum(w < nw ? (uint32_t)__popcll(bits[w]) : 0u, wsum);
    if (threadIdx.x == 0) block_counts[blockIdx.x] = t;
}

// exclusive prefix over nb block sums in place, the total to *total: one workgroup, thread t the t-th run of blocks
template <typename T> __global__ __launch_bounds__(1024) void fp_scan_kernel(T *block_counts, int64_t nb, unsigned long long *total)
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

__global__ __launch_bounds__(FB) void fp_wbase_kernel(const unsigned long long *__restrict__ bits, int64_t nw, const uint32_t *__restrict__ block_offsets,
                                                     uint32_t *__restrict__ wbase)
{
    __shared__ uint32_t wsum[FB / 64];
    const int64_t w = (int64_t)blockIdx.x * FB + threadIdx.x;
    const uint32_t before = fp_block_prefix(w < nw ? (uint32_t)__popcll(bits[w]) : 0u, wsum);
    if (w < nw) wbase[w] = block_offsets[blockIdx.x] + before;
}

// state of the window [c, p) of stream cell c: x the compact index of p, y the orthogonal and z the diagonal steps from c to p, w the
// kept cells in the window.  A last cell: (itself, 0, 0, 0).  (On a cycle the counts wrap around; nobody reads them.)
__global__ __launch_bounds__(256) void fp_compact_kernel(const uint8_t *__restrict__ cls, const int32_t *__restrict__ lab, FpGeom g,
                                                        const unsigned long long *__restrict__ bits, const uint32_t *__restrict__ wbase, uint32_t n,
                                                        int64_t *__restrict__ cell, uint8_t *__restrict__ flags, uint4 *__restrict__ st)
{
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= g.N) return;
    const unsigned cl = cls[c];
    if (!(cl & CL_STREAM)) return;
    const uint32_t i = fp_rank(bits, wbase, c);
    if (i >= n) return;                         // (it is not: the prefix ends at n)
    const unsigned code = cl >> CL_CODE_SHIFT;
    const bool first = ((cl >> CL_INDEG_SHIFT) & 3u) != 1u;
    const int64_t d = fp_down(g, c, code);
    bool last = true;
    unsigned kind;
    if (code > 7u) kind = 2;
    else if (d < 0) kind = 1;
    else {
        const unsigned cd = cls[d];
        if (cd & CL_STREAM) {
            kind = 0;
            last = ((cd >> CL_INDEG_SHIFT) & 3u) >= 2u;
        } else
            kind = (lab && lab[d] != 0) ? 3 : 4;
    }
    const bool app = last && (kind == 0u || kind == 3u);
    const bool keep = first || (last && !app) || (cl & CL_PREDDIFF);
    cell[i] = c;
    flags[i] = (uint8_t)((first ? FL_FIRST : 0u) | (last ? FL_LAST : 0u) | (keep ? FL_KEEP : 0u) | (app ? FL_APP : 0u) | (last ? kind << FL_KIND_SHIFT : 0u));
    if (last)
        st[i] = make_uint4(i, 0u, 0u, 0u);
    else {
        uint32_t j = fp_rank(bits, wbase, d);
        j = j < n ? j : n - 1u;                 // (it is: d is a stream cell)
        st[i] = make_uint4(j, (code & 1u) ? 0u : 1u, code & 1u, keep ? 1u : 0u);
    }
}

__global__ __launch_bounds__(256) void fp_jump_kernel(const uint4 *__restrict__ in, uint4 *__restrict__ out, uint32_t n, unsigned int *moved)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool mv = false;
    if (e < n) {
        const uint4 a = in[e];
        const uint4 b = in[a.x];                // (a last cell: its own line, an empty window)
        mv = b.x != a.x;
        out[e] = make_uint4(b.x, a.y + b.y, a.z + b.z, a.w + b.w);
    }
    if (__any(mv) && (threadIdx.x & 63u) == 0u) *moved = 1u;
}

// (reaches << 32) | vertices that start at stream cell e; *unres: e does not reach a last cell
__device__ __forceinline__ unsigned long long fp_reach_weight(const uint4 *__restrict__ st, const uint8_t *__restrict__ flags, int64_t e, uint32_t n, bool *unres)
{
    *unres = false;
    if (e >= n) return 0ull;
    const uint4 t = st[e];
    const unsigned fl = flags[t.x];
    *unres = !(fl & FL_LAST);
    if (*unres || !(flags[e] & FL_FIRST)) return 0ull;
    return (1ull << 32) | (unsigned long long)(t.w + ((fl & FL_KEEP) ? 1u : 0u) + ((fl & FL_APP) ? 1u : 0u));
}

__global__ __launch_bounds__(FB) void fp_reach_count_kernel(const uint4 *__restrict__ st, const uint8_t *__restrict__ flags, uint32_t n,
                                                           unsigned long long *__restrict__ block_sums, unsigned long long *unresolved)
{
    __shared__ unsigned long long wsum[FB / 64];
    const int64_t e = (int64_t)blockIdx.x * FB + threadIdx.x;
    bool unres;
    const unsigned long long w = fp_reach_weight(st, flags, e, n, &unres);
    const unsigned long long u = __ballot(unres);
    if (u && (threadIdx.x & 63) == 0) atomicAdd(unresolved, (unsigned long long)__popcll(u));
    const unsigned long long t = fp_block_sum(w, wsum);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = t;
}

// rinfo, at the compact index of a reach's LAST cell: x the reach's number, y the offset of its vertices, z the kept cells in front of
// the last cell, w the compact index of its first cell
__global__ __launch_bounds__(FB) void fp_reach_emit_kernel(const uint4 *__restrict__ st, const uint8_t *__restrict__ flags, uint32_t n,
                                                          const unsigned long long *__restrict__ block_offsets, int64_t nreach, int64_t nvert,
                                                          uint4 *__restrict__ rinfo, int64_t *__restrict__ reach_offsets)
{
    __shared__ unsigned long long wsum[FB / 64];
    const int64_t e = (int64_t)blockIdx.x * FB + threadIdx.x;
    bool unres;
    const unsigned long long w = fp_reach_weight(st, flags, e, n, &unres);
    const unsigned long long at = block_offsets[blockIdx.x] + fp_block_prefix(w, wsum);
    if (w) {
        const uint32_t k = (uint32_t)(at >> 32), vo = (uint32_t)at;
        const uint4 t = st[e];
        rinfo[t.x] = make_uint4(k, vo, t.w, (uint32_t)e);
        if ((int64_t)k < nreach) reach_offsets[k] = (int64_t)vo;
    }
    if (e == 0) reach_offsets[nreach] = nvert;
}

__global__ __launch_bounds__(256) void fp_vertex_kernel(const uint4 *__restrict__ st, const uint8_t *__restrict__ flags, const int64_t *__restrict__ cell,
                                                       const uint8_t *__restrict__ cls, const uint4 *__restrict__ rinfo, FpGeom g, uint32_t n,
                                                       int64_t nvert, int2 *__restrict__ xy)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const unsigned f = flags[e];
    if (!(f & (FL_KEEP | FL_APP))) return;
    const uint4 t = st[e];
    if (!(flags[t.x] & FL_LAST)) return;        // on a cycle that nothing flows into
    const uint4 ri = rinfo[t.x];
    const int64_t c = cell[e];
    if (f & FL_KEEP) {
        const int64_t at = (int64_t)ri.y + (ri.z - t.w);
        const int64_t r = c / g.W;
        if (at < nvert) xy[at] = make_int2((int)(c - r * g.W), (int)r);
    }
    if (f & FL_APP) {                           // (a last cell: t.w is 0, the slot behind its own)
        const int64_t d = fp_down(g, c, cls[c] >> CL_CODE_SHIFT);
        const int64_t at = (int64_t)ri.y + ri.z + ((f & FL_KEEP) ? 1 : 0);
        const int64_t r = d / g.W;
        if (d >= 0 && at < nvert) xy[at] = make_int2((int)(d - r * g.W), (int)r);
    }
}

__global__ __launch_bounds__(256) void fp_record_kernel(const uint4 *__restrict__ st, const uint8_t *__restrict__ flags, const int64_t *__restrict__ cell,
                                                       const uint8_t *__restrict__ cls, const uint4 *__restrict__ rinfo,
                                                       const unsigned long long *__restrict__ bits, const uint32_t *__restrict__ wbase,
                                                       const uint8_t *__restrict__ fd, const double *__restrict__ acc, const int32_t *__restrict__ lab,
                                                       FpGeom g, double thr, uint32_t n, int64_t nreach, mhip_reach_record *__restrict__ rec)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n || !(flags[e] & FL_FIRST)) return;
    const uint4 t = st[e];
    const unsigned fl = flags[t.x];
    if (!(fl & FL_LAST)) return;                // (a first cell always reaches a last one)
    const uint4 ri = rinfo[t.x];
    if ((int64_t)ri.x >= nreach) return;
    const int64_t c0 = cell[e], ck = cell[t.x];
    const unsigned kind = (fl >> FL_KIND_SHIFT) & 7u, codek = cls[ck] >> CL_CODE_SHIFT;
    const bool app = (fl & FL_APP) != 0u;
    const int64_t d = (kind == 0u || kind == 3u || kind == 4u) ? fp_down(g, ck, codek) : -1;
    mhip_reach_record out;
    out.first_cell = c0;
    out.last_cell = ck;
    out.end_cell = d;
    out.up_cells = acc[c0];
    out.down_cells = acc[ck];
    out.n_orth = (int32_t)(t.y + (app && !(codek & 1u) ? 1u : 0u));
    out.n_diag = (int32_t)(t.z + (app && (codek & 1u) ? 1u : 0u));
    out.end_kind = (int32_t)kind;
    out.to_reach = -1;
    if (kind == 0u && d >= 0) {                 // d is a confluence: the number of its reach is held where that reach ends
        uint32_t j = fp_rank(bits, wbase, d);
        j = j < n ? j : n - 1u;
        out.to_reach = (int32_t)rinfo[st[j].x].x;
    }
    out.to_label = (kind == 3u && d >= 0 && lab) ? lab[d] : 0;
    int32_t from = 0;
    if (lab) {
        const int64_t r = c0 / g.W, col = c0 - r * g.W;
        double best = 0.0;
        for (int k = 0; k < 8; ++k) {
            const int64_t rr = r + dir_dr(k), cc = col + dir_dc(k);
            if (rr < 0 || rr >= g.H || cc < 0 || cc >= g.W) continue;
            const int64_t nb = rr * g.W + cc;
            if (fd[nb] != (uint8_t)((k + 4) & 7) || lab[nb] == 0) continue;
            const double a = acc[nb];
            if (a >= thr && (from == 0 || a > best)) {
                from = lab[nb];
                best = a;
            }
        }
    }
    out.from_label = from;
    out.order = 0;
    out.reserved = 0;
    rec[ri.x] = out;
}

// rc: the reach of every cell, k + 1 for the cells c0 .. ck of reach k, 0 for a cell that is no stream cell and for a
// stream cell on a cycle that nothing flows into.  Every cell is written.
// V cells a thread (V = 4: N is a multiple of four: one 4-byte load of the class bytes, one 16-byte store).
template <int V>
__global__ __launch_bounds__(256) void fp_reachcell_kernel(const uint8_t *__restrict__ cls, const unsigned long long *__restrict__ bits,
                                                          const uint32_t *__restrict__ wbase, const uint4 *__restrict__ st, const uint8_t *__restrict__ flags,
                                                          const uint4 *__restrict__ rinfo, int64_t N, uint32_t n, int64_t nreach, int32_t *__restrict__ rc)
{
    const int64_t c0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * V;
    if (c0 >= N) return;
    uint32_t cl4;
    if constexpr (V == 4) cl4 = *reinterpret_cast<const uint32_t *>(cls + c0);
    else cl4 = cls[c0];
    int32_t v[V];
#pragma unroll
    for (int e = 0; e < V; ++e) {
        v[e] = 0;
        if ((cl4 >> (8 * e)) & CL_STREAM) {
            uint32_t i = fp_rank(bits, wbase, c0 + e);
            i = i < n ? i : n - 1u;                 // (it is: the cell is a stream cell)
            const uint32_t t = st[i].x;             // (< n: a pointer is a compact index)
            if (t < n && (flags[t] & FL_LAST)) {
                const uint32_t k = rinfo[t].x;
                v[e] = (int64_t)k < nreach ? (int32_t)(k + 1u) : 0;
            }
        }
    }
    if constexpr (V == 4) *reinterpret_cast<int4 *>(rc + c0) = make_int4(v[0], v[1], v[2], v[3]);
    else rc[c0] = v[0];
}

}  // namespace

int flowpaths_check(int64_t H, int64_t W, double threshold)
{
    MH_ARG(H >= 1 && W >= 1 && W <= 0x7fffffff && H <= 0x7fffffff, "flowpaths: H, W in [1, 2**31 - 1]");
    MH_ARG(threshold >= 1.0 && threshold <= 1.7976931348623157e308, "flowpaths: the threshold must be finite and >= 1");      // (false for NaN)
    return MHIP_OK;
}

int flowpaths_dev(const uint8_t *d_fd, const double *d_acc, const int32_t *d_lab, int64_t H, int64_t W, double threshold, mhip_flowpaths *p, hipStream_t s,
                  int32_t *d_rc)
{
    FpGeom g;
    g.H = H; g.W = W; g.N = H * W;
    const int64_t nb = cdiv(g.N, FB), nw = cdiv(g.N, 64), nwb = cdiv(nw, FB);
    if (nb > 0x7fffffff) {
        set_error("flowpaths: %lld cells exceed the launch grid", (long long)g.N);
        return MHIP_ELIMIT;
    }
    // words the host reads: the stream cells, (reaches << 32) | vertices, the unresolved cells, a negative label, "round k moved a pointer"
    struct Words {
        unsigned long long cells, reaches, unresolved;
        unsigned int bad, pad, moved[FP_MAX_ROUNDS];
    } h;
    DevBuf d_words, d_cls, d_bits, d_bc, d_wbase;
    MH_TRY(d_words.alloc(sizeof(Words)));
    MH_HIP(hipMemsetAsync(d_words.p, 0, sizeof(Words), s));
    Words *dw = d_words.as<Words>();
    MH_TRY(d_cls.alloc((size_t)g.N));
    MH_TRY(d_bits.alloc(8 * (size_t)nw));
    MH_TRY(d_bc.alloc(4 * (size_t)nwb));
    unsigned long long *bits = d_bits.as<unsigned long long>();
    hipLaunchKernelGGL(fp_class_kernel, dim3((unsigned)nb), dim3(FB), 0, s, d_fd, d_acc, d_lab, g, threshold, d_cls.as<uint8_t>(), bits, &dw->bad);
    hipLaunchKernelGGL(fp_wcount_kernel, dim3((unsigned)nwb), dim3(FB), 0, s, bits, nw, d_bc.as<uint32_t>());
    hipLaunchKernelGGL(fp_scan_kernel<uint32_t>, dim3(1), dim3(1024), 0, s, d_bc.as<uint32_t>(), nwb, &dw->cells);
    MH_HIP(hipGetLastError());
    MH_HIP(hipMemcpyAsync(&h, d_words.p, sizeof(Words), hipMemcpyDeviceToHost, s));
    MH_HIP(stream_sync(s));
    if (h.bad) {
        set_error("invalid argument: flowpaths: a negative label");
        return MHIP_EINVAL;
    }
    if (h.cells > 0x7fffffffull) {
        set_error("flowpaths: %llu stream cells exceed 2**31 - 1", h.cells);
        return MHIP_ELIMIT;
    }
    p->nreach = p->nvert = p->unresolved = 0;
    const uint32_t n = (uint32_t)h.cells;
    if (n == 0) {                    // an empty mask: no reach, and the fetch writes the one offset itself
        if (d_rc) {
            MH_HIP(hipMemsetAsync(d_rc, 0, 4 * (size_t)g.N, s));
            MH_HIP(stream_sync(s));
        }
        return MHIP_OK;
    }
    const int64_t neb = cdiv((int64_t)n, FB);
    const unsigned ge = (unsigned)cdiv((int64_t)n, 256), gc = (unsigned)cdiv(g.N, 256);
    if (cdiv(g.N, 256) > 0x7fffffff) {
        set_error("flowpaths: %lld cells exceed the launch grid", (long long)g.N);
        return MHIP_ELIMIT;
    }
    DevBuf d_cell, d_flags, d_st[2], d_bs, d_rinfo;
    MH_TRY(d_wbase.alloc(4 * (size_t)nw));
    MH_TRY(d_cell.alloc(8 * (size_t)n));
    MH_TRY(d_flags.alloc((size_t)n));
    MH_TRY(d_st[0].alloc(16 * (size_t)n));
    MH_TRY(d_st[1].alloc(16 * (size_t)n));
    hipLaunchKernelGGL(fp_wbase_kernel, dim3((unsigned)nwb), dim3(FB), 0, s, bits, nw, d_bc.as<uint32_t>(), d_wbase.as<uint32_t>());
    hipLaunchKernelGGL(fp_compact_kernel, dim3(gc), dim3(256), 0, s, d_cls.as<uint8_t>(), d_lab, g, bits, d_wbase.as<uint32_t>(), n, d_cell.as<int64_t>(),
                       d_flags.as<uint8_t>(), d_st[0].as<uint4>());
    // ceil(log2(n)) rounds close every window (a chain has at most n - 1 steps), one more sees that nothing moves
    int cap = 1;
    while (cap <= 32 && (1ull << (cap - 1)) < (unsigned long long)n) ++cap;
    int cur = 0, round = 0;
    while (round < cap) {
        const int upto = round + FP_CHECK_EVERY < cap ? round + FP_CHECK_EVERY : cap;
        for (; round < upto; ++round, cur ^= 1)
            hipLaunchKernelGGL(fp_jump_kernel, dim3(ge), dim3(256), 0, s, d_st[cur].as<uint4>(), d_st[cur ^ 1].as<uint4>(), n, &dw->moved[round]);
        MH_HIP(hipGetLastError());
        unsigned int moved = 0;
        MH_HIP(hipMemcpyAsync(&moved, &dw->moved[round - 1], 4, hipMemcpyDeviceToHost, s));
        MH_HIP(stream_sync(s));
        if (!moved) break;
    }
    const uint4 *st = d_st[cur].as<uint4>();
    MH_TRY(d_bs.alloc(8 * (size_t)neb));
    hipLaunchKernelGGL(fp_reach_count_kernel, dim3((unsigned)neb), dim3(FB), 0, s, st, d_flags.as<uint8_t>(), n, d_bs.as<unsigned long long>(), &dw->unresolved);
    hipLaunchKernelGGL(fp_scan_kernel<unsigned long long>, dim3(1), dim3(1024), 0, s, d_bs.as<unsigned long long>(), neb, &dw->reaches);
    MH_HIP(hipGetLastError());
    MH_HIP(hipMemcpyAsync(&h, d_words.p, 24, hipMemcpyDeviceToHost, s));
    MH_HIP(stream_sync(s));
    const int64_t nr = (int64_t)(h.reaches >> 32), nv = (int64_t)(h.reaches & 0xffffffffull);
    p->unresolved = (int64_t)h.unresolved;
    if (nr == 0) {                   // every stream cell lies on a cycle that nothing flows into
        if (d_rc) {
            MH_HIP(hipMemsetAsync(d_rc, 0, 4 * (size_t)g.N, s));
            MH_HIP(stream_sync(s));
        }
        return MHIP_OK;
    }
    MH_TRY(d_rinfo.alloc(16 * (size_t)n));
    MH_TRY(p->xy.alloc(8 * (size_t)nv));
    MH_TRY(p->reach_offsets.alloc(8 * (size_t)(nr + 1)));
    MH_TRY(p->records.alloc(sizeof(mhip_reach_record) * (size_t)nr));
    hipLaunchKernelGGL(fp_reach_emit_kernel, dim3((unsigned)neb), dim3(FB), 0, s, st, d_flags.as<uint8_t>(), n, d_bs.as<unsigned long long>(), nr, nv,
                       d_rinfo.as<uint4>(), p->reach_offsets.as<int64_t>());
    hipLaunchKernelGGL(fp_vertex_kernel, dim3(ge), dim3(256), 0, s, st, d_flags.as<uint8_t>(), d_cell.as<int64_t>(), d_cls.as<uint8_t>(), d_rinfo.as<uint4>(),
                       g, n, nv, p->xy.as<int2>());
    hipLaunchKernelGGL(fp_record_kernel, dim3(ge), dim3(256), 0, s, st, d_flags.as<uint8_t>(), d_cell.as<int64_t>(), d_cls.as<uint8_t>(), d_rinfo.as<uint4>(),
                       bits, d_wbase.as<uint32_t>(), d_fd, d_acc, d_lab, g, threshold, n, nr, p->records.as<mhip_reach_record>());
    if (d_rc) {
        if (g.N % 4 == 0 && ((uintptr_t)d_rc % 16 == 0) && ((uintptr_t)d_cls.p % 4 == 0))
            hipLaunchKernelGGL(fp_reachcell_kernel<4>, dim3((unsigned)cdiv(g.N / 4, 256)), dim3(256), 0, s, d_cls.as<uint8_t>(), bits, d_wbase.as<uint32_t>(), st,
                               d_flags.as<uint8_t>(), d_rinfo.as<uint4>(), g.N, n, nr, d_rc);
        else
            hipLaunchKernelGGL(fp_reachcell_kernel<1>, dim3(gc), dim3(256), 0, s, d_cls.as<uint8_t>(), bits, d_wbase.as<uint32_t>(), st, d_flags.as<uint8_t>(),
                               d_rinfo.as<uint4>(), g.N, n, nr, d_rc);
    }
    MH_HIP(hipGetLastError());
    MH_HIP(stream_sync(s));      // (the work buffers may go)
    p->nreach = nr;
    p->nvert = nv;
    return MHIP_OK;
}

// the three buffers of a handle to the caller's arrays: copies on the null stream of the handle's device, one synchronisation; then the
// Strahler orders, one pass of Kahn's algorithm over to_reach: a reach is freed when all that end at its first cell are
int flowpaths_fetch_dev(const mhip_flowpaths *p, int32_t *xy, int64_t *reach_offsets, mhip_reach_record *records)
{
    if (p->nreach == 0) {
        reach_offsets[0] = 0;
        return MHIP_OK;
    }
    MH_HIP(hipSetDevice(p->device));
    hipStream_t s = 0;
    const int64_t nr = p->nreach;
    MH_HIP(hipMemcpyAsync(xy, p->xy.p, 8 * (size_t)p->nvert, hipMemcpyDeviceToHost, s));
    MH_HIP(hipMemcpyAsync(reach_offsets, p->reach_offsets.p, 8 * ((size_t)nr + 1), hipMemcpyDeviceToHost, s));
    MH_HIP(hipMemcpyAsync(records, p->records.p, sizeof(mhip_reach_record) * (size_t)nr, hipMemcpyDeviceToHost, s));
    MH_HIP(stream_sync(s));
    try {
        std::vector<int32_t> pending((size_t)nr, 0), top((size_t)nr, 0), ntop((size_t)nr, 0), queue;
        queue.reserve((size_t)nr);
        for (int64_t k = 0; k < nr; ++k) {
            const int32_t t = records[k].to_reach;
            if (t >= 0 && t < nr) ++pending[(size_t)t];
        }
        for (int64_t k = 0; k < nr; ++k)
            if (pending[(size_t)k] == 0) {      // nothing ends at its first cell: a head
                records[k].order = 1;
                queue.push_back((int32_t)k);
            }
        for (size_t q = 0; q < queue.size(); ++q) {
            const int32_t k = queue[q], o = records[k].order, t = records[k].to_reach;
            if (t < 0 || t >= nr) continue;
            if (o > top[(size_t)t]) {
                top[(size_t)t] = o;
                ntop[(size_t)t] = 1;
            } else if (o == top[(size_t)t])
                ++ntop[(size_t)t];
            if (--pending[(size_t)t] == 0) {
                records[t].order = top[(size_t)t] + (ntop[(size_t)t] >= 2 ? 1 : 0);
                queue.push_back(t);
            }
        }
    } catch (const std::bad_alloc &) {
        set_error("flowpaths: out of host memory");
        return MHIP_EHIP;
    }
    return MHIP_OK;
}

}  // namespace mh
