// zones.hip -- object exposure: polygons to a zone raster, statistics of a float32 raster per zone (gfx950).
//
// No reference counterpart; tests/_zones.py is the definition.  Vertices are (x, y) in cell coordinates, the centre of cell (r, c) is
// (c + 0.5, r + 0.5); all rings of one zone id form one object.  An edge is oriented so that y0 < y1 and is active on row r when
// y0 <= r + 0.5 < y1; its crossing there is
//   xc = x0 + (yc - y0) * (x1 - x0) / (y1 - y0),  yc = r + 0.5      (float64, one rounding per operation, in this order)
//   cf = the smallest integer c with c + 0.5 >= xc
// and cell (r, c) is inside zone z when the number of z's crossings on row r with cf <= c is odd; the raster holds the largest such z.
// A SCANLINE is a (zone, row) pair of the zone's row range inside the raster; its crossings share a bucket.
//   host                the checks, the rows of every edge clipped to the raster, the prefix over the edges' crossings, the zones' row
//                       ranges and -- by a difference array over the scanlines -- the buckets' offsets
//   zone_cross_kernel   one thread per crossing (edge by bisection): cf, clipped to [0, W], into its scanline's bucket
//   zone_fill_kernel    one thread per crossing: its rank in the bucket and the next larger cf, by a walk over the bucket (k * k steps
//                       for a scanline of k crossings); an even rank opens the span [cf, next): atomicMax(zone) into the zeroed raster,
//                       short spans by the thread, long ones by the wavefront together.  Crossings of equal cf open empty spans.
//   zone_grow_kernel    a cell of zone 0 takes the largest zone of its 8 neighbours; into a second buffer
//   zone_stats_kernel   32 x 256 tiles as label_ops.hip / wetat.hip: runs of equal zone folded in registers, a table per tile in LDS,
//                       one global atomic per (zone, tile) and field; a run without a slot goes to the global atomics itself
// The cost is crossings (times the crossings of their scanline) + covered cells + H * W, never polygons x cells.
#include <algorithm>
#include <cmath>
#include <vector>

#include "common.hpp"

namespace mh {
namespace {

constexpr double ZONE_COORD_MAX = 536870912.0;      // 2**29
constexpr int ZONE_SHORT_SPAN = 32;                 // spans up to this many cells are written by their own thread

struct ZoneEdge {      // an oriented edge on the device, its first row inside the raster, and scanline = sbase + row
    double x0, y0, x1, y1;
    int64_t sbase;
    int32_t zone, rlo;
};

// the smallest integer c with c + 0.5 >= x: ceil(x - 0.5), put right by the comparison itself (x - 0.5 may round)
__host__ __device__ inline int64_t first_centre(double x)
{
    int64_t c = (int64_t)ceil(x - 0.5);
    if ((double)(c - 1) + 0.5 >= x) --c;
    else if ((double)c + 0.5 < x) ++c;
    return c;
}

// thread x is crossing x: edge E[e] with P[e] <= x < P[e + 1], row rlo + (x - P[e])
__global__ __launch_bounds__(256) void zone_cross_kernel(const ZoneEdge *__restrict__ E, const int64_t *__restrict__ P, int64_t nedge, int64_t W,
                                                        const uint32_t *__restrict__ B, uint32_t *cursor, int32_t *__restrict__ cf_out,
                                                        uint32_t *__restrict__ sl_out, int32_t *sl_row, int32_t *sl_zone)
{
    const int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= P[nedge]) return;
    int64_t lo = 0, hi = nedge;      // the last edge whose prefix is <= x (it is not empty: x < P[nedge])
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (P[mid] <= x) lo = mid;
        else hi = mid;
    }
    const ZoneEdge g = E[lo];
    const int64_t r = (int64_t)g.rlo + (x - P[lo]);
    const double yc = (double)r + 0.5;
    const double xc = __dadd_rn(g.x0, __ddiv_rn(__dmul_rn(__dsub_rn(yc, g.y0), __dsub_rn(g.x1, g.x0)), __dsub_rn(g.y1, g.y0)));
    int64_t cf = first_centre(xc);
    cf = cf < 0 ? 0 : cf > W ? W : cf;      // left of the raster: counted by every column; right of it: by none
    const int64_t sl = g.sbase + r;
    const uint32_t at = B[sl] + atomicAdd(&cursor[sl], 1u);
    cf_out[at] = (int32_t)cf;
    sl_out[at] = (uint32_t)sl;
    sl_row[sl] = (int32_t)r;               // (every crossing of a scanline writes the same two words)
    sl_zone[sl] = g.zone;
}

__device__ __forceinline__ void zone_put(int32_t *p, int32_t z)
{
    // a look first: a stale value is never above the current one (the raster only rises), so a cell already at z or above needs no atomic
    if (*p < z) atomicMax(p, z);
}

__global__ __launch_bounds__(256) void zone_fill_kernel(const int32_t *__restrict__ cf, const uint32_t *__restrict__ sl_of, const uint32_t *__restrict__ B,
                                                       const int32_t *__restrict__ sl_row, const int32_t *__restrict__ sl_zone, int64_t total,
                                                       int64_t W, int32_t *zones)
{
    const int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int32_t c0 = 0, c1 = 0, row = 0, z = 0;      // the span [c0, c1) of row `row` this thread opens (empty: none)
    if (x < total) {
        const uint32_t sl = sl_of[x];
        const uint32_t b0 = B[sl], b1 = B[sl + 1];
        const int32_t a = cf[x];
        uint32_t rank = 0;
        int32_t next = (int32_t)W;               // (without a partner the row is inside to its end: cannot happen with closed rings)
        for (uint32_t j = b0; j < b1; ++j) {
            const int32_t v = cf[j];
            const bool before = v < a || (v == a && (int64_t)j < x);
            rank += before ? 1u : 0u;
            if (!before && (int64_t)j != x) next = v < next ? v : next;
        }
        if (!(rank & 1u)) {
            c0 = a;
            c1 = next;
            row = sl_row[sl];
            z = sl_zone[sl];
        }
    }
    const int32_t len = c1 - c0;
    if (len > 0 && len <= ZONE_SHORT_SPAN) {
        int32_t *p = zones + (int64_t)row * W;
        for (int32_t c = c0; c < c1; ++c) zone_put(p + c, z);
    }
    // the long spans of the wavefront, one after the other, 64 cells at a time
    unsigned long long todo = __ballot(len > ZONE_SHORT_SPAN);
    const int lane = (int)(threadIdx.x & 63u);
    while (todo) {
        const int lead = __ffsll((long long)todo) - 1;
        const int32_t s0 = __shfl(c0, lead), s1 = __shfl(c1, lead), sr = __shfl(row, lead), sz = __shfl(z, lead);
        int32_t *p = zones + (int64_t)sr * W;
        for (int64_t c = (int64_t)s0 + lane; c < s1; c += 64) zone_put(p + c, sz);
        todo &= todo - 1;
    }
}

__global__ __launch_bounds__(256) void zone_grow_kernel(const int32_t *__restrict__ in, int64_t H, int64_t W, int32_t *__restrict__ out)
{
    const int64_t n = H * W, step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
        int32_t z = in[i];
        if (z == 0) {
            const int64_t r = i / W, c = i - r * W;
#pragma unroll
            for (int dr = -1; dr <= 1; ++dr)
#pragma unroll
                for (int dc = -1; dc <= 1; ++dc) {
                    const int64_t rr = r + dr, cc = c + dc;
                    if (rr < 0 || rr >= H || cc < 0 || cc >= W) continue;
                    const int32_t v = in[rr * W + cc];
                    z = v > z ? v : z;
                }
        }
        out[i] = z;
    }
}

// ---- statistics ------------------------------------------------------------------------------------------------------------------
// The accumulators of a zone: the largest non-NaN value as its monotone key (f32_key), the smallest value > 0 as its bit pattern
// (positive floats order as their patterns), the cells and the cells > 0.  Float tests are made on the bits: no mode of the
// arithmetic (denormals) has a say.
constexpr uint32_t ZKEY_NEG_INF = 0x007fffffu;      // f32_key(-inf)
constexpr uint32_t ZBITS_POS_INF = 0x7f800000u;
constexpr int ZONE_SLOTS = 512;                     // LDS: 5 words a slot, 10 KB

__device__ __forceinline__ uint32_t zone_key(uint32_t u) { return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }

__global__ __launch_bounds__(256) void zone_stats_init_kernel(int64_t nzone, uint32_t *__restrict__ gmax, uint32_t *__restrict__ gmin,
                                                             unsigned long long *__restrict__ gcells, unsigned long long *__restrict__ gpos,
                                                             unsigned int *bad)
{
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= nzone; i += step) {
        gmax[i] = ZKEY_NEG_INF;
        gmin[i] = ZBITS_POS_INF;
        gcells[i] = 0ull;
        gpos[i] = 0ull;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *bad = 0u;
}

template <int V>      // 4 or 1
__global__ __launch_bounds__(256) void zone_stats_kernel(const float *__restrict__ data, const int32_t *__restrict__ zones, TileGeom g, int64_t nzone,
                                                        uint32_t *gmax, uint32_t *gmin, unsigned long long *gcells, unsigned long long *gpos,
                                                        unsigned int *bad)
{
    constexpr int TS = ZONE_SLOTS;
    __shared__ int keys[TS];
    __shared__ uint32_t tmax[TS], tmin[TS], tcells[TS], tpos[TS];
    constexpr int TPR = 256 / V;      // threads per tile row; V rows per pass of the workgroup
    const int tx = threadIdx.x % TPR, ty = threadIdx.x / TPR;
    unsigned int any_bad = 0;
    const int64_t ntiles = g.ntr * g.ntc;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        for (int k = threadIdx.x; k < TS; k += 256) {
            keys[k] = -1;
            tmax[k] = ZKEY_NEG_INF;
            tmin[k] = ZBITS_POS_INF;
            tcells[k] = 0u;
            tpos[k] = 0u;
        }
        __syncthreads();
        const int64_t tr = tile / g.ntc, tc = tile - tr * g.ntc;
        const int64_t col = tc * 256 + (int64_t)tx * V;
        int32_t cz = 0;      // the run: its zone and what its cells add up to (a thread sees at most TR * V cells of a tile)
        uint32_t cmax = ZKEY_NEG_INF, cmin = ZBITS_POS_INF, ccells = 0u, cpos = 0u;
        auto end_run = [&]() {
            if (!ccells) return;
            const int h = table_slot<TS>(keys, cz);
            if (h >= 0) {
                atomicAdd(&tcells[h], ccells);
                if (cmax != ZKEY_NEG_INF) atomicMax(&tmax[h], cmax);
                if (cpos) {
                    atomicAdd(&tpos[h], cpos);
                    atomicMin(&tmin[h], cmin);
                }
            } else {
                atomicAdd(&gcells[cz], (unsigned long long)ccells);
                if (cmax != ZKEY_NEG_INF) atomicMax(&gmax[cz], cmax);
                if (cpos) {
                    atomicAdd(&gpos[cz], (unsigned long long)cpos);
                    atomicMin(&gmin[cz], cmin);
                }
            }
        };
        for (int r = ty; r < TR; r += V) {
            const int64_t i = (tr * TR + r) * g.W + col;
            if (!(col < g.W && i < g.n)) continue;       // (V = 4: W is a multiple of four, the whole vector is inside)
            int32_t zv[V];
            uint32_t dv[V];
            if constexpr (V == 4) {
                const int4 z4 = *reinterpret_cast<const int4 *>(zones + i);
                const uint4 d4 = *reinterpret_cast<const uint4 *>(data + i);
                zv[0] = z4.x; zv[1] = z4.y; zv[2] = z4.z; zv[3] = z4.w;
                dv[0] = d4.x; dv[1] = d4.y; dv[2] = d4.z; dv[3] = d4.w;
            } else {
                zv[0] = zones[i];
                dv[0] = reinterpret_cast<const uint32_t *>(data)[i];
            }
#pragma unroll
            for (int e = 0; e < V; ++e) {
                int32_t z = zv[e];
                if (z < 0 || z > nzone) {
                    any_bad = 1;
                    z = 0;
                }
                if (z != cz) {
                    end_run();
                    cz = z;
                    cmax = ZKEY_NEG_INF;
                    cmin = ZBITS_POS_INF;
                    ccells = 0u;
                    cpos = 0u;
                }
                const uint32_t u = dv[e];
                const bool nan = (u & 0x7fffffffu) > ZBITS_POS_INF;
                const bool pos = u != 0u && u <= ZBITS_POS_INF;      // > 0: sign clear, not zero, not a NaN
                const uint32_t k = zone_key(u);
                ++ccells;
                cmax = (!nan && k > cmax) ? k : cmax;
                cpos += pos ? 1u : 0u;
                cmin = (pos && u < cmin) ? u : cmin;
            }
        }
        end_run();
        __syncthreads();
        for (int sl = threadIdx.x; sl < TS; sl += 256) {
            const int key = keys[sl];
            if (key < 0) continue;
            atomicAdd(&gcells[key], (unsigned long long)tcells[sl]);
            if (tmax[sl] != ZKEY_NEG_INF) atomicMax(&gmax[key], tmax[sl]);
            if (tpos[sl]) {
                atomicAdd(&gpos[key], (unsigned long long)tpos[sl]);
                atomicMin(&gmin[key], tmin[sl]);
            }
        }
        __syncthreads();
    }
    if (any_bad) atomicOr(bad, 1u);
}

__global__ __launch_bounds__(256) void zone_stats_finish_kernel(int64_t nzone, const uint32_t *__restrict__ gmax, const uint32_t *__restrict__ gmin,
                                                               const unsigned long long *__restrict__ gcells,
                                                               const unsigned long long *__restrict__ gpos, mhip_zone_record *__restrict__ rec)
{
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= nzone; i += step) {
        mhip_zone_record r;
        r.vmax = __dadd_rn((double)key_f32(gmax[i]), 0.0);      // (a zero maximum is +0.0)
        r.vmin_pos = (double)__uint_as_float(gmin[i]);
        r.cells = (int64_t)gcells[i];
        r.pos = (int64_t)gpos[i];
        rec[i] = r;
    }
}

inline unsigned flat_grid(int64_t n) { return (unsigned)(cdiv(n, 256) < 2048 ? std::max<int64_t>(cdiv(n, 256), 1) : 2048); }

}  // namespace

int zones_check(int64_t H, int64_t W, int64_t nvert, const double *xy, int64_t nring, const int64_t *ring_offsets, const int32_t *ring_zone,
                int64_t nzone, int grow)
{
    MH_ARG(H >= 1 && W >= 1 && W <= 0x7fffffff && H <= 0x7fffffff, "rasterize_zones: H, W in [1, 2**31 - 1]");
    MH_ARG(nvert >= 0 && nring >= 0 && nzone >= 0, "rasterize_zones: negative count");
    MH_ARG(nzone <= 0x7fffffff, "rasterize_zones: more than 2**31 - 1 zones");
    MH_ARG(grow == 0 || grow == 1, "rasterize_zones: grow must be 0 or 1");
    MH_ARG((nvert == 0 || xy) && ring_offsets && (nring == 0 || ring_zone), "rasterize_zones(H, W, nvert, xy, nring, ring_offsets, ring_zone, nzone, grow, out)");
    MH_ARG(ring_offsets[0] == 0 && ring_offsets[nring] == nvert, "rasterize_zones: ring_offsets must start at 0 and end at nvert");
    for (int64_t i = 0; i < nring; ++i) {
        MH_ARG(ring_offsets[i + 1] >= ring_offsets[i], "rasterize_zones: ring_offsets decrease");
        MH_ARG(ring_offsets[i + 1] - ring_offsets[i] >= 3, "rasterize_zones: a ring of fewer than 3 vertices");
        MH_ARG(ring_zone[i] >= 1 && ring_zone[i] <= nzone, "rasterize_zones: a zone id outside [1, nzone]");
    }
    for (int64_t i = 0; i < 2 * nvert; ++i) MH_ARG(std::fabs(xy[i]) <= ZONE_COORD_MAX, "rasterize_zones: a coordinate that is not finite or beyond 2**29");
    return MHIP_OK;
}

int zones_rasterize_dev(int32_t *d_out, int64_t H, int64_t W, int64_t nvert, const double *xy, int64_t nring, const int64_t *ring_offsets,
                        const int32_t *ring_zone, int64_t nzone, int grow, hipStream_t s)
{
    // edges, oriented, with the rows they are active on inside the raster; the row range of every zone
    std::vector<ZoneEdge> he;
    std::vector<int64_t> hp(1, 0);
    std::vector<int64_t> zlo((size_t)nzone + 1, H), zhi((size_t)nzone + 1, -1);      // rows [zlo, zhi] of a zone's scanlines
    he.reserve((size_t)nvert);
    hp.reserve((size_t)nvert + 1);
    for (int64_t k = 0; k < nring; ++k) {
        const int64_t a = ring_offsets[k], b = ring_offsets[k + 1];
        const int32_t z = ring_zone[k];
        for (int64_t i = a; i < b; ++i) {
            const int64_t j = i + 1 < b ? i + 1 : a;
            double x0 = xy[2 * i], y0 = xy[2 * i + 1], x1 = xy[2 * j], y1 = xy[2 * j + 1];
            if (y0 == y1) continue;
            if (y0 > y1) {
                std::swap(x0, x1);
                std::swap(y0, y1);
            }
            const int64_t rlo = std::max<int64_t>(first_centre(y0), 0), rhi = std::min<int64_t>(first_centre(y1), H);      // y0 <= r + 0.5 < y1
            if (rhi <= rlo) continue;
            he.push_back(ZoneEdge{x0, y0, x1, y1, 0, z, (int32_t)rlo});
            hp.push_back(hp.back() + (rhi - rlo));
            zlo[(size_t)z] = std::min(zlo[(size_t)z], rlo);
            zhi[(size_t)z] = std::max(zhi[(size_t)z], rhi - 1);
        }
    }
    const int64_t nedge = (int64_t)he.size(), total = hp.back();
    // scanlines: zone-major, a zone's rows [zlo, zhi]
    std::vector<int64_t> zoff((size_t)nzone + 2, 0);
    for (int64_t z = 1; z <= nzone; ++z) zoff[(size_t)z + 1] = zoff[(size_t)z] + (zhi[(size_t)z] >= zlo[(size_t)z] ? zhi[(size_t)z] - zlo[(size_t)z] + 1 : 0);
    const int64_t nscan = zoff[(size_t)nzone + 1];
    if (total > 0x7fffffff || nscan > 0x7fffffff) {
        set_error("rasterize_zones: %lld crossings on %lld scanlines exceed 2**31 - 1", (long long)total, (long long)nscan);
        return MHIP_ELIMIT;
    }
    const size_t n = (size_t)(H * W);
    DevBuf d_tmp;
    int32_t *d_ras = d_out;
    if (grow) {
        MH_TRY(d_tmp.alloc(4 * n));
        d_ras = d_tmp.as<int32_t>();
    }
    MH_HIP(hipMemsetAsync(d_ras, 0, 4 * n, s));
    DevBuf d_e, d_p, d_b, d_cur, d_cf, d_sl, d_row, d_zone;
    if (total > 0) {
        // the crossings of every scanline by a difference array over the edges' row intervals, then the buckets' offsets
        std::vector<uint32_t> hb((size_t)nscan + 1, 0u);      // (+1 / -1 modulo 2**32: the running sum is a count again)
        for (int64_t e = 0; e < nedge; ++e) {
            ZoneEdge &g = he[(size_t)e];
            g.sbase = zoff[(size_t)g.zone] - zlo[(size_t)g.zone];
            const int64_t cnt = hp[(size_t)e + 1] - hp[(size_t)e];
            hb[(size_t)(g.sbase + g.rlo)] += 1u;
            hb[(size_t)(g.sbase + g.rlo + cnt)] -= 1u;      // (entry nscan takes the ends at the last scanline)
        }
        uint32_t active = 0u, at = 0u;
        for (int64_t k = 0; k < nscan; ++k) {
            active += hb[(size_t)k];
            hb[(size_t)k] = at;
            at += active;
        }
        hb[(size_t)nscan] = at;      // == total
        MH_TRY(upload(d_e, he.data(), sizeof(ZoneEdge) * (size_t)nedge, s));
        MH_TRY(upload(d_p, hp.data(), 8 * ((size_t)nedge + 1), s));
        MH_TRY(upload(d_b, hb.data(), 4 * ((size_t)nscan + 1), s));
        MH_TRY(d_cur.alloc(4 * (size_t)nscan));
        MH_TRY(d_cf.alloc(4 * (size_t)total));
        MH_TRY(d_sl.alloc(4 * (size_t)total));
        MH_TRY(d_row.alloc(4 * (size_t)nscan));
        MH_TRY(d_zone.alloc(4 * (size_t)nscan));
        MH_HIP(hipMemsetAsync(d_cur.p, 0, 4 * (size_t)nscan, s));
        const unsigned gr = (unsigned)cdiv(total, 256);
        hipLaunchKernelGGL(zone_cross_kernel, dim3(gr), dim3(256), 0, s, d_e.as<ZoneEdge>(), d_p.as<int64_t>(), nedge, W, d_b.as<uint32_t>(),
                           d_cur.as<uint32_t>(), d_cf.as<int32_t>(), d_sl.as<uint32_t>(), d_row.as<int32_t>(), d_zone.as<int32_t>());
        hipLaunchKernelGGL(zone_fill_kernel, dim3(gr), dim3(256), 0, s, d_cf.as<int32_t>(), d_sl.as<uint32_t>(), d_b.as<uint32_t>(), d_row.as<int32_t>(),
                           d_zone.as<int32_t>(), total, W, d_ras);
    }
    if (grow) hipLaunchKernelGGL(zone_grow_kernel, dim3(flat_grid((int64_t)n)), dim3(256), 0, s, d_ras, H, W, d_out);
    MH_HIP(hipGetLastError());
    MH_HIP(stream_sync(s));      // (the host arrays and the buffers may go)
    return MHIP_OK;
}

int zone_stats_dev(const float *d_data, const int32_t *d_zones, int64_t n, int64_t W, int64_t nzone, mhip_zone_record *d_rec, hipStream_t s)
{
    DevBuf acc, bad;
    const size_t nz = (size_t)nzone + 1;
    MH_TRY(acc.alloc(24 * nz));
    MH_TRY(bad.alloc(4));
    unsigned long long *gcells = acc.as<unsigned long long>(), *gpos = gcells + nz;      // (the 64-bit words first: aligned)
    uint32_t *gmax = reinterpret_cast<uint32_t *>(gpos + nz), *gmin = gmax + nz;
    hipLaunchKernelGGL(zone_stats_init_kernel, dim3(flat_grid((int64_t)nz)), dim3(256), 0, s, nzone, gmax, gmin, gcells, gpos, bad.as<unsigned int>());
    const TileGeom g = tile_geom(n, W);
    const bool vec = W > 0 && n % W == 0 && W % 4 == 0 && ((uintptr_t)d_data | (uintptr_t)d_zones) % 16 == 0;
    if (vec) hipLaunchKernelGGL(zone_stats_kernel<4>, dim3(tile_grid(g)), dim3(256), 0, s, d_data, d_zones, g, nzone, gmax, gmin, gcells, gpos, bad.as<unsigned int>());
    else hipLaunchKernelGGL(zone_stats_kernel<1>, dim3(tile_grid(g)), dim3(256), 0, s, d_data, d_zones, g, nzone, gmax, gmin, gcells, gpos, bad.as<unsigned int>());
    hipLaunchKernelGGL(zone_stats_finish_kernel, dim3(flat_grid((int64_t)nz)), dim3(256), 0, s, nzone, gmax, gmin, gcells, gpos, d_rec);
    MH_HIP(hipGetLastError());
    unsigned int h = 0;
    MH_HIP(hipMemcpyAsync(&h, bad.p, sizeof(h), hipMemcpyDeviceToHost, s));
    MH_HIP(stream_sync(s));      // (the accumulators go back to the pool)
    if (h) {
        set_error("zone_stats: zone outside [0, nzone]");
        return MHIP_EINVAL;
    }
    return MHIP_OK;
}

}  // namespace mh
