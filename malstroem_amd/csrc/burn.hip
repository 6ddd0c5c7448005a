// burn.hip -- DEM adaptations: lower the DEM along culvert lines, raise it along dike lines (gfx950).
//
// No reference counterpart; tests/_burn.py is the definition.  A line is a chain of segments between cell coordinates.  Segment
// (r0, c0) -> (r1, c1): n = max(|dr|, |dc|) steps along the major axis (the column when |dc| >= |dr|), step k = 0 .. n sits at
//   major = start + sign * k,  minor = start + sign * m(k),  m(k) = (2 * k * dmin + n) / (2 * n)  (integers; 0 when n = 0)
// and, 4-connected, a step k >= 1 with m(k) != m(k - 1) also owns the corner cell (major of k, minor of k - 1).  The level of a
// step is z0 * (1 - t) + z1 * t in float64, t = (koff + k) / ntotal along the whole line, rounded to float32 once; a NaN z0 / z1 is
// the DEM at the line's first / last vertex BEFORE any line of the call has written.  All lower lines write min(dem, z), then all
// raise lines max(dem, z): both are exact and commutative, so the result depends on no order and no schedule.
//   burn_ends_kernel   one thread per line: the levels at the ends, the status, the record
//   burn_steps_kernel  one thread per step (lower / raise): the cell in closed form, the atomic min / max, the cells of a line
// The host clips the steps of a segment to those whose major coordinate lies in the raster (one interval of k), sorts lower before
// raise and builds the exclusive prefix of the step counts; a thread finds its (segment, k) by bisection.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "common.hpp"

namespace mh {
namespace {

constexpr int32_t BURN_COORD_MAX = 1 << 29;
constexpr double BURN_F32_MAX = 3.4028234663852886e38;

struct BurnSeg {      // a segment on the device: the caller's fields and the first step inside the raster
    int32_t r0, c0, r1, c1, line, koff, klo, pad;
};
struct BurnLine {     // a line on the device: the caller's fields and its first / last vertex
    double z0, z1;
    int32_t fr, fc, lr, lc, ntotal, flags;
};

__global__ __launch_bounds__(256) void burn_ends_kernel(const float *__restrict__ dem, int64_t H, int64_t W, const BurnLine *__restrict__ L, int64_t nline,
                                                       double nodata, mhip_burn_result *__restrict__ res)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nline) return;
    const BurnLine l = L[i];
    double z0 = l.z0, z1 = l.z1;
    const bool s0 = z0 != z0, s1 = z1 != z1;      // to be sampled
    const bool in0 = l.fr >= 0 && l.fr < H && l.fc >= 0 && l.fc < W, in1 = l.lr >= 0 && l.lr < H && l.lc >= 0 && l.lc < W;
    int32_t st = 0;
    if ((s0 && !in0) || (s1 && !in1)) {
        st = 1;
    } else {
        if (s0) z0 = (double)dem[(int64_t)l.fr * W + l.fc];
        if (s1) z1 = (double)dem[(int64_t)l.lr * W + l.lc];
        // (an explicit level is finite and never compared with nodata)
        if ((s0 && (!(fabs(z0) <= BURN_F32_MAX) || z0 == nodata)) || (s1 && (!(fabs(z1) <= BURN_F32_MAX) || z1 == nodata))) st = 2;
    }
    mhip_burn_result r;
    r.z0 = st ? __builtin_nan("") : z0;
    r.z1 = st ? __builtin_nan("") : z1;
    r.cells = 0;
    r.status = st;
    r.pad = 0;
    res[i] = r;
}

// dem[i] = min(dem[i], z) (RAISE: max) on the bit patterns: floats >= +0 order as signed integers, floats <= -0 order backwards as
// unsigned integers, and every pattern of the first kind is below every pattern of the second as unsigned, above it as signed.
// Neither side is a NaN.
template <bool RAISE> __device__ __forceinline__ void burn_apply(float *p, float z)
{
    const int32_t zi = __float_as_int(z);
    if (!RAISE) {
        if (zi >= 0) atomicMin(reinterpret_cast<int *>(p), zi);
        else atomicMax(reinterpret_cast<unsigned int *>(p), (unsigned int)zi);
    } else {
        if (zi >= 0) atomicMax(reinterpret_cast<int *>(p), zi);
        else atomicMin(reinterpret_cast<unsigned int *>(p), (unsigned int)zi);
    }
}

// S, P: the `ns` segments of this mode and their ns + 1 prefix entries; thread x of the launch is step P[0] + x
template <bool RAISE>
__global__ __launch_bounds__(256) void burn_steps_kernel(float *dem, int64_t H, int64_t W, const BurnSeg *__restrict__ S, const int64_t *__restrict__ P,
                                                        int64_t ns, const BurnLine *__restrict__ L, mhip_burn_result *res)
{
    const int64_t x = P[0] + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int32_t line = -1;
    int ncell = 0;      // in-raster cells of this step (0 .. 2)
    if (x < P[ns]) {
        int64_t lo = 0, hi = ns;      // the last segment whose prefix is <= x (it is not empty: x < P[ns])
        while (hi - lo > 1) {
            const int64_t mid = (lo + hi) >> 1;
            if (P[mid] <= x) lo = mid;
            else hi = mid;
        }
        const BurnSeg g = S[lo];
        const BurnLine l = L[g.line];
        if (res[g.line].status == 0) {
            line = g.line;
            const int64_t k = (int64_t)g.klo + (x - P[lo]);
            const int64_t dr = (int64_t)g.r1 - g.r0, dc = (int64_t)g.c1 - g.c0;
            const int64_t adr = dr < 0 ? -dr : dr, adc = dc < 0 ? -dc : dc;
            const bool colmajor = adc >= adr;
            const int64_t n = colmajor ? adc : adr, dmin = colmajor ? adr : adc;
            int64_t m = 0, mprev = 0;
            if (n > 0) {
                const uint64_t num = 2ull * (uint64_t)k * (uint64_t)dmin + (uint64_t)n, den = 2ull * (uint64_t)n;
                const uint64_t q = num / den, rem = num - q * den;
                m = (int64_t)q;
                mprev = (k >= 1 && rem < 2ull * (uint64_t)dmin) ? m - 1 : m;      // m(k - 1): the numerator is 2 * dmin smaller
            }
            const int64_t sr = dr > 0 ? 1 : dr < 0 ? -1 : 0, sc = dc > 0 ? 1 : dc < 0 ? -1 : 0;
            const int64_t r = colmajor ? g.r0 + sr * m : g.r0 + sr * k, c = colmajor ? g.c0 + sc * k : g.c0 + sc * m;
            const int64_t rc = colmajor ? g.r0 + sr * mprev : r, cc = colmajor ? c : g.c0 + sc * mprev;      // the corner cell
            const bool corner = (l.flags & 2) && mprev != m;
            const double z0 = res[g.line].z0, z1 = res[g.line].z1;
            float z;
            if (l.ntotal > 0) {
                const double t = __ddiv_rn((double)(g.koff + k), (double)l.ntotal);
                z = (float)__dadd_rn(__dmul_rn(z0, __dsub_rn(1.0, t)), __dmul_rn(z1, t));
            } else {
                z = (float)(RAISE ? (z0 > z1 ? z0 : z1) : (z0 < z1 ? z0 : z1));
            }
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int64_t rr = e ? rc : r, cq = e ? cc : c;
                if ((e && !corner) || rr < 0 || rr >= H || cq < 0 || cq >= W) continue;
                ++ncell;
                float *p = dem + rr * W + cq;
                // a look first: a NaN cell stays (nobody ever writes a NaN), and a cell already beyond z needs no atomic (a stale
                // value is never beyond the current one: lower lines only lower, raise lines only raise)
                const float v = *p;
                if (v != v || (RAISE ? !(z > v) : !(z < v))) continue;
                burn_apply<RAISE>(p, z);
            }
        }
    }
    // the cells of a line: one 64-bit add per wavefront and line met in it
    unsigned long long todo = __ballot(ncell > 0);
    const int lane = (int)(threadIdx.x & 63u);
    while (todo) {
        const int lead = __ffsll((long long)todo) - 1;
        const int32_t cur = __shfl(line, lead);
        const bool mine = ncell > 0 && line == cur;
        const unsigned long long m1 = __ballot(mine), m2 = __ballot(mine && ncell == 2);
        if (lane == lead) atomicAdd(reinterpret_cast<unsigned long long *>(&res[cur].cells), (unsigned long long)(__popcll(m1) + __popcll(m2)));
        todo &= ~m1;
    }
}

// what every line's record is when there is no segment at all (the host's answer: nothing runs on the device)
void burn_results_without_segments(int64_t nline, const mhip_burn_line *lines, mhip_burn_result *results)
{
    for (int64_t i = 0; i < nline; ++i) {
        const bool sampled = std::isnan(lines[i].z0) || std::isnan(lines[i].z1);
        results[i].z0 = sampled ? std::nan("") : lines[i].z0;
        results[i].z1 = sampled ? std::nan("") : lines[i].z1;
        results[i].cells = 0;
        results[i].status = sampled ? 1 : 0;      // (no vertex to sample: outside)
        results[i].pad = 0;
    }
}

}  // namespace

int burn_check(int64_t nseg, const mhip_burn_segment *segs, int64_t nline, const mhip_burn_line *lines, const mhip_burn_result *results)
{
    MH_ARG(nseg >= 0 && nline >= 0, "burn_lines: negative count");
    MH_ARG((nseg == 0 || segs) && (nline == 0 || (lines && results)), "burn_lines(nseg, segments, nline, lines, nodata, results)");
    for (int64_t i = 0; i < nline; ++i) {
        const mhip_burn_line &l = lines[i];
        MH_ARG(l.flags >= 0 && l.flags <= 3, "burn_lines: flags of a line outside 0 .. 3");
        MH_ARG(l.ntotal >= 0, "burn_lines: ntotal of a line is negative");
        MH_ARG((std::isnan(l.z0) || std::fabs(l.z0) <= BURN_F32_MAX) && (std::isnan(l.z1) || std::fabs(l.z1) <= BURN_F32_MAX),
               "burn_lines: an explicit level is infinite or beyond the float32 range");
    }
    for (int64_t i = 0; i < nseg; ++i) {
        const mhip_burn_segment &g = segs[i];
        MH_ARG(g.line >= 0 && g.line < nline, "burn_lines: line index of a segment out of range");
        for (int32_t v : {g.r0, g.c0, g.r1, g.c1}) MH_ARG(v >= -BURN_COORD_MAX && v <= BURN_COORD_MAX, "burn_lines: a coordinate beyond 2**29");
        const int64_t dr = std::llabs((int64_t)g.r1 - g.r0), dc = std::llabs((int64_t)g.c1 - g.c0);
        MH_ARG(g.koff >= 0 && (int64_t)g.koff + std::max(dr, dc) <= (int64_t)lines[g.line].ntotal, "burn_lines: koff < 0 or koff + n > ntotal of the line");
    }
    return MHIP_OK;
}

int burn_lines_dev(float *d_dem, int64_t H, int64_t W, int64_t nseg, const mhip_burn_segment *segs, int64_t nline, const mhip_burn_line *lines,
                   double nodata, mhip_burn_result *results, hipStream_t s)
{
    if (nseg == 0) {
        burn_results_without_segments(nline, lines, results);
        return MHIP_OK;
    }
    // lines: the first vertex is the one of the segment with the smallest koff, the last vertex the one of the segment with the largest
    // koff + n (among equals -- segments of no length, which share their vertex in a connected line -- the earliest / the latest)
    std::vector<BurnLine> hl((size_t)nline);
    std::vector<int64_t> kfirst((size_t)nline, -1), klast((size_t)nline, -1);
    for (int64_t i = 0; i < nline; ++i) hl[(size_t)i] = BurnLine{lines[i].z0, lines[i].z1, -1, -1, -1, -1, lines[i].ntotal, lines[i].flags};
    // segments: lower before raise, each clipped to the steps whose major coordinate is inside
    std::vector<BurnSeg> hs((size_t)nseg);
    std::vector<int64_t> hp((size_t)nseg + 1);
    int64_t nlower = 0;
    for (int64_t i = 0; i < nseg; ++i) nlower += (lines[segs[i].line].flags & 1) ? 0 : 1;
    int64_t at[2] = {0, nlower};
    for (int64_t i = 0; i < nseg; ++i) {
        const mhip_burn_segment &g = segs[i];
        const int64_t dr = (int64_t)g.r1 - g.r0, dc = (int64_t)g.c1 - g.c0;
        const int64_t adr = std::llabs(dr), adc = std::llabs(dc);
        const bool colmajor = adc >= adr;
        const int64_t n = colmajor ? adc : adr, a = colmajor ? g.c0 : g.r0, d = colmajor ? dc : dr, size = colmajor ? W : H;
        int64_t klo = 0, khi = n;
        if (d > 0) {
            klo = std::max<int64_t>(0, -a);
            khi = std::min<int64_t>(n, size - 1 - a);
        } else if (d < 0) {
            klo = std::max<int64_t>(0, a - (size - 1));
            khi = std::min<int64_t>(n, a);
        } else if (a < 0 || a >= size) {
            khi = -1;
        }
        BurnLine &l = hl[(size_t)g.line];
        if (kfirst[(size_t)g.line] < 0 || g.koff < kfirst[(size_t)g.line]) {
            kfirst[(size_t)g.line] = g.koff;
            l.fr = g.r0;
            l.fc = g.c0;
        }
        if (g.koff + n >= klast[(size_t)g.line]) {
            klast[(size_t)g.line] = g.koff + n;
            l.lr = g.r1;
            l.lc = g.c1;
        }
        const int64_t slot = at[lines[g.line].flags & 1]++;
        hs[(size_t)slot] = BurnSeg{g.r0, g.c0, g.r1, g.c1, g.line, g.koff, (int32_t)klo, 0};
        hp[(size_t)slot + 1] = khi >= klo ? khi - klo + 1 : 0;      // (the count; summed below)
    }
    hp[0] = 0;
    for (int64_t i = 0; i < nseg; ++i) hp[(size_t)i + 1] += hp[(size_t)i];
    const int64_t steps[2] = {hp[(size_t)nlower], hp[(size_t)nseg] - hp[(size_t)nlower]};
    if (std::max(steps[0], steps[1]) > (int64_t)0x7fffffff * 256) {
        set_error("burn_lines: %lld steps exceed one launch", (long long)std::max(steps[0], steps[1]));
        return MHIP_ELIMIT;
    }
    DevBuf d_s, d_p, d_l, d_r;
    MH_TRY(upload(d_s, hs.data(), sizeof(BurnSeg) * (size_t)nseg, s));
    MH_TRY(upload(d_p, hp.data(), 8 * ((size_t)nseg + 1), s));
    MH_TRY(upload(d_l, hl.data(), sizeof(BurnLine) * (size_t)nline, s));
    MH_TRY(d_r.alloc(sizeof(mhip_burn_result) * (size_t)nline));
    hipLaunchKernelGGL(burn_ends_kernel, dim3((unsigned)cdiv(nline, 256)), dim3(256), 0, s, d_dem, H, W, d_l.as<BurnLine>(), nline, nodata,
                       d_r.as<mhip_burn_result>());
    if (steps[0])
        hipLaunchKernelGGL(burn_steps_kernel<false>, dim3((unsigned)cdiv(steps[0], 256)), dim3(256), 0, s, d_dem, H, W, d_s.as<BurnSeg>(), d_p.as<int64_t>(),
                           nlower, d_l.as<BurnLine>(), d_r.as<mhip_burn_result>());
    if (steps[1])
        hipLaunchKernelGGL(burn_steps_kernel<true>, dim3((unsigned)cdiv(steps[1], 256)), dim3(256), 0, s, d_dem, H, W, d_s.as<BurnSeg>() + nlower,
                           d_p.as<int64_t>() + nlower, nseg - nlower, d_l.as<BurnLine>(), d_r.as<mhip_burn_result>());
    MH_HIP(hipGetLastError());
    return download(results, d_r, sizeof(mhip_burn_result) * (size_t)nline, s);      // (synchronises: the host arrays and the buffers may go)
}

}  // namespace mh
