// seaflood.hip -- the water level at the sources at which every cell floods (gfx950).
//
// No reference counterpart; tests/_seaflood.py is the definition.  With D the DEM, S the source cells and h_s their stages,
//     D'[c] = +inf where D[c] is NaN or D[c] > max_level, D[c] elsewhere
//     L[s]  = h_s                                   for s in S
//     L[c]  = max(D'[c], min over the 8 neighbours n inside the raster of L[n])   elsewhere
// and L is the GREATEST solution: the minimax cost of an 8-connected path to a source.  Only min and max of input values occur,
// so the result is the model's value for value.
//
// Schedule: chaotic relaxation from above, as fill.hip's.  With C[c] = h_s at a source and D'[c] elsewhere (sf_prepare_kernel
// writes it once), the start is L = C at the sources and +inf elsewhere, and a visit applies L[c] <- max(C[c], min(L[c], 8
// neighbours)): the operator is monotone and every state is an upper bound of the solution, so any order of visits ends at the
// same bits.  A source never moves, because L = C there.
//   * tiles of 64 x 64 cells, one workgroup of 256 a tile, the tile's window with a 1-cell halo in LDS (66 rows of 67 floats: the
//     odd stride keeps a wavefront's reads on 32 distinct banks along a row and along a column).  A thread owns 16 cells of a
//     column, then 16 cells of a row, and runs Gauss-Seidel passes down, up, right and left until no cell of the tile moves.
//   * a tile that moved is stored; where a cell on its perimeter moved, the neighbouring tiles that see that cell are appended to
//     the next round's list (marks de-duplicate; lists, marks and counts are double buffered).  A round is one launch; rounds go
//     out in batches with one read-back of the counts a batch.
//   * a visit may read a halo that a neighbour is storing in the same launch: every value it can see is an upper bound, a 4-byte
//     store does not tear, and the neighbour's wake-up is for the next launch, which sees every store.
// Proof: sf_check_kernel tests both equations at every cell against D' and the sources as they were given (not against C), writes
// the delivered raster (`nodata` where L is +inf) and counts the cells reached; a tile with a failing cell goes back on the list.
#include <algorithm>
#include <cmath>
#include <limits>

#include "common.hpp"

namespace mh {
namespace {

constexpr int SF_T = 64;                   // tile edge
constexpr int SF_WN = SF_T + 2;            // window edge (tile + halo)
constexpr int SF_S = 67;                   // LDS row stride in floats
constexpr int SF_LINE = 16;                // own cells of a thread along a column or a row
constexpr int SF_BATCH = 16;               // rounds between two read-backs (even: the parity of the lists is kept)
constexpr int64_t SF_MAX_ROUNDS = 1 << 20;
constexpr unsigned SF_MAX_BLOCKS = 2048;   // 8 workgroups a CU: a round's workgroups stride over its list

// the sources as they were given: a stage raster (NaN: no source), or the zone raster and a stage per zone (entry 0 and NaN: none)
struct SfSrc {
    const float *dem, *stage;
    const int32_t *zones;
    const float *zone_stage;
    int32_t nzone;
    float max_level;
};

// C of cell i; `src`: the cell is a source, `bad`: ... whose stage is not finite
__device__ __forceinline__ float sf_cost(const SfSrc &q, int64_t i, bool &src, bool &bad)
{
    float h;
    if (q.stage) {
        h = q.stage[i];
    } else {
        const int32_t z = q.zones[i];
        const bool in = z >= 1 && z <= q.nzone;
        h = q.zone_stage[in ? z : 0];      // (entry 0 holds a NaN)
    }
    src = h == h;
    bad = src && fabsf(h) == __builtin_inff();
    const float d = q.dem[i];
    const float dp = (d != d || d > q.max_level) ? __builtin_inff() : d;
    return src ? h : dp;
}

// The tiles that see cell (lr, lc) of a tile: bit (dr + 1) * 3 + (dc + 1) for the tile at (dr, dc) from it; bit 4 is the tile itself.
__device__ __forceinline__ unsigned sf_seen_by(int lr, int lc)
{
    const unsigned rows = 2u | (lr == 0 ? 1u : 0u) | (lr == SF_T - 1 ? 4u : 0u), cols = 2u | (lc == 0 ? 1u : 0u) | (lc == SF_T - 1 ? 4u : 0u);
    return ((rows & 1u) ? cols : 0u) | ((rows & 2u) ? cols << 3 : 0u) | ((rows & 4u) ? cols << 6 : 0u);
}

// tile (tr + dr, tc + dc) of direction bit k onto the list, once
__device__ __forceinline__ void sf_wake(int k, int tr, int tc, int ntr, int ntc, unsigned *mark, int *list, unsigned *cnt)
{
    const int r = tr + k / 3 - 1, c = tc + k % 3 - 1;
    if (r < 0 || r >= ntr || c < 0 || c >= ntc) return;
    const int t = r * ntc + c;
    if (atomicExch(&mark[t], 1u) == 0u) list[atomicAdd(cnt, 1u)] = t;
}

// ---- C and the start of L; the first list: the tiles that see a source ----------------------------------------------------------
__global__ __launch_bounds__(256) void sf_prepare_kernel(SfSrc q, int64_t n, int64_t W, int ntr, int ntc, float *__restrict__ cost, float *__restrict__ L,
                                                         unsigned *mark, int *list, unsigned *cnt, unsigned *badstage)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    bool src, bad;
    const float c = sf_cost(q, i, src, bad);
    cost[i] = c;
    L[i] = src ? c : __builtin_inff();
    if (!src) return;
    if (bad) atomicOr(badstage, 1u);
    const int64_t r = i / W, col = i - r * W;
    const int tr = (int)(r / SF_T), tc = (int)(col / SF_T);
    const unsigned bits = sf_seen_by((int)(r - (int64_t)tr * SF_T), (int)(col - (int64_t)tc * SF_T));
    for (int k = 0; k < 9; ++k) {
        if (!((bits >> k) & 1u)) continue;
        const int rr = tr + k / 3 - 1, cc = tc + k % 3 - 1;
        if (rr < 0 || rr >= ntr || cc < 0 || cc >= ntc) continue;
        if (*(volatile unsigned *)&mark[rr * ntc + cc] == 0u) sf_wake(k, tr, tc, ntr, ntc, mark, list, cnt);      // (a sea of sources: one atomic a tile, mostly)
    }
}

// the window of tile (r0, c0): L with its halo, +inf outside the raster
__device__ __forceinline__ void sf_load_window(float (&Lw)[SF_WN * SF_S], const float *L, int64_t H, int64_t W, int64_t r0, int64_t c0)
{
    for (int idx = threadIdx.x; idx < SF_WN * SF_WN; idx += 256) {
        const int wr = idx / SF_WN, wc = idx - wr * SF_WN;
        const int64_t r = r0 - 1 + wr, c = c0 - 1 + wc;
        const bool in = r >= 0 && r < H && c >= 0 && c < W;
        Lw[wr * SF_S + wc] = in ? L[r * W + c] : __builtin_inff();
    }
}

// One Gauss-Seidel pass along a line of 16 own cells.  p: the first cell in travel order, STEP: to the next one, SIDE: to the line's
// neighbours; d: C of the line in storage order (FWD: travel order).  Three cells across the line enter per step; the cell just
// updated is carried in a register.  L >= C always, so the new value is never above the old one.  Returns the tiles that see a
// cell this pass lowered (bf / bm / bl: sf_seen_by of the line's first / inner / last cell in storage order).
template <bool FWD, int STEP, int SIDE>
__device__ __forceinline__ unsigned sf_pass(float (&Lw)[SF_WN * SF_S], int p, const float (&d)[SF_LINE], unsigned bf, unsigned bm, unsigned bl)
{
    constexpr int step = STEP, side = SIDE;      // (constants: every access of a pass is one base register and an immediate offset)
    unsigned fl = 0;
    float a0 = Lw[p - step - side], a1 = Lw[p - step], a2 = Lw[p - step + side];
    float b0 = Lw[p - side], b1 = Lw[p], b2 = Lw[p + side];
#pragma unroll
    for (int i = 0; i < SF_LINE; ++i) {
        const int at = p + i * step;
        const float c0 = Lw[at + step - side], c1 = Lw[at + step], c2 = Lw[at + step + side];
        const float m = fminf(fminf(fminf(a0, a1), fminf(a2, b0)), fminf(fminf(b2, c0), fminf(c1, c2)));
        const int k = FWD ? i : SF_LINE - 1 - i;
        const float nv = fmaxf(d[k], fminf(b1, m));
        if (nv < b1) {
            Lw[at] = nv;
            fl |= k == 0 ? bf : k == SF_LINE - 1 ? bl : bm;
        }
        a0 = b0; a1 = nv; a2 = b2;
        b0 = c0; b1 = c1; b2 = c2;
        if ((i & 3) == 3) asm volatile("" ::: "memory");      // (the loads of four steps in flight, not of all four passes: registers)
    }
    return fl;
}

// ---- one round: the tiles of the current list to their local fixed points --------------------------------------------------------
__global__ __launch_bounds__(256) void sf_round_kernel(const float *__restrict__ cost, float *L, int64_t H, int64_t W, int ntr, int ntc,
                                                       const int *__restrict__ list_cur, unsigned *mark_cur, const unsigned *cnt_cur, int *list_next,
                                                       unsigned *mark_next, unsigned *cnt_next, unsigned long long *visits)
{
    __shared__ float Lw[SF_WN * SF_S];
    __shared__ unsigned s_bits;
    const int t = threadIdx.x, ln = t & 63, seg = t >> 6;
    const unsigned ncur = *cnt_cur;
    // the own cells: column ln, rows seg * 16 ..; then row ln, columns seg * 16 ..
    const int pv = (seg * SF_LINE + 1) * SF_S + ln + 1, ph = (ln + 1) * SF_S + seg * SF_LINE + 1;
    const unsigned vf = sf_seen_by(seg * SF_LINE, ln), vm = sf_seen_by(seg * SF_LINE + 1, ln), vl = sf_seen_by(seg * SF_LINE + SF_LINE - 1, ln);
    const unsigned hf = sf_seen_by(ln, seg * SF_LINE), hm = sf_seen_by(ln, seg * SF_LINE + 1), hl = sf_seen_by(ln, seg * SF_LINE + SF_LINE - 1);
    unsigned nvisit = 0;
    for (unsigned b = blockIdx.x; b < ncur; b += gridDim.x) {
        const int tile = list_cur[b];
        const int tr = tile / ntc, tc = tile - tr * ntc;
        const int64_t r0 = (int64_t)tr * SF_T, c0 = (int64_t)tc * SF_T;
        if (t == 0) {
            mark_cur[tile] = 0u;      // (this round's launches write the other set of marks only)
            s_bits = 0u;
        }
        // C in both orientations, through the window
        float dv[SF_LINE], dh[SF_LINE];
#pragma unroll
        for (int i = 0; i < SF_LINE; ++i) {
            const int64_t r = r0 + seg * SF_LINE + i, c = c0 + ln;
            dv[i] = (r < H && c < W) ? cost[r * W + c] : __builtin_inff();
            Lw[pv + i * SF_S] = dv[i];
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < SF_LINE; ++i) dh[i] = Lw[ph + i];
        __syncthreads();
        sf_load_window(Lw, L, H, W, r0, c0);
        __syncthreads();
        for (;;) {
            unsigned fl = sf_pass<true, SF_S, 1>(Lw, pv, dv, vf, vm, vl);
            fl |= sf_pass<false, -SF_S, 1>(Lw, pv + (SF_LINE - 1) * SF_S, dv, vf, vm, vl);
            __syncthreads();
            fl |= sf_pass<true, 1, SF_S>(Lw, ph, dh, hf, hm, hl);
            fl |= sf_pass<false, -1, SF_S>(Lw, ph + SF_LINE - 1, dh, hf, hm, hl);
            if (fl) atomicOr(&s_bits, fl);
            if (!__syncthreads_or(fl != 0u)) break;      // four passes in which nothing moved: every cell saw the final window
        }
        const unsigned bits = s_bits;
        if (bits) {      // something moved: the tile, and a wake-up for every tile that sees a cell that moved
#pragma unroll
            for (int i = 0; i < SF_LINE; ++i) {
                const int64_t r = r0 + seg * SF_LINE + i, c = c0 + ln;
                if (r < H && c < W) L[r * W + c] = Lw[pv + i * SF_S];
            }
            if (t < 9 && t != 4 && ((bits >> t) & 1u)) sf_wake(t, tr, tc, ntr, ntc, mark_next, list_next, cnt_next);
        }
        ++nvisit;
        __syncthreads();      // (the window and s_bits are the next tile's)
    }
    if (t == 0 && nvisit) atomicAdd(visits, (unsigned long long)nvisit);
}

// ---- the proof and the delivered raster ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sf_check_kernel(SfSrc q, const float *__restrict__ L, int64_t H, int64_t W, int ntr, int ntc, float nodata,
                                                       float *__restrict__ out, unsigned *mark, int *list, unsigned *cnt, unsigned long long *reached)
{
    __shared__ float Lw[SF_WN * SF_S];
    const int t = threadIdx.x, ln = t & 63, seg = t >> 6;
    const int ntiles = ntr * ntc;
    unsigned nreach = 0;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int tr = tile / ntc, tc = tile - tr * ntc;
        const int64_t r0 = (int64_t)tr * SF_T, c0 = (int64_t)tc * SF_T;
        sf_load_window(Lw, L, H, W, r0, c0);
        __syncthreads();
        bool fail = false;
        for (int i = 0; i < SF_LINE; ++i) {
            const int64_t r = r0 + seg * SF_LINE + i, c = c0 + ln;
            if (r >= H || c >= W) continue;
            const int p = (seg * SF_LINE + i + 1) * SF_S + ln + 1;
            const float cur = Lw[p];
            const float m = fminf(fminf(fminf(Lw[p - SF_S - 1], Lw[p - SF_S]), fminf(Lw[p - SF_S + 1], Lw[p - 1])),
                                  fminf(fminf(Lw[p + 1], Lw[p + SF_S - 1]), fminf(Lw[p + SF_S], Lw[p + SF_S + 1])));
            bool src, bad;
            const float d = sf_cost(q, r * W + c, src, bad);
            const float want = src ? d : fmaxf(d, m);
            fail |= !(want == cur);
            const bool fin = cur < __builtin_inff();
            out[r * W + c] = fin ? cur : nodata;
            nreach += fin ? 1u : 0u;
        }
        if (__syncthreads_or(fail) && t == 0) sf_wake(4, tr, tc, ntr, ntc, mark, list, cnt);
    }
    fd_count_add(nreach, reached);
}

// ---- the series pass ---------------------------------------------------------------------------------------------------------------
// first k with v <= lev[k]; K: none
__device__ __forceinline__ int sf_class(const float *lev, int K, float v)
{
    int lo = 0, hi = K;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (v <= lev[mid]) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

struct SfAcc {      // per class: the cells, the cells whose D is no NaN, the key of their smallest D, their sum
    unsigned long long *wet, *dcells;
    uint32_t *minkey;
    double *sum;
};

// A cell a thread and step, the grid bounded; a thread gathers the run of cells of one class it meets in registers and adds a run to
// the workgroup's table in LDS, the workgroup its table to the global one: where neighbouring cells fall into one class most
// atomics are never issued.
__global__ __launch_bounds__(256) void sf_series_kernel(const float *__restrict__ level, const float *__restrict__ dem, int64_t n, uint32_t nodata_bits,
                                                        int K, const float *__restrict__ levels, SfAcc acc)
{
    __shared__ float s_lev[MHIP_SEA_MAX_LEVELS];
    __shared__ unsigned s_wet[MHIP_SEA_MAX_LEVELS], s_dc[MHIP_SEA_MAX_LEVELS], s_min[MHIP_SEA_MAX_LEVELS];
    __shared__ double s_sum[MHIP_SEA_MAX_LEVELS];
    const int t = threadIdx.x;
    if (t < K) {
        s_lev[t] = levels[t];
        s_wet[t] = 0u;
        s_dc[t] = 0u;
        s_min[t] = 0xffffffffu;
        s_sum[t] = 0.0;
    }
    __syncthreads();
    int cls = -1;
    unsigned wet = 0, dc = 0, mk = 0xffffffffu;
    double sum = 0.0;
    auto flush = [&]() {
        if (cls >= 0 && wet) {
            atomicAdd(&s_wet[cls], wet);
            if (dc) {
                atomicAdd(&s_dc[cls], dc);
                atomicMin(&s_min[cls], mk);
                atomicAdd(&s_sum[cls], sum);
            }
        }
        wet = 0; dc = 0; mk = 0xffffffffu; sum = 0.0;
    };
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + t; i < n; i += step) {
        const float v = level[i];
        const int k = __float_as_uint(v) != nodata_bits ? sf_class(s_lev, K, v) : K;
        if (k >= K) continue;
        if (k != cls) {
            flush();
            cls = k;
        }
        const float d = dem[i];
        ++wet;
        if (d == d) {
            ++dc;
            mk = min(mk, f32_key(d));
            sum += (double)d;
        }
    }
    flush();
    __syncthreads();
    if (t < K && s_wet[t]) {
        atomicAdd(&acc.wet[t], (unsigned long long)s_wet[t]);
        if (s_dc[t]) {
            atomicAdd(&acc.dcells[t], (unsigned long long)s_dc[t]);
            atomicMin(&acc.minkey[t], s_min[t]);
            atomicAdd(&acc.sum[t], s_sum[t]);
        }
    }
}

// depth of one level: float32(z) - D as one subtraction where L <= z, L is not nodata and D is no NaN; +0.0 elsewhere
__global__ __launch_bounds__(256) void sf_depth_kernel(const float *__restrict__ level, const float *__restrict__ dem, int64_t n, uint32_t nodata_bits, float z,
                                                       float *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float v = level[i], d = dem[i];
    const float dep = __fsub_rn(z, d);
    const bool wet = __float_as_uint(v) != nodata_bits && v <= z && d == d;
    out[i] = wet ? dep : 0.0f;
}

// k + 1 of the first level that wets the cell, 0 elsewhere
__global__ __launch_bounds__(256) void sf_class_kernel(const float *__restrict__ level, int64_t n, uint32_t nodata_bits, int K, const float *__restrict__ levels,
                                                       int32_t *__restrict__ out)
{
    __shared__ float s_lev[MHIP_SEA_MAX_LEVELS];
    if ((int)threadIdx.x < K) s_lev[threadIdx.x] = levels[threadIdx.x];
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float v = level[i];
    const int k = __float_as_uint(v) != nodata_bits ? sf_class(s_lev, K, v) : K;
    out[i] = k < K ? k + 1 : 0;
}

int sf_grid(int64_t n, dim3 *grid)
{
    const int64_t nblk = cdiv(n, 256);
    if (nblk > 0x7fffffff) {
        set_error("sea_flood: %lld cells exceed the launch grid", (long long)n);
        return MHIP_ELIMIT;
    }
    *grid = dim3((unsigned)nblk);
    return MHIP_OK;
}

uint32_t bits_of(float v)
{
    uint32_t u;
    memcpy(&u, &v, 4);
    return u;
}

}  // namespace

int sea_flood_check(float max_level, float nodata)
{
    MH_ARG(max_level == max_level, "sea_flood: max_level is a NaN");
    MH_ARG(nodata == nodata, "sea_flood: nodata is a NaN");
    return MHIP_OK;
}

int sea_levels_check(int64_t K, const float *levels, float max_level)
{
    MH_ARG(K >= 1 && K <= MHIP_SEA_MAX_LEVELS && levels, "sea levels: 1 to 256 levels");
    for (int64_t k = 0; k < K; ++k) {
        MH_ARG(std::isfinite(levels[k]) && (k == 0 || levels[k] > levels[k - 1]), "sea levels: the levels must be finite and strictly increasing");
        MH_ARG(levels[k] <= max_level, "sea levels: a level above the max_level of the flood");
    }
    return MHIP_OK;
}

int sea_flood_dev(const float *d_dem, const float *d_stage, const int32_t *d_zones, const float *d_zone_stage, int64_t nzone, int64_t H, int64_t W,
                  float max_level, float nodata, float *d_out, int64_t *reached, SeaStats *st, hipStream_t s)
{
    const int64_t n = H * W, ntr64 = cdiv(H, SF_T), ntc64 = cdiv(W, SF_T);
    if (ntr64 * ntc64 > 0x7fffffff) {
        set_error("sea_flood: %lld cells exceed the int32 tile domain", (long long)n);
        return MHIP_ELIMIT;
    }
    const int ntr = (int)ntr64, ntc = (int)ntc64, ntiles = ntr * ntc;
    dim3 cells;
    MH_TRY(sf_grid(n, &cells));
    const SfSrc q{d_dem, d_stage, d_zones, d_zone_stage, (int32_t)nzone, max_level};
    DevBuf cost, L, ws;
    MH_TRY(cost.alloc(4 * (size_t)n));
    MH_TRY(L.alloc(4 * (size_t)n));
    // workspace: lists[2][ntiles] | marks[2][ntiles] | count[SF_BATCH + 1] | bad stage | visits, reached (64-bit)
    const size_t off_marks = 4 * 2 * (size_t)ntiles, off_cnt = 2 * off_marks, off_bad = off_cnt + 4 * (SF_BATCH + 1);
    const size_t off_u64 = (off_bad + 4 + 7) & ~size_t(7), total = off_u64 + 16;
    MH_TRY(ws.alloc(total));
    MH_HIP(hipMemsetAsync(ws.as<char>() + off_marks, 0, total - off_marks, s));
    int *lists[2] = {ws.as<int>(), ws.as<int>() + ntiles};
    unsigned *marks[2] = {reinterpret_cast<unsigned *>(ws.as<char>() + off_marks), reinterpret_cast<unsigned *>(ws.as<char>() + off_marks) + ntiles};
    unsigned *cnt = reinterpret_cast<unsigned *>(ws.as<char>() + off_cnt), *bad = reinterpret_cast<unsigned *>(ws.as<char>() + off_bad);
    unsigned long long *visits = reinterpret_cast<unsigned long long *>(ws.as<char>() + off_u64), *d_reached = visits + 1;

    hipLaunchKernelGGL(sf_prepare_kernel, cells, dim3(256), 0, s, q, n, W, ntr, ntc, cost.as<float>(), L.as<float>(), marks[0], lists[0], cnt, bad);
    MH_HIP(hipGetLastError());
    unsigned h_first[SF_BATCH + 2];      // the first count ... and the word behind the counts: a stage that is not finite
    MH_HIP(hipMemcpyAsync(h_first, cnt, sizeof(h_first), hipMemcpyDeviceToHost, s));
    MH_HIP(stream_sync(s));
    if (h_first[SF_BATCH + 1]) {
        set_error("invalid argument: sea_flood: the stage of a source is not finite");
        return MHIP_EINVAL;
    }
    const dim3 tiles_grid(std::min<unsigned>((unsigned)ntiles, SF_MAX_BLOCKS));
    int64_t rounds = 0, rechecks = 0;
    unsigned pending = h_first[0];
    for (;;) {
        while (pending) {      // a batch of rounds; round b reads list b & 1 and count b, and appends to the other list and count b + 1
            if (rounds + SF_BATCH > SF_MAX_ROUNDS) {
                set_error("sea_flood did not converge within %lld rounds", (long long)SF_MAX_ROUNDS);
                return MHIP_ENOTCONV;
            }
            for (int b = 0; b < SF_BATCH; ++b)
                hipLaunchKernelGGL(sf_round_kernel, tiles_grid, dim3(256), 0, s, cost.as<float>(), L.as<float>(), H, W, ntr, ntc, lists[b & 1], marks[b & 1],
                                   cnt + b, lists[(b + 1) & 1], marks[(b + 1) & 1], cnt + b + 1, visits);
            MH_HIP(hipGetLastError());
            unsigned h_cnt[SF_BATCH];
            MH_HIP(hipMemcpyAsync(h_cnt, cnt + 1, sizeof(h_cnt), hipMemcpyDeviceToHost, s));
            MH_HIP(stream_sync(s));
            int used = SF_BATCH;
            for (int b = 0; b < SF_BATCH; ++b)
                if (h_cnt[b] == 0) {      // round b appended nothing: the later launches were no-ops, and every mark is clear
                    used = b + 1;
                    break;
                }
            rounds += used;
            pending = used == SF_BATCH ? h_cnt[SF_BATCH - 1] : 0;
            MH_HIP(hipMemsetAsync(cnt, 0, 4 * (SF_BATCH + 1), s));
            if (pending) MH_HIP(hipMemcpyAsync(cnt, &pending, 4, hipMemcpyHostToDevice, s));      // (the last list is list 0 again)
        }
        MH_HIP(hipMemsetAsync(d_reached, 0, 8, s));
        hipLaunchKernelGGL(sf_check_kernel, tiles_grid, dim3(256), 0, s, q, L.as<float>(), H, W, ntr, ntc, nodata, d_out, marks[0], lists[0], cnt, d_reached);
        MH_HIP(hipGetLastError());
        MH_HIP(hipMemcpyAsync(&pending, cnt, 4, hipMemcpyDeviceToHost, s));
        MH_HIP(stream_sync(s));
        if (!pending) break;
        rechecks += pending;      // tiles that failed the proof: relaxed again, and everything is proven again
    }
    unsigned long long h64[2];
    MH_HIP(hipMemcpyAsync(h64, visits, sizeof(h64), hipMemcpyDeviceToHost, s));
    MH_HIP(stream_sync(s));
    if (reached) *reached = (int64_t)h64[1];
    if (st) {
        st->rounds = rounds;
        st->visits = (int64_t)h64[0];
        st->rechecks = rechecks;
    }
    return MHIP_OK;
}

int sea_levels_dev(const float *d_level, const float *d_dem, int64_t n, float nodata, int K, const float *levels, mhip_sea_record *records, hipStream_t s)
{
    // accumulators: wet[K] | dcells[K] | sum[K] (64-bit) | minkey[K] | levels[K]
    DevBuf buf;
    const size_t off_key = 24 * (size_t)K, off_lev = off_key + 4 * (size_t)K;
    MH_TRY(buf.alloc(off_lev + 4 * (size_t)K));
    MH_HIP(hipMemsetAsync(buf.p, 0, off_key, s));
    MH_HIP(hipMemsetAsync(buf.as<char>() + off_key, 0xff, 4 * (size_t)K, s));
    MH_HIP(hipMemcpyAsync(buf.as<char>() + off_lev, levels, 4 * (size_t)K, hipMemcpyHostToDevice, s));
    const SfAcc acc{buf.as<unsigned long long>(), buf.as<unsigned long long>() + K, reinterpret_cast<uint32_t *>(buf.as<char>() + off_key),
                    buf.as<double>() + 2 * (size_t)K};
    const dim3 grid((unsigned)std::min<int64_t>(std::max<int64_t>(cdiv(n, 256), 1), 4096));
    hipLaunchKernelGGL(sf_series_kernel, grid, dim3(256), 0, s, d_level, d_dem, n, bits_of(nodata), K, reinterpret_cast<const float *>(buf.as<char>() + off_lev),
                       acc);
    MH_HIP(hipGetLastError());
    std::vector<unsigned long long> h((size_t)3 * K);
    std::vector<uint32_t> hk((size_t)K);
    MH_HIP(hipMemcpyAsync(h.data(), buf.p, off_key, hipMemcpyDeviceToHost, s));
    MH_HIP(hipMemcpyAsync(hk.data(), buf.as<char>() + off_key, 4 * (size_t)K, hipMemcpyDeviceToHost, s));
    MH_HIP(stream_sync(s));
    // prefix over the classes: a level wets what the levels below it wet
    int64_t wet = 0, dc = 0;
    uint32_t mk = 0xffffffffu;
    double sum = 0.0;
    for (int k = 0; k < K; ++k) {
        double sk;
        memcpy(&sk, &h[(size_t)2 * K + k], 8);
        wet += (int64_t)h[(size_t)k];
        dc += (int64_t)h[(size_t)K + k];
        mk = std::min(mk, hk[(size_t)k]);
        sum += sk;
        records[k].dem_sum = sum;
        records[k].wet_cells = wet;
        records[k].dem_cells = dc;
        records[k].dem_min = dc ? key_f32(mk) : std::numeric_limits<float>::infinity();
        records[k].pad = 0;
    }
    return MHIP_OK;
}

int sea_depths_dev(const float *d_level, const float *d_dem, int64_t n, float nodata, float z, float *d_out, hipStream_t s)
{
    dim3 grid;
    MH_TRY(sf_grid(n, &grid));
    hipLaunchKernelGGL(sf_depth_kernel, grid, dim3(256), 0, s, d_level, d_dem, n, bits_of(nodata), z, d_out);
    MH_HIP(hipGetLastError());
    MH_HIP(stream_sync(s));
    return MHIP_OK;
}

int sea_classes_dev(const float *d_level, int64_t n, float nodata, int K, const float *levels, int32_t *d_out, hipStream_t s)
{
    dim3 grid;
    MH_TRY(sf_grid(n, &grid));
    DevBuf d_lev;
    MH_TRY(upload(d_lev, levels, 4 * (size_t)K, s));
    hipLaunchKernelGGL(sf_class_kernel, grid, dim3(256), 0, s, d_level, n, bits_of(nodata), K, d_lev.as<float>(), d_out);
    MH_HIP(hipGetLastError());
    MH_HIP(stream_sync(s));      // (d_lev goes back to the pool)
    return MHIP_OK;
}

}  // namespace mh
