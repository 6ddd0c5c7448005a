// mfd.hip -- multiple-flow-direction accumulation: fixed-point fractions of a surface, their exact uint64 sums (gfx950).
//
// No reference counterpart; tests/_mfd.py is the definition.  Two stateless functions:
//   fractions   per interior cell with a finite z the eight downhill slopes s_k (d8.hip's neighbour order and INV_SQRT2; a drop that
//               is not in (0, inf) counts 0), m the first largest one (the D8 choice), t_k = (s_k / s_m) ** exponent by repeated
//               multiplication, T their sum in order, q_k = floor(t_k / T * ONE) and the remainder ONE - sum(q) added to q_m: uint16
//               fractions of ONE = 32768 that sum to ONE, or to 0 at a sink, on the border and where z is not finite.  Every float64
//               operation is rounded on its own (the explicit _rn intrinsics; the library is built with -ffp-contract=off).
//   accumulate  acc[c] = weight[c] + what the neighbours send; a cell sends once, when every in-edge (a neighbour with a positive
//               fraction towards it) has delivered: out_k = (acc * p_k) >> 15 for k != m (m: the first largest p_k), and
//               out_m = acc - the others, so nothing is lost.  The floor is not additive: the result is defined by Kahn's order.  The
//               cells Kahn never releases (a cycle of caller-made fractions and everything downstream) hold MHIP_WACC_UNRESOLVED.
//
// Engine of the accumulation: the schedule of seaflood.hip.  Tiles of 64 x 64 cells, one workgroup of 256 a tile, rounds of one
// launch each over double-buffered lists with marks, rounds sent in batches with one read-back of the counts a batch.
//   * state per cell in global memory: the sum so far (the output raster itself) and a 16-bit word: WAIT, the mask of the directions
//     from which an inflow is still awaited, and FIRED.  A delivery is identified by its edge: it can never be taken twice.
//   * a visit holds the tile's sums in LDS as 64-bit words (32 KB) and WAIT as bytes (4 KB), the fractions of a thread's 16 cells in
//     registers.  Sweeps fire every cell of the thread whose WAIT is 0: 64-bit LDS adds to the receivers, then the receiver's bit is
//     cleared with a release; the owner reads WAIT with an acquire before it reads the sum.  A vote ends the loop when no cell fired.
//     The sending code exists once and takes the cell's fractions out of the registers by selects (sixteen unrolled copies made
//     the compiler index the fractions in a private segment); the state is stored by a rolled loop that keeps no addresses live.
//   * a share that crosses a tile edge goes to a slot of its own: one 8-byte word per cell and in-direction on the receiving tile's
//     perimeter (768 a tile), written once, by its only producer, with one 8-byte atomic store of share + 1 (0: nothing yet).  The
//     receiving tile goes on the next round's list.  A visit reads the slots of the bits it still awaits: one a neighbour writes in
//     the same launch is seen whole or not at all, and if not, the wake-up is for the next launch, which sees every store.  A tile
//     is on a list once, so its state has one writer: no fence inside a launch, and no kernel waits on another workgroup.
//   * the first round visits every tile, derives WAIT from the neighbours' fractions (a 66 x 66 window of out-masks in LDS) and
//     checks that a cell's fractions sum to 0 or ONE; when the lists are empty mfd_final_kernel writes the sentinel where a cell
//     never fired and counts.  Every round that has a list follows a round that fired a cell: at most as many rounds as cells.
// LDS of a visit: 32 KB of sums + 4.3 KB (the window, then WAIT) + the vote words = 37 152 B: four workgroups per CU of 160 KB by LDS;
// the registers (the fractions alone are 64) allow two.  No private segment.  Traffic per cell: the first round reads 16 B of fractions
// + 4 B of weight and writes 10 B; a later visit of a tile reads and writes 10 B and reads the fractions of the cells not yet fired.
#include <algorithm>

#include "common.hpp"

namespace mh {
namespace {

constexpr int MF_T = 64;                    // tile edge
constexpr int MF_TN = 256;                  // threads per tile
constexpr int MF_CPT = MF_T * MF_T / MF_TN; // cells per thread: cell j of thread t is (t / 64 + 4 j, t % 64)
constexpr int MF_SLOTS = 4 * MF_T * 3;      // words per tile: side, position along it, offset of the sender along it
constexpr int MF_WN = MF_T + 2;             // the window of out-masks of the first round
constexpr int MF_BATCH = 16;                // rounds between two read-backs (even: the parity of the lists is kept)
constexpr int64_t MF_MAX_ROUNDS = 1ll << 31;
constexpr unsigned MF_MAX_BLOCKS = 2048;
constexpr uint32_t MF_ONE = MHIP_MFD_ONE;
constexpr uint16_t MF_FIRED = 0x100;

// ---- the fractions of a surface -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mfd_fractions_kernel(const double *__restrict__ z, int64_t H, int64_t W, int exponent, uint4 *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= H * W) return;
    const int64_t r = i / W, c = i - r * W;
    uint32_t q[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const double zc = z[i];
    if (r > 0 && r < H - 1 && c > 0 && c < W - 1 && fabs(zc) < __builtin_inf()) {
        const double INV_SQRT2 = 0.7071067811865475;      // d8.hip's
        double s[8];
        int m = -1;
        double sm = 0.0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            double dz = __dsub_rn(zc, z[(r + dir_dr(k)) * W + c + dir_dc(k)]);
            if (k & 1) dz = __dmul_rn(dz, INV_SQRT2);
            s[k] = (dz > 0.0 && dz < __builtin_inf()) ? dz : 0.0;
            if (s[k] > sm) {      // (strict: the first maximum wins)
                sm = s[k];
                m = k;
            }
        }
        if (m >= 0) {
            double t[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const double rk = __ddiv_rn(s[k], sm);
                t[k] = rk;
                for (int e = 1; e < exponent; ++e) t[k] = __dmul_rn(t[k], rk);
            }
            double T = __dadd_rn(t[0], t[1]);
#pragma unroll
            for (int k = 2; k < 8; ++k) T = __dadd_rn(T, t[k]);
            uint32_t sum = 0;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                q[k] = (uint32_t)__dmul_rn(__ddiv_rn(t[k], T), (double)MF_ONE);      // (not negative: the conversion is the floor)
                sum += q[k];
            }
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (k == m) q[k] += MF_ONE - sum;
        }
    }
    out[i] = make_uint4(q[0] | q[1] << 16, q[2] | q[3] << 16, q[4] | q[5] << 16, q[6] | q[7] << 16);
}

// ---- the accumulation -----------------------------------------------------------------------------------------------------------
struct MfArgs {
    const uint4 *fr;              // the fractions, 16 B a cell
    const uint32_t *wt;           // the weights, or null: `wconst` everywhere
    uint32_t wconst;
    unsigned long long *acc;      // the sums so far: the output raster
    uint16_t *st;                 // WAIT | FIRED
    unsigned long long *slots;    // [tile][MF_SLOTS]: share + 1
    int H, W;                     // (fewer than 2**31 cells: a cell's index is an int)
    int ntr, ntc;
};

// The slot of receiving cell (lr, lc) of a tile for in-direction j, whose neighbour lies outside the tile.  A corner's diagonal
// belongs to the top or bottom side.
__device__ __forceinline__ int mf_slot_of(int lr, int lc, int j)
{
    const int nr = lr + dir_dr(j), nc = lc + dir_dc(j);
    if (nr < 0) return lc * 3 + dir_dc(j) + 1;
    if (nr >= MF_T) return 3 * MF_T + lc * 3 + dir_dc(j) + 1;
    if (nc < 0) return 6 * MF_T + lr * 3 + dir_dr(j) + 1;
    return 9 * MF_T + lr * 3 + dir_dr(j) + 1;
}

struct MfFr {      // the eight fractions of a cell, two to a word
    uint32_t w[4];
};
__device__ __forceinline__ MfFr mf_load(const uint4 *p)
{
    const uint4 v = *p;
    MfFr f;
    f.w[0] = v.x; f.w[1] = v.y; f.w[2] = v.z; f.w[3] = v.w;
    return f;
}
__device__ __forceinline__ uint32_t mf_p(const MfFr &f, int k) { return (k & 1) ? f.w[k >> 1] >> 16 : f.w[k >> 1] & 0xffffu; }

__device__ __forceinline__ unsigned mf_outmask(const MfFr &f, bool &valid)
{
    unsigned m = 0, sum = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint32_t p = mf_p(f, k);
        m |= p ? 1u << k : 0u;
        sum += p;
    }
    valid = sum == 0u || sum == MF_ONE;
    return m;
}

// (a * p) >> 15 for a < 2**63 and p <= 2**15: the 78-bit product in two halves
__device__ __forceinline__ unsigned long long mf_share(unsigned long long a, uint32_t p)
{
    return (((a >> 32) * p) << 17) + (((a & 0xffffffffull) * p) >> 15);
}

template <bool FIRST>
__global__ __launch_bounds__(MF_TN) void mfd_round_kernel(MfArgs a, const int *__restrict__ list_cur, unsigned *mark_cur, const unsigned *cnt_cur, int *list_next,
                                                         unsigned *mark_next, unsigned *cnt_next, unsigned *bad, unsigned long long *visits)
{
    __shared__ unsigned long long acc_l[MF_T * MF_T];
    __shared__ uint32_t wait_w[(MF_WN * MF_WN + 3) / 4];      // WAIT of the 4096 cells; the first round's window of out-masks in front of it
    __shared__ int vote_w[3];
    __shared__ unsigned s_wake;
    uint8_t *wait_b = reinterpret_cast<uint8_t *>(wait_w);
    const int tid = threadIdx.x, lc = tid & 63, lr0 = tid >> 6;
    const unsigned ncur = FIRST ? (unsigned)(a.ntr * a.ntc) : *cnt_cur;
    unsigned nvisit = 0;
    for (unsigned b = blockIdx.x; b < ncur; b += gridDim.x) {
        const int tile = FIRST ? (int)b : list_cur[b];
        const int tr = tile / a.ntc, tc = tile - tr * a.ntc;
        const int r0 = tr * MF_T, c0 = tc * MF_T;
        if (tid < 3) vote_w[tid] = 0;
        if (tid == 0) {
            s_wake = 0u;
            if (!FIRST) mark_cur[tile] = 0u;      // (this round's launches write the other set of marks only)
        }
        MfFr fr[MF_CPT];
        unsigned fired = 0;      // bit j: cell j has fired, or is no raster cell
#pragma unroll
        for (int j = 0; j < MF_CPT; ++j) {
            const int i = tid + MF_TN * j;
            const int gr = r0 + lr0 + 4 * j, gc = c0 + lc;
            const bool inside = gr < a.H && gc < a.W;
            fr[j].w[0] = fr[j].w[1] = fr[j].w[2] = fr[j].w[3] = 0u;
            unsigned long long v = 0ull;
            unsigned w = 0u;
            if (!inside) {
                fired |= 1u << j;
            } else if (FIRST) {
                fr[j] = mf_load(a.fr + gr * a.W + gc);
                v = a.wt ? a.wt[gr * a.W + gc] : a.wconst;
            } else {
                const unsigned s = a.st[gr * a.W + gc];
                v = a.acc[gr * a.W + gc];
                w = s & 0xffu;
                if (s & MF_FIRED) fired |= 1u << j;
                else fr[j] = mf_load(a.fr + gr * a.W + gc);
            }
            acc_l[i] = v;
            if (!FIRST) wait_b[i] = (uint8_t)w;
        }
        if (FIRST) {
            // WAIT from the out-masks of the neighbours: a window of 66 x 66 bytes
            uint8_t *om = wait_b;
            bool invalid = false;
#pragma unroll
            for (int j = 0; j < MF_CPT; ++j) {
                bool valid;
                const unsigned m = mf_outmask(fr[j], valid);
                invalid |= !valid;
                om[(lr0 + 4 * j + 1) * MF_WN + lc + 1] = (uint8_t)m;
            }
            for (int h = tid; h < 4 * MF_T + 4; h += MF_TN) {      // the halo: top row, bottom row, left column, right column
                int wr, wc;
                if (h < MF_WN) { wr = 0; wc = h; }
                else if (h < 2 * MF_WN) { wr = MF_WN - 1; wc = h - MF_WN; }
                else if (h < 2 * MF_WN + MF_T) { wr = h - 2 * MF_WN + 1; wc = 0; }
                else { wr = h - 2 * MF_WN - MF_T + 1; wc = MF_WN - 1; }
                const int gr = r0 - 1 + wr, gc = c0 - 1 + wc;
                unsigned m = 0;
                if (gr >= 0 && gr < a.H && gc >= 0 && gc < a.W) {
                    bool valid;      // (checked by the cell's own tile)
                    m = mf_outmask(mf_load(a.fr + gr * a.W + gc), valid);
                }
                om[wr * MF_WN + wc] = (uint8_t)m;
            }
            __syncthreads();
            unsigned wait[MF_CPT];
#pragma unroll
            for (int j = 0; j < MF_CPT; ++j) {
                const int lr = lr0 + 4 * j;
                unsigned w = 0;
#pragma unroll
                for (int d = 0; d < 8; ++d) {      // the neighbour in direction d sends along (d + 4) & 7
                    const unsigned m = om[(lr + 1 + dir_dr(d)) * MF_WN + lc + 1 + dir_dc(d)];
                    w |= ((m >> ((d + 4) & 7)) & 1u) << d;
                }
                wait[j] = ((fired >> j) & 1u) ? 0u : w;
            }
            __syncthreads();      // (the window has been read: its bytes are WAIT from here on)
#pragma unroll
            for (int j = 0; j < MF_CPT; ++j) wait_b[tid + MF_TN * j] = (uint8_t)wait[j];
            if (invalid) *bad = 1u;
        }
        __syncthreads();
        // the shares that have arrived from other tiles: a thread per perimeter cell
        if (tid < 4 * MF_T - 4) {
            int lr, lcp;
            if (tid < MF_T) { lr = 0; lcp = tid; }
            else if (tid < 2 * MF_T) { lr = MF_T - 1; lcp = tid - MF_T; }
            else if (tid < 3 * MF_T - 2) { lr = tid - 2 * MF_T + 1; lcp = 0; }
            else { lr = tid - (3 * MF_T - 2) + 1; lcp = MF_T - 1; }
            const int i = lr * MF_T + lcp;
            unsigned w = wait_b[i];
            if (w) {
                unsigned long long v = acc_l[i];
#pragma unroll
                for (int d = 0; d < 8; ++d) {
                    const int nr = lr + dir_dr(d), nc = lcp + dir_dc(d);
                    if (((w >> d) & 1u) && (nr < 0 || nr >= MF_T || nc < 0 || nc >= MF_T)) {
                        const unsigned long long got =
                            __hip_atomic_load(&a.slots[(int64_t)tile * MF_SLOTS + mf_slot_of(lr, lcp, d)], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        if (got) {
                            v += got - 1ull;
                            w &= ~(1u << d);
                        }
                    }
                }
                acc_l[i] = v;
                wait_b[i] = (uint8_t)w;
            }
        }
        __syncthreads();

        unsigned wake = 0;      // bit (dr + 1) * 3 + (dc + 1): the tile at (dr, dc) from this one got a share
        WgVote vote(vote_w);
        bool more = true;
        while (more) {      // (a sweep that goes on has fired a cell: at most 4096 sweeps)
            bool mine;
            unsigned ready = 0;
#pragma unroll
            for (int j = 0; j < MF_CPT; ++j) {
                if ((fired >> j) & 1u) continue;
                const int i = tid + MF_TN * j;
                const uint32_t ww = __hip_atomic_load(&wait_w[i >> 2], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (((ww >> (8 * (i & 3))) & 0xffu) == 0u) ready |= 1u << j;
            }
            fired |= ready;
            mine = ready != 0u;
            while (ready) {      // (one copy of the sending code: the cell's fractions are picked out of the registers)
                const int js = __ffs((int)ready) - 1;
                ready &= ready - 1u;
                MfFr f = fr[0];
#pragma unroll
                for (int j = 1; j < MF_CPT; ++j)
                    if (j == js) f = fr[j];
                // every in-edge has delivered, and every add is in: the sum is final.  Send it on
                const int i = tid + MF_TN * js, lr = lr0 + 4 * js;
                const unsigned long long total = __hip_atomic_load(&acc_l[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                int m = 0;
                uint32_t pm = mf_p(f, 0);
#pragma unroll
                for (int k = 1; k < 8; ++k) {
                    const uint32_t p = mf_p(f, k);
                    if (p > pm) {      // (strict: the first maximum)
                        pm = p;
                        m = k;
                    }
                }
                unsigned long long o[8], others = 0ull;
#pragma unroll
                for (int k = 0; k < 8; ++k) {      // the seven floors, then what is left for m
                    o[k] = k == m ? 0ull : mf_share(total, mf_p(f, k));
                    others += o[k];
                }
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    if (!mf_p(f, k)) continue;
                    const unsigned long long ok = k == m ? total - others : o[k];
                    const int nr = lr + dir_dr(k), nc = lc + dir_dc(k);
                    const int gr = r0 + nr, gc = c0 + nc;
                    if (gr < 0 || gr >= a.H || gc < 0 || gc >= a.W) continue;      // the share leaves the raster
                    if (nr >= 0 && nr < MF_T && nc >= 0 && nc < MF_T) {
                        const int t = nr * MF_T + nc;
                        atomicAdd(&acc_l[t], ok);
                        __hip_atomic_fetch_and(&wait_w[t >> 2], ~((1u << ((k + 4) & 7)) << (8 * (t & 3))), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
                    } else {
                        const int ddr = nr < 0 ? -1 : nr >= MF_T ? 1 : 0, ddc = nc < 0 ? -1 : nc >= MF_T ? 1 : 0;
                        const int64_t tile2 = (int64_t)(tr + ddr) * a.ntc + tc + ddc;
                        __hip_atomic_store(&a.slots[tile2 * MF_SLOTS + mf_slot_of(nr - ddr * MF_T, nc - ddc * MF_T, (k + 4) & 7)], ok + 1ull, __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT);
                        wake |= 1u << ((ddr + 1) * 3 + ddc + 1);
                    }
                }
            }
            more = vote.any(mine);      // (its barrier ends the sweep)
        }
        if (wake) atomicOr(&s_wake, wake);
        // the tile's state (a rolled loop: no addresses are kept over the sweeps)
#pragma unroll 1
        for (int j = 0; j < MF_CPT; ++j) {
            const int gr = r0 + lr0 + 4 * j, gc = c0 + lc;
            if (gr < a.H && gc < a.W) {
                const int i = tid + MF_TN * j;
                a.acc[gr * a.W + gc] = acc_l[i];
                a.st[gr * a.W + gc] = (uint16_t)(wait_b[i] | (((fired >> j) & 1u) ? MF_FIRED : 0));
            }
        }
        __syncthreads();
        if (tid < 9 && tid != 4 && ((s_wake >> tid) & 1u)) {
            const int r = tr + tid / 3 - 1, c = tc + tid % 3 - 1;      // (inside the tile grid: the share went to a raster cell)
            const int t = r * a.ntc + c;
            if (atomicExch(&mark_next[t], 1u) == 0u) list_next[atomicAdd(cnt_next, 1u)] = t;
        }
        ++nvisit;
        __syncthreads();      // (the LDS is the next tile's)
    }
    if (tid == 0 && nvisit) atomicAdd(visits, (unsigned long long)nvisit);
}

// the cells that never fired: the sentinel, and their number
__global__ __launch_bounds__(256) void mfd_final_kernel(const uint16_t *__restrict__ st, int64_t n, unsigned long long *__restrict__ out, unsigned long long *unresolved)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned cnt = 0;
    if (i < n) {
        const unsigned s = st[i];
        if ((s & 0xffu) != 0u || !(s & MF_FIRED)) {
            out[i] = MHIP_WACC_UNRESOLVED;
            cnt = 1;
        }
    }
    fd_count_add(cnt, unresolved);
}

}  // namespace

int mfd_check(int64_t H, int64_t W)
{
    MH_ARG(H >= 1 && W >= 1 && H <= 0x7fffffff && W <= 0x7fffffff, "mfd: H, W in [1, 2**31 - 1]");
    if (H * W >= (1ll << 31)) {      // (a resolved sum stays below 2**63: the product with a fraction is split at 32 bits)
        set_error("mfd: %lld x %lld cells: a raster holds fewer than 2**31 cells", (long long)H, (long long)W);
        return MHIP_ELIMIT;
    }
    return MHIP_OK;
}

int mfd_fractions_dev(const double *d_z, int64_t H, int64_t W, int exponent, uint16_t *d_out, hipStream_t s)
{
    MH_TRY(mfd_check(H, W));
    MH_ARG(exponent >= 1 && exponent <= 8, "mfd_fractions: exponent in [1, 8]");
    hipLaunchKernelGGL(mfd_fractions_kernel, dim3((unsigned)cdiv(H * W, 256)), dim3(256), 0, s, d_z, H, W, exponent, reinterpret_cast<uint4 *>(d_out));
    MH_HIP(hipGetLastError());
    return MHIP_OK;
}

int mfd_accum_dev(const uint16_t *d_fr, const uint32_t *d_w, uint32_t wconst, int64_t H, int64_t W, unsigned long long *d_out, int64_t *unresolved,
                  MfdStats *stats, hipStream_t s)
{
    MH_TRY(mfd_check(H, W));
    const int64_t n = H * W;
    const int ntr = (int)cdiv(H, MF_T), ntc = (int)cdiv(W, MF_T);
    const int64_t ntiles64 = (int64_t)ntr * ntc;
    if (ntiles64 > (1ll << 24)) {      // (a raster a few cells high or wide)
        set_error("mfd: %lld x %lld cells: more than 2**24 tiles of 64 x 64", (long long)H, (long long)W);
        return MHIP_ELIMIT;
    }
    const int ntiles = (int)ntiles64;
    DevBuf st, slots, ws;
    MH_TRY(st.alloc(2 * (size_t)n));
    MH_TRY(slots.alloc(8 * (size_t)MF_SLOTS * (size_t)ntiles));
    // workspace: lists[2][ntiles] | marks[2][ntiles] | count[MF_BATCH + 1] | bad fractions | visits, unresolved (64-bit)
    const size_t off_marks = 4 * 2 * (size_t)ntiles, off_cnt = 2 * off_marks, off_bad = off_cnt + 4 * (MF_BATCH + 1);
    const size_t off_u64 = (off_bad + 4 + 7) & ~size_t(7), total = off_u64 + 16;
    MH_TRY(ws.alloc(total));
    MH_HIP(hipMemsetAsync(ws.as<char>() + off_marks, 0, total - off_marks, s));
    MH_HIP(hipMemsetAsync(slots.p, 0, 8 * (size_t)MF_SLOTS * (size_t)ntiles, s));
    int *lists[2] = {ws.as<int>(), ws.as<int>() + ntiles};
    unsigned *marks[2] = {reinterpret_cast<unsigned *>(ws.as<char>() + off_marks), reinterpret_cast<unsigned *>(ws.as<char>() + off_marks) + ntiles};
    unsigned *cnt = reinterpret_cast<unsigned *>(ws.as<char>() + off_cnt), *bad = reinterpret_cast<unsigned *>(ws.as<char>() + off_bad);
    unsigned long long *visits = reinterpret_cast<unsigned long long *>(ws.as<char>() + off_u64), *d_unres = visits + 1;
    const MfArgs a{reinterpret_cast<const uint4 *>(d_fr), d_w, wconst, d_out, st.as<uint16_t>(), slots.as<unsigned long long>(), (int)H, (int)W, ntr, ntc};
    const dim3 grid(std::min<unsigned>((unsigned)ntiles, MF_MAX_BLOCKS));

    // the first round: every tile; it appends to list 0
    hipLaunchKernelGGL((mfd_round_kernel<true>), grid, dim3(MF_TN), 0, s, a, (const int *)nullptr, (unsigned *)nullptr, (const unsigned *)nullptr, lists[0], marks[0],
                       cnt, bad, visits);
    MH_HIP(hipGetLastError());
    unsigned h_first[MF_BATCH + 2];      // the first count ... and the word behind the counts: fractions that sum to neither 0 nor ONE
    MH_HIP(hipMemcpyAsync(h_first, cnt, sizeof(h_first), hipMemcpyDeviceToHost, s));
    MH_HIP(stream_sync(s));
    if (h_first[MF_BATCH + 1]) {
        set_error("invalid argument: mfd_accum: the fractions of a cell sum to neither 0 nor %u", MF_ONE);
        return MHIP_EINVAL;
    }
    int64_t rounds = 1;
    unsigned pending = h_first[0];
    while (pending) {      // a batch of rounds; round b reads list b & 1 and count b, and appends to the other list and count b + 1
        if (rounds + MF_BATCH > MF_MAX_ROUNDS) {
            set_error("mfd_accum: more than %lld rounds", (long long)MF_MAX_ROUNDS);
            return MHIP_ELIMIT;
        }
        for (int b = 0; b < MF_BATCH; ++b)
            hipLaunchKernelGGL((mfd_round_kernel<false>), grid, dim3(MF_TN), 0, s, a, lists[b & 1], marks[b & 1], cnt + b, lists[(b + 1) & 1], marks[(b + 1) & 1],
                               cnt + b + 1, bad, visits);
        MH_HIP(hipGetLastError());
        unsigned h_cnt[MF_BATCH];
        MH_HIP(hipMemcpyAsync(h_cnt, cnt + 1, sizeof(h_cnt), hipMemcpyDeviceToHost, s));
        MH_HIP(stream_sync(s));
        int used = MF_BATCH;
        for (int b = 0; b < MF_BATCH; ++b)
            if (h_cnt[b] == 0) {      // round b appended nothing: the later launches were no-ops, and every mark is clear
                used = b + 1;
                break;
            }
        rounds += used;
        pending = used == MF_BATCH ? h_cnt[MF_BATCH - 1] : 0;
        MH_HIP(hipMemsetAsync(cnt, 0, 4 * (MF_BATCH + 1), s));
        if (pending) MH_HIP(hipMemcpyAsync(cnt, &pending, 4, hipMemcpyHostToDevice, s));      // (the last list is list 0 again)
    }
    hipLaunchKernelGGL(mfd_final_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, s, st.as<uint16_t>(), n, d_out, d_unres);
    MH_HIP(hipGetLastError());
    unsigned long long h64[2];
    MH_HIP(hipMemcpyAsync(h64, visits, sizeof(h64), hipMemcpyDeviceToHost, s));
    MH_HIP(stream_sync(s));      // (the workspace goes back to the pool)
    *unresolved = (int64_t)h64[1];
    if (stats) {
        stats->rounds = rounds;
        stats->visits = (int64_t)h64[0];
        stats->tiles = ntiles;
    }
    return MHIP_OK;
}

}  // namespace mh
