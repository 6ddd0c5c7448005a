// wetat.hip -- the rain of a series at which every cell gets wet, in one pass over the raster (gfx950).
//
// No reference counterpart.  K events (at most MHIP_WETAT_MAX_EVENTS) with draw-downs T[k][l] and rains values[k] (finite, > 0,
// strictly increasing).  A cell d of label l >= 1 is wet in event k when final_depths_kernel (hyps.hip) gives it water:
//   x = double(d) - T[k][l];  x > 0 and float(x) > 0          (a tie is dry, a NaN draw-down never wets)
//   out = values[k*], k* the FIRST k of the list that wets the cell; 0 when none does, 0 on background
//   wet[k][l] = wet cells of label l in event k, whatever k* is
// Nothing assumes that T[., l] falls with k.
// The thresholds sit label-major on the device in rows of KP = 4, 8 or 16 doubles (K = 16: one 128-byte line a label), padded with
// +inf; the counters are rows of KP 32-bit words next to them.  The traversal is final_depths_kernel's: 32 x 256 tiles, a thread
// owns V consecutive columns of every V-th row and keeps the row of the label of the run it is in in registers (final_depths' `ct`,
// K wide).  A thread sees at most 32 cells of a tile, so a run's K wet counters are 8-bit fields of KP / 4 registers; finished runs
// go to the tile's LDS table of KP counters per label, the table leaves as one atomic per non-zero (label, event, tile); a run that
// finds no slot goes to the global atomics itself.
#include <cmath>

#include "common.hpp"

namespace mh {
namespace {

struct WetAtValues {
    float v[MHIP_WETAT_MAX_EVENTS];
};

// event-major thresholds src[(k * (nlab + 1) + l) * stride] -> label-major rows of KP doubles, +inf behind event K - 1; every word of
// the rows and of the counters is written here (the pool hands out poisoned blocks), and the `bad` word
__global__ __launch_bounds__(256) void wet_at_rows_kernel(const double *__restrict__ src, int64_t stride, int64_t nlab, int K, int KP,
                                                         double *__restrict__ thr, unsigned int *__restrict__ cnt, unsigned int *bad)
{
    const int64_t total = (nlab + 1) * KP, step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += step) {
        const int64_t l = i / KP;
        const int k = (int)(i - l * KP);
        thr[i] = k < K ? src[((int64_t)k * (nlab + 1) + l) * stride] : (double)INFINITY;
        cnt[i] = 0u;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *bad = 0u;
}

// the counters back to event-major int64: dst[(k * (nlab + 1) + l) * stride]; label 0 counts nothing
__global__ __launch_bounds__(256) void wet_at_counts_kernel(const unsigned int *__restrict__ cnt, int64_t nlab, int K, int KP,
                                                           int64_t *__restrict__ dst, int64_t stride)
{
    const int64_t total = (nlab + 1) * K, step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += step) {
        const int64_t k = i / (nlab + 1), l = i - k * (nlab + 1);
        dst[i * stride] = l ? (int64_t)cnt[l * KP + k] : 0;
    }
}

// LDS: keys + KP counters a slot -- 10 KB (KP = 4), 18 KB (8), 17 KB (16: half the slots): eight workgroups and more per CU
template <int KP> constexpr int wet_at_slots() { return KP == 16 ? 256 : 512; }

template <int V, int KP>      // V: 4 or 1; KP: 4, 8 or 16
__global__ __launch_bounds__(256) void wet_at_kernel(const float *__restrict__ data, const int32_t *__restrict__ lab, TileGeom g, int64_t nlab,
                                                    const double *__restrict__ thr, WetAtValues vals, float *__restrict__ out, unsigned int *cnt,
                                                    unsigned int *bad)
{
    constexpr int TS = wet_at_slots<KP>(), NW = KP / 4;
    __shared__ int keys[TS];
    __shared__ unsigned int tcnt[TS * KP];
    constexpr int TPR = 256 / V;      // threads per tile row; V rows per pass of the workgroup
    const int tx = threadIdx.x % TPR, ty = threadIdx.x / TPR;
    unsigned int any_bad = 0;
    const int64_t ntiles = g.ntr * g.ntc;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        for (int k = threadIdx.x; k < TS; k += 256) keys[k] = -1;
        for (int k = threadIdx.x; k < TS * KP; k += 256) tcnt[k] = 0u;
        __syncthreads();
        const int64_t tr = tile / g.ntc, tc = tile - tr * g.ntc;
        const int64_t col = tc * 256 + (int64_t)tx * V;
        int32_t cl = 0;          // the label of the run, its K draw-downs, the run's wet cells per event (8 bits each: at most TR)
        double ct[KP];
        unsigned int cw[NW];
#pragma unroll
        for (int k = 0; k < KP; ++k) ct[k] = (double)INFINITY;
#pragma unroll
        for (int w = 0; w < NW; ++w) cw[w] = 0u;
        static_assert(TR <= 255, "a run's wet cells fit eight bits");
        auto end_run = [&]() {
            unsigned int any = 0u;
#pragma unroll
            for (int w = 0; w < NW; ++w) any |= cw[w];
            if (!any) return;
            const int h = table_slot<TS>(keys, cl);
#pragma unroll
            for (int k = 0; k < KP; ++k) {
                const unsigned int c = (cw[k >> 2] >> (8 * (k & 3))) & 0xffu;
                if (!c) continue;
                if (h >= 0) atomicAdd(&tcnt[h * KP + k], c);
                else atomicAdd(&cnt[(int64_t)cl * KP + k], c);
            }
        };
        for (int r = ty; r < TR; r += V) {
            const int64_t i = (tr * TR + r) * g.W + col;
            if (!(col < g.W && i < g.n)) continue;       // (V = 4: W is a multiple of four, the whole vector is inside)
            int32_t lv[V];
            float dv[V], ov[V];
            if constexpr (V == 4) {
                const int4 l4 = *reinterpret_cast<const int4 *>(lab + i);
                const float4 d4 = *reinterpret_cast<const float4 *>(data + i);
                lv[0] = l4.x; lv[1] = l4.y; lv[2] = l4.z; lv[3] = l4.w;
                dv[0] = d4.x; dv[1] = d4.y; dv[2] = d4.z; dv[3] = d4.w;
            } else {
                lv[0] = lab[i];
                dv[0] = data[i];
            }
#pragma unroll
            for (int e = 0; e < V; ++e) {
                int32_t l = lv[e];
                if (l < 0 || l > nlab) {
                    any_bad = 1;
                    l = 0;
                }
                float o = 0.0f;
                if (l > 0) {
                    if (l != cl) {
                        end_run();
                        cl = l;
                        const double2 *row = reinterpret_cast<const double2 *>(thr + (int64_t)l * KP);      // (rows of 32 bytes and more)
#pragma unroll
                        for (int k = 0; k < KP; k += 2) {
                            const double2 t = row[k >> 1];
                            ct[k] = t.x;
                            ct[k + 1] = t.y;
                        }
#pragma unroll
                        for (int w = 0; w < NW; ++w) cw[w] = 0u;
                    }
                    const double v = (double)dv[e];
                    // from the last event down: the first that wets the cell has the last word
#pragma unroll
                    for (int k = KP - 1; k >= 0; --k) {
                        const double x = v - ct[k];
                        const float f = x > 0.0 ? (float)x : 0.0f;      // final_depths_kernel's value: wet where it is > 0
                        const bool wet = f > 0.0f;
                        o = wet ? vals.v[k] : o;
                        cw[k >> 2] += wet ? 1u << (8 * (k & 3)) : 0u;
                    }
                }
                ov[e] = o;
            }
            if constexpr (V == 4) *reinterpret_cast<float4 *>(out + i) = make_float4(ov[0], ov[1], ov[2], ov[3]);
            else out[i] = ov[0];
        }
        end_run();
        __syncthreads();
        for (int sl = threadIdx.x; sl < TS; sl += 256) {
            const int key = keys[sl];
            if (key < 0) continue;
#pragma unroll
            for (int k = 0; k < KP; ++k) {
                const unsigned int c = tcnt[sl * KP + k];
                if (c) atomicAdd(&cnt[(int64_t)key * KP + k], c);
            }
        }
        __syncthreads();
    }
    if (any_bad) atomicOr(bad, 1u);
}

template <int V, int KP>
void wet_at_launch(const float *d_data, const int32_t *d_labels, const TileGeom &g, int64_t nlab, const double *thr, const WetAtValues &vals,
                   float *d_out, unsigned int *cnt, unsigned int *bad, hipStream_t s)
{
    hipLaunchKernelGGL((wet_at_kernel<V, KP>), dim3(tile_grid(g)), dim3(256), 0, s, d_data, d_labels, g, nlab, thr, vals, d_out, cnt, bad);
}

}  // namespace

bool wet_at_events_ok(int64_t K, const float *values)
{
    if (!values || K < 1 || K > MHIP_WETAT_MAX_EVENTS) return false;
    for (int64_t k = 0; k < K; ++k)
        if (!(values[k] > 0.0f && std::isfinite(values[k]) && (k == 0 || values[k] > values[k - 1]))) return false;
    return true;
}

int wet_at_dev(const float *d_data, const int32_t *d_labels, int64_t n, int64_t W, int64_t nlab, int K, const double *d_drawdown, int64_t stride,
               const float *values, float *d_out, int64_t *d_wet, int64_t wet_stride, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1)
{
    const int KP = K <= 4 ? 4 : K <= 8 ? 8 : 16;
    const int64_t words = (nlab + 1) * KP;
    DevBuf thr, cnt, bad;
    MH_TRY(thr.alloc(8 * (size_t)words));
    MH_TRY(cnt.alloc(4 * (size_t)words));
    MH_TRY(bad.alloc(4));
    WetAtValues vals;
    for (int k = 0; k < MHIP_WETAT_MAX_EVENTS; ++k) vals.v[k] = k < K ? values[k] : 0.0f;
    const unsigned gr = (unsigned)(cdiv(words, 256) < 2048 ? cdiv(words, 256) : 2048);
    hipLaunchKernelGGL(wet_at_rows_kernel, dim3(gr), dim3(256), 0, s, d_drawdown, stride, nlab, K, KP, thr.as<double>(), cnt.as<unsigned int>(),
                       bad.as<unsigned int>());
    const TileGeom g = tile_geom(n, W);
    const bool vec = W > 0 && n % W == 0 && W % 4 == 0 && ((uintptr_t)d_data | (uintptr_t)d_labels | (uintptr_t)d_out) % 16 == 0;
    if (ev0) MH_HIP(hipEventRecord(ev0, s));
#define MH_WETAT(V, P) wet_at_launch<V, P>(d_data, d_labels, g, nlab, thr.as<double>(), vals, d_out, cnt.as<unsigned int>(), bad.as<unsigned int>(), s)
    if (vec) {
        if (KP == 4) MH_WETAT(4, 4);
        else if (KP == 8) MH_WETAT(4, 8);
        else MH_WETAT(4, 16);
    } else {
        if (KP == 4) MH_WETAT(1, 4);
        else if (KP == 8) MH_WETAT(1, 8);
        else MH_WETAT(1, 16);
    }
#undef MH_WETAT
    if (ev1) MH_HIP(hipEventRecord(ev1, s));
    if (d_wet) {
        const int64_t nw = (nlab + 1) * K;
        const unsigned gc = (unsigned)(cdiv(nw, 256) < 2048 ? cdiv(nw, 256) : 2048);
        hipLaunchKernelGGL(wet_at_counts_kernel, dim3(gc), dim3(256), 0, s, cnt.as<unsigned int>(), nlab, K, KP, d_wet, wet_stride);
    }
    MH_HIP(hipGetLastError());
    unsigned int h = 0;
    MH_HIP(hipMemcpyAsync(&h, bad.p, sizeof(h), hipMemcpyDeviceToHost, s));
    MH_HIP(stream_sync(s));      // (the rows and counters go back to the pool)
    if (h) {
        set_error("wet_at: label outside [0, nlabels]");
        return MHIP_EINVAL;
    }
    return MHIP_OK;
}

}  // namespace mh
