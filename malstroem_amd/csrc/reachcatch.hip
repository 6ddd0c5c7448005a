// reachcatch.hip -- flood depths from a stage per reach over the reach catchments (gfx950).
//
// No reference counterpart; tests/_reachcatch.py is the definition.  The reach catchments themselves are made where their parts
// live: the reach of a stream cell in flowpaths.hip (fp_reachcell_kernel), the walk to the drainage cell and the gather in hand.hip
// (catch_final_kernel, reach_catchments_dev).  Here, with k = catch[c]:
//   depth[c] = stage[k] - hand[c] as one float32 subtraction where k > 0, hand[c] does not hold the bits of `nodata` and
//              stage[k] > hand[c] (a NaN on either side compares false); +0.0 elsewhere.  stage[0] is never read into a result.
// The records are zones.hip's reduction of depth over catch (zone_stats_dev), unchanged.
#include "common.hpp"

namespace mh {
namespace {

// A streaming pass, V cells a thread (V = 4: n is a multiple of four, 16-byte accesses): 8 B in, one gather from the stage table,
// 4 B out.  An id outside [0, nreach] raises `bad` and reads entry 0, so that no index leaves the table; every value is computed and
// then selected, and every cell is written.
template <int V>
__global__ __launch_bounds__(256) void inundate_kernel(const float *__restrict__ hand, const int32_t *__restrict__ cat, const float *__restrict__ stage,
                                                      int64_t n, int32_t nreach, uint32_t nodata_bits, float *__restrict__ depth, unsigned int *bad)
{
    const int64_t i0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * V;
    bool any_bad = false;
    if (i0 < n) {
        float h[V];
        int32_t k[V];
        if constexpr (V == 4) {
            const float4 hv = *reinterpret_cast<const float4 *>(hand + i0);
            const int4 kv = *reinterpret_cast<const int4 *>(cat + i0);
            h[0] = hv.x; h[1] = hv.y; h[2] = hv.z; h[3] = hv.w;
            k[0] = kv.x; k[1] = kv.y; k[2] = kv.z; k[3] = kv.w;
        } else {
            h[0] = hand[i0];
            k[0] = cat[i0];
        }
        float o[V];
#pragma unroll
        for (int e = 0; e < V; ++e) {
            const bool in = k[e] >= 0 && k[e] <= nreach;
            any_bad |= !in;
            const int32_t z = in ? k[e] : 0;
            const float sv = stage[z];
            const float d = __fsub_rn(sv, h[e]);
            const bool wet = z > 0 && __float_as_uint(h[e]) != nodata_bits && sv > h[e];      // (a NaN compares false)
            o[e] = wet ? d : 0.0f;
        }
        if constexpr (V == 4) *reinterpret_cast<float4 *>(depth + i0) = make_float4(o[0], o[1], o[2], o[3]);
        else depth[i0] = o[0];
    }
    if (__any(any_bad) && (threadIdx.x & 63) == 0) atomicOr(bad, 1u);
}

}  // namespace

int inundate_dev(const float *d_hand, const int32_t *d_catch, int64_t n, int64_t W, int64_t nreach, const float *d_stage, float nodata, float *d_depth,
                 mhip_zone_record *d_rec, hipStream_t s)
{
    DevBuf bad;
    MH_TRY(bad.alloc(4));
    MH_HIP(hipMemsetAsync(bad.p, 0, 4, s));
    uint32_t nb;
    memcpy(&nb, &nodata, 4);
    const bool vec = n % 4 == 0 && ((uintptr_t)d_hand | (uintptr_t)d_catch | (uintptr_t)d_depth) % 16 == 0;
    const int V = vec ? 4 : 1;
    const int64_t nblk = cdiv(cdiv(n, V), 256);
    if (nblk > 0x7fffffff) {
        set_error("inundate: %lld cells exceed the launch grid", (long long)n);
        return MHIP_ELIMIT;
    }
    const dim3 grid((unsigned)nblk), block(256);
    if (vec) hipLaunchKernelGGL(inundate_kernel<4>, grid, block, 0, s, d_hand, d_catch, d_stage, n, (int32_t)nreach, nb, d_depth, bad.as<unsigned int>());
    else hipLaunchKernelGGL(inundate_kernel<1>, grid, block, 0, s, d_hand, d_catch, d_stage, n, (int32_t)nreach, nb, d_depth, bad.as<unsigned int>());
    MH_HIP(hipGetLastError());
    unsigned int h = 0;
    MH_HIP(hipMemcpyAsync(&h, bad.p, sizeof(h), hipMemcpyDeviceToHost, s));
    MH_HIP(stream_sync(s));
    if (h) {
        set_error("invalid argument: inundate: a catchment id outside [0, nreach]");
        return MHIP_EINVAL;
    }
    if (d_rec) MH_TRY(zone_stats_dev(d_depth, d_catch, n, W, nreach, d_rec, s));      // (synchronises)
    return MHIP_OK;
}

}  // namespace mh
