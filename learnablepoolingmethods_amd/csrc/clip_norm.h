// The norm half of the clip + update passes over a flat parameter arena (clip_adam.hip, clip_update.hip): per-chunk sums of squares,
// then one workgroup per variable that reduces them in a fixed order to the clip factor.  The kernels are `static`: each file that
// includes this header launches its own copy, and both copies hold the same arithmetic in the same order.
#pragma once
#include "lpm_common.h"

namespace lpm {

constexpr int CA_CHUNK = 4096;   // == LPM_ARENA_ALIGN

// which variable owns the chunk that starts at `base`: binary search on the (chunk-aligned) offsets
__device__ __forceinline__ int ca_owner(const int64_t* __restrict__ offsets, int ntensors, int64_t base) {
    int lo = 0, hi = ntensors;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (offsets[mid] <= base) lo = mid; else hi = mid;
    }
    return lo;
}
// l2 (optional, [ntensors]): the analytic gradient of a variable's L2 penalty, coefficient * w (slim.l2_regularizer on the MoE weights,
// video_level_models.py:84-100: part of the loss whose gradient is clipped), formed HERE and in ca_apply_kernel from the parameter both
// passes can read, instead of by an add pass over the gradient arena before them (round 6: 68 us per cfg-5 step for two MoE matrices)
static __global__ __launch_bounds__(256) void ca_chunk_sumsq_kernel(const float* __restrict__ g, int64_t total,
                                                             float* __restrict__ chunk_ss, const float* __restrict__ p,
                                                             const int64_t* __restrict__ offsets, int ntensors,
                                                             const float* __restrict__ l2) {
    const int64_t base = (int64_t)blockIdx.x * CA_CHUNK;
    const float c = l2 ? l2[ca_owner(offsets, ntensors, base)] : 0.f;
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < CA_CHUNK / (256 * 4); ++i) {
        const int64_t e = base + (int64_t)(i * 256 + threadIdx.x) * 4;
        if (e + 3 < total) {
            float4 v = *reinterpret_cast<const float4*>(g + e);
            if (c != 0.f) {
                const float4 w = *reinterpret_cast<const float4*>(p + e);
                v.x = fmaf(c, w.x, v.x); v.y = fmaf(c, w.y, v.y); v.z = fmaf(c, w.z, v.z); v.w = fmaf(c, w.w, v.w);
            }
            s = fmaf(v.x, v.x, s); s = fmaf(v.y, v.y, s); s = fmaf(v.z, v.z, s); s = fmaf(v.w, v.w, s);
        }
    }
    s = wave_sum(s);
    __shared__ float w[4];
    if ((threadIdx.x & 63) == 0) w[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) chunk_ss[blockIdx.x] = (w[0] + w[1]) + (w[2] + w[3]);
}

// one block per variable: factor[t] = clip / max(||g_t||, clip)   (1 when clip <= 0)
static __global__ __launch_bounds__(1024) void ca_tensor_factor_kernel(const float* __restrict__ chunk_ss,
                                                                const int64_t* __restrict__ offsets, float clip,
                                                                float* __restrict__ factor) {
    const int t = blockIdx.x;
    const int64_t c0 = offsets[t] / CA_CHUNK, c1 = (offsets[t + 1] + CA_CHUNK - 1) / CA_CHUNK;
    // 1024 threads, eight independent loads per thread and round: the 33.8 k chunk sums of hidden1_weights are five rounds (one
    // load in flight per thread of a 256-thread workgroup: 132 dependent rounds, 42 us of pure latency; four in flight: 36 us).
    // The order of the additions is fixed.
    double s = 0.0;
    for (int64_t c = c0 + threadIdx.x; c < c1; c += 1024 * 8) {
        float a[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) a[u] = (c + 1024 * u < c1) ? chunk_ss[c + 1024 * u] : 0.f;
        s += (((double)a[0] + (double)a[1]) + ((double)a[2] + (double)a[3])) + (((double)a[4] + (double)a[5]) + ((double)a[6] + (double)a[7]));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    __shared__ double sh[16];
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = 0.0;
        for (int i = 0; i < 16; ++i) tot += sh[i];
        const float nrm = (float)sqrt(tot);
        factor[t] = clip > 0.f ? clip / fmaxf(nrm, clip) : 1.f;
    }
}

}  // namespace lpm
