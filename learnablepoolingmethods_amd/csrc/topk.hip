// Row top-k of the predictions (export_model.py: the top 20 classes per video; inference.py's CSV lines): for every row of an fp32
// [B, V] matrix the k largest entries in the order of torch.sort(p, dim=1, descending=True, stable=True)[:, :k] -- ties by ascending
// class index, NaN above +inf (NaNs among themselves by index), -0 equal to +0.
// Every entry becomes a distinct 48-bit key: the float's bits under an order-preserving map (all NaNs to one top value, -0 to +0) in
// the upper 32 bits, 65535 - index in the lower 16, so that "larger key" is exactly the sort's "earlier".  One workgroup per row
// selects the k largest keys one after the other: round i takes the largest key below the one round i - 1 took (each thread over its
// strided columns, then the four waves) -- k rounds over a row that stays in the cache.
#include "lpm_common.h"

namespace lpm {

constexpr int TOPK_MAX_K = 64;
constexpr int TOPK_MAX_V = 65536;

__device__ __forceinline__ uint64_t topk_key(float x, int i) {
    unsigned u = __float_as_uint(x);
    if (x != x) u = 0xFFFFFFFFu;                           // NaN: above the image of +inf (0xFF800000)
    else if (x == 0.f) u = 0x80000000u;                    // -0 and +0 tie
    else u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((uint64_t)u << 16) | (uint64_t)(TOPK_MAX_V - 1 - i);
}

__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint64_t w = __shfl_xor(v, o, 64);
        v = w > v ? w : v;
    }
    return v;
}

__global__ __launch_bounds__(256) void topk_rows_kernel(const float* __restrict__ p, int V, int k, int32_t* __restrict__ index,
                                                        float* __restrict__ value) {
    __shared__ uint64_t wmax[2][4];
    const int row = blockIdx.x, wave = threadIdx.x >> 6;
    const float* pr = p + (int64_t)row * V;
    uint64_t prev = (uint64_t)1 << 48;                    // above every key
    for (int r = 0; r < k; ++r) {
        uint64_t best = 0;                                 // below every key (the index part of a key is < 65536, its value part > 0)
        for (int i = threadIdx.x; i < V; i += 256) {
            const uint64_t key = topk_key(pr[i], i);
            if (key < prev && key > best) best = key;
        }
        best = wave_max_u64(best);
        if ((threadIdx.x & 63) == 0) wmax[r & 1][wave] = best;
        __syncthreads();                                   // (double-buffered: round r + 1 writes the other half)
        uint64_t m = wmax[r & 1][0];
#pragma unroll
        for (int w = 1; w < 4; ++w) m = wmax[r & 1][w] > m ? wmax[r & 1][w] : m;
        prev = m;
        if (threadIdx.x == 0) {
            const int i = TOPK_MAX_V - 1 - (int)(m & 0xFFFF);
            index[(int64_t)row * k + r] = i;
            value[(int64_t)row * k + r] = pr[i];           // the entry itself (its NaN payload, its sign of zero)
        }
    }
}

}  // namespace lpm

extern "C" int lpm_topk_rows(const float* p, int B, int V, int k, int32_t* index, float* value, lpm_stream_t stream) {
    using namespace lpm;
    LPM_REQUIRE(p && index && value, LPM_ERR_BADARG, "lpm_topk_rows: null pointer");
    LPM_REQUIRE(B > 0 && V > 0 && k >= 1 && k <= TOPK_MAX_K && k <= V && V <= TOPK_MAX_V && B <= 0x7FFFFFFF, LPM_ERR_UNSUPPORTED_SHAPE,
                "lpm_topk_rows: need 1 <= k <= %d, k <= V <= %d (B=%d V=%d k=%d)", TOPK_MAX_K, TOPK_MAX_V, B, V, k);
    hipLaunchKernelGGL(topk_rows_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, p, V, k, index, value);
    return check_launch("lpm_topk_rows");
}
