// Triangulation-embedding pooling (video_pooling_modules.py:1395-1497 WeightedTriangulationEmbedding + TriangulationTemporalEmbedding,
// aggregation_modules.py MaxMeanPoolingModule), fused: the four pooled [B, K*D] vectors of a stream straight from the frames.
//   r = x[b,t,:] - anchors[:,k];  e = s r rsqrt(max(|r|^2, 1e-12));  u = e_t - e_{t-1};  f = u rsqrt(max(|u|^2, 1e-12))   (t >= 1)
//   max_d / mean_d = max_t / mean_t of e over t = 0..T-1;   max_t / mean_t = the same of f over t = 1..T-1
// The reference tiles every frame against every anchor and keeps [B, T, K*D] tensors (79 MB per clip at T = 300, K = 64, D = 1024)
// through both normalisations and the pooling; here nothing of size T*K*D exists in either direction.
//
// Forward: tp_walk_fwd_kernel<D, no weights, maxima> (triangulation_common.h: the walk, its two-level sums and first-index maxima, and
// the contraction rule -- s eh is rounded before the difference u is taken, as the backward below forms u = s (eh_t - eh_{t-1})).
//
// Backward: the same ownership, t walked DOWNWARDS so that gu_{t+1} is at hand; e, u, f are recomputed from the frames.
//   gf_t = g_mean_t / (T-1) + [t = argmax_t] g_max_t                         gu_t = ip (gf_t - f_t (f_t . gf_t) [p > 1e-12])
//   ge_t = g_mean_d / T + [t = argmax_d] g_max_d + gu_t - gu_{t+1}            gr_t = s iq (ge_t - eh_t (eh_t . ge_t) [q > 1e-12])
// with eh = r iq (so e = s eh: r (r . ge) iq^3 = iq eh (eh . ge)).  dx[b,t,:] = sum_k gr_t in a FIXED order: the TP_BWD_WAVES waves
// of a workgroup (eight anchors of one clip, in lockstep on t) meet through LDS once per frame and are added wave 0, 1, ...; a
// workgroup takes its clip's anchor rounds g, g + G, ... in turn and adds each round onto what it wrote itself; G > 1 groups per
// clip (small batches: B * G >= 256 workgroups where K allows) write partials that a second pass adds g = 0, 1, ....
// danchors[:,k] = - sum_{b,t} gr_t: per-(clip, anchor) sums over t in registers, clips added b = 0, 1, ... by a second pass.
// No floating-point atomics anywhere: the same inputs give the same bits.
#include "triangulation_common.h"

namespace lpm {

constexpr int TP_BWD_WAVES = 8;
constexpr int TP_MAX_GROUPS = 8;      // dx partials per clip: the workspace stays <= TP_MAX_GROUPS x the size of the frames
constexpr int TP_MAX_FRAMES = 32767;  // the arg-max indices are an int16 pair

template <int D>
__global__ __launch_bounds__(64 * TP_BWD_WAVES) void tp_bwd_kernel(const float* __restrict__ x, const float* __restrict__ anchors,
                                                                   const int* __restrict__ argmax, const float* __restrict__ g_max_d,
                                                                   const float* __restrict__ g_mean_d, const float* __restrict__ g_max_t,
                                                                   const float* __restrict__ g_mean_t, int T, int K, float s, int G,
                                                                   float* __restrict__ dx_part, float* __restrict__ da_part) {
    constexpr int N = TpVec<D>::N, W = TP_BWD_WAVES;
    // LDS: the waves' gr_t of one frame, double-buffered (one barrier per frame), and behind them each wave's own rows of the two
    // max gradients (read back every frame: 32 registers less, which is what keeps D = 1024 inside two waves per SIMD)
    extern __shared__ __attribute__((aligned(16))) float tp_sh[];
    float (*gr_sh)[W][D] = reinterpret_cast<float (*)[W][D]>(tp_sh);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.x / G, g = blockIdx.x % G;
    const float* xb = x + (int64_t)b * T * D;
    float* dxo = dx_part + ((int64_t)b * G + g) * T * D;   // this workgroup's own [T, D] block (dx itself when G == 1)
    const int rounds = (K + W - 1) / W;
    const float inv_d = 1.f / (float)T, inv_t = 1.f / (float)(T - 1);
    float* gxd = tp_sh + (2 * W + 2 * wave) * D;
    float* gxt = gxd + D;
    int buf = 0;
    for (int r = g; r < rounds; r += G) {
        const bool first = r == g;
        const int nact = min(W, K - r * W), k = r * W + wave;
        const bool act = wave < nact;                      // (wave-uniform)
        float a[N], gmd[N], gmt[N], eh[N], gun[N], da[N];
        int idx[N];
        float iq = 0.f;
        bool qc = true;
        if (act) {
            const int64_t o = ((int64_t)b * K + k) * D;
            tp_load_anchor<D>(anchors, K, k, lane, a);
            tp_load<D>(g_mean_d + o, lane, gmd);
            tp_load<D>(g_mean_t + o, lane, gmt);
            {
                float v[N];
                tp_load<D>(g_max_d + o, lane, v);
                tp_store<D>(gxd, lane, v);
                tp_load<D>(g_max_t + o, lane, v);
                tp_store<D>(gxt, lane, v);
            }
            tp_load<D>(argmax + o, lane, idx);
            float xl[N];
            tp_load<D>(xb + (int64_t)(T - 1) * D, lane, xl);
            iq = tp_unit<N>(xl, a, eh, qc);
#pragma unroll
            for (int j = 0; j < N; ++j) {
                gmd[j] *= inv_d;
                gmt[j] *= inv_t;
                gun[j] = da[j] = 0.f;
            }
        }
        for (int t = T - 1; t >= 0; --t) {
            if (act) {
                float gu[N], ehp[N], iqp = 0.f;
                bool qcp = true;
                if (t >= 1) {
                    float xc[N];
                    tp_load<D>(xb + (int64_t)(t - 1) * D, lane, xc);
                    iqp = tp_unit<N>(xc, a, ehp, qcp);
                    float p = 0.f;
#pragma unroll
                    for (int j = 0; j < N; ++j) {
                        gu[j] = s * (eh[j] - ehp[j]);                        // u_t
                        p = fmaf(gu[j], gu[j], p);
                    }
                    p = wave_sum_dpp(p);
                    const float ip = rsqrtf(fmaxf(p, kL2Eps));
                    float dot = 0.f, gf[N];
                    tp_load<D>(gxt, lane, gf);
#pragma unroll
                    for (int j = 0; j < N; ++j) {
                        gu[j] *= ip;                                         // f_t
                        gf[j] = gmt[j] + (((idx[j] >> 16) & 0xffff) == t ? gf[j] : 0.f);
                        dot = fmaf(gu[j], gf[j], dot);
                    }
                    dot = p > kL2Eps ? wave_sum_dpp(dot) : 0.f;
#pragma unroll
                    for (int j = 0; j < N; ++j) gu[j] = ip * (gf[j] - gu[j] * dot);
                } else {
#pragma unroll
                    for (int j = 0; j < N; ++j) gu[j] = ehp[j] = 0.f;
                }
                float ge[N], dot2 = 0.f;
                tp_load<D>(gxd, lane, ge);
#pragma unroll
                for (int j = 0; j < N; ++j) {
                    ge[j] = gmd[j] + ((idx[j] & 0xffff) == t ? ge[j] : 0.f) + gu[j] - gun[j];
                    dot2 = fmaf(eh[j], ge[j], dot2);
                }
                dot2 = qc ? 0.f : wave_sum_dpp(dot2);
                const float c = s * iq;
#pragma unroll
                for (int j = 0; j < N; ++j) {
                    ge[j] = c * (ge[j] - eh[j] * dot2);                      // gr_t
                    da[j] += ge[j];
                    gun[j] = gu[j];
                    eh[j] = ehp[j];
                }
                iq = iqp;
                qc = qcp;
                tp_store<D>(&gr_sh[buf][wave][0], lane, ge);
            }
            __syncthreads();
            for (int d2 = threadIdx.x; d2 < D / 2; d2 += 64 * W) {
                float2 acc = reinterpret_cast<const float2*>(&gr_sh[buf][0][0])[d2];
                for (int w = 1; w < nact; ++w) {
                    const float2 v = reinterpret_cast<const float2*>(&gr_sh[buf][w][0])[d2];
                    acc.x += v.x;
                    acc.y += v.y;
                }
                float2* o = reinterpret_cast<float2*>(dxo + (int64_t)t * D) + d2;
                if (!first) {                                                // an earlier round of this workgroup: this thread wrote it
                    const float2 v = *o;
                    acc.x += v.x;
                    acc.y += v.y;
                }
                *o = acc;
            }
            buf ^= 1;
        }
        if (act) tp_store<D>(da_part + ((int64_t)b * K + k) * D, lane, da);
    }
}

static int tp_groups(int B, int K) {
    const int rounds = (K + TP_BWD_WAVES - 1) / TP_BWD_WAVES;
    int want = (256 + B - 1) / B;
    want = want < 1 ? 1 : (want > TP_MAX_GROUPS ? TP_MAX_GROUPS : want);
    return rounds < want ? rounds : want;
}

static int tp_pool_check(const char* name, int B, int T, int D, int K) {
    return tp_check(name, B, T, D, K, TP_MAX_FRAMES, "", (K + TP_WALK_WAVES - 1) / TP_WALK_WAVES);
}

}  // namespace lpm

extern "C" size_t lpm_triangulation_pool_workspace_bytes(int B, int T, int D, int K) {
    if (B <= 0 || T <= 0 || D <= 0 || K <= 0) return 0;
    const int G = lpm::tp_groups(B, K);
    return ((size_t)B * K * D + (G > 1 ? (size_t)B * G * T * D : 0)) * sizeof(float);
}

extern "C" int lpm_triangulation_pool_fwd(const float* x, const float* anchors, int B, int T, int D, int K, float scale, float* max_d,
                                          float* mean_d, float* max_t, float* mean_t, int32_t* argmax, lpm_stream_t stream) {
    using namespace lpm;
    LPM_REQUIRE(x && anchors && max_d && mean_d && max_t && mean_t && argmax, LPM_ERR_BADARG, "lpm_triangulation_pool_fwd: null pointer");
    if (const int rc = tp_pool_check("lpm_triangulation_pool_fwd", B, T, D, K)) return rc;
    LPM_REQUIRE((((uintptr_t)x | (uintptr_t)max_d | (uintptr_t)mean_d | (uintptr_t)max_t | (uintptr_t)mean_t | (uintptr_t)argmax) & 15) == 0,
                LPM_ERR_BADARG, "lpm_triangulation_pool_fwd: x and the outputs must be 16-byte aligned");
    tp_dispatch_d(D, [&](auto d) {
        hipLaunchKernelGGL((tp_walk_fwd_kernel<decltype(d)::value, false, false, true>), dim3(tp_walk_grid(B, K)), dim3(64 * TP_WALK_WAVES), 0,
                           (hipStream_t)stream, x, anchors, nullptr, nullptr, T, K, scale, mean_d, max_d, mean_t, max_t, argmax);
    });
    return check_launch("lpm_triangulation_pool_fwd");
}

extern "C" int lpm_triangulation_pool_bwd(const float* x, const float* anchors, const int32_t* argmax, const float* g_max_d,
                                          const float* g_mean_d, const float* g_max_t, const float* g_mean_t, int B, int T, int D, int K,
                                          float scale, float* dx, float* danchors, void* workspace, size_t workspace_bytes,
                                          lpm_stream_t stream) {
    using namespace lpm;
    LPM_REQUIRE(x && anchors && argmax && g_max_d && g_mean_d && g_max_t && g_mean_t && dx && danchors, LPM_ERR_BADARG,
                "lpm_triangulation_pool_bwd: null pointer");
    if (const int rc = tp_pool_check("lpm_triangulation_pool_bwd", B, T, D, K)) return rc;
    LPM_REQUIRE(workspace && workspace_bytes >= lpm_triangulation_pool_workspace_bytes(B, T, D, K), LPM_ERR_WORKSPACE,
                "lpm_triangulation_pool_bwd: workspace too small");
    LPM_REQUIRE((((uintptr_t)x | (uintptr_t)argmax | (uintptr_t)g_max_d | (uintptr_t)g_mean_d | (uintptr_t)g_max_t | (uintptr_t)g_mean_t |
                  (uintptr_t)dx | (uintptr_t)workspace) & 15) == 0,
                LPM_ERR_BADARG, "lpm_triangulation_pool_bwd: x, the saved indices, the gradients, dx and the workspace must be 16-byte aligned");
    const int G = tp_groups(B, K);
    LPM_REQUIRE((int64_t)B * G < (1ll << 31), LPM_ERR_UNSUPPORTED_SHAPE, "lpm_triangulation_pool_bwd: batch too large (B=%d)", B);
    float* da_part = (float*)workspace;
    float* dx_part = G > 1 ? da_part + (size_t)B * K * D : dx;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(B * G), block(64 * TP_BWD_WAVES);
    const size_t lds = (size_t)4 * TP_BWD_WAVES * D * sizeof(float);       // 128 KB at D = 1024
    if (const int rc = tp_reserve_lds<tp_bwd_kernel<1024>>("lpm_triangulation_pool_bwd", 4 * TP_BWD_WAVES * 1024 * (int)sizeof(float))) return rc;
    tp_dispatch_d(D, [&](auto d) {
        hipLaunchKernelGGL(tp_bwd_kernel<decltype(d)::value>, grid, block, lds, s, x, anchors, argmax, g_max_d, g_mean_d, g_max_t, g_mean_t, T, K,
                           scale, G, dx_part, da_part);
    });
    // (clips added b = 0, 1, ... in one level)
    if (const int rc = ta_reduce_partials(dx_part, da_part, B, T, D, K, G, B, dx, danchors, s, "lpm_triangulation_pool_bwd")) return rc;
    return check_launch("lpm_triangulation_pool_bwd");
}
