// Per-variable clip_by_norm fused with the update rules tf.train offers beside Adam (train.py:106,252,577: --optimizer), over the same
// flat parameter arena and in the same three stages as clip_adam.hip:
//   utils.clip_gradient_norms (utils.py:170-189): g *= c / max(||g||_2, c), per variable
//   GradientDescent  p -= lr g
//   Momentum         a = mu a + g;                    p -= lr a                       (no Nesterov)
//   Adagrad          a = a + g g;                     p -= lr g / sqrt(a)
//   RMSProp          s = s + (g g - s)(1 - decay);    p -= lr g / sqrt(s + eps)       (momentum 0, not centred)
//   Adadelta         a = rho a + (1 - rho) g g;  u = sqrt(d + eps) / sqrt(a + eps) g;  d = rho d + (1 - rho) u u;  p -= lr u
// Stages 1 and 2 are clip_norm.h's.  Stage 3 is ONE kernel templated on the rule: a rule streams only the arenas it keeps -- 12 bytes
// per parameter for GradientDescent, 20 with one slot, 28 with two (Adam's traffic) -- and never touches the pointers of the others.
#include "clip_norm.h"

namespace lpm {

template <int KIND> struct UpdateRule;
template <> struct UpdateRule<LPM_UPDATE_GRADIENT_DESCENT> { static constexpr int slots = 0; };
template <> struct UpdateRule<LPM_UPDATE_MOMENTUM> { static constexpr int slots = 1; };
template <> struct UpdateRule<LPM_UPDATE_ADAGRAD> { static constexpr int slots = 1; };
template <> struct UpdateRule<LPM_UPDATE_RMSPROP> { static constexpr int slots = 1; };
template <> struct UpdateRule<LPM_UPDATE_ADADELTA> { static constexpr int slots = 2; };

// One element given its CLIPPED gradient g.  adam_element's rule: every product and sum is rounded on its own, the square roots and
// the divisions are the IEEE ones -- the order of operations written here is the contract the host route (optimizers.py) restates.
// h0, h1: Momentum (mu, -), RMSProp (decay, eps), Adadelta (rho, eps); unused otherwise.
template <int KIND>
__device__ __forceinline__ void update_element(float g, float& p, float& s0, float& s1, float lr, float h0, float h1) {
#pragma clang fp contract(off)
    if constexpr (KIND == LPM_UPDATE_GRADIENT_DESCENT) {
        p = p - lr * g;
    } else if constexpr (KIND == LPM_UPDATE_MOMENTUM) {
        s0 = h0 * s0 + g;
        p = p - lr * s0;
    } else if constexpr (KIND == LPM_UPDATE_ADAGRAD) {
        s0 = s0 + g * g;
        p = p - lr * g / sqrtf(s0);
    } else if constexpr (KIND == LPM_UPDATE_RMSPROP) {
        s0 = s0 + (g * g - s0) * (1.f - h0);
        p = p - lr * g / sqrtf(s0 + h1);
    } else {
        s0 = h0 * s0 + (1.f - h0) * g * g;
        const float u = sqrtf(s1 + h1) / sqrtf(s0 + h1) * g;
        s1 = h0 * s1 + (1.f - h0) * u * u;
        p = p - lr * u;
    }
}

__device__ __forceinline__ float4 cu_load(const float* a) {
    const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(a));
    return make_float4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ void cu_store(float* a, const float4& v) {
    __builtin_nontemporal_store(f32x4{v.x, v.y, v.z, v.w}, reinterpret_cast<f32x4*>(a));
}

// every byte of the arenas a rule keeps is touched once per step and not again before the next one: non-temporal, as ca_apply_kernel
template <int KIND>
__global__ __launch_bounds__(256) void cu_apply_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ s0,
                                                       float* __restrict__ s1, const int64_t* __restrict__ offsets, int ntensors,
                                                       int64_t total, const float* __restrict__ factor, float lr, float h0, float h1,
                                                       const float* __restrict__ l2) {
    constexpr int NS = UpdateRule<KIND>::slots;
    const int64_t base = (int64_t)blockIdx.x * CA_CHUNK;
    const int lo = ca_owner(offsets, ntensors, base);
    const float f = factor[lo];
    const float c2 = l2 ? l2[lo] : 0.f;
#pragma unroll
    for (int i = 0; i < CA_CHUNK / (256 * 4); ++i) {
        const int64_t e = base + (int64_t)(i * 256 + threadIdx.x) * 4;
        if (e + 3 < total) {
            float4 pp = cu_load(p + e), gg = cu_load(g + e);
            float4 aa = make_float4(0.f, 0.f, 0.f, 0.f), bb = aa;
            if constexpr (NS >= 1) aa = cu_load(s0 + e);
            if constexpr (NS >= 2) bb = cu_load(s1 + e);
            if (c2 != 0.f) {                 // + the L2 penalty's gradient (the same fmaf as the norm pass)
                gg.x = fmaf(c2, pp.x, gg.x); gg.y = fmaf(c2, pp.y, gg.y); gg.z = fmaf(c2, pp.z, gg.z); gg.w = fmaf(c2, pp.w, gg.w);
            }
#define LPM_UPDATE1(c) update_element<KIND>(gg.c * f, pp.c, aa.c, bb.c, lr, h0, h1);
            LPM_UPDATE1(x) LPM_UPDATE1(y) LPM_UPDATE1(z) LPM_UPDATE1(w)
#undef LPM_UPDATE1
            cu_store(p + e, pp);
            if constexpr (NS >= 1) cu_store(s0 + e, aa);
            if constexpr (NS >= 2) cu_store(s1 + e, bb);
        }
    }
}

template <int KIND>
static void cu_launch_apply(hipStream_t s, int64_t nchunk, float* param, const float* grad, float* slot0, float* slot1,
                            const int64_t* offsets, int ntensors, int64_t total, const float* factor, float lr, float h0, float h1,
                            const float* l2coef) {
    hipLaunchKernelGGL(cu_apply_kernel<KIND>, dim3((unsigned)nchunk), dim3(256), 0, s, param, grad, slot0, slot1, offsets, ntensors, total,
                       factor, lr, h0, h1, l2coef);
}

}  // namespace lpm

extern "C" int lpm_multi_tensor_clip_update(int kind, float* param, const float* grad, float* slot0, float* slot1, const int64_t* offsets,
                                            const float* l2coef, int ntensors, int64_t total, float clip_norm, float lr, float h0, float h1,
                                            float* scratch, lpm_stream_t stream) {
    using namespace lpm;
    int slots;
    switch (kind) {
        case LPM_UPDATE_GRADIENT_DESCENT: slots = 0; break;
        case LPM_UPDATE_MOMENTUM: case LPM_UPDATE_ADAGRAD: case LPM_UPDATE_RMSPROP: slots = 1; break;
        case LPM_UPDATE_ADADELTA: slots = 2; break;
        default:
            set_error("lpm_multi_tensor_clip_update: unknown kind %d", kind);
            return LPM_ERR_BADARG;
    }
    LPM_REQUIRE(param && grad && offsets && scratch, LPM_ERR_BADARG, "lpm_multi_tensor_clip_update: null pointer");
    LPM_REQUIRE((slots < 1 || slot0) && (slots < 2 || slot1), LPM_ERR_BADARG,
                "lpm_multi_tensor_clip_update: kind %d keeps %d slot arena(s) and got a null pointer for one of them", kind, slots);
    LPM_REQUIRE(ntensors > 0 && total > 0, LPM_ERR_BADARG, "lpm_multi_tensor_clip_update: bad sizes");
    LPM_REQUIRE(total % 4 == 0, LPM_ERR_UNSUPPORTED_SHAPE, "lpm_multi_tensor_clip_update: arena length must be a multiple of 4");
    // (a slot the rule does not keep is never looked at: not even its alignment)
    const uintptr_t used = (uintptr_t)param | (uintptr_t)grad | (slots >= 1 ? (uintptr_t)slot0 : 0) | (slots >= 2 ? (uintptr_t)slot1 : 0);
    LPM_REQUIRE((used & 15) == 0, LPM_ERR_BADARG, "lpm_multi_tensor_clip_update: arenas must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int64_t nchunk = (total + CA_CHUNK - 1) / CA_CHUNK;
    float* chunk_ss = scratch;
    float* factor = scratch + nchunk;
    hipLaunchKernelGGL(ca_chunk_sumsq_kernel, dim3((unsigned)nchunk), dim3(256), 0, s, grad, total, chunk_ss, (const float*)param, offsets, ntensors,
                       l2coef);
    hipLaunchKernelGGL(ca_tensor_factor_kernel, dim3(ntensors), dim3(1024), 0, s, chunk_ss, offsets, clip_norm, factor);
#define LPM_APPLY(K) cu_launch_apply<K>(s, nchunk, param, grad, slot0, slot1, offsets, ntensors, total, factor, lr, h0, h1, l2coef)
    switch (kind) {
        case LPM_UPDATE_GRADIENT_DESCENT: LPM_APPLY(LPM_UPDATE_GRADIENT_DESCENT); break;
        case LPM_UPDATE_MOMENTUM: LPM_APPLY(LPM_UPDATE_MOMENTUM); break;
        case LPM_UPDATE_ADAGRAD: LPM_APPLY(LPM_UPDATE_ADAGRAD); break;
        case LPM_UPDATE_RMSPROP: LPM_APPLY(LPM_UPDATE_RMSPROP); break;
        default: LPM_APPLY(LPM_UPDATE_ADADELTA); break;
    }
#undef LPM_APPLY
    return check_launch("lpm_multi_tensor_clip_update");
}
