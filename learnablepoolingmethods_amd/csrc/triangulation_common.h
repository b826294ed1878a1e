// Device helpers shared by triangulation_pool.hip and triangulation_attention.hip: the lane layout of a D-vector over one wave and the
// clamped unit residual  eh = (x - a) rsqrt(max(|x - a|^2, 1e-12)).
#pragma once
#include "lpm_common.h"

namespace lpm {

constexpr int TP_SUM_CHUNK = 32;      // two-level sums over t: this many frames into a partial, partials into the total

// lane layout of a D-vector: register j of lane l holds element (j / V * 64 + l) * V + j % V -- V-wide (16 / 8 byte) accesses
template <int D> struct TpVec { static constexpr int V = D >= 256 ? 4 : 2, N = D / 64, C = N / V; };

template <int D, typename T>
__device__ __forceinline__ void tp_load(const T* __restrict__ row, int lane, T (&v)[D / 64]) {
    constexpr int V = TpVec<D>::V, C = TpVec<D>::C;
    typedef T vec __attribute__((ext_vector_type(V)));
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const vec t = *reinterpret_cast<const vec*>(row + (c * 64 + lane) * V);
#pragma unroll
        for (int i = 0; i < V; ++i) v[c * V + i] = t[i];
    }
}
template <int D, typename T>
__device__ __forceinline__ void tp_store(T* __restrict__ row, int lane, const T (&v)[D / 64]) {
    constexpr int V = TpVec<D>::V, C = TpVec<D>::C;
    typedef T vec __attribute__((ext_vector_type(V)));
#pragma unroll
    for (int c = 0; c < C; ++c) {
        vec t;
#pragma unroll
        for (int i = 0; i < V; ++i) t[i] = v[c * V + i];
        *reinterpret_cast<vec*>(row + (c * 64 + lane) * V) = t;
    }
}
// column k of the [D, K] anchor variable in the lane layout
template <int D>
__device__ __forceinline__ void tp_load_anchor(const float* __restrict__ anchors, int K, int k, int lane, float (&a)[D / 64]) {
    constexpr int V = TpVec<D>::V, N = TpVec<D>::N;
#pragma unroll
    for (int j = 0; j < N; ++j) a[j] = anchors[(int64_t)((j / V * 64 + lane) * V + j % V) * K + k];
}
// eh = (x - a) rsqrt(max(|x - a|^2, eps)); returns the factor, `clamped` = the squared norm did not exceed eps
template <int N>
__device__ __forceinline__ float tp_unit(const float (&x)[N], const float (&a)[N], float (&eh)[N], bool& clamped) {
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        eh[j] = x[j] - a[j];
        q = fmaf(eh[j], eh[j], q);
    }
    q = wave_sum_dpp(q);
    clamped = !(q > kL2Eps);
    const float iq = rsqrtf(fmaxf(q, kL2Eps));
#pragma unroll
    for (int j = 0; j < N; ++j) eh[j] *= iq;
    return iq;
}

}  // namespace lpm
