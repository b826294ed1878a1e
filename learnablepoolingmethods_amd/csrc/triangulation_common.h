// Shared by triangulation_pool.hip, triangulation_attention.hip and triangulation_mean.hip: the lane layout of a D-vector over one wave,
// the clamped unit residual  eh = (x - a) rsqrt(max(|x - a|^2, 1e-12)), and the tile sizes, shape checks and partial-sum passes of the
// two attention-weighted poolings.
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

// ---- the two attention-weighted poolings (triangulation_attention.hip, triangulation_mean.hip) ----
constexpr int TA_MAX_FRAMES = 320;    // the backward keeps three [T, 33] tiles in LDS (135 KB at 320)
constexpr int TA_CH = 32;             // columns of D per chunk
constexpr int TA_LD = TA_CH + 1;      // LDS row stride (floats): rows 33 apart fall on different banks
constexpr int TA_WAVES = 4;
constexpr int TA_WALK_WAVES = 4;    // (clip, anchor) pairs per workgroup of the two frame walks
constexpr int TA_MAX_SLICES = 16;     // partial Grams per clip
constexpr int TA_MAX_GROUPS = 16;     // dx partials per clip: the workspace stays <= TA_MAX_GROUPS x the size of the frames
constexpr int TA_FAST_FRAMES = 64;    // ta_bwd_kernel<D, 64>, tm_bwd_kernel<D, 64>

// e[t, c] of a frame from its norm: ((x - a) iq) s, the bits tp_unit followed by the scale gives
__device__ __forceinline__ float ta_eh(float x, float a, float iq) { return (x - a) * iq; }

static int ta_tiles(int T) { return (T + 63) / 64; }
static int ta_groups(int B, int K) {                       // at most two workgroups per CU (512 in all), where the anchors allow
    int want = 512 / B;
    want = want < 1 ? 1 : (want > TA_MAX_GROUPS ? TA_MAX_GROUPS : want);
    return K < want ? K : want;
}
static int ta_check(const char* name, int B, int T, int D, int K) {
    LPM_REQUIRE(B > 0 && K > 0 && T > 0, LPM_ERR_BADARG, "%s: need B, T, K >= 1 (B=%d T=%d K=%d)", name, B, T, K);
    LPM_REQUIRE(D == 128 || D == 1024, LPM_ERR_UNSUPPORTED_SHAPE, "%s: need D in {128, 1024} (D=%d)", name, D);
    LPM_REQUIRE(T >= 2 && T <= TA_MAX_FRAMES, LPM_ERR_UNSUPPORTED_SHAPE,
                "%s: need 2 <= T <= %d frames (T=%d): the temporal embedding is a frame-to-frame difference, and the backward keeps a "
                "[T, %d] tile of each embedding in LDS", name, TA_MAX_FRAMES, T, TA_CH);
    LPM_REQUIRE((int64_t)K * D < (1ll << 31) && (int64_t)B * K * ta_tiles(T) * ta_tiles(T) < (1ll << 31), LPM_ERR_UNSUPPORTED_SHAPE,
                "%s: B * K or K * D too large (B=%d K=%d)", name, B, K);
    return LPM_OK;
}
// (defined in triangulation_attention.hip)  out[o][i] = sum_s part[o][s][i], s = 0, 1, ...
int ta_sum_slices(const float* part, int64_t outer, int64_t n, int S, float* out, hipStream_t s, const char* name);
// (likewise)  dx[b] = sum_g dx_part[b][g], g = 0, 1, ... when G > 1;  danchors[d][k] = - sum_b da_part[b][k][d], b = 0, 1, ... (two-level)
int ta_reduce_partials(const float* dx_part, const float* da_part, int B, int T, int D, int K, int G, float* dx, float* danchors,
                       hipStream_t s, const char* name);

}  // namespace lpm
