// Shared by the five triangulation_*.hip files, each fact once: the lane layout of a D-vector over one wave, the clamped unit residual
//   eh = (x - a) rsqrt(max(|x - a|^2, 1e-12)),
// the frame walks (one wave per (clip, anchor): the forward of the three poolings, dw of the two attention-weighted ones), the per-frame
// norm pass of the Gram and backward kernels, and the host helpers (D dispatch, dynamic LDS, shape refusals, partial-sum passes).
//
// THE CONTRACTION RULE.  u = e_t - e_{t-1} must be exactly zero for identical frames, and every kernel that rebuilds e = (eh s) or
// f = u ip must round as the walk does: no product may be fused into a sum or a difference (neither s eh into u or into the sum of e,
// nor u ip into the sum of f).  The .hip files turn contraction off
// for the whole file BELOW this include, so whatever forms e, u or f in this header carries the pragma inside its own body.
#pragma once
#include "lpm_common.h"
#include <type_traits>

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

// ---- the frame walks: ONE WAVE owns a (clip, anchor) pair and walks t -------------------------------------------------------------
constexpr int TP_WALK_WAVES = 4;      // (clip, anchor) pairs per workgroup
static int tp_walk_grid(int B, int K) { return B * ((K + TP_WALK_WAVES - 1) / TP_WALK_WAVES); }

// The forward of triangulation_pool / _attention / _mean:  e_t = eh_t s,  u_t = e_t - e_{t-1},  f_t = u_t rsqrt(max(|u_t|^2, 1e-12));
//   mean_e = (1/T) sum_t [w_e[b,t]] e_t      mean_f = (1/(T-1)) sum_{t>=1} [w_f[b,t-1]] f_t      (WE / WF: with the weight)
//   max_e, max_f and the packed indices (MAXIMA): the FIRST frame that attains the maximum (strict > walking t upwards); the int16 pair
//   (low: e, high: f) per element is what a backward gets -- exact ties cannot be re-matched walking t downwards.
// D = 1024 is 16 elements per lane: the anchor, the previous e, the sums, the maxima and the indices stay in registers; |r|^2 and |u|^2
// are wave reductions on the VALU (wave_sum_dpp: every lane gets the same bits).  The sums over t are two-level (TP_SUM_CHUNK frames
// into a partial, partials into the total): mean_e's terms share a sign (the anchor's direction), so a plain running sum rounds every
// term to the ulp of a total that keeps growing.  An unweighted term is a plain add, a weighted one the explicit fmaf(w, v, part).
template <int D, bool WE, bool WF, bool MAXIMA>
__global__ __launch_bounds__(64 * TP_WALK_WAVES) void tp_walk_fwd_kernel(const float* __restrict__ x, const float* __restrict__ anchors,
                                                                         const float* __restrict__ w_e, const float* __restrict__ w_f, int T, int K,
                                                                         float s, float* __restrict__ mean_e, float* __restrict__ max_e,
                                                                         float* __restrict__ mean_f, float* __restrict__ max_f,
                                                                         int* __restrict__ argmax) {
#pragma clang fp contract(off)
    constexpr int N = TpVec<D>::N;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int kg = (K + TP_WALK_WAVES - 1) / TP_WALK_WAVES;
    const int b = blockIdx.x / kg, k = (blockIdx.x % kg) * TP_WALK_WAVES + wave;
    if (k >= K) return;                                   // (no barrier in this kernel)
    float a[N], ep[N], tot_e[N], part_e[N], mx_e[N], tot_f[N], part_f[N], mx_f[N];
    int idx[N];
    tp_load_anchor<D>(anchors, K, k, lane, a);
#pragma unroll
    for (int j = 0; j < N; ++j) {
        ep[j] = 0.f;
        tot_e[j] = part_e[j] = tot_f[j] = part_f[j] = 0.f;
        mx_e[j] = mx_f[j] = -INFINITY;
        idx[j] = 0;
    }
    const float* xb = x + (int64_t)b * T * D;
    const float* we = WE ? w_e + (int64_t)b * T : nullptr;
    const float* wf = WF ? w_f + (int64_t)b * (T - 1) : nullptr;
    float xv[N], xn[N];
    tp_load<D>(xb, lane, xv);
    for (int t = 0; t < T; ++t) {
        tp_load<D>(xb + (int64_t)min(t + 1, T - 1) * D, lane, xn);          // the next frame is under way while this one is worked on
        float e[N];
        bool clamped;
        tp_unit<N>(xv, a, e, clamped);
        const float wet = WE ? we[t] : 1.f;
#pragma unroll
        for (int j = 0; j < N; ++j) {
            e[j] *= s;
            part_e[j] = WE ? fmaf(wet, e[j], part_e[j]) : part_e[j] + e[j];
            if (MAXIMA) {
                const bool up = e[j] > mx_e[j];
                mx_e[j] = up ? e[j] : mx_e[j];
                idx[j] = up ? ((idx[j] & (int)0xffff0000u) | t) : idx[j];
            }
        }
        if (t > 0) {
            float u[N], p = 0.f;
#pragma unroll
            for (int j = 0; j < N; ++j) {
                u[j] = e[j] - ep[j];
                p = fmaf(u[j], u[j], p);
            }
            p = wave_sum_dpp(p);
            const float ip = rsqrtf(fmaxf(p, kL2Eps)), wft = WF ? wf[t - 1] : 1.f;
#pragma unroll
            for (int j = 0; j < N; ++j) {
                const float f = u[j] * ip;
                part_f[j] = WF ? fmaf(wft, f, part_f[j]) : part_f[j] + f;
                if (MAXIMA) {
                    const bool up = f > mx_f[j];
                    mx_f[j] = up ? f : mx_f[j];
                    idx[j] = up ? ((idx[j] & 0xffff) | (t << 16)) : idx[j];
                }
            }
        }
        if ((t & (TP_SUM_CHUNK - 1)) == TP_SUM_CHUNK - 1) {
#pragma unroll
            for (int j = 0; j < N; ++j) {
                tot_e[j] += part_e[j];
                tot_f[j] += part_f[j];
                part_e[j] = part_f[j] = 0.f;
            }
        }
#pragma unroll
        for (int j = 0; j < N; ++j) {
            ep[j] = e[j];
            xv[j] = xn[j];
        }
    }
    const float nd = (float)T, nt = (float)(T - 1);
#pragma unroll
    for (int j = 0; j < N; ++j) {
        tot_e[j] = (tot_e[j] + part_e[j]) / nd;
        tot_f[j] = (tot_f[j] + part_f[j]) / nt;
    }
    const int64_t o = ((int64_t)b * K + k) * D;             // k-major: element k * D + d
    tp_store<D>(mean_e + o, lane, tot_e);
    tp_store<D>(mean_f + o, lane, tot_f);
    if (MAXIMA) {
        tp_store<D>(max_e + o, lane, mx_e);
        tp_store<D>(max_f + o, lane, mx_f);
        tp_store<D>(argmax + o, lane, idx);
    }
}

// The same walk for dw of the weighted means: part_e[b][k][t] = <g_e[b, k, :], e_t> / T and (TEMPORAL)
// part_f[b][k][t-1] = <g_f[b, k, :], f_t> / (T - 1); the caller adds the anchors k = 0, 1, ... (ta_sum_slices)
template <int D, bool TEMPORAL>
__global__ __launch_bounds__(64 * TP_WALK_WAVES) void tp_walk_dw_kernel(const float* __restrict__ x, const float* __restrict__ anchors,
                                                                        const float* __restrict__ g_e, int T, int K, float s,
                                                                        float* __restrict__ part_e, const float* __restrict__ g_f,
                                                                        float* __restrict__ part_f) {
#pragma clang fp contract(off)
    constexpr int N = TpVec<D>::N;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int kg = (K + TP_WALK_WAVES - 1) / TP_WALK_WAVES;
    const int b = blockIdx.x / kg, k = (blockIdx.x % kg) * TP_WALK_WAVES + wave;
    if (k >= K) return;                                   // (no barrier in this kernel)
    float a[N], ep[N], ge[N], gf[N];
    tp_load_anchor<D>(anchors, K, k, lane, a);
    tp_load<D>(g_e + ((int64_t)b * K + k) * D, lane, ge);
    if (TEMPORAL) tp_load<D>(g_f + ((int64_t)b * K + k) * D, lane, gf);
#pragma unroll
    for (int j = 0; j < N; ++j) ep[j] = 0.f;
    const float* xb = x + (int64_t)b * T * D;
    float* oe = part_e + ((int64_t)b * K + k) * T;
    float* of = TEMPORAL ? part_f + ((int64_t)b * K + k) * (T - 1) : nullptr;
    const float inv_e = 1.f / (float)T, inv_f = 1.f / (float)(T - 1);
    for (int t = 0; t < T; ++t) {
        float xv[N], e[N], dot = 0.f;
        bool clamped;
        tp_load<D>(xb + (int64_t)t * D, lane, xv);
        tp_unit<N>(xv, a, e, clamped);
#pragma unroll
        for (int j = 0; j < N; ++j) {
            e[j] *= s;
            dot = fmaf(e[j], ge[j], dot);
        }
        dot = wave_sum_dpp(dot);
        if (lane == 0) oe[t] = dot * inv_e;
        if (TEMPORAL && t > 0) {
            float u[N], p = 0.f, dt = 0.f;
#pragma unroll
            for (int j = 0; j < N; ++j) {
                u[j] = e[j] - ep[j];
                p = fmaf(u[j], u[j], p);
            }
            p = wave_sum_dpp(p);
            const float ip = rsqrtf(fmaxf(p, kL2Eps));
#pragma unroll
            for (int j = 0; j < N; ++j) dt = fmaf(u[j] * ip, gf[j], dt);
            dt = wave_sum_dpp(dt);
            if (lane == 0) of[t - 1] = dt * inv_f;
        }
#pragma unroll
        for (int j = 0; j < N; ++j) ep[j] = e[j];
    }
}

// ---- the Gram and backward kernels of the attention-weighted poolings (triangulation_attention.hip, _mean.hip; tiles: _moments, _bn_moments) ----
constexpr int TA_MAX_FRAMES = 320;    // the backward keeps three [T, 33] tiles in LDS (135 KB at 320)
constexpr int TA_CH = 32;             // columns of D per chunk
constexpr int TA_LD = TA_CH + 1;      // LDS row stride (floats): rows 33 apart fall on different banks
constexpr int TA_WAVES = 4;
constexpr int TA_MAX_SLICES = 16;     // partial Grams per clip
constexpr int TA_MAX_GROUPS = 16;     // dx partials per clip: the workspace stays <= TA_MAX_GROUPS x the size of the frames
constexpr int TA_FAST_FRAMES = 64;    // ta_bwd_kernel<D, 64>, tm_bwd_kernel<D, 64>

// e[t, c] of a frame from its norm: ((x - a) iq) s, the bits tp_unit followed by the scale gives
__device__ __forceinline__ float ta_eh(float x, float a, float iq) { return (x - a) * iq; }
// e[t, c] from the chunk's frames in LDS; 0 for t >= T (iq = 0 there)
__device__ __forceinline__ float ta_e(const float (*tX)[TA_LD], const float* iq, int t, int c, float av, float s) {
#pragma clang fp contract(off)
    return ta_eh(tX[t][c], av, iq[t]) * s;
}

// The per-frame pass of one (clip, anchor) over whole rows, one wave per frame; a (anchor) in the lane layout.  Entry i belongs to frame
// f0 + i, i < n; frames outside [0, T) get zeros (f0 = -1 in the Gram: f of a tile's first frame needs e of the frame before it).
//   iq = rsqrt(max(|x - a|^2, eps))                                                        always
//   ip = the same of u = e_t - e_{t-1}                                                     TN_TEMPORAL
//   qg / pg = 1 where the squared norm exceeded eps, else 0                                TN_GATES
//   dotf = (f_t . gf), gf[D / 64] in the lane layout                                            TN_DOTF (with TN_TEMPORAL)
// What WHAT leaves out is neither computed nor stored, and its pointer is not read (pass nullptr).
enum { TN_TEMPORAL = 1, TN_GATES = 2, TN_DOTF = 4 };
template <int D, int WHAT>
__device__ __forceinline__ void ta_norms(const float* __restrict__ xb, const float (&a)[D / 64], const float* gf, int T, int f0, int n,
                                         float s, float* iq, float* qg, float* ip, float* pg, float* dotf) {
#pragma clang fp contract(off)
    constexpr int N = TpVec<D>::N;
    static_assert(!(WHAT & TN_DOTF) || (WHAT & TN_TEMPORAL), "(f . gf) needs the temporal half");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i = wave; i < n; i += TA_WAVES) {
        const int t = f0 + i;
        float viq = 0.f, vqg = 0.f, vip = 0.f, vpg = 0.f, vdf = 0.f;
        if (t >= 0 && t < T) {                              // (wave-uniform)
            float xv[N], e[N];
            bool c;
            tp_load<D>(xb + (int64_t)t * D, lane, xv);
            viq = tp_unit<N>(xv, a, e, c);
            vqg = c ? 0.f : 1.f;
            if ((WHAT & TN_TEMPORAL) && t >= 1) {
                float ep[N], u[N], p = 0.f;
                bool c2;
                tp_load<D>(xb + (int64_t)(t - 1) * D, lane, xv);
                tp_unit<N>(xv, a, ep, c2);
#pragma unroll
                for (int j = 0; j < N; ++j) {
                    u[j] = e[j] * s - ep[j] * s;
                    p = fmaf(u[j], u[j], p);
                }
                p = wave_sum_dpp(p);
                vip = rsqrtf(fmaxf(p, kL2Eps));
                vpg = p > kL2Eps ? 1.f : 0.f;
                if (WHAT & TN_DOTF) {
#pragma unroll
                    for (int j = 0; j < N; ++j) vdf = fmaf(u[j] * vip, gf[j], vdf);
                    vdf = wave_sum_dpp(vdf);
                }
            }
        }
        if (lane == 0) {
            iq[i] = viq;
            if (WHAT & TN_TEMPORAL) ip[i] = vip;
            if (WHAT & TN_GATES) qg[i] = vqg;
            if ((WHAT & TN_GATES) && (WHAT & TN_TEMPORAL)) pg[i] = vpg;
            if (WHAT & TN_DOTF) dotf[i] = vdf;
        }
    }
}

static int ta_tiles(int T) { return (T + 63) / 64; }
static int ta_groups(int B, int K) {                       // at most two workgroups per CU (512 in all), where the anchors allow
    int want = 512 / B;
    want = want < 1 ? 1 : (want > TA_MAX_GROUPS ? TA_MAX_GROUPS : want);
    return K < want ? K : want;
}

// ---- host helpers -----------------------------------------------------------------------------------------------------------------
// f(std::integral_constant<int, D>) with D, one of the two supported widths, as a compile-time constant
template <typename F>
static void tp_dispatch_d(int D, F&& f) {
    if (D == 1024) f(std::integral_constant<int, 1024>{}); else f(std::integral_constant<int, 128>{});
}
// Lets the listed kernels ask for `bytes` of dynamic LDS (beyond the default 64 KB), once per process and list (a race sets the same
// attributes twice)
template <auto... Kernels>
static int tp_reserve_lds(const char* name, int bytes) {
    static bool lds_set = false;
    if (lds_set) return LPM_OK;
    for (const void* kernel : {(const void*)Kernels...}) {
        if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) {
            (void)hipGetLastError();
            set_error("%s: cannot reserve %d bytes of LDS", name, bytes);
            return LPM_ERR_LAUNCH;
        }
    }
    lds_set = true;
    return LPM_OK;
}
// The shape refusals of the family.  The op's own: its frame limit, why it has one (appended to the message), and the workgroups per clip
// of its largest launch.
static int tp_check(const char* name, int B, int T, int D, int K, int max_frames, const char* why, int64_t wg_per_clip) {
    LPM_REQUIRE(B > 0 && K > 0 && T > 0, LPM_ERR_BADARG, "%s: need B, T, K >= 1 (B=%d T=%d K=%d)", name, B, T, K);
    LPM_REQUIRE(D == 128 || D == 1024, LPM_ERR_UNSUPPORTED_SHAPE, "%s: need D in {128, 1024} (D=%d)", name, D);
    LPM_REQUIRE(T >= 2 && T <= max_frames, LPM_ERR_UNSUPPORTED_SHAPE,
                "%s: need 2 <= T <= %d frames (T=%d): the temporal embedding is a frame-to-frame difference%s", name, max_frames, T, why);
    LPM_REQUIRE((int64_t)K * D < (1ll << 31) && B * wg_per_clip < (1ll << 31), LPM_ERR_UNSUPPORTED_SHAPE,
                "%s: B * K or K * D too large (B=%d K=%d)", name, B, K);
    return LPM_OK;
}
static int ta_check(const char* name, int B, int T, int D, int K) {
    const int64_t nt = ta_tiles(T < TA_MAX_FRAMES ? T : TA_MAX_FRAMES);     // (the Gram's tile pairs)
    return tp_check(name, B, T, D, K, TA_MAX_FRAMES, ", and the backward keeps a [T, 32] tile of each embedding in LDS", K * nt * nt);
}
static_assert(TA_CH == 32, "ta_check's message names the tile width");
// (defined in triangulation_attention.hip)  out[o][i] = sum_s part[o][s][i], s = 0, 1, ...
int ta_sum_slices(const float* part, int64_t outer, int64_t n, int S, float* out, hipStream_t s, const char* name);
// (likewise)  dx[b] = sum_g dx_part[b][g], g = 0, 1, ... when G > 1;  danchors[d][k] = - sum_b da_part[b][k][d], b = 0, 1, ..., two-level:
// da_chunk clips into a partial, partials into the total (da_chunk >= B: one level)
int ta_reduce_partials(const float* dx_part, const float* da_part, int B, int T, int D, int K, int G, int da_chunk, float* dx, float* danchors,
                       hipStream_t s, const char* name);

}  // namespace lpm
