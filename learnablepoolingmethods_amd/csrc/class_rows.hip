// The row-wise glue over [B, C] class scores behind FishMoeModel3 (video_level_models.py:431-436) and the class-gating modules
// (attention_modules.py:157-273): where class_filter.hip owns columns, a workgroup here owns a ROW.  For a [B, C] fp32 row-major,
// 1 <= B <= 1024, 1 <= C <= 16384:
//   t   = a (+ bias[C])
//   pre = phi(t) (+ residual[B, C])         phi: identity | relu6(t) = min(max(t, 0), 6) | neg_relu6(t) = -relu6(-t)
//   y   = pre                                           norm none
//       = exp(pre - max_j pre) / sum_j exp(pre - max)   norm softmax
//       = gamma (pre - mean) rstd + beta                norm layer_norm: tf.contrib.layers.layer_norm at rank 2 -- the mean and the BIASED
//                                                       variance over the row, rstd = 1 / sqrt(var + eps); stats[b] = (mean, rstd)
// Backward: dpre = dy | y (dy - sum_j y_j dy_j) | rstd (g - mean_j g - xhat mean_j (g xhat)) with g = dy gamma; dresidual = dpre;
// da = dpre phi'(t), phi' = [0 < t < 6] | [-6 < t < 0]; dbias = sum_b da, dgamma = sum_b dy xhat, dbeta = sum_b dy.  t and xhat are
// RECOMPUTED from a, bias, the residual and stats (the autograd node keeps no [B, C] tensor of its own); the softmax reads y.
// Layout: 256 threads per row, element k * 256 + tid in register slot k of its thread -- NPT = 1, 4, 16 or 64 slots, the smallest that
// covers C -- so every load of the row is issued before any value is used (unconditional loads of a clamped index: cr_load), the row is
// read from HBM ONCE each way and every later pass (the maximum, the two moments, the normalisation) walks registers.  Element by element:
// no alignment beyond fp32's is assumed (rows of C = 3862 floats start on 8-byte boundaries, of odd C on 4-byte ones).  phi' is one bit
// per slot, kept from the load to the store.
// Moments: two passes -- the mean first, then the sum of (pre - mean)^2 -- never E[x^2] - mean^2.  Every row sum and every column sum is
// accumulated in fp64 (16384 columns or 1024 rows in fp32 cost ulps of the mean; the passes are bound by their loads, not by the adds):
// a thread adds its slots in order, the 64 lanes of a wave meet by a butterfly, the 4 waves through LDS in wave order.
// In the backward xhat = (pre - mean) rstd is formed with the fp32 mean the forward wrote; its own row mean -- the rounding of that mean
// times rstd, up to 3e-5 where |mean| = 1e3 std -- is taken out again (as class_filter_bwd_kernel does per column).
// The column sums cross workgroups: a second, column-owned launch of the backward (16 columns per workgroup, the walk of
// class_filter.hip) adds da, dy and dy xhat over the rows in a fixed order.  It exists only with a bias or a layer norm.  No atomics:
// the same inputs give the same bits both ways.
#include "lpm_common.h"

namespace lpm {

constexpr int CR_THREADS = 256;
constexpr int CR_WAVES = CR_THREADS / kWave;
constexpr int CR_MAX_ROWS = 1024;
constexpr int CR_MAX_COLS = 16384;
constexpr int CR_COLS = 16;                    // the column launch: columns of a workgroup,
constexpr int CR_RG = CR_THREADS / CR_COLS;    // its row groups
constexpr int CR_UNROLL = 8;                   // and the independent rows in flight per thread

__device__ __forceinline__ float cr_phi(int phi, float t) {
    if (phi == LPM_CLASS_ROWS_RELU6) return fminf(fmaxf(t, 0.f), 6.f);
    if (phi == LPM_CLASS_ROWS_NEG_RELU6) return -fminf(fmaxf(-t, 0.f), 6.f);
    return t;
}
__device__ __forceinline__ bool cr_dphi(int phi, float t) {
    if (phi == LPM_CLASS_ROWS_RELU6) return t > 0.f && t < 6.f;
    if (phi == LPM_CLASS_ROWS_NEG_RELU6) return t < 0.f && t > -6.f;
    return true;
}

// the sum over the workgroup of N values per thread, on every thread: lanes by a butterfly, waves in wave order
template <int N>
__device__ __forceinline__ void cr_block_sum(double (*sh)[CR_WAVES], double (&v)[N]) {
#pragma unroll
    for (int n = 0; n < N; ++n)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[n] += __shfl_xor(v[n], o, 64);
    __syncthreads();                               // (the previous reduction's readers are done with sh)
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int n = 0; n < N; ++n) sh[n][threadIdx.x >> 6] = v[n];
    __syncthreads();
#pragma unroll
    for (int n = 0; n < N; ++n) {
        v[n] = sh[n][0];
#pragma unroll
        for (int w = 1; w < CR_WAVES; ++w) v[n] += sh[n][w];
    }
}
__device__ __forceinline__ float cr_block_max(float* sh, float v) {
    v = wave_max(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    v = sh[0];
#pragma unroll
    for (int w = 1; w < CR_WAVES; ++w) v = fmaxf(v, sh[w]);
    return v;
}

// One [C] or [B, C] operand's slots of the row: element min(k * 256 + tid, C - 1) -- every load is in bounds and UNCONDITIONAL, so that all
// NPT of them can be in flight at once (a load under `i < C` sits in a branch of its own; class_filter.hip's rule).
// Slots past C hold a copy of the last element; the callers do not count them.
template <int NPT>
__device__ __forceinline__ void cr_load(const float* __restrict__ p, int64_t base, int C, float (&v)[NPT]) {
#pragma unroll
    for (int k = 0; k < NPT; ++k) v[k] = p[base + min(k * CR_THREADS + (int)threadIdx.x, C - 1)];
}

// pre of the row's slots (and phi' as bits); slots past C hold 0 and a clear bit
template <int NPT>
__device__ __forceinline__ uint64_t cr_load_pre(const float* __restrict__ a, const float* __restrict__ bias,
                                                const float* __restrict__ residual, int64_t base, int C, int phi, float (&pre)[NPT]) {
    float b[NPT], r[NPT];
    cr_load<NPT>(a, base, C, pre);
    if (bias) cr_load<NPT>(bias, 0, C, b);         // (uniform over the launch)
    if (residual) cr_load<NPT>(residual, base, C, r);
    uint64_t bits = 0;
#pragma unroll
    for (int k = 0; k < NPT; ++k) {
        const bool ok = k * CR_THREADS + (int)threadIdx.x < C;
        const float t = bias ? pre[k] + b[k] : pre[k];
        bits |= (uint64_t)(ok && cr_dphi(phi, t)) << k;
        const float p = residual ? cr_phi(phi, t) + r[k] : cr_phi(phi, t);
        pre[k] = ok ? p : 0.f;
    }
    return bits;
}

template <int NORM, int NPT>
__global__ __launch_bounds__(CR_THREADS) void class_rows_fwd_kernel(const float* __restrict__ a, const float* __restrict__ bias,
                                                                    const float* __restrict__ residual, int C, int phi,
                                                                    const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                    float eps, float* __restrict__ y, float* __restrict__ stats) {
    __shared__ double sh[1][CR_WAVES];
    __shared__ float shm[CR_WAVES];
    const int tid = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * C;
    float pre[NPT];
    cr_load_pre<NPT>(a, bias, residual, base, C, phi, pre);
    if constexpr (NORM == LPM_CLASS_ROWS_SOFTMAX) {
        float m = -INFINITY;
#pragma unroll
        for (int k = 0; k < NPT; ++k)
            if (k * CR_THREADS + tid < C) m = fmaxf(m, pre[k]);
        m = cr_block_max(shm, m);
        double s[1] = {0.0};
#pragma unroll
        for (int k = 0; k < NPT; ++k) {
            pre[k] = expf(pre[k] - m);
            s[0] += (k * CR_THREADS + tid < C) ? (double)pre[k] : 0.0;
        }
        cr_block_sum<1>(sh, s);
        const float sf = (float)s[0];
#pragma unroll
        for (int k = 0; k < NPT; ++k) pre[k] = pre[k] / sf;
    } else if constexpr (NORM == LPM_CLASS_ROWS_LAYER_NORM) {
        double s[1] = {0.0};
#pragma unroll
        for (int k = 0; k < NPT; ++k) s[0] += (double)pre[k];         // (slots past C hold 0)
        cr_block_sum<1>(sh, s);
        const double mean_d = s[0] / (double)C;
        double q[1] = {0.0};
#pragma unroll
        for (int k = 0; k < NPT; ++k) {
            const double d = (double)pre[k] - mean_d;
            q[0] += (k * CR_THREADS + tid < C) ? d * d : 0.0;
        }
        cr_block_sum<1>(sh, q);
        const double rstd_d = 1.0 / sqrt(q[0] / (double)C + (double)eps);
        if (tid == 0) {
            stats[2 * (int64_t)blockIdx.x] = (float)mean_d;
            stats[2 * (int64_t)blockIdx.x + 1] = (float)rstd_d;
        }
        float g[NPT], bt[NPT];
        cr_load<NPT>(gamma, 0, C, g);
        cr_load<NPT>(beta, 0, C, bt);
#pragma unroll
        for (int k = 0; k < NPT; ++k) pre[k] = (float)(((double)pre[k] - mean_d) * rstd_d) * g[k] + bt[k];
    }
#pragma unroll
    for (int k = 0; k < NPT; ++k) {
        const int i = k * CR_THREADS + tid;
        if (i < C) y[base + i] = pre[k];
    }
}

template <int NORM, int NPT>
__global__ __launch_bounds__(CR_THREADS) void class_rows_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ a,
                                                                    const float* __restrict__ bias, const float* __restrict__ residual,
                                                                    const float* __restrict__ y, int C, int phi,
                                                                    const float* __restrict__ gamma, const float* __restrict__ stats,
                                                                    float* __restrict__ da, float* __restrict__ dresidual) {
    __shared__ double sh[3][CR_WAVES];
    const int tid = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * C;
    float d[NPT];                                  // dy, then dpre
    cr_load<NPT>(dy, base, C, d);
    uint64_t bits = ~(uint64_t)0;
    if constexpr (NORM == LPM_CLASS_ROWS_LAYER_NORM) {
        float xh[NPT], gm[NPT];
        cr_load<NPT>(gamma, 0, C, gm);
        bits = cr_load_pre<NPT>(a, bias, residual, base, C, phi, xh);
        const float mean = stats[2 * (int64_t)blockIdx.x], rstd = stats[2 * (int64_t)blockIdx.x + 1];
        double s[3] = {0.0, 0.0, 0.0};             // sum g, sum g xhat, sum xhat
#pragma unroll
        for (int k = 0; k < NPT; ++k) {
            const bool ok = k * CR_THREADS + tid < C;
            xh[k] = ok ? (xh[k] - mean) * rstd : 0.f;
            d[k] = ok ? d[k] * gm[k] : 0.f;
            s[0] += (double)d[k];
            s[1] += (double)d[k] * (double)xh[k];
            s[2] += (double)xh[k];
        }
        cr_block_sum<3>(sh, s);
        const double mx = s[2] / (double)C;        // the row mean of xhat as this pass forms it: taken out again
        const float m_x = (float)mx, m_g = (float)(s[0] / (double)C), m_gx = (float)((s[1] - mx * s[0]) / (double)C);
#pragma unroll
        for (int k = 0; k < NPT; ++k) d[k] = rstd * ((d[k] - m_g) - (xh[k] - m_x) * m_gx);
    } else {
        if (phi != LPM_CLASS_ROWS_IDENTITY) {      // (uniform over the launch) t = a + bias, for phi' alone
            float t[NPT];
            bits = cr_load_pre<NPT>(a, bias, nullptr, base, C, phi, t);
        }
        if constexpr (NORM == LPM_CLASS_ROWS_SOFTMAX) {
            // With the fp32 y the forward wrote, sum_j y_j is 1 only to an ulp, and where one class holds nearly all of a row that ulp
            // does not cancel out of dy - sum_j y_j dy_j (1e-5 of the largest |dpre| of a row of five with y_max = 0.997).  The y are
            // taken as weights instead, normalised again in fp64: dpre = (y / S) (dy - sum_j y_j dy_j / S), S = sum_j y_j.
            float p[NPT];
            double s[2] = {0.0, 0.0};
            cr_load<NPT>(y, base, C, p);
#pragma unroll
            for (int k = 0; k < NPT; ++k) {
                if (k * CR_THREADS + tid >= C) p[k] = 0.f;
                s[0] += (double)p[k] * (double)d[k];
                s[1] += (double)p[k];
            }
            cr_block_sum<2>(sh, s);
            const double inv = 1.0 / s[1], r = s[0] * inv;
#pragma unroll
            for (int k = 0; k < NPT; ++k) d[k] = p[k] * (float)(((double)d[k] - r) * inv);
        }
    }
#pragma unroll
    for (int k = 0; k < NPT; ++k) {
        const int i = k * CR_THREADS + tid;
        if (i < C) {
            if (dresidual) dresidual[base + i] = d[k];
            da[base + i] = ((bits >> k) & 1) ? d[k] : 0.f;
        }
    }
}

// the sum over the 16 row groups of one value per thread, in group order, on every thread of the column
__device__ __forceinline__ double cr_group_sum(double (*sh)[CR_COLS], double v, int rg, int cl) {
    __syncthreads();
    sh[rg][cl] = v;
    __syncthreads();
    double s = sh[0][cl];
#pragma unroll
    for (int i = 1; i < CR_RG; ++i) s += sh[i][cl];
    return s;
}

// The column launch of the backward: dbias = sum_b da (when dbias), dbeta = sum_b dy and dgamma = sum_b dy xhat (LN).  A workgroup owns
// 16 columns and walks all B rows, 16 row groups of 16 lanes; rows past B and columns past C read the last valid element instead (every
// load is in bounds and unconditional) and do not count.
template <bool LN>
__global__ __launch_bounds__(CR_THREADS) void class_rows_colsums_kernel(const float* __restrict__ da, const float* __restrict__ dy,
                                                                        const float* __restrict__ a, const float* __restrict__ bias,
                                                                        const float* __restrict__ residual, int B, int C, int phi,
                                                                        const float* __restrict__ stats, float* __restrict__ dbias,
                                                                        float* __restrict__ dgamma, float* __restrict__ dbeta) {
    __shared__ double sh[CR_RG][CR_COLS];
    const int cl = threadIdx.x & (CR_COLS - 1), rg = threadIdx.x / CR_COLS;
    const int col = blockIdx.x * CR_COLS + cl;
    const bool live = col < C;
    const int c = min(col, C - 1);
    const float bs = bias ? bias[c] : 0.f;
    double sa = 0.0, sb = 0.0, sg = 0.0;
    for (int r0 = rg; r0 < B; r0 += CR_RG * CR_UNROLL) {
        float va[CR_UNROLL], vd[CR_UNROLL], vx[CR_UNROLL];
#pragma unroll
        for (int i = 0; i < CR_UNROLL; ++i) {
            const int r = min(r0 + CR_RG * i, B - 1);
            const int64_t e = (int64_t)r * C + c;
            va[i] = dbias ? da[e] : 0.f;
            if constexpr (LN) {
                vd[i] = dy[e];
                float pre = cr_phi(phi, a[e] + bs);
                if (residual) pre += residual[e];
                vx[i] = (pre - stats[2 * r]) * stats[2 * r + 1];
            }
        }
#pragma unroll
        for (int i = 0; i < CR_UNROLL; ++i) {
            const bool ok = r0 + CR_RG * i < B;
            sa += ok ? (double)va[i] : 0.0;
            if constexpr (LN) {
                sb += ok ? (double)vd[i] : 0.0;
                sg += ok ? (double)vd[i] * (double)vx[i] : 0.0;
            }
        }
    }
    if (dbias) {                                   // (uniform over the launch)
        const double s = cr_group_sum(sh, sa, rg, cl);
        if (rg == 0 && live) dbias[c] = (float)s;
    }
    if constexpr (LN) {
        const double b = cr_group_sum(sh, sb, rg, cl), g = cr_group_sum(sh, sg, rg, cl);
        if (rg == 0 && live) {
            dbeta[c] = (float)b;
            dgamma[c] = (float)g;
        }
    }
}

static bool class_rows_phi_ok(int phi) {
    return phi == LPM_CLASS_ROWS_IDENTITY || phi == LPM_CLASS_ROWS_RELU6 || phi == LPM_CLASS_ROWS_NEG_RELU6;
}
static bool class_rows_norm_ok(int norm) {
    return norm == LPM_CLASS_ROWS_NONE || norm == LPM_CLASS_ROWS_SOFTMAX || norm == LPM_CLASS_ROWS_LAYER_NORM;
}

}  // namespace lpm

// LAUNCH(NORM, NPT) for the runtime norm and the smallest NPT in {1, 4, 16, 64} with NPT * 256 >= C
#define LPM_CR_DISPATCH_NPT(LAUNCH, NORM)                   \
    do {                                                    \
        if (C <= 1 * CR_THREADS) LAUNCH(NORM, 1);           \
        else if (C <= 4 * CR_THREADS) LAUNCH(NORM, 4);      \
        else if (C <= 16 * CR_THREADS) LAUNCH(NORM, 16);    \
        else LAUNCH(NORM, 64);                              \
    } while (0)
#define LPM_CR_DISPATCH(LAUNCH)                                                                     \
    do {                                                                                            \
        if (norm == LPM_CLASS_ROWS_NONE) LPM_CR_DISPATCH_NPT(LAUNCH, LPM_CLASS_ROWS_NONE);          \
        else if (norm == LPM_CLASS_ROWS_SOFTMAX) LPM_CR_DISPATCH_NPT(LAUNCH, LPM_CLASS_ROWS_SOFTMAX); \
        else LPM_CR_DISPATCH_NPT(LAUNCH, LPM_CLASS_ROWS_LAYER_NORM);                                \
    } while (0)

extern "C" int lpm_class_rows_fwd(const float* a, const float* bias, const float* residual, int B, int C, int phi, int norm,
                                  const float* gamma, const float* beta, float eps, float* y, float* stats, lpm_stream_t stream) {
    using namespace lpm;
    static_assert(64 * CR_THREADS == CR_MAX_COLS, "the widest form covers the widest row");
    LPM_REQUIRE(a && y, LPM_ERR_BADARG, "lpm_class_rows_fwd: null pointer (a, y)");
    LPM_REQUIRE(class_rows_phi_ok(phi), LPM_ERR_BADARG, "lpm_class_rows_fwd: phi must be %d (identity), %d (relu6) or %d (neg_relu6), got %d",
                LPM_CLASS_ROWS_IDENTITY, LPM_CLASS_ROWS_RELU6, LPM_CLASS_ROWS_NEG_RELU6, phi);
    LPM_REQUIRE(class_rows_norm_ok(norm), LPM_ERR_BADARG, "lpm_class_rows_fwd: norm must be %d (none), %d (softmax) or %d (layer_norm), got %d",
                LPM_CLASS_ROWS_NONE, LPM_CLASS_ROWS_SOFTMAX, LPM_CLASS_ROWS_LAYER_NORM, norm);
    LPM_REQUIRE(B >= 1 && B <= CR_MAX_ROWS && C >= 1 && C <= CR_MAX_COLS, LPM_ERR_UNSUPPORTED_SHAPE,
                "lpm_class_rows_fwd: need 1 <= B <= %d and 1 <= C <= %d (got %d, %d)", CR_MAX_ROWS, CR_MAX_COLS, B, C);
    if (norm == LPM_CLASS_ROWS_LAYER_NORM)
        LPM_REQUIRE(gamma && beta && stats, LPM_ERR_BADARG, "lpm_class_rows_fwd: layer_norm needs gamma, beta [C] and stats [B, 2]");
    else
        LPM_REQUIRE(!gamma && !beta, LPM_ERR_BADARG, "lpm_class_rows_fwd: gamma and beta go with norm %d (layer_norm) only, got norm %d",
                    LPM_CLASS_ROWS_LAYER_NORM, norm);
    LPM_REQUIRE(eps > 0.f, LPM_ERR_BADARG, "lpm_class_rows_fwd: eps must be positive, got %g", (double)eps);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)B), block(CR_THREADS);
#define LPM_CR_FWD(NORM, NPT) \
    hipLaunchKernelGGL((class_rows_fwd_kernel<NORM, NPT>), grid, block, 0, s, a, bias, residual, C, phi, gamma, beta, eps, y, stats)
    LPM_CR_DISPATCH(LPM_CR_FWD);
#undef LPM_CR_FWD
    return check_launch("lpm_class_rows_fwd");
}

extern "C" int lpm_class_rows_bwd(const float* dy, const float* a, const float* bias, const float* residual, const float* y, int B, int C,
                                  int phi, int norm, const float* gamma, const float* stats, float* da, float* dresidual, float* dbias,
                                  float* dgamma, float* dbeta, lpm_stream_t stream) {
    using namespace lpm;
    LPM_REQUIRE(dy && a && da, LPM_ERR_BADARG, "lpm_class_rows_bwd: null pointer (dy, a, da)");
    LPM_REQUIRE(class_rows_phi_ok(phi), LPM_ERR_BADARG, "lpm_class_rows_bwd: phi must be %d (identity), %d (relu6) or %d (neg_relu6), got %d",
                LPM_CLASS_ROWS_IDENTITY, LPM_CLASS_ROWS_RELU6, LPM_CLASS_ROWS_NEG_RELU6, phi);
    LPM_REQUIRE(class_rows_norm_ok(norm), LPM_ERR_BADARG, "lpm_class_rows_bwd: norm must be %d (none), %d (softmax) or %d (layer_norm), got %d",
                LPM_CLASS_ROWS_NONE, LPM_CLASS_ROWS_SOFTMAX, LPM_CLASS_ROWS_LAYER_NORM, norm);
    LPM_REQUIRE(B >= 1 && B <= CR_MAX_ROWS && C >= 1 && C <= CR_MAX_COLS, LPM_ERR_UNSUPPORTED_SHAPE,
                "lpm_class_rows_bwd: need 1 <= B <= %d and 1 <= C <= %d (got %d, %d)", CR_MAX_ROWS, CR_MAX_COLS, B, C);
    const bool ln = norm == LPM_CLASS_ROWS_LAYER_NORM;
    if (ln)
        LPM_REQUIRE(gamma && stats && dgamma && dbeta, LPM_ERR_BADARG,
                    "lpm_class_rows_bwd: layer_norm needs gamma [C], stats [B, 2] (what the forward wrote), dgamma and dbeta [C]");
    else
        LPM_REQUIRE(!gamma && !dgamma && !dbeta, LPM_ERR_BADARG,
                    "lpm_class_rows_bwd: gamma, dgamma and dbeta go with norm %d (layer_norm) only, got norm %d", LPM_CLASS_ROWS_LAYER_NORM, norm);
    LPM_REQUIRE(norm != LPM_CLASS_ROWS_SOFTMAX || y, LPM_ERR_BADARG, "lpm_class_rows_bwd: the softmax's backward reads y (what the forward wrote)");
    LPM_REQUIRE((bias == nullptr) == (dbias == nullptr), LPM_ERR_BADARG, "lpm_class_rows_bwd: bias and dbias go together");
    LPM_REQUIRE(!dresidual || residual, LPM_ERR_BADARG, "lpm_class_rows_bwd: dresidual without a residual");
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)B), block(CR_THREADS);
#define LPM_CR_BWD(NORM, NPT) \
    hipLaunchKernelGGL((class_rows_bwd_kernel<NORM, NPT>), grid, block, 0, s, dy, a, bias, residual, y, C, phi, gamma, stats, da, dresidual)
    LPM_CR_DISPATCH(LPM_CR_BWD);
#undef LPM_CR_BWD
    if (ln || dbias) {                             // the column sums: they read the da the launch above wrote (the same stream)
        const dim3 cgrid((unsigned)((C + CR_COLS - 1) / CR_COLS));
        if (ln)
            hipLaunchKernelGGL((class_rows_colsums_kernel<true>), cgrid, block, 0, s, da, dy, a, bias, residual, B, C, phi, stats, dbias, dgamma,
                               dbeta);
        else
            hipLaunchKernelGGL((class_rows_colsums_kernel<false>), cgrid, block, 0, s, da, dy, a, bias, residual, B, C, phi, stats, dbias, dgamma,
                               dbeta);
    }
    return check_launch("lpm_class_rows_bwd");
}
#undef LPM_CR_DISPATCH
#undef LPM_CR_DISPATCH_NPT
