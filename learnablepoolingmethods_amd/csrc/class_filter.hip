// The glue between the three GEMMs of the "class filter" behind MoeModel2 / JuhanMoeModel (video_level_models.py:518-539, :600-620):
// one launch forward and one backward serve all three stages.  For a [B, C] fp32 row-major, 1 <= B <= 1024, any C >= 1:
//   pre = a (+ bias[C]) (+ residual[B, C])
//   u   = act(pre)                          relu | leaky_relu(alpha) = (pre > 0 ? pre : alpha pre) | sigmoid
//   v   = gamma (u - mean) rstd + beta      tf.layers.batch_normalization (optional): training -- the batch mean and the BIASED batch
//                                           variance per column over the B rows, rstd = 1 / sqrt(var + eps), both written out, and both
//                                           moving statistics updated in place, m = decay m + (1 - decay) (mean | var) (the biased
//                                           variance: the rank-2 input takes TF1's non-fused path); eval -- mean and rstd from the moving
//                                           statistics
//   y   = keep ? v / keep_prob : 0          tf.nn.dropout's keep mask [B, C], one byte per element (optional, training only)
// Backward: dv = keep ? dy / keep_prob : 0, dbeta = sum_b dv, dgamma = sum_b dv xhat, du = gamma rstd (dv - dbeta / B - xhat dgamma / B)
// (training; eval: gamma rstd dv; no batch norm: dv), dpre = du act'(pre) -- the gradient of a and of the residual alike -- and
// dbias = sum_b dpre.  u is RECOMPUTED from a, bias and the residual (the autograd node keeps no [B, C] tensor of its own).  In training
// xhat is centred once more by its own batch mean (the fp32 rounding of `mean`, times rstd): see class_filter_bwd_kernel.
// Layout: a workgroup owns 16 columns and walks all B rows, 16 row groups of 16 lanes -- a wave instruction reads four 64-byte row
// pieces, element by element: no alignment is assumed (rows of C = 3862 floats start on 8-byte boundaries, of odd C on 4-byte ones).
// The slab (B x 64 bytes, at most 64 KiB) is read from HBM by the first pass and from L2 by the ones behind it.
// Moments: two passes -- the mean first, then the sum of (u - mean)^2 -- never E[u^2] - mean^2.  Every column sum of either direction
// (the two moments, dbeta, dgamma, dbias) is accumulated in fp64: at 1024 rows an fp32 running sum loses a few ulp of the mean, which
// the normalised values and the moving averages would carry; the passes are bound by their loads, not by the adds.
// Every thread adds its rows in row order, the 16 row groups meet through LDS and are added in group order by every thread alike: no
// atomics, the same inputs give the same bits.
#include "lpm_common.h"

namespace lpm {

constexpr int CF_THREADS = 256;
constexpr int CF_COLS = 16;                    // columns of a workgroup
constexpr int CF_RG = CF_THREADS / CF_COLS;    // row groups
constexpr int CF_UNROLL = 8;                   // independent rows in flight per thread
constexpr int CF_MAX_ROWS = 1024;
enum { CF_BN_NONE = 0, CF_BN_TRAIN = 1, CF_BN_EVAL = 2 };

template <int ACT>
__device__ __forceinline__ float cf_act(float pre, float alpha) {
    if constexpr (ACT == LPM_CLASS_FILTER_RELU) return pre > 0.f ? pre : 0.f;
    else if constexpr (ACT == LPM_CLASS_FILTER_LEAKY_RELU) return pre > 0.f ? pre : alpha * pre;
    else return 1.f / (1.f + expf(-pre));
}
// act'(pre), given u = act(pre)
template <int ACT>
__device__ __forceinline__ float cf_dact(float pre, float u, float alpha) {
    if constexpr (ACT == LPM_CLASS_FILTER_RELU) return pre > 0.f ? 1.f : 0.f;
    else if constexpr (ACT == LPM_CLASS_FILTER_LEAKY_RELU) return pre > 0.f ? 1.f : alpha;
    else return u * (1.f - u);
}

// the sum over the 16 row groups of one value per thread, in group order, on every thread of the column
__device__ __forceinline__ double cf_group_sum(double (*sh)[CF_COLS], double v, int rg, int cl) {
    __syncthreads();                               // (the previous reduction's readers are done with sh)
    sh[rg][cl] = v;
    __syncthreads();
    double s = sh[0][cl];
#pragma unroll
    for (int i = 1; i < CF_RG; ++i) s += sh[i][cl];
    return s;
}

// One thread's walk over its rows rg, rg + 16, ...: CF_UNROLL rows are loaded before any is used.  Rows past B and columns past C read
// the last valid element instead (every load is in bounds and unconditional) and `f` is told that they do not count.
template <typename F>
__device__ __forceinline__ void cf_walk(int B, int rg, F&& f) {
    for (int r0 = rg; r0 < B; r0 += CF_RG * CF_UNROLL) {
#pragma unroll
        for (int i = 0; i < CF_UNROLL; ++i) {
            const int r = r0 + CF_RG * i;
            f(min(r, B - 1), r < B);
        }
    }
}

template <int ACT, int BN>
__global__ __launch_bounds__(CF_THREADS) void class_filter_fwd_kernel(const float* __restrict__ a, const float* __restrict__ bias,
                                                                      const float* __restrict__ residual, int B, int C, float alpha,
                                                                      const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                      float* __restrict__ moving_mean, float* __restrict__ moving_var,
                                                                      float eps, double decay, const uint8_t* __restrict__ keep,
                                                                      float keep_prob, float* __restrict__ y, float* __restrict__ mean_out,
                                                                      float* __restrict__ rstd_out) {
    __shared__ double sh[CF_RG][CF_COLS];
    const int cl = threadIdx.x & (CF_COLS - 1), rg = threadIdx.x / CF_COLS;
    const int col = blockIdx.x * CF_COLS + cl;
    const bool live = col < C;
    const int c = min(col, C - 1);
    const float bs = bias ? bias[c] : 0.f;
    const bool has_res = residual != nullptr, has_keep = keep != nullptr;
    auto u_at = [&](int64_t e) {
        float pre = a[e] + bs;
        if (has_res) pre += residual[e];
        return cf_act<ACT>(pre, alpha);
    };

    float mean = 0.f, rstd = 1.f, g = 1.f, bt = 0.f;
    if constexpr (BN == CF_BN_TRAIN) {
        double s = 0.0;
        cf_walk(B, rg, [&](int r, bool ok) {
            const float u = u_at((int64_t)r * C + c);
            s += ok ? (double)u : 0.0;
        });
        const double mean_d = cf_group_sum(sh, s, rg, cl) / (double)B;
        double q = 0.0;
        cf_walk(B, rg, [&](int r, bool ok) {
            const double d = (double)u_at((int64_t)r * C + c) - mean_d;
            q += ok ? d * d : 0.0;
        });
        const double var_d = cf_group_sum(sh, q, rg, cl) / (double)B;
        mean = (float)mean_d;
        rstd = (float)(1.0 / sqrt(var_d + (double)eps));
        if (rg == 0 && live) {
            mean_out[c] = mean;
            rstd_out[c] = rstd;
            moving_mean[c] = (float)(decay * (double)moving_mean[c] + (1.0 - decay) * mean_d);
            moving_var[c] = (float)(decay * (double)moving_var[c] + (1.0 - decay) * var_d);
        }
    } else if constexpr (BN == CF_BN_EVAL) {
        mean = moving_mean[c];
        rstd = 1.f / sqrtf(moving_var[c] + eps);
        if (rg == 0 && live && mean_out) {
            mean_out[c] = mean;
            rstd_out[c] = rstd;
        }
    }
    if constexpr (BN != CF_BN_NONE) {
        g = gamma[c];
        bt = beta[c];
    }
    for (int r0 = rg; r0 < B; r0 += CF_RG * CF_UNROLL) {
        float v[CF_UNROLL];
        uint8_t k[CF_UNROLL];
#pragma unroll
        for (int i = 0; i < CF_UNROLL; ++i) {
            const int64_t e = (int64_t)min(r0 + CF_RG * i, B - 1) * C + c;
            v[i] = u_at(e);
            k[i] = has_keep ? keep[e] : (uint8_t)1;
        }
#pragma unroll
        for (int i = 0; i < CF_UNROLL; ++i) {
            const int r = r0 + CF_RG * i;
            float o = v[i];
            if constexpr (BN != CF_BN_NONE) o = ((o - mean) * rstd) * g + bt;
            if (has_keep) o = k[i] ? o / keep_prob : 0.f;
            if (r < B && live) y[(int64_t)r * C + c] = o;
        }
    }
}

template <int ACT, int BN>
__global__ __launch_bounds__(CF_THREADS) void class_filter_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ a,
                                                                      const float* __restrict__ bias, const float* __restrict__ residual,
                                                                      int B, int C, float alpha, const float* __restrict__ gamma,
                                                                      const float* __restrict__ mean_in, const float* __restrict__ rstd_in,
                                                                      const uint8_t* __restrict__ keep, float keep_prob,
                                                                      float* __restrict__ dpre, float* __restrict__ dbias,
                                                                      float* __restrict__ dgamma, float* __restrict__ dbeta) {
    __shared__ double sh[CF_RG][CF_COLS];
    const int cl = threadIdx.x & (CF_COLS - 1), rg = threadIdx.x / CF_COLS;
    const int col = blockIdx.x * CF_COLS + cl;
    const bool live = col < C;
    const int c = min(col, C - 1);
    const float bs = bias ? bias[c] : 0.f;
    const bool has_res = residual != nullptr, has_keep = keep != nullptr;
    auto pre_at = [&](int64_t e) {
        float pre = a[e] + bs;
        if (has_res) pre += residual[e];
        return pre;
    };
    auto dv_at = [&](int64_t e) {
        const float d = dy[e];
        if (!has_keep) return d;
        return keep[e] ? d / keep_prob : 0.f;
    };

    // m_x (training): the batch mean of xhat as THIS pass forms it, (u - mean) rstd with the fp32 mean the forward wrote.  It is the
    // rounding of that mean times rstd, not zero; where |mean| >> std it reaches 1e-5, and the backward's "sum_b xhat = 0" would leave
    // that much of dgamma / B in every dpre (and their sum in dbias).  xhat - m_x is centred again.
    float mean = 0.f, rstd = 1.f, g = 1.f, m_dv = 0.f, m_dvx = 0.f, m_x = 0.f;
    if constexpr (BN != CF_BN_NONE) {
        mean = mean_in[c];
        rstd = rstd_in[c];
        g = gamma[c];
        double s = 0.0, t = 0.0, x = 0.0;
        cf_walk(B, rg, [&](int r, bool ok) {
            const int64_t e = (int64_t)r * C + c;
            const float u = cf_act<ACT>(pre_at(e), alpha), dv = dv_at(e), xh = (u - mean) * rstd;
            s += ok ? (double)dv : 0.0;
            t += ok ? (double)dv * (double)xh : 0.0;
            if constexpr (BN == CF_BN_TRAIN) x += ok ? (double)xh : 0.0;
        });
        const double sb = cf_group_sum(sh, s, rg, cl);
        double sg = cf_group_sum(sh, t, rg, cl);
        if constexpr (BN == CF_BN_TRAIN) {
            const double mx = cf_group_sum(sh, x, rg, cl) / (double)B;
            sg -= mx * sb;
            m_x = (float)mx;
        }
        if (rg == 0 && live) {
            dbeta[c] = (float)sb;
            dgamma[c] = (float)sg;
        }
        m_dv = (float)(sb / (double)B);
        m_dvx = (float)(sg / (double)B);
    }
    double sbias = 0.0;
    for (int r0 = rg; r0 < B; r0 += CF_RG * CF_UNROLL) {
        float p[CF_UNROLL], d[CF_UNROLL];
#pragma unroll
        for (int i = 0; i < CF_UNROLL; ++i) {
            const int64_t e = (int64_t)min(r0 + CF_RG * i, B - 1) * C + c;
            p[i] = pre_at(e);
            d[i] = dv_at(e);
        }
#pragma unroll
        for (int i = 0; i < CF_UNROLL; ++i) {
            const int r = r0 + CF_RG * i;
            const float u = cf_act<ACT>(p[i], alpha);
            float du = d[i];
            if constexpr (BN == CF_BN_TRAIN) du = (g * rstd) * ((du - m_dv) - ((u - mean) * rstd - m_x) * m_dvx);
            else if constexpr (BN == CF_BN_EVAL) du = (g * rstd) * du;
            const float dp = du * cf_dact<ACT>(p[i], u, alpha);
            if (r < B && live) {
                dpre[(int64_t)r * C + c] = dp;
                sbias += (double)dp;
            }
        }
    }
    if (dbias) {                                   // (uniform over the launch)
        const double sb = cf_group_sum(sh, sbias, rg, cl);
        if (rg == 0 && live) dbias[c] = (float)sb;
    }
}

static bool class_filter_act_ok(int act) {
    return act == LPM_CLASS_FILTER_RELU || act == LPM_CLASS_FILTER_LEAKY_RELU || act == LPM_CLASS_FILTER_SIGMOID;
}

}  // namespace lpm

#define LPM_CF_DISPATCH(LAUNCH)                                                                  \
    do {                                                                                         \
        if (act == LPM_CLASS_FILTER_RELU) {                                                      \
            if (bn == CF_BN_NONE) LAUNCH(LPM_CLASS_FILTER_RELU, CF_BN_NONE);                     \
            else if (bn == CF_BN_TRAIN) LAUNCH(LPM_CLASS_FILTER_RELU, CF_BN_TRAIN);              \
            else LAUNCH(LPM_CLASS_FILTER_RELU, CF_BN_EVAL);                                      \
        } else if (act == LPM_CLASS_FILTER_LEAKY_RELU) {                                         \
            if (bn == CF_BN_NONE) LAUNCH(LPM_CLASS_FILTER_LEAKY_RELU, CF_BN_NONE);               \
            else if (bn == CF_BN_TRAIN) LAUNCH(LPM_CLASS_FILTER_LEAKY_RELU, CF_BN_TRAIN);        \
            else LAUNCH(LPM_CLASS_FILTER_LEAKY_RELU, CF_BN_EVAL);                                \
        } else {                                                                                 \
            if (bn == CF_BN_NONE) LAUNCH(LPM_CLASS_FILTER_SIGMOID, CF_BN_NONE);                  \
            else if (bn == CF_BN_TRAIN) LAUNCH(LPM_CLASS_FILTER_SIGMOID, CF_BN_TRAIN);           \
            else LAUNCH(LPM_CLASS_FILTER_SIGMOID, CF_BN_EVAL);                                   \
        }                                                                                        \
    } while (0)

extern "C" int lpm_class_filter_fwd(const float* a, const float* bias, const float* residual, int B, int C, int act, float alpha,
                                    const float* gamma, const float* beta, float* moving_mean, float* moving_variance, int is_training,
                                    float eps, double decay, const uint8_t* keep, float keep_prob, float* y, float* mean, float* rstd,
                                    lpm_stream_t stream) {
    using namespace lpm;
    LPM_REQUIRE(a && y, LPM_ERR_BADARG, "lpm_class_filter_fwd: null pointer (a, y)");
    LPM_REQUIRE(class_filter_act_ok(act), LPM_ERR_BADARG, "lpm_class_filter_fwd: act must be %d (relu), %d (leaky_relu) or %d (sigmoid), got %d",
                LPM_CLASS_FILTER_RELU, LPM_CLASS_FILTER_LEAKY_RELU, LPM_CLASS_FILTER_SIGMOID, act);
    LPM_REQUIRE(B >= 1 && B <= CF_MAX_ROWS && C >= 1, LPM_ERR_UNSUPPORTED_SHAPE,
                "lpm_class_filter_fwd: need 1 <= B <= %d and C >= 1 (got %d, %d)", CF_MAX_ROWS, B, C);
    const bool has_bn = gamma || beta || moving_mean || moving_variance;
    LPM_REQUIRE(!has_bn || (gamma && beta && moving_mean && moving_variance), LPM_ERR_BADARG,
                "lpm_class_filter_fwd: batch norm needs gamma, beta, moving_mean and moving_variance (all four NULL: no batch norm)");
    LPM_REQUIRE(!has_bn || eps > 0.f, LPM_ERR_BADARG, "lpm_class_filter_fwd: eps must be positive, got %g", (double)eps);
    const int bn = !has_bn ? CF_BN_NONE : is_training ? CF_BN_TRAIN : CF_BN_EVAL;
    LPM_REQUIRE(bn != CF_BN_TRAIN || (mean && rstd), LPM_ERR_BADARG, "lpm_class_filter_fwd: training-mode batch norm writes mean and rstd [C]");
    LPM_REQUIRE(bn != CF_BN_EVAL || ((mean == nullptr) == (rstd == nullptr)), LPM_ERR_BADARG,
                "lpm_class_filter_fwd: mean and rstd go together (both or neither in eval mode)");
    LPM_REQUIRE(bn != CF_BN_TRAIN || (decay >= 0.0 && decay <= 1.0), LPM_ERR_BADARG, "lpm_class_filter_fwd: decay must be in [0, 1], got %g", decay);
    LPM_REQUIRE(!keep || is_training, LPM_ERR_BADARG, "lpm_class_filter_fwd: a keep mask is applied in training only");
    LPM_REQUIRE(!keep || (keep_prob > 0.f && keep_prob <= 1.f), LPM_ERR_BADARG, "lpm_class_filter_fwd: keep_prob must be in (0, 1], got %g",
                (double)keep_prob);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)((C + CF_COLS - 1) / CF_COLS)), block(CF_THREADS);
#define LPM_CF_FWD(ACT, BNMODE)                                                                                                          \
    hipLaunchKernelGGL((class_filter_fwd_kernel<ACT, BNMODE>), grid, block, 0, s, a, bias, residual, B, C, alpha, gamma, beta, moving_mean, \
                       moving_variance, eps, decay, keep, keep_prob, y, mean, rstd)
    LPM_CF_DISPATCH(LPM_CF_FWD);
#undef LPM_CF_FWD
    return check_launch("lpm_class_filter_fwd");
}

extern "C" int lpm_class_filter_bwd(const float* dy, const float* a, const float* bias, const float* residual, int B, int C, int act,
                                    float alpha, const float* gamma, const float* mean, const float* rstd, int is_training,
                                    const uint8_t* keep, float keep_prob, float* dpre, float* dbias, float* dgamma, float* dbeta,
                                    lpm_stream_t stream) {
    using namespace lpm;
    LPM_REQUIRE(dy && a && dpre, LPM_ERR_BADARG, "lpm_class_filter_bwd: null pointer (dy, a, dpre)");
    LPM_REQUIRE(class_filter_act_ok(act), LPM_ERR_BADARG, "lpm_class_filter_bwd: act must be %d (relu), %d (leaky_relu) or %d (sigmoid), got %d",
                LPM_CLASS_FILTER_RELU, LPM_CLASS_FILTER_LEAKY_RELU, LPM_CLASS_FILTER_SIGMOID, act);
    LPM_REQUIRE(B >= 1 && B <= CF_MAX_ROWS && C >= 1, LPM_ERR_UNSUPPORTED_SHAPE,
                "lpm_class_filter_bwd: need 1 <= B <= %d and C >= 1 (got %d, %d)", CF_MAX_ROWS, B, C);
    const bool has_bn = gamma || mean || rstd || dgamma || dbeta;
    LPM_REQUIRE(!has_bn || (gamma && mean && rstd && dgamma && dbeta), LPM_ERR_BADARG,
                "lpm_class_filter_bwd: batch norm needs gamma, mean, rstd, dgamma and dbeta (all five NULL: no batch norm)");
    LPM_REQUIRE((bias == nullptr) == (dbias == nullptr), LPM_ERR_BADARG, "lpm_class_filter_bwd: bias and dbias go together");
    LPM_REQUIRE(!keep || is_training, LPM_ERR_BADARG, "lpm_class_filter_bwd: a keep mask is applied in training only");
    LPM_REQUIRE(!keep || (keep_prob > 0.f && keep_prob <= 1.f), LPM_ERR_BADARG, "lpm_class_filter_bwd: keep_prob must be in (0, 1], got %g",
                (double)keep_prob);
    const int bn = !has_bn ? CF_BN_NONE : is_training ? CF_BN_TRAIN : CF_BN_EVAL;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)((C + CF_COLS - 1) / CF_COLS)), block(CF_THREADS);
#define LPM_CF_BWD(ACT, BNMODE)                                                                                                       \
    hipLaunchKernelGGL((class_filter_bwd_kernel<ACT, BNMODE>), grid, block, 0, s, dy, a, bias, residual, B, C, alpha, gamma, mean, rstd, \
                       keep, keep_prob, dpre, dbias, dgamma, dbeta)
    LPM_CF_DISPATCH(LPM_CF_BWD);
#undef LPM_CF_BWD
    return check_launch("lpm_class_filter_bwd");
}
#undef LPM_CF_DISPATCH
