// The batch-normalised attention moments of TriangulationCnnIndirectAttentionModule (video_pooling_modules.py:431-571, JuhanTestModelV1):
// per row n = b T + t of x [(B T), D], anchor k of the [D, K] anchors (as they are: not normalised) and feature j = k D + d
//   q = |x - a_k|^2, iq = 1 / sqrt(max(q, 1e-12)), e[n,j] = (x[n,d] - a[d,k]) iq                        (tf.nn.l2_normalize)
//   g[n,j] = e[n,j] - e[n,(j-1) mod J]  (tf.manip.roll over the FEATURE axis, :506), frame 0 of every clip dropped, NOT normalised again
//   V_s = sc_s (e - mu_s) + beta_s,  V_t = sc_t (g - mu_t) + beta_t       (slim.batch_norm: sc = gamma rsqrt(var + eps); per feature)
//   G = V V^T per clip,  w = softmax_t(sum_u relu(G[t,u])),  pool = [ (1/T') sum_t w_t V_t | mean_t (V_t - mean_t V)^2 ]
// Batch norm is affine per feature, so its statistics, the Gram and both poolings are formed straight from the frames: nothing of size
// B T K D is written in either direction.  What IS written: q and iq [2, B T, K], the statistics [J], the Grams [B, T', T'], per-clip
// [B, J] sums, and in the backward one [B T, K] dot product, one danchors partial per clip.  No floating-point atomics: every
// cross-workgroup sum has a fixed order.  The Gram and the backward's M V products run on v_mfma_f32_32x32x2_f32 (exact fp32).
//
// _stats: tb_norms (one wave per row and 16 anchors) -> tb_stats<0> (a thread per (clip, feature): the sum over the frames) -> tb_colsum
//   (clips added b = 0, 1, ..., two-level: the mean) -> tb_stats<1> (deviations from that mean: their squares and their plain sum) ->
//   tb_colsum (the biased variance) -> tb_colsum (the mean of the deviations added onto the mean: the rounded mean's own error, the same
//   in every row, would add up over the rows in danchors -- 2.4 x the tests' bound at B = 1, T = 320 in an fp32 emulation, 0.6 x with it).
// _gram:  triangulation_attention.hip's Gram kernel with the affine map applied where the operand is generated.
// _pool:  a thread per (clip, feature) walks the frames twice: sum_t w_t raw and sum_t raw, then the deviations from the clip's mean
//   (their squares: the variance; their sum: what the rounded mean is off by, which the backward takes out again).
//   mean = sc ((1/T') sum_t w_t raw - mu / T') + beta / T'  (sum w = 1);  var = sc^2 var_t(raw).
// _dw:    dw[b,t] = <V_t, gm> / T', a workgroup per frame.
// _bwd:   per clip, with M[t,u] = [G[t,u] > 0] (dr_t + dr_u) from the caller (symmetric):
//     dV_t  = (w_t / T') gm + (2 / T') sc ((raw_t - mean_t raw) - c) gq + sum_u M[t,u] V_u          (c: the rounded mean's own error)
//     dbeta = sum_n dV,  dgamma = sum_n dV hat,  hat = (raw - mu) rsqrt(var + eps)
//     draw  = sc (dV - dbeta / N - hat dgamma / N)  (training; with given statistics draw = sc dV)
//     de[n,j] = draw_s[n,j] + draw_t[n,j] - draw_t[n,(j+1) mod J]      gr = iq (de - e (e . de) [q > 1e-12])
//     dx[n,:] = sum_k gr,  danchors[:,k] = - sum_n gr
//   The sums over all rows (dbeta, dgamma) and over D ((e . de)) must be complete before what follows them, so the chain runs three
//   times (tb_bwd<1>, <2>, <3>), each time per (clip, anchor, 32-column chunk): V of the chunk to LDS, M V on the matrix cores, a thread
//   per (frame, column) for the rest.  The temporal tile has a 33rd column (feature j + 32, which may be the next anchor's first): its
//   M V product is a plain loop.  Sweeps 1 and 2 give a workgroup a (clip, anchor) and walk the chunks; sweep 3 gives it a (clip, chunk)
//   and walks the anchors, adding onto its own columns of dx in turn.
// The CONV policy of tb_bwd (triangulation_cnn_attention, JuhanTestModelV2; entry points at the end of the file): V is e / g itself, there
//   is no batch norm (sweeps 2 and 3 only), and dV = M V + W_k^T dout, the per-anchor convolution's input gradient accumulated behind the
//   M V product in the same MFMA accumulators (dout [B T, K F] and W [K, F, D] from global memory).
// The MAG policy on top of CONV (triangulation_magnitude, JuhanTestModelV3; entry points at the end of the file): the temporal operand is
//   h = g it, it = 1 / sqrt(max(|g_k|^2, 1e-12)) per (row, anchor) from tv_norms, in the Gram and in the chain alike, and both norms are
//   outputs.  gh = M_t H + W_t^T dto is no longer the gradient of g:  gg = it (gh - h (h . gh) [p > eps]) + dtau [p > eps] h.  The dot
//   product (h . gh) holds a per-anchor block of the Gram, which the saved G_t (summed over the anchors) does not contain, so it takes a
//   sweep of its own in front of the other two (tb_mag_s1); sweep 3 adds dn [q > eps] e.
#include "triangulation_common.h"

// g = e[j] - e[j-1] must be exactly zero where both are equal, and every kernel must form V with the same roundings: no fused products
#pragma clang fp contract(off)

namespace lpm {

constexpr int TB_KC = 16;             // anchors per wave of tb_norms
constexpr int TB_LDV = TA_CH + 3;     // LDS row stride of the 33-column tiles (odd: rows fall on different banks)

__device__ __forceinline__ float tb_e(const float* __restrict__ xr, const float* __restrict__ anchors, const float* __restrict__ iqr, int K,
                                      int k, int d) {
    return ta_eh(xr[d], anchors[(int64_t)d * K + k], iqr[k]);
}
// the rolled difference: feature 0 of anchor k takes feature D - 1 of anchor (k - 1) mod K
template <int D>
__device__ __forceinline__ float tb_g(const float* __restrict__ xr, const float* __restrict__ anchors, const float* __restrict__ iqr, int K,
                                      int k, int d) {
    const int dp = d ? d - 1 : D - 1, kp = d ? k : (k ? k - 1 : K - 1);
    return tb_e(xr, anchors, iqr, K, k, d) - tb_e(xr, anchors, iqr, K, kp, dp);
}
__device__ __forceinline__ float tb_affine(float raw, float sc, float mu, float be) { return sc * (raw - mu) + be; }

// q[n,k] = |x_n - a_k|^2 and iq = 1 / sqrt(max(q, 1e-12)) (the second half of the buffer): direct sums of squares, one wave per row
template <int D>
__global__ __launch_bounds__(64 * TA_WAVES) void tb_norms_kernel(const float* __restrict__ x, const float* __restrict__ anchors, int64_t BT, int K,
                                                                 float* __restrict__ q) {
    constexpr int N = TpVec<D>::N;
    float* __restrict__ iqo = q + BT * K;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nkc = (K + TB_KC - 1) / TB_KC;
    const int64_t wid = (int64_t)blockIdx.x * TA_WAVES + wave;
    if (wid >= BT * nkc) return;                           // (wave-uniform; no barrier in this kernel)
    const int64_t row = wid / nkc;
    const int k0 = (int)(wid % nkc) * TB_KC, k1 = min(k0 + TB_KC, K);
    float xv[N], a[N];
    tp_load<D>(x + row * D, lane, xv);
    for (int k = k0; k < k1; ++k) {
        tp_load_anchor<D>(anchors, K, k, lane, a);
        float sq = 0.f;
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const float r = xv[j] - a[j];
            sq = fmaf(r, r, sq);
        }
        sq = wave_sum_dpp(sq);
        if (lane == 0) {
            q[row * K + k] = sq;
            iqo[row * K + k] = 1.f / sqrtf(fmaxf(sq, kL2Eps));
        }
    }
}

// a thread per (clip, feature), blockIdx.z = stream: PASS 0: part = sum_t raw;  PASS 1: part = sum_t (raw - mean)^2 and, behind both
// streams' blocks, sum_t (raw - mean): what the rounded mean is off by, times the count (two-level over t)
template <int D, int PASS>
__global__ __launch_bounds__(256) void tb_stats_kernel(const float* __restrict__ x, const float* __restrict__ anchors, const float* __restrict__ iq,
                                                       const float* __restrict__ mean, int B, int T, int K, float* __restrict__ part) {
    const int J = K * D, j = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y, z = blockIdx.z;
    if (j >= J) return;
    const int k = j / D, d = j % D;
    const float mu = PASS ? mean[(int64_t)z * 2 * J + j] : 0.f;       // (mean_s, var_s, mean_t, var_t: rows 0 and 2)
    float tot = 0.f, acc = 0.f, dtot = 0.f, dacc = 0.f;
    for (int t = z; t < T; ++t) {
        const int64_t n = (int64_t)b * T + t;
        const float raw = z ? tb_g<D>(x + n * D, anchors, iq + n * K, K, k, d) : tb_e(x + n * D, anchors, iq + n * K, K, k, d);
        if (PASS) {
            const float dev = raw - mu;
            acc = fmaf(dev, dev, acc);
            dacc += dev;
        } else {
            acc += raw;
        }
        if (((t - z) & (TP_SUM_CHUNK - 1)) == TP_SUM_CHUNK - 1) {
            tot += acc;
            dtot += dacc;
            acc = dacc = 0.f;
        }
    }
    part[((int64_t)z * B + b) * J + j] = tot + acc;
    if (PASS) part[((int64_t)(2 + z) * B + b) * J + j] = dtot + dacc;
}

// out[z * zstride + j] (+)= scale_z * sum_b part[z][b][j], b = 0, 1, ... (two-level); blockIdx.y = z; `add`: onto what is there
__global__ __launch_bounds__(256) void tb_colsum_kernel(const float* __restrict__ part, int B, int J, int64_t zstride, float scale0, float scale1,
                                                        int add, float* __restrict__ out) {
    const int j = blockIdx.x * 256 + threadIdx.x, z = blockIdx.y;
    if (j >= J) return;
    const float* p = part + (int64_t)z * B * J + j;
    float tot = 0.f;
    for (int b0 = 0; b0 < B; b0 += TP_SUM_CHUNK) {
        float acc = 0.f;
        for (int b = b0; b < min(b0 + TP_SUM_CHUNK, B); ++b) acc += p[(int64_t)b * J];
        tot += acc;
    }
    const float v = tot * ((z & 1) ? scale1 : scale0);
    out[z * zstride + j] = add ? out[z * zstride + j] + v : v;
}

// triangulation_attention.hip's Gram kernel on V_s (frames 0 .. T-1) and V_t (frames 1 .. T-1; row 0 of the tile is zero)
// MAG: V_t = h = g it, it [B T, K] the reciprocal norm of the rolled difference (triangulation_magnitude)
template <int D, bool MAG = false>
__global__ __launch_bounds__(64 * TA_WAVES) void tb_gram_kernel(const float* __restrict__ x, const float* __restrict__ anchors,
                                                                const float* __restrict__ iq, const float* __restrict__ it,
                                                                const float* __restrict__ aff, int T, int K, int S,
                                                                int NT, float* __restrict__ part_s, float* __restrict__ part_t) {
    __shared__ float tile[2][2][64][TA_LD];                // [tile I / J][V_s / V_t]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int J = K * D;
    int id = blockIdx.x;
    const int tj = id % NT; id /= NT;
    const int ti = id % NT; id /= NT;
    const int sl = id % S, b = id / S;
    const bool diag = ti == tj;
    const int nside = diag ? 1 : 2;
    const float* xb = x + (int64_t)b * T * D;
    const float* iqb = iq + (int64_t)b * T * K;
    const float* itb = MAG ? it + (int64_t)b * T * K : nullptr;
    const int c = threadIdx.x & 31, r0 = threadIdx.x >> 5;
    const int qi = wave >> 1, qj = wave & 1;
    const float (*tI)[64][TA_LD] = tile[0];
    const float (*tJ)[64][TA_LD] = tile[diag ? 0 : 1];
    f32x16 tot_s, tot_t;
#pragma unroll
    for (int r = 0; r < 16; ++r) tot_s[r] = tot_t[r] = 0.f;
    for (int k = sl; k < K; k += S) {
        f32x16 acc_s, acc_t;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc_s[r] = acc_t[r] = 0.f;
        for (int c0 = 0; c0 < D; c0 += TA_CH) {
            const int d = c0 + c, j = k * D + d;
            const float sc_s = aff[j], mu_s = aff[J + j], be_s = aff[2 * J + j];
            const float sc_t = aff[4 * J + j], mu_t = aff[5 * J + j], be_t = aff[6 * J + j];
            for (int side = 0; side < nside; ++side) {
                const int f0 = (side ? tj : ti) * 64;
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const int r = r0 + 8 * i, t = f0 + r;
                    float vs = 0.f, vt = 0.f;
                    if (t < T) {
                        const float* xr = xb + (int64_t)t * D;
                        const float* iqr = iqb + (int64_t)t * K;
                        vs = tb_affine(tb_e(xr, anchors, iqr, K, k, d), sc_s, mu_s, be_s);
                        if (t >= 1) {
                            const float g = tb_g<D>(xr, anchors, iqr, K, k, d);
                            vt = tb_affine(MAG ? g * itb[(int64_t)t * K + k] : g, sc_t, mu_t, be_t);
                        }
                    }
                    tile[side][0][r][c] = vs;
                    tile[side][1][r][c] = vt;
                }
            }
            __syncthreads();
#pragma unroll
            for (int kk = 0; kk < TA_CH; kk += 2) {
                const int col = kk + (lane >> 5), ra = 32 * qi + (lane & 31), rb = 32 * qj + (lane & 31);
                acc_s = mfma32(tI[0][ra][col], tJ[0][rb][col], acc_s);
                acc_t = mfma32(tI[1][ra][col], tJ[1][rb][col], acc_t);
            }
            __syncthreads();
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            tot_s[r] += acc_s[r];
            tot_t[r] += acc_t[r];
        }
    }
    const int T1 = T - 1;
    float* os = part_s + ((int64_t)b * S + sl) * T * T;
    float* ot = part_t + ((int64_t)b * S + sl) * T1 * T1;
    const int u = tj * 64 + 32 * qj + (lane & 31);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int t = ti * 64 + 32 * qi + mfma32_row(r, lane);
        if (t < T && u < T) {
            os[(int64_t)t * T + u] = tot_s[r];
            if (t >= 1 && u >= 1) ot[(int64_t)(t - 1) * T1 + (u - 1)] = tot_t[r];
        }
    }
}

// a thread per (clip, feature), blockIdx.z = stream: pool[b] = [mean | var], rawbar and corr [2, B, J] for the backward
template <int D>
__global__ __launch_bounds__(256) void tb_pool_kernel(const float* __restrict__ x, const float* __restrict__ anchors, const float* __restrict__ iq,
                                                      const float* __restrict__ aff, const float* __restrict__ w_s, const float* __restrict__ w_t,
                                                      int B, int T, int K, float* __restrict__ pool_s, float* __restrict__ pool_t,
                                                      float* __restrict__ rawbar, float* __restrict__ corr) {
    const int J = K * D, j = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y, z = blockIdx.z;
    if (j >= J) return;
    const int k = j / D, d = j % D, Tz = T - z;
    const float* w = z ? w_t : w_s;                          // null: the plain mean
    if (w) w += (int64_t)b * Tz;
    const float cnt = (float)Tz;
    float tot = 0.f, acc = 0.f, wtot = 0.f, wacc = 0.f;
    for (int t = z; t < T; ++t) {
        const int64_t n = (int64_t)b * T + t;
        const float raw = z ? tb_g<D>(x + n * D, anchors, iq + n * K, K, k, d) : tb_e(x + n * D, anchors, iq + n * K, K, k, d);
        acc += raw;
        if (w) wacc = fmaf(w[t - z], raw, wacc);
        if (((t - z) & (TP_SUM_CHUNK - 1)) == TP_SUM_CHUNK - 1) {
            tot += acc;
            wtot += wacc;
            acc = wacc = 0.f;
        }
    }
    const float rb = (tot + acc) / cnt, wsum = wtot + wacc;
    float dtot = 0.f, dacc = 0.f;
    tot = acc = 0.f;
    for (int t = z; t < T; ++t) {
        const int64_t n = (int64_t)b * T + t;
        const float raw = z ? tb_g<D>(x + n * D, anchors, iq + n * K, K, k, d) : tb_e(x + n * D, anchors, iq + n * K, K, k, d);
        const float dev = raw - rb;
        acc = fmaf(dev, dev, acc);
        dacc += dev;
        if (((t - z) & (TP_SUM_CHUNK - 1)) == TP_SUM_CHUNK - 1) {
            tot += acc;
            dtot += dacc;
            acc = dacc = 0.f;
        }
    }
    const float* a = aff + (int64_t)z * 4 * J;
    const float sc = a[j], mu = a[J + j], be = a[2 * J + j];
    float* pool = (z ? pool_t : pool_s) + (int64_t)b * 2 * J;
    pool[j] = w ? sc * (wsum / cnt - mu / cnt) + be / cnt : tb_affine(rb, sc, mu, be);
    pool[J + j] = (sc * sc) * ((tot + acc) / cnt);
    rawbar[((int64_t)z * B + b) * J + j] = rb;
    corr[((int64_t)z * B + b) * J + j] = (dtot + dacc) / cnt;
}

// a workgroup per (clip, frame), blockIdx.y = stream: dw[b,t] = <V_t, gm[b]> / T'
template <int D>
__global__ __launch_bounds__(256) void tb_dw_kernel(const float* __restrict__ x, const float* __restrict__ anchors, const float* __restrict__ iq,
                                                    const float* __restrict__ aff, const float* __restrict__ g_s, const float* __restrict__ g_t,
                                                    int T, int K, float* __restrict__ dw_s, float* __restrict__ dw_t) {
    __shared__ float red[4];
    const int J = K * D, z = blockIdx.y, b = blockIdx.x / T, t = blockIdx.x % T;
    if (z && t == 0) return;                               // (uniform over the workgroup)
    const int64_t n = (int64_t)b * T + t;
    const float* xr = x + n * D;
    const float* iqr = iq + n * K;
    const float* a = aff + (int64_t)z * 4 * J;
    const float* gm = (z ? g_t : g_s) + (int64_t)b * 2 * J;
    float acc = 0.f;
    for (int j = threadIdx.x; j < J; j += 256) {
        const int k = j / D, d = j % D;
        const float raw = z ? tb_g<D>(xr, anchors, iqr, K, k, d) : tb_e(xr, anchors, iqr, K, k, d);
        acc = fmaf(tb_affine(raw, a[j], a[J + j], a[2 * J + j]), gm[j], acc);
    }
    acc = wave_sum_dpp(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        const float v = ((red[0] + red[1]) + (red[2] + red[3])) / (float)(T - z);
        if (z) dw_t[(int64_t)b * (T - 1) + t - 1] = v; else dw_s[n] = v;
    }
}

struct TbBwdArgs {
    const float *x, *anchors, *q, *iq, *aff, *w_s, *w_t, *m_s, *m_t, *rawbar, *corr, *g_s, *g_t;
    const float* dgrad;       // [4, J]: dbeta_s, dgamma_s, dbeta_t, dgamma_t (sweeps 2, 3, training)
    float inv_ns, inv_nt;     // 1 / (B T), 1 / (B (T - 1)) in training mode; 0 with given statistics or without batch norm
    int B, T, K;
    float *dpart, *dot, *dx, *da_part;
    // CONV (triangulation_cnn_attention's chain): the convolutions' weights [K, F, D] and upstream tensors dso, dto [B T, K F]
    const float *cnn_s, *cnn_t, *dso, *dto;
    int F;
    // MAG (triangulation_magnitude's chain), all [B T, K]: it = 1 / sqrt(max(p, eps)) (0 on frame 0 of a clip), s1g = (h . gh) [p > eps]
    // (written by tb_mag_s1, read by the sweeps), dtg = dtau [p > eps], dng = dn [q > eps]
    const float *it, *dtg, *dng;
    float* s1g;
    const float* p;
};

// the temporal operand of a chain: g itself, or (MAG) h = g it
template <int D, bool MAG>
__device__ __forceinline__ float tb_gh(const float* __restrict__ xr, const float* __restrict__ anchors, const float* __restrict__ iqr,
                                       const float* __restrict__ itr, int K, int k, int d) {
    const float g = tb_g<D>(xr, anchors, iqr, K, k, d);
    return MAG ? g * itr[k] : g;
}

// the M V product of one 32-column chunk: tP[t][c] = sum_u M[t,u] tV[u][c], rows by frame index (off = 1: M is over the frames 1 .. T-1)
// CONV: m may be null (no attention), and the convolution's input gradient is added in the same accumulators:
//   tP[t][c] += sum_f dout[t][f] w[f][c],  dout the (clip, anchor)'s [T, F] block (rows KF floats apart), w the anchor's [F, D] block at the chunk
template <bool CONV>
__device__ __forceinline__ void tb_mv(const float* __restrict__ m, int T, int Tp, int off, const float (*tV)[TB_LDV], float (*tP)[TB_LDV],
                                      const float* __restrict__ dout = nullptr, const float* __restrict__ w = nullptr, int64_t KF = 0, int F = 0,
                                      int ldw = 0) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 31;
    const int Tk = T - off;
    for (int job = wave; job < Tp / 32; job += TA_WAVES) {
        const int t0 = 32 * job, tcol = t0 + c - off;
        const bool tok = tcol >= 0 && tcol < Tk;
        f32x16 ac;
#pragma unroll
        for (int r = 0; r < 16; ++r) ac[r] = 0.f;
        if (!CONV || m)
        for (int s2 = 0; s2 < Tp; s2 += 2) {               // A[t][u] = M[u][t] (symmetric): read along M's rows
            const int srow = s2 + (lane >> 5), sr = srow - off;
            const float mv = (tok && sr >= 0 && sr < Tk) ? m[(int64_t)sr * Tk + tcol] : 0.f;
            ac = mfma32(mv, tV[srow][c], ac);
        }
        if (CONV)
            for (int f2 = 0; f2 < F; f2 += 2) {
                const int f = f2 + (lane >> 5);
                const bool fok = f < F;
                const float dv = (tok && fok) ? dout[(int64_t)(t0 + c) * KF + f] : 0.f;
                ac = mfma32(dv, fok ? w[(int64_t)f * ldw + c] : 0.f, ac);
            }
#pragma unroll
        for (int r = 0; r < 16; ++r) tP[t0 + mfma32_row(r, lane)][c] = ac[r];
    }
}

// one (clip, anchor, chunk) of a sweep; `first`: the first anchor this workgroup adds onto its columns of dx (sweep 3)
template <int D, int SWEEP, bool CONV, bool MAG>
__device__ __forceinline__ void tb_bwd_chunk(const TbBwdArgs& A, int b, int k, int c0, bool first, int Tp, float (*tV)[TB_LDV],
                                             float (*tP)[TB_LDV], float (*tR)[TA_LD], float* cw_s, float* cw_t, float* dotacc, float* dacc) {
    const int T = A.T, K = A.K, J = K * D, T1 = T - 1;
    const int c = threadIdx.x & 31, r0 = threadIdx.x >> 5;
    const int d = c0 + c, j = k * D + d;
    const float* xb = A.x + (int64_t)b * T * D;
    const float* iqb = A.iq + (int64_t)b * T * K;
    const float* itb = MAG ? A.it + (int64_t)b * T * K : iqb;       // (read under MAG only)
    const bool attention = A.m_s != nullptr;
    const float two_s = 2.f / (float)T, two_t = 2.f / (float)T1;
    // CONV: V is e / g itself (no affine map), and dV = M V + W^T dout comes whole from tb_mv
    const int64_t KF = (int64_t)K * A.F;
    const float* dout_s = CONV ? A.dso + ((int64_t)b * T * K + k) * A.F : nullptr;
    const float* dout_t = CONV ? A.dto + ((int64_t)b * T * K + k) * A.F : nullptr;
    // ---- spatial ----
    {
        const float sc = CONV ? 1.f : A.aff[j], mu = CONV ? 0.f : A.aff[J + j], be = CONV ? 0.f : A.aff[2 * J + j];
        const float istd = CONV ? 1.f : A.aff[3 * J + j];
        const float gm = CONV ? 0.f : A.g_s[(int64_t)b * 2 * J + j], gq = CONV ? 0.f : A.g_s[(int64_t)b * 2 * J + J + j];
        const float rb = CONV ? 0.f : A.rawbar[(int64_t)b * J + j], cr = CONV ? 0.f : A.corr[(int64_t)b * J + j];
        float c1 = 0.f, c2 = 0.f;
        if (SWEEP > 1) {
            c1 = A.dgrad[j] * A.inv_ns;
            c2 = A.dgrad[J + j] * A.inv_ns;
        }
        if (CONV) {
            if (attention)
                for (int t = r0; t < Tp; t += 8)
                    tV[t][c] = t < T ? tb_e(xb + (int64_t)t * D, A.anchors, iqb + (int64_t)t * K, K, k, d) : 0.f;
            __syncthreads();
            tb_mv<true>(attention ? A.m_s + (int64_t)b * T * T : nullptr, T, Tp, 0, tV, tP, dout_s, A.cnn_s + ((int64_t)k * A.F) * D + c0, KF, A.F,
                        D);
            __syncthreads();
        } else if (attention) {
            for (int t = r0; t < Tp; t += 8)
                tV[t][c] = t < T ? tb_affine(tb_e(xb + (int64_t)t * D, A.anchors, iqb + (int64_t)t * K, K, k, d), sc, mu, be) : 0.f;
            __syncthreads();
            tb_mv<false>(A.m_s + (int64_t)b * T * T, T, Tp, 0, tV, tP);
            __syncthreads();
        }
        float sb = 0.f, sg = 0.f;
        for (int t = r0; t < Tp; t += 8) {
            float draw = 0.f;
            if (t < T) {
                const float raw = tb_e(xb + (int64_t)t * D, A.anchors, iqb + (int64_t)t * K, K, k, d);
                const float hat = (raw - mu) * istd;
                const float dV = CONV ? tP[t][c] : cw_s[t] * gm + (two_s * (sc * ((raw - rb) - cr))) * gq + (attention ? tP[t][c] : 0.f);
                if (SWEEP == 1) {
                    sb += dV;
                    sg = fmaf(dV, hat, sg);
                } else {
                    draw = CONV ? dV : sc * ((dV - c1) - hat * c2);
                }
            }
            if (SWEEP > 1) tR[t][c] = draw;
        }
        if (SWEEP == 1) {                                   // the eight row groups' sums, r = 0, 1, ...
            __syncthreads();
            dacc[r0 * 32 + c] = sb;
            dacc[256 + r0 * 32 + c] = sg;
            __syncthreads();
            if (threadIdx.x < 64) {
                const float* p = dacc + (threadIdx.x >> 5) * 256 + c;
                float acc = p[0];
                for (int r = 1; r < 8; ++r) acc += p[r * 32];
                A.dpart[((int64_t)(threadIdx.x >> 5) * A.B + b) * J + j] = acc;
            }
        }
    }
    __syncthreads();
    // ---- temporal: columns 0 .. 31 are this chunk's; column 32 is feature j0 + 32 (sweeps 2, 3: the roll's other term) ----
    {
        const float* af = CONV ? nullptr : A.aff + (int64_t)4 * J;
        const int jx = (k * D + c0 + TA_CH) % J, kx = jx / D, dx_ = jx % D;         // the 33rd column
        const float sc = CONV ? 1.f : af[j], mu = CONV ? 0.f : af[J + j], be = CONV ? 0.f : af[2 * J + j], istd = CONV ? 1.f : af[3 * J + j];
        const float gm = CONV ? 0.f : A.g_t[(int64_t)b * 2 * J + j], gq = CONV ? 0.f : A.g_t[(int64_t)b * 2 * J + J + j];
        const float rb = CONV ? 0.f : A.rawbar[((int64_t)A.B + b) * J + j], cr = CONV ? 0.f : A.corr[((int64_t)A.B + b) * J + j];
        const float scx = CONV ? 1.f : af[jx], mux = CONV ? 0.f : af[J + jx], bex = CONV ? 0.f : af[2 * J + jx], istdx = CONV ? 1.f : af[3 * J + jx];
        float c1 = 0.f, c2 = 0.f, c1x = 0.f, c2x = 0.f;
        if (SWEEP > 1) {
            c1 = A.dgrad[2 * J + j] * A.inv_nt;
            c2 = A.dgrad[3 * J + j] * A.inv_nt;
            c1x = A.dgrad[2 * J + jx] * A.inv_nt;
            c2x = A.dgrad[3 * J + jx] * A.inv_nt;
        }
        const float* mt = attention ? A.m_t + (int64_t)b * T1 * T1 : nullptr;
        if (CONV) {
            if (attention) {
                for (int t = r0; t < Tp; t += 8)
                    tV[t][c] = (t >= 1 && t < T) ? tb_gh<D, MAG>(xb + (int64_t)t * D, A.anchors, iqb + (int64_t)t * K, itb + (int64_t)t * K, K, k, d) : 0.f;
                for (int t = threadIdx.x; t < Tp; t += 64 * TA_WAVES)
                    tV[t][TA_CH] =
                        (t >= 1 && t < T) ? tb_gh<D, MAG>(xb + (int64_t)t * D, A.anchors, iqb + (int64_t)t * K, itb + (int64_t)t * K, K, kx, dx_) : 0.f;
            }
            __syncthreads();
            tb_mv<true>(mt, T, Tp, 1, tV, tP, dout_t, A.cnn_t + ((int64_t)k * A.F) * D + c0, KF, A.F, D);
            for (int t = threadIdx.x; t < Tp; t += 64 * TA_WAVES) {             // the 33rd column: plain loops over u and over f
                float acc = 0.f;
                if (t >= 1 && t < T) {
                    if (attention)
                        for (int u = 1; u < T; ++u) acc = fmaf(mt[(int64_t)(u - 1) * T1 + (t - 1)], tV[u][TA_CH], acc);
                    const float* dr = A.dto + (((int64_t)b * T + t) * K + kx) * A.F;
                    const float* wx = A.cnn_t + ((int64_t)kx * A.F) * D + dx_;
                    for (int f = 0; f < A.F; ++f) acc = fmaf(dr[f], wx[(int64_t)f * D], acc);
                }
                tP[t][TA_CH] = acc;
            }
            __syncthreads();
        } else if (attention) {
            for (int t = r0; t < Tp; t += 8)
                tV[t][c] = (t >= 1 && t < T) ? tb_affine(tb_g<D>(xb + (int64_t)t * D, A.anchors, iqb + (int64_t)t * K, K, k, d), sc, mu, be) : 0.f;
            if (SWEEP > 1)
                for (int t = threadIdx.x; t < Tp; t += 64 * TA_WAVES)
                    tV[t][TA_CH] = (t >= 1 && t < T) ? tb_affine(tb_g<D>(xb + (int64_t)t * D, A.anchors, iqb + (int64_t)t * K, K, kx, dx_), scx, mux, bex)
                                                     : 0.f;
            __syncthreads();
            tb_mv<false>(mt, T, Tp, 1, tV, tP);
            if (SWEEP > 1)
                for (int t = threadIdx.x; t < Tp; t += 64 * TA_WAVES) {
                    float acc = 0.f;
                    if (t >= 1 && t < T)
                        for (int u = 1; u < T; ++u) acc = fmaf(mt[(int64_t)(u - 1) * T1 + (t - 1)], tV[u][TA_CH], acc);
                    tP[t][TA_CH] = acc;
                }
            __syncthreads();
        }
        float sb = 0.f, sg = 0.f;
        for (int t = r0; t < Tp; t += 8) {
            float draw = 0.f;
            if (t >= 1 && t < T) {
                const float raw = tb_g<D>(xb + (int64_t)t * D, A.anchors, iqb + (int64_t)t * K, K, k, d);
                const float hat = (raw - mu) * istd;
                const float dV = CONV ? tP[t][c] : cw_t[t] * gm + (two_t * (sc * ((raw - rb) - cr))) * gq + (attention ? tP[t][c] : 0.f);
                if (SWEEP == 1) {
                    sb += dV;
                    sg = fmaf(dV, hat, sg);
                } else if (MAG) {                          // gg from gh = dV: the second normalisation's backward and tau's own gradient
                    const int64_t m = ((int64_t)b * T + t) * K + k;
                    const float itau = A.it[m], h = raw * itau;
                    draw = itau * (dV - h * A.s1g[m]) + A.dtg[m] * h;
                } else {
                    draw = CONV ? dV : sc * ((dV - c1) - hat * c2);
                }
            }
            if (SWEEP > 1) tV[t][c] = draw;                 // (this thread's own element: nothing else reads it before the barrier)
        }
        if (SWEEP == 1) {
            __syncthreads();
            dacc[r0 * 32 + c] = sb;
            dacc[256 + r0 * 32 + c] = sg;
            __syncthreads();
            if (threadIdx.x < 64) {
                const float* p = dacc + (threadIdx.x >> 5) * 256 + c;
                float acc = p[0];
                for (int r = 1; r < 8; ++r) acc += p[r * 32];
                A.dpart[((int64_t)(2 + (threadIdx.x >> 5)) * A.B + b) * J + j] = acc;
            }
            __syncthreads();
            return;
        }
        // the 33rd column's draw
        const float gmx = CONV ? 0.f : A.g_t[(int64_t)b * 2 * J + jx], gqx = CONV ? 0.f : A.g_t[(int64_t)b * 2 * J + J + jx];
        const float rbx = CONV ? 0.f : A.rawbar[((int64_t)A.B + b) * J + jx], crx = CONV ? 0.f : A.corr[((int64_t)A.B + b) * J + jx];
        for (int t = threadIdx.x; t < Tp; t += 64 * TA_WAVES) {
            float draw = 0.f;
            if (t >= 1 && t < T) {
                const float raw = tb_g<D>(xb + (int64_t)t * D, A.anchors, iqb + (int64_t)t * K, K, kx, dx_);
                const float hat = (raw - mux) * istdx;
                const float dV = CONV ? tP[t][TA_CH] : cw_t[t] * gmx + (two_t * (scx * ((raw - rbx) - crx))) * gqx + (attention ? tP[t][TA_CH] : 0.f);
                if (MAG) {
                    const int64_t m = ((int64_t)b * T + t) * K + kx;
                    const float itau = A.it[m], h = raw * itau;
                    draw = itau * (dV - h * A.s1g[m]) + A.dtg[m] * h;
                } else {
                    draw = CONV ? dV : scx * ((dV - c1x) - hat * c2x);
                }
            }
            tV[t][TA_CH] = draw;
        }
    }
    __syncthreads();
    // ---- de = draw_s + draw_t - draw_t[next feature], then the clamped normalisation ----
    float da = 0.f;
    for (int t = r0; t < Tp; t += 8) {
        const bool valid = t < T;
        float v = 0.f;
        if (valid) {
            const int64_t n = (int64_t)b * T + t;
            const float de = tR[t][c] + tV[t][c] - tV[t][c + 1];
            const float eh = tb_e(xb + (int64_t)t * D, A.anchors, iqb + (int64_t)t * K, K, k, d);
            if (SWEEP == 2) {
                v = eh * de;
            } else {
                const float qg = A.q[n * K + k] > kL2Eps ? 1.f : 0.f;
                float gr = A.iq[n * K + k] * (de - eh * (A.dot[n * K + k] * qg));
                if (MAG) gr = gr + A.dng[n * K + k] * eh;  // n = |x - a_k| is an output
                float* po = A.dx + n * D + d;
                *po = first ? gr : *po + gr;               // (an earlier anchor of this workgroup: this thread wrote it)
                da += gr;
            }
        }
        if (SWEEP == 2) {
            v = half_sum(v);                                // the 32 columns of the chunk: one half-wave per frame
            if (c == 0 && valid) dotacc[t] += v;
        }
    }
    if (SWEEP == 3) {
        dacc[r0 * 32 + c] = da;
        __syncthreads();
        if (threadIdx.x < 32) {
            float acc = dacc[c];
            for (int r = 1; r < 8; ++r) acc += dacc[r * 32 + c];
            A.da_part[((int64_t)b * K + k) * D + d] = acc;
        }
    }
    __syncthreads();
}

// MAG's sweep in front of the other two, one (clip, anchor, chunk): dotacc[t] += sum_c h[t][c] gh[t][c],  gh = M_t H + W_t^T dto
template <int D>
__device__ __forceinline__ void tb_mag_s1_chunk(const TbBwdArgs& A, int b, int k, int c0, int Tp, float (*tV)[TB_LDV], float (*tP)[TB_LDV],
                                                float* dotacc) {
    const int T = A.T, K = A.K, T1 = T - 1;
    const int c = threadIdx.x & 31, r0 = threadIdx.x >> 5;
    const int d = c0 + c;
    const float* xb = A.x + (int64_t)b * T * D;
    const float* iqb = A.iq + (int64_t)b * T * K;
    const float* itb = A.it + (int64_t)b * T * K;
    for (int t = r0; t < Tp; t += 8)
        tV[t][c] = (t >= 1 && t < T) ? tb_gh<D, true>(xb + (int64_t)t * D, A.anchors, iqb + (int64_t)t * K, itb + (int64_t)t * K, K, k, d) : 0.f;
    __syncthreads();
    tb_mv<true>(A.m_t ? A.m_t + (int64_t)b * T1 * T1 : nullptr, T, Tp, 1, tV, tP, A.dto + ((int64_t)b * T * K + k) * A.F,
                A.cnn_t + ((int64_t)k * A.F) * D + c0, (int64_t)K * A.F, A.F, D);
    __syncthreads();
    for (int t = r0; t < Tp; t += 8) {
        const float v = half_sum(tV[t][c] * tP[t][c]);     // the 32 columns of the chunk: one half-wave per frame
        if (c == 0 && t < T) dotacc[t] += v;
    }
    __syncthreads();
}

// a workgroup per (clip, anchor): s1g[n,k] = (h . gh) [p > eps]
template <int D>
__global__ __launch_bounds__(64 * TA_WAVES) void tb_mag_s1_kernel(const TbBwdArgs A) {
    extern __shared__ __attribute__((aligned(16))) float tb_sh[];
    const int T = A.T, K = A.K, Tp = (T + 31) & ~31;
    float (*tV)[TB_LDV] = reinterpret_cast<float (*)[TB_LDV]>(tb_sh);
    float (*tP)[TB_LDV] = tV + Tp;
    float* dotacc = tb_sh + 2 * Tp * TB_LDV;
    const int b = blockIdx.x / K, k = blockIdx.x % K;
    for (int t = threadIdx.x; t < Tp; t += 64 * TA_WAVES) dotacc[t] = 0.f;
    __syncthreads();
    for (int c0 = 0; c0 < D; c0 += TA_CH) tb_mag_s1_chunk<D>(A, b, k, c0, Tp, tV, tP, dotacc);
    for (int t = threadIdx.x; t < T; t += 64 * TA_WAVES) {
        const int64_t m = ((int64_t)b * T + t) * K + k;
        A.s1g[m] = A.p[m] > kL2Eps ? dotacc[t] : 0.f;      // (frame 0 of a clip: p = -1)
    }
}

template <int D, int SWEEP, bool CONV = false, bool MAG = false>
__global__ __launch_bounds__(64 * TA_WAVES) void tb_bwd_kernel(const TbBwdArgs A) {
    extern __shared__ __attribute__((aligned(16))) float tb_sh[];
    const int T = A.T, K = A.K, Tp = (T + 31) & ~31;
    float (*tV)[TB_LDV] = reinterpret_cast<float (*)[TB_LDV]>(tb_sh);
    float (*tP)[TB_LDV] = tV + Tp;
    float (*tR)[TA_LD] = reinterpret_cast<float (*)[TA_LD]>(tb_sh + 2 * Tp * TB_LDV);
    float* cw_s = tb_sh + 2 * Tp * TB_LDV + Tp * TA_LD;
    float *cw_t = cw_s + Tp, *dotacc = cw_t + Tp, *dacc = dotacc + Tp;
    constexpr int NCH = D / TA_CH;
    const int b = SWEEP == 3 ? blockIdx.x / NCH : blockIdx.x / K;
    const int rest = SWEEP == 3 ? blockIdx.x % NCH : blockIdx.x % K;
    for (int t = threadIdx.x; t < Tp; t += 64 * TA_WAVES) {    // the mean's weight of every frame, by frame index
        cw_s[t] = (!CONV && t < T) ? (A.w_s ? A.w_s[(int64_t)b * T + t] : 1.f) / (float)T : 0.f;
        cw_t[t] = (!CONV && t >= 1 && t < T) ? (A.w_t ? A.w_t[(int64_t)b * (T - 1) + t - 1] : 1.f) / (float)(T - 1) : 0.f;
        dotacc[t] = 0.f;
    }
    __syncthreads();
    if (SWEEP == 3) {
        for (int k = 0; k < K; ++k) tb_bwd_chunk<D, SWEEP, CONV, MAG>(A, b, k, rest * TA_CH, k == 0, Tp, tV, tP, tR, cw_s, cw_t, dotacc, dacc);
    } else {
        for (int c0 = 0; c0 < D; c0 += TA_CH) tb_bwd_chunk<D, SWEEP, CONV, MAG>(A, b, rest, c0, false, Tp, tV, tP, tR, cw_s, cw_t, dotacc, dacc);
        if (SWEEP == 2)
            for (int t = threadIdx.x; t < T; t += 64 * TA_WAVES) A.dot[((int64_t)b * T + t) * K + rest] = dotacc[t];
    }
}

static int tb_slices(int B, int T, int K) {
    const int64_t wg = (int64_t)B * ta_tiles(T) * ta_tiles(T);
    int64_t want = (512 + wg - 1) / wg;
    want = want < 1 ? 1 : (want > TA_MAX_SLICES ? TA_MAX_SLICES : want);
    return (int)(K < want ? K : want);
}
static size_t tb_bwd_lds(int T) {
    const int Tp = (T + 31) & ~31;
    return ((size_t)Tp * (2 * TB_LDV + TA_LD + 3) + 2 * 8 * 32) * sizeof(float);
}
static int tb_check(const char* name, int B, int T, int D, int K) {
    if (const int rc = ta_check(name, B, T, D, K)) return rc;
    LPM_REQUIRE(B <= 65535 && (int64_t)B * T * K < (1ll << 31) && (int64_t)B * K * D < (1ll << 29), LPM_ERR_UNSUPPORTED_SHAPE,
                "%s: B, B * T * K or B * K * D too large (B=%d T=%d K=%d)", name, B, T, K);
    return LPM_OK;
}

// the body of the two Gram entries: the slices' partial Grams (or the Grams themselves with one slice), then their sums in slice order;
// it [B T, K] is read under MAG only
template <bool MAG>
static int tb_gram_launch(const char* name, const float* x, const float* anchors, const float* iq, const float* it, const float* aff, int B, int T,
                          int D, int K, float* gram_s, float* gram_t, void* workspace, size_t workspace_bytes, hipStream_t s) {
    if (const int rc = tb_check(name, B, T, D, K)) return rc;
    const size_t need = lpm_triangulation_bn_moments_workspace_bytes(1, B, T, D, K);
    LPM_REQUIRE(need == 0 || (workspace && workspace_bytes >= need), LPM_ERR_WORKSPACE, "%s: workspace too small", name);
    const int S = tb_slices(B, T, K), NT = ta_tiles(T), T1 = T - 1;
    float* part_s = S > 1 ? (float*)workspace : gram_s;
    float* part_t = S > 1 ? part_s + (size_t)B * S * T * T : gram_t;
    const dim3 grid((unsigned)(B * S * NT * NT)), block(64 * TA_WAVES);
    tp_dispatch_d(D, [&](auto d) {
        hipLaunchKernelGGL((tb_gram_kernel<decltype(d)::value, MAG>), grid, block, 0, s, x, anchors, iq, it, aff, T, K, S, NT, part_s, part_t);
    });
    if (S > 1) {
        if (const int rc = ta_sum_slices(part_s, B, (int64_t)T * T, S, gram_s, s, name)) return rc;
        if (const int rc = ta_sum_slices(part_t, B, (int64_t)T1 * T1, S, gram_t, s, name)) return rc;
    }
    return check_launch(name);
}

// What the three chains share.  A arrives value-initialised with the fields its policy reads and the entry's carving of the workspace
// (dot, da_part among it); this fills in the operands every policy reads, runs the entry's own `sweep1(d, A, grid_k, block, lds)` -- the
// sweeps in front of the other two differ in kind --, then sweeps 2 and 3 and the sum of the danchors partials.
template <bool CONV, bool MAG, class Sweep1>
static int tb_chain_launch(const char* name, TbBwdArgs A, const float* x, const float* anchors, const float* q, const float* m_s, const float* m_t,
                           int B, int T, int D, int K, float* dx, float* danchors, hipStream_t s, Sweep1 sweep1) {
    A.x = x; A.anchors = anchors; A.q = q; A.iq = q + (int64_t)B * T * K; A.m_s = m_s; A.m_t = m_t;
    A.B = B; A.T = T; A.K = K;
    A.dx = dx;
    const size_t lds = tb_bwd_lds(T);
    const dim3 block(64 * TA_WAVES), grid_k((unsigned)(B * K)), grid_c((unsigned)(B * (D / TA_CH)));
    tp_dispatch_d(D, [&](auto d) {
        constexpr int DD = decltype(d)::value;
        sweep1(d, A, grid_k, block, lds);
        hipLaunchKernelGGL((tb_bwd_kernel<DD, 2, CONV, MAG>), grid_k, block, lds, s, A);
        hipLaunchKernelGGL((tb_bwd_kernel<DD, 3, CONV, MAG>), grid_c, block, lds, s, A);
    });
    if (const int rc = ta_reduce_partials(dx, A.da_part, B, T, D, K, 1, TP_SUM_CHUNK, dx, danchors, s, name)) return rc;
    return check_launch(name);
}

}  // namespace lpm

extern "C" size_t lpm_triangulation_bn_moments_workspace_bytes(int which, int B, int T, int D, int K) {
    if (B <= 0 || T <= 1 || D <= 0 || K <= 0) return 0;
    const size_t J = (size_t)K * D, T1 = (size_t)T - 1;
    if (which == 0) return 4 * (size_t)B * J * sizeof(float);                      // stats: per-clip sums of both streams, twice
    if (which == 1) {                                                               // gram: the slices' partial Grams
        const int S = lpm::tb_slices(B, T, K);
        return S > 1 ? (size_t)B * S * ((size_t)T * T + T1 * T1) * sizeof(float) : 0;
    }
    // bwd: per-clip dbeta / dgamma sums, the dot products, danchors partials
    return (4 * (size_t)B * J + (size_t)B * T * K + (size_t)B * J) * sizeof(float);
}

extern "C" int lpm_triangulation_bn_moments_stats(const float* x, const float* anchors, int B, int T, int D, int K, int want_stats, float* q,
                                                  float* stats, void* workspace, size_t workspace_bytes, lpm_stream_t stream) {
    using namespace lpm;
    const char* name = "lpm_triangulation_bn_moments_stats";
    LPM_REQUIRE(x && anchors && q && (stats || !want_stats), LPM_ERR_BADARG, "%s: null pointer", name);
    if (const int rc = tb_check(name, B, T, D, K)) return rc;
    LPM_REQUIRE(!want_stats || (workspace && workspace_bytes >= lpm_triangulation_bn_moments_workspace_bytes(0, B, T, D, K)), LPM_ERR_WORKSPACE,
                "%s: workspace too small", name);
    LPM_REQUIRE(((uintptr_t)x & 15) == 0, LPM_ERR_BADARG, "%s: x must be 16-byte aligned", name);
    hipStream_t s = (hipStream_t)stream;
    const int64_t BT = (int64_t)B * T;
    const int J = K * D, nj = (J + 255) / 256;
    const dim3 grid_n((unsigned)((BT * ((K + TB_KC - 1) / TB_KC) + TA_WAVES - 1) / TA_WAVES)), block(64 * TA_WAVES);
    const float* iq = q + BT * K;
    float* part = (float*)workspace;
    const float inv_s = 1.f / (float)BT, inv_t = 1.f / (float)(BT - B);
    tp_dispatch_d(D, [&](auto d) {
        constexpr int DD = decltype(d)::value;
        hipLaunchKernelGGL(tb_norms_kernel<DD>, grid_n, block, 0, s, x, anchors, BT, K, q);
        if (!want_stats) return;
        hipLaunchKernelGGL((tb_stats_kernel<DD, 0>), dim3(nj, B, 2), dim3(256), 0, s, x, anchors, iq, stats, B, T, K, part);
        hipLaunchKernelGGL(tb_colsum_kernel, dim3(nj, 2), dim3(256), 0, s, part, B, J, (int64_t)2 * J, inv_s, inv_t, 0, stats);
        hipLaunchKernelGGL((tb_stats_kernel<DD, 1>), dim3(nj, B, 2), dim3(256), 0, s, x, anchors, iq, stats, B, T, K, part);
        hipLaunchKernelGGL(tb_colsum_kernel, dim3(nj, 2), dim3(256), 0, s, part, B, J, (int64_t)2 * J, inv_s, inv_t, 0, stats + J);
        hipLaunchKernelGGL(tb_colsum_kernel, dim3(nj, 2), dim3(256), 0, s, part + (size_t)2 * B * J, B, J, (int64_t)2 * J, inv_s, inv_t, 1, stats);
    });
    return check_launch(name);
}

extern "C" int lpm_triangulation_bn_moments_gram(const float* x, const float* anchors, const float* iq, const float* aff, int B, int T, int D,
                                                 int K, float* gram_s, float* gram_t, void* workspace, size_t workspace_bytes,
                                                 lpm_stream_t stream) {
    using namespace lpm;
    const char* name = "lpm_triangulation_bn_moments_gram";
    LPM_REQUIRE(x && anchors && iq && aff && gram_s && gram_t, LPM_ERR_BADARG, "%s: null pointer", name);
    return tb_gram_launch<false>(name, x, anchors, iq, nullptr, aff, B, T, D, K, gram_s, gram_t, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int lpm_triangulation_bn_moments_pool(const float* x, const float* anchors, const float* iq, const float* aff, const float* w_s,
                                                 const float* w_t, int B, int T, int D, int K, float* pool_s, float* pool_t, float* rawbar,
                                                 float* corr, lpm_stream_t stream) {
    using namespace lpm;
    const char* name = "lpm_triangulation_bn_moments_pool";
    LPM_REQUIRE(x && anchors && iq && aff && pool_s && pool_t && rawbar && corr && !w_s == !w_t, LPM_ERR_BADARG, "%s: null pointer", name);
    if (const int rc = tb_check(name, B, T, D, K)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((K * D + 255) / 256, B, 2), block(256);
    tp_dispatch_d(D, [&](auto d) {
        hipLaunchKernelGGL(tb_pool_kernel<decltype(d)::value>, grid, block, 0, s, x, anchors, iq, aff, w_s, w_t, B, T, K, pool_s, pool_t, rawbar, corr);
    });
    return check_launch(name);
}

extern "C" int lpm_triangulation_bn_moments_dw(const float* x, const float* anchors, const float* iq, const float* aff, const float* g_s,
                                               const float* g_t, int B, int T, int D, int K, float* dw_s, float* dw_t, lpm_stream_t stream) {
    using namespace lpm;
    const char* name = "lpm_triangulation_bn_moments_dw";
    LPM_REQUIRE(x && anchors && iq && aff && g_s && g_t && dw_s && dw_t, LPM_ERR_BADARG, "%s: null pointer", name);
    if (const int rc = tb_check(name, B, T, D, K)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(B * T, 2), block(256);
    tp_dispatch_d(D, [&](auto d) {
        hipLaunchKernelGGL(tb_dw_kernel<decltype(d)::value>, grid, block, 0, s, x, anchors, iq, aff, g_s, g_t, T, K, dw_s, dw_t);
    });
    return check_launch(name);
}

extern "C" int lpm_triangulation_bn_moments_bwd(const float* x, const float* anchors, const float* q, const float* aff, const float* w_s,
                                                const float* w_t, const float* m_s, const float* m_t, const float* rawbar, const float* corr,
                                                const float* g_s, const float* g_t, int B, int T, int D, int K, int affine_grads, int training,
                                                float* dx, float* danchors, float* dgrad, void* workspace, size_t workspace_bytes,
                                                lpm_stream_t stream) {
    using namespace lpm;
    const char* name = "lpm_triangulation_bn_moments_bwd";
    LPM_REQUIRE(x && anchors && q && aff && rawbar && corr && g_s && g_t && dx && danchors && dgrad, LPM_ERR_BADARG, "%s: null pointer", name);
    LPM_REQUIRE(!w_s == !w_t && !m_s == !m_t && !w_s == !m_s, LPM_ERR_BADARG, "%s: the weights and M of both streams, or none", name);
    LPM_REQUIRE(affine_grads || !training, LPM_ERR_BADARG, "%s: training mode needs the affine gradients", name);
    if (const int rc = tb_check(name, B, T, D, K)) return rc;
    LPM_REQUIRE(workspace && workspace_bytes >= lpm_triangulation_bn_moments_workspace_bytes(2, B, T, D, K), LPM_ERR_WORKSPACE,
                "%s: workspace too small", name);
    hipStream_t s = (hipStream_t)stream;
    const int64_t BT = (int64_t)B * T;
    const int J = K * D;
    if (const int rc = tp_reserve_lds<tb_bwd_kernel<1024, 1>, tb_bwd_kernel<1024, 2>, tb_bwd_kernel<1024, 3>, tb_bwd_kernel<128, 1>,
                                      tb_bwd_kernel<128, 2>, tb_bwd_kernel<128, 3>>(name, (int)tb_bwd_lds(TA_MAX_FRAMES)))
        return rc;
    TbBwdArgs A{};
    A.aff = aff; A.w_s = w_s; A.w_t = w_t; A.rawbar = rawbar; A.corr = corr; A.g_s = g_s; A.g_t = g_t; A.dgrad = dgrad;
    A.inv_ns = training ? 1.f / (float)BT : 0.f;
    A.inv_nt = training ? 1.f / (float)(BT - B) : 0.f;
    A.dpart = (float*)workspace;
    A.dot = A.dpart + (size_t)4 * B * J;
    A.da_part = A.dot + (size_t)BT * K;
    return tb_chain_launch<false, false>(name, A, x, anchors, q, m_s, m_t, B, T, D, K, dx, danchors, s,
                                         [&](auto d, const TbBwdArgs& args, dim3 grid_k, dim3 block, size_t lds) {
        if (affine_grads) {
            hipLaunchKernelGGL((tb_bwd_kernel<decltype(d)::value, 1>), grid_k, block, lds, s, args);
            hipLaunchKernelGGL(tb_colsum_kernel, dim3((J + 255) / 256, 4), dim3(256), 0, s, args.dpart, B, J, (int64_t)J, 1.f, 1.f, 0, dgrad);
        } else {
            (void)hipMemsetAsync(dgrad, 0, (size_t)4 * J * sizeof(float), s);
        }
    });
}

// ---- the chain of triangulation_cnn_attention (TriangulationNsCnnIndirectAttentionModule, JuhanTestModelV2): tb_bwd's sweeps 2 and 3 under the
// CONV policy -- V = e / g themselves, dV = M V + W^T dout from one accumulator, no batch norm, hence no sweep 1 ----
extern "C" size_t lpm_triangulation_cnn_attention_workspace_bytes(int B, int T, int D, int K) {
    if (B <= 0 || T <= 1 || D <= 0 || K <= 0) return 0;
    return ((size_t)B * T * K + (size_t)B * K * D) * sizeof(float);                 // the dot products, danchors partials
}

extern "C" int lpm_triangulation_cnn_attention_bwd(const float* x, const float* anchors, const float* q, const float* cnn_s, const float* cnn_t,
                                                   const float* dso, const float* dto, const float* m_s, const float* m_t, int B, int T, int D,
                                                   int K, int F, float* dx, float* danchors, void* workspace, size_t workspace_bytes,
                                                   lpm_stream_t stream) {
    using namespace lpm;
    const char* name = "lpm_triangulation_cnn_attention_bwd";
    LPM_REQUIRE(x && anchors && q && cnn_s && cnn_t && dso && dto && dx && danchors, LPM_ERR_BADARG, "%s: null pointer", name);
    LPM_REQUIRE(!m_s == !m_t, LPM_ERR_BADARG, "%s: M of both streams, or none", name);
    if (const int rc = tb_check(name, B, T, D, K)) return rc;
    LPM_REQUIRE(F >= 1 && (int64_t)B * T * K * F < (1ll << 31), LPM_ERR_UNSUPPORTED_SHAPE, "%s: need F >= 1 and B * T * K * F < 2^31 (F=%d)", name, F);
    LPM_REQUIRE(workspace && workspace_bytes >= lpm_triangulation_cnn_attention_workspace_bytes(B, T, D, K), LPM_ERR_WORKSPACE,
                "%s: workspace too small", name);
    if (const int rc = tp_reserve_lds<tb_bwd_kernel<1024, 2, true>, tb_bwd_kernel<1024, 3, true>, tb_bwd_kernel<128, 2, true>,
                                      tb_bwd_kernel<128, 3, true>>(name, (int)tb_bwd_lds(TA_MAX_FRAMES)))
        return rc;
    TbBwdArgs A{};
    A.cnn_s = cnn_s; A.cnn_t = cnn_t; A.dso = dso; A.dto = dto; A.F = F;
    A.dot = (float*)workspace;
    A.da_part = A.dot + (size_t)B * T * K;
    return tb_chain_launch<true, false>(name, A, x, anchors, q, m_s, m_t, B, T, D, K, dx, danchors, (hipStream_t)stream,
                                        [](auto, const TbBwdArgs&, dim3, dim3, size_t) {});      // no batch norm: no sweep 1
}

// ---- triangulation_magnitude (TriangulationMagnitudeNsCnnIndirectAttentionModule, JuhanTestModelV3): the Grams with the temporal operand
// normalised again, and the chain under the MAG policy -- tb_mag_s1, then tb_bwd's sweeps 2 and 3.  q, p [2, B T, K] are tv_norms'
// (lpm_triangulation_magnitude_norms): the squared norms, then their clamped reciprocal roots ----
extern "C" int lpm_triangulation_magnitude_gram(const float* x, const float* anchors, const float* q, const float* p, const float* aff, int B, int T,
                                                int D, int K, float* gram_s, float* gram_t, void* workspace, size_t workspace_bytes,
                                                lpm_stream_t stream) {
    using namespace lpm;
    const char* name = "lpm_triangulation_magnitude_gram";
    LPM_REQUIRE(x && anchors && q && p && aff && gram_s && gram_t, LPM_ERR_BADARG, "%s: null pointer", name);
    const int64_t BTK = (int64_t)B * T * K;                // (tb_check comes first in the launcher: nothing is read through these before it)
    return tb_gram_launch<true>(name, x, anchors, q + BTK, p + BTK, aff, B, T, D, K, gram_s, gram_t, workspace, workspace_bytes,
                                (hipStream_t)stream);
}

extern "C" size_t lpm_triangulation_magnitude_workspace_bytes(int B, int T, int D, int K) {
    if (B <= 0 || T <= 1 || D <= 0 || K <= 0) return 0;
    return (2 * (size_t)B * T * K + (size_t)B * K * D) * sizeof(float);             // s1g, the dot products, danchors partials
}

extern "C" int lpm_triangulation_magnitude_bwd(const float* x, const float* anchors, const float* q, const float* p, const float* cnn_s,
                                               const float* cnn_t, const float* dso, const float* dto, const float* dng, const float* dtg,
                                               const float* m_s, const float* m_t, int B, int T, int D, int K, int F, float* dx, float* danchors,
                                               void* workspace, size_t workspace_bytes, lpm_stream_t stream) {
    using namespace lpm;
    const char* name = "lpm_triangulation_magnitude_bwd";
    LPM_REQUIRE(x && anchors && q && p && cnn_s && cnn_t && dso && dto && dng && dtg && dx && danchors, LPM_ERR_BADARG, "%s: null pointer", name);
    LPM_REQUIRE(!m_s == !m_t, LPM_ERR_BADARG, "%s: M of both streams, or none", name);
    if (const int rc = tb_check(name, B, T, D, K)) return rc;
    LPM_REQUIRE(F >= 1 && (int64_t)B * T * K * F < (1ll << 31), LPM_ERR_UNSUPPORTED_SHAPE, "%s: need F >= 1 and B * T * K * F < 2^31 (F=%d)", name, F);
    LPM_REQUIRE(workspace && workspace_bytes >= lpm_triangulation_magnitude_workspace_bytes(B, T, D, K), LPM_ERR_WORKSPACE,
                "%s: workspace too small", name);
    hipStream_t s = (hipStream_t)stream;
    const int64_t BT = (int64_t)B * T;
    if (const int rc = tp_reserve_lds<tb_mag_s1_kernel<1024>, tb_mag_s1_kernel<128>, tb_bwd_kernel<1024, 2, true, true>,
                                      tb_bwd_kernel<1024, 3, true, true>, tb_bwd_kernel<128, 2, true, true>, tb_bwd_kernel<128, 3, true, true>>(
            name, (int)tb_bwd_lds(TA_MAX_FRAMES)))
        return rc;
    TbBwdArgs A{};
    A.cnn_s = cnn_s; A.cnn_t = cnn_t; A.dso = dso; A.dto = dto; A.F = F;
    A.p = p; A.it = p + BT * K; A.dtg = dtg; A.dng = dng;
    A.s1g = (float*)workspace;
    A.dot = A.s1g + (size_t)BT * K;
    A.da_part = A.dot + (size_t)BT * K;
    return tb_chain_launch<true, true>(name, A, x, anchors, q, m_s, m_t, B, T, D, K, dx, danchors, s,
                                       [&](auto d, const TbBwdArgs& args, dim3 grid_k, dim3 block, size_t lds) {
        hipLaunchKernelGGL(tb_mag_s1_kernel<decltype(d)::value>, grid_k, block, lds, s, args);
    });
}
