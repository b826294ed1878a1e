// The pooled convolution moments of TriangulationV5Module (video_pooling_modules.py:182-276, JuhanTestModelV5): per anchor k of the
// [D, K] anchors (as they are: not normalised) and frame row m = b T + t of x [(B T), D]
//   q = |x - a_k|^2, n = sqrt(q), e = (x - a_k) rsqrt(max(q, 1e-12))                                    (tf.norm, tf.nn.l2_normalize)
//   g[k,d] = e[k,d] - e[k,d-1] with e[k,-1] := e[(k-1) mod K, D-1]  (tf.manip.roll over the FEATURE axis of the flattened [K D] row,
//   :216), frame 0 of every clip dropped;  p = |g|^2, tau = sqrt(p), h = g rsqrt(max(p, 1e-12))
//   so[m,k,f] = sum_d Ws[k,f,d] e[m,k,d]       to[m,k,f] = sum_d Wt[k,f,d] h[m,k,d]                      (the per-anchor convolutions)
//   pool = [mean_t | mean_t (. - mean)^2] of [so | n] over the T frames and of [to | tau] over the T - 1 frames t >= 1.
// The variance does not commute with the convolution, so both products run over every frame: 2 (B T) K F D FLOP each.  Nothing of
// size B T K D is written in either direction: e and h are generated from the frames where a product reads them (the residual x - a
// is formed first, as tp_unit does; h takes column d-1 from the frames as well).  What IS written: q, p [2, B T, K] (the squared norms and their clamped reciprocal roots), so, to [B T, K F]
// (saved for the backward: the gradient of a variance needs every frame's value), and in the backward the two upstream tensors
// dso, dto [B T, K F], a handful of [B T, K] sums, one danchors partial per 128-row tile and at most TV_MAX_GROUPS partial copies of dx.
// No floating-point atomics: every cross-workgroup sum has a fixed order.  All products on v_mfma_f32_32x32x2_f32 (exact fp32).
//
// forward: tv_norms (one wave per frame row and 16 anchors: q, p by direct sums of squares) -> tv_conv (a workgroup owns an anchor, 32
// filters and 128 frame rows ACROSS clips: per 32-column chunk of D the e and h tiles [128, 33] and the two weight tiles go to LDS, one
// 32x32 product per wave and stream; the row tiles of one weight tile are neighbours in the grid) -> tm_pool (a thread per clip and
// column: the mean, then the squared deviations from it, both two-level over t).
//
// backward, with (gm, gv) the upstream gradient of a pool and T' its frame count: dout[t] = (gm + 2 gv ((out[t] - mean) - c)) / T', where
// c = mean_t (out[t] - mean) is what the rounded mean is off by (zero in exact arithmetic; autograd has the same term through d mean /
// d out: without it the error of the mean, the same for every frame of a clip, adds up over the frames in danchors).
//   dW[k] = sum_m dout (x) operand:  tv_dw, a wave owns a 32 x 32 tile of dW[k] and walks all B T rows (operands straight from the
//   frames into the MFMA's registers; two-level over the rows).
//   operand gradients ge = Ws_k^T dso, gh = Wt_k^T dto, then the two normalisations with the norms' own gradients dn, dtau:
//     gg[d] = itau (gh[d] - h[d] (h . gh) [p > eps]) + dtau [p > eps] h[d]              (gradient of g; (h . gh) = sum_f dto to)
//     get[d] = ge[d] + gg[d] - gg[next(d)]     (next(k, D-1) = (k+1 mod K, 0): the boundary term, taken from tv_dout's [B T, K] column)
//     gr[d] = iq (get[d] - e[d] (e . get) [q > eps]) + dn [q > eps] e[d]                dx = sum_k gr,  danchors[:,k] = - sum_m gr
//   (e . get) needs no sweep of its own:  (e . get) = sum_f dso so + ([p > eps] ? dtau tau : (h . gh)) + e[k-1,D-1] gg[k,0] - e[k,D-1] gg[k+1,0].
//   tv_dout (a wave per (row, anchor): dso, dto, the sums over f, gg at the first column of every d-range) -> tv_s2 -> tv_dx (a
//   workgroup owns 128 rows, a d-range and the anchors g, g + G, ...: per 32-column chunk, from the top of the range down, ge and gh on
//   the matrix cores over F in 32-filter steps, then the chain with a thread per (row, column); dx accumulates in the workgroup's own
//   block).  Where a squared norm does not exceed eps the norm's gradient is defined as zero (the reference: 0 / 0).
#include "triangulation_common.h"

// no product may be fused into the differences e[d] - e[d-1] and out[t] - mean
#pragma clang fp contract(off)

namespace lpm {

constexpr int TV_ROWS = 128;          // frame rows per workgroup of tv_conv and tv_dx (one 32-row tile per wave)
constexpr int TV_KC = 16;             // anchors per wave of tv_norms
constexpr int TV_MAX_GROUPS = 8;      // dx partials per row tile
constexpr int TV_MAX_RANGES = 8;      // d-ranges of tv_dx

// 1 / sqrt(max(sq, eps)) from the correctly rounded root and quotient; taken once per (row, anchor) by tv_norms and stored beside the
// squared norm, so every later kernel scales by the same bits
__device__ __forceinline__ float tv_inv(float sq) { return 1.f / sqrtf(fmaxf(sq, kL2Eps)); }

static int tv_range(int D) { return D >= 1024 ? 256 : D; }               // columns per d-range of tv_dx
static int tv_row_tiles(int64_t BT) { return (int)((BT + TV_ROWS - 1) / TV_ROWS); }
static int tv_groups(int64_t BT, int D, int K) {
    const int64_t wg = (int64_t)tv_row_tiles(BT) * (D / tv_range(D));
    int64_t want = 256 / wg;
    want = want < 1 ? 1 : (want > TV_MAX_GROUPS ? TV_MAX_GROUPS : want);
    return (int)(K < want ? K : want);
}

// q[m,k] = |x_m - a_k|^2, p[m,k] = |g|^2 (-1 for frame 0 of a clip) and their clamped reciprocal roots: direct sums of squares, one wave per row
template <int D>
__global__ __launch_bounds__(64 * TA_WAVES) void tv_norms_kernel(const float* __restrict__ x, const float* __restrict__ anchors, int64_t BT, int T,
                                                                 int K, float* __restrict__ q, float* __restrict__ p) {
    constexpr int N = TpVec<D>::N, V = TpVec<D>::V;
    float* __restrict__ iqo = q + BT * K;                  // the second halves: 1 / max(norm, 1e-6); 0 where there is no temporal row
    float* __restrict__ ito = p + BT * K;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nkc = (K + TV_KC - 1) / TV_KC;
    const int64_t wid = (int64_t)blockIdx.x * TA_WAVES + wave;
    if (wid >= BT * nkc) return;                           // (wave-uniform; no barrier in this kernel)
    const int64_t row = wid / nkc;
    const int k0 = (int)(wid % nkc) * TV_KC, k1 = min(k0 + TV_KC, K);
    const float* xr = x + row * D;
    const bool first_frame = row % T == 0;
    float xv[N], xs[N], a[N];
    tp_load<D>(xr, lane, xv);
#pragma unroll
    for (int j = 0; j < N; ++j) {                          // the frame shifted by one column: element d - 1 (d = 0: D - 1)
        const int d = (j / V * 64 + lane) * V + j % V;
        xs[j] = xr[d ? d - 1 : D - 1];
    }
    int km1 = (k0 + K - 1) % K;
    tp_load_anchor<D>(anchors, K, km1, lane, a);
    float sq = 0.f;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const float r = xv[j] - a[j];
        sq = fmaf(r, r, sq);
    }
    float iq_prev = tv_inv(wave_sum_dpp(sq));
    for (int k = k0; k < k1; ++k) {
        tp_load_anchor<D>(anchors, K, k, lane, a);
        sq = 0.f;
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const float r = xv[j] - a[j];
            sq = fmaf(r, r, sq);
        }
        sq = wave_sum_dpp(sq);
        const float iq = tv_inv(sq);
        float pp = -1.f;
        if (!first_frame) {                                // (wave-uniform)
            pp = 0.f;
#pragma unroll
            for (int j = 0; j < N; ++j) {
                const int d = (j / V * 64 + lane) * V + j % V;
                const float ap = d ? anchors[(int64_t)(d - 1) * K + k] : anchors[(int64_t)(D - 1) * K + km1];
                const float g = ta_eh(xv[j], a[j], iq) - ta_eh(xs[j], ap, d ? iq : iq_prev);
                pp = fmaf(g, g, pp);
            }
            pp = wave_sum_dpp(pp);
        }
        if (lane == 0) {
            q[row * K + k] = sq;
            p[row * K + k] = pp;
            iqo[row * K + k] = iq;
            ito[row * K + k] = first_frame ? 0.f : tv_inv(pp);
        }
        iq_prev = iq;
        km1 = k;
    }
}

// tv_conv's FRAMES output policy (triangulation_magnitude_frames): the squared norms q, p [B T, K] of tv_norms, the frames per clip and
// the row stride of the two feature matrices; all unread under the other policies
struct TvFrames {
    const float *sq_s, *sq_t;
    int T, ld;
};

// so[m,k,f], to[m,k,f] for 128 rows, one anchor and 32 filters (to = 0 on frame 0 of a clip); RELU: both rectified (triangulation_magnitude)
// FRAMES (with RELU; triangulation_magnitude_frames): so, to are the per-frame feature matrices [B T, ld] and [B (T-1), ld], the same
// values at column k F + f of rows fr.ld floats apart, the temporal rows COMPACTED (row b (T-1) + t-1; frame 0 is not written).  The
// workgroups of filter tile 0 also write their anchor's norm column K F + k = sqrt(squared norm), those of anchor 0 the zero columns
// K F + K .. ld-1 as well.
template <int D, bool RELU = false, bool FRAMES = false>
__global__ __launch_bounds__(64 * TA_WAVES) void tv_conv_kernel(const float* __restrict__ x, const float* __restrict__ anchors,
                                                                const float* __restrict__ ws, const float* __restrict__ wt,
                                                                const float* __restrict__ iq, const float* __restrict__ it, int64_t BT, int K, int F,
                                                                int NR, float* __restrict__ so, float* __restrict__ to, const TvFrames fr) {
    static_assert(RELU || !FRAMES, "the per-frame features are rectified");
    __shared__ float tE[TV_ROWS][TA_LD], tH[TV_ROWS][TA_LD], tWs[32][TA_LD], tWt[32][TA_LD];
    __shared__ float iqs[TV_ROWS], iqp[TV_ROWS], its[TV_ROWS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int NF = (F + 31) / 32;
    int id = blockIdx.x;
    const int rt = id % NR; id /= NR;                      // (the row tiles of one weight tile are neighbours)
    const int ft = id % NF, k = id / NF;
    const int km1 = (k + K - 1) % K, f0 = ft * 32;
    const int64_t R0 = (int64_t)rt * TV_ROWS;
    if (threadIdx.x < TV_ROWS) {
        const int64_t R = R0 + threadIdx.x;
        const bool valid = R < BT;
        iqs[threadIdx.x] = valid ? iq[R * K + k] : 0.f;
        iqp[threadIdx.x] = valid ? iq[R * K + km1] : 0.f;
        its[threadIdx.x] = valid ? it[R * K + k] : 0.f;
        if (FRAMES && valid && ft == 0) {                  // (ft is uniform over the workgroup)
            const int KF = K * F, W = KF + K;
            const int64_t b = R / fr.T;
            float* rs = so + R * fr.ld;
            float* rt = R - b * fr.T >= 1 ? to + (R - b - 1) * fr.ld : nullptr;
            rs[KF + k] = sqrtf(fr.sq_s[R * K + k]);
            if (rt) rt[KF + k] = sqrtf(fr.sq_t[R * K + k]);
            if (k == 0)
                for (int j = W; j < fr.ld; ++j) {
                    rs[j] = 0.f;
                    if (rt) rt[j] = 0.f;
                }
        }
    }
    __syncthreads();
    const int c = threadIdx.x & 31, r0 = threadIdx.x >> 5;
    f32x16 acc_s, acc_t;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc_s[r] = acc_t[r] = 0.f;
    for (int c0 = 0; c0 < D; c0 += TA_CH) {
        const int d = c0 + c, dp = d ? d - 1 : D - 1;
        const float av = anchors[(int64_t)d * K + k], ap = anchors[(int64_t)dp * K + (d ? k : km1)];
#pragma unroll 4
        for (int i = 0; i < TV_ROWS / 8; ++i) {
            const int row = r0 + 8 * i;
            const int64_t R = R0 + row;
            float xv = 0.f, xp = 0.f;
            if (R < BT) {
                xv = x[R * D + d];
                xp = x[R * D + dp];
            }
            const float e = ta_eh(xv, av, iqs[row]);        // (0 outside the rows: the factor is 0 there)
            const float ep = ta_eh(xp, ap, d ? iqs[row] : iqp[row]);
            tE[row][c] = e;
            tH[row][c] = (e - ep) * its[row];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int f = r0 + 8 * i, ff = f0 + f;
            tWs[f][c] = ff < F ? ws[((int64_t)k * F + ff) * D + d] : 0.f;
            tWt[f][c] = ff < F ? wt[((int64_t)k * F + ff) * D + d] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < TA_CH; kk += 2) {
            const int col = kk + (lane >> 5), rr = 32 * wave + (lane & 31);
            acc_s = mfma32(tE[rr][col], tWs[lane & 31][col], acc_s);
            acc_t = mfma32(tH[rr][col], tWt[lane & 31][col], acc_t);
        }
        __syncthreads();
    }
    const int f = f0 + (lane & 31);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int64_t R = R0 + 32 * wave + mfma32_row(r, lane);
        if (R < BT && f < F) {
            if (FRAMES) {
                const int64_t b = R / fr.T;
                so[R * fr.ld + k * F + f] = fmaxf(acc_s[r], 0.f);
                if (R - b * fr.T >= 1) to[(R - b - 1) * fr.ld + k * F + f] = fmaxf(acc_t[r], 0.f);
            } else {
                so[(R * K + k) * F + f] = RELU ? fmaxf(acc_s[r], 0.f) : acc_s[r];
                to[(R * K + k) * F + f] = RELU ? fmaxf(acc_t[r], 0.f) : acc_t[r];
            }
        }
    }
}

// one column of tm_pool, its values `stride` floats apart from frame z on (norm: squared norms, their roots taken as they are read): the
// plain mean, then the deviations from it -- sum_t w_t val, the mean, the mean of the squared deviations and the mean of the deviations
// themselves (what the rounded mean is off by); every sum over t two-level.  ROOTS: some lane of the wave walks a norm column.  The
// walks are bound by their chain of loads and what hangs on it, so a wave of convolution columns alone takes the instantiation without
// the root, and a mixed wave walks once with a select per lane, not once per kind.
template <bool ROOTS>
__device__ __forceinline__ void tm_pool_column(const float* __restrict__ v, int64_t stride, bool norm, const float* __restrict__ w, int z, int T,
                                               float cnt, float& wsum, float& mean, float& var, float& corr) {
    float tot = 0.f, acc = 0.f, wtot = 0.f, wacc = 0.f;
    for (int t = z; t < T; ++t) {
        const float val = (ROOTS && norm) ? sqrtf(v[t * stride]) : v[t * stride];
        acc += val;
        if (w) wacc = fmaf(w[t - z], val, wacc);
        if (((t - z) & (TP_SUM_CHUNK - 1)) == TP_SUM_CHUNK - 1) {
            tot += acc;
            wtot += wacc;
            acc = wacc = 0.f;
        }
    }
    mean = (tot + acc) / cnt;
    wsum = wtot + wacc;
    float dtot = 0.f, dacc = 0.f;
    tot = acc = 0.f;
    for (int t = z; t < T; ++t) {
        const float dev = ((ROOTS && norm) ? sqrtf(v[t * stride]) : v[t * stride]) - mean;
        acc = fmaf(dev, dev, acc);
        dacc += dev;
        if (((t - z) & (TP_SUM_CHUNK - 1)) == TP_SUM_CHUNK - 1) {
            tot += acc;
            dtot += dacc;
            acc = dacc = 0.f;
        }
    }
    var = (tot + acc) / cnt;
    corr = (dtot + dacc) / cnt;
}

// The moments of all three pooled ops.  A thread per (clip, column of [conv | norm]), blockIdx.y = stream: pool [B, 2 W] = [(1/T') sum_t w_t out_t
// (the plain mean where the weights are null) | the mean of the squared deviations from the plain mean]; mean_out (nullable: without
// weights it is the pool's own first half) and corr_out, element z zstride + b W + j = the stream's plain mean and the rounding error
// of that mean, which the backward takes out again.  W = K F + NC with NC = K norm columns sqrt(q), sqrt(p), or NC = 0 without them (q, p
// are then unread and may be null).
__global__ __launch_bounds__(256) void tm_pool_kernel(const float* __restrict__ so, const float* __restrict__ to, const float* __restrict__ q,
                                                      const float* __restrict__ p, const float* __restrict__ w_s, const float* __restrict__ w_t,
                                                      int B, int T, int K, int F, int NC, float* __restrict__ pool_s, float* __restrict__ pool_t,
                                                      float* __restrict__ mean_out, float* __restrict__ corr_out, int64_t zstride) {
    const int64_t KF = (int64_t)K * F, W = KF + NC;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= B * W) return;
    const int64_t b = i / W, j = i % W;
    const int z = blockIdx.y, Tz = T - z;
    const bool norm = j >= KF;
    const float* v = norm ? (z ? p : q) + b * T * K + (j - KF) : (z ? to : so) + b * T * KF + j;
    const int64_t stride = norm ? K : KF;
    const float* w = z ? w_t : w_s;                          // null: the plain mean
    if (w) w += b * Tz;
    const float cnt = (float)Tz;
    float wsum, mean, var, corr;
    if (__ballot(norm) != 0)                               // (uniform over the wave)
        tm_pool_column<true>(v, stride, norm, w, z, T, cnt, wsum, mean, var, corr);
    else
        tm_pool_column<false>(v, stride, false, w, z, T, cnt, wsum, mean, var, corr);
    float* pool = (z ? pool_t : pool_s) + b * 2 * W;
    pool[j] = w ? wsum / cnt : mean;
    pool[W + j] = var;
    const int64_t o = z * zstride + b * W + j;
    if (mean_out) mean_out[o] = mean;
    corr_out[o] = corr;
}

// one wave per (row, anchor): dso, dto [B T, K F]; sa = sum_f dso so + ([p > eps] ? dtau tau : (h . gh)); s1g = (h . gh) [p > eps];
// dtg = dtau [p > eps]; dn (ungated: tv_s2 gates it); ggb[m,k,r] = gg at column r DR
template <int D>
__global__ __launch_bounds__(64 * TA_WAVES) void tv_dout_kernel(const float* __restrict__ x, const float* __restrict__ anchors,
                                                                const float* __restrict__ wt, const float* __restrict__ q, const float* __restrict__ p,
                                                                const float* __restrict__ so, const float* __restrict__ to,
                                                                const float* __restrict__ pool_s, const float* __restrict__ pool_t,
                                                                const float* __restrict__ corr, const float* __restrict__ g_s,
                                                                const float* __restrict__ g_t, int64_t BT, int T, int K,
                                                                int F, int DR, float* __restrict__ dso, float* __restrict__ dto,
                                                                float* __restrict__ sa, float* __restrict__ s1g, float* __restrict__ dtg,
                                                                float* __restrict__ dn, float* __restrict__ ggb) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t wid = (int64_t)blockIdx.x * TA_WAVES + wave;
    if (wid >= BT * K) return;                             // (wave-uniform; no barrier in this kernel)
    const int64_t R = wid / K;
    const int k = (int)(wid % K), km1 = (k + K - 1) % K, NDR = D / DR;
    const int64_t b = R / T, KF = (int64_t)K * F, W = KF + K;
    const bool has_t = R % T != 0;
    const float cnt_s = (float)T, cnt_t = (float)(T - 1);
    const float *iqa = q + BT * K, *ita = p + BT * K;
    const float *cs = corr + b * W, *ct = corr + (BT / T + b) * W;
    const float *ps = pool_s + b * 2 * W, *pt = pool_t + b * 2 * W, *gs = g_s + b * 2 * W, *gt = g_t + b * 2 * W;
    float sso = 0.f, s1 = 0.f, gh[TV_MAX_RANGES];
#pragma unroll
    for (int r = 0; r < TV_MAX_RANGES; ++r) gh[r] = 0.f;
    for (int f = lane; f < F; f += 64) {
        const int64_t j = (int64_t)k * F + f, o = R * KF + j;
        const float vs = so[o];
        const float ds = (gs[j] + 2.f * gs[W + j] * ((vs - ps[j]) - cs[j])) / cnt_s;
        dso[o] = ds;
        sso = fmaf(ds, vs, sso);
        float dt = 0.f;
        if (has_t) {
            const float vt = to[o];
            dt = (gt[j] + 2.f * gt[W + j] * ((vt - pt[j]) - ct[j])) / cnt_t;
            s1 = fmaf(dt, vt, s1);
#pragma unroll
            for (int r = 0; r < TV_MAX_RANGES; ++r)
                if (r < NDR) gh[r] = fmaf(dt, wt[j * D + r * DR], gh[r]);
        }
        dto[o] = dt;
    }
    sso = wave_sum_dpp(sso);
    s1 = wave_sum_dpp(s1);
#pragma unroll
    for (int r = 0; r < TV_MAX_RANGES; ++r) gh[r] = wave_sum_dpp(gh[r]);
    const int64_t m = R * K + k, jn = KF + k;
    const float qq = q[m], pp = p[m];
    const float iq = iqa[m], iqm = iqa[R * K + km1], itau = ita[m];
    const float gp = pp > kL2Eps ? 1.f : 0.f;
    const float tau = has_t ? sqrtf(pp) : 0.f;
    const float dtau = has_t ? (gt[jn] + 2.f * gt[W + jn] * ((tau - pt[jn]) - ct[jn])) / cnt_t : 0.f;
    const float* xr = x + R * D;
#pragma unroll
    for (int r = 0; r < TV_MAX_RANGES; ++r) {
        if (r < NDR && lane == r) {
            const int d = r * DR, dp = d ? d - 1 : D - 1;
            const float e = ta_eh(xr[d], anchors[(int64_t)d * K + k], iq);
            const float ep = ta_eh(xr[dp], anchors[(int64_t)dp * K + (d ? k : km1)], d ? iq : iqm);
            const float h = (e - ep) * itau;
            ggb[m * NDR + r] = itau * (gh[r] - h * (s1 * gp)) + (dtau * gp) * h;
        }
    }
    if (lane == 0) {
        const float n = sqrtf(qq);
        dn[m] = (gs[jn] + 2.f * gs[W + jn] * ((n - ps[jn]) - cs[jn])) / cnt_s;
        sa[m] = sso + (gp != 0.f ? dtau * tau : s1);
        s1g[m] = s1 * gp;
        dtg[m] = dtau * gp;
    }
}

// a thread per (row, anchor): s2g = (e . get) [q > eps], dn *= [q > eps]
__global__ __launch_bounds__(256) void tv_s2_kernel(const float* __restrict__ x, const float* __restrict__ anchors, const float* __restrict__ q,
                                                    const float* __restrict__ sa, const float* __restrict__ ggb, int64_t BT, int D, int K, int NDR,
                                                    float* __restrict__ s2g, float* __restrict__ dn) {
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= BT * K) return;
    const int64_t R = m / K;
    const int k = (int)(m % K), km1 = (k + K - 1) % K, kp1 = (k + 1) % K;
    const float qq = q[m], xl = x[R * D + D - 1];
    const float* iqa = q + BT * K;
    const float e_last = ta_eh(xl, anchors[(int64_t)(D - 1) * K + k], iqa[m]);
    const float e_prev = ta_eh(xl, anchors[(int64_t)(D - 1) * K + km1], iqa[R * K + km1]);
    const float gq = qq > kL2Eps ? 1.f : 0.f;
    const float s2 = sa[m] + e_prev * ggb[m * NDR] - e_last * ggb[(R * K + kp1) * NDR];
    s2g[m] = s2 * gq;
    dn[m] *= gq;
}

// dW[k,f,d] = sum_m dout[m,k,f] operand[m,k,d]: a wave owns 32 filters x 32 columns of one anchor and walks all rows
template <int D>
__global__ __launch_bounds__(64 * TA_WAVES) void tv_dw_kernel(const float* __restrict__ x, const float* __restrict__ anchors,
                                                              const float* __restrict__ iqa, const float* __restrict__ ita, const float* __restrict__ dso,
                                                              const float* __restrict__ dto, int64_t BT, int K, int F, float* __restrict__ dws,
                                                              float* __restrict__ dwt) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr int NQ = D / (32 * TA_WAVES);
    const int NF = (F + 31) / 32;
    int id = blockIdx.x;
    const int dq = id % NQ; id /= NQ;
    const int ft = id % NF, k = id / NF;
    const int km1 = (k + K - 1) % K, f0 = ft * 32, d0 = (dq * TA_WAVES + wave) * 32;
    const int c = lane & 31, hp = lane >> 5;
    const int d = d0 + c, dp = d ? d - 1 : D - 1, f = f0 + c;
    const float av = anchors[(int64_t)d * K + k], ap = anchors[(int64_t)dp * K + (d ? k : km1)];
    f32x16 tot_s, tot_t;
#pragma unroll
    for (int r = 0; r < 16; ++r) tot_s[r] = tot_t[r] = 0.f;
    for (int64_t rb = 0; rb < BT; rb += TP_SUM_CHUNK) {    // two-level over the rows
        f32x16 acc_s, acc_t;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc_s[r] = acc_t[r] = 0.f;
#pragma unroll 4
        for (int i = 0; i < TP_SUM_CHUNK / 2; ++i) {
            const int64_t R = rb + 2 * i + hp;
            float a_s = 0.f, a_t = 0.f, e = 0.f, h = 0.f;
            if (R < BT) {
                const float iq = iqa[R * K + k], itau = ita[R * K + k];
                const float iqp = d ? iq : iqa[R * K + km1];
                e = ta_eh(x[R * D + d], av, iq);
                h = (e - ta_eh(x[R * D + dp], ap, iqp)) * itau;
                if (f < F) {
                    a_s = dso[(R * K + k) * F + f];
                    a_t = dto[(R * K + k) * F + f];
                }
            }
            acc_s = mfma32(a_s, e, acc_s);
            acc_t = mfma32(a_t, h, acc_t);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            tot_s[r] += acc_s[r];
            tot_t[r] += acc_t[r];
        }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int ff = f0 + mfma32_row(r, lane);
        if (ff < F) {
            dws[((int64_t)k * F + ff) * D + d] = tot_s[r];
            dwt[((int64_t)k * F + ff) * D + d] = tot_t[r];
        }
    }
}

// dx partials and danchors partials: 128 rows, the d-range dr and the anchors g, g + G, ... per workgroup
template <int D>
__global__ __launch_bounds__(64 * TA_WAVES) void tv_dx_kernel(const float* __restrict__ x, const float* __restrict__ anchors,
                                                              const float* __restrict__ ws, const float* __restrict__ wt, const float* __restrict__ iqa,
                                                              const float* __restrict__ ita, const float* __restrict__ dso,
                                                              const float* __restrict__ dto, const float* __restrict__ s1g_,
                                                              const float* __restrict__ dtg_, const float* __restrict__ s2g_,
                                                              const float* __restrict__ dng_, const float* __restrict__ ggb, int64_t BT, int K, int F,
                                                              int DR, int G, float* __restrict__ dx_part, float* __restrict__ da_part) {
    __shared__ float tA[TV_ROWS][TA_LD], tB[TV_ROWS][TA_LD], tG[TV_ROWS][TA_LD];
    __shared__ float halo[2][TV_ROWS], iqs[TV_ROWS], iqp[TV_ROWS], its[TV_ROWS], s1g[TV_ROWS], dtg[TV_ROWS], s2g[TV_ROWS], dng[TV_ROWS];
    __shared__ float dacc[8 * 32];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int NDR = D / DR;
    int id = blockIdx.x;
    const int dr = id % NDR; id /= NDR;
    const int g = id % G, rt = id / G;
    const int64_t R0 = (int64_t)rt * TV_ROWS;
    const int c = threadIdx.x & 31, r0 = threadIdx.x >> 5, hp = lane >> 5;
    // this workgroup's own [128, D] block (dx itself when G == 1: rows past the end are never touched)
    float* dxo = G > 1 ? dx_part + ((int64_t)rt * G + g) * TV_ROWS * D : dx_part + R0 * D;
    for (int k = g; k < K; k += G) {
        const bool first = k == g;
        const int km1 = (k + K - 1) % K;
        __syncthreads();
        if (threadIdx.x < TV_ROWS) {
            const int row = threadIdx.x;
            const int64_t R = R0 + row, m = R * K + k;
            const bool valid = R < BT;
            iqs[row] = valid ? iqa[m] : 0.f;
            iqp[row] = valid ? iqa[R * K + km1] : 0.f;
            its[row] = valid ? ita[m] : 0.f;
            s1g[row] = valid ? s1g_[m] : 0.f;
            dtg[row] = valid ? dtg_[m] : 0.f;
            s2g[row] = valid ? s2g_[m] : 0.f;
            dng[row] = valid ? dng_[m] : 0.f;
            // gg of the column behind the range: the next range's first column, or column 0 of the next anchor
            const bool wrap = (dr + 1) * DR == D;
            halo[0][row] = valid ? (wrap ? ggb[(R * K + (k + 1) % K) * NDR] : ggb[m * NDR + dr + 1]) : 0.f;
        }
        __syncthreads();
        int hb = 0;
        for (int c0 = (dr + 1) * DR - TA_CH; c0 >= dr * DR; c0 -= TA_CH) {      // from the top of the range down
            const int d = c0 + c, dp = d ? d - 1 : D - 1;
            const float av = anchors[(int64_t)d * K + k], ap = anchors[(int64_t)dp * K + (d ? k : km1)];
            f32x16 acc_e, acc_h;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc_e[r] = acc_h[r] = 0.f;
            for (int f0 = 0; f0 < F; f0 += 32) {
                const int ff = f0 + c;
#pragma unroll 4
                for (int i = 0; i < TV_ROWS / 8; ++i) {
                    const int row = r0 + 8 * i;
                    const int64_t R = R0 + row;
                    const bool in = R < BT && ff < F;
                    tA[row][c] = in ? dso[(R * K + k) * F + ff] : 0.f;
                    tB[row][c] = in ? dto[(R * K + k) * F + ff] : 0.f;
                }
                __syncthreads();
#pragma unroll
                for (int kk = 0; kk < 32; kk += 2) {
                    const int fc = kk + hp, fw = f0 + fc, rr = 32 * wave + (lane & 31);
                    const float bs = fw < F ? ws[((int64_t)k * F + fw) * D + d] : 0.f;
                    const float bt = fw < F ? wt[((int64_t)k * F + fw) * D + d] : 0.f;
                    acc_e = mfma32(tA[rr][fc], bs, acc_e);
                    acc_h = mfma32(tB[rr][fc], bt, acc_h);
                }
                __syncthreads();
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = 32 * wave + mfma32_row(r, lane);
                tA[row][lane & 31] = acc_e[r];              // ge
                tB[row][lane & 31] = acc_h[r];              // gh
            }
            __syncthreads();
            float ev[TV_ROWS / 8];
#pragma unroll 4
            for (int i = 0; i < TV_ROWS / 8; ++i) {
                const int row = r0 + 8 * i;
                const int64_t R = R0 + row;
                float xv = 0.f, xp = 0.f;
                if (R < BT) {
                    xv = x[R * D + d];
                    xp = x[R * D + dp];
                }
                const float e = ta_eh(xv, av, iqs[row]);
                const float h = (e - ta_eh(xp, ap, d ? iqs[row] : iqp[row])) * its[row];
                const float gg = its[row] * (tB[row][c] - h * s1g[row]) + dtg[row] * h;
                tG[row][c] = gg;
                if (c == 0) halo[hb ^ 1][row] = gg;
                ev[i] = e;
            }
            __syncthreads();
            float da = 0.f;
#pragma unroll 4
            for (int i = 0; i < TV_ROWS / 8; ++i) {
                const int row = r0 + 8 * i;
                const int64_t R = R0 + row;
                const float nxt = c < 31 ? tG[row][c + 1] : halo[hb][row];
                const float get = tA[row][c] + tG[row][c] - nxt;
                const float gr = iqs[row] * (get - ev[i] * s2g[row]) + dng[row] * ev[i];
                if (R < BT) {
                    float* o = dxo + (int64_t)row * D + d;
                    *o = first ? gr : *o + gr;             // (an earlier anchor of this workgroup: this thread wrote it)
                    da += gr;
                }
            }
            dacc[r0 * 32 + c] = da;
            __syncthreads();
            if (threadIdx.x < 32) {
                float acc_a = dacc[c];
                for (int r = 1; r < 8; ++r) acc_a += dacc[r * 32 + c];
                da_part[((int64_t)rt * K + k) * D + d] = acc_a;
            }
            hb ^= 1;
            __syncthreads();
        }
    }
}

// dx[m] = sum_g dx_part[tile(m)][g][m - tile start], g = 0, 1, ...  (The sum of the attention poolings' dx pass over row tiles instead of
// clips, but a float at a time: this op's workspace puts dx_part behind a count of floats that need not be a multiple of four.)
__global__ __launch_bounds__(256) void tv_dx_reduce_kernel(const float* __restrict__ part, int64_t total, int D, int G, float* __restrict__ dx) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int64_t R = i / D, rt = R / TV_ROWS, blk = (int64_t)TV_ROWS * D;
    const float* pp = part + rt * G * blk + (i - rt * blk);
    float acc = pp[0];
    for (int g = 1; g < G; ++g) acc += pp[g * blk];
    dx[i] = acc;
}

static int tv_check(const char* name, int B, int T, int D, int K, int F) {
    if (const int rc = ta_check(name, B, T, D, K)) return rc;
    LPM_REQUIRE(F >= 1, LPM_ERR_BADARG, "%s: need F >= 1 (F=%d)", name, F);
    const int64_t BT = (int64_t)B * T, NF = (F + 31) / 32;
    LPM_REQUIRE(BT * K * F < (1ll << 31) && (int64_t)K * NF * (D / 128) < (1ll << 31), LPM_ERR_UNSUPPORTED_SHAPE,
                "%s: B * T * K * F or K * F * D too large (B=%d T=%d K=%d F=%d)", name, B, T, K, F);
    return LPM_OK;
}

// tv_conv's launch: a workgroup per (anchor, 32 filters, 128 rows); iq, it [B T, K] scale the spatial and the temporal operand
template <bool RELU, bool FRAMES>
static void tv_conv_launch(const float* x, const float* anchors, const float* cnn_s, const float* cnn_t, const float* iq, const float* it, int B,
                           int T, int D, int K, int F, float* so, float* to, const TvFrames fr, hipStream_t s) {
    const int64_t BT = (int64_t)B * T;
    const int NR = tv_row_tiles(BT), NF = (F + 31) / 32;
    tp_dispatch_d(D, [&](auto d) {
        hipLaunchKernelGGL((tv_conv_kernel<decltype(d)::value, RELU, FRAMES>), dim3((unsigned)((int64_t)K * NF * NR)), dim3(64 * TA_WAVES), 0, s, x,
                           anchors, cnn_s, cnn_t, iq, it, BT, K, F, NR, so, to, fr);
    });
}

}  // namespace lpm

extern "C" size_t lpm_triangulation_moments_workspace_bytes(int B, int T, int D, int K, int F) {
    using namespace lpm;
    if (B <= 0 || T <= 1 || K <= 0 || F <= 0 || (D != 128 && D != 1024)) return 0;
    const size_t BT = (size_t)B * T, NRT = tv_row_tiles(BT), NDR = D / tv_range(D), G = tv_groups(BT, D, K);
    // dso, dto; sa, s1g, dtg, dn, s2g; ggb; danchors partials; dx partials
    return (2 * BT * K * F + (5 + NDR) * BT * K + NRT * K * D + (G > 1 ? NRT * G * TV_ROWS * D : 0)) * sizeof(float);
}

extern "C" int lpm_triangulation_moments_fwd(const float* x, const float* anchors, const float* cnn_s, const float* cnn_t, int B, int T, int D,
                                             int K, int F, float* q, float* p, float* so, float* to, float* pool_s, float* pool_t,
                                             float* corr, lpm_stream_t stream) {
    using namespace lpm;
    const char* name = "lpm_triangulation_moments_fwd";
    LPM_REQUIRE(x && anchors && cnn_s && cnn_t && q && p && so && to && pool_s && pool_t && corr, LPM_ERR_BADARG, "%s: null pointer", name);
    if (const int rc = tv_check(name, B, T, D, K, F)) return rc;
    LPM_REQUIRE(((uintptr_t)x & 15) == 0, LPM_ERR_BADARG, "%s: x must be 16-byte aligned", name);
    hipStream_t s = (hipStream_t)stream;
    const int64_t BT = (int64_t)B * T;
    const dim3 grid_n((unsigned)((BT * ((K + TV_KC - 1) / TV_KC) + TA_WAVES - 1) / TA_WAVES));
    tp_dispatch_d(D, [&](auto d) {
        hipLaunchKernelGGL(tv_norms_kernel<decltype(d)::value>, grid_n, dim3(64 * TA_WAVES), 0, s, x, anchors, BT, T, K, q, p);
    });
    tv_conv_launch<false, false>(x, anchors, cnn_s, cnn_t, q + BT * K, p + BT * K, B, T, D, K, F, so, to, TvFrames{}, s);
    // no weights: the plain mean is the pool's first half, and only corr [2, B, W] is kept beside it
    const int64_t W = (int64_t)K * F + K, cols = B * W;
    hipLaunchKernelGGL(tm_pool_kernel, dim3((unsigned)((cols + 255) / 256), 2), dim3(256), 0, s, so, to, q, p, (const float*)nullptr,
                       (const float*)nullptr, B, T, K, F, K, pool_s, pool_t, (float*)nullptr, corr, B * W);
    return check_launch(name);
}

extern "C" int lpm_triangulation_moments_bwd(const float* x, const float* anchors, const float* cnn_s, const float* cnn_t, const float* q,
                                             const float* p, const float* so, const float* to, const float* pool_s, const float* pool_t,
                                             const float* corr, const float* g_s, const float* g_t, int B, int T, int D, int K, int F, float* dx, float* danchors,
                                             float* dcnn_s, float* dcnn_t, void* workspace, size_t workspace_bytes, lpm_stream_t stream) {
    using namespace lpm;
    const char* name = "lpm_triangulation_moments_bwd";
    LPM_REQUIRE(x && anchors && cnn_s && cnn_t && q && p && so && to && pool_s && pool_t && corr && g_s && g_t && dx && danchors && dcnn_s && dcnn_t,
                LPM_ERR_BADARG, "%s: null pointer", name);
    if (const int rc = tv_check(name, B, T, D, K, F)) return rc;
    LPM_REQUIRE(workspace && workspace_bytes >= lpm_triangulation_moments_workspace_bytes(B, T, D, K, F), LPM_ERR_WORKSPACE,
                "%s: workspace too small", name);
    hipStream_t s = (hipStream_t)stream;
    const int64_t BT = (int64_t)B * T, BTK = BT * K;
    const int DR = tv_range(D), NDR = D / DR, NRT = tv_row_tiles(BT), G = tv_groups(BT, D, K), NF = (F + 31) / 32;
    float* dso = (float*)workspace;
    float* dto = dso + BTK * F;
    float* sa = dto + BTK * F;
    float *s1g = sa + BTK, *dtg = s1g + BTK, *dn = dtg + BTK, *s2g = dn + BTK, *ggb = s2g + BTK;
    float* da_part = ggb + BTK * NDR;
    float* dx_part = G > 1 ? da_part + (int64_t)NRT * K * D : dx;
    const dim3 block(64 * TA_WAVES);
    const dim3 grid_o((unsigned)((BTK + TA_WAVES - 1) / TA_WAVES)), grid_w((unsigned)((int64_t)K * NF * (D / (32 * TA_WAVES)))),
        grid_x((unsigned)((int64_t)NRT * G * NDR));
    tp_dispatch_d(D, [&](auto d) {
        constexpr int DD = decltype(d)::value;
        hipLaunchKernelGGL(tv_dout_kernel<DD>, grid_o, block, 0, s, x, anchors, cnn_t, q, p, so, to, pool_s, pool_t, corr, g_s, g_t, BT, T, K, F, DR, dso,
                           dto, sa, s1g, dtg, dn, ggb);
        hipLaunchKernelGGL(tv_s2_kernel, dim3((unsigned)((BTK + 255) / 256)), dim3(256), 0, s, x, anchors, q, sa, ggb, BT, D, K, NDR, s2g, dn);
        hipLaunchKernelGGL(tv_dw_kernel<DD>, grid_w, block, 0, s, x, anchors, q + BTK, p + BTK, dso, dto, BT, K, F, dcnn_s, dcnn_t);
        hipLaunchKernelGGL(tv_dx_kernel<DD>, grid_x, block, 0, s, x, anchors, cnn_s, cnn_t, q + BTK, p + BTK, dso, dto, s1g, dtg, s2g, dn, ggb, BT, K, F,
                           DR, G, dx_part, da_part);
    });
    if (G > 1) {
        const int64_t total = BT * D;
        hipLaunchKernelGGL(tv_dx_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, dx_part, total, D, G, dx);
    }
    // danchors[d][k] = - sum over the row tiles, in order (the dx partials are reduced above: the tiles are not clips)
    if (const int rc = ta_reduce_partials(dx, da_part, NRT, TV_ROWS, D, K, 1, TP_SUM_CHUNK, dx, danchors, s, name)) return rc;
    return check_launch(name);
}

// ---- the convolution side of triangulation_cnn_attention (TriangulationNsCnnIndirectAttentionModule :1108-1268, JuhanTestModelV2) ----
// The temporal operand is g itself, NOT normalised again: tv_conv and tv_dw run as they are with `it` = ind [B T, K], 1 on the frames
// t >= 1 and 0 on frame 0 of a clip (a product with 1 is exact), so the walks above exist once.  The pools take the softmax weights of
// the caller's Grams:  pool = [ (1/T') sum_t w_t out_t  |  mean_t (out_t - mean_t out)^2 ]  (the plain mean without weights), and the
// backward's  dout[t] = (w_t gm + 2 gv ((out[t] - mean) - c)) / T',  dw[t] = <gm, out[t]> / T':  tm_pool without norm columns and tm_dout<false>.
namespace lpm {

__global__ __launch_bounds__(256) void tc_ind_kernel(int64_t BTK, int T, int K, float* __restrict__ ind) {
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m < BTK) ind[m] = (m / K) % T ? 1.f : 0.f;
}

// a workgroup per (clip, frame), blockIdx.y = stream: dout [B T, K F] (the temporal one zero on frame 0) and dw[b,t] = <gm[b], out_t> / T'
// over all W = K F + NC columns (tm_pool's).  RELU (triangulation_magnitude): dout times [out > 0], and the gradient of the norm columns times
// [squared norm > eps] into dng / dtg [B T, K] (always written: zero without the norm columns).  Without RELU (triangulation_cnn_attention)
// there are no norm columns, NC = 0: q, p, dng and dtg are not touched and may be null.
template <bool RELU>
__global__ __launch_bounds__(256) void tm_dout_kernel(const float* __restrict__ so, const float* __restrict__ to, const float* __restrict__ q,
                                                      const float* __restrict__ p, const float* __restrict__ w_s, const float* __restrict__ w_t,
                                                      const float* __restrict__ stats, const float* __restrict__ g_s, const float* __restrict__ g_t,
                                                      int B, int T, int K, int F, int NC, float* __restrict__ dso, float* __restrict__ dto,
                                                      float* __restrict__ dng, float* __restrict__ dtg, float* __restrict__ dw_s,
                                                      float* __restrict__ dw_t) {
    __shared__ float red[4];
    const int64_t KF = (int64_t)K * F, W = KF + NC;
    const int z = blockIdx.y, b = blockIdx.x / T, t = blockIdx.x % T, Tz = T - z;
    const int64_t n = (int64_t)b * T + t;
    float* dout = (z ? dto : dso) + n * KF;
    float* dnorm = RELU ? (z ? dtg : dng) + n * K : nullptr;
    if (RELU && ((z && t == 0) || NC == 0))                // (uniform over the workgroup)
        for (int k = threadIdx.x; k < K; k += 256) dnorm[k] = 0.f;
    if (z && t == 0) {
        for (int64_t j = threadIdx.x; j < KF; j += 256) dout[j] = 0.f;
        return;
    }
    const float* out = (z ? to : so) + n * KF;
    const float* sq = RELU ? (z ? p : q) + n * K : nullptr;
    const float* g = (z ? g_t : g_s) + (int64_t)b * 2 * W;
    const float* st = stats + (int64_t)z * 2 * B * W;
    const float *mean = st + (int64_t)b * W, *corr = st + (int64_t)(B + b) * W;
    const float* w = z ? w_t : w_s;
    const float wt = w ? w[(int64_t)b * Tz + t - z] : 1.f, cnt = (float)Tz;
    float acc = 0.f;
    int64_t j = threadIdx.x;
    for (; j < KF; j += 256) {                              // the convolution columns ...
        const float v = out[j], gm = g[j];
        const float d = (wt * gm + 2.f * g[W + j] * ((v - mean[j]) - corr[j])) / cnt;
        dout[j] = (!RELU || v > 0.f) ? d : 0.f;
        acc = fmaf(gm, v, acc);
    }
    for (; RELU && j < W; j += 256) {                       // ... then the norm columns, each thread going on in its own stride
        const float s = sq[j - KF], v = sqrtf(s), gm = g[j];
        const float d = (wt * gm + 2.f * g[W + j] * ((v - mean[j]) - corr[j])) / cnt;
        dnorm[j - KF] = s > kL2Eps ? d : 0.f;
        acc = fmaf(gm, v, acc);
    }
    acc = wave_sum_dpp(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0 && w) {
        const float d = ((red[0] + red[1]) + (red[2] + red[3])) / cnt;
        if (z) dw_t[(int64_t)b * (T - 1) + t - 1] = d; else dw_s[n] = d;
    }
}

}  // namespace lpm

extern "C" int lpm_triangulation_cnn_attention_conv(const float* x, const float* anchors, const float* cnn_s, const float* cnn_t, const float* iq,
                                                    int B, int T, int D, int K, int F, float* ind, float* so, float* to, lpm_stream_t stream) {
    using namespace lpm;
    const char* name = "lpm_triangulation_cnn_attention_conv";
    LPM_REQUIRE(x && anchors && cnn_s && cnn_t && iq && ind && so && to, LPM_ERR_BADARG, "%s: null pointer", name);
    if (const int rc = tv_check(name, B, T, D, K, F)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int64_t BTK = (int64_t)B * T * K;
    hipLaunchKernelGGL(tc_ind_kernel, dim3((unsigned)((BTK + 255) / 256)), dim3(256), 0, s, BTK, T, K, ind);
    tv_conv_launch<false, false>(x, anchors, cnn_s, cnn_t, iq, ind, B, T, D, K, F, so, to, TvFrames{}, s);
    return check_launch(name);
}

extern "C" int lpm_triangulation_cnn_attention_pool(const float* so, const float* to, const float* w_s, const float* w_t, int B, int T, int K, int F,
                                                    float* pool_s, float* pool_t, float* stats, lpm_stream_t stream) {
    using namespace lpm;
    const char* name = "lpm_triangulation_cnn_attention_pool";
    LPM_REQUIRE(so && to && pool_s && pool_t && stats && !w_s == !w_t, LPM_ERR_BADARG, "%s: null pointer", name);
    if (const int rc = tv_check(name, B, T, 128, K, F)) return rc;
    const int64_t cols = (int64_t)B * K * F;                // stats [2, 2, B, K F]: each stream's mean, then its corr
    hipLaunchKernelGGL(tm_pool_kernel, dim3((unsigned)((cols + 255) / 256), 2), dim3(256), 0, (hipStream_t)stream, so, to, (const float*)nullptr,
                       (const float*)nullptr, w_s, w_t, B, T, K, F, 0, pool_s, pool_t, stats, stats + cols, 2 * cols);
    return check_launch(name);
}

extern "C" int lpm_triangulation_cnn_attention_dout(const float* so, const float* to, const float* w_s, const float* w_t, const float* stats,
                                                    const float* g_s, const float* g_t, int B, int T, int K, int F, float* dso, float* dto,
                                                    float* dw_s, float* dw_t, lpm_stream_t stream) {
    using namespace lpm;
    const char* name = "lpm_triangulation_cnn_attention_dout";
    LPM_REQUIRE(so && to && stats && g_s && g_t && dso && dto && !w_s == !w_t && !w_s == !dw_s && !w_t == !dw_t, LPM_ERR_BADARG,
                "%s: null pointer (the weights and dw of both streams, or none)", name);
    if (const int rc = tv_check(name, B, T, 128, K, F)) return rc;
    hipLaunchKernelGGL(tm_dout_kernel<false>, dim3((unsigned)(B * T), 2), dim3(256), 0, (hipStream_t)stream, so, to, (const float*)nullptr,
                       (const float*)nullptr, w_s, w_t, stats, g_s, g_t, B, T, K, F, 0, dso, dto, (float*)nullptr, (float*)nullptr, dw_s, dw_t);
    return check_launch(name);
}

extern "C" int lpm_triangulation_cnn_attention_dweights(const float* x, const float* anchors, const float* iq, const float* ind, const float* dso,
                                                        const float* dto, int B, int T, int D, int K, int F, float* dcnn_s, float* dcnn_t,
                                                        lpm_stream_t stream) {
    using namespace lpm;
    const char* name = "lpm_triangulation_cnn_attention_dweights";
    LPM_REQUIRE(x && anchors && iq && ind && dso && dto && dcnn_s && dcnn_t, LPM_ERR_BADARG, "%s: null pointer", name);
    if (const int rc = tv_check(name, B, T, D, K, F)) return rc;
    const int NF = (F + 31) / 32;
    tp_dispatch_d(D, [&](auto d) {
        hipLaunchKernelGGL(tv_dw_kernel<decltype(d)::value>, dim3((unsigned)((int64_t)K * NF * (D / (32 * TA_WAVES)))), dim3(64 * TA_WAVES), 0,
                           (hipStream_t)stream, x, anchors, iq, ind, dso, dto, (int64_t)B * T, K, F, dcnn_s, dcnn_t);
    });
    return check_launch(name);
}

// ---- the convolution side of triangulation_magnitude (TriangulationMagnitudeNsCnnIndirectAttentionModule :634-888, JuhanTestModelV3) ----
// V5's two normalisations (tv_norms, tv_conv with both reciprocal norms, tv_dw through lpm_triangulation_cnn_attention_dweights with `ind` = the
// temporal reciprocal norm) under V2's attention weights, both convolutions rectified before they are pooled.  The pools are over the
// W = K F + K columns [relu(conv) | norm]:  pool = [ (1/T') sum_t w_t out_t | mean_t (out_t - mean_t out)^2 ], the norms sqrt(q), sqrt(p)
// taken where they are read.  Backward: dout[t] = (w_t gm + 2 gv ((out[t] - mean) - c)) / T' on every column -- on a convolution column
// times [out > 0], on a norm column times [squared norm > eps] into dng / dtg [B T, K] -- and dw[t] = <gm, out[t]> / T' over all W columns:
// tm_pool and tm_dout<true>, above.
extern "C" int lpm_triangulation_magnitude_norms(const float* x, const float* anchors, int B, int T, int D, int K, float* q, float* p,
                                                 lpm_stream_t stream) {
    using namespace lpm;
    const char* name = "lpm_triangulation_magnitude_norms";
    LPM_REQUIRE(x && anchors && q && p, LPM_ERR_BADARG, "%s: null pointer", name);
    if (const int rc = tv_check(name, B, T, D, K, 1)) return rc;
    LPM_REQUIRE(((uintptr_t)x & 15) == 0, LPM_ERR_BADARG, "%s: x must be 16-byte aligned", name);
    const int64_t BT = (int64_t)B * T;
    const dim3 grid((unsigned)((BT * ((K + TV_KC - 1) / TV_KC) + TA_WAVES - 1) / TA_WAVES));
    tp_dispatch_d(D, [&](auto d) {
        hipLaunchKernelGGL(tv_norms_kernel<decltype(d)::value>, grid, dim3(64 * TA_WAVES), 0, (hipStream_t)stream, x, anchors, BT, T, K, q, p);
    });
    return check_launch(name);
}

extern "C" int lpm_triangulation_magnitude_conv(const float* x, const float* anchors, const float* cnn_s, const float* cnn_t, const float* q,
                                                const float* p, int B, int T, int D, int K, int F, float* so, float* to, lpm_stream_t stream) {
    using namespace lpm;
    const char* name = "lpm_triangulation_magnitude_conv";
    LPM_REQUIRE(x && anchors && cnn_s && cnn_t && q && p && so && to, LPM_ERR_BADARG, "%s: null pointer", name);
    if (const int rc = tv_check(name, B, T, D, K, F)) return rc;
    const int64_t BTK = (int64_t)B * T * K;
    tv_conv_launch<true, false>(x, anchors, cnn_s, cnn_t, q + BTK, p + BTK, B, T, D, K, F, so, to, TvFrames{}, (hipStream_t)stream);
    return check_launch(name);
}

extern "C" int lpm_triangulation_magnitude_pool(const float* so, const float* to, const float* q, const float* p, const float* w_s,
                                                const float* w_t, int B, int T, int K, int F, int add_norm, float* pool_s, float* pool_t,
                                                float* stats, lpm_stream_t stream) {
    using namespace lpm;
    const char* name = "lpm_triangulation_magnitude_pool";
    LPM_REQUIRE(so && to && q && p && pool_s && pool_t && stats && !w_s == !w_t, LPM_ERR_BADARG, "%s: null pointer", name);
    if (const int rc = tv_check(name, B, T, 128, K, F)) return rc;
    const int NC = add_norm ? K : 0;
    const int64_t cols = (int64_t)B * ((int64_t)K * F + NC);   // stats [2, 2, B, W]: each stream's mean, then its corr
    hipLaunchKernelGGL(tm_pool_kernel, dim3((unsigned)((cols + 255) / 256), 2), dim3(256), 0, (hipStream_t)stream, so, to, q, p, w_s, w_t, B, T, K, F,
                       NC, pool_s, pool_t, stats, stats + cols, 2 * cols);
    return check_launch(name);
}

extern "C" int lpm_triangulation_magnitude_dout(const float* so, const float* to, const float* q, const float* p, const float* w_s,
                                                const float* w_t, const float* stats, const float* g_s, const float* g_t, int B, int T, int K,
                                                int F, int add_norm, float* dso, float* dto, float* dng, float* dtg, float* dw_s, float* dw_t,
                                                lpm_stream_t stream) {
    using namespace lpm;
    const char* name = "lpm_triangulation_magnitude_dout";
    LPM_REQUIRE(so && to && q && p && stats && g_s && g_t && dso && dto && dng && dtg && !w_s == !w_t && !w_s == !dw_s && !w_t == !dw_t,
                LPM_ERR_BADARG, "%s: null pointer (the weights and dw of both streams, or none)", name);
    if (const int rc = tv_check(name, B, T, 128, K, F)) return rc;
    hipLaunchKernelGGL(tm_dout_kernel<true>, dim3((unsigned)(B * T), 2), dim3(256), 0, (hipStream_t)stream, so, to, q, p, w_s, w_t, stats, g_s, g_t, B, T,
                       K, F, add_norm ? K : 0, dso, dto, dng, dtg, dw_s, dw_t);
    return check_launch(name);
}

// ---- the per-frame features of triangulation_magnitude (TriangulationMagnitudeNsCnnNetVladModule :891-1040, JuhanTestModelV4): the rows
// [relu(conv) | norm | 0 ..] that the module hands to its two NetVLADs, one per frame (the temporal ones of the frames t >= 1, compacted).
// Forward: tv_norms as it is, then tv_conv under the FRAMES policy.  Backward: tf_dout turns the two feature gradients into the operands
// lpm_triangulation_cnn_attention_dweights and lpm_triangulation_magnitude_bwd (m_s = m_t = NULL) take. ----
namespace lpm {

// a workgroup per (clip, frame), blockIdx.y = stream: dout [B T, K F] = dfeat [feat > 0] (the temporal rows expanded back to T per clip,
// frame 0 zero) and the norm columns' gradients [B T, K] times [squared norm > eps]; VEC: 16-byte accesses of the convolution columns
template <bool VEC>
__global__ __launch_bounds__(256) void tf_dout_kernel(const float* __restrict__ feat_s, const float* __restrict__ feat_t,
                                                      const float* __restrict__ q, const float* __restrict__ p, const float* __restrict__ dfeat_s,
                                                      const float* __restrict__ dfeat_t, int T, int K, int F, int ld, float* __restrict__ dso,
                                                      float* __restrict__ dto, float* __restrict__ dng, float* __restrict__ dtg) {
    const int KF = K * F;
    const int z = blockIdx.y, b = blockIdx.x / T, t = blockIdx.x % T;
    const int64_t n = (int64_t)b * T + t;
    float* dout = (z ? dto : dso) + n * KF;
    float* dnorm = (z ? dtg : dng) + n * K;
    if (z && t == 0) {                                     // (uniform over the workgroup)
        for (int j = threadIdx.x; j < KF; j += 256) dout[j] = 0.f;
        for (int k = threadIdx.x; k < K; k += 256) dnorm[k] = 0.f;
        return;
    }
    const int64_t m = z ? n - b - 1 : n;                   // the row of the (compacted) feature matrix
    const float* feat = (z ? feat_t : feat_s) + m * ld;
    const float* g = (z ? dfeat_t : dfeat_s) + m * ld;
    const float* sq = (z ? p : q) + n * K;
    if (VEC) {
        const float4* f4 = reinterpret_cast<const float4*>(feat);
        const float4* g4 = reinterpret_cast<const float4*>(g);
        float4* d4 = reinterpret_cast<float4*>(dout);
        for (int j = threadIdx.x; j < KF / 4; j += 256) {
            const float4 v = f4[j], d = g4[j];
            d4[j] = make_float4(v.x > 0.f ? d.x : 0.f, v.y > 0.f ? d.y : 0.f, v.z > 0.f ? d.z : 0.f, v.w > 0.f ? d.w : 0.f);
        }
    } else {
        for (int j = threadIdx.x; j < KF; j += 256) dout[j] = feat[j] > 0.f ? g[j] : 0.f;
    }
    for (int k = threadIdx.x; k < K; k += 256) dnorm[k] = sq[k] > kL2Eps ? g[KF + k] : 0.f;
}

static int tf_check(const char* name, int B, int T, int D, int K, int F, int ld) {
    if (const int rc = tv_check(name, B, T, D, K, F)) return rc;
    const int64_t W = (int64_t)K * F + K;
    LPM_REQUIRE(ld >= W && (int64_t)B * T * ld < (1ll << 31), LPM_ERR_UNSUPPORTED_SHAPE,
                "%s: need K * F + K <= ld and B * T * ld < 2^31 (ld=%d, K * F + K = %lld)", name, ld, (long long)W);
    return LPM_OK;
}

}  // namespace lpm

extern "C" int lpm_triangulation_magnitude_frames_fwd(const float* x, const float* anchors, const float* cnn_s, const float* cnn_t, const float* q,
                                                      const float* p, int B, int T, int D, int K, int F, int ld, float* feat_s, float* feat_t,
                                                      lpm_stream_t stream) {
    using namespace lpm;
    const char* name = "lpm_triangulation_magnitude_frames_fwd";
    LPM_REQUIRE(x && anchors && cnn_s && cnn_t && q && p && feat_s && feat_t, LPM_ERR_BADARG, "%s: null pointer", name);
    if (const int rc = tf_check(name, B, T, D, K, F, ld)) return rc;
    const int64_t BTK = (int64_t)B * T * K;
    tv_conv_launch<true, true>(x, anchors, cnn_s, cnn_t, q + BTK, p + BTK, B, T, D, K, F, feat_s, feat_t, TvFrames{q, p, T, ld}, (hipStream_t)stream);
    return check_launch(name);
}

extern "C" int lpm_triangulation_magnitude_frames_dout(const float* feat_s, const float* feat_t, const float* q, const float* p,
                                                       const float* dfeat_s, const float* dfeat_t, int B, int T, int K, int F, int ld, float* dso,
                                                       float* dto, float* dng, float* dtg, lpm_stream_t stream) {
    using namespace lpm;
    const char* name = "lpm_triangulation_magnitude_frames_dout";
    LPM_REQUIRE(feat_s && feat_t && q && p && dfeat_s && dfeat_t && dso && dto && dng && dtg, LPM_ERR_BADARG, "%s: null pointer", name);
    if (const int rc = tf_check(name, B, T, 128, K, F, ld)) return rc;
    const uintptr_t bits = (uintptr_t)feat_s | (uintptr_t)feat_t | (uintptr_t)dfeat_s | (uintptr_t)dfeat_t | (uintptr_t)dso | (uintptr_t)dto;
    const bool vec = (bits & 15) == 0 && ld % 4 == 0 && ((int64_t)K * F) % 4 == 0;
    const dim3 grid((unsigned)(B * T), 2), block(256);
    if (vec)
        hipLaunchKernelGGL(tf_dout_kernel<true>, grid, block, 0, (hipStream_t)stream, feat_s, feat_t, q, p, dfeat_s, dfeat_t, T, K, F, ld, dso, dto,
                           dng, dtg);
    else
        hipLaunchKernelGGL(tf_dout_kernel<false>, grid, block, 0, (hipStream_t)stream, feat_s, feat_t, q, p, dfeat_s, dfeat_t, T, K, F, ld, dso,
                           dto, dng, dtg);
    return check_launch(name);
}
