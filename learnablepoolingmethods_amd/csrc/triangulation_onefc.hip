// The one-FC attention-cluster pooling of TriangulationV6Module (video_pooling_modules.py:39-138 with attention_modules.OneFcAttention,
// JuhanTestModelV6): per row n = b T + t of x [(B T), D], anchor k (anchors_t [K, D]: the [D, K] variable transposed by the caller),
// feature j = k D + d, J = K D, C clusters
//   e[n,k,:] = (x - a_k) iq,  iq = 1 / sqrt(max(|x - a_k|^2, 1e-12));   s[n,j] = e[n,j] r[n],  r = 1 / sqrt(max(sum_j e^2, 1e-12))
//   v = g s + h  (batch norm folded: g = gamma rsqrt(var + eps), h = beta - g mu; per feature)
//   l[b,t,c] = (1 / sqrt(J)) sum_j s[b,t,j] g_j W[j,c]   (h adds the same number to every frame's logit: the softmax drops it)
//   p = softmax_t(l)  (the caller's [B, T, C] work);   S[b,c,j] = sum_t p[b,t,c] s[b,t,j];   A = g S + h  (sum_t p = 1)
//   z = alpha A + shift;   y[b,c,:] = z / sqrt(max(|z|^2, 1e-12)) / sqrt(C)
// Nothing of size B T K D is written in either direction.  What IS written: the norms [B T, 3 K + 2], per-clip column sums [B, J], the
// logits' per-slice partials [B, SL, T, C], S and dA [B, C, J] (the size of the output), in the backward one [B T, K] dot product, a
// [B, C, J] partial of R and one danchors partial per clip.  No floating-point atomics: every cross-workgroup sum has a fixed order.
// Every product is a VALU fp32 fmaf (exact fp32 operands).  An element of s is rebuilt everywhere by to_s: ((x - a) iq) r, unfused.
//
// _norms:   one wave per row: iq, the gate [q > eps] and |e_k|^2 per anchor, r and the gate of the second norm per row.
// _stats:   a thread per (clip, feature) sums s over the frames, clips added b = 0, 1, ...; then the deviations from that rounded mean:
//           their squares and their plain sum (what the rounded mean is off by); the caller forms mean and variance from the three.
// _project: out[b,t,c] = scale sum_j s[b,t,j] cs_j w[.,j,c]: the logits (w = W [J, C]) and, in the backward, dp (w = dA [B, C, J]).  A
//           workgroup takes 32 frames, all C clusters and every SL-th 32-feature chunk; the slices' partials are added sl = 0, 1, ...
// _pool:    out[b,c,j] = sum_t p[b,t,c] s[b,t,j], a thread per feature, eight clusters at a time with their weights in LDS (10 KB at
//           T = 320): S, and in the backward the per-clip partials of R with dl in place of p, added b = 0, 1, ...
// _finish:  a workgroup per (clip, cluster): z, |z|^2 in a fixed order, y.
// _dz:      a workgroup per (clip, cluster): dz from dY, the partial sums of dalpha and dshift, dA = alpha dz; then the column sums
//           dh_j = sum dA and dg_j = sum dA S, 32 rows into a partial, partials in order.
// _bwd:     ds[n,j] = sum_c p[n,c] g_j dA[b,c,j] + (g_j / sqrt(J)) sum_c dl[n,c] W[j,c] + c1_j + c2_j (s - mu_j)    (c1 = dmu / N,
//           c2 = 2 dvar / N from the caller; null with given statistics), formed per (32 frames, 32 features) tile from LDS.
//   sweep 1 (a workgroup per (clip, anchor), walking D): ed[n,k] = sum_d e ds.  With ee = |e_k|^2 both dot products that must be complete
//           follow from it (to_dots): (s . ds) = r sum_k ed, and (e_k . de) = r (ed - r (s . ds) ee) -- so the chain needs two sweeps, not three.
//   sweep 2 (a workgroup per (clip, 32-column chunk), walking the anchors): de = r (ds - s (s . ds)), gr = iq (de - e (e . de)),
//           dx += gr (its own columns, in anchor order), danchors partial per clip.
//   LDS of a sweep at T = 320, C = 64: 35.8 KB (two [64][33] operand tiles, two [32][65] weight tiles, the frames' dot products).
#include "triangulation_common.h"

// an element of s must round the same way wherever it is rebuilt: no fused products
#pragma clang fp contract(off)

namespace lpm {

constexpr int TO_MAX_CLUSTERS = 64;
constexpr int TO_TT = 32;             // frames per tile
constexpr int TO_CH = 32;             // features per chunk
constexpr int TO_LDW = TO_MAX_CLUSTERS + 1;
constexpr int TO_PC = 8;              // clusters per pass of to_pool
constexpr int TO_MAX_SLICES = 16;
constexpr int TO_ROWS = 32;           // rows per partial of the column sums

struct ToNorms {
    const float *iq, *qg, *ee, *r, *g2;
};
__host__ __device__ inline ToNorms to_norms_of(const float* n, int64_t BT, int K) {
    return {n, n + BT * K, n + 2 * BT * K, n + 3 * BT * K, n + 3 * BT * K + BT};
}

template <int D>
__device__ __forceinline__ float to_e(const float* __restrict__ xr, const float* __restrict__ at, const float* __restrict__ iqr, int k, int d) {
    return ta_eh(xr[d], at[(int64_t)k * D + d], iqr[k]);
}
template <int D>
__device__ __forceinline__ float to_s(const float* __restrict__ xr, const float* __restrict__ at, const float* __restrict__ iqr, float rn, int k,
                                      int d) {
    return to_e<D>(xr, at, iqr, k, d) * rn;
}

template <int D>
__global__ __launch_bounds__(64 * TA_WAVES) void to_norms_kernel(const float* __restrict__ x, const float* __restrict__ at, int64_t BT, int K,
                                                                 float* __restrict__ norms) {
    constexpr int N = TpVec<D>::N;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t row = (int64_t)blockIdx.x * TA_WAVES + wave;
    if (row >= BT) return;                                 // (wave-uniform; no barrier in this kernel)
    float* iq = norms;
    float* qg = norms + BT * K;
    float* ee = norms + 2 * BT * K;
    float* r = norms + 3 * BT * K;
    float* g2 = r + BT;
    float xv[N], a[N], eh[N];
    tp_load<D>(x + row * D, lane, xv);
    float q2 = 0.f;
    for (int k = 0; k < K; ++k) {
        tp_load<D>(at + (int64_t)k * D, lane, a);
        bool clamped;
        const float viq = tp_unit<N>(xv, a, eh, clamped);
        float sq = 0.f;
#pragma unroll
        for (int j = 0; j < N; ++j) sq = fmaf(eh[j], eh[j], sq);
        sq = wave_sum_dpp(sq);
        q2 += sq;
        if (lane == 0) {
            iq[row * K + k] = viq;
            qg[row * K + k] = clamped ? 0.f : 1.f;
            ee[row * K + k] = sq;
        }
    }
    if (lane == 0) {
        r[row] = 1.f / sqrtf(fmaxf(q2, kL2Eps));
        g2[row] = q2 > kL2Eps ? 1.f : 0.f;
    }
}

// a thread per (clip, feature): PASS 0: part[b][j] = sum_t s;  PASS 1: part[0][b][j] = sum_t (s - mu)^2, part[1][b][j] = sum_t (s - mu),
// mu = sum0[j] inv_n (two-level over t)
template <int D, int PASS>
__global__ __launch_bounds__(256) void to_stats_kernel(const float* __restrict__ x, const float* __restrict__ at, const float* __restrict__ norms,
                                                       const float* __restrict__ sum0, float inv_n, int B, int T, int K, float* __restrict__ part) {
    const int J = K * D, j = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (j >= J) return;
    const int k = j / D, d = j % D;
    const ToNorms nm = to_norms_of(norms, (int64_t)B * T, K);
    const float mu = PASS ? sum0[j] * inv_n : 0.f;
    float tot = 0.f, acc = 0.f, dtot = 0.f, dacc = 0.f;
    for (int t = 0; t < T; ++t) {
        const int64_t n = (int64_t)b * T + t;
        const float s = to_s<D>(x + n * D, at, nm.iq + n * K, nm.r[n], k, d);
        if (PASS) {
            const float dev = s - mu;
            acc = fmaf(dev, dev, acc);
            dacc += dev;
        } else {
            acc += s;
        }
        if ((t & (TP_SUM_CHUNK - 1)) == TP_SUM_CHUNK - 1) {
            tot += acc;
            dtot += dacc;
            acc = dacc = 0.f;
        }
    }
    part[(int64_t)b * J + j] = tot + acc;
    if (PASS) part[((int64_t)B + b) * J + j] = dtot + dacc;
}

// out[b][sl][t][c] = scale sum_{j in slice} s[b,t,j] cs_j w(b,j,c);  MODE 0: w [J, C];  MODE 1: w [B, C, J].  blockIdx.x = (b, tile, slice)
template <int D>
__global__ __launch_bounds__(256) void to_project_kernel(const float* __restrict__ x, const float* __restrict__ at, const float* __restrict__ norms,
                                                         const float* __restrict__ w, const float* __restrict__ cs, int mode, float scale, int B,
                                                         int T, int K, int C, int SL, float* __restrict__ out) {
    __shared__ float sT[TO_TT][TO_CH + 1];
    __shared__ float wT[TO_CH][TO_LDW];
    const int J = K * D, nch = J / TO_CH, ntt = (T + TO_TT - 1) / TO_TT;
    int id = blockIdx.x;
    const int sl = id % SL; id /= SL;
    const int tt = id % ntt, b = id / ntt;
    const int t0 = tt * TO_TT;
    const int cc = threadIdx.x & 31, r0 = threadIdx.x >> 5;
    const ToNorms nm = to_norms_of(norms, (int64_t)B * T, K);
    const int nout = TO_TT * C;
    float acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = 0.f;
    for (int ch = sl; ch < nch; ch += SL) {
        const int j0 = ch * TO_CH, k = j0 / D, d0 = j0 % D;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int tl = r0 + 8 * i, t = t0 + tl;
            float v = 0.f;
            if (t < T) {
                const int64_t n = (int64_t)b * T + t;
                v = to_s<D>(x + n * D, at, nm.iq + n * K, nm.r[n], k, d0 + cc);
            }
            sT[tl][cc] = v;
        }
        for (int idx = threadIdx.x; idx < TO_CH * C; idx += 256) {
            int jj, c;
            float v;
            if (mode == 0) {
                c = idx % C; jj = idx / C;
                v = w[(int64_t)(j0 + jj) * C + c];
            } else {
                jj = idx % TO_CH; c = idx / TO_CH;
                v = w[((int64_t)b * C + c) * J + j0 + jj];
            }
            wT[jj][c] = cs ? v * cs[j0 + jj] : v;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int o = threadIdx.x + 256 * i;
            if (o < nout) {
                const int tl = o / C, c = o % C;
                float a = acc[i];
#pragma unroll 8
                for (int jj = 0; jj < TO_CH; ++jj) a = fmaf(sT[tl][jj], wT[jj][c], a);
                acc[i] = a;
            }
        }
        __syncthreads();
    }
    float* po = out + ((int64_t)b * SL + sl) * T * C;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int o = threadIdx.x + 256 * i;
        if (o < nout) {
            const int tl = o / C, c = o % C;
            if (t0 + tl < T) po[(int64_t)(t0 + tl) * C + c] = acc[i] * scale;
        }
    }
}

// out[b,c,j] = sum_t p[b,t,c] s[b,t,j]: grid (J / 256, B, C / 8), a thread per feature
template <int D>
__global__ __launch_bounds__(256) void to_pool_kernel(const float* __restrict__ x, const float* __restrict__ at, const float* __restrict__ norms,
                                                      const float* __restrict__ p, int B, int T, int K, int C, float* __restrict__ out) {
    __shared__ float pT[TA_MAX_FRAMES][TO_PC];
    const int J = K * D, j = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y, c0 = blockIdx.z * TO_PC;
    for (int idx = threadIdx.x; idx < T * TO_PC; idx += 256) {
        const int t = idx / TO_PC, c = c0 + idx % TO_PC;
        pT[t][idx % TO_PC] = c < C ? p[((int64_t)b * T + t) * C + c] : 0.f;
    }
    __syncthreads();
    if (j >= J) return;                                    // (no barrier below)
    const int k = j / D, d = j % D;
    const ToNorms nm = to_norms_of(norms, (int64_t)B * T, K);
    float acc[TO_PC];
#pragma unroll
    for (int c = 0; c < TO_PC; ++c) acc[c] = 0.f;
    for (int t = 0; t < T; ++t) {
        const int64_t n = (int64_t)b * T + t;
        const float s = to_s<D>(x + n * D, at, nm.iq + n * K, nm.r[n], k, d);
#pragma unroll
        for (int c = 0; c < TO_PC; ++c) acc[c] = fmaf(pT[t][c], s, acc[c]);
    }
#pragma unroll
    for (int c = 0; c < TO_PC; ++c)
        if (c0 + c < C) out[((int64_t)b * C + c0 + c) * J + j] = acc[c];
}

// the four waves' totals in wave order; every thread gets the same bits
__device__ __forceinline__ float to_block_sum(float v, float* red) {
    v = wave_sum_dpp(v);
    __syncthreads();                                       // (red may still be read from the call before)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}
__device__ __forceinline__ float to_a(float S, float g, float h) { return g * S + h; }
__device__ __forceinline__ float to_z(float A, float alpha, float shift) { return alpha * A + shift; }

// a workgroup per (clip, cluster)
__global__ __launch_bounds__(256) void to_finish_kernel(const float* __restrict__ S, const float* __restrict__ g, const float* __restrict__ h,
                                                        const float* __restrict__ alpha, const float* __restrict__ shift, int J, float isc,
                                                        float* __restrict__ y, float* __restrict__ nrm2) {
    __shared__ float red[4];
    const int64_t o = (int64_t)blockIdx.x * J;
    const float al = alpha[0], sh = shift[0];
    float acc = 0.f;
    for (int j = threadIdx.x; j < J; j += 256) {
        const float z = to_z(to_a(S[o + j], g[j], h[j]), al, sh);
        acc = fmaf(z, z, acc);
    }
    const float n2 = to_block_sum(acc, red);
    const float inv = 1.f / sqrtf(fmaxf(n2, kL2Eps));
    for (int j = threadIdx.x; j < J; j += 256) y[o + j] = (to_z(to_a(S[o + j], g[j], h[j]), al, sh) * inv) * isc;
    if (threadIdx.x == 0) nrm2[blockIdx.x] = n2;
}

// a workgroup per (clip, cluster): dA = alpha dz;  scal[.][0] = sum_j dz A, scal[.][1] = sum_j dz
__global__ __launch_bounds__(256) void to_dz_kernel(const float* __restrict__ S, const float* __restrict__ g, const float* __restrict__ h,
                                                    const float* __restrict__ alpha, const float* __restrict__ shift,
                                                    const float* __restrict__ nrm2, const float* __restrict__ dy, int J, float isc,
                                                    float* __restrict__ dA, float* __restrict__ scal) {
    __shared__ float red[4];
    const int64_t o = (int64_t)blockIdx.x * J;
    const float al = alpha[0], sh = shift[0];
    const float n2 = nrm2[blockIdx.x];
    const bool open = n2 > kL2Eps;
    const float inv = 1.f / sqrtf(fmaxf(n2, kL2Eps));
    float acc = 0.f;
    if (open)
        for (int j = threadIdx.x; j < J; j += 256) acc = fmaf(to_z(to_a(S[o + j], g[j], h[j]), al, sh) * inv, dy[o + j], acc);
    const float dot = to_block_sum(acc, red);              // (0 where clamped)
    float sa = 0.f, ss = 0.f;
    for (int j = threadIdx.x; j < J; j += 256) {
        const float A = to_a(S[o + j], g[j], h[j]);
        const float yp = to_z(A, al, sh) * inv;
        const float dz = ((dy[o + j] - yp * dot) * inv) * isc;     // clamped: dot = 0, inv = 1e6
        sa = fmaf(dz, A, sa);
        ss += dz;
        dA[o + j] = al * dz;
    }
    sa = to_block_sum(sa, red);
    ss = to_block_sum(ss, red);
    if (threadIdx.x == 0) {
        scal[2 * (int64_t)blockIdx.x] = sa;
        scal[2 * (int64_t)blockIdx.x + 1] = ss;
    }
}

// part[0][chunk][j] = sum_rows dA, part[1][chunk][j] = sum_rows dA S over the chunk's TO_ROWS rows of [R, J]; blockIdx.y = chunk
__global__ __launch_bounds__(256) void to_colsum2_kernel(const float* __restrict__ dA, const float* __restrict__ S, int R, int J, int NC,
                                                         float* __restrict__ part) {
    const int j = blockIdx.x * 256 + threadIdx.x, ch = blockIdx.y;
    if (j >= J) return;
    float a = 0.f, b = 0.f;
    for (int r = ch * TO_ROWS; r < min((ch + 1) * TO_ROWS, R); ++r) {
        const float v = dA[(int64_t)r * J + j];
        a += v;
        b = fmaf(v, S[(int64_t)r * J + j], b);
    }
    part[(int64_t)ch * J + j] = a;
    part[((int64_t)NC + ch) * J + j] = b;
}

struct ToBwdArgs {
    const float *x, *at, *norms, *p, *dl, *dA, *w, *g, *mu, *c1, *c2;
    int B, T, K, C;
    float isj;                // 1 / sqrt(J)
    float *ed, *rowdot, *dx, *da_part;
};

// a thread per row: rowdot[n] = (s . ds) [q2 > eps] = r sum_k ed;  ed[n,k] <- (e_k . de) [q > eps] = r (ed - r rowdot ee)
__global__ __launch_bounds__(256) void to_dots_kernel(const float* __restrict__ norms, int64_t BT, int K, float* __restrict__ ed,
                                                      float* __restrict__ rowdot) {
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= BT) return;
    const ToNorms nm = to_norms_of(norms, BT, K);
    float acc = 0.f;
    for (int k = 0; k < K; ++k) acc += ed[n * K + k];
    const float r = nm.r[n], rd = (r * acc) * nm.g2[n];
    rowdot[n] = rd;
    for (int k = 0; k < K; ++k) ed[n * K + k] = (r * (ed[n * K + k] - (r * rd) * nm.ee[n * K + k])) * nm.qg[n * K + k];
}

// SWEEP 1: blockIdx.x = (clip, anchor), walks the chunks of D;  SWEEP 2: blockIdx.x = (clip, chunk), walks the anchors
template <int D, int SWEEP>
__global__ __launch_bounds__(256) void to_bwd_kernel(const ToBwdArgs A) {
    __shared__ float dSt[TO_MAX_CLUSTERS][TO_CH + 1], gWt[TO_MAX_CLUSTERS][TO_CH + 1];
    __shared__ float pT[TO_TT][TO_LDW], lT[TO_TT][TO_LDW];
    __shared__ float dotacc[TA_MAX_FRAMES], dacc[8 * 32];
    constexpr int NCH = D / TO_CH;
    const int T = A.T, K = A.K, C = A.C, J = K * D;
    const int b = SWEEP == 1 ? blockIdx.x / K : blockIdx.x / NCH;
    const int rest = SWEEP == 1 ? blockIdx.x % K : blockIdx.x % NCH;
    const int cc = threadIdx.x & 31, r0 = threadIdx.x >> 5;
    const ToNorms nm = to_norms_of(A.norms, (int64_t)A.B * T, K);
    if (SWEEP == 1)
        for (int t = threadIdx.x; t < T; t += 256) dotacc[t] = 0.f;
    const int steps = SWEEP == 1 ? NCH : K;
    for (int step = 0; step < steps; ++step) {
        const int k = SWEEP == 1 ? rest : step, c0 = (SWEEP == 1 ? step : rest) * TO_CH;
        const int d = c0 + cc, j = k * D + d;
        __syncthreads();                                   // (the step before has read the tiles and dacc)
        for (int idx = threadIdx.x; idx < C * TO_CH; idx += 256) {
            const int c = idx / TO_CH, jc = idx % TO_CH, jj = k * D + c0 + jc;
            const float gj = A.g[jj];
            dSt[c][jc] = gj * A.dA[((int64_t)b * C + c) * J + jj];
            gWt[c][jc] = (gj * A.isj) * A.w[(int64_t)jj * C + c];
        }
        const float c1 = A.c1 ? A.c1[j] : 0.f, c2 = A.c2 ? A.c2[j] : 0.f, mu = A.c2 ? A.mu[j] : 0.f;
        float da = 0.f;
        for (int t0 = 0; t0 < T; t0 += TO_TT) {
            __syncthreads();                               // (the tile before has been read; the first: dSt, gWt are written)
            for (int idx = threadIdx.x; idx < TO_TT * C; idx += 256) {
                const int tl = idx / C, c = idx % C, t = t0 + tl;
                const bool ok = t < T;
                pT[tl][c] = ok ? A.p[((int64_t)b * T + t) * C + c] : 0.f;
                lT[tl][c] = ok ? A.dl[((int64_t)b * T + t) * C + c] : 0.f;
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int tl = r0 + 8 * i, t = t0 + tl;
                const bool valid = t < T;                  // (uniform over the half-wave)
                float v = 0.f;
                if (valid) {
                    const int64_t n = (int64_t)b * T + t;
                    float ds = 0.f;
                    for (int c = 0; c < C; ++c) {
                        ds = fmaf(pT[tl][c], dSt[c][cc], ds);
                        ds = fmaf(lT[tl][c], gWt[c][cc], ds);
                    }
                    const float rn = nm.r[n];
                    const float e = to_e<D>(A.x + n * D, A.at, nm.iq + n * K, k, d);
                    const float s = e * rn;
                    ds = ds + (c1 + c2 * (s - mu));
                    if (SWEEP == 1) {
                        v = e * ds;
                    } else {
                        const float de = rn * (ds - s * A.rowdot[n]);
                        const float gr = nm.iq[n * K + k] * (de - e * A.ed[n * K + k]);
                        float* po = A.dx + n * D + d;
                        *po = step == 0 ? gr : *po + gr;   // (an earlier anchor of this workgroup: this thread wrote it)
                        da += gr;
                    }
                }
                if (SWEEP == 1) {
                    v = half_sum(v);                        // the 32 columns of the chunk: one half-wave per frame
                    if (cc == 0 && valid) dotacc[t] += v;   // (this thread's own entry in every chunk)
                }
            }
        }
        if (SWEEP == 2) {
            dacc[r0 * 32 + cc] = da;
            __syncthreads();
            if (threadIdx.x < 32) {
                float acc = dacc[cc];
                for (int r = 1; r < 8; ++r) acc += dacc[r * 32 + cc];
                A.da_part[((int64_t)b * K + k) * D + d] = acc;
            }
        }
    }
    if (SWEEP == 1) {
        __syncthreads();
        for (int t = threadIdx.x; t < T; t += 256) A.ed[((int64_t)b * T + t) * K + rest] = dotacc[t];
    }
}

static int to_slices(int B, int T, int J) {
    const int64_t wg = (int64_t)B * ((T + TO_TT - 1) / TO_TT);
    int64_t want = (512 + wg - 1) / wg;
    want = want < 1 ? 1 : (want > TO_MAX_SLICES ? TO_MAX_SLICES : want);
    const int nch = J / TO_CH;
    return (int)(nch < want ? nch : want);
}
static int to_check(const char* name, int B, int T, int D, int K, int C) {
    LPM_REQUIRE(B > 0 && K > 0, LPM_ERR_BADARG, "%s: need B, K >= 1 (B=%d K=%d)", name, B, K);
    LPM_REQUIRE(D == 128 || D == 1024, LPM_ERR_UNSUPPORTED_SHAPE, "%s: need D in {128, 1024} (D=%d)", name, D);
    LPM_REQUIRE(T >= 1 && T <= TA_MAX_FRAMES, LPM_ERR_UNSUPPORTED_SHAPE, "%s: need 1 <= T <= %d frames (T=%d): a clip's attention weights stay in LDS",
                name, TA_MAX_FRAMES, T);
    LPM_REQUIRE(C >= 1 && C <= TO_MAX_CLUSTERS, LPM_ERR_UNSUPPORTED_SHAPE, "%s: need 1 <= C <= %d clusters (C=%d)", name, TO_MAX_CLUSTERS, C);
    LPM_REQUIRE(B <= 65535 && (int64_t)K * D < (1ll << 24) && (int64_t)B * T * K < (1ll << 31) && (int64_t)B * C < (1ll << 24) &&
                    (int64_t)B * K * D < (1ll << 31),
                LPM_ERR_UNSUPPORTED_SHAPE, "%s: B, K * D, B * T * K, B * C or B * K * D too large (B=%d T=%d K=%d C=%d)", name, B, T, K, C);
    return LPM_OK;
}

}  // namespace lpm

extern "C" int lpm_triangulation_onefc_max_clusters(void) { return lpm::TO_MAX_CLUSTERS; }

extern "C" size_t lpm_triangulation_onefc_workspace_bytes(int which, int B, int T, int D, int K, int C) {
    if (B <= 0 || T <= 0 || D <= 0 || K <= 0 || C <= 0) return 0;
    const size_t J = (size_t)K * D;
    if (which == 0) return 2 * (size_t)B * J * sizeof(float);                       // stats: per-clip sums, two in the second pass
    if (which == 1) {                                                                // project: the slices' partials
        const int SL = lpm::to_slices(B, T, (int)J);
        return SL > 1 ? (size_t)B * SL * T * C * sizeof(float) : 0;
    }
    if (which == 2) return 2 * (((size_t)B * C + lpm::TO_ROWS - 1) / lpm::TO_ROWS) * J * sizeof(float);     // dz: the column sums' partials
    return ((size_t)B * T * K + (size_t)B * T + (size_t)B * J) * sizeof(float);     // bwd: dot products, danchors partials
}

extern "C" int lpm_triangulation_onefc_norms(const float* x, const float* anchors_t, int B, int T, int D, int K, float* norms,
                                             lpm_stream_t stream) {
    using namespace lpm;
    const char* name = "lpm_triangulation_onefc_norms";
    LPM_REQUIRE(x && anchors_t && norms, LPM_ERR_BADARG, "%s: null pointer", name);
    if (const int rc = to_check(name, B, T, D, K, 1)) return rc;
    LPM_REQUIRE((((uintptr_t)x | (uintptr_t)anchors_t) & 15) == 0, LPM_ERR_BADARG, "%s: x and anchors_t must be 16-byte aligned", name);
    const int64_t BT = (int64_t)B * T;
    const dim3 grid((unsigned)((BT + TA_WAVES - 1) / TA_WAVES)), block(64 * TA_WAVES);
    tp_dispatch_d(D, [&](auto d) {
        hipLaunchKernelGGL((to_norms_kernel<decltype(d)::value>), grid, block, 0, (hipStream_t)stream, x, anchors_t, BT, K, norms);
    });
    return check_launch(name);
}

extern "C" int lpm_triangulation_onefc_stats(const float* x, const float* anchors_t, const float* norms, int B, int T, int D, int K, float* sums,
                                             void* workspace, size_t workspace_bytes, lpm_stream_t stream) {
    using namespace lpm;
    const char* name = "lpm_triangulation_onefc_stats";
    LPM_REQUIRE(x && anchors_t && norms && sums, LPM_ERR_BADARG, "%s: null pointer", name);
    if (const int rc = to_check(name, B, T, D, K, 1)) return rc;
    LPM_REQUIRE(workspace && workspace_bytes >= lpm_triangulation_onefc_workspace_bytes(0, B, T, D, K, 1), LPM_ERR_WORKSPACE,
                "%s: workspace too small", name);
    hipStream_t s = (hipStream_t)stream;
    const int J = K * D;
    const dim3 grid((J + 255) / 256, B), block(256);
    float* part = (float*)workspace;
    const float inv_n = 1.f / (float)((int64_t)B * T);
    int rc = LPM_OK;
    tp_dispatch_d(D, [&](auto d) {
        constexpr int DD = decltype(d)::value;
        hipLaunchKernelGGL((to_stats_kernel<DD, 0>), grid, block, 0, s, x, anchors_t, norms, nullptr, 0.f, B, T, K, part);
        if ((rc = ta_sum_slices(part, 1, J, B, sums, s, name))) return;
        hipLaunchKernelGGL((to_stats_kernel<DD, 1>), grid, block, 0, s, x, anchors_t, norms, sums, inv_n, B, T, K, part);
        rc = ta_sum_slices(part, 2, J, B, sums + J, s, name);
    });
    if (rc) return rc;
    return check_launch(name);
}

extern "C" int lpm_triangulation_onefc_project(const float* x, const float* anchors_t, const float* norms, const float* w, const float* colscale,
                                               int mode, float scale, int B, int T, int D, int K, int C, float* out, void* workspace,
                                               size_t workspace_bytes, lpm_stream_t stream) {
    using namespace lpm;
    const char* name = "lpm_triangulation_onefc_project";
    LPM_REQUIRE(x && anchors_t && norms && w && out, LPM_ERR_BADARG, "%s: null pointer", name);
    LPM_REQUIRE(mode == 0 || mode == 1, LPM_ERR_BADARG, "%s: mode must be 0 (w [J, C]) or 1 (w [B, C, J])", name);
    if (const int rc = to_check(name, B, T, D, K, C)) return rc;
    const size_t need = lpm_triangulation_onefc_workspace_bytes(1, B, T, D, K, C);
    LPM_REQUIRE(need == 0 || (workspace && workspace_bytes >= need), LPM_ERR_WORKSPACE, "%s: workspace too small", name);
    hipStream_t s = (hipStream_t)stream;
    const int J = K * D, SL = to_slices(B, T, J), ntt = (T + TO_TT - 1) / TO_TT;
    float* part = SL > 1 ? (float*)workspace : out;
    const dim3 grid((unsigned)(B * ntt * SL)), block(256);
    tp_dispatch_d(D, [&](auto d) {
        hipLaunchKernelGGL((to_project_kernel<decltype(d)::value>), grid, block, 0, s, x, anchors_t, norms, w, colscale, mode, scale, B, T, K, C, SL,
                           part);
    });
    if (SL > 1)
        if (const int rc = ta_sum_slices(part, B, (int64_t)T * C, SL, out, s, name)) return rc;
    return check_launch(name);
}

extern "C" int lpm_triangulation_onefc_pool(const float* x, const float* anchors_t, const float* norms, const float* p, int B, int T, int D, int K,
                                            int C, float* out, float* sum_out, lpm_stream_t stream) {
    using namespace lpm;
    const char* name = "lpm_triangulation_onefc_pool";
    LPM_REQUIRE(x && anchors_t && norms && p && out, LPM_ERR_BADARG, "%s: null pointer", name);
    if (const int rc = to_check(name, B, T, D, K, C)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int J = K * D;
    const dim3 grid((J + 255) / 256, B, (C + TO_PC - 1) / TO_PC), block(256);
    tp_dispatch_d(D, [&](auto d) {
        hipLaunchKernelGGL((to_pool_kernel<decltype(d)::value>), grid, block, 0, s, x, anchors_t, norms, p, B, T, K, C, out);
    });
    if (sum_out)
        if (const int rc = ta_sum_slices(out, 1, (int64_t)C * J, B, sum_out, s, name)) return rc;
    return check_launch(name);
}

extern "C" int lpm_triangulation_onefc_finish(const float* S, const float* g, const float* h, const float* alpha, const float* shift, int B, int C,
                                              int J, float* y, float* nrm2, lpm_stream_t stream) {
    using namespace lpm;
    const char* name = "lpm_triangulation_onefc_finish";
    LPM_REQUIRE(S && g && h && alpha && shift && y && nrm2, LPM_ERR_BADARG, "%s: null pointer", name);
    LPM_REQUIRE(B > 0 && C > 0 && C <= TO_MAX_CLUSTERS && J > 0 && (int64_t)B * C < (1ll << 24), LPM_ERR_UNSUPPORTED_SHAPE,
                "%s: need B, J >= 1, 1 <= C <= %d (B=%d C=%d J=%d)", name, TO_MAX_CLUSTERS, B, C, J);
    hipLaunchKernelGGL(to_finish_kernel, dim3((unsigned)(B * C)), dim3(256), 0, (hipStream_t)stream, S, g, h, alpha, shift, J,
                       1.f / sqrtf((float)C), y, nrm2);
    return check_launch(name);
}

extern "C" int lpm_triangulation_onefc_dz(const float* S, const float* g, const float* h, const float* alpha, const float* shift, const float* nrm2,
                                          const float* dy, int B, int C, int J, float* dA, float* scal, float* dhg, void* workspace,
                                          size_t workspace_bytes, lpm_stream_t stream) {
    using namespace lpm;
    const char* name = "lpm_triangulation_onefc_dz";
    LPM_REQUIRE(S && g && h && alpha && shift && nrm2 && dy && dA && scal && dhg, LPM_ERR_BADARG, "%s: null pointer", name);
    LPM_REQUIRE(B > 0 && C > 0 && C <= TO_MAX_CLUSTERS && J > 0 && (int64_t)B * C < (1ll << 24), LPM_ERR_UNSUPPORTED_SHAPE,
                "%s: need B, J >= 1, 1 <= C <= %d (B=%d C=%d J=%d)", name, TO_MAX_CLUSTERS, B, C, J);
    const int R = B * C, NC = (R + TO_ROWS - 1) / TO_ROWS;
    LPM_REQUIRE(workspace && workspace_bytes >= 2 * (size_t)NC * J * sizeof(float), LPM_ERR_WORKSPACE, "%s: workspace too small", name);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(to_dz_kernel, dim3((unsigned)R), dim3(256), 0, s, S, g, h, alpha, shift, nrm2, dy, J, 1.f / sqrtf((float)C), dA, scal);
    hipLaunchKernelGGL(to_colsum2_kernel, dim3((J + 255) / 256, NC), dim3(256), 0, s, dA, S, R, J, NC, (float*)workspace);
    if (const int rc = ta_sum_slices((const float*)workspace, 2, J, NC, dhg, s, name)) return rc;
    return check_launch(name);
}

extern "C" int lpm_triangulation_onefc_bwd(const float* x, const float* anchors_t, const float* norms, const float* p, const float* dl,
                                           const float* dA, const float* w, const float* g, const float* mu, const float* c1, const float* c2, int B,
                                           int T, int D, int K, int C, float* dx, float* danchors, void* workspace, size_t workspace_bytes,
                                           lpm_stream_t stream) {
    using namespace lpm;
    const char* name = "lpm_triangulation_onefc_bwd";
    LPM_REQUIRE(x && anchors_t && norms && p && dl && dA && w && g && dx && danchors, LPM_ERR_BADARG, "%s: null pointer", name);
    LPM_REQUIRE((!c1 && !c2 && !mu) || (c1 && c2 && mu), LPM_ERR_BADARG, "%s: mu, c1 and c2 come together", name);
    if (const int rc = to_check(name, B, T, D, K, C)) return rc;
    LPM_REQUIRE(workspace && workspace_bytes >= lpm_triangulation_onefc_workspace_bytes(3, B, T, D, K, C), LPM_ERR_WORKSPACE,
                "%s: workspace too small", name);
    hipStream_t s = (hipStream_t)stream;
    const int64_t BT = (int64_t)B * T;
    ToBwdArgs A{};
    A.x = x; A.at = anchors_t; A.norms = norms; A.p = p; A.dl = dl; A.dA = dA; A.w = w; A.g = g; A.mu = mu; A.c1 = c1; A.c2 = c2;
    A.B = B; A.T = T; A.K = K; A.C = C;
    A.isj = 1.f / sqrtf((float)((int64_t)K * D));
    A.ed = (float*)workspace;
    A.rowdot = A.ed + BT * K;
    A.da_part = A.rowdot + BT;
    A.dx = dx;
    const dim3 block(256), grid_k((unsigned)(B * K)), grid_c((unsigned)(B * (D / TO_CH)));
    tp_dispatch_d(D, [&](auto d) {
        constexpr int DD = decltype(d)::value;
        hipLaunchKernelGGL((to_bwd_kernel<DD, 1>), grid_k, block, 0, s, A);
        hipLaunchKernelGGL(to_dots_kernel, dim3((unsigned)((BT + 255) / 256)), block, 0, s, norms, BT, K, A.ed, A.rowdot);
        hipLaunchKernelGGL((to_bwd_kernel<DD, 2>), grid_c, block, 0, s, A);
    });
    if (const int rc = ta_reduce_partials(dx, A.da_part, B, T, D, K, 1, TP_SUM_CHUNK, dx, danchors, s, name)) return rc;
    return check_launch(name);
}
