// Mean-only pooling of the triangulation embedding for TriangulationCnnClusterModel (frame_level_models.py:757-939:
// IndirectClusterMeanPoolModule over TriangulationEmbedding, MeanStdPoolModule over TriangulationTemporalEmbedding, each behind a
// per-anchor linear map that commutes with the pooling and is applied to the pooled vectors by the caller).  With e, f exactly as in
// triangulation_pool.hip (the same clamps, f = 0 for identical frames):
//   G_d[t,s] = <e_t, e_s> over all K*D;  w = softmax_t(sum_s relu(G_d[t,s]))  (the caller: tiny)
//   m_d = (1/T) sum_t w[t] e_t;  m_t = (1/(T-1)) sum_{t>=1} f_t
// triangulation_attention.hip computes a superset (the temporal Gram, both maxima and their arg-max tensor, a weighted temporal mean);
// what is here drops all of that: no f tile and no f MFMAs in the Gram, no maxima in the walk, one M V product in the backward
// instead of two, and one sweep over D fewer.  Nothing of size T*K*D exists in either direction; no floating-point atomics: every
// cross-workgroup sum has a fixed order.  The Gram and the backward's M_d E run on v_mfma_f32_32x32x2_f32 -- exact fp32 products,
// fp32 accumulation (the logits enter a softmax: see triangulation_attention.hip).
//
// lpm_triangulation_mean_gram: a workgroup (4 waves) owns a clip, a pair I <= J of 64-frame tiles (G_d is symmetric: the block is
// written to both places) and a slice of the anchors.  Per anchor: the norms of its 64 (128) frames, one wave per frame, then D in
// 32-column chunks -- e of the chunk to LDS, each wave adds its 32x32 quadrant of E_I E_J^T.  Two-level sums: an anchor's product in
// registers, onto the slice's total; the slices' partial Grams are added s = 0, 1, ... by a second pass.
//
// lpm_triangulation_mean_pool_fwd / _dw: tp_walk_fwd_kernel<D, w, no weight on f, no maxima> and tp_walk_dw_kernel<D, not temporal>
// (triangulation_common.h; tests/test_gpu_triangulation_family.py holds m_t bitwise equal to triangulation_pool's mean_t).
//
// lpm_triangulation_mean_bwd: with M = dG_d + dG_d^T (symmetric, from the caller) and gf = g_t[k] / (T-1), ONE row per anchor:
//   gu_t = ip (gf - f_t (f_t . gf) [p > 1e-12])  (t >= 1)         ge_t = (w[t] / T) g_d[k] + (M E_k)[t] + gu_t - gu_{t+1}
//   gr_t = s iq (ge_t - eh_t (eh_t . ge_t) [q > 1e-12])           dx[b,t,:] = sum_k gr_t      danchors[:,k] = - sum_{b,t} gr_t
// A workgroup owns a clip and the anchors k = g, g + G, ...; per anchor the pass that takes the norms of all frames (ta_norms: one
// wave per frame, the whole row in registers) takes (f_t . gf) as well, so D is walked twice in 32-column chunks, not three times: (eh . ge),
// then gr.  Per chunk: the frames to LDS ([T,33]), M E on the matrix cores into a second [T,33] tile, a thread per (t, column) for the
// chain.  Partials and their reductions as in triangulation_attention.hip.
#include "triangulation_common.h"

// the contraction rule (triangulation_common.h) for everything below
#pragma clang fp contract(off)

namespace lpm {

constexpr int TM_MAX_JOBS = (TA_MAX_FRAMES / 32 + TA_WAVES - 1) / TA_WAVES;    // 32-row tiles of M E per wave and chunk

static int tm_pairs(int T) { return ta_tiles(T) * (ta_tiles(T) + 1) / 2; }
static int tm_slices(int B, int T, int K) {
    const int64_t wg = (int64_t)B * tm_pairs(T);
    int64_t want = (512 + wg - 1) / wg;
    want = want < 1 ? 1 : (want > TA_MAX_SLICES ? TA_MAX_SLICES : want);
    return (int)(K < want ? K : want);
}

template <int D>
__global__ __launch_bounds__(64 * TA_WAVES) void tm_gram_kernel(const float* __restrict__ x, const float* __restrict__ anchors, int T, int K,
                                                                float s, int S, int NT, float* __restrict__ part) {
    constexpr int N = TpVec<D>::N;
    __shared__ float nrm[2][64];                           // [tile I / J]
    __shared__ float tile[2][64][TA_LD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int NP = NT * (NT + 1) / 2;
    int id = blockIdx.x;
    int tj = id % NP, ti = 0; id /= NP;                    // pair number -> (ti <= tj): row ti holds NT - ti pairs
    while (tj >= NT - ti) { tj -= NT - ti; ++ti; }
    tj += ti;
    const int sl = id % S, b = id / S;
    const bool diag = ti == tj;
    const int nside = diag ? 1 : 2;
    const float* xb = x + (int64_t)b * T * D;
    const int c = threadIdx.x & 31, r0 = threadIdx.x >> 5;
    const int qi = wave >> 1, qj = wave & 1;
    const float (*tI)[TA_LD] = tile[0];
    const float (*tJ)[TA_LD] = tile[diag ? 0 : 1];
    f32x16 tot;
#pragma unroll
    for (int r = 0; r < 16; ++r) tot[r] = 0.f;
    // a thread's frames of the NEXT chunk and its anchor column are loaded while the current chunk's products run
    float xr[2][8], avn = anchors[(int64_t)c * K + sl];
#pragma unroll
    for (int side = 0; side < 2; ++side) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int t = (side ? tj : ti) * 64 + r0 + 8 * i;
            xr[side][i] = (side < nside && t < T) ? xb[(int64_t)t * D + c] : 0.f;
        }
    }
    for (int k = sl; k < K; k += S) {
        {
            float a[N];
            tp_load_anchor<D>(anchors, K, k, lane, a);
            for (int side = 0; side < nside; ++side)
                ta_norms<D, 0>(xb, a, nullptr, T, (side ? tj : ti) * 64, 64, s, nrm[side], nullptr, nullptr, nullptr, nullptr);
        }
        __syncthreads();
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        for (int c0 = 0; c0 < D; c0 += TA_CH) {
            const float av = avn;
#pragma unroll
            for (int side = 0; side < 2; ++side) {
                if (side < nside) {
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        const int r = r0 + 8 * i;
                        tile[side][r][c] = ta_eh(xr[side][i], av, nrm[side][r]) * s;      // (0 for t >= T: the norm is 0 there)
                    }
                }
            }
            __syncthreads();
            {                                              // the next chunk's frames (they do not depend on the anchor) and anchor column
                const int cn = (c0 + TA_CH) % D + c;
                avn = anchors[(int64_t)cn * K + (c0 + TA_CH < D ? k : min(k + S, K - 1))];
#pragma unroll
                for (int side = 0; side < 2; ++side) {
                    if (side < nside) {
#pragma unroll
                        for (int i = 0; i < 8; ++i) {
                            const int t = (side ? tj : ti) * 64 + r0 + 8 * i;
                            xr[side][i] = t < T ? xb[(int64_t)t * D + cn] : 0.f;
                        }
                    }
                }
            }
#pragma unroll
            for (int kk = 0; kk < TA_CH; kk += 2) {
                const int col = kk + (lane >> 5), ra = 32 * qi + (lane & 31), rb = 32 * qj + (lane & 31);
                acc = mfma32(tI[ra][col], tJ[rb][col], acc);
            }
            __syncthreads();
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) tot[r] += acc[r];
    }
    float* o = part + ((int64_t)b * S + sl) * T * T;
    const int u = tj * 64 + 32 * qj + (lane & 31);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int t = ti * 64 + 32 * qi + mfma32_row(r, lane);
        if (t < T && u < T) {
            o[(int64_t)t * T + u] = tot[r];
            if (!diag) o[(int64_t)u * T + t] = tot[r];       // (a diagonal pair's four quadrants cover both halves themselves)
        }
    }
}

// TP = 64: T <= 64, every loop over the frames unrolled, M of the clip in LDS (two 32-row tiles of M E per chunk: waves 2 and 3 take
// no part in the product); TP = 0: any T <= TA_MAX_FRAMES, M from global memory (L2), up to TM_MAX_JOBS tiles per wave.
template <int D, int TP>
__global__ __launch_bounds__(64 * TA_WAVES) void tm_bwd_kernel(const float* __restrict__ x, const float* __restrict__ anchors,
                                                               const float* __restrict__ w, const float* __restrict__ m,
                                                               const float* __restrict__ g_d, const float* __restrict__ g_t, int T, int K,
                                                               float s, int G, float* __restrict__ dx_part, float* __restrict__ da_part) {
    constexpr int N = TpVec<D>::N, MAXJ = TP ? (TP / 32 + TA_WAVES - 1) / TA_WAVES : TM_MAX_JOBS;
    constexpr int UNR = TP ? TP / 8 : 1;                   // a thread's frames: loops unrolled and loads issued early when their count is known
    constexpr int UNRB = TP ? UNR / 4 : 1;                 // ... in batches of four
    // LDS: the frames of one chunk of D for all t ([Tp][33]), (M E)[t] of the chunk (the same shape), the frames' norms, gates and
    // (f . gf), (eh . ge) per frame, the clip's weights, the eight row groups' column sums for danchors, and (TP) M
    extern __shared__ __attribute__((aligned(16))) float tm_sh[];
    const int Tp = TP ? TP : ((T + 31) & ~31), ntt = Tp / 32;
    float (*tX)[TA_LD] = reinterpret_cast<float (*)[TA_LD]>(tm_sh);
    float (*tP)[TA_LD] = tX + Tp;
    float* iq = tm_sh + 2 * Tp * TA_LD;
    float *qg = iq + Tp, *ip = qg + Tp, *pg = ip + Tp, *dotf = pg + Tp, *dote = dotf + Tp, *wl = dote + Tp, *dacc = wl + Tp;
    float* mL = dacc + 8 * 32;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = threadIdx.x & 31, r0 = threadIdx.x >> 5;           // (c is lane & 31 as well: the column of the MFMA operands)
    const int b = blockIdx.x / G, g = blockIdx.x % G;
    const float* xb = x + (int64_t)b * T * D;
    float* dxo = dx_part + ((int64_t)b * G + g) * T * D;   // this workgroup's own [T, D] block (dx itself when G == 1)
    const float* mb = m + (int64_t)b * T * T;
    const float inv_d = 1.f / (float)T, inv_t = 1.f / (float)(T - 1);
    for (int t = threadIdx.x; t < Tp; t += 64 * TA_WAVES) wl[t] = t < T ? w[(int64_t)b * T + t] : 0.f;
    // the frames of the NEXT chunk are loaded while the current one is worked on (they depend on neither the anchor nor the sweep)
    float xr[UNR], dxold[UNR];
    if (TP) {
#pragma unroll
        for (int i = 0; i < UNR; ++i) xr[i] = r0 + 8 * i < T ? xb[(int64_t)(r0 + 8 * i) * D + c] : 0.f;
        for (int i = threadIdx.x; i < TP * TP; i += 64 * TA_WAVES) {   // zero outside the frames
            const int sr = i / (TP ? TP : 1), tc = i % (TP ? TP : 1);
            mL[i] = (sr < T && tc < T) ? mb[(int64_t)sr * T + tc] : 0.f;
        }
    }
    for (int k = g; k < K; k += G) {
        const bool first = k == g;
        const int64_t o = ((int64_t)b * K + k) * D;
        {
            float a[N], gf[N];
            tp_load_anchor<D>(anchors, K, k, lane, a);
            tp_load<D>(g_t + o, lane, gf);
#pragma unroll
            for (int j = 0; j < N; ++j) gf[j] *= inv_t;
            ta_norms<D, TN_TEMPORAL | TN_GATES | TN_DOTF>(xb, a, gf, T, 0, Tp, s, iq, qg, ip, pg, dotf);
        }
        for (int t = threadIdx.x; t < Tp; t += 64 * TA_WAVES) dote[t] = 0.f;
        __syncthreads();
        for (int sweep = 0; sweep < 2; ++sweep) {          // 0: (eh . ge) of every frame; 1: gr
            for (int c0 = 0; c0 < D; c0 += TA_CH) {
                const float av = anchors[(int64_t)(c0 + c) * K + k];
                if (TP) {
#pragma unroll
                    for (int i = 0; i < UNR; ++i) tX[r0 + 8 * i][c] = xr[i];
                } else {                                   // (every load issued before the first store: one latency per chunk, not one per frame)
                    float xv[TA_MAX_FRAMES / 8];
#pragma unroll
                    for (int i = 0; i < TA_MAX_FRAMES / 8; ++i) {
                        const int t = r0 + 8 * i;
                        if (8 * i < Tp) xv[i] = t < T ? xb[(int64_t)t * D + c0 + c] : 0.f;
                    }
#pragma unroll
                    for (int i = 0; i < TA_MAX_FRAMES / 8; ++i)
                        if (8 * i < Tp) tX[r0 + 8 * i][c] = xv[i];
                }
                __syncthreads();
                // (issued here, used behind the matrix product)
                const float gmd = g_d[o + c0 + c] * inv_d, gmt = g_t[o + c0 + c] * inv_t;
                if (TP) {
                    const int cn = (c0 + TA_CH) % D + c;
#pragma unroll
                    for (int i = 0; i < UNR; ++i) {
                        const int t = r0 + 8 * i;
                        xr[i] = t < T ? xb[(int64_t)t * D + cn] : 0.f;
                        dxold[i] = (sweep == 1 && !first && t < T) ? dxo[(int64_t)t * D + c0 + c] : 0.f;
                    }
                }
#pragma unroll
                for (int ji = 0; ji < MAXJ; ++ji) {
                    const int j = wave + TA_WAVES * ji;
                    if (j < ntt) {                         // (wave-uniform)
                        const int t0 = 32 * j;
                        f32x16 ac;
#pragma unroll
                        for (int r = 0; r < 16; ++r) ac[r] = 0.f;
                        // A[t][s] = M[t][s] = M[s][t]: read along M's rows.  B[s][c] = e of frame s, from the frames in LDS
                        if (TP) {
                            const float* mp = mL + t0 + c;
#pragma unroll 8
                            for (int s2 = 0; s2 < TP; s2 += 2) {
                                const int srow = s2 + (lane >> 5);
                                ac = mfma32(mp[srow * TP], ta_e(tX, iq, srow, c, av, s), ac);
                            }
                        } else {
                            // M comes from L2: the 16 values of the NEXT 32 rows are in flight while the matrix cores take the
                            // current ones (one load per product, waited for in turn, left them idle nine tenths of the time)
                            const int tcol = t0 + c, sh = lane >> 5;
                            const float* mp = mb + tcol;
                            float cur[16], nxt[16];
#pragma unroll
                            for (int i = 0; i < 16; ++i) cur[i] = (tcol < T && 2 * i + sh < T) ? mp[(int64_t)(2 * i + sh) * T] : 0.f;
                            for (int s0 = 0; s0 < Tp; s0 += 32) {
#pragma unroll
                                for (int i = 0; i < 16; ++i) {
                                    const int srow = s0 + 32 + 2 * i + sh;                 // (>= Tp behind the last block: nothing is read)
                                    nxt[i] = (tcol < T && srow < T) ? mp[(int64_t)srow * T] : 0.f;
                                }
#pragma unroll
                                for (int i = 0; i < 16; ++i) ac = mfma32(cur[i], ta_e(tX, iq, s0 + 2 * i + sh, c, av, s), ac);
#pragma unroll
                                for (int i = 0; i < 16; ++i) cur[i] = nxt[i];
                            }
                        }
#pragma unroll
                        for (int r = 0; r < 16; ++r) tP[t0 + mfma32_row(r, lane)][c] = ac[r];
                    }
                }
                __syncthreads();
                // tP[t] = (M E)[t] for this chunk; one thread per (t, column)
                float da = 0.f;
                // four frames at a time: their LDS reads and (second and later anchors) their dx values are in flight together
#pragma unroll UNRB
                for (int i0 = 0; i0 < Tp / 8; i0 += 4) {
                    float old[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int t = r0 + 8 * (i0 + j);
                        // an earlier anchor of this workgroup: this thread wrote it
                        old[j] = TP ? dxold[TP ? i0 + j : 0] : ((sweep == 1 && !first && t < T) ? dxo[(int64_t)t * D + c0 + c] : 0.f);
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int t = r0 + 8 * (i0 + j);
                        const bool valid = t < T;
                        float v = 0.f;
                        if (valid) {
                            const float eh = ta_eh(tX[t][c], av, iq[t]), e = eh * s;
                            float gu = 0.f, gun = 0.f;
                            if (t >= 1) {
                                const float f = (e - ta_e(tX, iq, t - 1, c, av, s)) * ip[t];
                                gu = ip[t] * (gmt - f * (dotf[t] * pg[t]));
                            }
                            if (t + 1 < T) {
                                const float fn = (ta_e(tX, iq, t + 1, c, av, s) - e) * ip[t + 1];
                                gun = ip[t + 1] * (gmt - fn * (dotf[t + 1] * pg[t + 1]));
                            }
                            const float ge = wl[t] * gmd + tP[t][c] + gu - gun;
                            if (sweep == 0) {
                                v = eh * ge;
                            } else {
                                const float gr = (s * iq[t]) * (ge - eh * (dote[t] * qg[t]));
                                dxo[(int64_t)t * D + c0 + c] = first ? gr : old[j] + gr;
                                da += gr;
                            }
                        }
                        if (sweep == 0) {
                            v = half_sum_dpp(v);            // the 32 columns of the chunk: one half-wave per frame
                            if (c == 0 && valid) dote[t] += v;
                        }
                    }
                }
                if (sweep == 1) {
                    dacc[r0 * 32 + c] = da;
                    __syncthreads();
                    if (threadIdx.x < 32) {
                        float acc_a = dacc[c];
                        for (int r = 1; r < 8; ++r) acc_a += dacc[r * 32 + c];
                        da_part[o + c0 + c] = acc_a;
                    }
                }
                __syncthreads();
            }
        }
    }
}

static size_t tm_bwd_lds(int T) {
    const bool fast = T <= TA_FAST_FRAMES;
    const int Tp = fast ? TA_FAST_FRAMES : (T + 31) & ~31;
    return ((size_t)2 * Tp * TA_LD + 7 * Tp + 8 * 32 + (fast ? TA_FAST_FRAMES * TA_FAST_FRAMES : 0)) * sizeof(float);
}

}  // namespace lpm

extern "C" size_t lpm_triangulation_mean_workspace_bytes(int which, int B, int T, int D, int K) {
    if (B <= 0 || T <= 1 || D <= 0 || K <= 0) return 0;
    if (which == 0) {                                       // gram: the slices' partial Grams
        const int S = lpm::tm_slices(B, T, K);
        return S > 1 ? (size_t)B * S * T * T * sizeof(float) : 0;
    }
    if (which == 1) return (size_t)B * K * T * sizeof(float);                     // dw: per-(clip, anchor) dot products
    const int G = lpm::ta_groups(B, K);                     // bwd: danchors partials, dx partials
    return ((size_t)B * K * D + (G > 1 ? (size_t)B * G * T * D : 0)) * sizeof(float);
}

extern "C" int lpm_triangulation_mean_gram(const float* x, const float* anchors, int B, int T, int D, int K, float scale, float* gram_d,
                                           void* workspace, size_t workspace_bytes, lpm_stream_t stream) {
    using namespace lpm;
    const char* name = "lpm_triangulation_mean_gram";
    LPM_REQUIRE(x && anchors && gram_d, LPM_ERR_BADARG, "%s: null pointer", name);
    if (const int rc = ta_check(name, B, T, D, K)) return rc;
    const size_t need = lpm_triangulation_mean_workspace_bytes(0, B, T, D, K);
    LPM_REQUIRE(need == 0 || (workspace && workspace_bytes >= need), LPM_ERR_WORKSPACE, "%s: workspace too small", name);
    LPM_REQUIRE(((uintptr_t)x & 15) == 0, LPM_ERR_BADARG, "%s: x must be 16-byte aligned", name);
    const int S = tm_slices(B, T, K), NT = ta_tiles(T);
    float* part = S > 1 ? (float*)workspace : gram_d;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)(B * S * tm_pairs(T))), block(64 * TA_WAVES);
    tp_dispatch_d(D, [&](auto d) { hipLaunchKernelGGL(tm_gram_kernel<decltype(d)::value>, grid, block, 0, s, x, anchors, T, K, scale, S, NT, part); });
    if (S > 1) {
        if (const int rc = ta_sum_slices(part, B, (int64_t)T * T, S, gram_d, s, name)) return rc;
    }
    return check_launch(name);
}

extern "C" int lpm_triangulation_mean_pool_fwd(const float* x, const float* anchors, const float* w_d, int B, int T, int D, int K, float scale,
                                               float* m_d, float* m_t, lpm_stream_t stream) {
    using namespace lpm;
    const char* name = "lpm_triangulation_mean_pool_fwd";
    LPM_REQUIRE(x && anchors && w_d && m_d && m_t, LPM_ERR_BADARG, "%s: null pointer", name);
    if (const int rc = ta_check(name, B, T, D, K)) return rc;
    LPM_REQUIRE((((uintptr_t)x | (uintptr_t)m_d | (uintptr_t)m_t) & 15) == 0, LPM_ERR_BADARG, "%s: x and the outputs must be 16-byte aligned", name);
    tp_dispatch_d(D, [&](auto d) {
        hipLaunchKernelGGL((tp_walk_fwd_kernel<decltype(d)::value, true, false, false>), dim3(tp_walk_grid(B, K)), dim3(64 * TP_WALK_WAVES), 0,
                           (hipStream_t)stream, x, anchors, w_d, nullptr, T, K, scale, m_d, nullptr, m_t, nullptr, nullptr);
    });
    return check_launch(name);
}

extern "C" int lpm_triangulation_mean_dw(const float* x, const float* anchors, const float* g_d, int B, int T, int D, int K, float scale,
                                         float* dw_d, void* workspace, size_t workspace_bytes, lpm_stream_t stream) {
    using namespace lpm;
    const char* name = "lpm_triangulation_mean_dw";
    LPM_REQUIRE(x && anchors && g_d && dw_d, LPM_ERR_BADARG, "%s: null pointer", name);
    if (const int rc = ta_check(name, B, T, D, K)) return rc;
    LPM_REQUIRE(workspace && workspace_bytes >= lpm_triangulation_mean_workspace_bytes(1, B, T, D, K), LPM_ERR_WORKSPACE,
                "%s: workspace too small", name);
    LPM_REQUIRE((((uintptr_t)x | (uintptr_t)g_d) & 15) == 0, LPM_ERR_BADARG, "%s: x and the gradient must be 16-byte aligned", name);
    float* part = (float*)workspace;
    hipStream_t s = (hipStream_t)stream;
    tp_dispatch_d(D, [&](auto d) {
        hipLaunchKernelGGL((tp_walk_dw_kernel<decltype(d)::value, false>), dim3(tp_walk_grid(B, K)), dim3(64 * TP_WALK_WAVES), 0, s, x, anchors,
                           g_d, T, K, scale, part, nullptr, nullptr);
    });
    if (const int rc = ta_sum_slices(part, B, T, K, dw_d, s, name)) return rc;
    return check_launch(name);
}

extern "C" int lpm_triangulation_mean_bwd(const float* x, const float* anchors, const float* w_d, const float* m_d, const float* g_d,
                                          const float* g_t, int B, int T, int D, int K, float scale, float* dx, float* danchors,
                                          void* workspace, size_t workspace_bytes, lpm_stream_t stream) {
    using namespace lpm;
    const char* name = "lpm_triangulation_mean_bwd";
    LPM_REQUIRE(x && anchors && w_d && m_d && g_d && g_t && dx && danchors, LPM_ERR_BADARG, "%s: null pointer", name);
    if (const int rc = ta_check(name, B, T, D, K)) return rc;
    LPM_REQUIRE(workspace && workspace_bytes >= lpm_triangulation_mean_workspace_bytes(2, B, T, D, K), LPM_ERR_WORKSPACE,
                "%s: workspace too small", name);
    LPM_REQUIRE((((uintptr_t)x | (uintptr_t)dx | (uintptr_t)g_t | (uintptr_t)workspace) & 15) == 0, LPM_ERR_BADARG,
                "%s: x, dx, g_t and the workspace must be 16-byte aligned", name);
    const int G = ta_groups(B, K);
    LPM_REQUIRE((int64_t)B * G < (1ll << 31), LPM_ERR_UNSUPPORTED_SHAPE, "%s: batch too large (B=%d)", name, B);
    float* da_part = (float*)workspace;
    float* dx_part = G > 1 ? da_part + (size_t)B * K * D : dx;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(B * G), block(64 * TA_WAVES);
    const size_t lds = tm_bwd_lds(T);
    if (const int rc = tp_reserve_lds<tm_bwd_kernel<1024, 0>, tm_bwd_kernel<128, 0>, tm_bwd_kernel<1024, TA_FAST_FRAMES>,
                                      tm_bwd_kernel<128, TA_FAST_FRAMES>>(name, (int)tm_bwd_lds(TA_MAX_FRAMES)))     // (more than the fast form's)
        return rc;
    tp_dispatch_d(D, [&](auto d) {
        constexpr int DD = decltype(d)::value;
        auto* kernel = T <= TA_FAST_FRAMES ? tm_bwd_kernel<DD, TA_FAST_FRAMES> : tm_bwd_kernel<DD, 0>;
        hipLaunchKernelGGL(kernel, grid, block, lds, s, x, anchors, w_d, m_d, g_d, g_t, T, K, scale, G, dx_part, da_part);
    });
    if (const int rc = ta_reduce_partials(dx_part, da_part, B, T, D, K, G, TP_SUM_CHUNK, dx, danchors, s, name)) return rc;
    return check_launch(name);
}
