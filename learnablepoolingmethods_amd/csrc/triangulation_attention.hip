// Soft-attention pooling of the triangulation embedding (aggregation_modules.py:74-108 IndirectClusterMaxMeanPoolModule over
// video_pooling_modules' TriangulationEmbedding + TriangulationTemporalEmbedding), fused.  With v = e over the T frames or v = f over
// the T - 1 frame-to-frame differences (e, f exactly as in triangulation_pool.hip -- one walk, triangulation_common.h -- with the same
// clamps and the same first-index maximum; tests/test_gpu_triangulation_family.py holds the two ops' maxima bitwise equal):
//   G[t,s] = <v_t, v_s> over all K*D features;  l[t] = sum_s relu(G[t,s]);  w = softmax_t(l)
//   mean = (1/T') sum_t w[t] v_t;  max = max_t v_t
// Nothing of size T*K*D exists in either direction; the Grams [B,T,T] / [B,T-1,T-1] and the weights [B,T] / [B,T-1] do (the caller
// takes relu, row sums and softmax on them: they are tiny).  No floating-point atomics: every cross-workgroup sum has a fixed order.
// The Gram and the backward's M V products run on v_mfma_f32_32x32x2_f32 -- exact fp32 products, fp32 accumulation: the logits are
// sums of up to T*K terms that enter a softmax, a bf16 / fp16 pass would not do.
//
// lpm_triangulation_attention_gram: a workgroup (4 waves) owns a clip, a pair (I, J) of 64-frame tiles and a slice of the anchors
// (k = slice, slice + S, ...).  Per anchor it takes the two norms of its frames once (ta_norms: one wave per frame),
// then walks D in 32-column chunks: the threads rebuild e and f of the chunk in LDS, each wave adds its 32x32 quadrant of
// V_I V_J^T for both kinds on the matrix cores.  An anchor's product is summed in registers and added onto the slice's total (a
// two-level sum, as the walk's over t); the slices' partial Grams are added s = 0, 1, ... by ta_sum_slices_kernel.
//
// lpm_triangulation_attention_pool_fwd: tp_walk_fwd_kernel<D, w_d, w_t, maxima> (triangulation_common.h).
//
// lpm_triangulation_attention_dw: dw[b,t] = <g_mean, v_t> / T', per (clip, anchor) by tp_walk_dw_kernel<D, temporal>, then over anchors
// k = 0, 1, ....
//
// lpm_triangulation_attention_bwd: with M = dG + dG^T (symmetric, from the caller) the per-frame cotangents of triangulation_pool.hip's
// backward gain one term each:
//   gf_t = w_t[t] g_mean_t / (T-1) + [t = argmax_t] g_max_t + (M_t F_k)[t]     gu_t = ip (gf_t - f_t (f_t . gf_t) [p > 1e-12])
//   ge_t = w_d[t] g_mean_d / T + [t = argmax_d] g_max_d + (M_d E_k)[t] + gu_t - gu_{t+1}
//   gr_t = s iq (ge_t - eh_t (eh_t . ge_t) [q > 1e-12])            dx[b,t,:] = sum_k gr_t      danchors[:,k] = - sum_{b,t} gr_t
// A workgroup owns a clip and the anchors k = g, g + G, ...; per anchor it takes the norms of ALL frames, then walks D in 32-column
// chunks: the chunk's frames go to LDS ([T,33]), the waves form M V on the matrix cores (M's operand is read along its rows: M is
// symmetric; V's operand, e or f of a frame, is computed from the frames tile and the norms on the fly) into two more [T,33] tiles, and
// a thread per (t, column) does the chain above (gu_{t+1} recomputed from row t + 1: no dependence between frames).  The two dot
// products are sums over D, so D is walked three times: (f . gf), then (eh . ge), then gr.  A workgroup adds its anchors onto its own
// [T, D] block in turn; G > 1 groups per clip write partials that a second pass adds g = 0, 1, ...; danchors from per-(clip, anchor)
// sums, clips added b = 0, 1, ... (ta_reduce_partials below: the one pair of reduce kernels of the whole family).
#include "triangulation_common.h"

// the contraction rule (triangulation_common.h) for everything below
#pragma clang fp contract(off)

namespace lpm {

constexpr int TA_MAX_JOBS = (2 * (TA_MAX_FRAMES / 32) + TA_WAVES - 1) / TA_WAVES;    // 32-row tiles of M V per wave and chunk

template <int D>
__global__ __launch_bounds__(64 * TA_WAVES) void ta_gram_kernel(const float* __restrict__ x, const float* __restrict__ anchors, int T, int K,
                                                                float s, int S, int NT, float* __restrict__ part_d,
                                                                float* __restrict__ part_t) {
    constexpr int N = TpVec<D>::N;
    // entry i of the norms belongs to frame f0 - 1 + i: f of a tile's first frame needs e of the frame before it
    __shared__ float nrm[2][2][72];                        // [tile I / J][iq / ip]
    __shared__ float tile[2][2][64][TA_LD];                // [tile I / J][e / f]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int id = blockIdx.x;
    const int tj = id % NT; id /= NT;
    const int ti = id % NT; id /= NT;
    const int sl = id % S, b = id / S;
    const bool diag = ti == tj;
    const int nside = diag ? 1 : 2;
    const float* xb = x + (int64_t)b * T * D;
    const int c = threadIdx.x & 31, r0 = threadIdx.x >> 5;
    const int qi = wave >> 1, qj = wave & 1;
    const float (*tI)[64][TA_LD] = tile[0];
    const float (*tJ)[64][TA_LD] = tile[diag ? 0 : 1];
    f32x16 tot_d, tot_t;
#pragma unroll
    for (int r = 0; r < 16; ++r) tot_d[r] = tot_t[r] = 0.f;
    for (int k = sl; k < K; k += S) {
        {
            float a[N];
            tp_load_anchor<D>(anchors, K, k, lane, a);
            for (int side = 0; side < nside; ++side)
                ta_norms<D, TN_TEMPORAL>(xb, a, nullptr, T, (side ? tj : ti) * 64 - 1, 65, s, nrm[side][0], nullptr, nrm[side][1], nullptr, nullptr);
        }
        __syncthreads();
        f32x16 acc_d, acc_t;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc_d[r] = acc_t[r] = 0.f;
        for (int c0 = 0; c0 < D; c0 += TA_CH) {
            const float av = anchors[(int64_t)(c0 + c) * K + k];
            for (int side = 0; side < nside; ++side) {
                const int f0 = (side ? tj : ti) * 64;
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const int r = r0 + 8 * i, t = f0 + r;
                    float e = 0.f, f = 0.f;
                    if (t < T) {
                        e = ta_eh(xb[(int64_t)t * D + c0 + c], av, nrm[side][0][r + 1]) * s;
                        if (t >= 1) {
                            const float ep = ta_eh(xb[(int64_t)(t - 1) * D + c0 + c], av, nrm[side][0][r]) * s;
                            f = (e - ep) * nrm[side][1][r + 1];
                        }
                    }
                    tile[side][0][r][c] = e;
                    tile[side][1][r][c] = f;
                }
            }
            __syncthreads();
#pragma unroll
            for (int kk = 0; kk < TA_CH; kk += 2) {
                const int col = kk + (lane >> 5), ra = 32 * qi + (lane & 31), rb = 32 * qj + (lane & 31);
                acc_d = mfma32(tI[0][ra][col], tJ[0][rb][col], acc_d);
                acc_t = mfma32(tI[1][ra][col], tJ[1][rb][col], acc_t);
            }
            __syncthreads();
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            tot_d[r] += acc_d[r];
            tot_t[r] += acc_t[r];
        }
    }
    const int T1 = T - 1;
    float* od = part_d + ((int64_t)b * S + sl) * T * T;
    float* ot = part_t + ((int64_t)b * S + sl) * T1 * T1;
    const int u = tj * 64 + 32 * qj + (lane & 31);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int t = ti * 64 + 32 * qi + mfma32_row(r, lane);
        if (t < T && u < T) {
            od[(int64_t)t * T + u] = tot_d[r];
            if (t >= 1 && u >= 1) ot[(int64_t)(t - 1) * T1 + (u - 1)] = tot_t[r];
        }
    }
}

// out[o][i] = sum_s part[o][s][i], s = 0, 1, ...
__global__ __launch_bounds__(256) void ta_sum_slices_kernel(const float* __restrict__ part, int64_t total, int64_t n, int S,
                                                            float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int64_t o = i / n, r = i % n;
    const float* p = part + o * S * n + r;
    float acc = p[0];
    for (int sl = 1; sl < S; ++sl) acc += p[(int64_t)sl * n];
    out[i] = acc;
}

// f[t, c] as ta_e: 0 for t = 0 and t >= T (ip = 0 there)
__device__ __forceinline__ float ta_f(const float (*tX)[TA_LD], const float* iq, const float* ip, int t, int c, float av, float s) {
    return (ta_e(tX, iq, t, c, av, s) - ta_e(tX, iq, max(t - 1, 0), c, av, s)) * ip[t];
}

// TP = 64: T <= 64 (the model's default), every loop over the frames unrolled, M_d and M_t of the clip in LDS, one 32-row tile of M V per
// wave; TP = 0: any T <= TA_MAX_FRAMES, M from global memory (L2), up to TA_MAX_JOBS tiles per wave.
template <int D, int TP>
__global__ __launch_bounds__(64 * TA_WAVES) void ta_bwd_kernel(const float* __restrict__ x, const float* __restrict__ anchors,
                                                               const int* __restrict__ argmax, const float* __restrict__ w_d,
                                                               const float* __restrict__ w_t, const float* __restrict__ m_d,
                                                               const float* __restrict__ m_t, const float* __restrict__ g_mean_d,
                                                               const float* __restrict__ g_max_d, const float* __restrict__ g_mean_t,
                                                               const float* __restrict__ g_max_t, int T, int K, float s, int G,
                                                               float* __restrict__ dx_part, float* __restrict__ da_part) {
    constexpr int N = TpVec<D>::N, MAXJ = TP ? (2 * (TP / 32) + TA_WAVES - 1) / TA_WAVES : TA_MAX_JOBS;
    constexpr int UNR = TP ? TP / 8 : 1;                   // a thread's frames: loops unrolled and loads issued early when their count is known
    // LDS: the frames of one chunk of D for all t ([Tp][33]), (M_d E)[t] and (M_t F)[t] of the chunk (the same shape), the frames' norms
    // and gates, the two dot products per frame, the clip's weights by frame index, the eight row groups' column sums for danchors,
    // and (TP) M_d and M_t by frame index
    extern __shared__ __attribute__((aligned(16))) float ta_sh[];
    const int Tp = TP ? TP : ((T + 31) & ~31), T1 = T - 1, ntt = Tp / 32;
    float (*tX)[TA_LD] = reinterpret_cast<float (*)[TA_LD]>(ta_sh);
    float (*tPd)[TA_LD] = tX + Tp;
    float (*tPt)[TA_LD] = tPd + Tp;
    float* iq = ta_sh + 3 * Tp * TA_LD;
    float *qg = iq + Tp, *ip = qg + Tp, *pg = ip + Tp, *dotf = pg + Tp, *dote = dotf + Tp, *wdl = dote + Tp, *wtl = wdl + Tp, *dacc = wtl + Tp;
    float *mD = dacc + 8 * 32, *mT = mD + TP * TP;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = threadIdx.x & 31, r0 = threadIdx.x >> 5;           // (c is lane & 31 as well: the column of the MFMA operands)
    const int b = blockIdx.x / G, g = blockIdx.x % G;
    const float* xb = x + (int64_t)b * T * D;
    float* dxo = dx_part + ((int64_t)b * G + g) * T * D;   // this workgroup's own [T, D] block (dx itself when G == 1)
    const float* md = m_d + (int64_t)b * T * T;
    const float* mt = m_t + (int64_t)b * T1 * T1;
    const float inv_d = 1.f / (float)T, inv_t = 1.f / (float)T1;
    for (int t = threadIdx.x; t < Tp; t += 64 * TA_WAVES) {
        wdl[t] = t < T ? w_d[(int64_t)b * T + t] : 0.f;
        wtl[t] = (t >= 1 && t < T) ? w_t[(int64_t)b * T1 + t - 1] : 0.f;
    }
    // the frames of the NEXT chunk are loaded while the current one is worked on (they depend on neither the anchor nor the sweep)
    float xr[UNR], dxold[UNR];
    if (TP) {
#pragma unroll
        for (int i = 0; i < UNR; ++i) xr[i] = r0 + 8 * i < T ? xb[(int64_t)(r0 + 8 * i) * D + c] : 0.f;
    }
    if (TP) {                                              // entry [s][t] by FRAME index; zero outside the frames (and for frame 0 of M_t)
        for (int i = threadIdx.x; i < TP * TP; i += 64 * TA_WAVES) {
            const int sr = i / (TP ? TP : 1), tc = i % (TP ? TP : 1);
            const bool in = sr < T && tc < T;
            mD[i] = in ? md[(int64_t)sr * T + tc] : 0.f;
            mT[i] = (in && sr >= 1 && tc >= 1) ? mt[(int64_t)(sr - 1) * T1 + (tc - 1)] : 0.f;
        }
    }
    for (int k = g; k < K; k += G) {
        const bool first = k == g;
        {
            float a[N];
            tp_load_anchor<D>(anchors, K, k, lane, a);
            ta_norms<D, TN_TEMPORAL | TN_GATES>(xb, a, nullptr, T, 0, Tp, s, iq, qg, ip, pg, nullptr);
        }
        for (int t = threadIdx.x; t < Tp; t += 64 * TA_WAVES) dotf[t] = dote[t] = 0.f;
        __syncthreads();
        const int64_t o = ((int64_t)b * K + k) * D;
        for (int sweep = 1; sweep <= 3; ++sweep) {
            const int njobs = sweep == 1 ? ntt : 2 * ntt;  // jobs 0 .. ntt-1: M_t F (every sweep); ntt .. 2 ntt - 1: M_d E
            for (int c0 = 0; c0 < D; c0 += TA_CH) {
                const float av = anchors[(int64_t)(c0 + c) * K + k];
                if (TP) {
#pragma unroll
                    for (int i = 0; i < UNR; ++i) tX[r0 + 8 * i][c] = xr[i];
                } else {
                    for (int t = r0; t < Tp; t += 8) tX[t][c] = t < T ? xb[(int64_t)t * D + c0 + c] : 0.f;
                }
                __syncthreads();
                // (issued here, used behind the matrix products)
                const float gmd = g_mean_d[o + c0 + c] * inv_d, gxd = g_max_d[o + c0 + c];
                const float gmt = g_mean_t[o + c0 + c] * inv_t, gxt = g_max_t[o + c0 + c];
                const int idx = argmax[o + c0 + c], id_d = idx & 0xffff, id_t = (idx >> 16) & 0xffff;
                if (TP) {
                    const int cn = (c0 + TA_CH) % D + c;
#pragma unroll
                    for (int i = 0; i < UNR; ++i) {
                        const int t = r0 + 8 * i;
                        xr[i] = t < T ? xb[(int64_t)t * D + cn] : 0.f;
                        dxold[i] = (sweep == 3 && !first && t < T) ? dxo[(int64_t)t * D + c0 + c] : 0.f;
                    }
                }
#pragma unroll
                for (int ji = 0; ji < MAXJ; ++ji) {
                    const int j = wave + TA_WAVES * ji;
                    if (j < njobs) {                       // (wave-uniform)
                        const bool kd = j >= ntt;
                        const int t0 = 32 * (kd ? j - ntt : j);
                        f32x16 ac;
#pragma unroll
                        for (int r = 0; r < 16; ++r) ac[r] = 0.f;
                        // A[t][s] = M[t][s] = M[s][t]: read along M's rows.  B[s][c] = e or f of frame s, from the frames in LDS
                        if (TP) {
                            const float* m = (kd ? mD : mT) + t0 + c;
#pragma unroll 8
                            for (int s2 = 0; s2 < TP; s2 += 2) {
                                const int srow = s2 + (lane >> 5);
                                const float bv = kd ? ta_e(tX, iq, srow, c, av, s) : ta_f(tX, iq, ip, srow, c, av, s);
                                ac = mfma32(m[srow * TP], bv, ac);
                            }
                        } else {
                            const int off = kd ? 0 : 1, Tk = T - off, tcol = t0 + c - off;
                            const float* m = kd ? md : mt;
                            const bool tok = tcol >= 0 && tcol < Tk;
                            for (int s2 = 0; s2 < Tp; s2 += 2) {
                                const int srow = s2 + (lane >> 5), sr = srow - off;
                                const float mv = (tok && sr >= 0 && sr < Tk) ? m[(int64_t)sr * Tk + tcol] : 0.f;
                                const float bv = kd ? ta_e(tX, iq, srow, c, av, s) : ta_f(tX, iq, ip, srow, c, av, s);
                                ac = mfma32(mv, bv, ac);
                            }
                        }
                        float (*tile)[TA_LD] = kd ? tPd : tPt;
#pragma unroll
                        for (int r = 0; r < 16; ++r) tile[t0 + mfma32_row(r, lane)][c] = ac[r];
                    }
                }
                __syncthreads();
                // tPt[t] = (M_t F)[t], tPd[t] = (M_d E)[t] (sweeps 2, 3) for this chunk; one thread per (t, column)
                float da = 0.f;
#pragma unroll UNR
                for (int i = 0; i < Tp / 8; ++i) {
                    const int t = r0 + 8 * i;
                    const bool valid = t < T;
                    float v = 0.f;
                    if (valid) {
                        const float eh = ta_eh(tX[t][c], av, iq[t]), e = eh * s;
                        float f = 0.f, gf = 0.f;
                        if (t >= 1) {
                            f = (e - ta_e(tX, iq, t - 1, c, av, s)) * ip[t];
                            gf = wtl[t] * gmt + (id_t == t ? gxt : 0.f) + tPt[t][c];
                        }
                        if (sweep == 1) {
                            v = f * gf;
                        } else {
                            float gu = 0.f, gun = 0.f;
                            if (t >= 1) gu = ip[t] * (gf - f * (dotf[t] * pg[t]));
                            if (t + 1 < T) {
                                const float fn = (ta_e(tX, iq, t + 1, c, av, s) - e) * ip[t + 1];
                                const float gfn = wtl[t + 1] * gmt + (id_t == t + 1 ? gxt : 0.f) + tPt[t + 1][c];
                                gun = ip[t + 1] * (gfn - fn * (dotf[t + 1] * pg[t + 1]));
                            }
                            const float ge = wdl[t] * gmd + (id_d == t ? gxd : 0.f) + tPd[t][c] + gu - gun;
                            if (sweep == 2) {
                                v = eh * ge;
                            } else {
                                const float gr = (s * iq[t]) * (ge - eh * (dote[t] * qg[t]));
                                float* po = dxo + (int64_t)t * D + c0 + c;
                                // an earlier anchor of this workgroup: this thread wrote it
                                *po = first ? gr : (TP ? dxold[TP ? i : 0] : *po) + gr;
                                da += gr;
                            }
                        }
                    }
                    if (sweep < 3) {
                        // the 32 columns of the chunk: one half-wave per frame.  (The shuffle form: half_sum_dpp adds in another order,
                        // which would change this kernel's bits.)
                        v = half_sum(v);
                        if (c == 0 && valid) (sweep == 1 ? dotf : dote)[t] += v;
                    }
                }
                if (sweep == 3) {
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

// dx[b] = sum_g dx_part[b][g], g = 0, 1, ... (n4 = T * D / 4 float4 per block)
__global__ __launch_bounds__(256) void tp_dx_reduce_kernel(const float4* __restrict__ part, int64_t total4, int64_t n4, int G,
                                                           float4* __restrict__ dx) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total4) return;
    const int64_t b = i / n4, r = i % n4;
    const float4* p = part + b * G * n4 + r;
    float4 acc = p[0];
    for (int g = 1; g < G; ++g) {
        const float4 v = p[(int64_t)g * n4];
        acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
    dx[i] = acc;
}

// danchors[d][k] = - sum_b da_part[b][k][d], b = 0, 1, ... (two-level: `chunk` clips into a partial, partials into the total; every
// partial starts from +0 and 0 + acc is exact, so chunk >= B gives the bits of a plain loop over the clips)
__global__ __launch_bounds__(256) void tp_da_reduce_kernel(const float* __restrict__ part, int B, int K, int D, int chunk,
                                                           float* __restrict__ danchors) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= K * D) return;
    const int k = i / D, d = i % D;
    float tot = 0.f;
    for (int b0 = 0; b0 < B; b0 += chunk) {
        float acc = 0.f;
        for (int b = b0; b < min(b0 + chunk, B); ++b) acc += part[(int64_t)b * K * D + i];
        tot += acc;
    }
    danchors[(int64_t)d * K + k] = -tot;
}

static int ta_slices(int B, int T, int K) {
    const int64_t wg = (int64_t)B * ta_tiles(T) * ta_tiles(T);
    int64_t want = (512 + wg - 1) / wg;
    want = want < 1 ? 1 : (want > TA_MAX_SLICES ? TA_MAX_SLICES : want);
    return (int)(K < want ? K : want);
}
static size_t ta_bwd_lds(int T) {
    const bool fast = T <= TA_FAST_FRAMES;
    const int Tp = fast ? TA_FAST_FRAMES : (T + 31) & ~31;
    return ((size_t)3 * Tp * TA_LD + 8 * Tp + 8 * 32 + (fast ? 2 * TA_FAST_FRAMES * TA_FAST_FRAMES : 0)) * sizeof(float);
}

int ta_sum_slices(const float* part, int64_t outer, int64_t n, int S, float* out, hipStream_t s, const char* name) {
    const int64_t total = outer * n;
    LPM_REQUIRE((total + 255) / 256 < (1ll << 31), LPM_ERR_UNSUPPORTED_SHAPE, "%s: too large", name);
    hipLaunchKernelGGL(ta_sum_slices_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, part, total, n, S, out);
    return LPM_OK;
}

int ta_reduce_partials(const float* dx_part, const float* da_part, int B, int T, int D, int K, int G, int da_chunk, float* dx,
                       float* danchors, hipStream_t s, const char* name) {
    if (G > 1) {
        const int64_t n4 = (int64_t)T * D / 4, total4 = n4 * B;
        LPM_REQUIRE((total4 + 255) / 256 < (1ll << 31), LPM_ERR_UNSUPPORTED_SHAPE, "%s: B * T * D too large", name);
        hipLaunchKernelGGL(tp_dx_reduce_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, s, (const float4*)dx_part, total4, n4, G,
                           (float4*)dx);
    }
    hipLaunchKernelGGL(tp_da_reduce_kernel, dim3((K * D + 255) / 256), dim3(256), 0, s, da_part, B, K, D, da_chunk, danchors);
    return LPM_OK;
}

}  // namespace lpm

extern "C" int lpm_triangulation_attention_max_frames(void) { return lpm::TA_MAX_FRAMES; }

extern "C" size_t lpm_triangulation_attention_workspace_bytes(int which, int B, int T, int D, int K) {
    if (B <= 0 || T <= 1 || D <= 0 || K <= 0) return 0;
    const size_t T1 = (size_t)T - 1;
    if (which == 0) {                                       // gram: the slices' partial Grams
        const int S = lpm::ta_slices(B, T, K);
        return S > 1 ? (size_t)B * S * ((size_t)T * T + T1 * T1) * sizeof(float) : 0;
    }
    if (which == 1) return (size_t)B * K * ((size_t)T + T1) * sizeof(float);      // dw: per-(clip, anchor) dot products
    const int G = lpm::ta_groups(B, K);                     // bwd: danchors partials, dx partials
    return ((size_t)B * K * D + (G > 1 ? (size_t)B * G * T * D : 0)) * sizeof(float);
}

extern "C" int lpm_triangulation_attention_gram(const float* x, const float* anchors, int B, int T, int D, int K, float scale, float* gram_d,
                                                float* gram_t, void* workspace, size_t workspace_bytes, lpm_stream_t stream) {
    using namespace lpm;
    const char* name = "lpm_triangulation_attention_gram";
    LPM_REQUIRE(x && anchors && gram_d && gram_t, LPM_ERR_BADARG, "%s: null pointer", name);
    if (const int rc = ta_check(name, B, T, D, K)) return rc;
    const size_t need = lpm_triangulation_attention_workspace_bytes(0, B, T, D, K);
    LPM_REQUIRE(need == 0 || (workspace && workspace_bytes >= need), LPM_ERR_WORKSPACE, "%s: workspace too small", name);
    LPM_REQUIRE(((uintptr_t)x & 15) == 0, LPM_ERR_BADARG, "%s: x must be 16-byte aligned", name);
    const int S = ta_slices(B, T, K), NT = ta_tiles(T), T1 = T - 1;
    float* part_d = S > 1 ? (float*)workspace : gram_d;
    float* part_t = S > 1 ? part_d + (size_t)B * S * T * T : gram_t;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)(B * S * NT * NT)), block(64 * TA_WAVES);
    tp_dispatch_d(D, [&](auto d) {
        hipLaunchKernelGGL(ta_gram_kernel<decltype(d)::value>, grid, block, 0, s, x, anchors, T, K, scale, S, NT, part_d, part_t);
    });
    if (S > 1) {
        if (const int rc = ta_sum_slices(part_d, B, (int64_t)T * T, S, gram_d, s, name)) return rc;
        if (const int rc = ta_sum_slices(part_t, B, (int64_t)T1 * T1, S, gram_t, s, name)) return rc;
    }
    return check_launch(name);
}

extern "C" int lpm_triangulation_attention_pool_fwd(const float* x, const float* anchors, const float* w_d, const float* w_t, int B, int T,
                                                    int D, int K, float scale, float* mean_d, float* max_d, float* mean_t, float* max_t,
                                                    int32_t* argmax, lpm_stream_t stream) {
    using namespace lpm;
    const char* name = "lpm_triangulation_attention_pool_fwd";
    LPM_REQUIRE(x && anchors && w_d && w_t && mean_d && max_d && mean_t && max_t && argmax, LPM_ERR_BADARG, "%s: null pointer", name);
    if (const int rc = ta_check(name, B, T, D, K)) return rc;
    LPM_REQUIRE((((uintptr_t)x | (uintptr_t)max_d | (uintptr_t)mean_d | (uintptr_t)max_t | (uintptr_t)mean_t | (uintptr_t)argmax) & 15) == 0,
                LPM_ERR_BADARG, "%s: x and the outputs must be 16-byte aligned", name);
    tp_dispatch_d(D, [&](auto d) {
        hipLaunchKernelGGL((tp_walk_fwd_kernel<decltype(d)::value, true, true, true>), dim3(tp_walk_grid(B, K)), dim3(64 * TP_WALK_WAVES), 0,
                           (hipStream_t)stream, x, anchors, w_d, w_t, T, K, scale, mean_d, max_d, mean_t, max_t, argmax);
    });
    return check_launch(name);
}

extern "C" int lpm_triangulation_attention_dw(const float* x, const float* anchors, const float* g_mean_d, const float* g_mean_t, int B, int T,
                                              int D, int K, float scale, float* dw_d, float* dw_t, void* workspace, size_t workspace_bytes,
                                              lpm_stream_t stream) {
    using namespace lpm;
    const char* name = "lpm_triangulation_attention_dw";
    LPM_REQUIRE(x && anchors && g_mean_d && g_mean_t && dw_d && dw_t, LPM_ERR_BADARG, "%s: null pointer", name);
    if (const int rc = ta_check(name, B, T, D, K)) return rc;
    LPM_REQUIRE(workspace && workspace_bytes >= lpm_triangulation_attention_workspace_bytes(1, B, T, D, K), LPM_ERR_WORKSPACE,
                "%s: workspace too small", name);
    LPM_REQUIRE((((uintptr_t)x | (uintptr_t)g_mean_d | (uintptr_t)g_mean_t) & 15) == 0, LPM_ERR_BADARG,
                "%s: x and the gradients must be 16-byte aligned", name);
    float* part_d = (float*)workspace;
    float* part_t = part_d + (size_t)B * K * T;
    hipStream_t s = (hipStream_t)stream;
    tp_dispatch_d(D, [&](auto d) {
        hipLaunchKernelGGL((tp_walk_dw_kernel<decltype(d)::value, true>), dim3(tp_walk_grid(B, K)), dim3(64 * TP_WALK_WAVES), 0, s, x, anchors,
                           g_mean_d, T, K, scale, part_d, g_mean_t, part_t);
    });
    if (const int rc = ta_sum_slices(part_d, B, T, K, dw_d, s, name)) return rc;
    if (const int rc = ta_sum_slices(part_t, B, T - 1, K, dw_t, s, name)) return rc;
    return check_launch(name);
}

extern "C" int lpm_triangulation_attention_bwd(const float* x, const float* anchors, const int32_t* argmax, const float* w_d, const float* w_t,
                                               const float* m_d, const float* m_t, const float* g_mean_d, const float* g_max_d,
                                               const float* g_mean_t, const float* g_max_t, int B, int T, int D, int K, float scale, float* dx,
                                               float* danchors, void* workspace, size_t workspace_bytes, lpm_stream_t stream) {
    using namespace lpm;
    const char* name = "lpm_triangulation_attention_bwd";
    LPM_REQUIRE(x && anchors && argmax && w_d && w_t && m_d && m_t && g_mean_d && g_max_d && g_mean_t && g_max_t && dx && danchors,
                LPM_ERR_BADARG, "%s: null pointer", name);
    if (const int rc = ta_check(name, B, T, D, K)) return rc;
    LPM_REQUIRE(workspace && workspace_bytes >= lpm_triangulation_attention_workspace_bytes(2, B, T, D, K), LPM_ERR_WORKSPACE,
                "%s: workspace too small", name);
    LPM_REQUIRE((((uintptr_t)x | (uintptr_t)dx | (uintptr_t)workspace) & 15) == 0, LPM_ERR_BADARG,
                "%s: x, dx and the workspace must be 16-byte aligned", name);
    const int G = ta_groups(B, K);
    LPM_REQUIRE((int64_t)B * G < (1ll << 31), LPM_ERR_UNSUPPORTED_SHAPE, "%s: batch too large (B=%d)", name, B);
    float* da_part = (float*)workspace;
    float* dx_part = G > 1 ? da_part + (size_t)B * K * D : dx;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(B * G), block(64 * TA_WAVES);
    const size_t lds = ta_bwd_lds(T);
    if (const int rc = tp_reserve_lds<ta_bwd_kernel<1024, 0>, ta_bwd_kernel<128, 0>, ta_bwd_kernel<1024, TA_FAST_FRAMES>,
                                      ta_bwd_kernel<128, TA_FAST_FRAMES>>(name, (int)ta_bwd_lds(TA_MAX_FRAMES)))     // (more than the fast form's)
        return rc;
    tp_dispatch_d(D, [&](auto d) {
        constexpr int DD = decltype(d)::value;
        auto* kernel = T <= TA_FAST_FRAMES ? ta_bwd_kernel<DD, TA_FAST_FRAMES> : ta_bwd_kernel<DD, 0>;
        hipLaunchKernelGGL(kernel, grid, block, lds, s, x, anchors, argmax, w_d, w_t, m_d, m_t, g_mean_d, g_max_d, g_mean_t, g_max_t, T, K, scale,
                           G, dx_part, da_part);
    });
    if (const int rc = ta_reduce_partials(dx_part, da_part, B, T, D, K, G, TP_SUM_CHUNK, dx, danchors, s, name)) return rc;
    return check_launch(name);
}
