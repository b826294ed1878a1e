// a2 + a3 -- SampleUniformFrames fused with the input batch-norm.
//   idx[b,j] = int32(fp32(j * fp32(1/S)) * fp32(num_frames[b]))      model_utils.py:112-118
//   y[b*S+j, :] = raw[b, idx[b,j], :] * scale + shift                 model_utils.py:119-122 +
//                                                                      frame_level_models.py:2265-2271
// The gathered [B,S,F] tensor is never materialised un-normalised: one pass reduces the column
// statistics of the gathered rows (per-block partials -> lpm_frame_bn_fold), a second pass gathers again
// and writes the normalised rows that K1 and K2 consume.  Both are pure HBM streams (float4,
// row-contiguous 4.6 KB reads).
// Eval mode from the reader's quantised frames (the *_q8 entry points): the apply kernels read the uint8 frames of the sampled
// rows and one inverse L2 norm per sampled row (lpm_frame_inv_norm_q8), and produce bit for bit what they produce from
// lpm_dequantize_l2_normalize's fp32 frames -- without writing (and re-reading) the fp32 frames of all max_frames.
// Training mode from the quantised frames (lpm_frame_stats_q8, lpm_frame_bn_bwd*_q8): the statistics and the dgamma / dbeta partial
// kernels are templated on the same source.  A thread of the uint8 form owns FOUR adjacent columns (one uchar4 load per row; a byte
// load per lane would use a quarter of each 64-byte request) with one accumulator pair per column, so every column still sums the rows
// of its 32-row block in order, s += v, q = fma(v, v, q) -- the partials are bit for bit those of the fp32 form on the fp32 frames.
#include "lpm_common.h"

namespace lpm {

constexpr int FP_ROWS = 32;  // gathered rows per statistics block

__device__ __forceinline__ int sample_index(int j, float step, int nf) {
    // fp32 product then truncation toward zero, exactly as tf.linspace * num_frames -> tf.cast(int32)
    const float v = __fmul_rn((float)j, step);
    return (int)__fmul_rn(fminf(v, 1.0f), (float)nf);
}

// Which frame of clip b the sampled row r = b S + j reads (before the clamp to [0, max_frames - 1], which every kernel applies itself).
// UniformIdx: SampleUniformFrames' formula.  TableIdx: a frame_index table int32 [B S] the caller drew (SampleRandomFrames: model_utils.
// random_frame_index) -- the *_idx entry points; one 4-byte read per row, the frame rows themselves are still gathered whole.
struct UniformIdx {
    const int32_t* __restrict__ num_frames;
    float step;
    __device__ __forceinline__ int operator()(int b, int j, int64_t) const { return sample_index(j, step, num_frames[b]); }
};
struct TableIdx {
    const int32_t* __restrict__ table;
    __device__ __forceinline__ int operator()(int, int, int64_t r) const { return table[r]; }
};

// One wave's share of a quantised frame row (lane owns the uchar4 columns lane + 64 i, F <= 2048): the dequantised values
// (utils.Dequantize: u * range/255 + range/512 + min) into v, and the row's inverse L2 norm rsqrt(max(sum x^2, 1e-12)).
// dequantize_l2_normalize_kernel and frame_inv_norm_q8_kernel both use it: one summation order, one rounding.
__device__ __forceinline__ float dequant_row_inv_norm(const uchar4* __restrict__ src, int lane, int F4, float scalar, float bias,
                                                      float4 (&v)[8]) {
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int c = lane + 64 * i;
        v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c < F4) {
            const uchar4 u = src[c];
            v[i] = make_float4(fmaf((float)u.x, scalar, bias), fmaf((float)u.y, scalar, bias), fmaf((float)u.z, scalar, bias),
                               fmaf((float)u.w, scalar, bias));
        }
        ss += v[i].x * v[i].x + v[i].y * v[i].y + v[i].z * v[i].z + v[i].w * v[i].w;
    }
    ss = wave_sum(ss);
    return rsqrtf(fmaxf(ss, 1e-12f));
}

// Where the apply kernels read the sampled frames.  FrameSrc<float>: the fp32 batch [B, max_frames, F].  FrameSrc<unsigned char>:
// the reader's uint8 batch plus one inverse norm per SAMPLED row (lpm_frame_inv_norm_q8; 0 marks a frame at or past num_frames,
// which the reader pads with zeros) -- each value is dequantised and rounded to fp32 times the inverse norm, exactly the value
// lpm_dequantize_l2_normalize stores, before the kernel's own arithmetic.  load4: four consecutive features at element offset off
// of sampled row `row` (= b S + j).
template <typename T>
struct FrameSrc;
template <>
struct FrameSrc<float> {
    const float* __restrict__ raw;
    __device__ __forceinline__ float4 load4(int64_t off, int64_t) const { return *reinterpret_cast<const float4*>(raw + off); }
    // the column-partial kernels: W adjacent columns per thread
    static constexpr int W = 1;
    __device__ __forceinline__ void loadw(int64_t off, int64_t, float (&v)[1]) const { v[0] = raw[off]; }
};
template <>
struct FrameSrc<unsigned char> {
    const unsigned char* __restrict__ raw;
    const float* __restrict__ inv;
    float scalar, bias;
    __device__ __forceinline__ float4 load4(int64_t off, int64_t row) const {
        const float s = inv[row];
        if (s == 0.f) return make_float4(0.f, 0.f, 0.f, 0.f);
        const uchar4 u = *reinterpret_cast<const uchar4*>(raw + off);
        return make_float4(__fmul_rn(fmaf((float)u.x, scalar, bias), s), __fmul_rn(fmaf((float)u.y, scalar, bias), s),
                           __fmul_rn(fmaf((float)u.z, scalar, bias), s), __fmul_rn(fmaf((float)u.w, scalar, bias), s));
    }
    static constexpr int W = 4;
    __device__ __forceinline__ void loadw(int64_t off, int64_t row, float (&v)[4]) const {
        const float4 f = load4(off, row);
        v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
    }
};

// W consecutive floats at p (W = 4: p 16-byte aligned)
template <int W>
__device__ __forceinline__ void loadw_f32(const float* __restrict__ p, float (&v)[W]) {
    if constexpr (W == 4) {
        const float4 f = *reinterpret_cast<const float4*>(p);
        v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
    } else {
#pragma unroll
        for (int k = 0; k < W; ++k) v[k] = p[k];
    }
}
template <int W>
__device__ __forceinline__ void storew_f32(float* __restrict__ p, const float (&v)[W]) {
    if constexpr (W == 4) {
        *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int k = 0; k < W; ++k) p[k] = v[k];
    }
}

// Column statistics of the gathered rows: per 32-row block the raw sums (s, q) = (sum v, sum v^2) -> partial [nblk][2][F], and beside them,
// in the same pass, the sums of (v - K) and (v - K)^2 -> shifted [nblk][2][F], pivot [F] (then bn_fold_kernel, bn.hip, which says why: the
// raw fold var = q/n - mean^2 loses eps32 (mean/std)^2 of the variance -- measured at mean/std = 30: batch_var 100 .. 360 times the bound of
// tests/test_gpu_frame_prep_bounds.py, a quantised feature at 200 +- 3 levels 6 .. 15 times).  The raw sums keep their operations, their
// order and their layout; the fold takes them wherever 4 mean^2 <= var, bit for bit as before the shifted sums existed.
// K = the column's mean over FP_PIVOT_ROWS gathered rows spread evenly over ALL B S rows, row (u rows) / p for u < p = min(rows, 8), summed
// in that order: every workgroup forms it itself (eight rows, in L2 after the first workgroup) and gets the same bits -- no pass, no launch,
// nothing exchanged.  Spread over the batch, not the first eight rows: those are rows of ONE clip whenever S >= 8, and frames of one clip
// lie close together (emulated on the CPU, tests/test_frame_prep_ref_host.py: the first eight rows leave batch_var at up to 1.9 of its
// bound, row 0 alone at up to 3.1, the spread rows at 0.32).
constexpr int FP_PIVOT_ROWS = 8;
template <typename Src, typename Idx>
__global__ __launch_bounds__(256) void frame_stats_kernel(Src raw, Idx ix, int B, int max_frames, int F, int S,
                                                          float* __restrict__ partial, float* __restrict__ shifted,
                                                          float* __restrict__ pivot) {
    constexpr int W = Src::W;
    const int r0 = blockIdx.x * FP_ROWS;
    const int rows = B * S;
    const int r1 = min(rows, r0 + FP_ROWS);
    const int pr = min(rows, FP_PIVOT_ROWS);
    __shared__ int64_t base[FP_ROWS];
    __shared__ int64_t pbase[FP_PIVOT_ROWS];
    __shared__ int prow[FP_PIVOT_ROWS];
    if (threadIdx.x < FP_ROWS) {
        const int r = r0 + threadIdx.x;
        if (r < rows) {
            const int b = r / S, j = r % S;
            const int idx = max(0, min(ix(b, j, r), max_frames - 1));
            base[threadIdx.x] = ((int64_t)b * max_frames + idx) * F;
        }
    } else if (threadIdx.x >= 64 && threadIdx.x < 64 + pr) {        // (the second wave)
        const int u = threadIdx.x - 64;
        const int r = (int)(((int64_t)u * rows) / pr);              // < rows
        const int b = r / S, j = r % S;
        const int idx = max(0, min(ix(b, j, r), max_frames - 1));
        pbase[u] = ((int64_t)b * max_frames + idx) * F;
        prow[u] = r;
    }
    __syncthreads();
    const float inv_pr = 1.f / (float)pr;
    for (int c = threadIdx.x * W; c < F; c += 256 * W) {
        float s[W], q[W], ss[W], sq[W], K[W];
#pragma unroll
        for (int k = 0; k < W; ++k) s[k] = q[k] = ss[k] = sq[k] = K[k] = 0.f;
        for (int u = 0; u < pr; ++u) {
            float v[W];
            raw.loadw(pbase[u] + c, prow[u], v);
#pragma unroll
            for (int k = 0; k < W; ++k) K[k] += v[k];
        }
#pragma unroll
        for (int k = 0; k < W; ++k) K[k] *= inv_pr;
        for (int r = 0; r < r1 - r0; ++r) {
            float v[W];
            raw.loadw(base[r] + c, r0 + r, v);
#pragma unroll
            for (int k = 0; k < W; ++k) {
                s[k] += v[k];
                q[k] = fmaf(v[k], v[k], q[k]);
                const float d = v[k] - K[k];
                ss[k] += d;
                sq[k] = fmaf(d, d, sq[k]);
            }
        }
        float* p = partial + (int64_t)blockIdx.x * 2 * F;
        storew_f32<W>(p + c, s);
        storew_f32<W>(p + F + c, q);
        float* ps = shifted + (int64_t)blockIdx.x * 2 * F;
        storew_f32<W>(ps + c, ss);
        storew_f32<W>(ps + F + c, sq);
        if (blockIdx.x == 0) storew_f32<W>(pivot + c, K);
    }
}

// y2 != null: the column blocks [0, Dv) and [Dv, F) leave as TWO contiguous matrices, y [B S, Dv] and y2 [B S, F - Dv]
template <typename Src, typename Idx>
__global__ __launch_bounds__(256) void frame_apply_kernel(Src raw, Idx ix, int B, int max_frames, int F, int S,
                                                          const float* __restrict__ scale,
                                                          const float* __restrict__ shift, float* __restrict__ y,
                                                          float* __restrict__ y2, int Dv, const float* __restrict__ centre) {
    // centre != null: y = (v - centre) * scale + shift.  lpm_frame_bn_fold leaves centre = the column's fp32 mean where it took the shifted
    // sums (4 mean^2 > var), eval mode (ops.frame_eval_affine) where moving_mean^2 > moving_var, and both 0 elsewhere
    // (there v - 0 is v: the bits of the two-vector form): with v - mean formed first, exactly, shift stays of the size of beta and its
    // rounding with it -- v * scale + (beta - mean * scale) carries half an ulp of mean * scale, eps32 (mean/std) of the result.
    const int F4 = F / 4;
    const int64_t total = (int64_t)B * S * F4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int r = (int)(i / F4), c = (int)(i % F4) * 4;
        const int b = r / S, j = r % S;
        const int idx = max(0, min(ix(b, j, r), max_frames - 1));
        float4 v = raw.load4(((int64_t)b * max_frames + idx) * F + c, r);
        if (scale) {
            const float4 sc = *reinterpret_cast<const float4*>(scale + c);
            const float4 sh = *reinterpret_cast<const float4*>(shift + c);
            if (centre) {
                const float4 ce = *reinterpret_cast<const float4*>(centre + c);
                v.x -= ce.x; v.y -= ce.y; v.z -= ce.z; v.w -= ce.w;
            }
            v.x = fmaf(v.x, sc.x, sh.x); v.y = fmaf(v.y, sc.y, sh.y);
            v.z = fmaf(v.z, sc.z, sh.z); v.w = fmaf(v.w, sc.w, sh.w);
        }
        if (!y2) *reinterpret_cast<float4*>(y + (int64_t)r * F + c) = v;
        else if (c < Dv) *reinterpret_cast<float4*>(y + (int64_t)r * Dv + c) = v;
        else *reinterpret_cast<float4*>(y2 + (int64_t)r * (F - Dv) + (c - Dv)) = v;
    }
}

// Same as frame_apply_kernel, but one work item owns 8 consecutive sampled frames of 4 columns so that it can
// ALSO emit the split-bf16 MFMA-fragment tiles K2 consumes (vlad_tiles.hip: XT[b][s][d/32][plane][lane][8]) for
// the rgb columns [0, Dv) and the audio columns [Dv, Dv+Da) -- the normalised frames are then written once in
// fp32 (for K1 / the backward GEMMs) and once in tile order, with no separate re-read for the split.
__device__ __forceinline__ unsigned fp_bf16_rne(float v) {
    unsigned u = __float_as_uint(v);
    u += 0x7fffu + ((u >> 16) & 1u);
    return u >> 16;
}
template <typename Src>
__global__ __launch_bounds__(256) void frame_apply_tiles_kernel(Src raw, const int32_t* __restrict__ num_frames, int B,
                                                                int max_frames, int F, int S, float step,
                                                                const float* __restrict__ scale,
                                                                const float* __restrict__ shift, float* __restrict__ y,
                                                                uint4* __restrict__ xtv, int Dv,
                                                                uint4* __restrict__ xta, int Da, float* __restrict__ y2,
                                                                const float* __restrict__ centre) {
    // y2 != null: the two column blocks leave as TWO contiguous matrices, y [B S, Dv] and y2 [B S, Da] (NetVladV2: each stream's encoder
    // and aggregation want whole rows -- no strided slices, no contiguous copies of them)
    const int F4 = F / 4, NS = (S + 15) / 16;
    const int64_t total = (int64_t)B * NS * 2 * F4;
    for (int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x; w < total; w += (int64_t)gridDim.x * 256) {
        const int c4 = (int)(w % F4);
        const int64_t r = w / F4;
        const int kh = (int)(r & 1), st = (int)((r >> 1) % NS), b = (int)((r >> 1) / NS);
        const int c = 4 * c4;
        float4 sc = make_float4(1.f, 1.f, 1.f, 1.f), sh = make_float4(0.f, 0.f, 0.f, 0.f), ce = sh;
        if (scale) {
            sc = *reinterpret_cast<const float4*>(scale + c);
            sh = *reinterpret_cast<const float4*>(shift + c);
            if (centre) ce = *reinterpret_cast<const float4*>(centre + c);       // (frame_apply_kernel says what it is)
        }
        const int nf = num_frames[b];
        float v[4][8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int j = 16 * st + 8 * kh + e;
            float4 f = make_float4(0.f, 0.f, 0.f, 0.f);
            if (j < S) {
                int idx = sample_index(j, step, nf);
                idx = max(0, min(idx, max_frames - 1));
                f = raw.load4(((int64_t)b * max_frames + idx) * F + c, (int64_t)b * S + j);
                f.x = fmaf(f.x - ce.x, sc.x, sh.x); f.y = fmaf(f.y - ce.y, sc.y, sh.y);
                f.z = fmaf(f.z - ce.z, sc.z, sh.z); f.w = fmaf(f.w - ce.w, sc.w, sh.w);
                const int64_t row = (int64_t)b * S + j;
                if (!y2) *reinterpret_cast<float4*>(y + row * F + c) = f;
                else if (c < Dv) *reinterpret_cast<float4*>(y + row * Dv + c) = f;
                else *reinterpret_cast<float4*>(y2 + row * Da + (c - Dv)) = f;
            }
            v[0][e] = f.x; v[1][e] = f.y; v[2][e] = f.z; v[3][e] = f.w;
        }
        uint4* xt = (c < Dv) ? xtv : xta;
        const int DT = ((c < Dv) ? Dv : Da) / 32;
        const int cb = (c < Dv) ? c : c - Dv;
        if (xt == nullptr) continue;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            unsigned h[8], l[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                h[e] = fp_bf16_rne(v[q][e]);
                l[e] = fp_bf16_rne(v[q][e] - __uint_as_float(h[e] << 16));
            }
            const int d = cb + q, dt = d >> 5, jj = d & 31;
            const int64_t base = ((((int64_t)b * NS + st) * DT + dt) * 2) * 64 + kh * 32 + jj;
            xt[base] = make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
            xt[base + 64] = make_uint4(l[0] | (l[1] << 16), l[2] | (l[3] << 16), l[4] | (l[5] << 16), l[6] | (l[7] << 16));
        }
    }
}

// the centre the two backward kernels take off a column's frames: both form it from the same (mean, var), so they agree with each other.
// It is chosen independently of the forward's centre (the fold's 4 mean^2 > var, eval mode's moving_mean^2 > moving_var) and need not
// agree with it: dgamma = rstd (sum dy (x - c0) - (mean - c0) sum dy) is the same number for ANY c0, and only its rounding depends on it.
__device__ __forceinline__ float fbb_centre(float mean, float var) { return mean * mean > var ? mean : 0.f; }

// column partials of (sum dy, sum dy * (x - c0)) over the gathered rows, for dgamma/dbeta of input_bn
template <typename Src, typename Idx>
__global__ __launch_bounds__(256) void frame_bn_bwd_partial_kernel(const float* __restrict__ dy, int64_t lddy, Src raw, Idx ix, int B,
                                                                   int max_frames, int F, int S,
                                                                   float* __restrict__ partial, const float* __restrict__ dy2,
                                                                   int64_t lddy2, int Dv, const float* __restrict__ mean,
                                                                   const float* __restrict__ var) {
    // The second sum is sum dy (x - c0) with c0 = fbb_centre(mean, var): the column's fp32 mean where mean^2 > var, 0 elsewhere (there
    // x - 0 is x and every bit is what it was).  sum dy x from fp32 products loses eps32 (mean/std) of dgamma = rstd (sum dy x - mean sum dy):
    // measured in eval mode at mean/std = 30, dgamma 6 .. 11 times the bound of tests/test_gpu_frame_prep_bounds.py.
    // dy2 != null: the gradient arrives as two matrices, columns [0, Dv) in dy and [Dv, F) in dy2 (lpm_frame_apply_tiles_split's outputs)
    constexpr int W = Src::W;       // W = 4: Dv, both row strides and both pointers are multiples of four floats (checked by the host)
    const int r0 = blockIdx.x * FP_ROWS;
    const int rows = B * S;
    const int r1 = min(rows, r0 + FP_ROWS);
    __shared__ int64_t base[FP_ROWS];
    if (threadIdx.x < FP_ROWS) {
        const int r = r0 + threadIdx.x;
        if (r < rows) {
            const int b = r / S, j = r % S;
            const int idx = max(0, min(ix(b, j, r), max_frames - 1));
            base[threadIdx.x] = ((int64_t)b * max_frames + idx) * F;
        }
    }
    __syncthreads();
    for (int c = threadIdx.x * W; c < F; c += 256 * W) {
        float s[W], q[W], c0[W];
#pragma unroll
        for (int k = 0; k < W; ++k) {
            s[k] = q[k] = 0.f;
            c0[k] = fbb_centre(mean[c + k], var[c + k]);
        }
        for (int r = 0; r < r1 - r0; ++r) {
            float g[W], x[W];
            loadw_f32<W>((dy2 && c >= Dv) ? dy2 + (int64_t)(r0 + r) * lddy2 + (c - Dv) : dy + (int64_t)(r0 + r) * lddy + c, g);
            raw.loadw(base[r] + c, r0 + r, x);
#pragma unroll
            for (int k = 0; k < W; ++k) {
                s[k] += g[k];
                q[k] = fmaf(g[k], x[k] - c0[k], q[k]);
            }
        }
        float* p = partial + (int64_t)blockIdx.x * 2 * F;
        storew_f32<W>(p + c, s);
        storew_f32<W>(p + F + c, q);
    }
}

__global__ __launch_bounds__(1024) void frame_bn_bwd_reduce_kernel(const float* __restrict__ partial, int nblk,
                                                                   int F, const float* __restrict__ mean,
                                                                   const float* __restrict__ var, float eps,
                                                                   float* dgamma, float* dbeta) {
    double s, q;
    int c;
    partial_colsums16(partial, nblk, 2 * (int64_t)F, F, F, s, q, c);
    if (threadIdx.x < 16 && c < F) {
        // sum dy * xhat = rstd * (sum dy*(x - c0) - (mean - c0) * sum dy)
        const double rstd = 1.0 / sqrt((double)var[c] + (double)eps);
        dbeta[c] = (float)s;
        dgamma[c] = (float)(rstd * (q - ((double)mean[c] - (double)fbb_centre(mean[c], var[c])) * s));
    }
}

// The reader's output folded into the same pass (readers.py:176-193 + utils.py:28-43 + train.py:262-264): quantised uint8
// frames -> Dequantize (q * range/255 + range/512 + min) -> zero the frames at and beyond num_frames (the reader pads
// AFTER dequantising, so padding is exactly 0) -> L2-normalise each frame.  1 byte read, 4 bytes written per feature.
__global__ __launch_bounds__(256) void dequantize_l2_normalize_kernel(const unsigned char* __restrict__ q,
                                                                      const int32_t* __restrict__ num_frames, int64_t rows,
                                                                      int max_frames, int F, float scalar, float bias,
                                                                      float* __restrict__ y) {
    const int lane = threadIdx.x & 63;
    const int F4 = F >> 2;
    for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * 4) {
        const int b = (int)(r / max_frames), t = (int)(r % max_frames);
        float4* dst = reinterpret_cast<float4*>(y + r * F);
        if (t >= num_frames[b]) {                       // wave-uniform
            for (int c = lane; c < F4; c += 64) dst[c] = make_float4(0.f, 0.f, 0.f, 0.f);
            continue;
        }
        float4 v[8];
        const float inv = dequant_row_inv_norm(reinterpret_cast<const uchar4*>(q + r * F), lane, F4, scalar, bias, v);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int c = lane + 64 * i;
            if (c < F4) dst[c] = make_float4(v[i].x * inv, v[i].y * inv, v[i].z * inv, v[i].w * inv);
        }
    }
}

// The inverse L2 norm of the dequantised frame behind every SAMPLED row r = b S + j (the frame idx = sample_index(j) of clip b), for
// the FrameSrc<unsigned char> apply kernels: 1 byte read per feature of the S sampled frames, 4 bytes written per row.  A frame at
// or past num_frames[b] -- zero after the reader's padding -- gets 0.  Same wave split and order as dequantize_l2_normalize_kernel.
// (Idx = TableIdx: the frame frame_index[r], lpm_frame_inv_norm_q8_idx.)
template <typename Idx>
__global__ __launch_bounds__(256) void frame_inv_norm_q8_kernel(const unsigned char* __restrict__ q, const int32_t* __restrict__ num_frames,
                                                                Idx ix, int B, int max_frames, int F, int S, float scalar, float bias,
                                                                float* __restrict__ inv) {
    const int lane = threadIdx.x & 63;
    const int F4 = F >> 2;
    const int64_t rows = (int64_t)B * S;
    for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * 4) {
        const int b = (int)(r / S), j = (int)(r % S);
        const int nf = num_frames[b];
        const int idx = max(0, min(ix(b, j, r), max_frames - 1));
        float s = 0.f;
        if (idx < nf) {                                   // wave-uniform
            float4 v[8];
            s = dequant_row_inv_norm(reinterpret_cast<const uchar4*>(q + ((int64_t)b * max_frames + idx) * F), lane, F4, scalar, bias, v);
        }
        if (lane == 0) inv[r] = s;
    }
}

// Input normalisation of the training step (train.py:262-264, tf.nn.l2_normalize(model_input_raw, 2)): every frame row
// x <- x * rsqrt(max(sum x^2, 1e-12)).  One wave per row, float4 lanes; one read and one write of the batch.
__global__ __launch_bounds__(256) void l2_normalize_rows_kernel(const float* __restrict__ x, int64_t rows, int F,
                                                                float* __restrict__ y) {
    const int lane = threadIdx.x & 63;
    const int F4 = F >> 2;
    for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * 4) {
        const float4* src = reinterpret_cast<const float4*>(x + r * F);
        float4 v[8];
        float ss = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int c = lane + 64 * i;
            v[i] = (c < F4) ? src[c] : make_float4(0.f, 0.f, 0.f, 0.f);
            ss += v[i].x * v[i].x + v[i].y * v[i].y + v[i].z * v[i].z + v[i].w * v[i].w;
        }
        ss = wave_sum(ss);
        const float inv = rsqrtf(fmaxf(ss, 1e-12f));
        float4* dst = reinterpret_cast<float4*>(y + r * F);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int c = lane + 64 * i;
            if (c < F4) dst[c] = make_float4(v[i].x * inv, v[i].y * inv, v[i].z * inv, v[i].w * inv);
        }
    }
}

// bf16 storage (BASELINE cfg-5): the sampled, batch-normalised frames leave ONLY as plain bf16 operand tiles -- frame tiles
// [b][step][column tile][lane] (K2's operand, reduction over frames) and row tiles [b][row tile][column step][lane] (K1's
// operand, reduction over features), both padded with zero frames to whole 64-frame blocks (NSP = 4 ceil(S / 64) steps, MT = NSP / 2
// row tiles) -- and, when y is given, as the fp32 matrix.  Work item = (clip, step, frame half, 8 consecutive columns).
// PL = 2 (fp32 storage, lpm_frame_apply_tiles2): the same pass writes the SPLIT-bf16 forms -- frame tiles with ceil(S / 16) steps per
// clip (the layout of lpm_split_frames) and row tiles with 2 ceil(S / 64) tiles per clip (the layout of lpm_split_rows_tiles), hi and
// lo planes -- so that K1 needs no tile-split pass of its own over the fp32 matrix.
template <int PL, typename Src>
__global__ __launch_bounds__(256) void frame_apply_tiles_bf16_kernel(Src raw, const int32_t* __restrict__ num_frames,
                                                                     int B, int max_frames, int F, int S, float step,
                                                                     const float* __restrict__ scale, const float* __restrict__ shift,
                                                                     float* __restrict__ y, uint4* __restrict__ xtv, uint4* __restrict__ xrv,
                                                                     int Dv, uint4* __restrict__ xta, uint4* __restrict__ xra, int Da,
                                                                     const float* __restrict__ centre) {
    const int F8 = F / 8, NSP = 4 * ((S + 63) / 64), MT = NSP / 2;
    const int64_t total = (int64_t)B * NSP * 2 * F8;
    for (int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x; w < total; w += (int64_t)gridDim.x * 256) {
        const int c8 = (int)(w % F8);
        const int64_t r = w / F8;
        const int kh = (int)(r & 1), st = (int)((r >> 1) % NSP), b = (int)((r >> 1) / NSP);
        const int c = 8 * c8;
        float sc[8], sh[8], ce[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            sc[q] = scale ? scale[c + q] : 1.f;
            sh[q] = scale ? shift[c + q] : 0.f;
            ce[q] = (scale && centre) ? centre[c + q] : 0.f;                   // (frame_apply_kernel says what it is)
        }
        const int nf = num_frames[b];
        float v[8][8];                    // [frame e][column q]
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int j = 16 * st + 8 * kh + e;
            float4 f0 = make_float4(0.f, 0.f, 0.f, 0.f), f1 = f0;
            if (j < S) {
                int idx = sample_index(j, step, nf);
                idx = max(0, min(idx, max_frames - 1));
                const int64_t src = ((int64_t)b * max_frames + idx) * F + c, row = (int64_t)b * S + j;
                f0 = raw.load4(src, row);
                f1 = raw.load4(src + 4, row);
                f0.x = fmaf(f0.x - ce[0], sc[0], sh[0]); f0.y = fmaf(f0.y - ce[1], sc[1], sh[1]);
                f0.z = fmaf(f0.z - ce[2], sc[2], sh[2]); f0.w = fmaf(f0.w - ce[3], sc[3], sh[3]);
                f1.x = fmaf(f1.x - ce[4], sc[4], sh[4]); f1.y = fmaf(f1.y - ce[5], sc[5], sh[5]);
                f1.z = fmaf(f1.z - ce[6], sc[6], sh[6]); f1.w = fmaf(f1.w - ce[7], sc[7], sh[7]);
                if (y) {
                    float* dst = y + ((int64_t)b * S + j) * F + c;
                    *reinterpret_cast<float4*>(dst) = f0;
                    *reinterpret_cast<float4*>(dst + 4) = f1;
                }
            }
            v[e][0] = f0.x; v[e][1] = f0.y; v[e][2] = f0.z; v[e][3] = f0.w; v[e][4] = f1.x; v[e][5] = f1.y; v[e][6] = f1.z; v[e][7] = f1.w;
        }
        const bool video = c < Dv;
        uint4* xt = video ? xtv : xta;
        uint4* xr = video ? xrv : xra;
        if (xt == nullptr) continue;
        const int Dn = video ? Dv : Da, cb = video ? c : c - Dv;
        unsigned h[8][8], l[8][8];
#pragma unroll
        for (int e = 0; e < 8; ++e)
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                h[e][q] = fp_bf16_rne(v[e][q]);
                if (PL == 2) l[e][q] = fp_bf16_rne(v[e][q] - __uint_as_float(h[e][q] << 16));
            }
        const int DT = Dn / 32, CS = Dn / 16;
        const int NSF = PL == 2 ? (S + 15) / 16 : NSP;        // frame-tile steps per clip
        if (st < NSF) {
#pragma unroll
            for (int q = 0; q < 8; ++q) {       // frame tiles: lane = (frame half, column), 8 frames per lane
                const int d = cb + q;
                const int64_t base = ((((int64_t)b * NSF + st) * DT + (d >> 5)) * PL) * 64 + kh * 32 + (d & 31);
                xt[base] = make_uint4(h[0][q] | (h[1][q] << 16), h[2][q] | (h[3][q] << 16), h[4][q] | (h[5][q] << 16), h[6][q] | (h[7][q] << 16));
                if (PL == 2)
                    xt[base + 64] = make_uint4(l[0][q] | (l[1][q] << 16), l[2][q] | (l[3][q] << 16), l[4][q] | (l[5][q] << 16), l[6][q] | (l[7][q] << 16));
            }
        }
        if (xr == nullptr) continue;
#pragma unroll
        for (int e = 0; e < 8; ++e) {       // row tiles: lane = (column half, frame), 8 columns per lane
            const int j = 16 * st + 8 * kh + e;
            const int64_t base = ((((int64_t)b * MT + (j >> 5)) * CS + (cb >> 4)) * PL) * 64 + ((cb >> 3) & 1) * 32 + (j & 31);
            xr[base] = make_uint4(h[e][0] | (h[e][1] << 16), h[e][2] | (h[e][3] << 16), h[e][4] | (h[e][5] << 16), h[e][6] | (h[e][7] << 16));
            if (PL == 2)
                xr[base + 64] = make_uint4(l[e][0] | (l[e][1] << 16), l[e][2] | (l[e][3] << 16), l[e][4] | (l[e][5] << 16), l[e][6] | (l[e][7] << 16));
        }
    }
}

}  // namespace lpm

static inline int fp_nblk(int B, int S) { return (B * S + lpm::FP_ROWS - 1) / lpm::FP_ROWS; }

extern "C" size_t lpm_frame_stats_workspace_bytes(int B, int S, int F) {
    return (size_t)fp_nblk(B, S) * 2 * F * sizeof(float);
}
extern "C" int lpm_frame_stats_nblk(int B, int S) { return fp_nblk(B, S); }
// `partial` of the lpm_frame_stats* forms: the raw partials [nblk][2][F], the shifted partials [nblk][2][F], the pivots [F] -- what
// lpm_frame_bn_fold reads (lpm_bn_fold reads the first array alone)
extern "C" size_t lpm_frame_stats_partial_bytes(int B, int S, int F) {
    return ((size_t)fp_nblk(B, S) * 4 * F + (size_t)F) * sizeof(float);
}

// index: num_frames (the uniform forms) or frame_index (the *_idx forms)
#define LPM_FRAME_CHECK_(name, index)                                                                               \
    LPM_REQUIRE(raw && index, LPM_ERR_BADARG, name ": null pointer");                                               \
    LPM_REQUIRE(B > 0 && max_frames > 0 && F > 0 && S > 0, LPM_ERR_BADARG, name ": bad sizes");                      \
    LPM_REQUIRE(F % 4 == 0, LPM_ERR_UNSUPPORTED_SHAPE, name ": need F %% 4 == 0 (F=%d)", F)
#define LPM_FRAME_CHECK(name) LPM_FRAME_CHECK_(name, num_frames)
// the *_idx fp32 forms: float4 reads of the frame rows
#define LPM_FRAME_IDX_CHECK(name)                                                                                   \
    LPM_FRAME_CHECK_(name, frame_index);                                                                            \
    LPM_REQUIRE(((uintptr_t)raw & 15) == 0, LPM_ERR_UNSUPPORTED_SHAPE, name ": need 16-byte aligned frames")

// The quantised forms (*_q8): q [B, max_frames, F] uint8 (4-byte aligned), inv_norm [B S] from lpm_frame_inv_norm_q8 with the same
// num_frames / S / quantisation range.
#define LPM_FRAME_Q8_CHECK_(name, index)                                                                                             \
    LPM_REQUIRE(q && inv_norm && index, LPM_ERR_BADARG, name ": null pointer");                                                      \
    LPM_REQUIRE(max_quantized_value > min_quantized_value, LPM_ERR_BADARG, name ": empty quantisation range");                       \
    LPM_REQUIRE(B > 0 && max_frames > 0 && F > 0 && S > 0, LPM_ERR_BADARG, name ": bad sizes");                                       \
    LPM_REQUIRE(F % 4 == 0 && ((uintptr_t)q & 3) == 0, LPM_ERR_UNSUPPORTED_SHAPE, name ": need F %% 4 == 0, aligned input (F=%d)", F)
#define LPM_FRAME_Q8_CHECK(name) LPM_FRAME_Q8_CHECK_(name, num_frames)
#define LPM_FRAME_Q8_IDX_CHECK(name) LPM_FRAME_Q8_CHECK_(name, frame_index)

// centre (the apply forms' last parameter, may be NULL): one value per column, taken off the frames before scale and shift
#define LPM_FRAME_CENTRE_CHECK(name)                                                                                          \
    LPM_REQUIRE(centre == nullptr || (scale != nullptr && ((uintptr_t)centre & 15) == 0), LPM_ERR_BADARG,                      \
                "%s: centre needs scale and shift, and 16-byte alignment", name)

namespace {

using lpm::FrameSrc;
using lpm::TableIdx;

lpm::UniformIdx uniform_idx(const int32_t* num_frames, int S) { return lpm::UniformIdx{num_frames, 1.0f / (float)S}; }

// utils.Dequantize's affine, computed as lpm_dequantize_l2_normalize computes it
FrameSrc<unsigned char> q8_src(const unsigned char* q, const float* inv_norm, float max_quantized_value, float min_quantized_value) {
    const float range = max_quantized_value - min_quantized_value;
    return FrameSrc<unsigned char>{q, inv_norm, range / 255.0f, range / 512.0f + min_quantized_value};
}

// y2 == NULL: one [B S, F] matrix y; else y [B S, Dv] and y2 [B S, F - Dv] (the *_split_idx forms)
template <typename Src, typename Idx>
int launch_frame_apply(Src raw, Idx ix, int B, int max_frames, int F, int S, const float* scale, const float* shift, float* y, float* y2,
                       int Dv, hipStream_t stream, const char* name, const float* centre) {
    using namespace lpm;
    LPM_REQUIRE(y && ((scale == nullptr) == (shift == nullptr)), LPM_ERR_BADARG, "%s: bad pointers", name);
    LPM_FRAME_CENTRE_CHECK(name);
    if (y2 != nullptr)
        LPM_REQUIRE(Dv > 0 && Dv < F && Dv % 4 == 0 && (((uintptr_t)y | (uintptr_t)y2 | (uintptr_t)scale | (uintptr_t)shift) & 15) == 0,
                    LPM_ERR_UNSUPPORTED_SHAPE, "%s: need 0 < Dv < F, Dv %% 4 == 0, 16-byte aligned buffers (F=%d Dv=%d)", name, F, Dv);
    const int64_t total = (int64_t)B * S * (F / 4);
    const int64_t want = (total + 255) / 256;
    hipLaunchKernelGGL((frame_apply_kernel<Src, Idx>), dim3((unsigned)(want < 4096 ? want : 4096)), dim3(256), 0, stream, raw, ix, B,
                       max_frames, F, S, scale, shift, y, y2, Dv, centre);
    return check_launch(name);
}

// y2 == NULL: one [B S, F] matrix y (lpm_frame_apply_tiles); else y [B S, Dv] and y2 [B S, Da] (lpm_frame_apply_tiles_split)
template <typename Src>
int launch_frame_apply_tiles(Src raw, const int32_t* num_frames, int B, int max_frames, int F, int S, const float* scale,
                             const float* shift, float* y, float* y2, void* xt_video, int Dv, void* xt_audio, int Da, hipStream_t stream,
                             const char* name, const float* centre) {
    using namespace lpm;
    LPM_FRAME_CENTRE_CHECK(name);
    if (y2 == nullptr) {
        LPM_REQUIRE(y && ((scale == nullptr) == (shift == nullptr)), LPM_ERR_BADARG, "%s: bad pointers", name);
        LPM_REQUIRE(Dv > 0 && Da >= 0 && Dv + Da == F && Dv % 32 == 0 && Da % 32 == 0, LPM_ERR_UNSUPPORTED_SHAPE,
                    "%s: need Dv + Da == F, both multiples of 32 (F=%d Dv=%d Da=%d)", name, F, Dv, Da);
    } else {
        LPM_REQUIRE(y && ((scale == nullptr) == (shift == nullptr)), LPM_ERR_BADARG, "%s: bad pointers", name);
        LPM_REQUIRE(Dv > 0 && Da > 0 && Dv + Da == F && Dv % 32 == 0 && Da % 32 == 0 && (((uintptr_t)y | (uintptr_t)y2) & 15) == 0,
                    LPM_ERR_UNSUPPORTED_SHAPE, "%s: need Dv + Da == F, both multiples of 32, aligned outputs (F=%d Dv=%d Da=%d)", name, F,
                    Dv, Da);
    }
    const float step = 1.0f / (float)S;
    const int64_t total = (int64_t)B * ((S + 15) / 16) * 2 * (F / 4);
    const int64_t want = (total + 255) / 256;
    hipLaunchKernelGGL(frame_apply_tiles_kernel<Src>, dim3((unsigned)(want < 8192 ? want : 8192)), dim3(256), 0, stream, raw, num_frames,
                       B, max_frames, F, S, step, scale, shift, y, (uint4*)xt_video, Dv, (uint4*)xt_audio, Da, y2, centre);
    return check_launch(name);
}

// PL = 1: lpm_frame_apply_tiles_bf16 (y optional, row tiles required); PL = 2: lpm_frame_apply_tiles2 (y required, row tiles optional)
template <int PL, typename Src>
int launch_frame_apply_tiles_bf16(Src raw, const int32_t* num_frames, int B, int max_frames, int F, int S, const float* scale,
                                  const float* shift, float* y, void* xt_video, void* xr_video, int Dv, void* xt_audio, void* xr_audio,
                                  int Da, hipStream_t stream, const char* name, const float* centre) {
    using namespace lpm;
    LPM_FRAME_CENTRE_CHECK(name);
    if (PL == 1)
        LPM_REQUIRE(xt_video && xr_video && ((scale == nullptr) == (shift == nullptr)) && ((xt_audio == nullptr) == (xr_audio == nullptr)),
                    LPM_ERR_BADARG, "%s: bad pointers", name);
    else
        LPM_REQUIRE(y && xt_video && ((scale == nullptr) == (shift == nullptr)) && (Da == 0 || xt_audio), LPM_ERR_BADARG,
                    "%s: bad pointers", name);
    LPM_REQUIRE(Dv > 0 && Da >= 0 && Dv + Da == F && Dv % 32 == 0 && Da % 32 == 0, LPM_ERR_UNSUPPORTED_SHAPE,
                "%s: need Dv + Da == F, both multiples of 32 (F=%d Dv=%d Da=%d)", name, F, Dv, Da);
    const float step = 1.0f / (float)S;
    const int64_t total = (int64_t)B * 4 * ((S + 63) / 64) * 2 * (F / 8);
    const int64_t want = (total + 255) / 256;
    hipLaunchKernelGGL((frame_apply_tiles_bf16_kernel<PL, Src>), dim3((unsigned)(want < 16384 ? want : 16384)), dim3(256), 0, stream, raw,
                       num_frames, B, max_frames, F, S, step, scale, shift, y, (uint4*)xt_video, (uint4*)xr_video, Dv, (uint4*)xt_audio,
                       (uint4*)xr_audio, Da, centre);
    return check_launch(name);
}

template <typename Src, typename Idx>
int launch_frame_stats(Src raw, Idx ix, int B, int max_frames, int F, int S, float* partial, size_t partial_bytes, hipStream_t stream,
                       const char* name) {
    using namespace lpm;
    LPM_REQUIRE(partial, LPM_ERR_BADARG, "%s: null workspace", name);
    LPM_REQUIRE(partial_bytes >= lpm_frame_stats_partial_bytes(B, S, F), LPM_ERR_WORKSPACE,
                "%s: partial too small (the raw partials, the shifted partials and the pivots: lpm_frame_stats_partial_bytes)", name);
    LPM_REQUIRE(Src::W == 1 || ((uintptr_t)partial & 15) == 0, LPM_ERR_UNSUPPORTED_SHAPE, "%s: need a 16-byte aligned workspace", name);
    const size_t raw_floats = (size_t)fp_nblk(B, S) * 2 * F;       // `partial` holds lpm_frame_stats_partial_bytes(B, S, F)
    hipLaunchKernelGGL((frame_stats_kernel<Src, Idx>), dim3(fp_nblk(B, S)), dim3(256), 0, stream, raw, ix, B, max_frames, F, S, partial,
                       partial + raw_floats, partial + 2 * raw_floats);
    return check_launch(name);
}

// dy2 == NULL: one gradient matrix dy [B S, F] (lpm_frame_bn_bwd); else dy [B S, Dv] and dy2 [B S, F - Dv] (lpm_frame_bn_bwd_split)
template <typename Src, typename Idx>
int launch_frame_bn_bwd(const float* dy, int64_t lddy, const float* dy2, int64_t lddy2, int Dv, Src raw, Idx ix, int B,
                        int max_frames, int F, int S, const float* mean, const float* var, float eps, float* dgamma, float* dbeta,
                        void* workspace, size_t workspace_bytes, hipStream_t stream, const char* name) {
    using namespace lpm;
    if (dy2 == nullptr)
        LPM_REQUIRE(dy && mean && var && dgamma && dbeta && workspace && lddy >= F, LPM_ERR_BADARG, "%s: bad pointers", name);
    else
        LPM_REQUIRE(dy && mean && var && dgamma && dbeta && workspace && Dv > 0 && Dv < F && lddy >= Dv && lddy2 >= F - Dv, LPM_ERR_BADARG,
                    "%s: bad pointers / strides", name);
    LPM_REQUIRE(workspace_bytes >= lpm_frame_stats_workspace_bytes(B, S, F), LPM_ERR_WORKSPACE, "%s: workspace too small", name);
    if (Src::W == 4)        // float4 reads of the gradient, float4 writes of the partials
        LPM_REQUIRE((((uintptr_t)dy | (uintptr_t)dy2 | (uintptr_t)workspace) & 15) == 0 && lddy % 4 == 0 &&
                        (dy2 == nullptr || (lddy2 % 4 == 0 && Dv % 4 == 0)),
                    LPM_ERR_UNSUPPORTED_SHAPE, "%s: need 16-byte aligned gradients and workspace, row strides and Dv multiples of 4", name);
    const int nblk = fp_nblk(B, S);
    hipLaunchKernelGGL((frame_bn_bwd_partial_kernel<Src, Idx>), dim3(nblk), dim3(256), 0, stream, dy, lddy, raw, ix, B, max_frames, F, S,
                       (float*)workspace, dy2, lddy2, dy2 ? Dv : F, mean, var);
    hipLaunchKernelGGL(frame_bn_bwd_reduce_kernel, dim3((F + 15) / 16), dim3(1024), 0, stream, (const float*)workspace, nblk, F, mean, var,
                       eps, dgamma, dbeta);
    return check_launch(name);
}

}  // namespace

extern "C" int lpm_frame_stats(const float* raw, const int32_t* num_frames, int B, int max_frames, int F, int S,
                               float* partial, size_t partial_bytes, lpm_stream_t stream) {
    LPM_FRAME_CHECK("lpm_frame_stats");
    return launch_frame_stats(FrameSrc<float>{raw}, uniform_idx(num_frames, S), B, max_frames, F, S, partial, partial_bytes, (hipStream_t)stream, "lpm_frame_stats");
}

extern "C" int lpm_frame_apply(const float* raw, const int32_t* num_frames, int B, int max_frames, int F, int S,
                               const float* scale, const float* shift, float* y, lpm_stream_t stream, const float* centre) {
    LPM_FRAME_CHECK("lpm_frame_apply");
    return launch_frame_apply(FrameSrc<float>{raw}, uniform_idx(num_frames, S), B, max_frames, F, S, scale, shift, y, nullptr, F,
                              (hipStream_t)stream, "lpm_frame_apply", centre);
}

extern "C" int lpm_frame_apply_tiles(const float* raw, const int32_t* num_frames, int B, int max_frames, int F, int S,
                                     const float* scale, const float* shift, float* y, void* xt_video, int Dv,
                                     void* xt_audio, int Da, lpm_stream_t stream, const float* centre) {
    LPM_FRAME_CHECK("lpm_frame_apply_tiles");
    return launch_frame_apply_tiles(FrameSrc<float>{raw}, num_frames, B, max_frames, F, S, scale, shift, y, nullptr, xt_video, Dv, xt_audio,
                                    Da, (hipStream_t)stream, "lpm_frame_apply_tiles", centre);
}
// ... with the two column blocks as two contiguous matrices y_video [B S, Dv] and y_audio [B S, Da] (round 6: NetVladV2)
extern "C" int lpm_frame_apply_tiles_split(const float* raw, const int32_t* num_frames, int B, int max_frames, int F, int S,
                                           const float* scale, const float* shift, float* y_video, float* y_audio, void* xt_video, int Dv,
                                           void* xt_audio, int Da, lpm_stream_t stream, const float* centre) {
    LPM_FRAME_CHECK("lpm_frame_apply_tiles_split");
    LPM_REQUIRE(y_video && y_audio, LPM_ERR_BADARG, "lpm_frame_apply_tiles_split: bad pointers");
    return launch_frame_apply_tiles(FrameSrc<float>{raw}, num_frames, B, max_frames, F, S, scale, shift, y_video, y_audio, xt_video, Dv,
                                    xt_audio, Da, (hipStream_t)stream, "lpm_frame_apply_tiles_split", centre);
}

// bf16 storage: see frame_apply_tiles_bf16_kernel.  y may be NULL (then the fp32 frames are not written at all); the tile buffers
// hold lpm_frame_tiles_bf16_bytes(B, S, D) bytes each (frame tiles and row tiles have the same size).
extern "C" size_t lpm_frame_tiles_bf16_bytes(int B, int S, int D) { return (size_t)B * 4 * ((S + 63) / 64) * (D / 32) * 1024; }
extern "C" int lpm_frame_apply_tiles_bf16(const float* raw, const int32_t* num_frames, int B, int max_frames, int F, int S,
                                          const float* scale, const float* shift, float* y, void* xt_video, void* xr_video, int Dv,
                                          void* xt_audio, void* xr_audio, int Da, lpm_stream_t stream, const float* centre) {
    LPM_FRAME_CHECK("lpm_frame_apply_tiles_bf16");
    return launch_frame_apply_tiles_bf16<1>(FrameSrc<float>{raw}, num_frames, B, max_frames, F, S, scale, shift, y, xt_video, xr_video, Dv,
                                            xt_audio, xr_audio, Da, (hipStream_t)stream, "lpm_frame_apply_tiles_bf16", centre);
}

// fp32 storage: a2 + a3 -> y (fp32 [B*S, F]) AND the split-bf16 frame tiles (lpm_xt_bytes each: K2's operand) AND row tiles
// (lpm_row_tiles_bytes each: K1's operand; NULL: not wanted) of both streams in one pass over the sampled frames.
extern "C" int lpm_frame_apply_tiles2(const float* raw, const int32_t* num_frames, int B, int max_frames, int F, int S,
                                      const float* scale, const float* shift, float* y, void* xt_video, void* xr_video, int Dv,
                                      void* xt_audio, void* xr_audio, int Da, lpm_stream_t stream, const float* centre) {
    LPM_FRAME_CHECK("lpm_frame_apply_tiles2");
    return launch_frame_apply_tiles_bf16<2>(FrameSrc<float>{raw}, num_frames, B, max_frames, F, S, scale, shift, y, xt_video, xr_video, Dv,
                                            xt_audio, xr_audio, Da, (hipStream_t)stream, "lpm_frame_apply_tiles2", centre);
}

// ---- eval mode from the reader's quantised frames -----------------------------------------------------------------------------
namespace {
template <typename Idx>
int launch_frame_inv_norm_q8(const unsigned char* q, const int32_t* num_frames, Idx ix, int B, int max_frames, int F, int S,
                             float max_quantized_value, float min_quantized_value, float* inv_norm, hipStream_t stream, const char* name) {
    using namespace lpm;
    LPM_REQUIRE(F <= 2048, LPM_ERR_UNSUPPORTED_SHAPE, "%s: need F <= 2048 (F=%d)", name, F);
    const FrameSrc<unsigned char> src = q8_src(q, inv_norm, max_quantized_value, min_quantized_value);
    const int64_t rows = (int64_t)B * S, want = (rows + 3) / 4;
    hipLaunchKernelGGL(frame_inv_norm_q8_kernel<Idx>, dim3((unsigned)(want < 16384 ? want : 16384)), dim3(256), 0, stream, q, num_frames, ix,
                       B, max_frames, F, S, src.scalar, src.bias, inv_norm);
    return check_launch(name);
}
}  // namespace

extern "C" int lpm_frame_inv_norm_q8(const unsigned char* q, const int32_t* num_frames, int B, int max_frames, int F, int S,
                                     float max_quantized_value, float min_quantized_value, float* inv_norm, lpm_stream_t stream) {
    LPM_FRAME_Q8_CHECK("lpm_frame_inv_norm_q8");
    return launch_frame_inv_norm_q8(q, num_frames, uniform_idx(num_frames, S), B, max_frames, F, S, max_quantized_value, min_quantized_value,
                                    inv_norm, (hipStream_t)stream, "lpm_frame_inv_norm_q8");
}

extern "C" int lpm_frame_apply_q8(const unsigned char* q, const float* inv_norm, float max_quantized_value, float min_quantized_value,
                                  const int32_t* num_frames, int B, int max_frames, int F, int S, const float* scale, const float* shift,
                                  float* y, lpm_stream_t stream, const float* centre) {
    LPM_FRAME_Q8_CHECK("lpm_frame_apply_q8");
    return launch_frame_apply(q8_src(q, inv_norm, max_quantized_value, min_quantized_value), uniform_idx(num_frames, S), B, max_frames, F, S,
                              scale, shift, y, nullptr, F, (hipStream_t)stream, "lpm_frame_apply_q8", centre);
}

extern "C" int lpm_frame_apply_tiles_q8(const unsigned char* q, const float* inv_norm, float max_quantized_value,
                                        float min_quantized_value, const int32_t* num_frames, int B, int max_frames, int F, int S,
                                        const float* scale, const float* shift, float* y, void* xt_video, int Dv, void* xt_audio, int Da,
                                        lpm_stream_t stream, const float* centre) {
    LPM_FRAME_Q8_CHECK("lpm_frame_apply_tiles_q8");
    return launch_frame_apply_tiles(q8_src(q, inv_norm, max_quantized_value, min_quantized_value), num_frames, B, max_frames, F, S, scale,
                                    shift, y, nullptr, xt_video, Dv, xt_audio, Da, (hipStream_t)stream, "lpm_frame_apply_tiles_q8", centre);
}

extern "C" int lpm_frame_apply_tiles_split_q8(const unsigned char* q, const float* inv_norm, float max_quantized_value,
                                              float min_quantized_value, const int32_t* num_frames, int B, int max_frames, int F, int S,
                                              const float* scale, const float* shift, float* y_video, float* y_audio, void* xt_video,
                                              int Dv, void* xt_audio, int Da, lpm_stream_t stream, const float* centre) {
    LPM_FRAME_Q8_CHECK("lpm_frame_apply_tiles_split_q8");
    LPM_REQUIRE(y_video && y_audio, LPM_ERR_BADARG, "lpm_frame_apply_tiles_split_q8: bad pointers");
    return launch_frame_apply_tiles(q8_src(q, inv_norm, max_quantized_value, min_quantized_value), num_frames, B, max_frames, F, S, scale,
                                    shift, y_video, y_audio, xt_video, Dv, xt_audio, Da, (hipStream_t)stream, "lpm_frame_apply_tiles_split_q8", centre);
}

extern "C" int lpm_frame_apply_tiles_bf16_q8(const unsigned char* q, const float* inv_norm, float max_quantized_value,
                                             float min_quantized_value, const int32_t* num_frames, int B, int max_frames, int F, int S,
                                             const float* scale, const float* shift, float* y, void* xt_video, void* xr_video, int Dv,
                                             void* xt_audio, void* xr_audio, int Da, lpm_stream_t stream, const float* centre) {
    LPM_FRAME_Q8_CHECK("lpm_frame_apply_tiles_bf16_q8");
    return launch_frame_apply_tiles_bf16<1>(q8_src(q, inv_norm, max_quantized_value, min_quantized_value), num_frames, B, max_frames, F, S,
                                            scale, shift, y, xt_video, xr_video, Dv, xt_audio, xr_audio, Da, (hipStream_t)stream,
                                            "lpm_frame_apply_tiles_bf16_q8", centre);
}

extern "C" int lpm_frame_apply_tiles2_q8(const unsigned char* q, const float* inv_norm, float max_quantized_value,
                                         float min_quantized_value, const int32_t* num_frames, int B, int max_frames, int F, int S,
                                         const float* scale, const float* shift, float* y, void* xt_video, void* xr_video, int Dv,
                                         void* xt_audio, void* xr_audio, int Da, lpm_stream_t stream, const float* centre) {
    LPM_FRAME_Q8_CHECK("lpm_frame_apply_tiles2_q8");
    return launch_frame_apply_tiles_bf16<2>(q8_src(q, inv_norm, max_quantized_value, min_quantized_value), num_frames, B, max_frames, F, S,
                                            scale, shift, y, xt_video, xr_video, Dv, xt_audio, xr_audio, Da, (hipStream_t)stream,
                                            "lpm_frame_apply_tiles2_q8", centre);
}

extern "C" int lpm_frame_bn_bwd(const float* dy, int64_t lddy, const float* raw, const int32_t* num_frames, int B,
                                int max_frames, int F, int S, const float* mean, const float* var, float eps,
                                float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes,
                                lpm_stream_t stream) {
    LPM_FRAME_CHECK("lpm_frame_bn_bwd");
    return launch_frame_bn_bwd(dy, lddy, nullptr, 0, F, FrameSrc<float>{raw}, uniform_idx(num_frames, S), B, max_frames, F, S, mean, var, eps,
                               dgamma, dbeta, workspace, workspace_bytes, (hipStream_t)stream, "lpm_frame_bn_bwd");
}
// ... with the gradient as two matrices: dy_video [B S, Dv] (row stride ldv) and dy_audio [B S, F - Dv] (row stride lda)
extern "C" int lpm_frame_bn_bwd_split(const float* dy_video, int64_t ldv, const float* dy_audio, int64_t lda, int Dv, const float* raw,
                                      const int32_t* num_frames, int B, int max_frames, int F, int S, const float* mean, const float* var,
                                      float eps, float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes, lpm_stream_t stream) {
    LPM_FRAME_CHECK("lpm_frame_bn_bwd_split");
    LPM_REQUIRE(dy_audio, LPM_ERR_BADARG, "lpm_frame_bn_bwd_split: bad pointers / strides");
    return launch_frame_bn_bwd(dy_video, ldv, dy_audio, lda, Dv, FrameSrc<float>{raw}, uniform_idx(num_frames, S), B, max_frames, F, S, mean, var,
                               eps, dgamma, dbeta, workspace, workspace_bytes, (hipStream_t)stream, "lpm_frame_bn_bwd_split");
}

// ---- training mode from the reader's quantised frames: the batch statistics and the dgamma / dbeta partials, bit for bit those of the
// fp32 forms on lpm_dequantize_l2_normalize's frames (inv_norm from lpm_frame_inv_norm_q8; gradients and workspace 16-byte aligned) ----
extern "C" int lpm_frame_stats_q8(const unsigned char* q, const float* inv_norm, float max_quantized_value, float min_quantized_value,
                                  const int32_t* num_frames, int B, int max_frames, int F, int S, float* partial, size_t partial_bytes, lpm_stream_t stream) {
    LPM_FRAME_Q8_CHECK("lpm_frame_stats_q8");
    return launch_frame_stats(q8_src(q, inv_norm, max_quantized_value, min_quantized_value), uniform_idx(num_frames, S), B, max_frames, F, S,
                              partial, partial_bytes, (hipStream_t)stream, "lpm_frame_stats_q8");
}

extern "C" int lpm_frame_bn_bwd_q8(const float* dy, int64_t lddy, const unsigned char* q, const float* inv_norm, float max_quantized_value,
                                   float min_quantized_value, const int32_t* num_frames, int B, int max_frames, int F, int S,
                                   const float* mean, const float* var, float eps, float* dgamma, float* dbeta, void* workspace,
                                   size_t workspace_bytes, lpm_stream_t stream) {
    LPM_FRAME_Q8_CHECK("lpm_frame_bn_bwd_q8");
    return launch_frame_bn_bwd(dy, lddy, nullptr, 0, F, q8_src(q, inv_norm, max_quantized_value, min_quantized_value),
                               uniform_idx(num_frames, S), B, max_frames, F, S, mean, var, eps, dgamma, dbeta, workspace, workspace_bytes,
                               (hipStream_t)stream, "lpm_frame_bn_bwd_q8");
}

extern "C" int lpm_frame_bn_bwd_split_q8(const float* dy_video, int64_t ldv, const float* dy_audio, int64_t lda, int Dv,
                                         const unsigned char* q, const float* inv_norm, float max_quantized_value,
                                         float min_quantized_value, const int32_t* num_frames, int B, int max_frames, int F, int S,
                                         const float* mean, const float* var, float eps, float* dgamma, float* dbeta, void* workspace,
                                         size_t workspace_bytes, lpm_stream_t stream) {
    LPM_FRAME_Q8_CHECK("lpm_frame_bn_bwd_split_q8");
    LPM_REQUIRE(dy_audio, LPM_ERR_BADARG, "lpm_frame_bn_bwd_split_q8: bad pointers / strides");
    return launch_frame_bn_bwd(dy_video, ldv, dy_audio, lda, Dv, q8_src(q, inv_norm, max_quantized_value, min_quantized_value),
                               uniform_idx(num_frames, S), B, max_frames, F, S, mean, var, eps, dgamma, dbeta, workspace, workspace_bytes,
                               (hipStream_t)stream, "lpm_frame_bn_bwd_split_q8");
}

// ---- the index-table forms (*_idx): sampled row r = b S + j reads frame frame_index[r] of clip b (clamped to [0, max_frames - 1]) instead
// of SampleUniformFrames' own index -- SampleRandomFrames for the triangulation models.  Same kernels, same arithmetic; the frames leave
// as two contiguous fp32 matrices and no operand tiles.  The q8 forms take inv_norm from lpm_frame_inv_norm_q8_idx with the same table. ----
extern "C" int lpm_frame_inv_norm_q8_idx(const unsigned char* q, const int32_t* num_frames, const int32_t* frame_index, int B, int max_frames,
                                         int F, int S, float max_quantized_value, float min_quantized_value, float* inv_norm,
                                         lpm_stream_t stream) {
    LPM_FRAME_Q8_CHECK("lpm_frame_inv_norm_q8_idx");
    LPM_REQUIRE(frame_index, LPM_ERR_BADARG, "lpm_frame_inv_norm_q8_idx: null pointer");
    return launch_frame_inv_norm_q8(q, num_frames, TableIdx{frame_index}, B, max_frames, F, S, max_quantized_value, min_quantized_value,
                                    inv_norm, (hipStream_t)stream, "lpm_frame_inv_norm_q8_idx");
}

extern "C" int lpm_frame_stats_idx(const float* raw, const int32_t* frame_index, int B, int max_frames, int F, int S, float* partial, size_t partial_bytes,
                                   lpm_stream_t stream) {
    LPM_FRAME_IDX_CHECK("lpm_frame_stats_idx");
    return launch_frame_stats(FrameSrc<float>{raw}, TableIdx{frame_index}, B, max_frames, F, S, partial, partial_bytes, (hipStream_t)stream,
                              "lpm_frame_stats_idx");
}
extern "C" int lpm_frame_stats_idx_q8(const unsigned char* q, const float* inv_norm, float max_quantized_value, float min_quantized_value,
                                      const int32_t* frame_index, int B, int max_frames, int F, int S, float* partial, size_t partial_bytes, lpm_stream_t stream) {
    LPM_FRAME_Q8_IDX_CHECK("lpm_frame_stats_idx_q8");
    return launch_frame_stats(q8_src(q, inv_norm, max_quantized_value, min_quantized_value), TableIdx{frame_index}, B, max_frames, F, S,
                              partial, partial_bytes, (hipStream_t)stream, "lpm_frame_stats_idx_q8");
}

extern "C" int lpm_frame_apply_split_idx(const float* raw, const int32_t* frame_index, int B, int max_frames, int F, int S, const float* scale,
                                         const float* shift, float* y_video, float* y_audio, int Dv, lpm_stream_t stream, const float* centre) {
    LPM_FRAME_IDX_CHECK("lpm_frame_apply_split_idx");
    LPM_REQUIRE(y_video && y_audio, LPM_ERR_BADARG, "lpm_frame_apply_split_idx: bad pointers");
    return launch_frame_apply(FrameSrc<float>{raw}, TableIdx{frame_index}, B, max_frames, F, S, scale, shift, y_video, y_audio, Dv,
                              (hipStream_t)stream, "lpm_frame_apply_split_idx", centre);
}
extern "C" int lpm_frame_apply_split_idx_q8(const unsigned char* q, const float* inv_norm, float max_quantized_value,
                                            float min_quantized_value, const int32_t* frame_index, int B, int max_frames, int F, int S,
                                            const float* scale, const float* shift, float* y_video, float* y_audio, int Dv,
                                            lpm_stream_t stream, const float* centre) {
    LPM_FRAME_Q8_IDX_CHECK("lpm_frame_apply_split_idx_q8");
    LPM_REQUIRE(y_video && y_audio, LPM_ERR_BADARG, "lpm_frame_apply_split_idx_q8: bad pointers");
    return launch_frame_apply(q8_src(q, inv_norm, max_quantized_value, min_quantized_value), TableIdx{frame_index}, B, max_frames, F, S, scale,
                              shift, y_video, y_audio, Dv, (hipStream_t)stream, "lpm_frame_apply_split_idx_q8", centre);
}

extern "C" int lpm_frame_bn_bwd_split_idx(const float* dy_video, int64_t ldv, const float* dy_audio, int64_t lda, int Dv, const float* raw,
                                          const int32_t* frame_index, int B, int max_frames, int F, int S, const float* mean,
                                          const float* var, float eps, float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes,
                                          lpm_stream_t stream) {
    LPM_FRAME_IDX_CHECK("lpm_frame_bn_bwd_split_idx");
    LPM_REQUIRE(dy_audio, LPM_ERR_BADARG, "lpm_frame_bn_bwd_split_idx: bad pointers / strides");
    return launch_frame_bn_bwd(dy_video, ldv, dy_audio, lda, Dv, FrameSrc<float>{raw}, TableIdx{frame_index}, B, max_frames, F, S, mean, var,
                               eps, dgamma, dbeta, workspace, workspace_bytes, (hipStream_t)stream, "lpm_frame_bn_bwd_split_idx");
}
extern "C" int lpm_frame_bn_bwd_split_idx_q8(const float* dy_video, int64_t ldv, const float* dy_audio, int64_t lda, int Dv,
                                             const unsigned char* q, const float* inv_norm, float max_quantized_value,
                                             float min_quantized_value, const int32_t* frame_index, int B, int max_frames, int F, int S,
                                             const float* mean, const float* var, float eps, float* dgamma, float* dbeta, void* workspace,
                                             size_t workspace_bytes, lpm_stream_t stream) {
    LPM_FRAME_Q8_IDX_CHECK("lpm_frame_bn_bwd_split_idx_q8");
    LPM_REQUIRE(dy_audio, LPM_ERR_BADARG, "lpm_frame_bn_bwd_split_idx_q8: bad pointers / strides");
    return launch_frame_bn_bwd(dy_video, ldv, dy_audio, lda, Dv, q8_src(q, inv_norm, max_quantized_value, min_quantized_value),
                               TableIdx{frame_index}, B, max_frames, F, S, mean, var, eps, dgamma, dbeta, workspace, workspace_bytes,
                               (hipStream_t)stream, "lpm_frame_bn_bwd_split_idx_q8");
}

extern "C" int lpm_l2_normalize_rows(const float* x, int64_t rows, int F, float* y, lpm_stream_t stream) {
    using namespace lpm;
    LPM_REQUIRE(x && y, LPM_ERR_BADARG, "lpm_l2_normalize_rows: null pointer");
    LPM_REQUIRE(rows > 0 && F > 0 && F % 4 == 0 && F <= 2048 && (((uintptr_t)x | (uintptr_t)y) & 15) == 0, LPM_ERR_UNSUPPORTED_SHAPE,
                "lpm_l2_normalize_rows: need F %% 4 == 0, F <= 2048, 16-byte aligned pointers (F=%d)", F);
    const int64_t want = (rows + 3) / 4;
    hipLaunchKernelGGL(l2_normalize_rows_kernel, dim3((unsigned)(want < 16384 ? want : 16384)), dim3(256), 0, (hipStream_t)stream, x, rows,
                       F, y);
    return check_launch("lpm_l2_normalize_rows");
}

extern "C" int lpm_dequantize_l2_normalize(const unsigned char* q, const int32_t* num_frames, int B, int max_frames, int F,
                                           float max_quantized_value, float min_quantized_value, float* y, lpm_stream_t stream) {
    using namespace lpm;
    LPM_REQUIRE(q && num_frames && y, LPM_ERR_BADARG, "lpm_dequantize_l2_normalize: null pointer");
    LPM_REQUIRE(max_quantized_value > min_quantized_value, LPM_ERR_BADARG, "lpm_dequantize_l2_normalize: empty quantisation range");
    LPM_REQUIRE(B > 0 && max_frames > 0 && F > 0 && F % 4 == 0 && F <= 2048 && (((uintptr_t)q & 3) | ((uintptr_t)y & 15)) == 0,
                LPM_ERR_UNSUPPORTED_SHAPE, "lpm_dequantize_l2_normalize: need F %% 4 == 0, F <= 2048, aligned pointers (F=%d)", F);
    const float range = max_quantized_value - min_quantized_value;
    const float scalar = range / 255.0f, bias = range / 512.0f + min_quantized_value;
    const int64_t rows = (int64_t)B * max_frames, want = (rows + 3) / 4;
    hipLaunchKernelGGL(dequantize_l2_normalize_kernel, dim3((unsigned)(want < 16384 ? want : 16384)), dim3(256), 0, (hipStream_t)stream, q,
                       num_frames, rows, max_frames, F, scalar, bias, y);
    return check_launch("lpm_dequantize_l2_normalize");
}
