// HingeLoss and SoftmaxLoss of the predictions (losses.py:54-69, :72-96), whichever head made them: one row reduction forward, one
// element-wise pass backward.  predictions fp32 [B, V] contiguous; labels ONE BYTE per element (bool / uint8, nonzero = positive), read
// as they are -- no fp32 copy of the labels exists.
//   hinge    s = 2 y - 1:  row loss = sum_j max(0, b - s_j p_j);                       d/dp_j = -s_j where b - s_j p_j > 0 STRICTLY, else 0
//            (tf.maximum(zeros, .): MaximumGrad hands a tie to its first argument).  s p is exact, so the fp32 difference b - s p is zero
//            exactly when the exact one is: the mask is the fp64 mask at every element.
//   softmax  cnt = sum_j y_j, n = y / max(cnt, 1e-7):  row loss = -sum_j n_j log softmax(p)_j = [cnt > 0] (lse - sum_{y_j} p_j / cnt),
//            lse = max + log sum_j exp(p_j - max);                                     d/dp_j = [cnt > 0] softmax(p)_j - n_j
//            A row without labels gives exactly 0 both ways (no 0 * -inf is ever formed).
//   loss = mean over the rows; the backward scales by dloss / B.
// Forward: a workgroup per row, grid stride over the rows.  Every thread walks its strided share of the row once (the softmax keeps a
// running maximum and rescales its running sum: no second read), the 64 lanes meet by shuffles, the four waves through LDS, thread 0
// adds them in wave order: no floating-point atomics, the same inputs give the same bits.  A second one-workgroup launch adds the row
// losses in a fixed order (fp64) into the batch mean.
// Wide loads: element e = row * V + column of a CONTIGUOUS matrix sits at byte 4 e of the predictions and byte e of the labels, so with
// the predictions' base on 16 bytes and the labels' on 4, every group of four elements with e % 4 == 0 is one 16-byte and one 4-byte
// load whatever V is (rows of V = 3862 floats start on 8-byte boundaries, of V = 257 on 4-byte ones: a row's first e % 4 and last
// elements outside its aligned groups are read one by one).  Other bases take the element-by-element kernels.
#include "lpm_common.h"

namespace lpm {

constexpr int LL_THREADS = 256;
constexpr int LL_MAX_GRID_ROWS = 1024;        // forward: workgroups per launch (256 CUs x 4); more rows -> grid stride
constexpr int LL_MAX_GRID_ELEMS = 2048;       // backward

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// one thread's share of a row
template <int KIND>
struct RowAcc;
template <>
struct RowAcc<LPM_LABEL_LOSS_HINGE> {
    float h = 0.f;
    __device__ __forceinline__ void add(float p, bool y, float b) {
        const float m = y ? b - p : b + p;                 // b - s p, s = +-1
        h += m > 0.f ? m : 0.f;
    }
    __device__ __forceinline__ void add4(f32x4 p, uint32_t y4, float b) {
#pragma unroll
        for (int u = 0; u < 4; ++u) add(p[u], ((y4 >> (8 * u)) & 0xFFu) != 0, b);
    }
};
template <>
struct RowAcc<LPM_LABEL_LOSS_SOFTMAX> {
    float m = -INFINITY, s = 0.f;                          // running maximum, sum of exp(p - m)
    double sp = 0.0;                                       // sum of the positives' predictions (few terms; fp64 keeps lse - sp / cnt exact)
    int cnt = 0;
    __device__ __forceinline__ void raise(float top) {
        if (top > m) {
            s *= expf(m - top);                            // (first element: 0 * exp(-inf) = 0)
            m = top;
        }
    }
    __device__ __forceinline__ void take(float p, bool y) {
        s += expf(p - m);
        if (y) {
            sp += (double)p;
            ++cnt;
        }
    }
    __device__ __forceinline__ void add(float p, bool y, float) {
        raise(p);
        take(p, y);
    }
    __device__ __forceinline__ void add4(f32x4 p, uint32_t y4, float) {
        raise(fmaxf(fmaxf(p[0], p[1]), fmaxf(p[2], p[3])));
#pragma unroll
        for (int u = 0; u < 4; ++u) take(p[u], ((y4 >> (8 * u)) & 0xFFu) != 0);
    }
};

template <int KIND, bool VEC>
__global__ __launch_bounds__(LL_THREADS) void label_loss_fwd_kernel(const float* __restrict__ pred, const uint8_t* __restrict__ lab, int B,
                                                                    int V, float b, float* __restrict__ row_state,
                                                                    float* __restrict__ row_loss) {
    __shared__ float sh_f[2][4];
    __shared__ double sh_d[4];
    __shared__ int sh_i[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int r = blockIdx.x; r < B; r += gridDim.x) {
        const int64_t e0 = (int64_t)r * V, e1 = e0 + V;
        // [e0, v0) one by one, [v0, v1) in aligned groups of four, [v1, e1) one by one
        const int64_t v0 = VEC ? min((e0 + 3) & ~(int64_t)3, e1) : e1;
        const int64_t v1 = VEC ? max(v0, e1 & ~(int64_t)3) : e1;
        RowAcc<KIND> acc;
        for (int64_t e = e0 + tid; e < v0; e += LL_THREADS) acc.add(pred[e], lab[e] != 0, b);
        for (int64_t e = v0 + 4 * (int64_t)tid; e < v1; e += 4 * LL_THREADS)
            acc.add4(*reinterpret_cast<const f32x4*>(pred + e), *reinterpret_cast<const uint32_t*>(lab + e), b);
        for (int64_t e = v1 + tid; e < e1; e += LL_THREADS) acc.add(pred[e], lab[e] != 0, b);

        if constexpr (KIND == LPM_LABEL_LOSS_HINGE) {
            const float w = wave_sum(acc.h);
            if (lane == 0) sh_f[0][wave] = w;
            __syncthreads();
            if (tid == 0) row_loss[r] = ((sh_f[0][0] + sh_f[0][1]) + sh_f[0][2]) + sh_f[0][3];
        } else {
            const float wm = wave_max(acc.m);
            if (lane == 0) sh_f[0][wave] = wm;
            __syncthreads();
            const float M = fmaxf(fmaxf(sh_f[0][0], sh_f[0][1]), fmaxf(sh_f[0][2], sh_f[0][3]));
            const float s = acc.m == M ? acc.s : acc.s * expf(acc.m - M);     // (a thread without elements: s = 0)
            const float ws = wave_sum(s);
            const double wp = wave_sum_f64(acc.sp);
            const int wc = wave_sum_i32(acc.cnt);
            if (lane == 0) {
                sh_f[1][wave] = ws;
                sh_d[wave] = wp;
                sh_i[wave] = wc;
            }
            __syncthreads();
            if (tid == 0) {
                const float S = ((sh_f[1][0] + sh_f[1][1]) + sh_f[1][2]) + sh_f[1][3];
                const double sp = ((sh_d[0] + sh_d[1]) + sh_d[2]) + sh_d[3];
                const int cnt = sh_i[0] + sh_i[1] + sh_i[2] + sh_i[3];
                const double lse = (double)M + log((double)S);
                row_state[3 * (int64_t)r] = M;
                row_state[3 * (int64_t)r + 1] = S;
                row_state[3 * (int64_t)r + 2] = (float)cnt;
                row_loss[r] = cnt > 0 ? (float)(lse - sp / (double)cnt) : 0.f;
            }
        }
        __syncthreads();                                   // the next row reuses the LDS slots
    }
}

// loss = (sum of the row losses, in a fixed order, fp64) / B
__global__ __launch_bounds__(LL_THREADS) void label_loss_mean_kernel(const float* __restrict__ row_loss, int B, float* __restrict__ loss) {
    __shared__ double sh[4];
    double s = 0.0;
    for (int r = threadIdx.x; r < B; r += LL_THREADS) s += (double)row_loss[r];
    s = wave_sum_f64(s);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) loss[0] = (float)((((sh[0] + sh[1]) + sh[2]) + sh[3]) / (double)B);
}

// the row an element's gradient needs: nothing for the hinge; the maximum, 1 / sum exp(p - maximum) and 1 / cnt for the softmax.
// softmax(p)_j = exp(p_j - max) / sum: the log-sum-exp stays in its two parts, because exp(p_j - fp32(lse)) would carry lse's rounding
// (2e-6 of the value at lse = 32) into the row's largest entries, where p_j - max is small and exact.
template <int KIND>
struct RowGrad {
    float top = 0.f, inv_sum = 0.f, inv = 0.f;
    bool any = false;
    __device__ __forceinline__ void load(const float* __restrict__ row_state, int64_t r) {
        if constexpr (KIND == LPM_LABEL_LOSS_SOFTMAX) {
            top = row_state[3 * r];
            inv_sum = 1.f / row_state[3 * r + 1];
            const float cnt = row_state[3 * r + 2];
            any = cnt > 0.f;
            inv = any ? 1.f / cnt : 0.f;
        }
    }
    __device__ __forceinline__ float grad(float p, bool y, float b, float scale) const {
        if constexpr (KIND == LPM_LABEL_LOSS_HINGE) {
            const float m = y ? b - p : b + p;
            return m > 0.f ? (y ? -scale : scale) : 0.f;
        } else {
            return any ? (expf(p - top) * inv_sum - (y ? inv : 0.f)) * scale : 0.f;
        }
    }
};

template <int KIND, bool VEC>
__global__ __launch_bounds__(LL_THREADS) void label_loss_bwd_kernel(const float* __restrict__ pred, const uint8_t* __restrict__ lab,
                                                                    const float* __restrict__ row_state, const float* __restrict__ dloss,
                                                                    int64_t n, int V, int B, float b, float* __restrict__ dpred) {
    const float scale = dloss[0] / (float)B;
    const int64_t first = (int64_t)blockIdx.x * LL_THREADS + threadIdx.x, stride = (int64_t)gridDim.x * LL_THREADS;
    const int64_t ngroups = VEC ? n >> 2 : 0;
    const bool small = n <= (int64_t)INT32_MAX;            // (wave-uniform: the 32-bit division where it is enough)
    RowGrad<KIND> row;
    for (int64_t g = first; g < ngroups; g += stride) {
        const int64_t e = g << 2;
        const f32x4 p = *reinterpret_cast<const f32x4*>(pred + e);
        const uint32_t y4 = *reinterpret_cast<const uint32_t*>(lab + e);
        int64_t r = small ? (int64_t)((uint32_t)e / (uint32_t)V) : e / V;
        int c = (int)(e - r * V);
        row.load(row_state, r);
        f32x4 o;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (c == V) {                                  // the group runs into the next row
                c = 0;
                ++r;
                row.load(row_state, r);
            }
            o[u] = row.grad(p[u], ((y4 >> (8 * u)) & 0xFFu) != 0, b, scale);
            ++c;
        }
        *reinterpret_cast<f32x4*>(dpred + e) = o;
    }
    for (int64_t e = 4 * ngroups + first; e < n; e += stride) {
        const int64_t r = small ? (int64_t)((uint32_t)e / (uint32_t)V) : e / V;
        row.load(row_state, r);
        dpred[e] = row.grad(pred[e], lab[e] != 0, b, scale);
    }
}

static bool label_loss_kind_ok(int kind) { return kind == LPM_LABEL_LOSS_HINGE || kind == LPM_LABEL_LOSS_SOFTMAX; }
static bool label_loss_wide(const void* f32a, const void* f32b, const void* bytes) {
    return (uintptr_t)f32a % 16 == 0 && (uintptr_t)f32b % 16 == 0 && (uintptr_t)bytes % 4 == 0;
}

}  // namespace lpm

extern "C" int lpm_label_loss_fwd(int kind, const float* predictions, const uint8_t* labels, int B, int V, float b, float* row_state,
                                  float* row_loss, float* loss, lpm_stream_t stream) {
    using namespace lpm;
    LPM_REQUIRE(label_loss_kind_ok(kind), LPM_ERR_BADARG, "lpm_label_loss_fwd: kind must be %d (hinge) or %d (softmax), got %d",
                LPM_LABEL_LOSS_HINGE, LPM_LABEL_LOSS_SOFTMAX, kind);
    LPM_REQUIRE(predictions && labels && row_loss && loss, LPM_ERR_BADARG, "lpm_label_loss_fwd: null pointer");
    LPM_REQUIRE(kind != LPM_LABEL_LOSS_SOFTMAX || row_state, LPM_ERR_BADARG, "lpm_label_loss_fwd: the softmax kind needs row_state [B, 3]");
    LPM_REQUIRE(B >= 1 && V >= 1, LPM_ERR_UNSUPPORTED_SHAPE, "lpm_label_loss_fwd: need B >= 1 and V >= 1 (got %d, %d)", B, V);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(B < LL_MAX_GRID_ROWS ? B : LL_MAX_GRID_ROWS), block(LL_THREADS);
    const bool wide = label_loss_wide(predictions, predictions, labels);
#define LPM_LL_FWD(KIND, VEC) \
    hipLaunchKernelGGL((label_loss_fwd_kernel<KIND, VEC>), grid, block, 0, s, predictions, labels, B, V, b, row_state, row_loss)
    if (kind == LPM_LABEL_LOSS_HINGE) {
        if (wide) LPM_LL_FWD(LPM_LABEL_LOSS_HINGE, true);
        else LPM_LL_FWD(LPM_LABEL_LOSS_HINGE, false);
    } else {
        if (wide) LPM_LL_FWD(LPM_LABEL_LOSS_SOFTMAX, true);
        else LPM_LL_FWD(LPM_LABEL_LOSS_SOFTMAX, false);
    }
#undef LPM_LL_FWD
    hipLaunchKernelGGL(label_loss_mean_kernel, dim3(1), block, 0, s, row_loss, B, loss);
    return check_launch("lpm_label_loss_fwd");
}

extern "C" int lpm_label_loss_bwd(int kind, const float* predictions, const uint8_t* labels, const float* row_state, const float* dloss,
                                  int B, int V, float b, float* dpredictions, lpm_stream_t stream) {
    using namespace lpm;
    LPM_REQUIRE(label_loss_kind_ok(kind), LPM_ERR_BADARG, "lpm_label_loss_bwd: kind must be %d (hinge) or %d (softmax), got %d",
                LPM_LABEL_LOSS_HINGE, LPM_LABEL_LOSS_SOFTMAX, kind);
    LPM_REQUIRE(predictions && labels && dloss && dpredictions, LPM_ERR_BADARG, "lpm_label_loss_bwd: null pointer");
    LPM_REQUIRE(kind != LPM_LABEL_LOSS_SOFTMAX || row_state, LPM_ERR_BADARG, "lpm_label_loss_bwd: the softmax kind needs row_state [B, 3]");
    LPM_REQUIRE(B >= 1 && V >= 1, LPM_ERR_UNSUPPORTED_SHAPE, "lpm_label_loss_bwd: need B >= 1 and V >= 1 (got %d, %d)", B, V);
    hipStream_t s = (hipStream_t)stream;
    const int64_t n = (int64_t)B * V;
    const bool wide = label_loss_wide(predictions, dpredictions, labels);
    const int64_t work = wide ? (n + 3) / 4 : n;           // threads' worth of work
    const int64_t nblk = (work + LL_THREADS - 1) / LL_THREADS;
    const dim3 grid((unsigned)(nblk < LL_MAX_GRID_ELEMS ? nblk : LL_MAX_GRID_ELEMS)), block(LL_THREADS);
#define LPM_LL_BWD(KIND, VEC)                                                                                                        \
    hipLaunchKernelGGL((label_loss_bwd_kernel<KIND, VEC>), grid, block, 0, s, predictions, labels, row_state, dloss, n, V, B, b, \
                       dpredictions)
    if (kind == LPM_LABEL_LOSS_HINGE) {
        if (wide) LPM_LL_BWD(LPM_LABEL_LOSS_HINGE, true);
        else LPM_LL_BWD(LPM_LABEL_LOSS_HINGE, false);
    } else {
        if (wide) LPM_LL_BWD(LPM_LABEL_LOSS_SOFTMAX, true);
        else LPM_LL_BWD(LPM_LABEL_LOSS_SOFTMAX, false);
    }
#undef LPM_LL_BWD
    return check_launch("lpm_label_loss_bwd");
}
