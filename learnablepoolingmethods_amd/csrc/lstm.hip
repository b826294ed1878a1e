// One layer of TF1's BasicLSTMCell(H, forget_bias) under tf.nn.dynamic_rnn(sequence_length=...): the recurrent half of every time step
// as ONE kernel each way.  The products that do not depend on the recurrence (X Wx before the loop, dX = dZ Wx^T and
// dkernel = [X ; H_prev]^T dZ after it) are ordinary large GEMMs of the caller's; what is left per step is a skinny product
// [B, H] x [H, 4H] (forward) or [B, 4H] x [4H, H] (backward) followed by gate arithmetic that is element-wise in the hidden unit.
//   z = xw[:, t] + h_{t-1} Wh + bias,  columns gate-major  i | j | f | o,  each H wide
//   c' = c sigmoid(f + forget_bias) + sigmoid(i) tanh(j),   h' = tanh(c') sigmoid(o)
//   t >= min(lengths[b], T): the state is copied through and outputs[b, t] = 0 (a length of 0: zeros everywhere; above T: T)
// Forward step t (lstm_step_fwd_kernel): a workgroup owns a slice of 16 P hidden units (P = 1 or 2 per lane) and a tile of 16 batch rows
// (rows past B are padded with zeros in registers, nothing past B is read or written).  Its eight waves split the reduction over H; each
// forms the slice's FOUR gate column blocks on v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulation), the eight partial tiles
// meet in LDS and are added in wave order.  The epilogue adds the xw row and the bias, applies the gates and the length mask and writes
// c_t, h_t, the output row and the ACTIVATED gates (sigmoid(i), tanh(j), sigmoid(f + forget_bias), sigmoid(o)) for the backward: no
// pre-activation reaches memory.
// Backward step s (lstm_step_bwd_kernel): a workgroup owns 16 hidden units and 16 rows.  It forms dh_s = dZ_{s+1} Wh^T for them (the
// reduction over 4H split over the eight waves, both operands read as 16-byte runs along the reduction), adds the carried gradient of
// masked steps and d outputs[:, s], does step s's gate arithmetic with the carried dc and writes dZ_s.  dc and the pass-through dh are
// [B, H] buffers every element of which is read and written by the one thread that owns it.
// The MFMA's four reduction slots of a lane group q = lane >> 4 hold k = k0 + 4 q + s in step s = 0 .. 3 (not k0 + 4 s + q): the A row of
// a lane is then ONE 16-byte load per 16 reduction steps.  Which k a slot holds is free as long as both operands agree.
// Steps are ordered by the stream alone: one launch per step, h double-buffered by time (hs [B, T + 1, H]); no grid-wide barrier, no
// cooperative launch, no spin wait.  No atomics: the same inputs give the same bits.
// The row tiles of one slice are neighbours in the grid (blockIdx.x), so that they read the slice's weights at about the same time.
// Shapes: H % 128 == 0 (eight waves x 16 reduction steps), H <= 2^19, any B >= 1, T >= 1; Wh's rows ldw floats apart, its base on 16 bytes.
#include "lpm_common.h"

namespace lpm {

constexpr int LSTM_WAVES = 8;
constexpr int LSTM_THREADS = 64 * LSTM_WAVES;
constexpr int LSTM_ROWS = 16;              // batch rows per workgroup (one MFMA tile)
constexpr int LSTM_WIDE_MIN_H = 2048;      // from here a forward slice is 32 units: 128-byte runs of every Wh row

__device__ __forceinline__ float lstm_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

template <int P>
__global__ __launch_bounds__(LSTM_THREADS) void lstm_step_fwd_kernel(const float* __restrict__ xw, const float* __restrict__ wh, int64_t ldw,
                                                                     const float* __restrict__ bias, const int* __restrict__ lengths,
                                                                     float* __restrict__ hs, float* __restrict__ cs,
                                                                     float* __restrict__ gates, float* __restrict__ outputs, int B, int T,
                                                                     int H, int t, float forget_bias) {
    constexpr int U = 16 * P;
    __shared__ float sh[LSTM_WAVES][4][P][256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 15, q = lane >> 4;
    const int u0 = blockIdx.y * U, row0 = blockIdx.x * LSTM_ROWS;
    const bool row_ok = row0 + j < B;
    const float* hrow = hs + ((int64_t)min(row0 + j, B - 1) * (T + 1) + t) * H;
    f32x4 acc[4][P];
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int p = 0; p < P; ++p) acc[g][p] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (t > 0) {                            // h_0 = 0: the product is zero
        const int kper = H / LSTM_WAVES, kbeg = wave * kper;
#pragma unroll 2
        for (int kb = kbeg; kb < kbeg + kper; kb += 16) {
            float4 a4 = *reinterpret_cast<const float4*>(hrow + kb + 4 * q);
            if (!row_ok) a4 = make_float4(0.f, 0.f, 0.f, 0.f);
            const float a[4] = {a4.x, a4.y, a4.z, a4.w};
            const float* wrow = wh + (int64_t)(kb + 4 * q) * ldw + u0 + P * j;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    if constexpr (P == 1) {
                        acc[g][0] = mfma16(a[s], wrow[s * ldw + (int64_t)g * H], acc[g][0]);
                    } else {
                        const float2 b2 = *reinterpret_cast<const float2*>(wrow + s * ldw + (int64_t)g * H);
                        acc[g][0] = mfma16(a[s], b2.x, acc[g][0]);
                        acc[g][1] = mfma16(a[s], b2.y, acc[g][1]);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int p = 0; p < P; ++p)
#pragma unroll
            for (int r = 0; r < 4; ++r) sh[wave][g][p][(4 * q + r) * 16 + j] = acc[g][p][r];
    __syncthreads();
    for (int e = threadIdx.x; e < LSTM_ROWS * U; e += LSTM_THREADS) {
        const int ri = e / U, uu = e % U, b = row0 + ri;
        if (b >= B) continue;
        const int idx = ri * 16 + uu / P, p = uu % P, u = u0 + uu;
        float z[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            float s = sh[0][g][p][idx];
#pragma unroll
            for (int w = 1; w < LSTM_WAVES; ++w) s += sh[w][g][p][idx];
            z[g] = s + xw[((int64_t)b * T + t) * 4 * H + (int64_t)g * H + u] + bias[(int64_t)g * H + u];
        }
        const float gi = lstm_sigmoid(z[0]), gj = tanhf(z[1]), gf = lstm_sigmoid(z[2] + forget_bias), go = lstm_sigmoid(z[3]);
        const int64_t st = ((int64_t)b * (T + 1) + t) * H + u;
        const float c_prev = cs[st], h_prev = hs[st];
        const float c_new = c_prev * gf + gi * gj;
        const float h_new = tanhf(c_new) * go;
        const bool valid = t < min(lengths[b], T);
        cs[st + H] = valid ? c_new : c_prev;
        hs[st + H] = valid ? h_new : h_prev;
        outputs[((int64_t)b * T + t) * H + u] = valid ? h_new : 0.f;
        float* gp = gates + ((int64_t)b * T + t) * 4 * H + u;
        gp[0] = gi;
        gp[(int64_t)H] = gj;
        gp[(int64_t)2 * H] = gf;
        gp[(int64_t)3 * H] = go;
    }
}

// dz_next: dZ_{s+1} (the [B, T, 4H] buffer; read only when s + 1 < T).  g_out may be null (no gradient reached the outputs).
__global__ __launch_bounds__(LSTM_THREADS) void lstm_step_bwd_kernel(const float* __restrict__ wh, int64_t ldw, const int* __restrict__ lengths,
                                                                     const float* __restrict__ cs, const float* __restrict__ gates,
                                                                     const float* __restrict__ g_out, float* __restrict__ dhp,
                                                                     float* __restrict__ dc, float* dz, int B, int T, int H, int s) {
    __shared__ float sh[LSTM_WAVES][256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 15, q = lane >> 4;
    const int u0 = blockIdx.y * 16, row0 = blockIdx.x * LSTM_ROWS;
    const bool rec = s + 1 < T;
    if (rec) {
        const bool row_ok = row0 + j < B;
        const float* arow = dz + ((int64_t)min(row0 + j, B - 1) * T + s + 1) * 4 * H;
        const float* wrow = wh + (int64_t)(u0 + j) * ldw;
        f32x4 acc0 = f32x4{0.f, 0.f, 0.f, 0.f}, acc1 = acc0;       // two chains: a dependent 16x16x4 MFMA waits 40 cycles, an independent one 32
        const int kper = 4 * H / LSTM_WAVES, kbeg = wave * kper;  // (kper = H / 2: a multiple of 64)
        for (int kb = kbeg; kb < kbeg + kper; kb += 64) {
            float4 a4[4], b4[4];
#pragma unroll
            for (int v = 0; v < 4; ++v) {                         // all eight loads of a round before its MFMAs
                a4[v] = *reinterpret_cast<const float4*>(arow + kb + 16 * v + 4 * q);
                b4[v] = *reinterpret_cast<const float4*>(wrow + kb + 16 * v + 4 * q);
            }
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                if (!row_ok) a4[v] = make_float4(0.f, 0.f, 0.f, 0.f);
                acc0 = mfma16(a4[v].x, b4[v].x, acc0);
                acc1 = mfma16(a4[v].y, b4[v].y, acc1);
                acc0 = mfma16(a4[v].z, b4[v].z, acc0);
                acc1 = mfma16(a4[v].w, b4[v].w, acc1);
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) sh[wave][(4 * q + r) * 16 + j] = acc0[r] + acc1[r];
    }
    __syncthreads();
    const int e = threadIdx.x;
    if (e >= 256) return;
    const int ri = e >> 4, b = row0 + ri, u = u0 + (e & 15);
    if (b >= B) return;
    float dh = 0.f;
    if (rec) {
        dh = sh[0][e];
#pragma unroll
        for (int w = 1; w < LSTM_WAVES; ++w) dh += sh[w][e];
    }
    const int64_t bu = (int64_t)b * H + u;
    dh += dhp[bu];
    float* zp = dz + ((int64_t)b * T + s) * 4 * H + u;
    if (s < min(lengths[b], T)) {
        if (g_out) dh += g_out[((int64_t)b * T + s) * H + u];
        const float* gp = gates + ((int64_t)b * T + s) * 4 * H + u;
        const float gi = gp[0], gj = gp[(int64_t)H], gf = gp[(int64_t)2 * H], go = gp[(int64_t)3 * H];
        const int64_t st = ((int64_t)b * (T + 1) + s) * H + u;
        const float c_prev = cs[st], tc = tanhf(cs[st + H]);
        const float dcs = dc[bu] + dh * go * (1.f - tc * tc);
        zp[0] = dcs * gj * gi * (1.f - gi);
        zp[(int64_t)H] = dcs * gi * (1.f - gj * gj);
        zp[(int64_t)2 * H] = dcs * c_prev * gf * (1.f - gf);
        zp[(int64_t)3 * H] = dh * tc * go * (1.f - go);
        dc[bu] = dcs * gf;
        dhp[bu] = 0.f;
    } else {                                // the state was copied through: so are its gradients
        zp[0] = 0.f;
        zp[(int64_t)H] = 0.f;
        zp[(int64_t)2 * H] = 0.f;
        zp[(int64_t)3 * H] = 0.f;
        dhp[bu] = dh;
    }
}

static int lstm_check(const char* what, const void* wh, int64_t ldw, int B, int T, int H) {
    LPM_REQUIRE(B >= 1 && T >= 1 && H >= 1, LPM_ERR_BADARG, "%s: need B, T, H >= 1 (got %d, %d, %d)", what, B, T, H);
    LPM_REQUIRE(lpm_lstm_supported(B, T, H), LPM_ERR_UNSUPPORTED_SHAPE, "%s: the hidden size must be a multiple of 128 (got %d)", what, H);
    LPM_REQUIRE(ldw >= 4 * (int64_t)H && ldw % 4 == 0 && ((uintptr_t)wh & 15) == 0, LPM_ERR_BADARG,
                "%s: the recurrent weights need a base on 16 bytes and rows ldw >= 4 H floats apart, ldw a multiple of 4", what);
    return LPM_OK;
}

}  // namespace lpm

extern "C" int lpm_lstm_supported(int B, int T, int H) { return B >= 1 && T >= 1 && H >= 128 && H % 128 == 0 && H <= (1 << 19); }

extern "C" int lpm_lstm_layer_fwd(const float* xw, const float* wh, int64_t ldw, const float* bias, const int* lengths, int B, int T, int H,
                                  float forget_bias, float* hs, float* cs, float* gates, float* outputs, lpm_stream_t stream) {
    using namespace lpm;
    LPM_REQUIRE(xw && wh && bias && lengths && hs && cs && gates && outputs, LPM_ERR_BADARG, "lpm_lstm_layer_fwd: null pointer");
    if (int rc = lstm_check("lpm_lstm_layer_fwd", wh, ldw, B, T, H)) return rc;
    LPM_REQUIRE((((uintptr_t)hs | (uintptr_t)cs) & 15) == 0, LPM_ERR_BADARG, "lpm_lstm_layer_fwd: hs and cs need a base on 16 bytes");
    hipStream_t s = (hipStream_t)stream;
    const bool wide = H >= LSTM_WIDE_MIN_H;
    const dim3 grid((B + LSTM_ROWS - 1) / LSTM_ROWS, H / (wide ? 32 : 16)), block(LSTM_THREADS);
    for (int t = 0; t < T; ++t) {
        if (wide)
            hipLaunchKernelGGL(lstm_step_fwd_kernel<2>, grid, block, 0, s, xw, wh, ldw, bias, lengths, hs, cs, gates, outputs, B, T, H, t,
                               forget_bias);
        else
            hipLaunchKernelGGL(lstm_step_fwd_kernel<1>, grid, block, 0, s, xw, wh, ldw, bias, lengths, hs, cs, gates, outputs, B, T, H, t,
                               forget_bias);
    }
    return check_launch("lpm_lstm_layer_fwd");
}

extern "C" int lpm_lstm_layer_bwd(const float* wh, int64_t ldw, const int* lengths, const float* cs, const float* gates, const float* g_out,
                                  float* dhp, float* dc, float* dz, int B, int T, int H, lpm_stream_t stream) {
    using namespace lpm;
    LPM_REQUIRE(wh && lengths && cs && gates && dhp && dc && dz, LPM_ERR_BADARG, "lpm_lstm_layer_bwd: null pointer");
    if (int rc = lstm_check("lpm_lstm_layer_bwd", wh, ldw, B, T, H)) return rc;
    LPM_REQUIRE(((uintptr_t)dz & 15) == 0, LPM_ERR_BADARG, "lpm_lstm_layer_bwd: dz needs a base on 16 bytes");
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((B + LSTM_ROWS - 1) / LSTM_ROWS, H / 16), block(LSTM_THREADS);
    for (int t = T - 1; t >= 0; --t)
        hipLaunchKernelGGL(lstm_step_bwd_kernel, grid, block, 0, s, wh, ldw, lengths, cs, gates, g_out, dhp, dc, dz, B, T, H, t);
    return check_launch("lpm_lstm_layer_bwd");
}
