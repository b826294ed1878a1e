// The batch statistics of the evaluation loop behind lpm_eval_rows (DeviceEvaluationMetrics.accumulate, eval.py:254-262): ONE launch turns the
// batch's row outputs and its labels into
//   batch [4] fp64     mean of hit1 | mean over the rows of hits_at_n / num_labels (0 where num_labels == 0) | mean loss | B
//   sum_loss [1] fp64  += mean loss * B          (a product, then a sum: two roundings, what the torch route does)
//   class_pos [V] i64  += the column sums of the labels
// Row statistics: workgroup 0 alone.  Every thread takes the rows tid, tid + 256, ... (hit1 as an integer count, the other two in fp64), the 64
// lanes meet by a butterfly, the four waves through LDS, thread 0 adds them in wave order: a fixed order, no floating-point atomics, the same
// inputs give the same bits.  The mean loss is the mean of loss_row or, when the caller hands one over (a losses.BaseLoss value: one fp32 or fp64
// number on the device), that number itself, bit for bit.
// Labels: every workgroup walks its share of the flat byte range once (eval_batch_walk.h: the head bytes up to the first 16-byte boundary, aligned
// 16-byte loads, the tail bytes; any base address, any V).  A YT8M row holds about three positives in 3862 bytes, so a 16-byte group is looked at
// closer only when it is not all zero.  Positives are counted with INTEGER atomics (exact, order-free):
//   V <= 4096   into a 16 KiB int32 image of the columns in LDS; afterwards one 64-bit global atomic per nonzero counter.  At most 256
//               workgroups, so at label density 1 a column of class_pos takes at most 256 adds instead of B.
//   V >  4096   straight into class_pos (up to V = 65536 an int32 image would take 256 KiB, more than a CU's 160 KiB of LDS).
// A global counter that B rows add to is a same-address atomic (about 90 adds per microsecond per address); real labels add three per row.
#include "lpm_common.h"
#include "eval_batch_walk.h"

namespace lpm {

constexpr int EBS_THREADS = 256;
constexpr int EBS_MAX_V = 65536;            // lpm_eval_rows' limit
constexpr int EBS_LDS_V = 4096;             // columns of the LDS image
constexpr int EBS_GRID_LDS = 256;           // one workgroup per CU
constexpr int EBS_GRID_GLOBAL = 1024;

__device__ __forceinline__ double ebs_wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ int ebs_wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// s + a * b with the product rounded on its own, never one fused multiply-add: the torch route's two operations
__device__ __forceinline__ double ebs_add_product(double s, double a, double b) {
#pragma clang fp contract(off)
    const double ab = a * b;
    return s + ab;
}

// given_kind: 0 = the mean of loss_row, 1 = *given_loss is a float, 2 = a double
template <bool LDS_IMAGE>
__global__ __launch_bounds__(EBS_THREADS) void eval_batch_stats_kernel(const unsigned char* __restrict__ hit1, const int32_t* __restrict__ num_labels,
                                                                       const int32_t* __restrict__ hits_at_n, const double* __restrict__ loss_row,
                                                                       const void* __restrict__ given_loss, int given_kind,
                                                                       const unsigned char* __restrict__ labels, EvalWalk walk, int B,
                                                                       double* __restrict__ batch, double* __restrict__ sum_loss,
                                                                       unsigned long long* __restrict__ class_pos) {
    __shared__ int image[LDS_IMAGE ? EBS_LDS_V : 1];
    __shared__ double red_d[2][4];
    __shared__ int red_i[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int V = walk.V;

    if constexpr (LDS_IMAGE) {
        for (int c = tid; c < V; c += EBS_THREADS) image[c] = 0;
        __syncthreads();
    }
    const int64_t worker = (int64_t)blockIdx.x * EBS_THREADS + tid, workers = (int64_t)gridDim.x * EBS_THREADS;
    eval_walk_worker(walk, labels, worker, workers, [&](int c) {
        if constexpr (LDS_IMAGE) atomicAdd(&image[c], 1);
        else atomicAdd(class_pos + c, 1ull);
    });
    if constexpr (LDS_IMAGE) {
        __syncthreads();
        for (int c = tid; c < V; c += EBS_THREADS) {
            const int cnt = image[c];
            if (cnt != 0) atomicAdd(class_pos + c, (unsigned long long)cnt);
        }
    }

    if (blockIdx.x != 0) return;
    int hits = 0;                                          // (B < 2^31 rows of 0 / 1)
    double perr = 0.0, loss = 0.0;
    for (int r = tid; r < B; r += EBS_THREADS) {
        hits += hit1[r] != 0;
        const int n = num_labels[r];
        if (n > 0) perr += (double)hits_at_n[r] / (double)n;
        if (given_kind == 0) loss += loss_row[r];
    }
    hits = ebs_wave_sum_i(hits);
    perr = ebs_wave_sum_d(perr);
    loss = ebs_wave_sum_d(loss);
    if (lane == 0) {
        red_i[wave] = hits;
        red_d[0][wave] = perr;
        red_d[1][wave] = loss;
    }
    __syncthreads();
    if (tid == 0) {
        const double rows = (double)B;
        const int h = red_i[0] + red_i[1] + red_i[2] + red_i[3];
        const double p = ((red_d[0][0] + red_d[0][1]) + red_d[0][2]) + red_d[0][3];
        double mean_loss;
        if (given_kind == 1) mean_loss = (double)*reinterpret_cast<const float*>(given_loss);
        else if (given_kind == 2) mean_loss = *reinterpret_cast<const double*>(given_loss);
        else mean_loss = (((red_d[1][0] + red_d[1][1]) + red_d[1][2]) + red_d[1][3]) / rows;
        batch[0] = (double)h / rows;
        batch[1] = p / rows;
        batch[2] = mean_loss;
        batch[3] = rows;
        sum_loss[0] = ebs_add_product(sum_loss[0], mean_loss, rows);
    }
}

}  // namespace lpm

extern "C" int lpm_eval_batch_stats(const unsigned char* hit1, const int32_t* num_labels, const int32_t* hits_at_n, const double* loss_row,
                                    const void* given_loss, int given_loss_is_f64, const unsigned char* labels, int B, int V, double* batch,
                                    double* sum_loss, int64_t* class_pos, lpm_stream_t stream) {
    using namespace lpm;
    LPM_REQUIRE(hit1 && num_labels && hits_at_n && labels && batch && sum_loss && class_pos, LPM_ERR_BADARG,
                "lpm_eval_batch_stats: null pointer");
    LPM_REQUIRE((loss_row != nullptr) != (given_loss != nullptr), LPM_ERR_BADARG,
                "lpm_eval_batch_stats: need exactly one of loss_row [B] and given_loss [1]");
    LPM_REQUIRE(B > 0 && V > 0 && V <= EBS_MAX_V, LPM_ERR_UNSUPPORTED_SHAPE, "lpm_eval_batch_stats: need B > 0 and 1 <= V <= %d (B=%d V=%d)",
                EBS_MAX_V, B, V);
    LPM_REQUIRE((uintptr_t)num_labels % 4 == 0 && (uintptr_t)hits_at_n % 4 == 0 && (uintptr_t)loss_row % 8 == 0 && (uintptr_t)batch % 8 == 0
                    && (uintptr_t)sum_loss % 8 == 0 && (uintptr_t)class_pos % 8 == 0
                    && (uintptr_t)given_loss % (given_loss_is_f64 ? 8 : 4) == 0,
                LPM_ERR_BADARG, "lpm_eval_batch_stats: a pointer is not aligned to its element size (the labels alone may start at any byte)");
    const EvalWalk walk = eval_walk_make((uintptr_t)labels, B, V);
    const bool image = V <= EBS_LDS_V;
    const int64_t want = (walk.nvec + EBS_THREADS - 1) / EBS_THREADS, cap = image ? EBS_GRID_LDS : EBS_GRID_GLOBAL;
    const dim3 grid((unsigned)(want < 1 ? 1 : want > cap ? cap : want)), block(EBS_THREADS);      // (head and tail: workers 0 .. 14 of workgroup 0)
    const int given_kind = given_loss ? (given_loss_is_f64 ? 2 : 1) : 0;
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* cp = reinterpret_cast<unsigned long long*>(class_pos);
    if (image)
        hipLaunchKernelGGL(eval_batch_stats_kernel<true>, grid, block, 0, st, hit1, num_labels, hits_at_n, loss_row, given_loss, given_kind,
                           labels, walk, B, batch, sum_loss, cp);
    else
        hipLaunchKernelGGL(eval_batch_stats_kernel<false>, grid, block, 0, st, hit1, num_labels, hits_at_n, loss_row, given_loss, given_kind,
                           labels, walk, B, batch, sum_loss, cp);
    return check_launch("lpm_eval_batch_stats");
}
