// Per-row evaluation metrics (eval.py's loop over eval_util.EvaluationMetrics.accumulate): for every row of fp32 predictions p [B, V] and
// uint8 labels y [B, V] (0 / 1) one workgroup writes
//   hit1       the label at the arg-max (ties: lowest index, NaN above +inf)                     -- calculate_hit_at_one's summand
//   num_labels n, the positives of the row
//   hits_at_n  the positives with p > 0 among the row's first n entries in the order of torch.sort(p, descending=True, stable=True)
//                                                                                              -- calculate_precision_at_equal_recall_rate
//   loss_row   (optional) sum over the row of -[y log(p + 1e-5) + (1 - y) log(1 - p + 1e-5)]: losses.py CrossEntropyLoss on the
//              predictions; every term in fp32 with logf, the sum in fp64 in a fixed order
//   top_*      the k best entries (index, value, label), bit-identical to lpm_topk_rows
// Keys are lpm_topk_rows' 48-bit keys: the float's order-preserving image in the upper 32 bits (NaN -> all ones, -0 -> +0), 65535 -
// index in the lower 16, so "larger key" is exactly the stable descending sort's "earlier" and all keys of a row are distinct.  The n-th
// and the k-th largest key are found together by a 48-round bitwise search, from the top bit down: round b keeps bit b of a threshold
// when at least n (k) keys are >= it.  A round counts with the compare's own lane mask (ballot + popcount, wave-uniform, no shuffles),
// then one barrier joins the four waves: the cost does not depend on n or k.  One pass then counts hits_at_n (key >= the n-th key), one
// compacts the k keys >= the k-th key into LDS (per-wave ballot offsets), and one wave ranks those k keys and writes them in order.
// Rows of V <= 256 E (E = 4, 16, 32) keep their keys in registers, E per thread (element j * 256 + tid); larger rows re-read the
// predictions from global memory (L2) every round.  No atomics: the fp64 loss sum is a wave butterfly plus a fixed-order sum over waves.
#include "lpm_common.h"

namespace lpm {

constexpr int EVAL_MAX_K = 64;          // lpm_topk_rows' limits
constexpr int EVAL_MAX_V = 65536;
constexpr int EVAL_THREADS = 256;
// LDS carve (16-byte aligned offsets): wave partials, then the k compacted keys
constexpr int EVAL_RED_D = 0;           // double [4]
constexpr int EVAL_RED_I = 32;          // int [32]: [0, 4) pass 0, [8, 24) the search (double-buffered), [24, 32) the hit / member pass
constexpr int EVAL_TOPKEY = 160;        // uint64 [64]
constexpr int EVAL_LDS = 672;

// the upper 32 bits of lpm_topk_rows' key (topk.hip: topk_key)
__device__ __forceinline__ unsigned eval_image(float x) {
    unsigned u = __float_as_uint(x);
    if (x != x) u = 0xFFFFFFFFu;
    else if (x == 0.f) u = 0x80000000u;
    else u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return u;
}

__device__ __forceinline__ uint64_t eval_key(unsigned image, int i) {
    return ((uint64_t)image << 16) | (uint64_t)(EVAL_MAX_V - 1 - i);
}

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ int wave_count(bool pred) { return __popcll(__ballot(pred)); }

// E > 0: the row's keys live in registers, E per thread (V <= 256 E); E = 0: every pass re-reads the row
template <int E>
__global__ __launch_bounds__(EVAL_THREADS) void eval_rows_kernel(const float* __restrict__ p, const unsigned char* __restrict__ y, int V,
                                                                 int k, unsigned char* __restrict__ hit1, int32_t* __restrict__ num_labels,
                                                                 int32_t* __restrict__ hits_at_n, double* __restrict__ loss_row,
                                                                 int32_t* __restrict__ top_index, float* __restrict__ top_value,
                                                                 unsigned char* __restrict__ top_label) {
    __shared__ __attribute__((aligned(16))) char smem[EVAL_LDS];
    double* red_d = reinterpret_cast<double*>(smem + EVAL_RED_D);
    int* red_i = reinterpret_cast<int*>(smem + EVAL_RED_I);
    uint64_t* topkey = reinterpret_cast<uint64_t*>(smem + EVAL_TOPKEY);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t row = blockIdx.x;
    const float* pr = p + row * V;
    const unsigned char* yr = y + row * V;
    const int J = E > 0 ? E : (V + EVAL_THREADS - 1) / EVAL_THREADS;   // element j of this thread: j * 256 + tid
    constexpr int UNROLL = E > 0 ? E : 1;
    uint64_t keys[UNROLL];
    // key of element j (0 past the row's end: below every candidate threshold, which is >= 1)
    auto key_at = [&](int j) -> uint64_t {
        if constexpr (E > 0) return keys[j];
        const int i = j * EVAL_THREADS + tid;
        return i < V ? eval_key(eval_image(pr[i]), i) : 0;
    };

    // pass 0: the keys; n and the loss
    int n_t = 0;
    double loss_t = 0.0;
#pragma unroll UNROLL
    for (int j = 0; j < J; ++j) {
        const int i = j * EVAL_THREADS + tid;
        uint64_t key = 0;
        if (i < V) {
            const float x = pr[i];
            const unsigned char l = yr[i];
            key = eval_key(eval_image(x), i);
            n_t += l != 0;
            if (loss_row) {
                const float f = l ? 1.f : 0.f;
                const float t = f * logf(x + 1e-5f) + (1.f - f) * logf(1.f - x + 1e-5f);
                loss_t -= (double)t;
            }
        }
        if constexpr (E > 0) keys[j] = key;
    }
    n_t = wave_sum_i(n_t);
    loss_t = wave_sum_d(loss_t);
    if (lane == 0) {
        red_i[wave] = n_t;
        red_d[wave] = loss_t;
    }
    __syncthreads();
    const int n = red_i[0] + red_i[1] + red_i[2] + red_i[3];
    const double loss = ((red_d[0] + red_d[1]) + red_d[2]) + red_d[3];

    // the n-th (n >= 1) and the k-th largest key: the largest P with #{key >= P} >= target, built bit by bit from the top
    uint64_t Pn = 0, Pk = 0;
    for (int b = 47; b >= 0; --b) {
        const uint64_t cn = Pn | ((uint64_t)1 << b), ck = Pk | ((uint64_t)1 << b);
        int c_n = 0, c_k = 0;
#pragma unroll UNROLL
        for (int j = 0; j < J; ++j) {
            const uint64_t key = key_at(j);
            c_n += wave_count(key >= cn);
            c_k += wave_count(key >= ck);
        }
        int* rb = red_i + 8 + (b & 1) * 8;                 // round b + 1's reads of this half ended before the last barrier
        if (lane == 0) {
            rb[2 * wave] = c_n;
            rb[2 * wave + 1] = c_k;
        }
        __syncthreads();
        if (rb[0] + rb[2] + rb[4] + rb[6] >= n) Pn = cn;  // (n = 0: every round accepts; Pn is not used)
        if (rb[1] + rb[3] + rb[5] + rb[7] >= k) Pk = ck;
    }

    // hits_at_n, and the members (key >= Pk, exactly k of them) per wave
    int h = 0, members = 0;
#pragma unroll UNROLL
    for (int j = 0; j < J; ++j) {
        const int i = j * EVAL_THREADS + tid;
        const uint64_t key = key_at(j);
        // p > 0 from the key's image: above +0's image, and not NaN
        const unsigned u = (unsigned)(key >> 16);
        h += wave_count(n > 0 && key >= Pn && u > 0x80000000u && u != 0xFFFFFFFFu && i < V && yr[i] != 0);
        members += wave_count(key >= Pk);
    }
    if (lane == 0) {
        red_i[24 + wave] = h;
        red_i[28 + wave] = members;
    }
    __syncthreads();
    const int hits = red_i[24] + red_i[25] + red_i[26] + red_i[27];
    int off = 0;
    for (int w = 0; w < wave; ++w) off += red_i[28 + w];

    // compaction of the k members into LDS (unordered)
#pragma unroll UNROLL
    for (int j = 0; j < J; ++j) {
        const uint64_t key = key_at(j);
        const bool m = key >= Pk;
        const unsigned long long mask = __ballot(m);
        const int slot = off + __popcll(mask & ((1ull << lane) - 1ull));
        if (m && slot < EVAL_MAX_K) topkey[slot] = key;
        off += __popcll(mask);
    }
    __syncthreads();

    // one wave ranks the k keys (rank = how many are larger) and writes them in the sort's order
    if (wave == 0) {
        if (lane < k) {
            const uint64_t key = topkey[lane];
            int r = 0;
            for (int j = 0; j < k; ++j) r += topkey[j] > key;
            const int i = min(EVAL_MAX_V - 1 - (int)(key & 0xFFFF), V - 1);   // (a member's index is < V: the min only bounds the reads)
            const unsigned char l = yr[i];
            top_index[row * k + r] = i;
            top_value[row * k + r] = pr[i];                // the entry itself (its NaN payload, its sign of zero)
            top_label[row * k + r] = l;
            if (r == 0) hit1[row] = l;
        }
        if (lane == 0) {
            num_labels[row] = n;
            hits_at_n[row] = hits;
            if (loss_row) loss_row[row] = loss;
        }
    }
}

}  // namespace lpm

extern "C" int lpm_eval_rows(const float* p, const unsigned char* labels, int B, int V, int k, unsigned char* hit1, int32_t* num_labels,
                             int32_t* hits_at_n, double* loss_row, int32_t* top_index, float* top_value, unsigned char* top_label,
                             lpm_stream_t stream) {
    using namespace lpm;
    LPM_REQUIRE(p && labels && hit1 && num_labels && hits_at_n && top_index && top_value && top_label, LPM_ERR_BADARG,
                "lpm_eval_rows: null pointer");
    LPM_REQUIRE(B > 0 && V > 0 && k >= 1 && k <= EVAL_MAX_K && k <= V && V <= EVAL_MAX_V, LPM_ERR_UNSUPPORTED_SHAPE,
                "lpm_eval_rows: need 1 <= k <= %d, k <= V <= %d (B=%d V=%d k=%d)", EVAL_MAX_K, EVAL_MAX_V, B, V, k);
    const dim3 grid((unsigned)B), block(EVAL_THREADS);
    hipStream_t st = (hipStream_t)stream;
    if (V <= 4 * EVAL_THREADS)
        hipLaunchKernelGGL(eval_rows_kernel<4>, grid, block, 0, st, p, labels, V, k, hit1, num_labels, hits_at_n, loss_row, top_index,
                           top_value, top_label);
    else if (V <= 16 * EVAL_THREADS)
        hipLaunchKernelGGL(eval_rows_kernel<16>, grid, block, 0, st, p, labels, V, k, hit1, num_labels, hits_at_n, loss_row, top_index,
                           top_value, top_label);
    else if (V <= 32 * EVAL_THREADS)
        hipLaunchKernelGGL(eval_rows_kernel<32>, grid, block, 0, st, p, labels, V, k, hit1, num_labels, hits_at_n, loss_row, top_index,
                           top_value, top_label);
    else
        hipLaunchKernelGGL(eval_rows_kernel<0>, grid, block, 0, st, p, labels, V, k, hit1, num_labels, hits_at_n, loss_row, top_index,
                           top_value, top_label);
    return check_launch("lpm_eval_rows");
}
