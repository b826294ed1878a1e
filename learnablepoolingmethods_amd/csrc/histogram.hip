// Histograms for the TensorBoard writer (summaries.py; tensorflow::histogram::Histogram::Add's semantics).
//
// lpm_histogram_segments: for every segment (seg_start[s], seg_len[s]) of an fp32 buffer x, counts[s][b] = the number of finite elements
// whose bucket is b = the index of the first limit strictly greater than (double)v (std::upper_bound over an ascending fp64 table that is an
// INPUT: TensorFlow builds it by a loop in which rounding accumulates, so nothing here recomputes a limit), stats[s] = (min, max, num, sum,
// sum_squares) of the finite elements in fp64, nonfinite[s] = the NaN / +-Inf elements, which enter nothing else.  -0.0 compares equal to
// 0.0 and lands in its bucket.
//
// Three launches on the caller's stream, after a memset of counts:
//   1. hist_tables_kernel: (a) for each of the 4096 values of (sign, exponent, top 3 mantissa bits) the bucket of the SMALLEST float with
//      those bits (upper_bound by bisection): a lower bound of the bucket of every float that shares them, because upper_bound is monotonic;
//      (b) for every limit the smallest FLOAT that is >= it.  For an fp32 value v, "limit <= (double)v" and "that float <= v" are the same
//      statement, so the hot loop compares in fp32 against a 4-byte table and stays exact at every limit.
//   2. hist_segments_kernel, grid (gx, segments): workgroup (bx, s) walks chunks bx, bx + gx, ... (4096 elements each) of segment s with
//      aligned 16-byte loads -- a segment may start at any element; the elements of the first and last 16-byte granule that lie outside it
//      are masked (only a segment's first and last chunk pay for the test), and an aligned granule that holds one byte of the buffer
//      cannot cross a page.  Per element: the guess from LDS, then "while (v >= limit_as_float[b]) ++b" against the table in LDS: exact
//      for ANY ascending table; with TensorFlow's 1.1-spaced table a guess cell spans at most 1.125x, i.e. at most two steps.
//      Contention: a weight tensor puts nearly all of its elements into about ten adjacent buckets, so one set of bins per workgroup (let
//      alone per segment) would serialise on a few addresses.  Every WAVE owns a private set of bins in LDS (ds_add_u32, no return); a wave
//      whose 64 elements all share one bucket -- constants: zero biases, unit gammas, padding -- adds their number with one lane.  At the end
//      the four sets are summed and only the non-zero bins go out as 64-bit integer atomic adds: integers, so the counts do not depend on
//      the order.  sum / sum_squares / min / max / num never touch an atomic: thread -> wave butterfly -> the waves in order -> one
//      partial record per workgroup in the workspace.
//   3. hist_finish_kernel, one workgroup per segment: the partial records in a fixed order (thread t takes records t, t + 256, ...; then
//      the same butterfly).  Two runs give the same bits.
//
// lpm_histogram_frames_q8: counts of the byte values of quantised frames q [B, max_frames, F] over t < num_frames[b], entry 256 = the
// elements of the padded frames (not read at all: a row's frame index decides).  Same per-wave bins.
#include "lpm_common.h"

namespace lpm {

constexpr int HIST_THREADS = 256;
constexpr int HIST_WAVES = HIST_THREADS / kWave;
constexpr int HIST_UNROLL = 4;                                   // 16-byte loads in flight per thread
constexpr int HIST_CHUNK_VEC = HIST_THREADS * HIST_UNROLL;       // 1024 granules = 4096 elements per chunk
constexpr int HIST_MAX_GX = 512;
constexpr int HIST_MAX_LIMITS = 2048;                            // LDS: 20 L + 8 KiB
constexpr int HIST_MAX_SEGMENTS = 65535;
constexpr int HIST_GUESS = 4096;                                 // sign | exponent | 3 mantissa bits
constexpr size_t HIST_GUESS_BYTES = HIST_GUESS * sizeof(uint16_t);
constexpr size_t HIST_TABLE_BYTES = HIST_GUESS_BYTES + HIST_MAX_LIMITS * sizeof(float);   // the workspace's head: guesses, float limits

struct HistPartial {
    double mn, mx, sum, sumsq;
    int64_t num, nonfinite;
};

__host__ __device__ inline int hist_gx(int64_t max_seg_len) {
    const int64_t chunks = (max_seg_len + 3 + 4 * HIST_CHUNK_VEC - 1) / (4 * HIST_CHUNK_VEC);   // (+3: a start two bits off alignment)
    return (int)(chunks < 1 ? 1 : chunks > HIST_MAX_GX ? HIST_MAX_GX : chunks);
}

// what the segment kernel and the finish kernel both derive from (start, len): the granules and chunks of the segment.  A segment that
// does not lie inside [0, x_len) has none (the wrapper refuses it before any launch; this keeps a stray table from reading outside x).
struct HistSeg {
    int64_t start, len, nvec, nchunk;
    int shift;
};
__device__ __forceinline__ HistSeg hist_seg(const float* x, int64_t x_len, const int64_t* seg_start, const int64_t* seg_len, int s) {
    HistSeg g;
    g.start = seg_start[s];
    g.len = seg_len[s];
    if (g.start < 0 || g.len < 1 || g.start > x_len - g.len) g.len = 0;
    g.shift = g.len ? (int)((reinterpret_cast<uintptr_t>(x + g.start) >> 2) & 3) : 0;
    g.nvec = g.len ? (g.shift + g.len + 3) / 4 : 0;
    g.nchunk = (g.nvec + HIST_CHUNK_VEC - 1) / HIST_CHUNK_VEC;
    return g;
}

__device__ __forceinline__ int hist_upper_bound(const double* __restrict__ limits, int L, double v) {
    int lo = 0, hi = L;                       // first index with limits[i] > v
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (limits[mid] <= v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(HIST_THREADS) void hist_tables_kernel(const double* __restrict__ limits, int L, uint16_t* __restrict__ guess,
                                                                   float* __restrict__ limf) {
    const int k = blockIdx.x * HIST_THREADS + threadIdx.x;      // k = bits >> 20
    if (k >= HIST_GUESS) return;
    if (k < L) {
        // the smallest float >= limits[k] (round to nearest, then one float up if that fell below); the last limit closes the table:
        // +inf, so that the bucket search stops at L - 1 without a bound test
        const double l = limits[k];
        float t = (float)l;
        if ((double)t < l) {
            const unsigned u = __float_as_uint(t);
            t = t == 0.f ? __uint_as_float(1u) : __uint_as_float(t > 0.f ? u + 1u : u - 1u);
        }
        limf[k] = k == L - 1 ? __uint_as_float(0x7f800000u) : t;
    }
    // the smallest float of the cell: positive cells start at their lowest magnitude, negative cells at their largest.  (Cells of exponent
    // 255 hold no finite value; their entry is never read.)
    const unsigned mag = ((unsigned)(k & 2047) << 20) | ((k & 2048) ? 0xFFFFFu : 0u);
    double low = (double)__uint_as_float(mag);
    if ((k & 2047) >= (255 << 3)) low = 3.4028234663852886e38;
    if (k & 2048) low = -low;
    const int b = hist_upper_bound(limits, L, low);
    guess[k] = (uint16_t)(b < L - 1 ? b : L - 1);
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ int64_t wave_sum_i64(int64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (int64_t)__shfl_xor((long long)v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_min_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ double wave_max_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

// one count into the wave's private bins; a full wave whose 64 elements share one bucket adds 64 with one lane
__device__ __forceinline__ void hist_wave_add(unsigned* __restrict__ bins, int b, bool valid, int lane) {
    if (__ballot(valid) == ~0ull) {
        const int b0 = __builtin_amdgcn_readfirstlane(b);
        if (__ballot(b != b0) == 0) {
            if (lane == 0) atomicAdd(&bins[b0], 64u);
            return;
        }
    }
    if (valid) atomicAdd(&bins[b], 1u);
}

// block-level join of the per-thread statistics (every thread calls it); the result is valid on thread 0
__device__ __forceinline__ HistPartial hist_block_join(HistPartial p, HistPartial* __restrict__ sh) {
    p.mn = wave_min_f64(p.mn);
    p.mx = wave_max_f64(p.mx);
    p.sum = wave_sum_f64(p.sum);
    p.sumsq = wave_sum_f64(p.sumsq);
    p.num = wave_sum_i64(p.num);
    p.nonfinite = wave_sum_i64(p.nonfinite);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) sh[wave] = p;
    __syncthreads();
    if (threadIdx.x == 0) {
        p = sh[0];
        for (int w = 1; w < HIST_WAVES; ++w) {
            p.mn = fmin(p.mn, sh[w].mn);
            p.mx = fmax(p.mx, sh[w].mx);
            p.sum += sh[w].sum;
            p.sumsq += sh[w].sumsq;
            p.num += sh[w].num;
            p.nonfinite += sh[w].nonfinite;
        }
    }
    return p;
}

// per-thread running statistics of the segment kernel
struct HistAcc {
    float mn, mx;
    double sum, sumsq;
    int num, nonfinite;                                          // (a thread sees < 2^31 elements: lpm_histogram_segments checks x_len)
};

// one chunk: HIST_UNROLL aligned 16-byte loads per thread, then the elements.  EDGE: the chunk holds granules or elements outside the
// segment (its first and last chunk only), which are masked; an interior chunk tests nothing.
template <bool EDGE>
__device__ __forceinline__ void hist_chunk(const f32x4* __restrict__ xv, int64_t v0, const HistSeg& g, const uint16_t* __restrict__ gs,
                                           const float* __restrict__ limf, unsigned* __restrict__ mybins, int lane, HistAcc& a) {
    f32x4 v[HIST_UNROLL];
#pragma unroll
    for (int u = 0; u < HIST_UNROLL; ++u) {
        const int64_t iv = v0 + u * HIST_THREADS;
        v[u] = (!EDGE || iv < g.nvec) ? xv[iv] : f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int u = 0; u < HIST_UNROLL; ++u) {
        const int64_t e0 = (v0 + u * HIST_THREADS) * 4 - g.shift;                // element index of component 0 (EDGE: may lie outside)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float f = v[u][j];
            const unsigned bits = __float_as_uint(f);
            const bool inside = !EDGE || (e0 + j >= 0 && e0 + j < g.len);
            const bool finite = (bits & 0x7fffffffu) < 0x7f800000u;
            const bool valid = inside && finite;
            int b = 0;
            if (valid) {
                const double d = (double)f;
                b = gs[bits >> 20];
                while (f >= limf[b]) ++b;                                        // (limf[L - 1] = +inf ends it)
                a.mn = fminf(a.mn, f);
                a.mx = fmaxf(a.mx, f);
                a.sum += d;
                a.sumsq += d * d;
                ++a.num;
            }
            a.nonfinite += inside && !finite;
            hist_wave_add(mybins, b, valid, lane);
        }
    }
}

__global__ __launch_bounds__(HIST_THREADS) void hist_segments_kernel(const float* __restrict__ x, int64_t x_len,
                                                                     const int64_t* __restrict__ seg_start,
                                                                     const int64_t* __restrict__ seg_len, int L,
                                                                     const uint16_t* __restrict__ guess, const float* __restrict__ limf_g,
                                                                     unsigned long long* __restrict__ counts, HistPartial* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) char hist_smem[];
    __shared__ HistPartial join_sh[HIST_WAVES];
    const int s = blockIdx.y, bx = blockIdx.x, gx = gridDim.x;
    const HistSeg g = hist_seg(x, x_len, seg_start, seg_len, s);
    if (bx >= g.nchunk) return;                                  // (block-uniform: before any barrier)
    float* limf = reinterpret_cast<float*>(hist_smem);           // [L]
    uint16_t* gs = reinterpret_cast<uint16_t*>(hist_smem + (size_t)L * 4);                       // [4096]
    unsigned* bins = reinterpret_cast<unsigned*>(hist_smem + (size_t)L * 4 + HIST_GUESS_BYTES);   // [waves][L]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < L; i += HIST_THREADS) limf[i] = limf_g[i];
    for (int i = tid; i < HIST_GUESS / 2; i += HIST_THREADS)
        reinterpret_cast<unsigned*>(gs)[i] = reinterpret_cast<const unsigned*>(guess)[i];
    for (int i = tid; i < HIST_WAVES * L; i += HIST_THREADS) bins[i] = 0u;
    __syncthreads();
    unsigned* mybins = bins + wave * L;

    const f32x4* xv = reinterpret_cast<const f32x4*>(x + g.start - g.shift);    // 16-byte aligned
    HistAcc a{__uint_as_float(0x7f800000u), __uint_as_float(0xff800000u), 0.0, 0.0, 0, 0};
    for (int64_t c = bx; c < g.nchunk; c += gx) {
        const int64_t v0 = c * HIST_CHUNK_VEC + tid;
        // interior: every granule of the chunk lies inside the segment (block-uniform)
        if (c * (4 * HIST_CHUNK_VEC) >= g.shift && (c + 1) * (4 * HIST_CHUNK_VEC) - g.shift <= g.len)
            hist_chunk<false>(xv, v0, g, gs, limf, mybins, lane, a);
        else
            hist_chunk<true>(xv, v0, g, gs, limf, mybins, lane, a);
    }
    __syncthreads();
    unsigned long long* out = counts + (int64_t)s * L;
    for (int i = tid; i < L; i += HIST_THREADS) {
        unsigned long long c = 0;
#pragma unroll
        for (int w = 0; w < HIST_WAVES; ++w) c += bins[w * L + i];
        if (c) atomicAdd(&out[i], c);
    }
    HistPartial p{(double)a.mn, (double)a.mx, a.sum, a.sumsq, (int64_t)a.num, (int64_t)a.nonfinite};
    p = hist_block_join(p, join_sh);
    if (tid == 0) part[(int64_t)s * gx + bx] = p;
}

__global__ __launch_bounds__(HIST_THREADS) void hist_finish_kernel(const float* __restrict__ x, int64_t x_len,
                                                                   const int64_t* __restrict__ seg_start,
                                                                   const int64_t* __restrict__ seg_len, int gx,
                                                                   const HistPartial* __restrict__ part, double* __restrict__ stats,
                                                                   int64_t* __restrict__ nonfinite) {
    __shared__ HistPartial join_sh[HIST_WAVES];
    const int s = blockIdx.x;
    const HistSeg g = hist_seg(x, x_len, seg_start, seg_len, s);
    const int nact = (int)(g.nchunk < gx ? g.nchunk : gx);       // the workgroups of the segment that wrote a record
    HistPartial p{__longlong_as_double(0x7ff0000000000000ll), __longlong_as_double(0xfff0000000000000ll), 0.0, 0.0, 0, 0};
    for (int i = threadIdx.x; i < nact; i += HIST_THREADS) {
        const HistPartial q = part[(int64_t)s * gx + i];
        p.mn = fmin(p.mn, q.mn);
        p.mx = fmax(p.mx, q.mx);
        p.sum += q.sum;
        p.sumsq += q.sumsq;
        p.num += q.num;
        p.nonfinite += q.nonfinite;
    }
    p = hist_block_join(p, join_sh);
    if (threadIdx.x == 0) {
        // an empty histogram keeps tensorflow::histogram::Histogram::Clear's values
        stats[s * 5 + 0] = p.num ? p.mn : 1.7976931348623157e308;
        stats[s * 5 + 1] = p.num ? p.mx : -1.7976931348623157e308;
        stats[s * 5 + 2] = (double)p.num;
        stats[s * 5 + 3] = p.sum;
        stats[s * 5 + 4] = p.sumsq;
        nonfinite[s] = p.nonfinite;
    }
}

constexpr int HISTQ_BINS = 257;

__global__ __launch_bounds__(HIST_THREADS) void hist_frames_q8_kernel(const unsigned* __restrict__ q, const int32_t* __restrict__ num_frames,
                                                                      int64_t rows, int max_frames, int words,
                                                                      unsigned long long* __restrict__ counts) {
    __shared__ unsigned bins[HIST_WAVES][256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < HIST_WAVES * 256; i += HIST_THREADS) (&bins[0][0])[i] = 0u;
    __syncthreads();
    unsigned long long padded = 0;                               // rows at and beyond num_frames (thread 0 counts them; not read)
    for (int64_t r = blockIdx.x; r < rows; r += gridDim.x) {
        const int b = (int)(r / max_frames), t = (int)(r % max_frames);
        if (t >= num_frames[b]) {                                // (block-uniform)
            padded += 1;
            continue;
        }
        const unsigned* row = q + r * words;
        const int rounds = (words + HIST_THREADS - 1) / HIST_THREADS;
        for (int i = 0; i < rounds; ++i) {                       // (every lane makes every round: hist_wave_add is wave-wide)
            const int w = i * HIST_THREADS + tid;
            const bool valid = w < words;
            const unsigned x = valid ? row[w] : 0u;
#pragma unroll
            for (int j = 0; j < 4; ++j) hist_wave_add(bins[wave], (int)((x >> (8 * j)) & 255u), valid, lane);
        }
    }
    __syncthreads();
    {
        unsigned long long c = 0;
#pragma unroll
        for (int w = 0; w < HIST_WAVES; ++w) c += bins[w][tid];
        if (c) atomicAdd(&counts[tid], c);
    }
    if (tid == 0 && padded) atomicAdd(&counts[256], padded * 4ull * (unsigned long long)words);
}

}  // namespace lpm

extern "C" size_t lpm_histogram_segments_workspace_bytes(int num_segments, int64_t max_seg_len) {
    using namespace lpm;
    if (num_segments < 1 || max_seg_len < 1) return 0;
    return HIST_TABLE_BYTES + (size_t)num_segments * hist_gx(max_seg_len) * sizeof(HistPartial);
}

extern "C" int lpm_histogram_segments(const float* x, int64_t x_len, const int64_t* seg_start, const int64_t* seg_len, int num_segments,
                                      int64_t max_seg_len, const double* limits, int num_limits, int64_t* counts, double* stats,
                                      int64_t* nonfinite, void* workspace, size_t workspace_bytes, lpm_stream_t stream) {
    using namespace lpm;
    LPM_REQUIRE(x && seg_start && seg_len && limits && counts && stats && nonfinite && workspace, LPM_ERR_BADARG,
                "lpm_histogram_segments: null pointer");
    LPM_REQUIRE((reinterpret_cast<uintptr_t>(x) & 3) == 0 && (reinterpret_cast<uintptr_t>(workspace) & 15) == 0, LPM_ERR_BADARG,
                "lpm_histogram_segments: x must be 4-byte aligned and the workspace 16-byte aligned");
    LPM_REQUIRE(num_segments >= 1 && num_segments <= HIST_MAX_SEGMENTS && num_limits >= 1 && num_limits <= HIST_MAX_LIMITS,
                LPM_ERR_UNSUPPORTED_SHAPE, "lpm_histogram_segments: need 1 <= segments <= %d and 1 <= limits <= %d (segments=%d limits=%d)",
                HIST_MAX_SEGMENTS, HIST_MAX_LIMITS, num_segments, num_limits);
    LPM_REQUIRE(x_len >= 1 && x_len < ((int64_t)1 << 40) && max_seg_len >= 1 && max_seg_len <= x_len, LPM_ERR_BADARG,
                "lpm_histogram_segments: need 1 <= max_seg_len <= x_len < 2^40 (x_len=%lld max_seg_len=%lld)", (long long)x_len,
                (long long)max_seg_len);
    LPM_REQUIRE(workspace_bytes >= lpm_histogram_segments_workspace_bytes(num_segments, max_seg_len), LPM_ERR_WORKSPACE,
                "lpm_histogram_segments: workspace of %zu bytes, need %zu", workspace_bytes,
                lpm_histogram_segments_workspace_bytes(num_segments, max_seg_len));
    hipStream_t st = (hipStream_t)stream;
    const int gx = hist_gx(max_seg_len), L = num_limits;
    uint16_t* guess = reinterpret_cast<uint16_t*>(workspace);
    float* limf = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + HIST_GUESS_BYTES);
    HistPartial* part = reinterpret_cast<HistPartial*>(reinterpret_cast<char*>(workspace) + HIST_TABLE_BYTES);
    if (hipMemsetAsync(counts, 0, (size_t)num_segments * L * sizeof(int64_t), st) != hipSuccess) return check_launch("lpm_histogram_segments");
    hipLaunchKernelGGL(hist_tables_kernel, dim3(HIST_GUESS / HIST_THREADS), dim3(HIST_THREADS), 0, st, limits, L, guess, limf);
    const size_t lds = (size_t)L * 4 + HIST_GUESS_BYTES + (size_t)HIST_WAVES * L * sizeof(unsigned);
    hipLaunchKernelGGL(hist_segments_kernel, dim3((unsigned)gx, (unsigned)num_segments), dim3(HIST_THREADS), lds, st, x, x_len, seg_start,
                       seg_len, L, guess, limf, reinterpret_cast<unsigned long long*>(counts), part);
    hipLaunchKernelGGL(hist_finish_kernel, dim3((unsigned)num_segments), dim3(HIST_THREADS), 0, st, x, x_len, seg_start, seg_len, gx, part,
                       stats, nonfinite);
    return check_launch("lpm_histogram_segments");
}

extern "C" int lpm_histogram_frames_q8(const void* q, const int32_t* num_frames, int B, int max_frames, int F, int64_t* counts,
                                       lpm_stream_t stream) {
    using namespace lpm;
    LPM_REQUIRE(q && num_frames && counts, LPM_ERR_BADARG, "lpm_histogram_frames_q8: null pointer");
    LPM_REQUIRE((reinterpret_cast<uintptr_t>(q) & 3) == 0, LPM_ERR_BADARG, "lpm_histogram_frames_q8: q must be 4-byte aligned");
    LPM_REQUIRE(B >= 1 && max_frames >= 1 && F >= 4 && F % 4 == 0, LPM_ERR_UNSUPPORTED_SHAPE,
                "lpm_histogram_frames_q8: need B, max_frames >= 1 and F a positive multiple of 4 (B=%d max_frames=%d F=%d)", B, max_frames, F);
    hipStream_t st = (hipStream_t)stream;
    const int64_t rows = (int64_t)B * max_frames;
    if (hipMemsetAsync(counts, 0, HISTQ_BINS * sizeof(int64_t), st) != hipSuccess) return check_launch("lpm_histogram_frames_q8");
    const unsigned grid = (unsigned)(rows < 2048 ? rows : 2048);
    hipLaunchKernelGGL(hist_frames_q8_kernel, dim3(grid), dim3(HIST_THREADS), 0, st, reinterpret_cast<const unsigned*>(q), num_frames, rows,
                       max_frames, F / 4, reinterpret_cast<unsigned long long*>(counts));
    return check_launch("lpm_histogram_frames_q8");
}
