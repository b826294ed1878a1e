// The rows of the inference CSV (inference.py:88-96: "<class> <score> <class> <score> ...\n" behind every video id) as text:
//   device  lpm_format_pairs       the rows of a batch from the top-k arrays (lpm_topk_rows' index / value), one wave per row
//   host    lpm_format_pairs_host  the same bytes on the CPU (format_pairs.h is one source for both)
//   host    lpm_csv_join_rows      "<id>,<row>" for every row of a batch: the bytes inference.write_csv hands to one write()
// Kernel: lane j < k formats pair j ("%i %g" and a space, the last one a newline; at most 25 bytes) into a 28-byte LDS slot of its own
// (seven dwords, an odd count: the slots of any 32 consecutive lanes start in the 32 different banks an LDS write sees), an inclusive
// wave scan of the lengths places the pairs, every lane copies its bytes into the wave's row buffer in LDS, and the row leaves as
// 16-byte stores (the slot of a row is 16-byte aligned when the text buffer is: stride is a multiple of 16; any other buffer takes byte
// stores).  The bytes of the last 16-byte store behind the row's length are zeros.  No atomics: the same input gives the same bytes.
#include "lpm_common.h"
#include "format_pairs.h"

#include <string.h>

namespace lpm {

constexpr int CSV_MAX_K = 64;
constexpr int CSV_PAIR_SLOT = 28;                                   // bytes of a lane's staging slot, >= fmt::kMaxPair
constexpr int CSV_ROW_MAX = 1600;                                   // lpm_format_pairs_stride(64)
constexpr int CSV_WAVES = 4;
static_assert(CSV_PAIR_SLOT >= fmt::kMaxPair && CSV_PAIR_SLOT % 4 == 0, "staging slot");
static_assert(CSV_ROW_MAX == (fmt::kMaxPair * CSV_MAX_K + 15) / 16 * 16, "row buffer");

__host__ __device__ constexpr int csv_stride(int k) { return (fmt::kMaxPair * k + 15) / 16 * 16; }

__global__ __launch_bounds__(64 * CSV_WAVES) void format_pairs_kernel(const int32_t* __restrict__ index, const uint32_t* __restrict__ value,
                                                                       int B, int k, int stride, int wide, unsigned char* __restrict__ text,
                                                                       int32_t* __restrict__ length) {
    __shared__ unsigned char stage[CSV_WAVES][64 * CSV_PAIR_SLOT];
    __shared__ uint4 rowbuf[CSV_WAVES][CSV_ROW_MAX / 16];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int row = blockIdx.x * CSV_WAVES + wave;
    const bool live = row < B;                                      // (every wave reaches both barriers)
    unsigned char* mine = stage[wave] + lane * CSV_PAIR_SLOT;
    unsigned char* rb = reinterpret_cast<unsigned char*>(rowbuf[wave]);
    int len = 0;
    if (live && lane < k) {
        const int64_t at = (int64_t)row * k + lane;
        len = fmt::format_pair(index[at], value[at], lane == k - 1 ? (unsigned char)'\n' : (unsigned char)' ', mine);
    }
    for (int i = lane; i < CSV_ROW_MAX / 16; i += 64) rowbuf[wave][i] = make_uint4(0u, 0u, 0u, 0u);
    int incl = len;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
    }
    const int total = __shfl(incl, 63, 64);                          // at most 25 k <= stride
    __syncthreads();                                                 // the zeros are in place (a lane's slot is read by that lane only)
    for (int i = 0; i < len; ++i) rb[incl - len + i] = mine[i];
    __syncthreads();
    if (!live) return;
    unsigned char* dst = text + (int64_t)row * stride;
    if (wide) {
        uint4* dst16 = reinterpret_cast<uint4*>(dst);
        for (int i = lane; i < (total + 15) / 16; i += 64) dst16[i] = rowbuf[wave][i];
    } else {
        for (int i = lane; i < total; i += 64) dst[i] = rb[i];
    }
    if (lane == 0) length[row] = total;
}

}  // namespace lpm

extern "C" int lpm_format_pairs_stride(int k) { return (k >= 1 && k <= lpm::CSV_MAX_K) ? lpm::csv_stride(k) : 0; }

extern "C" int lpm_format_pairs(const int32_t* index, const float* value, int B, int k, unsigned char* text, int32_t* length,
                                lpm_stream_t stream) {
    using namespace lpm;
    LPM_REQUIRE(index && value && text && length, LPM_ERR_BADARG, "lpm_format_pairs: null pointer");
    LPM_REQUIRE(B >= 1 && k >= 1 && k <= CSV_MAX_K, LPM_ERR_UNSUPPORTED_SHAPE, "lpm_format_pairs: need B >= 1 and 1 <= k <= %d (B=%d k=%d)",
                CSV_MAX_K, B, k);
    LPM_REQUIRE(((uintptr_t)index & 3) == 0 && ((uintptr_t)value & 3) == 0 && ((uintptr_t)length & 3) == 0, LPM_ERR_BADARG,
                "lpm_format_pairs: index, value and length must be 4-byte aligned");
    const int wide = ((uintptr_t)text & 15) == 0;
    const unsigned blocks = (unsigned)(((int64_t)B + CSV_WAVES - 1) / CSV_WAVES);
    hipLaunchKernelGGL(format_pairs_kernel, dim3(blocks), dim3(64 * CSV_WAVES), 0, (hipStream_t)stream, index,
                       reinterpret_cast<const uint32_t*>(value), B, k, csv_stride(k), wide, text, length);
    return check_launch("lpm_format_pairs");
}

extern "C" int lpm_format_pairs_host(const int32_t* index, const float* value, int B, int k, unsigned char* text, int32_t* length) {
    using namespace lpm;
    LPM_REQUIRE(index && value && text && length, LPM_ERR_BADARG, "lpm_format_pairs_host: null pointer");
    LPM_REQUIRE(B >= 1 && k >= 1 && k <= CSV_MAX_K, LPM_ERR_UNSUPPORTED_SHAPE,
                "lpm_format_pairs_host: need B >= 1 and 1 <= k <= %d (B=%d k=%d)", CSV_MAX_K, B, k);
    const int stride = csv_stride(k);
    for (int64_t r = 0; r < B; ++r) {
        unsigned char* out = text + r * stride;
        int n = 0;
        for (int j = 0; j < k; ++j) {
            uint32_t bits;
            memcpy(&bits, value + r * k + j, 4);
            n += fmt::format_pair(index[r * k + j], bits, j == k - 1 ? (unsigned char)'\n' : (unsigned char)' ', out + n);
        }
        length[r] = n;
    }
    return LPM_OK;
}

extern "C" int lpm_csv_join_rows(const void* ids, const int64_t* id_begin, const int64_t* id_end, const unsigned char* text,
                                 const int32_t* length, int B, int stride, unsigned char* out, int64_t out_capacity, int64_t* out_length) {
    using namespace lpm;
    LPM_REQUIRE(id_begin && id_end && text && length && out && out_length && B >= 1 && stride >= 1 && out_capacity >= 0, LPM_ERR_BADARG,
                "lpm_csv_join_rows: bad argument");
    const unsigned char* blob = static_cast<const unsigned char*>(ids);
    int64_t n = 0;
    for (int64_t r = 0; r < B; ++r) {
        const int64_t idn = id_end[r] - id_begin[r], len = length[r];
        LPM_REQUIRE(idn >= 0 && (idn == 0 || blob) && len >= 0 && len <= stride, LPM_ERR_BADARG,
                    "lpm_csv_join_rows: row %lld: id of %lld bytes, row text of %lld bytes (stride %d)", (long long)r, (long long)idn,
                    (long long)len, stride);
        LPM_REQUIRE(n + idn + 1 + len <= out_capacity, LPM_ERR_WORKSPACE, "lpm_csv_join_rows: the output buffer of %lld bytes is too small",
                    (long long)out_capacity);
        if (idn) memcpy(out + n, blob + id_begin[r], (size_t)idn);
        n += idn;
        out[n++] = ',';
        memcpy(out + n, text + r * stride, (size_t)len);
        n += len;
    }
    *out_length = n;
    return LPM_OK;
}
