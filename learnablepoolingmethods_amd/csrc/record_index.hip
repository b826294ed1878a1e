// The reader's device path: YT8M TFRecord bytes -> padded uint8 frame batch + dense labels.
//   host  lpm_tfrecord_frame / lpm_yt8m_locate   (record_index.h: TFRecord framing, and the offsets of every frame payload, label list and
//                                                 video id of a buffer of tf.train.SequenceExample records; header bytes only)
//   HIP   lpm_gather_frames                       raw record bytes + offset table -> uint8 [B, max_frames, sum(feature_sizes)], zero rows at
//                                                 and beyond num_frames
//   HIP   lpm_labels_dense                        CSR label lists -> uint8 (bool) [B, num_classes]
// and the same for the video-level files (tf.train.Example records of float lists):
//   host  lpm_yt8m_locate_examples                (record_index.h: offset and stride of every selected float list)
//   HIP   lpm_gather_examples                     raw record bytes + offset / stride tables -> fp32 [B, sum(feature_sizes)], bit for bit
// The gather's sources are byte-aligned and nothing better (an rgb frame lies 1033 bytes after the one before it, an audio frame 137), its
// destination is 16-byte aligned.  A lane owns 16 destination bytes (four dwords of the flat output): it loads the two ALIGNED 16-byte words
// that hold its 16 source bytes, picks the five dwords that cover them and funnels neighbouring dwords through v_alignbyte_b32; one 16-byte
// store.  Lanes of a row read consecutive sources: the loads of a wave cover one contiguous kilobyte (plus the overlap of one word per lane,
// which hits the same cache lines).  No load starts outside the allocation: the second word's index is clamped to the last word of the
// buffer's capacity (its bytes are shifted out in that case), and a lane whose source range is not inside [0, nbytes) writes zeros, so a
// wrong table cannot make the kernel read out of bounds.  Four destination dwords that do not share one frame of one feature (feature sizes
// that are multiples of 4 but not of 16) take the same route one dword at a time.  The example gather is the same scheme with a dword as
// its unit: a lane owns four destination floats, values a stride of 5 bytes apart (unpacked lists) go one dword at a time.
#include "lpm_common.h"

#if !defined(__HIP_DEVICE_COMPILE__)
#include "record_index.h"
#endif

namespace lpm {

constexpr int GATHER_MAX_FEATURES = 8;       // record_index.h: MAX_FEATURES
constexpr int GATHER_THREADS = 256;

struct GatherFeatures {
    int n;
    int start4[GATHER_MAX_FEATURES + 1];     // column of feature f in dwords; start4[n] = the row's length in dwords
};

__device__ __forceinline__ unsigned funnel(unsigned hi, unsigned lo, unsigned byte_shift) {
    return __builtin_amdgcn_alignbyte(hi, lo, byte_shift);     // ({hi, lo} >> 8 byte_shift)[31:0], byte_shift in [0, 4)
}

// the 16 bytes at byte offset src of the buffer (any alignment) from the two aligned 16-byte words that hold them; zeros unless
// [src, src + 16) lies inside [0, nbytes).  cap16: the allocation in 16-byte words -- the second word's index is clamped to it
__device__ __forceinline__ uint4 load16_bytes(const uint4* __restrict__ buf16, int64_t cap16, int64_t src, int64_t nbytes) {
    if (src < 0 || src > nbytes - 16) return make_uint4(0u, 0u, 0u, 0u);
    const int64_t q = src >> 4;
    const unsigned s = (unsigned)(src & 15), bs = s & 3u;
    const uint4 lo = buf16[q];
    const int64_t q1 = q + 1 < cap16 ? q + 1 : cap16 - 1;          // (s == 0 at the very end: loaded again, shifted out)
    const uint4 hi = buf16[q1];
    unsigned w0, w1, w2, w3, w4;
    switch (s >> 2) {
        case 0: w0 = lo.x, w1 = lo.y, w2 = lo.z, w3 = lo.w, w4 = hi.x; break;
        case 1: w0 = lo.y, w1 = lo.z, w2 = lo.w, w3 = hi.x, w4 = hi.y; break;
        case 2: w0 = lo.z, w1 = lo.w, w2 = hi.x, w3 = hi.y, w4 = hi.z; break;
        default: w0 = lo.w, w1 = hi.x, w2 = hi.y, w3 = hi.z, w4 = hi.w; break;
    }
    return make_uint4(funnel(w1, w0, bs), funnel(w2, w1, bs), funnel(w3, w2, bs), funnel(w4, w3, bs));
}

// the same for 4 bytes, from two aligned dwords; last4: the index of the allocation's last dword
__device__ __forceinline__ unsigned load4_bytes(const unsigned* __restrict__ buf4, int64_t last4, int64_t sb, int64_t nbytes) {
    if (sb < 0 || sb > nbytes - 4) return 0u;
    const int64_t a = sb >> 2;
    const unsigned lo = buf4[a], hi = buf4[a + 1 <= last4 ? a + 1 : last4];
    return funnel(hi, lo, (unsigned)(sb & 3));
}

// where dword c4 of destination row `row` comes from: the byte offset into buf, or -1 for a zero
__device__ __forceinline__ int64_t gather_source(int64_t row, int c4, const int64_t* __restrict__ offset, const int32_t* __restrict__ num_frames,
                                                 int T, const GatherFeatures& ft, int64_t nbytes, int& f_out) {
    const int64_t b = row / T;
    const int t = (int)(row - b * T);
    int f = 0;
#pragma unroll
    for (int j = 1; j < GATHER_MAX_FEATURES; ++j)
        if (j < ft.n && c4 >= ft.start4[j]) f = j;
    f_out = f;
    if (t >= num_frames[b]) return -1;
    const int64_t o = offset[(b * ft.n + f) * T + t];
    if (o < 0 || o > nbytes - 4 * (int64_t)(ft.start4[f + 1] - ft.start4[f])) return -1;       // the whole frame inside [0, nbytes), or zeros
    return o + 4 * (int64_t)(c4 - ft.start4[f]);
}

__global__ __launch_bounds__(GATHER_THREADS) void gather_frames_kernel(const unsigned char* __restrict__ buf, int64_t nbytes, int64_t cap16,
                                                                       const int64_t* __restrict__ offset,
                                                                       const int32_t* __restrict__ num_frames, int T, GatherFeatures ft,
                                                                       unsigned* __restrict__ out, int64_t total4) {
    const int64_t d0 = 4 * ((int64_t)blockIdx.x * GATHER_THREADS + threadIdx.x);
    if (d0 >= total4) return;
    const int F4 = ft.start4[ft.n];
    const int64_t row = d0 / F4;
    const int c4 = (int)(d0 - row * F4);
    const uint4* buf16 = reinterpret_cast<const uint4*>(buf);
    const unsigned* buf4 = reinterpret_cast<const unsigned*>(buf);

    int f0, f3 = -1;
    const int64_t src = gather_source(row, c4, offset, num_frames, T, ft, nbytes, f0);
    bool whole = d0 + 3 < total4 && c4 + 3 < F4;
    if (whole) {
        gather_source(row, c4 + 3, offset, num_frames, T, ft, nbytes, f3);
        whole = f3 == f0;
    }
    if (whole) {
        *reinterpret_cast<uint4*>(out + d0) = load16_bytes(buf16, cap16, src, nbytes);
        return;
    }
    // the four dwords one by one (a row's end, a feature boundary or the output's end inside this lane's 16 bytes)
    const int64_t last4 = cap16 * 4 - 1;
    for (int i = 0; i < 4 && d0 + i < total4; ++i) {
        const int64_t r = (d0 + i) / F4;
        const int c = (int)(d0 + i - r * F4);
        int f;
        const int64_t sb = gather_source(r, c, offset, num_frames, T, ft, nbytes, f);
        out[d0 + i] = load4_bytes(buf4, last4, sb, nbytes);
    }
}

// where float c of example b comes from: the byte offset into buf, or -1 for a zero.  A feature is refused as a whole: a negative offset,
// a stride other than 4 or 5, a last value that would end beyond nbytes
__device__ __forceinline__ int64_t example_source(int64_t b, int c, const int64_t* __restrict__ offset, const int32_t* __restrict__ stride,
                                                  const GatherFeatures& ft, int64_t nbytes, int& f_out, int& stride_out) {
    int f = 0;
#pragma unroll
    for (int j = 1; j < GATHER_MAX_FEATURES; ++j)
        if (j < ft.n && c >= ft.start4[j]) f = j;
    f_out = f;
    const int64_t o = offset[b * ft.n + f];
    const int st = stride[b * ft.n + f];
    stride_out = st;
    if (o < 0 || (st != 4 && st != 5)) return -1;
    if (o > nbytes - 4 - (int64_t)st * (ft.start4[f + 1] - ft.start4[f] - 1)) return -1;
    return o + (int64_t)st * (c - ft.start4[f]);
}

// a lane owns four floats of the flat [B, F] output (its base is 16-byte aligned; rows are not when F % 4 != 0)
__global__ __launch_bounds__(GATHER_THREADS) void gather_examples_kernel(const unsigned char* __restrict__ buf, int64_t nbytes, int64_t cap16,
                                                                         const int64_t* __restrict__ offset,
                                                                         const int32_t* __restrict__ stride, GatherFeatures ft,
                                                                         unsigned* __restrict__ out, int64_t total4) {
    const int64_t d0 = 4 * ((int64_t)blockIdx.x * GATHER_THREADS + threadIdx.x);
    if (d0 >= total4) return;
    const int F4 = ft.start4[ft.n];
    const int64_t b = d0 / F4;
    const int c = (int)(d0 - b * F4);
    int f0, f3, st0, st3;
    const int64_t src = example_source(b, c, offset, stride, ft, nbytes, f0, st0);
    bool whole = d0 + 3 < total4 && c + 3 < F4;
    if (whole) {
        example_source(b, c + 3, offset, stride, ft, nbytes, f3, st3);
        whole = f3 == f0 && (st0 == 4 || src < 0);             // (a refused feature: sixteen zero bytes)
    }
    if (whole) {
        *reinterpret_cast<uint4*>(out + d0) = load16_bytes(reinterpret_cast<const uint4*>(buf), cap16, src, nbytes);
        return;
    }
    // the four floats one by one (values 5 bytes apart, a feature boundary, a row's end or the output's end inside this lane's 16 bytes)
    const int64_t last4 = cap16 * 4 - 1;
    for (int i = 0; i < 4 && d0 + i < total4; ++i) {
        const int64_t r = (d0 + i) / F4;
        int f, st;
        const int64_t sb = example_source(r, (int)(d0 + i - r * F4), offset, stride, ft, nbytes, f, st);
        out[d0 + i] = load4_bytes(reinterpret_cast<const unsigned*>(buf), last4, sb, nbytes);
    }
}

// one thread per four bytes of the flat [B * V] matrix (its base is 4-byte aligned; the tail byte by byte)
__global__ __launch_bounds__(GATHER_THREADS) void labels_dense_kernel(const int32_t* __restrict__ label_start,
                                                                      const int32_t* __restrict__ label_index, int num_labels, int V,
                                                                      int64_t total, unsigned char* __restrict__ out) {
    const int64_t i0 = 4 * ((int64_t)blockIdx.x * GATHER_THREADS + threadIdx.x);
    if (i0 >= total) return;
    unsigned word = 0;
    const int n = (int)(total - i0 < 4 ? total - i0 : 4);
    for (int k = 0; k < n; ++k) {
        const int64_t b = (i0 + k) / V;
        const int v = (int)(i0 + k - b * V);
        const int lo = max(label_start[b], 0), hi = min(label_start[b + 1], num_labels);      // (a wrong table reads nothing out of bounds)
        unsigned hit = 0;
        for (int j = lo; j < hi; ++j) hit |= label_index[j] == v;
        word |= hit << (8 * k);
    }
    if (n == 4) *reinterpret_cast<unsigned*>(out + i0) = word;
    else
        for (int k = 0; k < n; ++k) out[i0 + k] = (unsigned char)(word >> (8 * k));
}

}  // namespace lpm

extern "C" int lpm_gather_frames(const void* buf, int64_t nbytes, int64_t capacity, const int64_t* frame_offset, const int32_t* num_frames,
                                 int B, int max_frames, const int* feature_sizes, int num_features, void* out, lpm_stream_t stream) {
    using namespace lpm;
    LPM_REQUIRE(buf && frame_offset && num_frames && feature_sizes && out, LPM_ERR_BADARG, "lpm_gather_frames: null pointer");
    LPM_REQUIRE(B > 0 && max_frames > 0 && nbytes >= 0, LPM_ERR_BADARG, "lpm_gather_frames: need B > 0, max_frames > 0, nbytes >= 0");
    LPM_REQUIRE(num_features >= 1 && num_features <= GATHER_MAX_FEATURES, LPM_ERR_UNSUPPORTED_SHAPE,
                "lpm_gather_frames: 1 to %d features (got %d)", GATHER_MAX_FEATURES, num_features);
    LPM_REQUIRE(capacity >= 16 && capacity >= ((nbytes + 15) & ~(int64_t)15), LPM_ERR_BADARG,
                "lpm_gather_frames: the buffer's capacity (%lld) must cover nbytes (%lld) rounded up to 16", (long long)capacity,
                (long long)nbytes);
    LPM_REQUIRE(((uintptr_t)buf & 15) == 0 && ((uintptr_t)out & 15) == 0, LPM_ERR_BADARG, "lpm_gather_frames: buf and out must be 16-byte aligned");
    GatherFeatures ft;
    ft.n = num_features;
    int64_t col = 0;
    for (int f = 0; f < num_features; ++f) {
        LPM_REQUIRE(feature_sizes[f] > 0 && feature_sizes[f] % 4 == 0, LPM_ERR_UNSUPPORTED_SHAPE,
                    "lpm_gather_frames: feature sizes must be positive multiples of 4 (feature %d: %d)", f, feature_sizes[f]);
        ft.start4[f] = (int)(col / 4);
        col += feature_sizes[f];
        LPM_REQUIRE(col <= (1 << 24), LPM_ERR_UNSUPPORTED_SHAPE, "lpm_gather_frames: rows of more than 2^24 bytes");
    }
    for (int f = num_features; f <= GATHER_MAX_FEATURES; ++f) ft.start4[f] = (int)(col / 4);
    const int64_t total4 = (int64_t)B * max_frames * (col / 4);
    const int64_t lanes = (total4 + 3) / 4, blocks = (lanes + GATHER_THREADS - 1) / GATHER_THREADS;
    LPM_REQUIRE(blocks <= 0x7FFFFFFF, LPM_ERR_UNSUPPORTED_SHAPE, "lpm_gather_frames: batch too large");
    hipLaunchKernelGGL(gather_frames_kernel, dim3((unsigned)blocks), dim3(GATHER_THREADS), 0, (hipStream_t)stream,
                       (const unsigned char*)buf, nbytes, capacity / 16, frame_offset, num_frames, max_frames, ft, (unsigned*)out, total4);
    return check_launch("lpm_gather_frames");
}

extern "C" int lpm_gather_examples(const void* buf, int64_t nbytes, int64_t capacity, const int64_t* feature_offset,
                                   const int32_t* feature_stride, int B, const int* feature_sizes, int num_features, void* out,
                                   lpm_stream_t stream) {
    using namespace lpm;
    LPM_REQUIRE(buf && feature_offset && feature_stride && feature_sizes && out, LPM_ERR_BADARG, "lpm_gather_examples: null pointer");
    LPM_REQUIRE(B > 0 && nbytes >= 0, LPM_ERR_BADARG, "lpm_gather_examples: need B > 0, nbytes >= 0");
    LPM_REQUIRE(num_features >= 1 && num_features <= GATHER_MAX_FEATURES, LPM_ERR_UNSUPPORTED_SHAPE,
                "lpm_gather_examples: 1 to %d features (got %d)", GATHER_MAX_FEATURES, num_features);
    LPM_REQUIRE(capacity >= 16 && capacity >= ((nbytes + 15) & ~(int64_t)15), LPM_ERR_BADARG,
                "lpm_gather_examples: the buffer's capacity (%lld) must cover nbytes (%lld) rounded up to 16", (long long)capacity,
                (long long)nbytes);
    LPM_REQUIRE(((uintptr_t)buf & 15) == 0 && ((uintptr_t)out & 15) == 0, LPM_ERR_BADARG,
                "lpm_gather_examples: buf and out must be 16-byte aligned");
    GatherFeatures ft;
    ft.n = num_features;
    int64_t col = 0;
    for (int f = 0; f < num_features; ++f) {
        LPM_REQUIRE(feature_sizes[f] > 0, LPM_ERR_UNSUPPORTED_SHAPE, "lpm_gather_examples: feature sizes must be positive (feature %d: %d)", f,
                    feature_sizes[f]);
        ft.start4[f] = (int)col;
        col += feature_sizes[f];
        LPM_REQUIRE(col <= (1 << 22), LPM_ERR_UNSUPPORTED_SHAPE, "lpm_gather_examples: rows of more than 2^22 floats");
    }
    for (int f = num_features; f <= GATHER_MAX_FEATURES; ++f) ft.start4[f] = (int)col;
    const int64_t total4 = (int64_t)B * col;
    const int64_t lanes = (total4 + 3) / 4, blocks = (lanes + GATHER_THREADS - 1) / GATHER_THREADS;
    LPM_REQUIRE(blocks <= 0x7FFFFFFF, LPM_ERR_UNSUPPORTED_SHAPE, "lpm_gather_examples: batch too large");
    hipLaunchKernelGGL(gather_examples_kernel, dim3((unsigned)blocks), dim3(GATHER_THREADS), 0, (hipStream_t)stream,
                       (const unsigned char*)buf, nbytes, capacity / 16, feature_offset, feature_stride, ft, (unsigned*)out, total4);
    return check_launch("lpm_gather_examples");
}

extern "C" int lpm_labels_dense(const int32_t* label_start, const int32_t* label_index, int num_labels, int B, int num_classes, void* out,
                                lpm_stream_t stream) {
    using namespace lpm;
    LPM_REQUIRE(label_start && out && num_labels >= 0 && (label_index || num_labels == 0), LPM_ERR_BADARG, "lpm_labels_dense: null pointer");
    LPM_REQUIRE(B > 0 && num_classes > 0, LPM_ERR_BADARG, "lpm_labels_dense: need B > 0 and num_classes > 0");
    LPM_REQUIRE(((uintptr_t)out & 3) == 0, LPM_ERR_BADARG, "lpm_labels_dense: out must be 4-byte aligned");
    const int64_t total = (int64_t)B * num_classes;
    const int64_t blocks = ((total + 3) / 4 + GATHER_THREADS - 1) / GATHER_THREADS;
    LPM_REQUIRE(blocks <= 0x7FFFFFFF, LPM_ERR_UNSUPPORTED_SHAPE, "lpm_labels_dense: batch too large");
    hipLaunchKernelGGL(labels_dense_kernel, dim3((unsigned)blocks), dim3(GATHER_THREADS), 0, (hipStream_t)stream, label_start, label_index,
                       num_labels, num_classes, total, (unsigned char*)out);
    return check_launch("lpm_labels_dense");
}

// ---- the host indexer (record_index.h) behind the C ABI; nothing here touches a device --------------------------------------------------
#if !defined(__HIP_DEVICE_COMPILE__)
static lpm_index::Err last_error_sink(char* tmp, size_t n) { return lpm_index::Err{tmp, n}; }

extern "C" int lpm_tfrecord_frame(const void* buf, int64_t nbytes, int verify_crc, int max_records, int64_t record_base, int64_t* rec_offset,
                                  int64_t* rec_length, int* num_records, int64_t* consumed) {
    LPM_REQUIRE((buf || nbytes == 0) && nbytes >= 0 && max_records >= 0 && (max_records == 0 || (rec_offset && rec_length)) && num_records &&
                    consumed,
                LPM_ERR_BADARG, "lpm_tfrecord_frame: bad argument");
    char why[256] = "";
    const int st = lpm_index::frame_records((const uint8_t*)buf, nbytes, verify_crc, max_records, record_base, rec_offset, rec_length,
                                            num_records, consumed, last_error_sink(why, sizeof why));
    if (st != LPM_OK) lpm::set_error("lpm_tfrecord_frame: %s", why);
    return st;
}

extern "C" int lpm_yt8m_locate(const void* buf, int64_t nbytes, const int64_t* rec_offset, const int64_t* rec_length, int num_records,
                               int64_t record_base, const char* const* feature_names, const int* feature_sizes, int num_features,
                               int max_frames, int num_classes, int32_t* num_frames, int64_t* frame_offset, int32_t* label_start,
                               int32_t* label_index, int64_t label_capacity, int64_t* labels_needed, int64_t* id_offset, int32_t* id_length,
                               int* failed_record) {
    LPM_REQUIRE(num_records >= 0 && nbytes >= 0 && (buf || nbytes == 0) && feature_names && feature_sizes && label_start && labels_needed &&
                    failed_record && label_capacity >= 0 && (label_index || label_capacity == 0),
                LPM_ERR_BADARG, "lpm_yt8m_locate: bad argument");
    LPM_REQUIRE(num_records == 0 || (rec_offset && rec_length && num_frames && frame_offset && id_offset && id_length), LPM_ERR_BADARG,
                "lpm_yt8m_locate: null output");
    LPM_REQUIRE(num_features >= 1 && num_features <= lpm_index::MAX_FEATURES && max_frames > 0 && num_classes >= 0, LPM_ERR_UNSUPPORTED_SHAPE,
                "lpm_yt8m_locate: 1 to %d features, max_frames > 0 (got %d, %d)", lpm_index::MAX_FEATURES, num_features, max_frames);
    for (int f = 0; f < num_features; ++f)
        LPM_REQUIRE(feature_names[f] && feature_sizes[f] > 0, LPM_ERR_BADARG, "lpm_yt8m_locate: feature %d has no name or size", f);
    const lpm_index::Selection sel{num_features, feature_names, feature_sizes, max_frames, num_classes};
    char why[320] = "";
    const int st = lpm_index::locate_records((const uint8_t*)buf, nbytes, rec_offset, rec_length, num_records, record_base, sel, num_frames,
                                             frame_offset, label_start, label_index, label_capacity, labels_needed, id_offset, id_length,
                                             failed_record, last_error_sink(why, sizeof why));
    if (st != LPM_OK) lpm::set_error("lpm_yt8m_locate: %s", why);
    return st;
}
extern "C" int lpm_yt8m_locate_examples(const void* buf, int64_t nbytes, const int64_t* rec_offset, const int64_t* rec_length, int num_records,
                                        int64_t record_base, const char* const* feature_names, const int* feature_sizes, int num_features,
                                        int num_classes, int64_t* feature_offset, int32_t* feature_stride, int32_t* label_start,
                                        int32_t* label_index, int64_t label_capacity, int64_t* labels_needed, int64_t* id_offset,
                                        int32_t* id_length, int* failed_record) {
    LPM_REQUIRE(num_records >= 0 && nbytes >= 0 && (buf || nbytes == 0) && feature_names && feature_sizes && label_start && labels_needed &&
                    failed_record && label_capacity >= 0 && (label_index || label_capacity == 0),
                LPM_ERR_BADARG, "lpm_yt8m_locate_examples: bad argument");
    LPM_REQUIRE(num_records == 0 || (rec_offset && rec_length && feature_offset && feature_stride && id_offset && id_length), LPM_ERR_BADARG,
                "lpm_yt8m_locate_examples: null output");
    LPM_REQUIRE(num_features >= 1 && num_features <= lpm_index::MAX_FEATURES && num_classes >= 0, LPM_ERR_UNSUPPORTED_SHAPE,
                "lpm_yt8m_locate_examples: 1 to %d features (got %d)", lpm_index::MAX_FEATURES, num_features);
    for (int f = 0; f < num_features; ++f)
        LPM_REQUIRE(feature_names[f] && feature_sizes[f] > 0 && feature_sizes[f] <= (1 << 22), LPM_ERR_BADARG,
                    "lpm_yt8m_locate_examples: feature %d has no name or size", f);
    const lpm_index::Selection sel{num_features, feature_names, feature_sizes, 1, num_classes};
    char why[320] = "";
    const int st = lpm_index::locate_example_records((const uint8_t*)buf, nbytes, rec_offset, rec_length, num_records, record_base, sel,
                                                     feature_offset, feature_stride, label_start, label_index, label_capacity, labels_needed,
                                                     id_offset, id_length, failed_record, last_error_sink(why, sizeof why));
    if (st != LPM_OK) lpm::set_error("lpm_yt8m_locate_examples: %s", why);
    return st;
}
#endif
