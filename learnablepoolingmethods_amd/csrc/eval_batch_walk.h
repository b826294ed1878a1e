// The address walk of lpm_eval_batch_stats (eval_batch_stats.hip) over the labels of one batch: n = B * V bytes, row-contiguous, at ANY
// byte address.  The flat range [0, n) is cut into
//   head   [0, head)                       the bytes in front of the first 16-byte boundary (at most 15, all n of them when the range ends first)
//   body   [head, head + 16 nvec)          nvec aligned 16-byte groups, one 16-byte load each
//   tail   [head + 16 nvec, n)             at most 15 bytes
// and byte e of the range belongs to column e % V (element e of a contiguous [B, V] matrix).  Worker w of W (a thread of the grid, or one turn
// of a host loop) takes the head bytes, the tail bytes and the groups numbered w, w + W, w + 2 W, ...; a group whose 16 bytes are all zero costs one load and
// one compare, and only a group with a nonzero byte looks up its column.  Every byte of the range is visited by exactly one worker.
// __host__ __device__: the kernel and tools/check_eval_batch_walk.cc (a host program, built with sanitizers) run the same code.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LPM_WALK_HD __host__ __device__ __forceinline__
#else
#define LPM_WALK_HD inline
#endif

namespace lpm {

struct alignas(16) EvalWalkGroup {
    uint32_t w[4];                                         // 16 label bytes, byte i of the group in bits [8 (i % 4), 8 (i % 4) + 8) of w[i / 4]
};

struct EvalWalk {
    int64_t n;                                             // bytes of the range
    int64_t head;                                          // bytes in front of the body
    int64_t nvec;                                          // 16-byte groups of the body
    int V;
    LPM_WALK_HD int64_t tail_begin() const { return head + 16 * nvec; }
    LPM_WALK_HD int64_t tail() const { return n - tail_begin(); }
};

LPM_WALK_HD EvalWalk eval_walk_make(uintptr_t address, int64_t B, int V) {
    EvalWalk wk;
    wk.n = B * (int64_t)V;
    wk.V = V;
    const int64_t to_boundary = (int64_t)((16u - (unsigned)(address & 15u)) & 15u);
    wk.head = to_boundary < wk.n ? to_boundary : wk.n;
    wk.nvec = (wk.n - wk.head) >> 4;
    return wk;
}

// the column of flat byte e (the 32-bit division where the range allows it)
LPM_WALK_HD int eval_walk_column(const EvalWalk& wk, int64_t e) {
    if (wk.n <= (int64_t)UINT32_MAX) return (int)((uint32_t)e % (uint32_t)wk.V);
    return (int)(e % wk.V);
}

// add(column) for every nonzero byte that worker `worker` of `workers` owns.  y: the first byte of the range.
template <typename Add>
LPM_WALK_HD void eval_walk_worker(const EvalWalk& wk, const unsigned char* y, int64_t worker, int64_t workers, Add add) {
    for (int64_t e = worker; e < wk.head; e += workers)
        if (y[e] != 0) add(eval_walk_column(wk, e));
    for (int64_t e = wk.tail_begin() + worker; e < wk.n; e += workers)
        if (y[e] != 0) add(eval_walk_column(wk, e));
    for (int64_t g = worker; g < wk.nvec; g += workers) {
        const int64_t e0 = wk.head + 16 * g;
        const EvalWalkGroup v = *reinterpret_cast<const EvalWalkGroup*>(y + e0);
        if ((v.w[0] | v.w[1] | v.w[2] | v.w[3]) == 0u) continue;
        int c = eval_walk_column(wk, e0);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t word = v.w[q];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if ((word >> (8 * u)) & 0xFFu) add(c);
                if (++c == wk.V) c = 0;                    // the group runs into the next row (several times when V < 16)
            }
        }
    }
}

}  // namespace lpm
