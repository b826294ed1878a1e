// Host check of lpm_eval_batch_stats' address walk (learnablepoolingmethods_amd/csrc/eval_batch_walk.h: the head bytes, the aligned 16-byte
// groups, the tail bytes, and the column of every byte) against a plain double loop over rows and columns.
//     c++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all tools/check_eval_batch_walk.cc -o check_eval_batch_walk
//     ./check_eval_batch_walk [--cases N] [--seed S]
// Every case draws B, V, the start offset of the labels inside a 16-byte aligned allocation (0 .. 15), a label density (0, sparse, 0.5, 1) and a
// worker count, fills exactly B * V bytes -- the allocation ends where the labels end, so AddressSanitizer sees any read past them -- and runs
// every worker of the walk in turn.  It checks that the counts per column equal the double loop's and that every nonzero byte was visited once.
// Prints one JSON line; exit status 0 when nothing differs.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../learnablepoolingmethods_amd/csrc/eval_batch_walk.h"

namespace {

struct Case {
    int B, V, offset, workers;
    double density;
};

// -> the number of columns whose count differs (0 = the walk is right)
int64_t run_case(const Case& c, std::mt19937_64& rng) {
    const int64_t n = (int64_t)c.B * c.V;
    std::vector<unsigned char> exact((size_t)(c.offset + n));
    std::uniform_real_distribution<double> u(0.0, 1.0);
    for (int64_t e = 0; e < n; ++e) {
        unsigned char b = 0;
        if (c.density >= 1.0 || (c.density > 0.0 && u(rng) < c.density)) b = (rng() & 1) ? 1 : (unsigned char)(1 + rng() % 255);   // any nonzero byte counts
        exact[(size_t)(c.offset + e)] = b;
    }
    // a 16-byte aligned allocation of exactly offset + n bytes: a read past the last label lands in the sanitizer's red zone
    const size_t bytes = (size_t)(c.offset + n);
    void* mem = nullptr;
    if (posix_memalign(&mem, 16, bytes) != 0) std::abort();
    unsigned char* buf = static_cast<unsigned char*>(mem);
    std::memcpy(buf, exact.data(), bytes);
    const unsigned char* y = buf + c.offset;

    std::vector<int64_t> want((size_t)c.V, 0), got((size_t)c.V, 0);
    for (int r = 0; r < c.B; ++r)
        for (int col = 0; col < c.V; ++col) want[(size_t)col] += y[(int64_t)r * c.V + col] != 0;

    const lpm::EvalWalk wk = lpm::eval_walk_make((uintptr_t)y, c.B, c.V);
    int64_t bad = 0;
    if (wk.head < 0 || wk.head > 15 || wk.nvec < 0 || wk.tail() < 0 || wk.tail() > 15 || wk.head + 16 * wk.nvec + wk.tail() != n) ++bad;
    if (wk.nvec > 0 && ((uintptr_t)(y + wk.head) & 15u) != 0) ++bad;
    for (int64_t w = 0; w < c.workers; ++w)
        lpm::eval_walk_worker(wk, y, w, (int64_t)c.workers, [&](int col) {
            if (col < 0 || col >= c.V) std::abort();
            ++got[(size_t)col];
        });
    for (int col = 0; col < c.V; ++col) bad += want[(size_t)col] != got[(size_t)col];
    std::free(buf);
    return bad;
}

}  // namespace

int main(int argc, char** argv) {
    int cases = 400;
    uint64_t seed = 1;
    for (int i = 1; i < argc; ++i) {
        if (!std::strcmp(argv[i], "--cases") && i + 1 < argc) cases = std::atoi(argv[++i]);
        else if (!std::strcmp(argv[i], "--seed") && i + 1 < argc) seed = std::strtoull(argv[++i], nullptr, 10);
        else {
            std::fprintf(stderr, "usage: %s [--cases N] [--seed S]\n", argv[0]);
            return 2;
        }
    }
    std::mt19937_64 rng(seed);
    const double densities[4] = {0.0, 0.002, 0.5, 1.0};
    // fixed cases first: one byte, rows shorter than a group, the model's row length, a walk with fewer than 15 workers
    std::vector<Case> list = {{1, 1, 0, 1, 1.0},   {1, 1, 15, 256, 1.0}, {1, 2, 7, 256, 1.0},   {3, 5, 1, 256, 1.0},   {7, 3, 13, 64, 0.5},
                              {5, 16, 0, 3, 1.0},  {5, 17, 9, 3, 1.0},    {80, 3862, 2, 512, 0.002}, {9, 3862, 3, 512, 1.0}, {2, 65536, 5, 1024, 0.5}};
    for (int i = 0; i < cases; ++i) {
        Case c;
        const int kind = (int)(rng() % 4);
        c.B = kind == 0 ? 1 + (int)(rng() % 4) : 1 + (int)(rng() % 300);
        c.V = kind == 1 ? 1 + (int)(rng() % 40) : kind == 2 ? 3800 + (int)(rng() % 400) : 1 + (int)(rng() % 700);
        c.offset = (int)(rng() % 16);
        c.workers = 1 << (int)(rng() % 12);
        c.density = densities[rng() % 4];
        list.push_back(c);
    }
    int64_t bad_cases = 0, bytes = 0;
    for (const Case& c : list) {
        const int64_t bad = run_case(c, rng);
        bytes += (int64_t)c.B * c.V;
        if (bad) {
            ++bad_cases;
            std::fprintf(stderr, "mismatch: B=%d V=%d offset=%d workers=%d density=%g (%lld columns)\n", c.B, c.V, c.offset, c.workers, c.density,
                         (long long)bad);
        }
    }
    std::printf("{\"cases\": %zu, \"bytes\": %lld, \"bad_cases\": %lld}\n", list.size(), (long long)bytes, (long long)bad_cases);
    return bad_cases ? 1 : 0;
}
