// Checks csrc/format_pairs.h's "%g" against the C library's snprintf("%g") of the widened double, byte for byte and in length (every
// NaN is expected as "nan", Python's text), and its "%i" against snprintf("%i").  A stand-alone host program:
//
//     c++ -O2 -std=c++17 -pthread tools/format_pairs_exhaustive.cc -o format_pairs_exhaustive
//     ./format_pairs_exhaustive --all [--threads 16]       all 2^32 bit patterns
//     ./format_pairs_exhaustive --subset                   a stratified subset: for both signs and every exponent field the
//                                                          mantissas 0, 1, 2^23 - 1 and every 4099th one (about a million patterns)
//
// (the subset is what tests/test_format_pairs_host.py runs, also in a build with -fsanitize=address,undefined).  Prints one JSON line
// and returns 1 on any mismatch.
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "../learnablepoolingmethods_amd/csrc/format_pairs.h"

namespace {

std::atomic<uint64_t> g_checked{0}, g_bad{0};
std::atomic<uint32_t> g_first_bad{0};

bool check_bits(uint32_t bits) {
    float f;
    std::memcpy(&f, &bits, 4);
    char want[64];
    int nw;
    if (f != f) {
        std::strcpy(want, "nan");
        nw = 3;
    } else {
        nw = std::snprintf(want, sizeof want, "%g", (double)f);
    }
    unsigned char got[32];
    std::memset(got, 0xAA, sizeof got);
    const int ng = lpm::fmt::format_g_bits(bits, got);
    bool ok = ng == nw && ng <= lpm::fmt::kMaxFloat && std::memcmp(got, want, (size_t)nw) == 0;
    for (int i = ng > 0 ? ng : 0; i < (int)sizeof got; ++i) ok = ok && got[i] == 0xAA;      // nothing written behind the length
    return ok;
}

void record(bool ok, uint32_t bits) {
    if (!ok && g_bad.fetch_add(1) == 0) g_first_bad = bits;
}

void range(uint64_t lo, uint64_t hi) {
    uint64_t n = 0;
    for (uint64_t b = lo; b < hi; ++b, ++n) record(check_bits((uint32_t)b), (uint32_t)b);
    g_checked += n;
}

bool check_int(int32_t v) {
    char want[32];
    const int nw = std::snprintf(want, sizeof want, "%i", (int)v);
    unsigned char got[16];
    const int ng = lpm::fmt::format_int(v, got);
    return ng == nw && ng <= lpm::fmt::kMaxInt && std::memcmp(got, want, (size_t)nw) == 0;
}

}  // namespace

int main(int argc, char** argv) {
    bool all = false;
    int threads = 1;
    for (int i = 1; i < argc; ++i) {
        if (!std::strcmp(argv[i], "--all")) all = true;
        else if (!std::strcmp(argv[i], "--subset")) all = false;
        else if (!std::strcmp(argv[i], "--threads") && i + 1 < argc) threads = std::atoi(argv[++i]);
        else {
            std::fprintf(stderr, "usage: %s --all | --subset [--threads N]\n", argv[0]);
            return 2;
        }
    }
    if (threads < 1) threads = 1;
    if (threads > 16) threads = 16;
    uint64_t ints = 0, ints_bad = 0;
    const int32_t edge[] = {0, 1, -1, 9, 10, 99, 100, 65535, 65536, 2147483647, -2147483647 - 1, 1000000000, -1000000000, 999999999};
    for (int32_t v : edge) ints_bad += !check_int(v), ++ints;
    for (int64_t v = -2147483648LL; v <= 2147483647LL; v += 65521) ints_bad += !check_int((int32_t)v), ++ints;
    if (all) {
        std::vector<std::thread> pool;
        const uint64_t total = 1ull << 32, per = total / (uint64_t)threads + 1;
        for (int t = 0; t < threads; ++t) {
            const uint64_t lo = per * (uint64_t)t, hi = lo + per < total ? lo + per : total;
            if (lo < hi) pool.emplace_back(range, lo, hi);
        }
        for (auto& th : pool) th.join();
    } else {
        uint64_t n = 0;
        for (uint32_t sign = 0; sign < 2; ++sign)
            for (uint32_t field = 0; field < 256; ++field) {
                const uint32_t base = (sign << 31) | (field << 23);
                const uint32_t fixed[] = {0u, 1u, 0x7FFFFFu, 0x400000u, 0x3FFFFFu};
                for (uint32_t m : fixed) record(check_bits(base | m), base | m), ++n;
                for (uint32_t m = field % 4099u; m < 0x800000u; m += 4099u) record(check_bits(base | m), base | m), ++n;
            }
        for (uint32_t v = 100000; v <= 999999; v += 37) {     // n + 0.5: the exact ties
            const float f = (float)v + 0.5f;
            uint32_t b;
            std::memcpy(&b, &f, 4);
            record(check_bits(b), b), ++n;
        }
        g_checked += n;
    }
    std::printf("{\"mode\": \"%s\", \"float_patterns\": %llu, \"float_mismatches\": %llu, \"first_mismatch_bits\": \"0x%08x\", "
                "\"ints\": %llu, \"int_mismatches\": %llu}\n",
                all ? "all" : "subset", (unsigned long long)g_checked.load(), (unsigned long long)g_bad.load(), g_first_bad.load(),
                (unsigned long long)ints, (unsigned long long)ints_bad);
    return (g_bad.load() || ints_bad) ? 1 : 0;
}
