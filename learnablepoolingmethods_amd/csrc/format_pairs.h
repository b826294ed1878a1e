// The text of an int32 as "%i" and of an fp32 as Python's "%g" % float(x) (precision 6, of the exactly widened value), byte for byte,
// for the host and the device from one source: csv_rows.hip's kernel and its host entry, tools/format_pairs_exhaustive.cc.
//
// %g: a finite non-zero float is m * 2^e with m < 2^24 and e in [-149, 104].  With X the decimal exponent and p = 5 - X the six digits
// are q = round-half-even(m * 2^e * 10^p) = round(m * 5^p * 2^(e + p)), formed in integers only (five 32-bit limbs: m * 5^50 has 141
// bits):
//   p >= 0:  N = m * 5^p, shifted by e + p; the bits shifted out say whether the remainder is below, at or above one half;
//   p <  0:  m * 2^max(e + p, 0) divided by 5^(-p) * 2^max(-(e + p), 0) by restoring division (the quotient is below 2^21), the
//            doubled remainder compared with the divisor.
// X is first taken from the binary exponent (floor(log10(2^k)) for 2^k <= |x| < 2^(k+1): the true X or one below it); q >= 10^6 --
// from the value itself or from the rounding's carry -- means X + 1, and the digits are formed again there.  Style, zero stripping and
// the exponent's form follow C's %g; every NaN prints "nan" (Python's text, not glibc's "-nan").
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LPM_FMT_HD __host__ __device__ inline
#else
#define LPM_FMT_HD inline
#endif
#if defined(__clang__)
#define LPM_FMT_UNROLL _Pragma("unroll")
#else
#define LPM_FMT_UNROLL
#endif

namespace lpm {
namespace fmt {

constexpr int kMaxInt = 11;       // "-2147483648"
constexpr int kMaxFloat = 12;     // "-1.17549e-38"
constexpr int kMaxPair = kMaxInt + 1 + kMaxFloat + 1;      // index, space, score, space or newline: 25

struct U160 {
    uint32_t w[5];                // w[0] the least significant limb
};

// limb i of u, zero outside [0, 5): selects, so that a variable i never indexes the array (registers on the device)
LPM_FMT_HD uint32_t limb(const U160& u, int i) {
    uint32_t r = 0;
LPM_FMT_UNROLL
    for (int j = 0; j < 5; ++j) r = (i == j) ? u.w[j] : r;
    return r;
}

LPM_FMT_HD void mul_small(U160& u, uint32_t c) {
    uint64_t carry = 0;
LPM_FMT_UNROLL
    for (int j = 0; j < 5; ++j) {
        const uint64_t t = (uint64_t)u.w[j] * c + carry;
        u.w[j] = (uint32_t)t;
        carry = t >> 32;
    }
}

// u * 5^n, 0 <= n <= 50
LPM_FMT_HD void mul_pow5(U160& u, int n) {
    for (; n >= 13; n -= 13) mul_small(u, 1220703125u);           // 5^13, the largest power in 32 bits
    uint32_t c = 1;
    for (int i = 0; i < n; ++i) c *= 5u;
    mul_small(u, c);
}

// u << n, 0 <= n < 160 (the bits above 160 are dropped: the callers stay below)
LPM_FMT_HD U160 shl(const U160& u, int n) {
    const int ws = n >> 5, bs = n & 31;
    U160 r;
LPM_FMT_UNROLL
    for (int j = 0; j < 5; ++j) {
        const uint32_t hi = limb(u, j - ws), lo = limb(u, j - ws - 1);
        r.w[j] = bs ? (hi << bs) | (lo >> (32 - bs)) : hi;
    }
    return r;
}

// the low 32 bits of u >> n, 0 <= n < 160
LPM_FMT_HD uint32_t shr32(const U160& u, int n) {
    const int ws = n >> 5, bs = n & 31;
    const uint32_t lo = limb(u, ws), hi = limb(u, ws + 1);
    return bs ? (lo >> bs) | (hi << (32 - bs)) : lo;
}

// whether any of the bits [0, n) of u is set, 0 <= n <= 160
LPM_FMT_HD bool any_below(const U160& u, int n) {
    const int ws = n >> 5, bs = n & 31;
    uint32_t acc = 0;
LPM_FMT_UNROLL
    for (int j = 0; j < 5; ++j) acc |= (j < ws) ? u.w[j] : 0u;
    if (bs) acc |= limb(u, ws) & ((1u << bs) - 1u);
    return acc != 0;
}

LPM_FMT_HD void shr1(U160& u) {
LPM_FMT_UNROLL
    for (int j = 0; j < 4; ++j) u.w[j] = (u.w[j] >> 1) | (u.w[j + 1] << 31);
    u.w[4] >>= 1;
}

LPM_FMT_HD bool geq(const U160& a, const U160& b) {          // a >= b
    bool r = true;                                           // (equal so far, from the lowest limb up: a higher limb overrides)
LPM_FMT_UNROLL
    for (int j = 0; j < 5; ++j) r = (a.w[j] != b.w[j]) ? (a.w[j] > b.w[j]) : r;
    return r;
}

LPM_FMT_HD bool equal(const U160& a, const U160& b) {
    uint32_t d = 0;
LPM_FMT_UNROLL
    for (int j = 0; j < 5; ++j) d |= a.w[j] ^ b.w[j];
    return d == 0;
}

LPM_FMT_HD void sub(U160& a, const U160& b) {                // a -= b, a >= b
    uint32_t borrow = 0;
LPM_FMT_UNROLL
    for (int j = 0; j < 5; ++j) {
        const uint64_t t = (uint64_t)a.w[j] - b.w[j] - borrow;
        a.w[j] = (uint32_t)t;
        borrow = (uint32_t)(t >> 32) & 1u;
    }
}

// round-half-even(m * 2^e * 10^p) for a result below 2^24: 0 < m < 2^24, e in [-149, 104], p in [-33, 50]
LPM_FMT_HD uint32_t scaled_digits(uint32_t m, int e, int p) {
    const int s = e + p;
    U160 n = {{m, 0, 0, 0, 0}};
    uint32_t q;
    int half;                                                // the remainder against one half: -1 below, 0 at, 1 above
    if (p >= 0) {
        mul_pow5(n, p);
        if (s >= 0) return shr32(shl(n, s), 0);              // an integer
        const int r = -s;                                    // q = n >> r; r is at most 105 (the float just below 2^-126)
        q = shr32(n, r);
        const bool top = (shr32(n, r - 1) & 1u) != 0, rest = any_below(n, r - 1);
        half = !top ? -1 : (rest ? 1 : 0);
    } else {
        U160 d = {{1, 0, 0, 0, 0}};
        mul_pow5(d, -p);
        if (s >= 0) n = shl(n, s);
        else d = shl(d, -s);
        U160 ds = shl(d, 23);                                // (d has at most 84 bits, n at most 95)
        q = 0;
        for (int i = 23; i >= 0; --i) {
            if (geq(n, ds)) {
                sub(n, ds);
                q |= 1u << i;
            }
            if (i) shr1(ds);
        }
        const U160 twice = shl(n, 1);                        // the remainder n < d
        half = equal(twice, d) ? 0 : (geq(twice, d) ? 1 : -1);
    }
    if (half > 0 || (half == 0 && (q & 1u))) ++q;
    return q;
}

// "%i": -> the number of bytes written (at most kMaxInt)
template <typename P>
LPM_FMT_HD int format_int(int32_t v, P out) {
    uint32_t a = v < 0 ? 0u - (uint32_t)v : (uint32_t)v;
    int nd = 1;
    for (uint32_t t = a; t >= 10u; t /= 10u) ++nd;
    int n = 0;
    if (v < 0) out[n++] = '-';
    for (int i = nd - 1; i >= 0; --i) {
        out[n + i] = (unsigned char)('0' + a % 10u);
        a /= 10u;
    }
    return n + nd;
}

// "%g" of the float with these bits: -> the number of bytes written (at most kMaxFloat)
template <typename P>
LPM_FMT_HD int format_g_bits(uint32_t bits, P out) {
    int n = 0;
    const uint32_t frac = bits & 0x7FFFFFu;
    const int field = (int)((bits >> 23) & 0xFFu);
    if (field == 0xFF && frac) {
        out[0] = 'n'; out[1] = 'a'; out[2] = 'n';
        return 3;
    }
    if (bits >> 31) out[n++] = '-';
    if (field == 0xFF) {
        out[n] = 'i'; out[n + 1] = 'n'; out[n + 2] = 'f';
        return n + 3;
    }
    if (field == 0 && frac == 0) {
        out[n] = '0';
        return n + 1;
    }
    const uint32_t m = field ? (frac | 0x800000u) : frac;
    const int e = (field ? field : 1) - 150;
    int k = e - 1;                                           // 2^k <= |x| < 2^(k+1): the position of m's highest bit
    for (uint32_t t = m; t; t >>= 1) ++k;
    const int t = k * 78913;                                 // floor(k log10(2)) = floor(k * 78913 / 2^18) for |k| <= 1650
    int X = t >= 0 ? t >> 18 : -((-t + 262143) >> 18);
    uint32_t q = scaled_digits(m, e, 5 - X);
    if (q >= 1000000u) {
        ++X;
        q = scaled_digits(m, e, 5 - X);
    }
    unsigned char d[6];
LPM_FMT_UNROLL
    for (int i = 5; i >= 0; --i) {
        d[i] = (unsigned char)('0' + q % 10u);
        q /= 10u;
    }
    int nz = 6;                                              // significant digits without the trailing zeros
LPM_FMT_UNROLL
    for (int i = 5; i >= 1; --i) nz = (nz == i + 1 && d[i] == '0') ? i : nz;
    if (X < -4 || X >= 6) {
        out[n++] = d[0];
        if (nz > 1) out[n++] = '.';
LPM_FMT_UNROLL
        for (int i = 1; i < 6; ++i)
            if (i < nz) out[n++] = d[i];
        out[n++] = 'e';
        out[n++] = X < 0 ? '-' : '+';
        const int a = X < 0 ? -X : X;                        // at most 45: two digits
        out[n++] = (unsigned char)('0' + a / 10);
        out[n++] = (unsigned char)('0' + a % 10);
    } else if (X >= 0) {
LPM_FMT_UNROLL
        for (int i = 0; i < 6; ++i) {
            if (i <= X || i < nz) out[n++] = d[i];
            if (i == X && nz > X + 1) out[n++] = '.';
        }
    } else {
        out[n++] = '0';
        out[n++] = '.';
        for (int i = 0; i < -X - 1; ++i) out[n++] = '0';
LPM_FMT_UNROLL
        for (int i = 0; i < 6; ++i)
            if (i < nz) out[n++] = d[i];
    }
    return n;
}

// "<index> <score>" followed by `last`: one item of a row.  -> the number of bytes written (at most kMaxPair)
template <typename P>
LPM_FMT_HD int format_pair(int32_t index, uint32_t score_bits, unsigned char last, P out) {
    int n = format_int(index, out);
    out[n++] = ' ';
    n += format_g_bits(score_bits, out + n);
    out[n++] = last;
    return n;
}

}  // namespace fmt
}  // namespace lpm
