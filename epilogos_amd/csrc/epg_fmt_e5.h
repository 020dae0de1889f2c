// "%.5e" of a float64 in [0, 1] in integer arithmetic, for the device metrics writer (epg_metrics_text.hip) and, compiled for the host,
// for the program that holds it against snprintf (tests/fmt_e5_check.cpp).  Plain C++: no floating-point operation and no library
// call decides a digit.  The domain is what a p-value is: sign bit clear, value <= 1, denormals included.  Everything else -- a set
// sign bit (-0.0 too), a value above 1, NaN, infinity -- is refused: e5_scale returns false.
//
//   x     = m * 2^e, m < 2^53 an integer (e = exponent - 1075; denormals: e = -1074), k = floor(log10 x)
//   p     = 5 - k >= 5: x * 10^p = m * 5^p * 2^(e + p) lies in [10^5, 10^6); no division anywhere
//   s     = -(e + p).  In the domain the shift is always a right shift: with E = floor(log2 x), p <= 7 + 0.30103 |E|, and e <= -52 with
//           E = e + 52 (normal) or e = -1074 with |E| <= 1074 (denormal) give e + p <= -45; and s <= 1074 - 313 = 761 stays inside the
//           product.  e5_scale still checks both before it indexes
//   q     = round-half-even(m * 5^p >> s): the bit below the cut and the OR of all bits below that one are "half" and "more"
//   k is first ESTIMATED as floor(floor(log2 x) * log10 2), which is k or k - 1 (and the constant's own error could make it k + 1):
//           an estimate that is off shows as q < 10^5 or q >= 10^6 BEFORE rounding and is corrected then; q == 10^6 AFTER rounding
//           is 1.00000 of k + 1
//   text  = d.ddddd 'e' sign of k, |k| in at least two digits: 11 bytes, 12 below 1e-99; zero is 0.00000e+00
//
// m * 5^p has at most 53 + 767 bits (p <= 330).  5^p = 5^(p & 15) * 5^(16 * (p >> 4)): the first factor fits 35 bits, the second is
// one of 21 rows of a table of 24 32-bit limbs that a constexpr function builds at compile time.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define EPG_E5_FN __host__ __device__ inline
#else
#define EPG_E5_FN inline
#endif

namespace epgfmt {

constexpr int E5_MAX_LEN = 12;                              // "d.ddddde-ddd"
constexpr int E5_ROWS = 21, E5_LIMBS = 24, E5_PROD = E5_LIMBS + 3;

struct E5Pow16 {
    uint32_t w[E5_ROWS][E5_LIMBS];                          // w[j] = 5^(16 j), little-endian limbs
};

constexpr E5Pow16 e5_make_pow16() {
    E5Pow16 t{};
    t.w[0][0] = 1u;
    for (int j = 1; j < E5_ROWS; ++j) {
        for (int i = 0; i < E5_LIMBS; ++i) t.w[j][i] = t.w[j - 1][i];
        for (int twice = 0; twice < 2; ++twice) {           // times 5^8 = 390625, twice: a limb times 19 bits stays in 64
            uint64_t carry = 0;
            for (int i = 0; i < E5_LIMBS; ++i) {
                const uint64_t v = (uint64_t)t.w[j][i] * 390625ull + carry;
                t.w[j][i] = (uint32_t)v;
                carry = v >> 32;
            }
        }
    }
    return t;
}

// 5^0 .. 5^15
constexpr uint64_t E5_POW_LO[16] = {1ull, 5ull, 25ull, 125ull, 625ull, 3125ull, 15625ull, 78125ull, 390625ull, 1953125ull, 9765625ull, 48828125ull,
                                    244140625ull, 1220703125ull, 6103515625ull, 30517578125ull};

// round-half-even(m * 5^p / 2^s) and floor of the same, for 5 <= p <= 335 and 1 <= s < 32 * (E5_PROD - 1); the quotient must fit 32 bits
EPG_E5_FN uint32_t e5_shifted(uint64_t m, int p, int s, uint32_t* floor_q) {
    static constexpr E5Pow16 T = e5_make_pow16();
    // a = m * 5^(p & 15): 53 + 35 bits in three limbs
    const uint64_t f = E5_POW_LO[p & 15];
    const uint64_t m0 = m & 0xffffffffull, m1 = m >> 32, f0 = f & 0xffffffffull, f1 = f >> 32;
    const uint64_t c00 = m0 * f0, c01 = m0 * f1, c10 = m1 * f0, c11 = m1 * f1;
    uint32_t a[3];
    a[0] = (uint32_t)c00;
    uint64_t mid = (c00 >> 32) + (c01 & 0xffffffffull) + (c10 & 0xffffffffull);
    a[1] = (uint32_t)mid;
    mid = (mid >> 32) + (c01 >> 32) + (c10 >> 32) + c11;   // < 2^32: the product has 88 bits
    a[2] = (uint32_t)mid;
    // N = a * 5^(16 (p >> 4)), schoolbook
    const uint32_t* t = T.w[p >> 4];
    uint32_t N[E5_PROD];
    for (int i = 0; i < E5_PROD; ++i) N[i] = 0u;
    for (int i = 0; i < 3; ++i) {
        uint64_t carry = 0;
        for (int j = 0; j < E5_LIMBS; ++j) {
            const uint64_t v = (uint64_t)a[i] * t[j] + N[i + j] + carry;
            N[i + j] = (uint32_t)v;
            carry = v >> 32;
        }
        N[i + E5_LIMBS] = (uint32_t)carry;
    }
    const int w = s >> 5, b = s & 31;
    uint32_t q = N[w] >> b;
    if (b) q |= N[w + 1] << (32 - b);
    const int hs = s - 1, hw = hs >> 5, hb = hs & 31;
    const bool half = (N[hw] >> hb) & 1u;
    uint32_t more = N[hw] & ((1u << hb) - 1u);
    for (int i = 0; i < hw; ++i) more |= N[i];
    *floor_q = q;
    if (half && (more != 0u || (q & 1u))) ++q;
    return q;
}

// q in [100000, 1000000) and k with x = q * 10^(k - 5) after rounding (q = 0, k = 0 for zero); false when the value is refused
// (then *q = 0 and *k = 0: the value formats as zero)
EPG_E5_FN bool e5_scale(uint64_t bits, uint32_t* q, int* k) {
    *q = 0u;
    *k = 0;
    if (bits > 0x3ff0000000000000ull) return false;         // the sign bit, NaN, inf and everything above 1.0 order above its bits
    if (bits == 0ull) return true;
    const int ex = (int)(bits >> 52);
    const uint64_t man = bits & 0xfffffffffffffull;
    const uint64_t m = ex ? (man | (1ull << 52)) : man;
    const int e = ex ? ex - 1075 : -1074;
    int top = 52;                                           // the highest set bit of m
    while (!((m >> top) & 1ull)) --top;
    const long long E = (long long)e + top;                 // floor(log2 x) <= 0
    // floor(E * log10(2)) with log10(2) = 1292913986 / 2^32 (rounded down): E <= 0, so the floor is minus the ceiling of the positive product
    const long long pos = -E * 1292913986ll;
    int kk = -(int)((pos + 0xffffffffll) >> 32);
    uint32_t qq = 0u, fl = 0u;
    for (int turn = 0; turn < 3; ++turn) {
        const int p = 5 - kk, s = -(e + p);
        if (p < 5 || p > 335 || s < 1 || s >= 32 * (E5_PROD - 1)) return false;    // (not reached in the domain, see above)
        qq = e5_shifted(m, p, s, &fl);
        if (fl < 100000u) --kk;
        else if (fl >= 1000000u) ++kk;
        else break;
    }
    if (qq == 1000000u) {
        qq = 100000u;
        ++kk;
    }
    *q = qq;
    *k = kk;
    return true;
}

// bytes of the text of a value with exponent k
EPG_E5_FN int e5_len(int k) { return k <= -100 ? 12 : 11; }

// put(i, c) for every byte i = 0 .. e5_len - 1 of the text, in no particular order; -> e5_len
template <typename PUT>
EPG_E5_FN int e5_emit(uint32_t q, int k, PUT&& put) {
    uint32_t d = q;
    for (int i = 6; i >= 2; --i) {
        put(i, (char)('0' + (int)(d % 10u)));
        d /= 10u;
    }
    put(1, '.');
    put(0, (char)('0' + (int)d));
    put(7, 'e');
    put(8, k < 0 ? '-' : '+');
    uint32_t a = (uint32_t)(k < 0 ? -k : k);
    const int nd = a >= 100u ? 3 : 2;
    for (int i = nd - 1; i >= 0; --i) {
        put(9 + i, (char)('0' + (int)(a % 10u)));
        a /= 10u;
    }
    return 9 + nd;
}

}  // namespace epgfmt
