// "%.5f" of a float32 in integer arithmetic, for the device text writer (epg_textout.hip) and, compiled for the host, for the
// program that holds it against fmt_f5 of epg_io.cpp (tests/fmt_f5_check.cpp).  Plain C++: no floating-point operation and no
// library call decides a digit.
//
//   value = (-1)^sign * m * 2^e, m < 2^24 an integer (e = exponent - 150; denormals: e = -149)
//   q     = round-half-even(m * 100000 * 2^e): for e >= 0 a shift left (|value| < 2^31 means e <= 7, so q < 2^48); for e < 0 a shift
//           right by sh = -e with the remainder compared against half; sh >= 64 gives 0 because m * 100000 < 2^41
//   text  = ['-'] integer part of q / 100000 (1 .. 10 digits) '.' q % 100000 as five digits
// The sign is kept for -0.0 and for negatives that round to zero ("-0.00000"), as Python's float formatting and fmt_f5 keep it.
// Values the 48-bit path does not cover (NaN, +-inf, |value| >= 2^31: exponent field >= 158) are refused: f5_scale returns false.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define EPG_F5_FN __host__ __device__ inline
#else
#define EPG_F5_FN inline
#endif

namespace epgfmt {

constexpr int F5_MAX_LEN = 17;                              // '-' + 10 digits + '.' + 5 digits

// q of the header comment; false when the value is refused (then *q = 0: the value formats as 0.00000 of its sign)
EPG_F5_FN bool f5_scale(uint32_t bits, uint64_t* q) {
    const uint32_t ex = (bits >> 23) & 0xffu, man = bits & 0x7fffffu;
    *q = 0;
    if (ex >= 158u) return false;
    const uint64_t num = (uint64_t)(ex ? (man | 0x800000u) : man) * 100000ull;      // < 2^41
    const int e = ex ? (int)ex - 150 : -149;
    if (e >= 0) {
        *q = num << e;
        return true;
    }
    const int sh = -e;
    if (sh >= 64) return true;
    uint64_t qq = num >> sh;
    const uint64_t rem = num & ((1ull << sh) - 1ull), half = 1ull << (sh - 1);
    if (rem > half || (rem == half && (qq & 1ull))) ++qq;
    *q = qq;
    return true;
}

EPG_F5_FN int f5_int_digits(uint32_t ip) {
    int n = 1;
    if (ip >= 10u) n = 2;
    if (ip >= 100u) n = 3;
    if (ip >= 1000u) n = 4;
    if (ip >= 10000u) n = 5;
    if (ip >= 100000u) n = 6;
    if (ip >= 1000000u) n = 7;
    if (ip >= 10000000u) n = 8;
    if (ip >= 100000000u) n = 9;
    if (ip >= 1000000000u) n = 10;
    return n;
}

// bytes of the text of a value with scaled magnitude q
EPG_F5_FN int f5_len(uint32_t bits, uint64_t q) { return (int)(bits >> 31) + f5_int_digits((uint32_t)(q / 100000ull)) + 6; }

// put(i, c) for every byte i = 0 .. f5_len - 1 of the text, in no particular order; -> f5_len
template <typename PUT>
EPG_F5_FN int f5_emit(uint32_t bits, uint64_t q, PUT&& put) {
    const int neg = (int)(bits >> 31);
    uint32_t ip = (uint32_t)(q / 100000ull), frac = (uint32_t)(q - (uint64_t)ip * 100000ull);
    const int nd = f5_int_digits(ip);
    if (neg) put(0, '-');
    for (int k = nd - 1; k >= 0; --k) {
        put(neg + k, (char)('0' + (int)(ip % 10u)));
        ip /= 10u;
    }
    const int dot = neg + nd;
    put(dot, '.');
    for (int k = 5; k >= 1; --k) {
        put(dot + k, (char)('0' + (int)(frac % 10u)));
        frac /= 10u;
    }
    return dot + 6;
}

}  // namespace epgfmt
