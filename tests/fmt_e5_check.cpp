// Stand-alone host program: the device writer's "%.5e" (csrc/epg_fmt_e5.h, integer arithmetic, compiled here for the host) against
// snprintf("%.5e"), which is what epgio_write_metrics (csrc/epg_io.cpp) prints, over the edge values, their neighbours, doubles in
// [0, 1] drawn three ways and decimal six-digit ties.
//   g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -Iepilogos_amd/csrc tests/fmt_e5_check.cpp \
//       -o fmt_e5_check && ./fmt_e5_check 10000000
// Exit code 0 and "fmt_e5_check: N values, M refused, 0 differ" when every value of the domain formats to snprintf's bytes and every
// value outside it -- sign bit set, above 1, NaN, infinite -- is refused, and no value of the domain is.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "epg_fmt_e5.h"

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint64_t next64() {
    g_state ^= g_state << 13;
    g_state ^= g_state >> 7;
    g_state ^= g_state << 17;
    return g_state * 0x2545F4914F6CDD1Dull;
}

static double as_double(uint64_t u) {
    double d;
    memcpy(&d, &u, 8);
    return d;
}
static uint64_t as_bits(double d) {
    uint64_t u;
    memcpy(&u, &d, 8);
    return u;
}

static long long g_done = 0, g_refused = 0, g_differ = 0, g_three = 0;

static bool in_domain(uint64_t u) {
    const double d = as_double(u);
    return !(u >> 63) && d <= 1.0;                          // (NaN compares false)
}

static void check(uint64_t u) {
    ++g_done;
    uint32_t q;
    int k;
    const bool ok = epgfmt::e5_scale(u, &q, &k);
    if (ok != in_domain(u)) {
        if (g_differ < 10) printf("%016llx: %s\n", (unsigned long long)u, ok ? "accepted outside the domain" : "refused inside the domain");
        ++g_differ;
        return;
    }
    if (!ok) {
        ++g_refused;
        return;
    }
    char want[64], got[16];
    const int n = snprintf(want, sizeof want, "%.5e", as_double(u));
    memset(got, 0, sizeof got);
    const int L = epgfmt::e5_emit(q, k, [&](int at, char c) {
        if (at < 0 || at >= epgfmt::E5_MAX_LEN) abort();
        got[at] = c;
    });
    if (L == 12) ++g_three;
    if (L != epgfmt::e5_len(k) || L != n || memcmp(got, want, (size_t)n) != 0) {
        if (g_differ < 10) printf("%016llx: snprintf %s device %.*s\n", (unsigned long long)u, want, L, got);
        ++g_differ;
    }
}

static void check_around(double v) {
    const uint64_t u = as_bits(v);
    check(u);
    check(u + 1);
    if (u) check(u - 1);
}

int main(int argc, char** argv) {
    const long long N = argc > 1 ? atoll(argv[1]) : 10000000ll;
    for (double v : {0.0, 1.0, 0.5, 0.1, 5e-324, 2.2250738585072014e-308, 1e-99, 9.999996e-100, 1e-100, 9.999995e-5, 0.9999995, 9.9999995e-100,
                     9.9999949999999e-100, 1e-5, 1e-10, 0.99999949999999, 0.3, 1.5e-323})
        check_around(v);
    // outside the domain: every one is refused (check() holds e5_scale's answer against in_domain)
    for (double v : {-0.0, -1e-5, -1.0, -5e-324, 2.0, 1e300, (double)INFINITY, (double)-INFINITY, (double)NAN, -(double)NAN}) check(as_bits(v));
    check(0x3ff0000000000001ull);                           // the double above 1
    check(0x7ff0000000000001ull);
    check(0xfff8000000000000ull);
    const long long refused_edges = g_refused;
    if (refused_edges != 14) { printf("expected 14 refused edge values, got %lld\n", refused_edges); return 1; }   // (1.0 + 1 ulp of check_around too)
    // decimal six-digit ties d.ddddd5e-k and the doubles next to them
    for (int i = 0; i < 100000; ++i) {
        char txt[40];
        const unsigned d = 100000u + (unsigned)(next64() % 900000ull), ex = (unsigned)(next64() % 324ull);
        snprintf(txt, sizeof txt, "%u.%05u5e-%u", d / 100000u, d % 100000u, ex);
        double v = strtod(txt, nullptr);
        if (v > 1.0) v = 1.0;
        check_around(v);
    }
    const long long third = N / 3;
    for (long long i = 0; i < third; ++i) check(as_bits((double)(next64() >> 11) * (1.0 / 9007199254740992.0)));     // uniform in [0, 1)
    for (long long i = 0; i < third; ++i)                                                                             // every exponent alike
        check(((next64() % 1023ull) << 52) | (next64() >> 12));
    for (long long i = 0; i < N - 2 * third; ++i) {                                                                   // random bit patterns:
        uint64_t u = next64();                                                                                        // one in 16 as it comes,
        if (i & 15) u &= 0x3fffffffffffffffull;                                                                       // the others below 2.0
        check(u);
    }
    printf("fmt_e5_check: %lld values, %lld refused, %lld with a three-digit exponent, %lld differ\n", g_done, g_refused, g_three, g_differ);
    return g_differ ? 1 : 0;
}
