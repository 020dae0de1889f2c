// Stand-alone host program: the device writer's "%.5f" (csrc/epg_fmt_f5.h, integer arithmetic, compiled here for the host) against
// the host writer's fmt_f5 (csrc/epg_io.cpp, through epgio_format_f5) over random float32 bit patterns and the edge values.
//   g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -pthread -Iinclude -Iepilogos_amd/csrc \
//       tests/fmt_f5_check.cpp epilogos_amd/csrc/epg_io.cpp -lz -o fmt_f5_check && ./fmt_f5_check 10000000
// Exit code 0 and "fmt_f5_check: N patterns, M refused, 0 differ" when every accepted pattern formats to the same bytes and every
// refused one is NaN, an infinity or at least 2^31 in magnitude.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "epg_fmt_f5.h"
#include "epilogos_io.h"

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t next_bits() {
    g_state ^= g_state << 13;
    g_state ^= g_state >> 7;
    g_state ^= g_state << 17;
    return (uint32_t)(g_state >> 16);
}

static float as_float(uint32_t u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}
static uint32_t as_bits(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

int main(int argc, char** argv) {
    const long long N = argc > 1 ? atoll(argv[1]) : 10000000ll;
    std::vector<uint32_t> edge;
    for (float v : {0.0f, 1e-6f, 0.015625f, 0.046875f, 9.999995f, 99999.99f, 1.401298464e-45f, 2147483520.0f, 0.5f, 1.0f, 0.000005f, 0.999995f,
                    1073741824.0f, 16777216.0f, 8388608.0f}) {
        edge.push_back(as_bits(v));
        edge.push_back(as_bits(v) | 0x80000000u);
    }
    const int B = 4096;
    std::vector<float> vals(B);
    std::vector<char> want(48 * B + 1), got(20);
    long long done = 0, refused = 0, differ = 0;
    size_t e = 0;
    while (done < N) {
        int n = 0;
        while (n < B && done + n < N) {
            const bool is_edge = e < edge.size();
            uint32_t u = is_edge ? edge[e++] : next_bits();
            if (!is_edge && (next_bits() & 3) == 0) u = (u & 0x807fffffu) | ((100u + next_bits() % 60u) << 23);   // the exponents scores have
            uint64_t q;
            if (!epgfmt::f5_scale(u, &q)) {
                const uint32_t ex = (u >> 23) & 0xffu;
                if (ex < 158u) { printf("refused a value below 2^31: %08x\n", u); return 1; }
                ++refused;
                ++done;
                continue;
            }
            vals[n++] = as_float(u);
        }
        const int64_t len = epgio_format_f5(vals.data(), n, '\n', want.data(), (int64_t)want.size());
        if (len < 0) { printf("epgio_format_f5 failed\n"); return 1; }
        const char* p = want.data();
        for (int i = 0; i < n; ++i) {
            const char* nl = (const char*)memchr(p, '\n', (size_t)(want.data() + len - p));
            const uint32_t u = as_bits(vals[i]);
            uint64_t q;
            epgfmt::f5_scale(u, &q);
            memset(got.data(), 0, got.size());
            const int L = epgfmt::f5_emit(u, q, [&](int at, char c) { got.at((size_t)at) = c; });
            if (L != epgfmt::f5_len(u, q) || L > epgfmt::F5_MAX_LEN || L != (int)(nl - p) || memcmp(got.data(), p, (size_t)L) != 0) {
                if (differ < 10) printf("%08x: host %.*s device %.*s\n", u, (int)(nl - p), p, L, got.data());
                ++differ;
            }
            p = nl + 1;
        }
        done += n;
    }
    printf("fmt_f5_check: %lld patterns, %lld refused, %lld differ\n", done, refused, differ);
    return differ ? 1 : 0;
}
