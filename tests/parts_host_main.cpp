// Host check of epg_parts.h: pack_parts and PartCursor together, against expectations written from the definition (a direct
// loop over parts and rows).  Built and run by tests/test_parts_host.py; exit status 0 = every case held.
#include "epg_parts.h"

#include <stdio.h>
#include <vector>

struct TestParts {                         // the form of NhParts with 4 slots, so that more parts than a launch holds is cheap
    int id[4];                             // stands for the pointers: the part that slot k was filled from
    long rows[4];
    long t0[5];
    int n;
};

static long g_checks = 0, g_failed = 0;
#define CHECK(cond, ...)                                                       \
    do {                                                                       \
        ++g_checks;                                                            \
        if (!(cond)) {                                                         \
            if (++g_failed <= 20) { printf("FAILED %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } \
        }                                                                      \
    } while (0)

// R = rows of every part, T = rows per tile; every_other: the rows-callable leaves the odd parts out
static void run_case(const std::vector<long>& R, int T, bool every_other) {
    const int nparts = (int)R.size();
    auto contributes = [&](int p) { return every_other && (p & 1) ? 0L : R[p]; };
    static const int strides[3] = {1, 4, 7};
    // visits[s][p][r]: how often the waves of stride s, all launches together, were handed row r of part p
    std::vector<std::vector<std::vector<int>>> visits(3, std::vector<std::vector<int>>(nparts));
    for (int s = 0; s < 3; ++s)
        for (int p = 0; p < nparts; ++p) visits[s][p].assign((size_t)R[p], 0);
    int launches = 0;
    for (int p0 = 0; p0 < nparts;) {       // the callers' loop
        // from the definition: this launch takes the first four parts at or after p0 that contribute rows
        std::vector<int> taken;
        long tiles = 0;
        for (int p = p0; p < nparts; ++p)
            if (contributes(p) && taken.size() < 4) {
                taken.push_back(p);
                tiles += contributes(p) / T + (contributes(p) % T ? 1 : 0);
            }
        const int next = taken.size() == 4 ? taken.back() + 1 : nparts;
        TestParts pt;
        int fills = 0;
        const int got = epg::pack_parts(pt, p0, nparts, T, contributes, [&](int k, int p) {
            CHECK(k == fills, "fill slot %d, expected %d", k, fills);
            ++fills;
            pt.id[k] = p;
        });
        CHECK(got == next, "p0=%d: returned %d, expected %d", p0, got, next);
        CHECK(pt.n == (int)taken.size() && fills == pt.n, "p0=%d: n=%d fills=%d, expected %zu", p0, pt.n, fills, taken.size());
        if (pt.n != (int)taken.size()) return;
        if (pt.n == 0) {                   // the remaining parts are all empty: the callers stop here
            CHECK(got == nparts && pt.t0[0] == 0, "empty launch: returned %d of %d, t0[0]=%ld", got, nparts, pt.t0[0]);
            break;
        }
        CHECK(++launches <= nparts, "no progress");
        CHECK(pt.t0[0] == 0 && pt.t0[pt.n] == tiles, "t0[0]=%ld t0[n]=%ld, expected 0 and %ld", pt.t0[0], pt.t0[pt.n], tiles);
        for (int k = 0; k < pt.n; ++k)
            CHECK(pt.id[k] == taken[k] && pt.rows[k] == contributes(taken[k]), "slot %d: part %d rows %ld", k, pt.id[k], pt.rows[k]);
        for (int s = 0; s < 3; ++s) {
            long visited = 0;
            for (int off = 0; off < strides[s]; ++off) {              // one wave
                epg::PartCursor at;
                int last_part = 0;
                for (long tile = off; tile < pt.t0[pt.n]; tile += strides[s]) {
                    const long r0 = at.advance(pt.t0, tile, T);
                    ++visited;
                    CHECK(at.part >= last_part && at.part < pt.n, "tile %ld: part %d after %d of %d", tile, at.part, last_part, pt.n);
                    if (at.part < 0 || at.part >= pt.n) return;
                    last_part = at.part;
                    const long rows = pt.rows[at.part];
                    CHECK(r0 >= 0 && r0 < rows && r0 % T == 0, "tile %ld: first row %ld of %ld in part %d", tile, r0, rows, at.part);
                    if (r0 < 0 || r0 >= rows) return;
                    // the tile's rows, all in this one part
                    for (long r = r0; r < r0 + T && r < rows; ++r) ++visits[s][pt.id[at.part]][(size_t)r];
                }
            }
            CHECK(visited == pt.t0[pt.n], "stride %d: %ld tiles visited, t0[n]=%ld", strides[s], visited, pt.t0[pt.n]);
        }
        p0 = got;
    }
    for (int s = 0; s < 3; ++s)
        for (int p = 0; p < nparts; ++p)
            for (long r = 0; r < R[p]; ++r) {
                const int want = contributes(p) ? 1 : 0;
                CHECK(visits[s][p][(size_t)r] == want, "T=%d stride %d: row %ld of part %d visited %d times, expected %d", T, strides[s], r, p,
                      visits[s][p][(size_t)r], want);
            }
}

int main() {
    static const int tile_sizes[3] = {8, 32, 64};
    long cases = 0;
    for (int T : tile_sizes) {
        const long choice[6] = {0, 1, T - 1, T, T + 1, 3 * T + 5};
        for (int nparts = 0; nparts <= 11; ++nparts) {
            std::vector<std::vector<long>> sets;
            for (int shift = 0; shift < 6; ++shift) {                 // the six counts in turn, from every starting point
                std::vector<long> R(nparts);
                for (int p = 0; p < nparts; ++p) R[p] = choice[(p + shift) % 6];
                sets.push_back(R);
                if (nparts) { R[0] = 0; R[nparts - 1] = 0; R[nparts / 2] = 0; }   // empty parts first, last and in the middle
                sets.push_back(R);
            }
            sets.push_back(std::vector<long>(nparts, 0));            // nothing but empty parts
            sets.push_back(std::vector<long>(nparts, 3 * T + 5));
            unsigned lcg = 12345u + 97u * nparts + T;
            for (int draw = 0; draw < 8; ++draw) {
                std::vector<long> R(nparts);
                for (int p = 0; p < nparts; ++p) { lcg = lcg * 1664525u + 1013904223u; R[p] = choice[(lcg >> 16) % 6]; }
                sets.push_back(R);
            }
            for (const auto& R : sets)
                for (int every_other = 0; every_other < 2; ++every_other) { run_case(R, T, every_other != 0); ++cases; }
        }
    }
    printf("%ld cases, %ld checks, %ld failed\n", cases, g_checks, g_failed);
    return g_failed ? 1 : 0;
}
