// State census: per-COLUMN state counts of a state matrix, the bytes that are no state, and the first of them
// (include/epilogos_census.h).  gfx950 only.
//
// Every other count kernel here reduces per bin; this one reduces per biosample column, so the counters are S + 1 per column
// (the states and "other") and live in LDS.  Work split:
//   * a lane loads CB = 16 bytes of a row (16 columns) where X and ldx are multiples of 16, CB = 1 byte otherwise;
//   * a wave covers a "strip" of nl = 2^k chunks of CB columns and 64 / nl rows per load (nl = 64: one row of 1024 columns);
//   * a block of 16 waves walks "items" = (strip, tile of 512 rows); a block gets one contiguous range of items, strip-major, and
//     walks it in runs of consecutive tiles of one strip -- one loop per run, a wave's next 4 loads in flight while it counts 4;
//   * the block's table is tab[state 0 .. S][k & 7][slot], slot = lane & (TW - 1): for a given byte k of the load every lane of
//     a 32-lane half adds into a bank of its own whatever the states are, so the ds_add_u32 of a wave never conflict at TW = 64
//     (S <= 31); wider models fold the slots (TW = 32, 16) to stay inside 64 KB.  TW is a template parameter: the address of a
//     byte's counter is (min(byte, S) << shift) + the lane's base, the rest is the instruction's immediate offset -- two VALU
//     operations and one ds_add_u32 per byte;
//   * all 16 bytes of a loaded chunk are counted, the row padding behind column N too: the table has their columns and the
//     flush leaves them out.  Whether a chunk holds a byte >= S is one SWAR test per dword; only then are its bytes looked at
//     one by one (and the padding told apart) for first_bad;
//   * with CB = 16 a dword packs TWO 16-bit counters, bytes k and k + 8 of the lane.  A counter gets at most one add per row of
//     a run, so a run is at most 127 tiles (65 024 rows) and the table is flushed between runs;
//   * the flush adds every non-zero counter to census / other with 64-bit global atomics, each block starting at another place of
//     the table; first_bad is a per-lane minimum, reduced over the wave, then one 64-bit atomic minimum per wave that saw one.
// All sums are integers: the result is exact whatever the grid.
#include "epg_common.h"
#include "epilogos_census.h"

namespace epg {

constexpr int CE_THREADS = 1024;          // 16 waves share one table: 8 waves took 0.66 ms where 16 take 0.47 (tools/census_bench.py)
constexpr int CE_WAVES = CE_THREADS / 64;
constexpr int CE_TILE = 512;             // rows of an item
constexpr int CE_UNROLL = 4;             // loads of a batch: one batch is counted while the next is in flight (8: spills at 128 VGPRs)
constexpr long CE_RUN_TILES = 65535 / CE_TILE;     // tiles between two flushes: their rows are what a 16-bit counter holds
constexpr long long CE_NONE = 0x7fffffffffffffffLL;

struct CensusGeom {
    int nl_log2;      // chunks of a strip
    int tw_log2;      // slots of the table
    long nstrips, ntiles;
};

// the table slots that (S + 1) x KH dwords per slot leave room for in 64 KB: 64 up to S = 31, then 32, 16
static inline int census_tw_log2(int S, int KH) {
    int tw = 6;
    while (tw > 0 && (long)(S + 1) * KH * (4L << tw) > 65536) --tw;
    return tw;
}

template <int CB>
static inline CensusGeom census_geom(long R, int N, int S) {
    constexpr int KH = CB == 16 ? 8 : 1;
    CensusGeom g;
    const int chunks = (N + CB - 1) / CB;
    g.tw_log2 = census_tw_log2(S, KH);
    g.nl_log2 = 0;
    while (g.nl_log2 < g.tw_log2 && (1 << g.nl_log2) < chunks) ++g.nl_log2;
    g.nstrips = (chunks + (1 << g.nl_log2) - 1) >> g.nl_log2;
    g.ntiles = (R + CE_TILE - 1) / CE_TILE;
    return g;
}

template <int CB, int TWL>
__global__ __launch_bounds__(CE_THREADS) void k_state_census(const char* __restrict__ X, long R, int N, long ldx, int S, const CensusGeom geo,
                                                              u64* __restrict__ census, u64* __restrict__ other, long long* first_bad) {
    constexpr int KH = CB == 16 ? 8 : 1;          // dwords of a slot per state
    constexpr int NW = CB == 16 ? 4 : 1;          // dwords of a load
    constexpr int TW = 1 << TWL;
    extern __shared__ u32 s_tab[];                // [S + 1][KH][TW]
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nl_log2 = geo.nl_log2;
    const int rpw_log2 = 6 - nl_log2;             // rows of a wave's load
    const int cl = lane & ((1 << nl_log2) - 1), rr = lane >> nl_log2;
    u32* const lane_tab = s_tab + (lane & (TW - 1));
    const int total = (S + 1) * KH * TW;
    const int strip_cols = CB << nl_log2;
    // byte >= S in any of a dword's four bytes (S <= 127): bit 7 set, or the low seven bits + (128 - S) carry into bit 7
    const u32 swar_add = (u32)(128 - S) * 0x01010101u;

    for (int e = threadIdx.x; e < total; e += CE_THREADS) s_tab[e] = 0;
    __syncthreads();

    // add what the table holds of strip `strip` to the outputs and zero it (the caller puts the barriers around it); the
    // columns at and behind N (row padding that was counted with its chunk) are dropped here
    auto flush = [&](long strip) {
        const int rot = (int)(((long)blockIdx.x * 2357) % total);
        for (int i = threadIdx.x; i < total; i += CE_THREADS) {
            int e = i + rot;
            if (e >= total) e -= total;
            const u32 w = s_tab[e];
            if (w == 0) continue;
            s_tab[e] = 0;
            const int sl = e & (TW - 1);
            const int kk = (e >> TWL) % KH, s = (e >> TWL) / KH;
            const int col = (int)(strip * strip_cols) + (sl & ((1 << nl_log2) - 1)) * CB + kk;
            const u32 lo = CB == 16 ? w & 0xffffu : w, hi = CB == 16 ? w >> 16 : 0u;
            if (s < S) {
                if (lo && col < N) atomicAdd(&census[(long)col * S + s], (u64)lo);
                if (hi && col + 8 < N) atomicAdd(&census[(long)(col + 8) * S + s], (u64)hi);
            } else if (other) {
                if (lo && col < N) atomicAdd(&other[col], (u64)lo);
                if (hi && col + 8 < N) atomicAdd(&other[col + 8], (u64)hi);
            }
        }
    };

    const long items = geo.nstrips * geo.ntiles;
    const long item0 = items * blockIdx.x / gridDim.x, item1 = items * (blockIdx.x + 1) / gridDim.x;
    long cur_strip = -1;
    long long fb = CE_NONE;
    // the block's items in "runs": consecutive tiles of one strip, at most CE_RUN_TILES of them (what the 16-bit counters hold);
    // a run is one loop over its rows, the next batch of loads in flight while a batch is counted; the table is flushed between runs
    for (long item = item0; item < item1;) {
        const long strip = item / geo.ntiles, tile = item - strip * geo.ntiles;
        long ntile = geo.ntiles - tile;
        ntile = ntile < item1 - item ? ntile : item1 - item;
        ntile = ntile < CE_RUN_TILES ? ntile : CE_RUN_TILES;
        item += ntile;
        if (cur_strip >= 0) {
            __syncthreads();
            flush(cur_strip);
            __syncthreads();
        }
        cur_strip = strip;
        const long r0 = tile * CE_TILE;
        const long rend = (tile + ntile) * CE_TILE;
        const int rows = (int)((R < rend ? R : rend) - r0);
        const int ngroups = (rows + (1 << rpw_log2) - 1) >> rpw_log2;
        const int col0 = (int)(strip * strip_cols) + cl * CB;
        const int nvalid = N - col0 < CB ? N - col0 : CB;         // columns of the lane's chunk that exist (<= 0: none)
        const char* base = X + r0 * ldx + col0;
        u32 w[CE_UNROLL][NW], wn[CE_UNROLL][NW];
        auto load = [&](int g0, u32 (&dst)[CE_UNROLL][NW]) {
#pragma unroll
            for (int u = 0; u < CE_UNROLL; ++u) {
                const int lr = ((g0 + u * CE_WAVES) << rpw_log2) + rr;      // row of the run
                if (nvalid > 0 && lr < rows) {
                    if constexpr (CB == 16) {
                        const uint4 v = *reinterpret_cast<const uint4*>(base + lr * ldx);
                        dst[u][0] = v.x; dst[u][1] = v.y; dst[u][2] = v.z; dst[u][3] = v.w;
                    } else {
                        dst[u][0] = (unsigned char)base[lr * ldx];
                    }
                }
            }
        };
        load(wave, w);
        for (int g0 = wave; g0 < ngroups; g0 += CE_WAVES * CE_UNROLL) {
            load(g0 + CE_WAVES * CE_UNROLL, wn);                            // (rows behind the run: no lane loads)
#pragma unroll
            for (int u = 0; u < CE_UNROLL; ++u) {
                const int lr = ((g0 + u * CE_WAVES) << rpw_log2) + rr;
                if (nvalid > 0 && lr < rows) {
                    u32 bad = 0;
#pragma unroll
                    for (int d = 0; d < NW; ++d) bad |= w[u][d] | ((w[u][d] & 0x7f7f7f7fu) + swar_add);
                    if (bad & (CB == 16 ? 0x80808080u : 0x80u)) {                  // rare: find the chunk's first such byte that is a column
                        const long long at0 = (r0 + lr) * N + col0;
                        for (int k = 0; k < nvalid; ++k)
                            if ((int)((w[u][k >> 2] >> (8 * (k & 3))) & 0xffu) >= S) {
                                fb = at0 + k < fb ? at0 + k : fb;
                                break;
                            }
                    }
#pragma unroll
                    for (int k = 0; k < CB; ++k) {
                        const u32 b = (w[u][k >> 2] >> (8 * (k & 3))) & 0xffu;
                        const u32 st = b < (u32)S ? b : (u32)S;
                        atomicAdd(&lane_tab[st * (KH * TW) + (k & (KH - 1)) * TW], k < 8 ? 1u : 0x10000u);
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < CE_UNROLL; ++u)
#pragma unroll
                for (int d = 0; d < NW; ++d) w[u][d] = wn[u][d];
        }
    }
    if (cur_strip >= 0) {
        __syncthreads();
        flush(cur_strip);
    }
    if (first_bad) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const long long o = __shfl_xor(fb, d, 64);
            fb = o < fb ? o : fb;
        }
        if (lane == 0 && fb != CE_NONE) atomicMin(first_bad, fb);
    }
}

template <int CB>
static int launch_census(const char* X, long R, int N, long ldx, int S, u64* census, u64* other, long long* first_bad, hipStream_t st) {
    constexpr int KH = CB == 16 ? 8 : 1;
    const CensusGeom geo = census_geom<CB>(R, N, S);
    const long items = geo.nstrips * geo.ntiles;
    const long grid = items < num_cus() ? items : num_cus();
    const size_t lds = (size_t)(S + 1) * KH * (4u << geo.tw_log2);
    if constexpr (CB == 16) {
        with_constant<6, 5, 4>(geo.tw_log2, [&](auto TWL) {
            hipLaunchKernelGGL((k_state_census<16, decltype(TWL)::value>), dim3((unsigned)grid), dim3(CE_THREADS), lds, st, X, R, N, ldx, S, geo,
                               census, other, first_bad);
        });
    } else {                                           // one dword per slot and state: 64 slots fit for every S <= 127
        hipLaunchKernelGGL((k_state_census<1, 6>), dim3((unsigned)grid), dim3(CE_THREADS), lds, st, X, R, N, ldx, S, geo, census, other,
                           first_bad);
    }
    EPG_LAUNCH_CHECK("k_state_census");
    return EPG_OK;
}

extern "C" int epg_state_census(const int8_t* X8, int64_t R, int32_t N, int64_t ldx, int32_t S, int64_t* census, int64_t* other,
                                int64_t* first_bad, void* stream) {
    if (R < 0 || N < 0 || S < 1 || ldx < (N > 1 ? N : 1))
        return fail(EPG_ERR_INVALID_ARG, "state_census: bad shape R=%lld N=%d ldx=%lld S=%d", (long long)R, N, (long long)ldx, S);
    if (S > 127) return fail(EPG_ERR_UNSUPPORTED, "state_census: S=%d > 127", S);
    if (N > 65535) return fail(EPG_ERR_UNSUPPORTED, "state_census: N=%d > 65535", N);
    if (!census) return fail(EPG_ERR_INVALID_ARG, "state_census: census is NULL");
    if (R == 0 || N == 0) return EPG_OK;
    if (!X8) return fail(EPG_ERR_INVALID_ARG, "state_census: X is NULL");
    const char* X = reinterpret_cast<const char*>(X8);
    u64* c = reinterpret_cast<u64*>(census);
    u64* o = reinterpret_cast<u64*>(other);
    long long* fb = reinterpret_cast<long long*>(first_bad);
    hipStream_t st = (hipStream_t)stream;
    if (((reinterpret_cast<uintptr_t>(X) | (uintptr_t)ldx) & 15) == 0) return launch_census<16>(X, R, N, ldx, S, c, o, fb, st);
    return launch_census<1>(X, R, N, ldx, S, c, o, fb, st);
}

}  // namespace epg
