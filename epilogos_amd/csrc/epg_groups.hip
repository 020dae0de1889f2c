// Column groups: per-bin histograms of up to four column subsets of ONE matrix in one pass (include/epilogos_groups.h).
// gfx950 only.  The counting core, the tile loop and the store of whole lines are k_bin_hist's (epg_count.h: count_group's decode,
// for_each_group, tile_loop, quad_state_count):
// a row is loaded once, transposed once and decoded once per state; a group costs one AND with the lane's membership word and one
// v_bcnt per state on top (2 VALU per state, group and 32 bytes).
#include "epg_count.h"
#include "epilogos_groups.h"

namespace epg {

constexpr int GR_MAX = EPG_GROUPS_MAX;

struct GroupOut {
    u16* h[GR_MAX];
};

// The membership words of one 32-byte group of a lane: mb[8] = the lane's 32 membership bytes in the order of the data dwords.
// Bit g of every byte goes through the SAME transpose as the states; plane 0 of the result holds sample (dword, byte) at the bit
// where every plane of the states holds it, so ind & M[g] selects the group's samples whatever that order is.
template <int G>
__device__ __forceinline__ void member_words(const u32 (&mb)[8], u32 (&M)[GR_MAX]) {
#pragma unroll
    for (int gg = 0; gg < GR_MAX; ++gg) {
        M[gg] = 0;
        if (gg < G) {
            u32 v[8], P[5];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = (mb[k] >> gg) & 0x01010101u;
            bit_planes(v, P);
            M[gg] = P[0];
        }
    }
}

// one group of 32 state bytes: cnt[g * S + s] += #bytes equal to s among the samples of M[g]
template <int S, int G>
__device__ __forceinline__ void count_group_members(const u32 (&w)[8], const uint4 m, u32 (&cnt)[G * S]) {
    const u32 M[GR_MAX] = {m.x, m.y, m.z, m.w};
    u32 P[5], L[8];
    bit_planes(w, P);
    low_three(P, L);
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const u32 ind = indicator(L, P, s);
#pragma unroll
        for (int gg = 0; gg < G; ++gg) cnt[gg * S + s] += (u32)__builtin_popcount(ind & M[gg]);
    }
}

// The row counter tile_loop calls: the any-width load schedule (for_each_group, epg_count.h: four 32-byte groups in flight), the
// membership words of group t and quad lane j read from the block's LDS table as one ds_read_b128.
template <int S, int G>
struct CountRowGroups {
    const uint4* mtab;               // [ngroups][4 quad lanes]
    __device__ __forceinline__ void operator()(const char* rowp, int j, const RowGeom& g, u32 (&cnt)[G * S]) const {
        for_each_group(rowp, j, g, cnt, [m = mtab, j](int t, const u32 (&w)[8], u32 (&c)[G * S]) { count_group_members<S, G>(w, m[t * 4 + j], c); });
    }
};

// S = the counting core (15, 18, 25, 31), Sout <= S the model's size = columns of every H_g.  LDS: the membership table
// (dynamic, 64 bytes per 128 columns: 32 KB at N = 65535), a staging area of 32 rows per wave and group, the block's counts.
// Two blocks per CU like k_bin_hist, so 256 VGPRs: G x S counters (124 at most) + 32 dwords of loads in flight + the decode.
template <int S, int G>
__global__ __launch_bounds__(256, 2) void k_bin_hist_groups(const char* __restrict__ X, long R, int N, long ldx, int Sout,
                                                             const unsigned char* __restrict__ member, const GroupOut out,
                                                             u64* __restrict__ counts) {
    constexpr int NACC = (G * S + 63) / 64;
    extern __shared__ uint4 s_member[];
    __shared__ u64 s_cnt[G * S];
    __shared__ __attribute__((aligned(16))) char s_stage[4][G][32 * 2 * S];
    const int ROWB = 2 * Sout;                         // bytes of one row of H
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 3, b = lane >> 2;

    // the membership words, once per block: entry (t, jj) = group t of quad lane jj, bytes at or past N read as 0
    {
        const RowGeom g = make_geom(N);
        const int ngroups = (g.chunks + 7) >> 3;
        for (int e = threadIdx.x; e < ngroups * 4; e += 256) {
            const int t = e >> 2, jj = e & 3;
            u32 mb[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int at = 16 * (4 * (2 * t + (k >> 2)) + jj) + 4 * (k & 3);      // chunk 4 * slot + jj, dword k & 3
                u32 v = 0;
#pragma unroll
                for (int by = 0; by < 4; ++by) v |= (at + by < N ? (u32)member[at + by] : 0u) << (8 * by);
                mb[k] = v;
            }
            u32 M[GR_MAX];
            member_words<G>(mb, M);
            s_member[e] = make_uint4(M[0], M[1], M[2], M[3]);
        }
        if (threadIdx.x < G * S) s_cnt[threadIdx.x] = 0;
    }
    __syncthreads();

    u64 acc[NACC];                                     // column sums of the staged rows: lane e owns (g, s) = e, e + 64
#pragma unroll
    for (int i = 0; i < NACC; ++i) acc[i] = 0;

    // `valid` is not looked at: a lane past the last row counted row R - 1 again and stages it like any other; finish() stores and
    // sums only the `rows` real rows of the super-tile.  finish() reads what other lanes of the wave staged: LDS operations of a
    // wave complete in order (the convention of k_bin_hist's store_staged).
    auto epilogue = [&](int half, long row, bool valid, u32 (&cnt)[G * S]) {
#pragma unroll
        for (int gg = 0; gg < G; ++gg) {
            // pack_reduce of the group's counters, four states at a time: lane j of the quad stages state 4k + j
            char* srow = &s_stage[wave][gg][(half * 16 + b) * ROWB];
#pragma unroll
            for (int k = 0; k < (S + 3) / 4; ++k) {
                const u32 c0 = cnt[gg * S + 4 * k], c1 = 4 * k + 1 < S ? cnt[gg * S + 4 * k + 1] : 0u;
                const u32 c2 = 4 * k + 2 < S ? cnt[gg * S + 4 * k + 2] : 0u, c3 = 4 * k + 3 < S ? cnt[gg * S + 4 * k + 3] : 0u;
                const u32 d[2] = {quad_sum(c0 | (c1 << 16)), quad_sum(c2 | (c3 << 16))};
                const u32 c = quad_state_count(d, 0, j);
                if (4 * k + j < Sout) *reinterpret_cast<u16*>(srow + 2 * (4 * k + j)) = (u16)c;
            }
        }
    };
    auto finish = [&](long st, long row0, int rows) {
#pragma unroll
        for (int gg = 0; gg < G; ++gg)
            if (out.h[gg]) store_staged(s_stage[wave][gg], reinterpret_cast<char*>(out.h[gg]) + row0 * ROWB, rows * ROWB, lane);
        if (counts) {
#pragma unroll
            for (int i = 0; i < NACC; ++i) {
                const int e = lane + 64 * i;
                if (e < G * Sout) {
                    const u16* col = reinterpret_cast<const u16*>(s_stage[wave][e / Sout]) + e % Sout;
                    u32 sum = 0;                       // (32 rows x 65535 fits)
                    for (int r = 0; r < rows; ++r) sum += col[r * Sout];
                    acc[i] += sum;
                }
            }
        }
    };
    tile_loop<G * S, 0>(X, R, N, ldx, epilogue, finish, CountRowGroups<S, G>{s_member});

    if (counts) {
#pragma unroll
        for (int i = 0; i < NACC; ++i) {
            const int e = lane + 64 * i;
            if (e < G * Sout && acc[i]) atomicAdd(&s_cnt[e], acc[i]);
        }
        __syncthreads();
        if ((int)threadIdx.x < G * Sout && s_cnt[threadIdx.x]) atomicAdd(&counts[threadIdx.x], s_cnt[threadIdx.x]);
    }
}

// Any shape, never reads past a row's N bytes: one wave per bin, LDS atomics.  For the matrix's last row(s) when the pitch is
// shorter than the fast kernel's last 16-byte chunk (k_bin_hist_safe's job in epg_bin_hist); the same five-bit decode.
__global__ __launch_bounds__(256) void k_bin_hist_groups_safe(const char* __restrict__ X, long row_begin, long row_end, int N, long ldx,
                                                               int S, int G, const unsigned char* __restrict__ member, const GroupOut out,
                                                               u64* __restrict__ counts) {
    __shared__ u32 s_h[4][GR_MAX * 32];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long row = row_begin + (long)blockIdx.x * 4 + wave; row < row_end; row += (long)gridDim.x * 4) {
        for (int e = lane; e < GR_MAX * 32; e += 64) s_h[wave][e] = 0;
        __builtin_amdgcn_wave_barrier();
        const char* rp = X + row * ldx;
        for (int n = lane; n < N; n += 64) {
            const int v = (unsigned char)rp[n] & 31;
            const u32 m = member[n];
            if (v < S)
                for (int gg = 0; gg < G; ++gg)
                    if ((m >> gg) & 1u) atomicAdd(&s_h[wave][gg * 32 + v], 1u);
        }
        __builtin_amdgcn_wave_barrier();
        for (int e = lane; e < G * S; e += 64) {
            const int gg = e / S, s = e % S;
            const u32 c = s_h[wave][gg * 32 + s];
            if (out.h[gg]) out.h[gg][row * S + s] = (u16)c;
            if (counts && c) atomicAdd(&counts[e], (u64)c);
        }
        __builtin_amdgcn_wave_barrier();
    }
}

extern "C" int epg_bin_hist_groups(const int8_t* X8, int64_t R, int32_t N, int64_t ldx, int32_t S, int32_t G, const uint8_t* member,
                                   uint16_t* const* H, int64_t* counts, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (R < 0 || N < 1 || ldx < N || S < 1 || G < 1)
        return fail(EPG_ERR_INVALID_ARG, "bin_hist_groups: bad shape R=%lld N=%d ldx=%lld S=%d G=%d", (long long)R, N, (long long)ldx, S, G);
    if (S > 31) return fail(EPG_ERR_UNSUPPORTED, "bin_hist_groups: S=%d > 31 (gather the columns for a wider model)", S);
    if (G > GR_MAX) return fail(EPG_ERR_UNSUPPORTED, "bin_hist_groups: G=%d > %d groups per call", G, GR_MAX);
    if (N > 65535) return fail(EPG_ERR_UNSUPPORTED, "bin_hist_groups: N=%d > 65535 (uint16 per-bin counts)", N);
    if (!X8 || !member) return fail(EPG_ERR_INVALID_ARG, "bin_hist_groups: X or member is NULL");
    GroupOut out = {};
    bool any = counts != nullptr;
    for (int g = 0; g < G; ++g) {
        out.h[g] = H ? H[g] : nullptr;
        if (reinterpret_cast<uintptr_t>(out.h[g]) & 15) return fail(EPG_ERR_INVALID_ARG, "bin_hist_groups: H[%d] must be 16-byte aligned", g);
        any = any || out.h[g];
    }
    if (!any) return fail(EPG_ERR_INVALID_ARG, "bin_hist_groups: H and counts are both NULL");
    if (R == 0) return EPG_OK;
    const char* X = reinterpret_cast<const char*>(X8);
    u64* cnt = reinterpret_cast<u64*>(counts);
    const long Rf = fast_rows(R, N, ldx);
    if (Rf > 0) {
        const size_t lds = (size_t)((N + 127) / 128) * 4 * sizeof(uint4);
        with_constant<31, 15, 18, 25>(S <= 15 ? 15 : S <= 18 ? 18 : S <= 25 ? 25 : 31, [&](auto SC) {
            with_constant<4, 1, 2, 3>(G, [&](auto GC) {
                hipLaunchKernelGGL((k_bin_hist_groups<decltype(SC)::value, decltype(GC)::value>), dim3(grid_for_tiles(Rf)), dim3(256), lds, st, X,
                                   Rf, N, ldx, S, member, out, cnt);
            });
        });
        EPG_LAUNCH_CHECK("k_bin_hist_groups");
    }
    if (Rf < R) {
        hipLaunchKernelGGL(k_bin_hist_groups_safe, dim3((unsigned)((R - Rf + 3) / 4 < 1024 ? (R - Rf + 3) / 4 : 1024)), dim3(256), 0, st, X, Rf,
                           (long)R, N, ldx, S, G, member, out, cnt);
        EPG_LAUNCH_CHECK("k_bin_hist_groups_safe");
    }
    return EPG_OK;
}

}  // namespace epg
