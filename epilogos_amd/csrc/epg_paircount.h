// S2 state-pair counts, C[i,j] += sum_b h_i h_j (i != j), h_i (h_i - 1) (i == j) (expected.py:146-158), from histogram rows that a
// wave has re-packed in LDS as bin PAIRS per state: word (i, k) = the counts of state i in bins 2k and 2k + 1, row stride `ld` words,
// rows past the model's last state zero.  The states go in groups of three; a lane owns one 3 x 3 block of state pairs (groups
// gi <= gj: its "role") and a slice of the pair words, so six LDS words feed nine v_dot2_u32_u16 (the one-pair-per-thread form read
// two words per product).  Used by k_s2_hist_wave (epg_s2.hip: tiles of 64 bins of H) and by bin_hist_body<PAIRS> (epg_s1.hip: the
// 32 rows of a super-tile that the count pass has staged anyway).
#pragma once
#include "epg_common.h"

namespace epg {

typedef unsigned short v2u16 __attribute__((ext_vector_type(2)));

// block role -> its groups (gi <= gj): the upper triangle of the ng x ng blocks, row by row
__device__ __forceinline__ void pair_role(int role, int ng, int& gi, int& gj) {
    int t = role, i = 0;
    while (t >= ng - i) { t -= ng - i; ++i; }
    gi = i; gj = i + t;
}

// part[3 t + u] = sum over the lane's pair words k = k0, k0 + kstep, ... < kend of <pi[t][k], pj[u][k]>, and on a diagonal block
// ps[t] = the sum of pi[t]'s counts (the diagonal's - sum h_i).  Exact in 32 bits while counts are < 4096 (a lane takes at most 32
// pair words per call: 64 x 4095^2 < 2^32).
__device__ __forceinline__ void pair_tile_dot(const u32* pi, const u32* pj, int ld, int k0, int kend, int kstep, bool diag, u32 (&part)[9],
                                              u32 (&ps)[3]) {
#pragma unroll
    for (int c = 0; c < 9; ++c) part[c] = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) ps[c] = 0;
    for (int k = k0; k < kend; k += kstep) {
        const u32 av[3] = {pi[k], pi[ld + k], pi[2 * ld + k]};
        const u32 bv[3] = {pj[k], pj[ld + k], pj[2 * ld + k]};
#pragma unroll
        for (int t = 0; t < 3; ++t)
#pragma unroll
            for (int u = 0; u < 3; ++u)
                part[3 * t + u] = __builtin_amdgcn_udot2(__builtin_bit_cast(v2u16, av[t]), __builtin_bit_cast(v2u16, bv[u]), part[3 * t + u], false);
        if (diag) {
#pragma unroll
            for (int t = 0; t < 3; ++t)
                ps[t] = __builtin_amdgcn_udot2(__builtin_bit_cast(v2u16, av[t]), __builtin_bit_cast(v2u16, 0x00010001u), ps[t], false);
        }
    }
}

// A lane's nine sums into the block's LDS copy of C (zeroed, S x S): C[i,j] = sum h_i h_j in both orders, C[i,i] = sum h_i^2 -
// sum h_i.  The block's lanes meet here and pair_commit sends one global atomic per cell and block: with every lane adding its nine
// sums straight to global memory 7.7 M atomics queued up on 324 addresses and k_s2_hist_wave took 3.9 ms.
__device__ __forceinline__ void pair_fold(const u64 (&acc)[9], const u64 (&rs)[3], int gi, int gj, int S, u64* s_c) {
    const bool diag = gi == gj;
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
        for (int u = 0; u < 3; ++u) {
            const int i = 3 * gi + t, j = 3 * gj + u;
            u64 v = acc[3 * t + u];
            if (diag && t == u) v -= rs[t];                  // two's complement
            if (i >= S || j >= S || !v) continue;
            atomicAdd(&s_c[i * S + j], v);
            if (!diag) atomicAdd(&s_c[j * S + i], v);
        }
}

// after every lane's pair_fold: the block's C into the global counts (a 256-thread block)
__device__ __forceinline__ void pair_commit(const u64* s_c, int S, u64* __restrict__ counts) {
    __syncthreads();
    for (int e = threadIdx.x; e < S * S; e += 256)
        if (s_c[e]) atomicAdd(&counts[e], s_c[e]);
}

}  // namespace epg
