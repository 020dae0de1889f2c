// The workgroup scan the text kernels share (epg_scores_text.hip, epg_statebyline.hip): both count delimiters per 16 bytes of a
// thread and need each thread's offset among the workgroup's.  And the one-workgroup scan of the tiles' sums that the two text
// writers share (epg_textout.hip, epg_metrics_text.hip).
#pragma once
#include "epg_common.h"

namespace epg {

// exclusive scan of v over the workgroup (`NW` waves); *total = the sum.  `part` is LDS, NW words.
template <int NW>
__device__ __forceinline__ u32 st_block_scan(u32 v, u32* part, u32* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u32 inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const u32 up = __shfl_up(inc, o);
        if (lane >= o) inc += up;
    }
    if (lane == 63) part[wave] = inc;
    __syncthreads();
    u32 before = 0, sum = 0;
    for (int w = 0; w < NW; ++w) {
        const u32 p = part[w];
        if (w < wave) before += p;
        sum += p;
    }
    __syncthreads();                                             // part may be written again by the caller's next turn
    *total = sum;
    return before + inc - v;
}

// one workgroup of T threads: the tiles' sums become, in place, the text offsets of the tiles' first rows; row_off[R] = the size of the
// text.  A template so that only the sources that launch it carry it.
template <int T>
__global__ __launch_bounds__(T) void k_text_tile_offsets(u64* __restrict__ tile_sum, long ntiles, long R, long long* __restrict__ row_off) {
    __shared__ u64 s_sum[T];
    const int tid = threadIdx.x;
    const long chunk = (ntiles + T - 1) / T;
    const long lo = tid * chunk < ntiles ? tid * chunk : ntiles, hi = lo + chunk < ntiles ? lo + chunk : ntiles;
    u64 sum = 0;
    for (long b = lo; b < hi; ++b) sum += tile_sum[b];
    s_sum[tid] = sum;
    __syncthreads();
    u64 run = 0;
    for (int k = 0; k < tid; ++k) run += s_sum[k];
    for (long b = lo; b < hi; ++b) {
        const u64 own = tile_sum[b];
        tile_sum[b] = run;
        run += own;
    }
    if (tid == T - 1) row_off[R] = (long long)run;
}

}  // namespace epg
