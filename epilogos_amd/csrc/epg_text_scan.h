// The workgroup scan the text kernels share (epg_scores_text.hip, epg_statebyline.hip): both count delimiters per 16 bytes of a
// thread and need each thread's offset among the workgroup's.
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

}  // namespace epg
