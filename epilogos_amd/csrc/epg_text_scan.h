// The index / scan toolkit of the text kernels, each piece once:
//   st_block_scan      the workgroup scan: a thread's offset among the workgroup's (delimiter counts, row lengths, bit counts);
//   st_scan_segments   one workgroup: segment counts -> exclusive offsets with a carry, the total returned (k_st_scan, k_sbl_scan,
//                      k_seg_scan: each keeps its own tail behind it);
//   st_byte_mask, st_text_index   the two-pass delimiter index, templated on the byte predicate (k_st_index: tab or newline,
//                      k_seg_index: newline).  sbl_window (epg_statebyline.hip) keeps its own 20-byte window: it needs the four bytes
//                      before the thread's 16 and would pay for going through the shared mask;
//   st_scan_chunks     one workgroup: the chunked exclusive scan of a 64-bit field (k_text_tile_offsets here, k_bgzf_offsets in
//                      epg_textout.hip: each keeps its own tail);
//   st_store_span      an LDS area that is shifted to its destination's alignment, stored in aligned 16-byte chunks with ragged ends
//                      (the row writer's window in epg_text_rows.h, k_bgzf_emit, k_bgzf_inflate).
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

// one workgroup of NW waves: seg[0 .. nseg) counts -> exclusive offsets, in place; -> their sum.  `part` is LDS, NW words.
template <int NW>
__device__ __forceinline__ u32 st_scan_segments(u32* __restrict__ seg, int nseg, u32* part) {
    u32 carry = 0;
    for (int i0 = 0; i0 < nseg; i0 += NW * 64) {
        const int i = i0 + (int)threadIdx.x;
        const u32 v = i < nseg ? seg[i] : 0;
        u32 total;
        const u32 off = st_block_scan<NW>(v, part, &total);
        if (i < nseg) seg[i] = carry + off;
        carry += total;
    }
    return carry;
}

struct StIsNewline {
    __device__ __forceinline__ bool operator()(u32 c) const { return c == '\n'; }
};
struct StIsTabOrNewline {
    __device__ __forceinline__ bool operator()(u32 c) const { return c == '\t' || c == '\n'; }
};

// bit j = the byte at position p0 + j is one of `is`, for the 16 positions from p0 (positions beyond n are none)
template <class Is>
__device__ __forceinline__ u32 st_byte_mask(const char* __restrict__ text, long n, long p0, Is is) {
    u32 m = 0;
    if (p0 + 16 <= n) {
        const uint4 v = ld16(text + p0);
        const u32 w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if (is((w[j >> 2] >> (8 * (j & 3))) & 0xffu)) m |= 1u << j;
    } else {
        for (int j = 0; j < 16; ++j) {
            const long p = p0 + j;
            if (p < n) {
                if (is((unsigned char)text[p])) m |= 1u << j;
            } else if (p == n && n > 0 && text[n - 1] != '\n') {
                m |= 1u << j;                                    // the virtual newline of a text that ends inside its last row
            }
        }
    }
    return m;
}

// The body of an index kernel of NW waves, 16 bytes of text per thread.  FILL false: seg[workgroup] = the number of bytes of `is` in
// the workgroup's text.  FILL true (seg scanned in between): pos[i] = the position of the i-th such byte, for i < cap
// (0xffffffff: no cap).  `part` is LDS, NW words.
template <bool FILL, int NW, class Is>
__device__ __forceinline__ void st_text_index(const char* __restrict__ text, long n, u32* __restrict__ seg, u32* __restrict__ pos, u32 cap,
                                              u32* part, Is is) {
    const long p0 = ((long)blockIdx.x * (NW * 64) + (long)threadIdx.x) * 16;
    u32 m = p0 <= n ? st_byte_mask(text, n, p0, is) : 0;
    u32 total;
    const u32 off = st_block_scan<NW>(__popc(m), part, &total);
    if (!FILL) {
        if (threadIdx.x == 0) seg[blockIdx.x] = total;
    } else {
        u32 at = seg[blockIdx.x] + off;
        while (m && at < cap) {
            pos[at++] = (u32)(p0 + __ffs(m) - 1);
            m &= m - 1;
        }
    }
}

// One workgroup of T threads: the exclusive scan of n 64-bit values, a chunk of consecutive values per thread.  get(i) reads value i,
// put(i, x) takes its offset (they may be the same field).  -> in thread T - 1, the sum of all.  `s_sum` is LDS, T words.
template <int T, class Get, class Put>
__device__ __forceinline__ u64 st_scan_chunks(long n, u64* s_sum, Get get, Put put) {
    const int tid = threadIdx.x;
    const long chunk = (n + T - 1) / T;
    const long lo = tid * chunk < n ? tid * chunk : n, hi = lo + chunk < n ? lo + chunk : n;
    u64 sum = 0;
    for (long b = lo; b < hi; ++b) sum += get(b);
    s_sum[tid] = sum;
    __syncthreads();
    u64 run = 0;
    for (int k = 0; k < tid; ++k) run += s_sum[k];
    for (long b = lo; b < hi; ++b) {
        const u64 own = get(b);
        put(b, run);
        run += own;
    }
    return run;
}

// one workgroup of T threads: the tiles' sums become, in place, the text offsets of the tiles' first rows; row_off[R] = the size of the
// text.  A template so that only the sources that launch it carry it.
template <int T>
__global__ __launch_bounds__(T) void k_text_tile_offsets(u64* __restrict__ tile_sum, long ntiles, long R, long long* __restrict__ row_off) {
    __shared__ u64 s_sum[T];
    const u64 run = st_scan_chunks<T>(ntiles, s_sum, [&](long b) { return tile_sum[b]; }, [&](long b, u64 x) { tile_sum[b] = x; });
    if (threadIdx.x == T - 1) row_off[R] = (long long)run;
}

// Bytes [a, a + size) of the LDS area `chunks`, a < 16, go to base + a ...: the area is shifted so that its 16-byte chunks are
// 16-byte chunks of the destination (base is 16-byte aligned).  Whole chunks are stored as uint4, the chunks at the two ragged ends
// byte by byte; thread t of T takes every T-th chunk.  `zeros`: store zeros instead of the area's bytes.
__device__ __forceinline__ void st_store_span(const uint4* chunks, unsigned char* __restrict__ base, u32 a, u32 size, int t, int T,
                                              bool zeros = false) {
    const unsigned char* bytes = reinterpret_cast<const unsigned char*>(chunks);
    const int nchunks = (int)((a + size + 15u) >> 4);
    for (int c = t; c < nchunks; c += T) {
        const u32 lo = 16u * c;
        if (lo >= a && lo + 16u <= a + size) {
            *reinterpret_cast<uint4*>(base + lo) = zeros ? make_uint4(0, 0, 0, 0) : chunks[c];
        } else {
            for (u32 j = 0; j < 16; ++j)
                if (lo + j >= a && lo + j < a + size) base[lo + j] = zeros ? (unsigned char)0 : bytes[lo + j];
        }
    }
}

}  // namespace epg
