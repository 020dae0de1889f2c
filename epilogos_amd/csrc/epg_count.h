// Per-bin state counting core (gfx950).
//
// Work split: a quad (4 lanes) owns one bin, a wave owns 16 consecutive bins, a 256-thread block 64.  A row of N
// state bytes is cut into 16-byte chunks; chunk c of the row goes to quad lane c & 3, load slot c >> 2, so one
// global_load_dwordx4 per slot covers 64 contiguous bytes of each of the wave's 16 rows.  Two slots (32 bytes per
// lane) make a "group": its 8 dwords are bit-transposed in registers into five 32-bit planes P0..P4 (bit b of
// every state byte), from which the indicator word of each state is three ANDs away and v_bcnt_u32_b32
// accumulates it.  Cost: 38 VALU for the transpose + 16 + 2*S for the decode per 32 bytes (~2.8 VALU/byte at
// S = 18), no LDS, no atomics, no data-dependent control flow (so skewed real data -- 71 % of cells in one
// state -- runs at the same speed as uniform data).
//
// Bytes that are not states (row padding, chunks past the row end, rows past R) are forced to 0xFF, which has
// bits 0..4 set and therefore decodes to state 31: never counted for S <= 31.  Only bits 0..4 of a byte are decoded:
// an input byte b is counted as state b & 31 when that is < S and not at all otherwise.  So -1 (0xFF) and S..31 are
// "not a state" (the count check sum(counts) != R*N reports them), while a byte in 32..254 whose low five bits are < S
// aliases that state -- the contract of the ABI is bytes in 0..31 or 0xFF; the host parser (epg_io.cpp) stores anything
// outside 0..30 as -1 so that files cannot produce an aliasing byte.
#pragma once
#include "epg_common.h"
#include "epg_parts.h"

namespace epg {

// gfx950 VALU issue rates measured with tools/ubench/valu_rate*.hip (SIMD cycles per wave64 instruction):
//   2: v_bitop3_b32, v_and/or/xor/not, v_add/sub_u32, v_lshrrev_b32, v_mov, v_fma_f32
//   4: v_lshlrev_b32, v_bfi_b32, v_bcnt_u32_b32, v_lshl_or/and_or/or3/add3, v_perm, v_bfe, v_cndmask, every DPP/SDWA op
// so the transpose below selects with v_bitop3 (not v_bfi), shifts right where it can, and doubles with v_add.
#define EPG_B3(a, b, c, tt) ((u32)__builtin_amdgcn_bitop3_b32((int)(a), (int)(b), (int)(c), (tt)))

// (m & x) | (~m & y) as one full-rate v_bitop3_b32
__device__ __forceinline__ u32 sel(u32 m, u32 x, u32 y) { return EPG_B3(m, x, y, 0xCA); }

// x << 1 as a full-rate v_add_u32 (LLVM would canonicalise x + x back to the half-rate v_lshlrev_b32)
__device__ __forceinline__ u32 dbl(u32 x) {
    u32 r;
    asm("v_add_u32 %0, %1, %1" : "=v"(r) : "v"(x));
    return r;
}

// the bit transpose of one group: 8 dwords = 32 state bytes -> the five planes P[0..4] (bit b of every byte)
__device__ __forceinline__ void bit_planes(const u32 (&w)[8], u32 (&P)[5]) {
    // stage 1: low nibbles of dword pairs (2i, 2i+1) share a byte
    const u32 n0 = sel(0x0f0f0f0fu, w[0], w[1] << 4);
    const u32 n1 = sel(0x0f0f0f0fu, w[2], w[3] << 4);
    const u32 n2 = sel(0x0f0f0f0fu, w[4], w[5] << 4);
    const u32 n3 = sel(0x0f0f0f0fu, w[6], w[7] << 4);
    // stage 2: bit pairs (b0,b1) and (b2,b3)
    const u32 m0 = sel(0x33333333u, n0, n1 << 2), m1 = sel(0x33333333u, n2, n3 << 2);
    const u32 r0 = sel(0xccccccccu, n1, n0 >> 2), r1 = sel(0xccccccccu, n3, n2 >> 2);
    // stage 3: single bit planes; sample (dword k = 4a+2g+h, byte j) sits at bit 8j + 4h + 2g + a in every plane
    P[0] = sel(0x55555555u, m0, dbl(m1)); P[1] = sel(0xaaaaaaaau, m1, m0 >> 1);
    P[2] = sel(0x55555555u, r0, dbl(r1)); P[3] = sel(0xaaaaaaaau, r1, r0 >> 1);
    // bit 4 plane, same sample order; the selects leave no garbage behind
    const u32 c00 = sel(0x10101010u, w[0], dbl(w[4])), c01 = sel(0x10101010u, w[1], dbl(w[5]));
    const u32 c10 = sel(0x10101010u, w[2], dbl(w[6])), c11 = sel(0x10101010u, w[3], dbl(w[7]));
    const u32 d0 = sel(0x30303030u, c00, c10 << 2), d1 = sel(0x30303030u, c01, c11 << 2);
    P[4] = sel(0xf0f0f0f0u, d1, d0 >> 4);
}

// decode, first half: L[k] = samples whose low three bits equal k (one bitop3 each)
__device__ __forceinline__ void low_three(const u32 (&P)[5], u32 (&L)[8]) {
    L[0] = EPG_B3(P[0], P[1], P[2], 0x01); L[1] = EPG_B3(P[0], P[1], P[2], 0x10); L[2] = EPG_B3(P[0], P[1], P[2], 0x04); L[3] = EPG_B3(P[0], P[1], P[2], 0x40);
    L[4] = EPG_B3(P[0], P[1], P[2], 0x02); L[5] = EPG_B3(P[0], P[1], P[2], 0x20); L[6] = EPG_B3(P[0], P[1], P[2], 0x08); L[7] = EPG_B3(P[0], P[1], P[2], 0x80);
}

// decode, second half: the indicator word of state s (a compile-time value after unrolling), one bitop3 for bits 3,4
__device__ __forceinline__ u32 indicator(const u32 (&L)[8], const u32 (&P)[5], int s) {
    switch (s >> 3) {                                            // (bit3, bit4) of s
        case 0: return EPG_B3(L[s & 7], P[3], P[4], 0x10);       // L & ~P3 & ~P4
        case 1: return EPG_B3(L[s & 7], P[3], P[4], 0x40);       // L &  P3 & ~P4
        case 2: return EPG_B3(L[s & 7], P[3], P[4], 0x20);       // L & ~P3 &  P4
        default: return EPG_B3(L[s & 7], P[3], P[4], 0x80);      // L &  P3 &  P4
    }
}

// one group: 8 dwords = 32 state bytes -> cnt[s] += #bytes equal to s
template <int S>
__device__ __forceinline__ void count_group(const u32 (&w)[8], u32 (&cnt)[S]) {
    u32 P[5], L[8];
    bit_planes(w, P);
    low_three(P, L);
#pragma unroll
    for (int s = 0; s < S; ++s) cnt[s] += (u32)__builtin_popcount(indicator(L, P, s));
}

// Per-launch constants of the row geometry (wave-uniform, live in SGPRs)
struct RowGeom {
    int chunks;     // ceil(N / 16)
    int last;       // chunks - 1
    u32 tail[4];    // OR-mask for the last chunk: 0xFF on bytes >= N - 16*last
};

__device__ __forceinline__ RowGeom make_geom(int N) {
    RowGeom g;
    g.chunks = (N + 15) >> 4;
    g.last = g.chunks - 1;
    const int t = N - 16 * g.last;  // 1..16 valid bytes in the last chunk
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        int v = t - 4 * d;
        v = v < 0 ? 0 : (v > 4 ? 4 : v);
        g.tail[d] = v == 4 ? 0u : (0xffffffffu << (8 * v));
    }
    return g;
}

// load slot i (chunk c = 4i + j) of the lane's row; slots that can touch the row end are clamped and masked
template <bool MAYBE_TAIL>
__device__ __forceinline__ void load_slot(const char* rowp, int i, int j, const RowGeom& g, u32* w) {
    const int c = 4 * i + j;
    if (!MAYBE_TAIL) {
        const uint4 v = ld16(rowp + 16 * c);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    } else {
        const int cc = c < g.last ? c : g.last;
        const uint4 v = ld16(rowp + 16 * cc);
        const u32 inv = c > g.last ? 0xffffffffu : 0u;
        const bool is_last = c == g.last;
        w[0] = v.x | inv | (is_last ? g.tail[0] : 0u);
        w[1] = v.y | inv | (is_last ? g.tail[1] : 0u);
        w[2] = v.z | inv | (is_last ? g.tail[2] : 0u);
        w[3] = v.w | inv | (is_last ? g.tail[3] : 0u);
    }
}

// both load slots of group t (32 bytes per lane) into w[8]
template <bool MAYBE_TAIL>
__device__ __forceinline__ void load_group(const char* rowp, int t, int j, const RowGeom& g, u32 (&w)[8]) {
    load_slot<MAYBE_TAIL>(rowp, 2 * t, j, g, &w[0]);
    load_slot<MAYBE_TAIL>(rowp, 2 * t + 1, j, g, &w[4]);
}

// All 2*NG loads of a row of NG groups (128*(NG-1) < N <= 128*NG); only the last group can touch the row end.
template <int NG>
__device__ __forceinline__ void load_groups(const char* rowp, int j, const RowGeom& g, u32 (&w)[NG][8]) {
#pragma unroll
    for (int t = 0; t < NG; ++t) {
        if (t < NG - 1) load_group<false>(rowp, t, j, g, w[t]);
        else load_group<true>(rowp, t, j, g, w[t]);
    }
}

// A row of any width: group(t, w, cnt) for every group t of the row, in batches of four, the batch's eight loads issued before its
// first group is counted (one group at a time measured 2.81-2.86 ms against 2.40 ms for 7.5 M bins x 1698 on one box).
// (cnt goes through as an argument: a callable that CAPTURES it costs k_bin_hist<18, 0> 3 VGPRs and k_score_s1<18, 0> 14.)
template <int NC, typename Group>
__device__ __forceinline__ void for_each_group(const char* rowp, int j, const RowGeom& g, u32 (&cnt)[NC], Group group) {
    const int ngroups = (g.chunks + 7) >> 3;
    for (int t0 = 0; t0 < ngroups; t0 += 4) {
        u32 w[4][8];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int t = t0 + k;
            if (t < ngroups - 1) load_group<false>(rowp, t, j, g, w[k]);          // wave-uniform
            else if (t == ngroups - 1) load_group<true>(rowp, t, j, g, w[k]);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (t0 + k < ngroups) group(t0 + k, w[k], cnt);
    }
}

// Count one row's states for this lane's share of chunks.  NG > 0: compile-time number of groups, all 2*NG loads are issued up
// front (load_groups).  NG == 0: any N, four groups in flight (for_each_group).
template <int S, int NG>
__device__ __forceinline__ void count_row(const char* rowp, int j, const RowGeom& g, u32 (&cnt)[S]) {
    if constexpr (NG > 0) {
        u32 w[NG][8];
        load_groups<NG>(rowp, j, g, w);
#pragma unroll
        for (int t = 0; t < NG; ++t) count_group<S>(w[t], cnt);
    } else {
        for_each_group(rowp, j, g, cnt, [](int, const u32 (&w)[8], u32 (&c)[S]) { count_group<S>(w, c); });
    }
}

// Tile loop.  A wave owns "super-tiles" of 32 consecutive bins = two 16-bin tiles counted back to back; NG > 0
// issues all 2*NG loads of a tile up front (13.5 KB in flight per wave at N = 833), NG == 0 handles any N four groups
// at a time.  epilogue(half, row, valid, cnt) gets the lane's partial counts of one tile; finish(st, row0, rows) runs
// once per super-tile so the outputs of 32 bins can be written as whole 128-byte lines (32 rows of H are 1152 bytes
// = 9 lines; 36-byte row pieces written straight from the quads cost 0.35 ms of a 2.4 ms launch: partial-line
// writes interleaved with the read stream).
// Round 2 (profiles/r02d, r02e): with the H store the kernel keeps ~20 % fewer read requests in flight than without it
// while no L2->fabric stall counter moves; the guess that a counting wave's vmcnt (loads and stores in one in-order counter)
// puts the store latency on its load path was tested with a dedicated store wave per block (three counting waves hand
// their super-tiles' H rows to the fourth through an LDS ring): same placement-dependent levels, same mean (2.51 against
// 2.41 ms over four alternating bench runs each, 2.48 against 2.44 ms over eight placements) -- removed.
// Measured alternatives that were NOT faster and were removed: (a) refilling group t of the next tile right after
// counting it, with inline-asm loads and hand-counted vmcnt (2.46 vs 2.33 ms); (b) flat line-granular loads staged
// through LDS so that no 128-byte line is requested twice (2.40 ms); (c) nt / sc1 / sc0 sc1 loads (3.1-3.4 ms).
// count(rowp, j, g, cnt) adds one row's share of this lane to cnt[S]: count_row by default; the column-group kernel
// (epg_groups.hip) passes its own, with S = groups x states counters.
template <int S, int NG>
struct CountRow {
    __device__ __forceinline__ void operator()(const char* rowp, int j, const RowGeom& g, u32 (&cnt)[S]) const { count_row<S, NG>(rowp, j, g, cnt); }
};

// one super-tile: local index lst of a matrix X[R, ldx], the lane's row b of each 16-bin half, quad lane j
template <int S, typename Count, typename Epilogue, typename Finish>
__device__ __forceinline__ void super_tile(const char* __restrict__ X, long R, long ldx, const RowGeom& g, long lst, int j, int b, Count&& count,
                                           Epilogue&& epilogue, Finish&& finish) {
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const long row = lst * 32 + half * 16 + b;
        const bool valid = row < R;
        u32 cnt[S];
#pragma unroll
        for (int s = 0; s < S; ++s) cnt[s] = 0;
        count(X + (valid ? row : R - 1) * ldx, j, g, cnt);
        epilogue(half, row, valid, cnt);
    }
    const long row0 = lst * 32;
    finish(lst, row0, (int)(R - row0 < 32 ? R - row0 : 32));
}

template <int S, int NG, int NW = 4, typename Epilogue, typename Finish, typename Count = CountRow<S, NG>>
__device__ __forceinline__ void tile_loop(const char* __restrict__ X, long R, int N, long ldx, Epilogue&& epilogue, Finish&& finish,
                                          Count&& count = Count()) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = lane & 3, b = lane >> 2;
    const RowGeom g = make_geom(N);
    const long nsuper = (R + 31) >> 5;
    for (long st = (long)blockIdx.x * NW + wave; st < nsuper; st += (long)gridDim.x * NW)
        super_tile<S>(X, R, ldx, g, st, j, b, count, epilogue, finish);
}

// ---- The same words through LDS: a non-temporal LDS-DMA stream (k_bin_hist on the 15-, 18- and 25-state models, NG = 1..8) ----
// load_groups asks for every 128-byte line twice (64-byte halves of 16 rows per instruction), which is why plain nt loads lose
// (3.1-3.4 ms) and the launch reads at 5.3-5.4 TB/s in that shape.  global_load_lds_dwordx4 with per-lane SOURCE addresses fetches
// the same 16 rows as 1 KiB pieces that run along the rows -- piece p = 64 i + lane of instruction i is chunk p % C of row p / C
// (C = chunks per row), every line asked for once -- and takes nt: 7.0-7.1 TB/s for the bare stream against 5.3-5.4
// (tools/ubench/dma_stream.hip, profiles/r07a_*; the ring's depth and the waves per CU make no difference there).
// One slot of 16 rows per wave (16 x 16 C bytes, at most 16 KiB; 13.25 KiB at N = 833), lane-linear: chunk c of row r at 16 (r C + c).
// The wave that fills the slot is the wave that reads it, so nothing but its own vmcnt orders the two (no barrier, no hand-off):
//     read the slot into w[NG][8] (ds_read_b128, the lanes and the order of load_groups) | lgkmcnt(0): the slot is free |
//     DMA of the NEXT half tile | count this one from registers | vmcnt(0): the next has landed | epilogue, finish (H stores)
// -- one half tile ahead with the registers as the second buffer, and the wait stands BEFORE the H stores, so no load waits for
// a store.  The reads are inline asm: the compiler puts vmcnt(0) before any LDS access it sees while a DMA is pending.
// LDS budget of a workgroup: 4 slots = 1 KiB x C <= 64 KiB dynamic + bin_hist_body's static <= 6.6 KiB: two workgroups per CU
// (grid_for_tiles) fit the 160 KiB at every width.
// Needs X and ldx 16-byte aligned and 16 ldx < 2^32 (per-lane 32-bit offsets); the host takes load_groups otherwise.
// Rows past R (the last super-tile) and lanes past the 16 C pieces ask for X's first chunk or for nothing: no byte outside
// [X, X + R ldx) is requested.
typedef u32 epg_ldsx4 __attribute__((ext_vector_type(4)));

template <int NG>
struct DmaHalfTile {
    static constexpr int NI = 2 * NG;      // DMA instructions per half tile: pieces 64 i .. 64 i + 63, the last one or two partly or not used
    u32 soff[NI];                          // this lane's piece of instruction i: byte offset from the half tile's first row
    u64 rpack;                             // its row in the half tile, 4 bits per instruction
    char* slot;                            // the wave's slot
    u32 rd, rd_tail[2];                    // LDS addresses this lane reads: chunk j of row b; the clamped chunks of the last group
    int npieces;                           // 16 C

    __device__ __forceinline__ void init(char* ring, int wave, int lane, const RowGeom& g, long ldx) {
        const int j = lane & 3, b = lane >> 2, C = g.chunks;
        npieces = 16 * C;
        slot = ring + wave * (256 * C);
        rpack = 0;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int p = 64 * i + lane;
            int r = p / C;
            const int c = p - r * C;
            const bool used = r < 16;
            r = used ? r : 0;
            soff[i] = used ? (u32)r * (u32)ldx + 16u * (u32)c : 0u;
            rpack |= (u64)r << (4 * i);
        }
        const u32 row = (u32)(uintptr_t)slot + 16u * (u32)(b * C);
        rd = row + 16u * j;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int c = 4 * (NI - 2 + k) + j;
            rd_tail[k] = row + 16u * (u32)(c < g.last ? c : g.last);
        }
    }

    // request rows row0 .. row0 + 15 of X[R, ldx]
    __device__ __forceinline__ void fill(const char* __restrict__ X, long R, long ldx, long row0, int lane) const {
        const char* Xh = X + row0 * ldx;
        const long left = R - row0;        // rows of the half tile that exist (wave-uniform, may be <= 0)
        auto piece = [&](int i, const char* src) {
            if (i < NI - 2 || 64 * i + lane < npieces)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                                 (__attribute__((address_space(3))) void*)(slot + 1024 * i), 16, 0, 2 /* nt */);
        };
        if (left >= 16) {                  // (two loops: one with a select per piece costs every half tile 7 VALU per piece)
#pragma unroll
            for (int i = 0; i < NI; ++i) piece(i, Xh + soff[i]);
        } else {
#pragma unroll
            for (int i = 0; i < NI; ++i) piece(i, (long)((rpack >> (4 * i)) & 15) < left ? Xh + soff[i] : X);
        }
    }

    // every DMA this wave has issued has landed
    static __device__ __forceinline__ void wait() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

    // the slot's words in load_groups' layout (load_slot<true>'s masks on the last group); on return the slot may be refilled
    __device__ __forceinline__ void read(const RowGeom& g, int j, u32 (&w)[NG][8]) const {
        epg_ldsx4 v[NI];
        __builtin_amdgcn_sched_barrier(0);                                                           // (nothing between the reads and their wait)
#pragma unroll
        for (int i = 0; i < NI - 2; ++i) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v[i]) : "v"(rd), "n"(64 * i) : "memory");
        asm volatile("ds_read_b128 %0, %1" : "=v"(v[NI - 2]) : "v"(rd_tail[0]) : "memory");
        asm volatile("ds_read_b128 %0, %1" : "=v"(v[NI - 1]) : "v"(rd_tail[1]) : "memory");
#pragma unroll
        for (int i = 0; i < NI; ++i) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(v[i])::"memory");   // (names every destination)
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            u32* o = &w[i >> 1][4 * (i & 1)];
            o[0] = v[i].x; o[1] = v[i].y; o[2] = v[i].z; o[3] = v[i].w;
            if (i >= NI - 2) {
                const int c = 4 * i + j;
                const u32 inv = c > g.last ? 0xffffffffu : 0u;
                const bool is_last = c == g.last;
#pragma unroll
                for (int d = 0; d < 4; ++d) o[d] |= inv | (is_last ? g.tail[d] : 0u);
            }
        }
    }
};

// tile_loop with DmaHalfTile as the source of the words: the same super-tiles per wave, the same epilogue / finish calls
template <int S, int NG, int NW = 4, typename Epilogue, typename Finish>
__device__ __forceinline__ void tile_loop_dma(const char* __restrict__ X, long R, int N, long ldx, char* ring, Epilogue&& epilogue, Finish&& finish) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = lane & 3, b = lane >> 2;
    const RowGeom g = make_geom(N);
    const long nsuper = (R + 31) >> 5, stride = (long)gridDim.x * NW;
    long st = (long)blockIdx.x * NW + wave;
    if (st >= nsuper) return;              // (wave-uniform; the callers' barriers come after the loop, every wave reaches them)
    DmaHalfTile<NG> dma;
    dma.init(ring, wave, lane, g, ldx);
    dma.fill(X, R, ldx, st * 32, lane);
    dma.wait();
    for (; st < nsuper; st += stride) {
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const long row = st * 32 + half * 16 + b;
            u32 w[NG][8];
            dma.read(g, j, w);
            if (half == 0) dma.fill(X, R, ldx, st * 32 + 16, lane);
            else if (st + stride < nsuper) dma.fill(X, R, ldx, (st + stride) * 32, lane);
            u32 cnt[S];
#pragma unroll
            for (int s = 0; s < S; ++s) cnt[s] = 0;
#pragma unroll
            for (int t = 0; t < NG; ++t) count_group<S>(w[t], cnt);
            dma.wait();
            epilogue(half, row, row < R, cnt);
        }
        const long row0 = st * 32;
        finish(st, row0, (int)(R - row0 < 32 ? R - row0 : 32));
    }
}

// The same loop over SEVERAL matrices ("parts", epg_parts.h) in one launch, in super-tiles of 32 rows.  enter(part) tells the
// caller which part the following epilogue / finish calls belong to.  Every part must have a width in the instantiation's range
// (128 (NG - 1) < N <= 128 NG, or NG == 0).
constexpr int KH_MAXP = 48;
struct KhParts {
    const char* x[KH_MAXP];
    u16* h[KH_MAXP];                       // (not used by the loop: the caller's enter() picks it up)
    long rows[KH_MAXP];
    long ldx[KH_MAXP];
    long t0[KH_MAXP + 1];                  // first super-tile of every part, and their total
    int n_cols[KH_MAXP];
    int n;
};

template <int S, int NG, int NW = 4, typename Enter, typename Epilogue, typename Finish>
__device__ __forceinline__ void tile_loop_parts(const KhParts& pt, Enter&& enter, Epilogue&& epilogue, Finish&& finish) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = lane & 3, b = lane >> 2;
    const long nsuper = pt.t0[pt.n];
    PartCursor at;
    int part = -1;
    const char* X = nullptr;
    long R = 0, ldx = 0, base = 0;
    RowGeom g = make_geom(16);
    for (long st = (long)blockIdx.x * NW + wave; st < nsuper; st += (long)gridDim.x * NW) {
        at.advance(pt.t0, st, 32);               // (rows from the cached `base` below: with advance's own result every instantiation takes a VGPR more)
        if (at.part != part) {
            part = at.part;
            X = pt.x[part];
            R = pt.rows[part];
            ldx = pt.ldx[part];
            base = pt.t0[part];
            g = make_geom(pt.n_cols[part]);
            enter(part);
        }
        super_tile<S>(X, R, ldx, g, st - base, j, b, CountRow<S, NG>(), epilogue, finish);
    }
}

// Pack pairs of per-lane counts into uint16 halves and sum over the quad: d[m] = cnt[2m] | cnt[2m+1] << 16,
// every lane of the quad gets the bin's totals (a total never exceeds N <= 65535, so halves cannot carry).
// Half the DPP adds of an unpacked reduction, and d[] is already the uint16 row layout of H.
template <int S>
__device__ __forceinline__ void pack_reduce(const u32 (&cnt)[S], u32 (&d)[(S + 1) / 2]) {
#pragma unroll
    for (int m = 0; m < (S + 1) / 2; ++m) {
        const u32 hi = 2 * m + 1 < S ? cnt[2 * m + 1] : 0u;
        d[m] = quad_sum(cnt[2 * m] | (hi << 16));
    }
}

// pick x[j] for a quad lane j in 0..3 (3 v_cndmask)
__device__ __forceinline__ u32 sel4(u32 x0, u32 x1, u32 x2, u32 x3, int j) {
    const u32 lo = (j & 1) ? x1 : x0;
    const u32 hi = (j & 1) ? x3 : x2;
    return (j & 2) ? hi : lo;
}

// lane j of the quad takes the count of state 4k + j out of the packed d[] (0 past the last state).  Both halves are read before
// the pick: written as j & 2 ? d[2k + 1] : d[2k] the compiler picks between two ADDRESSES and d[] stays in memory (the 15- and
// 31-state count kernels held it in 8 KB of LDS or 48-80 bytes of scratch per lane).
template <int ND>
__device__ __forceinline__ u32 quad_state_count(const u32 (&d)[ND], int k, int j) {
    const u32 lo = d[2 * k], hi = 2 * k + 1 < ND ? d[2 * k + 1] : 0u;
    const u32 v = (j & 2) ? hi : lo;
    return (j & 1) ? v >> 16 : v & 0xffffu;
}

// Stage a bin's uint16 row of H (Sout <= S columns) at srow: d[] already is that layout, one dword per pair of states.
// WHOLE_DWORDS (even S, Sout == S): a quad lane stores whole dwords; else uint16 by uint16.
template <int S, bool WHOLE_DWORDS>
__device__ __forceinline__ void stage_hist_row(char* srow, const u32 (&d)[(S + 1) / 2], int j, int Sout) {
    constexpr int ND = (S + 1) / 2;
    if constexpr (WHOLE_DWORDS) {
        static_assert((S & 1) == 0, "whole dwords need an even row");
#pragma unroll
        for (int k = 0; k < (ND + 3) / 4; ++k) {
            const u32 v = sel4(d[4 * k], 4 * k + 1 < ND ? d[4 * k + 1] : 0u, 4 * k + 2 < ND ? d[4 * k + 2] : 0u, 4 * k + 3 < ND ? d[4 * k + 3] : 0u, j);
            if (4 * k + j < ND) *reinterpret_cast<u32*>(srow + 4 * (4 * k + j)) = v;
        }
    } else {
#pragma unroll
        for (int k = 0; k < (S + 3) / 4; ++k) {
            const u32 c = quad_state_count(d, k, j);
            if (4 * k + j < Sout) *reinterpret_cast<u16*>(srow + 2 * (4 * k + j)) = (u16)c;
        }
    }
}

// Running state totals of the bins a lane has counted, as packed uint16 pairs like d[]: added per epilogue, flushed into the
// block's s_cnt[S + 1] (u64, __shared__, zeroed by the kernel) before a half can overflow -- every flush_every epilogues, from the
// WIDEST row of the launch (nmax).  Every lane of a quad holds the same totals; lane j == 0 adds them.
template <int S>
struct StateTotals {
    static constexpr int ND = (S + 1) / 2;
    u32 accp[ND];
    int since, flush_every;
    __device__ __forceinline__ void init(int nmax) {
#pragma unroll
        for (int m = 0; m < ND; ++m) accp[m] = 0;
        flush_every = 65535 / nmax > 1 ? 65535 / nmax - 1 : 1;
        since = 0;
    }
    __device__ __forceinline__ void flush(u64* s_cnt, int j) {
        if (j == 0) {
#pragma unroll
            for (int m = 0; m < ND; ++m) {
                const u32 lo = accp[m] & 0xffffu, hi = accp[m] >> 16;
                if (lo) atomicAdd(&s_cnt[2 * m], (u64)lo);
                if (hi) atomicAdd(&s_cnt[2 * m + 1], (u64)hi);
            }
        }
#pragma unroll
        for (int m = 0; m < ND; ++m) accp[m] = 0;
        since = 0;
    }
    __device__ __forceinline__ void add(const u32 (&d)[ND], bool valid, u64* s_cnt, int j) {
#pragma unroll
        for (int m = 0; m < ND; ++m) accp[m] += valid ? d[m] : 0u;
        if (++since >= flush_every) flush(s_cnt, j);
    }
    // the whole block, after its loop: the last flush, then one global atomic per state
    __device__ __forceinline__ void commit(u64* s_cnt, int j, u64* __restrict__ counts, int Sout) {
        flush(s_cnt, j);
        __syncthreads();
        if ((int)threadIdx.x < Sout && s_cnt[threadIdx.x]) atomicAdd(&counts[threadIdx.x], s_cnt[threadIdx.x]);
    }
};

}  // namespace epg
