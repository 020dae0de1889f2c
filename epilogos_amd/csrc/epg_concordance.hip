// Biosample concordance: for every PAIR of columns of a state matrix, the bins in which both hold the same state (agree) and the
// bins in which both hold a state at all (both) (include/epilogos_concordance.h).  gfx950 only.
//
// Two kernels per chunk of bins, no matrix cores:
//   * k_concordance_planes turns 32 consecutive bins of a column into NP + 1 dwords: bit b of plane k < NP is bit k of the state of
//     bin b, plane NP says which of the 32 bytes are states (whole bytes compared, S <= 127; rows behind R and the columns
//     N .. npad - 1 are "no state").  NP = 5 for models of up to 32 states, 7 above.  A thread takes 4 columns x 32 bins: one
//     dword load per bin (byte loads in the one column quad that crosses N), the bits of a plane gathered four columns at a
//     time with shifted masks, then 16-byte stores.  Layout P[word][plane][column], npad = N rounded up to 64 columns.
//   * k_concordance_pairs: a wave owns a tile of 16 columns i x 64 columns j and a segment of the chunk's words.  LANES RUN OVER j:
//     a lane loads the NP + 1 dwords of its column j (256 contiguous bytes per plane and wave), the dwords of the 16 columns i
//     are wave-uniform (scalar loads, SGPR operands).  Per pair and word: v_xor, NP - 1 v_bitop3 (d |= a ^ b), one v_bitop3
//     (~d & valid_a & valid_b), v_bcnt accumulating agree; v_and and v_bcnt for both: NP + 4 VALU instructions for 32 bins of a
//     pair.  The lane's 2 x 16 counters ARE the pairs' sums, no reduction over the wave.  Only tiles that hold a pair i <= j are
//     computed; the epilogue adds a tile's pairs i <= j to [i, j] (lanes along a row) and its pairs i < j to [j, i], transposed
//     through the wave's LDS so that 16 lanes cover 128 contiguous bytes of a row there too.  64-bit global atomics.
// A call of fewer than 32 bins has no full word: k_concordance_few compares the bytes themselves, one thread per pair.
// Counters: a lane's u32 counter grows by at most 32 per word and a segment is at most 2^26 words, so it stays below 2^31; the
// outputs are 64-bit.  All sums are integers: the result is exact and the same on any grid, for any R.
// Workspace: words x (NP + 1) x npad dwords; what does not fit in R * N + 2^20 bytes is walked in chunks of words (one word of
// all columns is at most 32 (N + 63) bytes, which R >= 32 bins always pay for).
#include "epg_count.h"
#include "epilogos_concordance.h"

namespace epg {

constexpr int CC_TI = 16;                  // columns i of a tile: their plane words are the wave's scalar operands
constexpr int CC_TJ = 64;                  // columns j of a tile: one per lane
constexpr int CC_WAVES = 4;                // waves of a pair block: four tiles i of one j-block (CC_TJ / CC_TI of them make a square)
constexpr int CC_LD = CC_TJ + 1;           // row stride of the epilogue's LDS tile
constexpr long CC_SEG_WORDS = 1L << 26;    // most words of an item: 32 x 2^26 = 2^31 bins per u32 counter
constexpr int CC_FEW = 32;                 // calls of fewer bins take k_concordance_few

static inline int cc_planes(int S) { return S <= 32 ? 5 : 7; }
static inline int cc_npad(int N) { return (N + CC_TJ - 1) / CC_TJ * CC_TJ; }
static inline int64_t cc_word_bytes(int N, int S) { return (int64_t)cc_npad(N) * (cc_planes(S) + 1) * 4; }

static int64_t cc_ws_bytes(int64_t R, int N, int S) {
    if (R < CC_FEW) return 256;
    const __int128 words = ((__int128)R + 31) / 32;
    const __int128 full = (words * cc_word_bytes(N, S) + 255) / 256 * 256;
    const __int128 cap = ((__int128)R * N + (1 << 20)) / 256 * 256;
    const __int128 need = full < cap ? full : cap;
    return need > INT64_MAX ? INT64_MAX / 256 * 256 : (int64_t)need;
}

template <int NP>
__global__ __launch_bounds__(256) void k_concordance_planes(const char* __restrict__ X, long R, int N, long ldx, int S, long w0, long nw, int npad,
                                                            u32* __restrict__ P) {
    const int nq = npad >> 2;
    const long total = nw * nq;
    // byte >= S in a dword's four bytes (S <= 127): bit 7 set, or the low seven bits + (128 - S) carry into bit 7
    const u32 swar_add = (u32)(128 - S) * 0x01010101u;
    for (long t = blockIdx.x * 256L + threadIdx.x; t < total; t += gridDim.x * 256L) {
        const long wl = t / nq;
        const int c0 = (int)(t - wl * nq) * 4;
        const int nc = N - c0;                               // columns of the four that exist (<= 0: none)
        const long row0 = (w0 + wl) * 32;
        u32 T[NP + 1][4];                                    // T[k][g]: byte c = bit k of column c0 + c in bins 8g .. 8g + 7
#pragma unroll
        for (int k = 0; k <= NP; ++k)
#pragma unroll
            for (int g = 0; g < 4; ++g) T[k][g] = 0;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                const long row = row0 + 8 * g + b;
                u32 w = 0xffffffffu;                         // what does not exist is no state
                if (row < R && nc > 0) {
                    const char* p = X + row * ldx + c0;
                    if (nc >= 4) {
                        __builtin_memcpy(&w, p, 4);          // (any alignment: one global_load_dword)
                    } else {                                 // the quad that crosses N: the row may end at N
                        w = 0xffffff00u | (unsigned char)p[0];
                        if (nc > 1) w = (w & 0xffff00ffu) | ((u32)(unsigned char)p[1] << 8);
                        if (nc > 2) w = (w & 0xff00ffffu) | ((u32)(unsigned char)p[2] << 16);
                    }
                }
                const u32 bad = w | ((w & 0x7f7f7f7fu) + swar_add);
#pragma unroll
                for (int k = 0; k < NP; ++k) T[k][g] |= ((w >> k) & 0x01010101u) << b;
                T[NP][g] |= ((~bad >> 7) & 0x01010101u) << b;
            }
        }
        u32* out = P + (wl * (NP + 1)) * npad + c0;
#pragma unroll
        for (int k = 0; k <= NP; ++k) {
            u32 o[4];
#pragma unroll
            for (int c = 0; c < 4; ++c)
                o[c] = ((T[k][0] >> (8 * c)) & 0xffu) | (((T[k][1] >> (8 * c)) & 0xffu) << 8) | (((T[k][2] >> (8 * c)) & 0xffu) << 16) |
                       (((T[k][3] >> (8 * c)) & 0xffu) << 24);
            *reinterpret_cast<uint4*>(out + (long)k * npad) = make_uint4(o[0], o[1], o[2], o[3]);
        }
    }
}

// the tiles that hold a pair i <= j: j-block tj has the 4 (tj + 1) tiles ti = 0 .. 4 tj + 3, the blocks before it 2 tj (tj + 1)
static inline long cc_tiles(int npad) {
    const long ntj = npad / CC_TJ;
    return 2 * ntj * (ntj + 1);
}

template <int NP, bool BOTH>
__global__ __launch_bounds__(CC_WAVES * 64) void k_concordance_pairs(const u32* __restrict__ P, long nw, int npad, int N, long ntiles, int nseg,
                                                                    long seg_words, u64* __restrict__ agree, u64* __restrict__ both) {
    __shared__ u32 s_tile[CC_WAVES][CC_TI * CC_LD];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    u32* const tl = s_tile[wave];
    // a block's four waves take four consecutive tiles of ONE j-block (a j-block has a multiple of four) and the same segment:
    // they load the same words of the columns j at about the same time, so three of the four find them in the CU's L1
    const long items = ntiles / CC_WAVES * nseg;
    for (long it = blockIdx.x; it < items; it += gridDim.x) {
        const long tile = it / nseg * CC_WAVES + wave;
        const int seg = (int)(it % nseg);
        int tj = (int)((sqrt(1.0 + 2.0 * (double)tile) - 1.0) * 0.5);
        while (2L * (tj + 1) * (tj + 2) <= tile) ++tj;
        while (2L * tj * (tj + 1) > tile) --tj;
        const int i0 = (int)(tile - 2L * tj * (tj + 1)) * CC_TI, j0 = tj * CC_TJ;
        const long wa = seg * seg_words, wb = wa + seg_words < nw ? wa + seg_words : nw;
        u32 ca[CC_TI], cb[CC_TI];
#pragma unroll
        for (int ii = 0; ii < CC_TI; ++ii) ca[ii] = cb[ii] = 0;
        for (long w = wa; w < wb; ++w) {
            const u32* pw = P + w * (NP + 1) * npad;
            u32 b[NP + 1];
#pragma unroll
            for (int k = 0; k <= NP; ++k) b[k] = pw[(long)k * npad + j0 + lane];
#pragma unroll
            for (int ii = 0; ii < CC_TI; ++ii) {
                const u32* pa = pw + i0 + ii;                        // wave-uniform
                u32 d = pa[0] ^ b[0];
#pragma unroll
                for (int k = 1; k < NP; ++k) d = EPG_B3(d, pa[(long)k * npad], b[k], 0xF6);      // d | (a ^ b)
                const u32 va = pa[(long)NP * npad];
                ca[ii] += (u32)__builtin_popcount(EPG_B3(d, va, b[NP], 0x08));                   // ~d & va & vb
                if constexpr (BOTH) cb[ii] += (u32)__builtin_popcount(va & b[NP]);
            }
        }
        // pairs i <= j of the tile to [i, j]: a wave instruction covers 64 consecutive counts of row i
        const int j = j0 + lane;
#pragma unroll
        for (int ii = 0; ii < CC_TI; ++ii) {
            const int i = i0 + ii;
            if (j < N && i <= j) {
                if (ca[ii]) atomicAdd(&agree[(long)i * N + j], (u64)ca[ii]);
                if constexpr (BOTH)
                    if (cb[ii]) atomicAdd(&both[(long)i * N + j], (u64)cb[ii]);
            }
        }
        // pairs i < j to [j, i], transposed through LDS: 16 lanes cover the 16 columns i of a row j, four rows an instruction
#pragma unroll
        for (int pass = 0; pass < (BOTH ? 2 : 1); ++pass) {
            u64* const out = pass ? both : agree;
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int ii = 0; ii < CC_TI; ++ii) tl[ii * CC_LD + lane] = pass ? cb[ii] : ca[ii];
            __builtin_amdgcn_wave_barrier();
            const int ii = lane & (CC_TI - 1), i = i0 + ii;
            for (int jj = lane >> 4; jj < CC_TJ; jj += 64 / CC_TI) {
                const u32 v = tl[ii * CC_LD + jj];
                const int jr = j0 + jj;
                if (jr < N && i < jr && v) atomicAdd(&out[(long)jr * N + i], (u64)v);
            }
            __builtin_amdgcn_wave_barrier();
        }
    }
}

// fewer than 32 bins: one thread per ordered pair, the bytes themselves
__global__ __launch_bounds__(256) void k_concordance_few(const char* __restrict__ X, int R, int N, long ldx, int S, u64* __restrict__ agree,
                                                         u64* __restrict__ both) {
    const long total = (long)N * N;
    for (long p = blockIdx.x * 256L + threadIdx.x; p < total; p += gridDim.x * 256L) {
        const int i = (int)(p / N), j = (int)(p - (long)i * N);
        u32 a = 0, c = 0;
        for (int r = 0; r < R; ++r) {
            const u32 xi = (unsigned char)X[r * ldx + i], xj = (unsigned char)X[r * ldx + j];
            const bool vv = xi < (u32)S && xj < (u32)S;
            c += vv;
            a += vv && xi == xj;
        }
        if (a) agree[p] += a;                                 // (the pair is this thread's alone)
        if (both && c) both[p] += c;
    }
}

template <int NP>
static int launch_concordance(const char* X, long R, int N, long ldx, int S, u64* agree, u64* both, u32* P, long chunk_words, hipStream_t st) {
    const int npad = cc_npad(N);
    const long words = (R + 31) / 32;
    const long ntiles = cc_tiles(npad);
    const long slots = (long)num_cus() * 8 * CC_WAVES;                 // waves the device holds at once
    for (long w0 = 0; w0 < words; w0 += chunk_words) {
        const long nw = words - w0 < chunk_words ? words - w0 : chunk_words;
        const long threads = nw * (npad >> 2);
        long grid = (threads + 255) / 256;
        grid = grid < (long)num_cus() * 8 ? grid : (long)num_cus() * 8;
        hipLaunchKernelGGL((k_concordance_planes<NP>), dim3((unsigned)grid), dim3(256), 0, st, X, R, N, ldx, S, w0, nw, npad, P);
        EPG_LAUNCH_CHECK("k_concordance_planes");
        // segments of the chunk's words: as many as keep every wave slot busy in one round, none longer than the counters allow
        long nseg = slots / ntiles;
        nseg = nseg < 1 ? 1 : (nseg > nw ? nw : nseg);
        long seg_words = (nw + nseg - 1) / nseg;
        seg_words = seg_words < CC_SEG_WORDS ? seg_words : CC_SEG_WORDS;
        nseg = (nw + seg_words - 1) / seg_words;
        grid = ntiles / CC_WAVES * nseg;                                 // a block: four tiles of a j-block, one segment
        grid = grid < (long)num_cus() * 8 ? grid : (long)num_cus() * 8;
        if (both)
            hipLaunchKernelGGL((k_concordance_pairs<NP, true>), dim3((unsigned)grid), dim3(CC_WAVES * 64), 0, st, P, nw, npad, N, ntiles, (int)nseg,
                               seg_words, agree, both);
        else
            hipLaunchKernelGGL((k_concordance_pairs<NP, false>), dim3((unsigned)grid), dim3(CC_WAVES * 64), 0, st, P, nw, npad, N, ntiles, (int)nseg,
                               seg_words, agree, both);
        EPG_LAUNCH_CHECK("k_concordance_pairs");
    }
    return EPG_OK;
}

static int cc_check_shape(const char* who, int64_t R, int32_t N, int64_t ldx, int32_t S) {
    if (R < 0 || N < 1 || S < 1 || ldx < N)
        return fail(EPG_ERR_INVALID_ARG, "%s: bad shape R=%lld N=%d ldx=%lld S=%d", who, (long long)R, N, (long long)ldx, S);
    if (S > 127) return fail(EPG_ERR_UNSUPPORTED, "%s: S=%d > 127", who, S);
    if (N > 65535) return fail(EPG_ERR_UNSUPPORTED, "%s: N=%d > 65535", who, N);
    return EPG_OK;
}

extern "C" int64_t epg_concordance_ws_bytes(int64_t R, int32_t N, int32_t S) {
    if (cc_check_shape("concordance_ws_bytes", R, N, N, S) != EPG_OK) return -1;
    return cc_ws_bytes(R, N, S);
}

extern "C" int epg_concordance(const int8_t* X8, int64_t R, int32_t N, int64_t ldx, int32_t S, int64_t* agree, int64_t* both, void* ws,
                               int64_t ws_bytes, void* stream) {
    const int rc = cc_check_shape("concordance", R, N, ldx, S);
    if (rc != EPG_OK) return rc;
    if (R == 0) return EPG_OK;
    if (!X8) return fail(EPG_ERR_INVALID_ARG, "concordance: X is NULL");
    if (!agree) return fail(EPG_ERR_INVALID_ARG, "concordance: agree is NULL");
    if (!ws) return fail(EPG_ERR_INVALID_ARG, "concordance: ws is NULL");
    if (reinterpret_cast<uintptr_t>(ws) & 255) return fail(EPG_ERR_INVALID_ARG, "concordance: ws is not 256-byte aligned");
    const int64_t need = cc_ws_bytes(R, N, S);
    if (ws_bytes < need) return fail(EPG_ERR_WORKSPACE, "concordance: workspace %lld < %lld bytes", (long long)ws_bytes, (long long)need);
    const char* X = reinterpret_cast<const char*>(X8);
    u64* a = reinterpret_cast<u64*>(agree);
    u64* b = reinterpret_cast<u64*>(both);
    hipStream_t st = (hipStream_t)stream;
    if (R < CC_FEW) {
        long grid = ((long)N * N + 255) / 256;
        grid = grid < (long)num_cus() * 8 ? grid : (long)num_cus() * 8;
        hipLaunchKernelGGL(k_concordance_few, dim3((unsigned)grid), dim3(256), 0, st, X, (int)R, N, ldx, S, a, b);
        EPG_LAUNCH_CHECK("k_concordance_few");
        return EPG_OK;
    }
    const long chunk_words = ws_bytes / cc_word_bytes(N, S);          // >= 1: see cc_ws_bytes
    if (cc_planes(S) == 5) return launch_concordance<5>(X, R, N, ldx, S, a, b, static_cast<u32*>(ws), chunk_words, st);
    return launch_concordance<7>(X, R, N, ldx, S, a, b, static_cast<u32*>(ws), chunk_words, st);
}

}  // namespace epg
