// Similarity search, the front of a live query (simsearch -q -s): the block reduction of the gridded genome and the block-reduced
// slices of query windows, both on the device -- similaritySearch_max_mean.py reduceGenome (:139-160) and makeSlice (:80-102) of the
// reference on exact integers.
//
// X is the gridded genome, int32 [R, S] ("%.5f" scores x 1e5).  A block is blockSize consecutive rows; its best row is the one
// with the largest exact (int64) row sum, the lowest row on ties (best_row, the one definition of the rule).
//
//   k_simsearch_reduce  one workgroup per tile of `tb` consecutive blocks of the genome: G_out[b] = X[best row of block b], a
//                       partial last block included.
//   k_simsearch_slices  grid (tiles of a window, queries): Q[i][b] = X[best row of block b of the window that starts at row
//                       first[i]].
//
// Both are reduce_tile on a run of rows: a single streaming pass.  The rows of a tile are contiguous in memory, so the tile is
// staged in LDS with 16-byte loads whatever S is (rows of S * 4 bytes are not 16-byte aligned for most S: the LDS copy keeps the
// source's alignment modulo 16 and only the tile's first and last partial chunk are loaded by dwords), each thread then sums one
// row out of LDS, one thread per block picks the best row, and the output rows leave LDS as 16-byte stores (same scheme on the
// destination's alignment).  Rows too long for a block of them to fit in LDS (blockSize * S > SP_TILE_MAX_INTS; no model of the
// reference comes near) take the unstaged form: one block per workgroup, one wave per row with lane-strided loads, the best row
// copied from global memory.
#include "epg_common.h"

namespace epg {

static constexpr int SP_THREADS = 256;
static constexpr int SP_MAX_ROWS = 512;          // rows of a tile, hence the largest blockSize
static constexpr int SP_TILE_INTS = 4096;        // values of a tile when blocks are small: 16 KB, several workgroups per CU
static constexpr int SP_TILE_MAX_INTS = 14000;   // values of a tile at most (with the sums and picks below 64 KB of LDS)
static constexpr int SP_MAX_NBLK = 64;           // blocks of a query window (epg_simsearch's SS_MAX_W)
static constexpr int SP_FIRSTS = 256;            // query windows per launch of k_simsearch_slices (their first rows are arguments)
static constexpr int SP_HEAD_BYTES = SP_MAX_ROWS * 8 + SP_MAX_ROWS * 4;   // sums, picks; a multiple of 16

typedef int epg_i32x4 __attribute__((ext_vector_type(4)));

// The best row of a block of n rows with the exact row sums `sums`: the largest sum, the lowest row on ties.
__device__ __forceinline__ int best_row(const long long* sums, int n) {
    int best = 0;
    long long top = sums[0];
    for (int r = 1; r < n; ++r) {
        if (sums[r] > top) {
            top = sums[r];
            best = r;
        }
    }
    return best;
}

// `rows` consecutive rows at src (row `row0` of the genome) -> the best row of each of their ceil(rows / bs) blocks at dst; kept
// (may be NULL) receives their genome row indices.  STAGED: rows * S <= SP_TILE_MAX_INTS.  rows <= SP_MAX_ROWS.
template <bool STAGED>
__device__ __forceinline__ void reduce_tile(const int32_t* __restrict__ src, int rows, int S, int bs, int32_t* __restrict__ dst,
                                            int64_t* __restrict__ kept, long row0) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    long long* sums = reinterpret_cast<long long*>(smem);
    int* pick = reinterpret_cast<int*>(smem + SP_MAX_ROWS * 8);
    int32_t* tile = reinterpret_cast<int32_t*>(smem + SP_HEAD_BYTES);
    const int t = threadIdx.x;
    const int32_t* data = src;                   // where the rows are read from after staging

    if (STAGED) {
        const int n = rows * S;
        const int mis = (int)((reinterpret_cast<uintptr_t>(src) >> 2) & 3);     // tile[mis + i] = src[i]: same alignment mod 16
        const int32_t* base = src - mis;                                        // 16-byte aligned; read from base[mis] on only
        const int total = mis + n;
        const int nvec = total >> 2;
        for (int v = t; v < nvec; v += SP_THREADS) {
            if (4 * v >= mis) {
                *reinterpret_cast<epg_i32x4*>(tile + 4 * v) = *reinterpret_cast<const epg_i32x4*>(base + 4 * v);
            } else {
                for (int i = mis; i < 4; ++i) tile[i] = base[i];
            }
        }
        for (int i = 4 * nvec + t; i < total; i += SP_THREADS)
            if (i >= mis) tile[i] = base[i];
        __syncthreads();
        data = tile + mis;
        for (int r = t; r < rows; r += SP_THREADS) {
            const int32_t* row = tile + mis + r * S;
            int j = (S & 1) ? 0 : r % S;         // an even S: neighbouring rows start a column apart, off each other's banks
            long long acc = 0;
            for (int k = 0; k < S; ++k) {
                acc += row[j];
                if (++j == S) j = 0;
            }
            sums[r] = acc;
        }
    } else {
        const int wave = t >> 6, lane = t & 63;
        for (int r = wave; r < rows; r += SP_THREADS / 64) {
            const int32_t* row = src + (long)r * S;
            long long acc = 0;
            for (int j = lane; j < S; j += 64) acc += row[j];
            for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
            if (lane == 0) sums[r] = acc;
        }
    }
    __syncthreads();
    const int nb = (rows + bs - 1) / bs;
    for (int b = t; b < nb; b += SP_THREADS) {
        const int r0 = b * bs;
        const int w = r0 + best_row(sums + r0, rows - r0 < bs ? rows - r0 : bs);
        pick[b] = w;
        if (kept) kept[b] = row0 + w;
    }
    __syncthreads();

    // the nb picked rows, contiguous at dst: whole 16-byte chunks of dst's alignment, dwords at the two ends
    typedef typename std::conditional<STAGED, int, long>::type idx_t;
    const idx_t nout = (idx_t)nb * S;
    const int misd = (int)((reinterpret_cast<uintptr_t>(dst) >> 2) & 3);
    int32_t* dbase = dst - misd;                 // written from dbase[misd] on only
    const idx_t totald = misd + nout;
    const idx_t nvecd = totald >> 2;
    for (idx_t v = t; v < nvecd; v += SP_THREADS) {
        if (4 * v >= misd) {
            const idx_t e = 4 * v - misd;
            int b = (int)(e / S);
            idx_t c = e - (idx_t)b * S;
            epg_i32x4 o;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                o[k] = data[(idx_t)pick[b] * S + c];
                if (++c == S) {
                    c = 0;
                    if (b + 1 < nb) ++b;
                }
            }
            *reinterpret_cast<epg_i32x4*>(dbase + 4 * v) = o;
        } else {
            for (int i = misd; i < 4; ++i) {
                const idx_t e = i - misd;
                dbase[i] = data[(idx_t)pick[e / S] * S + e % S];
            }
        }
    }
    for (idx_t i = 4 * nvecd + t; i < totald; i += SP_THREADS) {
        if (i >= misd) {
            const idx_t e = i - misd;
            dbase[i] = data[(idx_t)pick[e / S] * S + e % S];
        }
    }
}

template <bool STAGED>
__global__ __launch_bounds__(SP_THREADS) void k_simsearch_reduce(const int32_t* __restrict__ X, long R, int S, int bs, int tb,
                                                                  int32_t* __restrict__ G_out, int64_t* __restrict__ kept) {
    const long b0 = (long)blockIdx.x * tb;
    const long r0 = b0 * bs;
    const long left = R - r0;
    const int rows = left < (long)tb * bs ? (int)left : tb * bs;
    reduce_tile<STAGED>(X + r0 * S, rows, S, bs, G_out + b0 * S, kept ? kept + b0 : nullptr, r0);
}

struct SliceFirsts {
    long first[SP_FIRSTS];
};

template <bool STAGED>
__global__ __launch_bounds__(SP_THREADS) void k_simsearch_slices(const int32_t* __restrict__ X, int S, int bs, int nblk, int tb,
                                                                  SliceFirsts f, int32_t* __restrict__ Q) {
    const int i = blockIdx.y;
    const int b0 = blockIdx.x * tb;
    const int nb = nblk - b0 < tb ? nblk - b0 : tb;
    const long r0 = f.first[i] + (long)b0 * bs;
    reduce_tile<STAGED>(X + r0 * S, nb * bs, S, bs, Q + ((long)i * nblk + b0) * S, nullptr, r0);
}

// Blocks per tile: as many as fit SP_TILE_INTS values and SP_MAX_ROWS rows; a block larger than that alone, up to SP_TILE_MAX_INTS;
// 0 = a block does not fit in LDS (the unstaged form, one block per workgroup).
static int tile_blocks(int32_t S, int32_t bs) {
    const int64_t per = (int64_t)bs * S;
    if (per > SP_TILE_MAX_INTS) return 0;
    int64_t tb = SP_TILE_INTS / per;
    if (tb < 1) tb = 1;
    if (tb > SP_MAX_ROWS / bs) tb = SP_MAX_ROWS / bs;
    return (int)tb;
}

static size_t tile_lds_bytes(int tb, int32_t S, int32_t bs) {
    return (size_t)SP_HEAD_BYTES + (tb ? ((size_t)tb * bs * S + 4) * 4 : 0);
}

static int prep_check(const char* what, int64_t R, int32_t S, int32_t bs) {
    if (R < 1 || S < 1) return fail(EPG_ERR_INVALID_ARG, "%s: bad shape (%lld rows, %d states)", what, (long long)R, S);
    if (bs < 1 || bs > SP_MAX_ROWS) return fail(EPG_ERR_INVALID_ARG, "%s: block size %d outside 1..%d", what, bs, SP_MAX_ROWS);
    if (R > INT64_MAX / 4 / S) return fail(EPG_ERR_INVALID_ARG, "%s: %lld rows of %d states overflow", what, (long long)R, S);
    return EPG_OK;
}

extern "C" int epg_simsearch_reduce(const int32_t* X, int64_t R, int32_t S, int32_t blockSize, int32_t* G_out, int64_t* kept,
                                    void* stream) {
    hipStream_t st = (hipStream_t)stream;
    int rc = prep_check("simsearch_reduce", R, S, blockSize);
    if (rc) return rc;
    if (!X || !G_out) return fail(EPG_ERR_INVALID_ARG, "simsearch_reduce: NULL argument");
    const int64_t nblocks = (R + blockSize - 1) / blockSize;
    const int tb = tile_blocks(S, blockSize);
    const int64_t grid = tb ? (nblocks + tb - 1) / tb : nblocks;
    if (grid > INT32_MAX) return fail(EPG_ERR_INVALID_ARG, "simsearch_reduce: %lld tiles exceed the grid", (long long)grid);
    if (tb)
        hipLaunchKernelGGL(k_simsearch_reduce<true>, dim3((unsigned)grid), dim3(SP_THREADS), tile_lds_bytes(tb, S, blockSize), st, X,
                           (long)R, S, blockSize, tb, G_out, kept);
    else
        hipLaunchKernelGGL(k_simsearch_reduce<false>, dim3((unsigned)grid), dim3(SP_THREADS), tile_lds_bytes(0, S, blockSize), st, X,
                           (long)R, S, blockSize, 1, G_out, kept);
    EPG_LAUNCH_CHECK("k_simsearch_reduce");
    return EPG_OK;
}

extern "C" int epg_simsearch_slices(const int32_t* X, int64_t R, int32_t S, int32_t blockSize, int32_t nblk, const int64_t* first,
                                    int32_t B, int32_t* Q, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    int rc = prep_check("simsearch_slices", R, S, blockSize);
    if (rc) return rc;
    if (nblk < 1 || nblk > SP_MAX_NBLK) return fail(EPG_ERR_INVALID_ARG, "simsearch_slices: window of %d blocks outside 1..%d", nblk, SP_MAX_NBLK);
    if (B < 1) return fail(EPG_ERR_INVALID_ARG, "simsearch_slices: bad batch size %d", B);
    if (!X || !first || !Q) return fail(EPG_ERR_INVALID_ARG, "simsearch_slices: NULL argument");
    const int64_t span = (int64_t)nblk * blockSize;
    for (int32_t i = 0; i < B; ++i)
        if (first[i] < 0 || first[i] > R - span)
            return fail(EPG_ERR_INVALID_ARG, "simsearch_slices: window %d (rows %lld .. %lld) is outside the %lld rows of the genome", i,
                        (long long)first[i], (long long)(first[i] + span), (long long)R);
    int tb = tile_blocks(S, blockSize);
    const bool staged = tb > 0;
    if (!staged) tb = 1;
    const unsigned tiles = (unsigned)((nblk + tb - 1) / tb);
    const size_t lds = tile_lds_bytes(staged ? tb : 0, S, blockSize);
    for (int32_t i0 = 0; i0 < B; i0 += SP_FIRSTS) {
        const int32_t nq = B - i0 < SP_FIRSTS ? B - i0 : SP_FIRSTS;
        SliceFirsts f;
        for (int32_t i = 0; i < SP_FIRSTS; ++i) f.first[i] = i < nq ? (long)first[i0 + i] : 0;
        int32_t* q = Q + (int64_t)i0 * nblk * S;
        if (staged)
            hipLaunchKernelGGL(k_simsearch_slices<true>, dim3(tiles, (unsigned)nq), dim3(SP_THREADS), lds, st, X, S, blockSize, nblk, tb, f, q);
        else
            hipLaunchKernelGGL(k_simsearch_slices<false>, dim3(tiles, (unsigned)nq), dim3(SP_THREADS), lds, st, X, S, blockSize, nblk, tb, f, q);
        EPG_LAUNCH_CHECK("k_simsearch_slices");
    }
    return EPG_OK;
}

}  // namespace epg
