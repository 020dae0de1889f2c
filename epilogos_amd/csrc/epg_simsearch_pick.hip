// The device STEP 1 of `simsearch -b --step1 gpu` (include/epilogos_simsearch_pick.h): centre scores, rolling maximum, the rank of
// every window by (rolling max, rolling mean, centre score) and the greedy pick of non-overlapping windows, as a fixed point of
// local rules that a workgroup iterates inside an LDS tile.
//
// Both windowed passes -- the rolling maximum over W values and the pick's minimum over the 2 W - 1 neighbours of a position -- use
// van Herk's decomposition: the tile is cut into segments of the window's length L, a thread walks a segment once for its running
// prefix (another for its suffix), and a window that starts at a is op(suffix[a], prefix[a + L - 1]): two LDS reads per element
// whatever the window.  L is odd or the walkers few, so the walkers' LDS addresses (stride L words) do not pile on a bank.
#include "epg_common.h"
#include "epilogos_simsearch_pick.h"

#include <rocprim/device/device_radix_sort.hpp>

namespace epg {

constexpr int PK_THREADS = 256;
constexpr int PK_TILE = EPG_PICK_TILE;
constexpr int PK_PER_THREAD = PK_TILE / PK_THREADS;
constexpr int PK_MAX_W = EPG_PICK_MAX_W;
constexpr int PK_ELEMS = PK_TILE + 2 * (PK_MAX_W - 1);           // a pick tile and its two halos
constexpr int PK_BATCH = 4;                                      // sweeps between two reads of the counters
constexpr int RM_TILE = 1024;                                    // outputs of a rolling-max tile (float64: half a pick tile)
constexpr int RM_ELEMS = RM_TILE + PK_MAX_W - 1;
constexpr u32 PK_INF = 0xffffffffu;
enum : unsigned char { ST_UNDECIDED = 0, ST_PICKED = 1, ST_DROPPED = 2 };

static_assert(PK_TILE % PK_THREADS == 0, "a thread owns PK_PER_THREAD positions of a tile");
static_assert(3 * PK_ELEMS * 4 <= 49152 && 3 * RM_ELEMS * 8 <= 49152, "key, prefix and suffix of a tile in 48 KB of LDS");

// pre[j] = op(key[segment start .. j]), suf[j] = op(key[j .. segment end]) for the segments of L of key[0, m): the first half of
// the workgroup walks prefixes, the second suffixes.  The caller synchronises before (key complete) and after.
template <typename T, typename Op>
__device__ __forceinline__ void vh_scan(const T* key, T* pre, T* suf, int m, int L, Op op) {
    const int nseg = (m + L - 1) / L;
    const int half = PK_THREADS / 2;
    const bool back = (int)threadIdx.x >= half;
    for (int s = (int)threadIdx.x - (back ? half : 0); s < nseg; s += half) {
        const int a = s * L, b = min(a + L, m);
        if (!back) {
            T acc = key[a];
            pre[a] = acc;
            for (int j = a + 1; j < b; ++j) pre[j] = acc = op(acc, key[j]);
        } else {
            T acc = key[b - 1];
            suf[b - 1] = acc;
            for (int j = b - 2; j >= a; --j) suf[j] = acc = op(key[j], acc);
        }
    }
}

struct MinU32 {
    __device__ __forceinline__ u32 operator()(u32 a, u32 b) const { return a < b ? a : b; }
};
struct MaxF64 {
    __device__ __forceinline__ double operator()(double a, double b) const { return a > b ? a : b; }
};

// ---- centre scores -------------------------------------------------------------------------------------------------------------
constexpr int RS_ROWS = 256, RS_COLS = 32;

// A workgroup sums RS_ROWS rows, a thread one row; the rows pass through LDS RS_COLS columns at a time so that the loads are whole
// 128-byte pieces of a row (pitch RS_COLS + 1: the threads' reads of one column fall on different banks).
__global__ __launch_bounds__(RS_ROWS) void k_rowscore(const int* __restrict__ X, long R, int S, double* __restrict__ score) {
#pragma clang fp contract(off)
    __shared__ int tile[RS_ROWS][RS_COLS + 1];
    const long r0 = (long)blockIdx.x * RS_ROWS;
    const int rows = (int)min((long)RS_ROWS, R - r0);
    const int tid = threadIdx.x;
    double acc = 0.0;
    for (int c0 = 0; c0 < S; c0 += RS_COLS) {
        const int cw = min(RS_COLS, S - c0);
        __syncthreads();
        for (int idx = tid; idx < rows * RS_COLS; idx += RS_ROWS) {
            const int r = idx / RS_COLS, c = idx % RS_COLS;
            if (c < cw) tile[r][c] = X[(r0 + r) * S + c0 + c];
        }
        __syncthreads();
        if (tid < rows)
            for (int c = 0; c < cw; ++c) acc = acc + (double)tile[tid][c] / 100000.0;
    }
    if (tid < rows) score[r0 + tid] = acc;
}

// ---- rolling maximum -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PK_THREADS) void k_rolling_max(const double* __restrict__ v, long n, int W, double* __restrict__ out) {
    __shared__ double key[RM_ELEMS], pre[RM_ELEMS], suf[RM_ELEMS];
    const long t0 = (long)blockIdx.x * RM_TILE;
    const int core = (int)min((long)RM_TILE, n - t0);
    const int backw = W / 2, fwd = (W - 1) / 2;
    const int m = core + W - 1;                                  // tile element j is v[t0 - backw + j]
    for (int j = threadIdx.x; j < m; j += PK_THREADS) {
        const long g = t0 - backw + j;
        key[j] = g >= 0 && g < n ? v[g] : -__builtin_inf();
    }
    __syncthreads();
    vh_scan(key, pre, suf, m, W, MaxF64());
    __syncthreads();
    for (int k = threadIdx.x; k < core; k += PK_THREADS) {
        const long i = t0 + k;
        out[i] = i - backw < 0 || i + fwd >= n ? __builtin_nan("") : MaxF64()(suf[k], pre[k + W - 1]);
    }
}

// ---- rank ----------------------------------------------------------------------------------------------------------------------
// the order-preserving 64-bit image of a double (no NaN): a < b <=> image(a) < image(b); -0.0 and +0.0 share one
__device__ __forceinline__ u64 f64_image(double x) {
    if (x == 0.0) x = 0.0;
    const u64 b = (u64)__double_as_longlong(x);
    return b >> 63 ? ~b : b | 0x8000000000000000ull;
}

__global__ __launch_bounds__(256) void k_rank_keys(const double* __restrict__ src, const u32* __restrict__ perm, long n, u64* __restrict__ keys,
                                                   u32* __restrict__ iota) {
    const long j = (long)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    keys[j] = f64_image(src[perm ? perm[j] : j]);
    if (iota) iota[j] = (u32)j;
}

__global__ __launch_bounds__(256) void k_rank_scatter(const u32* __restrict__ perm, long n, u32* __restrict__ rank) {
    const long j = (long)blockIdx.x * 256 + threadIdx.x;
    if (j < n) rank[perm[j]] = (u32)j;
}

struct RankLayout {
    int64_t keys_a, keys_b, perm_a, perm_b, temp, total;
};

static int rank_layout(int64_t n, RankLayout& L) {
    L.keys_a = 0;
    L.keys_b = L.keys_a + align_up(n * 8, 256);
    L.perm_a = L.keys_b + align_up(n * 8, 256);
    L.perm_b = L.perm_a + align_up(n * 4, 256);
    L.temp = L.perm_b + align_up(n * 4, 256);
    size_t tb = 0;
    if (n > 0) {
        hipError_t e = rocprim::radix_sort_pairs_desc(nullptr, tb, (const u64*)nullptr, (u64*)nullptr, (const u32*)nullptr, (u32*)nullptr,
                                                      (size_t)n, 0, 64, (hipStream_t)0);
        if (e != hipSuccess) return fail(EPG_ERR_HIP, "simsearch_rank: radix sort size query failed: %s", hipGetErrorString(e));
    }
    L.total = align_up(L.temp + (int64_t)tb, 256);
    return EPG_OK;
}

// ---- pick ----------------------------------------------------------------------------------------------------------------------
// what a position shows its neighbours: 0 when picked (it drops them), its rank + 1 while undecided (the smallest wins), nothing
// once dropped
__device__ __forceinline__ u32 pick_key(unsigned char st, u32 rank) { return st == ST_PICKED ? 0u : st == ST_UNDECIDED ? rank + 1u : PK_INF; }

// One sweep: a workgroup takes a tile's states to the fixed point of the two rules, halo states frozen at st_in's, and writes the
// tile's states to st_out (a function of st_in alone: the sweeps are deterministic whatever runs beside what).  remaining receives
// the positions left undecided.
__global__ __launch_bounds__(PK_THREADS) void k_pick_sweep(const u32* __restrict__ rank, long n, int W, const unsigned char* __restrict__ st_in,
                                                           unsigned char* __restrict__ st_out, int* __restrict__ remaining) {
    __shared__ u32 key[PK_ELEMS], pre[PK_ELEMS], suf[PK_ELEMS];
    const long t0 = (long)blockIdx.x * PK_TILE;
    const int core = (int)min((long)PK_TILE, n - t0);
    const int H = W - 1, L = 2 * W - 1;
    const int m = core + 2 * H;                                  // tile element j is position t0 - H + j
    const int tid = threadIdx.x;
    u32 rk[PK_PER_THREAD];
    unsigned char st[PK_PER_THREAD];
    int und = 0;
#pragma unroll
    for (int e = 0; e < PK_PER_THREAD; ++e) {
        const int k = tid + e * PK_THREADS;
        st[e] = ST_DROPPED;
        rk[e] = 0;
        if (k < core) {
            st[e] = st_in[t0 + k];
            rk[e] = rank[t0 + k];
            und += st[e] == ST_UNDECIDED;
        }
    }
    if (__syncthreads_or(und)) {
        for (int j = tid; j < H; j += PK_THREADS) {
            const long gl = t0 - H + j, gr = t0 + core + j;
            key[j] = gl >= 0 ? pick_key(st_in[gl], rank[gl]) : PK_INF;
            key[H + core + j] = gr < n ? pick_key(st_in[gr], rank[gr]) : PK_INF;
        }
        int changed;
        do {
#pragma unroll
            for (int e = 0; e < PK_PER_THREAD; ++e) {
                const int k = tid + e * PK_THREADS;
                if (k < core) key[H + k] = pick_key(st[e], rk[e]);
            }
            __syncthreads();
            vh_scan(key, pre, suf, m, L, MinU32());
            __syncthreads();
            changed = 0;
#pragma unroll
            for (int e = 0; e < PK_PER_THREAD; ++e) {
                const int k = tid + e * PK_THREADS;
                if (k < core && st[e] == ST_UNDECIDED) {
                    const u32 mn = MinU32()(suf[k], pre[k + L - 1]);        // over positions t0 + k - H .. t0 + k + H
                    if (mn == 0u) st[e] = ST_DROPPED, changed = 1;
                    else if (mn == rk[e] + 1u) st[e] = ST_PICKED, changed = 1;
                }
            }
        } while (__syncthreads_or(changed));
    }
    und = 0;
#pragma unroll
    for (int e = 0; e < PK_PER_THREAD; ++e) {
        const int k = tid + e * PK_THREADS;
        if (k < core) {
            st_out[t0 + k] = st[e];
            und += st[e] == ST_UNDECIDED;
        }
    }
    if (und) atomicAdd(remaining, und);
}

// ---- compaction of the picked positions, ascending ------------------------------------------------------------------------------
// A workgroup takes PK_TILE positions, a thread PK_PER_THREAD consecutive ones, so that the order of the output is the order of
// the positions: count per workgroup, one exclusive scan over the workgroups' counts, scatter behind a scan over the threads'.
__device__ __forceinline__ bool pick_kept(const unsigned char* __restrict__ st, const u32* __restrict__ rank, long i, const u32* __restrict__ thr) {
    return st[i] == ST_PICKED && (!thr || rank[i] <= *thr);
}

// inclusive scan of one value per thread over the workgroup, through sc[PK_THREADS]
__device__ __forceinline__ u32 block_scan(u32* sc, u32 v) {
    const int tid = threadIdx.x;
    sc[tid] = v;
    __syncthreads();
    for (int d = 1; d < PK_THREADS; d <<= 1) {
        const u32 a = tid >= d ? sc[tid - d] : 0u;
        __syncthreads();
        sc[tid] += a;
        __syncthreads();
    }
    return sc[tid];
}

__global__ __launch_bounds__(PK_THREADS) void k_compact_count(const unsigned char* __restrict__ st, const u32* __restrict__ rank, long n,
                                                              const u32* __restrict__ thr, u32* __restrict__ blockcnt) {
    __shared__ u32 sc[PK_THREADS];
    const long i0 = (long)blockIdx.x * PK_TILE + (long)threadIdx.x * PK_PER_THREAD;
    u32 c = 0;
    for (int k = 0; k < PK_PER_THREAD; ++k)
        if (i0 + k < n) c += pick_kept(st, rank, i0 + k, thr);
    c = block_scan(sc, c);
    if (threadIdx.x == PK_THREADS - 1) blockcnt[blockIdx.x] = c;
}

// one workgroup: blockoff[b] = blockcnt[0] + ... + blockcnt[b - 1], *total = their sum
__global__ __launch_bounds__(PK_THREADS) void k_compact_offsets(const u32* __restrict__ blockcnt, long nb, u32* __restrict__ blockoff,
                                                                unsigned long long* __restrict__ total) {
    __shared__ u32 sc[PK_THREADS];
    u32 carry = 0;
    for (long base = 0; base < nb; base += PK_THREADS) {
        const long b = base + threadIdx.x;
        const u32 v = b < nb ? blockcnt[b] : 0u;
        const u32 incl = block_scan(sc, v);
        if (b < nb) blockoff[b] = carry + incl - v;
        carry += sc[PK_THREADS - 1];
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry;
}

// POSITIONS: out int64, the kept positions; else out uint32, their ranks.  out holds `room` entries: a permutation never yields
// more, and ranks that are none (equal ranks side by side are both picked) must not write past them.
template <bool POSITIONS>
__global__ __launch_bounds__(PK_THREADS) void k_compact_scatter(const unsigned char* __restrict__ st, const u32* __restrict__ rank, long n,
                                                                const u32* __restrict__ thr, const u32* __restrict__ blockoff, void* __restrict__ out, long room) {
    __shared__ u32 sc[PK_THREADS];
    const long i0 = (long)blockIdx.x * PK_TILE + (long)threadIdx.x * PK_PER_THREAD;
    u32 mask = 0, c = 0;
    for (int k = 0; k < PK_PER_THREAD; ++k)
        if (i0 + k < n && pick_kept(st, rank, i0 + k, thr)) mask |= 1u << k, ++c;
    long o = (long)blockoff[blockIdx.x] + block_scan(sc, c) - c;
    for (int k = 0; k < PK_PER_THREAD; ++k)
        if (mask >> k & 1 && o < room) {
            if (POSITIONS) reinterpret_cast<long long*>(out)[o++] = i0 + k;
            else reinterpret_cast<u32*>(out)[o++] = rank[i0 + k];
        }
}

// the largest rank that stays: the maxRegions-th smallest of the picked ranks when there are more than maxRegions
__global__ void k_pick_threshold(const u32* __restrict__ sorted, const unsigned long long* __restrict__ count, long maxRegions, u32* __restrict__ thr) {
    *thr = *count > (unsigned long long)maxRegions ? sorted[maxRegions - 1] : PK_INF;
}

struct PickLayout {
    int64_t st_a, st_b, cr, sorted, blockcnt, blockoff, count, thr, remaining, temp, temp_bytes, total;
};

static int pick_layout(int64_t n, int32_t W, PickLayout& L) {
    const int64_t cap = (n + W - 1) / W, tiles = (n + PK_TILE - 1) / PK_TILE;
    int64_t o = 0;
    auto take = [&](int64_t bytes) { const int64_t at = o; o += align_up(bytes, 256); return at; };
    L.st_a = take(n), L.st_b = take(n);
    L.cr = take(cap * 4), L.sorted = take(cap * 4);
    L.blockcnt = take(tiles * 4), L.blockoff = take(tiles * 4);
    L.count = take(8), L.thr = take(4), L.remaining = take(PK_BATCH * 4);
    size_t tb = 0;
    if (n > 0) {
        hipError_t e = rocprim::radix_sort_keys(nullptr, tb, (const u32*)nullptr, (u32*)nullptr, (size_t)cap, 0, 32, (hipStream_t)0);
        if (e != hipSuccess) return fail(EPG_ERR_HIP, "simsearch_pick: radix sort size query failed: %s", hipGetErrorString(e));
    }
    L.temp_bytes = (int64_t)tb;
    L.temp = take(L.temp_bytes);
    L.total = o;
    return EPG_OK;
}

static int pick_shape(int64_t n, int32_t W) {
    if (n < 0 || n > INT32_MAX - 1 || W < 1) return fail(EPG_ERR_INVALID_ARG, "simsearch_pick: bad shape (n=%lld, W=%d)", (long long)n, W);
    if (W > PK_MAX_W) return fail(EPG_ERR_UNSUPPORTED, "simsearch_pick: W=%d beyond %d", W, PK_MAX_W);
    return EPG_OK;
}

}  // namespace epg

using namespace epg;

extern "C" int epg_simsearch_rowscore(const int32_t* X, int64_t R, int32_t S, double* score, void* stream) {
    if (R < 0 || S < 1) return fail(EPG_ERR_INVALID_ARG, "simsearch_rowscore: bad shape (R=%lld, S=%d)", (long long)R, S);
    if (R == 0) return EPG_OK;
    if (!X || !score) return fail(EPG_ERR_INVALID_ARG, "simsearch_rowscore: NULL argument");
    if (R > (int64_t)INT32_MAX * RS_ROWS) return fail(EPG_ERR_INVALID_ARG, "simsearch_rowscore: %lld rows are too many", (long long)R);
    hipLaunchKernelGGL(k_rowscore, dim3((unsigned)((R + RS_ROWS - 1) / RS_ROWS)), dim3(RS_ROWS), 0, (hipStream_t)stream, X, (long)R, S, score);
    EPG_LAUNCH_CHECK("k_rowscore");
    return EPG_OK;
}

extern "C" int epg_simsearch_rolling_max(const double* v, int64_t n, int32_t W, double* out, void* stream) {
    if (n < 0 || W < 1) return fail(EPG_ERR_INVALID_ARG, "simsearch_rolling_max: bad shape (n=%lld, W=%d)", (long long)n, W);
    if (W > PK_MAX_W) return fail(EPG_ERR_UNSUPPORTED, "simsearch_rolling_max: W=%d beyond %d", W, PK_MAX_W);
    if (n == 0) return EPG_OK;
    if (!v || !out) return fail(EPG_ERR_INVALID_ARG, "simsearch_rolling_max: NULL argument");
    if (n > (int64_t)INT32_MAX * RM_TILE) return fail(EPG_ERR_INVALID_ARG, "simsearch_rolling_max: %lld values are too many", (long long)n);
    hipLaunchKernelGGL(k_rolling_max, dim3((unsigned)((n + RM_TILE - 1) / RM_TILE)), dim3(PK_THREADS), 0, (hipStream_t)stream, v, (long)n, W, out);
    EPG_LAUNCH_CHECK("k_rolling_max");
    return EPG_OK;
}

extern "C" int64_t epg_simsearch_rank_ws_bytes(int64_t n) {
    if (n < 0 || n > INT32_MAX) return fail(EPG_ERR_INVALID_ARG, "simsearch_rank: %lld windows outside 0 .. 2^31 - 1", (long long)n);
    RankLayout L;
    const int rc = rank_layout(n, L);
    return rc ? rc : L.total;
}

extern "C" int epg_simsearch_rank(const double* rmax, const double* rmean, const double* score, int64_t n, uint32_t* rank, void* ws,
                                  int64_t ws_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (n < 0 || n > INT32_MAX) return fail(EPG_ERR_INVALID_ARG, "simsearch_rank: %lld windows outside 0 .. 2^31 - 1", (long long)n);
    if (n == 0) return EPG_OK;
    if (!rmax || !rmean || !score || !rank || !ws) return fail(EPG_ERR_INVALID_ARG, "simsearch_rank: NULL argument");
    if (reinterpret_cast<uintptr_t>(ws) & 255) return fail(EPG_ERR_INVALID_ARG, "simsearch_rank: the workspace must be 256-byte aligned");
    RankLayout L;
    int rc = rank_layout(n, L);
    if (rc) return rc;
    if (ws_bytes < L.total) return fail(EPG_ERR_WORKSPACE, "simsearch_rank: workspace of %lld bytes, %lld needed", (long long)ws_bytes, (long long)L.total);
    char* base = (char*)ws;
    u64* keys_a = (u64*)(base + L.keys_a);
    u64* keys_b = (u64*)(base + L.keys_b);
    u32* perm[2] = {(u32*)(base + L.perm_a), (u32*)(base + L.perm_b)};
    const unsigned blocks = (unsigned)((n + 255) / 256);
    const double* cols[3] = {score, rmean, rmax};                // least significant key first: each pass is stable
    for (int p = 0; p < 3; ++p) {
        u32* from = perm[p & 1];
        u32* to = perm[(p + 1) & 1];
        hipLaunchKernelGGL(k_rank_keys, dim3(blocks), dim3(256), 0, st, cols[p], p ? from : (const u32*)nullptr, (long)n, keys_a, p ? (u32*)nullptr : from);
        EPG_LAUNCH_CHECK("k_rank_keys");
        size_t tb = (size_t)(L.total - L.temp);
        hipError_t e = rocprim::radix_sort_pairs_desc(base + L.temp, tb, keys_a, keys_b, from, to, (size_t)n, 0, 64, st);
        if (e != hipSuccess) return fail(EPG_ERR_HIP, "simsearch_rank: radix sort failed: %s", hipGetErrorString(e));
    }
    hipLaunchKernelGGL(k_rank_scatter, dim3(blocks), dim3(256), 0, st, perm[1], (long)n, rank);
    EPG_LAUNCH_CHECK("k_rank_scatter");
    return EPG_OK;
}

extern "C" int64_t epg_simsearch_pick_ws_bytes(int64_t n, int32_t W) {
    int rc = pick_shape(n, W);
    if (rc) return rc;
    PickLayout L;
    rc = pick_layout(n, W, L);
    return rc ? rc : L.total;
}

extern "C" int epg_simsearch_pick(const uint32_t* rank, int64_t n, int32_t W, int64_t maxRegions, int64_t* picked, int64_t* n_picked,
                                  int32_t* launches, void* ws, int64_t ws_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    int rc = pick_shape(n, W);
    if (rc) return rc;
    if (maxRegions < 0) return fail(EPG_ERR_INVALID_ARG, "simsearch_pick: maxRegions=%lld", (long long)maxRegions);
    if (!n_picked || !launches || (n > 0 && (!rank || !picked || !ws))) return fail(EPG_ERR_INVALID_ARG, "simsearch_pick: NULL argument");
    if (reinterpret_cast<uintptr_t>(ws) & 255) return fail(EPG_ERR_INVALID_ARG, "simsearch_pick: the workspace must be 256-byte aligned");
    PickLayout L;
    rc = pick_layout(n, W, L);
    if (rc) return rc;
    if (n > 0 && ws_bytes < L.total) return fail(EPG_ERR_WORKSPACE, "simsearch_pick: workspace of %lld bytes, %lld needed", (long long)ws_bytes, (long long)L.total);
    *launches = 0;
    if (n == 0 || maxRegions == 0) {
        EPG_HIP(hipMemsetAsync(n_picked, 0, 8, st));
        return EPG_OK;
    }
    char* base = (char*)ws;
    unsigned char* state[2] = {(unsigned char*)(base + L.st_a), (unsigned char*)(base + L.st_b)};
    u32* cr = (u32*)(base + L.cr);
    u32* sorted = (u32*)(base + L.sorted);
    unsigned long long* count = (unsigned long long*)(base + L.count);
    u32* thr = (u32*)(base + L.thr);
    int* remaining = (int*)(base + L.remaining);
    const int64_t cap = (n + W - 1) / W;
    const unsigned tiles = (unsigned)((n + PK_TILE - 1) / PK_TILE);

    EPG_HIP(hipMemsetAsync(state[0], 0, (size_t)n, st));         // ST_UNDECIDED
    int sweeps = 0, cur = 0, needed = 0;
    while (!needed) {
        if (sweeps > n) return fail(EPG_ERR_HIP, "simsearch_pick: %d sweeps left positions undecided (is rank a permutation?)", sweeps);
        EPG_HIP(hipMemsetAsync(remaining, 0, PK_BATCH * 4, st));
        for (int s = 0; s < PK_BATCH; ++s, cur ^= 1) {
            hipLaunchKernelGGL(k_pick_sweep, dim3(tiles), dim3(PK_THREADS), 0, st, rank, (long)n, W, state[cur], state[cur ^ 1], remaining + s);
            EPG_LAUNCH_CHECK("k_pick_sweep");
        }
        int left[PK_BATCH];
        EPG_HIP(hipMemcpyAsync(left, remaining, PK_BATCH * 4, hipMemcpyDeviceToHost, st));
        EPG_HIP(hipStreamSynchronize(st));
        for (int s = 0; s < PK_BATCH && !needed; ++s)
            if (left[s] == 0) needed = sweeps + s + 1;
        sweeps += PK_BATCH;
    }
    *launches = needed;
    const unsigned char* fin = state[cur];                       // the last sweep's output (the sweeps after `needed` only copied)

    u32* blockcnt = (u32*)(base + L.blockcnt);
    u32* blockoff = (u32*)(base + L.blockoff);
    const u32* keep_below = nullptr;
    if (maxRegions < cap) {                                      // (more than `cap` are never picked)
        EPG_HIP(hipMemsetAsync(cr, 0xff, (size_t)cap * 4, st));  // behind the picked ranks: PK_INF, sorted last
        hipLaunchKernelGGL(k_compact_count, dim3(tiles), dim3(PK_THREADS), 0, st, fin, rank, (long)n, (const u32*)nullptr, blockcnt);
        EPG_LAUNCH_CHECK("k_compact_count");
        hipLaunchKernelGGL(k_compact_offsets, dim3(1), dim3(PK_THREADS), 0, st, (const u32*)blockcnt, (long)tiles, blockoff, count);
        EPG_LAUNCH_CHECK("k_compact_offsets");
        hipLaunchKernelGGL(k_compact_scatter<false>, dim3(tiles), dim3(PK_THREADS), 0, st, fin, rank, (long)n, (const u32*)nullptr, (const u32*)blockoff, (void*)cr, (long)cap);
        EPG_LAUNCH_CHECK("k_compact_scatter");
        size_t tb = (size_t)L.temp_bytes;
        hipError_t e = rocprim::radix_sort_keys(base + L.temp, tb, (const u32*)cr, sorted, (size_t)cap, 0, 32, st);
        if (e != hipSuccess) return fail(EPG_ERR_HIP, "simsearch_pick: sort of the picked ranks failed: %s", hipGetErrorString(e));
        hipLaunchKernelGGL(k_pick_threshold, dim3(1), dim3(1), 0, st, (const u32*)sorted, (const unsigned long long*)count, (long)maxRegions, thr);
        EPG_LAUNCH_CHECK("k_pick_threshold");
        keep_below = thr;
    }
    hipLaunchKernelGGL(k_compact_count, dim3(tiles), dim3(PK_THREADS), 0, st, fin, rank, (long)n, keep_below, blockcnt);
    EPG_LAUNCH_CHECK("k_compact_count");
    hipLaunchKernelGGL(k_compact_offsets, dim3(1), dim3(PK_THREADS), 0, st, (const u32*)blockcnt, (long)tiles, blockoff,
                       reinterpret_cast<unsigned long long*>(n_picked));
    EPG_LAUNCH_CHECK("k_compact_offsets");
    hipLaunchKernelGGL(k_compact_scatter<true>, dim3(tiles), dim3(PK_THREADS), 0, st, fin, rank, (long)n, keep_below, (const u32*)blockoff, (void*)picked, (long)cap);
    EPG_LAUNCH_CHECK("k_compact_scatter");
    return EPG_OK;
}
