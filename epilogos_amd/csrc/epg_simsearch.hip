// Similarity search (simsearch -b, STEP 2): for a batch of regions of interest (ROIs), the squared Euclidean distance of every
// W-row window of the block-reduced genome to each ROI, the stable order of those distances, their mode and the greedy pick of
// up to n non-overlapping windows closer than half the mode -- the reference's runEuclideanDistance
// (similaritySearch_calc.py:67-123) on exact integers.
//
// Scores are the "%.5f" values of the scores file scaled by 1e5 (int32).  D[r][p] = sum_{k<W} sum_s (G[p+k][s] - Q_r[k][s])^2 is
// accumulated in fp64 on integer-valued doubles: exact while every partial sum is below 2^53, which the caller's key_bound
// certifies (a bound of every D of the call; the entry point refuses key_bound >= 2^53 with EPG_ERR_UNSUPPORTED).
//
//   k_simsearch_dist    grid (position tiles, ROI groups of RB): a tile of TP + W - 1 genome rows staged in LDS once (dynamic
//                       LDS of just that size, so small models keep many workgroups per CU), each thread
//                       one window position and RB ROIs (the genome value read from LDS once serves RB ROIs; the ROI values are
//                       wave-uniform loads).  keys[r][p] = D as uint64.
//   rocprim radix sort  per ROI, stable, (key, position) pairs, over the bit length of key_bound only.
//   k_simsearch_select  one workgroup per ROI: the mode (longest run of the sorted keys, the first -- smallest -- on ties), then
//                       wave 0 walks the sorted pairs: overlap with the ROI's own window or a picked window first, then the
//                       threshold 2*D > mode (-1 fill), else pick; candidates that run out leave zeros.
#include "epg_common.h"

#include <rocprim/device/device_radix_sort.hpp>

namespace epg {

static constexpr int SS_RB = 4;              // ROIs per thread of the distance kernel
static constexpr int SS_LDS_INTS = 16000;    // genome tile budget (at most 64 000 bytes of dynamic LDS, sized per call)
static constexpr int SS_MAX_W = 64;          // window rows

template <int TP>
__global__ __launch_bounds__(TP) void k_simsearch_dist(const int32_t* __restrict__ G, long Pg, int S, int W,
                                                        const int32_t* __restrict__ Q, int B, u64* __restrict__ keys) {
    extern __shared__ int32_t tile[];          // (TP + W - 1) * S values
    const long P = Pg - W + 1;
    const long p0 = (long)blockIdx.x * TP;
    const int t = threadIdx.x;
    const long row_end = (p0 + TP + W - 1 < Pg) ? p0 + TP + W - 1 : Pg;
    const long n_ints = (row_end - p0) * S;
    const int32_t* src = G + p0 * S;
    for (long i = t; i < n_ints; i += TP) tile[i] = src[i];
    __syncthreads();
    const long p = p0 + t;
    if (p >= P) return;
    const int WS = W * S;
    const int r0 = blockIdx.y * SS_RB;
    const int nr = (B - r0 < SS_RB) ? B - r0 : SS_RB;
    const int32_t* q = Q + (long)r0 * WS;
    const int32_t* g = tile + t * S;
    double acc[SS_RB];
#pragma unroll
    for (int rr = 0; rr < SS_RB; ++rr) acc[rr] = 0.0;
    if (nr == SS_RB) {
        for (int j = 0; j < WS; ++j) {
            const double gv = (double)g[j];
#pragma unroll
            for (int rr = 0; rr < SS_RB; ++rr) {
                const double d = gv - (double)q[(long)rr * WS + j];
                acc[rr] = fma(d, d, acc[rr]);
            }
        }
    } else {
        for (int j = 0; j < WS; ++j) {
            const double gv = (double)g[j];
            for (int rr = 0; rr < nr; ++rr) {
                const double d = gv - (double)q[(long)rr * WS + j];
                acc[rr] = fma(d, d, acc[rr]);
            }
        }
    }
    for (int rr = 0; rr < nr; ++rr) keys[(long)(r0 + rr) * P + p] = (u64)acc[rr];
}

__global__ void k_simsearch_iota(int32_t* __restrict__ v, long n) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) v[i] = (int32_t)i;
}

// first index in (i, n) whose key differs from k[i] (k sorted ascending), by galloping then bisection
__device__ static long run_end(const u64* k, long i, long n) {
    const u64 v = k[i];
    long lo = i, step = 1;                  // k[lo] == v
    while (lo + step < n && k[lo + step] == v) {
        lo += step;
        step <<= 1;
    }
    long hi = (lo + step < n) ? lo + step : n;   // k[hi] != v or hi == n
    while (hi - lo > 1) {
        const long mid = lo + (hi - lo) / 2;
        if (k[mid] == v) lo = mid; else hi = mid;
    }
    return hi;
}

static constexpr int SEL_THREADS = 256;
static constexpr int SEL_E = 8;              // contiguous keys per thread and step of the mode scan

__global__ __launch_bounds__(SEL_THREADS) void k_simsearch_select(const u64* __restrict__ skeys, const int32_t* __restrict__ spos,
                                                                  long P, const int32_t* __restrict__ self_start, int W, int n,
                                                                  int32_t* __restrict__ idx, u64* __restrict__ mode_out) {
    __shared__ u64 red[SEL_THREADS];
    __shared__ int32_t picked[1024];
    const int r = blockIdx.x;
    const int t = threadIdx.x;
    const u64* k = skeys + (long)r * P;
    const int32_t* pos = spos + (long)r * P;

    // ---- mode: the longest run, the first run on ties; packed (length << 32 | ~start) so that one max picks it
    u64 best = 0;
    for (long base = (long)t * SEL_E; base < P; base += (long)SEL_THREADS * SEL_E) {
        const long end = (base + SEL_E < P) ? base + SEL_E : P;
        u64 prev = base ? k[base - 1] : 0;
        for (long i = base; i < end; ++i) {
            const u64 v = k[i];
            if (i == 0 || v != prev) {
                long e = i + 1;
                while (e < end && k[e] == v) ++e;
                if (e == end && e < P && k[e] == v) e = run_end(k, e, P);
                const u64 cand = ((u64)(e - i) << 32) | (u64)(0xFFFFFFFFu - (u32)i);
                if (cand > best) best = cand;
            }
            prev = v;
        }
    }
    red[t] = best;
    __syncthreads();
    for (int s = SEL_THREADS / 2; s > 0; s >>= 1) {
        if (t < s && red[t + s] > red[t]) red[t] = red[t + s];
        __syncthreads();
    }
    const long mstart = (long)(0xFFFFFFFFu - (u32)(red[0] & 0xFFFFFFFFu));
    const u64 mode = k[mstart];
    if (t >= 64) return;                      // the greedy pick is wave 0's (no barrier below)

    // ---- greedy pick over the sorted pairs: 64 candidates per load, tested one after the other against the ROI's own window
    // and the picked windows (one per lane, strided); all lanes write a pick (the same value) so that each sees it
    const long rs = self_start[r];
    int npicked = 0;
    int fill = 0;                             // value of the slots after the last pick: 0 = candidates ran out, -1 = threshold
    bool done = false;
    for (long base = 0; base < P && !done; base += 64) {
        const long i = base + t;
        const u64 ck = i < P ? k[i] : 0;
        const int cp = i < P ? pos[i] : 0;
        const int m = (P - base < 64) ? (int)(P - base) : 64;
        for (int c = 0; c < m; ++c) {
            const u64 d = __shfl(ck, c);
            const long h = __shfl(cp, c);
            bool ov = (h - rs < W) && (rs - h < W);
            for (int j = t; j < npicked; j += 64) {
                const long q = picked[j];
                ov |= (h - q < W) && (q - h < W);
            }
            if (__any(ov)) continue;
            if (2 * d > mode) {
                fill = -1;
                done = true;
                break;
            }
            picked[npicked] = (int32_t)h;
            ++npicked;
            if (npicked >= n) {
                done = true;
                break;
            }
        }
    }
    int32_t* out = idx + (long)r * n;
    for (int j = t; j < n; j += 64) out[j] = j < npicked ? picked[j] : fill;
    if (t == 0) mode_out[r] = mode;
}

static int bit_length(u64 x) {
    int b = 0;
    while (x) {
        ++b;
        x >>= 1;
    }
    return b;
}

struct SimsearchLayout {
    int64_t keys, skeys, spos, iota, temp, total;
};

static int simsearch_layout(int64_t Pg, int32_t S, int32_t W, int32_t B, SimsearchLayout& L, bool query_sort) {
    const int64_t P = Pg - W + 1;
    int64_t off = 0;
    L.keys = off;  off = align_up(off + B * P * 8, 256);
    L.skeys = off; off = align_up(off + B * P * 8, 256);
    L.spos = off;  off = align_up(off + B * P * 4, 256);
    L.iota = off;  off = align_up(off + P * 4, 256);
    L.temp = off;
    size_t tb = 0;
    if (query_sort) {
        hipError_t e = rocprim::radix_sort_pairs(nullptr, tb, (const u64*)nullptr, (u64*)nullptr, (const int32_t*)nullptr,
                                                 (int32_t*)nullptr, (size_t)P, 0, 64, (hipStream_t)0);
        if (e != hipSuccess) return fail(EPG_ERR_HIP, "simsearch: radix sort size query failed: %s", hipGetErrorString(e));
    }
    L.total = align_up(off + (int64_t)tb, 256);
    return EPG_OK;
}

static int simsearch_check(int64_t Pg, int32_t S, int32_t W, int32_t B, int32_t n) {
    if (S < 1) return fail(EPG_ERR_INVALID_ARG, "simsearch: S=%d", S);
    if (W < 1 || W > SS_MAX_W) return fail(EPG_ERR_INVALID_ARG, "simsearch: window of %d rows outside 1..%d", W, SS_MAX_W);
    if (Pg < W || Pg - W + 1 > INT32_MAX) return fail(EPG_ERR_INVALID_ARG, "simsearch: bad shape (%lld genome rows, window %d)", (long long)Pg, W);
    if (B < 1 || B > 65535 * SS_RB) return fail(EPG_ERR_INVALID_ARG, "simsearch: bad batch size %d", B);
    if (n < 1 || n > 1024) return fail(EPG_ERR_INVALID_ARG, "simsearch: n=%d outside 1..1024", n);
    if ((int64_t)(64 + W - 1) * S > SS_LDS_INTS)
        return fail(EPG_ERR_UNSUPPORTED, "simsearch: a tile of %d x %d genome values does not fit in LDS", 64 + W - 1, S);
    return EPG_OK;
}

extern "C" int64_t epg_simsearch_ws_bytes(int64_t Pg, int32_t S, int32_t W, int32_t B) {
    int rc = simsearch_check(Pg, S, W, B, 1);
    if (rc) return rc;
    SimsearchLayout L;
    rc = simsearch_layout(Pg, S, W, B, L, true);
    return rc ? rc : L.total;
}

extern "C" int epg_simsearch(const int32_t* G, int64_t Pg, int32_t S, int32_t W, const int32_t* Q, int32_t B, const int32_t* self_start,
                             int32_t n, uint64_t key_bound, void* ws, int64_t ws_bytes, int32_t* idx, uint64_t* mode, uint64_t* dist,
                             void* stream) {
    hipStream_t st = (hipStream_t)stream;
    int rc = simsearch_check(Pg, S, W, B, n);
    if (rc) return rc;
    if (key_bound >= (1ull << 53))
        return fail(EPG_ERR_UNSUPPORTED, "simsearch: distances up to %llu are not exact in fp64 (the bound is 2^53 = %llu)",
                    (unsigned long long)key_bound, 1ull << 53);
    if (!G || !Q || !self_start || !ws || !idx || !mode) return fail(EPG_ERR_INVALID_ARG, "simsearch: NULL argument");
    SimsearchLayout L;
    if ((rc = simsearch_layout(Pg, S, W, B, L, true))) return rc;
    if (ws_bytes < L.total)
        return fail(EPG_ERR_WORKSPACE, "simsearch: workspace of %lld bytes, %lld needed", (long long)ws_bytes, (long long)L.total);
    char* base = (char*)ws;
    u64* keys = (u64*)(base + L.keys);
    u64* skeys = (u64*)(base + L.skeys);
    int32_t* spos = (int32_t*)(base + L.spos);
    int32_t* iota = (int32_t*)(base + L.iota);
    const long P = (long)(Pg - W + 1);

    const dim3 grid_y(1, (unsigned)((B + SS_RB - 1) / SS_RB));
    if ((int64_t)(128 + W - 1) * S <= SS_LDS_INTS) {
        hipLaunchKernelGGL(k_simsearch_dist<128>, dim3((unsigned)((P + 127) / 128), grid_y.y), dim3(128), (size_t)(128 + W - 1) * S * 4,
                           st, G, (long)Pg, S, W,
                           Q, B, keys);
    } else {
        hipLaunchKernelGGL(k_simsearch_dist<64>, dim3((unsigned)((P + 63) / 64), grid_y.y), dim3(64), (size_t)(64 + W - 1) * S * 4,
                           st, G, (long)Pg, S, W,
                           Q, B, keys);
    }
    EPG_LAUNCH_CHECK("k_simsearch_dist");
    if (dist) EPG_HIP(hipMemcpyAsync(dist, keys, (size_t)B * P * 8, hipMemcpyDeviceToDevice, st));
    {
        long blocks = (P + 255) / 256;
        if (blocks > 4096) blocks = 4096;
        hipLaunchKernelGGL(k_simsearch_iota, dim3((unsigned)blocks), dim3(256), 0, st, iota, P);
        EPG_LAUNCH_CHECK("k_simsearch_iota");
    }
    const int bits = bit_length(key_bound) ? bit_length(key_bound) : 1;
    for (int r = 0; r < B; ++r) {
        size_t tb = (size_t)(L.total - L.temp);
        hipError_t e = rocprim::radix_sort_pairs(base + L.temp, tb, keys + (long)r * P, skeys + (long)r * P, iota, spos + (long)r * P,
                                                 (size_t)P, 0, bits, st);
        if (e != hipSuccess) return fail(EPG_ERR_HIP, "simsearch: radix sort failed: %s", hipGetErrorString(e));
    }
    hipLaunchKernelGGL(k_simsearch_select, dim3((unsigned)B), dim3(SEL_THREADS), 0, st, skeys, spos, P, self_start, W, n, idx, (u64*)mode);
    EPG_LAUNCH_CHECK("k_simsearch_select");
    return EPG_OK;
}

}  // namespace epg
