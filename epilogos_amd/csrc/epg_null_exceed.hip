// Exceedance counts of the real paired distances against a chunk of the pooled null (include/epilogos_nulldraws.h):
// exceed[b] += #{ x in chunk : |x| >= |d[b]| }.  The key of a float is the bit pattern of its absolute value -- monotone for
// floats, -0.0 and 0.0 the same key, every NaN above infinity --, so one radix sort over 31 bits puts the entries that count in
// ascending order with the left-out ones (NaN: the rows the draws kernel did not draw) behind them, and a real bin's count is the
// number of kept keys minus its lower bound among them.  A lane per real bin, two binary searches, one int64 add: no atomics.
#include "epg_common.h"
#include "epilogos_nulldraws.h"

#include <rocprim/device/device_radix_sort.hpp>

namespace epg {

constexpr u32 NX_INF = 0x7f800000u;        // keys above it are NaN

__global__ __launch_bounds__(256) void k_null_keys(const float* __restrict__ x, long n, u32* __restrict__ keys) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) keys[i] = __float_as_uint(x[i]) & 0x7fffffffu;
}

// first position in the ascending keys[0, n) whose key is >= v
__device__ __forceinline__ long nx_lower_bound(const u32* __restrict__ keys, long n, u32 v) {
    long lo = 0, hi = n;
    while (lo < hi) {
        const long mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void k_null_exceed(const u32* __restrict__ keys, long n, const float* __restrict__ d, long R,
                                                      long long* __restrict__ exceed) {
    const long b = (long)blockIdx.x * 256 + threadIdx.x;
    if (b >= R) return;
    const u32 v = __float_as_uint(d[b]) & 0x7fffffffu;
    if (v > NX_INF) return;                                      // a NaN distance counts nothing
    const long kept = nx_lower_bound(keys, n, NX_INF + 1u);
    exceed[b] += (long long)(kept - nx_lower_bound(keys, kept, v));
}

struct ExceedLayout {
    int64_t keys, sorted, temp, total;
};

static int exceed_layout(int64_t n, ExceedLayout& L) {
    L.keys = 0;
    L.sorted = align_up(n * 4, 256);
    L.temp = L.sorted + align_up(n * 4, 256);
    size_t tb = 0;
    if (n > 0) {
        hipError_t e = rocprim::radix_sort_keys(nullptr, tb, (const u32*)nullptr, (u32*)nullptr, (size_t)n, 0, 31, (hipStream_t)0);
        if (e != hipSuccess) return fail(EPG_ERR_HIP, "null_exceed: radix sort size query failed: %s", hipGetErrorString(e));
    }
    L.total = align_up(L.temp + (int64_t)tb, 256);
    return EPG_OK;
}

extern "C" int64_t epg_null_exceed_ws_bytes(int64_t n) {
    if (n < 0 || n > INT32_MAX) return fail(EPG_ERR_INVALID_ARG, "null_exceed: %lld null distances outside 0 .. 2^31 - 1", (long long)n);
    ExceedLayout L;
    const int rc = exceed_layout(n, L);
    return rc ? rc : L.total;
}

extern "C" int epg_null_exceed(const float* null, int64_t n, const float* d, int64_t R, int64_t* exceed, void* ws, int64_t ws_bytes,
                               void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (n < 0 || n > INT32_MAX || R < 0) return fail(EPG_ERR_INVALID_ARG, "null_exceed: bad shape (%lld null distances, %lld real)", (long long)n, (long long)R);
    if (n == 0 || R == 0) return EPG_OK;
    if (!null || !d || !exceed || !ws) return fail(EPG_ERR_INVALID_ARG, "null_exceed: NULL argument");
    if (reinterpret_cast<uintptr_t>(ws) & 255) return fail(EPG_ERR_INVALID_ARG, "null_exceed: the workspace must be 256-byte aligned");
    ExceedLayout L;
    int rc = exceed_layout(n, L);
    if (rc) return rc;
    if (ws_bytes < L.total) return fail(EPG_ERR_WORKSPACE, "null_exceed: workspace of %lld bytes, %lld needed", (long long)ws_bytes, (long long)L.total);
    char* base = (char*)ws;
    u32* keys = (u32*)(base + L.keys);
    u32* sorted = (u32*)(base + L.sorted);
    long blocks = (n + 255) / 256;
    if (blocks > num_cus() * 16L) blocks = num_cus() * 16L;
    hipLaunchKernelGGL(k_null_keys, dim3((unsigned)blocks), dim3(256), 0, st, null, (long)n, keys);
    EPG_LAUNCH_CHECK("k_null_keys");
    size_t tb = (size_t)(L.total - L.temp);
    hipError_t e = rocprim::radix_sort_keys(base + L.temp, tb, keys, sorted, (size_t)n, 0, 31, st);
    if (e != hipSuccess) return fail(EPG_ERR_HIP, "null_exceed: radix sort failed: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(k_null_exceed, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, st, sorted, (long)n, d, (long)R,
                       reinterpret_cast<long long*>(exceed));
    EPG_LAUNCH_CHECK("k_null_exceed");
    return EPG_OK;
}

}  // namespace epg
