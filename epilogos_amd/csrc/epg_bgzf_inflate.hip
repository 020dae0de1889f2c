// The device BGZF reader (epg_bgzf_inflate.h): members inflated one wave each, and the newline index of the text.  gfx950 only.
//
//   * k_bgzf_inflate   a workgroup of ONE wave per member.  The phases are in epg_bgzf_inflate_block.h, which also says how a match is
//                      ordered behind the bytes it reads: the member's text is put together in LDS (a window of 64 KB, shifted so that
//                      16-byte chunks of LDS are 16-byte chunks of `out`), the payload comes through a 4 KB ring, lane 0 decodes
//                      into tokens, all lanes copy them, all lanes take the CRC-32, and the window goes out by st_store_span
//                      (epg_text_scan.h) once the trailer agrees (zeros when it does not).  LDS: ~75 KB, so two workgroups -- two
//                      waves -- per CU.
//   * k_newline_index  a wave per segment, four per workgroup: 16 bytes per lane and turn, newlines counted four at a time in a
//                      word, the wave's sum and maximum by shuffles.
// Nothing synchronises.
#include "epg_common.h"
#include "epg_bgzf_inflate.h"
#include "epg_bgzf_inflate_block.h"
#include "epg_text_scan.h"

namespace epg {

using epgbi::BI_T;

__global__ __launch_bounds__(BI_T) void k_bgzf_inflate(const unsigned char* __restrict__ comp, long long comp_bytes, const long long* __restrict__ table,
                                                       unsigned char* __restrict__ out, long long out_bytes, int* __restrict__ status,
                                                       int* __restrict__ flags) {
    extern __shared__ uint4 s_inflate4[];
    epgbi::Shared& sh = *reinterpret_cast<epgbi::Shared*>(s_inflate4);
    const int t = threadIdx.x;
    const long long m = blockIdx.x;
    const long long* row = table + m * EPGZ_TABLE_COLS;
    const long long poff = row[0], pbytes = row[1], ooff = row[2], isize = row[3], crc = row[4];
    if (poff < 0 || pbytes < 0 || pbytes > 65536 || poff > comp_bytes || pbytes > comp_bytes - poff || ooff < 0 || isize < 0 ||
        isize > EPGZ_MAX_ISIZE || ooff > out_bytes || isize > out_bytes - ooff || crc < 0 || crc > 0xffffffffll) {
        if (t == 0) {
            status[m] = epgbi::BI_E_ROW;
            atomicAdd(flags, 1);
        }
        return;
    }
    const unsigned char* payload = comp + poff;
    unsigned char* dst = out + ooff;
    epgbi::inflate_init(sh, (u32)pbytes, (u32)isize, (u32)(reinterpret_cast<uintptr_t>(dst) & 15), t);
    __syncthreads();
    const u32 turns = 8u * (u32)pbytes + (u32)isize + (u32)epgbi::BI_STEP_SLACK;      // (every turn but a refill's takes a bit or writes a byte)
    bool done = false;
    for (u32 turn = 0; turn < 2u * turns && !done; ++turn) {
        epgbi::inflate_refill(sh, payload, t);
        __syncthreads();
        if (t == 0) {
            epgbi::inflate_refilled(sh);
            epgbi::inflate_decode(sh);
        }
        __syncthreads();
        const int ntok = (int)sh.ntok;
        done = sh.state == epgbi::BI_ST_DONE;
        for (int k = 0; k < ntok; ++k) {
            epgbi::inflate_copy(sh, payload, k, t);
            __syncthreads();
        }
    }
    if (!done && t == 0) sh.status = epgbi::BI_E_BITS;
    __syncthreads();
    epgbi::inflate_crc(sh, t);
    __syncthreads();
    if (t == 0) {
        const u32 why = epgbi::inflate_finish(sh, (u32)crc);
        status[m] = (int)why;
        if (why) atomicAdd(flags, 1);
    }
    __syncthreads();
    const bool good = sh.status == epgbi::BI_OK;             // a member that was given up leaves zeros: two identical calls, identical bytes
    const u32 a = sh.a;
    st_store_span(reinterpret_cast<const uint4*>(sh.win4), dst - a, a, (u32)isize, t, BI_T, !good);
}

constexpr int NL_WAVES = 4;

__device__ __forceinline__ u32 newlines_of(u32 x, int& top) {      // bit 8 k + 7 set for every byte k of x that is '\n'
    x ^= 0x0a0a0a0au;
    const u32 z = ~((((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) | 0x7f7f7f7fu);
    top = z ? (31 - __clz((int)z)) >> 3 : -1;
    return (u32)__popc(z);
}

__global__ __launch_bounds__(64 * NL_WAVES) void k_newline_index(const unsigned char* __restrict__ text, long long n, long long seg_bytes, long long nseg,
                                                                 long long* __restrict__ count, long long* __restrict__ last) {
    const int lane = threadIdx.x & 63;
    const long long s = (long long)blockIdx.x * NL_WAVES + (threadIdx.x >> 6);
    if (s >= nseg) return;
    const long long s0 = s * seg_bytes, s1 = s0 + seg_bytes < n ? s0 + seg_bytes : n;
    long long cnt = 0, top = -1;
    for (long long p = s0 + 16ll * lane; p < s1; p += 16ll * 64) {
        if (p + 16 <= s1) {
            const uint4 v = *reinterpret_cast<const uint4*>(text + p);
            const u32 w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                int at;
                cnt += newlines_of(w[k], at);
                if (at >= 0) top = p + 4 * k + at;
            }
        } else {
            for (long long q = p; q < s1; ++q)
                if (text[q] == '\n') { ++cnt; top = q; }
        }
    }
    for (int d = 32; d >= 1; d >>= 1) {
        const long long oc = __shfl_xor(cnt, d, 64), ot = __shfl_xor(top, d, 64);
        cnt += oc;
        top = ot > top ? ot : top;
    }
    if (lane == 0) {
        count[s] = cnt;
        last[s] = top;
    }
}

// ---- entry points ----------------------------------------------------------------------------------------------------------------
extern "C" int64_t epgz_inflate_lds_bytes(void) { return (int64_t)sizeof(epgbi::Shared); }

extern "C" int epgz_bgzf_inflate(const char* comp, int64_t comp_bytes, const int64_t* table, int64_t M, char* out, int64_t out_bytes,
                                 int32_t* status, int32_t* flags, void* stream) {
    if (comp_bytes < 0 || M < 0 || out_bytes < 0)
        return fail(EPG_ERR_INVALID_ARG, "bgzf_inflate: bad shape comp_bytes=%lld M=%lld out_bytes=%lld", (long long)comp_bytes, (long long)M, (long long)out_bytes);
    if (M >= (1LL << 31)) return fail(EPG_ERR_UNSUPPORTED, "bgzf_inflate: M=%lld >= 2^31", (long long)M);
    if (comp_bytes >= (1LL << 40) || out_bytes >= (1LL << 40))
        return fail(EPG_ERR_UNSUPPORTED, "bgzf_inflate: comp_bytes=%lld or out_bytes=%lld >= 2^40", (long long)comp_bytes, (long long)out_bytes);
    if (comp_bytes > 0 && !comp) return fail(EPG_ERR_INVALID_ARG, "bgzf_inflate: comp is NULL");
    if (M > 0 && !table) return fail(EPG_ERR_INVALID_ARG, "bgzf_inflate: table is NULL");
    if (out_bytes > 0 && !out) return fail(EPG_ERR_INVALID_ARG, "bgzf_inflate: out is NULL");
    if (M > 0 && !status) return fail(EPG_ERR_INVALID_ARG, "bgzf_inflate: status is NULL");
    if (!flags) return fail(EPG_ERR_INVALID_ARG, "bgzf_inflate: flags is NULL");
    if (reinterpret_cast<uintptr_t>(table) & 7) return fail(EPG_ERR_INVALID_ARG, "bgzf_inflate: table is not 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    EPG_HIP(hipMemsetAsync(flags, 0, sizeof(int32_t), st));
    if (M) {
        static DynLds lds_attr;
        const int lds = (int)sizeof(epgbi::Shared);
        EPG_HIP(ensure_dyn_lds(lds_attr, reinterpret_cast<const void*>(k_bgzf_inflate), lds));
        hipLaunchKernelGGL(k_bgzf_inflate, dim3((unsigned)M), dim3(BI_T), lds, st, reinterpret_cast<const unsigned char*>(comp), (long long)comp_bytes,
                           reinterpret_cast<const long long*>(table), reinterpret_cast<unsigned char*>(out), (long long)out_bytes, status, flags);
        EPG_LAUNCH_CHECK("k_bgzf_inflate");
    }
    return EPG_OK;
}

extern "C" int64_t epgz_newline_segments(int64_t n, int64_t seg_bytes) {
    if (n < 0 || n >= (1LL << 40) || seg_bytes < 16 || (seg_bytes & 15) || seg_bytes > (1LL << 30)) {
        fail(EPG_ERR_INVALID_ARG, "newline_segments: bad shape n=%lld seg_bytes=%lld", (long long)n, (long long)seg_bytes);
        return -1;
    }
    return (n + seg_bytes - 1) / seg_bytes;
}

extern "C" int epgz_newline_index(const char* text, int64_t n, int64_t seg_bytes, int64_t* count, int64_t* last, void* stream) {
    if (n < 0 || seg_bytes < 16 || (seg_bytes & 15) || seg_bytes > (1LL << 30))
        return fail(EPG_ERR_INVALID_ARG, "newline_index: bad shape n=%lld seg_bytes=%lld", (long long)n, (long long)seg_bytes);
    if (n >= (1LL << 40)) return fail(EPG_ERR_UNSUPPORTED, "newline_index: n=%lld >= 2^40", (long long)n);
    if (n > 0 && !text) return fail(EPG_ERR_INVALID_ARG, "newline_index: text is NULL");
    if (n > 0 && !count) return fail(EPG_ERR_INVALID_ARG, "newline_index: count is NULL");
    if (n > 0 && !last) return fail(EPG_ERR_INVALID_ARG, "newline_index: last is NULL");
    if (reinterpret_cast<uintptr_t>(text) & 15) return fail(EPG_ERR_INVALID_ARG, "newline_index: text is not 16-byte aligned");
    if (n == 0) return EPG_OK;
    const long long nseg = (n + seg_bytes - 1) / seg_bytes;
    if (nseg >= (1LL << 31)) return fail(EPG_ERR_UNSUPPORTED, "newline_index: %lld segments >= 2^31", nseg);
    hipLaunchKernelGGL(k_newline_index, dim3((unsigned)((nseg + NL_WAVES - 1) / NL_WAVES)), dim3(64 * NL_WAVES), 0, (hipStream_t)stream,
                       reinterpret_cast<const unsigned char*>(text), (long long)n, (long long)seg_bytes, nseg, reinterpret_cast<long long*>(count),
                       reinterpret_cast<long long*>(last));
    EPG_LAUNCH_CHECK("k_newline_index");
    return EPG_OK;
}

}  // namespace epg
