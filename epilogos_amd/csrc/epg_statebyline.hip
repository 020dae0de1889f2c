// ChromHMM state-by-line calls read on the device (include/epilogos_statebyline.h): the text of one biosample's file -> a column of
// int8 states, and a batch of columns -> the [bins, biosamples] matrix.
//
// A line is 2 .. 4 bytes long, so the bin of a byte is the number of newlines before it: the index / scan / parse split of
// epg_scores_text.hip, without the position array -- a line is short enough to be read backwards from its newline.
//
//   k_sbl_count  one workgroup per segment of SBL_SEG bytes: the number of newlines of the segment.  A text whose last byte is not
//                '\n' has a virtual '\n' at position nbytes, so positions 0 .. nbytes are looked at.
//   k_sbl_scan   one workgroup: exclusive scan of the segment counts in place (st_scan_segments of epg_text_scan.h); info[]
//                initialised from the total.
//   k_sbl_parse  the same walk again.  A thread holds 16 bytes of text and the 4 before them; the newline at byte j of its 16 ends
//                line (newlines before it), and the line's 1 .. 3 digits are the bytes before j up to the previous newline: all inside
//                the thread's 20-byte window.  The lines of a workgroup are consecutive bins, so their states are staged in LDS
//                (with the destination's alignment modulo 16) and go out as 16-byte stores.
//   k_sbl_transpose  one workgroup per SBL_TILE_BINS bins of a batch of up to 64 columns.  A thread loads 16 bins of 4 columns
//                (16 lanes side by side: 256 contiguous bytes of a column), turns the 4 x 16 bytes into 16 dwords of 4 biosamples
//                in registers and stores them into an LDS image [bin][64 biosamples]; the dword slot of a bin's row is rotated
//                by (bin / 16), so that the 16 lanes that hold bins 16 apart meet 16 banks, not one (the rows are 16 dwords:
//                unrotated, every one of them would start on bank 0 or 16).  The image is read back a bin's row at a time,
//                16 lanes a row -- two rows of a half-wave lie on the two halves of the 32 banks -- and stored as dwords where X
//                allows it (col0, ldx and X multiples of 4), else by bytes: either way consecutive lanes write consecutive bytes
//                of a bin's run of nb bytes.
//
// Nothing here reads outside text[0, nbytes) and cols[nb][col_pitch], or writes outside col[0, min(rows, cap)), info[0..4), the
// workspace and the named columns of X.
#include "epg_common.h"
#include "epg_text_scan.h"
#include "epilogos_statebyline.h"

namespace epg {

static constexpr int SBL_THREADS = 256;
static constexpr int SBL_THREAD_BYTES = 16;
static constexpr int SBL_SEG = SBL_THREADS * SBL_THREAD_BYTES;   // bytes of text per workgroup
static constexpr int SBL_SCAN_THREADS = 1024;
static constexpr int SBL_TILE_BINS = 256;
static constexpr int SBL_MAX_BATCH = 64;

// The thread's window: w[] holds text[p0 - 4, p0 + 16) as 5 little-endian words (0 outside the text, '\n' at position n of a text
// that ends inside its last line).  -> bit j = position p0 + j ends a line.  Not st_byte_mask of epg_text_scan.h: the parse needs the
// four bytes before the thread's 16 in registers as well.
__device__ __forceinline__ u32 sbl_window(const char* __restrict__ text, long n, long p0, u32 w[5]) {
    if (p0 >= 4 && p0 + 16 <= n) {
        __builtin_memcpy(&w[0], text + p0 - 4, 4);
        const uint4 v = ld16(text + p0);
        w[1] = v.x, w[2] = v.y, w[3] = v.z, w[4] = v.w;
    } else {
        w[0] = w[1] = w[2] = w[3] = w[4] = 0;
#pragma unroll
        for (int i = 0; i < 20; ++i) {
            const long p = p0 - 4 + i;
            u32 c = 0;
            if (p >= 0 && p < n) c = (unsigned char)text[p];
            else if (p == n && n > 0 && text[n - 1] != '\n') c = '\n';
            w[i >> 2] |= c << (8 * (i & 3));
        }
    }
    u32 m = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j)
        if (((w[(j + 4) >> 2] >> (8 * ((j + 4) & 3))) & 0xffu) == '\n') m |= 1u << j;
    return m;
}

__global__ __launch_bounds__(SBL_THREADS) void k_sbl_count(const char* __restrict__ text, long n, u32* __restrict__ seg) {
    __shared__ u32 part[SBL_THREADS / 64];
    const long p0 = (long)blockIdx.x * SBL_SEG + (long)threadIdx.x * SBL_THREAD_BYTES;
    u32 w[5];
    const u32 m = p0 <= n ? sbl_window(text, n, p0, w) : 0;
    u32 total;
    st_block_scan<SBL_THREADS / 64>(__popc(m), part, &total);
    if (threadIdx.x == 0) seg[blockIdx.x] = total;
}

// seg[0 .. nseg): counts -> exclusive offsets; info initialised from the number of lines
__global__ __launch_bounds__(SBL_SCAN_THREADS) void k_sbl_scan(u32* __restrict__ seg, int nseg, long long* __restrict__ info) {
    __shared__ u32 part[SBL_SCAN_THREADS / 64];
    const u32 carry = st_scan_segments<SBL_SCAN_THREADS / 64>(seg, nseg, part);
    if (threadIdx.x == 0) {
        const long long rows = carry >= 2 ? (long long)carry - 2 : 0;
        info[0] = rows;
        info[1] = rows ? 128 : 0;
        info[2] = 0;
        info[3] = carry >= 2 ? -1 : (long long)carry;             // a header line is missing
    }
}

__global__ __launch_bounds__(SBL_THREADS) void k_sbl_parse(const char* __restrict__ text, long n, const u32* __restrict__ seg,
                                                           int8_t* __restrict__ col, long cap, long long* __restrict__ info) {
    __shared__ u32 part[SBL_THREADS / 64];
    __shared__ __attribute__((aligned(16))) unsigned char stage[SBL_SEG + 32];
    const int t = threadIdx.x;
    const long p0 = (long)blockIdx.x * SBL_SEG + (long)t * SBL_THREAD_BYTES;
    u32 w[5];
    const u32 m = p0 <= n ? sbl_window(text, n, p0, w) : 0;
    u32 total;
    const u32 off = st_block_scan<SBL_THREADS / 64>(__popc(m), part, &total);
    const u32 line0 = seg[blockIdx.x];                           // lines that end before this workgroup's text
    // the workgroup's bins: lines line0 .. line0 + total - 1, less the headers
    const long row_lo = (long)(line0 > 2 ? line0 : 2) - 2;
    const long row_hi = (long)(line0 + total > 2 ? line0 + total : 2) - 2;
    const int mis = (int)(reinterpret_cast<uintptr_t>(col + row_lo) & 15);   // stage[mis + i] = col[row_lo + i]

    u32 vmin = 128, vmax = 0, bad = 0xffffffffu;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        if (!((m >> j) & 1u)) continue;
        const u32 line = line0 + off + __popc(m & ((1u << j) - 1u));
        if (line < 2) continue;
        // the bytes before the newline, nearest first (byte j of the 16 is byte j + 4 of the window)
        const u32 c1 = (w[(j + 3) >> 2] >> (8 * ((j + 3) & 3))) & 0xffu;
        const u32 c2 = (w[(j + 2) >> 2] >> (8 * ((j + 2) & 3))) & 0xffu;
        const u32 c3 = (w[(j + 1) >> 2] >> (8 * ((j + 1) & 3))) & 0xffu;
        const u32 c4 = (w[j >> 2] >> (8 * (j & 3))) & 0xffu;
        const u32 d1 = c1 - '0', d2 = c2 - '0', d3 = c3 - '0';
        u32 v = 0;                                               // 0: outside the grammar
        if (d1 < 10u) {
            if (c2 == '\n') v = d1;
            else if (d2 < 10u) {
                if (c3 == '\n') v = d2 ? d2 * 10 + d1 : 0;
                else if (d3 < 10u && c4 == '\n') v = d3 ? d3 * 100 + d2 * 10 + d1 : 0;
            }
        }
        if (v > 127u) v = 0;
        if (v) {
            vmin = v < vmin ? v : vmin;
            vmax = v > vmax ? v : vmax;
        } else {
            bad = line < bad ? line : bad;
        }
        stage[mis + (int)((long)line - 2 - row_lo)] = (unsigned char)(v - 1u);      // (0 - 1 = 0xff: -1)
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const u32 a = __shfl_xor(vmin, o), b = __shfl_xor(vmax, o), c = __shfl_xor(bad, o);
        vmin = a < vmin ? a : vmin;
        vmax = b > vmax ? b : vmax;
        bad = c < bad ? c : bad;
    }
    if ((t & 63) == 0) {
        unsigned long long* u = reinterpret_cast<unsigned long long*>(info);
        if (vmin < 128u) atomicMin(u + 1, (unsigned long long)vmin);
        if (vmax > 0u) atomicMax(u + 2, (unsigned long long)vmax);
        if (bad != 0xffffffffu) atomicMin(u + 3, (unsigned long long)bad);           // (-1 is the largest unsigned)
    }
    __syncthreads();

    // stage -> col[row_lo, min(row_hi, cap)): bytes up to the first 16-byte boundary, whole vectors, bytes
    const long end = row_hi < cap ? row_hi : cap;
    if (end <= row_lo) return;
    const int len = (int)(end - row_lo);
    int8_t* dst = col + row_lo;
    int head = mis ? 16 - mis : 0;
    if (head > len) head = len;
    if (t < head) dst[t] = (int8_t)stage[mis + t];
    const int nvec = (len - head) >> 4;
    for (int v = t; v < nvec; v += SBL_THREADS)
        *reinterpret_cast<uint4*>(dst + head + 16 * v) = *reinterpret_cast<const uint4*>(stage + mis + head + 16 * v);
    for (int i = head + 16 * nvec + t; i < len; i += SBL_THREADS) dst[i] = (int8_t)stage[mis + i];
}

// byte m of a, b, c, d -> one dword (a lowest)
__device__ __forceinline__ u32 sbl_gather(u32 a, u32 b, u32 c, u32 d, int m) {
    return ((a >> (8 * m)) & 0xffu) | (((b >> (8 * m)) & 0xffu) << 8) | (((c >> (8 * m)) & 0xffu) << 16) | (((d >> (8 * m)) & 0xffu) << 24);
}

__global__ __launch_bounds__(SBL_THREADS) void k_sbl_transpose(const int8_t* __restrict__ cols, int nb, long col_pitch, long R,
                                                               int8_t* __restrict__ X, long ldx, long col0, int dwords) {
    __shared__ u32 img[SBL_TILE_BINS * 16];                      // [bin][16 dwords of 4 biosamples], the slot rotated by bin / 16
    const int t = threadIdx.x;
    const long r0 = (long)blockIdx.x * SBL_TILE_BINS;
    {
        const int jb = t & 15;                                   // which 16 bins of the tile
        const int q = t >> 4;                                    // which 4 columns of the 64
        u32 in[4][4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = 4 * q + k;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (c < nb && r0 + 16 * jb < R)                      // (col_pitch is a multiple of 16 and >= R: the 16 bytes are the column's)
                v = *reinterpret_cast<const uint4*>(cols + (long)c * col_pitch + r0 + 16 * jb);
            in[k][0] = v.x, in[k][1] = v.y, in[k][2] = v.z, in[k][3] = v.w;
        }
        const int slot = (q + jb) & 15;
#pragma unroll
        for (int i = 0; i < 16; ++i)
            img[(16 * jb + i) * 16 + slot] = sbl_gather(in[0][i >> 2], in[1][i >> 2], in[2][i >> 2], in[3][i >> 2], i & 3);
    }
    __syncthreads();
    const int k = t & 15;                                        // the dword of a bin's run: columns 4k .. 4k + 3 of the batch
    const int have = nb - 4 * k < 4 ? nb - 4 * k : 4;            // how many of them the batch holds
    if (have <= 0) return;
    for (int b = t >> 4; b < SBL_TILE_BINS; b += SBL_THREADS / 16) {
        const long r = r0 + b;
        if (r >= R) break;
        const u32 v = img[b * 16 + ((k + (b >> 4)) & 15)];
        int8_t* dst = X + r * ldx + col0 + 4 * k;
        if (dwords && have == 4) {
            *reinterpret_cast<u32*>(dst) = v;
        } else {
            for (int i = 0; i < have; ++i) dst[i] = (int8_t)(v >> (8 * i));
        }
    }
}

static int64_t sbl_seg_words(int64_t nbytes) { return nbytes / SBL_SEG + 1; }

extern "C" int64_t epg_sbl_ws_bytes(int64_t nbytes) {
    if (nbytes < 0 || nbytes > EPG_SBL_MAX_TEXT_BYTES)
        return fail(EPG_ERR_INVALID_ARG, "sbl_ws_bytes: %lld bytes outside 0..%lld", (long long)nbytes, (long long)EPG_SBL_MAX_TEXT_BYTES);
    return align_up(sbl_seg_words(nbytes) * 4, 256);
}

extern "C" int32_t epg_sbl_constant(int32_t which) {
    switch (which) {
        case EPG_SBL_THREAD_BYTES: return SBL_THREAD_BYTES;
        case EPG_SBL_BLOCK_BYTES: return SBL_SEG;
        case EPG_SBL_TILE_BINS: return SBL_TILE_BINS;
        case EPG_SBL_MAX_BATCH: return SBL_MAX_BATCH;
    }
    return -1;
}

extern "C" int epg_sbl_parse(const char* text, int64_t nbytes, int8_t* col, int64_t cap, int64_t* info, void* ws, int64_t ws_bytes,
                             void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (nbytes < 0 || nbytes > EPG_SBL_MAX_TEXT_BYTES)
        return fail(EPG_ERR_INVALID_ARG, "sbl_parse: %lld bytes outside 0..%lld", (long long)nbytes, (long long)EPG_SBL_MAX_TEXT_BYTES);
    if (cap < 0) return fail(EPG_ERR_INVALID_ARG, "sbl_parse: a column of %lld rows", (long long)cap);
    if ((nbytes > 0 && !text) || !ws || !info) return fail(EPG_ERR_INVALID_ARG, "sbl_parse: NULL argument");
    if (cap > 0 && !col) return fail(EPG_ERR_INVALID_ARG, "sbl_parse: NULL column");
    if (reinterpret_cast<uintptr_t>(ws) & 15) return fail(EPG_ERR_INVALID_ARG, "sbl_parse: the workspace is not 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(info) & 7) return fail(EPG_ERR_INVALID_ARG, "sbl_parse: info is not 8-byte aligned");
    const int64_t need = epg_sbl_ws_bytes(nbytes);
    if (ws_bytes < need) return fail(EPG_ERR_WORKSPACE, "sbl_parse: workspace of %lld bytes, %lld needed", (long long)ws_bytes, (long long)need);
    const int nseg = (int)sbl_seg_words(nbytes);
    u32* seg = reinterpret_cast<u32*>(ws);
    hipLaunchKernelGGL(k_sbl_count, dim3((unsigned)nseg), dim3(SBL_THREADS), 0, st, text, (long)nbytes, seg);
    EPG_LAUNCH_CHECK("k_sbl_count");
    hipLaunchKernelGGL(k_sbl_scan, dim3(1), dim3(SBL_SCAN_THREADS), 0, st, seg, nseg, reinterpret_cast<long long*>(info));
    EPG_LAUNCH_CHECK("k_sbl_scan");
    hipLaunchKernelGGL(k_sbl_parse, dim3((unsigned)nseg), dim3(SBL_THREADS), 0, st, text, (long)nbytes, (const u32*)seg, col, (long)cap,
                       reinterpret_cast<long long*>(info));
    EPG_LAUNCH_CHECK("k_sbl_parse");
    return EPG_OK;
}

extern "C" int epg_sbl_transpose(const int8_t* cols, int32_t nb, int64_t col_pitch, int64_t R, int8_t* X, int64_t ldx, int64_t col0,
                                 void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (nb < 0 || R < 0 || col0 < 0 || col_pitch < 0 || ldx < 0)
        return fail(EPG_ERR_INVALID_ARG, "sbl_transpose: bad shape nb=%d R=%lld col0=%lld", nb, (long long)R, (long long)col0);
    if (nb > SBL_MAX_BATCH) return fail(EPG_ERR_UNSUPPORTED, "sbl_transpose: a batch of %d columns, %d at most", nb, SBL_MAX_BATCH);
    if (R > (int64_t)SBL_TILE_BINS * 0x7fffffff) return fail(EPG_ERR_UNSUPPORTED, "sbl_transpose: %lld bins", (long long)R);
    if (nb == 0 || R == 0) return EPG_OK;
    if (col_pitch < R || (col_pitch & 15)) return fail(EPG_ERR_INVALID_ARG, "sbl_transpose: a column pitch of %lld for %lld bins (a multiple of 16, >= R)",
                                                       (long long)col_pitch, (long long)R);
    if (ldx < col0 + nb) return fail(EPG_ERR_INVALID_ARG, "sbl_transpose: columns %lld..%lld in rows of %lld", (long long)col0, (long long)(col0 + nb), (long long)ldx);
    if (!cols || !X) return fail(EPG_ERR_INVALID_ARG, "sbl_transpose: NULL argument");
    if (reinterpret_cast<uintptr_t>(cols) & 15) return fail(EPG_ERR_INVALID_ARG, "sbl_transpose: the columns are not 16-byte aligned");
    const int dwords = ((reinterpret_cast<uintptr_t>(X) | (uintptr_t)ldx | (uintptr_t)col0) & 3) == 0;
    hipLaunchKernelGGL(k_sbl_transpose, dim3((unsigned)((R + SBL_TILE_BINS - 1) / SBL_TILE_BINS)), dim3(SBL_THREADS), 0, st, cols, (int)nb,
                       (long)col_pitch, (long)R, X, (long)ldx, (long)col0, dwords);
    EPG_LAUNCH_CHECK("k_sbl_transpose");
    return EPG_OK;
}

}  // namespace epg
