// The device text writer (epg_textout.h): score text and its BGZF compression.  gfx950 only.
//
// Format, three launches on the caller's stream:
//   * k_tw_lengths   a thread per row: the row's length from its location bytes and its values' digit counts (epg_fmt_f5.h: integer
//                    arithmetic only), refused values and bad locations OR-ed into the flag word; the tile's sum by the workgroup
//                    scan of epg_text_scan.h;
//   * k_text_tile_offsets (epg_text_scan.h)  one workgroup: the exclusive scan of the tiles' sums, the text's size into row_off[R];
//   * k_tw_write     a workgroup per TW_ROWS rows, a thread per row: the rows' offsets (the tile's offset + the workgroup scan of
//                    their lengths) into row_off, then the text.  The rows' text is put together in LDS, a window of TW_WIN bytes
//                    of the text at a time (a tile of 256 rows of an 18-state model is ~46 KB: two windows; a thread skips the
//                    fields that lie outside the window), and every window goes out in 16-byte stores, aligned in the text: only the
//                    up to 15 bytes at a tile's two ends, which share their 16 bytes with the neighbouring tile, are stored byte by
//                    byte.  LDS: TW_WIN = 32 KB.
// Compress, three launches (the phases are in epg_bgzf_block.h, which also says what is matched):
//   * k_bgzf_plan    a workgroup per block of 65 280 text bytes: histogram walk + CRC-32, one thread builds the code and the block
//                    header, second walk for the threads' bit counts, workgroup scan (epg_text_scan.h), the block's record (size,
//                    code, header bits, bit offsets: 2.3 KB) into the workspace.  LDS: ~9 KB.
//   * k_bgzf_offsets one workgroup: the exclusive scan of the blocks' sizes, the stream's size into n_out.
//   * k_bgzf_emit    a workgroup per block (and one for the end-of-file block): the member is put together in 64 KB of zeroed LDS
//                    -- header, DEFLATE bits by atomic OR at the recorded bit offsets (third walk) or the stored bytes, CRC-32 and
//                    ISIZE -- shifted so that 16-byte chunks of LDS are 16-byte chunks of `out`, and stored as the text is.
//                    LDS: 64 KB + 1 KB, two workgroups per CU.
// Nothing synchronises: the text's size reaches epgw_bgzf_compress as the host value n, see the header.
#include "epg_common.h"
#include "epg_textout.h"
#include "epg_text_scan.h"
#include "epg_fmt_f5.h"
#include "epg_bgzf_block.h"

namespace epg {

constexpr int TW_ROWS = 256;
constexpr int TW_WIN = 32768;

__global__ __launch_bounds__(TW_ROWS) void k_tw_lengths(const float* __restrict__ scores, long R, int S, long ld, const long long* __restrict__ loc_off,
                                                        u32* __restrict__ lens, u64* __restrict__ tile_sum, int* __restrict__ flags) {
    __shared__ u32 s_part[TW_ROWS / 64];
    const long r = (long)blockIdx.x * TW_ROWS + threadIdx.x;
    u32 len = 0;
    if (r < R) {
        long long L = loc_off[r + 1] - loc_off[r] - 1;
        int bad = 0;
        if (L < 0 || L > (1 << 20)) { L = 0; bad = 2; }      // (a location of a megabyte is no location: the tile's sum stays 32 bits)
        const float* row = scores + r * ld;
        for (int s = 0; s < S; ++s) {
            const u32 bits = __float_as_uint(row[s]);
            uint64_t q;
            if (!epgfmt::f5_scale(bits, &q)) bad |= 1;
            L += 1 + epgfmt::f5_len(bits, q);
        }
        len = (u32)(L + 1);
        lens[r] = len;
        if (bad) atomicOr(flags, bad);
    }
    u32 total;
    st_block_scan<TW_ROWS / 64>(len, s_part, &total);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}

__global__ __launch_bounds__(TW_ROWS) void k_tw_write(const float* __restrict__ scores, long R, int S, long ld, const char* __restrict__ loc,
                                                      const long long* __restrict__ loc_off, const u32* __restrict__ lens, const u64* __restrict__ tile_off,
                                                      long long* __restrict__ row_off, char* __restrict__ text, long long text_cap, int* __restrict__ flags) {
    __shared__ uint4 s_win4[TW_WIN / 16];
    __shared__ u32 s_part[TW_ROWS / 64];
    char* win = reinterpret_cast<char*>(s_win4);
    const int tid = threadIdx.x;
    const long r0 = (long)blockIdx.x * TW_ROWS, r1 = r0 + TW_ROWS < R ? r0 + TW_ROWS : R, r = r0 + tid;
    const u32 len = r < r1 ? lens[r] : 0u;
    u32 tile_len;
    const u32 before = st_block_scan<TW_ROWS / 64>(len, s_part, &tile_len);
    const long long T0 = (long long)tile_off[blockIdx.x], T1 = T0 + tile_len;
    const long long rs = T0 + before, re = rs + len;
    if (r < r1) row_off[r] = rs;
    if (row_off[R] > text_cap) {                             // (written by k_text_tile_offsets, before this kernel)
        if (blockIdx.x == 0 && tid == 0) atomicOr(flags, 2);
        return;
    }
    long long lo0 = 0, llen = 0;
    if (r < r1) {
        lo0 = loc_off[r];
        llen = loc_off[r + 1] - lo0 - 1;
        if (llen < 0 || llen > (1 << 20)) llen = 0;
    }
    for (long long w0 = T0 & ~15ll; w0 < T1; w0 += TW_WIN) {
        const long long w1 = w0 + TW_WIN;
        if (r < r1 && rs < w1 && re > w0) {
            auto put = [&](long long at, char c) {
                const long long k = at - w0;
                if (k >= 0 && k < TW_WIN) win[k] = c;
            };
            long long i0 = w0 - rs, i1 = w1 - rs;
            if (i0 < 0) i0 = 0;
            if (i1 > llen) i1 = llen;
            for (long long i = i0; i < i1; ++i) win[rs + i - w0] = loc[lo0 + i];
            long long pos = rs + llen;
            const float* row = scores + r * ld;
            for (int s = 0; s < S && pos < w1; ++s) {
                const u32 bits = __float_as_uint(row[s]);
                uint64_t q;
                epgfmt::f5_scale(bits, &q);
                const int L = 1 + epgfmt::f5_len(bits, q);
                if (pos + L > w0) {
                    put(pos, '\t');
                    const long long at = pos + 1;
                    epgfmt::f5_emit(bits, q, [&](int i, char c) { put(at + i, c); });
                }
                pos += L;
            }
            put(re - 1, '\n');
        }
        __syncthreads();
        const long long lo = w0 > T0 ? w0 : T0, hi = w1 < T1 ? w1 : T1;
        for (int c = tid; c < TW_WIN / 16; c += TW_ROWS) {
            const long long g = w0 + 16ll * c;
            if (g >= hi || g + 16 <= lo) continue;
            if (g >= lo && g + 16 <= hi) {
                *reinterpret_cast<uint4*>(text + g) = s_win4[c];
            } else {
                for (int j = 0; j < 16; ++j)
                    if (g + j >= lo && g + j < hi) text[g + j] = win[16 * c + j];
            }
        }
        __syncthreads();
    }
}

// ---- BGZF ----------------------------------------------------------------------------------------------------------------------------
using epgbg::BG_T;
using epgbg::BG_TEXT;
constexpr int BG_STAGE = 65536 + 64;
constexpr int BG_SCAN_THREADS = 1024;

__global__ __launch_bounds__(BG_T) void k_bgzf_plan(const unsigned char* __restrict__ text, long long n, const long long* __restrict__ row_off, long long R,
                                                    epgbg::Rec* __restrict__ recs) {
    __shared__ epgbg::Shared sh;
    __shared__ u32 s_part[BG_T / 64];
    const int t = threadIdx.x;
    const long long B0 = (long long)blockIdx.x * BG_TEXT, B1 = B0 + BG_TEXT < n ? B0 + BG_TEXT : n;
    const epgbg::Rows rw = epgbg::make_rows(row_off, R, n);
    epgbg::Rec& rec = recs[blockIdx.x];
    epgbg::plan_init(sh, t);
    __syncthreads();
    if (t == 0) epgbg::plan_rows(sh, rw, B0, B1);
    __syncthreads();
    epgbg::plan_hist(sh, text, rw, B0, B1, t);
    __syncthreads();
    if (t == 0) {
        sh.hist[256] += 1;                                  // the end-of-block symbol
        epgbg::build_block_code(sh);
    }
    __syncthreads();
    u32 total;
    const u32 before = st_block_scan<BG_T / 64>(epgbg::plan_bits(sh, text, rw, B0, B1, t), s_part, &total);
    rec.tbits[t] = sh.hdr_bits + before;
    for (int i = t; i < epgbg::BG_NSYM; i += BG_T) {
        rec.code[i] = sh.code[i];
        rec.len[i] = sh.len[i];
    }
    for (int i = t; i < epgbg::BG_HDR_WORDS; i += BG_T) rec.hdr[i] = sh.hdr[i];
    if (t == 0) epgbg::plan_finish(sh, rec, total, B0, B1);
}

__global__ __launch_bounds__(BG_SCAN_THREADS) void k_bgzf_offsets(const epgbg::Rec* __restrict__ recs, long nblocks, int eof, long long* __restrict__ blk_off,
                                                                  long long* __restrict__ n_out) {
    __shared__ long long s_sum[BG_SCAN_THREADS];
    const int tid = threadIdx.x;
    const long chunk = (nblocks + BG_SCAN_THREADS - 1) / BG_SCAN_THREADS;
    const long lo = tid * chunk < nblocks ? tid * chunk : nblocks, hi = lo + chunk < nblocks ? lo + chunk : nblocks;
    long long sum = 0;
    for (long b = lo; b < hi; ++b) sum += recs[b].size;
    s_sum[tid] = sum;
    __syncthreads();
    long long run = 0;
    for (int k = 0; k < tid; ++k) run += s_sum[k];
    for (long b = lo; b < hi; ++b) {
        blk_off[b] = run;
        run += recs[b].size;
    }
    if (tid == BG_SCAN_THREADS - 1) {
        blk_off[nblocks] = run;
        n_out[0] = run + (eof ? 28 : 0);
    }
}

__global__ __launch_bounds__(BG_T) void k_bgzf_emit(const unsigned char* __restrict__ text, long long n, const long long* __restrict__ row_off, long long R,
                                                    const epgbg::Rec* __restrict__ recs, const long long* __restrict__ blk_off, long nblocks,
                                                    unsigned char* __restrict__ out, long long out_cap, int* __restrict__ flags) {
    extern __shared__ uint4 s_stage4[];
    __shared__ u16 s_code[epgbg::BG_NSYM];
    __shared__ unsigned char s_len[epgbg::BG_NSYM];
    const int t = threadIdx.x;
    if ((long)blockIdx.x == nblocks) {                       // the end-of-file block
        const unsigned char eof_block[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        const long long at = blk_off[nblocks];
        if (at + 28 > out_cap) {
            if (t == 0) atomicOr(flags, 1);
        } else if (t < 28) {
            out[at + t] = eof_block[t];
        }
        return;
    }
    const epgbg::Rec& rec = recs[blockIdx.x];
    const long long at = blk_off[blockIdx.x];
    const u32 size = rec.size;
    if (at + size > out_cap) {
        if (t == 0) atomicOr(flags, 1);
        return;
    }
    const long long B0 = (long long)blockIdx.x * BG_TEXT, B1 = B0 + BG_TEXT < n ? B0 + BG_TEXT : n;
    const u32 a = (u32)(at & 15);
    u32* words = reinterpret_cast<u32*>(s_stage4);
    unsigned char* bytes = reinterpret_cast<unsigned char*>(s_stage4);
    const int nchunks = (int)((a + size + 15u) >> 4);
    for (int c = t; c < nchunks + 1; c += BG_T) s_stage4[c] = make_uint4(0, 0, 0, 0);
    for (int i = t; i < epgbg::BG_NSYM; i += BG_T) {
        s_code[i] = rec.code[i];
        s_len[i] = rec.len[i];
    }
    __syncthreads();
    epgbg::emit_frame(words, a, rec, t);
    const bool stored = rec.stored != 0;
    if (stored) {
        __syncthreads();                                    // the frame's atomics are done before bytes of the same words are stored
        for (u32 i = t; i < rec.n_text; i += BG_T) bytes[a + 23u + i] = text[B0 + i];
    } else {
        const epgbg::Rows rw = epgbg::make_rows(row_off, R, n);
        epgbg::emit_tokens(words, a, rec, s_code, s_len, text, rw, B0, B1, t);
    }
    __syncthreads();
    unsigned char* base = out + (at - a);
    for (int c = t; c < nchunks; c += BG_T) {
        const u32 lo = 16u * c;
        if (lo >= a && lo + 16u <= a + size) {
            *reinterpret_cast<uint4*>(base + lo) = s_stage4[c];
        } else {
            for (u32 j = 0; j < 16; ++j)
                if (lo + j >= a && lo + j < a + size) base[lo + j] = bytes[lo + j];
        }
    }
}

// ---- entry points ----------------------------------------------------------------------------------------------------------------
struct TwLayout {
    int64_t lens, tiles, total, ntiles;
};

static void tw_layout(int64_t R, TwLayout& L) {
    L.ntiles = (R + TW_ROWS - 1) / TW_ROWS;
    L.lens = 0;
    L.tiles = align_up((R > 0 ? R : 1) * 4, 256);
    L.total = L.tiles + align_up((L.ntiles > 0 ? L.ntiles : 1) * 8, 256);
}

static int64_t bg_blocks(int64_t n) { return (n + BG_TEXT - 1) / BG_TEXT; }
static int64_t bg_recs_at(int64_t nblocks) { return align_up((nblocks + 1) * 8, 256); }

extern "C" int64_t epgw_text_bytes_max(int64_t R, int32_t S, int64_t loc_bytes) {
    if (R < 0 || S < 1 || S > 4096 || loc_bytes < 0 || R >= (1LL << 31) || loc_bytes >= (1LL << 61)) {
        fail(EPG_ERR_INVALID_ARG, "text_bytes_max: bad shape R=%lld S=%d loc_bytes=%lld", (long long)R, S, (long long)loc_bytes);
        return -1;
    }
    return loc_bytes + R * 18 * (int64_t)S;
}

extern "C" int64_t epgw_format_ws_bytes(int64_t R) {
    if (R < 0 || R >= (1LL << 31)) {
        fail(EPG_ERR_INVALID_ARG, "format_ws_bytes: bad shape R=%lld", (long long)R);
        return -1;
    }
    TwLayout L;
    tw_layout(R, L);
    return L.total;
}

extern "C" int epgw_format_scores(const float* scores, int64_t R, int32_t S, int64_t ld, const char* loc, const int64_t* loc_off, char* text,
                                  int64_t text_cap, int64_t* row_off, int32_t* flags, void* ws, int64_t ws_bytes, void* stream) {
    if (R < 0 || S < 1 || S > 4096 || ld < S) return fail(EPG_ERR_INVALID_ARG, "format_scores: bad shape R=%lld S=%d ld=%lld", (long long)R, S, (long long)ld);
    if (R >= (1LL << 31)) return fail(EPG_ERR_UNSUPPORTED, "format_scores: R=%lld >= 2^31", (long long)R);
    if (R > 0 && !scores) return fail(EPG_ERR_INVALID_ARG, "format_scores: scores is NULL");
    if (R > 0 && !loc) return fail(EPG_ERR_INVALID_ARG, "format_scores: loc is NULL");
    if (R > 0 && !loc_off) return fail(EPG_ERR_INVALID_ARG, "format_scores: loc_off is NULL");
    if (!text) return fail(EPG_ERR_INVALID_ARG, "format_scores: text is NULL");
    if (!row_off) return fail(EPG_ERR_INVALID_ARG, "format_scores: row_off is NULL");
    if (!flags) return fail(EPG_ERR_INVALID_ARG, "format_scores: flags is NULL");
    if (!ws) return fail(EPG_ERR_INVALID_ARG, "format_scores: ws is NULL");
    if (reinterpret_cast<uintptr_t>(text) & 255) return fail(EPG_ERR_INVALID_ARG, "format_scores: text is not 256-byte aligned");
    if (reinterpret_cast<uintptr_t>(ws) & 255) return fail(EPG_ERR_INVALID_ARG, "format_scores: ws is not 256-byte aligned");
    if (text_cap < 0) return fail(EPG_ERR_INVALID_ARG, "format_scores: text_cap=%lld < 0", (long long)text_cap);
    TwLayout L;
    tw_layout(R, L);
    if (ws_bytes < L.total) return fail(EPG_ERR_WORKSPACE, "format_scores: workspace %lld < %lld bytes", (long long)ws_bytes, (long long)L.total);
    hipStream_t st = (hipStream_t)stream;
    char* base = static_cast<char*>(ws);
    u32* lens = reinterpret_cast<u32*>(base + L.lens);
    u64* tiles = reinterpret_cast<u64*>(base + L.tiles);
    long long* roff = reinterpret_cast<long long*>(row_off);
    const long long* loff = reinterpret_cast<const long long*>(loc_off);
    EPG_HIP(hipMemsetAsync(flags, 0, sizeof(int32_t), st));
    if (L.ntiles) {
        hipLaunchKernelGGL(k_tw_lengths, dim3((unsigned)L.ntiles), dim3(TW_ROWS), 0, st, scores, (long)R, (int)S, (long)ld, loff, lens, tiles, flags);
        EPG_LAUNCH_CHECK("k_tw_lengths");
    }
    hipLaunchKernelGGL(k_text_tile_offsets<1024>, dim3(1), dim3(1024), 0, st, tiles, (long)L.ntiles, (long)R, roff);
    EPG_LAUNCH_CHECK("k_text_tile_offsets");
    if (L.ntiles) {
        hipLaunchKernelGGL(k_tw_write, dim3((unsigned)L.ntiles), dim3(TW_ROWS), 0, st, scores, (long)R, (int)S, (long)ld, loc, loff, (const u32*)lens,
                           (const u64*)tiles, roff, text, (long long)text_cap, flags);
        EPG_LAUNCH_CHECK("k_tw_write");
    }
    return EPG_OK;
}

extern "C" int64_t epgw_bgzf_bytes_max(int64_t n, int32_t eof) {
    if (n < 0 || n >= (1LL << 40)) {
        fail(EPG_ERR_INVALID_ARG, "bgzf_bytes_max: bad size n=%lld", (long long)n);
        return -1;
    }
    return n + bg_blocks(n) * (epgbg::BG_MEMBER_EXTRA + 5) + (eof ? 28 : 0);
}

extern "C" int64_t epgw_bgzf_ws_bytes(int64_t n) {
    if (n < 0 || n >= (1LL << 40)) {
        fail(EPG_ERR_INVALID_ARG, "bgzf_ws_bytes: bad size n=%lld", (long long)n);
        return -1;
    }
    const int64_t nb = bg_blocks(n);
    return align_up(bg_recs_at(nb) + nb * (int64_t)sizeof(epgbg::Rec), 256);
}

extern "C" int epgw_bgzf_compress(const char* text, int64_t n, const int64_t* row_off, int64_t R, int32_t eof, char* out, int64_t out_cap,
                                  int64_t* n_out, int32_t* flags, void* ws, int64_t ws_bytes, void* stream) {
    if (n < 0 || R < 0) return fail(EPG_ERR_INVALID_ARG, "bgzf_compress: bad shape n=%lld R=%lld", (long long)n, (long long)R);
    if (n >= (1LL << 40)) return fail(EPG_ERR_UNSUPPORTED, "bgzf_compress: n=%lld >= 2^40", (long long)n);
    if (R >= (1LL << 31)) return fail(EPG_ERR_UNSUPPORTED, "bgzf_compress: R=%lld >= 2^31", (long long)R);
    if (n > 0 && !text) return fail(EPG_ERR_INVALID_ARG, "bgzf_compress: text is NULL");
    if (R > 0 && !row_off) return fail(EPG_ERR_INVALID_ARG, "bgzf_compress: row_off is NULL");
    if (!out) return fail(EPG_ERR_INVALID_ARG, "bgzf_compress: out is NULL");
    if (!n_out) return fail(EPG_ERR_INVALID_ARG, "bgzf_compress: n_out is NULL");
    if (!flags) return fail(EPG_ERR_INVALID_ARG, "bgzf_compress: flags is NULL");
    if (!ws) return fail(EPG_ERR_INVALID_ARG, "bgzf_compress: ws is NULL");
    if (reinterpret_cast<uintptr_t>(out) & 255) return fail(EPG_ERR_INVALID_ARG, "bgzf_compress: out is not 256-byte aligned");
    if (reinterpret_cast<uintptr_t>(ws) & 255) return fail(EPG_ERR_INVALID_ARG, "bgzf_compress: ws is not 256-byte aligned");
    if (out_cap < 0) return fail(EPG_ERR_INVALID_ARG, "bgzf_compress: out_cap=%lld < 0", (long long)out_cap);
    const int64_t nb = bg_blocks(n);
    const int64_t need = align_up(bg_recs_at(nb) + nb * (int64_t)sizeof(epgbg::Rec), 256);
    if (ws_bytes < need) return fail(EPG_ERR_WORKSPACE, "bgzf_compress: workspace %lld < %lld bytes", (long long)ws_bytes, (long long)need);
    hipStream_t st = (hipStream_t)stream;
    char* base = static_cast<char*>(ws);
    long long* blk_off = reinterpret_cast<long long*>(base);
    epgbg::Rec* recs = reinterpret_cast<epgbg::Rec*>(base + bg_recs_at(nb));
    const unsigned char* txt = reinterpret_cast<const unsigned char*>(text);
    const long long* roff = reinterpret_cast<const long long*>(row_off);
    EPG_HIP(hipMemsetAsync(flags, 0, sizeof(int32_t), st));
    if (nb) {
        hipLaunchKernelGGL(k_bgzf_plan, dim3((unsigned)nb), dim3(BG_T), 0, st, txt, (long long)n, roff, (long long)R, recs);
        EPG_LAUNCH_CHECK("k_bgzf_plan");
    }
    hipLaunchKernelGGL(k_bgzf_offsets, dim3(1), dim3(BG_SCAN_THREADS), 0, st, (const epgbg::Rec*)recs, (long)nb, (int)eof, blk_off,
                       reinterpret_cast<long long*>(n_out));
    EPG_LAUNCH_CHECK("k_bgzf_offsets");
    const unsigned grid = (unsigned)(nb + (eof ? 1 : 0));
    if (grid) {
        static DynLds lds_attr;
        EPG_HIP(ensure_dyn_lds(lds_attr, reinterpret_cast<const void*>(k_bgzf_emit), BG_STAGE));
        hipLaunchKernelGGL(k_bgzf_emit, dim3(grid), dim3(BG_T), BG_STAGE, st, txt, (long long)n, roff, (long long)R, (const epgbg::Rec*)recs,
                           (const long long*)blk_off, (long)nb, reinterpret_cast<unsigned char*>(out), (long long)out_cap, flags);
        EPG_LAUNCH_CHECK("k_bgzf_emit");
    }
    return EPG_OK;
}

}  // namespace epg
