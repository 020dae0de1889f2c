// The row writer of the device text writers (epg_textout.hip: score rows, epg_metrics_text.hip: pairwiseMetrics rows), once.
// Package-internal: no entry point is declared here.
//
// A writer is a row policy `Rows`, passed to the kernels by value:
//   long R                                      the number of rows;
//   typename Rows::Row                          what a thread keeps of its row between the checks and the text;
//   Rows::FLAG_CAP                              the flag bit for "the text does not fit text_cap";
//   u32 load(long r, Row& row, int& bad) const  reads and checks row r's inputs: refused inputs set bits of `bad` (and format as
//                                               nothing or zero); -> the row's length in bytes, its newline included.  Both passes
//                                               call it; the second uses the record only, so what serves the length alone is dropped
//                                               there by the compiler;
//   void emit(long r, const Row& row, TextSink& sink) const   the row's bytes without the newline, in order, through the sink.
//
// Three launches on the caller's stream (text_rows_launch), nothing synchronises:
//   * k_text_rows_lengths  a thread per row: load(), the row's length into the workspace, `bad` OR-ed into the flag word; the tile's
//                          sum by the workgroup scan of epg_text_scan.h;
//   * k_text_tile_offsets (epg_text_scan.h)  one workgroup: the exclusive scan of the tiles' sums, the text's size into row_off[R];
//   * k_text_rows_write    a workgroup per TEXT_ROWS rows, a thread per row: the rows' offsets (the tile's offset + the workgroup scan
//                          of their lengths) into row_off, then the text.  The rows' text is put together in LDS, a window of
//                          TEXT_WIN bytes of the text at a time (256 score rows of an 18-state model are ~46 KB: two windows; 256
//                          metrics rows ~20 KB: one): the sink drops what lies outside the window, and a policy may ask it whether a
//                          field lies in front of the window, or the window behind the row's position, to skip the work.  Every
//                          window goes out by st_store_span: 16-byte stores, aligned in the text; only the up to 15 bytes at a
//                          tile's two ends, which share their 16 bytes with the neighbouring tile, are stored byte by byte.
//                          LDS: TEXT_WIN = 32 KB.
// Every byte of text lies below row_off[R] <= text_cap.
#pragma once
#include "epg_common.h"
#include "epg_text_scan.h"

namespace epg {

constexpr int TEXT_ROWS = 256;
constexpr int TEXT_WIN = 32768;

// Where a row's bytes go: the window [w0, w0 + TEXT_WIN) of the text, in LDS, and the row's position `pos` in the text.
struct TextSink {
    char* win;
    long long w0, pos;

    __device__ __forceinline__ void put_at(long long at, char c) const {
        const long long k = at - w0;
        if (k >= 0 && k < TEXT_WIN) win[k] = c;
    }
    __device__ __forceinline__ void put(char c) { put_at(pos++, c); }
    __device__ __forceinline__ void skip(long long n) { pos += n; }
    // n bytes of a blob: the window's part of them
    __device__ __forceinline__ void bytes(const char* __restrict__ src, long long n) {
        long long i0 = w0 - pos, i1 = w0 + TEXT_WIN - pos;
        if (i0 < 0) i0 = 0;
        if (i1 > n) i1 = n;
        for (long long i = i0; i < i1; ++i) win[pos + i - w0] = src[i];
        pos += n;
    }
    // v in nd decimal digits
    __device__ __forceinline__ void digits(u64 v, int nd) {
        for (int k = nd - 1; k >= 0; --k) {
            put_at(pos + k, (char)('0' + (int)(v % 10ull)));
            v /= 10ull;
        }
        pos += nd;
    }
    // the put(i, c) of epg_fmt_f5.h / epg_fmt_e5.h at the current position: sink.skip(f5_emit(bits, q, sink.at()))
    __device__ __forceinline__ auto at() const {
        const TextSink here = *this;
        return [here](int i, char c) { here.put_at(here.pos + i, c); };
    }
    // the next len bytes all lie in front of the window / the window lies behind the position: nothing more of the row is in it
    __device__ __forceinline__ bool in_front(long long len) const { return pos + len <= w0; }
    __device__ __forceinline__ bool past() const { return pos >= w0 + TEXT_WIN; }
};

template <class Rows>
__global__ __launch_bounds__(TEXT_ROWS) void k_text_rows_lengths(Rows p, u32* __restrict__ lens, u64* __restrict__ tile_sum, int* __restrict__ flags) {
    __shared__ u32 s_part[TEXT_ROWS / 64];
    const long r = (long)blockIdx.x * TEXT_ROWS + threadIdx.x;
    u32 len = 0;
    if (r < p.R) {
        typename Rows::Row row;
        int bad = 0;
        len = p.load(r, row, bad);
        lens[r] = len;
        if (bad) atomicOr(flags, bad);
    }
    u32 total;
    st_block_scan<TEXT_ROWS / 64>(len, s_part, &total);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}

template <class Rows>
__global__ __launch_bounds__(TEXT_ROWS) void k_text_rows_write(Rows p, const u32* __restrict__ lens, const u64* __restrict__ tile_off,
                                                               long long* __restrict__ row_off, char* __restrict__ text, long long text_cap,
                                                               int* __restrict__ flags) {
    __shared__ uint4 s_win4[TEXT_WIN / 16];
    __shared__ u32 s_part[TEXT_ROWS / 64];
    char* win = reinterpret_cast<char*>(s_win4);
    const int tid = threadIdx.x;
    const long R = p.R;
    const long r0 = (long)blockIdx.x * TEXT_ROWS, r1 = r0 + TEXT_ROWS < R ? r0 + TEXT_ROWS : R, r = r0 + tid;
    const u32 len = r < r1 ? lens[r] : 0u;
    u32 tile_len;
    const u32 before = st_block_scan<TEXT_ROWS / 64>(len, s_part, &tile_len);
    const long long T0 = (long long)tile_off[blockIdx.x], T1 = T0 + tile_len;
    const long long rs = T0 + before, re = rs + len;
    if (r < r1) row_off[r] = rs;
    if (row_off[R] > text_cap) {                             // (written by k_text_tile_offsets, before this kernel)
        if (blockIdx.x == 0 && tid == 0) atomicOr(flags, (int)Rows::FLAG_CAP);
        return;
    }
    typename Rows::Row row;
    if (r < r1) {
        int bad = 0;
        p.load(r, row, bad);
    }
    for (long long w0 = T0 & ~15ll; w0 < T1; w0 += TEXT_WIN) {
        const long long w1 = w0 + TEXT_WIN;
        if (r < r1 && rs < w1 && re > w0) {
            TextSink sink = {win, w0, rs};
            p.emit(r, row, sink);
            sink.put_at(re - 1, '\n');
        }
        __syncthreads();
        const long long lo = w0 > T0 ? w0 : T0, hi = w1 < T1 ? w1 : T1;
        st_store_span(s_win4, reinterpret_cast<unsigned char*>(text) + w0, (u32)(lo - w0), (u32)(hi - lo), tid, TEXT_ROWS);
        __syncthreads();
    }
}

// the workspace: lens[R] u32 | tiles[ntiles] u64
struct TextRowsLayout {
    int64_t lens, tiles, total, ntiles;
};

static inline void text_rows_layout(int64_t R, TextRowsLayout& L) {
    L.ntiles = (R + TEXT_ROWS - 1) / TEXT_ROWS;
    L.lens = 0;
    L.tiles = align_up((R > 0 ? R : 1) * 4, 256);
    L.total = L.tiles + align_up((L.ntiles > 0 ? L.ntiles : 1) * 8, 256);
}

static inline int64_t text_rows_ws_bytes(int64_t R) {
    TextRowsLayout L;
    text_rows_layout(R, L);
    return L.total;
}

// The checks every writer's entry point ends on, behind its own shape and input checks: the outputs and the workspace (`need` bytes).
static inline int text_rows_check_out(const char* name, const char* text, int64_t text_cap, const int64_t* row_off, const int32_t* flags,
                                      const void* ws, int64_t ws_bytes, int64_t need) {
    if (!text) return fail(EPG_ERR_INVALID_ARG, "%s: text is NULL", name);
    if (!row_off) return fail(EPG_ERR_INVALID_ARG, "%s: row_off is NULL", name);
    if (!flags) return fail(EPG_ERR_INVALID_ARG, "%s: flags is NULL", name);
    if (!ws) return fail(EPG_ERR_INVALID_ARG, "%s: ws is NULL", name);
    if (reinterpret_cast<uintptr_t>(text) & 255) return fail(EPG_ERR_INVALID_ARG, "%s: text is not 256-byte aligned", name);
    if (reinterpret_cast<uintptr_t>(ws) & 255) return fail(EPG_ERR_INVALID_ARG, "%s: ws is not 256-byte aligned", name);
    if (text_cap < 0) return fail(EPG_ERR_INVALID_ARG, "%s: text_cap=%lld < 0", name, (long long)text_cap);
    if (ws_bytes < need) return fail(EPG_ERR_WORKSPACE, "%s: workspace %lld < %lld bytes", name, (long long)ws_bytes, (long long)need);
    return EPG_OK;
}

// The one launch sequence.  lengths_name / write_name: what a failed launch is called in the error message.
template <class Rows>
static int text_rows_launch(const Rows& p, int64_t R, char* text, int64_t text_cap, int64_t* row_off, int32_t* flags, void* ws, hipStream_t st,
                            const char* lengths_name, const char* write_name) {
    TextRowsLayout L;
    text_rows_layout(R, L);
    char* base = static_cast<char*>(ws);
    u32* lens = reinterpret_cast<u32*>(base + L.lens);
    u64* tiles = reinterpret_cast<u64*>(base + L.tiles);
    long long* roff = reinterpret_cast<long long*>(row_off);
    EPG_HIP(hipMemsetAsync(flags, 0, sizeof(int32_t), st));
    if (L.ntiles) {
        hipLaunchKernelGGL(k_text_rows_lengths<Rows>, dim3((unsigned)L.ntiles), dim3(TEXT_ROWS), 0, st, p, lens, tiles, flags);
        EPG_LAUNCH_CHECK(lengths_name);
    }
    hipLaunchKernelGGL(k_text_tile_offsets<1024>, dim3(1), dim3(1024), 0, st, tiles, (long)L.ntiles, (long)R, roff);
    EPG_LAUNCH_CHECK("k_text_tile_offsets");
    if (L.ntiles) {
        hipLaunchKernelGGL(k_text_rows_write<Rows>, dim3((unsigned)L.ntiles), dim3(TEXT_ROWS), 0, st, p, (const u32*)lens, (const u64*)tiles, roff,
                           text, (long long)text_cap, flags);
        EPG_LAUNCH_CHECK(write_name);
    }
    return EPG_OK;
}

}  // namespace epg
