/*
 * epg_textout.h -- C ABI of the device text writer (csrc/epg_textout.hip), part of libepilogos_hip.so: the scores_*.txt.gz and
 * pairwiseDelta_*.txt.gz files formatted ("chr\tstart\tend" + "\t%.5f" per state + "\n") and compressed to BGZF on the device, so
 * that only compressed bytes cross to the host.  epilogos --writer gpu runs them; the host writer is epgio_write_scores.
 *
 * PACKAGE-INTERNAL.  This header lives next to the kernels and not under include/: the binding tests pin the ten public headers
 * and their names (tests/test_abi_symbols.py), and every public prototype that ends in a stream has its capture case in the
 * tables of tests/test_hip_abi_contract.py / tests/test_hip_abi_streams.py.  The entry points are exported extern "C" with the
 * prefix epgw_, bound by the table _abi.WRITER["textout"] (build.WRITER_HEADERS), held against this header by tests/test_writer_host.py, and their
 * stream and arena cases live in tests/test_hip_textout.py.  A later change that may edit tests/test_abi_symbols.py should promote
 * this header to include/epilogos_textout.h and its table to build.PUBLIC_HEADERS / _abi.HEADERS; nothing else has to move.
 *
 * Conventions are those of include/epilogos_amd.h: plain pointers and sizes, caller-owned buffers, the stream last, every argument
 * validated before the first HIP call, EPG_OK or a negative EPG_ERR_* code with the message in epg_last_error().  The library
 * retains nothing, enqueues only on `stream` and waits for nothing.  Every output byte is written by exactly one thread and the
 * flag words by integer atomics, so two identical calls give identical bytes.  EPG_ABI_VERSION is not changed.
 *
 * The two calls of a part and the ONE host synchronisation between them.  epgw_format_scores leaves the size of the text in device
 * memory (row_off[R]); epgw_bgzf_compress takes it as the host value n, because the number of BGZF blocks -- its grid -- follows
 * from it.  A caller that formats and then compresses therefore reads row_off[R] (and the flags) back once per part: one stream
 * synchronisation, the caller's, between the two calls.  Neither entry point synchronises.
 */
#ifndef EPG_TEXTOUT_H
#define EPG_TEXTOUT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* An upper bound of the text of R rows of S values whose locations blob holds loc_bytes bytes: every value takes at most 18 bytes
 * with its tab ("\t-2147483520.00000"), a row's location bytes are copied without their newline and the row gets its own.
 * -1 (and a message) when R < 0, S < 1, S > 4096, loc_bytes < 0 or the bound does not fit 2^62. */
int64_t epgw_text_bytes_max(int64_t R, int32_t S, int64_t loc_bytes);

/* Bytes of workspace of epgw_format_scores for R rows: the rows' lengths and the offsets of the tiles of 256 rows.  A multiple of 256.
 * -1 (and a message) when R < 0 or R >= 2^31. */
int64_t epgw_format_ws_bytes(int64_t R);

/* text = the bytes epgio_write_scores formats for float32 scores [R, S] (row r at scores + r * ld) and the rows' locations, byte
 * for byte: per row the bytes loc[loc_off[r] .. loc_off[r + 1] - 1) -- "chr\tstart\tend" without the blob's newline -- then S times a
 * tab and the value as "%.5f" (round-half-even of the exact binary value times 1e5, "-0.00000" kept for -0.0 and for negatives
 * that round to zero; csrc/epg_fmt_f5.h), then "\n".
 *     row_off  int64 [R + 1]: row r is text[row_off[r] .. row_off[r + 1]); row_off[0] = 0 and row_off[R] = the size of the text
 *     flags    int32 [1], set by the call: bit 0 = a value that is not finite or whose magnitude is >= 2^31 (it is formatted as
 *              0.00000 of its sign); bit 1 = the text does not fit text_cap (then no byte of text is written) or a row of the
 *              locations is shorter than one byte.  When flags[0] != 0 nothing of the call may be used.
 * Bytes of text behind row_off[R] are not written.
 * Limits: 0 <= R < 2^31, 1 <= S <= 4096, ld >= S.  scores, loc, loc_off, text, row_off, flags and ws are device memory; text and ws
 * are 256-byte aligned, the others need their type's alignment; ws holds ws_bytes >= epgw_format_ws_bytes(R) bytes of scratch.
 * scores, loc and loc_off are only read (with R = 0 they may be NULL, loc_off too: the text is empty).
 * EPG_ERR_INVALID_ARG: a bad shape; scores, loc, loc_off (R > 0), text, row_off, flags or ws NULL; text or ws misaligned;
 * text_cap < 0.  EPG_ERR_UNSUPPORTED: R >= 2^31.  EPG_ERR_WORKSPACE: ws_bytes too small.  Order of the checks: the shape, the
 * unsupported size, the pointers in the order scores, loc, loc_off, text, row_off, flags, ws, then alignments, then sizes. */
int epgw_format_scores(const float* scores, int64_t R, int32_t S, int64_t ld, const char* loc, const int64_t* loc_off, char* text,
                       int64_t text_cap, int64_t* row_off, int32_t* flags, void* ws, int64_t ws_bytes, void* stream);

/* Bytes that always hold the BGZF stream of n bytes of text: every block of at most 65 280 text bytes is at most a stored member
 * (18 + 5 + text + 8 bytes), plus the 28-byte end-of-file block when eof != 0.  -1 (and a message) when n < 0 or n >= 2^40. */
int64_t epgw_bgzf_bytes_max(int64_t n, int32_t eof);

/* Bytes of workspace of epgw_bgzf_compress for n bytes of text: per block its offset, its code and its threads' bit offsets.
 * A multiple of 256.  -1 (and a message) when n < 0 or n >= 2^40. */
int64_t epgw_bgzf_ws_bytes(int64_t n);

/* out = text[0 .. n) as BGZF: the text is cut every 65 280 bytes, every piece becomes one gzip member with the 'BC' extra subfield
 * (BSIZE = member size - 1), one DEFLATE block, the CRC-32 of the piece (computed on the device: a table-driven slice per thread,
 * combined by the "advance by L zero bytes" operator) and ISIZE; the members lie back to back, then the 28-byte end-of-file block
 * when eof != 0.  n = 0 gives that block alone, or nothing.
 * A piece is coded with a dynamic Huffman code built from its own histogram (code lengths <= 15) over literals and matches.  The
 * only matches looked for are "the same bytes one row earlier at the same column": distance = the length of the row above, split
 * at 258 bytes, never reaching before the piece's own start, at least 6 bytes long.  row_off (int64 [R + 1], the row offsets
 * epgw_format_scores wrote: non-decreasing, row_off[0] = 0, row_off[R] = n) says where rows start; with row_off NULL (then R = 0)
 * no match is looked for.  A piece whose rows are not in order, or whose coded size is not below its stored size, is emitted as a
 * stored block: every member is at most 65 536 bytes, and any bytes round-trip.
 *     n_out   int64 [1]: the size of the stream
 *     flags   int32 [1], set by the call: bit 0 = the stream does not fit out_cap (then out holds only the members that did fit,
 *             at their places).  epgw_bgzf_bytes_max(n, eof) always fits.
 * Bytes of out behind n_out are not written.
 * Limits: 0 <= n < 2^40, 0 <= R < 2^31.  text, row_off, out, n_out, flags and ws are device memory; out and ws are 256-byte
 * aligned; ws holds ws_bytes >= epgw_bgzf_ws_bytes(n) bytes of scratch.  text and row_off are only read; text and out must not
 * overlap.
 * EPG_ERR_INVALID_ARG: n < 0, R < 0, R > 0 without row_off; text NULL with n > 0; out, n_out, flags or ws NULL; out or ws
 * misaligned; out_cap < 0.  EPG_ERR_UNSUPPORTED: n >= 2^40 or R >= 2^31.  EPG_ERR_WORKSPACE: ws_bytes too small.  Order of the
 * checks: the shape, the unsupported sizes, the pointers in the order text, row_off, out, n_out, flags, ws, then alignments, then
 * sizes. */
int epgw_bgzf_compress(const char* text, int64_t n, const int64_t* row_off, int64_t R, int32_t eof, char* out, int64_t out_cap,
                       int64_t* n_out, int32_t* flags, void* ws, int64_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EPG_TEXTOUT_H */
