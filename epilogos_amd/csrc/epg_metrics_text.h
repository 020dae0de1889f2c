/*
 * epg_metrics_text.h -- C ABI of the device metrics writer (csrc/epg_metrics_text.hip), part of libepilogos_hip.so: the rows of
 * pairwiseMetrics_*.txt.gz formatted on the device, byte for byte what epgio_write_metrics (csrc/epg_io.cpp) formats.  The text goes
 * through epgw_bgzf_compress (csrc/epg_textout.h) with the row offsets this call leaves, so that only compressed bytes cross to the
 * host.  epilogos --metrics gpu runs it; the host writer is epgio_write_metrics.
 *
 * PACKAGE-INTERNAL.  This header lives next to the kernels and not under include/: the binding tests pin the ten public headers
 * and their names (tests/test_abi_symbols.py), and every public prototype that ends in a stream has its capture case in the
 * tables of tests/test_hip_abi_contract.py / tests/test_hip_abi_streams.py.  The entry points are exported extern "C" with the
 * prefix epgm_, bound by the table _abi.METRICS["metrics_text"] (build.METRICS_HEADERS), held against this header by
 * tests/test_metrics_host.py, and their stream and arena cases live in tests/test_hip_metrics_text.py.  A later change that may edit
 * tests/test_abi_symbols.py should promote this header to include/epilogos_metrics_text.h and its table to build.PUBLIC_HEADERS /
 * _abi.HEADERS; nothing else has to move.
 *
 * Conventions are those of csrc/epg_textout.h: plain pointers and sizes, caller-owned buffers, the stream last, every argument
 * validated before the first HIP call, EPG_OK or a negative EPG_ERR_* code with the message in epg_last_error().  The library
 * retains nothing, enqueues only on `stream` and waits for nothing.  Every output byte is written by exactly one thread and the
 * flag word by integer atomics, so two identical calls give identical bytes.  EPG_ABI_VERSION is not changed.
 *
 * As with epgw_format_scores, the size of the text is left in device memory (row_off[R]); a caller that compresses reads it (and the
 * flags) back once: that synchronisation is the caller's.
 */
#ifndef EPG_METRICS_TEXT_H
#define EPG_METRICS_TEXT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Names of the two tables (chromosomes, states) longer than this many bytes are refused by the kernel (flag bits 2 and 3). */
#define EPGM_NAME_MAX 4096

/* flag bits of epgm_format_metrics */
#define EPGM_FLAG_DIST 1      /* a distance "%.5f" does not cover: not finite, or a magnitude >= 2^31 (csrc/epg_fmt_f5.h) */
#define EPGM_FLAG_PVAL 2      /* a p or adjusted p outside the "%.5e" domain: sign bit set (-0.0 too), above 1, NaN (csrc/epg_fmt_e5.h) */
#define EPGM_FLAG_STATE 4     /* a maxdiff outside 1 .. n_names, or an entry of the state table that is no name */
#define EPGM_FLAG_CHROM 8     /* a chromosome index outside 0 .. n_chrom - 1, or an entry of the chromosome table that is no name */
#define EPGM_FLAG_COORD 16    /* a negative start or end */
#define EPGM_FLAG_CAP 32      /* the text does not fit text_cap: no byte of text is written */

/* An upper bound of the text of R rows whose chromosome names hold at most chrom_max bytes and whose state names at most name_max:
 * a row is name TAB start TAB end TAB name TAB %.5f TAB sign [TAB %.5e TAB %.5e] NEWLINE with at most 19 digits a coordinate,
 * 16 bytes the distance and 12 a p-value.  -1 (and a message) when R < 0, R >= 2^31, chrom_max or name_max is outside
 * 0 .. EPGM_NAME_MAX. */
int64_t epgm_text_bytes_max(int64_t R, int64_t chrom_max, int64_t name_max, int32_t with_p);

/* Bytes of workspace of epgm_format_metrics for R rows: the rows' lengths and the offsets of the tiles of 256 rows.  A multiple of
 * 256.  -1 (and a message) when R < 0 or R >= 2^31. */
int64_t epgm_format_ws_bytes(int64_t R);

/* text = the bytes epgio_write_metrics formats for R rows, byte for byte.  Row r is
 *     chrom[chrom_off[c] .. chrom_off[c + 1])  with c = chrom_idx[r]
 *     TAB start[r] TAB end[r]                  as "%lld"
 *     TAB names[names_off[s] .. names_off[s + 1])  with s = maxdiff[r] - 1
 *     TAB |dist[r]| as "%.5f"                  (the float32 through csrc/epg_fmt_f5.h, the sign dropped: -0.0 prints 0.00000)
 *     TAB '+' when dist[r] >= 0, else '-'      (-0.0 is '+')
 *     TAB pvals[r] TAB mh[r] as "%.5e"         only when pvals and mh are given (both or neither; csrc/epg_fmt_e5.h)
 *     NEWLINE
 *     row_off  int64 [R + 1]: row r is text[row_off[r] .. row_off[r + 1]); row_off[0] = 0 and row_off[R] = the size of the text
 *     flags    int32 [1], set by the call: the OR of the EPGM_FLAG_* bits above.  A refused field is formatted as nothing (a name)
 *              or as zero (a number).  When flags[0] != 0 nothing of the call may be used.
 * Bytes of text behind row_off[R] are not written.  With R = 0 the text is empty and the row arrays may be NULL.
 * Limits: 0 <= R < 2^31, 0 <= n_chrom, n_names < 2^31, 0 <= chrom_bytes, names_bytes.  Every pointer is device memory; chrom and
 * names are the tables' blobs of chrom_bytes and names_bytes bytes, chrom_off int64 [n_chrom + 1] and names_off int64 [n_names + 1]
 * their offsets (an entry that is not inside its blob, not in order or longer than EPGM_NAME_MAX sets the table's flag for the rows
 * that name it); chrom_idx and maxdiff int32 [R], start and end int64 [R], dist float32 [R], pvals and mh float64 [R].  text and ws
 * are 256-byte aligned, the others need their type's alignment; ws holds ws_bytes >= epgm_format_ws_bytes(R) bytes of scratch.
 * Everything but text, row_off, flags and ws is only read.
 * EPG_ERR_INVALID_ARG: a bad shape; with R > 0 one of chrom, chrom_off, chrom_idx, start, end, names, names_off, maxdiff, dist
 * NULL; one of pvals and mh without the other; text, row_off, flags or ws NULL; text or ws misaligned; text_cap < 0.
 * EPG_ERR_UNSUPPORTED: R >= 2^31.  EPG_ERR_WORKSPACE: ws_bytes too small.  Order of the checks: the shape, the unsupported size,
 * the pointers in the order chrom, chrom_off, chrom_idx, start, end, names, names_off, maxdiff, dist, pvals with mh, text, row_off,
 * flags, ws, then alignments, then sizes. */
int epgm_format_metrics(const char* chrom, const int64_t* chrom_off, int32_t n_chrom, int64_t chrom_bytes, const int32_t* chrom_idx,
                        const int64_t* start, const int64_t* end, const char* names, const int64_t* names_off, int32_t n_names,
                        int64_t names_bytes, const int32_t* maxdiff, const float* dist, const double* pvals, const double* mh, int64_t R,
                        char* text, int64_t text_cap, int64_t* row_off, int32_t* flags, void* ws, int64_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EPG_METRICS_TEXT_H */
