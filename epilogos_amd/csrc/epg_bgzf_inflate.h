/*
 * epg_bgzf_inflate.h -- C ABI of the device BGZF reader (csrc/epg_bgzf_inflate.hip), part of libepilogos_hip.so: the members of a BGZF
 * file (scores_*.txt.gz written with EPILOGOS_BGZF=1 or --writer gpu, simsearch.bed.gz, anything bgzip wrote) inflated on the device,
 * one wave per member, so that only compressed bytes cross from the host, and the newline index the host needs to cut the inflated
 * text into chunks of whole rows without seeing it.  simsearch --inflate gpu runs them (scoresText.read_scores_device); the host
 * inflate is csrc/epg_inflate.h.
 *
 * PACKAGE-INTERNAL.  This header lives next to the kernels and not under include/: the binding tests pin the ten public headers
 * and their names (tests/test_abi_symbols.py), and every public prototype that ends in a stream has its capture case in the
 * tables of tests/test_hip_abi_contract.py / tests/test_hip_abi_streams.py.  The entry points are exported extern "C" with the
 * prefix epgz_, bound by the table _abi.READER["bgzf_inflate"] (build.READER_HEADERS), held against this header by
 * tests/test_inflate_host.py, and their stream and arena cases live in tests/test_hip_bgzf_inflate.py.  A later change that may edit
 * tests/test_abi_symbols.py should promote this header to include/epilogos_bgzf_inflate.h and its table to build.PUBLIC_HEADERS /
 * _abi.HEADERS; nothing else has to move.
 *
 * Conventions are those of include/epilogos_amd.h: plain pointers and sizes, caller-owned buffers, the stream last, every argument
 * validated before the first HIP call, EPG_OK or a negative EPG_ERR_* code with the message in epg_last_error().  The library
 * retains nothing, enqueues only on `stream` and waits for nothing.  Every output byte is written by exactly one thread and the
 * flag word by integer atomics, so two identical calls give identical bytes.  EPG_ABI_VERSION is not changed.
 */
#ifndef EPG_BGZF_INFLATE_H
#define EPG_BGZF_INFLATE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Columns of a row of the member table. */
#define EPGZ_TABLE_COLS 5
/* The largest ISIZE of a member. */
#define EPGZ_MAX_ISIZE 65536

/* Bytes of LDS a workgroup (one wave, one member) of epgz_bgzf_inflate holds: the 160 KB of a CU divided by it is the number of
 * members -- waves -- a CU works on at a time. */
int64_t epgz_inflate_lds_bytes(void);

/* The members of a BGZF stream inflated, each into its own range of `out`.
 *     comp     the compressed bytes (only the members' raw DEFLATE payloads are read)
 *     table    int64 [M, 5], a row per member: the payload's offset in comp, its bytes, the text's offset in out, ISIZE, CRC-32.
 *              The host fills it from the member chain (bgzfIndex.members); rows may come in any order and their output ranges
 *              must not overlap.  The kernel checks every row before it touches anything: the payload inside [0, comp_bytes) and
 *              of at most 65 536 bytes, the text inside [0, out_bytes), ISIZE <= 65 536, the CRC below 2^32.
 *     status   int32 [M]: 0, or why member m was given up (enum Reason of csrc/epg_bgzf_inflate_block.h):
 *                 1 BI_E_ROW             the table's row is refused
 *                 2 BI_E_BTYPE           block type 3
 *                 3 BI_E_STORED_LEN      a stored block whose LEN and NLEN disagree
 *                 4 BI_E_OVERSUBSCRIBED  an over-subscribed code
 *                 5 BI_E_INCOMPLETE      an incomplete code (other than no distance code, or the single code of one bit zlib allows)
 *                 6 BI_E_REPEAT_FIRST    repeat symbol 16 with nothing before it
 *                 7 BI_E_REPEAT_RUN      a run of lengths past HLIT + HDIST
 *                 8 BI_E_LITLEN_SYM      literal/length symbol 286 or 287
 *                 9 BI_E_DIST_SYM        distance symbol 30 or 31
 *                10 BI_E_DIST_FAR        a distance that reaches before the member's first byte
 *                11 BI_E_OUTPUT          output beyond ISIZE
 *                12 BI_E_BITS            bits past the payload
 *                13 BI_E_CRC             the CRC-32 of the text is not the trailer's
 *                14 BI_E_ISIZE           fewer bytes than ISIZE
 *                15 BI_E_CODE            bits that are no code of the block
 *                16 BI_E_HEADER          HLIT above 286, HDIST above 30, or no end-of-block code
 *                17 BI_E_TRAILING        the stream ends before the payload does
 *     flags    int32 [1], set by the call: the number of members whose status is not 0
 * A member's text is put together in LDS and stored once, after its CRC-32 (taken on the device by all threads) and its size
 * were held against the row: the bytes of `out` that belong to a member that was given up are zeros (those of a refused row,
 * reason 1, are not written).  Bytes of out outside the rows' ranges are not written.  A member with ISIZE 0 (the end-of-file
 * block, anywhere in the chain) writes nothing and has status 0 when its payload is a valid empty stream.  M = 0 is a valid
 * call: flags[0] = 0.
 * Limits: 0 <= M < 2^31, comp_bytes and out_bytes below 2^40.  comp, table, out, status and flags are device memory; table needs
 * 8-byte alignment, status and flags 4; comp and table are only read; comp and out must not overlap.
 * EPG_ERR_INVALID_ARG: comp_bytes, M or out_bytes negative; comp NULL with comp_bytes > 0; table or status NULL with M > 0; out
 * NULL with out_bytes > 0; flags NULL; table misaligned.  EPG_ERR_UNSUPPORTED: M >= 2^31, comp_bytes or out_bytes >= 2^40.
 * Order of the checks: the sizes, the unsupported sizes, the pointers in the order comp, table, out, status, flags, then the
 * alignment. */
int epgz_bgzf_inflate(const char* comp, int64_t comp_bytes, const int64_t* table, int64_t M, char* out, int64_t out_bytes,
                      int32_t* status, int32_t* flags, void* stream);

/* The number of segments of epgz_newline_index for n bytes of text: ceil(n / seg_bytes).  -1 (and a message) when n < 0, n >= 2^40,
 * seg_bytes < 16, seg_bytes is no multiple of 16 or above 2^30. */
int64_t epgz_newline_segments(int64_t n, int64_t seg_bytes);

/* For every segment s of seg_bytes bytes of text[0, n) (the last one may be shorter):
 *     count  int64 [segments]: the number of '\n' in it
 *     last   int64 [segments]: the offset in text of the last one, or -1 when there is none
 * What the host needs to cut chunks at row ends and to know every chunk's rows, without the text.  n = 0 writes nothing.
 * Limits: 0 <= n < 2^40, seg_bytes a multiple of 16 in 16 .. 2^30.  text, count and last are device memory; text is 16-byte
 * aligned and only read, count and last need 8-byte alignment.
 * EPG_ERR_INVALID_ARG: n < 0 or a bad seg_bytes; text, count or last NULL with n > 0; text misaligned.  EPG_ERR_UNSUPPORTED:
 * n >= 2^40.  Order of the checks: the sizes, the unsupported size, the pointers in the order text, count, last, then the
 * alignment. */
int epgz_newline_index(const char* text, int64_t n, int64_t seg_bytes, int64_t* count, int64_t* last, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EPG_BGZF_INFLATE_H */
