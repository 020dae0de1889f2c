/*
 * epilogos_statebyline.h -- C ABI of the GPU reader of ChromHMM state-by-line calls (csrc/epg_statebyline.hip), part of
 * libepilogos_hip.so, and the layout of the binary matrix file the preprocessing command writes from them.
 *
 * ChromHMM -printstatebyline writes one file per biosample and chromosome: two header lines, then one state per 200 bp bin.
 * epg_sbl_parse turns the text of one file into a column of int8 states; epg_sbl_transpose puts a batch of columns into the
 * [bins, biosamples] matrix the count kernels stream (epilogos_amd.h).  Python: epilogos_amd/stateByLine.py.
 *
 * Conventions are those of epilogos_amd.h: plain pointers and sizes, caller-owned device buffers, the stream last, every argument
 * validated before the first HIP call, EPG_OK or a negative EPG_ERR_* code with the message in epg_last_error().  No call
 * allocates or synchronises.
 *
 * Strict grammar of a state-by-line text.  Lines are ended by '\n'; the '\n' of the last line may be missing.
 *   lines 0 and 1  headers: any bytes
 *   line 2 + r     the state of bin r: 1 .. 3 ASCII digits, the first not '0', value 1 .. 127
 * Nothing else: no '\r', blank, sign or empty line.  A text with fewer than two lines is outside the grammar at the first
 * line that is missing.  Values above the model's state count are the caller's business (the parser keeps 1 .. 127).
 *
 * The binary matrix file, matrix_<chromosome>.epgm: a 128-byte header, little-endian, then R x N int8 states, 0-based, row-major
 * with a row pitch of N bytes (no padding).  Coordinates are not stored: row i is <chromosome> TAB i*width TAB (i+1)*width.
 *   offset  0  char[8]   "EPGM1" and three NUL bytes
 *           8  int64     R, the number of bins
 *          16  int64     N, the number of biosamples
 *          24  int64     the row pitch in bytes (= N)
 *          32  int32     the bin width in bp (200)
 *          36  int32     the lowest state of the matrix as written in the calls (1-based; 0 when R * N == 0)
 *          40  int32     the highest
 *          44  int32     0
 *          48  char[80]  the chromosome name, NUL-padded (79 bytes at most)
 */
#ifndef EPILOGOS_STATEBYLINE_H
#define EPILOGOS_STATEBYLINE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Largest text, and the bytes of workspace a text of nbytes needs (< 0: nbytes outside 0 .. EPG_SBL_MAX_TEXT_BYTES). */
#define EPG_SBL_MAX_TEXT_BYTES 0x7fff0000
int64_t epg_sbl_ws_bytes(int64_t nbytes);

/* The kernels' tile constants, for callers that size batches and tests that aim at the boundaries:
 *   EPG_SBL_THREAD_BYTES  bytes of text per thread of the parser
 *   EPG_SBL_BLOCK_BYTES   bytes of text per workgroup of the parser
 *   EPG_SBL_TILE_BINS     bins per workgroup of the transpose
 *   EPG_SBL_MAX_BATCH     the most columns one epg_sbl_transpose takes
 * -1 for any other `which`. */
#define EPG_SBL_THREAD_BYTES 0
#define EPG_SBL_BLOCK_BYTES 1
#define EPG_SBL_TILE_BINS 2
#define EPG_SBL_MAX_BATCH 3
int32_t epg_sbl_constant(int32_t which);

/* Parse text[0, nbytes) (device memory, any alignment), the whole text of one state-by-line file:
 *   col   int8 [cap]   col[r] = state of bin r minus 1, for r < min(rows, cap); -1 where line 2 + r is outside the grammar.
 *                      Nothing behind min(rows, cap) is written.  May be NULL when cap == 0.
 *   info  int64 [4]    written, not accumulated:
 *                      [0] rows: the number of lines minus the two headers (0 when there are fewer)
 *                      [1] the lowest and [2] the highest state as written (1-based) over the lines of the grammar; 128 and 0 when
 *                          there is none but rows > 0; 0 and 0 when rows == 0
 *                      [3] the index of the first line outside the grammar (lines count from 0, headers included, so bin r is
 *                          line r + 2), -1 when the text is of the grammar
 *   ws    epg_sbl_ws_bytes(nbytes) bytes, 16-byte aligned.
 * rows > cap is not an error: the caller compares info[0] with what it expects.  nbytes == 0 is a text without lines
 * (info = 0, 0, 0, 0). */
int epg_sbl_parse(const char* text, int64_t nbytes, int8_t* col, int64_t cap, int64_t* info, void* ws, int64_t ws_bytes, void* stream);

/* Transpose a batch of columns into the state matrix:  X[r * ldx + col0 + k] = cols[k * col_pitch + r]  for r < R, k < nb.
 *   cols  int8 [nb][col_pitch]  biosample-major, 16-byte aligned, col_pitch a multiple of 16 and >= R.  The bytes of a column
 *                               behind R may be read; they reach nothing.
 *   X     int8 [R, ldx]         row-major, any alignment, ldx >= col0 + nb.  Only columns col0 .. col0 + nb - 1 of rows 0 .. R - 1 are
 *                               written (row padding, columns >= N: the caller's, as everywhere in epilogos_amd.h).
 * nb <= EPG_SBL_MAX_BATCH (more: EPG_ERR_UNSUPPORTED).  R == 0 or nb == 0 does nothing. */
int epg_sbl_transpose(const int8_t* cols, int32_t nb, int64_t col_pitch, int64_t R, int8_t* X, int64_t ldx, int64_t col0, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EPILOGOS_STATEBYLINE_H */
