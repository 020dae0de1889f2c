/*
 * epilogos_segments.h -- C ABI of the GPU reader of ChromHMM segment files (csrc/epg_segments.hip), part of libepilogos_hip.so.
 *
 * ChromHMM writes <cell>_<n>_segments.bed by default: one file per biosample for the whole genome, one line
 * chrom TAB start TAB end TAB label per run of equal states.  epg_seg_parse turns the text of one file into its lines' first bins
 * and states and the run of lines of every chromosome of a table; epg_seg_expand writes one chromosome's column of int8 states
 * from them.  The columns go into the [bins, biosamples] matrix with epg_sbl_transpose (epilogos_statebyline.h), and the matrix
 * into the file that header lays out.  Python: epilogos_amd/segments.py.
 *
 * Conventions are those of epilogos_amd.h: plain pointers and sizes, caller-owned device buffers, the stream last, every argument
 * validated before the first HIP call, EPG_OK or a negative EPG_ERR_* code with the message in epg_last_error().  No call
 * allocates or synchronises.
 *
 * Strict grammar of a segment text, for a bin width W.  Lines are ended by '\n'; the '\n' of the last line may be missing.
 * Every line has exactly four tab-separated fields:
 *   chrom       1 .. 79 bytes, none of them tab, newline or '\r'
 *   start, end  1 .. 10 ASCII digits each, no sign, no blank, no leading zero unless the value is 0; both multiples of W,
 *               end > start, end / W < 2^31
 *   label       one optional ASCII letter, then 1 .. 3 digits, the first not '0', value 1 .. 127, then optionally '_' and any
 *               bytes up to the line end except tab and '\r': E7, 7, U12 and 7_TssFlnk are labels.  The state is the number.
 * Across lines: the lines of one chromosome form one run of consecutive lines; the first line of a run starts at 0; every other
 * line's start is the previous line's end; a chromosome of the table appears in one run only (the line that starts its second
 * run is outside the grammar).  The rows of chromosome c are R_c = the end of its last segment / W.
 * Lines of chromosomes that are not in the table are held to the per-line grammar only.
 */
#ifndef EPILOGOS_SEGMENTS_H
#define EPILOGOS_SEGMENTS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Largest text, the bytes of a chromosome name of the table (NUL-padded), and the bytes of workspace a text of nbytes and a table
 * of nchrom names need (< 0: nbytes outside 0 .. EPG_SEG_MAX_TEXT_BYTES or nchrom outside 0 .. EPG_SEG_MAX_CHROMS). */
#define EPG_SEG_MAX_TEXT_BYTES 0x7fff0000
#define EPG_SEG_NAME_BYTES 80
int64_t epg_seg_ws_bytes(int64_t nbytes, int32_t nchrom);

/* The kernels' constants, for callers that size tables and tests that aim at the boundaries:
 *   EPG_SEG_THREAD_BYTES      bytes of text per thread of the line index
 *   EPG_SEG_BLOCK_BYTES       bytes of text per workgroup of the line index
 *   EPG_SEG_EXPAND_TILE_BINS  bins per workgroup of the expansion
 *   EPG_SEG_MAX_CHROMS        the most names a table holds
 * -1 for any other `which`. */
#define EPG_SEG_THREAD_BYTES 0
#define EPG_SEG_BLOCK_BYTES 1
#define EPG_SEG_EXPAND_TILE_BINS 2
#define EPG_SEG_MAX_CHROMS 3
int32_t epg_seg_constant(int32_t which);

/* Parse text[0, nbytes) (device memory, any alignment), the whole text of one biosample's segment file.
 *   names  char [nchrom][EPG_SEG_NAME_BYTES]  the table: NUL-padded chromosome names (device memory); of two equal names the
 *                       first is found.  May be NULL when nchrom == 0.
 *   width  W > 0
 *   first  int32 [cap]  first[l] = start / W of line l           } for l < min(lines, cap); -1 where line l is outside the
 *   state  int8 [cap]   state[l] = the label's number minus 1    } per-line grammar.  Nothing behind min(lines, cap) is written.
 *                       Both may be NULL when cap == 0.
 *   runs   int64 [nchrom][3]  the first line, the number of lines and R_c of chromosome c of the table; 0, 0, 0 when the text
 *                       does not hold it, or when its run does not end below cap
 *   info   int64 [4]    written, not accumulated:
 *                       [0] lines
 *                       [1] the lowest and [2] the highest state as written (1-based) over the lines of the table's chromosomes
 *                           that are of the per-line grammar; 128 and 0 when there is none but lines > 0; 0 and 0 when lines == 0
 *                       [3] the index of the first line (from 0) outside the grammar or the cross-line rules, -1 when there is none
 *   ws     epg_seg_ws_bytes(nbytes, nchrom) bytes, 16-byte aligned; info 8-byte aligned, first 4-byte aligned.
 * lines > cap is not an error: the caller sizes cap from a count of the newlines and compares info[0].  When info[3] >= 0 the
 * caller reads the file some other way: first, state and runs then hold what the lines before and behind the offence gave, and
 * epg_seg_expand on them stays inside its buffers but writes no column worth keeping.  nbytes == 0 is a text without lines. */
int epg_seg_parse(const char* text, int64_t nbytes, const char* names, int32_t nchrom, int32_t width,
                  int32_t* first, int8_t* state, int64_t cap, int64_t* runs, int64_t* info,
                  void* ws, int64_t ws_bytes, void* stream);

/* Expand chromosome c of a parsed file into its column: col[r] = state[l] for the line l of the run with
 * first[l] <= r < first[l] + length, for r < min(R, runs[c][2]).  The run is read from `runs` ON THE DEVICE: no host copy of it
 * is needed to launch.  first, state and runs are those one epg_seg_parse wrote (runs: the whole table, c indexes it).
 *   col    int8 [R]     16-byte aligned.  Bytes r >= runs[c][2] are not written.
 * R == 0 does nothing. */
int epg_seg_expand(const int32_t* first, const int8_t* state, const int64_t* runs, int32_t c,
                   int8_t* col, int64_t R, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EPILOGOS_SEGMENTS_H */
