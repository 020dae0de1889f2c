/*
 * epilogos_scores_text.h -- C ABI of the GPU scores-text parser (csrc/epg_scores_text.hip), part of libepilogos_hip.so.
 *
 * A scores file is "chr\tstart\tend\t" + S values written "%.5f", one line per bin (epilogos_io.h, epgio_write_scores).  Each
 * value is an integer times 1e-5 written in decimal, so the int32 grid value similarity search works on
 * (similaritySearch_max_mean.to_grid) is the digits themselves: read as text it is exact by construction.  The parser is
 * STRICT: it takes only what it can prove equal to the general reader's result and reports everything else, with the first
 * offending row, so that the caller can hand the file to the general reader.
 *
 * Conventions are those of epilogos_amd.h: plain pointers and sizes, caller-owned device buffers, the stream last, every argument
 * validated before the first HIP call, EPG_OK or a negative EPG_ERR_* code with the message in epg_last_error().  The prefix
 * is epgt_ so that the two headers' entry points are told apart by name.
 *
 * The text of a call is a CHUNK: whole rows.  It ends with the '\n' of its last row, or -- the end of a file without a final
 * newline -- with the last byte of its last row.  F = S + 3 is the number of fields of a row.
 *
 * Strict grammar.  Row: F fields separated by '\t', ended by '\n'.  Every byte of a field is printable ASCII (0x21 .. 0x7e),
 * so blanks, '\r' and bytes >= 0x80 are refused; no field is empty (a blank line is a row of one empty field).
 *   chromosome  first byte a letter or '_' (a column of "-1", ".5" or "+inf" would be numbers to the general reader)
 *   start, end  1 .. 19 digits, value <= INT64_MAX
 *   score       [-] digits [. 1..5 digits], at most 24 bytes, |value x 1e5| < 2^31; "-0.00000" is 0
 * No exponent, no '+', no "nan" / "inf".
 */
#ifndef EPILOGOS_SCORES_TEXT_H
#define EPILOGOS_SCORES_TEXT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The status word: EPGT_CLEAN, or (row << 4 | reason) of the first offending row (the smallest reason when a row has several).
 * Rows count from row0 of the call, so a word that several calls share names the row of the file. */
#define EPGT_CLEAN INT64_MAX
#define EPGT_REASON_FIELDS 1  /* a number of fields other than F, the first row's (a blank line included) */
#define EPGT_REASON_EMPTY 2   /* an empty field */
#define EPGT_REASON_BYTE 3    /* a blank, a control character or a byte outside ASCII */
#define EPGT_REASON_CHROM 4   /* a chromosome field that does not start with a letter or '_' */
#define EPGT_REASON_COORD 5   /* start or end is not a plain decimal integer that fits int64 */
#define EPGT_REASON_SCORE 6   /* a score that is not [-]digits[.1-5 digits] */
#define EPGT_REASON_RANGE 7   /* |score x 1e5| >= 2^31 */
#define EPGT_REASON_ROWS 8    /* the text holds more rows than the call was given */

/* Largest chunk, and the bytes of workspace a chunk of nbytes needs (< 0: nbytes outside 0 .. EPGT_MAX_CHUNK_BYTES). */
#define EPGT_MAX_CHUNK_BYTES 0x7fff0000
int64_t epgt_scores_ws_bytes(int64_t nbytes);

/* Parse the `rows` rows of text[0, nbytes) (device memory, any alignment), F fields each:
 *   X      int32 [.., F - 3]  row row0 + r receives the scores of row r, x 1e5
 *   start  int64 [..]         likewise
 *   end    int64 [..]
 *   chrom_at int32 [..]       -1 where the chromosome field equals the previous row's byte for byte, else the offset of the row's
 *                             first byte in `text`; row 0 of a call always gets its offset (0): the caller compares across calls
 *   status int64 [2]          [0]: atomic minimum of itself and this call's status word -- the caller sets it to EPGT_CLEAN before
 *                             the first call; [1]: the number of whole rows the device found in the text
 * `rows` (<= nbytes) is the caller's count of the chunk's rows (the '\n' of the text, plus one when the last byte is not '\n'); a text that
 * holds fewer rows reports EPGT_REASON_FIELDS at the first row that is short, one that holds more EPGT_REASON_ROWS at row
 * row0 + rows.  When status[0] is not EPGT_CLEAN the four outputs hold nothing of use.  ws: epgt_scores_ws_bytes(nbytes) bytes.
 * nbytes == 0 (then rows == 0) is valid and does nothing: no launch, nothing written. */
int epgt_scores_parse(const char* text, int64_t nbytes, int32_t F, int64_t rows, int64_t row0, int32_t* X, int64_t* start,
                      int64_t* end, int32_t* chrom_at, void* ws, int64_t ws_bytes, int64_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EPILOGOS_SCORES_TEXT_H */
