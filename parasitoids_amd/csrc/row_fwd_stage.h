// Staging area of the staged persistent forward row kernel (k_row_fwd_rsps): the 2 NP source rows of a
// unit, copied HBM -> LDS 16 bytes per lane in chunks of 1 KB (one wave instruction: 64 words = 128
// doubles) while the unit before is transformed.
// A source row is K doubles (K odd: rows of a K x K box) and starts on an 8-byte boundary only, so the
// copy starts at the row's address ROUNDED DOWN to 16 bytes and the first stage adds the row's parity
// e = (address / 8) & 1 to its slot: a staged row is a plain image of the aligned span, element `col` at
// double e + col.  The 16-byte words of a row are 0 .. last, last = (e + K - 1) / 2; lanes past `last`
// copy word `last` again (to their own place in the chunk, which nobody reads).  With e = 0 the word
// `last` reaches one double past the row: the next row's first element, except where the row ends the
// source buffer.  There (`room`, the doubles from the aligned start to the end of the buffer, is short
// of 2 last + 2) no lane copies a word >= last and the row's last element travels as two 4-byte words
// instead (fstage_tail), so nothing is read past the buffer.
// Plain integers, host and device: tests walk it through ps_row_fwd_stage_walk.
#pragma once
#include "fft_core.h"

PS_HD int fstage_chunks(int K) { return (K + 1 + 127) / 128; }              // 1 KB chunks of a staged row
PS_HD int fstage_row(int K) { return fstage_chunks(K) * 128; }              // doubles of a staged row
PS_HD size_t fstage_bytes(int np, int K) { return (size_t)2 * np * fstage_chunks(K) * 1024; }
// staged row r (2 * half + {0: row a, 1: row b}) of parity e, source column col -> double in the staging area
PS_HD int fstage_slot(int K, int r, int e, int col) { return r * fstage_row(K) + e + col; }
PS_HD int fstage_last(int K, int e) { return (e + K - 1) >> 1; }
// the row's last word would reach past the end of the buffer
PS_HD bool fstage_tail(int K, int e, int64_t room) { return 2 * (int64_t)fstage_last(K, e) + 2 > room; }
// 16-byte word (from the aligned start of the row) that `lane` copies in chunk c, -1: none
PS_HD int fstage_word(int K, int e, int64_t room, int c, int lane) {
  const int w = c * 64 + lane, last = fstage_last(K, e);
  if (fstage_tail(K, e, room)) return w < last ? w : -1;
  return w < last ? w : last;
}
