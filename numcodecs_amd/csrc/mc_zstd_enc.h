// mc_zstd_enc.h -- Zstandard (RFC 8878) frames written: the rules, shared by
// the gfx950 kernels (mc_zstd_enc.hip) and the host build of the CPU suite
// (tests/native_zstd_enc).  mc_zstd_encode_chunk below is the plain scalar
// statement of the format written here; the kernels produce the same bytes for
// every input.  The planning of a block (mc_ze_plan: Huffman lengths, the
// weight description, the three normalisations, modes, encoding tables, the
// state chains and every size) is one piece of code for both: the host runs it
// with one "lane", the device with the 64 lanes of a wave over LDS (loops
// strided by lane, serial steps on lane 0, the three state chains on lanes
// 0 ... 2).  The format tables, the FSE cell rule and spread step, and XXH64 are
// mc_zstd.h's; the length-limited Huffman construction is mc_deflate.h's
// mc_dfl_code_lengths.
//
// Frame.  No dictionary; Frame_Content_Size always declared.  1 <= n <= 65536:
// Single_Segment, FCS of 1 byte (n <= 255: descriptor 20) or 2 bytes holding
// n - 256 (descriptor 60).  n > 65536: descriptor 80, Window_Descriptor 30 (a
// 64 KiB window), FCS of 4 bytes; the window holds because no match reaches
// before its segment, so no offset exceeds 65535.  The checksum flag (04) adds
// the low 32 bits of XXH64(seed 0) of the content behind the last block.  n = 0
// is written by the caller on the host (28 B5 2F FD 20 00 01 00 00, libzstd's
// bytes; with the checksum 24 and 99 E9 D8 51 behind); n >= 2^30 is refused.
//
// Segments and blocks.  A chunk is cut into segments of 65536 bytes, the last
// one shorter; each becomes exactly one block and is parsed with no reference
// to anything before it.  The block type is chosen by exact size, ties to the
// earlier of: Raw_Block (3 + n_k bytes); RLE_Block (4 bytes, only when every
// byte of the segment is equal); Compressed_Block (only when its content is
// smaller than n_k).  So mc_zstd_enc_bound(n, checksum) = header(n) + 3 *
// nsegments + n + 4 * checksum: no frame exceeds it and noise meets it.
//
// Parse: mc_deflate.h's (windows of 64 positions, a 4096-entry hash of 4-byte
// words, the lowest slot with a valid candidate wins, backward then forward
// extension, insertion of the consumed positions only), with two differences:
// a candidate is valid at any distance inside the segment (<= 65535), and a
// match of any length is one sequence.  A sequence covers 4 bytes or more: at
// most n_k / 4 <= 16384 of them, so Number_of_Sequences takes 1 or 2 bytes.
// The literals are gathered in order into a buffer of their own.
//
// Offsets.  A real offset is written as Offset_Value offset + 3.  A sequence
// whose offset equals the previous sequence's offset in the same block, and
// whose literal length is not 0, is written as Offset_Value 1.  The first
// sequence of a block and a sequence with literal length 0 are never repeat
// codes.  The decoder's rep[0] then always equals "the previous offset of this
// block" when it is asked for: a real offset moves into rep[0]; Offset_Value 1
// with a literal length above 0 reads rep[0] and changes nothing, and by
// induction the sequence before it left its own offset there; the first
// sequence, whose rep[0] is another block's, is never a repeat code.  So no
// block depends on the history another block left.
//
// Literals section, by exact size, ties to the earlier of: Raw;
// Huffman-compressed (two or more distinct bytes).  RLE literals are not
// written: the first occurrence of a byte value in a segment is always a
// literal, so all literals of a block are one byte only when the whole segment
// is, and then the block is an RLE_Block (or, for one byte, a Raw_Block).  The
// header takes the smallest Size_Format holding
// its sizes.  Compressed: code lengths from mc_dfl_code_lengths limited to 11
// bits; weight = longest length + 1 - length; one stream below 256 literals,
// four otherwise (the first three carry (L + 3) / 4 symbols).  The tree
// description is the smaller (ties: direct) of direct 4-bit weights (128
// weights or fewer) and FSE-compressed weights (two weights or more, two
// distinct values or more, fewer than 120 bytes behind the header byte): two interleaved states, the
// normalisation and count writer below with an accuracy log of 5 or 6.  If
// neither can be written the compressed form is no candidate.  Treeless
// literals are not used.
//
// Sequences section.  Each of LL / OF / ML: RLE_Mode when one code occurs;
// else FSE_Compressed_Mode if cost(fse) < cost(predefined), else
// Predefined_Mode, where cost(table) = sum over the codes of count *
// (256 * log - mc_ze_log2q8(normalised count)) (a "less than one" count of the
// predefined tables as 1) and the FSE form adds 2048 per byte of its
// description; mc_ze_log2q8(v) = 256 * floor(log2 v) + the next 8 bits of v
// below its top bit: integer arithmetic, the same on host and device.
// Repeat_Mode is not used.
//
// Normalisation (mc_ze_normalise).  log = floor(log2(total)) clamped to
// [max(5, ceil(log2(codes in use))), the table's limit (9 / 8 / 9; 6 for
// weights)].  A code in use gets max(1, floor(count << log / total)); what is
// missing from 1 << log goes to the most frequent code (the lowest of equals);
// what is too much is taken, one at a time, from the code whose normalised
// count is largest (the lowest of equals), which is above 1 while anything is
// too much.  No count of -1 is written.
//
// Encoding tables follow from mc_zstd_fse_step and the cell rule of
// mc_zstd_fse_cell: the cells are spread as the decoder's builder spreads
// them ("less than one" codes of the predefined tables from the top), cell u
// of code s is that code's state number n_s + (its rank among the code's cells
// by position), reads nb = log - highbit(state number) bits and covers the
// states [(number << nb) - size, +2^nb).  The bitstreams are written for a
// decoder that reads backwards: the last sequence is encoded first and starts
// from the first cell of its code; each stream ends with the 1-bit end mark.
// The last two weights of an FSE weight stream start from the first cell of
// their value, which reads one bit or more: that is where the decoder runs
// out of bits and stops.
//
// Termination and bounds.  The parse advances p by 4 or more per sequence or
// 64 per window to n_k; normalisation takes fewer than 53 corrections; the
// count writer passes each code once; every chain passes each sequence (weight)
// once; the spread visits each cell once.  No source byte outside [0, n) is
// read: a slot's word needs pos + 4 <= n_k, extensions stop at the segment's
// ends.  The frame's exact size is known after the plan of its blocks, before
// any frame byte is written: a frame larger than its slot is refused (E_SPACE
// and the size it needs) and the slot stays untouched; no byte outside [0,
// frame size) is written.  Every table index is a code below the table's code
// count or a state below 1 << log.
#pragma once

#include "mc_deflate.h"
#include "mc_zstd.h"

#define MC_ZE_SEGMENT 65536u
#define MC_ZE_TABLE 4096u
#define MC_ZE_WINDOW 64u
#define MC_ZE_MIN_MATCH 4u
#define MC_ZE_MAX_SEQS (MC_ZE_SEGMENT / MC_ZE_MIN_MATCH)
#define MC_ZE_MAX_BYTES 0x40000000u

// the histogram of one segment: literal bytes, then the LL / OF / ML codes
#define MC_ZE_H_LL 256u
#define MC_ZE_H_OF 320u
#define MC_ZE_H_ML 352u
#define MC_ZE_HIST 416u

#define MC_ZE_RAW 0u  // block types; literals forms (no RLE)
#define MC_ZE_RLE 1u
#define MC_ZE_COMPRESSED 2u
#define MC_ZE_PREDEFINED 0u  // modes (RLE 1, FSE 2)
#define MC_ZE_FSE 2u
#define MC_ZE_W_NONE 0u
#define MC_ZE_W_DIRECT 1u
#define MC_ZE_W_FSE 2u
#define MC_ZE_W_FSE_MAX 120u  // an FSE weight description holds fewer bytes than this behind its header byte

#define MC_ZE_F_CHECKSUM 1u  // the chunk record's flags

// error record of the batch (0 = none)
#define MC_ZE_E_SPACE 1  // the frame does not fit its slot; second word: the frame's size
#define MC_ZE_E_TABLE 2  // the caller's chunk record is out of range

// One sequence of the parse: a = literal run | offset << 16, b = match length.
struct mc_ze_seq {
  uint32_t a, b;
};
// What the chains leave per sequence q: the bits read between sequence q and
// q + 1 by each state, value | count << 9.
struct mc_ze_trans {
  uint16_t ll, of, ml, pad;
};

// One segment, as the kernels leave it in the workspace and the reporting form
// of the scalar encoder hands it to the tests.
struct mc_ze_seg {
  uint32_t nseq, nlit;   // parse: sequences, literals
  uint32_t same;         // parse: every byte of the segment is equal
  uint32_t nrep;         // parse: sequences written as Repeated_Offset1
  uint32_t type, bytes;  // MC_ZE_RAW / RLE / COMPRESSED; the block with its 3-byte header
  uint32_t lit_form, streams, wdesc;  // MC_ZE_RAW / COMPRESSED; 0, 1 or 4; MC_ZE_W_*
  uint32_t mode[3];      // LL, OF, ML (0 where the block has no sequences)
  uint32_t lit_bytes, seq_bytes;  // the two sections of a compressed block's content
  uint32_t off;          // the block's first byte in the frame
  uint32_t reserved;
};

// What the plan of a compressed block hands to its emitter.
struct alignas(8) mc_ze_plan_out {
  uint8_t lens[256];      // Huffman code lengths
  uint8_t wdesc[160];     // the tree description (an FSE form is given up before it passes 140 bytes)
  uint8_t tdesc[3][64];   // the LL / OF / ML table descriptions (RLE: the code)
  uint32_t wdesc_bytes, maxlen;
  uint32_t tdesc_bytes[3];
  uint32_t stream_bytes[4];
  uint32_t log[3], state0[3];
  uint32_t seq_bits;      // the sequence bitstream without its end mark
  uint32_t lit_header, lit_comp;  // the literals header's bytes and Compressed_Size
};

// One record of the encode batch's chunk table (device table, one per chunk
// with nbytes > 0; include/mcodec.h): src is relative to the entry point's
// `src` base (0: absolute device addresses).
struct mc_zstd_enc_chunk {
  uint64_t src;       // the chunk's bytes
  uint64_t dst;       // device address of its output slot (the frame)
  uint32_t nbytes;
  uint32_t dst_cap;   // the slot's size; mc_zstd_enc_bound(nbytes, checksum) always suffices
  uint32_t seg_base;  // index of the chunk's first segment in the batch
  uint32_t seq_base;  // index of the chunk's first sequence record: it takes ceil(nbytes / 4)
  uint32_t flags;     // MC_ZE_F_CHECKSUM
  uint32_t reserved;  // 0
};

MC_ZSTD_HD uint32_t mc_ze_nsegments(uint32_t n) { return (n + MC_ZE_SEGMENT - 1) / MC_ZE_SEGMENT; }  // n < 2^30
MC_ZSTD_HD uint32_t mc_ze_seg_len(uint32_t n, uint32_t k) {
  const uint32_t start = k * MC_ZE_SEGMENT;
  return n - start < MC_ZE_SEGMENT ? n - start : MC_ZE_SEGMENT;
}
MC_ZSTD_HD uint32_t mc_ze_header_bytes(uint64_t n) { return n <= 255u ? 6u : n <= MC_ZE_SEGMENT ? 7u : 10u; }
MC_ZSTD_HD uint64_t mc_zstd_enc_bound(uint64_t n, uint32_t checksum) {
  const uint64_t nseg = n ? (n + MC_ZE_SEGMENT - 1) / MC_ZE_SEGMENT : 1;
  return mc_ze_header_bytes(n) + 3 * nseg + n + (checksum ? 4u : 0u);
}
MC_ZSTD_HD uint32_t mc_ze_seq_records(uint32_t n) { return (n + MC_ZE_MIN_MATCH - 1u) / MC_ZE_MIN_MATCH; }
MC_ZSTD_HD bool mc_ze_chunk_ok(const mc_zstd_enc_chunk &c, uint32_t nsegments_total, uint64_t nsequences_total) {
  if (c.nbytes < 1 || c.nbytes >= MC_ZE_MAX_BYTES || !c.dst) return false;
  if ((uint64_t)c.seq_base + mc_ze_seq_records(c.nbytes) > nsequences_total) return false;
  return (uint64_t)c.seg_base + mc_ze_nsegments(c.nbytes) <= nsegments_total;
}
// the frame header of n >= 1 bytes: mc_ze_header_bytes(n) bytes
MC_ZSTD_HD void mc_ze_put_header(uint8_t *dst, uint32_t n, uint32_t checksum) {
  dst[0] = 0x28, dst[1] = 0xB5, dst[2] = 0x2F, dst[3] = 0xFD;
  const uint32_t c = checksum ? 4u : 0u;
  if (n <= 255u) {
    dst[4] = (uint8_t)(0x20u | c), dst[5] = (uint8_t)n;
  } else if (n <= MC_ZE_SEGMENT) {
    dst[4] = (uint8_t)(0x60u | c), dst[5] = (uint8_t)(n - 256u), dst[6] = (uint8_t)((n - 256u) >> 8);
  } else {
    dst[4] = (uint8_t)(0x80u | c), dst[5] = 0x30;
    for (uint32_t k = 0; k < 4u; ++k) dst[6u + k] = (uint8_t)(n >> (8u * k));
  }
}
MC_ZSTD_HD uint32_t mc_ze_block_header(uint32_t last, uint32_t type, uint32_t size) { return last | (type << 1) | (size << 3); }

// a table entry (position + 1, 0 = empty) as a candidate for `pos`
MC_ZSTD_HD bool mc_ze_entry_ok(uint32_t entry, uint32_t pos) { return entry != 0 && entry - 1 < pos; }

// ---- codes ---------------------------------------------------------------------
MC_ZSTD_HD uint32_t mc_ze_ll_code(uint32_t ll) {  // ll <= 65536
  if (ll < 16u) return ll;
  uint32_t c = 16u;
  while (c < MC_ZSTD_LL_MAX && ll >= mc_zstd_ll_base(c + 1u)) ++c;
  return c;
}
MC_ZSTD_HD uint32_t mc_ze_ml_code(uint32_t ml) {  // 3 <= ml <= 65536
  if (ml < 35u) return ml - 3u;
  uint32_t c = 32u;
  while (c < MC_ZSTD_ML_MAX && ml >= mc_zstd_ml_base(c + 1u)) ++c;
  return c;
}
// the three codes of a sequence and their extra bits; prev_off: the offset of
// the sequence before it in the block, 0 for the first.  w: 0 LL, 1 OF, 2 ML.
struct mc_ze_sym {
  uint32_t c[3], xb[3], xv[3];
};
MC_ZSTD_HD mc_ze_sym mc_ze_symbols(mc_ze_seq s, uint32_t prev_off) {
  const uint32_t ll = s.a & 0xffffu, off = s.a >> 16, ml = s.b;
  mc_ze_sym y;
  y.c[0] = mc_ze_ll_code(ll), y.xb[0] = mc_zstd_ll_bits(y.c[0]), y.xv[0] = ll - mc_zstd_ll_base(y.c[0]);
  const uint32_t ov = (off == prev_off && ll != 0u) ? 1u : off + 3u;
  y.c[1] = mc_zstd_highbit(ov), y.xb[1] = y.c[1], y.xv[1] = ov - (1u << y.c[1]);
  y.c[2] = mc_ze_ml_code(ml), y.xb[2] = mc_zstd_ml_bits(y.c[2]), y.xv[2] = ml - mc_zstd_ml_base(y.c[2]);
  return y;
}
MC_ZSTD_HD uint32_t mc_ze_pick(const uint32_t (&a)[3], uint32_t w) { return w == 0 ? a[0] : w == 1 ? a[1] : a[2]; }
MC_ZSTD_HD uint32_t mc_ze_hist_at(uint32_t w) { return w == 0 ? MC_ZE_H_LL : w == 1 ? MC_ZE_H_OF : MC_ZE_H_ML; }
MC_ZSTD_HD uint32_t mc_ze_ncodes(uint32_t w) { return w == 0 ? MC_ZSTD_LL_MAX + 1u : w == 1 ? MC_ZSTD_OF_MAX + 1u : MC_ZSTD_ML_MAX + 1u; }
MC_ZSTD_HD uint32_t mc_ze_max_log(uint32_t w) { return w == 1 ? MC_ZSTD_OF_LOG : MC_ZSTD_LL_LOG; }

MC_ZSTD_HD uint32_t mc_ze_log2q8(uint32_t v) {  // v >= 1
  const uint32_t hb = mc_zstd_highbit(v);
  return 256u * hb + ((hb >= 8u ? v >> (hb - 8u) : v << (8u - hb)) & 255u);
}
MC_ZSTD_HD uint32_t mc_ze_lit_header(uint32_t L) { return L < 32u ? 1u : L < 4096u ? 2u : 3u; }
MC_ZSTD_HD uint32_t mc_ze_nseq_bytes(uint32_t nseq) { return nseq < 128u ? 1u : 2u; }  // nseq <= 16384

// ---- FSE, the write direction -------------------------------------------------------
// One encoding table (LDS on the device): 64 codes, 512 cells at the most.
struct mc_ze_fse {
  int16_t norm[64];
  uint16_t cum[64];    // the first entry of each code in enc[]
  uint16_t fill[64];
  uint16_t enc[512];   // the cells of each code by position: entry cum[s] + k is state number n_s + k
  uint8_t cell[512];   // the code of each cell
  uint32_t log, nsym;
};

// hist[0, nsym) (two codes or more in use, `total` their sum) -> norm[0, nsym); returns the log
MC_ZSTD_HD uint32_t mc_ze_normalise(const uint32_t *hist, uint32_t nsym, uint32_t total, uint32_t max_log, int16_t *norm) {
  uint32_t used = 0, best = 0;
  for (uint32_t s = 0; s < nsym; ++s) {
    used += hist[s] != 0u;
    if (hist[s] > hist[best]) best = s;
  }
  uint32_t lo = mc_zstd_highbit(used - 1u) + 1u;
  if (lo < 5u) lo = 5u;
  uint32_t log = mc_zstd_highbit(total);
  log = log < lo ? lo : log > max_log ? max_log : log;
  const uint32_t size = 1u << log;
  uint32_t sum = 0;
  for (uint32_t s = 0; s < nsym; ++s) {
    uint32_t v = (uint32_t)(((uint64_t)hist[s] << log) / total);
    if (hist[s] != 0u && v == 0u) v = 1u;
    norm[s] = (int16_t)v;
    sum += v;
  }
  if (sum < size) norm[best] = (int16_t)(norm[best] + (int16_t)(size - sum));
  for (; sum > size; --sum) {  // (fewer than nsym passes: only a count raised to 1 adds to the sum)
    uint32_t top = 0;
    for (uint32_t s = 1; s < nsym; ++s)
      if (norm[s] > norm[top]) top = s;
    --norm[top];
  }
  return log;
}

// the count description mc_zstd_read_counts reads back; returns its bytes (at most 64)
MC_ZSTD_HD uint32_t mc_ze_write_counts(const int16_t *norm, uint32_t nsym, uint32_t log, uint8_t *out) {
  uint64_t acc = log - 5u;
  uint32_t cnt = 4u, bytes = 0;
  int32_t remaining = (int32_t)(1u << log) + 1, threshold = (int32_t)(1u << log);
  uint32_t nb = log + 1u, sym = 0;
  bool prev0 = false;
  while (remaining > 1 && sym < nsym) {
    if (prev0) {
      uint32_t n0 = sym;
      while (n0 < nsym && norm[n0] == 0) ++n0;
      uint32_t run = n0 - sym;
      for (; run >= 3u; run -= 3u) acc |= (uint64_t)3u << cnt, cnt += 2u;
      acc |= (uint64_t)run << cnt, cnt += 2u;
      while (cnt >= 8u) out[bytes++] = (uint8_t)acc, acc >>= 8, cnt -= 8u;
      sym = n0;
      prev0 = false;
      if (sym >= nsym) break;  // (never: remaining > 1 means a count is still to come)
    }
    const int32_t count = norm[sym++];
    const int32_t max = (2 * threshold - 1) - remaining;
    remaining -= count;
    int32_t v = count + 1;
    if (v >= threshold) v += max;
    acc |= (uint64_t)(uint32_t)v << cnt;
    cnt += nb - (v < max ? 1u : 0u);
    prev0 = count == 0;
    while (remaining < threshold && threshold > 1) --nb, threshold >>= 1;  // (remaining >= 1: it ends at 1)
    while (cnt >= 8u) out[bytes++] = (uint8_t)acc, acc >>= 8, cnt -= 8u;
  }
  if (cnt) out[bytes++] = (uint8_t)acc;
  return bytes;
}

// norm[0, nsym) and log -> the cells and enc[] (one lane)
MC_ZSTD_HD void mc_ze_build(mc_ze_fse *F) {
  const uint32_t size = 1u << F->log, mask = size - 1u, step = mc_zstd_fse_step(F->log);
  uint32_t high = size - 1u, c = 0;
  for (uint32_t s = 0; s < F->nsym; ++s) {
    F->cum[s] = (uint16_t)c, F->fill[s] = 0;
    c += F->norm[s] == -1 ? 1u : (uint32_t)F->norm[s];
    if (F->norm[s] == -1) F->cell[high--] = (uint8_t)s;
  }
  uint32_t pos = 0;
  for (uint32_t s = 0; s < F->nsym; ++s)
    for (int32_t i = 0; i < F->norm[s]; ++i) {
      F->cell[pos] = (uint8_t)s;
      do pos = (pos + step) & mask; while (pos > high);
    }
  for (uint32_t u = 0; u < size; ++u) {
    const uint32_t s = F->cell[u];
    F->enc[F->cum[s] + F->fill[s]++] = (uint16_t)u;
  }
}
MC_ZSTD_HD uint32_t mc_ze_count_of(const mc_ze_fse *F, uint32_t s) { return F->norm[s] == -1 ? 1u : (uint32_t)F->norm[s]; }
// the first cell of code s: where the last symbol of a chain starts
MC_ZSTD_HD uint32_t mc_ze_first(const mc_ze_fse *F, uint32_t s) { return F->log ? F->enc[F->cum[s]] : 0u; }
// code s in front of state t: the cell it is written from; *bits = value | count << 9
MC_ZSTD_HD uint32_t mc_ze_encode(const mc_ze_fse *F, uint32_t s, uint32_t t, uint32_t *bits) {
  if (F->log == 0u) {  // RLE_Mode
    *bits = 0;
    return 0;
  }
  const uint32_t ns0 = mc_ze_count_of(F, s), T = t + (1u << F->log);
  uint32_t nb = F->log - mc_zstd_highbit(ns0);
  if ((T >> nb) < ns0) --nb;
  const uint32_t ns = T >> nb;  // ns0 <= ns < 2 ns0: the cell rule of mc_zstd_fse_cell
  *bits = (T & ((1u << nb) - 1u)) | (nb << 9);
  return F->enc[F->cum[s] + (ns - ns0)];
}

// a forward bit writer over bytes (host emit, weight streams)
struct mc_ze_bitw {
  uint8_t *p;
  uint64_t acc;
  uint32_t cnt, pos;
  MC_ZSTD_HD void put(uint32_t v, uint32_t nb) {  // nb <= 32, cnt < 8
    acc |= (uint64_t)v << cnt;
    cnt += nb;
    while (cnt >= 8u) p[pos++] = (uint8_t)acc, acc >>= 8, cnt -= 8u;
  }
  MC_ZSTD_HD void finish() {  // the end mark
    put(1u, 1u);
    if (cnt) p[pos++] = (uint8_t)acc, acc = 0, cnt = 0;
  }
};

// ---- the plan of a block -----------------------------------------------------------
// the work area of one segment's plan (LDS on the device)
struct alignas(16) mc_ze_work {
  mc_dfl_work huf;
  mc_ze_fse fse[4];      // LL, OF, ML, the Huffman weights
  uint32_t whist[16];
  uint32_t sbits[4];
  uint8_t weights[256];
};

// The Huffman side: code lengths, weights, the tree description, the streams'
// sizes.  Returns the literals section's bytes in the compressed form, 0 if it
// is no candidate.  lits[0, L): the block's literals, L >= 1; hist[0, 256) theirs.
template <class X>
MC_ZSTD_HD uint32_t mc_ze_plan_huffman(X &x, mc_ze_work *W, const uint32_t *hist, const uint8_t *lits, uint32_t L,
                                       mc_ze_plan_out *P, uint32_t *wform, uint32_t *nstreams) {
  mc_dfl_code_lengths(x, &W->huf, hist, 256u, MC_ZSTD_HUF_LOG, P->lens);
  uint32_t ml = 0, last = 0;
  for (uint32_t s = x.lane; s < 256u; s += x.nlanes) {
    if (P->lens[s] > ml) ml = P->lens[s];
    if (P->lens[s]) last = s;
  }
  ml = x.max(ml), last = x.max(last);  // two codes or more: last >= 1
  const uint32_t nw = last;            // the last code's weight is implied
  for (uint32_t s = x.lane; s < 256u; s += x.nlanes) W->weights[s] = (uint8_t)(P->lens[s] ? ml + 1u - P->lens[s] : 0u);
  for (uint32_t s = x.lane; s < 16u; s += x.nlanes) W->whist[s] = 0;
  x.sync();
  for (uint32_t s = x.lane; s < nw; s += x.nlanes) x.add(&W->whist[W->weights[s]], 1u);
  x.sync();
  uint32_t used = 0;
  for (uint32_t s = 0; s < 12u; ++s) used += W->whist[s] != 0u;
  uint32_t fse_bytes = 0;
  if (nw >= 2u && used >= 2u) {
    if (x.lane == 0) {
      mc_ze_fse *F = &W->fse[3];
      F->nsym = 12u;
      F->log = mc_ze_normalise(W->whist, 12u, nw, MC_ZSTD_W_LOG, F->norm);
      const uint32_t cb = mc_ze_write_counts(F->norm, 12u, F->log, P->wdesc + 1);
      mc_ze_build(F);
      // the chain, last weight first; a stream of at most 255 * 6 + 13 bits.  A
      // description that reaches MC_ZE_W_FSE_MAX bytes is dropped, and written no further
      mc_ze_bitw bw{P->wdesc + 1 + cb, 0, 0, 0};
      uint32_t st[2], bits;
      st[(nw - 1u) & 1u] = mc_ze_first(F, W->weights[nw - 1u]);
      st[(nw - 2u) & 1u] = mc_ze_first(F, W->weights[nw - 2u]);
      for (uint32_t i = nw - 2u; i-- > 0u && cb + bw.pos < MC_ZE_W_FSE_MAX;) {
        st[i & 1u] = mc_ze_encode(F, W->weights[i], st[i & 1u], &bits);
        bw.put(bits & 511u, bits >> 9);
      }
      bw.put(st[1], F->log);
      bw.put(st[0], F->log);
      bw.finish();
      P->wdesc_bytes = cb + bw.pos >= MC_ZE_W_FSE_MAX ? 0u : 1u + cb + bw.pos;
    }
    x.sync();
    fse_bytes = P->wdesc_bytes;
  }
  const uint32_t direct_bytes = nw <= 128u ? 1u + (nw + 1u) / 2u : 0u;
  uint32_t tree;
  if (direct_bytes && (fse_bytes == 0u || direct_bytes <= fse_bytes)) {
    tree = direct_bytes, *wform = MC_ZE_W_DIRECT;
    x.sync();
    for (uint32_t k = x.lane; k < direct_bytes; k += x.nlanes) {
      if (k == 0u) {
        P->wdesc[0] = (uint8_t)(127u + nw);
      } else {
        const uint32_t a = W->weights[2u * (k - 1u)], b = 2u * k - 1u < nw ? W->weights[2u * k - 1u] : 0u;
        P->wdesc[k] = (uint8_t)((a << 4) | b);
      }
    }
  } else if (fse_bytes) {
    tree = fse_bytes, *wform = MC_ZE_W_FSE;
    if (x.lane == 0) P->wdesc[0] = (uint8_t)(fse_bytes - 1u);
  } else {
    *wform = MC_ZE_W_NONE;
    return 0;
  }
  x.sync();
  // the streams
  const uint32_t ns = L < 256u ? 1u : 4u, share = ns == 1u ? L : (L + 3u) / 4u;
  uint32_t total = 0;
  for (uint32_t k = 0; k < 4u; ++k) {
    uint32_t bits = 0;
    if (k < ns) {
      const uint32_t from = k * share, to = (k + 1u == ns) ? L : from + share;
      for (uint32_t i = from + x.lane; i < to; i += x.nlanes) bits += P->lens[lits[i]];
      bits = x.sum(bits);
    }
    P->stream_bytes[k] = k < ns ? bits / 8u + 1u : 0u;  // (every lane the same word)
    total += P->stream_bytes[k];
  }
  const uint32_t comp = tree + (ns == 4u ? 6u : 0u) + total;
  const uint32_t lh = ns == 1u ? 3u : (L < 1024u && comp < 1024u) ? 3u : (L < 16384u && comp < 16384u) ? 4u : 5u;
  P->wdesc_bytes = tree, P->maxlen = ml, P->lit_header = lh, P->lit_comp = comp;
  *nstreams = ns;
  x.sync();
  return lh + comp;
}

// One of the three tables and its chain (one lane each): mode, description,
// encoding table, the bits between the sequences.  Returns the chain's bits
// with the first state's.
MC_ZSTD_HD uint32_t mc_ze_plan_table(uint32_t w, mc_ze_fse *F, const uint32_t *hist, const mc_ze_seq *seqs, uint32_t nseq,
                                     mc_ze_plan_out *P, mc_ze_trans *trans, uint32_t *mode) {
  const uint32_t *h = hist + mc_ze_hist_at(w);
  const uint32_t ncodes = mc_ze_ncodes(w);
  uint32_t used = 0, only = 0;
  for (uint32_t s = 0; s < ncodes; ++s)
    if (h[s]) ++used, only = s;
  if (used == 1u) {
    *mode = MC_ZE_RLE;
    F->log = 0, F->nsym = ncodes;
    P->tdesc[w][0] = (uint8_t)only, P->tdesc_bytes[w] = 1;
  } else {
    F->nsym = ncodes;
    F->log = mc_ze_normalise(h, ncodes, nseq, mc_ze_max_log(w), F->norm);
    const uint32_t db = mc_ze_write_counts(F->norm, ncodes, F->log, P->tdesc[w]);
    const uint32_t dn = mc_zstd_default_nsym(w), dl = mc_zstd_default_log(w);
    uint32_t cf = 2048u * db, cp = 0;
    bool reach = true;  // can the predefined table write every code in use?
    for (uint32_t s = 0; s < ncodes; ++s) {
      if (!h[s]) continue;
      cf += h[s] * (256u * F->log - mc_ze_log2q8((uint32_t)F->norm[s]));
      if (s >= dn) {
        reach = false;
      } else {
        const int32_t d = mc_zstd_default_count(w, s);
        cp += h[s] * (256u * dl - mc_ze_log2q8(d < 0 ? 1u : (uint32_t)d));
      }
    }
    if (reach && cp <= cf) {
      *mode = MC_ZE_PREDEFINED;
      F->nsym = dn, F->log = dl;
      for (uint32_t s = 0; s < dn; ++s) F->norm[s] = (int16_t)mc_zstd_default_count(w, s);
      P->tdesc_bytes[w] = 0;
    } else {
      *mode = MC_ZE_FSE;
      P->tdesc_bytes[w] = db;
    }
    mc_ze_build(F);
  }
  // the chain: the last sequence first
  uint32_t prev = nseq >= 2u ? seqs[nseq - 2u].a >> 16 : 0u;
  uint32_t st = mc_ze_first(F, mc_ze_pick(mc_ze_symbols(seqs[nseq - 1u], prev).c, w)), total = F->log;
  for (uint32_t q = nseq - 1u; q-- > 0u;) {
    const mc_ze_seq cur = seqs[q];
    prev = q ? seqs[q - 1u].a >> 16 : 0u;
    uint32_t bits;
    st = mc_ze_encode(F, mc_ze_pick(mc_ze_symbols(cur, prev).c, w), st, &bits);
    uint16_t *slot = w == 0 ? &trans[q].ll : w == 1 ? &trans[q].of : &trans[q].ml;
    *slot = (uint16_t)bits;
    total += bits >> 9;
  }
  P->log[w] = F->log, P->state0[w] = st;
  return total;
}

// A segment's block from its parse: the literals form, the modes, every size
// and the block type.  S: nseq, nlit, same filled; the rest is filled here
// (off excepted).  hist: MC_ZE_HIST words; lits: the literals; trans: nseq records.
template <class X>
MC_ZSTD_HD void mc_ze_plan(X &x, mc_ze_work *W, const uint32_t *hist, const uint8_t *lits, const mc_ze_seq *seqs,
                           uint32_t nk, mc_ze_seg *S, mc_ze_plan_out *P, mc_ze_trans *trans) {
  const uint32_t L = S->nlit, nseq = S->nseq;
  // ---- literals ----
  uint32_t distinct = 0;
  for (uint32_t s = x.lane; s < 256u; s += x.nlanes) distinct += hist[s] != 0u;
  distinct = x.sum(distinct);
  const uint32_t hb = mc_ze_lit_header(L);
  uint32_t form = MC_ZE_RAW, lit_bytes = hb + L, streams = 0, wform = MC_ZE_W_NONE;
  if (distinct >= 2u) {
    uint32_t ns = 0;
    const uint32_t hf = mc_ze_plan_huffman(x, W, hist, lits, L, P, &wform, &ns);
    if (hf && hf < lit_bytes) form = MC_ZE_COMPRESSED, lit_bytes = hf, streams = ns;
    else wform = MC_ZE_W_NONE;
  }
  // ---- sequences ----
  uint32_t seq_bytes = 1, extra = 0;
  S->mode[0] = S->mode[1] = S->mode[2] = 0;
  if (nseq) {
    for (uint32_t s = x.lane; s < 4u; s += x.nlanes) W->sbits[s] = 0;
    x.sync();
    for (uint32_t w = x.lane; w < 3u; w += x.nlanes) {
      uint32_t mode;
      W->sbits[w] = mc_ze_plan_table(w, &W->fse[w], hist, seqs, nseq, P, trans, &mode);
      W->whist[w] = mode;
    }
    for (uint32_t q = x.lane; q < nseq; q += x.nlanes) {
      const mc_ze_sym y = mc_ze_symbols(seqs[q], q ? seqs[q - 1u].a >> 16 : 0u);
      extra += y.xb[0] + y.xb[1] + y.xb[2];
    }
    extra = x.sum(extra);
    x.sync();
    const uint32_t bits = extra + W->sbits[0] + W->sbits[1] + W->sbits[2];
    for (uint32_t w = 0; w < 3u; ++w) S->mode[w] = W->whist[w];
    seq_bytes = mc_ze_nseq_bytes(nseq) + 1u + P->tdesc_bytes[0] + P->tdesc_bytes[1] + P->tdesc_bytes[2] + bits / 8u + 1u;
    P->seq_bits = bits;
  }
  S->lit_form = form, S->streams = streams, S->wdesc = wform;
  S->lit_bytes = lit_bytes, S->seq_bytes = seq_bytes;
  const uint32_t content = lit_bytes + seq_bytes;
  S->type = MC_ZE_RAW, S->bytes = 3u + nk;
  if (S->same && 4u < S->bytes) S->type = MC_ZE_RLE, S->bytes = 4u;
  if (content < nk && 3u + content < S->bytes) S->type = MC_ZE_COMPRESSED, S->bytes = 3u + content;
  S->reserved = 0;
}

// the canonical code of each literal byte as the decoder's table has it: code | length << 16
template <class X>
MC_ZSTD_HD void mc_ze_huf_codes(X &x, const uint8_t *lens, uint32_t maxlen, uint32_t *tab) {
  for (uint32_t s = x.lane; s < 256u; s += x.nlanes) {
    const uint32_t l = lens[s];
    uint32_t below = 0, rank = 0;  // cells of longer codes, in units of 2^-maxlen; equal codes before s
    if (l)
      for (uint32_t j = 0; j < 256u; ++j) {
        const uint32_t lj = lens[j];
        if (lj > l) below += 1u << (maxlen - lj);
        else if (lj == l && j < s) ++rank;
      }
    tab[s] = l ? ((below >> (maxlen - l)) + rank) | (l << 16) : 0u;
  }
  x.sync();
}
// the literals header of the compressed form: lh bytes
MC_ZSTD_HD uint64_t mc_ze_huf_header(uint32_t lh, uint32_t nstreams, uint32_t L, uint32_t comp) {
  if (lh == 3u) return 2u | ((nstreams == 1u ? 0u : 1u) << 2) | (L << 4) | (comp << 14);
  if (lh == 4u) return 2u | (2u << 2) | (L << 4) | ((uint64_t)comp << 18);
  return 2u | (3u << 2) | (L << 4) | ((uint64_t)comp << 22);
}
// the header of a raw literals section: mc_ze_lit_header(L) bytes
MC_ZSTD_HD uint32_t mc_ze_plain_header(uint32_t L) {
  return L < 32u ? L << 3 : L < 4096u ? (1u << 2) | (L << 4) : (3u << 2) | (L << 4);
}
// the bits of sequence q of the stream, lowest first: its extra bits (LL, ML,
// OF), then what the states read before it (OF, ML, LL) or, for q = 0, the
// first states (ML, OF, LL).  At most 48 bits in *lo and 26 in *hi.
MC_ZSTD_HD void mc_ze_seq_bits(const mc_ze_sym &y, uint32_t q, const mc_ze_trans *trans, const mc_ze_plan_out *P,
                               uint64_t *lo, uint32_t *nlo, uint32_t *hi, uint32_t *nhi) {
  uint64_t v = y.xv[0];
  uint32_t nb = y.xb[0];
  v |= (uint64_t)y.xv[2] << nb, nb += y.xb[2];
  v |= (uint64_t)y.xv[1] << nb, nb += y.xb[1];
  *lo = v, *nlo = nb;
  uint32_t h, nh;
  if (q) {
    const mc_ze_trans t = trans[q - 1u];
    h = t.of & 511u, nh = t.of >> 9;
    h |= (uint32_t)(t.ml & 511u) << nh, nh += t.ml >> 9;
    h |= (uint32_t)(t.ll & 511u) << nh, nh += t.ll >> 9;
  } else {
    h = P->state0[2], nh = P->log[2];
    h |= P->state0[1] << nh, nh += P->log[1];
    h |= P->state0[0] << nh, nh += P->log[0];
  }
  *hi = h, *nhi = nh;
}

// ---- the scalar model (host) ---------------------------------------------------------
// The parse of one segment: sequences, literals, histogram, repeat codes.
static inline void mc_ze_parse_segment(const uint8_t *src, uint32_t n, mc_ze_seq *seqs, uint8_t *lits, uint32_t *hist,
                                       mc_ze_seg *S) {
  uint32_t table[MC_ZE_TABLE];
  for (uint32_t i = 0; i < MC_ZE_TABLE; ++i) table[i] = 0;
  for (uint32_t i = 0; i < MC_ZE_HIST; ++i) hist[i] = 0;
  const uint32_t limit = n >= MC_ZE_MIN_MATCH ? n - (MC_ZE_MIN_MATCH - 1u) : 0u;  // slots own pos < limit
  uint32_t p = 0, anchor = 0, nseq = 0, nlit = 0, prev = 0, nrep = 0;
  while (p < limit) {
    const uint32_t wend = (limit - p < MC_ZE_WINDOW) ? limit : p + MC_ZE_WINDOW;
    uint32_t m = 0, c = 0;
    bool found = false;
    for (uint32_t pos = p; pos < wend && !found; ++pos) {
      const uint32_t w = mc_dfl_le32(src + pos);
      const uint32_t e = table[mc_dfl_hash(w)];
      if (mc_ze_entry_ok(e, pos) && mc_dfl_le32(src + (e - 1)) == w) m = pos, c = e - 1, found = true;
    }
    uint32_t consumed = wend;
    if (found) {
      while (m > anchor && c > 0 && src[m - 1] == src[c - 1]) --m, --c;
      uint32_t ml = MC_ZE_MIN_MATCH;
      while (m + ml < n && src[c + ml] == src[m + ml]) ++ml;
      const uint32_t lit = m - anchor, off = m - c;
      const mc_ze_seq s{lit | (off << 16), ml};
      const mc_ze_sym y = mc_ze_symbols(s, prev);
      nrep += y.c[1] == 0u;
      prev = off;
      seqs[nseq++] = s;
      for (uint32_t k = 0; k < lit; ++k) ++hist[src[anchor + k]], lits[nlit++] = src[anchor + k];
      for (uint32_t w = 0; w < 3u; ++w) ++hist[mc_ze_hist_at(w) + y.c[w]];
      if (m + ml < consumed) consumed = m + ml;
      anchor = m + ml;
    }
    for (uint32_t pos = p; pos < consumed; ++pos)  // ascending: the highest position wins an entry
      table[mc_dfl_hash(mc_dfl_le32(src + pos))] = pos + 1;
    p = found ? anchor : p + MC_ZE_WINDOW;
  }
  for (uint32_t k = anchor; k < n; ++k) ++hist[src[k]], lits[nlit++] = src[k];
  bool same = true;
  for (uint32_t k = 1; k < n && same; ++k) same = src[k] == src[0];
  S->nseq = nseq, S->nlit = nlit, S->same = same ? 1u : 0u, S->nrep = nrep;
}

// One planned segment into exactly S.bytes bytes at dst; the bytes written.
static inline uint32_t mc_ze_emit_segment(const uint8_t *src, uint32_t n, const mc_ze_seq *seqs, const uint8_t *lits,
                                          const mc_ze_trans *trans, const mc_ze_seg &S, const mc_ze_plan_out &P,
                                          uint32_t last, uint8_t *dst) {
  const uint32_t bh = mc_ze_block_header(last, S.type, S.type == MC_ZE_COMPRESSED ? S.bytes - 3u : n);
  dst[0] = (uint8_t)bh, dst[1] = (uint8_t)(bh >> 8), dst[2] = (uint8_t)(bh >> 16);
  uint32_t at = 3;
  if (S.type == MC_ZE_RAW) {
    for (uint32_t k = 0; k < n; ++k) dst[at++] = src[k];
    return at;
  }
  if (S.type == MC_ZE_RLE) {
    dst[at++] = src[0];
    return at;
  }
  const uint32_t L = S.nlit;
  if (S.lit_form != MC_ZE_COMPRESSED) {
    const uint32_t h = mc_ze_plain_header(L), hb = mc_ze_lit_header(L);
    for (uint32_t k = 0; k < hb; ++k) dst[at++] = (uint8_t)(h >> (8u * k));
    for (uint32_t k = 0; k < L; ++k) dst[at++] = lits[k];
  } else {
    mc_dfl_scalar x;
    uint32_t tab[256];
    mc_ze_huf_codes(x, P.lens, P.maxlen, tab);
    const uint64_t h = mc_ze_huf_header(P.lit_header, S.streams, L, P.lit_comp);
    for (uint32_t k = 0; k < P.lit_header; ++k) dst[at++] = (uint8_t)(h >> (8u * k));
    for (uint32_t k = 0; k < P.wdesc_bytes; ++k) dst[at++] = P.wdesc[k];
    if (S.streams == 4u)
      for (uint32_t k = 0; k < 3u; ++k) dst[at++] = (uint8_t)P.stream_bytes[k], dst[at++] = (uint8_t)(P.stream_bytes[k] >> 8);
    const uint32_t share = S.streams == 1u ? L : (L + 3u) / 4u;
    for (uint32_t k = 0; k < S.streams; ++k) {
      const uint32_t from = k * share, to = (k + 1u == S.streams) ? L : from + share;
      mc_ze_bitw bw{dst + at, 0, 0, 0};
      for (uint32_t i = to; i-- > from;) bw.put(tab[lits[i]] & 0xffffu, tab[lits[i]] >> 16);
      bw.finish();
      at += bw.pos;
    }
  }
  if (S.nseq == 0u) {
    dst[at++] = 0;
    return at;
  }
  if (S.nseq < 128u) dst[at++] = (uint8_t)S.nseq;
  else dst[at++] = (uint8_t)(128u + (S.nseq >> 8)), dst[at++] = (uint8_t)S.nseq;
  dst[at++] = (uint8_t)((S.mode[0] << 6) | (S.mode[1] << 4) | (S.mode[2] << 2));
  for (uint32_t w = 0; w < 3u; ++w)
    for (uint32_t k = 0; k < P.tdesc_bytes[w]; ++k) dst[at++] = P.tdesc[w][k];
  mc_ze_bitw bw{dst + at, 0, 0, 0};
  for (uint32_t q = S.nseq; q-- > 0u;) {
    const mc_ze_sym y = mc_ze_symbols(seqs[q], q ? seqs[q - 1u].a >> 16 : 0u);
    uint64_t lo;
    uint32_t nlo, hi, nhi;
    mc_ze_seq_bits(y, q, trans, &P, &lo, &nlo, &hi, &nhi);
    bw.put((uint32_t)lo, nlo < 32u ? nlo : 32u);
    if (nlo > 32u) bw.put((uint32_t)(lo >> 32), nlo - 32u);
    bw.put(hi, nhi);
  }
  bw.finish();
  return at + bw.pos;
}

// The scalar encoder (host): the frame of n source bytes into at most cap
// bytes at dst.  Returns the frame's size, or 0 when the chunk is refused
// (n == 0, n >= 2^30, or the frame would exceed cap): nothing is written then.
// *need (if given) = the frame's size either way.  segs (if given) receives
// one record per segment.  Two passes over the segments: the first only adds
// the sizes up.
static inline uint64_t mc_zstd_encode_chunk_report(const uint8_t *src, uint64_t n, uint8_t *dst, uint64_t cap,
                                                   uint32_t checksum, mc_ze_seg *segs, uint64_t *need) {
  if (need) *need = 0;
  if (n < 1 || n >= MC_ZE_MAX_BYTES) return 0;
  static thread_local mc_ze_seq seqs[MC_ZE_MAX_SEQS];
  static thread_local mc_ze_trans trans[MC_ZE_MAX_SEQS];
  static thread_local uint8_t lits[MC_ZE_SEGMENT];
  static thread_local mc_ze_work W;
  static thread_local mc_ze_plan_out P;
  uint32_t hist[MC_ZE_HIST];
  mc_dfl_scalar x;
  const uint32_t nseg = mc_ze_nsegments((uint32_t)n), head = mc_ze_header_bytes(n);
  uint64_t total = head;
  for (int emit = 0; emit < 2; ++emit) {
    uint32_t at = head;
    for (uint32_t k = 0; k < nseg; ++k) {
      const uint32_t nk = mc_ze_seg_len((uint32_t)n, k), last = k + 1 == nseg;
      const uint8_t *sp = src + (size_t)k * MC_ZE_SEGMENT;
      mc_ze_seg S;
      mc_ze_parse_segment(sp, nk, seqs, lits, hist, &S);
      mc_ze_plan(x, &W, hist, lits, seqs, nk, &S, &P, trans);
      S.off = at;
      if (emit) {
        if (mc_ze_emit_segment(sp, nk, seqs, lits, trans, S, P, last, dst + at) != S.bytes) return 0;  // never
        if (segs) segs[k] = S;
      }
      at += S.bytes;
    }
    if (!emit) {
      total = (uint64_t)at + (checksum ? 4u : 0u);
      if (need) *need = total;
      if (total > cap) return 0;
    } else {
      mc_ze_put_header(dst, (uint32_t)n, checksum);
      if (checksum) {
        const uint32_t h = (uint32_t)mc_xxh64(src, (uint32_t)n);
        for (uint32_t k = 0; k < 4u; ++k) dst[at + k] = (uint8_t)(h >> (8u * k));
      }
    }
  }
  return total;
}
static inline uint64_t mc_zstd_encode_chunk(const uint8_t *src, uint64_t n, uint8_t *dst, uint64_t cap, uint32_t checksum) {
  return mc_zstd_encode_chunk_report(src, n, dst, cap, checksum, (mc_ze_seg *)0, (uint64_t *)0);
}
