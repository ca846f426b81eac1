// mc_lz4_enc.h -- LZ4 block compression and Blosc1 frame assembly, shared by
// the gfx950 kernels (mc_blosc_enc.hip) and the host build of the CPU suite
// (tests/native_lz4enc).  The match-finding and emission rules are defined
// here once; mc_lz4_encode_stream below is their plain scalar statement, and
// the compress kernel produces the same bytes for every input.
//
// The model (one 64-lane wave per stream on the device):
//   * positions are consumed in windows of 64 starting at p; slot i of a
//     window owns pos = p + i while pos < n - 12 (no match may start in the
//     last 12 bytes of a block);
//   * a slot's candidate is table[hash(le32(src + pos))]: 4096 entries, each
//     the latest inserted position with that hash (stored as position + 1,
//     0 = empty).  Every lookup of a window sees the table as it was before
//     the window;
//   * a candidate is valid if it exists, cand < pos, pos - cand <= 65535 and
//     its 4-byte word equals the slot's; the lowest slot with a valid
//     candidate wins;
//   * the match is extended backwards while m > anchor, c > 0 and the
//     preceding bytes are equal, then forwards up to n - 5 (the last 5 bytes
//     are always literals);
//   * one sequence is emitted: the literals since anchor, the offset, the
//     match length;
//   * only the positions consumed from this window are then inserted:
//     p .. min(p + 64, match end) - 1 (all 64 when nothing matched), each
//     while it owns a slot; the highest position wins a shared entry.
//     (Inserting all 64 fills the table with positions ahead of the next p
//     and loses the short-distance matches of low-entropy byte planes.)
//   * p = anchor = match end, or p += 64 when nothing matched; the stream
//     ends with the remaining literals.
//
// Output bound: cap is the stream's uncompressed size.  The exact length of
// a sequence (token, both extension runs, literals, offset) is checked before
// any byte of it is written, the closing literals likewise; 0 ("store raw")
// is returned when the result would not be strictly smaller than n.  Nothing
// is written at or past dst + cap.  Streams shorter than 13 bytes are
// literals only and therefore stored raw.
#pragma once

#include "mc_lz4.h"

#define MC_LZ4E_HASH_BITS 12u
#define MC_LZ4E_TABLE (1u << MC_LZ4E_HASH_BITS)
#define MC_LZ4E_WINDOW 64u
#define MC_LZ4E_MFLIMIT 12u    // no match starts in the last 12 bytes
#define MC_LZ4E_LASTLITS 5u    // the last 5 bytes are literals
#define MC_LZ4E_MINLEN 13u     // shorter streams are literals only
#define MC_LZ4E_MAX_OFFSET 65535u

MC_LZ4_HD uint32_t mc_lz4e_hash(uint32_t w) { return (w * 2654435761u) >> (32u - MC_LZ4E_HASH_BITS); }

// a table entry (position + 1, 0 = empty) as a candidate for `pos`
MC_LZ4_HD bool mc_lz4e_entry_ok(uint32_t entry, uint32_t pos) {
  return entry != 0 && entry - 1 < pos && pos - (entry - 1) <= MC_LZ4E_MAX_OFFSET;
}

// extension bytes of a length whose 4-bit field holds min(v, 15)
MC_LZ4_HD uint32_t mc_lz4e_ext_count(uint32_t v) { return v >= 15 ? (v - 15) / 255 + 1 : 0; }
// extension byte k of count: 255 ... 255, (v - 15) % 255
MC_LZ4_HD uint8_t mc_lz4e_ext_byte(uint32_t v, uint32_t count, uint32_t k) {
  return k + 1 == count ? (uint8_t)((v - 15) % 255) : (uint8_t)255;
}
MC_LZ4_HD uint8_t mc_lz4e_token(uint32_t lit, uint32_t ml_minus4) {
  return (uint8_t)(((lit < 15 ? lit : 15u) << 4) | (ml_minus4 < 15 ? ml_minus4 : 15u));
}
// exact encoded length of a sequence / of the closing literals (lit, ml < 2^30)
MC_LZ4_HD uint32_t mc_lz4e_seq_bytes(uint32_t lit, uint32_t ml) {
  return 1 + mc_lz4e_ext_count(lit) + lit + 2 + mc_lz4e_ext_count(ml - 4);
}
MC_LZ4_HD uint32_t mc_lz4e_last_bytes(uint32_t lit) { return 1 + mc_lz4e_ext_count(lit) + lit; }

// What a caller that stitches streams needs to know of one (mc_lz4_codec.h);
// set when the encoder returns non-zero.
struct mc_lz4e_marks {
  uint32_t first_lit;  // literal length of the first sequence
  uint32_t close_at;   // offset of the closing (literal-only) sequence's token in dst
  uint32_t tail_lit;   // its literal length
};

// The scalar encoder (host): n source bytes into at most cap bytes at dst.
// Returns the compressed size, or 0 when the stream is to be stored raw.
static inline uint32_t mc_lz4_encode_stream_marks(const uint8_t *src, uint32_t n, uint8_t *dst, uint32_t cap,
                                                  mc_lz4e_marks *marks) {
  if (n < MC_LZ4E_MINLEN || n >= MC_LZ4_MAX_USIZE) return 0;
  uint32_t table[MC_LZ4E_TABLE];
  for (uint32_t i = 0; i < MC_LZ4E_TABLE; ++i) table[i] = 0;
  const uint32_t mflimit = n - MC_LZ4E_MFLIMIT, matchlimit = n - MC_LZ4E_LASTLITS;
  uint32_t p = 0, anchor = 0, op = 0;
  while (p < mflimit) {
    const uint32_t wend = (mflimit - p < MC_LZ4E_WINDOW) ? mflimit : p + MC_LZ4E_WINDOW;  // slots own [p, wend)
    uint32_t m = 0, c = 0;
    bool found = false;
    for (uint32_t pos = p; pos < wend && !found; ++pos) {
      const uint32_t w = mc_lz4_le32(src + pos);
      const uint32_t e = table[mc_lz4e_hash(w)];
      if (mc_lz4e_entry_ok(e, pos) && mc_lz4_le32(src + (e - 1)) == w) m = pos, c = e - 1, found = true;
    }
    uint32_t consumed = wend;
    if (found) {
      while (m > anchor && c > 0 && src[m - 1] == src[c - 1]) --m, --c;
      uint32_t ml = 4;
      while (m + ml < matchlimit && src[c + ml] == src[m + ml]) ++ml;
      // (the 4 bytes at the slot's position are equal, so this also covers a
      // backward-extended match: the loop runs over them again)
      const uint32_t lit = m - anchor, need = mc_lz4e_seq_bytes(lit, ml);
      if (need > cap - op) return 0;
      if (op == 0) marks->first_lit = lit;
      dst[op++] = mc_lz4e_token(lit, ml - 4);
      const uint32_t nle = mc_lz4e_ext_count(lit), nme = mc_lz4e_ext_count(ml - 4);
      for (uint32_t k = 0; k < nle; ++k) dst[op++] = mc_lz4e_ext_byte(lit, nle, k);
      for (uint32_t k = 0; k < lit; ++k) dst[op++] = src[anchor + k];
      dst[op++] = (uint8_t)((m - c) & 255u);
      dst[op++] = (uint8_t)((m - c) >> 8);
      for (uint32_t k = 0; k < nme; ++k) dst[op++] = mc_lz4e_ext_byte(ml - 4, nme, k);
      if (m + ml < consumed) consumed = m + ml;
      anchor = m + ml;
    }
    for (uint32_t pos = p; pos < consumed; ++pos)  // ascending: the highest position wins an entry
      table[mc_lz4e_hash(mc_lz4_le32(src + pos))] = pos + 1;
    p = found ? anchor : p + MC_LZ4E_WINDOW;
  }
  const uint32_t lit = n - anchor, need = mc_lz4e_last_bytes(lit);
  if (need > cap - op) return 0;
  marks->close_at = op, marks->tail_lit = lit;
  dst[op++] = mc_lz4e_token(lit, 0);
  const uint32_t nle = mc_lz4e_ext_count(lit);
  for (uint32_t k = 0; k < nle; ++k) dst[op++] = mc_lz4e_ext_byte(lit, nle, k);
  for (uint32_t k = 0; k < lit; ++k) dst[op++] = src[anchor + k];
  return op < n ? op : 0;
}
static inline uint32_t mc_lz4_encode_stream(const uint8_t *src, uint32_t n, uint8_t *dst, uint32_t cap) {
  mc_lz4e_marks marks;
  return mc_lz4_encode_stream_marks(src, n, dst, cap, &marks);
}

// ---------------------------------------------------------------------------
// Frame assembly.  One record of the batch's frame table (device table, one
// per frame with nbytes > 0): addresses are relative to the entry point's
// `src` base (0: absolute device addresses).
// ---------------------------------------------------------------------------
struct mc_blosc_enc_frame {
  uint64_t src;          // the frame's filtered (shuffled) bytes
  uint64_t raw;          // its unfiltered bytes (copied when the frame is memcpyed)
  uint64_t dst;          // device address of its output slot, nbytes + 16 bytes
  uint64_t scratch_off;  // its nbytes scratch bytes inside the workspace's scratch area
  uint32_t nbytes;
  uint32_t blocksize;
  uint32_t typesize;     // as written to the header (1 ... 255)
  uint32_t flags;        // header flags; MC_BLOSC_F_MEMCPYED forces a stored frame
  uint32_t block_base;   // index of the frame's first block / stream in the batch
  uint32_t stream_base;
};

#define MC_BLOSC_VERSION 2u
#define MC_BLOSC_VERSIONLZ 1u
#define MC_BLOSC_MAX_OVERHEAD 16u

// may this record be encoded at all?  (the kernels skip a frame that fails)
MC_LZ4_HD bool mc_blosc_enc_frame_ok(const mc_blosc_enc_frame &f, uint32_t nblocks_total, uint32_t nstreams_total,
                                     uint64_t scratch_bytes) {
  if (f.nbytes < 1 || f.nbytes > 0x7fffffffu || f.blocksize < 1 || f.blocksize >= MC_LZ4_MAX_USIZE) return false;
  if (f.typesize < 1 || f.typesize > 255) return false;
  if (mc_blosc_nsplit(f.flags, f.typesize, f.blocksize, f.blocksize) > 1 && f.blocksize % f.typesize) return false;
  if ((uint64_t)f.block_base + mc_blosc_nblocks(f.nbytes, f.blocksize) > nblocks_total) return false;
  if ((uint64_t)f.stream_base + mc_blosc_nstreams(f.flags, f.typesize, f.nbytes, f.blocksize) > nstreams_total)
    return false;
  if (f.flags & MC_BLOSC_F_MEMCPYED) return true;  // stored by request: no scratch
  return f.scratch_off <= scratch_bytes && f.nbytes <= scratch_bytes - f.scratch_off;
}

// stream `s` (counted inside the frame) -> its block, its offset in the
// frame's bytes and its size; s < mc_blosc_nstreams(...)
MC_LZ4_HD void mc_blosc_enc_stream(const mc_blosc_enc_frame &f, uint32_t s, uint32_t *block, uint32_t *first,
                                   uint32_t *off, uint32_t *neb) {
  const uint32_t nsplit = mc_blosc_nsplit(f.flags, f.typesize, f.blocksize, f.blocksize);
  const uint32_t nfull = f.nbytes / f.blocksize;
  if (s < nfull * nsplit) {
    const uint32_t b = s / nsplit, j = s - b * nsplit;
    *block = b, *first = j == 0, *neb = f.blocksize / nsplit;
    *off = b * f.blocksize + j * *neb;
  } else {  // the short last block: one stream
    *block = nfull, *first = 1, *neb = f.nbytes - nfull * f.blocksize;
    *off = nfull * f.blocksize;
  }
}

// bytes a stream takes in the frame: its cbytes word and its data (csize 0 = stored raw)
MC_LZ4_HD uint32_t mc_blosc_enc_stream_bytes(uint32_t csize, uint32_t neb) { return 4u + (csize ? csize : neb); }
// A frame whose compressed form (header, bstarts, streams) would exceed
// nbytes + 16 is stored: header + the unfiltered bytes.
MC_LZ4_HD bool mc_blosc_enc_memcpyed(const mc_blosc_enc_frame &f, uint64_t total) {
  return (f.flags & MC_BLOSC_F_MEMCPYED) || total > (uint64_t)f.nbytes + MC_BLOSC_MAX_OVERHEAD;
}
MC_LZ4_HD void mc_lz4e_put32(uint8_t *p, uint32_t v) {
  p[0] = (uint8_t)v, p[1] = (uint8_t)(v >> 8), p[2] = (uint8_t)(v >> 16), p[3] = (uint8_t)(v >> 24);
}
MC_LZ4_HD void mc_blosc_enc_header(uint8_t *dst, const mc_blosc_enc_frame &f, bool memcpyed, uint32_t cbytes) {
  dst[0] = MC_BLOSC_VERSION, dst[1] = MC_BLOSC_VERSIONLZ;
  dst[2] = (uint8_t)(f.flags | (memcpyed ? MC_BLOSC_F_MEMCPYED : 0u));
  dst[3] = (uint8_t)f.typesize;
  mc_lz4e_put32(dst + 4, f.nbytes);
  mc_lz4e_put32(dst + 8, f.blocksize);
  mc_lz4e_put32(dst + 12, cbytes);
}
