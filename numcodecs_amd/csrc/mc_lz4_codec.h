// mc_lz4_codec.h -- the `lz4` codec's container (numcodecs lz4.pyx): a 4-byte
// little-endian size followed by ONE LZ4 block for the whole chunk.  Shared by
// the gfx950 kernels (mc_lz4_codec.hip) and the host build of the CPU suite
// (tests/native_lz4codec).  The segmenting and stitching rules are defined
// here once; mc_lz4c_encode_chunk below is their plain scalar statement, and
// the kernels produce the same bytes for every input.
//
// Segments.  A chunk of n bytes is cut into segments of MC_LZ4C_SEGMENT =
// 65536 bytes (the last one shorter).  Each is compressed on its own by
// mc_lz4_enc.h's rules (mc_lz4_encode_stream / encode_wave, cap = its length):
// its matches never reach before its start, its last 5 bytes are literals and
// no match starts in its last 12 bytes -- so the final segment gives the block
// the ending the format requires.  A segment's result is either "no match /
// not smaller" (csize 0: all of it is literals) or a body of complete
// sequences followed by one closing literal-only sequence of tail_lit >= 5
// bytes, whose token stands at offset close_at of the segment's scratch.
//
// Stitch.  A segment's closing literals are not emitted there: they are
// carried into the literal run of the next body segment's first sequence.
// The carried run is always a contiguous source range that ends at that
// segment's start.  A segment without a match adds all its bytes to the carry.
// A body segment with incoming carry c and first literal length l0 becomes the
// piece
//     token(high nibble min(c + l0, 15), low nibble unchanged)
//     the extension bytes of c + l0
//     the source bytes [start - c, start + l0)
//     scratch[1 + ext(l0) + l0, close_at)   -- from the first sequence's
//                                              offset field on, unchanged
// and resets the carry to its tail_lit.  The block ends with token(carry, 0),
// the extension bytes of carry and the last `carry` source bytes.  Match
// offsets stay valid because distances inside a segment are preserved.
//
// Size bounds (both asserted by tests/test_lz4_host.py):
//   * the stitched block is never larger than the sum of the segments encoded
//     as independent blocks (a no-match segment as one literal-only block): a
//     merge removes a token and the ext(t) bytes of the run it absorbs and
//     adds at most ext(c + l0) - ext(l0) <= ext(t) + 1 bytes;
//   * it is at most n + n / 255 + 2 bytes, because csize < n_k for every body
//     segment; so a frame fits the reference's 4 + LZ4_compressBound(n) =
//     4 + n + n / 255 + 16 byte slot.
// The exact total is computed before a byte is written; a chunk whose frame
// would not fit its slot is refused (0) and nothing is written.
#pragma once

#include "mc_lz4_enc.h"

#define MC_LZ4C_SEGMENT 65536u
#define MC_LZ4C_HEADER 4u

MC_LZ4_HD uint32_t mc_lz4c_nsegments(uint32_t n) { return (n + MC_LZ4C_SEGMENT - 1) / MC_LZ4C_SEGMENT; }  // n < 2^30
MC_LZ4_HD uint32_t mc_lz4c_seg_len(uint32_t n, uint32_t k) {
  const uint32_t start = k * MC_LZ4C_SEGMENT;
  return n - start < MC_LZ4C_SEGMENT ? n - start : MC_LZ4C_SEGMENT;
}
// scratch offset of the first sequence's offset field (first literal length l0)
MC_LZ4_HD uint32_t mc_lz4c_body_skip(uint32_t l0) { return 1 + mc_lz4e_ext_count(l0) + l0; }
// bytes of a body segment's piece: the rewritten head, then scratch[skip, close_at)
MC_LZ4_HD uint32_t mc_lz4c_piece_bytes(uint32_t carry, uint32_t l0, uint32_t close_at) {
  return 1 + mc_lz4e_ext_count(carry + l0) + carry + l0 + (close_at - mc_lz4c_body_skip(l0));
}
// the rewritten first token: the literal nibble of `lit`, the first sequence's match nibble
MC_LZ4_HD uint8_t mc_lz4c_head_token(uint32_t lit, uint8_t first_token) {
  return (uint8_t)((mc_lz4e_token(lit, 0) & 0xF0u) | (first_token & 0x0Fu));
}
// the largest block of an n-byte chunk, and the slot the reference gives a frame
MC_LZ4_HD uint32_t mc_lz4c_block_bound(uint32_t n) { return n + n / 255 + 2; }
MC_LZ4_HD uint32_t mc_lz4c_frame_slot(uint32_t n) { return MC_LZ4C_HEADER + n + n / 255 + 16; }

// The scalar encoder (host): the LZ4 block of n source bytes into at most cap
// bytes at dst.  Returns the block's size, or 0 when the chunk is refused
// (n == 0, n >= 2^30, or the block would exceed cap): nothing is written then.
// Two passes over the segments: the first only adds the sizes up.
static inline uint32_t mc_lz4c_encode_chunk(const uint8_t *src, uint32_t n, uint8_t *dst, uint32_t cap) {
  if (n < 1 || n >= MC_LZ4_MAX_USIZE) return 0;
  uint8_t scratch[MC_LZ4C_SEGMENT];
  const uint32_t nseg = mc_lz4c_nsegments(n);
  for (int emit = 0; emit < 2; ++emit) {
    uint32_t carry = 0, op = 0;  // op <= n + n / 255 + 2 < 2^31
    for (uint32_t k = 0; k < nseg; ++k) {
      const uint32_t start = k * MC_LZ4C_SEGMENT, nk = mc_lz4c_seg_len(n, k);
      mc_lz4e_marks mk;
      if (mc_lz4_encode_stream_marks(src + start, nk, scratch, nk, &mk) == 0) {
        carry += nk;
        continue;
      }
      const uint32_t lit = carry + mk.first_lit, skip = mc_lz4c_body_skip(mk.first_lit);
      if (emit) {
        uint8_t *q = dst + op;
        *q++ = mc_lz4c_head_token(lit, scratch[0]);
        const uint32_t ne = mc_lz4e_ext_count(lit);
        for (uint32_t i = 0; i < ne; ++i) *q++ = mc_lz4e_ext_byte(lit, ne, i);
        for (uint32_t i = 0; i < lit; ++i) *q++ = src[start - carry + i];
        for (uint32_t i = skip; i < mk.close_at; ++i) *q++ = scratch[i];
      }
      op += mc_lz4c_piece_bytes(carry, mk.first_lit, mk.close_at);
      carry = mk.tail_lit;
    }
    if (emit) {
      uint8_t *q = dst + op;
      *q++ = mc_lz4e_token(carry, 0);
      const uint32_t ne = mc_lz4e_ext_count(carry);
      for (uint32_t i = 0; i < ne; ++i) *q++ = mc_lz4e_ext_byte(carry, ne, i);
      for (uint32_t i = 0; i < carry; ++i) *q++ = src[n - carry + i];
    }
    op += mc_lz4e_last_bytes(carry);
    if (emit) return op;
    if (op > cap) return 0;
  }
  return 0;
}

// the whole frame (size word + block) into at most cap bytes; its length or 0
static inline uint32_t mc_lz4c_encode_frame(const uint8_t *src, uint32_t n, uint8_t *dst, uint32_t cap) {
  if (cap < MC_LZ4C_HEADER) return 0;
  const uint32_t block = mc_lz4c_encode_chunk(src, n, dst + MC_LZ4C_HEADER, cap - MC_LZ4C_HEADER);
  if (block == 0) return 0;
  mc_lz4e_put32(dst, n);
  return MC_LZ4C_HEADER + block;
}

// ---------------------------------------------------------------------------
// Encode batch.  One record of the chunk table (device table, one per chunk
// with nbytes > 0): src is relative to the entry point's `src` base (0:
// absolute device addresses).
// ---------------------------------------------------------------------------
struct mc_lz4c_enc_chunk {
  uint64_t src;          // the chunk's bytes
  uint64_t dst;          // device address of its output slot (the frame)
  uint64_t scratch_off;  // its nbytes scratch bytes inside the workspace's scratch area
  uint32_t nbytes;
  uint32_t dst_cap;      // the slot's size; mc_lz4c_frame_slot(nbytes) always suffices
  uint32_t seg_base;     // index of the chunk's first segment in the batch
  uint32_t reserved;
};

// may this record be encoded at all?  (the kernels skip a chunk that fails)
MC_LZ4_HD bool mc_lz4c_enc_chunk_ok(const mc_lz4c_enc_chunk &c, uint32_t nsegments_total, uint64_t scratch_bytes) {
  if (c.nbytes < 1 || c.nbytes >= MC_LZ4_MAX_USIZE || c.dst_cap < MC_LZ4C_HEADER + 2) return false;
  if ((uint64_t)c.seg_base + mc_lz4c_nsegments(c.nbytes) > nsegments_total) return false;
  return c.scratch_off <= scratch_bytes && c.nbytes <= scratch_bytes - c.scratch_off;
}

// ---------------------------------------------------------------------------
// Decode batch.  One record of the chunk table, as the host read it from the
// frame's size word; the plan re-reads the word on the device.
// ---------------------------------------------------------------------------
struct mc_lz4c_dec_chunk {
  uint64_t src_off;  // the frame's first byte (its size word) in the concatenated frames
  uint64_t src_len;  // its length, size word included
  uint64_t dst;      // device address of its usize output bytes
  uint32_t usize;    // the size word
  uint32_t reserved;
};

// The plan: chunk i's stream descriptor.  0, or MC_LZ4_E_TABLE when the record
// contradicts itself, the frame's size word or the batch's max_usize (the
// descriptor is left invalid then and nothing is decoded).
MC_LZ4_HD int mc_lz4c_plan_chunk(const uint8_t *frames, const mc_lz4c_dec_chunk &c, uint32_t index,
                                 uint32_t max_usize, mc_lz4_stream *out) {
  out->src_off = 0, out->dst = 0, out->cbytes = 0, out->usize = 0, out->frame = index, out->flags = 0;
  if (c.src_len < MC_LZ4C_HEADER + 1 || c.src_len - MC_LZ4C_HEADER > 0x7fffffffu) return MC_LZ4_E_TABLE;
  if (c.usize < 1 || c.usize >= MC_LZ4_MAX_USIZE || c.usize > max_usize) return MC_LZ4_E_TABLE;
  if (mc_lz4_le32(frames + c.src_off) != c.usize) return MC_LZ4_E_TABLE;
  out->src_off = c.src_off + MC_LZ4C_HEADER;
  out->dst = c.dst;
  out->cbytes = (uint32_t)(c.src_len - MC_LZ4C_HEADER);
  out->usize = c.usize;
  out->flags = MC_LZ4_S_VALID;
  return MC_LZ4_OK;
}
