// mc_zstd.h -- the Zstandard frame format (RFC 8878): the rules, shared by the
// gfx950 kernels (mc_zstd.hip) and the host build of the CPU suite
// (tests/native_zstd).  The header parser, the frame walk, the bit readers,
// the table descriptions, the block walker and the sequence chain below are the
// very code that guards the device; the kernels only supply what is wave-wide
// there (the bit window, the table builders, the literal streams, the sink).
//
// Where the RFC leaves a choice the rules are libzstd's one-shot
// ZSTD_decompress (asked, 1.4.8, through tests/golden/make_golden_zstd.py):
//   * the reserved bit of the descriptor is refused, its unused bit and the two
//     reserved bits of the sequences' mode byte are ignored;
//   * a Window_Descriptor above 2^31 is refused, any other is accepted: without
//     a dictionary an offset is bounded by the bytes produced, not the window;
//   * a Huffman description needs an even number, at least 2, of weight-1
//     symbols; FSE-coded weights end when the bitstream overflows, and more
//     than 255 of them are refused;
//   * a 4-stream literals section needs 10 bytes and four non-empty streams;
//   * a repeat-mode table needs an earlier block of the frame with sequences, a
//     treeless literals section an earlier one with a Huffman tree;
//   * an overrun of the sequence bitstream is looked for before each sequence,
//     so the bits the last sequence takes from before the stream's start are
//     zeros, not an error; behind the last sequence the stream may hold no more
//     bits than one more update of the three states would take (libzstd makes
//     that update and wants the stream used up);
//   * a sequences section of count 0 is one byte long.
// Stricter than libzstd's one-shot call, as the RFC has it: a block may not
// regenerate more than Block_Maximum_Size, the Huffman code has at most 11
// bits, and a repeat offset that resolves to 0 is corrupt.
// What follows the frame: nothing, or MC_ZSTD_E_MEMBER for a further (or a
// leading skippable) frame, which the reference would skip or concatenate.
//
// The order of the verdicts is the reference's: the frame walk (header, block
// headers, checksum field, what follows) first, then a declared size of 0,
// then the dictionary, then the blocks, then the declared size and the checksum.
//
// Termination: the frame walk and the block loop advance by at least 3 bytes a
// pass and stop at the frame's end; the count reader ends when `remaining`
// reaches 1 or the symbols run out, and every pass lowers the one or raises
// the other; the weights' chain emits at most 255 symbols; a Huffman stream
// decodes exactly its share of Regenerated_Size, the sequence loop exactly
// Number_of_Sequences.  The bit readers yield zeros outside their stream
// without reading memory and report the overrun.  No source byte outside
// [0, src_len) is read, no destination byte outside [0, capacity) and no
// literal byte outside [0, 128 KiB) is written, and every table index is
// masked by the table's accuracy log or bounded by the symbol count the table
// was built from.
#pragma once

#include <stddef.h>
#include <stdint.h>

#ifndef MC_ZSTD_HD
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define MC_ZSTD_HD __host__ __device__ __forceinline__
#else
#define MC_ZSTD_HD inline
#endif
#endif

// a value every lane of the wave holds alike, moved to a scalar register
#if defined(__HIP_DEVICE_COMPILE__)
#define MC_ZSTD_UNI(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))
#else
#define MC_ZSTD_UNI(x) ((uint32_t)(x))
#endif

// error codes of the device error record / the host model (0 = none)
enum mc_zstd_error {
  MC_ZSTD_OK = 0,
  MC_ZSTD_E_HEADER = 1,    // the frame walk: magic, reserved bit, window, truncation, block type 3, junk behind
  MC_ZSTD_E_EMPTY = 2,     // a declared Frame_Content_Size of 0 (the reference refuses empty content)
  MC_ZSTD_E_DICT = 3,      // a non-zero Dictionary_ID
  MC_ZSTD_E_MEMBER = 4,    // a skippable frame first, or a further frame behind this one
  MC_ZSTD_E_CORRUPT = 5,   // a fault inside a block (libzstd: corruption_detected)
  MC_ZSTD_E_SRCSIZE = 6,   // a block or a sequences header of the wrong size (libzstd: srcSize_wrong)
  MC_ZSTD_E_CAPACITY = 7,  // the output would exceed the capacity (libzstd: dstSize_tooSmall)
  MC_ZSTD_E_CHECK = 8,     // the content checksum differs
  MC_ZSTD_E_SIZE = 9,      // fewer bytes than the declared Frame_Content_Size (libzstd: corruption_detected)
  MC_ZSTD_E_TABLE = 10,    // the caller's frame record is out of range
};

#define MC_ZSTD_MAGIC 0xFD2FB528u
#define MC_ZSTD_SKIP_MAGIC 0x184D2A50u  // the low nibble is free
#define MC_ZSTD_MAX_BYTES 0x40000000u   // frames and outputs are shorter than this
#define MC_ZSTD_BLOCK_MAX 131072u
#define MC_ZSTD_UNKNOWN 0xffffffffffffffffull  // no Frame_Content_Size

#define MC_ZSTD_HUF_LOG 11u
#define MC_ZSTD_LL_LOG 9u
#define MC_ZSTD_OF_LOG 8u
#define MC_ZSTD_ML_LOG 9u
#define MC_ZSTD_W_LOG 6u
#define MC_ZSTD_LL_MAX 35u  // the largest symbol
#define MC_ZSTD_OF_MAX 31u
#define MC_ZSTD_ML_MAX 52u

// an FSE entry: symbol | nbBits << 8 | baseline << 16; a Huffman entry: symbol | nbBits << 8
#define MC_ZSTD_FSE_ENTRY(sym, nb, base) ((uint32_t)(sym) | ((uint32_t)(nb) << 8) | ((uint32_t)(base) << 16))

// kinds of literals the sequences read
#define MC_ZSTD_LIT_RAW 0u  // frame bytes
#define MC_ZSTD_LIT_RLE 1u  // one byte, repeated
#define MC_ZSTD_LIT_BUF 2u  // the literals buffer (Huffman output)

// One frame of a batch (device table, one record per frame; include/mcodec.h):
// mc_inf_frame's layout, its `container` word reserved.
struct mc_zstd_frame {
  uint64_t src_off;
  uint64_t src_len;
  uint64_t dst;        // device address of the frame's output (decode only)
  uint32_t capacity;   // bytes dst holds
  uint32_t reserved;   // 0
};

#define MC_ZSTD_S_VALID 1u     // the frame walk passed: the decode and check kernels run
#define MC_ZSTD_S_CHECKSUM 2u  // a Content_Checksum follows the last block
#define MC_ZSTD_S_SIZED 4u     // Frame_Content_Size is declared (`content`)

// One stream, as the plan kernel leaves it for the decode and check kernels.
struct mc_zstd_stream {
  uint64_t src_off;
  uint64_t dst;
  uint32_t src_len;
  uint32_t data_off;   // the first block header, from the frame's start
  uint32_t capacity;
  uint32_t flags;      // MC_ZSTD_S_*
  uint32_t block_max;  // min(window, 128 KiB)
  uint32_t content;    // the declared size (below 2^30: larger ones exceed every capacity)
  uint32_t end_off;    // the byte behind the frame (behind the checksum)
  uint32_t pad;
};

struct mc_zstd_header {
  uint64_t content;  // MC_ZSTD_UNKNOWN: not declared
  uint64_t window;
  uint32_t data_off;
  uint32_t dict_id;
  uint32_t checksum;
  uint32_t block_max;
};

// The tables of a frame (LDS on the device).  ll / of / ml and huf persist from
// block to block (repeat mode, treeless literals); the rest is scratch of a build.
struct alignas(16) mc_zstd_tables {
  uint32_t ll[1u << MC_ZSTD_LL_LOG];
  uint32_t of[1u << MC_ZSTD_OF_LOG];
  uint32_t ml[1u << MC_ZSTD_ML_LOG];
  uint32_t wfse[1u << MC_ZSTD_W_LOG];  // the FSE table of the Huffman weights
  uint16_t huf[1u << MC_ZSTD_HUF_LOG];
  int16_t norm[256];    // normalized counts of the table being built
  uint16_t cum[260];    // running totals of the positive counts
  uint16_t next[256];   // the next state number of each symbol
  uint8_t weights[256];
  uint8_t hsym[256];    // the symbols in order of weight
};

MC_ZSTD_HD uint32_t mc_zstd_highbit(uint32_t v) { return 31u - (uint32_t)__builtin_clz(v); }  // v != 0

// ---- the frame header and the frame walk --------------------------------------
MC_ZSTD_HD uint32_t mc_zstd_le(const uint8_t *p, uint32_t bytes) {  // bytes <= 4
  uint32_t v = 0;
  for (uint32_t k = 0; k < bytes; ++k) v |= (uint32_t)p[k] << (8u * k);
  return v;
}

// The header of frame f[0, n).  Reads f only below n.
MC_ZSTD_HD int mc_zstd_parse_header(const uint8_t *f, uint64_t n, mc_zstd_header *h) {
  h->content = MC_ZSTD_UNKNOWN, h->window = 0, h->data_off = 0, h->dict_id = 0, h->checksum = 0, h->block_max = 0;
  if (n < 4) return MC_ZSTD_E_HEADER;
  const uint32_t magic = mc_zstd_le(f, 4);
  if ((magic & 0xfffffff0u) == MC_ZSTD_SKIP_MAGIC) return MC_ZSTD_E_MEMBER;
  if (magic != MC_ZSTD_MAGIC || n < 5) return MC_ZSTD_E_HEADER;
  const uint32_t fhd = f[4];
  const uint32_t fcs_flag = fhd >> 6, single = (fhd >> 5) & 1u, did_flag = fhd & 3u;
  if (fhd & 8u) return MC_ZSTD_E_HEADER;  // the reserved bit
  const uint32_t did_bytes = did_flag == 3u ? 4u : did_flag;
  const uint32_t fcs_bytes = fcs_flag == 0u ? single : 1u << fcs_flag;
  uint32_t p = 5;
  if (n < (uint64_t)p + (1u - single) + did_bytes + fcs_bytes) return MC_ZSTD_E_HEADER;
  if (!single) {
    const uint32_t b = f[p++], wlog = 10u + (b >> 3);
    if (wlog > 31u) return MC_ZSTD_E_HEADER;
    h->window = (1ull << wlog) + ((1ull << wlog) >> 3) * (b & 7u);
  }
  h->dict_id = mc_zstd_le(f + p, did_bytes);
  p += did_bytes;
  if (fcs_bytes) {
    uint64_t v = mc_zstd_le(f + p, fcs_bytes < 4u ? fcs_bytes : 4u);
    if (fcs_bytes == 8u) v |= (uint64_t)mc_zstd_le(f + p + 4, 4) << 32;
    if (fcs_bytes == 2u) v += 256u;
    h->content = v;
    p += fcs_bytes;
  }
  if (single) h->window = h->content;
  h->checksum = (fhd >> 2) & 1u;
  h->data_off = p;
  h->block_max = h->window < MC_ZSTD_BLOCK_MAX ? (uint32_t)h->window : MC_ZSTD_BLOCK_MAX;
  return MC_ZSTD_OK;
}

// The block headers from data_off to the last block, the checksum field and
// what follows the frame: *end = the byte behind the frame.
MC_ZSTD_HD int mc_zstd_walk(const uint8_t *f, uint64_t n, const mc_zstd_header *h, uint32_t *end) {
  uint64_t p = h->data_off;  // <= n
  *end = (uint32_t)p;
  for (;;) {
    if (n - p < 3) return MC_ZSTD_E_HEADER;
    const uint32_t bh = mc_zstd_le(f + p, 3);
    const uint32_t type = (bh >> 1) & 3u, size = bh >> 3;
    if (type == 3u) return MC_ZSTD_E_HEADER;
    const uint32_t held = type == 1u ? 1u : size;
    p += 3;
    if (n - p < held) return MC_ZSTD_E_HEADER;
    p += held;
    if (bh & 1u) break;
  }
  if (h->checksum) {
    if (n - p < 4) return MC_ZSTD_E_HEADER;
    p += 4;
  }
  *end = (uint32_t)p;  // p <= n < 2^30
  if (p == n) return MC_ZSTD_OK;
  if (n - p >= 4) {
    const uint32_t magic = mc_zstd_le(f + p, 4);
    if (magic == MC_ZSTD_MAGIC || (magic & 0xfffffff0u) == MC_ZSTD_SKIP_MAGIC) return MC_ZSTD_E_MEMBER;
  }
  return MC_ZSTD_E_HEADER;
}

// header + walk + the verdicts that come before the blocks, in the reference's order
MC_ZSTD_HD int mc_zstd_open(const uint8_t *f, uint64_t n, mc_zstd_header *h, uint32_t *end) {
  *end = 0;
  int e = mc_zstd_parse_header(f, n, h);
  if (e != MC_ZSTD_OK) return e;
  e = mc_zstd_walk(f, n, h, end);
  if (e != MC_ZSTD_OK) return e;
  if (h->content == 0) return MC_ZSTD_E_EMPTY;
  if (h->dict_id != 0) return MC_ZSTD_E_DICT;
  return MC_ZSTD_OK;
}

// ---- XXH64 ----------------------------------------------------------------------
#define MC_XXH_P1 0x9E3779B185EBCA87ull
#define MC_XXH_P2 0xC2B2AE3D27D4EB4Full
#define MC_XXH_P3 0x165667B19E3779F9ull
#define MC_XXH_P4 0x85EBCA77C2B2AE63ull
#define MC_XXH_P5 0x27D4EB2F165667C5ull
MC_ZSTD_HD uint64_t mc_xxh_rotl(uint64_t x, uint32_t r) { return (x << r) | (x >> (64u - r)); }
MC_ZSTD_HD uint64_t mc_xxh_round(uint64_t acc, uint64_t v) { return mc_xxh_rotl(acc + v * MC_XXH_P2, 31) * MC_XXH_P1; }
MC_ZSTD_HD uint64_t mc_xxh_merge(uint64_t h, uint64_t acc) { return (h ^ mc_xxh_round(0, acc)) * MC_XXH_P1 + MC_XXH_P4; }
MC_ZSTD_HD uint64_t mc_xxh_le64(const uint8_t *p) {
  uint64_t v = 0;
  for (uint32_t k = 0; k < 8; ++k) v |= (uint64_t)p[k] << (8u * k);
  return v;
}
MC_ZSTD_HD uint64_t mc_xxh_seed(uint32_t k) {  // accumulator k of seed 0
  return k == 0 ? MC_XXH_P1 + MC_XXH_P2 : k == 1 ? MC_XXH_P2 : k == 2 ? 0ull : 0ull - MC_XXH_P1;
}
// from the four accumulators (n >= 32) or none, over the tail p[done, n)
MC_ZSTD_HD uint64_t mc_xxh_finish(const uint64_t *acc, const uint8_t *p, uint32_t done, uint32_t n) {
  uint64_t h;
  if (n >= 32u) {
    h = mc_xxh_rotl(acc[0], 1) + mc_xxh_rotl(acc[1], 7) + mc_xxh_rotl(acc[2], 12) + mc_xxh_rotl(acc[3], 18);
    for (uint32_t k = 0; k < 4; ++k) h = mc_xxh_merge(h, acc[k]);
  } else {
    h = MC_XXH_P5;
  }
  h += n;
  uint32_t i = done;
  for (; n - i >= 8u; i += 8) h = mc_xxh_rotl(h ^ mc_xxh_round(0, mc_xxh_le64(p + i)), 27) * MC_XXH_P1 + MC_XXH_P4;
  if (n - i >= 4u) {
    h = mc_xxh_rotl(h ^ ((uint64_t)mc_zstd_le(p + i, 4) * MC_XXH_P1), 23) * MC_XXH_P2 + MC_XXH_P3;
    i += 4;
  }
  for (; i < n; ++i) h = mc_xxh_rotl(h ^ (p[i] * MC_XXH_P5), 11) * MC_XXH_P1;
  h ^= h >> 33;
  h *= MC_XXH_P2;
  h ^= h >> 29;
  h *= MC_XXH_P3;
  h ^= h >> 32;
  return h;
}
MC_ZSTD_HD uint64_t mc_xxh64(const uint8_t *p, uint32_t n) {
  uint64_t acc[4];
  for (uint32_t k = 0; k < 4; ++k) acc[k] = mc_xxh_seed(k);
  uint32_t i = 0;
  if (n >= 32u)
    for (; n - i >= 32u; i += 32)
      for (uint32_t k = 0; k < 4; ++k) acc[k] = mc_xxh_round(acc[k], mc_xxh_le64(p + i + 8u * k));
  return mc_xxh_finish(acc, p, i, n);
}

// What the check stage decides: the declared size, then the checksum at end_off - 4.
MC_ZSTD_HD int mc_zstd_check(const uint8_t *f, uint32_t flags, uint32_t content, uint32_t end_off, uint32_t produced,
                             uint32_t check) {
  if ((flags & MC_ZSTD_S_SIZED) && produced != content) return MC_ZSTD_E_SIZE;
  if ((flags & MC_ZSTD_S_CHECKSUM) && mc_zstd_le(f + end_off - 4u, 4) != check) return MC_ZSTD_E_CHECK;
  return MC_ZSTD_OK;
}

// ---- bit sources ----------------------------------------------------------------
// A source answers bits64(lo): the frame's bits [lo, lo + 64), bit k of the
// frame being bit k % 8 of byte k / 8, bytes outside [0, n) as zeros (never read).
struct mc_zstd_mem_src {
  const uint8_t *p;
  uint32_t n;
  MC_ZSTD_HD uint64_t bits64(uint64_t lo) const {
    const uint64_t b = lo >> 3;
    const uint32_t sh = (uint32_t)lo & 7u;
    uint64_t v = 0;
    uint32_t top = 0;
    if (b + 9 <= n) {
      __builtin_memcpy(&v, p + b, 8);
      top = p[b + 8];
    } else {
      for (uint32_t k = 0; k < 8; ++k)
        if (b + k < n) v |= (uint64_t)p[b + k] << (8u * k);
      if (b + 8 < n) top = p[b + 8];
    }
    return sh ? (v >> sh) | ((uint64_t)top << (64u - sh)) : v;
  }
};

// A backward bitstream over frame bytes [start, end): `left` bits are unread,
// the next one to read is bit left - 1 of the stream.  Bits from before the
// stream's start are zeros; overrun() reports that some were taken.
template <class Src>
struct mc_zstd_rbits {
  Src &src;
  uint32_t start;
  int32_t left;
  MC_ZSTD_HD mc_zstd_rbits(Src &s) : src(s), start(0), left(0) {}
  // false: the stream is empty or its last byte, which holds the final-bit marker, is zero
  MC_ZSTD_HD bool open(uint32_t start_, uint32_t end, uint32_t last_byte) {
    start = start_;
    left = 0;
    if (end <= start_ || last_byte == 0) return false;
    left = (int32_t)(8u * (end - start_ - 1u) + mc_zstd_highbit(last_byte));
    return true;
  }
  // the next 64 bits, the first one to read on top
  MC_ZSTD_HD uint64_t peek64() const {
    if (left <= 0) return 0;
    if (left >= 64) return src.bits64(8ull * start + (uint32_t)(left - 64));
    // bits [0, left) of the stream, moved to the top: nothing below the start is looked at
    return src.bits64(8ull * start) << (64u - (uint32_t)left);
  }
  MC_ZSTD_HD void drop(uint32_t k) { left -= (int32_t)k; }
  MC_ZSTD_HD uint32_t read(uint32_t k) {  // k <= 32
    const uint64_t v = peek64();
    drop(k);
    return k ? (uint32_t)(v >> (64u - k)) : 0u;
  }
  MC_ZSTD_HD bool overrun() const { return left < 0; }
};

// A forward bit reader over frame bytes [pos, end), for the count descriptions.
struct mc_zstd_fbits {
  const uint8_t *f;
  uint32_t pos, end, used;  // used: bits taken
  MC_ZSTD_HD uint32_t peek(uint32_t k) const {  // k <= 16; bytes at and past end as zeros
    uint32_t v = 0;
    const uint32_t b = pos + (used >> 3);
    for (uint32_t i = 0; i < 3; ++i)
      if (b + i < end) v |= (uint32_t)f[b + i] << (8u * i);
    return (v >> (used & 7u)) & ((1u << k) - 1u);
  }
  MC_ZSTD_HD void drop(uint32_t k) { used += k; }
  MC_ZSTD_HD bool overrun() const { return used > 8u * (end - pos); }
  MC_ZSTD_HD uint32_t bytes() const { return (used + 7u) >> 3; }
};

// An FSE table description at f[pos, end): the normalized counts of symbols
// [0, *nsym) into norm[], the accuracy log, the bytes it takes.  0 or corrupt.
MC_ZSTD_HD int mc_zstd_read_counts(const uint8_t *f, uint32_t pos, uint32_t end, uint32_t max_log, uint32_t max_sym,
                                   int16_t *norm, uint32_t *log, uint32_t *nsym, uint32_t *bytes) {
  mc_zstd_fbits br{f, pos, end, 0u};
  const uint32_t al = br.peek(4) + 5u;
  br.drop(4);
  if (al > max_log) return MC_ZSTD_E_CORRUPT;
  int32_t remaining = (int32_t)(1u << al) + 1, threshold = (int32_t)(1u << al);
  uint32_t nb = al + 1u, sym = 0;
  bool prev0 = false;
  while (remaining > 1 && sym <= max_sym) {
    if (prev0) {
      uint32_t n0 = sym;
      for (;;) {  // two-bit repeat flags: every pass raises n0 or ends
        const uint32_t r = br.peek(2);
        br.drop(2);
        n0 += r;
        if (r != 3u || n0 > max_sym) break;
      }
      if (n0 > max_sym) return MC_ZSTD_E_CORRUPT;
      while (sym < n0) norm[sym++] = 0;
      prev0 = false;
      // (the next value belongs to symbol n0 <= max_sym)
    }
    const int32_t max = (2 * threshold - 1) - remaining;
    const uint32_t v = br.peek(nb);
    int32_t count;
    if ((int32_t)(v & (uint32_t)(threshold - 1)) < max) {
      count = (int32_t)(v & (uint32_t)(threshold - 1));
      br.drop(nb - 1u);
    } else {
      count = (int32_t)(v & (uint32_t)(2 * threshold - 1));
      if (count >= threshold) count -= max;
      br.drop(nb);
    }
    --count;  // -1: "less than 1"
    remaining -= count < 0 ? -count : count;
    norm[sym++] = (int16_t)count;
    prev0 = count == 0;
    while (remaining < threshold) {
      --nb;
      threshold >>= 1;
    }
    if (br.overrun()) return MC_ZSTD_E_CORRUPT;
  }
  if (remaining != 1 || br.overrun()) return MC_ZSTD_E_CORRUPT;
  *log = al, *nsym = sym, *bytes = br.bytes();
  return MC_ZSTD_OK;
}

// the predefined distributions (RFC 8878, 3.1.1.3.2.2)
MC_ZSTD_HD int32_t mc_zstd_default_count(uint32_t which, uint32_t s) {  // 0 LL, 1 OF, 2 ML
  static constexpr int8_t ll[36] = {4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2,
                                    2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1};
  static constexpr int8_t of[29] = {1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1};
  static constexpr int8_t ml[53] = {1, 4, 3, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
                                    1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1, -1, -1};
  return which == 0 ? ll[s] : which == 1 ? of[s] : ml[s];
}
MC_ZSTD_HD uint32_t mc_zstd_default_nsym(uint32_t which) { return which == 0 ? 36u : which == 1 ? 29u : 53u; }
MC_ZSTD_HD uint32_t mc_zstd_default_log(uint32_t which) { return which == 1 ? 5u : 6u; }

// baseline and extra bits of a literal-length code (<= 35) and a match-length code (<= 52)
MC_ZSTD_HD uint32_t mc_zstd_ll_bits(uint32_t c) {
  static constexpr uint8_t t[20] = {1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};
  return c < 16u ? 0u : t[c - 16u];
}
MC_ZSTD_HD uint32_t mc_zstd_ll_base(uint32_t c) {
  static constexpr uint32_t t[20] = {16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536};
  return c < 16u ? c : t[c - 16u];
}
MC_ZSTD_HD uint32_t mc_zstd_ml_bits(uint32_t c) {
  static constexpr uint8_t t[21] = {1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};
  return c < 32u ? 0u : t[c - 32u];
}
MC_ZSTD_HD uint32_t mc_zstd_ml_base(uint32_t c) {
  static constexpr uint32_t t[21] = {35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387, 32771, 65539};
  return c < 32u ? c + 3u : t[c - 32u];
}

// ---- table rules shared by the scalar and the wave builder ----------------------
MC_ZSTD_HD uint32_t mc_zstd_fse_step(uint32_t log) { return (1u << log >> 1) + (1u << log >> 3) + 3u; }
// the entry of a cell holding symbol s as that symbol's state number ns (norm[s] <= ns < 2 norm[s])
MC_ZSTD_HD uint32_t mc_zstd_fse_cell(uint32_t s, uint32_t ns, uint32_t log) {
  const uint32_t nb = log - mc_zstd_highbit(ns);
  return MC_ZSTD_FSE_ENTRY(s, nb, (ns << nb) - (1u << log));
}

// The weights of a Huffman description, checked from their counts (count[w] =
// weights equal to w for w <= 11, count[12] = larger ones; the builder's
// weigh()): the implied last weight is appended (weights[n]) and counted, *log
// = the code's longest length.  0 or corrupt.
MC_ZSTD_HD int mc_zstd_check_weights(uint8_t *weights, uint32_t n, uint32_t *log, uint32_t *count) {
  if (count[12]) return MC_ZSTD_E_CORRUPT;
  uint32_t total = 0;
#pragma unroll
  for (uint32_t w = 1; w <= MC_ZSTD_HUF_LOG; ++w) total += count[w] << (w - 1u);
  if (total == 0) return MC_ZSTD_E_CORRUPT;
  const uint32_t tl = mc_zstd_highbit(total) + 1u;
  if (tl > MC_ZSTD_HUF_LOG) return MC_ZSTD_E_CORRUPT;
  const uint32_t rest = (1u << tl) - total;  // >= 1
  if (rest & (rest - 1u)) return MC_ZSTD_E_CORRUPT;
  const uint32_t last = mc_zstd_highbit(rest) + 1u;  // <= tl
  weights[n] = (uint8_t)last;  // (every lane the same byte)
#pragma unroll
  for (uint32_t w = 1; w <= MC_ZSTD_HUF_LOG; ++w) count[w] += w == last ? 1u : 0u;
  if (count[1] < 2u || (count[1] & 1u)) return MC_ZSTD_E_CORRUPT;
  *log = tl;
  return MC_ZSTD_OK;
}

// the host's builder: scalar
struct mc_zstd_scalar_builder {
  MC_ZSTD_HD void sync() {}
  // norm[0, nsym) -> table[0, 1 << log)
  MC_ZSTD_HD void fse(mc_zstd_tables *T, uint32_t *table, uint32_t nsym, uint32_t log) {
    const uint32_t size = 1u << log, mask = size - 1u, step = mc_zstd_fse_step(log);
    uint32_t high = size - 1u;
    for (uint32_t s = 0; s < nsym; ++s) {
      if (T->norm[s] == -1) {
        table[high--] = s;
        T->next[s] = 1;
      } else {
        T->next[s] = (uint16_t)T->norm[s];
      }
    }
    uint32_t pos = 0;
    for (uint32_t s = 0; s < nsym; ++s)
      for (int32_t i = 0; i < T->norm[s]; ++i) {
        table[pos] = s;
        do pos = (pos + step) & mask; while (pos > high);
      }
    for (uint32_t u = 0; u < size; ++u) {
      const uint32_t s = table[u] & 255u;
      table[u] = mc_zstd_fse_cell(s, T->next[s]++, log);
    }
  }
  MC_ZSTD_HD void fse_rle(uint32_t *table, uint32_t sym) { table[0] = MC_ZSTD_FSE_ENTRY(sym, 0, 0); }
  // count[w] = weights equal to w (w <= 11), count[12] = larger ones
  MC_ZSTD_HD void weigh(const uint8_t *weights, uint32_t n, uint32_t *count) {
    for (uint32_t w = 0; w < 13; ++w) count[w] = 0;
    for (uint32_t s = 0; s < n; ++s) ++count[weights[s] < 12u ? weights[s] : 12u];
  }
  // weights[0, nsym) (checked, count[] theirs) -> huf[0, 1 << log)
  MC_ZSTD_HD void huf(mc_zstd_tables *T, uint32_t nsym, uint32_t log, const uint32_t *count) {
    uint32_t start[13];
    start[1] = 0;
    for (uint32_t w = 1; w < 12; ++w) start[w + 1] = start[w] + (count[w] << (w - 1u));
    for (uint32_t s = 0; s < nsym; ++s) {
      const uint32_t w = T->weights[s];
      if (!w) continue;
      const uint32_t len = 1u << (w - 1u);
      for (uint32_t k = 0; k < len; ++k) T->huf[start[w] + k] = (uint16_t)(s | ((log + 1u - w) << 8));
      start[w] += len;
    }
  }
};

// ---- Huffman ----------------------------------------------------------------------
// The weights of a tree description at f[pos, end) into T->weights: *nw of
// them, *bytes taken.  FSE-coded weights run the two-state chain here (serial
// by nature, at most 255 symbols), through the builder's table.
template <class Builder>
MC_ZSTD_HD int mc_zstd_read_weights(const uint8_t *f, uint32_t n, uint32_t pos, uint32_t end, Builder &bld,
                                    mc_zstd_tables *T, uint32_t *nw, uint32_t *bytes) {
  if (pos >= end) return MC_ZSTD_E_CORRUPT;
  const uint32_t hb = f[pos];
  if (hb >= 128u) {  // direct: 4 bits each, the high nibble first
    const uint32_t cnt = hb - 127u, held = (cnt + 1u) >> 1;
    if (held + 1u > end - pos) return MC_ZSTD_E_CORRUPT;
    bld.sync();
    for (uint32_t k = 0; k < cnt; ++k) {
      const uint32_t b = f[pos + 1u + (k >> 1)];
      T->weights[k] = (uint8_t)((k & 1u) ? b & 15u : b >> 4);
    }
    bld.sync();
    *nw = cnt, *bytes = held + 1u;
    return MC_ZSTD_OK;
  }
  if (hb + 1u > end - pos) return MC_ZSTD_E_CORRUPT;
  const uint32_t s0 = pos + 1u, s1 = s0 + hb;
  uint32_t log, nsym, cb;
  bld.sync();
  int e = mc_zstd_read_counts(f, s0, s1, MC_ZSTD_W_LOG, 255u, T->norm, &log, &nsym, &cb);
  if (e != MC_ZSTD_OK) return e;
  bld.sync();
  bld.fse(T, T->wfse, nsym, log);
  bld.sync();
  mc_zstd_mem_src src{f, n};
  mc_zstd_rbits<mc_zstd_mem_src> br(src);
  if (s0 + cb >= s1 || !br.open(s0 + cb, s1, f[s1 - 1u])) return MC_ZSTD_E_CORRUPT;
  const uint32_t mask = (1u << log) - 1u;
  uint32_t st[2];
  st[0] = br.read(log);
  st[1] = br.read(log);
  uint32_t cnt = 0, k = 0;
  for (;;) {  // emit, update; on overflow the other state's symbol ends it
    if (cnt > 253u) return MC_ZSTD_E_CORRUPT;
    const uint32_t en = MC_ZSTD_UNI(T->wfse[st[k] & mask]);
    T->weights[cnt++] = (uint8_t)en;
    st[k] = (en >> 16) + br.read((en >> 8) & 255u);
    if (br.overrun()) {
      T->weights[cnt++] = (uint8_t)MC_ZSTD_UNI(T->wfse[st[k ^ 1u] & mask]);
      break;
    }
    k ^= 1u;
  }
  bld.sync();
  *nw = cnt, *bytes = hb + 1u;
  return MC_ZSTD_OK;
}

// One Huffman stream f[start, end) of `count` symbols: put(i, byte) for each.
// 0, or corrupt when the stream does not end exactly at its start.
template <class Put>
MC_ZSTD_HD int mc_zstd_huf_stream(const uint8_t *f, uint32_t n, uint32_t start, uint32_t end, const uint16_t *huf,
                                  uint32_t log, uint32_t count, Put &put) {
  mc_zstd_mem_src src{f, n};
  mc_zstd_rbits<mc_zstd_mem_src> br(src);
  if (end <= start || !br.open(start, end, f[end - 1u])) return MC_ZSTD_E_CORRUPT;
  uint32_t i = 0;
  while (i < count) {
    const uint64_t v = br.peek64();
    uint32_t used = 0;
    for (uint32_t k = 0; k < 5u && i < count; ++k, ++i) {  // 5 codes of <= 11 bits out of 64
      const uint32_t en = huf[(uint32_t)((v << used) >> (64u - log))];  // an index below 1 << log
      put(i, en & 255u);
      used += en >> 8;
    }
    br.drop(used);
  }
  return br.left == 0 ? MC_ZSTD_OK : MC_ZSTD_E_CORRUPT;
}

// ---- the block walker ---------------------------------------------------------------
// What the walker keeps from block to block.
struct mc_zstd_state {
  uint32_t rep[3];
  uint32_t ll_log, of_log, ml_log, huf_log;
  uint32_t have_huf, have_fse;
};

// the four (or one) streams of a compressed literals section
struct mc_zstd_lit_streams {
  uint32_t nstreams;
  uint32_t start[4], end[4];  // frame bytes
  uint32_t out[4], len[4];    // their shares of the literals buffer
};

// One of the three sequence tables.  which: 0 LL, 1 OF, 2 ML.
template <class Builder>
MC_ZSTD_HD int mc_zstd_seq_table(const uint8_t *f, uint32_t *pos, uint32_t end, uint32_t mode, uint32_t which,
                                 Builder &bld, mc_zstd_tables *T, mc_zstd_state *S) {
  uint32_t *table = which == 0 ? T->ll : which == 1 ? T->of : T->ml;
  uint32_t *log = which == 0 ? &S->ll_log : which == 1 ? &S->of_log : &S->ml_log;
  const uint32_t max_sym = which == 0 ? MC_ZSTD_LL_MAX : which == 1 ? MC_ZSTD_OF_MAX : MC_ZSTD_ML_MAX;
  const uint32_t max_log = which == 0 ? MC_ZSTD_LL_LOG : which == 1 ? MC_ZSTD_OF_LOG : MC_ZSTD_ML_LOG;
  if (mode == 3u) return S->have_fse ? MC_ZSTD_OK : MC_ZSTD_E_CORRUPT;
  bld.sync();
  if (mode == 1u) {
    if (*pos >= end) return MC_ZSTD_E_SRCSIZE;
    const uint32_t sym = f[(*pos)++];
    if (sym > max_sym) return MC_ZSTD_E_CORRUPT;
    bld.fse_rle(table, sym);
    *log = 0;
    bld.sync();
    return MC_ZSTD_OK;
  }
  uint32_t nsym;
  if (mode == 0u) {
    nsym = mc_zstd_default_nsym(which);
    for (uint32_t s = 0; s < nsym; ++s) T->norm[s] = (int16_t)mc_zstd_default_count(which, s);
    *log = mc_zstd_default_log(which);
  } else {
    uint32_t bytes;
    const int e = mc_zstd_read_counts(f, *pos, end, max_log, max_sym, T->norm, log, &nsym, &bytes);
    if (e != MC_ZSTD_OK) return e;
    *pos += bytes;
  }
  bld.sync();
  bld.fse(T, table, nsym, *log);
  bld.sync();
  return MC_ZSTD_OK;
}

// The sequences of one block: nseq of them from the bitstream f[pos, end),
// executed through the sink.  lit_*: the block's literals.
template <class Src, class Sink>
MC_ZSTD_HD int mc_zstd_sequences(Src &src, Sink &out, const uint8_t *f, uint32_t pos, uint32_t end, uint32_t nseq,
                                 const mc_zstd_tables *T, mc_zstd_state *S, uint32_t lit_kind, uint32_t lit_at,
                                 uint32_t lit_left) {
  mc_zstd_rbits<Src> br(src);
  if (end <= pos || !br.open(pos, end, f[end - 1u])) return MC_ZSTD_E_CORRUPT;
  const uint32_t ll_mask = (1u << S->ll_log) - 1u, of_mask = (1u << S->of_log) - 1u, ml_mask = (1u << S->ml_log) - 1u;
  uint32_t st_ll = br.read(S->ll_log), st_of = br.read(S->of_log), st_ml = br.read(S->ml_log);
  uint32_t rep0 = S->rep[0], rep1 = S->rep[1], rep2 = S->rep[2];
  for (uint32_t i = 0; i < nseq; ++i) {
    if (br.overrun()) return MC_ZSTD_E_CORRUPT;
    const uint32_t e_ll = MC_ZSTD_UNI(T->ll[st_ll & ll_mask]), e_of = MC_ZSTD_UNI(T->of[st_of & of_mask]);
    const uint32_t e_ml = MC_ZSTD_UNI(T->ml[st_ml & ml_mask]);
    const uint32_t c_ll = e_ll & 255u, c_of = e_of & 255u, c_ml = e_ml & 255u;  // <= 35, 31, 52: the tables' symbols
    const uint32_t b_ll = mc_zstd_ll_bits(c_ll), b_ml = mc_zstd_ml_bits(c_ml);
    uint64_t v = br.peek64();  // offset, match length, literal length: at most 31 + 16 + 16 bits
    uint32_t ov = c_of ? (uint32_t)(v >> (64u - c_of)) : 0u;
    v = c_of ? v << c_of : v;
    const uint32_t ml = mc_zstd_ml_base(c_ml) + (b_ml ? (uint32_t)(v >> (64u - b_ml)) : 0u);
    v = b_ml ? v << b_ml : v;
    const uint32_t ll = mc_zstd_ll_base(c_ll) + (b_ll ? (uint32_t)(v >> (64u - b_ll)) : 0u);
    br.drop(c_of + b_ml + b_ll);
    uint32_t offset;
    if (c_of >= 2u) {  // Offset_Value - 3
      offset = (1u << c_of) + ov - 3u;
      rep2 = rep1, rep1 = rep0, rep0 = offset;
    } else {
      const uint32_t idx = (c_of ? 1u + ov : 0u) + (ll == 0u ? 1u : 0u);  // 0..3: rep1, rep2, rep3, rep1 - 1
      if (idx == 0u) {
        offset = rep0;
      } else {
        offset = idx == 1u ? rep1 : idx == 2u ? rep2 : rep0 - 1u;
        if (offset == 0u) return MC_ZSTD_E_CORRUPT;
        if (idx != 1u) rep2 = rep1;
        rep1 = rep0, rep0 = offset;
      }
    }
    // nothing of a refused sequence is written
    const uint32_t room = out.cap - out.op;
    if (ll > room || ml > room - ll) return MC_ZSTD_E_CAPACITY;
    if (ll > lit_left) return MC_ZSTD_E_CORRUPT;
    if (offset > out.op + ll) return MC_ZSTD_E_CORRUPT;  // no dictionary: nothing before the frame's first byte
    out.literals(lit_kind, lit_at, ll);
    if (lit_kind != MC_ZSTD_LIT_RLE) lit_at += ll;
    lit_left -= ll;
    out.match(ml, offset);
    const uint32_t n_ll = (e_ll >> 8) & 255u, n_ml = (e_ml >> 8) & 255u, n_of = (e_of >> 8) & 255u;  // <= 9, 9, 8
    if (i + 1u == nseq) {
      // libzstd updates the states once more and wants the stream used up by then, or overrun
      if (br.left > (int32_t)(n_ll + n_ml + n_of)) return MC_ZSTD_E_CORRUPT;
    } else {  // LL, ML, OF
      uint64_t u = br.peek64();
      st_ll = (e_ll >> 16) + (n_ll ? (uint32_t)(u >> (64u - n_ll)) : 0u);
      u = n_ll ? u << n_ll : u;
      st_ml = (e_ml >> 16) + (n_ml ? (uint32_t)(u >> (64u - n_ml)) : 0u);
      u = n_ml ? u << n_ml : u;
      st_of = (e_of >> 16) + (n_of ? (uint32_t)(u >> (64u - n_of)) : 0u);
      br.drop(n_ll + n_ml + n_of);
    }
  }
  S->rep[0] = rep0, S->rep[1] = rep1, S->rep[2] = rep2;
  if (lit_left > out.cap - out.op) return MC_ZSTD_E_CAPACITY;
  out.literals(lit_kind, lit_at, lit_left);
  return MC_ZSTD_OK;
}

// One compressed block f[pos, pos + size).
template <class Src, class Sink, class Builder>
MC_ZSTD_HD int mc_zstd_compressed_block(Src &src, Sink &out, Builder &bld, const uint8_t *f, uint32_t n, uint32_t pos,
                                        uint32_t size, mc_zstd_tables *T, mc_zstd_state *S) {
  if (size >= MC_ZSTD_BLOCK_MAX) return MC_ZSTD_E_SRCSIZE;
  if (size < 3u) return MC_ZSTD_E_CORRUPT;
  const uint32_t end = pos + size;  // <= n: the frame walk's
  // ---- the literals section ----
  const uint32_t b0 = f[pos], type = b0 & 3u, sf = (b0 >> 2) & 3u;
  uint32_t lit_kind, lit_at, regen, p;
  if (type < 2u) {
    const uint32_t lh = sf == 1u ? 2u : sf == 3u ? 3u : 1u;
    regen = lh == 1u ? b0 >> 3 : mc_zstd_le(f + pos, lh) >> 4;
    p = pos + lh;
    if (type == 0u) {
      if (regen > end - p) return MC_ZSTD_E_CORRUPT;
      lit_kind = MC_ZSTD_LIT_RAW, lit_at = p;
      p += regen;
    } else {
      if (p >= end || regen > MC_ZSTD_BLOCK_MAX) return MC_ZSTD_E_CORRUPT;
      lit_kind = MC_ZSTD_LIT_RLE, lit_at = f[p];
      p += 1u;
    }
  } else {
    if (size < 5u) return MC_ZSTD_E_CORRUPT;
    const uint32_t lhc = mc_zstd_le(f + pos, 4);
    uint32_t lh, comp;
    if (sf < 2u) lh = 3u, regen = (lhc >> 4) & 0x3ffu, comp = (lhc >> 14) & 0x3ffu;
    else if (sf == 2u) lh = 4u, regen = (lhc >> 4) & 0x3fffu, comp = lhc >> 18;
    else lh = 5u, regen = (lhc >> 4) & 0x3ffffu, comp = (lhc >> 22) + ((uint32_t)f[pos + 4u] << 10);
    if (regen > MC_ZSTD_BLOCK_MAX || comp > size - lh) return MC_ZSTD_E_CORRUPT;
    p = pos + lh;
    const uint32_t lit_end = p + comp;
    if (type == 3u) {
      if (!S->have_huf) return MC_ZSTD_E_CORRUPT;
    } else {
      if (regen == 0u) return MC_ZSTD_E_CORRUPT;
      uint32_t nw, bytes, count[13];
      int e = mc_zstd_read_weights(f, n, p, lit_end, bld, T, &nw, &bytes);
      if (e != MC_ZSTD_OK) return e;
      bld.weigh(T->weights, nw, count);
      e = mc_zstd_check_weights(T->weights, nw, &S->huf_log, count);
      if (e != MC_ZSTD_OK) return e;
      bld.sync();
      bld.huf(T, nw + 1u, S->huf_log, count);
      bld.sync();
      S->have_huf = 1;
      p += bytes;
    }
    if (p >= lit_end) return MC_ZSTD_E_CORRUPT;
    mc_zstd_lit_streams ls;
    ls.nstreams = sf == 0u ? 1u : 4u;
    if (sf == 0u) {
      ls.start[0] = p, ls.end[0] = lit_end, ls.out[0] = 0, ls.len[0] = regen;
    } else {
      if (lit_end - p < 10u) return MC_ZSTD_E_CORRUPT;
      const uint32_t seg = (regen + 3u) >> 2;
      if (3u * seg > regen) return MC_ZSTD_E_CORRUPT;
      uint32_t at = p + 6u;
      for (uint32_t k = 0; k < 4u; ++k) {
        const uint32_t l = k < 3u ? mc_zstd_le(f + p + 2u * k, 2) : lit_end - at;
        if (l == 0u || l > lit_end - at) return MC_ZSTD_E_CORRUPT;
        ls.start[k] = at, ls.end[k] = at + l;
        ls.out[k] = k * seg, ls.len[k] = k < 3u ? seg : regen - 3u * seg;
        at += l;
      }
    }
    const int e = out.huffman(ls, T->huf, S->huf_log);
    if (e != MC_ZSTD_OK) return e;
    lit_kind = MC_ZSTD_LIT_BUF, lit_at = 0;
    p = lit_end;
  }
  // ---- the sequences section ----
  if (p >= end) return MC_ZSTD_E_SRCSIZE;
  uint32_t nseq = f[p++];
  if (nseq == 0u) {
    if (p != end) return MC_ZSTD_E_SRCSIZE;
    if (regen > out.cap - out.op) return MC_ZSTD_E_CAPACITY;
    out.literals(lit_kind, lit_at, regen);
    return MC_ZSTD_OK;
  }
  if (nseq >= 128u) {
    if (nseq == 255u) {
      if (end - p < 2u) return MC_ZSTD_E_SRCSIZE;
      nseq = mc_zstd_le(f + p, 2) + 0x7f00u;
      p += 2u;
    } else {
      if (p >= end) return MC_ZSTD_E_SRCSIZE;
      nseq = ((nseq - 128u) << 8) + f[p++];
    }
  }
  if (p >= end) return MC_ZSTD_E_SRCSIZE;
  const uint32_t modes = f[p++];
  for (uint32_t which = 0; which < 3u; ++which) {
    const int e = mc_zstd_seq_table(f, &p, end, (modes >> (6u - 2u * which)) & 3u, which, bld, T, S);
    if (e != MC_ZSTD_OK) return e;
  }
  S->have_fse = 1;
  return mc_zstd_sequences(src, out, f, p, end, nseq, T, S, lit_kind, lit_at, regen);
}

// The blocks of frame f[0, n) from data_off to the last one.  Sink: cap, op;
// literals(kind, at, len) and match(len, offset) write what the walker has
// checked to fit; huffman(streams, table, log) fills the literals buffer.
template <class Src, class Sink, class Builder>
MC_ZSTD_HD int mc_zstd_blocks(Src &src, Sink &out, Builder &bld, const uint8_t *f, uint32_t n, uint32_t data_off,
                              uint32_t block_max, mc_zstd_tables *T) {
  mc_zstd_state S;
  S.rep[0] = 1, S.rep[1] = 4, S.rep[2] = 8;
  S.ll_log = S.of_log = S.ml_log = S.huf_log = 0;
  S.have_huf = S.have_fse = 0;
  uint32_t p = data_off;
  for (;;) {
    if (n - p < 3u) return MC_ZSTD_E_HEADER;  // (the frame walk has looked already)
    const uint32_t bh = mc_zstd_le(f + p, 3);
    const uint32_t last = bh & 1u, type = (bh >> 1) & 3u, size = bh >> 3;
    p += 3u;
    const uint32_t held = type == 1u ? 1u : size;
    if (type == 3u || held > n - p) return MC_ZSTD_E_HEADER;
    const uint32_t before = out.op;
    int e = MC_ZSTD_OK;
    if (type == 2u) {
      e = mc_zstd_compressed_block(src, out, bld, f, n, p, size, T, &S);
    } else if (size > out.cap - out.op) {  // (the capacity first: a declared size bounds both)
      e = MC_ZSTD_E_CAPACITY;
    } else if (size > block_max) {
      e = MC_ZSTD_E_CORRUPT;
    } else {
      out.literals(type == 0u ? MC_ZSTD_LIT_RAW : MC_ZSTD_LIT_RLE, type == 0u ? p : (uint32_t)f[p], size);
    }
    if (e != MC_ZSTD_OK) return e;
    if (out.op - before > block_max) return MC_ZSTD_E_CORRUPT;
    p += held;
    if (last) return MC_ZSTD_OK;
  }
}

// ---- the scalar model -----------------------------------------------------------------
struct mc_zstd_ptr_sink {
  const uint8_t *frame;
  uint32_t n;
  uint8_t *dst;  // NULL: count only
  uint8_t *lit;  // MC_ZSTD_BLOCK_MAX bytes (with dst)
  uint32_t cap, op;
  MC_ZSTD_HD void literals(uint32_t kind, uint32_t at, uint32_t len) {
    if (dst)
      for (uint32_t k = 0; k < len; ++k)
        dst[op + k] = kind == MC_ZSTD_LIT_RAW ? frame[at + k] : kind == MC_ZSTD_LIT_RLE ? (uint8_t)at : lit[at + k];
    op += len;
  }
  MC_ZSTD_HD void match(uint32_t len, uint32_t offset) {
    if (dst)
      for (uint32_t k = 0; k < len; ++k) dst[op + k] = dst[op + k - offset];  // byte-serial by definition
    op += len;
  }
  MC_ZSTD_HD int huffman(const mc_zstd_lit_streams &ls, const uint16_t *huf, uint32_t log) {
    if (!dst) return MC_ZSTD_OK;  // counting needs the sizes only
    for (uint32_t k = 0; k < ls.nstreams; ++k) {
      uint8_t *o = lit + ls.out[k];  // out + len <= Regenerated_Size <= 128 KiB
      auto put = [o](uint32_t i, uint32_t b) { o[i] = (uint8_t)b; };
      const int e = mc_zstd_huf_stream(frame, n, ls.start[k], ls.end[k], huf, log, ls.len[k], put);
      if (e != MC_ZSTD_OK) return e;
    }
    return MC_ZSTD_OK;
  }
};

// One frame f[0, n) into at most cap bytes at dst; dst == NULL only counts (up
// to cap), decodes no Huffman stream and skips the check stage.  lit: 128 KiB
// of scratch (with dst).  Returns 0 or an mc_zstd_error; *produced = bytes
// written (counted); *word = the error record's second word: the computed
// checksum for a checksum error, *produced otherwise.
MC_ZSTD_HD int mc_zstd_decode_frame(const uint8_t *f, uint64_t n, uint8_t *dst, uint32_t cap, uint8_t *lit,
                                    uint32_t *produced, uint32_t *word, mc_zstd_tables *T) {
  *produced = 0, *word = 0;
  if (n >= MC_ZSTD_MAX_BYTES || cap >= MC_ZSTD_MAX_BYTES) return MC_ZSTD_E_TABLE;
  mc_zstd_header h;
  uint32_t end_off;
  int e = mc_zstd_open(f, n, &h, &end_off);
  if (e != MC_ZSTD_OK) return e;
  mc_zstd_mem_src src{f, (uint32_t)n};
  mc_zstd_ptr_sink out{f, (uint32_t)n, dst, lit, cap, 0};
  mc_zstd_scalar_builder bld;
  e = mc_zstd_blocks(src, out, bld, f, (uint32_t)n, h.data_off, h.block_max, T);
  *produced = *word = out.op;
  if (e != MC_ZSTD_OK || !dst) return e;
  uint32_t flags = (h.checksum ? MC_ZSTD_S_CHECKSUM : 0u) | (h.content != MC_ZSTD_UNKNOWN ? MC_ZSTD_S_SIZED : 0u);
  const uint32_t content = h.content < MC_ZSTD_MAX_BYTES ? (uint32_t)h.content : MC_ZSTD_MAX_BYTES;
  const uint32_t check = h.checksum ? (uint32_t)mc_xxh64(dst, out.op) : 0u;
  e = mc_zstd_check(f, flags, content, end_off, out.op, check);
  if (e == MC_ZSTD_E_CHECK) *word = check;
  return e;
}
