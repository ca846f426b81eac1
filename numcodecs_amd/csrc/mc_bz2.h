// mc_bz2.h -- bzip2 streams: the rules, the error codes and a scalar decoder,
// shared by the gfx950 kernels (mc_bz2.hip) and the host build of the CPU
// suite (tests/native_bz2).  The bit reader, the block-header parser, the
// symbol loop and the stream walker below are the very code the kernels run;
// a worker type supplies what differs between one host thread and one wave:
// the Huffman symbol step, the move-to-front step, the run splat, and
// everything after the symbols of a block (counting sort, inverse BWT, RLE1
// undo, CRC).  Both workers give the same bytes and the same code.
//
// Acceptance is libbz2 1.0.8's (decompress.c, huffman.c), which Python's bz2
// wraps, not the format's:
//   * bits are asked for in libbz2's portions, and a portion that does not lie
//     inside the frame is "truncated" before any verdict on it; every byte of
//     a magic is checked as it is read;
//   * origPtr is checked against 10 + 100000 * level when read and against the
//     block's symbol count after the symbols;
//   * selectors beyond 18002 are read and discarded;
//   * Huffman symbols come from limit / base / perm tables built from the
//     lengths as hbCreateDecodeTables builds them: an over-subscribed set
//     decodes, an incomplete set fails at the first unused code (a code of
//     more than 20 bits, or an index outside the table);
//   * a run is refused once its weight reaches 2 * 1024 * 1024, and a block
//     that would exceed 100000 * level symbols after a run or at a symbol;
//   * the inverse BWT takes exactly nblock steps from origPtr, whatever the
//     cycle structure of the permutation;
//   * four equal bytes are followed by a count byte of any value; a block that
//     ends where the count byte should be is refused;
//   * a stream with no block is valid and empty.
// Two departures, reported with codes of their own: a block with the
// randomised bit set, and a further stream behind the first (trailing bytes
// that begin with "BZh1".."BZh9" or are a proper prefix of that; any other
// trailing bytes are ignored, as bz2.decompress ignores them).
//
// Termination and bounds: every pass of a loop over the frame consumes at
// least one bit and is preceded by the check that the bit lies inside the
// frame; the reader yields zeros past the frame without reading memory.  A
// block holds at most 100000 * level symbols (checked before a symbol or a run
// is stored), every successor the sort stores is a symbol index below nblock,
// so the inverse BWT never leaves [0, nblock); no destination byte at or past
// the capacity is written.
#pragma once

#include <stddef.h>
#include <stdint.h>

#ifndef MC_BZ2_HD
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define MC_BZ2_HD __host__ __device__ __forceinline__
#else
#define MC_BZ2_HD inline
#endif
#endif

// a value every lane of the wave holds alike, moved to a scalar register
#if defined(__HIP_DEVICE_COMPILE__)
#define MC_BZ2_UNI(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))
#else
#define MC_BZ2_UNI(x) ((uint32_t)(x))
#endif

// error codes of the device error record / the host model (0 = none)
enum mc_bz2_error {
  MC_BZ2_OK = 0,
  MC_BZ2_E_MAGIC = 1,         // the stream does not begin with "BZh"
  MC_BZ2_E_LEVEL = 2,         // the level digit is not '1'..'9'
  MC_BZ2_E_TRUNCATED = 3,     // a read past the frame's last bit
  MC_BZ2_E_BLOCK_MAGIC = 4,   // neither a block magic nor the end magic
  MC_BZ2_E_RANDOMISED = 5,    // departure: a block with the randomised bit
  MC_BZ2_E_ORIGPTR = 6,       // origPtr beyond the block
  MC_BZ2_E_SYMMAP = 7,        // no byte value in use
  MC_BZ2_E_NGROUPS = 8,       // fewer than 2 or more than 6 tables
  MC_BZ2_E_NSELECTORS = 9,    // no selector
  MC_BZ2_E_SELECTOR = 10,     // a selector names a missing table
  MC_BZ2_E_CODELEN = 11,      // a code length outside 1..20
  MC_BZ2_E_CODE = 12,         // an unused code
  MC_BZ2_E_GROUPS = 13,       // more symbol groups than selectors
  MC_BZ2_E_RUN = 14,          // a run's weight reached 2 * 1024 * 1024
  MC_BZ2_E_OVERFLOW = 15,     // more symbols than the block holds
  MC_BZ2_E_RLE = 16,          // the block ends where a count byte is due
  MC_BZ2_E_BLOCK_CRC = 17,
  MC_BZ2_E_STREAM_CRC = 18,
  MC_BZ2_E_CAPACITY = 19,     // the output would exceed the capacity
  MC_BZ2_E_FURTHER = 20,      // departure: a further stream follows
  MC_BZ2_E_TABLE = 21,        // the caller's frame record is out of range
};

// frames and outputs are shorter than this
#define MC_BZ2_MAX_BYTES 0x40000000u
#define MC_BZ2_MAX_SELECTORS 18002u
#define MC_BZ2_MAX_ALPHA 258u
#define MC_BZ2_MAX_CODE_LEN 20u
#define MC_BZ2_BLOCK_UNIT 100000u
#define MC_BZ2_POLY 0x04c11db7u

// One frame of a batch (device table, one record per frame; include/mcodec.h):
// the record of the inflate and zstd decoders, the last word unused.
struct mc_bz2_frame {
  uint64_t src_off;
  uint64_t src_len;
  uint64_t dst;
  uint32_t capacity;
  uint32_t reserved;
};

#define MC_BZ2_S_VALID 1u  // the header parsed: the decode kernel runs
#define MC_BZ2_S_EMPTY 2u  // a frame of no byte: an empty result

// One stream, as the plan kernel leaves it for the decode kernel.
struct mc_bz2_stream {
  uint64_t src_off;
  uint64_t dst;
  uint32_t src_len;
  uint32_t level;
  uint32_t capacity;
  uint32_t flags;
};

// The tables of one block (LDS on the device).
struct alignas(16) mc_bz2_tables {
  int32_t limit[6][24];  // libbz2's limit / base, 23 entries used
  int32_t base[6][24];
  uint32_t unzftab[256];  // the byte histogram, then the cumulative table of the sort
  uint16_t perm[6][MC_BZ2_MAX_ALPHA + 2];
  uint8_t len[6][MC_BZ2_MAX_ALPHA + 2];
  uint8_t minlen[8];
  uint8_t seq[256];  // symbol -> byte value
  uint8_t mtf[256];
  uint8_t selector[MC_BZ2_MAX_SELECTORS + 6];
};

struct mc_bz2_block {
  uint32_t crc, orig, nsel, ngroups, ninuse;
};

MC_BZ2_HD uint32_t mc_bz2_bswap(uint32_t v) {
  return (v >> 24) | ((v >> 8) & 0xff00u) | ((v << 8) & 0xff0000u) | (v << 24);
}

// ---- CRC-32, polynomial 0x04c11db7, MSB first ---------------------------------
MC_BZ2_HD uint32_t mc_bz2_mulx(uint32_t v, uint32_t times) {  // v * x^times mod P
  for (uint32_t k = 0; k < times; ++k) v = (v << 1) ^ ((v >> 31) ? MC_BZ2_POLY : 0u);
  return v;
}
MC_BZ2_HD uint32_t mc_bz2_gfmul(uint32_t a, uint32_t b) {  // a * b mod P
  uint32_t r = 0;
  for (int i = 31; i >= 0; --i) {
    r = (r << 1) ^ ((r >> 31) ? MC_BZ2_POLY : 0u);
    if ((b >> i) & 1u) r ^= a;
  }
  return r;
}
MC_BZ2_HD uint32_t mc_bz2_crc_byte(uint32_t crc, uint32_t b) { return mc_bz2_mulx(crc ^ (b << 24), 8); }

// ---- the stream header --------------------------------------------------------
// f[0, n): "BZh" and the level, each byte checked as libbz2 reads it.
MC_BZ2_HD int mc_bz2_parse_header(const uint8_t *f, uint64_t n, uint32_t *level, uint32_t *empty) {
  *level = 0;
  *empty = n == 0;
  if (n == 0) return MC_BZ2_OK;
  const uint8_t want[3] = {'B', 'Z', 'h'};
  for (uint32_t k = 0; k < 3; ++k) {
    if (k >= n) return MC_BZ2_E_TRUNCATED;
    if (f[k] != want[k]) return MC_BZ2_E_MAGIC;
  }
  if (n < 4) return MC_BZ2_E_TRUNCATED;
  if (f[3] < '1' || f[3] > '9') return MC_BZ2_E_LEVEL;
  *level = (uint32_t)(f[3] - '0');
  return MC_BZ2_OK;
}

// What lies behind the stream's last byte, at byte `at` <= n.
MC_BZ2_HD int mc_bz2_after(const uint8_t *f, uint64_t n, uint64_t at) {
  const uint64_t rest = n - at;
  const uint8_t want[3] = {'B', 'Z', 'h'};
  for (uint32_t k = 0; k < 3 && k < rest; ++k)
    if (f[at + k] != want[k]) return MC_BZ2_OK;
  if (rest == 0) return MC_BZ2_OK;
  if (rest <= 3) return MC_BZ2_E_FURTHER;
  return (f[at + 3] >= '1' && f[at + 3] <= '9') ? MC_BZ2_E_FURTHER : MC_BZ2_OK;
}

// ---- the bit reader: MSB first, a 64-bit buffer fed a dword at a time -----------
// Src::dword(i) is little-endian dword i of the frame, bytes at and past n as
// zeros.  pos counts the bits taken; nothing is taken past 8 * n.
struct mc_bz2_mem {
  const uint8_t *f;
  uint32_t n;
  MC_BZ2_HD uint32_t dword(uint32_t i) const {
    uint32_t v = 0;
    const uint64_t at = 4ull * i;
    for (uint32_t k = 0; k < 4; ++k)
      if (at + k < n) v |= (uint32_t)f[at + k] << (8u * k);
    return v;
  }
};

template <class Src>
struct mc_bz2_bits {
  Src &src;
  uint64_t buf, pos, end;
  uint32_t cnt, next;
  MC_BZ2_HD mc_bz2_bits(Src &s, uint32_t n) : src(s), buf(0), pos(0), end(8ull * n), cnt(0), next(0) {}
  MC_BZ2_HD void seek_byte(uint32_t at) {  // at is a multiple of 4
    pos = 8ull * at, next = at >> 2, buf = 0, cnt = 0;
  }
  MC_BZ2_HD uint64_t avail() const { return end - pos; }
  MC_BZ2_HD uint32_t peek(uint32_t nb) {  // 1 <= nb <= 32, zeros past the frame
    if (cnt < 32u) {
      buf |= (uint64_t)mc_bz2_bswap(src.dword(next++)) << (32u - cnt);
      cnt += 32u;
    }
    return (uint32_t)(buf >> (64u - nb));
  }
  MC_BZ2_HD void skip(uint32_t nb) {  // after peek(>= nb)
    buf <<= nb, cnt -= nb, pos += nb;
  }
  MC_BZ2_HD bool get(uint32_t nb, uint32_t *v) {
    if (avail() < nb) return false;
    *v = peek(nb);
    skip(nb);
    return true;
  }
};

// ---- the tables of a block, as hbCreateDecodeTables builds them -----------------
MC_BZ2_HD void mc_bz2_build_table(mc_bz2_tables *t, uint32_t g, uint32_t alpha) {
  uint32_t mn = 32, mx = 0;
  for (uint32_t i = 0; i < alpha; ++i) {
    const uint32_t l = t->len[g][i];
    if (l > mx) mx = l;
    if (l < mn) mn = l;
  }
  t->minlen[g] = (uint8_t)mn;
  int32_t *limit = t->limit[g], *base = t->base[g];
  uint32_t pp = 0;
  for (uint32_t i = mn; i <= mx; ++i)
    for (uint32_t j = 0; j < alpha; ++j)
      if (t->len[g][j] == i) t->perm[g][pp++] = (uint16_t)j;
  for (uint32_t i = 0; i < 23; ++i) base[i] = 0;
  for (uint32_t i = 0; i < alpha; ++i) base[t->len[g][i] + 1]++;
  for (uint32_t i = 1; i < 23; ++i) base[i] += base[i - 1];
  for (uint32_t i = 0; i < 23; ++i) limit[i] = 0;
  int32_t vec = 0;
  for (uint32_t i = mn; i <= mx; ++i) {
    vec += base[i + 1] - base[i];
    limit[i] = vec - 1;
    vec <<= 1;
  }
  for (uint32_t i = mn + 1; i <= mx; ++i) base[i] = ((limit[i - 1] + 1) << 1) - base[i];
}

// The symbol step once the first length zn at which the code matches is known
// (21: none up to 20 bits); peek21 = the next 21 bits.  libbz2 takes minLen
// bits, then one at a time, and refuses a 21st only after reading it.
template <class R>
MC_BZ2_HD int mc_bz2_take_symbol(R &br, const mc_bz2_tables *t, uint32_t g, uint32_t zn, uint32_t peek21, int32_t base_zn,
                                 uint32_t *sym) {
  if (br.avail() < zn) return MC_BZ2_E_TRUNCATED;
  if (zn > MC_BZ2_MAX_CODE_LEN) return MC_BZ2_E_CODE;
  const int32_t idx = (int32_t)(peek21 >> (21u - zn)) - base_zn;
  if (idx < 0 || idx >= (int32_t)MC_BZ2_MAX_ALPHA) return MC_BZ2_E_CODE;
  br.skip(zn);
  *sym = MC_BZ2_UNI(t->perm[g][idx]);
  return MC_BZ2_OK;
}

// ---- a block's header, behind the magic -----------------------------------------
// W: lead() (this thread writes the shared tables), sync(), first() / stride()
// (the share of a loop that may be split).
template <class R, class W>
MC_BZ2_HD int mc_bz2_block_header(R &br, mc_bz2_tables *t, W &w, uint32_t level, mc_bz2_block *b) {
  uint32_t v;
  if (!br.get(32, &b->crc)) return MC_BZ2_E_TRUNCATED;
  if (!br.get(1, &v)) return MC_BZ2_E_TRUNCATED;
  if (v) return MC_BZ2_E_RANDOMISED;
  if (!br.get(24, &b->orig)) return MC_BZ2_E_TRUNCATED;
  if (b->orig > 10u + MC_BZ2_BLOCK_UNIT * level) return MC_BZ2_E_ORIGPTR;
  uint32_t used16;
  if (!br.get(16, &used16)) return MC_BZ2_E_TRUNCATED;
  uint32_t ninuse = 0;
  for (uint32_t i = 0; i < 16; ++i) {
    if (!((used16 >> (15u - i)) & 1u)) continue;
    if (!br.get(16, &v)) return MC_BZ2_E_TRUNCATED;
    for (uint32_t j = 0; j < 16; ++j)
      if ((v >> (15u - j)) & 1u) {
        if (w.lead()) t->seq[ninuse] = (uint8_t)(16u * i + j);
        ++ninuse;
      }
  }
  if (ninuse == 0) return MC_BZ2_E_SYMMAP;
  b->ninuse = ninuse;
  const uint32_t alpha = ninuse + 2;
  if (!br.get(3, &b->ngroups)) return MC_BZ2_E_TRUNCATED;
  if (b->ngroups < 2 || b->ngroups > 6) return MC_BZ2_E_NGROUPS;
  if (!br.get(15, &b->nsel)) return MC_BZ2_E_TRUNCATED;
  if (b->nsel < 1) return MC_BZ2_E_NSELECTORS;
  uint32_t order = 0x543210u;  // the selectors' move-to-front list, a nibble per table
  for (uint32_t i = 0; i < b->nsel; ++i) {
    uint32_t j = 0;
    for (;;) {
      if (!br.get(1, &v)) return MC_BZ2_E_TRUNCATED;
      if (!v) break;
      if (++j >= b->ngroups) return MC_BZ2_E_SELECTOR;
    }
    if (i < MC_BZ2_MAX_SELECTORS) {
      const uint32_t sh = 4u * j, g = (order >> sh) & 15u;
      order = (order & ~((16u << sh) - 1u)) | ((order & ((1u << sh) - 1u)) << 4) | g;
      if (w.lead()) t->selector[i] = (uint8_t)g;
    }
  }
  if (b->nsel > MC_BZ2_MAX_SELECTORS) b->nsel = MC_BZ2_MAX_SELECTORS;
  for (uint32_t g = 0; g < b->ngroups; ++g) {
    uint32_t curr;
    if (!br.get(5, &curr)) return MC_BZ2_E_TRUNCATED;
    for (uint32_t i = 0; i < alpha; ++i) {
      for (;;) {
        if (curr < 1 || curr > MC_BZ2_MAX_CODE_LEN) return MC_BZ2_E_CODELEN;
        if (!br.get(1, &v)) return MC_BZ2_E_TRUNCATED;
        if (!v) break;
        if (!br.get(1, &v)) return MC_BZ2_E_TRUNCATED;
        curr = v ? curr - 1u : curr + 1u;
      }
      if (w.lead()) t->len[g][i] = (uint8_t)curr;
    }
  }
  w.sync();
  for (uint32_t g = w.first(); g < b->ngroups; g += w.stride()) mc_bz2_build_table(t, g, alpha);
  for (uint32_t i = w.first(); i < 256; i += w.stride()) t->mtf[i] = (uint8_t)i, t->unzftab[i] = 0;
  w.sync();
  return MC_BZ2_OK;
}

// ---- the symbols of a block -> the byte column and the histogram -------------------
// W: group(t, g) (table g becomes current), symbol(br, t, g, &sym),
// front(t, nn) (the list's entry nn, moved to the front), emit(t, at, byte, count).
template <class R, class W>
MC_BZ2_HD int mc_bz2_symbols(R &br, mc_bz2_tables *t, W &w, uint32_t level, const mc_bz2_block &b, uint32_t *nblock_out) {
  const uint32_t eob = b.ninuse + 1, nmax = MC_BZ2_BLOCK_UNIT * level;
  uint32_t group_no = 0, group_pos = 0, g = 0, nblock = 0, sym = 0;
  int e;
#define MC_BZ2_NEXT()                                      \
  do {                                                     \
    if (group_pos == 0) {                                  \
      if (group_no >= b.nsel) return MC_BZ2_E_GROUPS;      \
      group_pos = 50;                                      \
      g = MC_BZ2_UNI(t->selector[group_no++]);             \
      w.group(t, g);                                       \
    }                                                      \
    --group_pos;                                           \
    e = w.symbol(br, t, g, &sym);                          \
    if (e != MC_BZ2_OK) return e;                          \
  } while (0)
  MC_BZ2_NEXT();
  for (;;) {
    if (sym == eob) break;
    if (sym <= 1u) {  // RUNA / RUNB
      uint32_t es = 0, weight = 1;
      do {
        if (weight >= 2u * 1024u * 1024u) return MC_BZ2_E_RUN;
        es += weight << sym;
        weight <<= 1;
        MC_BZ2_NEXT();
      } while (sym <= 1u);
      if (es > nmax - nblock) return MC_BZ2_E_OVERFLOW;
      w.emit(t, nblock, MC_BZ2_UNI(t->seq[MC_BZ2_UNI(t->mtf[0])]), es);
      nblock += es;
      continue;
    }
    if (nblock >= nmax) return MC_BZ2_E_OVERFLOW;
    w.emit(t, nblock, MC_BZ2_UNI(t->seq[w.front(t, sym - 1u)]), 1u);
    ++nblock;
    MC_BZ2_NEXT();
  }
#undef MC_BZ2_NEXT
  *nblock_out = nblock;
  return MC_BZ2_OK;
}

// ---- the stream: blocks up to the end magic, the combined CRC, what follows --------
// W as above, and finish(t, nblock, orig, &crc): the sort, the inverse BWT and
// the RLE1 undo of the block; crc = the CRC of what the block decoded to.
// *blocks = the blocks completed (the error record's second word).
template <class R, class W>
MC_BZ2_HD int mc_bz2_blocks(R &br, mc_bz2_tables *t, W &w, uint32_t level, uint32_t *blocks) {
  const uint8_t block_magic[5] = {0x41, 0x59, 0x26, 0x53, 0x59}, end_magic[5] = {0x72, 0x45, 0x38, 0x50, 0x90};
  uint32_t combined = 0, v;
  *blocks = 0;
  for (;;) {
    if (!br.get(8, &v)) return MC_BZ2_E_TRUNCATED;
    if (v != 0x31u && v != 0x17u) return MC_BZ2_E_BLOCK_MAGIC;
    const bool last = v == 0x17u;
    for (uint32_t k = 0; k < 5; ++k) {
      if (!br.get(8, &v)) return MC_BZ2_E_TRUNCATED;
      if (v != (last ? end_magic[k] : block_magic[k])) return MC_BZ2_E_BLOCK_MAGIC;
    }
    if (last) break;
    mc_bz2_block b;
    int e = mc_bz2_block_header(br, t, w, level, &b);
    if (e != MC_BZ2_OK) return e;
    uint32_t nblock = 0, crc = 0;
    e = mc_bz2_symbols(br, t, w, level, b, &nblock);
    if (e != MC_BZ2_OK) return e;
    if (b.orig >= nblock) return MC_BZ2_E_ORIGPTR;
    e = w.finish(t, nblock, b.orig, &crc);
    if (e != MC_BZ2_OK) return e;
    if (crc != b.crc) return MC_BZ2_E_BLOCK_CRC;
    combined = ((combined << 1) | (combined >> 31)) ^ crc;
    ++*blocks;
  }
  if (!br.get(32, &v)) return MC_BZ2_E_TRUNCATED;
  if (v != combined) return MC_BZ2_E_STREAM_CRC;
  return MC_BZ2_OK;
}

// ---- the scalar worker: one host thread ----------------------------------------------
// col: 100000 * level bytes, tt: as many dwords.  dst NULL: count only.
struct mc_bz2_scalar {
  uint8_t *col;
  uint32_t *tt;
  uint8_t *dst;
  uint32_t cap, op;
  MC_BZ2_HD bool lead() const { return true; }
  MC_BZ2_HD void sync() {}
  MC_BZ2_HD uint32_t first() const { return 0; }
  MC_BZ2_HD uint32_t stride() const { return 1; }
  MC_BZ2_HD void group(const mc_bz2_tables *, uint32_t) {}
  template <class R>
  MC_BZ2_HD int symbol(R &br, const mc_bz2_tables *t, uint32_t g, uint32_t *sym) {
    const uint32_t peek21 = br.peek(21);
    uint32_t zn = t->minlen[g];
    for (; zn <= MC_BZ2_MAX_CODE_LEN; ++zn)
      if ((int32_t)(peek21 >> (21u - zn)) <= t->limit[g][zn]) break;
    return mc_bz2_take_symbol(br, t, g, zn, peek21, t->base[g][zn], sym);
  }
  MC_BZ2_HD uint32_t front(mc_bz2_tables *t, uint32_t nn) {
    const uint8_t v = t->mtf[nn];
    for (uint32_t k = nn; k > 0; --k) t->mtf[k] = t->mtf[k - 1];
    t->mtf[0] = v;
    return v;
  }
  MC_BZ2_HD void emit(mc_bz2_tables *t, uint32_t at, uint32_t byte, uint32_t count) {
    for (uint32_t k = 0; k < count; ++k) col[at + k] = (uint8_t)byte;
    t->unzftab[byte] += count;
  }
  MC_BZ2_HD int finish(mc_bz2_tables *t, uint32_t nblock, uint32_t orig, uint32_t *crc_out) {
    uint32_t sum = 0;
    for (uint32_t i = 0; i < 256; ++i) {
      const uint32_t c = t->unzftab[i];
      t->unzftab[i] = sum;
      sum += c;
    }
    // the successor and the byte of the sorted column in one word
    for (uint32_t i = 0; i < nblock; ++i) tt[t->unzftab[col[i]]++] = (i << 8) | col[i];
    uint32_t p = orig;
    for (uint32_t k = 0; k < nblock; ++k) {  // exactly nblock steps
      const uint32_t e = tt[p];
      col[k] = (uint8_t)e;
      p = e >> 8;
    }
    uint32_t crc = 0xffffffffu, run = 0, prev = 0;
    bool expect = false;
    for (uint32_t k = 0; k < nblock; ++k) {
      const uint32_t c = col[k];
      if (expect) {
        if (c > cap - op) return MC_BZ2_E_CAPACITY;
        for (uint32_t r = 0; r < c; ++r) {
          if (dst) dst[op + r] = (uint8_t)prev;
          crc = mc_bz2_crc_byte(crc, prev);
        }
        op += c, expect = false, run = 0;
        continue;
      }
      if (op >= cap) return MC_BZ2_E_CAPACITY;
      if (dst) dst[op] = (uint8_t)c;
      ++op;
      crc = mc_bz2_crc_byte(crc, c);
      if (run > 0 && c == prev) ++run;
      else run = 1, prev = c;
      if (run == 4) expect = true;
    }
    if (expect) return MC_BZ2_E_RLE;
    *crc_out = ~crc;
    return MC_BZ2_OK;
  }
};

// One frame f[0, n) into at most cap bytes at dst (NULL: count only, the same
// chain with no output stores): 0 or an mc_bz2_error.  work: 5 * 100000 *
// level bytes, 4-byte aligned (tt, then the byte column).
MC_BZ2_HD int mc_bz2_decode_stream(const uint8_t *f, uint64_t n, uint8_t *dst, uint32_t cap, uint32_t *produced,
                                   uint32_t *word, mc_bz2_tables *t, void *work, uint32_t work_level) {
  *produced = 0, *word = 0;
  if (n >= MC_BZ2_MAX_BYTES || cap >= MC_BZ2_MAX_BYTES) return MC_BZ2_E_TABLE;
  uint32_t level, empty;
  int e = mc_bz2_parse_header(f, n, &level, &empty);
  if (e != MC_BZ2_OK || empty) return e;
  if (level > work_level) return MC_BZ2_E_TABLE;
  mc_bz2_mem src{f, (uint32_t)n};
  mc_bz2_bits<mc_bz2_mem> br(src, (uint32_t)n);
  br.seek_byte(4);
  mc_bz2_scalar w{reinterpret_cast<uint8_t *>(work) + 4ull * MC_BZ2_BLOCK_UNIT * work_level,
                  reinterpret_cast<uint32_t *>(work), dst, cap, 0u};
  e = mc_bz2_blocks(br, t, w, level, word);
  *produced = w.op;
  if (e != MC_BZ2_OK) return e;
  return mc_bz2_after(f, n, (br.pos + 7u) >> 3);
}
