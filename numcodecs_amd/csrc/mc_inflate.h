// mc_inflate.h -- DEFLATE (RFC 1951) in the zlib (RFC 1950) and gzip (RFC
// 1952) containers: the rules, shared by the gfx950 kernels (mc_inflate.hip)
// and the host build of the CPU suite (tests/native_inflate).  The container
// parsers, the bit reader, the table checks, the block walker and the trailer
// classification below are the very code that guards the device; the kernels
// only supply their own source window, output sink and table builder.
//
// Where the RFCs leave a choice the rules are zlib's (inflate.c / inftrees.c),
// for the gzip container as Python's GzipFile applies them:
//   * a code-length, literal/length or distance set may not be over-subscribed;
//     an incomplete set is an error, except a literal/length or distance set
//     whose longest code has 1 bit (then the unused code is an invalid code of
//     1 bit); a set with no code at all is built without complaint and every
//     use of it is an invalid code of 1 bit (for the code-length code: the
//     length 0, taking 1 bit, as inflate.c reads inftrees.c's filler entry);
//   * a 16/17/18 repeat may run from the literal/length lengths into the
//     distance lengths, never past their end, and 16 needs a previous length;
//   * a code is accepted only if all of its bits (and of its extra bits) lie
//     inside the frame: a bit position past 8 * src_len is "truncated", and
//     that check comes before any other verdict on the same symbol;
//   * gzip: header and name CRCs are skipped, not verified; reserved flag bits
//     are ignored (GzipFile ignores them; MC_INF_E_GZ_FLAGS names the condition
//     zlib's own gzip reader refuses and is never raised here); zero bytes
//     after the trailer are padding; an empty frame is an empty result.
//
// Termination: the block loop ends at BFINAL or at the first error; every pass
// of the symbol loop and of the code-length loop consumes at least one bit and
// is followed by the truncation check, and the bit reader yields zeros past
// the frame without reading memory, so no loop outruns 8 * src_len + 64 bits;
// a table walk is at most 15 steps.  No source byte outside [0, src_len) is
// read, no destination byte outside [0, capacity) is written, and every table
// index is masked or bounded by the counts the table was built from.
#pragma once

#include <stddef.h>
#include <stdint.h>

#ifndef MC_INF_HD
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define MC_INF_HD __host__ __device__ __forceinline__
#else
#define MC_INF_HD inline
#endif
#endif

// a value every lane of the wave holds alike, moved to a scalar register (the
// compiler cannot see that a table entry read from LDS is wave-uniform)
#if defined(__HIP_DEVICE_COMPILE__)
#define MC_INF_UNI(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))
#else
#define MC_INF_UNI(x) ((uint32_t)(x))
#endif

// error codes of the device error record / the host model (0 = none), named
// after the condition zlib or GzipFile names
enum mc_inf_error {
  MC_INF_OK = 0,
  MC_INF_E_HEADER = 1,        // zlib: incorrect header check ((CMF << 8 | FLG) % 31)
  MC_INF_E_METHOD = 2,        // zlib: unknown compression method (CM != 8)
  MC_INF_E_WINDOW = 3,        // zlib: invalid window size (CINFO > 7)
  MC_INF_E_DICT = 4,          // zlib: a preset dictionary is requested (FDICT)
  MC_INF_E_GZ_MAGIC = 5,      // gzip: not a gzipped file
  MC_INF_E_GZ_METHOD = 6,     // gzip: unknown compression method
  MC_INF_E_GZ_FLAGS = 7,      // gzip: reserved flag bits (never raised, see above)
  MC_INF_E_TRUNCATED = 8,     // a read past the frame's last byte
  MC_INF_E_BTYPE = 9,         // invalid block type
  MC_INF_E_STORED = 10,       // invalid stored block lengths
  MC_INF_E_SYMBOLS = 11,      // too many length or distance symbols
  MC_INF_E_CODELENS = 12,     // invalid code lengths set
  MC_INF_E_REPEAT = 13,       // invalid bit length repeat
  MC_INF_E_LITLEN_SET = 14,   // invalid literal/lengths set
  MC_INF_E_DIST_SET = 15,     // invalid distances set
  MC_INF_E_NO_EOB = 16,       // invalid code -- missing end-of-block
  MC_INF_E_LITLEN_CODE = 17,  // invalid literal/length code
  MC_INF_E_DIST_CODE = 18,    // invalid distance code
  MC_INF_E_FAR = 19,          // invalid distance too far back
  MC_INF_E_CAPACITY = 20,     // the output would exceed the capacity
  MC_INF_E_CHECK = 21,        // incorrect data check (Adler-32 / CRC-32)
  MC_INF_E_LENGTH = 22,       // gzip: incorrect length (ISIZE)
  MC_INF_E_GZ_JUNK = 23,      // gzip: trailing junk
  MC_INF_E_GZ_MEMBER = 24,    // gzip: a further member follows
  MC_INF_E_TABLE = 25,        // the caller's frame record is out of range
};

#define MC_INF_ZLIB 0u
#define MC_INF_GZIP 1u
// frames and outputs are shorter than this (the bit position fits 32 bits of bytes)
#define MC_INF_MAX_BYTES 0x40000000u

#define MC_INF_LIT_BITS 10u   // primary lookup of the literal/length code
#define MC_INF_DIST_BITS 8u   // and of the distance code
#define MC_INF_INVALID 511u   // the symbol of an unused code
// a table entry: symbol | code length << 9; 0 = no code that short
#define MC_INF_ENTRY(sym, len) ((uint32_t)(sym) | ((uint32_t)(len) << 9))

// One frame of a batch (device table, one record per frame; include/mcodec.h).
struct mc_inf_frame {
  uint64_t src_off;    // the frame's first byte in the concatenated frames
  uint64_t src_len;
  uint64_t dst;        // device address of the frame's output (decode only)
  uint32_t capacity;   // bytes dst holds
  uint32_t container;  // MC_INF_ZLIB / MC_INF_GZIP
};

#define MC_INF_S_VALID 1u  // the header parsed: the decode and check kernels run
#define MC_INF_S_EMPTY 2u  // an empty gzip frame: an empty result, nothing to run

// One stream, as the plan kernel leaves it for the decode and check kernels.
struct mc_inf_stream {
  uint64_t src_off;
  uint64_t dst;
  uint32_t src_len;
  uint32_t data_off;  // first DEFLATE byte, from the frame's start
  uint32_t capacity;
  uint32_t flags;     // MC_INF_S_* | container << 8
};

// The tables of one block (LDS on the device).  count[l] codes of l bits,
// sym[] the symbols in canonical order, pri[] the primary lookup.
struct alignas(16) mc_inf_tables {
  uint16_t lit_pri[1u << MC_INF_LIT_BITS];
  uint16_t dist_pri[1u << MC_INF_DIST_BITS];
  uint16_t lit_sym[288];
  uint16_t dist_sym[32];
  uint16_t lit_count[16];
  uint16_t dist_count[16];
  uint16_t cl_count[16];
  uint16_t cl_sym[24];
  uint8_t lens[320];  // code lengths: literal/length, then distance
  uint8_t cl_lens[32];
};

// ---- containers -------------------------------------------------------------
// The header of frame f[0, n): *data_off = the first DEFLATE byte.  Reads f
// only below n.  *empty (gzip): the frame has no byte at all.
MC_INF_HD int mc_inf_parse_header(const uint8_t *f, uint64_t n, uint32_t container, uint32_t *data_off,
                                  uint32_t *empty) {
  *data_off = 0;
  *empty = 0;
  if (container == MC_INF_ZLIB) {
    if (n < 2) return MC_INF_E_TRUNCATED;
    const uint32_t cmf = f[0], flg = f[1];
    if (((cmf << 8) | flg) % 31u) return MC_INF_E_HEADER;
    if ((cmf & 15u) != 8u) return MC_INF_E_METHOD;
    if ((cmf >> 4) > 7u) return MC_INF_E_WINDOW;
    if (flg & 0x20u) return n < 6 ? MC_INF_E_TRUNCATED : MC_INF_E_DICT;  // the dictionary id is read first
    *data_off = 2;
    return MC_INF_OK;
  }
  if (container != MC_INF_GZIP) return MC_INF_E_TABLE;
  if (n == 0) {
    *empty = 1;
    return MC_INF_OK;
  }
  if (n < 2 || f[0] != 0x1fu || f[1] != 0x8bu) return MC_INF_E_GZ_MAGIC;
  if (n < 10) return MC_INF_E_TRUNCATED;
  if (f[2] != 8u) return MC_INF_E_GZ_METHOD;
  const uint32_t flg = f[3];
  uint64_t p = 10;
  if (flg & 4u) {  // FEXTRA
    if (n - p < 2) return MC_INF_E_TRUNCATED;
    const uint32_t xlen = (uint32_t)f[p] | ((uint32_t)f[p + 1] << 8);
    p += 2;
    if (n - p < xlen) return MC_INF_E_TRUNCATED;
    p += xlen;
  }
  for (uint32_t bit = 8u; bit <= 16u; bit <<= 1) {  // FNAME, FCOMMENT: to the zero byte
    if (!(flg & bit)) continue;
    while (p < n && f[p] != 0) ++p;
    if (p == n) return MC_INF_E_TRUNCATED;
    ++p;
  }
  if (flg & 2u) {  // FHCRC, not verified
    if (n - p < 2) return MC_INF_E_TRUNCATED;
    p += 2;
  }
  *data_off = (uint32_t)p;  // p <= n < 2^30
  return MC_INF_OK;
}

// What follows a gzip trailer, q = the first non-zero byte at or after it (n: none).
MC_INF_HD int mc_inf_after_trailer(const uint8_t *f, uint64_t n, uint64_t q) {
  if (q >= n) return MC_INF_OK;  // padding only
  if (n - q >= 2 && f[q] == 0x1fu && f[q + 1] == 0x8bu) return MC_INF_E_GZ_MEMBER;
  return MC_INF_E_GZ_JUNK;
}

// The trailer at byte pos of frame f[0, n), against the checksum and the
// length of what was produced.  *after = the byte behind the trailer.
MC_INF_HD int mc_inf_check_trailer(const uint8_t *f, uint64_t n, uint64_t pos, uint32_t container, uint32_t check,
                                   uint32_t produced, uint64_t *after) {
  *after = pos;
  if (container == MC_INF_ZLIB) {
    if (pos > n || n - pos < 4) return MC_INF_E_TRUNCATED;
    const uint32_t stored = ((uint32_t)f[pos] << 24) | ((uint32_t)f[pos + 1] << 16) | ((uint32_t)f[pos + 2] << 8) | f[pos + 3];
    *after = pos + 4;
    return stored == check ? MC_INF_OK : MC_INF_E_CHECK;  // what follows is ignored
  }
  if (pos > n || n - pos < 8) return MC_INF_E_TRUNCATED;
  const uint8_t *t = f + pos;
  const uint32_t crc = (uint32_t)t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
  const uint32_t isize = (uint32_t)t[4] | ((uint32_t)t[5] << 8) | ((uint32_t)t[6] << 16) | ((uint32_t)t[7] << 24);
  *after = pos + 8;
  if (crc != check) return MC_INF_E_CHECK;
  if (isize != produced) return MC_INF_E_LENGTH;
  return MC_INF_OK;
}

// ---- the bit reader ----------------------------------------------------------
// Src::dword(i) is the frame's little-endian dword i, bytes at and past n as
// zeros (never read).  64 bits, refilled a dword at a time: after fill() at
// least 33 bits are there, which covers every symbol with its extra bits.
template <class Src>
struct mc_inf_bits {
  Src &src;
  uint32_t n;    // the frame's length
  uint64_t buf;
  uint32_t cnt;  // valid bits in buf
  uint32_t nd;   // the next dword to load
  MC_INF_HD mc_inf_bits(Src &s, uint32_t n_) : src(s), n(n_), buf(0), cnt(0), nd(0) {}
  MC_INF_HD void seek(uint32_t bytepos) {
    nd = bytepos >> 2;
    const uint32_t skip = 8u * (bytepos & 3u);
    buf = (uint64_t)(src.dword(nd) >> skip);
    cnt = 32u - skip;
    ++nd;
  }
  MC_INF_HD void fill() {
    if (cnt <= 32u) {
      buf |= (uint64_t)src.dword(nd) << cnt;
      cnt += 32u;
      ++nd;
    }
  }
  MC_INF_HD uint32_t peek(uint32_t k) const { return (uint32_t)buf & ((1u << k) - 1u); }  // k < 32
  MC_INF_HD uint32_t peek32() const { return (uint32_t)buf; }
  MC_INF_HD void drop(uint32_t k) {
    buf >>= k;
    cnt -= k;
  }
  MC_INF_HD void align() { drop(cnt & 7u); }
  // the next unread byte (after align())
  MC_INF_HD uint32_t bytepos() const { return 4u * nd - (cnt >> 3); }
  // bits were taken from past the frame's end
  MC_INF_HD bool truncated() const {
    const int32_t over = (int32_t)(4u * nd) - (int32_t)n;  // bytes of buf's dwords past the end
    return over > 0 && (over > 8 || 8u * (uint32_t)over > cnt);
  }
};

// the host's source: plain memory
struct mc_inf_ptr_src {
  const uint8_t *p;
  uint32_t n;
  MC_INF_HD uint32_t dword(uint32_t i) const {
    uint32_t v = 0;
    for (uint32_t k = 0; k < 4; ++k) {
      const uint64_t at = 4ull * i + k;
      if (at < n) v |= (uint32_t)p[at] << (8 * k);
    }
    return v;
  }
};

// ---- tables ------------------------------------------------------------------
// The canonical walk: the code that `bits` (first bit lowest) begins with, as
// MC_INF_ENTRY(symbol, length), 0 if no code of at most maxlen bits matches.
MC_INF_HD uint32_t mc_inf_walk(const uint16_t *count, const uint16_t *sym, uint32_t bits, uint32_t maxlen) {
  uint32_t code = 0, first = 0, index = 0;
  for (uint32_t len = 1; len <= maxlen; ++len) {
    code |= bits & 1u;
    bits >>= 1;
    const uint32_t c = count[len];
    if (code - first < c) return MC_INF_ENTRY(sym[index + (code - first)], len);  // index + c <= the symbols counted
    index += c;
    first = (first + c) << 1;
    code <<= 1;
  }
  return 0;
}

// kinds of code, for the completeness rule
#define MC_INF_K_CODES 0
#define MC_INF_K_LENS 1
#define MC_INF_K_DISTS 2

// inftrees.c's check of the counts count[1..15]: 0, or 1 for an over-subscribed
// or a wrongly incomplete set.  *incomplete: unused codes exist (all of them
// invalid codes of 1 bit, by the rule above).
MC_INF_HD int mc_inf_check_counts(const uint32_t *count, int kind, uint32_t *incomplete) {
  int32_t left = 1;
  uint32_t maxlen = 0;
#pragma unroll
  for (uint32_t len = 1; len <= 15; ++len) {
    left <<= 1;
    left -= (int32_t)count[len];
    if (left < 0) return 1;
    if (count[len]) maxlen = len;
  }
  *incomplete = left > 0;
  if (maxlen == 0) return 0;
  return (left > 0 && (kind == MC_INF_K_CODES || maxlen != 1)) ? 1 : 0;
}

// entries [lane, lane + nlanes, ...) of a primary lookup of pbits bits
MC_INF_HD void mc_inf_fill_primary(uint16_t *pri, uint32_t pbits, const uint16_t *count, const uint16_t *sym,
                                   uint32_t incomplete, uint32_t lane, uint32_t nlanes) {
  for (uint32_t i = lane; i < (1u << pbits); i += nlanes) {
    uint32_t e = mc_inf_walk(count, sym, i, pbits);
    if (e == 0 && incomplete) e = MC_INF_ENTRY(MC_INF_INVALID, 1);
    pri[i] = (uint16_t)e;
  }
}

// the next symbol of a code, as MC_INF_ENTRY(symbol, length >= 1); bits: 15 bits ahead
MC_INF_HD uint32_t mc_inf_decode(const uint16_t *pri, uint32_t pbits, const uint16_t *count, const uint16_t *sym,
                                 uint32_t bits) {
  uint32_t e = MC_INF_UNI(pri[bits & ((1u << pbits) - 1u)]);
  if (e == 0) {
    e = MC_INF_UNI(mc_inf_walk(count, sym, bits, 15));
    if (e == 0) e = MC_INF_ENTRY(MC_INF_INVALID, 1);  // (a complete code matches every 15 bits)
  }
  return e;
}

// the host's builder: scalar.  A builder turns n code lengths into count[] /
// sym[] (+ the primary lookup) and answers 0 or 1 (refused).
struct mc_inf_scalar_builder {
  MC_INF_HD void sync() {}
  MC_INF_HD void set_lens(uint8_t *lens, uint32_t at, uint32_t rep, uint32_t val) {
    for (uint32_t k = 0; k < rep; ++k) lens[at + k] = (uint8_t)val;
  }
  MC_INF_HD void fixed_lens(uint8_t *lens) {
    for (uint32_t s = 0; s < 288; ++s) lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
    for (uint32_t s = 288; s < 320; ++s) lens[s] = 5;
  }
  MC_INF_HD int build(const uint8_t *lens, uint32_t n, int kind, uint16_t *count, uint16_t *sym, uint16_t *pri,
                      uint32_t pbits, uint32_t *incomplete) {
    uint32_t cnt[16], offs[16];
    for (uint32_t l = 0; l < 16; ++l) cnt[l] = 0;
    for (uint32_t s = 0; s < n; ++s) ++cnt[lens[s] & 15u];
    if (mc_inf_check_counts(cnt, kind, incomplete)) return 1;
    offs[1] = 0;
    for (uint32_t l = 1; l < 15; ++l) offs[l + 1] = offs[l] + cnt[l];
    for (uint32_t l = 0; l < 16; ++l) count[l] = (uint16_t)(l ? cnt[l] : 0);
    for (uint32_t s = 0; s < n; ++s)
      if (lens[s] & 15u) sym[offs[lens[s] & 15u]++] = (uint16_t)s;
    if (pri) mc_inf_fill_primary(pri, pbits, count, sym, *incomplete, 0, 1);
    return 0;
  }
};

// ---- the block walker --------------------------------------------------------
// base value and extra bits of length symbol 257 + i (i < 29) and of distance symbol d (d < 30)
MC_INF_HD uint32_t mc_inf_len_extra(uint32_t i) { return (i < 8u || i == 28u) ? 0u : (i - 4u) >> 2; }
MC_INF_HD uint32_t mc_inf_len_base(uint32_t i) {
  return i < 8u ? 3u + i : i == 28u ? 258u : ((4u + (i & 3u)) << mc_inf_len_extra(i)) + 3u;
}
MC_INF_HD uint32_t mc_inf_dist_extra(uint32_t d) { return d < 4u ? 0u : (d >> 1) - 1u; }
MC_INF_HD uint32_t mc_inf_dist_base(uint32_t d) { return d < 4u ? d + 1u : ((2u + (d & 1u)) << mc_inf_dist_extra(d)) + 1u; }

// The code lengths of a dynamic block and its two tables.
template <class Bits, class Builder>
MC_INF_HD int mc_inf_dynamic_tables(Bits &br, Builder &bld, mc_inf_tables *T, uint32_t *lit_incomplete,
                                    uint32_t *dist_incomplete) {
  br.fill();
  const uint32_t v = br.peek(14);
  br.drop(14);
  if (br.truncated()) return MC_INF_E_TRUNCATED;
  const uint32_t nlen = (v & 31u) + 257u, ndist = ((v >> 5) & 31u) + 1u, ncode = (v >> 10) + 4u;
  if (nlen > 286u || ndist > 30u) return MC_INF_E_SYMBOLS;
  bld.set_lens(T->cl_lens, 0, 19, 0);
  bld.sync();
  for (uint32_t i = 0; i < ncode; ++i) {
    // 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15, five bits each
    const uint32_t slot = i < 12u ? (uint32_t)((0x22caa324e804a30ull >> (5u * i)) & 31u)
                                  : (uint32_t)((0x3c2e1346cull >> (5u * (i - 12u))) & 31u);
    br.fill();
    T->cl_lens[slot] = (uint8_t)br.peek(3);
    br.drop(3);
  }
  if (br.truncated()) return MC_INF_E_TRUNCATED;
  bld.sync();
  uint32_t cl_incomplete;
  if (bld.build(T->cl_lens, 19, MC_INF_K_CODES, T->cl_count, T->cl_sym, (uint16_t *)0, 0, &cl_incomplete))
    return MC_INF_E_CODELENS;
  bld.sync();
  const uint32_t total = nlen + ndist;
  uint32_t have = 0, prev = 0;
  while (have < total) {
    br.fill();
    uint32_t e = MC_INF_UNI(mc_inf_walk(T->cl_count, T->cl_sym, br.peek(7), 7));
    if (e == 0) e = MC_INF_ENTRY(0, 1);  // only the empty code-length code leaves codes unused: length 0, 1 bit
    const uint32_t sym = e & 511u, l = e >> 9;
    if (sym < 16u) {
      br.drop(l);
      if (br.truncated()) return MC_INF_E_TRUNCATED;
      bld.set_lens(T->lens, have, 1, sym);
      prev = sym;
      ++have;
      continue;
    }
    const uint32_t xb = sym == 16u ? 2u : sym == 17u ? 3u : 7u;
    const uint32_t x = (br.peek(l + xb) >> l) & ((1u << xb) - 1u);
    br.drop(l + xb);
    if (br.truncated()) return MC_INF_E_TRUNCATED;
    if (sym == 16u && have == 0) return MC_INF_E_REPEAT;
    const uint32_t val = sym == 16u ? prev : 0u;
    const uint32_t rep = (sym == 18u ? 11u : 3u) + x;
    if (have + rep > total) return MC_INF_E_REPEAT;
    bld.set_lens(T->lens, have, rep, val);
    prev = val;
    have += rep;
  }
  bld.sync();
  if (MC_INF_UNI(T->lens[256]) == 0) return MC_INF_E_NO_EOB;
  if (bld.build(T->lens, nlen, MC_INF_K_LENS, T->lit_count, T->lit_sym, T->lit_pri, MC_INF_LIT_BITS, lit_incomplete))
    return MC_INF_E_LITLEN_SET;
  if (bld.build(T->lens + nlen, ndist, MC_INF_K_DISTS, T->dist_count, T->dist_sym, T->dist_pri, MC_INF_DIST_BITS,
                dist_incomplete))
    return MC_INF_E_DIST_SET;
  bld.sync();
  return MC_INF_OK;
}

template <class Builder>
MC_INF_HD void mc_inf_fixed_tables(Builder &bld, mc_inf_tables *T) {
  uint32_t inc;
  bld.fixed_lens(T->lens);
  bld.sync();
  bld.build(T->lens, 288, MC_INF_K_LENS, T->lit_count, T->lit_sym, T->lit_pri, MC_INF_LIT_BITS, &inc);
  bld.build(T->lens + 288, 32, MC_INF_K_DISTS, T->dist_count, T->dist_sym, T->dist_pri, MC_INF_DIST_BITS, &inc);
  bld.sync();
}

// The symbols of one compressed block, to its end-of-block code.
template <class Bits, class Sink>
MC_INF_HD int mc_inf_symbols(Bits &br, Sink &out, const mc_inf_tables *T) {
  for (;;) {
    br.fill();
    uint32_t e = mc_inf_decode(T->lit_pri, MC_INF_LIT_BITS, T->lit_count, T->lit_sym, br.peek(15));
    uint32_t sym = e & 511u, l = e >> 9;
    if (sym < 256u) {
      br.drop(l);
      if (br.truncated()) return MC_INF_E_TRUNCATED;
      if (!out.literal(sym)) return MC_INF_E_CAPACITY;
      continue;
    }
    if (sym == 256u || sym >= 286u) {
      br.drop(l);
      if (br.truncated()) return MC_INF_E_TRUNCATED;
      return sym == 256u ? MC_INF_OK : MC_INF_E_LITLEN_CODE;
    }
    uint32_t xb = mc_inf_len_extra(sym - 257u);
    const uint32_t len = mc_inf_len_base(sym - 257u) + ((br.peek(l + xb) >> l) & ((1u << xb) - 1u));
    br.drop(l + xb);
    if (br.truncated()) return MC_INF_E_TRUNCATED;
    br.fill();
    e = mc_inf_decode(T->dist_pri, MC_INF_DIST_BITS, T->dist_count, T->dist_sym, br.peek(15));
    sym = e & 511u, l = e >> 9;
    if (sym >= 30u) {
      br.drop(l);
      if (br.truncated()) return MC_INF_E_TRUNCATED;
      return MC_INF_E_DIST_CODE;
    }
    xb = mc_inf_dist_extra(sym);
    const uint32_t dist = mc_inf_dist_base(sym) + ((br.peek(l + xb) >> l) & ((1u << xb) - 1u));
    br.drop(l + xb);
    if (br.truncated()) return MC_INF_E_TRUNCATED;
    const int me = out.match(len, dist);
    if (me != MC_INF_OK) return me;
  }
}

// The blocks from the reader's position to BFINAL.  Sink: literal(byte) ->
// false when the capacity is reached; match(len, dist) and stored(frame byte,
// len) -> 0 or an error, nothing of the piece written then.
template <class Bits, class Sink, class Builder>
MC_INF_HD int mc_inf_blocks(Bits &br, Sink &out, Builder &bld, mc_inf_tables *T) {
  for (;;) {
    br.fill();
    const uint32_t hdr = br.peek(3);
    br.drop(3);
    if (br.truncated()) return MC_INF_E_TRUNCATED;
    const uint32_t last = hdr & 1u, type = hdr >> 1;
    int e = MC_INF_OK;
    if (type == 0u) {
      br.align();
      br.fill();
      const uint32_t v = br.peek32();
      br.drop(32);
      if (br.truncated()) return MC_INF_E_TRUNCATED;
      const uint32_t len = v & 0xffffu;
      if (len != ((~v >> 16) & 0xffffu)) return MC_INF_E_STORED;
      const uint32_t pos = br.bytepos();  // <= n: not truncated
      if (len > br.n - pos) return MC_INF_E_TRUNCATED;
      e = out.stored(pos, len);
      if (e == MC_INF_OK) br.seek(pos + len);
    } else if (type == 3u) {
      return MC_INF_E_BTYPE;
    } else {
      uint32_t li = 0, di = 0;
      if (type == 1u) mc_inf_fixed_tables(bld, T);
      else e = mc_inf_dynamic_tables(br, bld, T, &li, &di);
      if (e == MC_INF_OK) e = mc_inf_symbols(br, out, T);
    }
    if (e != MC_INF_OK) return e;
    if (last) return MC_INF_OK;
  }
}

// ---- the scalar model --------------------------------------------------------
struct mc_inf_ptr_sink {
  const uint8_t *frame;
  uint8_t *dst;  // NULL: count only
  uint32_t cap, op;
  MC_INF_HD bool literal(uint32_t b) {
    if (op >= cap) return false;
    if (dst) dst[op] = (uint8_t)b;
    ++op;
    return true;
  }
  MC_INF_HD int match(uint32_t len, uint32_t dist) {
    if (dist > op) return MC_INF_E_FAR;
    if (len > cap - op) return MC_INF_E_CAPACITY;
    if (dst)
      for (uint32_t k = 0; k < len; ++k) dst[op + k] = dst[op + k - dist];  // byte-serial by definition
    op += len;
    return MC_INF_OK;
  }
  MC_INF_HD int stored(uint32_t pos, uint32_t len) {
    if (len > cap - op) return MC_INF_E_CAPACITY;
    if (dst)
      for (uint32_t k = 0; k < len; ++k) dst[op + k] = frame[pos + k];
    op += len;
    return MC_INF_OK;
  }
};

MC_INF_HD uint32_t mc_inf_adler32(const uint8_t *p, uint32_t n) {
  uint32_t a = 1, b = 0;
  for (uint32_t i = 0; i < n; ++i) {
    a = (a + p[i]) % 65521u;
    b = (b + a) % 65521u;
  }
  return (b << 16) | a;
}
MC_INF_HD uint32_t mc_inf_crc32(const uint8_t *p, uint32_t n) {
  uint32_t c = 0xffffffffu;
  for (uint32_t i = 0; i < n; ++i) {
    c ^= p[i];
    for (int k = 0; k < 8; ++k) c = (c >> 1) ^ ((c & 1u) ? 0xedb88320u : 0u);
  }
  return ~c;
}

// One frame f[0, n) into at most cap bytes at dst; dst == NULL only counts (up
// to cap) and skips the trailer.  Returns 0 or an mc_inf_error; *produced =
// bytes written (counted), *consumed = the byte behind the trailer (behind the
// DEFLATE data when counting, or where an error stopped the reader), *word =
// the error record's second word: the computed checksum for a data-check
// error, *produced otherwise.
MC_INF_HD int mc_inflate_stream(const uint8_t *f, uint64_t n, uint32_t container, uint8_t *dst, uint32_t cap,
                                uint32_t *produced, uint64_t *consumed, uint32_t *word, mc_inf_tables *T) {
  *produced = 0, *consumed = 0, *word = 0;
  if (n >= MC_INF_MAX_BYTES || cap >= MC_INF_MAX_BYTES) return MC_INF_E_TABLE;
  uint32_t data_off, empty;
  int e = mc_inf_parse_header(f, n, container, &data_off, &empty);
  if (e != MC_INF_OK || empty) return e;
  mc_inf_ptr_src src{f, (uint32_t)n};
  mc_inf_bits<mc_inf_ptr_src> br(src, (uint32_t)n);
  br.seek(data_off);
  mc_inf_ptr_sink out{f, dst, cap, 0};
  mc_inf_scalar_builder bld;
  e = mc_inf_blocks(br, out, bld, T);
  *produced = *word = out.op;
  br.align();
  const uint32_t pos = br.bytepos();
  *consumed = pos < n ? pos : n;
  if (e != MC_INF_OK || !dst) return e;
  const uint32_t check = container == MC_INF_ZLIB ? mc_inf_adler32(dst, out.op) : mc_inf_crc32(dst, out.op);
  uint64_t after;
  e = mc_inf_check_trailer(f, n, pos, container, check, out.op, &after);
  *consumed = after;
  if (e == MC_INF_E_CHECK) *word = check;
  if (e != MC_INF_OK || container == MC_INF_ZLIB) return e;
  uint64_t q = after;
  while (q < n && f[q] == 0) ++q;
  return mc_inf_after_trailer(f, n, q);
}
