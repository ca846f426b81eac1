// mc_bz2_enc.h -- bzip2 encode: the format decisions, the bound, the error
// codes and the scalar model whose bytes the gfx950 kernels of mc_bz2_enc.hip
// reproduce exactly.  Compiled for the host (tests/native_bz2_enc) and the
// device.  The frames are valid bzip2 (libbz2 1.0.8 and csrc/mc_bz2.h decode
// them); they are not libbz2's bytes.
//
// Block cut.  A chunk of n bytes is cut into independent input segments of
// S(level) = 80000 * level - 16 bytes; each becomes one block.  RLE1 (a run of
// 4..255 equal bytes -> four bytes and a count byte) is applied per segment, a
// run never crosses a segment, so no block ends where a count byte is due.
// RLE1 gives at most floor(5 nk / 4) symbols for nk bytes: at most
// 100000 * level - 20 a block.  The block CRC is the CRC of the segment's
// input bytes, the stream CRC the rotate-and-xor chain over the blocks.
//
// Forward BWT.  The nblock cyclic rotations of the RLE1'd block are sorted by
// prefix doubling: after the first pass (a counting sort by the first byte)
// rank[i] is the number of rotations whose first h bytes are strictly smaller
// than rotation i's; a round orders the rotations by (rank[i], rank[i + h mod
// nblock]) and doubles h.  It stops when every rank is unique or h >= nblock:
// at most ceil(log2 nblock) rounds of linear work, whatever the block (the
// all-zero block included).  The column is the byte before each rotation;
// origPtr is the number of rotations strictly smaller than rotation 0, that
// is rank[0] at the end.  Equal rotations have equal preceding bytes, so
// neither depends on how ties were ordered: the model's counting sorts and the
// kernel's radix passes give the same column and origPtr.  The randomised bit
// is never set.
//
// MTF and zero runs: the in-use byte values in order form the list; a run of
// r list-front hits is written in bijective base 2 (RUNA = 1, RUNB = 2, low
// digit first); symbol j + 1 for list position j >= 1; EOB = in-use count + 1.
//
// Huffman, libbz2's shape: nGroups 2..6 from the symbol count (below 200, 600,
// 1200, 2400), groups of 50 symbols, a selector per group, the selectors
// move-to-front coded and written in unary, the code lengths delta coded.
// The tables come from libbz2's scheme in integers: a first split of the
// alphabet into nGroups ranges of about equal frequency (length 0 inside the
// range, 15 outside), then MC_BZ2E_ITERS passes, each giving every group to its
// cheapest table (the lowest index on a tie) and rebuilding every table's
// lengths from the frequencies of its groups (a symbol without one counts 1)
// with mc_deflate.h's length-limited builder at 15 bits.  The selectors are the
// last pass's.
//
// Bound by construction.  bzip2 has no stored block.  The code stage has the
// exact bit cost of the block with the refined tables, and with a fallback:
// two tables of equal-length codes of F = ceil(log2 alphaSize) bits, every
// selector 0.  It writes the smaller (the refined tables on a tie).  The
// fallback of a block of nk input bytes costs at most
//   48 + 32 + 1 + 24 (magic, CRC, randomised, origPtr) + 16 + 256 (symbol map)
//   + 3 + 15 (nGroups, nSelectors) + nsel (one bit a selector)
//   + 2 * (5 + 258) (two tables: 5 bits, then one bit a symbol)
//   + 9 * nmtf
// bits with nmtf <= floor(5 nk / 4) + 1 (a zero run takes no more symbols than
// it has bytes; then EOB) and nsel = ceil(nmtf / 50).  mc_bz2_enc_bound(n,
// level) is the sum over the blocks, plus 32 bits of stream header and 80 of
// end magic and stream CRC, rounded up to bytes.  No frame exceeds it.  A
// destination shorter than the frame is refused (MC_BZ2E_E_SPACE) and left
// untouched.
//
// Bit layout.  Blocks follow one another at bit granularity.  The layout
// stage clears the frame's bytes and writes the stream header and trailer;
// every block then ORs its bits in: a byte shared by two neighbouring blocks
// is OR-ed by both.  On the device the unit is the aligned dword: the first
// and the last dword of a block's span are OR-ed atomically, the dwords
// between them, which are the block's alone, are stored.
#pragma once

#include <stdlib.h>
#include <string.h>

#include "mc_bz2.h"
#include "mc_deflate.h"  // mc_dfl_code_lengths: the length-limited code-length builder

#define MC_BZ2E_MAX_BYTES 0x40000000u
#define MC_BZ2E_ITERS 4u
#define MC_BZ2E_GROUP 50u
#define MC_BZ2E_MAXLEN 15u
#define MC_BZ2E_LROW 264u  // a table's row of lengths (258 used)

#define MC_BZ2E_E_SPACE 1  // the frame does not fit its destination; second word: the frame's size
#define MC_BZ2E_E_TABLE 2  // the caller's chunk record is out of range

// One chunk of a batch (device table; include/mcodec.h).
struct mc_bz2e_chunk {
  uint64_t src;
  uint64_t dst;
  uint32_t nbytes;
  uint32_t dst_cap;
  uint32_t block_base;  // the chunk's first block in the batch
  uint32_t reserved;
};

// One block, as the stages leave it for one another.
struct mc_bz2e_block {
  uint32_t nblock, crc, orig, ninuse, nmtf, ngroups, nsel, bits;
  uint64_t bitoff;   // of the block's first bit in the frame
  uint32_t used[8];  // the in-use map, byte value v at bit v & 31 of word v >> 5
  uint32_t chunk, k;
};

MC_BZ2_HD uint32_t mc_bz2e_seg(uint32_t level) { return 80000u * level - 16u; }
MC_BZ2_HD uint32_t mc_bz2e_nblocks(uint32_t n, uint32_t level) {
  const uint32_t s = mc_bz2e_seg(level);
  return n / s + (n % s != 0u);
}
MC_BZ2_HD uint32_t mc_bz2e_seg_len(uint32_t n, uint32_t level, uint32_t k) {
  const uint32_t s = mc_bz2e_seg(level), at = k * s;
  return n - at < s ? n - at : s;
}
MC_BZ2_HD uint64_t mc_bz2e_block_bound_bits(uint64_t nk) {
  const uint64_t nmtf = nk + nk / 4u + 1u, nsel = (nmtf + MC_BZ2E_GROUP - 1u) / MC_BZ2E_GROUP;
  return 48u + 32u + 1u + 24u + 16u + 256u + 3u + 15u + nsel + 2u * (5u + 258u) + 9u * nmtf;
}
MC_BZ2_HD uint64_t mc_bz2_enc_bound(uint64_t n, uint32_t level) {
  const uint64_t s = mc_bz2e_seg(level), full = n / s, rest = n % s;
  const uint64_t bits = 32u + 80u + full * mc_bz2e_block_bound_bits(s) + (rest ? mc_bz2e_block_bound_bits(rest) : 0u);
  return (bits + 7u) / 8u;
}

// the most symbols a block of nk input bytes holds, rounded up to 64
MC_BZ2_HD uint32_t mc_bz2e_cap(uint32_t nk) { return (nk + nk / 4u + 63u) & ~63u; }
// the per-block arrays of the workspace, for blocks of at most cap symbols (a
// multiple of 64): the RLE1'd block, the column, the MTF symbols (at most cap +
// 1, stored 64 at a time), the selectors and their move-to-front positions,
// the lengths
MC_BZ2_HD uint64_t mc_bz2e_sel_room(uint32_t cap) { return ((uint64_t)cap / MC_BZ2E_GROUP + 15u) & ~7ull; }
MC_BZ2_HD uint64_t mc_bz2e_block_stride(uint32_t cap) {
  return (4ull * cap + 128u + 2u * mc_bz2e_sel_room(cap) + 6u * MC_BZ2E_LROW + 255u) & ~255ull;
}
struct mc_bz2e_arrays {
  uint8_t *rle, *col;
  uint16_t *sym;
  uint8_t *sel, *selmtf, *lens;
};
MC_BZ2_HD mc_bz2e_arrays mc_bz2e_arrays_at(uint8_t *base, uint32_t cap) {
  const uint64_t sr = mc_bz2e_sel_room(cap);
  mc_bz2e_arrays a;
  a.rle = base, a.col = base + cap, a.sym = reinterpret_cast<uint16_t *>(base + 2ull * cap);
  a.sel = base + 4ull * cap + 128u, a.selmtf = a.sel + sr, a.lens = a.selmtf + sr;
  return a;
}

MC_BZ2_HD uint32_t mc_bz2e_ngroups(uint32_t nmtf) {
  return nmtf < 200u ? 2u : nmtf < 600u ? 3u : nmtf < 1200u ? 4u : nmtf < 2400u ? 5u : 6u;
}
MC_BZ2_HD uint32_t mc_bz2e_flat_len(uint32_t alpha) {  // ceil(log2 alpha), alpha >= 3
  uint32_t f = 2;
  while ((1u << f) < alpha) ++f;
  return f;
}

// libbz2's first split: table t takes a range of the alphabet of about 1 / t
// of what is left of the frequency
MC_BZ2_HD void mc_bz2e_initial_split(const uint32_t *freq, uint32_t alpha, uint32_t nmtf, uint32_t ngroups, uint8_t *lens) {
  int32_t gs = 0, remf = (int32_t)nmtf;
  for (uint32_t npart = ngroups; npart > 0; --npart) {
    const int32_t tfreq = remf / (int32_t)npart;
    int32_t ge = gs - 1, afreq = 0;
    while (afreq < tfreq && ge < (int32_t)alpha - 1) afreq += (int32_t)freq[++ge];
    if (ge > gs && npart != ngroups && npart != 1u && ((ngroups - npart) % 2u == 1u)) afreq -= (int32_t)freq[ge--];
    uint8_t *row = lens + (npart - 1u) * MC_BZ2E_LROW;
    for (int32_t v = 0; v < (int32_t)alpha; ++v) row[v] = (v >= gs && v <= ge) ? 0u : (uint8_t)MC_BZ2E_MAXLEN;
    gs = ge + 1, remf -= afreq;
  }
}

// the six lengths of a symbol in 10-bit fields: a group's six costs in one sum
MC_BZ2_HD uint64_t mc_bz2e_pack_lens(const uint8_t *lens, uint32_t ngroups, uint32_t v) {
  uint64_t p = 0;
  for (uint32_t t = 0; t < ngroups; ++t) p |= (uint64_t)lens[t * MC_BZ2E_LROW + v] << (10u * t);
  return p;
}
// the cheapest table of a group (the lowest index on a tie) and its cost
MC_BZ2_HD uint32_t mc_bz2e_best(uint64_t acc, uint32_t ngroups, uint32_t *cost) {
  uint32_t bt = 0, bc = (uint32_t)acc & 1023u;
  for (uint32_t t = 1; t < ngroups; ++t) {
    const uint32_t c = (uint32_t)(acc >> (10u * t)) & 1023u;
    if (c < bc) bc = c, bt = t;
  }
  *cost = bc;
  return bt;
}
// the selectors' move-to-front positions; returns their bits in unary
MC_BZ2_HD uint32_t mc_bz2e_sel_mtf(const uint8_t *sel, uint32_t nsel, uint8_t *selmtf) {
  uint32_t order = 0x543210u, bits = 0;
  for (uint32_t i = 0; i < nsel; ++i) {
    const uint32_t g = sel[i];
    uint32_t j = 0;
    while (((order >> (4u * j)) & 15u) != g) ++j;
    const uint32_t sh = 4u * j;
    order = (order & ~((16u << sh) - 1u)) | ((order & ((1u << sh) - 1u)) << 4) | g;
    selmtf[i] = (uint8_t)j;
    bits += j + 1u;
  }
  return bits;
}
// a table's delta-coded lengths: 5 bits, then per symbol two bits a step and a 0
MC_BZ2_HD uint32_t mc_bz2e_lens_bits(const uint8_t *row, uint32_t alpha) {
  uint32_t bits = 5, curr = row[0];
  for (uint32_t i = 0; i < alpha; ++i) {
    const uint32_t l = row[i];
    bits += 2u * (l > curr ? l - curr : curr - l) + 1u;
    curr = l;
  }
  return bits;
}
// the canonical code of symbol s (hbAssignCodes)
MC_BZ2_HD uint32_t mc_bz2e_code(const uint8_t *row, uint32_t alpha, uint32_t s) {
  const uint32_t l = row[s];
  uint32_t code = 0;
  for (uint32_t j = 0; j < alpha; ++j) {
    const uint32_t lj = row[j];
    if (lj < l) code += 1u << (l - lj);
    else if (lj == l && j < s) code += 1u;
  }
  return code;
}
// the fixed fields of a block and its symbol map
MC_BZ2_HD uint32_t mc_bz2e_used16(const uint32_t *used) {
  uint32_t u = 0;
  for (uint32_t i = 0; i < 16; ++i)
    if ((used[i >> 1] >> (16u * (i & 1u))) & 0xffffu) u |= 0x8000u >> i;
  return u;
}
MC_BZ2_HD uint32_t mc_bz2e_map16(const uint32_t *used, uint32_t i) {  // values 16 i .. 16 i + 15, the first highest
  const uint32_t w = (used[i >> 1] >> (16u * (i & 1u))) & 0xffffu;
  return __builtin_bitreverse32(w) >> 16;
}
MC_BZ2_HD uint32_t mc_bz2e_fixed_bits(const uint32_t *used) {
  return 48u + 32u + 1u + 24u + 16u + 16u * (uint32_t)__builtin_popcount(mc_bz2e_used16(used)) + 3u + 15u;
}
// the delta code of one length after `prev`: value and bit count (at most 29)
MC_BZ2_HD uint32_t mc_bz2e_delta(uint32_t prev, uint32_t l, uint32_t *nb) {
  const uint32_t d = l > prev ? l - prev : prev - l;
  // "10" a step up, "11" a step down, then "0"
  const uint32_t pat = l > prev ? 0xaaaaaaaau : 0xffffffffu;
  *nb = 2u * d + 1u;
  return d ? (pat >> (32u - 2u * d)) << 1 : 0u;
}

#ifndef __HIP_DEVICE_COMPILE__
// ---- the scalar model (host) -----------------------------------------------------
static inline uint32_t mc_bz2e_rle1(const uint8_t *src, uint32_t n, uint8_t *out) {
  uint32_t o = 0, i = 0;
  while (i < n) {
    const uint8_t b = src[i];
    uint32_t run = 1;
    while (i + run < n && src[i + run] == b && run < 255u) ++run;
    for (uint32_t k = 0; k < (run < 4u ? run : 4u); ++k) out[o++] = b;
    if (run >= 4u) out[o++] = (uint8_t)(run - 4u);
    i += run;
  }
  return o;
}

// blk[0, n), n >= 1 -> col[0, n) and origPtr; w: 4 n dwords
static inline uint32_t mc_bz2e_bwt_model(const uint8_t *blk, uint32_t n, uint8_t *col, uint32_t *w, uint32_t *rounds_out) {
  uint32_t *sa = w, *tmp = w + n, *rank = w + 2ull * n, *rank2 = w + 3ull * n;
  uint32_t start[257] = {0};
  for (uint32_t i = 0; i < n; ++i) ++start[blk[i] + 1u];
  for (uint32_t v = 0; v < 256; ++v) start[v + 1] += start[v];
  uint32_t groups = 0;
  for (uint32_t v = 0; v < 256; ++v) groups += start[v + 1] != start[v];
  {
    uint32_t pos[256];
    for (uint32_t v = 0; v < 256; ++v) pos[v] = start[v];
    for (uint32_t i = 0; i < n; ++i) sa[pos[blk[i]]++] = i, rank[i] = start[blk[i]];
  }
  uint32_t rounds = 0;
  for (uint32_t h = 1; groups < n && h < n; h *= 2u, ++rounds) {
    for (uint32_t j = 0; j < n; ++j) tmp[j] = (sa[j] + n - h) % n;  // ordered by the second key
    for (uint32_t j = 0; j < n; ++j) rank2[j] = 0;                  // a counter per group, at its start
    for (uint32_t j = 0; j < n; ++j) {
      const uint32_t i = tmp[j], g = rank[i];
      sa[g + rank2[g]++] = i;
    }
    groups = 0;
    uint32_t cur = 0;
    for (uint32_t j = 0; j < n; ++j) {
      const uint32_t i = sa[j];
      if (j == 0 || rank[i] != rank[sa[j - 1]] || rank[(i + h) % n] != rank[(sa[j - 1] + h) % n]) cur = j, ++groups;
      tmp[i] = cur;
    }
    for (uint32_t i = 0; i < n; ++i) rank[i] = tmp[i];
  }
  for (uint32_t j = 0; j < n; ++j) col[j] = blk[(sa[j] + n - 1u) % n];
  if (rounds_out) *rounds_out = rounds;
  return rank[0];
}

// col[0, n) -> sym[0, nmtf) and freq[0, ninuse + 2); seq: byte value -> list index
static inline uint32_t mc_bz2e_mtf_model(const uint8_t *col, uint32_t n, const uint8_t *index, uint32_t ninuse, uint16_t *sym,
                                         uint32_t *freq) {
  uint8_t list[256];
  for (uint32_t i = 0; i < ninuse; ++i) list[i] = (uint8_t)i;
  for (uint32_t i = 0; i < ninuse + 2u; ++i) freq[i] = 0;
  uint32_t nmtf = 0, zrun = 0;
  auto flush = [&]() {
    while (zrun > 0) {
      const uint32_t s = (zrun & 1u) ? 0u : 1u;
      sym[nmtf++] = (uint16_t)s, ++freq[s];
      zrun = (zrun - 1u - s) >> 1;
    }
  };
  for (uint32_t i = 0; i < n; ++i) {
    const uint8_t v = index[col[i]];
    if (list[0] == v) {
      ++zrun;
      continue;
    }
    flush();
    uint32_t j = 1;
    while (list[j] != v) ++j;
    for (uint32_t k = j; k > 0; --k) list[k] = list[k - 1];
    list[0] = v;
    sym[nmtf++] = (uint16_t)(j + 1u), ++freq[j + 1u];
  }
  flush();
  sym[nmtf++] = (uint16_t)(ninuse + 1u), ++freq[ninuse + 1u];
  return nmtf;
}

// sym[0, nmtf), freq -> lens (6 rows), sel, selmtf, and the block's choice;
// fills b->ngroups, nsel, bits.  Returns 1 where the fallback was taken.
static inline int mc_bz2e_code_model(const uint16_t *sym, const uint32_t *freq, mc_bz2e_block *b, uint8_t *lens, uint8_t *sel,
                                     uint8_t *selmtf) {
  const uint32_t alpha = b->ninuse + 2u, nmtf = b->nmtf, ngroups = mc_bz2e_ngroups(nmtf);
  const uint32_t nsel = (nmtf + MC_BZ2E_GROUP - 1u) / MC_BZ2E_GROUP;
  static thread_local mc_dfl_work W;
  static thread_local uint32_t rfreq[6][MC_BZ2E_LROW];
  uint64_t len64[MC_BZ2_MAX_ALPHA];
  mc_dfl_scalar x;
  mc_bz2e_initial_split(freq, alpha, nmtf, ngroups, lens);
  uint32_t symbits = 0;
  for (uint32_t it = 0; it <= MC_BZ2E_ITERS; ++it) {  // the last pass only prices the selectors it has
    const bool price = it == MC_BZ2E_ITERS;
    for (uint32_t v = 0; v < alpha; ++v) len64[v] = mc_bz2e_pack_lens(lens, ngroups, v);
    for (uint32_t t = 0; t < ngroups; ++t)
      for (uint32_t v = 0; v < alpha; ++v) rfreq[t][v] = 0;
    for (uint32_t g = 0; g < nsel; ++g) {
      const uint32_t at = g * MC_BZ2E_GROUP, cnt = nmtf - at < MC_BZ2E_GROUP ? nmtf - at : MC_BZ2E_GROUP;
      uint64_t acc = 0;
      for (uint32_t k = 0; k < cnt; ++k) acc += len64[sym[at + k]];
      if (price) {
        symbits += (uint32_t)(acc >> (10u * sel[g])) & 1023u;
        continue;
      }
      uint32_t cost;
      const uint32_t bt = mc_bz2e_best(acc, ngroups, &cost);
      sel[g] = (uint8_t)bt;
      for (uint32_t k = 0; k < cnt; ++k) ++rfreq[bt][sym[at + k]];
    }
    if (price) break;
    for (uint32_t t = 0; t < ngroups; ++t) {
      for (uint32_t v = 0; v < alpha; ++v) rfreq[t][v] = rfreq[t][v] ? rfreq[t][v] : 1u;
      mc_dfl_code_lengths(x, &W, rfreq[t], alpha, MC_BZ2E_MAXLEN, lens + t * MC_BZ2E_LROW);
    }
  }
  uint32_t refined = mc_bz2e_fixed_bits(b->used) + mc_bz2e_sel_mtf(sel, nsel, selmtf) + symbits;
  for (uint32_t t = 0; t < ngroups; ++t) refined += mc_bz2e_lens_bits(lens + t * MC_BZ2E_LROW, alpha);
  const uint32_t flat = mc_bz2e_flat_len(alpha);
  const uint32_t fallback = mc_bz2e_fixed_bits(b->used) + nsel + 2u * (5u + alpha) + flat * nmtf;
  b->nsel = nsel;
  if (fallback < refined) {
    for (uint32_t t = 0; t < 2u; ++t)
      for (uint32_t v = 0; v < alpha; ++v) lens[t * MC_BZ2E_LROW + v] = (uint8_t)flat;
    for (uint32_t g = 0; g < nsel; ++g) sel[g] = 0, selmtf[g] = 0;
    b->ngroups = 2u, b->bits = fallback;
    return 1;
  }
  b->ngroups = ngroups, b->bits = refined;
  return 0;
}

// MSB-first bits OR-ed into bytes that were cleared
struct mc_bz2e_bitw {
  uint8_t *dst;
  uint64_t pos;
  void put(uint32_t v, uint32_t nb) {  // nb <= 32
    for (uint32_t k = 0; k < nb; ++k, ++pos)
      if ((v >> (nb - 1u - k)) & 1u) dst[pos >> 3] |= (uint8_t)(0x80u >> (pos & 7u));
  }
};

static inline void mc_bz2e_emit_model(mc_bz2e_bitw &w, const mc_bz2e_block &b, const uint16_t *sym, const uint8_t *lens,
                                      const uint8_t *sel, const uint8_t *selmtf) {
  const uint32_t alpha = b.ninuse + 2u;
  w.put(0x314159u, 24), w.put(0x265359u, 24);
  w.put(b.crc, 32), w.put(0, 1), w.put(b.orig, 24);
  const uint32_t u16 = mc_bz2e_used16(b.used);
  w.put(u16, 16);
  for (uint32_t i = 0; i < 16; ++i)
    if (u16 & (0x8000u >> i)) w.put(mc_bz2e_map16(b.used, i), 16);
  w.put(b.ngroups, 3), w.put(b.nsel, 15);
  for (uint32_t i = 0; i < b.nsel; ++i) w.put((1u << (selmtf[i] + 1u)) - 2u, selmtf[i] + 1u);
  for (uint32_t t = 0; t < b.ngroups; ++t) {
    const uint8_t *row = lens + t * MC_BZ2E_LROW;
    w.put(row[0], 5);
    uint32_t prev = row[0];
    for (uint32_t v = 0; v < alpha; ++v) {
      uint32_t nb;
      const uint32_t code = mc_bz2e_delta(prev, row[v], &nb);
      w.put(code, nb);
      prev = row[v];
    }
  }
  uint32_t codes[6][MC_BZ2_MAX_ALPHA];
  for (uint32_t t = 0; t < b.ngroups; ++t)
    for (uint32_t v = 0; v < alpha; ++v) codes[t][v] = mc_bz2e_code(lens + t * MC_BZ2E_LROW, alpha, v);
  for (uint32_t i = 0; i < b.nmtf; ++i) {
    const uint32_t t = sel[i / MC_BZ2E_GROUP], s = sym[i];
    w.put(codes[t][s], lens[t * MC_BZ2E_LROW + s]);
  }
}

struct mc_bz2e_census {
  uint64_t blocks, fallback, multi_table, rounds_max, bits;
};

// One chunk src[0, n) at `level` into dst[0, cap): the frame's size, or 0 with
// *err set (a frame is never empty).  dst is untouched when the frame is
// refused.
static inline uint64_t mc_bz2_encode_chunk(const uint8_t *src, uint64_t n, uint8_t *dst, uint64_t cap, uint32_t level,
                                           int *err, mc_bz2e_census *census) {
  *err = 0;
  if (n >= MC_BZ2E_MAX_BYTES || level < 1u || level > 9u) {
    *err = MC_BZ2E_E_TABLE;
    return 0;
  }
  const uint64_t bound = mc_bz2_enc_bound(n, level);
  const uint32_t nb = mc_bz2e_nblocks((uint32_t)n, level);
  uint8_t *frame = (uint8_t *)calloc(bound + 8u, 1);
  const uint32_t room = mc_bz2e_cap(n < mc_bz2e_seg(level) ? (uint32_t)n : mc_bz2e_seg(level));
  uint8_t *area = (uint8_t *)malloc(mc_bz2e_block_stride(room));
  uint32_t *sortw = (uint32_t *)malloc(16ull * room + 16u);
  const mc_bz2e_arrays a = mc_bz2e_arrays_at(area, room);
  mc_bz2e_bitw w{frame, 0};
  w.put(0x425a68u, 24), w.put('0' + level, 8);
  uint32_t combined = 0;
  for (uint32_t k = 0; k < nb; ++k) {
    const uint32_t nk = mc_bz2e_seg_len((uint32_t)n, level, k);
    const uint8_t *seg = src + (uint64_t)k * mc_bz2e_seg(level);
    mc_bz2e_block b;
    memset(&b, 0, sizeof b);
    uint32_t crc = 0xffffffffu;
    for (uint32_t i = 0; i < nk; ++i) crc = mc_bz2_crc_byte(crc, seg[i]);
    b.crc = ~crc;
    b.nblock = mc_bz2e_rle1(seg, nk, a.rle);
    for (uint32_t i = 0; i < b.nblock; ++i) b.used[a.rle[i] >> 5] |= 1u << (a.rle[i] & 31u);
    uint8_t index[256];
    for (uint32_t v = 0; v < 256; ++v) {
      index[v] = (uint8_t)b.ninuse;
      b.ninuse += (b.used[v >> 5] >> (v & 31u)) & 1u;
    }
    uint32_t rounds = 0;
    b.orig = mc_bz2e_bwt_model(a.rle, b.nblock, a.col, sortw, &rounds);
    uint32_t freq[MC_BZ2E_LROW];
    b.nmtf = mc_bz2e_mtf_model(a.col, b.nblock, index, b.ninuse, a.sym, freq);
    const int fb = mc_bz2e_code_model(a.sym, freq, &b, a.lens, a.sel, a.selmtf);
    const uint64_t before = w.pos;
    mc_bz2e_emit_model(w, b, a.sym, a.lens, a.sel, a.selmtf);
    if (w.pos - before != b.bits) *err = -1;  // the priced and the written bits differ: a bug
    combined = ((combined << 1) | (combined >> 31)) ^ b.crc;
    if (census) {
      ++census->blocks, census->fallback += fb, census->bits += b.bits;
      bool multi = false;
      for (uint32_t g = 1; g < b.nsel; ++g) multi |= a.sel[g] != a.sel[0];
      census->multi_table += multi;
      if (rounds > census->rounds_max) census->rounds_max = rounds;
    }
  }
  w.put(0x177245u, 24), w.put(0x385090u, 24), w.put(combined, 32);
  uint64_t size = (w.pos + 7u) / 8u;
  if (*err == 0 && size > bound) *err = -2;
  if (*err == 0 && size > cap) *err = MC_BZ2E_E_SPACE;
  if (*err == 0) memcpy(dst, frame, size);
  else size = 0;
  free(sortw), free(area), free(frame);
  return size;
}
#endif  // !__HIP_DEVICE_COMPILE__
