// mc_deflate.h -- DEFLATE (RFC 1951) compression into the zlib (RFC 1950) and
// gzip (RFC 1952) containers: the rules, shared by the gfx950 kernels
// (mc_deflate.hip) and the host build of the CPU suite (tests/native_deflate).
// mc_deflate_encode_chunk below is the plain scalar statement of the format
// written here; the kernels produce the same bytes for every input.  The code
// construction (mc_dfl_code_lengths, mc_dfl_plan, mc_dfl_codes) is one piece
// of code for both: the host runs it with one "lane", the device with the 64
// lanes of a wave over LDS (loops strided by lane, the serial steps on lane 0).
//
// Segments.  A chunk of n bytes (1 <= n < 2^30) is cut into segments of 65536
// bytes, the last one shorter.  Each segment becomes one DEFLATE block (two, if
// a full segment is stored) with no reference before its start, and its output
// is a whole number of bytes, so the pieces concatenate without bit shifts: a
// compressed segment that is not the chunk's last is followed by an empty
// stored block (3 zero header bits, zero padding to a byte, 00 00 FF FF); the
// last carries BFINAL = 1 and is zero-padded to a byte.
//
// Parse: mc_lz4_enc.h's window-of-64 finder restated with DEFLATE's limits.
//   * positions are consumed in windows of 64 starting at p; slot i owns
//     pos = p + i while pos + 4 <= n.  LZ4's end-of-block restrictions are
//     DROPPED: a match may start wherever four bytes remain and runs to the
//     segment's last byte;
//   * a slot's candidate is table[hash(le32(src + pos))]: 4096 entries, each
//     the latest inserted position with that hash; every lookup of a window
//     sees the table as it was before the window;
//   * a candidate is valid if it exists, cand < pos, pos - cand <= 32768 and
//     its 4-byte word equals the slot's; the lowest slot with one wins;
//   * the match is extended backwards while m > anchor, c > 0 and the preceding
//     bytes are equal, then forwards to the segment's end;
//   * one sequence (literal run, match length >= 4, distance) is recorded;
//   * only the positions consumed from this window are then inserted:
//     p .. min(p + 64, match end) - 1, each while it owns a slot; the highest
//     position wins a shared entry;
//   * p = anchor = match end, or p += 64 when nothing matched; the segment ends
//     with the closing literals.  At most n / 4 sequences.
//   * A match of length L > 258 is written as q + (r != 0) length/distance
//     pairs of the same distance, q = L / 258, r = L % 258: q pairs of 258 and
//     one of r -- unless r is 1 or 2, when the last two pairs are 255 + r and
//     3, so that no pair is shorter than 3 (mc_dfl_piece).
//
// Costs and block type.  From the parse: the histogram of the 286
// literal/length symbols (end-of-block counted once) and of the 30 distance
// symbols, and three exact sizes in bits, each a multiple of 8: stored
// (8 * (n + 5 * ceil(n / 65535)): a full segment needs two stored blocks, and
// no marker follows a stored segment, which ends on a byte anyway), fixed
// Huffman and dynamic Huffman, the latter two with the 3 header bits (dynamic:
// and the code description), the alignment and, unless the segment is the
// last, the marker.  The smallest wins; ties go to stored, then fixed.  Level 0
// forces stored.
//
// Code lengths (mc_dfl_code_lengths): as zlib's build_tree, a set with fewer
// than two symbols of non-zero frequency gets frequency 1 for its lowest
// unused symbols, so no incomplete or one-code table is ever written.  The
// used symbols are sorted by (frequency, symbol), merged by the two-queue
// Huffman construction (a leaf before an internal node of equal weight), the
// depths are cut at the limit (15; 7 for the code-length code) and the
// overflow repaired as zlib's gen_bitlen does; the lengths are then handed out
// in sorted order, the longest to the least frequent symbol, ties by symbol
// index.  The Kraft sum is exactly 1.  HLIT, HDIST and HCLEN are trimmed of
// trailing zeros.  The repeat symbols 16/17/18 are NOT used: every one of the
// HLIT + HDIST lengths is written as its own code-length symbol (some tens of
// bytes per 64 KiB block, for a header every lane can place on its own).
//
// Containers.  zlib: 78 01, the data, the big-endian Adler-32.  gzip: 1F 8B 08
// 00, MTIME 0 (the reference writes the wall clock; the bytes here depend on
// the input alone), XFL 4, OS 255, the data, little-endian CRC-32 and ISIZE.
// n = 0 is written by the caller on the host: the header, 03 00 (a final fixed
// block of end-of-block alone) and the trailer.
//
// Bound.  mc_deflate_bound(n, container) = the container's bytes + over the
// segments n_k + 5 * ceil(n_k / 65535) (+ 2 for n = 0): no frame exceeds it,
// because a segment never takes more than its stored form.  The exact frame
// size is known before a byte is written; a frame that would not fit its slot
// is refused and nothing of it is written.
#pragma once

#include "mc_inflate.h"

#define MC_DFL_HD MC_INF_HD

#define MC_DFL_SEGMENT 65536u
#define MC_DFL_HASH_BITS 12u
#define MC_DFL_TABLE (1u << MC_DFL_HASH_BITS)
#define MC_DFL_WINDOW 64u
#define MC_DFL_MAX_DIST 32768u
#define MC_DFL_MIN_MATCH 4u     // the finder compares 4-byte words
#define MC_DFL_MAX_LEN 258u
#define MC_DFL_MAX_SEQS (MC_DFL_SEGMENT / MC_DFL_MIN_MATCH)
#define MC_DFL_MAX_BYTES 0x40000000u
#define MC_DFL_NLL 286u         // literal/length symbols
#define MC_DFL_ND 30u           // distance symbols
#define MC_DFL_DOFF 288u        // the distance entries of a histogram / length array start here
#define MC_DFL_HIST 320u
#define MC_DFL_LENS 352u        // lengths per segment: 320 + the code-length code's 19 (from 320)

#define MC_DFL_STORED 0u
#define MC_DFL_FIXED 1u
#define MC_DFL_DYNAMIC 2u

// error record of the batch (0 = none)
#define MC_DFL_E_SPACE 1  // the frame does not fit its slot; second word: the frame's size
#define MC_DFL_E_TABLE 2  // the caller's chunk record is out of range

// One sequence of the parse: a = literal run | (distance - 1) << 17, b = match
// length (the closing literals are not a sequence).
struct mc_dfl_seq {
  uint32_t a, b;
};

// One segment, as the kernels leave it in the workspace and the reporting
// form of the scalar encoder hands it to the tests.
struct mc_dfl_seg {
  uint32_t nseq, tail_lit;  // parse: sequences, closing literals
  uint32_t type, bytes;     // MC_DFL_STORED / FIXED / DYNAMIC, the segment's output bytes
  uint32_t cost[3];         // bits of the stored, fixed and dynamic form
  uint32_t hlit, hdist, hclen;
  uint32_t off;             // its first byte in the frame
  uint32_t reserved;
};

// One record of the encode batch's chunk table (device table, one per chunk
// with nbytes > 0; include/mcodec.h): src is relative to the entry point's
// `src` base (0: absolute device addresses).
struct mc_dfl_enc_chunk {
  uint64_t src;        // the chunk's bytes
  uint64_t dst;        // device address of its output slot (the frame)
  uint32_t nbytes;
  uint32_t dst_cap;    // the slot's size; mc_deflate_bound(nbytes, container) always suffices
  uint32_t seg_base;   // index of the chunk's first segment in the batch
  uint32_t container;  // MC_INF_ZLIB / MC_INF_GZIP
  uint32_t level;      // 0: stored blocks; anything else: the one parse
  uint32_t seq_base;   // index of the chunk's first sequence record in the workspace: it takes ceil(nbytes / 4)
};

MC_DFL_HD uint32_t mc_dfl_nsegments(uint32_t n) { return (n + MC_DFL_SEGMENT - 1) / MC_DFL_SEGMENT; }  // n < 2^30
MC_DFL_HD uint32_t mc_dfl_seg_len(uint32_t n, uint32_t k) {
  const uint32_t start = k * MC_DFL_SEGMENT;
  return n - start < MC_DFL_SEGMENT ? n - start : MC_DFL_SEGMENT;
}
MC_DFL_HD uint32_t mc_dfl_header_bytes(uint32_t container) { return container == MC_INF_GZIP ? 10u : 2u; }
MC_DFL_HD uint32_t mc_dfl_trailer_bytes(uint32_t container) { return container == MC_INF_GZIP ? 8u : 4u; }
MC_DFL_HD uint32_t mc_dfl_stored_bytes(uint32_t nk) { return nk + 5u * ((nk + 65534u) / 65535u); }
MC_DFL_HD uint64_t mc_deflate_bound(uint64_t n, uint32_t container) {
  const uint64_t box = mc_dfl_header_bytes(container) + mc_dfl_trailer_bytes(container);
  if (n == 0) return box + 2;
  const uint64_t full = n / MC_DFL_SEGMENT, rest = n % MC_DFL_SEGMENT;
  return box + full * mc_dfl_stored_bytes(MC_DFL_SEGMENT) + (rest ? mc_dfl_stored_bytes((uint32_t)rest) : 0);
}
// sequence records a segment of nk bytes / a chunk of n bytes can need: a sequence covers 4 bytes or more.
// Segment k of a chunk keeps its records from k * MC_DFL_MAX_SEQS of the chunk's on.
MC_DFL_HD uint32_t mc_dfl_seq_records(uint32_t n) { return (n + MC_DFL_MIN_MATCH - 1u) / MC_DFL_MIN_MATCH; }
// may this record be encoded at all?  (the kernels skip a chunk that fails)
MC_DFL_HD bool mc_dfl_enc_chunk_ok(const mc_dfl_enc_chunk &c, uint32_t nsegments_total, uint64_t nsequences_total) {
  if (c.nbytes < 1 || c.nbytes >= MC_DFL_MAX_BYTES || c.container > MC_INF_GZIP || !c.dst) return false;
  if ((uint64_t)c.seq_base + mc_dfl_seq_records(c.nbytes) > nsequences_total) return false;
  return (uint64_t)c.seg_base + mc_dfl_nsegments(c.nbytes) <= nsegments_total;
}

MC_DFL_HD uint32_t mc_dfl_hash(uint32_t w) { return (w * 2654435761u) >> (32u - MC_DFL_HASH_BITS); }
// a table entry (position + 1, 0 = empty) as a candidate for `pos`
MC_DFL_HD bool mc_dfl_entry_ok(uint32_t entry, uint32_t pos) {
  return entry != 0 && entry - 1 < pos && pos - (entry - 1) <= MC_DFL_MAX_DIST;
}
MC_DFL_HD uint32_t mc_dfl_le32(const uint8_t *p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// ---- symbols -------------------------------------------------------------------
// length 3 ... 258 -> its symbol's index (symbol 257 + index)
MC_DFL_HD uint32_t mc_dfl_len_sym(uint32_t len) {
  if (len == 258u) return 28u;
  const uint32_t l = len - 3u;
  if (l < 8u) return l;
  const uint32_t e = (31u - (uint32_t)__builtin_clz(l)) - 2u;
  return 4u * e + 4u + ((l >> e) & 3u);
}
// distance 1 ... 32768 -> its symbol
MC_DFL_HD uint32_t mc_dfl_dist_sym(uint32_t dist) {
  const uint32_t d = dist - 1u;
  if (d < 4u) return d;
  const uint32_t hb = 31u - (uint32_t)__builtin_clz(d);
  return 2u * hb + ((d >> (hb - 1u)) & 1u);
}
// the pairs a match of length L >= 4 is written as, and pair j's length
MC_DFL_HD uint32_t mc_dfl_npairs(uint32_t L) { return L / MC_DFL_MAX_LEN + (L % MC_DFL_MAX_LEN != 0); }
MC_DFL_HD uint32_t mc_dfl_piece(uint32_t L, uint32_t j) {
  const uint32_t q = L / MC_DFL_MAX_LEN, r = L % MC_DFL_MAX_LEN;
  if (r == 0u || r >= 3u) return j < q ? MC_DFL_MAX_LEN : r;
  return j + 1u < q ? MC_DFL_MAX_LEN : j + 1u == q ? 255u + r : 3u;  // r is 1 or 2: L >= 259, q >= 1
}
MC_DFL_HD uint32_t mc_dfl_fixed_len(uint32_t s) { return s < 144u ? 8u : s < 256u ? 9u : s < 280u ? 7u : 8u; }
// slot i of the code-length code's lengths: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
MC_DFL_HD uint32_t mc_dfl_cl_slot(uint32_t i) {
  return i < 12u ? (uint32_t)((0x22caa324e804a30ull >> (5u * i)) & 31u)
                 : (uint32_t)((0x3c2e1346cull >> (5u * (i - 12u))) & 31u);
}
// the segment's bytes for `bits` bits of a compressed block
MC_DFL_HD uint32_t mc_dfl_block_bytes(uint32_t bits, uint32_t final) {
  return final ? (bits + 7u) / 8u : (bits + 3u + 7u) / 8u + 4u;
}

// ---- who runs the code construction ------------------------------------------------
// The host: one lane.  (The device's counterpart is mc_deflate.hip's wave_exec.)
struct mc_dfl_scalar {
  uint32_t lane, nlanes;
  MC_DFL_HD mc_dfl_scalar() : lane(0), nlanes(1) {}
  MC_DFL_HD void sync() {}
  MC_DFL_HD uint32_t sum(uint32_t v) { return v; }
  MC_DFL_HD uint32_t max(uint32_t v) { return v; }
  MC_DFL_HD void add(uint32_t *p, uint32_t v) { *p += v; }
};

// the work area of one segment's codes (LDS on the device)
struct alignas(16) mc_dfl_work {
  uint32_t freq[288];
  uint32_t weight[576];  // leaves in sorted order, then the internal nodes in the order they are made
  uint32_t bl_count[16];
  uint32_t cl_hist[32];
  uint16_t order[288];   // the used symbols by (frequency, symbol)
  uint16_t parent[576];
  uint8_t depth[576];
  uint8_t lens[MC_DFL_LENS];  // literal/length from 0, distance from 288, code-length code from 320
};

// hist[0, n) -> lens[0, n): see the file comment.  n >= 2, maxbits 15 or 7.
template <class X>
MC_DFL_HD void mc_dfl_code_lengths(X &x, mc_dfl_work *W, const uint32_t *hist, uint32_t n, uint32_t maxbits,
                                   uint8_t *lens) {
  uint32_t mine = 0;
  for (uint32_t i = x.lane; i < n; i += x.nlanes) {
    const uint32_t f = hist[i];
    W->freq[i] = f;
    lens[i] = 0;
    mine += f != 0u;
  }
  uint32_t m = x.sum(mine);
  x.sync();
  if (m < 2u) {  // zlib's build_tree: force two codes
    if (x.lane == 0) {
      uint32_t have = m;
      for (uint32_t i = 0; i < n && have < 2u; ++i)
        if (W->freq[i] == 0u) W->freq[i] = 1u, ++have;
    }
    m = 2u;
    x.sync();
  }
  // the used symbols by (frequency, symbol): each finds its own rank
  for (uint32_t i = x.lane; i < n; i += x.nlanes) {
    const uint32_t f = W->freq[i];
    if (f == 0u) continue;
    uint32_t r = 0;
    for (uint32_t j = 0; j < n; ++j) {
      const uint32_t g = W->freq[j];
      r += (g != 0u && (g < f || (g == f && j < i))) ? 1u : 0u;
    }
    W->order[r] = (uint16_t)i;
    W->weight[r] = f;
  }
  x.sync();
  if (x.lane == 0) {
    // two queues: the leaves [li, m) and the internal nodes [ni, nn), both by weight
    uint32_t li = 0, ni = m;
    for (uint32_t nn = m; nn < 2u * m - 1u; ++nn) {
      uint32_t pick[2];
      for (uint32_t k = 0; k < 2u; ++k) {
        if (li < m && (ni >= nn || W->weight[li] <= W->weight[ni])) pick[k] = li++;
        else pick[k] = ni++;
      }
      W->weight[nn] = W->weight[pick[0]] + W->weight[pick[1]];
      W->parent[pick[0]] = (uint16_t)nn;
      W->parent[pick[1]] = (uint16_t)nn;
    }
    // depths from the root down, cut at maxbits (gen_bitlen)
    for (uint32_t b = 0; b < 16u; ++b) W->bl_count[b] = 0;
    int32_t overflow = 0;
    W->depth[2u * m - 2u] = 0;
    for (uint32_t node = 2u * m - 2u; node-- > 0u;) {
      uint32_t bits = (uint32_t)W->depth[W->parent[node]] + 1u;
      if (bits > maxbits) bits = maxbits, ++overflow;
      W->depth[node] = (uint8_t)bits;
      if (node < m) ++W->bl_count[bits];
    }
    while (overflow > 0) {  // (at most one pass per two overflow items: it ends)
      uint32_t bits = maxbits - 1u;
      while (bits > 1u && W->bl_count[bits] == 0u) --bits;  // a shorter leaf exists: the tree is full
      --W->bl_count[bits];         // one leaf moves down the tree
      W->bl_count[bits + 1u] += 2u;  // and an overflow item becomes its brother
      --W->bl_count[maxbits];
      overflow -= 2;
    }
  }
  x.sync();
  // the longest codes to the least frequent symbols
  for (uint32_t i = x.lane; i < m; i += x.nlanes) {
    uint32_t acc = 0, L = 1u;
    for (uint32_t bits = maxbits; bits >= 1u; --bits) {
      acc += W->bl_count[bits];
      if (i < acc) {
        L = bits;
        break;
      }
    }
    lens[W->order[i]] = (uint8_t)L;
  }
  x.sync();
}

// lens[0, n) -> tab[0, n): the canonical code of each symbol, bit-reversed (as
// it is written, first bit lowest) | its length << 16; 0 for an unused symbol
template <class X>
MC_DFL_HD void mc_dfl_codes(X &x, const uint8_t *lens, uint32_t n, uint32_t *tab) {
  for (uint32_t s = x.lane; s < n; s += x.nlanes) {
    const uint32_t l = lens[s];
    uint32_t code = 0;
    if (l) {
      for (uint32_t j = 0; j < n; ++j) {
        const uint32_t lj = lens[j];
        if (lj != 0u && lj < l) code += 1u << (l - lj);
        else if (lj == l && j < s) code += 1u;
      }
      code = __builtin_bitreverse32(code) >> (32u - l);
    }
    tab[s] = code | (l << 16);
  }
  x.sync();
}

struct mc_dfl_planned {
  uint32_t type, bytes, cost[3], hlit, hdist, hclen;
};

// A segment's codes, costs and block type from its histogram (hist[0, 286)
// literal/length, hist[288, 318) distance).  Leaves W->lens filled.
template <class X>
MC_DFL_HD mc_dfl_planned mc_dfl_plan(X &x, mc_dfl_work *W, const uint32_t *hist, uint32_t nk, uint32_t final,
                                     uint32_t level) {
  mc_dfl_code_lengths(x, W, hist, MC_DFL_NLL, 15u, W->lens);
  mc_dfl_code_lengths(x, W, hist + MC_DFL_DOFF, MC_DFL_ND, 15u, W->lens + MC_DFL_DOFF);
  for (uint32_t i = x.lane; i < 32u; i += x.nlanes) {
    W->cl_hist[i] = 0;
    if (i < 2u) W->lens[MC_DFL_NLL + i] = 0, W->lens[MC_DFL_DOFF + MC_DFL_ND + i] = 0;
  }
  x.sync();
  uint32_t last_l = 0, last_d = 0;
  for (uint32_t s = x.lane; s < MC_DFL_NLL; s += x.nlanes)
    if (W->lens[s]) last_l = s;
  for (uint32_t s = x.lane; s < MC_DFL_ND; s += x.nlanes)
    if (W->lens[MC_DFL_DOFF + s]) last_d = s;
  last_l = x.max(last_l), last_d = x.max(last_d);
  mc_dfl_planned P;
  P.hlit = last_l < 256u ? 257u : last_l + 1u;
  P.hdist = last_d + 1u;
  for (uint32_t i = x.lane; i < P.hlit + P.hdist; i += x.nlanes)
    x.add(&W->cl_hist[i < P.hlit ? W->lens[i] : W->lens[MC_DFL_DOFF + (i - P.hlit)]], 1u);
  x.sync();
  mc_dfl_code_lengths(x, W, W->cl_hist, 19u, 7u, W->lens + MC_DFL_HIST);
  P.hclen = 4u;
  for (uint32_t i = 4u; i < 19u; ++i)
    if (W->lens[MC_DFL_HIST + mc_dfl_cl_slot(i)]) P.hclen = i + 1u;
  uint32_t fx = 0, dy = 0, hd = 0;
  for (uint32_t s = x.lane; s < MC_DFL_NLL; s += x.nlanes) {
    const uint32_t h = hist[s], xb = s > 256u ? mc_inf_len_extra(s - 257u) : 0u;
    fx += h * (mc_dfl_fixed_len(s) + xb);
    dy += h * ((uint32_t)W->lens[s] + xb);
  }
  for (uint32_t s = x.lane; s < MC_DFL_ND; s += x.nlanes) {
    const uint32_t h = hist[MC_DFL_DOFF + s], xb = mc_inf_dist_extra(s);
    fx += h * (5u + xb);
    dy += h * ((uint32_t)W->lens[MC_DFL_DOFF + s] + xb);
  }
  for (uint32_t v = x.lane; v < 16u; v += x.nlanes) hd += W->cl_hist[v] * (uint32_t)W->lens[MC_DFL_HIST + v];
  fx = x.sum(fx), dy = x.sum(dy), hd = x.sum(hd);
  P.cost[MC_DFL_STORED] = 8u * mc_dfl_stored_bytes(nk);
  P.cost[MC_DFL_FIXED] = 8u * mc_dfl_block_bytes(3u + fx, final);
  P.cost[MC_DFL_DYNAMIC] = 8u * mc_dfl_block_bytes(3u + 14u + 3u * P.hclen + hd + dy, final);
  P.type = MC_DFL_STORED;
  if (level != 0u && (P.cost[MC_DFL_FIXED] < P.cost[MC_DFL_STORED] || P.cost[MC_DFL_DYNAMIC] < P.cost[MC_DFL_STORED]))
    P.type = P.cost[MC_DFL_FIXED] <= P.cost[MC_DFL_DYNAMIC] ? MC_DFL_FIXED : MC_DFL_DYNAMIC;
  P.bytes = P.cost[P.type] / 8u;
  return P;
}

// the bits of one length/distance pair (at most 48): the length's code and
// extra bits, then the distance's.  lltab / dtab: mc_dfl_codes' tables.
MC_DFL_HD uint32_t mc_dfl_pair_bits(const uint32_t *lltab, const uint32_t *dtab, uint32_t len, uint32_t dist,
                                    uint64_t *val) {
  const uint32_t ls = mc_dfl_len_sym(len), ds = mc_dfl_dist_sym(dist);
  const uint32_t le = lltab[257u + ls], de = dtab[ds];
  uint64_t v = le & 0xffffu;
  uint32_t nb = le >> 16;
  v |= (uint64_t)(len - mc_inf_len_base(ls)) << nb;
  nb += mc_inf_len_extra(ls);
  v |= (uint64_t)(de & 0xffffu) << nb;
  nb += de >> 16;
  v |= (uint64_t)(dist - mc_inf_dist_base(ds)) << nb;
  nb += mc_inf_dist_extra(ds);
  *val = v;
  return nb;
}
// the dynamic block's first 17 bits: BFINAL, BTYPE = 2, HLIT, HDIST, HCLEN
MC_DFL_HD uint32_t mc_dfl_dynamic_head(uint32_t final, uint32_t hlit, uint32_t hdist, uint32_t hclen) {
  return final | (2u << 1) | ((hlit - 257u) << 3) | ((hdist - 1u) << 8) | ((hclen - 4u) << 13);
}

// ---- the scalar model (host) -------------------------------------------------------
// The parse of one segment: the sequences, the closing literals and the histogram.
static inline uint32_t mc_dfl_parse_segment(const uint8_t *src, uint32_t n, mc_dfl_seq *seqs, uint32_t *tail_lit,
                                            uint32_t *hist) {
  uint32_t table[MC_DFL_TABLE];
  for (uint32_t i = 0; i < MC_DFL_TABLE; ++i) table[i] = 0;
  for (uint32_t i = 0; i < MC_DFL_HIST; ++i) hist[i] = 0;
  const uint32_t limit = n >= MC_DFL_MIN_MATCH ? n - (MC_DFL_MIN_MATCH - 1u) : 0u;  // slots own pos < limit
  uint32_t p = 0, anchor = 0, nseq = 0;
  while (p < limit) {
    const uint32_t wend = (limit - p < MC_DFL_WINDOW) ? limit : p + MC_DFL_WINDOW;
    uint32_t m = 0, c = 0;
    bool found = false;
    for (uint32_t pos = p; pos < wend && !found; ++pos) {
      const uint32_t w = mc_dfl_le32(src + pos);
      const uint32_t e = table[mc_dfl_hash(w)];
      if (mc_dfl_entry_ok(e, pos) && mc_dfl_le32(src + (e - 1)) == w) m = pos, c = e - 1, found = true;
    }
    uint32_t consumed = wend;
    if (found) {
      while (m > anchor && c > 0 && src[m - 1] == src[c - 1]) --m, --c;
      uint32_t ml = MC_DFL_MIN_MATCH;
      while (m + ml < n && src[c + ml] == src[m + ml]) ++ml;
      const uint32_t lit = m - anchor, dist = m - c, np = mc_dfl_npairs(ml);
      seqs[nseq].a = lit | ((dist - 1u) << 17), seqs[nseq].b = ml;
      ++nseq;
      for (uint32_t k = 0; k < lit; ++k) ++hist[src[anchor + k]];
      for (uint32_t j = 0; j < np; ++j) ++hist[257u + mc_dfl_len_sym(mc_dfl_piece(ml, j))];
      hist[MC_DFL_DOFF + mc_dfl_dist_sym(dist)] += np;
      if (m + ml < consumed) consumed = m + ml;
      anchor = m + ml;
    }
    for (uint32_t pos = p; pos < consumed; ++pos)  // ascending: the highest position wins an entry
      table[mc_dfl_hash(mc_dfl_le32(src + pos))] = pos + 1;
    p = found ? anchor : p + MC_DFL_WINDOW;
  }
  *tail_lit = n - anchor;
  for (uint32_t k = anchor; k < n; ++k) ++hist[src[k]];
  ++hist[256];
  return nseq;
}

struct mc_dfl_bitw {
  uint8_t *p;
  uint64_t acc;
  uint32_t cnt, pos;
  void put(uint64_t v, uint32_t nb) {  // nb <= 48, cnt < 8
    acc |= v << cnt;
    cnt += nb;
    while (cnt >= 8u) p[pos++] = (uint8_t)acc, acc >>= 8, cnt -= 8u;
  }
  void align() {
    if (cnt) p[pos++] = (uint8_t)acc, acc = 0, cnt = 0;
  }
};

// One planned segment into exactly s.bytes bytes at dst; the bytes written.
static inline uint32_t mc_dfl_emit_segment(const uint8_t *src, uint32_t n, const mc_dfl_seq *seqs,
                                           const mc_dfl_seg &s, const uint8_t *lens, uint32_t final, uint8_t *dst) {
  if (s.type == MC_DFL_STORED) {
    uint32_t off = 0, out = 0;
    while (off < n) {
      const uint32_t bl = n - off < 65535u ? n - off : 65535u;
      dst[out] = (uint8_t)((final && off + bl == n) ? 1 : 0);
      dst[out + 1] = (uint8_t)bl, dst[out + 2] = (uint8_t)(bl >> 8);
      dst[out + 3] = (uint8_t)~bl, dst[out + 4] = (uint8_t)(~bl >> 8);
      for (uint32_t k = 0; k < bl; ++k) dst[out + 5 + k] = src[off + k];
      off += bl, out += 5u + bl;
    }
    return out;
  }
  mc_dfl_scalar x;
  uint32_t lltab[288], dtab[32], cltab[19];
  uint8_t flens[MC_DFL_HIST];
  mc_dfl_bitw bw{dst, 0, 0, 0};
  if (s.type == MC_DFL_FIXED) {
    for (uint32_t i = 0; i < 288u; ++i) flens[i] = (uint8_t)mc_dfl_fixed_len(i);
    for (uint32_t i = 288u; i < MC_DFL_HIST; ++i) flens[i] = 5;
    lens = flens;
    bw.put(final | (1u << 1), 3);
  }
  mc_dfl_codes(x, lens, 288u, lltab);
  mc_dfl_codes(x, lens + MC_DFL_DOFF, 32u, dtab);
  if (s.type == MC_DFL_DYNAMIC) {
    mc_dfl_codes(x, lens + MC_DFL_HIST, 19u, cltab);
    bw.put(mc_dfl_dynamic_head(final, s.hlit, s.hdist, s.hclen), 17);
    for (uint32_t i = 0; i < s.hclen; ++i) bw.put(lens[MC_DFL_HIST + mc_dfl_cl_slot(i)], 3);
    for (uint32_t i = 0; i < s.hlit + s.hdist; ++i) {
      const uint32_t e = cltab[i < s.hlit ? lens[i] : lens[MC_DFL_DOFF + (i - s.hlit)]];
      bw.put(e & 0xffffu, e >> 16);
    }
  }
  uint32_t pos = 0;
  for (uint32_t q = 0; q <= s.nseq; ++q) {  // the closing literals as a last run without a match
    const uint32_t lit = q < s.nseq ? (seqs[q].a & 0x1ffffu) : s.tail_lit;
    const uint32_t ml = q < s.nseq ? seqs[q].b : 0u, dist = q < s.nseq ? (seqs[q].a >> 17) + 1u : 0u;
    for (uint32_t k = 0; k < lit; ++k) {
      const uint32_t e = lltab[src[pos + k]];
      bw.put(e & 0xffffu, e >> 16);
    }
    const uint32_t np = ml ? mc_dfl_npairs(ml) : 0u;
    for (uint32_t j = 0; j < np; ++j) {
      uint64_t v;
      const uint32_t nb = mc_dfl_pair_bits(lltab, dtab, mc_dfl_piece(ml, j), dist, &v);
      bw.put(v, nb);
    }
    pos += lit + ml;
  }
  bw.put(lltab[256] & 0xffffu, lltab[256] >> 16);
  if (!final) bw.put(0, 3);
  bw.align();
  if (!final) bw.put(0xffff0000u, 32);
  return bw.pos;
}

MC_DFL_HD void mc_dfl_put_header(uint8_t *dst, uint32_t container) {
  if (container == MC_INF_GZIP) {
    dst[0] = 0x1f, dst[1] = 0x8b, dst[2] = 8, dst[3] = 0;
    dst[4] = dst[5] = dst[6] = dst[7] = 0;  // MTIME
    dst[8] = 4, dst[9] = 255;               // XFL: fastest; OS: unknown
  } else {
    dst[0] = 0x78, dst[1] = 0x01;
  }
}
// check: the Adler-32 (zlib) or CRC-32 (gzip) of the chunk
MC_DFL_HD void mc_dfl_put_trailer(uint8_t *dst, uint32_t container, uint32_t check, uint32_t n) {
  if (container == MC_INF_GZIP) {
    for (uint32_t k = 0; k < 4u; ++k) dst[k] = (uint8_t)(check >> (8u * k)), dst[4u + k] = (uint8_t)(n >> (8u * k));
  } else {
    for (uint32_t k = 0; k < 4u; ++k) dst[k] = (uint8_t)(check >> (24u - 8u * k));
  }
}

// The scalar encoder (host): the frame of n source bytes into at most cap
// bytes at dst.  Returns the frame's size, or 0 when the chunk is refused
// (n == 0, n >= 2^30, an unknown container, or the frame would exceed cap):
// nothing is written then.  *need (if given) = the frame's size either way.
// segs (if given) receives one record per segment.  Two passes over the
// segments: the first only adds the sizes up.
static inline uint64_t mc_deflate_encode_chunk_report(const uint8_t *src, uint64_t n, uint8_t *dst, uint64_t cap,
                                                      uint32_t container, uint32_t level, mc_dfl_seg *segs,
                                                      uint64_t *need) {
  if (need) *need = 0;
  if (n < 1 || n >= MC_DFL_MAX_BYTES || container > MC_INF_GZIP) return 0;
  static thread_local mc_dfl_seq seqs[MC_DFL_MAX_SEQS];
  static thread_local mc_dfl_work W;
  uint32_t hist[MC_DFL_HIST];
  mc_dfl_scalar x;
  const uint32_t nseg = mc_dfl_nsegments((uint32_t)n), head = mc_dfl_header_bytes(container);
  uint64_t total = head;
  for (int emit = 0; emit < 2; ++emit) {
    uint32_t at = head;
    for (uint32_t k = 0; k < nseg; ++k) {
      const uint32_t nk = mc_dfl_seg_len((uint32_t)n, k), final = k + 1 == nseg;
      const uint8_t *sp = src + (size_t)k * MC_DFL_SEGMENT;
      mc_dfl_seg s;
      s.nseq = mc_dfl_parse_segment(sp, nk, seqs, &s.tail_lit, hist);
      const mc_dfl_planned P = mc_dfl_plan(x, &W, hist, nk, final, level);
      s.type = P.type, s.bytes = P.bytes, s.hlit = P.hlit, s.hdist = P.hdist, s.hclen = P.hclen;
      for (int t = 0; t < 3; ++t) s.cost[t] = P.cost[t];
      s.off = at, s.reserved = 0;
      if (emit) {
        if (mc_dfl_emit_segment(sp, nk, seqs, s, W.lens, final, dst + at) != s.bytes) return 0;  // never
        if (segs) segs[k] = s;
      }
      at += s.bytes;
    }
    if (!emit) {
      total = (uint64_t)at + mc_dfl_trailer_bytes(container);
      if (need) *need = total;
      if (total > cap) return 0;
    } else {
      mc_dfl_put_header(dst, container);
      mc_dfl_put_trailer(dst + at, container,
                         container == MC_INF_GZIP ? mc_inf_crc32(src, (uint32_t)n) : mc_inf_adler32(src, (uint32_t)n),
                         (uint32_t)n);
    }
  }
  return total;
}
static inline uint64_t mc_deflate_encode_chunk(const uint8_t *src, uint64_t n, uint8_t *dst, uint64_t cap,
                                               uint32_t container, uint32_t level) {
  return mc_deflate_encode_chunk_report(src, n, dst, cap, container, level, (mc_dfl_seg *)0, (uint64_t *)0);
}
