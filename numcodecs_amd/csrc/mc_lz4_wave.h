// mc_lz4_wave.h -- the wave-wide LZ4 block encoder and decoder (device only):
// one 64-lane wave per stream, wave-uniform control flow.  Shared by the Blosc
// kernels (mc_blosc_enc.hip, mc_blosc_dec.hip) and the `lz4` codec's
// (mc_lz4_codec.hip).  The rules are mc_lz4_enc.h's (encode) and mc_lz4.h's
// (parser, validity predicate); the callers' file comments describe the
// schedules.
#pragma once

#include "mc_common.h"
#include "mc_lz4_enc.h"

namespace mc_lz4w {

constexpr uint32_t WAVE = 64;

MC_DEV uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// Orders this wave's LDS writes before its later LDS reads: the LDS executes
// one wave's instructions in issue order, the wait makes them complete, and
// the "memory" clobber keeps the compiler from moving an access across.
// (A workgroup barrier orders them too; its fence also waits for the streamed
// global stores, which nothing here needs.  Measured the same on MI355X.)
MC_DEV void lds_order() { __asm__ volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

MC_DEV uint32_t ld_le32(const uint8_t *p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// first lane whose predicate is false, 64 if none
MC_DEV uint32_t first_false(bool pred) {
  const uint64_t ne = ~__ballot(pred);
  return ne ? (uint32_t)__ffsll((long long)ne) - 1u : WAVE;
}

// length v's extension run at dst, by all lanes
MC_DEV void put_ext(uint8_t *dst, uint32_t v, uint32_t count, uint32_t lane) {
  for (uint32_t k = lane; k < count; k += WAVE) dst[k] = mc_lz4e_ext_byte(v, count, k);
}

// n source bytes -> at most cap bytes at dst; the compressed size or 0 (raw).
// Same bytes as mc_lz4_encode_stream.  Reads src[0, n) and writes dst[0, cap) only.
MC_DEV uint32_t encode_wave(const uint8_t *__restrict__ src, uint32_t n, uint8_t *__restrict__ dst, uint32_t cap,
                            uint32_t *tbl, uint32_t lane, mc_lz4e_marks *marks) {
  if (n < MC_LZ4E_MINLEN || n >= MC_LZ4_MAX_USIZE) return 0;
  for (uint32_t k = 4 * lane; k < MC_LZ4E_TABLE; k += 4 * WAVE)
    *reinterpret_cast<mc_u32x4 *>(tbl + k) = mc_u32x4{0u, 0u, 0u, 0u};
  lds_order();
  const uint32_t mflimit = n - MC_LZ4E_MFLIMIT, matchlimit = n - MC_LZ4E_LASTLITS;
  uint32_t p = 0, anchor = 0, op = 0;
  while (p < mflimit) {
    // the window's 67 bytes staged one per lane (+3 in lanes 0-2); every
    // lane's word is put together from its neighbours' registers
    const uint32_t pos = p + lane;
    const uint32_t b0 = pos < n ? src[pos] : 0u;
    const uint32_t b1 = (lane < 3 && n - p > WAVE + lane) ? src[p + WAVE + lane] : 0u;
    uint32_t w = b0;
#pragma unroll
    for (uint32_t k = 1; k < 4; ++k) {
      const uint32_t idx = lane + k;
      const uint32_t v = (uint32_t)__shfl((int)b0, (int)(idx & (WAVE - 1)), WAVE);
      const uint32_t t = (uint32_t)__shfl((int)b1, (int)(idx & (WAVE - 1)), WAVE);
      w |= (idx < WAVE ? v : t) << (8 * k);
    }
    const bool active = pos < mflimit;
    const uint32_t h = mc_lz4e_hash(w);
    const uint32_t entry = active ? tbl[h] : 0u;
    const uint32_t cand = entry - 1;
    bool ok = mc_lz4e_entry_ok(entry, pos);
    if (ok) ok = ld_le32(src + cand) == w;  // cand + 3 < pos + 3 < n
    const uint64_t hit = __ballot(ok);
    if (hit == 0) {
      if (active) atomicMax(&tbl[h], pos + 1);
      lds_order();
      p += WAVE;
      continue;
    }
    const uint32_t win = uni((uint32_t)__ffsll((long long)hit) - 1u);
    uint32_t m = (uint32_t)__builtin_amdgcn_readlane((int)pos, (int)win);
    uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)cand, (int)win);
    // backwards: at most min(m - anchor, c) bytes; forwards: the slot's 4
    // bytes are known equal, up to n - 5.  64 bytes a step; the first step of
    // both directions is one round of loads (neither depends on the other)
    const uint32_t maxback = m - anchor < c ? m - anchor : c;
    const bool beq = lane < maxback && src[m - 1 - lane] == src[c - 1 - lane];
    const bool feq = 4 + lane < matchlimit - m && src[c + 4 + lane] == src[m + 4 + lane];
    uint32_t back = first_false(beq), fwd = 4 + first_false(feq);
    while (back % WAVE == 0 && back) {  // every byte of the last step was equal
      const uint32_t i = back + lane;
      const uint32_t f = first_false(i < maxback && src[m - 1 - i] == src[c - 1 - i]);
      back += f;
      if (f < WAVE) break;
    }
    while ((fwd - 4) % WAVE == 0 && fwd > 4) {
      const uint32_t i = fwd + lane;
      const uint32_t f = first_false(i < matchlimit - m && src[c + i] == src[m + i]);
      fwd += f;
      if (f < WAVE) break;
    }
    m -= back, c -= back;
    const uint32_t len = uni(back + fwd);
    m = uni(m), c = uni(c);
    const uint32_t lit = m - anchor, mend = m + len;
    if (mc_lz4e_seq_bytes(lit, len) > cap - op) return 0;  // checked before any byte of the sequence
    if (op == 0) marks->first_lit = lit;
    const uint32_t nle = mc_lz4e_ext_count(lit), nme = mc_lz4e_ext_count(len - 4);
    if (lane == 0) dst[op] = mc_lz4e_token(lit, len - 4);
    uint8_t *q = dst + op + 1;
    put_ext(q, lit, nle, lane);
    q += nle;
    for (uint32_t k = lane; k < lit; k += WAVE) q[k] = src[anchor + k];
    q += lit;
    if (lane < 2) q[lane] = (uint8_t)((m - c) >> (8 * lane));
    q += 2;
    put_ext(q, len - 4, nme, lane);
    op += 1 + nle + lit + 2 + nme;
    // only the positions consumed from this window enter the table
    const uint32_t lim = mend - p < WAVE ? mend : p + WAVE;
    if (active && pos < lim) atomicMax(&tbl[h], pos + 1);
    lds_order();
    p = anchor = mend;
  }
  const uint32_t lit = n - anchor;
  if (mc_lz4e_last_bytes(lit) > cap - op) return 0;
  marks->close_at = op, marks->tail_lit = lit;
  const uint32_t nle = mc_lz4e_ext_count(lit);
  if (lane == 0) dst[op] = mc_lz4e_token(lit, 0);
  uint8_t *q = dst + op + 1;
  put_ext(q, lit, nle, lane);
  q += nle;
  for (uint32_t k = lane; k < lit; k += WAVE) q[k] = src[anchor + k];
  op += 1 + nle + lit;
  return op < n ? op : 0;
}

// the source stream through a 64-byte window held one byte per lane; the 64
// bytes after it are loaded ahead, so that a refill seldom waits for memory
struct wave_reader {
  const uint8_t *src;
  uint32_t n, base, lane;
  uint32_t w, ahead;
  MC_DEV uint32_t load(uint32_t at) { return (at + lane < n) ? src[at + lane] : 0u; }  // at <= n < 2^31
  MC_DEV void start() {
    base = 0;
    w = load(0);
    ahead = load(WAVE < n ? WAVE : n);
  }
  MC_DEV uint32_t byte(uint32_t i) {
    if (i - base >= WAVE) {  // wave-uniform: i and base are
      if (i - base < 2 * WAVE) {
        base += WAVE;
        w = ahead;
      } else {
        base = i;
        w = load(i);
      }
      ahead = load(n - base > WAVE ? base + WAVE : n);
    }
    return (uint32_t)__builtin_amdgcn_readlane((int)w, (int)uni(i - base));
  }
};

// One LZ4 block of n source bytes into exactly usize bytes at dst, through the
// LDS history ring (ring_mask + 1 bytes, a power of two >= min(usize, 64 KiB)).
// Returns 0 or an mc_lz4_error; *produced is the number of bytes written.  A
// sequence that fails the predicate is not copied at all.
MC_DEV int decode_wave(const uint8_t *__restrict__ src, uint32_t n, uint8_t *__restrict__ dst, uint32_t usize,
                       uint8_t *ring, uint32_t ring_mask, uint32_t lane, uint32_t *produced) {
  wave_reader rd{src, n, 0u, lane, 0u, 0u};
  rd.start();
  uint32_t ip = 0, op = 0;
  int e = MC_LZ4_OK;
  while (ip < n) {
    mc_lz4_seq s;
    e = mc_lz4_parse(rd, n, ip, &s);
    if (e == MC_LZ4_OK) e = mc_lz4_check(s, op, usize);
    e = (int)uni((uint32_t)e);
    if (e != MC_LZ4_OK) break;  // nothing of the sequence is copied
    const uint32_t lit_pos = uni(s.lit_pos), lit_len = uni(s.lit_len);
    const uint32_t offset = uni(s.offset), match_len = uni(s.match_len);
    // literals: source -> ring + global; a short run that the window still
    // holds comes out of its registers (no memory latency on the chain)
    if (lit_len && lit_pos >= rd.base && lit_pos - rd.base + lit_len <= WAVE) {
      const uint8_t v = (uint8_t)__shfl(rd.w, (int)((lit_pos - rd.base + lane) & (WAVE - 1)), WAVE);
      if (lane < lit_len) {
        ring[(op + lane) & ring_mask] = v;
        dst[op + lane] = v;
      }
    } else {
      for (uint32_t k = 0; k < lit_len; k += WAVE) {
        const uint32_t i = k + lane;
        if (i < lit_len) {
          const uint8_t v = src[lit_pos + i];
          ring[(op + i) & ring_mask] = v;
          dst[op + i] = v;
        }
      }
    }
    op += lit_len;
    if (lit_len) lds_order();
    // match: ring -> ring + global
    if (offset >= WAVE) {
      // 64 bytes a step: a step reads only bytes of earlier steps (offset >= 64)
      for (uint32_t k = 0; k < match_len; k += WAVE) {
        const uint32_t i = k + lane;
        if (i < match_len) {
          const uint8_t v = ring[(op + i - offset) & ring_mask];
          ring[(op + i) & ring_mask] = v;
          dst[op + i] = v;
        }
        lds_order();
      }
    } else if (match_len) {
      // replicating form: only the `offset` bytes before the match are read
      // (lane p < offset keeps byte p of them; a long match may wrap the ring
      // over them, so they are read once, before anything is written)
      uint32_t ph = lane % offset;  // (k + lane) % offset
      const uint32_t step = WAVE % offset;
      const uint32_t pat = ring[(op - offset + ph) & ring_mask];
      for (uint32_t k = 0; k < match_len; k += WAVE) {
        const uint32_t i = k + lane;
        const uint8_t v = (uint8_t)__shfl(pat, (int)ph, WAVE);
        if (i < match_len) {
          ring[(op + i) & ring_mask] = v;
          dst[op + i] = v;
        }
        ph += step;
        if (ph >= offset) ph -= offset;
      }
      lds_order();
    }
    op += match_len;
    ip = uni(s.next);
  }
  if (e == MC_LZ4_OK && op != usize) e = MC_LZ4_E_SIZE;
  *produced = op;
  return e;
}

// the LDS history ring for streams of at most max_stream bytes
// first error of a frame wins; plain vector atomics / stores
MC_DEV void record_error(int32_t *err, uint32_t frame, int code, uint32_t stream) {
  if (atomicCAS(reinterpret_cast<int *>(&err[2 * frame]), 0, code) == 0) err[2 * frame + 1] = (int32_t)stream;
}

// One stream of a Blosc batch's descriptor list by its wave: a stored stream
// is a wave-wide copy, another one LZ4 block through decode_wave.  fmt 0:
// every valid stream; else only the streams whose descriptor carries that
// format (a launch of mc_blosc_decode_batch_z).  The decode kernel of both
// Blosc entry points.
MC_DEV void blosc_lz4_stream(const uint8_t *__restrict__ frames, const mc_lz4_stream *__restrict__ streams,
                             uint32_t nstreams, uint32_t fmt, uint8_t *ring, uint32_t ring_mask,
                             int32_t *__restrict__ err) {
  const uint32_t sidx = blockIdx.x, lane = threadIdx.x;
  if (sidx >= nstreams) return;
  const mc_lz4_stream d = streams[sidx];
  if (!(d.flags & MC_LZ4_S_VALID) || (fmt && (d.flags >> MC_LZ4_S_FORMAT_SHIFT) != fmt)) return;
  const uint8_t *src = frames + d.src_off;
  uint8_t *dst = reinterpret_cast<uint8_t *>((uintptr_t)d.dst);
  const uint32_t n = uni(d.cbytes), usize = uni(d.usize);
  if (d.flags & MC_LZ4_S_RAW) {  // cbytes == usize (plan)
    for (uint32_t k = lane; k < usize; k += WAVE) dst[k] = src[k];
    return;
  }
  uint32_t produced;
  const int e = decode_wave(src, n, dst, usize, ring, ring_mask, lane, &produced);
  if (e != MC_LZ4_OK && lane == 0) record_error(err, d.frame, e, sidx);
}

inline uint32_t ring_bytes(size_t max_stream) {
  uint32_t r = 256;
  while (r < max_stream && r < 65536u) r <<= 1;
  return r;
}

}  // namespace mc_lz4w
