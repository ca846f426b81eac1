// mc_zstd_wave.h -- the wave-wide pieces of the Zstandard decoder (device
// only): the bit window, the table builders, the sink and the XXH64 of the
// output, one 64-lane wave per frame.  Shared by the `zstd` codec's kernels
// (mc_zstd.hip) and the Blosc kernels (mc_blosc_dec_z.hip); the rules they
// serve are mc_zstd.h's, and mc_zstd.hip's file comment describes the schedule.
#pragma once

#include "mc_common.h"
#include "mc_zstd.h"
#include "mc_lz4_wave.h"

namespace mc_zstdw {

using namespace mc_lz4w;

MC_DEV void wg_release_acquire() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// the frame's bits through a window of 64 dwords, one per lane, that moves
// down the frame; the 61 dwords below it are loaded ahead
struct wave_bits {
  const uint8_t *src;
  uint32_t n, lane;
  int32_t base;  // the window holds dwords [base, base + 64)
  uint32_t w, ahead;
  MC_DEV uint32_t load(int32_t first) const {  // dword first + lane; bytes outside [0, n) as zeros
    const int32_t idx = first + (int32_t)lane;  // |first| < 2^28
    if (idx < 0) return 0;
    const uint32_t at = 4u * (uint32_t)idx;
    uint32_t v = 0;
    if (at < n) {
      if (n - at >= 4u) {
        __builtin_memcpy(&v, src + at, 4);
      } else {
        for (uint32_t k = 0; k < n - at; ++k) v |= (uint32_t)src[at + k] << (8u * k);
      }
    }
    return v;
  }
  MC_DEV uint64_t bits64(uint64_t lo) {
    const int32_t d = (int32_t)uni((uint32_t)(lo >> 5));  // lo < 2^33
    const uint32_t s = uni((uint32_t)lo & 31u);
    if (d < base || d + 2 > base + 63) {  // wave-uniform
      if (d < base && d >= base - 61) {
        base -= 61;
        w = ahead;
      } else {
        base = d - 61;
        w = load(base);
      }
      ahead = load(base - 61);
    }
    const uint32_t at = (uint32_t)(d - base);  // 0..61
    const uint32_t x0 = (uint32_t)__builtin_amdgcn_readlane((int)w, (int)at);
    const uint32_t x1 = (uint32_t)__builtin_amdgcn_readlane((int)w, (int)(at + 1u));
    const uint32_t x2 = (uint32_t)__builtin_amdgcn_readlane((int)w, (int)(at + 2u));
    const uint64_t v = ((uint64_t)x1 << 32) | x0;
    return s ? (v >> s) | ((uint64_t)x2 << (64u - s)) : v;
  }
};

MC_DEV uint32_t wave_scan_incl(uint32_t v, uint32_t lane) {
#pragma unroll
  for (uint32_t d = 1; d < WAVE; d <<= 1) {
    const uint32_t t = (uint32_t)__shfl_up((int)v, (int)d, WAVE);
    if (lane >= d) v += t;
  }
  return v;
}

// the tables of a block, by the wave (the same cells as mc_zstd_scalar_builder's)
struct wave_builder {
  uint32_t lane;
  MC_DEV void sync() { lds_order(); }
  MC_DEV void fse_rle(uint32_t *table, uint32_t sym) {
    if (lane == 0) table[0] = MC_ZSTD_FSE_ENTRY(sym, 0, 0);
  }
  // norm[0, nsym) (their magnitudes sum to 1 << log) -> table[0, 1 << log)
  MC_DEV void fse(mc_zstd_tables *T, uint32_t *table, uint32_t nsym, uint32_t log) {
    const uint32_t size = 1u << log, mask = size - 1u, step = mc_zstd_fse_step(log);
    const uint64_t below = (1ull << lane) - 1ull;
    // the symbols "less than 1" from the top down, the running totals of the others
    uint32_t nneg = 0, run = 0;
    for (uint32_t first = 0; first < nsym; first += WAVE) {
      const uint32_t s = first + lane;
      const int32_t c = s < nsym ? (int32_t)T->norm[s] : 0;
      const bool neg = c == -1;
      const uint64_t m = __ballot(neg);
      if (neg) table[(size - 1u - (nneg + (uint32_t)__popcll(m & below))) & mask] = s;
      const uint32_t pc = c > 0 ? (uint32_t)c : 0u;
      const uint32_t incl = wave_scan_incl(pc, lane);
      if (s < nsym) {
        T->cum[s] = (uint16_t)(run + incl - pc);
        T->next[s] = (uint16_t)(neg ? 1u : pc);
      }
      run += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
      nneg += (uint32_t)__popcll(m);
    }
    if (lane == 0) T->cum[nsym] = (uint16_t)run;  // nsym <= 256; run + nneg == size
    lds_order();
    const int32_t high = (int32_t)size - 1 - (int32_t)nneg;
    // step j visits cell (j * step) & mask; the cells above `high` are passed over
    uint32_t ranks = 0;
    for (uint32_t first = 0; first < size; first += WAVE) {
      const uint32_t j = first + lane, cell = (j * step) & mask;
      const bool valid = j < size && (int32_t)cell <= high;
      const uint64_t m = __ballot(valid);
      const uint32_t r = ranks + (uint32_t)__popcll(m & below);  // < run
      if (valid) {
        uint32_t lo = 0, hi = nsym;  // cum[lo] <= r < cum[hi]
        while (hi - lo > 1u) {
          const uint32_t mid = (lo + hi) >> 1;
          if (T->cum[mid] <= r) lo = mid; else hi = mid;
        }
        table[cell] = lo;
      }
      ranks += (uint32_t)__popcll(m);
    }
    lds_order();
    // the cells in order: a symbol's k-th cell is its state number norm + k
    for (uint32_t first = 0; first < size; first += WAVE) {
      const uint32_t u = first + lane;
      const bool active = u < size;
      const uint32_t s = active ? table[u] & 255u : 0xffffffffu;
      uint64_t todo = __ballot(active);
      while (todo) {  // one pass per distinct symbol among the 64 cells
        const uint32_t l = (uint32_t)__ffsll((long long)todo) - 1u;
        const uint32_t sv = (uint32_t)__builtin_amdgcn_readlane((int)s, (int)l);
        const uint64_t m = __ballot(s == sv);
        const uint32_t b = uni(T->next[sv]);
        lds_order();
        if (s == sv) table[u] = mc_zstd_fse_cell(s, b + (uint32_t)__popcll(m & below), log);
        if (lane == l) T->next[sv] = (uint16_t)(b + (uint32_t)__popcll(m));
        lds_order();
        todo &= ~m;
      }
    }
    lds_order();
  }
  // count[w] = weights equal to w (w <= 11), count[12] = larger ones
  MC_DEV void weigh(const uint8_t *weights, uint32_t n, uint32_t *count) {
#pragma unroll
    for (int k = 0; k < 13; ++k) count[k] = 0;
    for (uint32_t first = 0; first < n; first += WAVE) {
      const uint32_t s = first + lane;
      const uint32_t w = s < n ? (uint32_t)weights[s] : 0x100u;  // n <= 255
#pragma unroll
      for (int k = 0; k < 12; ++k) count[k] += (uint32_t)__popcll(__ballot(w == (uint32_t)k));
      count[12] += (uint32_t)__popcll(__ballot(w >= 12u && w < 0x100u));
    }
  }
  // weights[0, nsym) (checked, count[] theirs) -> huf[0, 1 << log)
  MC_DEV void huf(mc_zstd_tables *T, uint32_t nsym, uint32_t log, const uint32_t *count) {
    uint32_t start[13], soff[13];
    start[1] = 0, soff[1] = 0;
#pragma unroll
    for (int k = 1; k < 12; ++k) {
      start[k + 1] = start[k] + (count[k] << (k - 1));
      soff[k + 1] = soff[k] + count[k];
    }
    const uint64_t below = (1ull << lane) - 1ull;
    uint32_t off[12];
#pragma unroll
    for (int k = 1; k < 12; ++k) off[k] = soff[k];
    for (uint32_t first = 0; first < nsym; first += WAVE) {
      const uint32_t s = first + lane;
      const uint32_t w = s < nsym ? (uint32_t)T->weights[s] : 0u;
#pragma unroll
      for (int k = 1; k < 12; ++k) {
        const uint64_t m = __ballot(w == (uint32_t)k);
        if (w == (uint32_t)k) T->hsym[(off[k] + (uint32_t)__popcll(m & below)) & 255u] = (uint8_t)s;
        off[k] += (uint32_t)__popcll(m);
      }
    }
    lds_order();
    const uint32_t size = 1u << log;  // == start[12]
    for (uint32_t i = lane; i < size; i += WAVE) {
      uint32_t w = 1, st = 0, so = 0;
#pragma unroll
      for (int k = 1; k < 12; ++k)
        if (start[k] <= i) w = (uint32_t)k, st = start[k], so = soff[k];
      const uint32_t s = T->hsym[(so + ((i - st) >> (w - 1u))) & 255u];
      T->huf[i] = (uint16_t)(s | ((log + 1u - w) << 8));
    }
    lds_order();
  }
};

// the output: literals and matches copied wave-wide through the history ring
// (STORE), or only counted
template <bool STORE>
struct wave_sink {
  const uint8_t *frame;
  uint32_t n;
  uint8_t *dst;
  uint8_t *lit;   // the frame's 128 KiB of the workspace
  uint8_t *ring;
  uint32_t mask, cap, op, lane;
  MC_DEV void literals(uint32_t kind, uint32_t at, uint32_t len) {  // len <= cap - op: the walker checked
    if constexpr (STORE) {
      for (uint32_t k = 0; k < len; k += WAVE) {
        const uint32_t i = k + lane;
        if (i < len) {
          const uint8_t v = kind == MC_ZSTD_LIT_RAW ? frame[at + i] : kind == MC_ZSTD_LIT_RLE ? (uint8_t)at : lit[at + i];
          ring[(op + i) & mask] = v;
          dst[op + i] = v;
        }
      }
      if (len) lds_order();
    }
    op += len;
  }
  MC_DEV void match(uint32_t len, uint32_t offset) {  // 1 <= offset <= op, len <= cap - op: the walker checked
    if constexpr (STORE) {
      if (offset > mask + 1u) {
        // beyond the ring: the frame's own output, written by this workgroup
        wg_release_acquire();
        for (uint32_t k = 0; k < len; k += WAVE) {
          if (k + WAVE > offset) wg_release_acquire();  // the step reads bytes of this match
          const uint32_t i = k + lane;
          if (i < len) {
            const uint8_t v = dst[op + i - offset];
            ring[(op + i) & mask] = v;
            dst[op + i] = v;
          }
        }
        if (len) lds_order();
      } else if (offset >= WAVE) {
        // 64 bytes a step: a step reads only bytes of earlier steps (offset >= 64)
        for (uint32_t k = 0; k < len; k += WAVE) {
          const uint32_t i = k + lane;
          if (i < len) {
            const uint8_t v = ring[(op + i - offset) & mask];
            ring[(op + i) & mask] = v;
            dst[op + i] = v;
          }
          lds_order();
        }
      } else if (len) {
        // replicating form: only the `offset` bytes before the match are read
        uint32_t ph = lane % offset;
        const uint32_t step = WAVE % offset;
        const uint32_t pat = ring[(op - offset + ph) & mask];
        for (uint32_t k = 0; k < len; k += WAVE) {
          const uint32_t i = k + lane;
          const uint8_t v = (uint8_t)__shfl(pat, (int)ph, WAVE);
          if (i < len) {
            ring[(op + i) & mask] = v;
            dst[op + i] = v;
          }
          ph += step;
          if (ph >= offset) ph -= offset;
        }
        lds_order();
      }
    }
    op += len;
  }
  // the streams of a compressed literals section, one lane each
  MC_DEV int huffman(const mc_zstd_lit_streams &ls, const uint16_t *huf, uint32_t log) {
    if constexpr (STORE) {
      int e = MC_ZSTD_OK;
      if (lane < ls.nstreams) {
        const uint32_t k = lane;
        const uint32_t start = k == 0 ? ls.start[0] : k == 1 ? ls.start[1] : k == 2 ? ls.start[2] : ls.start[3];
        const uint32_t end = k == 0 ? ls.end[0] : k == 1 ? ls.end[1] : k == 2 ? ls.end[2] : ls.end[3];
        const uint32_t at = k == 0 ? ls.out[0] : k == 1 ? ls.out[1] : k == 2 ? ls.out[2] : ls.out[3];
        const uint32_t len = k == 0 ? ls.len[0] : k == 1 ? ls.len[1] : k == 2 ? ls.len[2] : ls.len[3];
        uint8_t *o = lit + at;  // at + len <= Regenerated_Size <= 128 KiB
        uint32_t word = 0;
        auto put = [&](uint32_t i, uint32_t b) {
          word |= b << (8u * (i & 3u));
          if ((i & 3u) == 3u) {
            __builtin_memcpy(o + i - 3u, &word, 4);
            word = 0;
          }
        };
        e = mc_zstd_huf_stream(frame, n, start, end, huf, log, len, put);
        for (uint32_t i = len & ~3u; i < len; ++i) o[i] = (uint8_t)(word >> (8u * (i & 3u)));
      }
      wg_release_acquire();  // the sequences' lanes read what these four wrote
      return __ballot(e != MC_ZSTD_OK) ? MC_ZSTD_E_CORRUPT : MC_ZSTD_OK;
    } else {
      return MC_ZSTD_OK;
    }
  }
};

// the low 32 bits of XXH64 (seed 0) of out[0, np), by the wave: 512 bytes a
// step (the next step's loaded ahead), four lanes carry the four accumulators
MC_DEV uint32_t wave_xxh64(const uint8_t *out, uint32_t np, uint32_t lane) {
  // stripes of 32 bytes, accumulator k over their k-th 8 bytes; 16 stripes a step
  const uint32_t nstripes = np >> 5;
  uint64_t acc = mc_xxh_seed(lane & 3u);
  auto load = [&](uint32_t stripe0) {
    uint64_t v = 0;
    if (stripe0 + (lane >> 2) < nstripes) __builtin_memcpy(&v, out + 32ull * stripe0 + 8u * lane, 8);
    return v;
  };
  uint64_t nxt = load(0);
  for (uint32_t s0 = 0; s0 < nstripes; s0 += 16u) {
    const uint64_t cur = nxt;
    nxt = load(s0 + 16u);
    const uint32_t m = nstripes - s0 < 16u ? nstripes - s0 : 16u;
    for (uint32_t s = 0; s < m; ++s) {
      const int from = (int)(4u * s + (lane & 3u));
      const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)cur, from, WAVE);
      const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(cur >> 32), from, WAVE);
      acc = mc_xxh_round(acc, ((uint64_t)hi << 32) | lo);
    }
  }
  uint64_t a[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)acc, k, WAVE);
    const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(acc >> 32), k, WAVE);
    a[k] = ((uint64_t)hi << 32) | lo;
  }
  return (uint32_t)mc_xxh_finish(a, out, nstripes << 5, np);  // a tail of at most 31 bytes
}

}  // namespace mc_zstdw
