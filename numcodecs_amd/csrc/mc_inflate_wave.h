// mc_inflate_wave.h -- the wave-wide pieces of the inflater (device only): the
// source window, the table builder and the sink, one 64-lane wave per frame.
// Shared by the zlib / gzip kernels (mc_inflate.hip) and the Blosc kernels
// (mc_blosc_dec_z.hip); the rules they serve are mc_inflate.h's, and
// mc_inflate.hip's file comment describes the schedule.
#pragma once

#include "mc_common.h"
#include "mc_inflate.h"
#include "mc_lz4_wave.h"

namespace mc_infw {

using namespace mc_lz4w;

// the frame as little-endian dwords through a window of 64, one per lane; the
// 64 after it are loaded ahead, so that a refill seldom waits for memory
struct wave_dwords {
  const uint8_t *src;
  uint32_t n, lane;
  uint32_t base, w, ahead;
  MC_DEV uint32_t load(uint32_t first) const {  // dword first + lane, bytes at and past n as zeros
    const uint32_t at = 4u * (first + lane);    // first <= n / 4 + 130: no overflow
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
  MC_DEV void start(uint32_t first) {
    base = first;
    w = load(base);
    ahead = load(base + WAVE);
  }
  MC_DEV uint32_t dword(uint32_t i) {
    if (i - base >= WAVE) {  // wave-uniform: i and base are
      if (i - base < 2 * WAVE) {
        base += WAVE;
        w = ahead;
      } else {  // a stored block was skipped (or the reader stepped back a dword)
        base = i;  // i <= n / 4 + 2: the walker checks for truncation after every symbol
        w = load(base);
      }
      ahead = load(base + WAVE);
    }
    return (uint32_t)__builtin_amdgcn_readlane((int)w, (int)uni(i - base));
  }
};

// the tables of a block, by the wave
struct wave_builder {
  uint32_t lane;
  MC_DEV void sync() { lds_order(); }
  MC_DEV void set_lens(uint8_t *lens, uint32_t at, uint32_t rep, uint32_t val) {
    for (uint32_t k = lane; k < rep; k += WAVE) lens[at + k] = (uint8_t)val;
  }
  MC_DEV void fixed_lens(uint8_t *lens) {
    for (uint32_t s = lane; s < 320u; s += WAVE)
      lens[s] = (uint8_t)(s < 144u ? 8 : s < 256u ? 9 : s < 280u ? 7 : s < 288u ? 8 : 5);
  }
  // n <= 288 lengths -> count[] / sym[] (canonical order: by length, then by
  // symbol) and the primary lookup; 1 = refused.  Every sym[] index is below
  // the number of symbols counted, which is at most n.
  MC_DEV int build(const uint8_t *lens, uint32_t n, int kind, uint16_t *count, uint16_t *sym, uint16_t *pri,
                   uint32_t pbits, uint32_t *incomplete) {
    uint32_t cnt[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) cnt[k] = 0;
    for (uint32_t first = 0; first < n; first += WAVE) {
      const uint32_t s = first + lane;
      const uint32_t l = s < n ? (uint32_t)(lens[s] & 15u) : 0u;
#pragma unroll
      for (int k = 1; k < 16; ++k) cnt[k] += (uint32_t)__popcll(__ballot(l == (uint32_t)k));
    }
    if (mc_inf_check_counts(cnt, kind, incomplete)) return 1;
    uint32_t offs[16];
    offs[0] = offs[1] = 0;
#pragma unroll
    for (int k = 1; k < 15; ++k) offs[k + 1] = offs[k] + cnt[k];
    if (lane == 0) {
      count[0] = 0;
#pragma unroll
      for (int k = 1; k < 16; ++k) count[k] = (uint16_t)cnt[k];
    }
    const uint64_t below = (1ull << lane) - 1ull;
    for (uint32_t first = 0; first < n; first += WAVE) {
      const uint32_t s = first + lane;
      const uint32_t l = s < n ? (uint32_t)(lens[s] & 15u) : 0u;
#pragma unroll
      for (int k = 1; k < 16; ++k) {
        const uint64_t m = __ballot(l == (uint32_t)k);
        if (l == (uint32_t)k) sym[offs[k] + (uint32_t)__popcll(m & below)] = (uint16_t)s;
        offs[k] += (uint32_t)__popcll(m);
      }
    }
    lds_order();
    if (pri) mc_inf_fill_primary(pri, pbits, count, sym, *incomplete, lane, WAVE);
    return 0;
  }
};

// the output: literals gathered one per lane, matches and stored bytes copied
// wave-wide, all through the history ring (STORE), or only counted
template <bool STORE>
struct wave_sink {
  const uint8_t *frame;
  uint8_t *dst;
  uint8_t *ring;
  uint32_t mask, cap, op, lane;
  uint32_t npend, lit;
  MC_DEV bool literal(uint32_t b) {
    if (op + npend >= cap) return false;
    if constexpr (STORE) {
      if (lane == npend) lit = b;
      if (++npend == WAVE) flush();
    } else {
      ++op;
    }
    return true;
  }
  MC_DEV void flush() {
    if constexpr (STORE) {
      if (npend == 0) return;
      if (lane < npend) {  // op + npend <= cap
        ring[(op + lane) & mask] = (uint8_t)lit;
        dst[op + lane] = (uint8_t)lit;
      }
      lds_order();
      op += npend;
      npend = 0;
    }
  }
  MC_DEV int match(uint32_t len, uint32_t dist) {
    flush();
    if (dist > op) return MC_INF_E_FAR;  // dist <= op <= the ring's bytes
    if (len > cap - op) return MC_INF_E_CAPACITY;
    if constexpr (STORE) {
      if (dist >= WAVE) {
        // 64 bytes a step: a step reads only bytes of earlier steps (dist >= 64)
        for (uint32_t k = 0; k < len; k += WAVE) {
          const uint32_t i = k + lane;
          if (i < len) {
            const uint8_t v = ring[(op + i - dist) & mask];
            ring[(op + i) & mask] = v;
            dst[op + i] = v;
          }
          lds_order();
        }
      } else {
        // replicating form: only the `dist` bytes before the match are read
        uint32_t ph = lane % dist;  // (k + lane) % dist; dist >= 1: symbol bases start at 1
        const uint32_t step = WAVE % dist;
        const uint32_t pat = ring[(op - dist + ph) & mask];
        for (uint32_t k = 0; k < len; k += WAVE) {
          const uint32_t i = k + lane;
          const uint8_t v = (uint8_t)__shfl(pat, (int)ph, WAVE);
          if (i < len) {
            ring[(op + i) & mask] = v;
            dst[op + i] = v;
          }
          ph += step;
          if (ph >= dist) ph -= dist;
        }
        lds_order();
      }
    }
    op += len;
    return MC_INF_OK;
  }
  MC_DEV int stored(uint32_t pos, uint32_t len) {  // pos + len <= the frame's length: the walker checked
    flush();
    if (len > cap - op) return MC_INF_E_CAPACITY;
    if constexpr (STORE) {
      for (uint32_t k = 0; k < len; k += WAVE) {
        const uint32_t i = k + lane;
        if (i < len) {
          const uint8_t v = frame[pos + i];
          ring[(op + i) & mask] = v;
          dst[op + i] = v;
        }
      }
      lds_order();
    }
    op += len;
    return MC_INF_OK;
  }
};

}  // namespace mc_infw
