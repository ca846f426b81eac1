// bzip2 encode on gfx950: five launches per batch (format, bound and the scalar
// model whose bytes these kernels reproduce: mc_bz2_enc.h).
//
//   prepare  a wave per block: the block CRC (each lane the CRC of a slice,
//            folded by powers of x), RLE1 64 bytes a step (a ballot of "differs
//            from the left neighbour" with a carried run length, the mirror of
//            the decoder's undo), the in-use map in LDS.
//   sort     a workgroup of 1024 per block, blocks taken from a counter by at
//            most MC_BZ2E_SORT_WGS resident workgroups: a counting pass on the
//            first byte, then doubling rounds.  A round reads the rotations in
//            the order of their second key for free (sa[j] - h, in sa's order)
//            and sorts them by the first key with stable LSD radix passes of 8
//            bits: per tile of 1024 a wave-level multisplit (8 ballots), per-wave
//            digit counts in LDS, a scan across the waves.  New ranks are a
//            running maximum over the flags "differs from the predecessor".
//            The arrays (sa, temp, two rank arrays: 16 bytes a symbol) are a
//            slice per resident workgroup, not per block.
//   code     a wave per block: MTF with the list in registers, four entries a
//            lane: a ballot finds a byte, a lane shift moves the entries before
//            it (a 64-byte step that equals the list's front throughout is one
//            addition to the zero run), RUNA / RUNB, the symbol histogram in
//            LDS, then the table passes with a lane per group of 50, the
//            selectors' move-to-front positions a lane a selector, both exact
//            costs and the choice.
//   layout   a workgroup per chunk: the scan of the blocks' bit lengths, the
//            CRC chain, the capacity check, the frame cleared, the stream
//            header and the trailer.
//   emit     a wave per block: every field goes through one wave-wide bit
//            sink: a prefix sum of the lanes' bit counts, the codes OR-ed into
//            an LDS stage, whole dwords flushed MSB first at the block's bit
//            offset.  The first and the last dword of a block may be shared
//            with its neighbours: those two are OR-ed in atomically, the rest
//            is stored.  (The dwords are the aligned dwords of memory around
//            the frame: bytes of a shared dword outside the frame get zeros
//            OR-ed in, which leaves them as they are.)
//
// Bounds: a block whose chunk record is out of range, or whose symbols would
// not fit the workspace's per-block capacity, is marked (nblock = 0), skipped
// by every stage and reported by layout; RLE1 writes at most floor(5 nk / 4)
// symbols; the sort's indices are below nblock by construction (sa is a
// permutation of [0, nblock), ranks are positions); emit writes inside the
// frame's bit span, which layout checked against the capacity.
#include "mc_common.h"
#include "mc_bz2_enc.h"
#include "mc_lz4_wave.h"

namespace {

using namespace mc_lz4w;

constexpr uint32_t MC_BZ2E_SORT_WGS = 256;  // one workgroup of 1024 a CU
constexpr uint32_t SORT_T = 1024, SORT_W = SORT_T / WAVE;
constexpr size_t WS_ALIGN = 256;

MC_DEV void wg_order() { __syncthreads(); }  // a one-wave workgroup: orders its LDS and global accesses

struct wave_exec {  // who runs mc_dfl_code_lengths: one wave
  uint32_t lane, nlanes;
  MC_DEV void sync() { wg_order(); }
  MC_DEV uint32_t sum(uint32_t v) {
#pragma unroll
    for (int d = 1; d < (int)WAVE; d <<= 1) v += (uint32_t)__shfl_xor((int)v, d, WAVE);
    return uni(v);
  }
  MC_DEV uint32_t max(uint32_t v) {
#pragma unroll
    for (int d = 1; d < (int)WAVE; d <<= 1) {
      const uint32_t o = (uint32_t)__shfl_xor((int)v, d, WAVE);
      v = o > v ? o : v;
    }
    return uni(v);
  }
  MC_DEV void add(uint32_t *p, uint32_t v) { atomicAdd(p, v); }
};

MC_DEV uint32_t wave_xor(uint32_t v) {
#pragma unroll
  for (int k = 1; k < (int)WAVE; k <<= 1) v ^= (uint32_t)__shfl_xor((int)v, k, WAVE);
  return v;
}
MC_DEV uint32_t wave_incl_add(uint32_t v, uint32_t lane) {
#pragma unroll
  for (int d = 1; d < (int)WAVE; d <<= 1) {
    const uint32_t o = (uint32_t)__shfl_up((int)v, d, WAVE);
    if (lane >= (uint32_t)d) v += o;
  }
  return v;
}
MC_DEV uint32_t wave_incl_max(uint32_t v, uint32_t lane) {
#pragma unroll
  for (int d = 1; d < (int)WAVE; d <<= 1) {
    const uint32_t o = (uint32_t)__shfl_up((int)v, d, WAVE);
    if (lane >= (uint32_t)d && o > v) v = o;
  }
  return v;
}
MC_DEV uint64_t lanes_below(uint32_t lane) { return (1ull << lane) - 1ull; }

struct batch {
  const mc_bz2e_chunk *chunks;
  uint32_t nchunks, nblocks, level, cap;
  mc_bz2e_block *blocks;
  uint8_t *arrays;  // nblocks slices of mc_bz2e_block_stride(cap)
};

// the chunk of block b: the last record whose block_base is at or below b
MC_DEV uint32_t chunk_of(const batch &B, uint32_t b) {
  uint32_t lo = 0, hi = B.nchunks;
  while (hi - lo > 1u) {
    const uint32_t mid = (lo + hi) >> 1;
    if (B.chunks[mid].block_base <= b) lo = mid;
    else hi = mid;
  }
  return lo;
}

MC_DEV uint32_t xpow8(uint32_t m) {  // x^(8 m) mod P
  uint32_t r = 1u, base = mc_bz2_mulx(1u, 8u);
  for (; m; m >>= 1) {
    if (m & 1u) r = mc_bz2_gfmul(r, base);
    base = mc_bz2_gfmul(base, base);
  }
  return r;
}

// ---- prepare ------------------------------------------------------------------------
__global__ void __launch_bounds__(WAVE) bz2e_prepare_kernel(batch B) {
  __shared__ uint32_t used[8];
  const uint32_t lane = threadIdx.x, b = blockIdx.x;
  if (b >= B.nblocks) return;
  mc_bz2e_block *rec = B.blocks + b;
  const uint32_t ci = chunk_of(B, b);
  const mc_bz2e_chunk c = B.chunks[ci];
  const uint32_t k = b - c.block_base;
  bool ok = c.nbytes < MC_BZ2E_MAX_BYTES && c.nbytes > 0u && c.src != 0u && b >= c.block_base &&
            k < mc_bz2e_nblocks(c.nbytes, B.level);
  uint32_t nk = 0;
  if (ok) {
    nk = mc_bz2e_seg_len(c.nbytes, B.level, k);
    ok = mc_bz2e_cap(nk) <= B.cap;
  }
  if (lane < 8u) used[lane] = 0;
  wg_order();
  if (!ok) {
    if (lane == 0) rec->nblock = 0, rec->bits = 0, rec->crc = 0, rec->chunk = ci, rec->k = k;
    return;
  }
  const uint8_t *seg = mc_uniform_ptr(reinterpret_cast<const uint8_t *>((uintptr_t)c.src) + (size_t)k * mc_bz2e_seg(B.level));
  uint8_t *rle = mc_bz2e_arrays_at(B.arrays + (size_t)b * mc_bz2e_block_stride(B.cap), B.cap).rle;
  // the CRC: lane l takes bytes [l * sl, (l + 1) * sl)
  const uint32_t sl = (nk + WAVE - 1u) / WAVE;
  const uint32_t lo = lane * sl < nk ? lane * sl : nk, hi = lo + sl < nk ? lo + sl : nk;
  uint32_t crc = lane == 0 ? 0xffffffffu : 0u;
  for (uint32_t i = lo; i < hi; ++i) crc = mc_bz2_crc_byte(crc, seg[i]);
  crc = uni(~wave_xor(mc_bz2_gfmul(crc, xpow8(nk - hi))));
  // RLE1
  uint32_t out = 0, carry = 0;  // carry: the length of the run that reaches the step's start
  for (uint32_t first = 0; first < nk; first += WAVE) {
    const uint32_t cnt = nk - first < WAVE ? nk - first : WAVE, at = first + lane;
    const bool in = lane < cnt;
    const uint32_t v = in ? seg[at] : 0u;
    const uint32_t left = in && at > 0u ? seg[at - 1u] : 256u, right = in && at + 1u < nk ? seg[at + 1u] : 256u;
    const uint64_t starts = __ballot(in && v != left);
    const uint64_t mine = starts & (lanes_below(lane) | (1ull << lane));
    const uint32_t p = mine ? lane - (63u - (uint32_t)__builtin_clzll(mine)) : carry + lane;
    const uint32_t q = p % 255u;
    const bool last = q == 254u || v != right;
    const bool eb = in && q < 4u, ec = in && last && q >= 3u;
    const uint64_t EB = __ballot(eb), EC = __ballot(ec);
    const uint32_t o = out + (uint32_t)__popcll(EB & lanes_below(lane)) + (uint32_t)__popcll(EC & lanes_below(lane));
    if (eb) {
      rle[o] = (uint8_t)v;
      atomicOr(&used[v >> 5], 1u << (v & 31u));
    }
    if (ec) {
      const uint32_t n = q - 3u;
      rle[o + (eb ? 1u : 0u)] = (uint8_t)n;
      atomicOr(&used[n >> 5], 1u << (n & 31u));
    }
    out += (uint32_t)__popcll(EB) + (uint32_t)__popcll(EC);
    carry = starts ? cnt - (63u - (uint32_t)__builtin_clzll(starts)) : carry + cnt;
  }
  wg_order();
  if (lane == 0) {
    uint32_t ninuse = 0;
    for (uint32_t w = 0; w < 8; ++w) rec->used[w] = used[w], ninuse += (uint32_t)__popc(used[w]);
    rec->nblock = out, rec->crc = crc, rec->ninuse = ninuse, rec->chunk = ci, rec->k = k;
    rec->orig = 0, rec->nmtf = 0, rec->ngroups = 0, rec->nsel = 0, rec->bits = 0, rec->bitoff = 0;
  }
}

// ---- sort ---------------------------------------------------------------------------
struct sort_lds {
  uint32_t hist[3][256];         // a round's digit counts, then the running bases
  uint32_t wcount[SORT_W][256];  // a tile's per-wave digit counts (zero between tiles)
  uint32_t woff[SORT_W][256];    // where a wave's items of a digit go
  uint32_t wtot[2][SORT_W];      // the rank scan's per-wave maxima, by tile parity
  uint32_t groups, taken;
};

// exclusive scan of hist[p][0, 256) in place, by the first four waves
MC_DEV void scan256(uint32_t *h, uint32_t *scratch, uint32_t t) {
  uint32_t v = 0, incl = 0;
  if (t < 256u) {
    v = h[t];
    incl = wave_incl_add(v, t & 63u);
    if ((t & 63u) == 63u) scratch[t >> 6] = incl;
  }
  __syncthreads();
  if (t < 256u) {
    uint32_t before = 0;
    for (uint32_t w = 0; w < (t >> 6); ++w) before += scratch[w];
    h[t] = before + incl - v;
  }
  __syncthreads();
}

__global__ void __launch_bounds__(SORT_T) bz2e_sort_kernel(batch B, uint32_t *__restrict__ counter, uint32_t *__restrict__ work) {
  __shared__ sort_lds L;
  const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
  uint32_t *const w0 = work + (size_t)blockIdx.x * 4u * B.cap;
  for (;;) {
    __syncthreads();
    if (t == 0) L.taken = atomicAdd(counter, 1u);
    __syncthreads();
    const uint32_t b = L.taken;
    if (b >= B.nblocks) return;
    mc_bz2e_block *rec = B.blocks + b;
    const uint32_t n = rec->nblock;
    if (n == 0u) continue;
    const mc_bz2e_arrays A = mc_bz2e_arrays_at(B.arrays + (size_t)b * mc_bz2e_block_stride(B.cap), B.cap);
    const uint8_t *blk = A.rle;
    uint32_t *sa = w0, *tmp = w0 + B.cap, *rank = w0 + 2u * (size_t)B.cap, *rank2 = w0 + 3u * (size_t)B.cap;
    // the first pass: by the first byte (the order inside a bucket is free)
    for (uint32_t i = t; i < 3u * 256u; i += SORT_T) (&L.hist[0][0])[i] = 0;
    for (uint32_t i = t; i < SORT_W * 256u; i += SORT_T) (&L.wcount[0][0])[i] = 0;
    __syncthreads();
    for (uint32_t i = t; i < n; i += SORT_T) atomicAdd(&L.hist[0][blk[i]], 1u);
    __syncthreads();
    if (t < 256u) L.hist[1][t] = L.hist[0][t] != 0u;
    __syncthreads();
    if (t == 0) {
      uint32_t g = 0;
      for (uint32_t v = 0; v < 256; ++v) g += L.hist[1][v];
      L.groups = g;
    }
    scan256(L.hist[0], L.wtot[0], t);
    if (t < 256u) L.hist[1][t] = L.hist[0][t];  // the buckets' starts: the ranks
    __syncthreads();
    for (uint32_t i = t; i < n; i += SORT_T) {
      const uint32_t v = blk[i];
      sa[atomicAdd(&L.hist[0][v], 1u)] = i;
      rank[i] = L.hist[1][v];
    }
    __syncthreads();
    const uint32_t passes = n <= 256u ? 1u : n <= 65536u ? 2u : 3u;
    for (uint32_t h = 1; L.groups < n && h < n; h *= 2u) {
      __syncthreads();
      // the digit counts of every pass in one sweep
      for (uint32_t i = t; i < 3u * 256u; i += SORT_T) (&L.hist[0][0])[i] = 0;
      __syncthreads();
      for (uint32_t i = t; i < n; i += SORT_T) {
        const uint32_t r = rank[i];
        for (uint32_t p = 0; p < passes; ++p) atomicAdd(&L.hist[p][(r >> (8u * p)) & 255u], 1u);
      }
      __syncthreads();
      for (uint32_t p = 0; p < passes; ++p) scan256(L.hist[p], L.wtot[0], t);
      for (uint32_t p = 0; p < passes; ++p) {
        const uint32_t *src = (p & 1u) ? tmp : sa;
        uint32_t *dst = (p & 1u) ? sa : tmp;
        const uint32_t shift = 8u * p;
        for (uint32_t first = 0; first < n; first += SORT_T) {
          const uint32_t j = first + t;
          const bool in = j < n;
          uint32_t i = 0, d = 0;
          if (in) {
            i = src[j];
            if (p == 0u) i = i >= h ? i - h : i + n - h;  // ordered by the second key
            d = (rank[i] >> shift) & 255u;
          }
          uint64_t peers = __ballot(in);
#pragma unroll
          for (uint32_t bit = 0; bit < 8u; ++bit) {
            const bool one = (d >> bit) & 1u;
            const uint64_t m = __ballot(in && one);
            peers &= one ? m : ~m;
          }
          const uint32_t before = (uint32_t)__popcll(peers & lanes_below(lane));
          if (in && before == 0u) L.wcount[wave][d] = (uint32_t)__popcll(peers);
          __syncthreads();
          if (t < 256u) {
            uint32_t off = L.hist[p][t];
#pragma unroll
            for (uint32_t w = 0; w < SORT_W; ++w) {
              L.woff[w][t] = off;
              off += L.wcount[w][t];
            }
            L.hist[p][t] = off;
          }
          __syncthreads();
          if (in) {
            dst[L.woff[wave][d] + before] = i;
            if (before == 0u) L.wcount[wave][d] = 0;
          }
        }
        __syncthreads();
      }
      if (passes & 1u) {  // an odd number of passes ends in tmp
        uint32_t *x = sa;
        sa = tmp, tmp = x;
      }
      // the new ranks: the position of the last rotation that differs from its predecessor
      if (t == 0) L.groups = 0;
      __syncthreads();
      uint32_t carry = 0, mygroups = 0, parity = 0;
      for (uint32_t first = 0; first < n; first += SORT_T, parity ^= 1u) {
        const uint32_t j = first + t;
        const bool in = j < n;
        uint32_t i = 0, val = 0;
        if (in) {
          i = sa[j];
          bool flag = j == 0u;
          if (!flag) {
            const uint32_t pi = sa[j - 1u];
            const uint32_t i2 = i + h >= n ? i + h - n : i + h, p2 = pi + h >= n ? pi + h - n : pi + h;
            flag = rank[i] != rank[pi] || rank[i2] != rank[p2];
          }
          val = flag ? j : 0u;
          mygroups += flag;
        }
        const uint32_t incl = wave_incl_max(val, lane);
        if (lane == 63u) L.wtot[parity][wave] = incl;
        __syncthreads();
        uint32_t best = carry, all = carry;
        for (uint32_t w = 0; w < SORT_W; ++w) {
          const uint32_t m = L.wtot[parity][w];
          if (w < wave && m > best) best = m;
          if (m > all) all = m;
        }
        if (in) rank2[i] = incl > best ? incl : best;
        carry = all;
      }
      atomicAdd(&L.groups, mygroups);
      uint32_t *x = rank;
      rank = rank2, rank2 = x;
      __syncthreads();
    }
    __syncthreads();
    for (uint32_t j = t; j < n; j += SORT_T) {
      const uint32_t i = sa[j];
      A.col[j] = blk[i ? i - 1u : n - 1u];
    }
    if (t == 0) rec->orig = rank[0];
  }
}

// ---- code ---------------------------------------------------------------------------
struct code_lds {
  mc_dfl_work W;
  uint64_t len64[MC_BZ2E_LROW];
  uint32_t freq[MC_BZ2E_LROW];
  uint32_t rfreq[6][MC_BZ2E_LROW];
  uint32_t symbits;
  uint8_t lens[6 * MC_BZ2E_LROW];
  uint8_t index[256];
};

// the wave's pending symbols: lane k holds symbol (64 m + k) until 64 are there
struct sym_out {
  uint16_t *sym;
  uint32_t *freq;
  uint32_t nmtf, pend, lane;
  MC_DEV void put(uint32_t s) {
    if (lane == (nmtf & 63u)) pend = s;
    ++nmtf;
    if ((nmtf & 63u) == 0u) flush(WAVE);
  }
  MC_DEV void flush(uint32_t cnt) {  // the last cnt symbols, lanes [0, cnt)
    const uint32_t at = (nmtf - 1u) & ~63u;
    if (lane < cnt) {
      sym[at + lane] = (uint16_t)pend;
      atomicAdd(&freq[pend], 1u);
    }
  }
  MC_DEV void run(uint32_t r) {  // bijective base 2, low digit first
    while (r > 0u) {
      const uint32_t s = (r & 1u) ? 0u : 1u;
      put(s);
      r = (r - 1u - s) >> 1;
    }
  }
};

__global__ void __launch_bounds__(WAVE) bz2e_code_kernel(batch B) {
  __shared__ code_lds L;
  const uint32_t lane = threadIdx.x, b = blockIdx.x;
  if (b >= B.nblocks) return;
  mc_bz2e_block *rec = B.blocks + b;
  const uint32_t n = uni(rec->nblock);
  if (n == 0u) return;
  const mc_bz2e_arrays A = mc_bz2e_arrays_at(B.arrays + (size_t)b * mc_bz2e_block_stride(B.cap), B.cap);
  const uint32_t ninuse = uni(rec->ninuse), alpha = ninuse + 2u;
  uint32_t usedw[8];
  for (uint32_t w = 0; w < 8; ++w) usedw[w] = uni(rec->used[w]);
  // byte value -> list index
  for (uint32_t v = lane; v < 256u; v += WAVE) {
    uint32_t idx = 0;
    for (uint32_t w = 0; w < 8; ++w) {
      const uint32_t word = usedw[w];
      if (w < (v >> 5)) idx += (uint32_t)__popc(word);
      else if (w == (v >> 5)) idx += (uint32_t)__popc(word & ((1u << (v & 31u)) - 1u));
    }
    L.index[v] = (uint8_t)idx;
  }
  for (uint32_t v = lane; v < MC_BZ2E_LROW; v += WAVE) L.freq[v] = 0;
  wg_order();
  // MTF and the zero runs
  sym_out so{A.sym, L.freq, 0u, 0u, lane};
  uint32_t zrun = 0, front = 0;
  uint32_t e[4] = {lane, 64u + lane, 128u + lane, 192u + lane};  // entries at and past ninuse never match
  for (uint32_t first = 0; first < n; first += WAVE) {
    const uint32_t cnt = n - first < WAVE ? n - first : WAVE;
    const bool in = lane < cnt;
    const uint32_t v = in ? L.index[A.col[first + lane]] : 0u;
    if (__ballot(in && v != front) == 0ull) {
      zrun += cnt;
      continue;
    }
    for (uint32_t p = 0; p < cnt; ++p) {
      const uint32_t vp = (uint32_t)__builtin_amdgcn_readlane((int)v, (int)p);
      if (vp == front) {
        ++zrun;
        continue;
      }
      so.run(zrun);
      zrun = 0;
      // where vp is, then everything before it moves up by one: the list is
      // in registers, entry 64 q + lane in e[q]
      uint64_t hit = __ballot(e[0] == vp);
      uint32_t qj = 0;
      if (!hit) {
        hit = __ballot(e[1] == vp), qj = 1;
        if (!hit) {
          hit = __ballot(e[2] == vp), qj = 2;
          if (!hit) hit = __ballot(e[3] == vp), qj = 3;
        }
      }
      const uint32_t jin = (uint32_t)__ffsll((long long)hit) - 1u, j = 64u * qj + jin;
      uint32_t enter = vp;  // what comes into lane 0 of the next part
#pragma unroll
      for (uint32_t q = 0; q < 4u; ++q) {
        if (q <= qj) {
          const uint32_t leave = (uint32_t)__builtin_amdgcn_readlane((int)e[q], 63);
          const uint32_t up = (uint32_t)__shfl_up((int)e[q], 1, WAVE);
          const uint32_t moved = lane == 0 ? enter : up;
          e[q] = (q < qj || lane <= jin) ? moved : e[q];
          enter = leave;
        }
      }
      front = vp;
      so.put(j + 1u);
    }
  }
  so.run(zrun);
  so.put(ninuse + 1u);
  if (so.nmtf & 63u) so.flush(so.nmtf & 63u);
  wg_order();
  const uint32_t nmtf = so.nmtf, ngroups = mc_bz2e_ngroups(nmtf);
  const uint32_t nsel = (nmtf + MC_BZ2E_GROUP - 1u) / MC_BZ2E_GROUP;
  if (lane == 0) mc_bz2e_initial_split(L.freq, alpha, nmtf, ngroups, L.lens);
  wg_order();
  wave_exec x{lane, WAVE};
  for (uint32_t it = 0; it <= MC_BZ2E_ITERS; ++it) {  // the last pass only prices the selectors it has
    const bool price = it == MC_BZ2E_ITERS;
    for (uint32_t v = lane; v < alpha; v += WAVE) L.len64[v] = mc_bz2e_pack_lens(L.lens, ngroups, v);
    for (uint32_t v = lane; v < 6u * MC_BZ2E_LROW; v += WAVE) (&L.rfreq[0][0])[v] = 0;
    if (lane == 0) L.symbits = 0;
    wg_order();
    uint32_t bits = 0;
    for (uint32_t g = lane; g < nsel; g += WAVE) {
      const uint32_t at = g * MC_BZ2E_GROUP, cnt = nmtf - at < MC_BZ2E_GROUP ? nmtf - at : MC_BZ2E_GROUP;
      uint64_t acc = 0;
      for (uint32_t k = 0; k < cnt; ++k) acc += L.len64[A.sym[at + k]];
      if (price) {
        bits += (uint32_t)(acc >> (10u * A.sel[g])) & 1023u;
        continue;
      }
      uint32_t cost;
      const uint32_t bt = mc_bz2e_best(acc, ngroups, &cost);
      A.sel[g] = (uint8_t)bt;
      for (uint32_t k = 0; k < cnt; ++k) atomicAdd(&L.rfreq[bt][A.sym[at + k]], 1u);
    }
    if (price) {
      atomicAdd(&L.symbits, bits);
      wg_order();
      break;
    }
    wg_order();
    for (uint32_t tb = 0; tb < ngroups; ++tb) {
      for (uint32_t v = lane; v < alpha; v += WAVE)
        if (L.rfreq[tb][v] == 0u) L.rfreq[tb][v] = 1u;
      wg_order();
      mc_dfl_code_lengths(x, &L.W, L.rfreq[tb], alpha, MC_BZ2E_MAXLEN, L.lens + tb * MC_BZ2E_LROW);
      wg_order();
    }
  }
  // the selectors' move-to-front positions, a lane a selector: the tables met
  // walking back to the selector's last use stand before it in the list, in
  // the order met; with no earlier use, also the never-used tables below it
  // (mc_bz2e_sel_mtf's positions; the walks add up to at most 6 nsel steps)
  uint32_t selbits = 0;
  for (uint32_t g = lane; g < nsel; g += WAVE) {
    const uint32_t v = A.sel[g];
    uint32_t seen = 0, j = 0;
    bool found = false;
    for (uint32_t k = g; k-- > 0u;) {
      const uint32_t u = A.sel[k];
      if (u == v) {
        found = true;
        break;
      }
      if (!((seen >> u) & 1u)) seen |= 1u << u, ++j;
    }
    if (!found) j += v - (uint32_t)__popc(seen & ((1u << v) - 1u));
    A.selmtf[g] = (uint8_t)j;
    selbits += j + 1u;
  }
  selbits = x.sum(selbits);
  uint32_t fixed = 0, refined = 0;
  if (lane == 0) {
    fixed = mc_bz2e_fixed_bits(usedw);
    refined = fixed + selbits + L.symbits;
    for (uint32_t tb = 0; tb < ngroups; ++tb) refined += mc_bz2e_lens_bits(L.lens + tb * MC_BZ2E_LROW, alpha);
  }
  fixed = uni(fixed), refined = uni(refined);
  wg_order();
  const uint32_t flat = mc_bz2e_flat_len(alpha);
  const uint32_t fallback = fixed + nsel + 2u * (5u + alpha) + flat * nmtf;
  const bool fb = fallback < refined;
  if (fb) {
    for (uint32_t v = lane; v < 2u * MC_BZ2E_LROW; v += WAVE) L.lens[v] = (uint8_t)flat;
    for (uint32_t g = lane; g < nsel; g += WAVE) A.sel[g] = 0, A.selmtf[g] = 0;
    wg_order();
  }
  for (uint32_t v = lane; v < 6u * MC_BZ2E_LROW; v += WAVE) A.lens[v] = L.lens[v];
  if (lane == 0) {
    rec->nmtf = nmtf, rec->nsel = nsel;
    rec->ngroups = fb ? 2u : ngroups, rec->bits = fb ? fallback : refined;
  }
}

// ---- layout -------------------------------------------------------------------------
__global__ void __launch_bounds__(MC_BLOCK) bz2e_layout_kernel(batch B, uint32_t *__restrict__ cbytes, int32_t *__restrict__ err) {
  __shared__ uint32_t wsum[MC_BLOCK / WAVE];
  __shared__ uint32_t chain, bad;
  const uint32_t t = threadIdx.x, lane = t & 63u, ci = blockIdx.x;
  if (ci >= B.nchunks) return;
  const mc_bz2e_chunk c = B.chunks[ci];
  if (t == 0) chain = 0, bad = 0;
  __syncthreads();
  bool table_ok = c.nbytes > 0u && c.nbytes < MC_BZ2E_MAX_BYTES && c.src != 0u && c.dst != 0u;
  const uint32_t nb = table_ok ? mc_bz2e_nblocks(c.nbytes, B.level) : 0u;
  if (table_ok && ((uint64_t)c.block_base + nb > B.nblocks)) table_ok = false;
  uint64_t carry = 32u;  // the stream header
  if (table_ok) {
    for (uint32_t first = 0; first < nb; first += MC_BLOCK) {
      const uint32_t k = first + t;
      mc_bz2e_block *rec = B.blocks + c.block_base + (k < nb ? k : 0u);
      uint32_t bits = 0;
      if (k < nb) {
        bits = rec->bits;
        if (rec->nblock == 0u || rec->chunk != ci || rec->k != k || bits == 0u) atomicOr(&bad, 1u);
        const uint32_t crc = rec->crc, rot = (nb - 1u - k) & 31u;
        atomicXor(&chain, rot ? (crc << rot) | (crc >> (32u - rot)) : crc);
      }
      const uint32_t incl = wave_incl_add(bits, lane);
      if (lane == 63u) wsum[t >> 6] = incl;
      __syncthreads();
      uint64_t before = carry, total = carry;
      for (uint32_t w = 0; w < MC_BLOCK / WAVE; ++w) {
        if (w < (t >> 6)) before += wsum[w];
        total += wsum[w];
      }
      if (k < nb) rec->bitoff = before + incl - bits;
      carry = total;
      __syncthreads();
    }
  }
  __syncthreads();
  if (!table_ok || bad) {
    for (uint32_t k = t; k < nb; k += MC_BLOCK) B.blocks[c.block_base + k].bitoff = ~0ull;
    if (t == 0) cbytes[ci] = 0, err[2 * ci] = MC_BZ2E_E_TABLE, err[2 * ci + 1] = 0;
    return;
  }
  const uint64_t total_bits = carry + 80u;
  const uint64_t size = (total_bits + 7u) >> 3;
  if (size > c.dst_cap) {
    for (uint32_t k = t; k < nb; k += MC_BLOCK) B.blocks[c.block_base + k].bitoff = ~0ull;
    if (t == 0) cbytes[ci] = 0, err[2 * ci] = MC_BZ2E_E_SPACE, err[2 * ci + 1] = (int32_t)size;
    return;
  }
  // clear the frame: bytes up to the first aligned dword, dwords, the last bytes
  uint8_t *dst = reinterpret_cast<uint8_t *>((uintptr_t)c.dst);
  const uint64_t head = (4u - ((uintptr_t)dst & 3u)) & 3u;
  const uint64_t lead = head < size ? head : size, words = (size - lead) >> 2, tail = lead + 4u * words;
  if (t < lead) dst[t] = 0;
  uint32_t *dw = reinterpret_cast<uint32_t *>(dst + lead);
  for (uint64_t i = t; i < words; i += MC_BLOCK) dw[i] = 0;
  if (tail + t < size) dst[tail + t] = 0;
  __syncthreads();
  if (t == 0) {
    dst[0] = 'B', dst[1] = 'Z', dst[2] = 'h', dst[3] = (uint8_t)('0' + B.level);
    const uint32_t fields[3] = {0x177245u, 0x385090u, chain};
    uint64_t pos = carry;
    for (uint32_t f = 0; f < 3; ++f) {
      const uint32_t nbits = f < 2u ? 24u : 32u;
      for (uint32_t k = 0; k < nbits; ++k, ++pos)
        if ((fields[f] >> (nbits - 1u - k)) & 1u) dst[pos >> 3] |= (uint8_t)(0x80u >> (pos & 7u));
    }
    cbytes[ci] = (uint32_t)size;
  }
}

// ---- emit ---------------------------------------------------------------------------
// the wave's bit sink: stage[k] holds bits [32 k, 32 k + 32) of the stream from
// dword `word` of the destination on, MSB first
struct bit_sink {
  uint32_t *stage;  // LDS, 72 words, zero where no bit was put
  uint32_t *dw;     // the destination's aligned dwords
  uint64_t word;    // the dword stage[0] goes to
  uint64_t first;   // the block's first dword: OR-ed, like its last
  uint32_t fill, lane;
  MC_DEV void put(uint32_t v, uint32_t nb) {  // v < 2^nb, nb <= 32, 0: nothing
    const uint32_t incl = wave_incl_add(nb, lane);
    const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    if (nb) {
      const uint32_t off = fill + incl - nb, sh = off & 31u;
      const uint64_t bits = (((uint64_t)v << (64u - nb)) >> sh);
      atomicOr(&stage[off >> 5], (uint32_t)(bits >> 32));
      if ((uint32_t)bits) atomicOr(&stage[(off >> 5) + 1u], (uint32_t)bits);
    }
    fill += total;
    wg_order();
    const uint32_t full = fill >> 5;  // at most 65
    if (full == 0u) return;
    for (uint32_t k = lane; k < full; k += WAVE) {
      const uint32_t val = mc_bz2_bswap(stage[k]);
      if (word + k == first) atomicOr(&dw[word + k], val);
      else dw[word + k] = val;
    }
    const uint32_t rest = stage[full];
    wg_order();
    for (uint32_t k = lane; k <= full; k += WAVE) stage[k] = k == 0u ? rest : 0u;
    wg_order();
    word += full, fill &= 31u;
  }
  MC_DEV void finish() {
    if (fill && lane == 0) atomicOr(&dw[word], mc_bz2_bswap(stage[0]));
  }
};

__global__ void __launch_bounds__(WAVE) bz2e_emit_kernel(batch B) {
  __shared__ uint32_t stage[72];
  __shared__ uint32_t codes[6 * MC_BZ2E_LROW];  // the code | its length << 24
  __shared__ uint8_t lens[6 * MC_BZ2E_LROW];
  const uint32_t lane = threadIdx.x, b = blockIdx.x;
  if (b >= B.nblocks) return;
  const mc_bz2e_block *rec = B.blocks + b;
  const uint32_t n = uni(rec->nblock);
  const uint64_t bitoff = rec->bitoff;
  if (n == 0u || bitoff == ~0ull) return;
  const mc_bz2e_chunk c = B.chunks[uni(rec->chunk)];
  const mc_bz2e_arrays A = mc_bz2e_arrays_at(B.arrays + (size_t)b * mc_bz2e_block_stride(B.cap), B.cap);
  const uint32_t alpha = uni(rec->ninuse) + 2u, ngroups = uni(rec->ngroups), nsel = uni(rec->nsel), nmtf = uni(rec->nmtf);
  uint32_t usedw[8];
  for (uint32_t w = 0; w < 8; ++w) usedw[w] = uni(rec->used[w]);
  for (uint32_t v = lane; v < 6u * MC_BZ2E_LROW; v += WAVE) lens[v] = A.lens[v];
  for (uint32_t v = lane; v < 72u; v += WAVE) stage[v] = 0;
  wg_order();
  for (uint32_t v = lane; v < ngroups * MC_BZ2E_LROW; v += WAVE) {
    const uint32_t tb = v / MC_BZ2E_LROW, s = v % MC_BZ2E_LROW;
    codes[v] = s < alpha ? mc_bz2e_code(lens + tb * MC_BZ2E_LROW, alpha, s) | ((uint32_t)lens[v] << 24) : 0u;
  }
  wg_order();
  const uintptr_t dst = (uintptr_t)c.dst;
  const uint64_t pos = 8u * (uint64_t)(dst & 3u) + bitoff;
  bit_sink w{stage, reinterpret_cast<uint32_t *>(dst & ~(uintptr_t)3), pos >> 5, pos >> 5, (uint32_t)(pos & 31u), lane};
  {  // the fixed fields and the symbol map, a field a lane
    const uint32_t u16 = mc_bz2e_used16(usedw);
    uint32_t v = 0, nb = 0;
    if (lane == 0) v = 0x314159u, nb = 24;
    else if (lane == 1) v = 0x265359u, nb = 24;
    else if (lane == 2) v = rec->crc, nb = 32;
    else if (lane == 3) v = 0, nb = 1;
    else if (lane == 4) v = rec->orig, nb = 24;
    else if (lane == 5) v = u16, nb = 16;
    else if (lane < 22u) {
      if (u16 & (0x8000u >> (lane - 6u))) v = mc_bz2e_map16(usedw, lane - 6u), nb = 16;
    } else if (lane == 22u) v = ngroups, nb = 3;
    else if (lane == 23u) v = nsel, nb = 15;
    w.put(v, nb);
  }
  for (uint32_t first = 0; first < nsel; first += WAVE) {
    const bool in = first + lane < nsel;
    const uint32_t j = in ? A.selmtf[first + lane] : 0u;
    w.put(in ? (1u << (j + 1u)) - 2u : 0u, in ? j + 1u : 0u);
  }
  for (uint32_t tb = 0; tb < ngroups; ++tb) {
    const uint8_t *row = lens + tb * MC_BZ2E_LROW;
    w.put(lane == 0 ? row[0] : 0u, lane == 0 ? 5u : 0u);
    for (uint32_t first = 0; first < alpha; first += WAVE) {
      const uint32_t s = first + lane;
      uint32_t v = 0, nb = 0;
      if (s < alpha) v = mc_bz2e_delta(s ? row[s - 1u] : row[0], row[s], &nb);
      w.put(v, nb);
    }
  }
  for (uint32_t first = 0; first < nmtf; first += WAVE) {
    const uint32_t i = first + lane;
    uint32_t v = 0, nb = 0;
    if (i < nmtf) {
      const uint32_t e = codes[A.sel[i / MC_BZ2E_GROUP] * MC_BZ2E_LROW + A.sym[i]];
      v = e & 0xffffffu, nb = e >> 24;
    }
    w.put(v, nb);
  }
  w.finish();
}

size_t records_bytes(size_t nblocks) { return (nblocks * sizeof(mc_bz2e_block) + WS_ALIGN - 1) / WS_ALIGN * WS_ALIGN; }
size_t sort_wgs(size_t nblocks) { return nblocks < MC_BZ2E_SORT_WGS ? nblocks : MC_BZ2E_SORT_WGS; }

}  // namespace

static_assert(sizeof(mc_bz2e_chunk) == 32 && sizeof(mc_bz2e_block) == 80, "record layout (include/mcodec.h)");
static_assert(sizeof(sort_lds) <= 64 * 1024 && sizeof(code_lds) <= 64 * 1024, "static LDS");

extern "C" {

size_t mc_bz2_encode_bound(size_t nbytes, unsigned level) {
  if (level < 1 || level > 9) return 0;
  return (size_t)mc_bz2_enc_bound(nbytes, level);
}

size_t mc_bz2_encode_workspace(size_t nchunks, size_t nblocks, size_t max_chunk, unsigned level) {
  (void)nchunks;
  if (max_chunk >= MC_BZ2E_MAX_BYTES || level < 1 || level > 9) return 0;
  const uint32_t seg = mc_bz2e_seg(level);
  const uint32_t cap = mc_bz2e_cap(max_chunk < seg ? (uint32_t)max_chunk : seg);
  return WS_ALIGN + records_bytes(nblocks) + nblocks * (size_t)mc_bz2e_block_stride(cap) + sort_wgs(nblocks) * 16u * (size_t)cap;
}

int mc_bz2_encode_batch(const void *chunk_table, size_t nchunks, size_t nblocks, size_t max_chunk, unsigned level,
                        void *workspace, size_t workspace_bytes, uint32_t *cbytes_out, int32_t *err, mc_stream_t stream) {
  if (nchunks == 0) return MC_OK;
  if (!chunk_table || !workspace || !cbytes_out || !err) return MC_EINVAL;
  if (level < 1 || level > 9 || nblocks == 0 || nchunks > nblocks || nblocks > 0x7fffffffu || max_chunk == 0 ||
      max_chunk >= MC_BZ2E_MAX_BYTES)
    return MC_EINVAL;
  if (((uintptr_t)workspace & 7) || ((uintptr_t)chunk_table & 7) || ((uintptr_t)err & 3) || ((uintptr_t)cbytes_out & 3))
    return MC_EINVAL;
  if (workspace_bytes < mc_bz2_encode_workspace(nchunks, nblocks, max_chunk, level)) return MC_ENOSPC;
  hipStream_t st = (hipStream_t)stream;
  int rc = mc_hip_status(hipMemsetAsync(err, 0, nchunks * 2 * sizeof(int32_t), st));
  if (rc != MC_OK) return rc;
  uint8_t *base = static_cast<uint8_t *>(workspace);
  uint32_t *counter = reinterpret_cast<uint32_t *>(base);
  rc = mc_hip_status(hipMemsetAsync(counter, 0, WS_ALIGN, st));
  if (rc != MC_OK) return rc;
  const uint32_t seg = mc_bz2e_seg(level);
  batch B;
  B.chunks = static_cast<const mc_bz2e_chunk *>(chunk_table);
  B.nchunks = (uint32_t)nchunks, B.nblocks = (uint32_t)nblocks, B.level = level;
  B.cap = mc_bz2e_cap(max_chunk < seg ? (uint32_t)max_chunk : seg);
  B.blocks = reinterpret_cast<mc_bz2e_block *>(base + WS_ALIGN);
  B.arrays = base + WS_ALIGN + records_bytes(nblocks);
  uint32_t *sortw = reinterpret_cast<uint32_t *>(B.arrays + nblocks * (size_t)mc_bz2e_block_stride(B.cap));
  hipLaunchKernelGGL(bz2e_prepare_kernel, dim3((unsigned)nblocks), dim3(WAVE), 0, st, B);
  if ((rc = mc_last_launch()) != MC_OK) return rc;
  hipLaunchKernelGGL(bz2e_sort_kernel, dim3((unsigned)sort_wgs(nblocks)), dim3(SORT_T), 0, st, B, counter, sortw);
  if ((rc = mc_last_launch()) != MC_OK) return rc;
  hipLaunchKernelGGL(bz2e_code_kernel, dim3((unsigned)nblocks), dim3(WAVE), 0, st, B);
  if ((rc = mc_last_launch()) != MC_OK) return rc;
  hipLaunchKernelGGL(bz2e_layout_kernel, dim3((unsigned)nchunks), dim3(MC_BLOCK), 0, st, B, cbytes_out, err);
  if ((rc = mc_last_launch()) != MC_OK) return rc;
  hipLaunchKernelGGL(bz2e_emit_kernel, dim3((unsigned)nblocks), dim3(WAVE), 0, st, B);
  return mc_last_launch();
}

}  // extern "C"
