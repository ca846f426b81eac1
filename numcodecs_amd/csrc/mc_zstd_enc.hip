// mc_zstd_enc.hip -- Zstandard frames written on the device, a whole batch per
// call.  The format (frame, segments, parse rules, literals forms, modes,
// normalisation, bound) is mc_zstd_enc.h's, compiled for the host too
// (tests/native_zstd_enc): its scalar encoder defines the bytes, the kernels
// reproduce them.  The plan of a block is that header's very code (mc_ze_plan),
// run by the 64 lanes of a wave over LDS.  Four launches:
//
// parse:  one wave (a 64-lane workgroup) per 64 KiB segment of the batch,
//         wave-uniform control flow: mc_deflate.hip's window-of-64 finder with
//         the distance limit lifted to the segment, hash table in LDS.  A
//         sequence is one 8-byte record in the workspace, the literals go in
//         order into the segment's literal buffer there; the histograms of the
//         literal bytes and of the LL / OF / ML codes are counted in LDS; the
//         all-equal flag comes from a pass that stops at the first difference.
// code:   one wave per segment: mc_ze_plan -- Huffman lengths, weights and the
//         tree description, the streams' sizes; lanes 0 ... 2 each normalise,
//         choose the mode of, build the encoding table of and run the state
//         chain of one of LL / OF / ML, leaving the bits between the sequences
//         in the workspace; every size and the block type.
// layout: one workgroup per chunk: the prefix sum of the blocks' sizes, the
//         frame's size against its slot (a frame that does not fit is refused
//         before a byte of it is written), the frame header, and XXH64 of the
//         chunk by the workgroup's first wave (the decoder's check kernel's
//         way: accumulator k in the lanes with lane % 4 == k).
// emit:   one wave per segment: block and section headers; the literals 64
//         symbols a step from the stream's end backwards, a wave prefix sum of
//         the code lengths (the suffix sum of the stream) placing each code;
//         the sequences 64 a step from the last backwards, each lane its
//         sequence's extra bits and recorded state bits (up to 74 bits, in two
//         words).  Bits are OR-ed into an LDS stage of 512 dwords, flushed as
//         whole dwords and clipped to the stream's bytes as the plan placed
//         them.
// Plain vector stores only; no global atomics.
#include "mc_common.h"
#include "mc_lz4_wave.h"
#include "mc_zstd_enc.h"

namespace {

using mc_lz4w::first_false;
using mc_lz4w::ld_le32;
using mc_lz4w::lds_order;
using mc_lz4w::uni;
using mc_lz4w::WAVE;

constexpr uint32_t STAGE = 512;          // dwords of the emit stage
constexpr uint32_t STEP_BITS = 64 * 80;  // the most one step adds

struct enc_args {
  uint64_t base;
  const mc_zstd_enc_chunk *table;
  uint32_t nchunks, nsegs;
  uint64_t nseqs;          // sequence records in all
  mc_ze_seg *segs;         // per segment
  uint32_t *hist;          // per segment, MC_ZE_HIST words
  mc_ze_plan_out *plans;   // per segment
  mc_ze_seq *seqs;         // nseqs records: a chunk's ceil(nbytes / 4) from its seq_base on
  mc_ze_trans *trans;      // nseqs records, as seqs
  uint8_t *lits;           // 4 * nseqs bytes: a chunk's literals from 4 * seq_base on
  uint32_t *mode;          // per chunk: 0 refused, 1 encoded
  uint32_t *cbytes_out;
  int32_t *err;
};

// the chunk whose [seg_base, next seg_base) holds segment s
MC_DEV uint32_t chunk_of_segment(const mc_zstd_enc_chunk *table, uint32_t nchunks, uint32_t s) {
  uint32_t lo = 0, hi = nchunks - 1;
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1) >> 1;
    if (table[mid].seg_base <= s) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// who runs mc_zstd_enc.h's plan here: the wave
struct wave_exec {
  uint32_t lane, nlanes;
  MC_DEV void sync() { lds_order(); }
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

// the segment a wave works on; false: nothing to do
struct seg_view {
  mc_zstd_enc_chunk c;
  uint32_t ci, k, nk, last;
  uint32_t seq_cap;  // the segment's sequence records, from seq_at on
  uint64_t seq_at;
  const uint8_t *src;
};
MC_DEV bool view_segment(const enc_args &a, uint32_t seg, seg_view *v) {
  v->ci = chunk_of_segment(a.table, a.nchunks, seg);
  v->c = a.table[v->ci];
  if (!mc_ze_chunk_ok(v->c, a.nsegs, a.nseqs) || seg < v->c.seg_base) return false;
  v->k = uni(seg - v->c.seg_base);
  const uint32_t nseg = mc_ze_nsegments(v->c.nbytes);
  if (v->k >= nseg) return false;
  v->nk = uni(mc_ze_seg_len(v->c.nbytes, v->k));
  v->last = uni(v->k + 1 == nseg ? 1u : 0u);
  v->seq_cap = uni(mc_ze_seq_records(v->nk));
  v->seq_at = (uint64_t)v->c.seq_base + (uint64_t)v->k * MC_ZE_MAX_SEQS;  // inside the chunk's records: chunk_ok
  v->src = mc_uniform_ptr(reinterpret_cast<const uint8_t *>((uintptr_t)(a.base + v->c.src)) +
                          (size_t)v->k * MC_ZE_SEGMENT);
  return true;
}

__global__ void __launch_bounds__(WAVE) zstd_enc_parse_kernel(enc_args a) {
  __shared__ __attribute__((aligned(16))) uint32_t tbl[MC_ZE_TABLE];
  __shared__ uint32_t hist[MC_ZE_HIST];
  const uint32_t seg = blockIdx.x, lane = threadIdx.x;
  if (seg >= a.nsegs) return;
  seg_view v;
  if (!view_segment(a, seg, &v)) {
    if (lane == 0) a.segs[seg].nseq = 0, a.segs[seg].nlit = 0, a.segs[seg].same = 0, a.segs[seg].nrep = 0;
    return;
  }
  const uint8_t *__restrict__ src = v.src;
  const uint32_t n = v.nk;
  mc_ze_seq *seqs = a.seqs + v.seq_at;
  uint8_t *lits = a.lits + 4ull * v.seq_at;  // n bytes at the most: 4 * seq_cap >= n
  for (uint32_t k = 4 * lane; k < MC_ZE_TABLE; k += 4 * WAVE)
    *reinterpret_cast<mc_u32x4 *>(tbl + k) = mc_u32x4{0u, 0u, 0u, 0u};
  for (uint32_t k = lane; k < MC_ZE_HIST; k += WAVE) hist[k] = 0;
  lds_order();
  const uint32_t limit = n >= MC_ZE_MIN_MATCH ? n - (MC_ZE_MIN_MATCH - 1u) : 0u;  // slots own pos < limit
  uint32_t p = 0, anchor = 0, nseq = 0, nlit = 0, prev = 0, nrep = 0;
  while (p < limit) {
    // the window's 67 bytes staged one per lane (+3 in lanes 0-2); every
    // lane's word is put together from its neighbours' registers
    const uint32_t pos = p + lane;
    const uint32_t b0 = pos < n ? src[pos] : 0u;
    const uint32_t b1 = (lane < 3 && n - p > WAVE + lane) ? src[p + WAVE + lane] : 0u;
    uint32_t w = b0;
#pragma unroll
    for (uint32_t k = 1; k < 4; ++k) {
      const uint32_t idx = lane + k;
      const uint32_t x0 = (uint32_t)__shfl((int)b0, (int)(idx & (WAVE - 1)), WAVE);
      const uint32_t x1 = (uint32_t)__shfl((int)b1, (int)(idx & (WAVE - 1)), WAVE);
      w |= (idx < WAVE ? x0 : x1) << (8 * k);
    }
    const bool active = pos < limit;
    const uint32_t h = mc_dfl_hash(w);
    const uint32_t entry = active ? tbl[h] : 0u;
    const uint32_t cand = entry - 1;
    bool ok = mc_ze_entry_ok(entry, pos);
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
    // bytes are known equal, up to the segment's end.  64 bytes a step
    const uint32_t maxback = m - anchor < c ? m - anchor : c;
    const bool beq = lane < maxback && src[m - 1 - lane] == src[c - 1 - lane];
    const bool feq = 4 + lane < n - m && src[c + 4 + lane] == src[m + 4 + lane];
    uint32_t back = first_false(beq), fwd = 4 + first_false(feq);
    while (back % WAVE == 0 && back) {  // every byte of the last step was equal
      const uint32_t i = back + lane;
      const uint32_t f = first_false(i < maxback && src[m - 1 - i] == src[c - 1 - i]);
      back += f;
      if (f < WAVE) break;
    }
    while ((fwd - 4) % WAVE == 0 && fwd > 4) {
      const uint32_t i = fwd + lane;
      const uint32_t f = first_false(i < n - m && src[c + i] == src[m + i]);
      fwd += f;
      if (f < WAVE) break;
    }
    m -= back, c -= back;
    const uint32_t len = uni(back + fwd);
    m = uni(m), c = uni(c);
    const uint32_t lit = m - anchor, mend = m + len, off = m - c;  // off <= 65535: both inside the segment
    const mc_ze_seq s{lit | (off << 16), len};
    const mc_ze_sym y = mc_ze_symbols(s, prev);
    if (lane == 0 && nseq < v.seq_cap) seqs[nseq] = s;
    ++nseq;  // every sequence covers 4 bytes or more: at most n / 4 of them
    nrep += y.c[1] == 0u;
    prev = off;
    for (uint32_t k = lane; k < lit; k += WAVE) {
      const uint32_t b = src[anchor + k];
      atomicAdd(&hist[b], 1u);
      if (nlit + k < n) lits[nlit + k] = (uint8_t)b;
    }
    nlit += lit;
    if (lane < 3) atomicAdd(&hist[mc_ze_hist_at(lane) + mc_ze_pick(y.c, lane)], 1u);
    // only the positions consumed from this window enter the table
    const uint32_t lim = mend - p < WAVE ? mend : p + WAVE;
    if (active && pos < lim) atomicMax(&tbl[h], pos + 1);
    lds_order();
    p = anchor = mend;
  }
  for (uint32_t k = anchor + lane; k < n; k += WAVE) {
    const uint32_t b = src[k];
    atomicAdd(&hist[b], 1u);
    if (nlit + (k - anchor) < n) lits[nlit + (k - anchor)] = (uint8_t)b;
  }
  nlit += n - anchor;
  // every byte equal to the first?  stops at the first step that differs
  const uint32_t first = src[0];
  uint32_t same = 1;
  for (uint32_t k = 0; k < n; k += WAVE) {
    const bool eq = k + lane >= n || src[k + lane] == first;
    if (first_false(eq) < WAVE) {
      same = 0;
      break;
    }
  }
  lds_order();
  uint32_t *gh = a.hist + (size_t)seg * MC_ZE_HIST;
  for (uint32_t k = lane; k < MC_ZE_HIST; k += WAVE) gh[k] = hist[k];
  if (lane == 0) {
    mc_ze_seg *S = a.segs + seg;
    S->nseq = nseq < v.seq_cap ? nseq : v.seq_cap, S->nlit = nlit < n ? nlit : n, S->same = same, S->nrep = nrep;
  }
}

__global__ void __launch_bounds__(WAVE) zstd_enc_code_kernel(enc_args a) {
  __shared__ mc_ze_work W;
  __shared__ mc_ze_plan_out P;
  __shared__ uint32_t hist[MC_ZE_HIST];
  const uint32_t seg = blockIdx.x, lane = threadIdx.x;
  if (seg >= a.nsegs) return;
  seg_view v;
  if (!view_segment(a, seg, &v)) {
    if (lane == 0) a.segs[seg].type = MC_ZE_RAW, a.segs[seg].bytes = 0;
    return;
  }
  const uint32_t *gh = a.hist + (size_t)seg * MC_ZE_HIST;
  for (uint32_t k = lane; k < MC_ZE_HIST; k += WAVE) hist[k] = gh[k];
  uint32_t *pw = reinterpret_cast<uint32_t *>(&P);
  for (uint32_t k = lane; k < sizeof(mc_ze_plan_out) / 4; k += WAVE) pw[k] = 0;
  lds_order();
  wave_exec x{lane, WAVE};
  mc_ze_seg S = a.segs[seg];
  S.nseq = uni(S.nseq), S.nlit = uni(S.nlit), S.same = uni(S.same);
  if (S.nseq > v.seq_cap) S.nseq = v.seq_cap;
  if (S.nlit > v.nk) S.nlit = v.nk;
  mc_ze_plan(x, &W, hist, a.lits + 4ull * v.seq_at, a.seqs + v.seq_at, v.nk, &S, &P, a.trans + v.seq_at);
  lds_order();
  uint32_t *gp = reinterpret_cast<uint32_t *>(a.plans + seg);
  for (uint32_t k = lane; k < sizeof(mc_ze_plan_out) / 4; k += WAVE) gp[k] = pw[k];
  if (lane == 0) {
    S.off = 0;
    a.segs[seg] = S;
  }
}

// inclusive block-wide scan of v[] (MC_BLOCK entries) under +
MC_DEV void block_scan_add(uint32_t *v, uint32_t t) {
  for (uint32_t d = 1; d < MC_BLOCK; d <<= 1) {
    const uint32_t add = t >= d ? v[t - d] : 0;
    __syncthreads();
    v[t] += add;
    __syncthreads();
  }
}

// XXH64 of data[0, n) by one wave (mc_zstd.hip's check kernel): the low 32 bits
MC_DEV uint32_t wave_xxh64(const uint8_t *data, uint32_t n, uint32_t lane) {
  // stripes of 32 bytes, accumulator k over their k-th 8 bytes; 16 stripes a step
  const uint32_t nstripes = n >> 5;
  uint64_t acc = mc_xxh_seed(lane & 3u);
  auto load = [&](uint32_t stripe0) {
    uint64_t v = 0;
    if (stripe0 + (lane >> 2) < nstripes) __builtin_memcpy(&v, data + 32ull * stripe0 + 8u * lane, 8);
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
  uint64_t q[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)acc, k, WAVE);
    const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(acc >> 32), k, WAVE);
    q[k] = ((uint64_t)hi << 32) | lo;
  }
  return (uint32_t)mc_xxh_finish(q, data, nstripes << 5, n);  // a tail of at most 31 bytes
}

__global__ void __launch_bounds__(MC_BLOCK) zstd_enc_layout_kernel(enc_args a) {
  __shared__ uint32_t sums[MC_BLOCK];
  const uint32_t ci = blockIdx.x, t = threadIdx.x;
  if (ci >= a.nchunks) return;
  const mc_zstd_enc_chunk c = a.table[ci];
  if (!mc_ze_chunk_ok(c, a.nsegs, a.nseqs)) {  // the same for every thread
    if (t == 0) a.mode[ci] = 0, a.cbytes_out[ci] = 0, a.err[2 * ci] = MC_ZE_E_TABLE, a.err[2 * ci + 1] = 0;
    return;
  }
  const uint32_t n = c.nbytes, nseg = mc_ze_nsegments(n), checksum = c.flags & MC_ZE_F_CHECKSUM;
  mc_ze_seg *segs = a.segs + c.seg_base;
  // thread t owns segments [lo, hi)
  const uint32_t per = (nseg + MC_BLOCK - 1) / MC_BLOCK;
  const uint32_t lo = t * per < nseg ? t * per : nseg, hi = lo + per < nseg ? lo + per : nseg;
  uint32_t mine = 0;
  for (uint32_t s = lo; s < hi; ++s) mine += segs[s].bytes;  // <= n + 3 * nseg in all: 32 bits hold every offset
  sums[t] = mine;
  __syncthreads();
  block_scan_add(sums, t);
  const uint32_t head = mc_ze_header_bytes(n);
  const uint32_t data_end = head + sums[MC_BLOCK - 1], frame = data_end + (checksum ? 4u : 0u);
  if (frame > c.dst_cap) {  // the same for every thread: nothing of the chunk is written
    if (t == 0) a.mode[ci] = 0, a.cbytes_out[ci] = 0, a.err[2 * ci] = MC_ZE_E_SPACE, a.err[2 * ci + 1] = (int32_t)frame;
    return;
  }
  uint32_t at = head + sums[t] - mine;
  for (uint32_t s = lo; s < hi; ++s) {
    segs[s].off = at;
    at += segs[s].bytes;
  }
  if (t >= WAVE) return;  // the first wave: the header and the checksum
  uint8_t *dst = reinterpret_cast<uint8_t *>((uintptr_t)c.dst);
  uint32_t check = 0;
  if (checksum) check = wave_xxh64(mc_uniform_ptr(reinterpret_cast<const uint8_t *>((uintptr_t)(a.base + c.src))), n, t);
  if (t == 0) {
    mc_ze_put_header(dst, n, checksum);
    if (checksum)
      for (uint32_t k = 0; k < 4u; ++k) dst[data_end + k] = (uint8_t)(check >> (8u * k));
    a.mode[ci] = 1, a.cbytes_out[ci] = frame;
  }
}

// A byte-aligned bitstream on its way to the frame.  st[i] holds global dword
// base + i counted from g0, the 4-byte aligned address at or below the
// stream's first byte; cur is the bit cursor from g0.  Only bytes in [lo, hi)
// are ever stored.
struct bit_stage {
  uint32_t *st;
  uint8_t *g0, *lo, *hi;
  uint32_t base, cur, lane;
  MC_DEV void open(uint8_t *from, uint8_t *to) {  // the stage is all zeros
    const uint32_t lead = (uint32_t)((uintptr_t)from & 3u);
    g0 = from - lead, lo = from, hi = to, base = 0, cur = 8u * lead;
  }
  MC_DEV void store(uint32_t dword, uint32_t v) {
    uint8_t *q = g0 + 4ull * dword;
    if (q >= lo && q + 4 <= hi) {
      *reinterpret_cast<uint32_t *>(q) = v;
    } else {
#pragma unroll
      for (uint32_t b = 0; b < 4; ++b)
        if (q + b >= lo && q + b < hi) q[b] = (uint8_t)(v >> (8u * b));
    }
  }
  // everything (last) or every complete dword out; the incomplete one moves to st[0]
  MC_DEV void flush(bool last) {
    lds_order();
    const uint32_t fill = cur - 32u * base;  // < 32 * STAGE - 64
    const uint32_t nfull = last ? (fill + 31u) / 32u : fill / 32u;
    for (uint32_t i = lane; i < nfull; i += WAVE) store(base + i, st[i]);
    const uint32_t carry = last ? 0u : st[nfull];
    lds_order();
    for (uint32_t i = lane; i <= nfull && i < STAGE; i += WAVE) st[i] = 0;
    lds_order();
    if (lane == 0) st[0] = carry;
    lds_order();
    base += nfull;
  }
  MC_DEV void or_in(uint32_t off, uint64_t val) {  // 48 bits at the most, at bit `off` from g0
    const uint32_t d = (off >> 5) - base, sh = off & 31u;  // d + 2 < STAGE: put() saw to it
    const uint32_t w0 = (uint32_t)(val << sh);
    const uint64_t rem = sh ? val >> (32u - sh) : val >> 32;
    const uint32_t w1 = sh ? (uint32_t)rem : (uint32_t)(val >> 32), w2 = sh ? (uint32_t)(rem >> 32) : 0u;
    if (w0) atomicOr(&st[d], w0);
    if (w1) atomicOr(&st[d + 1], w1);
    if (w2) atomicOr(&st[d + 2], w2);
  }
  // lane l's nlo <= 48 bits, then its nhi <= 32 bits; the lanes' in lane order
  MC_DEV void put(uint64_t vlo, uint32_t nlo, uint32_t vhi = 0, uint32_t nhi = 0) {
    if (cur - 32u * base + STEP_BITS + 64u > 32u * STAGE) flush(false);
    const uint32_t nb = nlo + nhi;
    uint32_t inc = nb;
#pragma unroll
    for (uint32_t d = 1; d < WAVE; d <<= 1) {
      const uint32_t o = (uint32_t)__shfl_up((int)inc, d, WAVE);
      if (lane >= d) inc += o;
    }
    const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
    const uint32_t off = cur + inc - nb;
    if (nlo) or_in(off, vlo);
    if (nhi) or_in(off + nlo, vhi);
    cur += total;
  }
  MC_DEV void close() {  // the end mark, and everything out
    put(1u, lane == 0 ? 1u : 0u);
    flush(true);
  }
};

// Every offset below was derived by the code and layout kernels from the same
// records, and the frame's exact length was checked against the slot there.
// Every store is clipped to [off, off + bytes) of the slot all the same.
__global__ void __launch_bounds__(WAVE) zstd_enc_emit_kernel(enc_args a) {
  __shared__ uint32_t st[STAGE];
  __shared__ uint32_t tab[256];
  __shared__ uint8_t lens[256];
  const uint32_t seg = blockIdx.x, lane = threadIdx.x;
  if (seg >= a.nsegs) return;
  seg_view v;
  if (!view_segment(a, seg, &v) || a.mode[v.ci] == 0) return;
  const mc_ze_seg S = a.segs[seg];
  const mc_ze_plan_out *P = a.plans + seg;
  const uint32_t type = uni(S.type), bytes = uni(S.bytes), off = uni(S.off), n = v.nk;
  const uint8_t *__restrict__ src = v.src;
  // (a table whose chunks share segments could contradict the layout: such a segment is left alone)
  if (off < mc_ze_header_bytes(v.c.nbytes) || bytes < 4u || bytes > v.c.dst_cap || off > v.c.dst_cap - bytes) return;
  if (type == MC_ZE_RAW && bytes != 3u + n) return;
  uint8_t *dst = mc_uniform_ptr(reinterpret_cast<uint8_t *>((uintptr_t)v.c.dst) + off);
  uint8_t *end = dst + bytes;
  const uint32_t bh = mc_ze_block_header(v.last, type, type == MC_ZE_COMPRESSED ? bytes - 3u : n);
  if (lane < 3) dst[lane] = (uint8_t)(bh >> (8u * lane));
  if (type == MC_ZE_RAW) {
    for (uint32_t k = lane; k < n; k += WAVE) dst[3 + k] = src[k];
    return;
  }
  if (type == MC_ZE_RLE) {
    if (lane == 0) dst[3] = src[0];
    return;
  }
  // bytes [from, from + count) of the block from p[], clipped to the block
  auto copy = [&](uint32_t from, const uint8_t *p, uint32_t count) {
    for (uint32_t k = lane; k < count; k += WAVE)
      if (from + k < bytes) dst[from + k] = p[k];
  };
  auto put_le = [&](uint32_t from, uint64_t val, uint32_t count) {
    if (lane < count && from + lane < bytes) dst[from + lane] = (uint8_t)(val >> (8u * lane));
  };
  const uint8_t *lits = a.lits + 4ull * v.seq_at;
  const uint32_t L = uni(S.nlit) < n ? uni(S.nlit) : n;
  const uint32_t nseq = uni(S.nseq) < v.seq_cap ? uni(S.nseq) : v.seq_cap;
  for (uint32_t i = lane; i < STAGE; i += WAVE) st[i] = 0;
  lds_order();
  bit_stage bw{st, nullptr, nullptr, nullptr, 0u, 0u, lane};
  uint32_t at = 3;
  // ---- the literals section ----
  if (uni(S.lit_form) != MC_ZE_COMPRESSED) {
    const uint32_t hb = mc_ze_lit_header(L);
    put_le(at, mc_ze_plain_header(L), hb);
    copy(at + hb, lits, L);
    at += hb + L;
  } else {
    const uint32_t lh = uni(P->lit_header), ns = uni(S.streams) == 1u ? 1u : 4u, wb = uni(P->wdesc_bytes);
    put_le(at, mc_ze_huf_header(lh, ns, L, uni(P->lit_comp)), lh);
    copy(at + lh, P->wdesc, wb < sizeof(P->wdesc) ? wb : (uint32_t)sizeof(P->wdesc));
    at += lh + wb;
    uint32_t sb[4];
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) sb[k] = uni(P->stream_bytes[k]);
    if (ns == 4u) {
      put_le(at, (uint64_t)(sb[0] & 0xffffu) | ((uint64_t)(sb[1] & 0xffffu) << 16) | ((uint64_t)(sb[2] & 0xffffu) << 32), 6u);
      at += 6u;
    }
    for (uint32_t i = lane; i < 256u; i += WAVE) lens[i] = P->lens[i];
    lds_order();
    wave_exec x{lane, WAVE};
    mc_ze_huf_codes(x, lens, uni(P->maxlen), tab);
    const uint32_t share = ns == 1u ? L : (L + 3u) / 4u;
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
      if (k >= ns) break;
      const uint32_t from = k * share, to = (k + 1u == ns) ? L : from + share;
      if (at > bytes || sb[k] > bytes - at || to > L || from > to) return;  // (never: the plan's own sizes)
      bw.open(dst + at, dst + at + sb[k]);
      for (uint32_t j = 0; j < to - from; j += WAVE) {  // from the stream's end backwards
        const uint32_t i = j + lane;
        const uint32_t e = i < to - from ? tab[lits[to - 1u - i]] : 0u;
        bw.put(e & 0xffffu, e >> 16);
      }
      bw.close();
      at += sb[k];
    }
  }
  // ---- the sequences section ----
  if (nseq == 0u) {
    put_le(at, 0u, 1u);
    return;
  }
  const uint32_t nsb = mc_ze_nseq_bytes(nseq);
  put_le(at, nsb == 1u ? nseq : (128u + (nseq >> 8)) | ((nseq & 255u) << 8), nsb);
  at += nsb;
  put_le(at, (uni(S.mode[0]) << 6) | (uni(S.mode[1]) << 4) | (uni(S.mode[2]) << 2), 1u);
  at += 1u;
#pragma unroll
  for (uint32_t w = 0; w < 3u; ++w) {
    const uint32_t tb = uni(P->tdesc_bytes[w]) < 64u ? uni(P->tdesc_bytes[w]) : 64u;
    copy(at, P->tdesc[w], tb);
    at += tb;
  }
  if (at >= bytes) return;  // (never)
  const mc_ze_seq *seqs = a.seqs + v.seq_at;
  const mc_ze_trans *trans = a.trans + v.seq_at;
  bw.open(dst + at, end);
  for (uint32_t g = 0; g < nseq; g += WAVE) {  // from the last sequence backwards
    uint64_t lo = 0;
    uint32_t nlo = 0, hi = 0, nhi = 0;
    if (g + lane < nseq) {
      const uint32_t q = nseq - 1u - (g + lane);
      const mc_ze_sym y = mc_ze_symbols(seqs[q], q ? seqs[q - 1u].a >> 16 : 0u);
      mc_ze_seq_bits(y, q, trans, P, &lo, &nlo, &hi, &nhi);
    }
    bw.put(lo, nlo, hi, nhi);
  }
  bw.close();
}

constexpr size_t WS_ALIGN = 256;
size_t up(size_t v) { return (v + WS_ALIGN - 1) / WS_ALIGN * WS_ALIGN; }
struct ws_layout {
  size_t segs, hist, plans, mode, seqs, trans, lits, total;
};
ws_layout ws_plan(size_t nchunks, size_t nsegs, size_t nseqs) {
  ws_layout w;
  w.segs = 0;
  w.hist = w.segs + up(nsegs * sizeof(mc_ze_seg));
  w.plans = w.hist + up(nsegs * MC_ZE_HIST * sizeof(uint32_t));
  w.mode = w.plans + up(nsegs * sizeof(mc_ze_plan_out));
  w.seqs = w.mode + up(nchunks * sizeof(uint32_t));
  w.trans = w.seqs + up(nseqs * sizeof(mc_ze_seq));
  w.lits = w.trans + up(nseqs * sizeof(mc_ze_trans));
  w.total = w.lits + nseqs * 4;
  return w;
}

}  // namespace

static_assert(sizeof(mc_zstd_enc_chunk) == 40 && sizeof(mc_ze_seg) == 64 && sizeof(mc_ze_seq) == 8 &&
                  sizeof(mc_ze_trans) == 8 && sizeof(mc_ze_plan_out) % 8 == 0,
              "record layout (include/mcodec.h)");
static_assert(sizeof(mc_ze_work) + sizeof(mc_ze_plan_out) + MC_ZE_HIST * 4 <= 20 * 1024, "eight code workgroups share a CU's LDS");

extern "C" {

size_t mc_zstd_encode_workspace(size_t nchunks, size_t nsegments, size_t nsequences) {
  return ws_plan(nchunks, nsegments, nsequences).total;
}

int mc_zstd_encode_batch(const void *src, const void *chunk_table, size_t nchunks, size_t nsegments, size_t nsequences,
                         void *workspace, size_t workspace_bytes, uint32_t *cbytes_out, int32_t *err, mc_stream_t stream) {
  if (nchunks == 0) return MC_OK;
  if (!chunk_table || !workspace || !cbytes_out || !err) return MC_EINVAL;
  if (nchunks > 0x7fffffffu || nsegments > 0x7fffffffu || nsegments < nchunks) return MC_EINVAL;
  if (((uintptr_t)workspace & 7) || ((uintptr_t)chunk_table & 7) || ((uintptr_t)cbytes_out & 3) || ((uintptr_t)err & 3))
    return MC_EINVAL;
  const ws_layout w = ws_plan(nchunks, nsegments, nsequences);
  if (workspace_bytes < w.total) return MC_ENOSPC;
  hipStream_t st = (hipStream_t)stream;
  int rc = mc_hip_status(hipMemsetAsync(err, 0, nchunks * 2 * sizeof(int32_t), st));
  if (rc != MC_OK) return rc;
  uint8_t *ws = static_cast<uint8_t *>(workspace);
  enc_args a;
  a.base = (uint64_t)(uintptr_t)src;
  a.table = static_cast<const mc_zstd_enc_chunk *>(chunk_table);
  a.nchunks = (uint32_t)nchunks, a.nsegs = (uint32_t)nsegments;
  a.nseqs = nsequences;
  a.segs = reinterpret_cast<mc_ze_seg *>(ws + w.segs);
  a.hist = reinterpret_cast<uint32_t *>(ws + w.hist);
  a.plans = reinterpret_cast<mc_ze_plan_out *>(ws + w.plans);
  a.mode = reinterpret_cast<uint32_t *>(ws + w.mode);
  a.seqs = reinterpret_cast<mc_ze_seq *>(ws + w.seqs);
  a.trans = reinterpret_cast<mc_ze_trans *>(ws + w.trans);
  a.lits = ws + w.lits;
  a.cbytes_out = cbytes_out;
  a.err = err;
  hipLaunchKernelGGL(zstd_enc_parse_kernel, dim3((unsigned)nsegments), dim3(WAVE), 0, st, a);
  rc = mc_last_launch();
  if (rc != MC_OK) return rc;
  hipLaunchKernelGGL(zstd_enc_code_kernel, dim3((unsigned)nsegments), dim3(WAVE), 0, st, a);
  rc = mc_last_launch();
  if (rc != MC_OK) return rc;
  hipLaunchKernelGGL(zstd_enc_layout_kernel, dim3((unsigned)nchunks), dim3(MC_BLOCK), 0, st, a);
  rc = mc_last_launch();
  if (rc != MC_OK) return rc;
  hipLaunchKernelGGL(zstd_enc_emit_kernel, dim3((unsigned)nsegments), dim3(WAVE), 0, st, a);
  return mc_last_launch();
}

}  // extern "C"
