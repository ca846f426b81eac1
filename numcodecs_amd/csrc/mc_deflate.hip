// mc_deflate.hip -- zlib and gzip frames written on the device, a whole batch
// per call.  The format (segments, parse rules, pair split, costs, code
// lengths, containers, bound) is mc_deflate.h's, compiled for the host too
// (tests/native_deflate): its scalar encoder defines the bytes, the kernels
// reproduce them.  The code construction is that header's very code, run by
// the 64 lanes of a wave over LDS.  Four launches:
//
// parse:  one wave (a 64-lane workgroup) per 64 KiB segment of the batch,
//         wave-uniform control flow: mc_lz4_wave.h's window-of-64 finder
//         restated with DEFLATE's limits (the LZ4 kernels stay as they are),
//         hash table in LDS.  A sequence is one 8-byte record in the
//         workspace (at most n_k / 4 of them: 2 bytes per input byte); the
//         literal/length and distance histograms are counted in LDS on the
//         way.
// code:   one wave per segment: code lengths, the three costs, the block type,
//         the code-length code and the segment's byte count.
// layout: one workgroup per chunk: the prefix sum of the segments' sizes, the
//         frame's size against its slot (a frame that does not fit is refused
//         before a byte of it is written), the container header, the Adler-32
//         or CRC-32 of the chunk (a slice per thread, combined by Adler's
//         closed form / by powers of x, as the inflate check kernel does) and
//         the trailer.
// emit:   one wave per segment: the canonical codes rebuilt in LDS from the
//         lengths; then 64 symbols a step (the literals of a run, then its
//         length/distance pairs): each lane's code and extra bits (at most 48),
//         a wave prefix sum of the bit counts, the bits OR-ed into an LDS
//         stage of 512 dwords, which is flushed to the frame as whole dwords
//         (the segment's first and last dword, shared with its neighbours,
//         byte by byte).  Every store is clipped to the segment's bytes as the
//         layout placed them.  A stored segment is a straight copy.
// Plain vector stores only; no global atomics.
#include "mc_common.h"
#include "mc_checksum.h"
#include "mc_deflate.h"
#include "mc_lz4_wave.h"

namespace {

using mc_lz4w::first_false;
using mc_lz4w::ld_le32;
using mc_lz4w::lds_order;
using mc_lz4w::uni;
using mc_lz4w::WAVE;

constexpr uint32_t STAGE = 512;        // dwords of the emit stage
constexpr uint32_t STEP_BITS = 64 * 48;  // the most one step adds

struct enc_args {
  uint64_t base;
  const mc_dfl_enc_chunk *table;
  uint32_t nchunks, nsegs;
  uint64_t nseqs;      // sequence records in all
  mc_dfl_seg *segs;    // per segment
  uint32_t *hist;      // per segment, MC_DFL_HIST words
  uint8_t *lens;       // per segment, MC_DFL_LENS bytes
  mc_dfl_seq *seqs;    // nseqs records: a chunk's ceil(nbytes / 4) from its seq_base on
  uint32_t *mode;      // per chunk: 0 refused, 1 encoded
  uint32_t *cbytes_out;
  int32_t *err;
};

// the chunk whose [seg_base, next seg_base) holds segment s
MC_DEV uint32_t chunk_of_segment(const mc_dfl_enc_chunk *table, uint32_t nchunks, uint32_t s) {
  uint32_t lo = 0, hi = nchunks - 1;
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1) >> 1;
    if (table[mid].seg_base <= s) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// who runs mc_deflate.h's code construction here: the wave
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
  mc_dfl_enc_chunk c;
  uint32_t ci, k, nk, final;
  uint32_t seq_cap;  // the segment's sequence records, from seq_at on
  uint64_t seq_at;
  const uint8_t *src;
};
MC_DEV bool view_segment(const enc_args &a, uint32_t seg, seg_view *v) {
  v->ci = chunk_of_segment(a.table, a.nchunks, seg);
  v->c = a.table[v->ci];
  if (!mc_dfl_enc_chunk_ok(v->c, a.nsegs, a.nseqs) || seg < v->c.seg_base) return false;
  v->k = uni(seg - v->c.seg_base);
  const uint32_t nseg = mc_dfl_nsegments(v->c.nbytes);
  if (v->k >= nseg) return false;
  v->nk = uni(mc_dfl_seg_len(v->c.nbytes, v->k));
  v->final = uni(v->k + 1 == nseg ? 1u : 0u);
  v->seq_cap = uni(mc_dfl_seq_records(v->nk));
  v->seq_at = (uint64_t)v->c.seq_base + (uint64_t)v->k * MC_DFL_MAX_SEQS;  // inside the chunk's records: chunk_ok
  v->src = mc_uniform_ptr(reinterpret_cast<const uint8_t *>((uintptr_t)(a.base + v->c.src)) +
                          (size_t)v->k * MC_DFL_SEGMENT);
  return true;
}

__global__ void __launch_bounds__(WAVE) dfl_parse_kernel(enc_args a) {
  __shared__ __attribute__((aligned(16))) uint32_t tbl[MC_DFL_TABLE];
  __shared__ uint32_t hist[MC_DFL_HIST];
  const uint32_t seg = blockIdx.x, lane = threadIdx.x;
  if (seg >= a.nsegs) return;
  seg_view v;
  if (!view_segment(a, seg, &v)) {
    if (lane == 0) a.segs[seg].nseq = 0, a.segs[seg].tail_lit = 0;
    return;
  }
  const uint8_t *__restrict__ src = v.src;
  const uint32_t n = v.nk;
  mc_dfl_seq *seqs = a.seqs + v.seq_at;
  for (uint32_t k = 4 * lane; k < MC_DFL_TABLE; k += 4 * WAVE)
    *reinterpret_cast<mc_u32x4 *>(tbl + k) = mc_u32x4{0u, 0u, 0u, 0u};
  for (uint32_t k = lane; k < MC_DFL_HIST; k += WAVE) hist[k] = 0;
  lds_order();
  const uint32_t limit = n >= MC_DFL_MIN_MATCH ? n - (MC_DFL_MIN_MATCH - 1u) : 0u;  // slots own pos < limit
  uint32_t p = 0, anchor = 0, nseq = 0;
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
    bool ok = mc_dfl_entry_ok(entry, pos);
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
    const uint32_t lit = m - anchor, mend = m + len, dist = m - c;  // dist <= 32768: extension keeps it
    if (lane == 0 && nseq < v.seq_cap) seqs[nseq] = mc_dfl_seq{lit | ((dist - 1u) << 17), len};
    ++nseq;  // every sequence covers 4 bytes or more: at most n / 4 of them
    for (uint32_t k = lane; k < lit; k += WAVE) atomicAdd(&hist[src[anchor + k]], 1u);
    const uint32_t np = mc_dfl_npairs(len);
    for (uint32_t j = lane; j < np; j += WAVE) atomicAdd(&hist[257u + mc_dfl_len_sym(mc_dfl_piece(len, j))], 1u);
    if (lane == 0) atomicAdd(&hist[MC_DFL_DOFF + mc_dfl_dist_sym(dist)], np);
    // only the positions consumed from this window enter the table
    const uint32_t lim = mend - p < WAVE ? mend : p + WAVE;
    if (active && pos < lim) atomicMax(&tbl[h], pos + 1);
    lds_order();
    p = anchor = mend;
  }
  for (uint32_t k = anchor + lane; k < n; k += WAVE) atomicAdd(&hist[src[k]], 1u);
  if (lane == 0) atomicAdd(&hist[256], 1u);
  lds_order();
  uint32_t *gh = a.hist + (size_t)seg * MC_DFL_HIST;
  for (uint32_t k = lane; k < MC_DFL_HIST; k += WAVE) gh[k] = hist[k];
  if (lane == 0) a.segs[seg].nseq = nseq < v.seq_cap ? nseq : v.seq_cap, a.segs[seg].tail_lit = n - anchor;
}

__global__ void __launch_bounds__(WAVE) dfl_code_kernel(enc_args a) {
  __shared__ mc_dfl_work W;
  __shared__ uint32_t hist[MC_DFL_HIST];
  const uint32_t seg = blockIdx.x, lane = threadIdx.x;
  if (seg >= a.nsegs) return;
  seg_view v;
  if (!view_segment(a, seg, &v)) {
    if (lane == 0) a.segs[seg].type = MC_DFL_STORED, a.segs[seg].bytes = 0;
    return;
  }
  const uint32_t *gh = a.hist + (size_t)seg * MC_DFL_HIST;
  for (uint32_t k = lane; k < MC_DFL_HIST; k += WAVE) hist[k] = gh[k];
  lds_order();
  wave_exec x{lane, WAVE};
  const mc_dfl_planned P = mc_dfl_plan(x, &W, hist, v.nk, v.final, uni(v.c.level));
  uint8_t *gl = a.lens + (size_t)seg * MC_DFL_LENS;
  for (uint32_t k = lane; k < MC_DFL_LENS; k += WAVE) gl[k] = W.lens[k];
  if (lane == 0) {
    mc_dfl_seg *s = a.segs + seg;
    s->type = P.type, s->bytes = P.bytes;
    s->cost[0] = P.cost[0], s->cost[1] = P.cost[1], s->cost[2] = P.cost[2];
    s->hlit = P.hlit, s->hdist = P.hdist, s->hclen = P.hclen;
    s->reserved = 0;
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

// Adler-32 (zlib) or CRC-32 (gzip) of data[0, n) by the workgroup, the
// inflate check kernel's way: a slice per thread, then thread 0 combines.
// The result is valid in thread 0.
MC_DEV uint32_t wg_check32(uint32_t container, const uint8_t *__restrict__ data, uint32_t n, uint32_t *tab,
                           uint32_t (*part)[MC_BLOCK]) {
  const uint32_t t = threadIdx.x;
  const uint32_t per = ((n + MC_BLOCK - 1) / MC_BLOCK + 3u) & ~3u;
  const uint32_t lo = (uint64_t)t * per < n ? t * per : n, hi = n - lo < per ? n : lo + per;
  if (container == MC_INF_GZIP) {
    uint32_t r = t;
#pragma unroll
    for (int k = 0; k < 8; ++k) r = (r >> 1) ^ ((r & 1u) ? mcck::POLY_CRC32 : 0u);
    tab[t] = r;
  }
  __syncthreads();
  if (container == MC_INF_ZLIB) {
    // a = 1 + sum d_j, b = n + sum (n - j) d_j; the slice gives sum (hi - j) d_j and sum d_j
    uint64_t s1 = 0;
    uint32_t s0 = 0;
    for (uint32_t j = lo; j < hi; j += 4) {
      uint32_t w = 0;
      if (hi - j >= 4u) __builtin_memcpy(&w, data + j, 4);
      else for (uint32_t k = 0; k < hi - j; ++k) w |= (uint32_t)data[j + k] << (8u * k);
#pragma unroll
      for (uint32_t k = 0; k < 4; ++k) {
        const uint32_t b = (w >> (8u * k)) & 0xffu;
        s0 += b;
        s1 += (uint64_t)b * (hi - j - k);  // a byte past hi is zero: its (wrapped) weight does not count
      }
    }
    const uint32_t s = s0 % mcck::ADLER_P;
    part[0][t] = s;
    part[1][t] = (uint32_t)((s1 % mcck::ADLER_P + (uint64_t)((n - hi) % mcck::ADLER_P) * s) % mcck::ADLER_P);
  } else {
    uint32_t c = 0;  // raw(0, slice)
    for (uint32_t j = lo; j < hi; j += 4) {
      uint32_t w = 0;
      const uint32_t m = hi - j >= 4u ? 4u : hi - j;
      if (m == 4u) __builtin_memcpy(&w, data + j, 4);
      else for (uint32_t k = 0; k < m; ++k) w |= (uint32_t)data[j + k] << (8u * k);
      for (uint32_t k = 0; k < m; ++k) c = tab[(c ^ (w >> (8u * k))) & 0xffu] ^ (c >> 8);
    }
    // moved to the end of the data: times x^(8 * bytes behind the slice)
    part[0][t] = hi > lo ? mcck::gf_mul(c, mcck::xpow_tab(mcck::kCrc32.x2n, 8ull * (n - hi), mcck::POLY_CRC32),
                                        mcck::POLY_CRC32)
                         : 0u;
  }
  __syncthreads();
  uint32_t check = 0;
  if (t == 0) {
    if (container == MC_INF_ZLIB) {
      uint64_t s = 1, b = n % mcck::ADLER_P;
      for (uint32_t k = 0; k < MC_BLOCK; ++k) s += part[0][k], b += part[1][k];
      check = (uint32_t)((b % mcck::ADLER_P) << 16) | (uint32_t)(s % mcck::ADLER_P);
    } else {
      uint32_t r = 0;
      for (uint32_t k = 0; k < MC_BLOCK; ++k) r ^= part[0][k];
      // crc(D) = ~(0xffffffff * x^(8n) ^ raw(0, D))
      check = ~(mcck::gf_mul(0xffffffffu, mcck::xpow_tab(mcck::kCrc32.x2n, 8ull * n, mcck::POLY_CRC32),
                             mcck::POLY_CRC32) ^ r);
    }
  }
  return check;
}

__global__ void __launch_bounds__(MC_BLOCK) dfl_layout_kernel(enc_args a) {
  __shared__ uint32_t sums[MC_BLOCK];
  __shared__ uint32_t tab[256];
  __shared__ uint32_t part[2][MC_BLOCK];
  const uint32_t ci = blockIdx.x, t = threadIdx.x;
  if (ci >= a.nchunks) return;
  const mc_dfl_enc_chunk c = a.table[ci];
  if (!mc_dfl_enc_chunk_ok(c, a.nsegs, a.nseqs)) {  // the same for every thread
    if (t == 0) a.mode[ci] = 0, a.cbytes_out[ci] = 0, a.err[2 * ci] = MC_DFL_E_TABLE, a.err[2 * ci + 1] = 0;
    return;
  }
  const uint32_t n = c.nbytes, nseg = mc_dfl_nsegments(n);
  mc_dfl_seg *segs = a.segs + c.seg_base;
  // thread t owns segments [lo, hi)
  const uint32_t per = (nseg + MC_BLOCK - 1) / MC_BLOCK;
  const uint32_t lo = t * per < nseg ? t * per : nseg, hi = lo + per < nseg ? lo + per : nseg;
  uint32_t mine = 0;
  for (uint32_t s = lo; s < hi; ++s) mine += segs[s].bytes;  // <= n + 10 * nseg in all: 32 bits hold every offset
  sums[t] = mine;
  __syncthreads();
  block_scan_add(sums, t);
  const uint32_t head = mc_dfl_header_bytes(c.container), trail = mc_dfl_trailer_bytes(c.container);
  const uint32_t data_end = head + sums[MC_BLOCK - 1], frame = data_end + trail;
  if (frame > c.dst_cap) {  // the same for every thread: nothing of the chunk is written
    if (t == 0) a.mode[ci] = 0, a.cbytes_out[ci] = 0, a.err[2 * ci] = MC_DFL_E_SPACE, a.err[2 * ci + 1] = (int32_t)frame;
    return;
  }
  uint32_t at = head + sums[t] - mine;
  for (uint32_t s = lo; s < hi; ++s) {
    segs[s].off = at;
    at += segs[s].bytes;
  }
  const uint8_t *src = reinterpret_cast<const uint8_t *>((uintptr_t)(a.base + c.src));
  const uint32_t check = wg_check32(c.container, src, n, tab, part);
  if (t == 0) {
    uint8_t *dst = reinterpret_cast<uint8_t *>((uintptr_t)c.dst);
    mc_dfl_put_header(dst, c.container);
    mc_dfl_put_trailer(dst + data_end, c.container, check, n);
    a.mode[ci] = 1, a.cbytes_out[ci] = frame;
  }
}

// The segment's bits on their way to the frame.  st[i] holds global dword
// base + i counted from g0, the 4-byte aligned address at or below the
// segment's first byte; cur is the bit cursor from g0.  Only bytes in [lo, hi)
// are ever stored.
struct bit_stage {
  uint32_t *st;
  uint8_t *g0, *lo, *hi;
  uint32_t base, cur, lane;
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
  MC_DEV void room(uint32_t bits) {
    if (cur - 32u * base + bits + 64u > 32u * STAGE) flush(false);
  }
  // lane l's nb <= 48 bits, the lanes' in lane order
  MC_DEV void put(uint64_t val, uint32_t nb) {
    room(STEP_BITS);
    uint32_t inc = nb;
#pragma unroll
    for (uint32_t d = 1; d < WAVE; d <<= 1) {
      const uint32_t o = (uint32_t)__shfl_up((int)inc, d, WAVE);
      if (lane >= d) inc += o;
    }
    const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
    if (nb) {
      const uint32_t off = cur + inc - nb;
      const uint32_t d = (off >> 5) - base, sh = off & 31u;  // d + 2 < STAGE: room() saw to it
      const uint32_t w0 = (uint32_t)(val << sh);
      const uint64_t rem = val >> (32u - sh);
      const uint32_t w1 = (uint32_t)rem, w2 = (uint32_t)(rem >> 32);
      if (w0) atomicOr(&st[d], w0);
      if (w1) atomicOr(&st[d + 1], w1);
      if (w2) atomicOr(&st[d + 2], w2);
    }
    cur += total;
  }
  MC_DEV void skip(uint32_t bits) {  // zero bits
    room(bits);
    cur += bits;
  }
};

// Every offset below was derived by the code and layout kernels from the same
// records, and the frame's exact length was checked against the slot there:
// all writes land in [off, off + bytes) of the slot.
__global__ void __launch_bounds__(WAVE) dfl_emit_kernel(enc_args a) {
  __shared__ uint32_t st[STAGE];
  __shared__ uint32_t lltab[288], dtab[32], cltab[32];
  __shared__ uint8_t lens[MC_DFL_LENS];
  const uint32_t seg = blockIdx.x, lane = threadIdx.x;
  if (seg >= a.nsegs) return;
  seg_view v;
  if (!view_segment(a, seg, &v) || a.mode[v.ci] == 0) return;
  const mc_dfl_seg s = a.segs[seg];
  const uint32_t type = uni(s.type), bytes = uni(s.bytes), off = uni(s.off), n = v.nk, final = v.final;
  const uint8_t *__restrict__ src = v.src;
  // (a table whose chunks share segments could contradict the layout: such a segment is left alone)
  if (off < mc_dfl_header_bytes(v.c.container) || bytes > v.c.dst_cap || off > v.c.dst_cap - bytes) return;
  if (type == MC_DFL_STORED && bytes != mc_dfl_stored_bytes(n)) return;
  uint8_t *dst = mc_uniform_ptr(reinterpret_cast<uint8_t *>((uintptr_t)v.c.dst) + off);
  if (type == MC_DFL_STORED) {
    uint32_t from = 0, out = 0;
    while (from < n) {
      const uint32_t bl = n - from < 65535u ? n - from : 65535u;
      if (lane < 5) {
        const uint32_t nl = ~bl;
        const uint32_t hb = lane == 0 ? ((final && from + bl == n) ? 1u : 0u)
                          : lane == 1 ? bl : lane == 2 ? bl >> 8 : lane == 3 ? nl : nl >> 8;
        dst[out + lane] = (uint8_t)hb;
      }
      for (uint32_t k = lane; k < bl; k += WAVE) dst[out + 5 + k] = src[from + k];
      from += bl, out += 5u + bl;
    }
    return;
  }
  // ---- the codes ----
  wave_exec x{lane, WAVE};
  if (type == MC_DFL_FIXED) {
    for (uint32_t i = lane; i < MC_DFL_LENS; i += WAVE)
      lens[i] = (uint8_t)(i < 288u ? mc_dfl_fixed_len(i) : i < MC_DFL_HIST ? 5u : 0u);
  } else {
    const uint8_t *gl = a.lens + (size_t)seg * MC_DFL_LENS;
    for (uint32_t i = lane; i < MC_DFL_LENS; i += WAVE) lens[i] = gl[i];
  }
  for (uint32_t i = lane; i < STAGE; i += WAVE) st[i] = 0;
  lds_order();
  mc_dfl_codes(x, lens, 288u, lltab);
  mc_dfl_codes(x, lens + MC_DFL_DOFF, 32u, dtab);
  mc_dfl_codes(x, lens + MC_DFL_HIST, 19u, cltab);
  const uint32_t lead = (uint32_t)((uintptr_t)dst & 3u);
  bit_stage bw{st, dst - lead, dst, dst + bytes, 0u, 8u * lead, lane};
  // ---- the block header ----
  if (type == MC_DFL_FIXED) {
    bw.put(final | (1u << 1), lane == 0 ? 3u : 0u);
  } else {
    const uint32_t hlit = uni(s.hlit), hdist = uni(s.hdist), hclen = uni(s.hclen);
    bw.put(mc_dfl_dynamic_head(final, hlit, hdist, hclen), lane == 0 ? 17u : 0u);
    bw.put(lane < hclen ? lens[MC_DFL_HIST + mc_dfl_cl_slot(lane)] : 0u, lane < hclen ? 3u : 0u);  // hclen <= 19
    for (uint32_t k = 0; k < hlit + hdist; k += WAVE) {
      const uint32_t i = k + lane;
      uint32_t e = 0;
      if (i < hlit + hdist) e = cltab[(i < hlit ? lens[i] : lens[MC_DFL_DOFF + (i - hlit)]) & 15u];
      bw.put(e & 0xffffu, e >> 16);
    }
  }
  // ---- the symbols: 64 sequences' records at a time, one per lane ----
  const mc_dfl_seq *seqs = a.seqs + v.seq_at;
  const uint32_t nseq = uni(s.nseq < v.seq_cap ? s.nseq : v.seq_cap), tail = uni(s.tail_lit);
  uint32_t pos = 0;
  for (uint32_t g = 0; g <= nseq; g += WAVE) {  // the closing literals as a last run without a match
    const uint32_t q = g + lane;
    mc_dfl_seq r{q == nseq ? tail : 0u, 0u};
    if (q < nseq) r = seqs[q];
    const uint32_t cnt = nseq + 1u - g < WAVE ? nseq + 1u - g : WAVE;
    for (uint32_t j = 0; j < cnt; ++j) {
      const uint32_t ra = (uint32_t)__builtin_amdgcn_readlane((int)r.a, (int)uni(j));
      const uint32_t len = (uint32_t)__builtin_amdgcn_readlane((int)r.b, (int)uni(j));
      const uint32_t lit = ra & 0x1ffffu, dist = (ra >> 17) + 1u;
      const uint32_t items = lit + (len ? mc_dfl_npairs(len) : 0u);
      for (uint32_t k = 0; k < items; k += WAVE) {
        const uint32_t i = k + lane;
        uint64_t val = 0;
        uint32_t nb = 0;
        if (i < lit) {
          if (pos + i < n) {
            const uint32_t e = lltab[src[pos + i]];
            val = e & 0xffffu, nb = e >> 16;
          }
        } else if (i < items) {
          nb = mc_dfl_pair_bits(lltab, dtab, mc_dfl_piece(len, i - lit), dist, &val);
        }
        bw.put(val, nb);
      }
      pos += lit + len;
    }
  }
  bw.put(lltab[256] & 0xffffu, lane == 0 ? lltab[256] >> 16 : 0u);
  if (!final) bw.skip(3);
  bw.skip((0u - bw.cur) & 7u);
  if (!final) bw.put(0xffff0000u, lane == 0 ? 32u : 0u);
  bw.flush(true);
}

constexpr size_t WS_ALIGN = 256;
size_t up(size_t v) { return (v + WS_ALIGN - 1) / WS_ALIGN * WS_ALIGN; }
struct ws_layout {
  size_t segs, hist, lens, mode, seqs, total;
};
ws_layout ws_plan(size_t nchunks, size_t nsegs, size_t nseqs) {
  ws_layout w;
  w.segs = 0;
  w.hist = w.segs + up(nsegs * sizeof(mc_dfl_seg));
  w.lens = w.hist + up(nsegs * MC_DFL_HIST * sizeof(uint32_t));
  w.mode = w.lens + up(nsegs * MC_DFL_LENS);
  w.seqs = w.mode + up(nchunks * sizeof(uint32_t));
  w.total = w.seqs + nseqs * sizeof(mc_dfl_seq);
  return w;
}

}  // namespace

static_assert(sizeof(mc_dfl_enc_chunk) == 40 && sizeof(mc_dfl_seg) == 48 && sizeof(mc_dfl_seq) == 8,
              "record layout (include/mcodec.h)");

extern "C" {

size_t mc_deflate_encode_workspace(size_t nchunks, size_t nsegments, size_t nsequences) {
  return ws_plan(nchunks, nsegments, nsequences).total;
}

int mc_deflate_encode_batch(const void *src, const void *chunk_table, size_t nchunks, size_t nsegments,
                            size_t nsequences, void *workspace, size_t workspace_bytes, uint32_t *cbytes_out, int32_t *err,
                            mc_stream_t stream) {
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
  a.table = static_cast<const mc_dfl_enc_chunk *>(chunk_table);
  a.nchunks = (uint32_t)nchunks, a.nsegs = (uint32_t)nsegments;
  a.nseqs = nsequences;
  a.segs = reinterpret_cast<mc_dfl_seg *>(ws + w.segs);
  a.hist = reinterpret_cast<uint32_t *>(ws + w.hist);
  a.lens = ws + w.lens;
  a.mode = reinterpret_cast<uint32_t *>(ws + w.mode);
  a.seqs = reinterpret_cast<mc_dfl_seq *>(ws + w.seqs);
  a.cbytes_out = cbytes_out;
  a.err = err;
  hipLaunchKernelGGL(dfl_parse_kernel, dim3((unsigned)nsegments), dim3(WAVE), 0, st, a);
  rc = mc_last_launch();
  if (rc != MC_OK) return rc;
  hipLaunchKernelGGL(dfl_code_kernel, dim3((unsigned)nsegments), dim3(WAVE), 0, st, a);
  rc = mc_last_launch();
  if (rc != MC_OK) return rc;
  hipLaunchKernelGGL(dfl_layout_kernel, dim3((unsigned)nchunks), dim3(MC_BLOCK), 0, st, a);
  rc = mc_last_launch();
  if (rc != MC_OK) return rc;
  hipLaunchKernelGGL(dfl_emit_kernel, dim3((unsigned)nsegments), dim3(WAVE), 0, st, a);
  return mc_last_launch();
}

}  // extern "C"
