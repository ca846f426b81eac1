// mc_blosc_enc.hip -- already-filtered block bytes -> Blosc1 LZ4 frames on the
// device, for a whole batch of frames: three launches.  The match-finding and
// emission rules, the scalar encoder they are checked against and the frame
// layout helpers live in mc_lz4_enc.h (compiled for the host too,
// tests/native_lz4enc).  The forward shuffle is mc_blosc_filter's job.
//
// compress: one wave (a 64-lane workgroup) per stream, wave-uniform control
//           flow.  The source is read-only, so candidate words and match
//           extensions are read straight from global memory; the 4096-entry
//           hash table (16 KiB of LDS) holds position + 1 and is updated with
//           ds_max, so "the highest position wins an entry" does not depend
//           on which lane's write lands last (positions only grow along the
//           stream, so the highest is also the latest).  A window's lookups
//           all issue before its inserts, and lds_order() separates the
//           inserts from the next window's lookups.  Output: a scratch slot of
//           the stream's size, and its compressed size (0 = store raw).
// layout:   one workgroup per frame scans the streams' sizes into stream
//           offsets, the bstarts table, the frame's cbytes and the memcpyed
//           decision, and writes the header.
// gather:   one workgroup per stream copies the cbytes word and the stream's
//           bytes (scratch, or the filtered source when raw) into the frame's
//           slot; for a memcpyed frame its share of the unfiltered input.
#include "mc_common.h"
#include "mc_lz4_enc.h"

namespace {

constexpr uint32_t WAVE = 64;

MC_DEV uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
// see mc_blosc_dec.hip: orders this wave's LDS accesses across the call
MC_DEV void lds_order() { __asm__ volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

MC_DEV uint32_t ld_le32(const uint8_t *p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// the frame whose [stream_base, next stream_base) holds stream s
MC_DEV uint32_t frame_of_stream(const mc_blosc_enc_frame *table, uint32_t nframes, uint32_t s) {
  uint32_t lo = 0, hi = nframes - 1;
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1) >> 1;
    if (table[mid].stream_base <= s) lo = mid; else hi = mid - 1;
  }
  return lo;
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
                            uint32_t *tbl, uint32_t lane) {
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
  const uint32_t nle = mc_lz4e_ext_count(lit);
  if (lane == 0) dst[op] = mc_lz4e_token(lit, 0);
  uint8_t *q = dst + op + 1;
  put_ext(q, lit, nle, lane);
  q += nle;
  for (uint32_t k = lane; k < lit; k += WAVE) q[k] = src[anchor + k];
  op += 1 + nle + lit;
  return op < n ? op : 0;
}

struct enc_args {
  uint64_t base;
  const mc_blosc_enc_frame *table;
  uint32_t nframes, nblocks, nstreams;
  uint8_t *scratch;
  uint64_t scratch_bytes;
  uint32_t *csize;      // per stream: compressed size, 0 = raw
  uint32_t *out_off;    // per stream: offset of its cbytes word in the frame
  uint32_t *frame_mode; // per frame: 0 skipped (bad record), 1 compressed, 2 memcpyed
  uint32_t *cbytes_out; // per frame: the frame's length, 0 when the record was refused
};

__global__ void __launch_bounds__(WAVE) compress_kernel(enc_args a) {
  __shared__ __attribute__((aligned(16))) uint32_t tbl[MC_LZ4E_TABLE];
  const uint32_t sidx = blockIdx.x, lane = threadIdx.x;
  if (sidx >= a.nstreams) return;
  const uint32_t fi = frame_of_stream(a.table, a.nframes, sidx);
  const mc_blosc_enc_frame f = a.table[fi];
  uint32_t out = 0;
  if (mc_blosc_enc_frame_ok(f, a.nblocks, a.nstreams, a.scratch_bytes) && !(f.flags & MC_BLOSC_F_MEMCPYED) &&
      sidx - f.stream_base < mc_blosc_nstreams(f.flags, f.typesize, f.nbytes, f.blocksize)) {
    uint32_t block, first, off, neb;
    mc_blosc_enc_stream(f, sidx - f.stream_base, &block, &first, &off, &neb);
    const uint8_t *src = reinterpret_cast<const uint8_t *>((uintptr_t)(a.base + f.src)) + off;
    uint8_t *dst = a.scratch + f.scratch_off + off;
    neb = uni(neb);
    out = encode_wave(mc_uniform_ptr(src), neb, mc_uniform_ptr(dst), neb, tbl, lane);
  }
  if (lane == 0) a.csize[sidx] = out;
}

__global__ void __launch_bounds__(MC_BLOCK) layout_kernel(enc_args a) {
  __shared__ uint64_t sums[MC_BLOCK];
  const uint32_t fi = blockIdx.x, t = threadIdx.x;
  if (fi >= a.nframes) return;
  const mc_blosc_enc_frame f = a.table[fi];
  if (!mc_blosc_enc_frame_ok(f, a.nblocks, a.nstreams, a.scratch_bytes)) {
    if (t == 0) a.frame_mode[fi] = 0, a.cbytes_out[fi] = 0;
    return;
  }
  const uint32_t ns = mc_blosc_nstreams(f.flags, f.typesize, f.nbytes, f.blocksize);
  const uint32_t nblocks = mc_blosc_nblocks(f.nbytes, f.blocksize);
  const uint32_t *cs = a.csize + f.stream_base;
  // thread t owns streams [lo, hi): its sum, an exclusive scan of the sums, then its offsets
  const uint32_t per = (ns + MC_BLOCK - 1) / MC_BLOCK;
  const uint32_t lo = t * per < ns ? t * per : ns, hi = lo + per < ns ? lo + per : ns;
  uint64_t mine = 0;
  for (uint32_t s = lo; s < hi; ++s) {
    uint32_t block, first, off, neb;
    mc_blosc_enc_stream(f, s, &block, &first, &off, &neb);
    mine += mc_blosc_enc_stream_bytes(cs[s], neb);
  }
  sums[t] = mine;
  __syncthreads();
  for (uint32_t d = 1; d < MC_BLOCK; d <<= 1) {
    const uint64_t add = t >= d ? sums[t - d] : 0;
    __syncthreads();
    sums[t] += add;
    __syncthreads();
  }
  const uint64_t head = (uint64_t)MC_BLOSC_HEADER + 4ull * nblocks;
  const uint64_t total = head + sums[MC_BLOCK - 1];
  const bool stored = mc_blosc_enc_memcpyed(f, total);
  uint8_t *dst = reinterpret_cast<uint8_t *>((uintptr_t)f.dst);
  const uint32_t cbytes = stored ? f.nbytes + MC_BLOSC_MAX_OVERHEAD : (uint32_t)total;
  if (t == 0) {
    mc_blosc_enc_header(dst, f, stored, cbytes);
    a.frame_mode[fi] = stored ? 2u : 1u;
    a.cbytes_out[fi] = cbytes;
  }
  if (stored) return;  // total <= nbytes + 16 from here on: offsets fit 32 bits
  uint64_t at = head + sums[t] - mine;
  for (uint32_t s = lo; s < hi; ++s) {
    uint32_t block, first, off, neb;
    mc_blosc_enc_stream(f, s, &block, &first, &off, &neb);
    a.out_off[f.stream_base + s] = (uint32_t)at;
    if (first) mc_lz4e_put32(dst + MC_BLOSC_HEADER + 4ull * block, (uint32_t)at);
    at += mc_blosc_enc_stream_bytes(cs[s], neb);
  }
}

MC_DEV void wg_copy_bytes(const uint8_t *__restrict__ s, uint8_t *__restrict__ d, uint32_t n) {
  if ((((uintptr_t)s | (uintptr_t)d) & 3) == 0) {
    const uint32_t nw = n >> 2;
    for (uint32_t i = threadIdx.x; i < nw; i += MC_BLOCK)
      reinterpret_cast<uint32_t *>(d)[i] = reinterpret_cast<const uint32_t *>(s)[i];
    for (uint32_t i = (nw << 2) + threadIdx.x; i < n; i += MC_BLOCK) d[i] = s[i];
  } else {
    for (uint32_t i = threadIdx.x; i < n; i += MC_BLOCK) d[i] = s[i];
  }
}

__global__ void __launch_bounds__(MC_BLOCK) gather_kernel(enc_args a) {
  const uint32_t sidx = blockIdx.x;
  if (sidx >= a.nstreams) return;
  const uint32_t fi = frame_of_stream(a.table, a.nframes, sidx);
  const uint32_t mode = a.frame_mode[fi];
  if (mode == 0) return;
  const mc_blosc_enc_frame f = a.table[fi];
  if (sidx - f.stream_base >= mc_blosc_nstreams(f.flags, f.typesize, f.nbytes, f.blocksize)) return;
  uint32_t block, first, off, neb;
  mc_blosc_enc_stream(f, sidx - f.stream_base, &block, &first, &off, &neb);
  uint8_t *dst = reinterpret_cast<uint8_t *>((uintptr_t)f.dst);
  if (mode == 2) {  // the stream's share of the unfiltered input, behind the header
    wg_copy_bytes(reinterpret_cast<const uint8_t *>((uintptr_t)(a.base + f.raw)) + off, dst + MC_BLOSC_HEADER + off, neb);
    return;
  }
  const uint32_t cs = a.csize[sidx], at = a.out_off[sidx];
  const uint32_t nb = cs ? cs : neb;  // at + 4 + nb <= the frame's cbytes <= nbytes + 16 (layout)
  if (threadIdx.x < 4) dst[at + threadIdx.x] = (uint8_t)(nb >> (8 * threadIdx.x));
  const uint8_t *from = cs ? a.scratch + f.scratch_off + off
                           : reinterpret_cast<const uint8_t *>((uintptr_t)(a.base + f.src)) + off;
  wg_copy_bytes(from, dst + at + 4, nb);
}

constexpr size_t WS_ALIGN = 256;
size_t words_bytes(size_t nstreams) { return (3 * nstreams * sizeof(uint32_t) + WS_ALIGN - 1) / WS_ALIGN * WS_ALIGN; }

}  // namespace

extern "C" {

size_t mc_blosc_encode_workspace(size_t nstreams, size_t scratch_bytes) {
  return words_bytes(nstreams) + scratch_bytes;
}

int mc_blosc_encode_batch(const void *src, const void *frame_table, size_t nframes, size_t nblocks,
                          size_t nstreams, void *workspace, size_t workspace_bytes, uint32_t *cbytes_out,
                          mc_stream_t stream) {
  if (nframes == 0) return MC_OK;
  if (!frame_table || !workspace || !cbytes_out) return MC_EINVAL;
  if (nframes > 0x7fffffffu || nblocks > 0x7fffffffu || nstreams > 0x7fffffffu || nstreams < nblocks ||
      nblocks < nframes)
    return MC_EINVAL;
  if (((uintptr_t)workspace & 7) ||((uintptr_t)frame_table & 7) || ((uintptr_t)cbytes_out & 3)) return MC_EINVAL;
  if (workspace_bytes < words_bytes(nstreams)) return MC_ENOSPC;
  hipStream_t st = (hipStream_t)stream;
  uint32_t *words = static_cast<uint32_t *>(workspace);
  enc_args a;
  a.base = (uint64_t)(uintptr_t)src;
  a.table = static_cast<const mc_blosc_enc_frame *>(frame_table);
  a.nframes = (uint32_t)nframes, a.nblocks = (uint32_t)nblocks, a.nstreams = (uint32_t)nstreams;
  a.scratch = static_cast<uint8_t *>(workspace) + words_bytes(nstreams);
  a.scratch_bytes = workspace_bytes - words_bytes(nstreams);
  a.csize = words, a.out_off = words + nstreams, a.frame_mode = words + 2 * nstreams;
  a.cbytes_out = cbytes_out;
  hipLaunchKernelGGL(compress_kernel, dim3((unsigned)nstreams), dim3(WAVE), 0, st, a);
  int rc = mc_last_launch();
  if (rc != MC_OK) return rc;
  hipLaunchKernelGGL(layout_kernel, dim3((unsigned)nframes), dim3(MC_BLOCK), 0, st, a);
  rc = mc_last_launch();
  if (rc != MC_OK) return rc;
  hipLaunchKernelGGL(gather_kernel, dim3((unsigned)nstreams), dim3(MC_BLOCK), 0, st, a);
  return mc_last_launch();
}

}  // extern "C"
