// mc_lz4_codec.hip -- the `lz4` codec (a 4-byte size word + one LZ4 block per
// chunk) on the device, for a whole batch of chunks.  The segmenting and
// stitching rules, the scalar encoder the kernels are checked against, the
// record predicates and the decode plan live in mc_lz4_codec.h (compiled for
// the host too, tests/native_lz4codec); the wave-wide match finder and
// sequence decoder are mc_lz4_wave.h's, shared with the Blosc kernels.
//
// Encode, three launches:
// compress: one wave (a 64-lane workgroup) per 64 KiB segment of the batch:
//           encode_wave into the segment's scratch slot; per segment its
//           compressed size (0 = no match / not smaller), the first
//           sequence's literal length, the closing token's offset and the
//           closing literal length.
// layout:   one workgroup per chunk.  The carry that enters each segment is a
//           segmented sum (a no-match segment adds its length, a body segment
//           resets it to its tail): thread t composes its own run of segments,
//           a block-wide scan composes the runs.  A second scan turns the
//           pieces' sizes into offsets and the exact frame length, which is
//           checked against the slot before anything is written.  A walk back
//           gives every segment the place its own carried bytes land: behind
//           the token and extension bytes of the next body segment's piece,
//           or of the closing sequence.
// gather:   one workgroup per segment: a body segment writes its rewritten
//           head and copies the rest of its body from scratch; every segment
//           copies its own carried bytes (its tail, or all of it) to their
//           place, so an incompressible chunk is copied by all its
//           workgroups; the last segment's workgroup writes the closing token
//           and its extension bytes.  Plain vector stores only.
//
// Decode, two launches: a plan (one thread per chunk: the size word re-read
// and checked against the record) and decode_wave, one wave per chunk through
// the LDS history ring.  One block is one serial chain: throughput comes from
// the batch.
#include "mc_common.h"
#include "mc_lz4_codec.h"
#include "mc_lz4_wave.h"

namespace {

using namespace mc_lz4w;

struct enc_args {
  uint64_t base;
  const mc_lz4c_enc_chunk *table;
  uint32_t nchunks, nsegs;
  uint8_t *scratch;
  uint64_t scratch_bytes;
  // per segment
  uint32_t *csize;      // compressed size, 0 = all literals
  uint32_t *first_lit;  // literal length of the first sequence
  uint32_t *close_at;   // scratch offset of the closing token
  uint32_t *tail_lit;   // closing literal length
  uint32_t *carry_in;   // carried bytes that enter the segment
  uint32_t *piece_off;  // frame offset of a body segment's piece
  uint32_t *lit_at;     // frame offset of the segment's own carried bytes
  // per chunk
  uint32_t *mode;       // 0 refused, 1 encoded
  uint32_t *close_off;  // frame offset of the closing token
  uint32_t *last_carry; // the closing literal length
  uint32_t *cbytes_out; // the frame's length, 0 when the record was refused
};

// the chunk whose [seg_base, next seg_base) holds segment s
MC_DEV uint32_t chunk_of_segment(const mc_lz4c_enc_chunk *table, uint32_t nchunks, uint32_t s) {
  uint32_t lo = 0, hi = nchunks - 1;
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1) >> 1;
    if (table[mid].seg_base <= s) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__global__ void __launch_bounds__(WAVE) lz4c_compress_kernel(enc_args a) {
  __shared__ __attribute__((aligned(16))) uint32_t tbl[MC_LZ4E_TABLE];
  const uint32_t seg = blockIdx.x, lane = threadIdx.x;
  if (seg >= a.nsegs) return;
  const uint32_t ci = chunk_of_segment(a.table, a.nchunks, seg);
  const mc_lz4c_enc_chunk c = a.table[ci];
  uint32_t out = 0;
  mc_lz4e_marks marks{0u, 0u, 0u};
  if (mc_lz4c_enc_chunk_ok(c, a.nsegs, a.scratch_bytes) && seg - c.seg_base < mc_lz4c_nsegments(c.nbytes)) {
    const uint32_t k = seg - c.seg_base, start = k * MC_LZ4C_SEGMENT;
    const uint32_t nk = uni(mc_lz4c_seg_len(c.nbytes, k));
    const uint8_t *src = reinterpret_cast<const uint8_t *>((uintptr_t)(a.base + c.src)) + start;
    uint8_t *dst = a.scratch + c.scratch_off + start;  // start + nk <= nbytes <= the chunk's scratch range
    out = encode_wave(mc_uniform_ptr(src), nk, mc_uniform_ptr(dst), nk, tbl, lane, &marks);
  }
  if (lane == 0) {
    a.csize[seg] = out;
    a.first_lit[seg] = marks.first_lit;
    a.close_at[seg] = marks.close_at;
    a.tail_lit[seg] = marks.tail_lit;
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

__global__ void __launch_bounds__(MC_BLOCK) lz4c_layout_kernel(enc_args a) {
  __shared__ uint32_t run_v[MC_BLOCK], run_b[MC_BLOCK];  // carry scan: value, "holds a body segment"
  __shared__ uint32_t sums[MC_BLOCK];                    // piece sizes
  __shared__ uint32_t nx_has[MC_BLOCK], nx_lit[MC_BLOCK], nx_from[MC_BLOCK];  // a thread's first consumer
  const uint32_t ci = blockIdx.x, t = threadIdx.x;
  if (ci >= a.nchunks) return;
  const mc_lz4c_enc_chunk c = a.table[ci];
  if (!mc_lz4c_enc_chunk_ok(c, a.nsegs, a.scratch_bytes)) {
    if (t == 0) a.mode[ci] = 0, a.cbytes_out[ci] = 0;
    return;
  }
  const uint32_t n = c.nbytes, nseg = mc_lz4c_nsegments(n);
  const uint32_t *cs = a.csize + c.seg_base, *fl = a.first_lit + c.seg_base, *ca = a.close_at + c.seg_base,
                 *tl = a.tail_lit + c.seg_base;
  // thread t owns segments [lo, hi)
  const uint32_t per = (nseg + MC_BLOCK - 1) / MC_BLOCK;
  const uint32_t lo = t * per < nseg ? t * per : nseg, hi = lo + per < nseg ? lo + per : nseg;

  // ---- the carry: run t maps an incoming carry x to (b ? v : x + v) ----
  uint32_t v = 0, b = 0;
  for (uint32_t s = lo; s < hi; ++s) {
    if (cs[s]) v = tl[s], b = 1; else v += mc_lz4c_seg_len(n, s);
  }
  run_v[t] = v, run_b[t] = b;
  __syncthreads();
  for (uint32_t d = 1; d < MC_BLOCK; d <<= 1) {  // inclusive scan under composition
    const uint32_t lv = t >= d ? run_v[t - d] : 0, lb = t >= d ? run_b[t - d] : 0;
    __syncthreads();
    if (!run_b[t]) run_v[t] += lv, run_b[t] = lb;
    __syncthreads();
  }
  const uint32_t carry0 = t ? run_v[t - 1] : 0;  // the chunk starts with carry 0
  const uint32_t last_carry = run_v[MC_BLOCK - 1];

  // ---- the pieces' sizes -> offsets, and the exact frame length ----
  uint32_t mine = 0, carry = carry0;
  for (uint32_t s = lo; s < hi; ++s) {
    if (cs[s]) mine += mc_lz4c_piece_bytes(carry, fl[s], ca[s]), carry = tl[s];
    else carry += mc_lz4c_seg_len(n, s);
  }
  sums[t] = mine;
  __syncthreads();
  block_scan_add(sums, t);
  // pieces <= n + n / 255 + 2 < 2^31 (mc_lz4_codec.h): 32 bits hold every offset
  const uint32_t close_off = MC_LZ4C_HEADER + sums[MC_BLOCK - 1];
  const uint32_t cbytes = close_off + mc_lz4e_last_bytes(last_carry);
  if (cbytes > c.dst_cap) {  // the same for every thread: nothing of the chunk is written
    if (t == 0) a.mode[ci] = 0, a.cbytes_out[ci] = 0;
    return;
  }
  uint8_t *dst = reinterpret_cast<uint8_t *>((uintptr_t)c.dst);
  if (t == 0) {
    mc_lz4e_put32(dst, n);
    a.mode[ci] = 1, a.close_off[ci] = close_off, a.last_carry[ci] = last_carry, a.cbytes_out[ci] = cbytes;
  }
  uint32_t at = MC_LZ4C_HEADER + sums[t] - mine;
  carry = carry0;
  // this thread's first body segment: where the run of carried bytes that
  // ends at its start lands (behind its token and extension bytes), and the
  // source position the run begins at
  uint32_t has = 0, first_lit_at = 0, first_from = 0;
  for (uint32_t s = lo; s < hi; ++s) {
    a.carry_in[c.seg_base + s] = carry;
    a.piece_off[c.seg_base + s] = at;
    if (cs[s]) {
      if (!has) has = 1, first_lit_at = at + 1 + mc_lz4e_ext_count(carry + fl[s]), first_from = s * MC_LZ4C_SEGMENT - carry;
      at += mc_lz4c_piece_bytes(carry, fl[s], ca[s]);
      carry = tl[s];
    } else {
      carry += mc_lz4c_seg_len(n, s);
    }
  }
  nx_has[t] = has, nx_lit[t] = first_lit_at, nx_from[t] = first_from;
  __syncthreads();

  // ---- where each segment's own carried bytes go: walk back from the consumer ----
  uint32_t lit_at = close_off + 1 + mc_lz4e_ext_count(last_carry), from = n - last_carry;  // the closing sequence
  for (uint32_t u = t + 1; u < MC_BLOCK; ++u) {
    if (nx_has[u]) {
      lit_at = nx_lit[u], from = nx_from[u];
      break;
    }
  }
  for (uint32_t s = hi; s-- > lo;) {
    const uint32_t nk = mc_lz4c_seg_len(n, s), end = s * MC_LZ4C_SEGMENT + nk;
    const uint32_t own = cs[s] ? tl[s] : nk;
    a.lit_at[c.seg_base + s] = lit_at + (end - own - from);  // end - own >= from: the run starts no later
    if (cs[s]) {  // segments before s feed s
      const uint32_t cin = a.carry_in[c.seg_base + s];  // this thread's own store
      lit_at = a.piece_off[c.seg_base + s] + 1 + mc_lz4e_ext_count(cin + fl[s]);
      from = s * MC_LZ4C_SEGMENT - cin;
    }
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

// token(lit, low nibble of `low`) and lit's extension bytes at d, by the workgroup
MC_DEV void wg_put_head(uint8_t *d, uint32_t lit, uint8_t low) {
  const uint32_t ne = mc_lz4e_ext_count(lit);
  if (threadIdx.x == 0) d[0] = mc_lz4c_head_token(lit, low);
  for (uint32_t i = threadIdx.x; i < ne; i += MC_BLOCK) d[1 + i] = mc_lz4e_ext_byte(lit, ne, i);
}

// Every offset below was derived by the layout kernel from the same records
// and segment results, and the frame's exact length was checked against the
// slot there: all writes land in [4, cbytes) of the slot.
__global__ void __launch_bounds__(MC_BLOCK) lz4c_gather_kernel(enc_args a) {
  const uint32_t seg = blockIdx.x;
  if (seg >= a.nsegs) return;
  const uint32_t ci = chunk_of_segment(a.table, a.nchunks, seg);
  if (a.mode[ci] == 0) return;
  const mc_lz4c_enc_chunk c = a.table[ci];
  const uint32_t k = seg - c.seg_base, nseg = mc_lz4c_nsegments(c.nbytes);
  if (k >= nseg) return;
  const uint32_t start = k * MC_LZ4C_SEGMENT, nk = mc_lz4c_seg_len(c.nbytes, k);
  const uint8_t *src = reinterpret_cast<const uint8_t *>((uintptr_t)(a.base + c.src)) + start;
  uint8_t *dst = reinterpret_cast<uint8_t *>((uintptr_t)c.dst);
  const uint32_t cs = a.csize[seg];
  const uint32_t own = cs ? a.tail_lit[seg] : nk;
  wg_copy_bytes(src + (nk - own), dst + a.lit_at[seg], own);
  if (cs) {
    const uint8_t *scr = a.scratch + c.scratch_off + start;
    const uint32_t cin = a.carry_in[seg], l0 = a.first_lit[seg], at = a.piece_off[seg];
    const uint32_t lit = cin + l0, ne = mc_lz4e_ext_count(lit), skip = mc_lz4c_body_skip(l0);
    wg_put_head(dst + at, lit, scr[0]);
    wg_copy_bytes(src, dst + at + 1 + ne + cin, l0);  // the carried bytes before them are their owners' to copy
    wg_copy_bytes(scr + skip, dst + at + 1 + ne + lit, a.close_at[seg] - skip);
  }
  if (k + 1 == nseg) wg_put_head(dst + a.close_off[ci], a.last_carry[ci], 0);
}

// ---- decode ----------------------------------------------------------------
__global__ void __launch_bounds__(MC_BLOCK)
lz4c_plan_kernel(const uint8_t *__restrict__ frames, const mc_lz4c_dec_chunk *__restrict__ table, uint32_t nchunks,
            uint32_t max_usize, mc_lz4_stream *__restrict__ streams, int32_t *__restrict__ err) {
  const uint32_t i = blockIdx.x * MC_BLOCK + threadIdx.x;
  if (i >= nchunks) return;
  mc_lz4_stream d;
  const int e = mc_lz4c_plan_chunk(frames, table[i], i, max_usize, &d);
  streams[i] = d;
  if (e != MC_LZ4_OK) err[2 * i] = e, err[2 * i + 1] = 0;
}

__global__ void __launch_bounds__(WAVE)
lz4c_decode_kernel(const uint8_t *__restrict__ frames, const mc_lz4_stream *__restrict__ streams, uint32_t nchunks,
              uint32_t ring_mask, int32_t *__restrict__ err) {
  extern __shared__ uint8_t ring[];
  const uint32_t i = blockIdx.x, lane = threadIdx.x;
  if (i >= nchunks) return;
  const mc_lz4_stream d = streams[i];
  if (!(d.flags & MC_LZ4_S_VALID)) return;
  const uint8_t *src = frames + d.src_off;
  uint8_t *dst = reinterpret_cast<uint8_t *>((uintptr_t)d.dst);
  const uint32_t n = uni(d.cbytes), usize = uni(d.usize);
  uint32_t produced;
  const int e = decode_wave(src, n, dst, usize, ring, ring_mask, lane, &produced);
  if (lane == 0) err[2 * i] = e, err[2 * i + 1] = (int32_t)produced;  // one stream per chunk: no other writer
}

constexpr size_t WS_ALIGN = 256;
constexpr size_t SEG_WORDS = 7, CHUNK_WORDS = 3;
size_t words_bytes(size_t nchunks, size_t nsegs) {
  return ((SEG_WORDS * nsegs + CHUNK_WORDS * nchunks) * sizeof(uint32_t) + WS_ALIGN - 1) / WS_ALIGN * WS_ALIGN;
}

}  // namespace

extern "C" {

size_t mc_lz4_encode_workspace(size_t nchunks, size_t nsegments, size_t scratch_bytes) {
  return words_bytes(nchunks, nsegments) + scratch_bytes;
}

int mc_lz4_encode_batch(const void *src, const void *chunk_table, size_t nchunks, size_t nsegments, void *workspace,
                        size_t workspace_bytes, uint32_t *cbytes_out, mc_stream_t stream) {
  if (nchunks == 0) return MC_OK;
  if (!chunk_table || !workspace || !cbytes_out) return MC_EINVAL;
  if (nchunks > 0x7fffffffu || nsegments > 0x7fffffffu || nsegments < nchunks) return MC_EINVAL;
  if (((uintptr_t)workspace & 7) || ((uintptr_t)chunk_table & 7) || ((uintptr_t)cbytes_out & 3)) return MC_EINVAL;
  if (workspace_bytes < words_bytes(nchunks, nsegments)) return MC_ENOSPC;
  hipStream_t st = (hipStream_t)stream;
  uint32_t *w = static_cast<uint32_t *>(workspace);
  enc_args a;
  a.base = (uint64_t)(uintptr_t)src;
  a.table = static_cast<const mc_lz4c_enc_chunk *>(chunk_table);
  a.nchunks = (uint32_t)nchunks, a.nsegs = (uint32_t)nsegments;
  a.scratch = static_cast<uint8_t *>(workspace) + words_bytes(nchunks, nsegments);
  a.scratch_bytes = workspace_bytes - words_bytes(nchunks, nsegments);
  a.csize = w, a.first_lit = w + nsegments, a.close_at = w + 2 * nsegments, a.tail_lit = w + 3 * nsegments;
  a.carry_in = w + 4 * nsegments, a.piece_off = w + 5 * nsegments, a.lit_at = w + 6 * nsegments;
  uint32_t *pc = w + SEG_WORDS * nsegments;
  a.mode = pc, a.close_off = pc + nchunks, a.last_carry = pc + 2 * nchunks;
  a.cbytes_out = cbytes_out;
  hipLaunchKernelGGL(lz4c_compress_kernel, dim3((unsigned)nsegments), dim3(WAVE), 0, st, a);
  int rc = mc_last_launch();
  if (rc != MC_OK) return rc;
  hipLaunchKernelGGL(lz4c_layout_kernel, dim3((unsigned)nchunks), dim3(MC_BLOCK), 0, st, a);
  rc = mc_last_launch();
  if (rc != MC_OK) return rc;
  hipLaunchKernelGGL(lz4c_gather_kernel, dim3((unsigned)nsegments), dim3(MC_BLOCK), 0, st, a);
  return mc_last_launch();
}

size_t mc_lz4_decode_workspace(size_t nchunks) { return nchunks * sizeof(mc_lz4_stream) + 16; }

int mc_lz4_decode_batch(const void *frames, const void *chunk_table, size_t nchunks, size_t max_usize,
                        void *workspace, size_t workspace_bytes, int32_t *err, mc_stream_t stream) {
  if (nchunks == 0) return MC_OK;
  if (!frames || !chunk_table || !workspace || !err) return MC_EINVAL;
  if (nchunks > 0x7fffffffu) return MC_EINVAL;
  if (max_usize == 0 || max_usize >= MC_LZ4_MAX_USIZE) return MC_EINVAL;
  if (((uintptr_t)workspace & 7) || ((uintptr_t)chunk_table & 7) || ((uintptr_t)err & 3)) return MC_EINVAL;
  if (workspace_bytes < mc_lz4_decode_workspace(nchunks)) return MC_ENOSPC;
  hipStream_t st = (hipStream_t)stream;
  int rc = mc_hip_status(hipMemsetAsync(err, 0, nchunks * 2 * sizeof(int32_t), st));
  if (rc != MC_OK) return rc;
  const uint8_t *fr = static_cast<const uint8_t *>(frames);
  const mc_lz4c_dec_chunk *table = static_cast<const mc_lz4c_dec_chunk *>(chunk_table);
  mc_lz4_stream *streams = static_cast<mc_lz4_stream *>(workspace);
  const unsigned pgrid = (unsigned)((nchunks + MC_BLOCK - 1) / MC_BLOCK);
  hipLaunchKernelGGL(lz4c_plan_kernel, dim3(pgrid), dim3(MC_BLOCK), 0, st, fr, table, (uint32_t)nchunks,
                     (uint32_t)max_usize, streams, err);
  rc = mc_last_launch();
  if (rc != MC_OK) return rc;
  const uint32_t rb = ring_bytes(max_usize);
  hipLaunchKernelGGL(lz4c_decode_kernel, dim3((unsigned)nchunks), dim3(WAVE), rb, st, fr, streams, (uint32_t)nchunks,
                     rb - 1, err);
  return mc_last_launch();
}

}  // extern "C"
