// mc_blosc_enc.hip -- already-filtered block bytes -> Blosc1 LZ4 frames on the
// device, for a whole batch of frames: three launches.  The match-finding and
// emission rules, the scalar encoder they are checked against and the frame
// layout helpers live in mc_lz4_enc.h (compiled for the host too,
// tests/native_lz4enc); the wave-wide match finder (encode_wave) is
// mc_lz4_wave.h's.  The forward shuffle is mc_blosc_filter's job.
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
#include "mc_lz4_wave.h"  // encode_wave: the match finder, shared with mc_lz4_codec.hip

namespace {

using namespace mc_lz4w;

// the frame whose [stream_base, next stream_base) holds stream s
MC_DEV uint32_t frame_of_stream(const mc_blosc_enc_frame *table, uint32_t nframes, uint32_t s) {
  uint32_t lo = 0, hi = nframes - 1;
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1) >> 1;
    if (table[mid].stream_base <= s) lo = mid; else hi = mid - 1;
  }
  return lo;
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
    mc_lz4e_marks marks;  // a stitching caller's; unused here
    out = encode_wave(mc_uniform_ptr(src), neb, mc_uniform_ptr(dst), neb, tbl, lane, &marks);
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
