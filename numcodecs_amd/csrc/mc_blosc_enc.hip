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
//
// cname='zstd' (mc_blosc_encode_batch_z): the frames always carry the
// do-not-split bit, so a stream is a block, and every block becomes one
// Zstandard frame through mc_zstd_encode_batch's four kernels (parse / code /
// layout / emit: 64 KiB segments, Frame_Content_Size, no checksum) in the place
// of `compress`:
// chunks:   one thread per block writes the encoder's chunk record: the block's
//           filtered bytes -> its scratch slot, dst_cap = block size - 1;
//           seg_base / seq_base from the frame's bases (pure functions of the
//           sizes, the caller's) and the block's index.
// bridge:   one thread per block turns the encoder's size / error record into
//           `csize` (a refused frame -- it does not get smaller -- is 0: raw).
// layout and gather are the ones above.
#include "mc_common.h"
#include "mc_lz4_enc.h"
#include "mc_lz4_wave.h"  // encode_wave: the match finder, shared with mc_lz4_codec.hip
#include "mc_zstd_enc.h"  // mc_zstd_enc_chunk and the segment / sequence counts (mc_blosc_encode_batch_z)

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

// ---- cname='zstd' ----
struct z_args {
  enc_args e;
  const uint32_t *bases;     // per frame: index of its first segment, of its first sequence record
  mc_zstd_enc_chunk *chunks; // per stream
  uint32_t *zsize;           // per stream: the encoder's cbytes_out
  int32_t *zerr;             // per stream: the encoder's error record (2 words)
  uint32_t nsegs;
  uint64_t nseqs;
};

// the record of stream sidx; nbytes 0 (a chunk the encoder refuses) where the frame's record is bad
__global__ void __launch_bounds__(MC_BLOCK) z_chunks_kernel(z_args z) {
  const enc_args &a = z.e;
  const uint32_t sidx = blockIdx.x * MC_BLOCK + threadIdx.x;
  if (sidx >= a.nstreams) return;
  const uint32_t fi = frame_of_stream(a.table, a.nframes, sidx);
  const mc_blosc_enc_frame f = a.table[fi];
  mc_zstd_enc_chunk c;
  c.src = 0, c.dst = 0, c.nbytes = 0, c.dst_cap = 0, c.seg_base = 0, c.seq_base = 0, c.flags = 0, c.reserved = 0;
  // one stream per block: the do-not-split bit is required, a memcpyed frame is the lz4 entry point's
  if (mc_blosc_enc_frame_ok(f, a.nblocks, a.nstreams, a.scratch_bytes) && (f.flags & MC_BLOSC_F_NOSPLIT) &&
      !(f.flags & MC_BLOSC_F_MEMCPYED) && sidx - f.stream_base < mc_blosc_nblocks(f.nbytes, f.blocksize)) {
    uint32_t block, first, off, neb;
    mc_blosc_enc_stream(f, sidx - f.stream_base, &block, &first, &off, &neb);
    c.src = a.base + f.src + off;
    c.dst = (uint64_t)(uintptr_t)(a.scratch + f.scratch_off + off);
    c.nbytes = neb, c.dst_cap = neb - 1u;
    // the blocks before this one are full ones (the encoder checks the bases against the batch's totals)
    c.seg_base = z.bases[2 * fi] + block * mc_ze_nsegments(f.blocksize);
    c.seq_base = z.bases[2 * fi + 1] + block * mc_ze_seq_records(f.blocksize);
  }
  z.chunks[sidx] = c;
}

__global__ void __launch_bounds__(MC_BLOCK) z_bridge_kernel(z_args z) {
  const enc_args &a = z.e;
  const uint32_t sidx = blockIdx.x * MC_BLOCK + threadIdx.x;
  if (sidx >= a.nstreams) return;
  const uint32_t n = z.chunks[sidx].nbytes, cs = z.zsize[sidx];
  // a frame that was written is shorter than the block (dst_cap); anything else is stored raw
  a.csize[sidx] = (z.zerr[2 * sidx] == 0 && cs > 0 && cs < n) ? cs : 0u;
}

constexpr size_t WS_ALIGN = 256;
size_t up256(size_t v) { return (v + 255) / 256 * 256; }
struct z_layout {
  size_t words, chunks, zsize, zerr, zws, scratch;
};
z_layout z_plan(size_t nstreams, size_t nsegs, size_t nseqs) {
  z_layout w;
  w.words = 0;
  w.chunks = up256(3 * nstreams * sizeof(uint32_t));
  w.zsize = w.chunks + up256(nstreams * sizeof(mc_zstd_enc_chunk));
  w.zerr = w.zsize + up256(nstreams * sizeof(uint32_t));
  w.zws = w.zerr + up256(2 * nstreams * sizeof(int32_t));
  w.scratch = w.zws + up256(mc_zstd_encode_workspace(nstreams, nsegs, nseqs));
  return w;
}

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

size_t mc_blosc_encode_batch_z_workspace(size_t nstreams, size_t nsegments, size_t nsequences, size_t scratch_bytes) {
  return z_plan(nstreams, nsegments, nsequences).scratch + scratch_bytes;
}

int mc_blosc_encode_batch_z(const void *src, const void *frame_table, const uint32_t *frame_bases, size_t nframes,
                            size_t nblocks, size_t nsegments, size_t nsequences, void *workspace,
                            size_t workspace_bytes, uint32_t *cbytes_out, mc_stream_t stream) {
  if (nframes == 0) return MC_OK;
  if (!frame_table || !frame_bases || !workspace || !cbytes_out) return MC_EINVAL;
  if (nframes > 0x7fffffffu || nblocks > 0x7fffffffu || nblocks < nframes || nsegments > 0x7fffffffu ||
      nsegments < nblocks || nsequences > 0xffffffffu)
    return MC_EINVAL;
  if (((uintptr_t)workspace & 7) || ((uintptr_t)frame_table & 7) || ((uintptr_t)cbytes_out & 3) ||
      ((uintptr_t)frame_bases & 3))
    return MC_EINVAL;
  const size_t nstreams = nblocks;  // do-not-split: a stream is a block
  const z_layout w = z_plan(nstreams, nsegments, nsequences);
  if (workspace_bytes < w.scratch) return MC_ENOSPC;
  hipStream_t st = (hipStream_t)stream;
  uint8_t *ws = static_cast<uint8_t *>(workspace);
  uint32_t *words = reinterpret_cast<uint32_t *>(ws + w.words);
  z_args z;
  enc_args &a = z.e;
  a.base = (uint64_t)(uintptr_t)src;
  a.table = static_cast<const mc_blosc_enc_frame *>(frame_table);
  a.nframes = (uint32_t)nframes, a.nblocks = (uint32_t)nblocks, a.nstreams = (uint32_t)nstreams;
  a.scratch = ws + w.scratch;
  a.scratch_bytes = workspace_bytes - w.scratch;
  a.csize = words, a.out_off = words + nstreams, a.frame_mode = words + 2 * nstreams;
  a.cbytes_out = cbytes_out;
  z.bases = frame_bases;
  z.chunks = reinterpret_cast<mc_zstd_enc_chunk *>(ws + w.chunks);
  z.zsize = reinterpret_cast<uint32_t *>(ws + w.zsize);
  z.zerr = reinterpret_cast<int32_t *>(ws + w.zerr);
  z.nsegs = (uint32_t)nsegments, z.nseqs = nsequences;
  const unsigned sgrid = (unsigned)((nstreams + MC_BLOCK - 1) / MC_BLOCK);
  hipLaunchKernelGGL(z_chunks_kernel, dim3(sgrid), dim3(MC_BLOCK), 0, st, z);
  int rc = mc_last_launch();
  if (rc != MC_OK) return rc;
  // parse, code, layout, emit: the `zstd` encoder's own four launches (absolute addresses: no base)
  rc = mc_zstd_encode_batch(nullptr, z.chunks, nstreams, nsegments, nsequences, ws + w.zws, w.scratch - w.zws, z.zsize,
                            z.zerr, stream);
  if (rc != MC_OK) return rc;
  hipLaunchKernelGGL(z_bridge_kernel, dim3(sgrid), dim3(MC_BLOCK), 0, st, z);
  rc = mc_last_launch();
  if (rc != MC_OK) return rc;
  hipLaunchKernelGGL(layout_kernel, dim3((unsigned)nframes), dim3(MC_BLOCK), 0, st, a);
  rc = mc_last_launch();
  if (rc != MC_OK) return rc;
  hipLaunchKernelGGL(gather_kernel, dim3((unsigned)nstreams), dim3(MC_BLOCK), 0, st, a);
  return mc_last_launch();
}

}  // extern "C"
