// mc_blosc_dec_z.hip -- Blosc1 frames compressed with lz4 / lz4hc, zlib or zstd
// (and memcpyed frames), mixed in one batch -> still-filtered block bytes on
// the device: one plan launch plus one decode launch per format present.
// The container rules and the plan walker are mc_lz4.h's, what a zstd / zlib
// stream must satisfy inside Blosc is mc_blosc_z.h's (both compiled for the
// host too, tests/native_blosc_z); the wave-wide decoders are the stand-alone
// codecs' own: decode_wave (mc_lz4_wave.h), the Zstandard bit window, builder
// and sink (mc_zstd_wave.h), the inflater's (mc_inflate_wave.h).  The inverse
// shuffle is mc_blosc_filter's job.
//
// plan:   one thread per Blosc block of the batch: mc_blosc_plan_block's
//         descriptors, each with its frame's format above the MC_LZ4_S_* bits.
// decode: per format one launch of one wave (a 64-lane workgroup) per stream
//         over the shared descriptor list; a wave whose stream belongs to
//         another format leaves at once.  A stored stream is a wave-wide copy.
//   lz4   mc_blosc_dec.hip's decode.
//   zstd  every lane opens the frame header alike (mc_zstd_open), then
//         mc_zstd_blocks as in mc_zstd.hip with the stream's share as the
//         capacity; the literals of a block go to the stream's part of the
//         literals area (min(share, 128 KiB) bytes at the stream's offset in
//         its frame).  Then the share, and XXH64 of the output (behind a
//         workgroup-scope release / acquire) against a content checksum.
//   zlib  the container header, mc_inf_blocks as in mc_inflate.hip, the
//         share, and Adler-32 of the output (a slice per lane, combined by
//         Adler's closed form) against the trailer.
// LDS per workgroup: lz4 the ring (<= 64 KiB); zstd the ring (<= 64 KiB) +
// 11.3 KiB of tables; zlib the ring (<= 32 KiB) + 3.7 KiB of tables.
#include "mc_common.h"
#include "mc_checksum.h"
#include "mc_blosc_z.h"
#include "mc_lz4_wave.h"
#include "mc_zstd_wave.h"
#include "mc_inflate_wave.h"

namespace {

using namespace mc_lz4w;

__global__ void __launch_bounds__(MC_BLOCK)
plan_z_kernel(const uint8_t *__restrict__ frames, const mc_blosc_zframe *__restrict__ table, uint32_t nframes,
              uint32_t nblocks_total, mc_lz4_stream *__restrict__ streams, uint32_t nstreams_total,
              uint64_t lit_bytes, int32_t *__restrict__ err) {
  const uint32_t b = blockIdx.x * MC_BLOCK + threadIdx.x;
  if (b >= nblocks_total) return;
  // the frame whose [block_base, next block_base) holds b
  uint32_t lo = 0, hi = nframes - 1;
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1) >> 1;
    if (table[mid].f.block_base <= b) lo = mid; else hi = mid - 1;
  }
  const mc_blosc_zframe r = table[lo];
  const uint32_t fmt = mc_blosc_format(r.f.flags);
  const int shift = fmt == MC_BLOSC_FMT_LZ4 ? 0 : MC_BLOSC_Z_CONTAINER;
  // a format no launch decodes, or literals outside their area: no descriptor at all
  if (!mc_blosc_format_known(fmt) ||
      (fmt == MC_BLOSC_FMT_ZSTD && (r.lit_off > lit_bytes || lit_bytes - r.lit_off < r.f.nbytes))) {
    record_error(err, lo, shift + MC_LZ4_E_TABLE, 0);
    return;
  }
  uint32_t bad = 0;
  const uint32_t block = b - r.f.block_base;
  const int e = mc_blosc_plan_block(frames, r.f, lo, block, streams, nstreams_total, &bad);
  if (e != MC_LZ4_OK) {
    record_error(err, lo, shift + e, bad);
    return;  // (its descriptors are invalid)
  }
  const uint32_t nsplit = mc_blosc_nsplit(r.f.flags, r.f.typesize, r.f.blocksize,
                                          mc_blosc_block_size(r.f.nbytes, r.f.blocksize, block));
  mc_lz4_stream *out = streams + r.f.stream_base + mc_blosc_block_stream0(r.f.flags, r.f.typesize, r.f.blocksize, block);
  for (uint32_t j = 0; j < nsplit; ++j) out[j].flags |= fmt << MC_BLOSC_S_FORMAT_SHIFT;
}

// this launch's stream, or false: not valid, or another format's
MC_DEV bool mine(const mc_lz4_stream &d, uint32_t fmt) {
  return (d.flags & MC_LZ4_S_VALID) && (d.flags >> MC_BLOSC_S_FORMAT_SHIFT) == fmt;
}

MC_DEV void copy_raw(const uint8_t *src, uint8_t *dst, uint32_t usize, uint32_t lane) {  // cbytes == usize (plan)
  for (uint32_t k = lane; k < usize; k += WAVE) dst[k] = src[k];
}

__global__ void __launch_bounds__(WAVE)
lz4_stream_kernel(const uint8_t *__restrict__ frames, const mc_lz4_stream *__restrict__ streams, uint32_t nstreams,
                  uint32_t ring_mask, int32_t *__restrict__ err) {
  extern __shared__ __attribute__((aligned(16))) uint8_t ring[];
  blosc_lz4_stream(frames, streams, nstreams, MC_BLOSC_FMT_LZ4, ring, ring_mask, err);  // mc_blosc_dec.hip's decode
}

__global__ void __launch_bounds__(WAVE)
zstd_stream_kernel(const uint8_t *__restrict__ frames, const mc_blosc_zframe *__restrict__ table,
                   const mc_lz4_stream *__restrict__ streams, uint32_t nstreams, uint32_t ring_mask,
                   uint8_t *__restrict__ lits, int32_t *__restrict__ err) {
  extern __shared__ __attribute__((aligned(16))) uint8_t ring[];
  __shared__ mc_zstd_tables T;
  const uint32_t sidx = blockIdx.x, lane = threadIdx.x;
  if (sidx >= nstreams) return;
  const mc_lz4_stream d = streams[sidx];
  if (!mine(d, MC_BLOSC_FMT_ZSTD)) return;
  const uint8_t *src = mc_uniform_ptr(frames + d.src_off);
  uint8_t *dst = mc_uniform_ptr(reinterpret_cast<uint8_t *>((uintptr_t)d.dst));
  const uint32_t n = uni(d.cbytes), usize = uni(d.usize);
  if (d.flags & MC_LZ4_S_RAW) return copy_raw(src, dst, usize, lane);
  // the stream's literals: at its own offset in the frame's nbytes of the area (the plan checked the frame's)
  const mc_blosc_zframe r = table[d.frame];
  uint8_t *lit = mc_uniform_ptr(lits + r.lit_off + (d.dst - r.f.dst));
  mc_zstdw::wave_bits bits{src, n, lane, -0x10000000, 0u, 0u};
  mc_blosc_zstd_sink<mc_zstdw::wave_sink<true>> out{{src, n, dst, lit, ring, ring_mask, usize, 0u, lane},
                                                     mc_blosc_z_lit_cap(usize)};
  mc_zstdw::wave_builder bld{lane};
  auto hash = [&](uint32_t np) {
    mc_zstdw::wg_release_acquire();  // the lanes read what other lanes wrote
    return mc_zstdw::wave_xxh64(dst, np, lane);
  };
  const int e = (int)uni((uint32_t)mc_blosc_zstd_stream(bits, out, bld, src, n, usize, &T, hash));
  if (e != MC_ZSTD_OK && lane == 0) record_error(err, d.frame, e, sidx);
}

// Adler-32 of out[0, np) by the wave: a = 1 + sum d_j, b = np + sum (np - j) d_j;
// lane t's slice [lo, hi) gives sum d_j and sum (hi - j) d_j (mc_inflate.hip's check, over 64 slices)
MC_DEV uint32_t wave_adler32(const uint8_t *out, uint32_t np, uint32_t lane) {
  const uint32_t per = ((np + WAVE - 1) / WAVE + 3u) & ~3u;  // np < 2^30
  const uint32_t lo = lane * per < np ? lane * per : np, hi = np - lo < per ? np : lo + per;
  uint64_t s1 = 0;
  uint32_t s0 = 0;
  for (uint32_t j = lo; j < hi; j += 4) {
    uint32_t v = 0;
    if (hi - j >= 4u) __builtin_memcpy(&v, out + j, 4);
    else for (uint32_t k = 0; k < hi - j; ++k) v |= (uint32_t)out[j + k] << (8u * k);
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
      const uint32_t b = (v >> (8u * k)) & 0xffu;
      s0 += b;
      s1 += (uint64_t)b * (hi - j - k);  // a byte past hi is zero: its (wrapped) weight does not count
    }
  }
  uint32_t a = s0 % mcck::ADLER_P;
  uint32_t b = (uint32_t)((s1 % mcck::ADLER_P + (uint64_t)((np - hi) % mcck::ADLER_P) * a) % mcck::ADLER_P);
#pragma unroll
  for (uint32_t d = 1; d < WAVE; d <<= 1) {  // sums below 64 * 65521
    a += (uint32_t)__shfl_xor((int)a, (int)d, WAVE);
    b += (uint32_t)__shfl_xor((int)b, (int)d, WAVE);
  }
  return (((np % mcck::ADLER_P + b) % mcck::ADLER_P) << 16) | ((1u + a) % mcck::ADLER_P);
}

__global__ void __launch_bounds__(WAVE)
zlib_stream_kernel(const uint8_t *__restrict__ frames, const mc_lz4_stream *__restrict__ streams, uint32_t nstreams,
                   uint32_t ring_mask, int32_t *__restrict__ err) {
  extern __shared__ __attribute__((aligned(16))) uint8_t ring[];
  __shared__ mc_inf_tables T;
  const uint32_t sidx = blockIdx.x, lane = threadIdx.x;
  if (sidx >= nstreams) return;
  const mc_lz4_stream d = streams[sidx];
  if (!mine(d, MC_BLOSC_FMT_ZLIB)) return;
  const uint8_t *src = mc_uniform_ptr(frames + d.src_off);
  uint8_t *dst = mc_uniform_ptr(reinterpret_cast<uint8_t *>((uintptr_t)d.dst));
  const uint32_t n = uni(d.cbytes), usize = uni(d.usize);
  if (d.flags & MC_LZ4_S_RAW) return copy_raw(src, dst, usize, lane);
  uint32_t data_off;
  int e = (int)uni((uint32_t)mc_blosc_zlib_open(src, n, usize, &data_off));
  if (e == MC_INF_OK) {
    data_off = uni(data_off);  // <= n: the parser's
    mc_infw::wave_dwords win{src, n, lane, 0u, 0u, 0u};
    win.start(data_off >> 2);
    mc_inf_bits<mc_infw::wave_dwords> br(win, n);
    br.seek(data_off);
    mc_infw::wave_sink<true> out{src, dst, ring, ring_mask, usize, 0u, lane, 0u, 0u};
    mc_infw::wave_builder bld{lane};
    e = (int)uni((uint32_t)mc_inf_blocks(br, out, bld, &T));
    out.flush();
    auto adler = [&](uint32_t np) {
      mc_zstdw::wg_release_acquire();  // the lanes read what other lanes wrote
      return wave_adler32(dst, np, lane);
    };
    e = (int)uni((uint32_t)mc_blosc_zlib_finish(e, br, out.op, usize, src, n, adler));
  }
  if (e != MC_INF_OK && lane == 0) record_error(err, d.frame, e, sidx);
}

constexpr size_t WS_ALIGN = 16;
size_t streams_bytes(size_t nstreams) { return (nstreams * sizeof(mc_lz4_stream) + WS_ALIGN - 1) / WS_ALIGN * WS_ALIGN; }

}  // namespace

static_assert(sizeof(mc_blosc_zframe) == 56 && sizeof(mc_lz4_stream) == 32, "record layout (include/mcodec.h)");
static_assert(sizeof(mc_zstd_tables) + 65536 <= 80 * 1024, "two zstd workgroups share a CU's LDS");
static_assert(sizeof(mc_inf_tables) + 32768 <= 40 * 1024, "four inflate workgroups share a CU's LDS");

extern "C" {

size_t mc_blosc_decode_batch_z_workspace(size_t nstreams, size_t lit_bytes) {
  return streams_bytes(nstreams) + lit_bytes + 16;
}

int mc_blosc_decode_batch_z(const void *frames, const void *frame_table, size_t nframes, size_t nblocks,
                            size_t nstreams, size_t max_lz4, size_t max_zlib, size_t max_zstd, size_t lit_bytes,
                            void *workspace, size_t workspace_bytes, int32_t *err, mc_stream_t stream) {
  if (nframes == 0 || nblocks == 0) return MC_OK;
  if (!frames || !frame_table || !workspace || !err) return MC_EINVAL;
  if (nframes > 0x7fffffffu || nblocks > 0x7fffffffu || nstreams > 0x7fffffffu || nstreams < nblocks)
    return MC_EINVAL;
  if (max_lz4 >= MC_LZ4_MAX_USIZE || max_zlib >= MC_LZ4_MAX_USIZE || max_zstd >= MC_LZ4_MAX_USIZE) return MC_EINVAL;
  if (max_lz4 == 0 && max_zlib == 0 && max_zstd == 0) return MC_EINVAL;
  if (((uintptr_t)workspace & 7) || ((uintptr_t)frame_table & 7)) return MC_EINVAL;
  if (lit_bytes > ((size_t)1 << 40) || workspace_bytes < mc_blosc_decode_batch_z_workspace(nstreams, lit_bytes))
    return MC_ENOSPC;
  hipStream_t st = (hipStream_t)stream;
  int rc = mc_hip_status(hipMemsetAsync(err, 0, nframes * 2 * sizeof(int32_t), st));
  if (rc != MC_OK) return rc;
  // a descriptor the plan does not write stays invalid (flags 0) and is skipped
  rc = mc_hip_status(hipMemsetAsync(workspace, 0, nstreams * sizeof(mc_lz4_stream), st));
  if (rc != MC_OK) return rc;
  const uint8_t *fr = static_cast<const uint8_t *>(frames);
  const mc_blosc_zframe *table = static_cast<const mc_blosc_zframe *>(frame_table);
  mc_lz4_stream *streams = static_cast<mc_lz4_stream *>(workspace);
  uint8_t *lits = static_cast<uint8_t *>(workspace) + streams_bytes(nstreams);
  const unsigned pgrid = (unsigned)((nblocks + MC_BLOCK - 1) / MC_BLOCK);
  hipLaunchKernelGGL(plan_z_kernel, dim3(pgrid), dim3(MC_BLOCK), 0, st, fr, table, (uint32_t)nframes,
                     (uint32_t)nblocks, streams, (uint32_t)nstreams, (uint64_t)lit_bytes, err);
  rc = mc_last_launch();
  if (rc != MC_OK) return rc;
  const dim3 grid((unsigned)nstreams), wave(WAVE);
  if (max_lz4) {
    const uint32_t rb = ring_bytes(max_lz4);
    hipLaunchKernelGGL(lz4_stream_kernel, grid, wave, rb, st, fr, streams, (uint32_t)nstreams, rb - 1, err);
    rc = mc_last_launch();
    if (rc != MC_OK) return rc;
  }
  if (max_zlib) {
    // the history ring: DEFLATE reaches back 32768 bytes at most, and never past the output's start
    const uint32_t rb = ring_bytes(max_zlib < 32768 ? max_zlib : 32768);
    hipLaunchKernelGGL(zlib_stream_kernel, grid, wave, rb, st, fr, streams, (uint32_t)nstreams, rb - 1, err);
    rc = mc_last_launch();
    if (rc != MC_OK) return rc;
  }
  if (max_zstd) {
    // the history ring: what it does not hold a match reads from the output itself
    const uint32_t rb = ring_bytes(max_zstd < 65536 ? max_zstd : 65536);
    // (the ring and the tables together pass the 64 KiB a kernel may use unasked)
    rc = mc_hip_status(hipFuncSetAttribute(reinterpret_cast<const void *>(&zstd_stream_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)rb));
    if (rc != MC_OK) return rc;
    hipLaunchKernelGGL(zstd_stream_kernel, grid, wave, rb, st, fr, table, streams, (uint32_t)nstreams, rb - 1, lits,
                       err);
    rc = mc_last_launch();
    if (rc != MC_OK) return rc;
  }
  return MC_OK;
}

}  // extern "C"
