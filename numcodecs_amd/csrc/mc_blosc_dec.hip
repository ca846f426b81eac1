// mc_blosc_dec.hip -- Blosc1 frames (LZ4 / stored) -> still-filtered block
// bytes on the device, for a whole batch of frames: one plan launch plus one
// decode launch.  The frame and LZ4 rules, the sequence parser, the validity
// predicate and the plan walker live in mc_lz4.h (compiled for the host too,
// tests/native_lz4); the wave-wide sequence loop (decode_wave) is
// mc_lz4_wave.h's.  The inverse shuffle is mc_blosc_filter's job.
//
// plan:   one thread per Blosc block of the batch; writes one mc_lz4_stream
//         descriptor per stream, everything validated against the frame length.
// decode: one wave (a 64-lane workgroup) per stream, wave-uniform control
//         flow.  The sequence header is parsed once per wave out of a 64-byte
//         source window (one coalesced load, the next window loaded ahead,
//         bytes picked with v_readlane); the lanes then copy literals and
//         matches 64 bytes a step.  The stream's history lives in an LDS ring of min(pow2 >= stream, 64 KiB)
//         bytes: matches are served from the ring (LZ4 offsets are <= 65535),
//         never from global memory, and every produced byte is also streamed
//         to global memory.  Each step's LDS reads are complete before its LDS
//         writes issue (the written value is the read one), and lds_order()
//         -- s_waitcnt lgkmcnt(0) behind a compiler memory barrier; the LDS
//         runs one wave's instructions in issue order -- orders the writes
//         before the next step's reads.
//         A match with offset < 64 is copied in the replicating form (lane i
//         reads start + i % offset): it only reads bytes that existed before
//         the match began.
#include "mc_common.h"
#include "mc_lz4.h"
#include "mc_lz4_wave.h"  // decode_wave: the sequence loop, shared with mc_lz4_codec.hip

namespace {

using namespace mc_lz4w;

__global__ void __launch_bounds__(MC_BLOCK)
plan_kernel(const uint8_t *__restrict__ frames, const mc_blosc_frame *__restrict__ table, uint32_t nframes,
            uint32_t nblocks_total, mc_lz4_stream *__restrict__ streams, uint32_t nstreams_total,
            int32_t *__restrict__ err) {
  const uint32_t b = blockIdx.x * MC_BLOCK + threadIdx.x;
  if (b >= nblocks_total) return;
  // the frame whose [block_base, next block_base) holds b
  uint32_t lo = 0, hi = nframes - 1;
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1) >> 1;
    if (table[mid].block_base <= b) lo = mid; else hi = mid - 1;
  }
  const mc_blosc_frame f = table[lo];
  uint32_t bad = 0;
  const int e = mc_blosc_plan_block(frames, f, lo, b - f.block_base, streams, nstreams_total, &bad);
  if (e != MC_LZ4_OK) record_error(err, lo, e, bad);
}

__global__ void __launch_bounds__(WAVE)
decode_kernel(const uint8_t *__restrict__ frames, const mc_lz4_stream *__restrict__ streams, uint32_t nstreams,
              uint32_t ring_mask, int32_t *__restrict__ err) {
  extern __shared__ uint8_t ring[];
  blosc_lz4_stream(frames, streams, nstreams, 0u, ring, ring_mask, err);  // shared with mc_blosc_dec_z.hip
}

}  // namespace

extern "C" {

size_t mc_blosc_decode_workspace(size_t nstreams) { return nstreams * sizeof(mc_lz4_stream) + 16; }

int mc_blosc_decode_batch(const void *frames, const void *frame_table, size_t nframes, size_t nblocks,
                          size_t nstreams, size_t max_stream, void *workspace, size_t workspace_bytes,
                          int32_t *err, mc_stream_t stream) {
  if (nframes == 0 || nblocks == 0) return MC_OK;
  if (!frames || !frame_table || !workspace || !err) return MC_EINVAL;
  if (nframes > 0x7fffffffu || nblocks > 0x7fffffffu || nstreams > 0x7fffffffu || nstreams < nblocks)
    return MC_EINVAL;
  if (max_stream == 0 || max_stream >= MC_LZ4_MAX_USIZE) return MC_EINVAL;
  if (((uintptr_t)workspace & 7) || ((uintptr_t)frame_table & 7)) return MC_EINVAL;
  if (workspace_bytes < mc_blosc_decode_workspace(nstreams)) return MC_ENOSPC;
  hipStream_t st = (hipStream_t)stream;
  int rc = mc_hip_status(hipMemsetAsync(err, 0, nframes * 2 * sizeof(int32_t), st));
  if (rc != MC_OK) return rc;
  // a descriptor the plan does not write stays invalid (flags 0) and is skipped
  rc = mc_hip_status(hipMemsetAsync(workspace, 0, nstreams * sizeof(mc_lz4_stream), st));
  if (rc != MC_OK) return rc;
  const uint8_t *fr = static_cast<const uint8_t *>(frames);
  const mc_blosc_frame *table = static_cast<const mc_blosc_frame *>(frame_table);
  mc_lz4_stream *streams = static_cast<mc_lz4_stream *>(workspace);
  const unsigned pgrid = (unsigned)((nblocks + MC_BLOCK - 1) / MC_BLOCK);
  hipLaunchKernelGGL(plan_kernel, dim3(pgrid), dim3(MC_BLOCK), 0, st, fr, table, (uint32_t)nframes,
                     (uint32_t)nblocks, streams, (uint32_t)nstreams, err);
  rc = mc_last_launch();
  if (rc != MC_OK) return rc;
  const uint32_t rb = ring_bytes(max_stream);
  hipLaunchKernelGGL(decode_kernel, dim3((unsigned)nstreams), dim3(WAVE), rb, st, fr, streams,
                     (uint32_t)nstreams, rb - 1, err);
  return mc_last_launch();
}

}  // extern "C"
