// mc_zstd.hip -- Zstandard frames (RFC 8878) decoded on the device, a whole
// batch per call.  The rules (header parser, frame walk, bit readers, table
// descriptions, block walker, sequence chain) are mc_zstd.h's, compiled for the
// host too (tests/native_zstd): the kernels run that very code and supply only
// what is wave-wide here -- the bit window, the table builders, the literal
// streams, the sink.
//
// plan:    one thread per frame: the frame header and the walk over the block
//          headers -> a stream record (first block, Block_Maximum_Size, flags,
//          declared size, the frame's end) and every verdict that comes before
//          the blocks.
// decode:  one wave (a 64-lane workgroup) per frame, wave-uniform control
//          flow.  Per block:
//          tables    in LDS, by the wave.  FSE: the symbols "less than 1" and
//                    the running totals by ballots and a wave scan, the spread
//                    with the lanes over the steps (step j visits cell j * step,
//                    its symbol found by its rank among the cells not above the
//                    high threshold), the state numbers with the lanes over the
//                    cells, one ballot per distinct symbol of 64 cells.
//                    Huffman: the weights counted and the symbols put in order
//                    of weight by ballots, the lookup with the lanes over its
//                    entries.  Reading a count description and the FSE chain
//                    of the weights are serial by nature (mc_zstd.h) and run
//                    by every lane alike.  The tables stay in
//                    LDS from block to block (repeat mode, treeless literals).
//          literals  the four Huffman streams on four lanes at once, into the
//                    frame's 128 KiB of the workspace, 4 bytes a store; a
//                    workgroup-scope release / acquire pair before the
//                    sequences read them back.  Raw literals are read in place,
//                    RLE literals are a splat.
//          sequences the three-state chain wave-uniform: the backward bit
//                    buffer comes out of a window of 64 dwords held one per
//                    lane (the window below it is loaded ahead), two looks of
//                    64 bits per sequence.  Each sequence is executed wave-wide:
//                    the literal copy, then the match through the LDS history
//                    ring in the two forms of mc_lz4_wave.h's decode_wave; a
//                    match that reaches further back than the ring reads the
//                    frame's own output in global memory behind the same fence.
//          Raw and RLE blocks are wave-wide copies and splats through the ring.
//          STORE = false is the sizing pass: headers, Regenerated_Size and the
//          sequences' lengths only; no Huffman decode, no ring, no stores.
//          One frame is one serial chain: throughput comes from the batch.
// check:   one wave per frame, after the decode: the produced bytes against a
//          declared Frame_Content_Size, and XXH64 against the trailer: the
//          wave loads 512 bytes a step (the next step's ahead), four lanes
//          carry the four accumulators, lane 0 merges and finishes.  A frame
//          that carries an error is skipped.
// LDS per decode workgroup: the ring (<= 64 KiB) + 11.3 KiB of tables.
#include "mc_common.h"
#include "mc_zstd.h"
#include "mc_lz4_wave.h"
#include "mc_zstd_wave.h"  // wave_bits, wave_builder, wave_sink, wave_xxh64: shared with mc_blosc_dec_z.hip

namespace {

using namespace mc_zstdw;

__global__ void __launch_bounds__(MC_BLOCK)
zstd_plan_kernel(const uint8_t *__restrict__ frames, const mc_zstd_frame *__restrict__ table, uint32_t nframes,
                 uint32_t sizing, mc_zstd_stream *__restrict__ streams, uint32_t *__restrict__ produced,
                 int32_t *__restrict__ err) {
  const uint32_t i = blockIdx.x * MC_BLOCK + threadIdx.x;
  if (i >= nframes) return;
  const mc_zstd_frame r = table[i];
  mc_zstd_stream s;
  s.src_off = r.src_off, s.dst = r.dst, s.src_len = 0, s.data_off = 0, s.capacity = r.capacity, s.flags = 0;
  s.block_max = 0, s.content = 0, s.end_off = 0, s.pad = 0;
  int e;
  if (r.src_len >= MC_ZSTD_MAX_BYTES || r.capacity >= MC_ZSTD_MAX_BYTES || r.reserved != 0 ||
      (!sizing && r.capacity && !r.dst)) {
    e = MC_ZSTD_E_TABLE;
  } else {
    mc_zstd_header h;
    s.src_len = (uint32_t)r.src_len;
    e = mc_zstd_open(frames + r.src_off, r.src_len, &h, &s.end_off);
    s.data_off = h.data_off, s.block_max = h.block_max;
    if (h.checksum) s.flags |= MC_ZSTD_S_CHECKSUM;
    if (h.content != MC_ZSTD_UNKNOWN) {
      s.flags |= MC_ZSTD_S_SIZED;
      s.content = h.content < MC_ZSTD_MAX_BYTES ? (uint32_t)h.content : MC_ZSTD_MAX_BYTES;
    }
  }
  if (e == MC_ZSTD_OK) s.flags |= MC_ZSTD_S_VALID;
  streams[i] = s;
  produced[i] = 0;
  if (e != MC_ZSTD_OK) err[2 * i] = e, err[2 * i + 1] = 0;
}

template <bool STORE>
__global__ void __launch_bounds__(WAVE)
zstd_decode_kernel(const uint8_t *__restrict__ frames, const mc_zstd_stream *__restrict__ streams, uint32_t nframes,
                   uint32_t ring_mask, uint8_t *__restrict__ lits, uint32_t *__restrict__ produced,
                   int32_t *__restrict__ err) {
  extern __shared__ __attribute__((aligned(16))) uint8_t ring[];
  __shared__ mc_zstd_tables T;
  const uint32_t i = blockIdx.x, lane = threadIdx.x;
  if (i >= nframes) return;
  const mc_zstd_stream d = streams[i];
  if (!(d.flags & MC_ZSTD_S_VALID)) return;
  const uint8_t *f = mc_uniform_ptr(frames + d.src_off);
  const uint32_t n = uni(d.src_len);
  wave_bits src{f, n, lane, -0x10000000, 0u, 0u};
  wave_sink<STORE> out{f, n, mc_uniform_ptr(reinterpret_cast<uint8_t *>((uintptr_t)d.dst)),
                       STORE ? mc_uniform_ptr(lits + (size_t)i * MC_ZSTD_BLOCK_MAX) : nullptr, ring, ring_mask,
                       STORE ? uni(d.capacity) : MC_ZSTD_MAX_BYTES - 1u, 0u, lane};
  wave_builder bld{lane};
  const int e = (int)uni((uint32_t)mc_zstd_blocks(src, out, bld, f, n, uni(d.data_off), uni(d.block_max), &T));
  if (lane == 0) {  // one wave per frame: no other writer
    produced[i] = out.op;
    if (e != MC_ZSTD_OK) err[2 * i] = e, err[2 * i + 1] = (int32_t)out.op;
  }
}

__global__ void __launch_bounds__(WAVE)
zstd_check_kernel(const uint8_t *__restrict__ frames, const mc_zstd_stream *__restrict__ streams, uint32_t nframes,
                  const uint32_t *__restrict__ produced, int32_t *__restrict__ err) {
  const uint32_t i = blockIdx.x, lane = threadIdx.x;
  if (i >= nframes) return;
  const mc_zstd_stream d = streams[i];
  if (!(d.flags & MC_ZSTD_S_VALID) || err[2 * i] != 0) return;  // the same for every lane
  const uint32_t np = uni(produced[i]);
  const uint8_t *out = mc_uniform_ptr(reinterpret_cast<const uint8_t *>((uintptr_t)d.dst));  // np <= capacity bytes
  uint32_t check = 0;
  if (d.flags & MC_ZSTD_S_CHECKSUM) check = wave_xxh64(out, np, lane);
  if (lane == 0) {
    const int e = mc_zstd_check(frames + d.src_off, d.flags, d.content, d.end_off, np, check);
    if (e != MC_ZSTD_OK) err[2 * i] = e, err[2 * i + 1] = (int32_t)(e == MC_ZSTD_E_CHECK ? check : np);
  }
}

constexpr size_t WS_ALIGN = 16;
size_t streams_bytes(size_t nframes) { return (nframes * sizeof(mc_zstd_stream) + WS_ALIGN - 1) / WS_ALIGN * WS_ALIGN; }

int check_args(const void *frames, const void *table, size_t nframes, const void *ws, size_t ws_bytes, const void *out,
               const void *err) {
  if (!frames || !table || !ws || !out || !err) return MC_EINVAL;
  if (nframes > 0x7fffffffu) return MC_EINVAL;
  if (((uintptr_t)ws & 7) || ((uintptr_t)table & 7) || ((uintptr_t)err & 3) || ((uintptr_t)out & 3)) return MC_EINVAL;
  if (ws_bytes < mc_zstd_workspace(nframes)) return MC_ENOSPC;
  return MC_OK;
}

}  // namespace

static_assert(sizeof(mc_zstd_frame) == 32 && sizeof(mc_zstd_stream) == 48, "record layout (include/mcodec.h)");
static_assert(sizeof(mc_zstd_tables) + 65536 <= 80 * 1024, "two decode workgroups share a CU's LDS");

extern "C" {

size_t mc_zstd_workspace(size_t nframes) { return streams_bytes(nframes) + nframes * (size_t)MC_ZSTD_BLOCK_MAX + 16; }

int mc_zstd_size_batch(const void *frames, const void *frame_table, size_t nframes, void *workspace,
                       size_t workspace_bytes, uint32_t *sizes, int32_t *err, mc_stream_t stream) {
  if (nframes == 0) return MC_OK;
  int rc = check_args(frames, frame_table, nframes, workspace, workspace_bytes, sizes, err);
  if (rc != MC_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  rc = mc_hip_status(hipMemsetAsync(err, 0, nframes * 2 * sizeof(int32_t), st));
  if (rc != MC_OK) return rc;
  const uint8_t *fr = static_cast<const uint8_t *>(frames);
  mc_zstd_stream *streams = static_cast<mc_zstd_stream *>(workspace);
  const unsigned pgrid = (unsigned)((nframes + MC_BLOCK - 1) / MC_BLOCK);
  hipLaunchKernelGGL(zstd_plan_kernel, dim3(pgrid), dim3(MC_BLOCK), 0, st, fr,
                     static_cast<const mc_zstd_frame *>(frame_table), (uint32_t)nframes, 1u, streams, sizes, err);
  rc = mc_last_launch();
  if (rc != MC_OK) return rc;
  hipLaunchKernelGGL(zstd_decode_kernel<false>, dim3((unsigned)nframes), dim3(WAVE), 16, st, fr, streams,
                     (uint32_t)nframes, 0u, (uint8_t *)nullptr, sizes, err);
  return mc_last_launch();
}

int mc_zstd_decode_batch(const void *frames, const void *frame_table, size_t nframes, size_t max_capacity,
                         void *workspace, size_t workspace_bytes, uint32_t *produced, int32_t *err,
                         mc_stream_t stream) {
  if (nframes == 0) return MC_OK;
  int rc = check_args(frames, frame_table, nframes, workspace, workspace_bytes, produced, err);
  if (rc != MC_OK) return rc;
  if (max_capacity >= MC_ZSTD_MAX_BYTES) return MC_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  rc = mc_hip_status(hipMemsetAsync(err, 0, nframes * 2 * sizeof(int32_t), st));
  if (rc != MC_OK) return rc;
  const uint8_t *fr = static_cast<const uint8_t *>(frames);
  mc_zstd_stream *streams = static_cast<mc_zstd_stream *>(workspace);
  uint8_t *lits = static_cast<uint8_t *>(workspace) + streams_bytes(nframes);
  const unsigned pgrid = (unsigned)((nframes + MC_BLOCK - 1) / MC_BLOCK);
  hipLaunchKernelGGL(zstd_plan_kernel, dim3(pgrid), dim3(MC_BLOCK), 0, st, fr,
                     static_cast<const mc_zstd_frame *>(frame_table), (uint32_t)nframes, 0u, streams, produced, err);
  rc = mc_last_launch();
  if (rc != MC_OK) return rc;
  // the history ring: what it does not hold a match reads from the output itself
  const uint32_t rb = ring_bytes(max_capacity < 65536 ? max_capacity : 65536);
  // (the ring and the tables together pass the 64 KiB a kernel may use unasked)
  rc = mc_hip_status(hipFuncSetAttribute(reinterpret_cast<const void *>(&zstd_decode_kernel<true>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)rb));
  if (rc != MC_OK) return rc;
  hipLaunchKernelGGL(zstd_decode_kernel<true>, dim3((unsigned)nframes), dim3(WAVE), rb, st, fr, streams,
                     (uint32_t)nframes, rb - 1, lits, produced, err);
  rc = mc_last_launch();
  if (rc != MC_OK) return rc;
  hipLaunchKernelGGL(zstd_check_kernel, dim3((unsigned)nframes), dim3(WAVE), 0, st, fr, streams, (uint32_t)nframes,
                     produced, err);
  return mc_last_launch();
}

}  // extern "C"
