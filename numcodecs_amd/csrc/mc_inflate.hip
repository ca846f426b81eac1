// mc_inflate.hip -- zlib and gzip frames inflated on the device, a whole batch
// per call.  The rules (container parsers, bit reader, table checks, block
// walker, trailer classification) are mc_inflate.h's, compiled for the host
// too (tests/native_inflate): the kernels run that very code and supply only
// what is wave-wide here -- the source window, the table builder, the sink.
//
// plan:    one thread per frame: the container header -> a stream record
//          (first DEFLATE byte, length, destination, capacity, container) and
//          any header error.
// inflate: one wave (a 64-lane workgroup) per frame, wave-uniform control
//          flow.  The bit buffer is 64 bits, refilled a dword at a time from a
//          window of 64 dwords held one per lane (the next window is loaded
//          ahead), so the serial chain reads a lane's register, not memory.
//          The tables of a block are built in LDS by the wave: the counts and
//          the canonical symbol order by ballots over 64 symbols a pass, the
//          primary lookup (10 bits literal/length, 8 bits distance) with the
//          lanes over its entries; longer codes take the canonical walk.  The
//          fixed tables are built the same way from the fixed lengths.
//          Literals are gathered one per lane and flushed as one store to the
//          history ring and to global memory before a match, at a block's end
//          or when 64 are there.  Matches copy through the ring of
//          ring_bytes(min(capacity, 32768)) bytes in the two forms of
//          mc_lz4_wave.h's decode_wave, restated here (the LZ4 decoders stay
//          as they are): 64 bytes a step for distance >= 64, the replicating
//          form below it.  Stored blocks are wave-wide copies.
//          STORE = false is the sizing pass: the same chain with no ring and
//          no stores, only the byte count.
//          One frame is one serial chain: throughput comes from the batch.
// check:   one workgroup per frame, after the decode: Adler-32 (zlib) or
//          CRC-32 (gzip) of what was produced -- a slice per thread, combined
//          by Adler's closed form / by powers of x (mcck::gf_mul, xpow_tab) --
//          against the trailer at the byte the decode stopped at, ISIZE, and
//          what follows a gzip trailer.  A frame that carries an error is
//          skipped.
// LDS per inflate workgroup: the ring (<= 32 KiB) + 3.7 KiB of tables.
#include "mc_common.h"
#include "mc_checksum.h"
#include "mc_inflate.h"
#include "mc_lz4_wave.h"
#include "mc_inflate_wave.h"  // wave_dwords, wave_builder, wave_sink: shared with mc_blosc_dec_z.hip

namespace {

using namespace mc_infw;

__global__ void __launch_bounds__(MC_BLOCK)
inflate_plan_kernel(const uint8_t *__restrict__ frames, const mc_inf_frame *__restrict__ table, uint32_t nframes,
                    uint32_t sizing, mc_inf_stream *__restrict__ streams, uint32_t *__restrict__ produced,
                    uint32_t *__restrict__ endpos, int32_t *__restrict__ err) {
  const uint32_t i = blockIdx.x * MC_BLOCK + threadIdx.x;
  if (i >= nframes) return;
  const mc_inf_frame r = table[i];
  mc_inf_stream s;
  s.src_off = r.src_off, s.dst = r.dst, s.src_len = 0, s.data_off = 0, s.capacity = r.capacity;
  s.flags = r.container << 8;
  int e;
  uint32_t empty = 0;
  if (r.src_len >= MC_INF_MAX_BYTES || r.capacity >= MC_INF_MAX_BYTES || r.container > MC_INF_GZIP ||
      (!sizing && r.capacity && !r.dst)) {
    e = MC_INF_E_TABLE;
  } else {
    s.src_len = (uint32_t)r.src_len;
    e = mc_inf_parse_header(frames + r.src_off, r.src_len, r.container, &s.data_off, &empty);
  }
  if (e == MC_INF_OK) s.flags |= empty ? MC_INF_S_EMPTY : MC_INF_S_VALID;
  streams[i] = s;
  produced[i] = 0;
  endpos[i] = 0;
  if (e != MC_INF_OK) err[2 * i] = e, err[2 * i + 1] = 0;
}

template <bool STORE>
__global__ void __launch_bounds__(WAVE)
inflate_kernel(const uint8_t *__restrict__ frames, const mc_inf_stream *__restrict__ streams, uint32_t nframes,
               uint32_t ring_mask, uint32_t *__restrict__ produced, uint32_t *__restrict__ endpos,
               int32_t *__restrict__ err) {
  extern __shared__ __attribute__((aligned(16))) uint8_t ring[];
  __shared__ mc_inf_tables T;
  const uint32_t i = blockIdx.x, lane = threadIdx.x;
  if (i >= nframes) return;
  const mc_inf_stream d = streams[i];
  if (!(d.flags & MC_INF_S_VALID)) return;
  const uint8_t *f = mc_uniform_ptr(frames + d.src_off);
  const uint32_t n = uni(d.src_len), data_off = uni(d.data_off);  // data_off <= n: the parser's
  wave_dwords src{f, n, lane, 0u, 0u, 0u};
  src.start(data_off >> 2);
  mc_inf_bits<wave_dwords> br(src, n);
  br.seek(data_off);
  wave_sink<STORE> out{f, mc_uniform_ptr(reinterpret_cast<uint8_t *>((uintptr_t)d.dst)), ring, ring_mask,
                       STORE ? uni(d.capacity) : MC_INF_MAX_BYTES - 1u, 0u, lane, 0u, 0u};
  wave_builder bld{lane};
  const int e = (int)uni((uint32_t)mc_inf_blocks(br, out, bld, &T));
  out.flush();
  br.align();
  const uint32_t pos = br.bytepos();
  if (lane == 0) {  // one wave per frame: no other writer
    produced[i] = out.op;
    endpos[i] = pos;
    if (e != MC_INF_OK) err[2 * i] = e, err[2 * i + 1] = (int32_t)out.op;
  }
}

__global__ void __launch_bounds__(MC_BLOCK)
inflate_check_kernel(const uint8_t *__restrict__ frames, const mc_inf_stream *__restrict__ streams, uint32_t nframes,
                     const uint32_t *__restrict__ produced, const uint32_t *__restrict__ endpos,
                     int32_t *__restrict__ err) {
  __shared__ uint32_t tab[256];
  __shared__ uint32_t part[2][MC_BLOCK];
  __shared__ uint32_t first_nonzero, go;
  const uint32_t i = blockIdx.x, t = threadIdx.x;
  if (i >= nframes) return;
  const mc_inf_stream d = streams[i];
  if (!(d.flags & MC_INF_S_VALID) || err[2 * i] != 0) return;  // the same for every thread
  const uint32_t container = d.flags >> 8, np = produced[i], n = d.src_len;
  const uint8_t *f = frames + d.src_off;
  const uint8_t *out = reinterpret_cast<const uint8_t *>((uintptr_t)d.dst);  // np <= capacity bytes
  // thread t's slice [lo, hi) of the np bytes, a multiple of 4 long but for the last
  const uint32_t per = ((np + MC_BLOCK - 1) / MC_BLOCK + 3u) & ~3u;
  const uint32_t lo = t * per < np ? t * per : np, hi = np - lo < per ? np : lo + per;
  if (container == MC_INF_GZIP) {
    uint32_t r = t;
#pragma unroll
    for (int k = 0; k < 8; ++k) r = (r >> 1) ^ ((r & 1u) ? mcck::POLY_CRC32 : 0u);
    tab[t] = r;
  }
  if (t == 0) first_nonzero = n, go = 0;
  __syncthreads();
  if (container == MC_INF_ZLIB) {
    // a = 1 + sum d_j, b = np + sum (np - j) d_j; the slice gives sum (hi - j) d_j and sum d_j
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
    const uint32_t a = s0 % mcck::ADLER_P;
    part[0][t] = a;
    part[1][t] = (uint32_t)((s1 % mcck::ADLER_P + (uint64_t)((np - hi) % mcck::ADLER_P) * a) % mcck::ADLER_P);
  } else {
    uint32_t c = 0;  // raw(0, slice)
    for (uint32_t j = lo; j < hi; j += 4) {
      uint32_t v = 0;
      const uint32_t m = hi - j >= 4u ? 4u : hi - j;
      if (m == 4u) __builtin_memcpy(&v, out + j, 4);
      else for (uint32_t k = 0; k < m; ++k) v |= (uint32_t)out[j + k] << (8u * k);
      for (uint32_t k = 0; k < m; ++k) c = tab[(c ^ (v >> (8u * k))) & 0xffu] ^ (c >> 8);
    }
    // moved to the end of the data: times x^(8 * bytes behind the slice)
    part[0][t] = hi > lo ? mcck::gf_mul(c, mcck::xpow_tab(mcck::kCrc32.x2n, 8ull * (np - hi), mcck::POLY_CRC32),
                                        mcck::POLY_CRC32)
                         : 0u;
  }
  __syncthreads();
  if (t == 0) {
    uint32_t check;
    if (container == MC_INF_ZLIB) {
      uint64_t a = 1, b = np % mcck::ADLER_P;
      for (uint32_t k = 0; k < MC_BLOCK; ++k) a += part[0][k], b += part[1][k];
      check = (uint32_t)((b % mcck::ADLER_P) << 16) | (uint32_t)(a % mcck::ADLER_P);
    } else {
      uint32_t r = 0;
      for (uint32_t k = 0; k < MC_BLOCK; ++k) r ^= part[0][k];
      // crc(D) = ~(0xffffffff * x^(8n) ^ raw(0, D))
      check = ~(mcck::gf_mul(0xffffffffu, mcck::xpow_tab(mcck::kCrc32.x2n, 8ull * np, mcck::POLY_CRC32),
                             mcck::POLY_CRC32) ^ r);
    }
    uint64_t after;
    const int e = mc_inf_check_trailer(f, n, endpos[i], container, check, np, &after);
    if (e != MC_INF_OK) err[2 * i] = e, err[2 * i + 1] = (int32_t)(e == MC_INF_E_CHECK ? check : np);
    else if (container == MC_INF_GZIP) go = 1, part[0][0] = (uint32_t)after;
  }
  __syncthreads();
  if (!go) return;
  // what follows the gzip trailer: the first byte that is not zero
  const uint32_t after = part[0][0];
  for (uint32_t q = after + t; q < n; q += MC_BLOCK) {
    if (f[q] != 0) {
      atomicMin(&first_nonzero, q);
      break;
    }
  }
  __syncthreads();
  if (t == 0) {
    const int e = mc_inf_after_trailer(f, n, first_nonzero);
    if (e != MC_INF_OK) err[2 * i] = e, err[2 * i + 1] = (int32_t)np;
  }
}

constexpr size_t WS_ALIGN = 16;
size_t streams_bytes(size_t nframes) { return (nframes * sizeof(mc_inf_stream) + WS_ALIGN - 1) / WS_ALIGN * WS_ALIGN; }

int check_args(const void *frames, const void *table, size_t nframes, const void *ws, size_t ws_bytes, const void *out,
               const void *err) {
  if (!frames || !table || !ws || !out || !err) return MC_EINVAL;
  if (nframes > 0x7fffffffu) return MC_EINVAL;
  if (((uintptr_t)ws & 7) || ((uintptr_t)table & 7) || ((uintptr_t)err & 3) || ((uintptr_t)out & 3)) return MC_EINVAL;
  if (ws_bytes < mc_inflate_workspace(nframes)) return MC_ENOSPC;
  return MC_OK;
}

}  // namespace

static_assert(sizeof(mc_inf_frame) == 32 && sizeof(mc_inf_stream) == 32, "record layout (include/mcodec.h)");
static_assert(sizeof(mc_inf_tables) + 32768 <= 40 * 1024, "four inflate workgroups share a CU's LDS");

extern "C" {

size_t mc_inflate_workspace(size_t nframes) { return streams_bytes(nframes) + nframes * sizeof(uint32_t) + 16; }

int mc_inflate_size_batch(const void *frames, const void *frame_table, size_t nframes, void *workspace,
                          size_t workspace_bytes, uint32_t *sizes, int32_t *err, mc_stream_t stream) {
  if (nframes == 0) return MC_OK;
  int rc = check_args(frames, frame_table, nframes, workspace, workspace_bytes, sizes, err);
  if (rc != MC_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  rc = mc_hip_status(hipMemsetAsync(err, 0, nframes * 2 * sizeof(int32_t), st));
  if (rc != MC_OK) return rc;
  const uint8_t *fr = static_cast<const uint8_t *>(frames);
  mc_inf_stream *streams = static_cast<mc_inf_stream *>(workspace);
  uint32_t *endpos = reinterpret_cast<uint32_t *>(static_cast<uint8_t *>(workspace) + streams_bytes(nframes));
  const unsigned pgrid = (unsigned)((nframes + MC_BLOCK - 1) / MC_BLOCK);
  hipLaunchKernelGGL(inflate_plan_kernel, dim3(pgrid), dim3(MC_BLOCK), 0, st, fr,
                     static_cast<const mc_inf_frame *>(frame_table), (uint32_t)nframes, 1u, streams, sizes, endpos, err);
  rc = mc_last_launch();
  if (rc != MC_OK) return rc;
  hipLaunchKernelGGL(inflate_kernel<false>, dim3((unsigned)nframes), dim3(WAVE), 16, st, fr, streams,
                     (uint32_t)nframes, 0u, sizes, endpos, err);
  return mc_last_launch();
}

int mc_inflate_decode_batch(const void *frames, const void *frame_table, size_t nframes, size_t max_capacity,
                            void *workspace, size_t workspace_bytes, uint32_t *produced, int32_t *err,
                            mc_stream_t stream) {
  if (nframes == 0) return MC_OK;
  int rc = check_args(frames, frame_table, nframes, workspace, workspace_bytes, produced, err);
  if (rc != MC_OK) return rc;
  if (max_capacity >= MC_INF_MAX_BYTES) return MC_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  rc = mc_hip_status(hipMemsetAsync(err, 0, nframes * 2 * sizeof(int32_t), st));
  if (rc != MC_OK) return rc;
  const uint8_t *fr = static_cast<const uint8_t *>(frames);
  mc_inf_stream *streams = static_cast<mc_inf_stream *>(workspace);
  uint32_t *endpos = reinterpret_cast<uint32_t *>(static_cast<uint8_t *>(workspace) + streams_bytes(nframes));
  const unsigned pgrid = (unsigned)((nframes + MC_BLOCK - 1) / MC_BLOCK);
  hipLaunchKernelGGL(inflate_plan_kernel, dim3(pgrid), dim3(MC_BLOCK), 0, st, fr,
                     static_cast<const mc_inf_frame *>(frame_table), (uint32_t)nframes, 0u, streams, produced, endpos,
                     err);
  rc = mc_last_launch();
  if (rc != MC_OK) return rc;
  // the history ring: DEFLATE reaches back 32768 bytes at most, and never past the output's start
  const uint32_t rb = ring_bytes(max_capacity < 32768 ? max_capacity : 32768);
  hipLaunchKernelGGL(inflate_kernel<true>, dim3((unsigned)nframes), dim3(WAVE), rb, st, fr, streams,
                     (uint32_t)nframes, rb - 1, produced, endpos, err);
  rc = mc_last_launch();
  if (rc != MC_OK) return rc;
  hipLaunchKernelGGL(inflate_check_kernel, dim3((unsigned)nframes), dim3(MC_BLOCK), 0, st, fr, streams,
                     (uint32_t)nframes, produced, endpos, err);
  return mc_last_launch();
}

}  // extern "C"
