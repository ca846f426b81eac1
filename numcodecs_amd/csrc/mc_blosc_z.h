// mc_blosc_z.h -- Blosc1 frames whose streams are Zstandard frames (format
// bits 4) or zlib frames (format bits 3): what a stream must satisfy inside
// Blosc, shared by the gfx950 kernels (mc_blosc_dec_z.hip) and the host build
// of the CPU suite (tests/native_blosc_z).  The container is mc_lz4.h's (the
// plan walker is used as it is); a stream is decoded by mc_zstd.h's or
// mc_inflate.h's block walker with the stream's share of the block as its
// capacity, and the functions below add Blosc's own rule (c-blosc: nbytes !=
// neblock is an error): a stream produces exactly its share.
//
// Error codes of the frame's error record:
//   lz4 frames    mc_lz4_error, as mc_blosc_decode_batch reports them;
//   zstd frames   inside a stream mc_zstd_error (a declared Frame_Content_Size
//                 other than the share, or fewer bytes than the share:
//                 MC_ZSTD_E_SIZE; more: MC_ZSTD_E_CAPACITY);
//   zlib frames   inside a stream mc_inf_error (fewer bytes than the share:
//                 MC_INF_E_LENGTH; more: MC_INF_E_CAPACITY);
//   zstd and zlib frames report a violation of the container (bstarts, cbytes
//   words, the frame table: an mc_lz4_error) as MC_BLOSC_Z_CONTAINER + code,
//   so that the two enums do not collide.
#pragma once

#include "mc_inflate.h"
#include "mc_lz4.h"
#include "mc_zstd.h"

#define MC_BLOSC_FMT_LZ4 1u
#define MC_BLOSC_FMT_ZLIB 3u
#define MC_BLOSC_FMT_ZSTD 4u
#define MC_BLOSC_Z_CONTAINER 64
// a stream descriptor's flags carry its frame's format above the MC_LZ4_S_* bits
#define MC_BLOSC_S_FORMAT_SHIFT MC_LZ4_S_FORMAT_SHIFT

// One frame of a batch of mc_blosc_decode_batch_z (device table, one record
// per frame; include/mcodec.h): mc_blosc_decode_batch's record and the frame's
// place in the literals area.
struct mc_blosc_zframe {
  mc_blosc_frame f;
  uint64_t lit_off;  // zstd frames: the frame's nbytes bytes of the literals area (others: unused)
};

// the decoder of a frame's streams; a memcpyed frame is copied by the lz4 launch
MC_LZ4_HD uint32_t mc_blosc_format(uint32_t flags) {
  return (flags & MC_BLOSC_F_MEMCPYED) ? MC_BLOSC_FMT_LZ4 : flags >> 5;
}
MC_LZ4_HD bool mc_blosc_format_known(uint32_t fmt) {
  return fmt == MC_BLOSC_FMT_LZ4 || fmt == MC_BLOSC_FMT_ZLIB || fmt == MC_BLOSC_FMT_ZSTD;
}

// The literals buffer of a zstd stream of `usize` output bytes: every
// regenerated literal becomes an output byte, so a literals section above the
// stream's share cannot end well and is refused before it is decoded.
MC_LZ4_HD uint32_t mc_blosc_z_lit_cap(uint32_t usize) { return usize < MC_ZSTD_BLOCK_MAX ? usize : MC_ZSTD_BLOCK_MAX; }

// a zstd sink whose literals buffer holds lit_cap bytes only
template <class Base>
struct mc_blosc_zstd_sink : Base {
  uint32_t lit_cap;
  MC_ZSTD_HD int huffman(const mc_zstd_lit_streams &ls, const uint16_t *huf, uint32_t log) {
    const uint32_t regen = ls.nstreams == 1u ? ls.len[0] : ls.out[3] + ls.len[3];
    if (regen > lit_cap) return MC_ZSTD_E_CAPACITY;
    return Base::huffman(ls, huf, log);
  }
};

// One zstd stream f[0, n) into exactly usize bytes through `out` (cap ==
// usize): the stand-alone decoder's verdicts in its order, with the share in
// the place of the caller's capacity.  hash(np) = the low 32 bits of XXH64 of
// the np bytes produced.
template <class Src, class Sink, class Builder, class Hash>
MC_ZSTD_HD int mc_blosc_zstd_stream(Src &src, Sink &out, Builder &bld, const uint8_t *f, uint32_t n, uint32_t usize,
                                    mc_zstd_tables *T, Hash &hash) {
  if (n >= MC_ZSTD_MAX_BYTES || usize >= MC_ZSTD_MAX_BYTES) return MC_ZSTD_E_TABLE;
  mc_zstd_header h;
  uint32_t end_off;
  int e = (int)MC_ZSTD_UNI(mc_zstd_open(f, n, &h, &end_off));
  if (e != MC_ZSTD_OK) return e;
  if (h.content != MC_ZSTD_UNKNOWN && h.content != usize) return MC_ZSTD_E_SIZE;
  e = mc_zstd_blocks(src, out, bld, f, n, MC_ZSTD_UNI(h.data_off), MC_ZSTD_UNI(h.block_max), T);
  if (e != MC_ZSTD_OK) return e;
  if (out.op != usize) return MC_ZSTD_E_SIZE;
  if (h.checksum && mc_zstd_le(f + MC_ZSTD_UNI(end_off) - 4u, 4) != hash(out.op)) return MC_ZSTD_E_CHECK;
  return MC_ZSTD_OK;
}

// The zlib container header of stream f[0, n): *data_off = the first DEFLATE byte.
MC_INF_HD int mc_blosc_zlib_open(const uint8_t *f, uint32_t n, uint32_t usize, uint32_t *data_off) {
  *data_off = 0;
  if (n >= MC_INF_MAX_BYTES || usize >= MC_INF_MAX_BYTES) return MC_INF_E_TABLE;
  uint32_t empty;
  return mc_inf_parse_header(f, n, MC_INF_ZLIB, data_off, &empty);
}

// What follows mc_inf_blocks' verdict e (the sink flushed, `produced` bytes
// out): the share, then Adler-32 against the trailer where the reader stopped.
// adler(np) = the Adler-32 of the np bytes produced.  What follows the
// trailer is ignored, as the stand-alone inflater ignores it.
template <class Bits, class Hash>
MC_INF_HD int mc_blosc_zlib_finish(int e, Bits &br, uint32_t produced, uint32_t usize, const uint8_t *f, uint32_t n,
                                   Hash &adler) {
  if (e != MC_INF_OK) return e;
  if (produced != usize) return MC_INF_E_LENGTH;
  br.align();
  const uint32_t pos = br.bytepos();
  uint64_t after;
  return mc_inf_check_trailer(f, n, pos, MC_INF_ZLIB, adler(produced), produced, &after);
}
