// mc_lz4.h -- Blosc1 frame walking and LZ4 block decoding, shared by the
// gfx950 kernels (mc_blosc_dec.hip) and the host build of the CPU suite
// (tests/native_lz4): the parser, the validity predicate and the plan walker
// below are the very code that guards the device.
//
// Blosc1 frame (c-blosc 1.x; numcodecs blosc.pyx:211-326 hands buffers to it):
//   header, 16 bytes: version, versionlz, flags, typesize, then nbytes,
//     blocksize, cbytes as little-endian u32;
//   flags: bit 0 byte-shuffle, bit 1 memcpyed, bit 2 bit-shuffle, bit 4 (0x10)
//     do-not-split, bits 5-7 compressor format (1 = lz4 / lz4hc);
//   nblocks = ceil(nbytes / blocksize); nblocks little-endian i32 `bstarts`
//     (offsets from the frame's start) follow the header at offset 16;
//   a block is blocksize bytes, the last one nbytes % blocksize if that is not
//     zero.  It is split into typesize streams only if the do-not-split bit is
//     clear, it is a full block, typesize <= 16 and blocksize / typesize >= 128;
//     otherwise it is one stream.  (c-blosc keeps blocksize a multiple of
//     typesize; a split block that is not is rejected here.)
//   a stream is a little-endian i32 cbytes followed by cbytes bytes: stored raw
//     when cbytes equals the stream's uncompressed size, else one LZ4 block;
//   a memcpyed frame is nbytes raw bytes at offset 16, unfiltered, whatever
//     its format bits say (walked here as one stored stream per block).
//
// LZ4 block: sequences of token (literal length << 4 | match length - 4, 15 =
// extension bytes follow, each added, the last one != 255), literals, 2-byte
// little-endian offset, match-length extension.  The last sequence ends after
// its literals.
#pragma once

#include <stddef.h>
#include <stdint.h>

#ifndef MC_LZ4_HD
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define MC_LZ4_HD __host__ __device__ __forceinline__
#else
#define MC_LZ4_HD inline
#endif
#endif

// error codes of the device error record / the host decoder (0 = none)
enum mc_lz4_error {
  MC_LZ4_OK = 0,
  MC_LZ4_E_BSTART = 1,     // bstarts table or entry outside the frame
  MC_LZ4_E_CBYTES = 2,     // a stream's cbytes word or data outside the frame
  MC_LZ4_E_SPLIT = 3,      // split block whose size is no multiple of typesize
  MC_LZ4_E_TRUNCATED = 4,  // sequence header runs past the source stream
  MC_LZ4_E_LIT_SRC = 5,    // literal run leaves the source stream
  MC_LZ4_E_LIT_DST = 6,    // literal run leaves the destination
  MC_LZ4_E_OFFSET0 = 7,    // match offset 0
  MC_LZ4_E_OFFSET = 8,     // match offset beyond the bytes produced so far
  MC_LZ4_E_MATCH_DST = 9,  // match leaves the destination
  MC_LZ4_E_SIZE = 10,      // stream ended short of its uncompressed size
  MC_LZ4_E_MEMCPY = 11,    // memcpyed frame shorter than 16 + nbytes
  MC_LZ4_E_TABLE = 12,     // the caller's frame table contradicts itself
};

#define MC_BLOSC_F_SHUFFLE 0x1u
#define MC_BLOSC_F_MEMCPYED 0x2u
#define MC_BLOSC_F_BITSHUFFLE 0x4u
#define MC_BLOSC_F_NOSPLIT 0x10u
#define MC_BLOSC_HEADER 16u
// streams (blocks) are shorter than this: c-blosc's MAX_BLOCKSIZE is
// (INT_MAX - 255 * 4) / 3; the entry point refuses larger block sizes
#define MC_LZ4_MAX_USIZE 0x40000000u
#define MC_BLOSC_MAX_SPLITS 16u
#define MC_BLOSC_MIN_SPLIT_ELEMS 128u

// One frame of a batch, as the host read it from the 16-byte header (device
// table, one record per frame).
struct mc_blosc_frame {
  uint64_t src_off;      // the frame's first byte in the concatenated frames
  uint64_t src_len;      // its length
  uint64_t dst;          // device address the frame's (still filtered) bytes go to
  uint32_t nbytes;       // header fields
  uint32_t blocksize;
  uint32_t typesize;
  uint32_t flags;
  uint32_t block_base;   // index of the frame's first block / stream in the batch
  uint32_t stream_base;
};

#define MC_LZ4_S_RAW 1u    // stored: copy cbytes bytes
#define MC_LZ4_S_VALID 2u  // cleared when the plan rejected the block
#define MC_LZ4_S_FORMAT_SHIFT 8u  // above it: the frame's format, where the caller's plan kernel notes it (mc_blosc_z.h)

// One stream, as the plan kernel leaves it for the decode kernel.
struct mc_lz4_stream {
  uint64_t src_off;  // first data byte in the concatenated frames
  uint64_t dst;      // device address of the stream's first output byte
  uint32_t cbytes;
  uint32_t usize;    // uncompressed size
  uint32_t frame;
  uint32_t flags;
};

MC_LZ4_HD uint32_t mc_blosc_nblocks(uint32_t nbytes, uint32_t blocksize) {
  return blocksize ? (uint32_t)(((uint64_t)nbytes + blocksize - 1) / blocksize) : 0u;
}
MC_LZ4_HD uint32_t mc_blosc_block_size(uint32_t nbytes, uint32_t blocksize, uint32_t block) {
  const uint32_t nblocks = mc_blosc_nblocks(nbytes, blocksize), rem = nbytes % blocksize;
  return (block + 1 < nblocks || rem == 0) ? blocksize : rem;
}
// streams of a block of `bsize` bytes
MC_LZ4_HD uint32_t mc_blosc_nsplit(uint32_t flags, uint32_t typesize, uint32_t blocksize, uint32_t bsize) {
  if (flags & MC_BLOSC_F_MEMCPYED) return 1u;
  const bool split = !(flags & MC_BLOSC_F_NOSPLIT) && bsize == blocksize && typesize <= MC_BLOSC_MAX_SPLITS &&
                     typesize >= 1 && blocksize / typesize >= MC_BLOSC_MIN_SPLIT_ELEMS;
  return split ? typesize : 1u;
}
// streams of a whole frame, and the index of a block's first stream in it
MC_LZ4_HD uint32_t mc_blosc_block_stream0(uint32_t flags, uint32_t typesize, uint32_t blocksize, uint32_t block) {
  return block * mc_blosc_nsplit(flags, typesize, blocksize, blocksize);
}
MC_LZ4_HD uint32_t mc_blosc_nstreams(uint32_t flags, uint32_t typesize, uint32_t nbytes, uint32_t blocksize) {
  const uint32_t nblocks = mc_blosc_nblocks(nbytes, blocksize);
  if (!nblocks) return 0u;
  return mc_blosc_block_stream0(flags, typesize, blocksize, nblocks - 1) +
         mc_blosc_nsplit(flags, typesize, blocksize, mc_blosc_block_size(nbytes, blocksize, nblocks - 1));
}

MC_LZ4_HD uint32_t mc_lz4_le32(const uint8_t *p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// The plan walker: the descriptors of block `block` of frame `f` (whose bytes
// are frames + f.src_off, f.src_len long) into streams[f.stream_base + ...].
// Everything read is checked against f.src_len first.  Every descriptor of
// the block is written; on an error (returned) they are left without
// MC_LZ4_S_VALID, so that the decode kernel skips them.
MC_LZ4_HD int mc_blosc_plan_block(const uint8_t *frames, const mc_blosc_frame &f, uint32_t frame_index,
                                  uint32_t block, mc_lz4_stream *streams, uint32_t nstreams_total,
                                  uint32_t *bad_stream) {
  const uint8_t *fr = frames + f.src_off;
  const uint64_t len = f.src_len;
  const uint32_t nblocks = mc_blosc_nblocks(f.nbytes, f.blocksize);
  *bad_stream = 0;
  // a table that disagrees with the header fields writes no descriptor at all
  if (f.typesize < 1 || block >= nblocks ||
      (uint64_t)f.stream_base + mc_blosc_nstreams(f.flags, f.typesize, f.nbytes, f.blocksize) > nstreams_total)
    return MC_LZ4_E_TABLE;
  const uint32_t bsize = mc_blosc_block_size(f.nbytes, f.blocksize, block);
  const uint32_t nsplit = mc_blosc_nsplit(f.flags, f.typesize, f.blocksize, bsize);
  const uint32_t s0 = mc_blosc_block_stream0(f.flags, f.typesize, f.blocksize, block);
  const uint32_t neb = bsize / nsplit;
  const uint64_t dst0 = f.dst + (uint64_t)block * f.blocksize;
  mc_lz4_stream *out = streams + f.stream_base + s0;
  for (uint32_t j = 0; j < nsplit; ++j) {
    out[j].src_off = 0;
    out[j].dst = dst0 + (uint64_t)j * neb;
    out[j].cbytes = 0;
    out[j].usize = neb;
    out[j].frame = frame_index;
    out[j].flags = 0;
  }
  *bad_stream = s0;
  if (f.flags & MC_BLOSC_F_MEMCPYED) {
    if (len < (uint64_t)MC_BLOSC_HEADER + f.nbytes) return MC_LZ4_E_MEMCPY;
    out[0].src_off = f.src_off + MC_BLOSC_HEADER + (uint64_t)block * f.blocksize;
    out[0].cbytes = bsize;
    out[0].flags = MC_LZ4_S_RAW | MC_LZ4_S_VALID;
    return MC_LZ4_OK;
  }
  if (bsize % nsplit) return MC_LZ4_E_SPLIT;
  const uint64_t table_end = (uint64_t)MC_BLOSC_HEADER + 4ull * nblocks;
  if (table_end > len) return MC_LZ4_E_BSTART;
  const uint32_t bstart = mc_lz4_le32(fr + MC_BLOSC_HEADER + 4ull * block);
  if (bstart < table_end || bstart > len || (bstart & 0x80000000u)) return MC_LZ4_E_BSTART;
  uint64_t p = bstart;
  for (uint32_t j = 0; j < nsplit; ++j) {
    *bad_stream = s0 + j;
    if (p + 4 > len) return MC_LZ4_E_CBYTES;
    const uint32_t cb = mc_lz4_le32(fr + p);
    p += 4;
    if (cb == 0 || (cb & 0x80000000u) || p + cb > len) return MC_LZ4_E_CBYTES;
    out[j].src_off = f.src_off + p;
    out[j].cbytes = cb;
    p += cb;
  }
  // only a block whose every stream lies inside the frame is decoded
  for (uint32_t j = 0; j < nsplit; ++j)
    out[j].flags = MC_LZ4_S_VALID | (out[j].cbytes == neb ? MC_LZ4_S_RAW : 0u);
  return MC_LZ4_OK;
}

// One parsed sequence of a stream of n source bytes.
struct mc_lz4_seq {
  uint32_t lit_pos;    // source index of the first literal
  uint32_t lit_len;
  uint32_t offset;     // match distance (unset when last)
  uint32_t match_len;  // 0 when last
  uint32_t next;       // source index after the sequence
  uint32_t last;       // the stream ends after the literals
};

// a plain byte reader (the host's; the kernel reads through a wave-wide window)
struct mc_lz4_ptr_reader {
  const uint8_t *src;
  MC_LZ4_HD uint32_t byte(uint32_t i) { return src[i]; }
};

// The sequence-header parser: the sequence that starts at source index ip < n.
// Reads source bytes only at indices < n.  Returns 0, MC_LZ4_E_TRUNCATED or
// MC_LZ4_E_LIT_SRC (the literal run must stay inside the source stream).
template <class Reader>
MC_LZ4_HD int mc_lz4_parse(Reader &rd, uint32_t n, uint32_t ip, mc_lz4_seq *s) {
  const uint32_t tok = rd.byte(ip++);
  uint32_t lit = tok >> 4;
  if (lit == 15) {
    uint32_t b;
    do {
      if (ip >= n) return MC_LZ4_E_TRUNCATED;
      b = rd.byte(ip++);
      lit += b;
      if (lit > n) return MC_LZ4_E_LIT_SRC;  // cannot fit (and never overflows)
    } while (b == 255);
  }
  s->lit_pos = ip;
  s->lit_len = lit;
  if (lit > n - ip) return MC_LZ4_E_LIT_SRC;
  ip += lit;
  s->offset = 0;
  s->match_len = 0;
  s->last = ip == n;
  if (!s->last) {
    if (n - ip < 2) return MC_LZ4_E_TRUNCATED;
    s->offset = rd.byte(ip) | (rd.byte(ip + 1) << 8);
    ip += 2;
    uint32_t ml = tok & 15;
    if (ml == 15) {
      uint32_t b;
      do {
        if (ip >= n) return MC_LZ4_E_TRUNCATED;
        b = rd.byte(ip++);
        ml += b;
        if (ml > MC_LZ4_MAX_USIZE) ml = MC_LZ4_MAX_USIZE;  // saturate: no stream is that long, so it is rejected
      } while (b == 255);
    }
    s->match_len = ml + 4;
  }
  s->next = ip;
  return MC_LZ4_OK;
}

// The validity predicate: may sequence s be copied when `produced` of the
// stream's `usize` bytes exist?  Checked before any byte of it is copied.
MC_LZ4_HD int mc_lz4_check(const mc_lz4_seq &s, uint32_t produced, uint32_t usize) {
  if (s.lit_len > usize - produced) return MC_LZ4_E_LIT_DST;
  if (s.last) return MC_LZ4_OK;
  const uint32_t at = produced + s.lit_len;
  if (s.offset == 0) return MC_LZ4_E_OFFSET0;
  if (s.offset > at) return MC_LZ4_E_OFFSET;
  if (s.match_len > usize - at) return MC_LZ4_E_MATCH_DST;
  return MC_LZ4_OK;
}

// Plain scalar decoder built from the parser and the predicate: n source
// bytes into exactly usize destination bytes.  0 or an mc_lz4_error.
MC_LZ4_HD int lz4_decode_stream(const uint8_t *src, uint32_t n, uint8_t *dst, uint32_t usize) {
  mc_lz4_ptr_reader rd{src};
  uint32_t ip = 0, op = 0;
  while (ip < n) {
    mc_lz4_seq s;
    int e = mc_lz4_parse(rd, n, ip, &s);
    if (e == MC_LZ4_OK) e = mc_lz4_check(s, op, usize);
    if (e != MC_LZ4_OK) return e;
    for (uint32_t k = 0; k < s.lit_len; ++k) dst[op + k] = src[s.lit_pos + k];
    op += s.lit_len;
    for (uint32_t k = 0; k < s.match_len; ++k) dst[op + k] = dst[op + k - s.offset];  // byte-serial by definition
    op += s.match_len;
    ip = s.next;
  }
  return op == usize ? MC_LZ4_OK : MC_LZ4_E_SIZE;
}
