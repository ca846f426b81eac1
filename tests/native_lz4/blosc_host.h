// The product's Blosc plan walker and LZ4 parser / predicate / scalar decoder
// (numcodecs_amd/csrc/mc_lz4.h) driven on the host: one frame -> its
// still-filtered bytes.  Test infrastructure only.
#pragma once

#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../numcodecs_amd/csrc/mc_lz4.h"

enum { HC_OK = 0, HC_REJECTED = -1, HC_UNSUPPORTED = -2, HC_TOO_SMALL = -3 };

struct hc_info {
  int32_t flags, typesize, blocksize, nbytes, nstreams, bad_stream;
};

// the host checks numcodecs_amd.blosc makes before launching
static inline int hc_header(const uint8_t *frame, size_t len, mc_blosc_frame *f) {
  if (len < MC_BLOSC_HEADER) return HC_REJECTED;
  if (frame[0] != 2) return HC_REJECTED;
  memset(f, 0, sizeof(*f));
  f->flags = frame[2];
  f->typesize = frame[3];
  f->nbytes = mc_lz4_le32(frame + 4);
  f->blocksize = mc_lz4_le32(frame + 8);
  const uint32_t cbytes = mc_lz4_le32(frame + 12);
  f->src_len = len;
  if (cbytes != len || f->typesize < 1) return HC_REJECTED;
  if (f->nbytes > 0x7fffffffu || (f->nbytes && (f->blocksize < 1 || f->blocksize >= MC_LZ4_MAX_USIZE)))
    return HC_REJECTED;
  if (!(f->flags & MC_BLOSC_F_MEMCPYED) && (f->flags >> 5) != 1) return HC_UNSUPPORTED;
  return HC_OK;
}

// 0, HC_* or a positive mc_lz4_error; out receives nbytes bytes
static inline int hc_decode(const uint8_t *frame, size_t len, uint8_t *out, size_t out_cap, hc_info *info) {
  mc_blosc_frame f;
  const int h = hc_header(frame, len, &f);
  if (info) {
    memset(info, 0, sizeof(*info));
    if (len >= MC_BLOSC_HEADER) {
      info->flags = (int32_t)f.flags, info->typesize = (int32_t)f.typesize;
      info->blocksize = (int32_t)f.blocksize, info->nbytes = (int32_t)f.nbytes;
    }
  }
  if (h != HC_OK) return h;
  if (f.nbytes == 0) return HC_OK;
  if (out_cap < f.nbytes) return HC_TOO_SMALL;
  f.dst = (uint64_t)(uintptr_t)out;
  const uint32_t nblocks = mc_blosc_nblocks(f.nbytes, f.blocksize);
  const uint32_t nstreams = mc_blosc_nstreams(f.flags, f.typesize, f.nbytes, f.blocksize);
  if (info) info->nstreams = (int32_t)nstreams;
  std::vector<mc_lz4_stream> streams(nstreams);
  memset(streams.data(), 0, nstreams * sizeof(mc_lz4_stream));
  int first = MC_LZ4_OK;
  for (uint32_t b = 0; b < nblocks; ++b) {
    uint32_t bad = 0;
    const int e = mc_blosc_plan_block(frame, f, 0, b, streams.data(), nstreams, &bad);
    if (e != MC_LZ4_OK && first == MC_LZ4_OK) {
      first = e;
      if (info) info->bad_stream = (int32_t)bad;
    }
  }
  // like the decode kernel: every valid stream is decoded, the first error is kept
  for (uint32_t s = 0; s < nstreams; ++s) {
    const mc_lz4_stream &d = streams[s];
    if (!(d.flags & MC_LZ4_S_VALID)) continue;
    uint8_t *dst = reinterpret_cast<uint8_t *>((uintptr_t)d.dst);
    if (dst < out || dst + d.usize > out + f.nbytes) return 100;  // the walker left the output: a bug
    if (d.src_off + d.cbytes > len) return 101;                    // ... or the frame
    int e = MC_LZ4_OK;
    if (d.flags & MC_LZ4_S_RAW) memcpy(dst, frame + d.src_off, d.usize);
    else e = lz4_decode_stream(frame + d.src_off, d.cbytes, dst, d.usize);
    if (e != MC_LZ4_OK && first == MC_LZ4_OK) {
      first = e;
      if (info) info->bad_stream = (int32_t)s;
    }
  }
  return first;
}
