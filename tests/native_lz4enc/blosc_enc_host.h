// The product's LZ4 encoder rules and Blosc frame layout helpers
// (numcodecs_amd/csrc/mc_lz4_enc.h) driven on the host: already-filtered
// bytes -> one Blosc1 frame, with the stream split, the raw and the memcpyed
// decisions made by the same code as the kernels'.  Test infrastructure only.
#pragma once

#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../numcodecs_amd/csrc/mc_lz4_enc.h"

enum { HE_REFUSED = -1, HE_TOO_SMALL = -3 };

// filtered / raw: nbytes bytes each; out: a slot of out_cap >= nbytes + 16
// bytes.  Returns the frame's cbytes, or HE_*.
static inline long he_encode_frame(const uint8_t *filtered, const uint8_t *raw, uint32_t nbytes, uint32_t typesize,
                                   uint32_t blocksize, uint32_t flags, uint8_t *out, size_t out_cap) {
  mc_blosc_enc_frame f;
  memset(&f, 0, sizeof(f));
  f.nbytes = nbytes, f.blocksize = blocksize, f.typesize = typesize, f.flags = flags;
  if (out_cap < (size_t)nbytes + MC_BLOSC_MAX_OVERHEAD) return HE_TOO_SMALL;
  const uint32_t nblocks = mc_blosc_nblocks(nbytes, blocksize);
  const uint32_t ns = nbytes && blocksize ? mc_blosc_nstreams(flags, typesize, nbytes, blocksize) : 0;
  if (!mc_blosc_enc_frame_ok(f, nblocks, ns, nbytes)) return HE_REFUSED;
  // compress: every stream into its own exactly sized scratch slot
  std::vector<std::vector<uint8_t>> scratch(ns);
  std::vector<uint32_t> csize(ns, 0);
  uint64_t total = (uint64_t)MC_BLOSC_HEADER + 4ull * nblocks;
  for (uint32_t s = 0; s < ns; ++s) {
    uint32_t block, first, off, neb;
    mc_blosc_enc_stream(f, s, &block, &first, &off, &neb);
    if (!(flags & MC_BLOSC_F_MEMCPYED)) {
      scratch[s].resize(neb);
      csize[s] = mc_lz4_encode_stream(filtered + off, neb, scratch[s].data(), neb);
    }
    total += mc_blosc_enc_stream_bytes(csize[s], neb);
  }
  // layout + gather
  const bool stored = mc_blosc_enc_memcpyed(f, total);
  const uint32_t cbytes = stored ? nbytes + MC_BLOSC_MAX_OVERHEAD : (uint32_t)total;
  mc_blosc_enc_header(out, f, stored, cbytes);
  if (stored) {
    memcpy(out + MC_BLOSC_HEADER, raw, nbytes);
    return cbytes;
  }
  uint64_t at = (uint64_t)MC_BLOSC_HEADER + 4ull * nblocks;
  for (uint32_t s = 0; s < ns; ++s) {
    uint32_t block, first, off, neb;
    mc_blosc_enc_stream(f, s, &block, &first, &off, &neb);
    if (first) mc_lz4e_put32(out + MC_BLOSC_HEADER + 4ull * block, (uint32_t)at);
    const uint32_t nb = csize[s] ? csize[s] : neb;
    mc_lz4e_put32(out + at, nb);
    memcpy(out + at + 4, csize[s] ? scratch[s].data() : filtered + off, nb);
    at += mc_blosc_enc_stream_bytes(csize[s], neb);
  }
  return cbytes;
}
