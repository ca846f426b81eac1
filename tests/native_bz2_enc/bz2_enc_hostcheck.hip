// libbz2_enc_hostcheck.so: the scalar bzip2 encoder model of csrc/mc_bz2_enc.h
// compiled for the host, for ctypes use by the CPU suite
// (tests/test_bz2_enc_host.py) and as the exact model of the GPU suite
// (tests/test_gpu_bz2_enc.py).
#include <stdlib.h>

#include "../../numcodecs_amd/csrc/mc_bz2_enc.h"

extern "C" {

// One chunk into at most cap bytes at dst: 0 or an error code.  out[0] = the
// frame's size, out[1..5] = blocks, fallback blocks, blocks with more than one
// distinct selector, the most doubling rounds of a block, the blocks' bits.
int hb_bz2e_encode(const uint8_t *src, size_t n, uint8_t *dst, size_t cap, uint32_t level, uint64_t *out) {
  int err = 0;
  mc_bz2e_census c = {0, 0, 0, 0, 0};
  out[0] = mc_bz2_encode_chunk(src, n, dst, cap, level, &err, &c);
  out[1] = c.blocks, out[2] = c.fallback, out[3] = c.multi_table, out[4] = c.rounds_max, out[5] = c.bits;
  return err;
}

uint64_t hb_bz2e_bound(uint64_t n, uint32_t level) { return mc_bz2_enc_bound(n, level); }
uint32_t hb_bz2e_seg(uint32_t level) { return mc_bz2e_seg(level); }

uint32_t hb_bz2e_rle1(const uint8_t *src, uint32_t n, uint8_t *out) { return mc_bz2e_rle1(src, n, out); }

// the model's sort: blk[0, n), n >= 1 -> col[0, n); returns origPtr
uint32_t hb_bz2e_bwt(const uint8_t *blk, uint32_t n, uint8_t *col, uint32_t *rounds) {
  uint32_t *w = (uint32_t *)malloc(16ull * n);
  const uint32_t orig = mc_bz2e_bwt_model(blk, n, col, w, rounds);
  free(w);
  return orig;
}

size_t hb_bz2e_chunk_bytes(void) { return sizeof(mc_bz2e_chunk); }
size_t hb_bz2e_block_bytes(void) { return sizeof(mc_bz2e_block); }

}  // extern "C"
