// libbz2_hostcheck.so: the scalar bzip2 model of csrc/mc_bz2.h compiled for
// the host, for ctypes use by the CPU suite (tests/test_bz2_host.py) and as
// the exact model of the GPU suite (tests/test_gpu_bz2.py).
#include <stdlib.h>

#include "../../numcodecs_amd/csrc/mc_bz2.h"

extern "C" {

// One frame into at most cap bytes at dst (NULL: count only): 0 or an
// mc_bz2_error.  out[0] = bytes produced, out[1] = the error record's second
// word (the blocks completed).
int hb_bz2(const uint8_t *frame, size_t n, uint8_t *dst, size_t cap, uint64_t *out) {
  static thread_local mc_bz2_tables tables;
  static thread_local void *work = nullptr;  // level 9: 4.5 MB, kept
  if (!work) work = malloc(5u * (size_t)MC_BZ2_BLOCK_UNIT * 9u);
  uint32_t produced = 0, word = 0;
  const uint32_t c = cap >= MC_BZ2_MAX_BYTES ? MC_BZ2_MAX_BYTES - 1u : (uint32_t)cap;
  const int e = mc_bz2_decode_stream(frame, n, dst, c, &produced, &word, &tables, work, 9);
  out[0] = produced, out[1] = word;
  return e;
}

// the stream header alone
int hb_bz2_header(const uint8_t *frame, size_t n, uint32_t *level, uint32_t *empty) {
  return mc_bz2_parse_header(frame, n, level, empty);
}

// the CRC of n bytes (the block CRC of the format)
uint32_t hb_bz2_crc(const uint8_t *p, size_t n) {
  uint32_t crc = 0xffffffffu;
  for (size_t i = 0; i < n; ++i) crc = mc_bz2_crc_byte(crc, p[i]);
  return ~crc;
}

// a * b mod P, and x^(8 k) mod P: what the wave's CRC fold is made of
uint32_t hb_bz2_gfmul(uint32_t a, uint32_t b) { return mc_bz2_gfmul(a, b); }
uint32_t hb_bz2_mulx(uint32_t v, uint32_t times) { return mc_bz2_mulx(v, times); }

size_t hb_bz2_tables_bytes(void) { return sizeof(mc_bz2_tables); }
size_t hb_bz2_record_bytes(void) { return sizeof(mc_bz2_frame); }

}  // extern "C"
