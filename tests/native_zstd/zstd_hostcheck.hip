// libzstd_hostcheck.so: the scalar Zstandard model of csrc/mc_zstd.h compiled
// for the host, for ctypes use by the CPU suite (tests/test_zstd_host.py) and
// as the exact model of the GPU suite (tests/test_gpu_zstd.py).
#include <stdlib.h>

#include "../../numcodecs_amd/csrc/mc_zstd.h"

extern "C" {

// One frame into at most cap bytes at dst (NULL: count only, no Huffman decode,
// no check stage): 0 or an mc_zstd_error.  out[0] = bytes produced, out[1] =
// the error record's second word.
int hz_decode(const uint8_t *frame, size_t n, uint8_t *dst, size_t cap, uint64_t *out) {
  static thread_local mc_zstd_tables tables;
  static thread_local uint8_t lit[MC_ZSTD_BLOCK_MAX];
  uint32_t produced = 0, word = 0;
  const int e = mc_zstd_decode_frame(frame, n, dst, cap > 0xffffffffu ? 0xffffffffu : (uint32_t)cap, lit, &produced,
                                     &word, &tables);
  out[0] = produced, out[1] = word;
  return e;
}

// the frame header and the verdicts that come before the blocks: 0 or an error.
// out[0] = the declared size (all ones: none), out[1] = the window, out[2] =
// the first block header, out[3] = checksum flag, out[4] = Block_Maximum_Size,
// out[5] = the byte behind the frame, out[6] = Dictionary_ID
int hz_open(const uint8_t *frame, size_t n, uint64_t *out) {
  mc_zstd_header h;
  uint32_t end = 0;
  const int e = mc_zstd_open(frame, n, &h, &end);
  out[0] = h.content, out[1] = h.window, out[2] = h.data_off, out[3] = h.checksum, out[4] = h.block_max, out[5] = end;
  out[6] = h.dict_id;
  return e;
}

uint64_t hz_xxh64(const uint8_t *p, size_t n) { return mc_xxh64(p, (uint32_t)n); }

size_t hz_tables_bytes(void) { return sizeof(mc_zstd_tables); }
size_t hz_record_bytes(void) { return sizeof(mc_zstd_frame); }

}  // extern "C"
