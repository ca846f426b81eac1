// liblz4codec_hostcheck.so: the `lz4` codec's scalar stitched encoder, decode
// plan and scalar decoder compiled for the host, for ctypes use by the CPU
// suite (tests/test_lz4_host.py) and as the exact model of the GPU suite
// (tests/test_gpu_lz4.py).
#include "lz4codec_host.h"

extern "C" {

// n source bytes -> one LZ4 block of at most cap bytes at dst: its size, 0 = refused
size_t hl_lz4c_encode_chunk(const uint8_t *src, size_t n, uint8_t *dst, size_t cap) {
  if (n >= MC_LZ4_MAX_USIZE) return 0;
  return mc_lz4c_encode_chunk(src, (uint32_t)n, dst, cap > 0xffffffffu ? 0xffffffffu : (uint32_t)cap);
}

// the whole frame (size word + block): its length, 0 = refused
size_t hl_lz4c_encode_frame(const uint8_t *src, size_t n, uint8_t *dst, size_t cap) {
  if (n >= MC_LZ4_MAX_USIZE) return 0;
  return mc_lz4c_encode_frame(src, (uint32_t)n, dst, cap > 0xffffffffu ? 0xffffffffu : (uint32_t)cap);
}

size_t hl_lz4c_segment_sum(const uint8_t *src, size_t n) {
  return n < MC_LZ4_MAX_USIZE ? (size_t)hl_segment_sum(src, (uint32_t)n) : 0;
}

size_t hl_lz4c_block_bound(size_t n) { return mc_lz4c_block_bound((uint32_t)n); }
size_t hl_lz4c_frame_slot(size_t n) { return mc_lz4c_frame_slot((uint32_t)n); }

// a frame into dst: 0, a negative host error or a positive mc_lz4_error; *usize = its size word
int hl_lz4c_decode_frame(const uint8_t *frame, size_t len, uint8_t *dst, size_t dst_cap, uint32_t *usize) {
  return hl_decode_frame(frame, len, dst, dst_cap, usize);
}

// one LZ4 block into exactly usize bytes: 0 or an mc_lz4_error
int hl_lz4_decode_block(const uint8_t *src, size_t n, uint8_t *dst, size_t usize) {
  if (n > 0x7fffffffu || usize >= MC_LZ4_MAX_USIZE) return HL_INVALID;
  return lz4_decode_stream(src, (uint32_t)n, dst, (uint32_t)usize);
}

}  // extern "C"
