// libblosc_enc_hostcheck.so: the product's scalar LZ4 encoder and the frame
// layout helpers compiled for the host, for ctypes use by the CPU suite
// (tests/test_blosc_encode_host.py) and as the exact model of the GPU suite.
#include "blosc_enc_host.h"

extern "C" {

// n source bytes -> at most cap bytes at dst: the compressed size, 0 = store raw
size_t he_lz4_encode_stream(const uint8_t *src, size_t n, uint8_t *dst, size_t cap) {
  if (n >= MC_LZ4_MAX_USIZE || cap > 0xffffffffu) return 0;
  return mc_lz4_encode_stream(src, (uint32_t)n, dst, (uint32_t)cap);
}

// already-filtered bytes (+ the unfiltered ones) -> one frame in out; cbytes or < 0
long he_blosc_encode(const uint8_t *filtered, const uint8_t *raw, size_t nbytes, size_t typesize, size_t blocksize,
                     unsigned flags, uint8_t *out, size_t out_cap) {
  if (nbytes < 1 || nbytes > 0x7fffffffu || typesize > 255 || blocksize > 0xffffffffu) return HE_REFUSED;
  return he_encode_frame(filtered, raw, (uint32_t)nbytes, (uint32_t)typesize, (uint32_t)blocksize, flags, out,
                         out_cap);
}

}  // extern "C"
