// libblosc_hostcheck.so: the product's plan walker and scalar LZ4 decoder
// compiled for the host, for ctypes use by the CPU suite (tests/test_blosc_host.py).
#include "blosc_host.h"

extern "C" {

// one frame -> its still-filtered bytes; 0, -1 rejected by the header checks,
// -2 unsupported compressor, -3 out too small, > 0 an mc_lz4_error.
// info: 6 int32 {flags, typesize, blocksize, nbytes, nstreams, bad_stream}
int hc_blosc_decode(const uint8_t *frame, size_t len, uint8_t *out, size_t out_cap, int32_t *info) {
  return hc_decode(frame, len, out, out_cap, reinterpret_cast<hc_info *>(info));
}

int hc_lz4_decode_stream(const uint8_t *src, size_t n, uint8_t *dst, size_t usize) {
  if (n > 0x7fffffffu || usize >= MC_LZ4_MAX_USIZE) return HC_REJECTED;
  return lz4_decode_stream(src, (uint32_t)n, dst, (uint32_t)usize);
}

}  // extern "C"
