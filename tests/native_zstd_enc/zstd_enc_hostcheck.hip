// libzstd_enc_hostcheck.so: the scalar Zstandard encoder of csrc/mc_zstd_enc.h
// compiled for the host, for ctypes use by the CPU suite
// (tests/test_zstd_encode_host.py) and as the exact model of the GPU suite
// (tests/test_gpu_zstd_encode.py).
#include "../../numcodecs_amd/csrc/mc_zstd_enc.h"

extern "C" {

size_t hze_bound(size_t n, unsigned checksum) { return (size_t)mc_zstd_enc_bound(n, checksum); }

// n source bytes -> one frame of at most cap bytes at dst: its size, 0 =
// refused (nothing written).  segs (may be NULL): ceil(n / 65536) records of
// hze_seg_bytes() bytes; *need (may be NULL): the frame's size either way.
size_t hze_encode(const uint8_t *src, size_t n, uint8_t *dst, size_t cap, unsigned checksum, void *segs, uint64_t *need) {
  return (size_t)mc_zstd_encode_chunk_report(src, n, dst, cap, checksum, static_cast<mc_ze_seg *>(segs), need);
}

// hist[0, nsym) -> norm[0, nsym); returns the accuracy log
unsigned hze_normalise(const unsigned *hist, unsigned nsym, unsigned total, unsigned max_log, int16_t *norm) {
  return nsym <= 64 ? mc_ze_normalise(hist, nsym, total, max_log, norm) : 0;
}
// the count description of norm[0, nsym) (at most 64 bytes); returns its bytes
unsigned hze_write_counts(const int16_t *norm, unsigned nsym, unsigned log, uint8_t *out) {
  return mc_ze_write_counts(norm, nsym, log, out);
}
unsigned hze_ll_code(unsigned v) { return mc_ze_ll_code(v); }
unsigned hze_ml_code(unsigned v) { return mc_ze_ml_code(v); }
size_t hze_seg_bytes(void) { return sizeof(mc_ze_seg); }
size_t hze_record_bytes(void) { return sizeof(mc_zstd_enc_chunk); }

}  // extern "C"
