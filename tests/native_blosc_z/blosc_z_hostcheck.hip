// libblosc_z_hostcheck.so: the Blosc plan walker, the rules for zstd / zlib
// streams inside Blosc, the scalar decoders and, for cname='zstd', the scalar
// Zstandard encoder with the Blosc layout helpers (csrc/mc_lz4.h, mc_blosc_z.h,
// mc_zstd.h, mc_inflate.h, mc_zstd_enc.h, mc_lz4_enc.h) compiled for the host, for ctypes use by the CPU
// suite (tests/test_blosc_z_host.py) and as the exact model of the GPU suite
// (tests/test_gpu_blosc_z.py).
#include "blosc_z_host.h"

extern "C" {

// one frame -> its still-filtered bytes: 0, HCZ_* or the positive code of the
// frame's error record (mc_blosc_z.h); info: 8 int32 (hcz_info)
int hcz_blosc_decode(const uint8_t *frame, size_t len, uint8_t *out, size_t out_cap, int32_t *info) {
  return hcz_decode(frame, len, out, out_cap, reinterpret_cast<hcz_info *>(info));
}

// already-filtered bytes -> one Blosc1 zstd frame: its cbytes, or HCZ_*
long hcz_blosc_encode(const uint8_t *filtered, const uint8_t *raw, uint32_t nbytes, uint32_t typesize, uint32_t blocksize,
                      uint32_t flags, uint8_t *out, size_t out_cap) {
  return hcz_encode_frame(filtered, raw, nbytes, typesize, blocksize, flags, out, out_cap);
}

size_t hcz_record_bytes(void) { return sizeof(mc_blosc_zframe); }
int hcz_container_shift(void) { return MC_BLOSC_Z_CONTAINER; }

}  // extern "C"
