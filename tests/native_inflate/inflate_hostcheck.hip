// libinflate_hostcheck.so: the scalar inflate model of csrc/mc_inflate.h
// compiled for the host, for ctypes use by the CPU suite
// (tests/test_inflate_host.py) and as the exact model of the GPU suite
// (tests/test_gpu_inflate.py).
#include "../../numcodecs_amd/csrc/mc_inflate.h"

extern "C" {

// One frame into at most cap bytes at dst (NULL: count only, no trailer
// check): 0 or an mc_inf_error.  out[0] = bytes produced, out[1] = the error
// record's second word, out[2] = source bytes consumed.
int hi_inflate(const uint8_t *frame, size_t n, unsigned container, uint8_t *dst, size_t cap, uint64_t *out) {
  static thread_local mc_inf_tables tables;
  uint32_t produced = 0, word = 0;
  uint64_t consumed = 0;
  const int e = mc_inflate_stream(frame, n, container, dst, cap > 0xffffffffu ? 0xffffffffu : (uint32_t)cap, &produced,
                                  &consumed, &word, &tables);
  out[0] = produced, out[1] = word, out[2] = consumed;
  return e;
}

// the container header alone: 0 or an error; *data_off = the first DEFLATE byte
int hi_inflate_header(const uint8_t *frame, size_t n, unsigned container, uint32_t *data_off, uint32_t *empty) {
  return mc_inf_parse_header(frame, n, container, data_off, empty);
}

size_t hi_inflate_tables_bytes(void) { return sizeof(mc_inf_tables); }
size_t hi_inflate_record_bytes(void) { return sizeof(mc_inf_frame); }

}  // extern "C"
