// libdeflate_hostcheck.so: the scalar DEFLATE encoder of csrc/mc_deflate.h
// compiled for the host, for ctypes use by the CPU suite
// (tests/test_deflate_host.py) and as the exact model of the GPU suite
// (tests/test_gpu_deflate.py).
#include "../../numcodecs_amd/csrc/mc_deflate.h"

extern "C" {

size_t hd_deflate_bound(size_t n, unsigned container) { return (size_t)mc_deflate_bound(n, container); }

// n source bytes -> one frame of at most cap bytes at dst: its size, 0 =
// refused (nothing written).  segs (may be NULL): ceil(n / 65536) records of
// hd_deflate_seg_bytes() bytes; *need (may be NULL): the frame's size either way.
size_t hd_deflate_encode(const uint8_t *src, size_t n, uint8_t *dst, size_t cap, unsigned container, unsigned level,
                         void *segs, uint64_t *need) {
  return (size_t)mc_deflate_encode_chunk_report(src, n, dst, cap, container, level, static_cast<mc_dfl_seg *>(segs),
                                                need);
}

// the parse of one segment (n <= 65536): seqs receives n / 4 records of 8
// bytes at most, hist 320 words; returns the number of sequences
unsigned hd_deflate_parse(const uint8_t *src, unsigned n, void *seqs, unsigned *tail_lit, unsigned *hist) {
  if (n > MC_DFL_SEGMENT) return 0;
  return mc_dfl_parse_segment(src, n, static_cast<mc_dfl_seq *>(seqs), tail_lit, hist);
}

// code lengths of n <= 286 frequencies, at most maxbits bits
void hd_deflate_code_lengths(const unsigned *freq, unsigned n, unsigned maxbits, uint8_t *lens) {
  static thread_local mc_dfl_work W;
  mc_dfl_scalar x;
  if (n < 2 || n > 288) return;
  mc_dfl_code_lengths(x, &W, freq, n, maxbits, lens);
}

unsigned hd_deflate_npairs(unsigned len) { return mc_dfl_npairs(len); }
unsigned hd_deflate_piece(unsigned len, unsigned j) { return mc_dfl_piece(len, j); }
unsigned hd_deflate_len_sym(unsigned len) { return mc_dfl_len_sym(len); }
unsigned hd_deflate_dist_sym(unsigned dist) { return mc_dfl_dist_sym(dist); }
size_t hd_deflate_seg_bytes(void) { return sizeof(mc_dfl_seg); }
size_t hd_deflate_record_bytes(void) { return sizeof(mc_dfl_enc_chunk); }

}  // extern "C"
