// zstd_enc_hostcheck_main: built with -fsanitize=address,undefined, as a
// process of its own.  Generated inputs (the sizes around every rule of
// csrc/mc_zstd_enc.h: 1 ... 5, 12, 13, 64, around 255 / 256, around 65535 /
// 65536 / 131072, runs, periods at the longest offset, alphabets of more than
// 128 bytes, and 50 seeded ones of 0-200000 bytes) go through the scalar
// encoder, with and without checksum, into a heap buffer of exactly
// mc_zstd_enc_bound bytes filled with a pattern; nothing at or past the
// returned size may be touched; the frame is decoded back by csrc/mc_zstd.h's
// scalar decoder into exactly n bytes; a buffer one byte shorter than the
// frame is refused and left untouched.  Exit 0 only if nothing differed.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../numcodecs_amd/csrc/mc_zstd_enc.h"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {  // xorshift64*
  rng_state ^= rng_state >> 12, rng_state ^= rng_state << 25, rng_state ^= rng_state >> 27;
  return (uint32_t)((rng_state * 0x2545f4914f6cdd1dull) >> 32);
}

static std::vector<uint8_t> filled(uint32_t n, int kind) {
  std::vector<uint8_t> v(n);
  switch (kind % 8) {
    case 0: for (auto &b : v) b = (uint8_t)(rnd() % 3); break;           // small alphabet
    case 1: for (auto &b : v) b = (uint8_t)rnd(); break;                 // noise
    case 2: {                                                            // runs
      uint8_t cur = 0;
      for (auto &b : v) { if (rnd() % 97 == 0) cur = (uint8_t)rnd(); b = cur; }
      break;
    }
    case 3: {                                                            // noise and zeros in long stretches
      bool noise = false;
      for (uint32_t i = 0; i < n; ++i) {
        if (rnd() % 30000 == 0) noise = !noise;
        v[i] = noise ? (uint8_t)rnd() : 0;
      }
      break;
    }
    case 4: {                                                            // a skewed alphabet of 40
      for (auto &b : v) { uint32_t r = rnd(), s = 0; while ((r & 1) && s < 39) r >>= 1, ++s; b = (uint8_t)(s * 5); }
      break;
    }
    case 5: {                                                            // a skewed alphabet of 256: FSE-coded weights
      for (auto &b : v) { const uint32_t r = rnd(); b = (uint8_t)((r & 3) ? (r >> 8) % 9 : (r >> 8)); }
      break;
    }
    case 6: {                                                            // records: one offset again and again
      for (uint32_t i = 0; i < n; ++i) v[i] = (i % 12 < 8 && i >= 12) ? v[i - 12] : (uint8_t)rnd();
      break;
    }
    default: {                                                           // a slow walk
      uint8_t cur = 0;
      for (auto &b : v) b = (cur = (uint8_t)(cur + rnd() % 3 - 1));
    }
  }
  return v;
}

static std::vector<uint8_t> periodic(uint32_t period, uint32_t n) {
  std::vector<uint8_t> v(n);
  for (uint32_t i = 0; i < n; ++i) v[i] = i < period ? (uint8_t)rnd() : v[i - period];
  return v;
}

static uint8_t *exact(size_t n) { return (uint8_t *)malloc(n ? n : 1); }

static int check_chunk(const std::vector<uint8_t> &in, uint32_t checksum) {
  static mc_zstd_tables T;
  static uint8_t lit[MC_ZSTD_BLOCK_MAX];
  const uint32_t n = (uint32_t)in.size();
  if (n == 0) return mc_zstd_encode_chunk(in.data(), 0, nullptr, 0, checksum) != 0;  // the host writes that frame
  uint8_t *src = exact(n), *back = exact(n);
  memcpy(src, in.data(), n);
  int bad = 0;
  const size_t cap = (size_t)mc_zstd_enc_bound(n, checksum);
  uint8_t *dst = exact(cap);
  memset(dst, 0xA5, cap);
  std::vector<mc_ze_seg> segs(mc_ze_nsegments(n));
  uint64_t need = 0;
  const uint64_t fs = mc_zstd_encode_chunk_report(src, n, dst, cap, checksum, segs.data(), &need);
  if (fs == 0 || fs > cap || need != fs) bad |= 1;
  else {
    for (size_t i = fs; i < cap; ++i)
      if (dst[i] != 0xA5) bad |= 2;
    uint64_t sum = mc_ze_header_bytes(n) + (checksum ? 4u : 0u);
    for (const mc_ze_seg &s : segs) sum += s.bytes;
    if (sum != fs) bad |= 4;
    uint8_t *frame = exact(fs);
    memcpy(frame, dst, fs);
    uint32_t produced = 0, word = 0;
    const int e = mc_zstd_decode_frame(frame, fs, back, n, lit, &produced, &word, &T);
    if (e != MC_ZSTD_OK || produced != n || memcmp(back, src, n) != 0) bad |= 8;
    // one byte less than it needs: refused, nothing written
    uint8_t *small = exact(fs - 1);
    memset(small, 0x5A, fs - 1);
    if (mc_zstd_encode_chunk(src, n, small, fs - 1, checksum) != 0) bad |= 16;
    for (size_t i = 0; i + 1 < fs; ++i)
      if (small[i] != 0x5A) bad |= 32;
    free(small), free(frame);
  }
  free(dst), free(src), free(back);
  return bad;
}

int main() {
  long chunks = 0, failures = 0;
  std::vector<std::vector<uint8_t>> inputs;
  for (uint32_t n : {0u, 1u, 2u, 3u, 4u, 5u, 12u, 13u, 64u, 67u, 255u, 256u, 257u, 65535u, 65536u, 65537u, 65540u, 131072u, 200001u})
    inputs.push_back(filled(n, 0));
  for (uint32_t n : {1u, 2u, 5u, 70000u, 65537u}) inputs.push_back(std::vector<uint8_t>(n, 7));
  for (uint32_t p : {65535u, 65536u}) inputs.push_back(periodic(p, 131072));
  for (int k = 1; k < 8; ++k) inputs.push_back(filled(70000, k));
  for (uint32_t n : {200u, 300u, 1000u, 5000u}) inputs.push_back(filled(n, 5));
  for (int k = 0; k < 50; ++k) inputs.push_back(filled(rnd() % 200001, k));
  for (const auto &in : inputs)
    for (uint32_t checksum = 0; checksum < 2; ++checksum) {
      ++chunks;
      if (const int bad = check_chunk(in, checksum))
        fprintf(stderr, "%zu bytes, checksum %u: mismatch %d\n", in.size(), checksum, bad), ++failures;
    }
  printf("chunks %ld failures %ld\n", chunks, failures);
  return failures == 0 ? 0 : 1;
}
