// deflate_hostcheck_main: built with -fsanitize=address,undefined, as a process
// of its own.
//   * generated inputs (the sizes around every rule of csrc/mc_deflate.h: 1, 3,
//     4, 12, 13, 64, around 65535 / 65536 / 131072, runs around the 258 split,
//     periods around the distance limit, and 60 seeded ones of 0-200000 bytes)
//     go through the scalar encoder, both containers, levels 1 and 0, into a
//     heap buffer of exactly mc_deflate_bound bytes filled with a pattern;
//     nothing at or past the returned size may be touched; the frame is
//     inflated back by the project's scalar inflate model into exactly n bytes;
//     a buffer one byte shorter than the frame is refused and left untouched;
//   * code lengths of adversarial frequency sets (Fibonacci, one symbol, none,
//     all equal) are checked: limit kept, Kraft sum exactly 1.
// Exit 0 only if nothing differed.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../numcodecs_amd/csrc/mc_deflate.h"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {  // xorshift64*
  rng_state ^= rng_state >> 12, rng_state ^= rng_state << 25, rng_state ^= rng_state >> 27;
  return (uint32_t)((rng_state * 0x2545f4914f6cdd1dull) >> 32);
}

static std::vector<uint8_t> filled(uint32_t n, int kind) {
  std::vector<uint8_t> v(n);
  switch (kind % 6) {
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
    case 4: {                                                            // a skewed alphabet: dynamic codes
      for (auto &b : v) { uint32_t r = rnd(), s = 0; while ((r & 1) && s < 39) r >>= 1, ++s; b = (uint8_t)(s * 5); }
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

static int check_chunk(const std::vector<uint8_t> &in, uint32_t container, uint32_t level) {
  static mc_inf_tables T;
  const uint32_t n = (uint32_t)in.size();
  if (n == 0) return mc_deflate_encode_chunk(in.data(), 0, nullptr, 0, container, level) != 0;  // the host writes that frame
  uint8_t *src = exact(n), *back = exact(n);
  memcpy(src, in.data(), n);
  int bad = 0;
  const size_t cap = (size_t)mc_deflate_bound(n, container);
  uint8_t *dst = exact(cap);
  memset(dst, 0xA5, cap);
  std::vector<mc_dfl_seg> segs(mc_dfl_nsegments(n));
  uint64_t need = 0;
  const uint64_t fs = mc_deflate_encode_chunk_report(src, n, dst, cap, container, level, segs.data(), &need);
  if (fs == 0 || fs > cap || need != fs) bad |= 1;
  else {
    for (size_t i = fs; i < cap; ++i)
      if (dst[i] != 0xA5) bad |= 2;
    uint64_t sum = mc_dfl_header_bytes(container) + mc_dfl_trailer_bytes(container);
    for (const mc_dfl_seg &s : segs) {
      sum += s.bytes;
      if (level == 0 && s.type != MC_DFL_STORED) bad |= 64;
    }
    if (sum != fs) bad |= 4;
    uint8_t *frame = exact(fs);
    memcpy(frame, dst, fs);
    uint32_t produced = 0, word = 0;
    uint64_t consumed = 0;
    const int e = mc_inflate_stream(frame, fs, container, back, n, &produced, &consumed, &word, &T);
    if (e != MC_INF_OK || produced != n || consumed != fs || memcmp(back, src, n) != 0) bad |= 8;
    // one byte less than it needs: refused, nothing written
    uint8_t *small = exact(fs - 1);
    memset(small, 0x5A, fs - 1);
    if (mc_deflate_encode_chunk(src, n, small, fs - 1, container, level) != 0) bad |= 16;
    for (size_t i = 0; i + 1 < fs; ++i)
      if (small[i] != 0x5A) bad |= 32;
    free(small), free(frame);
  }
  free(dst), free(src), free(back);
  return bad;
}

static int check_lengths(const std::vector<uint32_t> &freq, uint32_t maxbits) {
  static mc_dfl_work W;
  mc_dfl_scalar x;
  std::vector<uint8_t> lens(freq.size());
  mc_dfl_code_lengths(x, &W, freq.data(), (uint32_t)freq.size(), maxbits, lens.data());
  uint64_t kraft = 0;
  uint32_t used = 0;
  for (size_t i = 0; i < freq.size(); ++i) {
    if (lens[i] > maxbits) return 1;
    if (freq[i] && !lens[i]) return 2;
    if (lens[i]) kraft += 1ull << (maxbits - lens[i]), ++used;
  }
  if (kraft != 1ull << maxbits) return 3;
  return used >= 2 ? 0 : 4;
}

int main() {
  long chunks = 0, failures = 0;
  std::vector<std::vector<uint8_t>> inputs;
  for (uint32_t n : {0u, 1u, 2u, 3u, 4u, 5u, 12u, 13u, 64u, 67u, 65535u, 65536u, 65537u, 65540u, 131072u, 200001u})
    inputs.push_back(filled(n, 0));
  for (uint32_t n : {258u, 259u, 260u, 261u, 262u, 516u, 517u, 518u, 519u, 70000u}) inputs.push_back(std::vector<uint8_t>(n, 7));
  for (uint32_t p : {32767u, 32768u, 32769u}) inputs.push_back(periodic(p, 65536));
  inputs.push_back(filled(70000, 1));
  inputs.push_back(filled(70000, 4));
  for (int k = 0; k < 60; ++k) inputs.push_back(filled(rnd() % 200001, k));
  for (const auto &in : inputs)
    for (uint32_t container = 0; container < 2; ++container)
      for (uint32_t level : {1u, 0u}) {
        if (level == 0 && chunks % 3) { ++chunks; continue; }  // level 0 on a third of them
        ++chunks;
        if (const int bad = check_chunk(in, container, level))
          fprintf(stderr, "%zu bytes, container %u, level %u: mismatch %d\n", in.size(), container, level, bad), ++failures;
      }
  long sets = 0;
  for (uint32_t maxbits : {15u, 7u}) {
    const uint32_t n = maxbits == 15 ? 286 : 19;
    std::vector<std::vector<uint32_t>> fs;
    fs.push_back(std::vector<uint32_t>(n, 0));
    fs.push_back(std::vector<uint32_t>(n, 1));
    fs.push_back(std::vector<uint32_t>(n, 0)), fs.back()[n - 1] = 5;
    fs.push_back(std::vector<uint32_t>(n, 0)), fs.back()[0] = 5;
    fs.push_back(std::vector<uint32_t>(n, 0));
    for (uint32_t i = 0, a = 1, b = 1; i < n && i < 24; ++i) { fs.back()[i] = a; const uint32_t c = a + b; a = b, b = c; }
    fs.push_back(std::vector<uint32_t>(n, 0));
    for (uint32_t i = 0; i < n; ++i) fs.back()[n - 1 - i] = i < 20 ? 1u << i : 0;
    for (int k = 0; k < 200; ++k) {
      fs.push_back(std::vector<uint32_t>(n, 0));
      for (auto &f : fs.back()) f = rnd() % 4 == 0 ? 0 : (rnd() % 8 == 0 ? rnd() % 60000 : rnd() % 16);
    }
    for (const auto &f : fs) {
      ++sets;
      if (const int bad = check_lengths(f, maxbits)) fprintf(stderr, "code lengths, limit %u: fault %d\n", maxbits, bad), ++failures;
    }
  }
  printf("chunks %ld length sets %ld failures %ld\n", chunks, sets, failures);
  return failures == 0 ? 0 : 1;
}
