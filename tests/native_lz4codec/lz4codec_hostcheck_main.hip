// lz4codec_hostcheck_main DIR [DIR ...]: built with
// -fsanitize=address,undefined, as a process of its own.
//   * every input file (*.bin) under the directories, and 120 seeded generated
//     inputs of 0-200000 bytes, go through the `lz4` codec's scalar stitched
//     encoder (csrc/mc_lz4_codec.h) into a heap buffer of exactly the bound's
//     size (n + n / 255 + 2 for the block, the reference's 4 + n + n / 255 + 16
//     for the frame) and are decoded back by the shared scalar decoder into a
//     buffer of exactly n bytes;
//   * every frame file (*.dat) is decoded into a heap buffer of exactly its
//     size word, then again under mutations of the size word, of tokens and
//     offsets, and truncated; a mutation may decode or be rejected, but a read
//     outside the frame or a write outside the destination ends the run.
// Exit 0 only if nothing differed.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <filesystem>
#include <fstream>
#include <string>
#include <vector>

#include "lz4codec_host.h"

namespace fs = std::filesystem;

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {  // xorshift64*
  rng_state ^= rng_state >> 12, rng_state ^= rng_state << 25, rng_state ^= rng_state >> 27;
  return (uint32_t)((rng_state * 0x2545f4914f6cdd1dull) >> 32);
}

static std::vector<uint8_t> generated(int k) {
  static const uint32_t edges[] = {0, 1, 12, 13, 64, 65535, 65536, 65537, 65536 + 12, 65536 + 13, 131072};
  const uint32_t n = k < 11 ? edges[k] : rnd() % 200001;
  std::vector<uint8_t> v(n);
  switch (k % 5) {
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
    default: {                                                           // a slow walk
      uint8_t cur = 0;
      for (auto &b : v) b = (cur = (uint8_t)(cur + rnd() % 3 - 1));
    }
  }
  return v;
}

static uint8_t *exact(size_t n) { return (uint8_t *)malloc(n ? n : 1); }

// 0 if the chunk round-trips through a block and through a frame
static int check_chunk(const std::vector<uint8_t> &in) {
  const uint32_t n = (uint32_t)in.size();
  if (n == 0) return mc_lz4c_encode_chunk(in.data(), 0, nullptr, 0) != 0;  // refused: the host writes that frame
  uint8_t *src = exact(n), *back = exact(n);
  memcpy(src, in.data(), n);
  int bad = 0;
  {
    const uint32_t cap = mc_lz4c_block_bound(n);
    uint8_t *dst = exact(cap);
    const uint32_t cs = mc_lz4c_encode_chunk(src, n, dst, cap);
    if (cs == 0 || cs > cap) bad |= 1;
    else {
      uint8_t *comp = exact(cs);
      memcpy(comp, dst, cs);
      if (lz4_decode_stream(comp, cs, back, n) != MC_LZ4_OK || memcmp(back, src, n) != 0) bad |= 2;
      if ((uint64_t)cs > hl_segment_sum(src, n)) bad |= 4;
      // one byte less than it needs: refused, nothing written
      uint8_t *small = exact(cs - 1);
      if (mc_lz4c_encode_chunk(src, n, small, cs - 1) != 0) bad |= 8;
      free(small), free(comp);
    }
    free(dst);
  }
  {
    const uint32_t cap = mc_lz4c_frame_slot(n);
    uint8_t *dst = exact(cap);
    const uint32_t fl = mc_lz4c_encode_frame(src, n, dst, cap);
    uint32_t usize = 0;
    if (fl <= MC_LZ4C_HEADER || fl > cap) bad |= 16;
    else {
      uint8_t *frame = exact(fl);
      memcpy(frame, dst, fl);
      memset(back, 0, n);
      if (hl_decode_frame(frame, fl, back, n, &usize) != HL_OK || usize != n || memcmp(back, src, n) != 0) bad |= 32;
      free(frame);
    }
    free(dst);
  }
  free(src), free(back);
  return bad;
}

// decode `frame` (exactly len heap bytes) into exactly its size word's bytes; the result code
static int decode_exact(const std::vector<uint8_t> &frame, std::vector<uint8_t> *out) {
  const size_t len = frame.size();
  uint8_t *f = exact(len);
  if (len) memcpy(f, frame.data(), len);
  uint32_t usize = 0;
  int rc = hl_decode_frame(f, len, nullptr, 0, &usize);  // the size word only
  if (rc == HL_TOO_SMALL && usize <= (1u << 24)) {       // (a mutated word may ask for more: the plan alone then)
    uint8_t *dst = exact(usize);
    rc = hl_decode_frame(f, len, dst, usize, &usize);
    if (out) out->assign(dst, dst + usize);
    free(dst);
  }
  free(f);
  return rc;
}

// 0 if the frame decodes; the mutations only have to stay inside their buffers
static int check_frame_file(const std::vector<uint8_t> &frame, long *mutations, long *rejected) {
  std::vector<uint8_t> plain;
  if (decode_exact(frame, &plain) != HL_OK) return 1;
  const size_t len = frame.size(), block = len - MC_LZ4C_HEADER;
  auto mutated = [&](std::vector<uint8_t> m) {
    ++*mutations;
    if (decode_exact(m, nullptr) != HL_OK) ++*rejected;
  };
  const uint32_t word = mc_lz4_le32(frame.data());
  for (uint32_t w : {0u, 1u, word - 1, word + 1, word / 2, word * 2, 0x3fffffffu, 0x40000000u, 0x80000000u, 0xffffffffu}) {
    std::vector<uint8_t> m = frame;
    mc_lz4e_put32(m.data(), w);
    mutated(m);
  }
  for (size_t k = 0; k < 200 && k < block; ++k) {  // tokens, extension bytes, offsets, literals: whatever is there
    const size_t at = MC_LZ4C_HEADER + (k * 37) % block;
    for (int v : {0x00, 0xFF, frame[at] ^ 0x10, frame[at] ^ 0x01, (frame[at] + 1) & 0xFF}) {
      std::vector<uint8_t> m = frame;
      m[at] = (uint8_t)v;
      mutated(m);
    }
  }
  for (size_t cut = 0; cut < len; cut += len / 64 + 1) mutated(std::vector<uint8_t>(frame.begin(), frame.begin() + cut));
  mutated(std::vector<uint8_t>(frame.begin(), frame.end() - 1));
  return 0;
}

int main(int argc, char **argv) {
  std::vector<std::string> inputs, frames;
  for (int a = 1; a < argc; ++a)
    for (auto &e : fs::recursive_directory_iterator(argv[a])) {
      if (!e.is_regular_file()) continue;
      if (e.path().extension().string() == ".bin") inputs.push_back(e.path().string());
      if (e.path().extension().string() == ".dat") frames.push_back(e.path().string());
    }
  std::sort(inputs.begin(), inputs.end());
  std::sort(frames.begin(), frames.end());
  auto slurp = [](const std::string &fn) {
    std::ifstream in(fn, std::ios::binary);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  };
  long chunks = 0, mutations = 0, rejected = 0, failures = 0;
  for (const std::string &fn : inputs) {
    ++chunks;
    if (const int bad = check_chunk(slurp(fn))) fprintf(stderr, "%s: mismatch %d\n", fn.c_str(), bad), ++failures;
  }
  for (int k = 0; k < 120; ++k) {
    ++chunks;
    const std::vector<uint8_t> in = generated(k);
    if (const int bad = check_chunk(in)) fprintf(stderr, "generated %d (%zu bytes): mismatch %d\n", k, in.size(), bad), ++failures;
  }
  for (const std::string &fn : frames)
    if (check_frame_file(slurp(fn), &mutations, &rejected)) fprintf(stderr, "%s: does not decode\n", fn.c_str()), ++failures;
  printf("chunks %ld files %zu frames %zu mutations %ld rejected %ld failures %ld\n", chunks, inputs.size(),
         frames.size(), mutations, rejected, failures);
  return failures == 0 ? 0 : 1;
}
