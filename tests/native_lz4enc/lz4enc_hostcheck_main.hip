// lz4enc_hostcheck_main DIR [DIR ...]: encode every input file (*.bin) under
// the directories, and 200 seeded generated inputs of 0-20000 bytes, with the
// product's scalar LZ4 encoder (csrc/mc_lz4_enc.h) into a heap buffer of
// exactly `cap` bytes, decode each result with lz4_decode_stream
// (csrc/mc_lz4.h) and compare; then the same inputs as whole frames (split
// and unsplit) into slots of exactly nbytes + 16 bytes, decoded by the shared
// plan walker.  Built with -fsanitize=address,undefined: a write at or past
// dst + cap, or a read outside the source, ends the run.  Exit 0 only if
// nothing differed.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <filesystem>
#include <fstream>
#include <string>

#include "../native_lz4/blosc_host.h"
#include "blosc_enc_host.h"

namespace fs = std::filesystem;

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {  // xorshift64*
  rng_state ^= rng_state >> 12, rng_state ^= rng_state << 25, rng_state ^= rng_state >> 27;
  return (uint32_t)((rng_state * 0x2545f4914f6cdd1dull) >> 32);
}

static std::vector<uint8_t> generated(int k) {
  const uint32_t n = k < 16 ? (uint32_t)k : rnd() % 20001;
  std::vector<uint8_t> v(n);
  switch (k % 5) {
    case 0: for (auto &b : v) b = (uint8_t)rnd(); break;                 // noise
    case 1: for (auto &b : v) b = (uint8_t)(rnd() % 3); break;           // small alphabet
    case 2: {                                                            // runs
      uint8_t cur = 0;
      for (auto &b : v) { if (rnd() % 97 == 0) cur = (uint8_t)rnd(); b = cur; }
      break;
    }
    case 3: {                                                            // copies of earlier chunks
      for (uint32_t i = 0; i < n;) {
        const uint32_t len = 1 + rnd() % 300;
        if (i > 8 && rnd() % 2) {
          const uint32_t from = rnd() % i;
          for (uint32_t j = 0; j < len && i < n; ++j, ++i) v[i] = v[from + j];
        } else {
          for (uint32_t j = 0; j < len && i < n; ++j, ++i) v[i] = (uint8_t)rnd();
        }
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

// 0 if the stream round-trips (or is stored raw)
static int check_stream(const std::vector<uint8_t> &in, long *raw, long *packed) {
  const uint32_t n = (uint32_t)in.size();
  uint8_t *src = exact(n), *dst = exact(n);
  if (n) memcpy(src, in.data(), n);
  const uint32_t cs = mc_lz4_encode_stream(src, n, dst, n);
  int bad = 0;
  if (cs == 0) {
    ++*raw;
  } else if (cs >= n) {
    bad = 1;
  } else {
    ++*packed;
    uint8_t *comp = exact(cs), *back = exact(n);
    memcpy(comp, dst, cs);
    bad = lz4_decode_stream(comp, cs, back, n) != MC_LZ4_OK || memcmp(back, src, n) != 0;
    free(comp), free(back);
  }
  free(src), free(dst);
  return bad;
}

// 0 if the frame of `in` (taken as already filtered) decodes back to it
static int check_frame(const std::vector<uint8_t> &in, uint32_t typesize, uint32_t blocksize, uint32_t flags) {
  const uint32_t n = (uint32_t)in.size();
  if (n == 0) return 0;
  uint8_t *src = exact(n), *slot = exact((size_t)n + 16), *back = exact(n);
  memcpy(src, in.data(), n);
  const long cb = he_encode_frame(src, src, n, typesize, blocksize, flags, slot, (size_t)n + 16);
  int bad = cb < 16 || cb > (long)n + 16;
  if (!bad) {
    uint8_t *frame = exact((size_t)cb);
    memcpy(frame, slot, (size_t)cb);
    hc_info info;
    bad = hc_decode(frame, (size_t)cb, back, n, &info) != HC_OK || memcmp(back, src, n) != 0;
    free(frame);
  }
  free(src), free(slot), free(back);
  return bad;
}

int main(int argc, char **argv) {
  std::vector<std::string> files;
  for (int a = 1; a < argc; ++a)
    for (auto &e : fs::recursive_directory_iterator(argv[a]))
      if (e.is_regular_file() && e.path().extension().string() == ".bin") files.push_back(e.path().string());
  std::sort(files.begin(), files.end());
  long inputs = 0, raw = 0, packed = 0, failures = 0;
  auto run = [&](const std::vector<uint8_t> &in, const char *what) {
    ++inputs;
    int bad = check_stream(in, &raw, &packed);
    const uint32_t n = (uint32_t)in.size();
    const uint32_t bs = n >= 2048 ? 1024 : (n ? n : 1);
    bad |= check_frame(in, 4, bs / 4 * 4 ? bs / 4 * 4 : bs, 0x20u) << 1;       // split where it can be
    bad |= check_frame(in, 1, bs, 0x20u | MC_BLOSC_F_NOSPLIT) << 2;             // one stream per block
    bad |= check_frame(in, 4, bs, 0x20u | MC_BLOSC_F_MEMCPYED) << 3;            // forced stored
    if (bad) {
      fprintf(stderr, "%s (%u bytes): mismatch %d\n", what, n, bad);
      ++failures;
    }
  };
  for (const std::string &fn : files) {
    std::ifstream in(fn, std::ios::binary);
    std::vector<uint8_t> data((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    run(data, fn.c_str());
  }
  for (int k = 0; k < 200; ++k) {
    char name[32];
    snprintf(name, sizeof(name), "generated %d", k);
    run(generated(k), name);
  }
  printf("inputs %ld files %zu raw %ld packed %ld failures %ld\n", inputs, files.size(), raw, packed, failures);
  return failures == 0 ? 0 : 1;
}
