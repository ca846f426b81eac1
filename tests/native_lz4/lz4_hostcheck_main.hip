// lz4_hostcheck_main DIR [DIR ...]: decode every frame file (*.dat, *.frame)
// under the directories with the product's shared plan walker / LZ4 decoder
// (blosc_host.h), then a few hundred deterministic mutations of each: byte
// flips in the header, the bstarts table, the streams' cbytes words, tokens and
// offsets, plus truncations.  Built with -fsanitize=address,undefined: every
// buffer is allocated at its exact size, so a read outside the frame or a
// write outside the output ends the run.  Exit 0 only if every frame was
// decoded or reported unsupported and every mutation was decoded within bounds
// or rejected.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <filesystem>
#include <fstream>
#include <string>

#include "blosc_host.h"

namespace fs = std::filesystem;

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {  // xorshift64*
  rng_state ^= rng_state >> 12, rng_state ^= rng_state << 25, rng_state ^= rng_state >> 27;
  return (uint32_t)((rng_state * 0x2545f4914f6cdd1dull) >> 32);
}

static const size_t OUT_LIMIT = 8u << 20;  // a mutated header may ask for gigabytes: counted as rejected

// decode a private, exactly sized copy; returns hc_decode's status
static int decode_copy(const std::vector<uint8_t> &frame, long *too_big) {
  uint8_t *copy = (uint8_t *)malloc(frame.size() ? frame.size() : 1);
  if (frame.size()) memcpy(copy, frame.data(), frame.size());
  size_t nbytes = frame.size() >= 16 ? mc_lz4_le32(copy + 4) : 0;
  int rc;
  if (nbytes > OUT_LIMIT) {
    ++*too_big;
    rc = HC_REJECTED;
  } else {
    uint8_t *out = (uint8_t *)malloc(nbytes ? nbytes : 1);
    hc_info info;
    rc = hc_decode(copy, frame.size(), out, nbytes, &info);
    free(out);
  }
  free(copy);
  return rc;
}

int main(int argc, char **argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s DIR [DIR ...]\n", argv[0]);
    return 2;
  }
  std::vector<std::string> files;
  for (int a = 1; a < argc; ++a)
    for (auto &e : fs::recursive_directory_iterator(argv[a])) {
      const std::string ext = e.path().extension().string();
      if (e.is_regular_file() && (ext == ".dat" || ext == ".frame")) files.push_back(e.path().string());
    }
  std::sort(files.begin(), files.end());
  long decoded = 0, unsupported = 0, mutations = 0, accepted = 0, rejected = 0, too_big = 0, failures = 0;
  for (const std::string &fn : files) {
    std::ifstream in(fn, std::ios::binary);
    std::vector<uint8_t> frame((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    const int rc = decode_copy(frame, &too_big);
    if (rc == HC_UNSUPPORTED) {
      ++unsupported;
    } else if (rc == HC_OK) {
      ++decoded;
    } else {
      fprintf(stderr, "%s: a valid frame was rejected with %d\n", fn.c_str(), rc);
      ++failures;
      continue;
    }
    if (frame.size() < 16) continue;
    // where the interesting words are: header, bstarts, the cbytes words
    std::vector<size_t> spots;
    for (size_t i = 0; i < 16; ++i) spots.push_back(i);
    mc_blosc_frame f;
    if (hc_header(frame.data(), frame.size(), &f) == HC_OK && f.nbytes && !(f.flags & MC_BLOSC_F_MEMCPYED)) {
      const uint32_t nblocks = mc_blosc_nblocks(f.nbytes, f.blocksize);
      for (size_t i = 16; i < 16 + 4ull * nblocks && i < frame.size(); ++i) spots.push_back(i);
      for (uint32_t b = 0; b < nblocks && 20 + 4ull * b <= frame.size(); ++b) {
        size_t p = mc_lz4_le32(frame.data() + 16 + 4ull * b);
        const uint32_t bsize = mc_blosc_block_size(f.nbytes, f.blocksize, b);
        const uint32_t ns = mc_blosc_nsplit(f.flags, f.typesize, f.blocksize, bsize);
        for (uint32_t j = 0; j < ns && p + 4 <= frame.size(); ++j) {
          for (size_t i = p; i < p + 4; ++i) spots.push_back(i);
          // the first token and the bytes after it (first offset / extension bytes)
          for (size_t i = p + 4; i < p + 12 && i < frame.size(); ++i) spots.push_back(i);
          p += 4 + (size_t)mc_lz4_le32(frame.data() + p);
        }
      }
    }
    for (int m = 0; m < 320; ++m) {
      std::vector<uint8_t> mut(frame);
      const uint32_t kind = m % 8;
      if (kind == 7) {  // truncation (the header's cbytes then disagrees) ...
        mut.resize(rnd() % frame.size());
      } else if (kind == 6) {  // ... and one that keeps the header consistent
        mut.resize(16 + rnd() % (frame.size() - 15));
        const uint32_t n = (uint32_t)mut.size();
        for (int k = 0; k < 4; ++k) mut[12 + k] = (uint8_t)(n >> (8 * k));
      } else {
        const size_t at = (kind < 4) ? spots[rnd() % spots.size()] : rnd() % frame.size();
        const uint32_t r = rnd();
        mut[at] = (kind & 1) ? (uint8_t)(mut[at] ^ (1u << (r & 7))) : (uint8_t)(r >> 8);
      }
      const int mrc = decode_copy(mut, &too_big);
      ++mutations;
      if (mrc == HC_OK) ++accepted; else ++rejected;
      if (mrc >= 100) {
        fprintf(stderr, "%s: mutation %d left its bounds (%d)\n", fn.c_str(), m, mrc);
        ++failures;
      }
    }
  }
  printf("frames %zu decoded %ld unsupported %ld mutations %ld accepted %ld rejected %ld too_big %ld failures %ld\n",
         files.size(), decoded, unsupported, mutations, accepted, rejected, too_big, failures);
  return (failures == 0 && !files.empty()) ? 0 : 1;
}
