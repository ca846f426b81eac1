// zstd_hostcheck_main PATH [PATH ...]: built with -fsanitize=address,undefined,
// as a process of its own.  Every frame file given (a directory stands for the
// *.zst and *.dat files under it) goes through the scalar model of
// csrc/mc_zstd.h from a heap copy of exactly its length:
//   * counted (no destination), then decoded into a heap buffer of exactly the
//     counted size; NAME.out beside a frame holds the bytes it must give, a
//     NAME.zst without one must be refused, a *.dat must decode;
//   * a frame that decodes is decoded again into one byte less, which must be
//     refused as exceeding the capacity;
//   * then under truncations and single-byte changes, each counted and decoded
//     into exactly its own counted size: such a frame may decode or be
//     refused, but a read outside the frame or a write outside the
//     destination ends the run.
// Exit 0 only if nothing differed.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <filesystem>
#include <fstream>
#include <string>
#include <vector>

#include "../../numcodecs_amd/csrc/mc_zstd.h"

namespace fs = std::filesystem;

static mc_zstd_tables tables;

static uint8_t *exact(size_t n) { return (uint8_t *)malloc(n ? n : 1); }

// count, then decode into exactly the counted size; the decode's result code
static int decode_exact(const std::vector<uint8_t> &frame, std::vector<uint8_t> *out, long *bad) {
  const size_t len = frame.size();
  uint8_t *f = exact(len);
  if (len) memcpy(f, frame.data(), len);
  uint8_t *lit = exact(MC_ZSTD_BLOCK_MAX);
  uint32_t counted = 0, produced = 0, word = 0;
  const int ce = mc_zstd_decode_frame(f, len, nullptr, MC_ZSTD_MAX_BYTES - 1, nullptr, &counted, &word, &tables);
  uint8_t *dst = exact(counted);
  const int e = mc_zstd_decode_frame(f, len, dst, counted, lit, &produced, &word, &tables);
  // the two modes walk the same blocks: where counting was refused the decode is, with no more bytes
  if (produced > counted) ++*bad;
  if (ce != MC_ZSTD_OK && e == MC_ZSTD_OK) ++*bad;
  if (e == MC_ZSTD_OK && produced != counted) ++*bad;
  if (out) out->assign(dst, dst + produced);
  if (e == MC_ZSTD_OK && counted > 0) {
    uint8_t *small = exact(counted - 1);
    if (mc_zstd_decode_frame(f, len, small, counted - 1, lit, &produced, &word, &tables) != MC_ZSTD_E_CAPACITY) ++*bad;
    free(small);
  }
  free(dst), free(lit), free(f);
  return e;
}

int main(int argc, char **argv) {
  std::vector<std::string> frames;
  auto wanted = [](const fs::path &p) { return p.extension() == ".zst" || p.extension() == ".dat"; };
  for (int a = 1; a < argc; ++a) {
    if (fs::is_directory(argv[a])) {
      for (auto &e : fs::recursive_directory_iterator(argv[a]))
        if (e.is_regular_file() && wanted(e.path())) frames.push_back(e.path().string());
    } else {
      frames.push_back(argv[a]);
    }
  }
  std::sort(frames.begin(), frames.end());
  auto slurp = [](const std::string &fn) {
    std::ifstream in(fn, std::ios::binary);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  };
  long accepted = 0, refused = 0, mutations = 0, mut_refused = 0, failures = 0;
  for (const std::string &path : frames) {
    const std::vector<uint8_t> frame = slurp(path);
    std::vector<uint8_t> got;
    long bad = 0;
    const int e = decode_exact(frame, &got, &bad);
    const bool fixture = fs::path(path).extension() == ".dat";
    const std::string want_fn = path + ".out";
    const bool has_out = fs::exists(want_fn);
    if (e == MC_ZSTD_OK) ++accepted; else ++refused;
    if (bad) fprintf(stderr, "%s: the two modes disagree\n", path.c_str()), ++failures;
    if (has_out) {
      if (e != MC_ZSTD_OK || got != slurp(want_fn)) fprintf(stderr, "%s: error %d or wrong bytes\n", path.c_str(), e), ++failures;
    } else if (fixture) {
      if (e != MC_ZSTD_OK) fprintf(stderr, "%s: error %d\n", path.c_str(), e), ++failures;
    } else if (e == MC_ZSTD_OK) {
      fprintf(stderr, "%s: accepted, must be refused\n", path.c_str()), ++failures;
    }
    // mutations: bounded work per frame
    const size_t len = frame.size();
    auto mutated = [&](const std::vector<uint8_t> &m) {
      long b = 0;
      ++mutations;
      if (decode_exact(m, nullptr, &b) != MC_ZSTD_OK) ++mut_refused;
      if (b) fprintf(stderr, "%s: a mutation's two modes disagree\n", path.c_str()), ++failures;
    };
    if (len == 0 || len > (1u << 17)) continue;  // the long frames are covered by their plain decode
    const size_t nmut = len < 32 ? len : 32;
    for (size_t k = 0; k < nmut; ++k) {
      const size_t at = k < 16 ? k % len : (k * 37 + len / 2) % len;  // the headers, then the entropy data
      for (int v : {frame[at] ^ 0x01, frame[at] ^ 0x80, 0xFF}) {
        std::vector<uint8_t> m = frame;
        m[at] = (uint8_t)v;
        mutated(m);
      }
    }
    for (size_t cut = 0; cut < len; cut += len / 12 + 1) mutated(std::vector<uint8_t>(frame.begin(), frame.begin() + cut));
    mutated(std::vector<uint8_t>(frame.begin(), frame.end() - 1));
  }
  printf("frames %zu accepted %ld refused %ld mutations %ld rejected %ld failures %ld\n", frames.size(), accepted,
         refused, mutations, mut_refused, failures);
  return failures == 0 ? 0 : 1;
}
