// bz2_hostcheck_main DIR [DIR ...]: built with -fsanitize=address,undefined, as
// a process of its own.  Every frame file under the directories (*.bz2, and
// the fixtures' *.dat) goes through the scalar model of csrc/mc_bz2.h from a
// heap copy of exactly its length, with a work area of exactly 5 * 100000 *
// its level bytes:
//   * counted (no destination), then decoded into a heap buffer of exactly the
//     counted size; NAME.out beside a frame holds the bytes it must give, a
//     frame without one (NAME.bz2 only) must be refused, in both modes with
//     the same code;
//   * a frame that decodes is decoded again into one byte less, which must be
//     refused as exceeding the capacity;
//   * then under truncations and single-byte changes, each counted and decoded
//     into exactly its own counted size: such a frame may decode or be
//     refused, but a read outside the frame or the work area, or a write
//     outside the destination, ends the run.
// Exit 0 only if nothing differed.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <filesystem>
#include <fstream>
#include <string>
#include <vector>

#include "../../numcodecs_amd/csrc/mc_bz2.h"

namespace fs = std::filesystem;

static mc_bz2_tables tables;

static uint8_t *exact(size_t n) { return (uint8_t *)malloc(n ? n : 1); }

// count, then decode into exactly the counted size; the decode's result code
static int decode_exact(const std::vector<uint8_t> &frame, std::vector<uint8_t> *out, long *bad) {
  const size_t len = frame.size();
  uint8_t *f = exact(len);
  if (len) memcpy(f, frame.data(), len);
  uint32_t level = 0, empty = 0;
  if (mc_bz2_parse_header(f, len, &level, &empty) != MC_BZ2_OK || level == 0) level = 1;
  void *work = malloc(5u * (size_t)MC_BZ2_BLOCK_UNIT * level);
  uint32_t counted = 0, produced = 0, word = 0;
  const int ce = mc_bz2_decode_stream(f, len, nullptr, MC_BZ2_MAX_BYTES - 1, &counted, &word, &tables, work, level);
  uint8_t *dst = exact(counted);
  const int e = mc_bz2_decode_stream(f, len, dst, counted, &produced, &word, &tables, work, level);
  // the two modes walk the same chain: same bytes, same verdict
  if (produced != counted || e != ce) ++*bad;
  if (out) out->assign(dst, dst + produced);
  if (e == MC_BZ2_OK && counted > 0) {
    uint8_t *small = exact(counted - 1);
    if (mc_bz2_decode_stream(f, len, small, counted - 1, &produced, &word, &tables, work, level) != MC_BZ2_E_CAPACITY)
      ++*bad;
    free(small);
  }
  free(dst), free(work), free(f);
  return e;
}

int main(int argc, char **argv) {
  std::vector<std::string> frames;
  for (int a = 1; a < argc; ++a)
    for (auto &e : fs::recursive_directory_iterator(argv[a])) {
      if (!e.is_regular_file()) continue;
      const std::string ext = e.path().extension().string();
      if (ext == ".bz2" || ext == ".dat") frames.push_back(e.path().string());
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
    if (e == MC_BZ2_OK) ++accepted; else ++refused;
    if (bad) fprintf(stderr, "%s: the two modes disagree\n", path.c_str()), ++failures;
    if (has_out) {
      if (e != MC_BZ2_OK || got != slurp(want_fn)) fprintf(stderr, "%s: error %d or wrong bytes\n", path.c_str(), e), ++failures;
    } else if (fixture) {
      if (e != MC_BZ2_OK) fprintf(stderr, "%s: error %d\n", path.c_str(), e), ++failures;
    } else if (e == MC_BZ2_OK) {
      fprintf(stderr, "%s: accepted, must be refused\n", path.c_str()), ++failures;
    }
    // mutations: bounded work per frame
    const size_t len = frame.size();
    auto mutated = [&](const std::vector<uint8_t> &m) {
      long b = 0;
      ++mutations;
      if (decode_exact(m, nullptr, &b) != MC_BZ2_OK) ++mut_refused;
      if (b) fprintf(stderr, "%s: a mutation's two modes disagree\n", path.c_str()), ++failures;
    };
    if (len == 0 || len > (1u << 14)) continue;  // the long frames are covered by their plain decode
    const size_t nmut = len < 24 ? len : 24;
    for (size_t k = 0; k < nmut; ++k) {
      const size_t at = (k * 37 + (k < 12 ? 0 : len / 2)) % len;
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
