// bz2_enc_hostcheck_main DIR [DIR ...]: built with -fsanitize=address,undefined,
// as a process of its own.  Every case file under the directories (NAME.L.bin:
// the input, L the level) goes through the scalar model of csrc/mc_bz2_enc.h
// from a heap copy of exactly its length:
//   * into a heap destination of exactly mc_bz2_enc_bound bytes, then again
//     into one of exactly the frame's length (the same bytes), then into one a
//     byte shorter, which must be refused with the destination untouched;
//   * the frame is decoded with csrc/mc_bz2.h's scalar decoder into exactly
//     the input's length and compared with the input.
// Exit 0 only if nothing differed.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <filesystem>
#include <fstream>
#include <string>
#include <vector>

#include "../../numcodecs_amd/csrc/mc_bz2_enc.h"

namespace fs = std::filesystem;

static mc_bz2_tables tables;

static uint8_t *exact(size_t n) { return (uint8_t *)malloc(n ? n : 1); }

int main(int argc, char **argv) {
  std::vector<std::string> cases;
  for (int a = 1; a < argc; ++a)
    for (auto &e : fs::recursive_directory_iterator(argv[a]))
      if (e.is_regular_file() && e.path().extension() == ".bin") cases.push_back(e.path().string());
  std::sort(cases.begin(), cases.end());
  long failures = 0;
  mc_bz2e_census census = {0, 0, 0, 0, 0};
  uint64_t in_bytes = 0, out_bytes = 0;
  for (const std::string &path : cases) {
    std::ifstream in(path, std::ios::binary);
    const std::vector<uint8_t> data((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    const std::string stem = fs::path(path).stem().string();  // NAME.L
    const uint32_t level = (uint32_t)(stem.back() - '0');
    if (level < 1 || level > 9) {
      fprintf(stderr, "%s: no level in the name\n", path.c_str()), ++failures;
      continue;
    }
    const size_t n = data.size();
    uint8_t *src = exact(n);
    if (n) memcpy(src, data.data(), n);
    const size_t bound = (size_t)mc_bz2_enc_bound(n, level);
    uint8_t *wide = exact(bound);
    int err = 0;
    const size_t size = (size_t)mc_bz2_encode_chunk(src, n, wide, bound, level, &err, &census);
    if (err || size == 0 || size > bound) {
      fprintf(stderr, "%s: error %d, size %zu, bound %zu\n", path.c_str(), err, size, bound), ++failures;
      free(wide), free(src);
      continue;
    }
    in_bytes += n, out_bytes += size;
    uint8_t *tight = exact(size);
    if ((size_t)mc_bz2_encode_chunk(src, n, tight, size, level, &err, nullptr) != size || err || memcmp(tight, wide, size))
      fprintf(stderr, "%s: the exactly sized destination differs\n", path.c_str()), ++failures;
    uint8_t *small = exact(size - 1);
    memset(small, 0xa5, size - 1);
    if (mc_bz2_encode_chunk(src, n, small, size - 1, level, &err, nullptr) != 0 || err != MC_BZ2E_E_SPACE)
      fprintf(stderr, "%s: a short destination was not refused\n", path.c_str()), ++failures;
    for (size_t i = 0; i + 1 < size; ++i)
      if (small[i] != 0xa5) {
        fprintf(stderr, "%s: a refused destination was written\n", path.c_str()), ++failures;
        break;
      }
    void *work = malloc(5u * (size_t)MC_BZ2_BLOCK_UNIT * level);
    uint8_t *back = exact(n);
    uint32_t produced = 0, word = 0;
    const int e = mc_bz2_decode_stream(tight, size, back, (uint32_t)n, &produced, &word, &tables, work, level);
    if (e != MC_BZ2_OK || produced != n || (n && memcmp(back, src, n)))
      fprintf(stderr, "%s: decodes with error %d to %u bytes\n", path.c_str(), e, produced), ++failures;
    free(back), free(work), free(small), free(tight), free(wide), free(src);
  }
  printf("cases %zu blocks %llu fallback %llu multi_table %llu rounds_max %llu in %llu out %llu failures %ld\n", cases.size(),
         (unsigned long long)census.blocks, (unsigned long long)census.fallback, (unsigned long long)census.multi_table,
         (unsigned long long)census.rounds_max, (unsigned long long)in_bytes, (unsigned long long)out_bytes, failures);
  return failures == 0 ? 0 : 1;
}
