// blosc_z_hostcheck_main PATH [PATH ...]: built with -fsanitize=address,undefined,
// as a process of its own.  Every frame file given (a directory stands for the
// *.dat and *.frame files under it) goes through the host model of
// blosc_z_host.h from a heap copy of exactly its length into a heap
// destination of exactly nbytes (every stream from a copy of exactly its own
// length, its literals into exactly min(share, 128 KiB) bytes):
//   * NAME.out beside a frame holds the still-filtered bytes it must give, a
//     NAME.code the code it must be refused with; a *.dat (a fixture frame of
//     the reference) must decode;
//   * then under truncations (the header's cbytes patched to match) and
//     single-byte changes: such a frame may decode or be refused, but a read
//     outside the frame or a write outside the destination ends the run.
//   * every frame that decodes is encoded again from its still-filtered bytes
//     as a cname='zstd' frame (one block, and blocks of 256, 4096 and 65537
//     bytes), from exactly sized heap copies, and must decode back to them.
// Exit 0 only if nothing differed.
#include <stdio.h>

#include <algorithm>
#include <filesystem>
#include <fstream>
#include <string>

#include "blosc_z_host.h"

namespace fs = std::filesystem;

static int decode_exact(const std::vector<uint8_t> &frame, std::vector<uint8_t> *out) {
  const size_t len = frame.size();
  uint8_t *f = (uint8_t *)malloc(len ? len : 1);
  if (len) memcpy(f, frame.data(), len);
  size_t nbytes = len >= 16 ? mc_lz4_le32(f + 4) : 0;
  if (nbytes > (1u << 26)) nbytes = 0;  // (a mutated size field: refused as too small)
  uint8_t *dst = (uint8_t *)malloc(nbytes ? nbytes : 1);
  const int e = hcz_decode(f, len, dst, nbytes, nullptr);
  if (out) out->assign(dst, dst + (e == HCZ_OK ? nbytes : 0));
  free(dst), free(f);
  return e;
}

int main(int argc, char **argv) {
  std::vector<std::string> frames;
  auto wanted = [](const fs::path &p) { return p.extension() == ".dat" || p.extension() == ".frame"; };
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
  long accepted = 0, refused = 0, mutations = 0, mut_refused = 0, failures = 0, encoded = 0;
  for (const std::string &path : frames) {
    const std::vector<uint8_t> frame = slurp(path);
    std::vector<uint8_t> got;
    const int e = decode_exact(frame, &got);
    if (e == HCZ_OK) ++accepted; else ++refused;
    const std::string out_fn = path + ".out", code_fn = path + ".code";
    if (fs::exists(out_fn)) {
      if (e != HCZ_OK || got != slurp(out_fn)) fprintf(stderr, "%s: code %d or wrong bytes\n", path.c_str(), e), ++failures;
    } else if (fs::exists(code_fn)) {
      const std::vector<uint8_t> t = slurp(code_fn);
      const int want = atoi(std::string(t.begin(), t.end()).c_str());
      if (e != want) fprintf(stderr, "%s: code %d, not %d\n", path.c_str(), e, want), ++failures;
    } else if (e != HCZ_OK) {
      fprintf(stderr, "%s: code %d\n", path.c_str(), e), ++failures;
    }
    // the other direction: what decoded (still filtered) as a zstd frame from exactly sized heap copies, and back
    if (e == HCZ_OK && !got.empty() && frame.size() >= 16) {
      const uint32_t n = (uint32_t)got.size(), ts = frame[3];
      for (uint32_t bs : {n, 256u, 4096u, 65536u + 1u}) {
        if (bs > n) continue;
        uint8_t *src = (uint8_t *)malloc(n), *out = (uint8_t *)malloc((size_t)n + 16), *back = (uint8_t *)malloc(n);
        memcpy(src, got.data(), n);
        const uint32_t flags = (MC_BLOSC_FMT_ZSTD << 5) | MC_BLOSC_F_NOSPLIT | (frame[2] & 5u);
        const long cb = hcz_encode_frame(src, src, n, ts, bs, flags, out, (size_t)n + 16);
        ++encoded;
        if (cb < 16 || cb > (long)n + 16 || hcz_decode(out, (size_t)cb, back, n, nullptr) != HCZ_OK ||
            ((out[2] & 2) ? memcmp(out + 16, src, n) : memcmp(back, src, n)))
          fprintf(stderr, "%s: encode with blocksize %u does not round-trip (%ld)\n", path.c_str(), bs, cb), ++failures;
        free(src), free(out), free(back);
      }
    }
    // mutations: bounded work per frame
    const size_t len = frame.size();
    if (len <= 16 || len > (1u << 17)) continue;  // the long frames are covered by their plain decode
    auto mutated = [&](std::vector<uint8_t> m) {
      const uint32_t l = (uint32_t)m.size();
      if (l >= 16) m[12] = (uint8_t)l, m[13] = (uint8_t)(l >> 8), m[14] = (uint8_t)(l >> 16), m[15] = (uint8_t)(l >> 24);
      ++mutations;
      if (decode_exact(m, nullptr) != HCZ_OK) ++mut_refused;
    };
    for (size_t k = 0; k < 48; ++k) {
      // the bstarts and the first stream's header, then the entropy data
      const size_t at = k < 24 ? 16 + k % (len - 16) : 16 + (k * 37 + len / 2) % (len - 16);
      for (int v : {frame[at] ^ 0x01, frame[at] ^ 0x80, 0xFF}) {
        std::vector<uint8_t> m = frame;
        m[at] = (uint8_t)v;
        mutated(m);
      }
    }
    for (size_t cut = 16; cut < len; cut += len / 12 + 1) mutated(std::vector<uint8_t>(frame.begin(), frame.begin() + cut));
    mutated(std::vector<uint8_t>(frame.begin(), frame.end() - 1));
  }
  printf("frames %zu accepted %ld refused %ld mutations %ld rejected %ld encoded %ld failures %ld\n", frames.size(),
         accepted, refused, mutations, mut_refused, encoded, failures);
  return failures == 0 ? 0 : 1;
}
