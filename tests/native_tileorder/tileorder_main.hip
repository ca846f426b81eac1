// tileorder_main.hip -- host check of the large-chunk tile order
// (mc_tile_steps / mc_tile_of_step, csrc/mc_shuffle.h).  For every ntiles in
// 1..NMAX and every R given (default: the R the variant word can select, plus
// a few that it cannot, since the map must hold for every R) it walks the
// steps exactly as MC_FOR_TILES does and prints one line per R:
//   R=<r> bijection=<ok|FAIL> identity=<ok|FAIL|->
// bijection: the steps whose image is < ntiles hit every tile of [0, ntiles)
// exactly once and no step's image is out of the step range; identity (R = 1
// only): step g takes tile g and there are ntiles steps.  Exit status 1 on
// any FAIL.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../numcodecs_amd/csrc/mc_shuffle.h"

int main(int argc, char **argv) {
  const size_t NMAX = 2048;
  std::vector<unsigned> rs;
  for (int i = 1; i < argc; ++i) rs.push_back((unsigned)std::strtoul(argv[i], nullptr, 10));
  if (rs.empty()) rs = {1, 8, 16, 32, 64, 128, 256, 2, 3, 5, 7, 100, 2047, 2048, 2049, 4096};
  bool all_ok = true;
  for (unsigned R : rs) {
    bool bij = true, ident = true;
    for (size_t ntiles = 1; ntiles <= NMAX; ++ntiles) {
      const size_t steps = mc_tile_steps(ntiles, R);
      if (steps < ntiles) bij = false;
      std::vector<unsigned char> seen(ntiles, 0);  // exactly sized: ASan sees an image past it
      size_t visited = 0;
      for (size_t g = 0; g < steps; ++g) {
        const size_t t = mc_tile_of_step(g, ntiles, R);
        if (R == 1 && t != g) ident = false;
        if (t >= ntiles) continue;  // a skipped step
        if (seen[t]) bij = false;
        seen[t] = 1;
        ++visited;
      }
      if (visited != ntiles) bij = false;
      if (R == 1 && steps != ntiles) ident = false;
    }
    std::printf("R=%u bijection=%s identity=%s\n", R, bij ? "ok" : "FAIL", R == 1 ? (ident ? "ok" : "FAIL") : "-");
    all_ok = all_ok && bij && ident;
  }
  return all_ok ? 0 : 1;
}
