// mc_shuffle.h -- tile geometry and quad I/O shared by the Shuffle kernels
// (mc_shuffle.hip) and the fused Shuffle+Fletcher32 chunk kernels
// (mc_fletcher.hip).
#pragma once

#include "mc_common.h"

template <int ES, int QMUL = 1>
struct Geom {
  static constexpr int Q = (ES >= 16 ? 2 : 4) * QMUL;  // quads per thread per tile
  static constexpr int TE = Q * 4 * MC_BLOCK;       // elements per tile
  static constexpr int TB = TE * ES;                // bytes per tile (either side)
  static constexpr int NV = TB / 16 / MC_BLOCK;     // 16-B units per thread per tile
  static constexpr int PU = TE / 16;                // 16-B units per plane per tile
};

struct ChunkMap {
  size_t count;            // elements per chunk
  size_t tiles_per_chunk;  // full tiles per chunk
  size_t src_stride;       // bytes between chunks (source)
  size_t dst_stride;       // bytes between chunks (destination)
  unsigned group;          // consecutive tiles a block takes per grid-stride step
  unsigned vrows;          // virtual rows of the tile order (1 = tiles in address order)
};

// Tile order of one large chunk ("virtual rows"): the chunk's tiles are cut
// into R runs of C = ceil(ntiles / R) consecutive tiles and the block steps
// walk the runs round-robin, so that the blocks in flight together work at R
// places of every plane stream, as they do on a batch of R rows.  Step g of
// mc_tile_steps(ntiles, R) takes tile (g % R) * C + g / R; a step whose image
// is >= ntiles has no tile and is skipped.  (r, k) -> r * C + k is one-to-one
// from [0, R) x [0, C) onto [0, R * C), which contains [0, ntiles), so the
// visited steps map one-to-one onto the tiles for every ntiles >= 1 and every
// R >= 1 (R > ntiles gives C = 1, the identity).  R = 1 is the identity.
// The arithmetic is 32-bit (one short division per tile, no 64-bit division
// routine in the kernels): ntiles + R must be below 2^32, which
// mc_shuffle_impl checks before it sets vrows > 1.
MC_HD size_t mc_tile_steps(size_t ntiles, unsigned vrows) {
  if (vrows <= 1) return ntiles;
  return (size_t)vrows * (((unsigned)ntiles + vrows - 1) / vrows);
}
MC_HD size_t mc_tile_of_step(size_t g, size_t ntiles, unsigned vrows) {
  if (vrows <= 1) return g;
  const unsigned c = ((unsigned)ntiles + vrows - 1) / vrows;
  return (size_t)((unsigned)g % vrows) * c + (unsigned)g / vrows;
}

// Tile schedule: tiles are taken in groups of m.group consecutive tiles, groups
// grid-strided over the blocks (group = 1 is a plain grid-stride loop).  With
// m.vrows > 1 (only with group = 1 and one chunk, mc_shuffle_impl) the steps
// take their tile from mc_tile_of_step.
#define MC_FOR_TILES(tile, ntiles, m)                                                          \
  for (size_t _g = blockIdx.x, _n = mc_tile_steps((ntiles), (m).vrows); _g * (m).group < _n;   \
       _g += gridDim.x)                                                                        \
    for (size_t tile = mc_tile_of_step(_g, (ntiles), (m).vrows) * (m).group,                   \
                _e = min((ntiles), tile + (m).group);                                          \
         tile < _e; ++tile)

// load / store the es dwords of one quad (16-B accesses where possible);
// NT selects nontemporal global accesses, LDS accesses use NT = false.
template <int ES, bool NT>
MC_DEV void load_quad(const uint8_t *p, uint32_t (&w)[ES]) {
  if constexpr (ES == 2) {
    const mc_u32x2 v = mc_ld8<NT>(p);
    w[0] = v.x; w[1] = v.y;
  } else {
#pragma unroll
    for (int k = 0; k < ES / 4; ++k) {
      const mc_u32x4 v = mc_ld16<NT>(p + 16 * k);
      w[4 * k] = v.x; w[4 * k + 1] = v.y; w[4 * k + 2] = v.z; w[4 * k + 3] = v.w;
    }
  }
}

template <int ES, bool NT>
MC_DEV void store_quad(uint8_t *p, const uint32_t (&w)[ES]) {
  if constexpr (ES == 2) {
    mc_st8<NT>(p, mc_u32x2{w[0], w[1]});
  } else {
#pragma unroll
    for (int k = 0; k < ES / 4; ++k)
      mc_st16<NT>(p + 16 * k, mc_u32x4{w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]});
  }
}

// Shared driver of every shuffle entry point (mc_shuffle.hip), also used by
// the fused Shuffle+Fletcher32 ops: variant 0 = the measured default schedule
// (the other layouts exist for the lab's sweeps, tools/lab); br != NULL fuses
// BitRound into the encode.
int mc_shuffle_impl(const void *src, size_t src_stride, void *dst, size_t dst_stride, size_t nchunks,
                    size_t chunk_bytes, size_t es, bool enc, int variant, int max_blocks, const McBitRound *br,
                    hipStream_t st);
