// mc_bz2.hip -- bzip2 streams decoded on the device, a whole batch per call.
// The rules (header, bit reader, block header, symbol loop, stream walker,
// trailer classification) are mc_bz2.h's, compiled for the host too
// (tests/native_bz2): the kernels run that very code and supply the wave
// worker below.
//
// plan:   one thread per frame: "BZh" and the level -> a stream record and any
//         header error.
// decode: a grid of at most MC_BZ2_WAVES waves (64-lane workgroups), each with
//         its own slice of the workspace (tt: 4 bytes a symbol, and a byte
//         column: 5 * 100000 * the batch's highest level in all), taking frames
//         from a counter and walking a frame's blocks in order.  Per block:
//   entropy  wave-uniform.  The bit buffer is the inflater's 64-bit buffer fed
//            from a register window of 64 dwords, MSB first.  The tables
//            (limit / base / perm per Huffman table, the selectors, the MTF
//            list, the byte histogram) are in LDS; table g is built by lane g.
//            A symbol is one ballot: lane l holds limit[l] and base[l] of the
//            current table and tests the code's first l bits.  An MTF move
//            shifts the list 64 entries a step.  A run is splatted wave-wide
//            into the byte column.
//   sort     64 symbols a step into tt[j] = i << 8 | byte: ranks within a step
//            from matching equal bytes across the wave (8 ballots), the
//            cumulative table in LDS.
//   inverse BWT  multi-start for blocks of MC_BZ2_MULTI_MIN symbols and more
//            (ibwt<true>), else the one-lane chase (ibwt<false>): every K-th
//            index of tt and origPtr are splitters (K a power of two, at most
//            2049 splitters); each lane walks from its splitters to the next
//            one, leaving length and successor in LDS; one walk over that table
//            from origPtr gives the offsets, until it is back at origPtr or
//            nblock steps are accounted for; each lane walks its sublists again
//            and stores the bytes at their places in the byte column.  A cycle
//            shorter than nblock is gone round again: the column repeats with
//            the cycle's period.  Splitters never reached are dropped.
//   RLE1 + CRC  64 bytes a step: where no four equal neighbours end in the
//            step (nor carried in), a straight copy; else the part up to the
//            fourth byte is copied and the count byte's run splatted.  The CRC
//            (MSB first) of a piece: lane l multiplies its byte by
//            x^(8 * bytes behind it) and the wave folds by exclusive or.
// STORE = false is the sizing pass: the same chain with no output stores.
// LDS per workgroup: 24.8 KiB of tables + 16 KiB of splitters: three
// workgroups share a CU.
#include "mc_common.h"
#include "mc_bz2.h"
#include "mc_lz4_wave.h"
#include "mc_inflate_wave.h"  // wave_dwords: the source window

namespace {

using namespace mc_infw;

constexpr uint32_t MC_BZ2_WAVES = 768;       // 3 workgroups x 256 CUs: what the LDS use allows
constexpr uint32_t MC_BZ2_MULTI_MIN = 2048;  // blocks below it take the one-lane chase
constexpr uint32_t SPLIT_MAX = 2048;         // regular splitters; origPtr may add one
constexpr uint32_t NONE = 0x7fffffffu, SEEN = 0x80000000u;

struct splitters {
  uint32_t len[SPLIT_MAX + 1];
  uint32_t next[SPLIT_MAX + 1];  // the successor's id; SEEN | offset once placed
};

MC_DEV void stage_order() { __syncthreads(); }  // one wave a workgroup: orders its LDS and global accesses

MC_DEV uint32_t wave_xor(uint32_t v) {
#pragma unroll
  for (int k = 1; k < (int)WAVE; k <<= 1) v ^= (uint32_t)__shfl_xor((int)v, k, WAVE);
  return v;
}

template <bool STORE>
struct wave_worker {
  uint8_t *col;
  uint32_t *tt;
  uint8_t *dst;
  splitters *sp;
  uint32_t cap, op, lane, multi_min;
  uint32_t pw;        // x^(8 * lane) mod P
  int32_t lim, bas;   // limit[lane], base[lane] of the current table
  uint32_t minlen;
  uint32_t crc;

  MC_DEV bool lead() const { return lane == 0; }
  MC_DEV void sync() { lds_order(); }
  MC_DEV uint32_t first() const { return lane; }
  MC_DEV uint32_t stride() const { return WAVE; }

  MC_DEV void group(const mc_bz2_tables *t, uint32_t g) {
    const uint32_t l = lane < 24u ? lane : 23u;
    lim = t->limit[g][l];
    bas = t->base[g][l];
    minlen = uni(t->minlen[g]);
  }
  template <class R>
  MC_DEV int symbol(R &br, const mc_bz2_tables *t, uint32_t g, uint32_t *sym) {
    const uint32_t peek21 = br.peek(21);
    const uint32_t bits = lane <= MC_BZ2_MAX_CODE_LEN ? lane : 0u;
    const bool hit = bits >= minlen && (int32_t)(peek21 >> (21u - bits)) <= lim;
    const uint64_t m = __ballot(hit);  // minlen >= 1: lane 0 never hits
    const uint32_t zn = m ? (uint32_t)__ffsll((long long)m) - 1u : 21u;
    const int32_t base_zn = __builtin_amdgcn_readlane(bas, (int)zn);
    return mc_bz2_take_symbol(br, t, g, zn, peek21, base_zn, sym);
  }
  MC_DEV uint32_t front(mc_bz2_tables *t, uint32_t nn) {  // nn <= 255
    const uint32_t v = uni(t->mtf[nn]);
    if (nn == 0) return v;
    uint32_t r[4];
#pragma unroll
    for (uint32_t c = 0; c < 4; ++c) {
      const uint32_t i = c * WAVE + lane;
      r[c] = i < nn ? t->mtf[i] : 0u;
    }
    lds_order();
#pragma unroll
    for (uint32_t c = 0; c < 4; ++c) {
      const uint32_t i = c * WAVE + lane;
      if (i < nn) t->mtf[i + 1] = (uint8_t)r[c];
    }
    if (lane == 0) t->mtf[0] = (uint8_t)v;
    lds_order();
    return v;
  }
  MC_DEV void emit(mc_bz2_tables *t, uint32_t at, uint32_t byte, uint32_t count) {  // at + count <= 100000 * level
    for (uint32_t k = lane; k < count; k += WAVE) col[at + k] = (uint8_t)byte;
    if (lane == 0) t->unzftab[byte] += count;
  }

  // ---- after the symbols ------------------------------------------------------
  MC_DEV void sort(mc_bz2_tables *t, uint32_t nblock) {
    if (lane == 0) {
      uint32_t sum = 0;
      for (uint32_t i = 0; i < 256; ++i) {
        const uint32_t c = t->unzftab[i];
        t->unzftab[i] = sum;
        sum += c;
      }
    }
    stage_order();  // the column's stores and the table
    const uint64_t below = (1ull << lane) - 1ull;
    for (uint32_t first = 0; first < nblock; first += WAVE) {
      const uint32_t i = first + lane;
      const bool valid = i < nblock;
      const uint32_t b = valid ? col[i] : 0u;
      uint64_t same = __ballot(valid);
#pragma unroll
      for (uint32_t k = 0; k < 8; ++k) {
        const uint64_t m = __ballot((b >> k) & 1u);
        same &= ((b >> k) & 1u) ? m : ~m;
      }
      // the histogram counted these very bytes: every slot is below nblock
      if (valid) tt[t->unzftab[b] + (uint32_t)__popcll(same & below)] = (i << 8) | b;
      lds_order();
      if (valid && (same & below) == 0) t->unzftab[b] += (uint32_t)__popcll(same);
      lds_order();
    }
    stage_order();
  }

  // the pre-RLE1 bytes of the block into col[0, nblock): exactly nblock steps from orig
  template <bool MULTI>
  MC_DEV void ibwt(uint32_t nblock, uint32_t orig) {
    if constexpr (!MULTI) {
      if (lane == 0) {
        uint32_t p = orig;
        for (uint32_t k = 0; k < nblock; ++k) {
          const uint32_t e = tt[p];  // p < nblock: a symbol index
          col[k] = (uint8_t)e;
          p = e >> 8;
        }
      }
    } else {
      uint32_t shift = 0;
      while (((nblock - 1u) >> shift) + 1u > SPLIT_MAX) ++shift;
      const uint32_t kmask = (1u << shift) - 1u, nreg = ((nblock - 1u) >> shift) + 1u;
      const bool extra = (orig & kmask) != 0;
      const uint32_t oid = extra ? nreg : orig >> shift, ns = nreg + (extra ? 1u : 0u);  // ns <= SPLIT_MAX + 1
      for (uint32_t s = lane; s < ns; s += WAVE) {
        uint32_t p = s == oid ? orig : s << shift, steps = 0;
        bool at_split;
        do {
          p = tt[p] >> 8;
          ++steps;
          at_split = (p & kmask) == 0 || p == orig;
        } while (!at_split && steps < nblock);
        sp->len[s] = steps;
        sp->next[s] = at_split ? (p == orig ? oid : p >> shift) : NONE;
      }
      lds_order();
      uint32_t s = oid, off = 0;
      for (uint32_t guard = 0; guard < ns; ++guard) {  // a splitter is placed once
        const uint32_t l = uni(sp->len[s]), nx = uni(sp->next[s]);
        lds_order();
        if (lane == 0) sp->next[s] = SEEN | off;
        off += l;
        s = nx;
        if (s == oid || s >= ns || off >= nblock) break;
      }
      lds_order();
      const uint32_t cycle = off < nblock ? off : nblock;
      for (uint32_t q = lane; q < ns; q += WAVE) {
        const uint32_t st = sp->next[q];
        if (!(st & SEEN)) continue;  // on a cycle the walk never reaches
        const uint32_t at = st & ~SEEN, l = sp->len[q];
        uint32_t p = q == oid ? orig : q << shift;
        for (uint32_t k = 0; k < l; ++k) {
          const uint32_t e = tt[p];
          if (at + k < nblock) col[at + k] = (uint8_t)e;
          p = e >> 8;
        }
      }
      if (cycle < nblock) {  // gone round again: col[i] = col[i mod cycle]
        stage_order();
        uint32_t ph = lane % cycle;
        const uint32_t step = WAVE % cycle;
        for (uint32_t i = cycle; i < nblock; i += WAVE) {
          if (i + lane < nblock) col[i + lane] = col[ph];
          ph += step;
          if (ph >= cycle) ph -= cycle;
        }
      }
    }
    stage_order();
  }

  // lanes [lo, hi) of a step give their byte b to the output and the CRC
  MC_DEV int put(uint32_t b, uint32_t lo, uint32_t hi) {
    const uint32_t n = hi - lo;
    if (n > cap - op) return MC_BZ2_E_CAPACITY;
    const bool mine = lane >= lo && lane < hi;
    if constexpr (STORE) {
      if (mine) dst[op + lane - lo] = (uint8_t)b;
    }
    // the register times x^(8 n), folded into the first byte's share
    uint32_t v = mine ? b << 24 : 0u;
    if (lane == lo) v ^= crc;
    v = mc_bz2_mulx(v, 8);
    const uint32_t p = (uint32_t)__shfl((int)pw, (int)((hi - 1u - lane) & 63u), WAVE);
    crc = wave_xor(mine ? mc_bz2_gfmul(v, p) : 0u);
    op += n;
    return MC_BZ2_OK;
  }

  MC_DEV int unrle(uint32_t nblock, uint32_t *crc_out) {
    crc = 0xffffffffu;
    uint32_t hist = 0, prevb = 0;  // equal bytes at the tail so far (< 4), and their value
    bool expect = false;           // the next byte is a count
    for (uint32_t first = 0; first < nblock; first += WAVE) {
      const uint32_t cnt = nblock - first < WAVE ? nblock - first : WAVE;
      const uint32_t b = lane < cnt ? col[first + lane] : 0u;
      const uint32_t left = (uint32_t)__shfl_up((int)b, 1, WAVE);
      uint32_t pos = 0;
      while (pos < cnt) {
        if (expect) {
          const uint32_t run = (uint32_t)__builtin_amdgcn_readlane((int)b, (int)pos);
          for (uint32_t k = 0; k < run; k += WAVE) {
            const int e = put(prevb, 0, run - k < WAVE ? run - k : WAVE);
            if (e != MC_BZ2_OK) return e;
          }
          expect = false, hist = 0, ++pos;
          continue;
        }
        // bit l: lane l's byte equals the one before it, from pos on
        const bool eq = lane < cnt && (lane > pos ? b == left : (lane == pos && hist > 0 && b == prevb));
        const uint64_t E = __ballot(eq);
        const uint64_t four = E & ((E << 1) | (hist >= 2u ? 1ull : 0ull)) & ((E << 2) | (hist >= 3u ? 3ull : hist == 2u ? 2ull : 0ull));
        if (four == 0) {
          const int e = put(b, pos, cnt);
          if (e != MC_BZ2_OK) return e;
          const uint64_t inside = cnt == WAVE ? ~0ull : (1ull << cnt) - 1ull;
          const uint64_t zeros = ~E & inside;
          if (zeros == 0) hist += cnt;  // every byte equals the carried one
          else hist = cnt - (63u - (uint32_t)__builtin_clzll(zeros));
          prevb = (uint32_t)__builtin_amdgcn_readlane((int)b, (int)(cnt - 1u));
          pos = cnt;
        } else {
          const uint32_t f = (uint32_t)__ffsll((long long)four) - 1u;  // the fourth equal byte
          const int e = put(b, pos, f + 1u);
          if (e != MC_BZ2_OK) return e;
          prevb = (uint32_t)__builtin_amdgcn_readlane((int)b, (int)f);
          expect = true, pos = f + 1u;
        }
      }
    }
    if (expect) return MC_BZ2_E_RLE;
    *crc_out = ~crc;
    return MC_BZ2_OK;
  }

  MC_DEV int finish(mc_bz2_tables *t, uint32_t nblock, uint32_t orig, uint32_t *crc_out) {
    sort(t, nblock);
    if (nblock >= multi_min) ibwt<true>(nblock, orig);
    else ibwt<false>(nblock, orig);
    return unrle(nblock, crc_out);
  }
};

__global__ void __launch_bounds__(MC_BLOCK)
bz2_plan_kernel(const uint8_t *__restrict__ frames, const mc_bz2_frame *__restrict__ table, uint32_t nframes,
                uint32_t sizing, uint32_t max_level, mc_bz2_stream *__restrict__ streams, uint32_t *__restrict__ produced,
                int32_t *__restrict__ err) {
  const uint32_t i = blockIdx.x * MC_BLOCK + threadIdx.x;
  if (i >= nframes) return;
  const mc_bz2_frame r = table[i];
  mc_bz2_stream s;
  s.src_off = r.src_off, s.dst = r.dst, s.src_len = 0, s.level = 0, s.capacity = r.capacity, s.flags = 0;
  int e;
  uint32_t empty = 0;
  if (r.src_len >= MC_BZ2_MAX_BYTES || r.capacity >= MC_BZ2_MAX_BYTES || (!sizing && r.capacity && !r.dst)) {
    e = MC_BZ2_E_TABLE;
  } else {
    s.src_len = (uint32_t)r.src_len;
    e = mc_bz2_parse_header(frames + r.src_off, r.src_len, &s.level, &empty);
    if (e == MC_BZ2_OK && s.level > max_level) e = MC_BZ2_E_TABLE;  // the workspace is sized for max_level
  }
  if (e == MC_BZ2_OK) s.flags = empty ? MC_BZ2_S_EMPTY : MC_BZ2_S_VALID;
  streams[i] = s;
  produced[i] = 0;
  if (e != MC_BZ2_OK) err[2 * i] = e, err[2 * i + 1] = 0;
}

template <bool STORE>
__global__ void __launch_bounds__(WAVE)
bz2_decode_kernel(const uint8_t *__restrict__ frames, const mc_bz2_stream *__restrict__ streams, uint32_t nframes,
                  uint32_t max_level, uint32_t multi_min, uint32_t *__restrict__ counter, uint8_t *__restrict__ work,
                  uint32_t *__restrict__ produced, int32_t *__restrict__ err) {
  __shared__ mc_bz2_tables T;
  __shared__ splitters SP;
  __shared__ uint32_t taken;
  const uint32_t lane = threadIdx.x;
  const size_t symbols = (size_t)MC_BZ2_BLOCK_UNIT * max_level;
  uint8_t *mine = work + (size_t)blockIdx.x * 5u * symbols;  // this wave's slice: tt, then the byte column
  wave_worker<STORE> w;
  w.tt = reinterpret_cast<uint32_t *>(mine);
  w.col = mine + 4u * symbols;
  w.sp = &SP;
  w.lane = lane, w.multi_min = multi_min;
  w.pw = mc_bz2_mulx(1u, 8u * lane);
  w.lim = w.bas = 0, w.minlen = 1, w.crc = 0;
  for (;;) {
    if (lane == 0) taken = atomicAdd(counter, 1u);
    stage_order();
    const uint32_t i = uni(taken);
    stage_order();
    if (i >= nframes) return;
    const mc_bz2_stream d = streams[i];
    if (!(d.flags & MC_BZ2_S_VALID)) continue;
    const uint8_t *f = mc_uniform_ptr(frames + d.src_off);
    const uint32_t n = uni(d.src_len), level = uni(d.level);  // level <= max_level: the plan's check
    wave_dwords src{f, n, lane, 0u, 0u, 0u};
    src.start(1);
    mc_bz2_bits<wave_dwords> br(src, n);
    br.seek_byte(4);
    w.dst = mc_uniform_ptr(reinterpret_cast<uint8_t *>((uintptr_t)d.dst));
    w.cap = STORE ? uni(d.capacity) : MC_BZ2_MAX_BYTES - 1u;
    w.op = 0;
    uint32_t blocks = 0;
    int e = (int)uni((uint32_t)mc_bz2_blocks(br, &T, w, level, &blocks));
    if (e == MC_BZ2_OK) e = mc_bz2_after(f, n, (br.pos + 7u) >> 3);
    if (lane == 0) {  // one wave per frame: no other writer
      produced[i] = w.op;
      if (e != MC_BZ2_OK) err[2 * i] = e, err[2 * i + 1] = (int32_t)blocks;
    }
  }
}

constexpr size_t WS_ALIGN = 256;
size_t head_bytes(size_t nframes) {
  return (nframes * sizeof(mc_bz2_stream) + 16 + WS_ALIGN - 1) / WS_ALIGN * WS_ALIGN;
}
size_t grid_waves(size_t nframes) { return nframes < MC_BZ2_WAVES ? nframes : MC_BZ2_WAVES; }

template <bool STORE>
int run(const void *frames, const void *table, size_t nframes, unsigned max_level, unsigned multi_min, void *ws,
        size_t ws_bytes, uint32_t *out, int32_t *err, mc_stream_t stream) {
  if (nframes == 0) return MC_OK;
  if (!frames || !table || !ws || !out || !err) return MC_EINVAL;
  if (nframes > 0x7fffffffu || max_level < 1 || max_level > 9) return MC_EINVAL;
  if (((uintptr_t)ws & 7) || ((uintptr_t)table & 7) || ((uintptr_t)err & 3) || ((uintptr_t)out & 3)) return MC_EINVAL;
  if (ws_bytes < mc_bz2_workspace(nframes, max_level)) return MC_ENOSPC;
  hipStream_t st = (hipStream_t)stream;
  int rc = mc_hip_status(hipMemsetAsync(err, 0, nframes * 2 * sizeof(int32_t), st));
  if (rc != MC_OK) return rc;
  uint8_t *base = static_cast<uint8_t *>(ws);
  mc_bz2_stream *streams = reinterpret_cast<mc_bz2_stream *>(base);
  uint32_t *counter = reinterpret_cast<uint32_t *>(base + nframes * sizeof(mc_bz2_stream));
  rc = mc_hip_status(hipMemsetAsync(counter, 0, 16, st));
  if (rc != MC_OK) return rc;
  // blocks of multi_min symbols and more go multi-start; 0: the measured default
  if (multi_min == 0) multi_min = MC_BZ2_MULTI_MIN;
  if (multi_min < 2) multi_min = 2;
  const uint8_t *fr = static_cast<const uint8_t *>(frames);
  const unsigned pgrid = (unsigned)((nframes + MC_BLOCK - 1) / MC_BLOCK);
  hipLaunchKernelGGL(bz2_plan_kernel, dim3(pgrid), dim3(MC_BLOCK), 0, st, fr, static_cast<const mc_bz2_frame *>(table),
                     (uint32_t)nframes, STORE ? 0u : 1u, (uint32_t)max_level, streams, out, err);
  rc = mc_last_launch();
  if (rc != MC_OK) return rc;
  hipLaunchKernelGGL(bz2_decode_kernel<STORE>, dim3((unsigned)grid_waves(nframes)), dim3(WAVE), 0, st, fr, streams,
                     (uint32_t)nframes, (uint32_t)max_level, multi_min, counter, base + head_bytes(nframes), out, err);
  return mc_last_launch();
}

}  // namespace

static_assert(sizeof(mc_bz2_frame) == 32 && sizeof(mc_bz2_stream) == 32, "record layout (include/mcodec.h)");
static_assert(sizeof(mc_bz2_tables) + sizeof(splitters) + 16 <= 53 * 1024, "three bz2 workgroups share a CU's LDS");

extern "C" {

size_t mc_bz2_workspace(size_t nframes, unsigned max_level) {
  if (max_level < 1 || max_level > 9) return 0;
  return head_bytes(nframes) + grid_waves(nframes) * 5u * (size_t)MC_BZ2_BLOCK_UNIT * max_level;
}

int mc_bz2_size_batch(const void *frames, const void *frame_table, size_t nframes, unsigned max_level,
                      unsigned multi_min, void *workspace, size_t workspace_bytes, uint32_t *sizes, int32_t *err,
                      mc_stream_t stream) {
  return run<false>(frames, frame_table, nframes, max_level, multi_min, workspace, workspace_bytes, sizes, err, stream);
}

int mc_bz2_decode_batch(const void *frames, const void *frame_table, size_t nframes, unsigned max_level,
                        unsigned multi_min, void *workspace, size_t workspace_bytes, uint32_t *produced, int32_t *err,
                        mc_stream_t stream) {
  return run<true>(frames, frame_table, nframes, max_level, multi_min, workspace, workspace_bytes, produced, err, stream);
}

}  // extern "C"
