"""Probe: GPU Blosc encode and decode of zstd frames (numcodecs_amd.blosc
compress_many / decompress_many with ``formats=ENCODE_FORMATS`` /
``DECODE_FORMATS``) beside their neighbours, on device-resident data: a batch
of 256 x 1 MiB float32 chunks, SHUFFLE, clevel 5 (128 KiB blocks).

  blosc_zstd_encode   the batch -> Blosc zstd frames
  blosc_zstd_decode   those frames -> arrays
  zstd_decode         the stand-alone ``zstd`` batch call on the very streams
                      of those frames (no container, no unshuffle)
  blosc_lz4_decode    the package's own Blosc lz4 frames of the same chunks
  blosc_lz4_encode / zstd_encode   the Blosc lz4 encoder and the stand-alone ``zstd_enc`` call

zstd_encode is the stand-alone encoder on the shuffled chunks whole (1 MiB
chunks, not 128 KiB blocks); zstd_decode takes the compressed streams out of
the Blosc frames on the host.

Every timed call is warmed up, gated on byte equality, and timed ``--reps``
times with device events around the whole call (its read-back of the error
record included); the best and the median are printed.

    python tools/probe_blosc_z.py [--copies 256] [--reps 7]

Prints one JSON line per input.
"""

import argparse
import json
import os
import statistics
import struct
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from numcodecs_amd import blosc, blosc_shuffle, zstd, zstd_enc  # noqa: E402

GIB = float(1 << 30)
BLOCK = 128 * 1024


def inputs(n, copies):
    """copies different chunks per input kind (no two frames alike)."""
    rng = np.random.default_rng(0)
    normal = rng.standard_normal((copies, n)).astype(np.float32)
    smooth = np.cumsum(normal / 64, axis=1).astype(np.float32)
    ramp = (np.arange(n, dtype=np.float32)[None, :] * 0.25 + np.arange(copies, dtype=np.float32)[:, None])
    return {"normal": normal, "smooth": smooth, "ramp": ramp}


def streams_of(frame):
    """[(compressed stream, its share)] of a Blosc zstd frame (one stream per block), raw streams left out."""
    nbytes, bs = struct.unpack("<II", frame[4:12])
    out = []
    for b in range(-(-nbytes // bs)):
        p = struct.unpack("<i", frame[16 + 4 * b:20 + 4 * b])[0]
        cb = struct.unpack("<i", frame[p:p + 4])[0]
        share = min(bs, nbytes - b * bs)
        if cb != share:
            out.append((frame[p + 4:p + 4 + cb], share))
    return out


def dev_bytes(b, dev):
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)


def timed(fn, reps):
    fn()  # warm-up: code objects, allocator
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e-3)
    return min(ts), statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--copies", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--mib", type=int, default=1)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n = args.mib * (1 << 20) // 4
    for name, chunks in inputs(n, args.copies).items():
        total = chunks.nbytes
        xs = [torch.from_numpy(c).to(dev) for c in chunks]
        zenc = lambda: blosc.compress_many(xs, "zstd", 5, blosc.SHUFFLE, formats=blosc.ENCODE_FORMATS)  # noqa: E731
        zf = zenc()
        zframes = [f.cpu().numpy().tobytes() for f in zf]
        assert all(f[8:12] == struct.pack("<I", BLOCK) and not f[2] & 2 for f in zframes)
        streams = [p for f in zframes for p in streams_of(f)]
        sf = [dev_bytes(s, dev) for s, _n in streams]
        sizes = [u for _s, u in streams]
        lf = blosc.compress_many(xs, "lz4", 5, blosc.SHUFFLE)
        # the gates
        got = blosc.decompress_many(zf, formats=blosc.DECODE_FORMATS)
        ok = all(torch.equal(g.view(torch.float32), x) for g, x in zip(got, xs))
        got = blosc.decompress_many(lf)
        ok = ok and all(torch.equal(g.view(torch.float32), x) for g, x in zip(got, xs))
        ok = ok and all(int(len(g)) == u for g, u in zip(zstd.decompress_many(sf, sizes=sizes), sizes))
        if not ok:
            print(json.dumps({"input": name, "error": "decoded bytes differ"}))
            return 1
        rec = {"input": name, "chunk_bytes": n * 4, "copies": args.copies, "blocksize": BLOCK,
               "zstd_ratio": round(total / sum(len(f) for f in zframes), 3),
               "lz4_ratio": round(total / sum(int(len(f)) for f in lf), 3),
               "zstd_streams": len(streams), "zstd_stream_bytes": sum(sizes)}
        shuffled = [blosc_shuffle.shuffle(x, 4, BLOCK, blosc.SHUFFLE) for x in xs]
        for key, fn, work in (
            ("blosc_zstd_decode", lambda: blosc.decompress_many(zf, formats=blosc.DECODE_FORMATS), total),
            ("zstd_decode", lambda: zstd.decompress_many(sf, sizes=sizes), sum(sizes)),
            ("blosc_zstd_encode", zenc, total),
            ("blosc_lz4_decode", lambda: blosc.decompress_many(lf), total),
            ("blosc_lz4_encode", lambda: blosc.compress_many(xs, "lz4", 5, blosc.SHUFFLE), total),
            ("zstd_encode", lambda: zstd_enc.compress_many(shuffled), total),
        ):
            best, med = timed(fn, args.reps)
            rec[key] = {"best_ms": round(best * 1e3, 3), "median_ms": round(med * 1e3, 3),
                        "gibs": round(work / best / GIB, 3) if work else None}
        print(json.dumps(rec), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
