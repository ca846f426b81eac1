"""Probe: GPU bz2 encode (numcodecs_amd.bz2_enc.compress_many) on the decoder's
two batch shapes and one buffer alone:

    256 x 1 MiB at level 9, 4096 x 8000 bytes at level 1, 1 x 1 MiB at level 9

The buffers cycle through four kinds (arange i4, linspace f8, normal f8,
integers i8), seeded.  The whole call is timed (host wall clock around a call
that ends in its read-back and a synchronise: staging, five launches, the sizes
coming back): the median of 5 after 2 warm-ups, behind a gate: a sample of the
frames must decode to their inputs with ``bz2.decompress`` before any timing
counts.  Beside it ``bz2.compress`` at the same level on one host core over an
eighth of the batch (at least one buffer), measured before the GPU is touched,
and the frames' total size against libbz2's.

    python tools/probe_bz2_encode.py [--out FILE] [--once SHAPE]

``--once 256x1M|4096x8000|1x1M`` makes one warmed call of that shape and
nothing else: the run to put under ``rocprofv3 --kernel-trace --stats`` for
the per-launch split.  Prints one JSON line per shape and writes them to
profiles/bz2_encode/probe_bz2_encode.jsonl.
"""

import argparse
import bz2
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"256x1M": (256, 1 << 20, 9), "4096x8000": (4096, 8000, 1), "1x1M": (1, 1 << 20, 9)}


def buffers(count, nbytes, seed=0):
    rng = np.random.default_rng(seed)
    kinds = [
        lambda k: np.arange(k * 1000, k * 1000 + nbytes // 4, dtype=np.int32),
        lambda k: np.linspace(k, k + 1000.0, nbytes // 8),
        lambda k: rng.standard_normal(nbytes // 8),
        lambda k: rng.integers(0, 1 << 40, nbytes // 8, dtype=np.int64),
    ]
    return [np.ascontiguousarray(kinds[k % 4](k)).view(np.uint8).reshape(-1) for k in range(count)]


def median_wall(fn, warm=2, reps=5):
    for _ in range(warm):
        fn()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--once", choices=sorted(SHAPES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bz2_encode", "probe_bz2_encode.jsonl"))
    args = ap.parse_args()

    shapes = {args.once: SHAPES[args.once]} if args.once else SHAPES
    data, host = {}, {}
    for name, (count, nbytes, level) in shapes.items():  # before the GPU is touched
        data[name] = buffers(count, nbytes)
        if args.once:
            continue
        part = data[name][:max(1, count // 8)]
        t0 = time.perf_counter()
        frames = [bz2.compress(b.tobytes(), level) for b in part]
        dt = time.perf_counter() - t0
        host[name] = (sum(len(b) for b in part) / dt / 1e9, sum(len(f) for f in frames), len(part))

    import torch

    from numcodecs_amd import bz2_enc

    dev = torch.device("cuda:0")
    lines = []
    for name, (count, nbytes, level) in shapes.items():
        srcs = [torch.from_numpy(b).to(dev) for b in data[name]]
        total = sum(len(b) for b in data[name])

        def call():
            out = bz2_enc.compress_many(srcs, level)
            torch.cuda.synchronize()
            return out

        out = call()  # the gate
        for k in sorted({0, 1, 2, 3, count // 2, count - 1} & set(range(count))):
            assert bz2.decompress(out[k].cpu().numpy().tobytes()) == data[name][k].tobytes(), (name, k)
        if args.once:
            call()
            print(json.dumps({"probe": "bz2_encode", "once": name}))
            return
        part = host[name][2]
        gpu_part_bytes = sum(len(o) for o in out[:part])
        frame_bytes = sum(len(o) for o in out)
        del out
        med, lo, hi = median_wall(call)
        line = {
            "probe": "bz2_encode", "shape": name, "buffers": count, "buffer_bytes": nbytes, "level": level,
            "frames_bytes": frame_bytes, "ratio": round(total / frame_bytes, 3),
            "frames_vs_libbz2": round(gpu_part_bytes / host[name][1], 4),
            "gpu_s_median": round(med, 5), "gpu_s_min": round(lo, 5), "gpu_s_max": round(hi, 5),
            "gpu_gb_s": round(total / med / 1e9, 4), "host_1core_gb_s": round(host[name][0], 4),
        }
        print(json.dumps(line))
        lines.append(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        for line in lines:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
