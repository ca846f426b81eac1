"""Probe: GPU deflate (numcodecs_amd.deflate.compress_many, zlib container) of a
1 MiB float32 chunk, 256 chunks in one call and one chunk alone.

Inputs: tools/probe_inflate.py's four (seeded N(0,1), a smooth signal, the
smooth signal after Shuffle(4), zeros).  The whole call is timed (host wall
clock around a synchronised call: staging, four launches, the read-back of the
sizes), behind a gate: the frames must inflate to the inputs through the stdlib
before any timing counts.  Beside it the project's CPU column:
``zlib.compress(level=1)`` of the same chunks on one host core and on 16
processes, measured before the GPU is touched, and the frame size against
zlib's -- the price of this match finder and of independent 64 KiB segments.
The kernels are separated with torch.profiler's device times (null when it
records none).

    python tools/probe_deflate.py [--copies 256] [--out FILE]

Prints one JSON line per input and batch and writes them to
profiles/r12/probe_deflate.jsonl.
"""

import argparse
import json
import multiprocessing
import os
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from probe_inflate import GIB, best_wall, inputs  # noqa: E402

KERNELS = ("dfl_parse", "dfl_code", "dfl_layout", "dfl_emit")


def _deflate_all(chunks):
    return sum(len(zlib.compress(c, 1)) for c in chunks)


def cpu_column(chunks, pool):
    one = best_wall(lambda: _deflate_all(chunks), 3)
    parts = [chunks[k::16] for k in range(16)]
    many = best_wall(lambda: pool.map(_deflate_all, parts), 3) if len(chunks) >= 16 else None
    return one, many


def kernel_times(torch, fn):
    try:
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        out, seen = {k: 0.0 for k in KERNELS}, False
        for ev in prof.events():
            t = getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0.0)
            for k in KERNELS:
                if k + "_kernel" in ev.name:
                    out[k] += t
                    seen = True
        return out if seen else None
    except Exception as e:  # the breakdown is optional; the wall time is not
        print(f"profiler breakdown unavailable: {e!r}", file=sys.stderr)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--copies", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12", "probe_deflate.jsonl"))
    args = ap.parse_args()

    data = inputs()
    zlib_size = {name: len(zlib.compress(d, 1)) for name, d in data.items()}
    cpu = {}
    with multiprocessing.get_context("fork").Pool(16) as pool:  # before the GPU is touched
        for name, d in data.items():
            cpu[name, args.copies] = cpu_column([d] * args.copies, pool)
            cpu[name, 1] = cpu_column([d], pool)

    import torch

    from numcodecs_amd import deflate

    dev = torch.device("cuda:0")
    lines = []
    for name, d in data.items():
        src = torch.frombuffer(bytearray(d), dtype=torch.uint8).to(dev)
        for copies, reps in ((args.copies, 5), (1, 20)):
            batch = [src] * copies
            out = deflate.compress_many(batch)  # the gate
            assert len(out) == copies
            for o in (out[0], out[-1], out[copies // 2]):
                assert zlib.decompress(o.cpu().numpy().tobytes()) == d
            frame_bytes = len(out[0])
            del out
            torch.cuda.synchronize()

            def call():
                deflate.compress_many(batch)
                torch.cuda.synchronize()

            t = best_wall(call, reps)
            total = copies * len(d)
            one, many = cpu[name, copies]
            line = {
                "probe": "deflate", "input": name, "chunks": copies, "chunk_bytes": len(d),
                "frame_bytes": frame_bytes, "ratio": round(len(d) / frame_bytes, 3),
                "zlib1_frame_bytes": zlib_size[name], "frame_vs_zlib1": round(frame_bytes / zlib_size[name], 4),
                "gpu_ms": round(t * 1e3, 3), "gpu_gib_s": round(total / t / GIB, 3),
                "cpu_1core_ms": round(one * 1e3, 3), "cpu_1core_gib_s": round(total / one / GIB, 3),
                "cpu_16proc_ms": None if many is None else round(many * 1e3, 3),
                "cpu_16proc_gib_s": None if many is None else round(total / many / GIB, 3),
                "kernels_us": kernel_times(torch, call),
            }
            print(json.dumps(line))
            lines.append(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        for line in lines:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
