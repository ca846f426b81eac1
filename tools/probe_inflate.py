"""Probe: GPU inflate (numcodecs_amd.zlib.decompress_many) of zlib frames of a
1 MiB float32 chunk, 256 frames in one call and one frame alone.

Inputs: seeded N(0,1), a smooth signal (a cumulative sum), the smooth signal
after Shuffle(4), zeros; each compressed by the stdlib at level 1.  The whole
call is timed (host wall clock around a synchronised call: staging, launches,
read-backs), with ``sizes=`` (plan + decode + check) and without (the sizing
pass first), behind a gate: the results must equal the inputs before any
timing counts.  Beside it the project's CPU column: ``zlib.decompress`` of the
same frames on one host core and on 16 processes, measured before the GPU is
touched.  The kernels are separated with torch.profiler's device times (null
when it records none).

    python tools/probe_inflate.py [--copies 256] [--out FILE]

Prints one JSON line per input and batch and writes them to
profiles/r11/probe_inflate.jsonl.
"""

import argparse
import json
import multiprocessing
import os
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GIB = float(1 << 30)
KERNELS = ("inflate_plan", "inflate_kernel<false>", "inflate_kernel<true>", "inflate_check")
N = 1 << 18  # float32 elements: 1 MiB


def inputs():
    rng = np.random.default_rng(0)
    normal = rng.standard_normal(N).astype(np.float32)
    smooth = np.cumsum(normal / 64).astype(np.float32)
    shuffled = np.ascontiguousarray(smooth.view(np.uint8).reshape(-1, 4).T)
    return {"normal": normal.tobytes(), "smooth": smooth.tobytes(), "smooth-shuffle4": shuffled.tobytes(),
            "zeros": bytes(4 * N)}


def _inflate_all(frames):
    return sum(len(zlib.decompress(f)) for f in frames)


def best_wall(fn, reps):
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t0)
    return best


def cpu_column(frames, pool):
    one = best_wall(lambda: _inflate_all(frames), 3)
    parts = [frames[k::16] for k in range(16)]
    many = best_wall(lambda: pool.map(_inflate_all, parts), 3) if len(frames) >= 16 else None
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
            if "inflate_plan" in ev.name:
                k = KERNELS[0]
            elif "inflate_check" in ev.name:
                k = KERNELS[3]
            elif "inflate_kernel" in ev.name:  # the sizing pass is the STORE = false instance
                k = KERNELS[1] if ("Lb0" in ev.name or "<false>" in ev.name) else KERNELS[2]
            else:
                continue
            out[k] += t
            seen = True
        return out if seen else None
    except Exception as e:  # the breakdown is optional; the wall time is not
        print(f"profiler breakdown unavailable: {e!r}", file=sys.stderr)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--copies", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11", "probe_inflate.jsonl"))
    args = ap.parse_args()

    data = inputs()
    frames = {name: zlib.compress(d, 1) for name, d in data.items()}
    cpu = {}
    with multiprocessing.get_context("fork").Pool(16) as pool:  # before the GPU is touched
        for name, f in frames.items():
            cpu[name, args.copies] = cpu_column([f] * args.copies, pool)
            cpu[name, 1] = cpu_column([f], pool)

    import torch

    from numcodecs_amd import zlib as nzlib

    dev = torch.device("cuda:0")
    lines = []
    for name, d in data.items():
        f = torch.frombuffer(bytearray(frames[name]), dtype=torch.uint8).to(dev)
        want = torch.frombuffer(bytearray(d), dtype=torch.uint8).to(dev)
        for copies, reps in ((args.copies, 5), (1, 20)):
            batch, sizes = [f] * copies, [len(d)] * copies
            for out in (nzlib.decompress_many(batch), nzlib.decompress_many(batch, sizes=sizes)):  # the gate
                assert len(out) == copies and all(torch.equal(o, want) for o in (out[0], out[-1], out[copies // 2]))
            torch.cuda.synchronize()

            def sized():
                nzlib.decompress_many(batch, sizes=sizes)
                torch.cuda.synchronize()

            def unsized():
                nzlib.decompress_many(batch)
                torch.cuda.synchronize()

            t_sized, t_unsized = best_wall(sized, reps), best_wall(unsized, reps)
            total = copies * len(d)
            one, many = cpu[name, copies]
            line = {
                "probe": "inflate", "input": name, "frames": copies, "frame_bytes": len(frames[name]),
                "chunk_bytes": len(d), "ratio": round(len(d) / len(frames[name]), 3),
                "gpu_sized_ms": round(t_sized * 1e3, 3), "gpu_sized_gib_s": round(total / t_sized / GIB, 3),
                "gpu_unsized_ms": round(t_unsized * 1e3, 3), "gpu_unsized_gib_s": round(total / t_unsized / GIB, 3),
                "cpu_1core_ms": round(one * 1e3, 3), "cpu_1core_gib_s": round(total / one / GIB, 3),
                "cpu_16proc_ms": None if many is None else round(many * 1e3, 3),
                "cpu_16proc_gib_s": None if many is None else round(total / many / GIB, 3),
                "kernels_us_unsized": kernel_times(torch, unsized),
            }
            print(json.dumps(line))
            lines.append(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        for line in lines:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
