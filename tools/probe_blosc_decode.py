"""Probe: GPU Blosc decode (numcodecs_amd.blosc.decompress_many) on frames
built the way numcodecs' defaults build them -- lz4, SHUFFLE, automatic
blocksize -- for a 1 MiB float32 chunk, replicated 256x into one call.

Inputs: seeded N(0,1), a smooth signal (a cumulative sum), zeros.  The frames
come from the test-side writer (tests/blosc_gen.py: a greedy LZ4 compressor,
not c-blosc's), so the ratios are that writer's.  The whole call is timed with
events behind a byte-equality gate; the plan, decode and unfilter kernels are
separated with torch.profiler's device times (null when it records none).

The CPU column is the product's scalar decoder compiled for the host
(tests/native_lz4) on ONE core, decompression only (no unshuffle).  It is not
c-blosc and not liblz4 -- neither is available to this probe.

    python tools/probe_blosc_decode.py [--copies 256] [--reps 5]

Prints one JSON line per input.
"""

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from numcodecs_amd import blosc, blosc_shuffle  # noqa: E402
from tests import blosc_gen as gen  # noqa: E402

GIB = float(1 << 30)


def inputs(n):
    rng = np.random.default_rng(0)
    normal = rng.standard_normal(n).astype(np.float32)
    return {"normal": normal, "smooth": np.cumsum(normal / 64).astype(np.float32), "zeros": np.zeros(n, np.float32)}


def kernel_times(fn):
    """{plan, decode, unfilter}: summed device microseconds of one call."""
    try:
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        out = {"plan": 0.0, "decode": 0.0, "unfilter": 0.0}
        seen = False
        for ev in prof.events():
            t = getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0.0)
            name = ev.name
            if "plan_kernel" in name:
                out["plan"] += t
            elif "decode_kernel" in name:
                out["decode"] += t
            elif "shuffle" in name or "k_unshuffle" in name or "transpose" in name:
                out["unfilter"] += t
            else:
                continue
            seen = True
        return out if seen else None
    except Exception as e:  # the breakdown is optional; the event timing is not
        print(f"profiler breakdown unavailable: {e!r}", file=sys.stderr)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--copies", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--mib", type=int, default=1)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n = args.mib * (1 << 20) // 4
    for name, x in inputs(n).items():
        raw = x.tobytes()
        bs = blosc_shuffle.compute_blocksize(len(raw), 4, 5, "lz4")
        frame = gen.blosc_frame(raw, 4, bs, gen.SHUFFLE)
        info = gen.host_decode(frame)[2]
        fd = torch.frombuffer(bytearray(frame), dtype=torch.uint8).to(dev)
        frames = [fd] * args.copies
        outs = blosc.decompress_many(frames)  # warm-up + the gate
        ok = all(o.cpu().numpy().tobytes() == raw for o in (outs[0], outs[-1], outs[len(outs) // 2]))
        if not ok:
            print(json.dumps({"input": name, "error": "decoded bytes differ"}))
            return 1
        best = float("inf")
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            blosc.decompress_many(frames)
            e1.record()
            e1.synchronize()
            best = min(best, e0.elapsed_time(e1) * 1e-3)
        total = len(raw) * args.copies
        kt = kernel_times(lambda: blosc.decompress_many(frames))
        # one host core, the scalar decoder (decompression only)
        t0 = time.perf_counter()
        cpu_reps = 5
        for _ in range(cpu_reps):
            assert gen.host_decode(frame)[0] == 0
        cpu_s = (time.perf_counter() - t0) / cpu_reps
        rec = {
            "input": name, "chunk_bytes": len(raw), "copies": args.copies, "blocksize": bs,
            "ratio": round(len(raw) / len(frame), 3), "streams_per_frame": info["nstreams"],
            "streams_in_call": info["nstreams"] * args.copies,
            "call_gibs": round(total / best / GIB, 3), "call_ms": round(best * 1e3, 3),
            "plan_gibs": kt and kt["plan"] and round(total / (kt["plan"] * 1e-6) / GIB, 2),
            "decode_gibs": kt and kt["decode"] and round(total / (kt["decode"] * 1e-6) / GIB, 3),
            "unfilter_gibs": kt and kt["unfilter"] and round(total / (kt["unfilter"] * 1e-6) / GIB, 2),
            "kernel_us": kt,
            "cpu_scalar_one_core_gibs": round(len(raw) / cpu_s / GIB, 3),
        }
        print(json.dumps(rec), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
