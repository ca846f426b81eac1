"""Probe: GPU Blosc encode (numcodecs_amd.blosc.compress_many) at numcodecs'
defaults -- lz4, clevel 5, SHUFFLE, automatic blocksize -- for a 1 MiB float32
chunk, replicated 256x into one call.

Inputs: seeded N(0,1), a smooth signal (a cumulative sum), zeros (the decode
probe's).  The whole call is timed with events behind a gate: the frames must
decode back to the input (the product's decoder and the oracle's walker)
before any timing counts.  The filter, compress, layout and gather kernels are
separated with torch.profiler's device times (null when it records none).

The CPU columns are ONE core, compression only (no shuffle): the product's
scalar encoder compiled for the host (tests/native_lz4enc) over the frame's
streams, and -- if liblz4.so.1 loads -- liblz4's LZ4_compress_default over the
same streams.  Neither is c-blosc.

    python tools/probe_blosc_encode.py [--copies 256] [--reps 5] [--out FILE]

Prints one JSON line per input and writes them to
profiles/r08/probe_blosc_encode.jsonl.
"""

import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from numcodecs_amd import blosc  # noqa: E402
from oracle import blosc as oblosc  # noqa: E402
from tests import blosc_enc_gen as eg  # noqa: E402
from tests import blosc_gen as gen  # noqa: E402

GIB = float(1 << 30)


def inputs(n):
    rng = np.random.default_rng(0)
    normal = rng.standard_normal(n).astype(np.float32)
    return {"normal": normal, "smooth": np.cumsum(normal / 64).astype(np.float32), "zeros": np.zeros(n, np.float32)}


def kernel_times(fn):
    """{filter, compress, layout, gather}: summed device microseconds of one call."""
    try:
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        out = {"filter": 0.0, "compress": 0.0, "layout": 0.0, "gather": 0.0}
        seen = False
        for ev in prof.events():
            t = getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0.0)
            name = ev.name
            if "compress_kernel" in name:
                out["compress"] += t
            elif "layout_kernel" in name:
                out["layout"] += t
            elif "gather_kernel" in name:
                out["gather"] += t
            elif "shuffle" in name or "transpose" in name:
                out["filter"] += t
            else:
                continue
            seen = True
        return out if seen else None
    except Exception as e:  # the breakdown is optional; the event timing is not
        print(f"profiler breakdown unavailable: {e!r}", file=sys.stderr)
        return None


def streams_of(raw, typesize, blocksize, flags):
    """The filtered streams the compress kernel sees for this frame."""
    filtered = oblosc.blosc_filter(raw, typesize, blocksize, gen.SHUFFLE, True)
    out = []
    for p in range(0, len(raw), blocksize):
        blk = filtered[p:p + blocksize]
        ns = gen.split_streams(flags, typesize, blocksize, len(blk))
        out += [blk[j * (len(blk) // ns):(j + 1) * (len(blk) // ns)] for j in range(ns)]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--copies", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--mib", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08", "probe_blosc_encode.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n = args.mib * (1 << 20) // 4
    try:
        liblz4 = ctypes.CDLL("liblz4.so.1")
    except OSError:
        liblz4 = None
    lines = []
    for name, x in inputs(n).items():
        raw = x.tobytes()
        xd = torch.from_numpy(x).to(dev)
        srcs = [xd] * args.copies
        frames = blosc.compress_many(srcs)  # warm-up + the gate
        picks = (frames[0], frames[-1], frames[len(frames) // 2])
        ok = all(d.cpu().numpy().tobytes() == raw for d in blosc.decompress_many(list(picks)))
        ok = ok and all(gen.oracle_decode(f.cpu().numpy().tobytes()) == raw for f in picks)
        if not ok:
            print(json.dumps({"input": name, "error": "the frames do not decode back to the input"}))
            return 1
        frame = frames[0].cpu().numpy().tobytes()
        flags, typesize, blocksize = frame[2], frame[3], int.from_bytes(frame[8:12], "little")
        best = float("inf")
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            blosc.compress_many(srcs)
            e1.record()
            e1.synchronize()
            best = min(best, e0.elapsed_time(e1) * 1e-3)
        total = len(raw) * args.copies
        kt = kernel_times(lambda: blosc.compress_many(srcs))
        # one host core, compression only
        streams = streams_of(raw, typesize, blocksize, flags)
        t0 = time.perf_counter()
        cpu_reps = 5
        for _ in range(cpu_reps):
            for s in streams:
                eg.encode_stream(s)
        cpu_s = (time.perf_counter() - t0) / cpu_reps
        lz4_s = None
        if liblz4 is not None:
            bufs = [ctypes.create_string_buffer(len(s) + len(s) // 255 + 16) for s in streams]
            t0 = time.perf_counter()
            for _ in range(cpu_reps):
                for s, b in zip(streams, bufs):
                    liblz4.LZ4_compress_default(s, b, len(s), len(b))
            lz4_s = (time.perf_counter() - t0) / cpu_reps
        rec = {
            "input": name, "chunk_bytes": len(raw), "copies": args.copies, "blocksize": blocksize,
            "flags": flags, "ratio": round(len(raw) / len(frame), 3), "streams_per_frame": len(streams),
            "streams_in_call": len(streams) * args.copies,
            "call_gibs": round(total / best / GIB, 3), "call_ms": round(best * 1e3, 3),
            "filter_gibs": kt and kt["filter"] and round(total / (kt["filter"] * 1e-6) / GIB, 2),
            "compress_gibs": kt and kt["compress"] and round(total / (kt["compress"] * 1e-6) / GIB, 3),
            "layout_us": kt and kt["layout"], "gather_gibs": kt and kt["gather"] and
            round(total / (kt["gather"] * 1e-6) / GIB, 2),
            "kernel_us": kt,
            "cpu_scalar_one_core_gibs": round(len(raw) / cpu_s / GIB, 3),
            "cpu_liblz4_one_core_gibs": lz4_s and round(len(raw) / lz4_s / GIB, 3),
        }
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
