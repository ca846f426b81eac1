"""Probe: the GPU `lz4` codec (numcodecs_amd.lz4.compress_many /
decompress_many) for a 1 MiB float32 chunk, replicated 256x into one call.

Inputs: seeded N(0,1), a smooth signal (a cumulative sum), zeros (the Blosc
probes').  No shuffle comes before this codec, so float32 noise and the smooth
signal's mantissas barely shrink; the figures are the codec's, not a
pipeline's.  Both calls are timed with events behind a gate: the frames must
equal the host model's (tests/native_lz4codec) and decode back to the input
before any timing counts.  The compress, layout, gather, plan and decode
kernels are separated with torch.profiler's device times (null when it
records none).

    python tools/probe_lz4.py [--copies 256] [--reps 5] [--out FILE]

Prints one JSON line per input and writes them to
profiles/r09/probe_lz4.jsonl.
"""

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from numcodecs_amd import lz4  # noqa: E402
from tests import lz4_gen as lg  # noqa: E402

GIB = float(1 << 30)
KERNELS = ("lz4c_compress", "lz4c_layout", "lz4c_gather", "lz4c_plan", "lz4c_decode")


def inputs(n):
    rng = np.random.default_rng(0)
    normal = rng.standard_normal(n).astype(np.float32)
    return {"normal": normal, "smooth": np.cumsum(normal / 64).astype(np.float32), "zeros": np.zeros(n, np.float32)}


def kernel_times(fn):
    """Summed device microseconds of one call, per kernel of KERNELS."""
    try:
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        out = {k: 0.0 for k in KERNELS}
        seen = False
        for ev in prof.events():
            t = getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0.0)
            for k in KERNELS:
                if k + "_kernel" in ev.name:
                    out[k] += t
                    seen = True
        return out if seen else None
    except Exception as e:  # the breakdown is optional; the event timing is not
        print(f"profiler breakdown unavailable: {e!r}", file=sys.stderr)
        return None


def best_of(fn, reps):
    best = float("inf")
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        best = min(best, e0.elapsed_time(e1) * 1e-3)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--copies", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--mib", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09", "probe_lz4.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n = args.mib * (1 << 20) // 4
    lines = []
    for name, x in inputs(n).items():
        raw = x.tobytes()
        xd = torch.from_numpy(x).to(dev)
        srcs = [xd] * args.copies
        frames = lz4.compress_many(srcs)  # warm-up + the gate
        model = lg.host_frame(raw)
        picks = (frames[0], frames[-1], frames[len(frames) // 2])
        ok = all(f.cpu().numpy().tobytes() == model for f in picks)
        back = lz4.decompress_many(frames)
        ok = ok and all(back[i].cpu().numpy().tobytes() == raw for i in (0, len(back) // 2, len(back) - 1))
        if not ok:
            print(json.dumps({"input": name, "error": "the frames differ from the model or do not decode back"}))
            return 1
        total = len(raw) * args.copies
        enc_s = best_of(lambda: lz4.compress_many(srcs), args.reps)
        dec_s = best_of(lambda: lz4.decompress_many(frames), args.reps)
        ke = kernel_times(lambda: lz4.compress_many(srcs))
        kd = kernel_times(lambda: lz4.decompress_many(frames))

        def rate(kt, key, digits=3):
            return kt and kt[key] and round(total / (kt[key] * 1e-6) / GIB, digits)

        rec = {
            "input": name, "chunk_bytes": len(raw), "copies": args.copies, "frame_bytes": len(model),
            "ratio": round(len(raw) / len(model), 3), "segments_in_call": -(-len(raw) // lg.SEGMENT) * args.copies,
            "encode_call_gibs": round(total / enc_s / GIB, 3), "encode_call_ms": round(enc_s * 1e3, 3),
            "compress_gibs": rate(ke, "lz4c_compress"), "layout_us": ke and ke["lz4c_layout"],
            "gather_gibs": rate(ke, "lz4c_gather", 2),
            "decode_call_gibs": round(total / dec_s / GIB, 3), "decode_call_ms": round(dec_s * 1e3, 3),
            "plan_us": kd and kd["lz4c_plan"], "decode_gibs": rate(kd, "lz4c_decode"),
            "decode_one_wave_mbs": kd and kd["lz4c_decode"] and round(len(raw) / (kd["lz4c_decode"] * 1e-6) / 1e6, 2),
            "encode_kernel_us": ke, "decode_kernel_us": kd,
        }
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
