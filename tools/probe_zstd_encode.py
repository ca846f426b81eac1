"""Probe: GPU zstd encode (numcodecs_amd.zstd_enc.compress_many) of a 1 MiB
float32 chunk, 256 chunks in one call (best of 5) and one chunk alone (best of
20).

Inputs: tools/probe_inflate.py's four (seeded N(0,1), a smooth signal, the
smooth signal after Shuffle(4), zeros).  The whole call is timed (host wall
clock around a synchronised call: staging, four launches, the read-back of the
sizes), behind a gate: the frames must decode to the inputs through libzstd
where it loads, through the project's GPU decoder otherwise, before any timing
counts.  Beside it: the frame size against libzstd levels 1 and 3 of the same
chunk (where libzstd does not load: the sizes libzstd 1.4.8 gave on the
development machine, marked ``"libzstd": "recorded 1.4.8"``), against the
project's own ``deflate`` frame of the same chunk, and libzstd's time on one
host core, measured before the GPU is touched.  The kernels are separated with
torch.profiler's device times from one profiled call (null when it records
none).

    python tools/probe_zstd_encode.py [--copies 256] [--out FILE]

Prints one JSON line per input and batch and writes them to
profiles/zstd_encode/probe_zstd_encode.jsonl.
"""

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from probe_inflate import GIB, best_wall, inputs  # noqa: E402

from tests import zstd_gen as zg  # noqa: E402

KERNELS = ("zstd_enc_parse", "zstd_enc_code", "zstd_enc_layout", "zstd_enc_emit")
# libzstd 1.4.8, levels 1 and 3, of the four inputs on the development machine:
# python tools/probe_zstd_encode.py --sizes-only
RECORDED = {
    "normal": (969111, 969110),
    "smooth": (949403, 949402),
    "smooth-shuffle4": (792837, 766968),
    "zeros": (51, 50),
}


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
    ap.add_argument("--sizes-only", action="store_true", help="print libzstd's frame sizes and stop (no GPU)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "zstd_encode", "probe_zstd_encode.jsonl"))
    args = ap.parse_args()

    data = inputs()
    z = zg.load_lib()
    sizes, cpu_ms = {}, {}
    for name, d in data.items():  # before the GPU is touched
        if z is None:
            sizes[name], cpu_ms[name] = RECORDED.get(name), (None, None)
        else:
            sizes[name] = (len(z.compress(d, 1)), len(z.compress(d, 3)))
            cpu_ms[name] = tuple(round(best_wall(lambda lv=lv: z.compress(d, lv), 3) * 1e3, 3) for lv in (1, 3))
    if args.sizes_only:
        print(json.dumps({"libzstd": z and z.version, "sizes": sizes}))
        return

    import torch

    from numcodecs_amd import deflate, zstd, zstd_enc

    dev = torch.device("cuda:0")
    lines = []
    for name, d in data.items():
        src = torch.frombuffer(bytearray(d), dtype=torch.uint8).to(dev)
        deflate_bytes = len(deflate.compress(src))
        for copies, reps in ((args.copies, 5), (1, 20)):
            batch = [src] * copies
            out = zstd_enc.compress_many(batch)  # the gate
            assert len(out) == copies
            for o in (out[0], out[-1], out[copies // 2]):
                if z is not None:
                    assert z.decompress(o.cpu().numpy().tobytes(), len(d)) == (d, None)
                else:
                    assert torch.equal(zstd.decompress(o), src)
            frame_bytes = len(out[0])
            del out
            torch.cuda.synchronize()

            def call():
                zstd_enc.compress_many(batch)
                torch.cuda.synchronize()

            t = best_wall(call, reps)
            total = copies * len(d)
            l1, l3 = sizes[name] or (None, None)
            line = {
                "probe": "zstd_encode", "input": name, "chunks": copies, "chunk_bytes": len(d),
                "frame_bytes": frame_bytes, "ratio": round(len(d) / frame_bytes, 3),
                "libzstd": z.version if z is not None else "recorded 1.4.8",
                "libzstd1_frame_bytes": l1, "libzstd3_frame_bytes": l3,
                "frame_vs_libzstd1": l1 and round(frame_bytes / l1, 4), "frame_vs_libzstd3": l3 and round(frame_bytes / l3, 4),
                "deflate_frame_bytes": deflate_bytes, "frame_vs_deflate": round(frame_bytes / deflate_bytes, 4),
                "gpu_ms": round(t * 1e3, 3), "gpu_gib_s": round(total / t / GIB, 3),
                "libzstd1_1core_ms_per_chunk": cpu_ms[name][0], "libzstd3_1core_ms_per_chunk": cpu_ms[name][1],
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
