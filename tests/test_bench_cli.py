"""bench.py's command line: a plain run prints the headline only, --full is
what adds the rest, and --dump-outputs writes what the last timed step
computed (a fixed sample, float32) so that two builds can be compared."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("cpu_baseline", "c5_sharded", "cfg_C1", "cfg_C2_f64", "cfg_C3", "cfg_C4", "cfg_C5", "cfg_e2e",
             "cfg_next")


def test_dump_index_is_fixed_and_bounded():
    import bench

    assert bench.dump_index(bench.DUMP_SAMPLE) is None  # short arrays are kept whole
    n = bench.CHUNK
    a, b = bench.dump_index(n), bench.dump_index(n)
    assert torch.equal(a, b) and a.numel() == bench.DUMP_SAMPLE
    assert int(a[0]) == 0 and int(a[-1]) == n - 1 and bool((a[1:] >= a[:-1]).all())
    e = bench.DUMP_EDGE
    assert torch.equal(a[:e], torch.arange(e)) and torch.equal(a[-e:], torch.arange(n - e, n))
    # the two arrays of a run, sampled, stay under the 64 MB a dump may take
    assert 2 * 4 * bench.DUMP_SAMPLE <= 64e6


def test_dump_outputs_writes_float32(tmp_path):
    import bench

    n = bench.DUMP_SAMPLE + 12345
    big = (torch.arange(n) % 251).to(torch.uint8)
    small = torch.linspace(-1, 1, 1000)
    bench.dump_outputs(str(tmp_path / "d"), 0, {"big": big, "small": small})
    bench.dump_outputs(str(tmp_path / "d"), 3, {"small": small})
    got = np.load(tmp_path / "d" / "big.npy")
    assert got.dtype == np.float32 and got.shape == (bench.DUMP_SAMPLE,)
    assert np.array_equal(got, big[bench.dump_index(n)].numpy().astype(np.float32))
    assert np.array_equal(np.load(tmp_path / "d" / "small.npy"), small.numpy())
    assert np.array_equal(np.load(tmp_path / "d" / "small_rank3.npy"), small.numpy())


@pytest.mark.gpu
def test_plain_run_is_headline_only_and_dumps_last_step(device, tmp_path):
    import bench

    steps = 2
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", "1", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["metric"] == bench.METRIC and d["unit"] == "GiB/s" and d["higher_is_better"] is True
    assert d["dtype"] == "u8" and d["steps"] == steps and d["value"] > 0 and d["ms_per_step"] > 0
    # value = 2 x 256 MiB per step over the step time (both rounded in the line)
    assert abs(d["value"] * d["ms_per_step"] * 1e-3 - 2 * bench.CHUNK / bench.GiB) < 1e-3
    assert not [k for k in FULL_ONLY if k in d] and "copy_calibration" not in d["roofline"]
    assert d["roofline"]["frac"] > 0

    files = sorted(os.listdir(out))
    assert files == ["decoded.npy", "encoded.npy"]
    assert sum(os.path.getsize(out / f) for f in files) <= 64e6
    enc, dec = np.load(out / "encoded.npy"), np.load(out / "decoded.npy")
    assert enc.dtype == np.float32 and dec.dtype == np.float32
    # the last timed step worked on buffer set (steps - 1) % 4 of the seeded inputs
    g = torch.Generator(device=device).manual_seed(1234)
    x = [torch.randn(bench.CHUNK // 4, generator=g, device=device, dtype=torch.float32) for _ in range(steps)][-1]
    assert np.array_equal(dec, x[bench.dump_index(x.numel()).to(device)].cpu().numpy())
    planes = x.view(torch.uint8).view(-1, 4).t().reshape(-1)  # Shuffle(4): byte j of every element, j = 0..3
    assert np.array_equal(enc, planes[bench.dump_index(bench.CHUNK).to(device)].cpu().numpy().astype(np.float32))
