"""The pure parts of numcodecs_amd._frames, the batch plumbing blosc.py and
lz4.py share: slot layout, packed offsets, destination checks and the batch's
device.  No GPU is needed or touched."""

import numpy as np
import pytest
import torch

from numcodecs_amd import _frames


def test_slot_layout():
    sizes = [1, 255, 256, 257, 0, 65537]
    offsets, total = _frames.slots(sizes)
    assert [_frames.up(n) for n in sizes] == [256, 256, 256, 512, 0, 65792]
    assert len(offsets) == len(sizes) and all(o % _frames.ALIGN == 0 for o in offsets)
    assert total == sum(_frames.up(n) for n in sizes)
    spans = sorted((o, o + n) for o, n in zip(offsets, sizes) if n)
    assert all(a_end <= b_start for (_a, a_end), (b_start, _b) in zip(spans, spans[1:]))  # no overlap
    assert spans[-1][1] <= total
    assert offsets[5] == offsets[4]  # the zero-size entry took no space
    assert _frames.slots([]) == ([], 0) and _frames.slots([0, 0]) == ([0, 0], 0)
    by_key, total2 = _frames.slot_map("abcdef", sizes)
    assert total2 == total and [by_key[k] for k in "abcdef"] == offsets


def test_packed_offsets():
    lengths = [10, 3, 7, 5]
    on_dev = [True, False, True, False]
    # host frames first in index order (1, 3), then device frames (0, 2): running sums, no alignment
    assert _frames.packed_offsets(lengths, on_dev) == [8, 0, 18, 3]
    assert _frames.packed_offsets(lengths, [False] * 4) == [0, 10, 13, 20]
    assert _frames.packed_offsets(lengths, [True] * 4) == [0, 10, 13, 20]
    assert _frames.packed_offsets([4, 0, 6], [True, False, False]) == [6, 0, 0]
    assert _frames.packed_offsets([], []) == []


def test_out_bytes():
    with pytest.raises(ValueError, match="^destination buffer too small; expected at least 500, got 499$"):
        _frames.out_bytes(np.zeros(499, np.uint8), 500)
    with pytest.raises(ValueError, match="^destination buffer too small; expected at least 9, got 8$"):
        _frames.out_bytes(np.zeros(2, "<f4"), 9)
    ro = np.zeros(500, np.uint8)
    ro.flags.writeable = False
    with pytest.raises(ValueError, match="^destination buffer is read-only$"):
        _frames.out_bytes(ro, 500)
    with pytest.raises(ValueError, match="^destination buffer is read-only$"):
        _frames.out_bytes(ro, 501)  # read-only is found first
    out = np.zeros((3, 4), "<i2")
    raw = _frames.out_bytes(out, 24)
    assert raw.dtype == np.uint8 and raw.shape == (24,) and np.shares_memory(raw, out)
    big = bytearray(30)
    raw = _frames.out_bytes(big, 24)  # larger than needed is fine
    raw[:2] = 7
    assert raw.shape == (30,) and big[:3] == b"\x07\x07\x00"


def test_flat_bytes():
    flat = _frames.flat_bytes(np.arange(6, dtype="<u2").reshape(2, 3), 100)
    assert flat.dtype == np.uint8 and flat.tobytes() == np.arange(6, dtype="<u2").tobytes()
    with pytest.raises(ValueError, match="^Codec does not support buffers of > 11 bytes$"):
        _frames.flat_bytes(np.zeros(12, np.uint8), 11)


def test_device_resolution_without_a_device(monkeypatch):
    def touched(*_a, **_k):
        raise AssertionError("HIP call")

    for name in ("current_device", "is_available", "device_count", "current_stream"):
        monkeypatch.setattr(torch.cuda, name, touched)
    srcs = [np.zeros(5, np.uint8), np.zeros(0, np.uint8)]
    on_dev = [False, False]
    assert _frames.batch_device(srcs, on_dev, [None, np.zeros(5, np.uint8)], "frames") is None
    assert _frames.batch_device(srcs, on_dev, what="buffers") is None
    assert _frames.batch_device(srcs, on_dev, [bytearray(5), torch.zeros(5, dtype=torch.uint8)]) is None  # a CPU tensor
    _frames.check_out_device([None, np.zeros(5, np.uint8)], None)
    srcs = [np.arange(9, dtype=np.uint8), np.frombuffer(b"abcdef", np.uint8)]
    heads = _frames.read_prefixes(srcs, on_dev, 4)  # host frames: no copy from a device
    assert heads.dtype == np.uint8 and heads.tolist() == [[0, 1, 2, 3], [97, 98, 99, 100]]
