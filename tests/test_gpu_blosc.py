"""GPU Blosc decode (numcodecs_amd.blosc; csrc/mc_blosc_dec.hip): the
reference's fixture frames, generated frame shapes, hand-assembled LZ4
sequences, batches, ``out=`` semantics and malformed frames.  Every generated
stream is <= 256 KiB: the smallest shapes at which the kernels can go wrong."""

import numpy as np
import pytest
import torch

from numcodecs_amd import blosc
from oracle import blosc as oblosc
from tests import blosc_gen as gen
from tests.helpers import fixture_cases
from tests.test_blosc_host import MALFORMED_CODES

pytestmark = pytest.mark.gpu

ERROR_RE = "^error during blosc decompression: -1$"


@pytest.fixture(scope="module")
def shapes():
    return gen.shape_cases()


@pytest.fixture(scope="module")
def sequences():
    return gen.sequence_cases()


def _dev(frame, device):
    return torch.frombuffer(bytearray(frame), dtype=torch.uint8).to(device)


# 1 ------------------------------------------------------------------------
def test_fixture_frames(device):
    frames, raws, others = [], [], []
    for arr, _j, _config, frame in fixture_cases("blosc"):
        flags = frame[2]
        if flags & oblosc.BLOSC_MEMCPYED or flags >> 5 == oblosc.LZ4_FORMAT:
            frames.append(frame)
            raws.append(arr.tobytes(order="A"))
        else:
            others.append(frame)
    assert (len(frames), len(others)) == (133, 36)
    for frame, raw in zip(frames, raws):  # one by one, from host bytes
        got = blosc.decompress(frame)
        assert isinstance(got, np.ndarray) and got.tobytes() == raw
    got = blosc.decompress_many([_dev(f, device) for f in frames])  # and from device tensors
    for g, raw in zip(got, raws):
        assert g.is_cuda and g.dtype == torch.uint8 and g.cpu().numpy().tobytes() == raw
    codec = blosc.Blosc()
    for frame in others:
        with pytest.raises(NotImplementedError, match="blosclz|snappy|zlib|zstd"):
            codec.decode(frame)


# 2 ------------------------------------------------------------------------
def test_frame_shapes(device, shapes):
    names = [n for n, _d, _f in shapes]
    got_host = blosc.decompress_many([f for _n, _d, f in shapes])
    got_dev = blosc.decompress_many([_dev(f, device) for _n, _d, f in shapes])
    for name, (_n, data, frame), gh, gd in zip(names, shapes, got_host, got_dev):
        assert gh.tobytes() == data, name
        assert gd.cpu().numpy().tobytes() == data, name
        assert gen.oracle_decode(frame) == data, name
        assert blosc.cbuffer_sizes(_dev(frame, device))[:2] == (len(data), len(frame))
    # and one at a time, through the codec
    codec = blosc.Blosc()
    for name, data, frame in shapes:
        assert codec.decode(frame).tobytes() == data, name


# 3 ------------------------------------------------------------------------
def test_hand_assembled_sequences(device, sequences):
    assert {f"offset{o}" for o in (1, 2, 3, 4, 7, 8, 63, 64, 65, 255, 256, 65535)} <= {n for n, _f, _o in sequences}
    for name, frame, out in sequences:  # one launch each: a stream alone on the device
        got = blosc.decompress(_dev(frame, device))
        assert got.cpu().numpy().tobytes() == out, name
    got = blosc.decompress_many([f for _n, f, _o in sequences])
    for (name, _f, out), g in zip(sequences, got):
        assert g.tobytes() == out, name


# 4 ------------------------------------------------------------------------
def _batch64(shapes, sequences):
    frames = [f for _n, _d, f in shapes] + [f for _n, f, _o in sequences]
    expect = [d for _n, d, _f in shapes] + [o for _n, _f, o in sequences]
    k = 0
    while len(frames) < 64:
        n, ts = 3000 + 517 * k, (1, 2, 4, 8)[k % 4]
        data = gen._payload(n // ts * ts, 100 + k)
        frames.append(gen.blosc_frame(data, ts, 1024 // ts * ts, (k % 3)))
        expect.append(data)
        k += 1
    return frames[:64], expect[:64]


def test_batch(device, shapes, sequences):
    frames, expect = _batch64(shapes, sequences)
    assert len(frames) == 64
    single = [blosc.decompress(f).tobytes() for f in frames]
    assert single == expect
    # mixed host and device frames in one call
    mixed = [(_dev(f, device) if i % 2 else f) for i, f in enumerate(frames)]
    got = blosc.decompress_many(mixed)
    for i, g in enumerate(got):
        assert (g.is_cuda if i % 2 else isinstance(g, np.ndarray)), i
        assert (g.cpu().numpy() if i % 2 else g).tobytes() == expect[i], i
    # caller-provided outs: device tensors, host arrays and None mixed
    outs = []
    for i, e in enumerate(expect):
        outs.append(None if i % 3 == 0 else torch.zeros(len(e), dtype=torch.uint8, device=device) if i % 3 == 1
                    else np.zeros(len(e), np.uint8))
    got = blosc.decompress_many(frames, outs)
    for i, g in enumerate(got):
        if outs[i] is not None:
            assert g is outs[i], i
        assert (g.cpu().numpy() if torch.is_tensor(g) else np.asarray(g)).tobytes() == expect[i], i


def test_batch_with_one_malformed_frame(device, shapes):
    frames = [f for _n, _d, f in shapes][:12]
    bad = dict(gen.malformed_cases())["offset-beyond-produced"]
    assert gen.host_decode(bad)[0] == MALFORMED_CODES["offset-beyond-produced"]  # rejected on the CPU first
    with pytest.raises(RuntimeError, match=ERROR_RE) as info:
        blosc.decompress_many(frames[:5] + [bad] + frames[5:])
    assert list(info.value.frame_errors) == [5]
    assert info.value.frame_errors[5][0] == MALFORMED_CODES["offset-beyond-produced"]


# 5 ------------------------------------------------------------------------
def test_out_semantics(device, shapes):
    _name, data, frame = next(c for c in shapes if c[0] == "ts4-split-shuffle")
    codec = blosc.Blosc()
    out = torch.zeros(len(data), dtype=torch.uint8, device=device)
    got = codec.decode(_dev(frame, device), out=out)
    assert got is out and out.cpu().numpy().tobytes() == data
    typed = torch.zeros(len(data) // 4 + 1, dtype=torch.float32, device=device)  # larger, another dtype
    assert codec.decode(frame, out=typed) is typed
    assert typed.view(torch.uint8).cpu().numpy()[:len(data)].tobytes() == data
    small = torch.zeros(len(data) - 1, dtype=torch.uint8, device=device)
    with pytest.raises(ValueError, match=f"destination buffer too small; expected at least {len(data)}, got {len(data) - 1}"):
        codec.decode(_dev(frame, device), out=small)
    host = np.zeros(len(data), np.uint8)
    assert codec.decode(_dev(frame, device), out=host) is host and host.tobytes() == data
    host2 = np.zeros(len(data), np.uint8)
    assert codec.decode(frame, out=host2) is host2 and host2.tobytes() == data


# 6 ------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(MALFORMED_CODES))
def test_malformed_frame(device, shapes, name):
    frame = dict(gen.malformed_cases())[name]
    # only a frame the shared validation code rejected on the CPU is launched, once
    assert gen.host_decode(frame)[0] == MALFORMED_CODES[name]
    nbytes = int.from_bytes(frame[4:8], "little")
    guard = 4096
    buf = torch.full((guard + nbytes + guard,), 0x5A, dtype=torch.uint8, device=device)
    out = buf[guard:guard + nbytes]
    with pytest.raises(RuntimeError, match=ERROR_RE) as info:
        blosc.decompress(_dev(frame, device), out)
    assert info.value.frame_errors[0][0] == MALFORMED_CODES[name]
    assert bool((buf[:guard] == 0x5A).all()) and bool((buf[guard + nbytes:] == 0x5A).all())
    _n, data, good = shapes[0]
    assert blosc.decompress(_dev(good, device)).cpu().numpy().tobytes() == data
