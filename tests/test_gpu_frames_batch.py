"""The branch corners of the batch plumbing blosc.py and lz4.py share
(numcodecs_amd._frames), through the four ``*_many`` calls: every kind of
destination against every kind of source, batches whose destinations are all
the caller's, the single-piece staging branches, batches with nothing to
launch, and a zero-length buffer in the middle of an encode batch.  No payload
is above 64 KiB + 1."""

import numpy as np
import pytest
import torch

from numcodecs_amd import _frames, _native, blosc, lz4
from tests import blosc_enc_gen as eg
from tests import lz4_gen as lg

pytestmark = pytest.mark.gpu

SIZES = (1, 255, 256, 257, 65536, 65537)  # the last one spans two encode segments


def _dev(data, device):
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).to(device) if len(data) else \
        torch.empty(0, dtype=torch.uint8, device=device)


def _host(data):
    return np.frombuffer(data, np.uint8)


def _bytes(x):
    return (x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)).tobytes()


def _put(data, on_device, device):
    return _dev(data, device) if on_device else _host(data)


def _kind_follows(result, on_device):
    return (torch.is_tensor(result) and result.is_cuda and result.dtype == torch.uint8) if on_device else \
        (isinstance(result, np.ndarray) and result.dtype == np.uint8)


@pytest.fixture(scope="module")
def payloads():
    return [lg.low_entropy(n, 500 + k) for k, n in enumerate(SIZES)]


@pytest.fixture(scope="module")
def lz4_frames(payloads, device):
    """Per payload: the frame compress_many wrote (from alternating host and
    device sources), which is the host model's."""
    got = lz4.compress_many([_put(d, k % 2, device) for k, d in enumerate(payloads)])
    frames = [_bytes(g) for g in got]
    assert frames == [lg.host_frame(d) for d in payloads]
    return frames


def _blosc_kw(k):
    return [dict(clevel=5, shuffle=blosc.SHUFFLE, typesize=4), dict(clevel=5, shuffle=blosc.NOSHUFFLE, typesize=1),
            dict(clevel=0, shuffle=blosc.BITSHUFFLE, typesize=2)][k % 3]


# ---- decode: destinations --------------------------------------------------
def _destinations(datas, device):
    """outs cycling None / exact device tensor / exact host array / larger
    host bytearray, and sources host or device so that each kind of
    destination meets both kinds of source."""
    outs, src_dev = [], []
    for i, d in enumerate(datas):
        n = len(d)
        outs.append([None, torch.full((n,), 0xA5, dtype=torch.uint8, device=device), np.full(n, 0xA5, np.uint8),
                     bytearray(b"\xa5" * (n + 37))][i % 4])
        src_dev.append(bool((i // 4 + i) % 2))
    assert len({(i % 4, s) for i, s in enumerate(src_dev)}) == 8
    return outs, src_dev


def _check_destinations(got, outs, src_dev, datas):
    for i, (g, o, d) in enumerate(zip(got, outs, datas)):
        n = len(d)
        if o is None:
            assert _kind_follows(g, src_dev[i]), i
            assert _bytes(g) == d, i
        else:
            assert g is o, i
            assert _bytes(o)[:n] == d, i
            assert _bytes(o)[n:] == b"\xa5" * (len(o) - n), i  # past n: untouched


def test_lz4_destinations(device, payloads, lz4_frames):
    datas = payloads + payloads  # 12 frames: the second half meets the other kind of source
    frames = lz4_frames + [lg.host_frame(d) for d in payloads]
    outs, src_dev = _destinations(datas, device)
    got = lz4.decompress_many([_put(f, s, device) for f, s in zip(frames, src_dev)], outs)
    _check_destinations(got, outs, src_dev, datas)


def test_blosc_destinations(device, payloads):
    datas = payloads + payloads
    frames = [eg.host_frame(d, kw["typesize"], kw["clevel"], kw["shuffle"], 0)
              for d, kw in ((d, _blosc_kw(k)) for k, d in enumerate(datas))]
    outs, src_dev = _destinations(datas, device)
    got = blosc.decompress_many([_put(f, s, device) for f, s in zip(frames, src_dev)], outs)
    _check_destinations(got, outs, src_dev, datas)


def test_own_buffer_is_empty_when_every_destination_is_a_device_tensor(device):
    sizes = [1, 255, 256, 257, 65537]
    outs = [torch.empty(n, dtype=torch.uint8, device=device) for n in sizes]
    own, own_off, final = _frames.place(range(len(sizes)), sizes, outs, device)
    assert own.numel() == 0 and own.device == device and own_off == {}
    assert [(final[i].data_ptr(), final[i].numel()) for i in range(len(sizes))] == \
        [(o.data_ptr(), n) for o, n in zip(outs, sizes)]
    own, own_off, _final = _frames.place([0, 2, 4], sizes, [None, outs[1], outs[2], None, None], device)
    assert own_off == {0: 0, 4: 256} and own.numel() == 256 + 65792  # 2 decodes in place, 1 and 3 are not live


def test_every_destination_is_a_device_tensor(device, payloads, lz4_frames):
    sizes = [len(d) for d in payloads]
    blosc_frames = [eg.host_frame(d, 4, 5, blosc.SHUFFLE, 0) for d in payloads]
    for decompress_many, frames in ((lz4.decompress_many, lz4_frames), (blosc.decompress_many, blosc_frames)):
        outs = [torch.full((n,), 0xA5, dtype=torch.uint8, device=device) for n in sizes]
        got = decompress_many([_put(f, k % 2, device) for k, f in enumerate(frames)], outs)
        assert all(g is o for g, o in zip(got, outs))
        assert [_bytes(o) for o in outs] == payloads


# ---- staging: exactly one piece of the other kind ---------------------------
@pytest.mark.parametrize("odd_one_on_device", [False, True])
def test_one_source_of_the_other_kind(device, payloads, lz4_frames, odd_one_on_device):
    """One host source among device sources (one upload of a single frame, not
    concatenated) and one device source among host sources (one device piece
    behind the uploaded blob): both codecs, both directions."""
    where = [odd_one_on_device if i == 2 else not odd_one_on_device for i in range(len(payloads))]
    blosc_frames = [eg.host_frame(d, 4, 5, blosc.SHUFFLE, 0) for d in payloads]
    for decompress_many, frames in ((lz4.decompress_many, lz4_frames), (blosc.decompress_many, blosc_frames)):
        got = decompress_many([_put(f, w, device) for f, w in zip(frames, where)])
        assert all(_kind_follows(g, w) for g, w in zip(got, where))
        assert [_bytes(g) for g in got] == payloads
    srcs = [_put(d, w, device) for d, w in zip(payloads, where)]
    got = lz4.compress_many(srcs)
    assert all(_kind_follows(g, w) for g, w in zip(got, where))
    assert [_bytes(g) for g in got] == lz4_frames
    got = blosc.compress_many(srcs, "lz4", 5, blosc.SHUFFLE, typesize=4)
    assert all(_kind_follows(g, w) for g, w in zip(got, where))
    assert [_bytes(g) for g in got] == blosc_frames
    # and a batch of one, either kind
    for w in (False, True):
        assert _bytes(lz4.decompress_many([_put(lz4_frames[3], w, device)])[0]) == payloads[3]
        assert _bytes(blosc.decompress_many([_put(blosc_frames[3], w, device)])[0]) == payloads[3]


# ---- nothing to launch -----------------------------------------------------
def test_blosc_batch_of_empty_frames_launches_nothing(device, monkeypatch):
    empty = blosc.compress(np.zeros(0, "<f4"), "lz4", 5).tobytes()
    assert len(empty) == 16
    frames = [_put(empty, k % 2, device) for k in range(6)]
    dev_out, host_out = torch.empty(0, dtype=torch.uint8, device=device), np.full(3, 0xA5, np.uint8)
    outs = [None, None, host_out, dev_out, None, None]

    def launched():
        raise AssertionError("a launch was prepared")

    monkeypatch.setattr(_native, "require_device", launched)
    got = blosc.decompress_many(frames, outs)
    assert got[2] is host_out and got[3] is dev_out and (host_out == 0xA5).all()
    for k in (0, 1, 4, 5):
        assert _kind_follows(got[k], k % 2) and len(got[k]) == 0
    assert got[1].device == device


# ---- encode: a zero-length buffer in the middle ----------------------------
def test_zero_length_buffer_in_the_middle(device, payloads):
    where = [bool(k % 2) for k in range(len(payloads))]
    srcs = [_put(d, w, device) for d, w in zip(payloads, where)]
    for compress_many, empty_len in ((lz4.compress_many, 5),
                                     (lambda s: blosc.compress_many(s, "lz4", 5, blosc.SHUFFLE, typesize=4), 16)):
        alone = [_bytes(compress_many([s])[0]) for s in srcs]
        plain = compress_many(srcs)
        for empty in (np.zeros(0, np.uint8), torch.empty(0, dtype=torch.uint8, device=device)):
            holed = compress_many(srcs[:3] + [empty] + srcs[3:])
            hole = holed.pop(3)
            assert _kind_follows(hole, torch.is_tensor(empty)) and len(hole) == empty_len
            assert all(_kind_follows(g, w) for g, w in zip(holed, where))
            assert [_bytes(g) for g in holed] == [_bytes(g) for g in plain] == alone
