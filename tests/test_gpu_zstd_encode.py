"""Zstd encode on the GPU (csrc/mc_zstd_enc.hip): every frame byte-equal to the
host model of csrc/mc_zstd_enc.h (tests/native_zstd_enc) and accepted by the
host decoder model and, where it loads, libzstd; batches of host and device
inputs, ``outs=``; device round trips through the zstd decoder; the Shuffle ->
zstd chain on the reference's fixture arrays; guard bytes and the refused short
slot through the C binding."""

import os

import numpy as np
import pytest
import torch

from numcodecs_amd import Shuffle, _zstd_enc, zstd_enc
from numcodecs_amd import zstd as nzstd
from numcodecs_amd._native import lib
from tests import zstd_enc_gen as eg
from tests import zstd_gen as zg
from tests.helpers import load_fixture_array

pytestmark = pytest.mark.gpu

CASES = [("empty", b"")] + eg.chunk_cases()
GUARD = 256
LIB = zg.load_lib()


def _dev(data, device):
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).to(device) if len(data) else \
        torch.empty(0, dtype=torch.uint8, device=device)


def _bytes(x):
    return (x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)).tobytes()


def _model(data, checksum=False):
    return eg.host_frame(data, checksum) if len(data) else _zstd_enc.empty_frame(checksum)


@pytest.mark.parametrize("checksum", [False, True])
def test_batch_equals_the_host_model(device, checksum):
    got = zstd_enc.compress_many([_dev(d, device) for _n, d in CASES], checksum=checksum)
    for (name, data), g in zip(CASES, got):
        assert g.is_cuda and g.dtype == torch.uint8, name
        frame = _bytes(g)
        assert frame == _model(data, checksum), name
        if len(data):
            rc, out, _w = zg.host_decode(frame)
            assert rc == 0 and out == data, name
            if LIB is not None:
                assert LIB.decompress(frame, len(data)) == (data, None), name


def test_one_input_alone_equals_the_host_model(device):
    for name, data in CASES:
        assert _bytes(zstd_enc.compress(_dev(data, device))) == _model(data), name
    for name in ("low13", "seam-runs", "mix3"):
        data = dict(CASES)[name]
        host = zstd_enc.compress(np.frombuffer(data, np.uint8), level=19, checksum=True)
        assert isinstance(host, np.ndarray) and host.dtype == np.uint8 and host.tobytes() == _model(data, True), name


def test_mixed_inputs_with_outs(device):
    picks = [dict(CASES)[n] for n in ("low13", "noise70000", "empty", "skewed70000", "low65537", "one-offset")]
    bufs = [(_dev(d, device) if i % 2 else np.frombuffer(d, np.uint8)) for i, d in enumerate(picks)]
    bounds = [_zstd_enc.bound(len(d)) for d in picks]
    outs = [None,
            torch.full((bounds[1] + 7,), 0xA5, dtype=torch.uint8, device=device),  # device source, device out
            np.full(bounds[2], 0xA5, np.uint8),                                    # empty, host out
            None,
            torch.full((bounds[4],), 0xA5, dtype=torch.uint8, device=device),      # host source, device out
            np.full(bounds[5] + 3, 0xA5, np.uint8)]                                # device source, host out
    got = zstd_enc.compress_many(bufs, outs=outs)
    for i, (d, g) in enumerate(zip(picks, got)):
        frame = _model(d)
        assert _bytes(g) == frame, i
        if outs[i] is None:
            assert (g.is_cuda if i % 2 else isinstance(g, np.ndarray)), i
        else:  # filled in place, from its start; the rest untouched
            assert _bytes(outs[i])[:len(frame)] == frame and set(_bytes(outs[i])[len(frame):]) <= {0xA5}, i
            if torch.is_tensor(outs[i]):
                assert g.data_ptr() == outs[i].data_ptr() and len(g) == len(frame), i
            else:
                assert g.base is outs[i] or g.base is outs[i].base, i
    with pytest.raises(ValueError, match="^destination buffer too small"):
        zstd_enc.compress_many([bufs[1]], outs=[torch.empty(bounds[1] - 1, dtype=torch.uint8, device=device)])


def test_device_round_trip(device, monkeypatch):
    """compress_many then the zstd decoder, with sizes= and without: the payload
    never visits the host, and the frames declare their size, so no sizing launch."""
    def no_sizing(*a, **k):
        raise AssertionError("the sizing launch ran")
    monkeypatch.setattr(lib, "mc_zstd_size_batch", no_sizing)
    datas = [d for _n, d in CASES if len(d)]
    srcs = [_dev(d, device) for d in datas]
    for checksum in (False, True):
        frames = zstd_enc.compress_many(srcs, checksum=checksum)
        for sizes in ([len(d) for d in datas], None):
            back = nzstd.decompress_many(frames, sizes=sizes)
            for s, b, f in zip(srcs, back, frames):
                assert f.is_cuda and b.is_cuda and torch.equal(s, b)


def test_shuffle_then_zstd_on_fixture_arrays(device):
    codec = zstd_enc.Zstd(level=1, checksum=True)
    for i in range(13):
        arr = load_fixture_array(os.path.join(zg.FIXTURE, "array.%02d.npy" % i))
        raw = np.frombuffer(arr.tobytes(order="A"), np.uint8)
        if len(raw) % 4 or len(raw) == 0:
            continue
        shuffled = Shuffle(4).encode(torch.from_numpy(raw.copy()).to(device))
        frame = codec.encode(shuffled)
        assert frame.is_cuda, i
        planes = codec.decode(frame)
        assert planes.is_cuda and torch.equal(planes, shuffled.view(torch.uint8).reshape(-1)), i
        back = planes.cpu().numpy().reshape(4, -1).T.reshape(-1)  # numpy's unshuffle
        assert back.tobytes() == raw.tobytes(), i


def _launch(datas, caps, checksum, device, ws_extra=GUARD):
    """mc_zstd_encode_batch on slots of caps[k] bytes with GUARD sentinel bytes around each."""
    n = len(datas)
    src = [_dev(d, device) for d in datas]
    offs, total = [], GUARD
    for c in caps:  # (slots at every alignment)
        offs.append(total)
        total += c + GUARD + 1
    out = torch.full((total,), 0xA5, dtype=torch.uint8, device=device)
    table = np.zeros(n, _zstd_enc._RECORD)
    nsegs = nseqs = 0
    for k, d in enumerate(datas):
        table[k] = (src[k].data_ptr(), out.data_ptr() + offs[k], len(d), caps[k], nsegs, nseqs, int(checksum), 0)
        nsegs += -(-len(d) // eg.SEGMENT)
        nseqs += -(-len(d) // 4)
    table_d = torch.from_numpy(table.view(np.uint8)).to(device)
    ws_bytes = lib.mc_zstd_encode_workspace(n, nsegs, nseqs)
    ws = torch.full((ws_bytes + ws_extra,), 0xA5, dtype=torch.uint8, device=device)
    words = torch.full((3 * n + 4,), 0x5A5A, dtype=torch.int32, device=device)
    rc = lib.mc_zstd_encode_batch(None, table_d.data_ptr(), n, nsegs, nseqs, ws.data_ptr(), ws_bytes, words.data_ptr(),
                                  words.data_ptr() + 4 * n, torch.cuda.current_stream(device).cuda_stream)
    assert rc == 0
    torch.cuda.synchronize(device)
    w = words.cpu().numpy()
    assert (w[3 * n:] == 0x5A5A).all() and (ws[ws_bytes:].cpu().numpy() == 0xA5).all()
    return out.cpu().numpy(), offs, w[:n].tolist(), w[n:3 * n].reshape(-1, 2)


def test_guard_bytes_through_the_binding(device):
    names = ("low1", "low13", "noise70000", "skewed70000", "low65536", "run70000", "wide-skewed", "mix3", "low257")
    datas = [dict(CASES)[n] for n in names]
    for checksum in (False, True):
        caps = [_zstd_enc.bound(len(d), checksum) for d in datas]  # slots of exactly the bound
        out, offs, sizes, err = _launch(datas, caps, checksum, device)
        assert not err.any()
        keep = np.ones(len(out), bool)
        for k, d in enumerate(datas):
            frame = _model(d, checksum)
            assert sizes[k] == len(frame) and out[offs[k]:offs[k] + sizes[k]].tobytes() == frame, names[k]
            keep[offs[k]:offs[k] + sizes[k]] = False
        assert (out[keep] == 0xA5).all()  # the sentinels, and every slot's bytes behind its frame
    # slots of exactly the frame; two of them one byte short: refused, nothing written, the error record set
    frames = [_model(d, True) for d in datas]
    for short in ((), (2, 4)):
        caps = [len(f) - (k in short) for k, f in enumerate(frames)]
        out, offs, sizes, err = _launch(datas, caps, True, device)
        for k, f in enumerate(frames):
            if k in short:
                assert sizes[k] == 0 and err[k].tolist() == [_zstd_enc.E_SPACE, len(f)], k
                assert (out[offs[k] - GUARD:offs[k] + caps[k] + GUARD] == 0xA5).all(), k
            else:
                assert sizes[k] == len(f) and not err[k].any() and out[offs[k]:offs[k] + len(f)].tobytes() == f, k
                assert (out[offs[k] + len(f):offs[k] + len(f) + GUARD] == 0xA5).all(), k
