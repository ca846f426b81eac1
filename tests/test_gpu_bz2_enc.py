"""bz2 encode on the GPU (csrc/mc_bz2_enc.hip): every frame byte-equal to the
host model of csrc/mc_bz2_enc.h (tests/native_bz2_enc) and read back by the
stdlib; round trips through the codec class; a batch of host and device inputs
with ``outs=`` and its one read-back; more blocks than resident sort
workgroups; device frames fed to the device decoder; guard bytes and the
refused short slot through the C binding."""

import bz2

import numpy as np
import pytest
import torch

from numcodecs_amd import _bz2_enc, bz2_enc
from numcodecs_amd import bz2 as nbz2
from numcodecs_amd._native import lib
from tests import bz2_enc_gen as g

pytestmark = pytest.mark.gpu

CASES = g.case_levels()
BY_NAME = dict((n, d) for n, d, _l in g.chunk_cases())
GUARD = 256


def _dev(data, device):
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).to(device) if len(data) else \
        torch.empty(0, dtype=torch.uint8, device=device)


def _bytes(x):
    return (x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)).tobytes()


def _model(data, level):
    return g.host_frame(data, level) if len(data) else _bz2_enc.empty_frame(level)


@pytest.mark.parametrize("level", [1, 5, 9])
def test_batch_equals_the_host_model(device, level):
    picks = [(n, d) for n, d, lv in CASES if lv == level]
    got = bz2_enc.compress_many([_dev(d, device) for _n, d in picks], level)
    for (name, data), f in zip(picks, got):
        assert f.is_cuda and f.dtype == torch.uint8, name
        frame = _bytes(f)
        assert frame == _model(data, level), name
        assert bz2.decompress(frame) == data, name


def test_codec_round_trips(device):
    data = BY_NAME["mixed"]
    codec = bz2_enc.BZ2(level=1)
    enc = codec.encode(_dev(data, device))  # device in, device out
    assert enc.is_cuda and _bytes(enc) == _model(data, 1)
    dec = codec.decode(enc)
    assert dec.is_cuda and _bytes(dec) == data
    host = codec.encode(np.frombuffer(data, np.uint8))  # host in, host out
    assert isinstance(host, np.ndarray) and host.dtype == np.uint8 and host.tobytes() == _model(data, 1)
    back = codec.decode(host)
    assert isinstance(back, np.ndarray) and back.tobytes() == data
    out = torch.empty(len(data), dtype=torch.uint8, device=device)  # into a given out
    assert codec.decode(enc, out=out) is out and _bytes(out) == data
    hout = np.empty(len(data), np.uint8)
    codec.decode(host, out=hout)
    assert hout.tobytes() == data


def test_mixed_batch_with_outs_and_one_read_back(device, monkeypatch):
    names = ("len1", "noise", "len0", "run-straddle", "text159975", "run260", "len0", "zrun1024", "nsym2400", "ab1000")
    picks = [BY_NAME[n] for n in names]
    bufs = [(_dev(d, device) if i % 2 else np.frombuffer(d, np.uint8)) for i, d in enumerate(picks)]
    bounds = [_bz2_enc.bound(len(d), 1) for d in picks]
    outs = [None,
            torch.full((bounds[1] + 7,), 0xA5, dtype=torch.uint8, device=device),  # device source, device out
            np.full(bounds[2], 0xA5, np.uint8),                                    # empty, host out
            None,
            torch.full((bounds[4],), 0xA5, dtype=torch.uint8, device=device),      # host source, device out
            np.full(bounds[5] + 3, 0xA5, np.uint8),                                # device source, host out
            None, None, None,
            torch.full((bounds[9] + 1,), 0xA5, dtype=torch.uint8, device=device)[1:]]  # an odd address
    got = bz2_enc.compress_many(bufs, 1, outs=outs)
    for i, (d, f) in enumerate(zip(picks, got)):
        frame = _model(d, 1)
        assert _bytes(f) == frame, names[i]
        assert _bytes(bz2_enc.compress(bufs[i], 1)) == frame, names[i]  # one at a time: the same
        if outs[i] is None:
            assert (f.is_cuda if i % 2 else isinstance(f, np.ndarray)), i
        else:  # filled in place, from its start; the rest untouched
            assert _bytes(outs[i])[:len(frame)] == frame and set(_bytes(outs[i])[len(frame):]) <= {0xA5}, i
            if torch.is_tensor(outs[i]):
                assert f.data_ptr() == outs[i].data_ptr() and len(f) == len(frame), i
    with pytest.raises(ValueError, match="^destination buffer too small"):
        bz2_enc.compress_many([bufs[1]], outs=[torch.empty(bounds[1] - 1, dtype=torch.uint8, device=device)])
    # all on the device: the sizes and error words come back in one copy, and nothing else does
    srcs = [_dev(d, device) for d in picks]
    calls = []
    real = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (calls.append(self.dtype), real(self, *a, **k))[1])
    res = bz2_enc.compress_many(srcs, 1)
    monkeypatch.undo()
    assert calls == [torch.int32]
    assert all(r.is_cuda for r in res)


def test_more_blocks_than_resident_sort_workgroups(device):
    rng = np.random.default_rng(77)
    small = [(np.cumsum(rng.integers(-1, 2, 8000)) % 11).astype(np.uint8) for _ in range(8)]
    datas = [small[i % 8][i:].tobytes() for i in range(300)] + [BY_NAME["text159975"]]
    got = bz2_enc.compress_many([_dev(d, device) for d in datas], 1)
    for i, (d, f) in enumerate(zip(datas, got)):
        frame = _bytes(f)
        if i < 8 or i >= 296:
            assert frame == _model(d, 1), i
        assert bz2.decompress(frame) == d, i


def test_device_frames_feed_the_device_decoder(device):
    datas = [BY_NAME[n] for n in ("mixed", "zeros1M", "text159975", "alpha256", "len1", "shuffled-floats")]
    srcs = [_dev(d, device) for d in datas]
    frames = bz2_enc.compress_many(srcs, 1)
    back = nbz2.decompress_many(frames)
    for s, b, f in zip(srcs, back, frames):
        assert f.is_cuda and b.is_cuda and torch.equal(s, b)


def _launch(datas, caps, level, device):
    """mc_bz2_encode_batch on slots of caps[k] bytes with GUARD sentinel bytes around each."""
    n = len(datas)
    src = [_dev(d, device) for d in datas]
    offs, total = [], GUARD
    for c in caps:  # (slots at every alignment)
        offs.append(total)
        total += c + GUARD + 1
    out = torch.full((total,), 0xA5, dtype=torch.uint8, device=device)
    table = np.zeros(n, _bz2_enc._RECORD)
    nblocks = 0
    for k, d in enumerate(datas):
        table[k] = (src[k].data_ptr(), out.data_ptr() + offs[k], len(d), caps[k], nblocks, 0)
        nblocks += -(-len(d) // g.seg(level))
    table_d = torch.from_numpy(table.view(np.uint8)).to(device)
    max_chunk = max(len(d) for d in datas)
    ws_bytes = lib.mc_bz2_encode_workspace(n, nblocks, max_chunk, level)
    ws = torch.full((ws_bytes + GUARD,), 0xA5, dtype=torch.uint8, device=device)
    words = torch.full((3 * n + 8,), 0x5A5A, dtype=torch.int32, device=device)
    rc = lib.mc_bz2_encode_batch(table_d.data_ptr(), n, nblocks, max_chunk, level, ws.data_ptr(), ws_bytes,
                                 words.data_ptr(), words.data_ptr() + 4 * n, torch.cuda.current_stream(device).cuda_stream)
    assert rc == 0
    torch.cuda.synchronize(device)
    w = words.cpu().numpy()
    assert (w[3 * n:] == 0x5A5A).all() and (ws[ws_bytes:].cpu().numpy() == 0xA5).all()
    return out.cpu().numpy(), offs, w[:n].tolist(), w[n:3 * n].reshape(-1, 2)


def test_guards_and_short_slots_through_the_c_binding(device):
    names = ("len1", "run260", "ab33", "nsym600", "mixed", "text159975", "len5")
    datas = [BY_NAME[n] for n in names]
    frames = [_model(d, 1) for d in datas]
    assert lib.mc_bz2_encode_bound(len(datas[4]), 1) == _bz2_enc.bound(len(datas[4]), 1)
    # exactly the frame's length succeeds; nothing outside a slot is written
    out, offs, sizes, err = _launch(datas, [len(f) for f in frames], 1, device)
    at = 0
    for k, f in enumerate(frames):
        assert sizes[k] == len(f) and err[k].tolist() == [0, 0], names[k]
        assert out[offs[k]:offs[k] + len(f)].tobytes() == f, names[k]
        assert (out[at:offs[k]] == 0xA5).all(), names[k]
        at = offs[k] + len(f)
    assert (out[at:] == 0xA5).all()
    # one byte short: refused with the size it needs, the slot untouched; the others unaffected
    caps = [len(f) - (1 if k % 2 == 0 else 0) for k, f in enumerate(frames)]
    out, offs, sizes, err = _launch(datas, caps, 1, device)
    at = 0
    for k, f in enumerate(frames):
        if k % 2 == 0:
            assert sizes[k] == 0 and err[k].tolist() == [_bz2_enc.E_SPACE, len(f)], names[k]
            continue
        assert sizes[k] == len(f) and err[k].tolist() == [0, 0], names[k]
        assert out[offs[k]:offs[k] + len(f)].tobytes() == f, names[k]
        assert (out[at:offs[k]] == 0xA5).all(), names[k]
        at = offs[k] + len(f)
    assert (out[at:] == 0xA5).all()
