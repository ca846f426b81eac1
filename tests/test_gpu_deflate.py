"""zlib / gzip encode on the GPU (csrc/mc_deflate.hip): every frame byte-equal to
the host model of csrc/mc_deflate.h (tests/native_deflate) and accepted by the
stdlib; batches of host and device inputs, ``outs=``; device round trips through
the inflater; the Shuffle -> deflate chain on the reference's fixture arrays;
guard bytes and the refused short slot through the C binding; level 0."""

import gzip as _gzip
import os
import zlib as _zlib

import numpy as np
import pytest
import torch

from numcodecs_amd import Shuffle, _deflate, deflate
from numcodecs_amd import gzip as ngzip
from numcodecs_amd import zlib as nzlib
from numcodecs_amd._native import lib
from tests import deflate_gen as dg
from tests.helpers import FIXTURE, load_fixture_array

pytestmark = pytest.mark.gpu

CASES = [("empty", b"")] + dg.chunk_cases()
GUARD = 256


def _dev(data, device):
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).to(device) if len(data) else \
        torch.empty(0, dtype=torch.uint8, device=device)


def _bytes(x):
    return (x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)).tobytes()


def _model(data, container, level=1):
    return dg.host_frame(data, container, level) if len(data) else _deflate.empty_frame(dg.CONTAINERS[container])


def _stdlib(container, frame):
    return _zlib.decompress(frame) if container == "zlib" else _gzip.decompress(frame)


@pytest.mark.parametrize("container", ["zlib", "gzip"])
def test_batch_equals_the_host_model(device, container):
    got = deflate.compress_many([_dev(d, device) for _n, d in CASES], container=container)
    for (name, data), g in zip(CASES, got):
        assert g.is_cuda and g.dtype == torch.uint8, name
        frame = _bytes(g)
        assert frame == _model(data, container), name
        assert _stdlib(container, frame) == data, name


def test_one_input_alone_equals_the_host_model(device):
    for name, data in CASES:
        assert _bytes(deflate.compress(_dev(data, device))) == _model(data, "zlib"), name
    for name in ("low13", "seam-runs", "mix3"):
        data = dict(CASES)[name]
        host = deflate.compress(np.frombuffer(data, np.uint8), container="gzip", level=6)
        assert isinstance(host, np.ndarray) and host.dtype == np.uint8 and host.tobytes() == _model(data, "gzip"), name


def test_mixed_inputs_with_outs(device):
    picks = [dict(CASES)[n] for n in ("low13", "stored70000", "empty", "skewed70000", "low65537", "run517")]
    bufs = [(_dev(d, device) if i % 2 else np.frombuffer(d, np.uint8)) for i, d in enumerate(picks)]
    bounds = [_deflate.bound(len(d), _deflate.ZLIB) for d in picks]
    outs = [None,
            torch.full((bounds[1] + 7,), 0xA5, dtype=torch.uint8, device=device),  # device source, device out
            np.full(bounds[2], 0xA5, np.uint8),                                    # empty, host out
            None,
            torch.full((bounds[4],), 0xA5, dtype=torch.uint8, device=device),      # host source, device out
            np.full(bounds[5] + 3, 0xA5, np.uint8)]                                # device source, host out
    got = deflate.compress_many(bufs, "zlib", outs=outs)
    for i, (d, g) in enumerate(zip(picks, got)):
        frame = _model(d, "zlib")
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
        deflate.compress_many([bufs[1]], outs=[torch.empty(bounds[1] - 1, dtype=torch.uint8, device=device)])


def test_device_round_trip(device):
    """compress_many then the inflater with sizes=: the payload never visits the host."""
    datas = [d for _n, d in CASES if len(d)]
    srcs = [_dev(d, device) for d in datas]
    for container, mod in (("zlib", nzlib), ("gzip", ngzip)):
        frames = deflate.compress_many(srcs, container=container)
        back = mod.decompress_many(frames, sizes=[len(d) for d in datas])
        for s, b, f in zip(srcs, back, frames):
            assert f.is_cuda and b.is_cuda and torch.equal(s, b)


def test_shuffle_then_deflate_on_fixture_arrays(device):
    for i in (0, 1):  # int32 and float64, 1000 elements each: both as 4-byte elements
        arr = load_fixture_array(os.path.join(FIXTURE, "zlib", "array.%02d.npy" % i))
        raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
        shuffled = Shuffle(4).encode(torch.from_numpy(raw.copy()).to(device))
        frame = deflate.Zlib(level=1).encode(shuffled)
        assert frame.is_cuda, i
        planes = np.frombuffer(_zlib.decompress(_bytes(frame)), np.uint8)
        back = planes.reshape(4, -1).T.reshape(-1)  # numpy's unshuffle
        assert back.tobytes() == raw.tobytes(), i
        gz = deflate.GZip().encode(raw)
        assert isinstance(gz, np.ndarray) and _gzip.decompress(gz.tobytes()) == raw.tobytes(), i


def _launch(datas, caps, container, level, device, ws_extra=GUARD):
    """mc_deflate_encode_batch on slots of caps[k] bytes with GUARD sentinel bytes around each."""
    n = len(datas)
    src = [_dev(d, device) for d in datas]
    offs, total = [], GUARD
    for c in caps:  # (slots at every alignment)
        offs.append(total)
        total += c + GUARD + 1
    out = torch.full((total,), 0xA5, dtype=torch.uint8, device=device)
    table = np.zeros(n, _deflate._RECORD)
    nsegs = nseqs = 0
    for k, d in enumerate(datas):
        table[k] = (src[k].data_ptr(), out.data_ptr() + offs[k], len(d), caps[k], nsegs, container, level, nseqs)
        nsegs += -(-len(d) // dg.SEGMENT)
        nseqs += -(-len(d) // 4)
    table_d = torch.from_numpy(table.view(np.uint8)).to(device)
    ws_bytes = lib.mc_deflate_encode_workspace(n, nsegs, nseqs)
    ws = torch.full((ws_bytes + ws_extra,), 0xA5, dtype=torch.uint8, device=device)
    words = torch.full((3 * n + 4,), 0x5A5A, dtype=torch.int32, device=device)
    rc = lib.mc_deflate_encode_batch(None, table_d.data_ptr(), n, nsegs, nseqs, ws.data_ptr(), ws_bytes, words.data_ptr(),
                                     words.data_ptr() + 4 * n, torch.cuda.current_stream(device).cuda_stream)
    assert rc == 0
    torch.cuda.synchronize(device)
    w = words.cpu().numpy()
    assert (w[3 * n:] == 0x5A5A).all() and (ws[ws_bytes:].cpu().numpy() == 0xA5).all()
    return out.cpu().numpy(), offs, w[:n].tolist(), w[n:3 * n].reshape(-1, 2)


def test_guard_bytes_through_the_binding(device):
    names = ("low1", "low13", "stored70000", "skewed70000", "low65536", "run70000", "period32768", "mix3")
    datas = [dict(CASES)[n] for n in names]
    for container in (_deflate.ZLIB, _deflate.GZIP):
        cname = "gzip" if container else "zlib"
        caps = [_deflate.bound(len(d), container) for d in datas]  # slots of exactly the bound
        out, offs, sizes, err = _launch(datas, caps, container, 1, device)
        assert not err.any()
        keep = np.ones(len(out), bool)
        for k, d in enumerate(datas):
            frame = _model(d, cname)
            assert sizes[k] == len(frame) and out[offs[k]:offs[k] + sizes[k]].tobytes() == frame, names[k]
            keep[offs[k]:offs[k] + sizes[k]] = False
        assert (out[keep] == 0xA5).all()  # the sentinels, and every slot's bytes behind its frame
    # a slot one byte short of its frame: refused, nothing written, the error record set; its neighbours encoded
    frames = [_model(d, "zlib") for d in datas]
    caps = [len(f) for f in frames]
    caps[2] -= 1
    caps[4] -= 1
    out, offs, sizes, err = _launch(datas, caps, _deflate.ZLIB, 1, device)
    for k, f in enumerate(frames):
        if k in (2, 4):
            assert sizes[k] == 0 and err[k].tolist() == [_deflate.E_SPACE, len(f)], k
            assert (out[offs[k] - GUARD:offs[k] + caps[k] + GUARD] == 0xA5).all(), k
        else:
            assert sizes[k] == len(f) and not err[k].any() and out[offs[k]:offs[k] + len(f)].tobytes() == f, k


def test_level_0_is_stored(device):
    datas = [dict(CASES)[n] for n in ("low13", "low65537", "run70000")]
    for container in ("zlib", "gzip"):
        got = deflate.compress_many([_dev(d, device) for d in datas], container=container, level=0)
        for d, g in zip(datas, got):
            assert len(g) == _deflate.bound(len(d), dg.CONTAINERS[container])
            assert _bytes(g) == _model(d, container, 0) and _stdlib(container, _bytes(g)) == d
