"""GPU Blosc encode (numcodecs_amd.blosc.compress; csrc/mc_blosc_enc.hip):
exact equality with the host build of the shared scalar encoder and frame
layout (tests/native_lz4enc), round trips through the product's decoder and
the oracle's walker, batches, guard bytes around every slot, and the
``BloscLZ4`` codec.  Every stream is <= 256 KiB."""

import numpy as np
import pytest
import torch

from numcodecs_amd import _native, blosc, codec_registry, get_codec
from numcodecs_amd._native import lib
from tests import blosc_enc_gen as eg
from tests import blosc_gen as gen
from tests.helpers import fixture_cases

pytestmark = pytest.mark.gpu


def _dev(data, device):
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).to(device) if len(data) else \
        torch.empty(0, dtype=torch.uint8, device=device)


def _bytes(x):
    return (x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)).tobytes()


@pytest.fixture(scope="module")
def streams():
    return eg.stream_cases()


@pytest.fixture(scope="module")
def shapes():
    """(name, data, kwargs, the host model's frame)"""
    out = []
    for name, data, itemsize, shuffle, blocksize, clevel in eg.shape_params():
        kw = dict(cname="lz4", clevel=clevel, shuffle=shuffle, blocksize=blocksize, typesize=itemsize)
        out.append((name, data, kw, eg.host_frame(data, itemsize, clevel, shuffle, blocksize)))
    return out


# G1 -----------------------------------------------------------------------
def test_streams_equal_the_host_model(device, streams):
    """Each C1 stream as a one-block, one-stream frame, all in one batch."""
    expect = [eg.host_frame(d, 1, 5, blosc.NOSHUFFLE, max(len(d), 1)) for _n, d in streams]
    for (name, d), frame in zip(streams, expect):  # one block, one stream
        if d:
            assert int.from_bytes(frame[8:12], "little") == len(d), name
    got = blosc.compress_many([_dev(d, device) for _n, d in streams], "lz4", 5, blosc.NOSHUFFLE, 1 << 30, 1)
    for (name, _d), g, e in zip(streams, got, expect):
        assert g.is_cuda and g.dtype == torch.uint8
        assert _bytes(g) == e, name
    again = blosc.compress_many([_dev(d, device) for _n, d in streams], "lz4", 5, blosc.NOSHUFFLE, 1 << 30, 1)
    assert [_bytes(g) for g in again] == expect  # same input, same bytes


def test_frame_shapes_equal_the_host_model(device, shapes):
    for name, data, kw, expect in shapes:
        got = blosc.compress(_dev(data, device), **kw)
        assert _bytes(got) == expect, name
        host = blosc.compress(np.frombuffer(data, np.uint8), **kw)
        assert isinstance(host, np.ndarray) and host.dtype == np.uint8 and host.tobytes() == expect, name


# G2 -----------------------------------------------------------------------
def test_round_trip_shapes(device, shapes):
    for name, data, kw, _expect in shapes:
        frame = blosc.compress(_dev(data, device), **kw)
        assert _bytes(blosc.decompress(frame)) == data, name
        assert gen.oracle_decode(_bytes(frame)) == data, name


def test_round_trip_fixture_arrays(device):
    arrays = {}
    for arr, _j, _config, _frame in fixture_cases("blosc"):
        arrays.setdefault((arr.dtype.str, arr.tobytes(order="A")), arr)
    arrays = list(arrays.values())
    assert len(arrays) == 13
    raws = [a.tobytes(order="A") for a in arrays]
    for clevel, shuffle, blocksize in eg.LZ4_CONFIGS:
        # host buffers: the itemsize comes from each array
        frames = blosc.compress_many(arrays, "lz4", clevel, shuffle, blocksize)
        back = blosc.decompress_many(frames)
        for a, raw, f, b in zip(arrays, raws, frames, back):
            assert isinstance(f, np.ndarray) and b.tobytes() == raw
            assert f.tobytes() == eg.host_frame(raw, a.dtype.itemsize, clevel, shuffle, blocksize)
            assert gen.oracle_decode(f.tobytes()) == raw
        # device tensors (uint8: typesize 1 unless given)
        dframes = blosc.compress_many([_dev(r, device) for r in raws], "lz4", clevel, shuffle, blocksize)
        dback = blosc.decompress_many(dframes)
        for raw, f, b in zip(raws, dframes, dback):
            assert f.is_cuda and b.is_cuda and _bytes(b) == raw
            assert gen.oracle_decode(_bytes(f)) == raw


def test_typed_device_tensor_uses_its_itemsize(device):
    x = torch.cumsum(torch.randn(50000, device=device, generator=torch.Generator(device).manual_seed(3)) / 64, 0)
    frame = blosc.compress(x, "lz4", 5)
    raw = x.cpu().numpy().tobytes()
    assert _bytes(frame) == eg.host_frame(raw, 4, 5, blosc.SHUFFLE, 0)
    assert _bytes(frame)[3] == 4 and len(frame) < len(raw)
    assert torch.equal(blosc.decompress(frame).view(torch.float32), x)


# G3 -----------------------------------------------------------------------
def test_batch_mix(device):
    rng = np.random.default_rng(5)
    smooth = np.cumsum(rng.standard_normal(40000) / 64).astype("<f4")
    xs = [np.zeros(0, "<f4"), np.ones(1, np.uint8), rng.integers(0, 256, 9000, dtype=np.uint8).view("<f4"), smooth,
          smooth[:100], np.frombuffer(gen._payload(70001, 9), np.uint8), np.arange(5000, dtype="<i8"),
          np.zeros(30000, "<i2")]
    for kw in (dict(clevel=5, shuffle=blosc.SHUFFLE), dict(clevel=9, shuffle=blosc.BITSHUFFLE, blocksize=4096),
               dict(clevel=0), dict(clevel=1, shuffle=blosc.AUTOSHUFFLE, blocksize=256)):
        single = [blosc.compress(x, "lz4", kw.get("clevel"), kw.get("shuffle", 1), kw.get("blocksize", 0)).tobytes()
                  for x in xs]
        for x, s in zip(xs, single):
            assert s == eg.host_frame(x.tobytes(), x.dtype.itemsize, kw["clevel"], kw.get("shuffle", 1),
                                      kw.get("blocksize", 0))
        flags = [s[2] for s in single]
        if kw["clevel"] == 0:
            assert all(f & 2 for f in flags[1:])
        elif kw.get("blocksize", 0) == 0:
            assert flags[2] & 2 and not flags[3] & 2  # incompressible: memcpyed; smooth: compressed
            assert not flags[3] & 0x10 and flags[4] & 0x10  # split and unsplit
        mixed = [(_dev(x.tobytes(), device).view(torch.uint8) if i % 2 else x) for i, x in enumerate(xs)]
        got = blosc.compress_many(mixed, typesize=None, **kw)
        for i, (x, g, s) in enumerate(zip(xs, got, single)):
            assert (g.is_cuda if i % 2 else isinstance(g, np.ndarray)), i
            if i % 2 == 0:
                assert _bytes(g) == s, i
            assert _bytes(blosc.decompress(g)) == x.tobytes(), i


# G4 -----------------------------------------------------------------------
def test_guard_bytes_through_the_binding(device):
    GUARD = 256
    rng = np.random.default_rng(8)
    datas = [gen._payload(70000, 21), rng.integers(0, 256, 5000, dtype=np.uint8).tobytes(), bytes(3000),
             (np.frombuffer(gen._payload(12288 + 21, 22), np.uint8) >> 4).tobytes(), (bytes(range(8)) * 13)[:100]]
    params = [blosc._frame_params(len(d), ts, cl, sh, bs) for d, (ts, cl, sh, bs) in
              zip(datas, [(1, 5, 0, 0), (4, 5, 1, 0), (2, 0, 0, 0), (4, 5, 1, 4096), (8, 5, 0, 0)])]
    st = torch.cuda.current_stream(device).cuda_stream
    raws = [_dev(d, device) for d in datas]
    srcs = []
    for r, d, (flags, bs, ts, mode) in zip(raws, datas, params):
        if mode:
            f = torch.empty_like(r)
            _native.check(lib.mc_blosc_filter(r.data_ptr(), f.data_ptr(), len(d), ts, bs, mode, 1, st))
            srcs.append(f)
        else:
            srcs.append(r)
    out_off, scr_off, o, s = [], [], GUARD, GUARD
    for d in datas:
        out_off.append(o)
        scr_off.append(s)
        o += len(d) + 16 + GUARD
        s += len(d) + GUARD
    out = torch.full((o,), 0xA5, dtype=torch.uint8, device=device)
    table = np.zeros(len(datas), blosc._ENC_RECORD)
    nblocks = nstreams = 0
    for k, (d, (flags, bs, ts, _m)) in enumerate(zip(datas, params)):
        b, n, _longest = blosc._nstreams(flags, ts, len(d), bs)
        table[k] = (srcs[k].data_ptr(), raws[k].data_ptr(), out.data_ptr() + out_off[k], scr_off[k], len(d), bs, ts,
                    flags, nblocks, nstreams)
        nblocks, nstreams = nblocks + b, nstreams + n
    table_d = torch.from_numpy(table.view(np.uint8)).to(device)
    ws_bytes = lib.mc_blosc_encode_workspace(nstreams, s)
    ws = torch.full((ws_bytes + GUARD,), 0xA5, dtype=torch.uint8, device=device)
    cbytes = torch.zeros(len(datas), dtype=torch.int32, device=device)
    _native.check(lib.mc_blosc_encode_batch(None, table_d.data_ptr(), len(datas), nblocks, nstreams, ws.data_ptr(),
                                            ws_bytes, cbytes.data_ptr(), st))
    cb = cbytes.cpu().numpy()
    out_h, ws_h = out.cpu().numpy(), ws.cpu().numpy()
    scratch = ws_h[ws_bytes - s:ws_bytes]
    assert (ws_h[ws_bytes:] == 0xA5).all()
    keep_out, keep_scr = np.ones(o, bool), np.ones(s, bool)
    for k, d in enumerate(datas):
        keep_out[out_off[k]:out_off[k] + len(d) + 16] = False
        keep_scr[scr_off[k]:scr_off[k] + len(d)] = False
        frame = out_h[out_off[k]:out_off[k] + cb[k]].tobytes()
        ts, cl, sh, bs = [(1, 5, 0, 0), (4, 5, 1, 0), (2, 0, 0, 0), (4, 5, 1, 4096), (8, 5, 0, 0)][k]
        assert frame == eg.host_frame(d, ts, cl, sh, bs), k
        assert 16 < cb[k] <= len(d) + 16
    assert keep_out.sum() == GUARD * (len(datas) + 1) and (out_h[keep_out] == 0xA5).all()
    assert keep_scr.sum() == GUARD * (len(datas) + 1) and (scratch[keep_scr] == 0xA5).all()
    assert [bool(out_h[out_off[k] + 2] & 2) for k in range(5)] == [False, True, True, False, False]
    # a refused record (blocksize 0) writes nothing and reports cbytes 0
    out.fill_(0xA5)
    table["blocksize"][0] = 0
    table_d = torch.from_numpy(table.view(np.uint8)).to(device)
    _native.check(lib.mc_blosc_encode_batch(None, table_d.data_ptr(), len(datas), nblocks, nstreams, ws.data_ptr(),
                                            ws_bytes, cbytes.data_ptr(), st))
    cb2 = cbytes.cpu().numpy()
    assert cb2[0] == 0 and (cb2[1:] == cb[1:]).all()
    assert bool((out[:out_off[1]] == 0xA5).all())
    # argument checks
    assert lib.mc_blosc_encode_batch(None, table_d.data_ptr() + 4, 5, nblocks, nstreams, ws.data_ptr(), ws_bytes,
                                     cbytes.data_ptr(), st) == _native.MC_EINVAL
    assert lib.mc_blosc_encode_batch(None, table_d.data_ptr(), 5, 2**31, 2**31, ws.data_ptr(), ws_bytes,
                                     cbytes.data_ptr(), st) == _native.MC_EINVAL
    assert lib.mc_blosc_encode_batch(None, table_d.data_ptr(), 5, nblocks, nstreams, ws.data_ptr(), 64,
                                     cbytes.data_ptr(), st) == _native.MC_ENOSPC


# G5 -----------------------------------------------------------------------
def test_codec(device):
    x = torch.cumsum(torch.randn(1 << 16, device=device, generator=torch.Generator(device).manual_seed(1)) / 64, 0)
    codec = blosc.BloscLZ4()
    enc = codec.encode(x)
    assert enc.is_cuda and enc.dtype == torch.uint8 and enc.numel() < x.numel() * 4
    assert blosc.cbuffer_sizes(enc) == (x.numel() * 4, enc.numel(), x.numel() * 4)
    assert torch.equal(codec.decode(enc).view(torch.float32), x)
    out = torch.empty_like(x)
    assert codec.decode(enc, out=out) is out and torch.equal(out, x)
    before = dict(codec_registry)
    try:
        blosc.register(full=True)
        got = get_codec({"id": "blosc", "cname": "lz4", "clevel": 9, "shuffle": 2, "blocksize": 0})
        assert type(got) is blosc.BloscLZ4
        host = x.cpu().numpy()
        enc2 = got.encode(host)
        assert isinstance(enc2, np.ndarray) and enc2[2] & 4
        assert got.decode(enc2).tobytes() == host.tobytes()
    finally:
        codec_registry.pop("blosc", None)
    assert dict(codec_registry) == before
