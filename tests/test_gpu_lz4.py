"""GPU `lz4` codec (numcodecs_amd.lz4; csrc/mc_lz4_codec.hip): the encoder's
frames byte-equal to the host build of the scalar stitched model
(tests/native_lz4codec), the reference's fixture frames and long-range
hand-written frames through the decoder, the ``LZ4`` codec with ``out=``,
guard bytes around every slot, and malformed frames.  No chunk is above
~300 KB."""

import numpy as np
import pytest
import torch

from numcodecs_amd import _native, lz4
from numcodecs_amd._native import lib
from tests import blosc_enc_gen as eg
from tests import blosc_gen as gen
from tests import lz4_gen as lg

pytestmark = pytest.mark.gpu


def _dev(data, device):
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).to(device) if len(data) else \
        torch.empty(0, dtype=torch.uint8, device=device)


def _bytes(x):
    return (x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)).tobytes()


@pytest.fixture(scope="module")
def cases():
    """(name, data, the host model's frame); length 0 included (the host path)."""
    return [(n, d, lg.host_frame(d)) for n, d in [("empty", b"")] + lg.chunk_cases()]


# ---- encode: byte-equal to the host model ----------------------------------
def test_batch_equals_the_host_model(device, cases):
    got = lz4.compress_many([_dev(d, device) for _n, d, _f in cases])
    for (name, _d, frame), g in zip(cases, got):
        assert g.is_cuda and g.dtype == torch.uint8, name
        assert _bytes(g) == frame, name
    # host buffers and device tensors mixed: one upload, same bytes
    mixed = lz4.compress_many([(_dev(d, device) if i % 2 else np.frombuffer(d, np.uint8))
                               for i, (_n, d, _f) in enumerate(cases)], acceleration=7)
    for i, ((name, _d, frame), g) in enumerate(zip(cases, mixed)):
        assert (g.is_cuda if i % 2 else isinstance(g, np.ndarray)), name
        assert _bytes(g) == frame, name
    # and back, in one call, from that mix of host and device frames
    back = lz4.decompress_many(mixed[1:])
    for (name, d, _f), b in zip(cases[1:], back):
        assert _bytes(b) == d, name


def test_one_input_alone_equals_the_host_model(device, cases):
    by_name = {n: (d, f) for n, d, f in cases}
    for name in ("noise-middle", "seam266", "low1"):
        d, frame = by_name[name]
        assert _bytes(lz4.compress(_dev(d, device))) == frame, name
        host = lz4.compress(np.frombuffer(d, np.uint8))
        assert isinstance(host, np.ndarray) and host.dtype == np.uint8 and host.tobytes() == frame, name
    x = torch.cumsum(torch.randn(50000, device=device, generator=torch.Generator(device).manual_seed(3)) / 64, 0)
    frame = lz4.compress(x)  # a typed tensor: its bytes
    assert _bytes(frame) == lg.host_frame(x.cpu().numpy().tobytes())
    assert torch.equal(lz4.decompress(frame).view(torch.float32), x)


# ---- decode ----------------------------------------------------------------
def test_fixture_frames_decode_in_one_call(device):
    fx = lg.fixture_frames()
    assert len(fx) == 91
    frames = [(_dev(f, device) if k % 3 else np.frombuffer(f, np.uint8)) for k, (_i, _j, _raw, f) in enumerate(fx)]
    back = lz4.decompress_many(frames)
    for k, ((i, j, raw, _f), b) in enumerate(zip(fx, back)):
        assert (b.is_cuda if k % 3 else isinstance(b, np.ndarray)), (i, j)
        assert _bytes(b) == raw, (i, j)


def _periodic(period, n, seed):
    """Every `period` bytes the same 3000 noise bytes and 20000 zeros, then filler that differs each time."""
    head = lg._noise(3000, seed) + bytes(20000)
    return b"".join(head + lg.low_entropy(period - 23000, seed + 1 + k) for k in range(n // period + 1))[:n]


def test_long_range_frames(device):
    """Frames of tests/blosc_gen.lz4_compress (an unbounded dictionary): matches
    that reach back 65535 bytes and run across 64 KiB boundaries -- the ring
    wraps above one segment, which the fixtures never do."""
    datas = [_periodic(65535, 200000, 1), _periodic(40000, 200000, 3)]
    frames = []
    for d in datas:
        block = gen.lz4_compress(d)
        frames.append(len(d).to_bytes(4, "little") + block)
    seqs = eg.parse_block(frames[0][4:], 200000)
    assert sum(off == 65535 and ml >= 3000 for _l, off, ml in seqs) == 3  # at 65535, 131070 and 196605
    for f in frames:  # long matches whose source starts in another segment than they end in
        pos, crossing = 0, 0
        for lit, off, ml in eg.parse_block(f[4:], 200000):
            pos += lit
            crossing += off is not None and ml >= 3000 and (pos - off) // lg.SEGMENT != (pos + ml - 1) // lg.SEGMENT
            pos += ml
        assert crossing >= 2
    for f, d in zip(frames, datas):
        assert lg.host_decode(f) == (0, d)
    got = lz4.decompress_many([_dev(frames[0], device), np.frombuffer(frames[1], np.uint8)])
    assert got[0].is_cuda and _bytes(got[0]) == datas[0]
    assert isinstance(got[1], np.ndarray) and got[1].tobytes() == datas[1]


def test_codec_round_trip_with_out(device):
    x = (torch.arange(1 << 16, device=device) // 8).to(torch.float32)  # runs of equal words: it shrinks unshuffled
    codec = lz4.LZ4()
    enc = codec.encode(x)
    assert enc.is_cuda and enc.dtype == torch.uint8 and 4 < enc.numel() < x.numel() * 4
    assert _bytes(enc[:4]) == (x.numel() * 4).to_bytes(4, "little")
    assert torch.equal(codec.decode(enc).view(torch.float32), x)
    out = torch.empty_like(x)
    assert codec.decode(enc, out=out) is out and torch.equal(out, x)
    host = x.cpu().numpy()
    enc_h = lz4.LZ4(acceleration=0).encode(host)
    assert isinstance(enc_h, np.ndarray) and enc_h.tobytes() == _bytes(enc)
    out_h = np.zeros_like(host)
    assert codec.decode(enc_h, out=out_h) is out_h and np.array_equal(out_h, host)
    big = np.full(host.size + 10, 7, host.dtype)  # larger than needed: the rest is left alone
    assert codec.decode(enc, out=big) is big and np.array_equal(big[:host.size], host) and (big[host.size:] == 7).all()
    with pytest.raises(ValueError, match="^destination buffer too small; expected at least 262144, got 262140$"):
        codec.decode(enc, out=np.zeros(host.size - 1, host.dtype))
    with pytest.raises(ValueError, match="^destination buffer too small; expected at least 262144, got 262140$"):
        codec.decode(enc, out=torch.empty(host.size - 1, device=device))
    ro = np.zeros_like(host)
    ro.flags.writeable = False
    with pytest.raises(ValueError, match="^destination buffer is read-only$"):
        codec.decode(enc_h, out=ro)
    assert not ro.any()


# ---- guard bytes through the binding ---------------------------------------
def test_guard_bytes_through_the_binding(device, cases):
    GUARD = 256
    by_name = {n: d for n, d, _f in cases}
    datas = [by_name[n] for n in ("mix", "low13", "noise-middle", "seam521", "low65549", "low1")]
    st = torch.cuda.current_stream(device).cuda_stream
    raws = [_dev(d, device) for d in datas]
    out_off, scr_off, o, s, nsegs = [], [], GUARD, GUARD, 0
    table = np.zeros(len(datas), lz4._ENC_RECORD)
    for k, d in enumerate(datas):
        out_off.append(o)
        scr_off.append(s)
        table[k] = (raws[k].data_ptr(), o, s, len(d), lg.frame_slot(len(d)), nsegs, 0)
        o += lg.frame_slot(len(d)) + GUARD
        s += len(d) + GUARD
        nsegs += -(-len(d) // lg.SEGMENT)
    out = torch.full((o,), 0xA5, dtype=torch.uint8, device=device)
    table["dst"] += out.data_ptr()
    table_d = torch.from_numpy(table.view(np.uint8)).to(device)
    ws_bytes = lib.mc_lz4_encode_workspace(len(datas), nsegs, s)
    ws = torch.full((ws_bytes + GUARD,), 0xA5, dtype=torch.uint8, device=device)
    cbytes = torch.zeros(len(datas), dtype=torch.int32, device=device)
    _native.check(lib.mc_lz4_encode_batch(None, table_d.data_ptr(), len(datas), nsegs, ws.data_ptr(), ws_bytes,
                                          cbytes.data_ptr(), st))
    cb = cbytes.cpu().numpy()
    out_h, ws_h = out.cpu().numpy(), ws.cpu().numpy()
    scratch = ws_h[ws_bytes - s:ws_bytes]
    assert (ws_h[ws_bytes:] == 0xA5).all()
    keep_out, keep_scr = np.ones(o, bool), np.ones(s, bool)
    for k, d in enumerate(datas):
        keep_out[out_off[k]:out_off[k] + lg.frame_slot(len(d))] = False
        keep_scr[scr_off[k]:scr_off[k] + len(d)] = False
        assert out_h[out_off[k]:out_off[k] + cb[k]].tobytes() == lg.host_frame(d), k
        # nothing behind the frame inside its slot either
        assert (out_h[out_off[k] + cb[k]:out_off[k] + lg.frame_slot(len(d))] == 0xA5).all(), k
    assert keep_out.sum() == GUARD * (len(datas) + 1) and (out_h[keep_out] == 0xA5).all()
    assert keep_scr.sum() == GUARD * (len(datas) + 1) and (scratch[keep_scr] == 0xA5).all()

    # refused records write nothing and report 0: nbytes 0, a slot one byte
    # short of the frame, a scratch range outside the batch's
    out.fill_(0xA5)
    bad = table.copy()
    bad["nbytes"][1] = 0
    bad["dst_cap"][2] = cb[2] - 1
    bad["scratch_off"][3] = s
    bad_d = torch.from_numpy(bad.view(np.uint8)).to(device)
    _native.check(lib.mc_lz4_encode_batch(None, bad_d.data_ptr(), len(datas), nsegs, ws.data_ptr(), ws_bytes,
                                          cbytes.data_ptr(), st))
    cb2 = cbytes.cpu().numpy()
    assert list(cb2[1:4]) == [0, 0, 0] and cb2[0] == cb[0] and (cb2[4:] == cb[4:]).all()
    out_h2 = out.cpu().numpy()
    assert (out_h2[out_off[1] - GUARD:out_off[4]] == 0xA5).all()
    for k in (0, 4, 5):
        assert out_h2[out_off[k]:out_off[k] + cb[k]].tobytes() == lg.host_frame(datas[k]), k
    # argument checks
    args = (nsegs, ws.data_ptr(), ws_bytes, cbytes.data_ptr(), st)
    assert lib.mc_lz4_encode_batch(None, table_d.data_ptr() + 4, len(datas), *args) == _native.MC_EINVAL
    assert lib.mc_lz4_encode_batch(None, table_d.data_ptr(), len(datas), 2**31, *args[1:]) == _native.MC_EINVAL
    assert lib.mc_lz4_encode_batch(None, table_d.data_ptr(), len(datas), nsegs, ws.data_ptr(), 64,
                                   cbytes.data_ptr(), st) == _native.MC_ENOSPC

    # decode: the frames just written, into guarded destinations
    frames = [out_h[out_off[k]:out_off[k] + cb[k]] for k in range(len(datas))]
    src = torch.from_numpy(np.concatenate(frames)).to(device)
    dst_off, p = [], GUARD
    for d in datas:
        dst_off.append(p)
        p += len(d) + GUARD
    dst = torch.full((p,), 0xA5, dtype=torch.uint8, device=device)
    dtab = np.zeros(len(datas), lz4._DEC_RECORD)
    pos = 0
    for k, d in enumerate(datas):
        dtab[k] = (pos, len(frames[k]), dst.data_ptr() + dst_off[k], len(d), 0)
        pos += len(frames[k])
    dtab_d = torch.from_numpy(dtab.view(np.uint8)).to(device)
    dws_bytes = lib.mc_lz4_decode_workspace(len(datas))
    dws = torch.full((dws_bytes + GUARD,), 0xA5, dtype=torch.uint8, device=device)
    err = torch.full((2 * len(datas) + 16,), 0x5A5A, dtype=torch.int32, device=device)
    longest = max(len(d) for d in datas)
    _native.check(lib.mc_lz4_decode_batch(src.data_ptr(), dtab_d.data_ptr(), len(datas), longest, dws.data_ptr(),
                                          dws_bytes, err.data_ptr(), st))
    err_h, dst_h = err.cpu().numpy(), dst.cpu().numpy()
    assert (err_h[2 * len(datas):] == 0x5A5A).all() and (dws.cpu().numpy()[dws_bytes:] == 0xA5).all()
    assert err_h[:2 * len(datas)].reshape(-1, 2).tolist() == [[0, len(d)] for d in datas]
    keep = np.ones(p, bool)
    for k, d in enumerate(datas):
        keep[dst_off[k]:dst_off[k] + len(d)] = False
        assert dst_h[dst_off[k]:dst_off[k] + len(d)].tobytes() == d, k
    assert keep.sum() == GUARD * (len(datas) + 1) and (dst_h[keep] == 0xA5).all()
    # a record whose size word disagrees with the frame's is refused by the plan: nothing written
    dst.fill_(0xA5)
    dtab["usize"][0] -= 1
    dtab_d = torch.from_numpy(dtab.view(np.uint8)).to(device)
    _native.check(lib.mc_lz4_decode_batch(src.data_ptr(), dtab_d.data_ptr(), len(datas), longest, dws.data_ptr(),
                                          dws_bytes, err.data_ptr(), st))
    codes = err.cpu().numpy()[:2 * len(datas)].reshape(-1, 2)
    assert codes[0].tolist() == [12, 0] and not codes[1:, 0].any()
    assert bool((dst[:dst_off[1]] == 0xA5).all())
    assert lib.mc_lz4_decode_batch(src.data_ptr(), dtab_d.data_ptr(), len(datas), 1 << 30, dws.data_ptr(),
                                   dws_bytes, err.data_ptr(), st) == _native.MC_EINVAL
    assert lib.mc_lz4_decode_batch(src.data_ptr(), dtab_d.data_ptr(), len(datas), longest, dws.data_ptr(), 8,
                                   err.data_ptr(), st) == _native.MC_ENOSPC


# ---- malformed frames ------------------------------------------------------
def _frame(usize, block):
    return np.frombuffer(usize.to_bytes(4, "little") + block, np.uint8)


def test_malformed_frames(device):
    """Every one is rejected by the sequence predicate before a byte of the
    offending sequence is copied (csrc/mc_lz4.h); the codes are its."""
    data = lg.low_entropy(3000, 7)
    good = np.frombuffer(lg.host_frame(data), np.uint8)
    block = good[4:].tobytes()
    tail = bytes([0x50]) + b"vwxyz"
    offset0 = _frame(13, bytes([0x40]) + b"abcd" + b"\x00\x00" + tail)   # a match 0 bytes back
    beyond = _frame(13, bytes([0x40]) + b"abcd" + b"\x05\x00" + tail)    # 5 back with 4 produced
    assert lg.host_decode(_frame(13, bytes([0x40]) + b"abcd" + b"\x04\x00" + tail).tobytes()) == (0, b"abcdabcdvwxyz")
    # the closing sequence holds >= 5 literals: 3 bytes short, its run leaves the source
    truncated = good[:-3]
    larger = _frame(3007, block)    # the block produces 3000 of 3007
    smaller = _frame(2999, block)   # the closing literals leave the destination
    expect = [(offset0, 7, "^LZ4 decompression error: -7$"), (beyond, 8, "^LZ4 decompression error: -8$"),
              (truncated, 5, "^LZ4 decompression error: -5$"),
              (larger, 10, "^LZ4 decompression error: expected to decompress 3007, got 3000$"),
              (smaller, 6, "^LZ4 decompression error: -6$")]
    for frame, code, text in expect:
        assert lg.host_decode(frame.tobytes())[0] == code  # the host model agrees
        for f in (frame, _dev(frame.tobytes(), device)):
            with pytest.raises(RuntimeError, match=text) as e:
                lz4.decompress(f)
            assert list(e.value.frame_errors) == [0] and e.value.frame_errors[0][0] == code
    with pytest.raises(RuntimeError, match="got 3000") as e:
        lz4.decompress(larger)
    assert e.value.frame_errors == {0: (10, 3000)}
    # a mixed batch names only its bad frames; the text is the first one's
    batch = [good, _dev(offset0.tobytes(), device), _dev(good.tobytes(), device), larger, good, truncated]
    with pytest.raises(RuntimeError, match="^LZ4 decompression error: -7$") as e:
        lz4.decompress_many(batch)
    assert {i: c for i, (c, _m) in e.value.frame_errors.items()} == {1: 7, 3: 10, 5: 5}
    assert e.value.frame_errors[3] == (10, 3000)
    # the good frames still decode afterwards
    assert lz4.decompress(good).tobytes() == data
