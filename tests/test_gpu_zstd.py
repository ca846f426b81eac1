"""GPU zstd decode (numcodecs_amd.zstd; csrc/mc_zstd.hip): the reference's 130
fixture frames and the case list of tests/zstd_gen.py (frames made by libzstd
1.4.8 and by hand, stored under tests/golden) through ``decompress_many``,
byte-equal to the formulas' data, by all three routes (no size, ``sizes=``,
device ``outs``); the invalid cases with the reference's exception class and
text and ``frame_errors``; the kernel's error record against the host model of
the same header (tests/native_zstd) for every invalid frame and for every
single-byte corruption and truncation of two short frames; the ``out`` rules of
``Zstd.decode``; a batch of 64 mixed frames.  No libzstd is needed here."""

import hashlib

import numpy as np
import pytest
import torch

from numcodecs_amd import _native, _zstd
from numcodecs_amd import zstd as nzstd
from tests import zstd_gen as g

pytestmark = pytest.mark.gpu

VALID = g.valid_cases()
INVALID = g.invalid_cases()


def _dev(data, device):
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).to(device) if len(data) else \
        torch.empty(0, dtype=torch.uint8, device=device)


def _bytes(x):
    return (x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)).tobytes()


def _host(frame):
    return np.frombuffer(frame, np.uint8)


@pytest.fixture(scope="module")
def datas():
    return {name: g.data_of(name) for name, *_ in VALID}


def test_fixture_frames_decode_in_one_call(device):
    fx = g.fixture_frames()
    assert len(fx) == 130
    got = nzstd.decompress_many([_host(f) for _i, _j, _raw, f in fx])
    for (i, j, raw, _f), out in zip(fx, got):
        assert isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.tobytes() == raw, (i, j)
    got = nzstd.decompress_many([_dev(f, device) for _i, _j, _raw, f in fx])
    for (i, j, raw, _f), out in zip(fx, got):
        assert out.is_cuda and out.dtype == torch.uint8 and _bytes(out) == raw, (i, j)


def test_valid_cases_three_ways(device, datas):
    frames = [_dev(f, device) for _n, f, _s, _z in VALID]
    sizes = [z for _n, _f, _s, z in VALID]
    # no sizes: the declared size, or the sizing pass
    got, produced = _zstd.decode_many(frames)
    assert produced == sizes
    for (name, *_), out in zip(VALID, got):
        assert out.is_cuda and _bytes(out) == datas[name], name
    # sizes=: an upper bound for the frames that declare none
    got, produced = _zstd.decode_many(frames, sizes=[z + 5 for z in sizes])
    assert produced == sizes
    for (name, *_), out in zip(VALID, got):
        assert out.numel() == len(datas[name]) and _bytes(out) == datas[name], name
    # outs=: filled in place and handed back
    outs = [torch.full((z,), 0xA5, dtype=torch.uint8, device=device) for z in sizes]
    got, produced = _zstd.decode_many(frames, outs=outs)
    assert produced == sizes
    for (name, *_), out, given in zip(VALID, got, outs):
        assert out is given and _bytes(out) == datas[name], name
    # host frames come back as numpy arrays
    small = [(n, f) for n, f, _s, z in VALID if z <= 70000]
    got = nzstd.decompress_many([_host(f) for _n, f in small])
    for (name, _f), out in zip(small, got):
        assert isinstance(out, np.ndarray) and out.tobytes() == datas[name], name


def _expected(meta):
    want = g.expected_exception(meta)
    if want is None:  # the stated exceptions (tests/test_zstd_host.py)
        return (NotImplementedError, None) if meta["expect"] == "E_MEMBER" else \
            (RuntimeError, "Zstd decompression error: Corrupted block detected")
    return want


def test_invalid_cases_alone_and_in_a_batch(device, datas):
    for name, frame, meta in INVALID:
        cls, text = _expected(meta)
        with pytest.raises(cls) as ei:
            nzstd.decompress(_dev(frame, device))
        assert type(ei.value) is cls and (text is None or str(ei.value) == text), (name, str(ei.value))
        assert list(ei.value.frame_errors) == [0] and ei.value.frame_errors[0][0] == getattr(g, meta["expect"]), name
    good = [(n, f) for n, f, _s, z in VALID if z <= 3000]
    batch, bad_at = [], []
    for k, (name, frame, _m) in enumerate(INVALID):
        batch.append(_dev(good[k % len(good)][1], device))
        bad_at.append(len(batch))
        batch.append(_dev(frame, device))
    with pytest.raises(Exception) as ei:
        nzstd.decompress_many(batch)
    assert sorted(ei.value.frame_errors) == bad_at  # exactly the bad ones
    cls, text = _expected(INVALID[0][2])
    assert type(ei.value) is cls and str(ei.value) == text  # the first one's exception
    got = nzstd.decompress_many(batch[0::2])
    for k, out in enumerate(got):
        assert _bytes(out) == datas[good[k % len(good)][0]], k


def _device_records(frames, cap, device):
    """(codes, words, produced, outputs) of one mc_zstd_decode_batch over `frames`, `cap` bytes each."""
    nf = len(frames)
    offsets = np.concatenate([[0], np.cumsum([len(f) for f in frames])]).astype(np.int64)
    src = _dev(b"".join(frames) + bytes(16), device)
    dst = torch.full((nf * cap + 16,), 0xA5, dtype=torch.uint8, device=device)
    table = np.zeros(nf, dtype=_zstd._RECORD)
    for i, f in enumerate(frames):
        table[i] = (offsets[i], len(f), dst.data_ptr() + i * cap, cap, 0)
    table_d = torch.from_numpy(table.view(np.uint8).copy()).to(device)
    ws_bytes = _native.lib.mc_zstd_workspace(nf)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
    words = torch.empty(3 * nf, dtype=torch.int32, device=device)
    st = torch.cuda.current_stream(device).cuda_stream
    _native.check(_native.lib.mc_zstd_decode_batch(src.data_ptr(), table_d.data_ptr(), nf, cap, ws.data_ptr(), ws_bytes,
                                                   words.data_ptr(), words.data_ptr() + 4 * nf, st), "mc_zstd_decode_batch")
    host = words.cpu().numpy()
    err = host[nf:].reshape(-1, 2)
    out = dst.cpu().numpy()
    produced = host[:nf].view(np.uint32).tolist()
    return err[:, 0].tolist(), err[:, 1].view(np.uint32).tolist(), produced, \
        [out[i * cap:i * cap + cap].tobytes() for i in range(nf)]


def _compare_with_host_model(frames, cap, device):
    codes, words, produced, outs = _device_records(frames, cap, device)
    for i, f in enumerate(frames):
        rc, data, word = g.host_decode(f, cap)
        if rc == 0:
            assert (codes[i], produced[i]) == (0, len(data)) and outs[i][:len(data)] == data, i
        else:
            assert (codes[i], words[i]) == (rc, word), (i, codes[i], words[i], rc, word)
        assert outs[i][produced[i]:] == b"\xa5" * (cap - produced[i]), i  # nothing behind what was produced


def test_error_records_equal_the_host_models_invalid_cases(device):
    _compare_with_host_model([f for _n, f, _m in INVALID if len(f) < 4000], 4096, device)
    _compare_with_host_model([f for _n, f, _m in INVALID if len(f) >= 4000], 140000, device)


@pytest.mark.parametrize("kind", ["checksummed", "plain"])
def test_error_records_equal_the_host_models_mutations(device, kind):
    frame, name, verdicts = g.mutation_record(kind)
    muts = [m for _w, _a, m in g.mutations(frame)]
    assert len(muts) == 3 * len(frame) == len(verdicts)
    _compare_with_host_model(muts, 4 * len(g.data_of(name)) + 1024, device)


def test_out_rules_of_decode(device, datas):
    by = {n: f for n, f, _s, _z in VALID}
    z = nzstd.Zstd()
    data = datas["small_plain"]  # 1100 bytes, declared by small_plain, not by small_nosize
    assert _bytes(z.decode(_dev(by["small_plain"], device))) == data
    assert z.decode(_host(by["small_nosize"])).tobytes() == data  # through the sizing pass
    # a declared size: `out` may be larger, not smaller
    out = torch.zeros(1200, dtype=torch.uint8, device=device)
    assert z.decode(_dev(by["small_plain"], device), out) is out and _bytes(out)[:1100] == data
    with pytest.raises(ValueError, match="^destination buffer too small; expected at least 1100, got 1099$"):
        z.decode(_dev(by["small_plain"], device), torch.zeros(1099, dtype=torch.uint8, device=device))
    # no declared size: `out` must be of the very size
    out = np.zeros(1100, np.uint8)
    assert z.decode(_host(by["small_nosize"]), out) is out and out.tobytes() == data
    with pytest.raises(RuntimeError, match="^Zstd decompression error: expected to decompress 1200, got 1100$"):
        z.decode(_dev(by["small_nosize"], device), torch.zeros(1200, dtype=torch.uint8, device=device))
    with pytest.raises(RuntimeError, match="^Zstd decompression error: Destination buffer is too small$") as ei:
        z.decode(_dev(by["small_nosize"], device), torch.zeros(1099, dtype=torch.uint8, device=device))
    assert ei.value.frame_errors[0][0] == g.E_CAPACITY


def test_a_batch_of_64_mixed_frames(device, datas):
    pool = [(n, f) for n, f, _s, z in VALID if z <= 131073 and n != "raw_two_blocks"]
    fx = g.fixture_frames()
    frames, want = [], []
    for k in range(64):
        if k % 3 == 2:
            _i, _j, raw, f = fx[(k * 7) % len(fx)]
            frames.append(f)
            want.append(raw)
        else:
            name, f = pool[(k * 5) % len(pool)]
            frames.append(f)
            want.append(datas[name])
    got = nzstd.decompress_many([_dev(f, device) if k & 1 else _host(f) for k, f in enumerate(frames)])
    for k, (out, w) in enumerate(zip(got, want)):
        assert torch.is_tensor(out) == bool(k & 1) and hashlib.sha256(_bytes(out)).digest() == hashlib.sha256(w).digest(), k
