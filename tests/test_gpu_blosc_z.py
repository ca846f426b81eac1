"""GPU Blosc decode of frames with zstd and zlib streams (numcodecs_amd.blosc
with ``formats=DECODE_FORMATS`` / ``BloscFull``; csrc/mc_blosc_dec_z.hip) and
encode of zstd frames (``formats=ENCODE_FORMATS``; csrc/mc_blosc_enc.hip): the
reference's fixture frames, the committed frame shapes
(tests/golden/blosc_z_cases.*), mixed batches and malformed frames.  No stream
is above 320 KiB: the smallest shapes at which the kernels can go wrong."""

import numpy as np
import pytest
import torch

from numcodecs_amd import blosc
from oracle import blosc as oblosc
from tests import blosc_z_gen as gen
from tests.helpers import fixture_cases

pytestmark = pytest.mark.gpu

ERROR_RE = "^error during blosc decompression: -1$"
ALL = blosc.DECODE_FORMATS


def _dev(frame, device):
    return torch.frombuffer(bytearray(frame), dtype=torch.uint8).to(device)


@pytest.fixture(scope="module")
def fixtures():
    """The 26 zlib / zstd fixture frames, and as many lz4 / memcpyed ones to mix in."""
    z = [(frame, want) for codec in (6, 7) for _j, frame, want in gen.fixture_frames(codec)]
    others = []
    for arr, _j, _config, frame in fixture_cases("blosc"):
        if frame[2] >> 5 == oblosc.LZ4_FORMAT and len(others) < len(z):
            others.append((frame, arr.tobytes(order="A")))
    assert len(z) == 26 and len(others) == 26 and any(f[2] & 2 for f, _w in others) and any(f[2] & 2 for f, _w in z)
    return z, others


# 1 ------------------------------------------------------------------------
def test_fixture_frames_one_by_one(device, fixtures):
    codec = blosc.BloscFull()
    for frame, want in fixtures[0]:
        got = codec.decode(frame)
        assert isinstance(got, np.ndarray) and got.tobytes() == want


def test_fixture_frames_as_one_mixed_batch(device, fixtures):
    z, others = fixtures
    mixed = [p for pair in zip(z, others) for p in pair]  # zlib / zstd interleaved with lz4 / memcpyed
    got = blosc.decompress_many([_dev(f, device) for f, _w in mixed], formats=ALL)
    for g, (_f, want) in zip(got, mixed):
        assert g.is_cuda and g.dtype == torch.uint8 and g.cpu().numpy().tobytes() == want


# 2 ------------------------------------------------------------------------
@pytest.mark.parametrize("case", gen.valid_cases(), ids=lambda c: c[0])
def test_generated_shapes(device, case):
    _name, _fname, frame, data, _code, _bad = case
    got = blosc.decompress(frame, formats=ALL)
    assert isinstance(got, np.ndarray) and got.tobytes() == data
    got = blosc.BloscFull().decode(_dev(frame, device))
    assert got.is_cuda and got.cpu().numpy().tobytes() == data


def test_generated_shapes_as_one_batch_with_outs(device):
    """Host and device sources, both formats, zero-length frames and ``outs``
    in one batch: one plan launch and a decode launch per format."""
    cases = gen.valid_cases()
    srcs = [_dev(c[2], device) if k % 2 else c[2] for k, c in enumerate(cases)]
    outs = [None] * len(cases)
    for k, c in enumerate(cases):
        if k % 3 == 0:
            outs[k] = torch.full((len(c[3]) + 5,), 0xEE, dtype=torch.uint8, device=device)
        elif k % 3 == 1 and k % 2 == 0:
            outs[k] = np.full(len(c[3]) + 5, 0xEE, np.uint8)
    got = blosc.decompress_many(srcs, outs, formats=ALL)
    for k, (g, c) in enumerate(zip(got, cases)):
        if outs[k] is not None:
            assert g is outs[k]
            flat = g.cpu().numpy() if isinstance(g, torch.Tensor) else g
            assert flat[:len(c[3])].tobytes() == c[3] and (flat[len(c[3]):] == 0xEE).all(), c[0]
        else:
            assert isinstance(g, torch.Tensor) == bool(k % 2), c[0]
            assert (g.cpu().numpy() if k % 2 else g).tobytes() == c[3], c[0]


# 3 ------------------------------------------------------------------------
@pytest.mark.parametrize("case", gen.malformed_cases(), ids=lambda c: c[0])
def test_malformed_frames(device, case):
    """The frame is refused with the recorded code and stream, named by its
    place in the batch; the batch's other frames decode without it."""
    _name, fname, frame, _data, code, bad = case
    good = [c for c in gen.valid_cases() if c[0].endswith(("-ts4", "-short-last", "-raw-stream"))]
    assert len(good) == 6
    batch = [c[2] for c in good[:3]] + [frame] + [c[2] for c in good[3:]]
    with pytest.raises(RuntimeError, match=ERROR_RE) as exc:
        blosc.decompress_many(batch, formats=ALL)
    # the stream's index counts over the batch's streams: those of the three frames before it, then its own
    before = sum(gen.host_decode(c[2])[2]["nstreams"] for c in good[:3])
    assert exc.value.frame_errors == {3: (code, before + bad)}
    with pytest.raises(RuntimeError, match=ERROR_RE) as exc:
        blosc.BloscFull().decode(_dev(frame, device))
    assert exc.value.frame_errors == {0: (code, bad)}
    del batch[3]
    for g, c in zip(blosc.decompress_many(batch, formats=ALL), good):
        assert g.tobytes() == c[3]


def test_container_violation_of_a_zstd_frame(device):
    good = next(c[2] for c in gen.valid_cases() if c[0] == "zstd-short-last")
    cut = good[:-3]
    cut = cut[:12] + len(cut).to_bytes(4, "little") + cut[16:]
    with pytest.raises(RuntimeError, match=ERROR_RE) as exc:
        blosc.decompress(cut, formats=ALL)
    assert exc.value.frame_errors == {0: (gen.CONTAINER + 2, 1)}  # 64 + MC_LZ4_E_CBYTES, the last stream


# 4 ------------------------------------------------------------------------
def test_defaults_still_refuse_on_the_gpu_path(device):
    zstd = next(c[2] for c in gen.valid_cases() if c[0] == "zstd-ts4")
    with pytest.raises(NotImplementedError, match="zstd"):
        blosc.decompress(_dev(zstd, device))
    with pytest.raises(NotImplementedError, match="zstd"):
        blosc.BloscLZ4().decode(_dev(zstd, device))
    x = torch.arange(1000, dtype=torch.float32, device=device)
    with pytest.raises(NotImplementedError, match="zstd"):
        blosc.BloscLZ4(cname="zstd").encode(x)
    # a batch of lz4 frames takes the same path whatever `formats` allows
    lz4 = blosc.compress(x, "lz4", 5)
    assert torch.equal(blosc.decompress(lz4, formats=ALL).view(torch.float32), x)


# 5 ------------------------------------------------------------------------
# encode, cname='zstd' (csrc/mc_blosc_enc.hip: mc_blosc_encode_batch_z)
@pytest.fixture(scope="module")
def encode_models():
    """{case name: the host model's frame}: made once."""
    return {name: gen.host_encode(x, x.dtype.itemsize, **kw) for name, x, kw, _c in gen.encode_cases()}


def _check_frame(name, x, frame, model, compressible):
    """Byte equality to the host model, the length rules and the condition against a hollow pass."""
    got = frame.cpu().numpy().tobytes() if isinstance(frame, torch.Tensor) else frame.tobytes()
    assert got == model, name
    assert int.from_bytes(got[12:16], "little") == len(got) <= x.nbytes + 16, name
    assert got[:2] == b"\x02\x01" and got[2] >> 5 == gen.FMT_ZSTD and got[2] & 0x10, name
    if compressible:
        assert not got[2] & 2 and 2 * len(got) < x.nbytes, name
        assert all(len(s) < share for s, share in gen.streams_of(got)), name
    return got


@pytest.mark.parametrize("case", gen.encode_cases(), ids=lambda c: c[0])
def test_encode_cases(device, case, encode_models):
    name, x, kw, compressible = case
    xd = torch.from_numpy(x.copy()).to(device)
    frame = blosc.compress(xd, "zstd", kw["clevel"], kw["shuffle"], kw.get("blocksize", 0), formats=blosc.ENCODE_FORMATS)
    assert frame.is_cuda and frame.dtype == torch.uint8
    _check_frame(name, x, frame, encode_models[name], compressible)
    codec = blosc.BloscFull(cname="zstd", **kw)
    enc = codec.encode(x)  # a host source: a numpy frame
    assert isinstance(enc, np.ndarray)
    got = _check_frame(name, x, enc, encode_models[name], compressible)
    back = blosc.BloscFull().decode(enc)
    assert isinstance(back, np.ndarray) and back.tobytes() == x.tobytes()
    assert blosc.BloscFull().decode(frame).cpu().numpy().tobytes() == x.tobytes()
    if name == "raw-between":
        assert [len(s) == share for s, share in gen.streams_of(got)] == [False, True, False]
    if name in ("all-noise", "clevel0"):
        assert got[2] & 2 and got[16:] == x.tobytes()


def test_encode_batch_mixing_host_and_device_sources(device, encode_models):
    """One compress_many call per configuration over host and device sources
    alike: every frame the host model's, and the batch decodes back in one call."""
    cases = [c for c in gen.encode_cases() if c[2] == dict(clevel=5, shuffle=gen.NOSHUFFLE, blocksize=4096)]
    assert len(cases) >= 2
    more = [("ramp-a", gen.ramp_f32(3000).view(np.uint8)), ("ramp-b", gen.ramp_f32(4096 * 5).view(np.uint8))]
    xs = [c[1] for c in cases] + [x for _n, x in more]
    srcs = [torch.from_numpy(x.copy()).to(device) if k % 2 else x for k, x in enumerate(xs)]
    frames = blosc.compress_many(srcs, cname="zstd", clevel=5, shuffle=gen.NOSHUFFLE, blocksize=4096,
                                 formats=blosc.ENCODE_FORMATS)
    for k, (f, x) in enumerate(zip(frames, xs)):
        assert isinstance(f, torch.Tensor) == bool(k % 2)
        model = gen.host_encode(x, 1, clevel=5, shuffle=gen.NOSHUFFLE, blocksize=4096)
        assert (f.cpu().numpy() if k % 2 else f).tobytes() == model
        assert len(model) <= x.nbytes + 16
    back = blosc.decompress_many(frames, formats=blosc.DECODE_FORMATS)
    for k, (b, x) in enumerate(zip(back, xs)):
        assert (b.cpu().numpy() if k % 2 else b).tobytes() == x.tobytes()
