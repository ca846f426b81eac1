"""Blosc encode, CPU side: the product's scalar LZ4 encoder and frame layout
compiled for the host (tests/native_lz4enc) against three independent
decoders, its output size against the test-side greedy writer, whole frames
against the oracle's walker and the reference's fixture headers, the
``compress`` / ``BloscLZ4`` surface, and the sanitized stand-alone run."""

import ctypes
import os
import subprocess

import numpy as np
import pytest

from numcodecs_amd import _native, blosc, codec_registry, get_codec
from oracle import blosc as oblosc
from tests import blosc_enc_gen as eg
from tests import blosc_gen as gen
from tests.helpers import fixture_cases
from tests.test_boundary import _header_functions


def _liblz4():
    try:
        lib = ctypes.CDLL("liblz4.so.1")
    except OSError:
        return None
    lib.LZ4_decompress_safe.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_int]
    lib.LZ4_decompress_safe.restype = ctypes.c_int
    return lib


STREAMS = eg.stream_cases()


# C1 -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def encoded_streams():
    return {name: eg.encode_stream(data) for name, data in STREAMS}


def test_stream_list_is_the_issues():
    names = [n for n, _d in STREAMS]
    assert len(names) == len(set(names)) == 17 + 2 + 2 + 2 + 6 + 6
    assert {len(d) for n, d in STREAMS if n.startswith("payload")} == \
        {0, 1, 4, 12, 13, 14, 63, 64, 65, 75, 76, 77, 127, 128, 129, 4096, 70000}


@pytest.mark.parametrize("name", [n for n, _d in STREAMS])
def test_scalar_encoder_stream(encoded_streams, name):
    data = dict(STREAMS)[name]
    n = len(data)
    comp = encoded_streams[name]
    if comp is None:  # stored raw
        return
    assert len(comp) < n
    assert oblosc.lz4_block_decompress(comp, n) == data
    back = np.zeros(n, np.uint8)
    assert gen.hostlib().hc_lz4_decode_stream(comp, len(comp), back.ctypes.data, n) == 0
    assert back.tobytes() == data
    eg.parse_block(comp, n)  # the block format's end rules


def test_scalar_encoder_expected_shapes(encoded_streams):
    """What the crafted streams are there for really happens."""
    data = dict(STREAMS)
    for name, d in STREAMS:
        if len(d) < 13:
            assert encoded_streams[name] is None, name  # literals only: stored raw
    assert encoded_streams["random5000"] is None
    zeros = eg.parse_block(encoded_streams["zeros140000"], 140000)
    assert zeros == [(1, 1, 139994), (5, None, 0)]  # several hundred 0xFF extension bytes
    assert encoded_streams["zeros140000"].count(b"\xff") >= 500
    near = eg.parse_block(encoded_streams["findable65535"], len(data["findable65535"]))
    assert (0, 65535, 3000) in near
    far = eg.parse_block(encoded_streams["findable65536"], len(data["findable65536"]))
    assert all(off is None or off < 65535 for _l, off, _m in far)
    for ll in (14, 15, 16, 269, 270, 271):
        seqs = eg.parse_block(encoded_streams[f"literals{ll}"], len(data[f"literals{ll}"]))
        assert [s[0] for s in seqs] == [64 + ll, ll, 16] and seqs[1][2] == 64, (ll, seqs)
    for ml in (18, 19, 20, 273, 274, 275):
        seqs = eg.parse_block(encoded_streams[f"match{ml}"], len(data[f"match{ml}"]))
        assert seqs == [(70 + ml, 30 + ml, ml), (20, None, 0)], (ml, seqs)


def test_scalar_encoder_against_liblz4(encoded_streams):
    lib = _liblz4()
    if lib is None:
        pytest.skip("liblz4.so.1 is not on this machine")
    checked = 0
    for name, data in STREAMS:
        comp = encoded_streams[name]
        if comp is None:
            continue
        out = ctypes.create_string_buffer(len(data))
        assert lib.LZ4_decompress_safe(comp, out, len(comp), len(data)) == len(data), name
        assert out.raw == data, name
        checked += 1
    assert checked >= 20


def test_scalar_encoder_is_deterministic():
    data = gen._payload(70000, 1)
    assert eg.encode_stream(data) == eg.encode_stream(bytes(bytearray(data)))


# C2 -----------------------------------------------------------------------
def test_size_against_the_greedy_writer():
    """Per input at most 1.10 x the size tests/blosc_gen.lz4_compress reaches
    with its unbounded dictionary (both capped at the stream's size: a stream
    that does not shrink is stored raw by either writer).  Measured:
    payload64k 1.074, smooth float32 planes 1.000 / 1.000 / 1.035 / 0.965,
    noise plane 3 0.998, int32 planes 1.000 / 0.975, zeros 1.000, text 0.999,
    payload300 1.000."""
    ratios = {}
    for name, data in eg.size_cases():
        comp = eg.encode_stream(data)
        ours = len(comp) if comp is not None else len(data)
        ref = min(len(gen.lz4_compress(data)), len(data))
        ratios[name] = ours / ref
        print(f"{name}: {ours} / {ref} = {ratios[name]:.3f}")
    assert len(ratios) == 11
    assert all(r <= 1.10 for r in ratios.values()), ratios


# C3 -----------------------------------------------------------------------
def _fixture_frames():
    """(array index, array bytes, itemsize, codec index, config, fixture frame) of the lz4 configs."""
    arrays = {}
    for arr, j, config, frame in fixture_cases("blosc"):
        if config["cname"] != "lz4":
            continue
        key = arr.tobytes(order="A")
        i = arrays.setdefault((key, arr.dtype.str), len(arrays))
        yield i, key, arr.dtype.itemsize, j, config, frame


def test_fixture_arrays_round_trip_and_headers():
    """Every fixture array under every lz4 config of the fixture set: the frame
    decodes (oracle walker, shared host walker), and bytes 0-11 (version,
    versionlz, flags, typesize, nbytes, blocksize) equal the fixture frame's
    exactly for the pairs of FIXTURE_HEADERS_AGREE below."""
    seen, agree, differ = set(), set(), set()
    for i, raw, itemsize, j, config, fixture in _fixture_frames():
        cfg = (config["clevel"], config["shuffle"], config["blocksize"])
        assert cfg in eg.LZ4_CONFIGS
        frame = eg.host_frame(raw, itemsize, *cfg)
        assert gen.oracle_decode(frame) == raw, (i, j)
        rc, _filtered, info = gen.host_decode(frame)
        assert rc == 0, (i, j, rc, info)
        assert int.from_bytes(frame[12:16], "little") == len(frame) <= len(raw) + 16
        (agree if frame[:12] == fixture[:12] else differ).add((i, cfg))
        seen.add((i, cfg))
    assert len({i for i, _c in seen}) == 13 and {c for _i, c in seen} == set(eg.LZ4_CONFIGS)
    # arrays 09-12 come from a recent c-blosc: all six configs agree
    for i in (9, 10, 11, 12):
        for cfg in eg.LZ4_CONFIGS:
            assert (i, cfg) in agree, (i, cfg)
    assert agree == FIXTURE_HEADERS_AGREE, (sorted(agree - FIXTURE_HEADERS_AGREE), sorted(FIXTURE_HEADERS_AGREE - agree))


# (array, (clevel, shuffle, blocksize)) whose bytes 0-11 equal the fixture
# frame's.  The others were written by older c-blosc versions and are not a
# target: arrays 00-08 under blocksize 0 carry the do-not-split bit where
# today's rule splits, and blocksize 128 / 256 / 255 where nbytes < 32 KiB
# gives one block today; array 03 (itemsize 1) carries that bit under
# blocksize 256 too.  Arrays 01 and 02 under (5, 1, 256) differ in the memcpyed
# bit only: c-blosc's match finder got those 256-byte blocks below nbytes + 16
# in total, this one does not and stores the frame.
FIXTURE_HEADERS_AGREE = {(i, cfg) for i in (9, 10, 11, 12) for cfg in eg.LZ4_CONFIGS} | \
    {(i, cfg) for i in (0, 4, 5, 6, 7, 8) for cfg in ((1, 0, 256), (5, 1, 256))} | \
    {(i, (1, 0, 256)) for i in (1, 2)}


@pytest.mark.parametrize("case", eg.shape_params(), ids=lambda c: c[0])
def test_frame_shapes(case):
    name, data, itemsize, shuffle, blocksize, clevel = case
    frame = eg.host_frame(data, itemsize, clevel, shuffle, blocksize)
    assert gen.oracle_decode(frame) == data
    rc, _filtered, info = gen.host_decode(frame)
    assert rc == 0, (rc, info)
    assert frame[0] == 2 and frame[1] == 1 and frame[2] >> 5 == 1 and frame[3] == itemsize
    assert int.from_bytes(frame[4:8], "little") == len(data)
    assert int.from_bytes(frame[12:16], "little") == len(frame) <= len(data) + 16
    memcpyed = bool(frame[2] & oblosc.BLOSC_MEMCPYED)
    assert memcpyed == (name in ("memcpyed-clevel0", "incompressible", "nbytes1"))
    if memcpyed:
        assert frame[16:] == data
    bs = int.from_bytes(frame[8:12], "little")
    if data:
        assert bool(frame[2] & oblosc.BLOSC_NOSPLIT) == (itemsize > 16 or bs // itemsize < 128)


def test_frame_parameters():
    p = blosc._frame_params
    assert eg.host_frame(b"", 1, 5, blosc.NOSHUFFLE) == gen.blosc_frame(b"") and len(gen.blosc_frame(b"")) == 16
    assert eg.host_frame(b"", 4, 5, blosc.SHUFFLE) == gen.blosc_frame(b"", 4, None, gen.SHUFFLE)
    assert p(1 << 20, 4, 5, blosc.SHUFFLE, 0)[:3] == (0x21, 512 * 1024, 4)  # numcodecs' defaults on a 1 MiB chunk
    assert p(8000, 8, 5, blosc.SHUFFLE, 0)[:3] == (0x21, 8000, 8)
    assert p(8000, 3, 5, blosc.SHUFFLE, 256)[1] == 255 and p(8000, 3, 5, blosc.SHUFFLE, 256)[0] & 0x10
    assert p(8000, 4, 5, blosc.SHUFFLE, 16)[1] == 128  # at least 128
    assert p(100, 4, 5, blosc.SHUFFLE, 256)[1] == 100  # at most nbytes
    assert p(3, 8, 5, blosc.SHUFFLE, 0)[1] == 3  # below typesize: not rounded to 0
    assert p(1 << 20, 4, 0, blosc.SHUFFLE, 0)[:2] == (0x21 | 0x02, 8192)  # clevel 0: memcpyed, 1/4 of 32 KiB
    assert [p(1 << 22, 1, c, 0, 0)[1] >> 10 for c in range(1, 10)] == [64, 64, 64, 128, 128, 256, 256, 256, 256]
    assert p(1 << 20, 17, 5, 0, 0)[0] & 0x10 and p(1 << 20, 17, 5, 0, 0)[1] == 131072 // 17 * 17
    assert p(1 << 20, 256, 5, blosc.SHUFFLE, 0)[2] == 1  # a typesize above 255 is written as 1


# C4 -----------------------------------------------------------------------
def test_blosclz4_class_surface():
    c = blosc.BloscLZ4()
    assert repr(c) == "BloscLZ4(cname='lz4', clevel=5, shuffle=SHUFFLE, blocksize=0)"
    assert c.get_config() == {"id": "blosc", "cname": "lz4", "clevel": 5, "shuffle": 1, "blocksize": 0}
    z = blosc.BloscLZ4(clevel=1, shuffle=blosc.BITSHUFFLE, blocksize=256)
    assert repr(z) == "BloscLZ4(cname='lz4', clevel=1, shuffle=BITSHUFFLE, blocksize=256)"
    cfg = z.get_config()
    assert cfg.pop("id") == "blosc"
    assert blosc.BloscLZ4.from_config(cfg) == z and z != c and c == blosc.BloscLZ4() and c == blosc.Blosc()
    assert issubclass(blosc.BloscLZ4, blosc.Blosc) and blosc.BloscLZ4.codec_id == "blosc"
    assert {"compress", "compress_many", "BloscLZ4"} <= set(blosc.__all__)
    with pytest.raises(ValueError, match="Cannot use typesize 0 less than 1"):
        blosc.BloscLZ4(typesize=0)
    with pytest.raises(NotImplementedError, match="not built"):
        blosc.Blosc().encode(np.zeros(16, "f4"))


def test_full_registration_is_on_request():
    before = dict(codec_registry)
    assert "blosc" not in before
    try:
        blosc.register()
        assert type(get_codec({"id": "blosc"})) is blosc.Blosc
        blosc.register(full=True)
        got = get_codec({"id": "blosc", "cname": "lz4", "clevel": 9, "shuffle": 2})
        assert type(got) is blosc.BloscLZ4 and got == blosc.BloscLZ4("lz4", 9, 2)
        assert set(codec_registry) == set(before) | {"blosc"}
    finally:
        codec_registry.pop("blosc", None)
    assert dict(codec_registry) == before


def test_compress_checks_need_no_device(monkeypatch):
    x = np.arange(100, dtype="f4")
    with pytest.raises(ValueError, match="^bad compressor or compressor not supported: 'lz5'"):
        blosc.compress(x, b"lz5", 5)
    for name in ("blosclz", "lz4hc", "snappy", "zlib", "zstd"):
        with pytest.raises(NotImplementedError, match=name):
            blosc.compress(x, name.encode(), 5)
        with pytest.raises(NotImplementedError, match=name):
            blosc.BloscLZ4(cname=name).encode(x)
    with pytest.raises(ValueError, match="^Cannot use typesize 0 less than 1.$"):
        blosc.compress(x, b"lz4", 5, typesize=0)
    with pytest.raises(ValueError, match="^invalid shuffle argument; expected -1, 0, 1 or 2, found 3$"):
        blosc.compress(x, b"lz4", 5, shuffle=3)
    assert blosc.BloscLZ4.max_buffer_size == 2**31 - 1
    monkeypatch.setattr(blosc.Blosc, "max_buffer_size", 1000)  # the limit itself would need 2 GiB
    with pytest.raises(ValueError, match="^Codec does not support buffers of > 1000 bytes$"):
        blosc.compress(np.zeros(1001, np.uint8), b"lz4", 5)
    monkeypatch.undo()
    # nothing to compress: the 16-byte frame, written without a device
    empty = blosc.compress(np.zeros(0, "f4"), b"lz4", 5)
    assert isinstance(empty, np.ndarray) and empty.tobytes() == gen.blosc_frame(b"", 4, None, gen.SHUFFLE)
    assert blosc.decompress(empty).tobytes() == b""
    assert blosc.compress_many([]) == []


def test_header_and_binding_name_the_encode_entry_points():
    names = set(_header_functions())
    assert {"mc_blosc_encode_workspace", "mc_blosc_encode_batch"} <= names
    assert names == set(_native.EXPORTED)
    assert _native.lib.mc_abi_version() == 2
    assert _native.lib.mc_blosc_encode_workspace(10, 1000) >= 1000 + 10 * 12
    assert blosc._ENC_RECORD.itemsize == 56


# C5 -----------------------------------------------------------------------
def test_sanitized_encode_run(tmp_path):
    """The ASan + UBSan build of the scalar encoder and the frame layout, as a
    process of its own (no LD_PRELOAD), over C1's streams and 200 seeded
    generated inputs of 0-20000 bytes: every output buffer has exactly `cap`
    bytes, every result is decoded back by the shared scalar decoder."""
    exe = os.path.join(eg.ENC_DIR, "lz4enc_hostcheck_main")
    assert os.path.exists(exe), "build with __graft_entry__.build() (make -C tests/native_lz4enc)"
    for k, (name, data) in enumerate(STREAMS):
        (tmp_path / f"{k:02d}-{name}.bin").write_bytes(data)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    run = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=600, env=env)
    assert run.returncode == 0, run.stdout + run.stderr
    assert f"inputs {len(STREAMS) + 200} files {len(STREAMS)} " in run.stdout and "failures 0" in run.stdout, run.stdout
