"""Blosc frames with zstd and zlib streams, CPU side: the host build of the
product's plan walker, stream rules and scalar decoders (tests/native_blosc_z)
against the reference's fixture frames and the committed case list
(tests/golden/blosc_z_cases.*), the ``formats`` / ``BloscFull`` surface, the
host model's ``cname='zstd'`` frames of the fixture arrays against three
decoders, and the sanitized stand-alone run of both directions."""

import os
import subprocess

import numpy as np
import pytest

from numcodecs_amd import _native, blosc, codec_registry, get_codec
from tests import blosc_gen as bgen
from tests import blosc_z_gen as gen

CASES = gen.load_cases()


# ---------------------------------------------------------------------------
# the host model
# ---------------------------------------------------------------------------
def test_host_model_decodes_the_fixture_frames():
    """codec.06 (zlib) and codec.07 (zstd): 26 frames, with the census the
    issue counted on the CPU."""
    compressed = {3: 0, 4: 0}
    memcpyed = streams = raw = 0
    for codec, fmt in ((6, gen.FMT_ZLIB), (7, gen.FMT_ZSTD)):
        for j, frame, want in gen.fixture_frames(codec):
            rc, filtered, info = gen.host_decode(frame)
            assert rc == 0, (codec, j, rc, info)
            assert bgen.unfilter(filtered, info["flags"], info["typesize"], info["blocksize"]) == want, (codec, j)
            assert info["format"] == fmt
            if frame[2] & 2:
                memcpyed += 1
                continue
            compressed[fmt] += 1
            streams += info["nstreams"]
            raw += info["raw_streams"]
            if fmt == gen.FMT_ZSTD:
                assert frame[2] & 0x10, "zstd frames carry the do-not-split bit"
    assert (compressed[3], compressed[4], memcpyed, streams, raw) == (12, 11, 3, 264, 2)


def test_recent_cblosc_header_bytes():
    for j, frame, _want in gen.fixture_frames(7)[9:13]:
        assert frame[:12] == bytes([2, 1, 0x91, 8]) + (8000).to_bytes(4, "little") * 2, j


def test_case_list_covers_the_issue():
    names = {c[0] for c in CASES}
    for fname in ("zlib", "zstd"):
        for tail in ("ts1", "ts3", "ts4", "ts8", "ts17", "short-last", "last-below-typesize", "raw-stream", "nbytes0",
                     "nbytes1", "incompressible"):
            assert f"{fname}-{tail}" in names
    assert {"zstd-block320k", "zstd-far-repeat192k", "zstd-stream65535", "zstd-stream65536", "zstd-stream65537",
            "zstd-rle-block", "zstd-raw-block", "zstd-checksum", "zstd-no-content-size", "zlib-split8",
            "zlib-stream96k", "zlib-stored-fixed-dynamic"} <= names
    assert {c[0] for c in gen.malformed_cases()} == {
        "zstd-bad-cut-short", "zstd-bad-magic", "zstd-bad-dictionary-id", "zstd-bad-content-size",
        "zstd-bad-fewer-bytes", "zstd-bad-more-bytes", "zstd-bad-checksum", "zstd-bad-second-frame",
        "zlib-bad-adler", "zlib-bad-truncated"}


@pytest.mark.parametrize("case", gen.valid_cases(), ids=lambda c: c[0])
def test_host_model_decodes_generated_frames(case):
    name, fname, frame, data, _code, _bad = case
    assert gen.host_array_bytes(frame) == data
    _rc, _f, info = gen.host_decode(frame)
    if name.endswith("incompressible"):
        assert info["raw_streams"] == info["nstreams"] > 0
    if name.endswith("-raw-stream"):
        assert info["raw_streams"] == 1
    if name == "zlib-split8":
        assert info["nstreams"] == 2 * 8 + 1
    if name == "zstd-block320k":
        assert info["nstreams"] == 1 and info["nbytes"] == 320 * 1024


@pytest.mark.parametrize("case", gen.malformed_cases(), ids=lambda c: c[0])
def test_host_model_refuses_malformed_frames_with_the_recorded_code(case):
    _name, _fname, frame, _data, code, bad = case
    rc, filtered, info = gen.host_decode(frame)
    assert (rc, info["bad_stream"]) == (code, bad) and filtered is None


def test_host_model_container_errors_are_shifted():
    """A violation of the container of a zstd / zlib frame is 64 + mc_lz4_error."""
    good = next(c[2] for c in CASES if c[0] == "zstd-short-last")
    cut = good[:-3]
    cut = cut[:12] + len(cut).to_bytes(4, "little") + cut[16:]
    rc, _f, info = gen.host_decode(cut)
    assert rc == gen.CONTAINER + 2 and info["bad_stream"] == info["nstreams"] - 1  # MC_LZ4_E_CBYTES
    lz4 = bgen.blosc_frame(bgen._payload(5000, 1), 4, 4096, bgen.SHUFFLE)
    cut = lz4[:-3]
    cut = cut[:12] + len(cut).to_bytes(4, "little") + cut[16:]
    assert gen.host_decode(cut)[0] == 2
    for fmt in (0, 2, 5):  # blosclz, snappy, an unknown one
        assert gen.host_decode(bytes([2, 1, (fmt << 5) | 1, 4]) + lz4[4:])[0] == gen.HCZ_UNSUPPORTED
    assert gen.host_decode(lz4)[0] == 0
    assert gen.hostlib().hcz_record_bytes() == blosc._FRAME_RECORD_Z.itemsize == 56


# ---------------------------------------------------------------------------
# the surface (no device needed: every check comes before a launch)
# ---------------------------------------------------------------------------
def test_defaults_still_refuse():
    zstd = next(c[2] for c in CASES if c[0] == "zstd-short-last")
    zlib_ = next(c[2] for c in CASES if c[0] == "zlib-short-last")
    for frame, name in ((zstd, "zstd"), (zlib_, "zlib")):
        with pytest.raises(NotImplementedError, match=name):
            blosc.decompress(frame)
        with pytest.raises(NotImplementedError, match=name):
            blosc.decompress_many([frame])
        with pytest.raises(NotImplementedError, match=name):
            blosc.Blosc().decode(frame)
        with pytest.raises(NotImplementedError, match=name):
            blosc.BloscLZ4().decode(frame)
    with pytest.raises(NotImplementedError, match="zstd"):
        blosc.decompress(zstd, formats=("lz4", "zlib"))
    with pytest.raises(NotImplementedError, match="zlib"):
        blosc.decompress(zlib_, formats=("zstd",))
    snappy = bytes([2, 1, (2 << 5) | 1, 4]) + zstd[4:]
    with pytest.raises(NotImplementedError, match="'snappy' .*only lz4 / lz4hc / zlib / zstd and memcpyed frames are\\)$"):
        blosc.BloscFull().decode(snappy)
    with pytest.raises(NotImplementedError, match="'zstd' .*only lz4 / lz4hc and memcpyed frames are\\)$"):
        blosc.decompress(zstd)  # the default's text, as before
    with pytest.raises(NotImplementedError, match="'zstd' .*only lz4 / lz4hc / zlib and memcpyed frames are; allow"):
        blosc.decompress(zstd, formats=("lz4", "zlib"))
    x = np.arange(100, dtype="f4")
    for name in ("blosclz", "lz4hc", "snappy", "zlib", "zstd"):  # the defaults: today's classes and texts
        text = f"^Blosc compression with '{name}' is not built in numcodecs_amd \\(only 'lz4' is\\)$"
        with pytest.raises(NotImplementedError, match=text):
            blosc.compress(x, name, 5)
        with pytest.raises(NotImplementedError, match=text):
            blosc.compress_many([x], name, 5)
        with pytest.raises(NotImplementedError, match=text):
            blosc.BloscLZ4(cname=name).encode(x)
    with pytest.raises(NotImplementedError, match="^Blosc compression is not built"):
        blosc.Blosc(cname="zstd").encode(x)
    for name in ("blosclz", "lz4hc", "snappy", "zlib"):  # with everything allowed: still not encoded
        with pytest.raises(NotImplementedError, match=f"'{name}' is not built .*only 'lz4' and 'zstd' are"):
            blosc.compress(x, name, 5, formats=blosc.ENCODE_FORMATS)
        with pytest.raises(NotImplementedError, match=name):
            blosc.BloscFull(cname=name).encode(x)
    with pytest.raises(NotImplementedError, match="'lz4' is not built .*only 'zstd' is"):
        blosc.compress(x, "lz4", 5, formats=("zstd",))
    # zstd is allowed: the argument checks behind the format's pass and fail as for lz4, before any launch
    with pytest.raises(ValueError, match="^Cannot use typesize 0 less than 1.$"):
        blosc.compress(x, "zstd", 5, typesize=0, formats=blosc.ENCODE_FORMATS)
    with pytest.raises(RuntimeError, match="^error during blosc compression: -10$"):
        blosc.compress(x, b"zstd", 10, formats=blosc.ENCODE_FORMATS)
    assert blosc.compress_many([], "zstd", 5, formats=blosc.ENCODE_FORMATS) == []


def test_formats_validation():
    assert blosc.DECODE_FORMATS == ("lz4", "zlib", "zstd")
    assert blosc.ENCODE_FORMATS == ("lz4", "zstd")
    frame = CASES[0][2]
    for bad in (("lz4", "snappy"), ("blosclz",), "lz4hc"):
        with pytest.raises(ValueError, match="bad Blosc format"):
            blosc.decompress(frame, formats=bad)
        with pytest.raises(ValueError, match="bad Blosc format"):
            blosc.decompress_many([], formats=bad)
        with pytest.raises(ValueError, match="bad Blosc format"):
            blosc.compress(b"abc", "lz4", 5, formats=bad)
        with pytest.raises(ValueError, match="bad Blosc format"):
            blosc.compress_many([], formats=bad)
    with pytest.raises(ValueError, match="bad Blosc format"):
        blosc.compress(b"abc", "lz4", 5, formats=("zlib",))  # decoded, not encoded
    with pytest.raises(TypeError):
        blosc.decompress(frame, None, blosc.DECODE_FORMATS)  # keyword-only
    # malformed headers are refused before the format is looked at, as by default
    with pytest.raises(RuntimeError, match="^error during blosc decompression: -1$"):
        blosc.decompress(frame[:12] + bytes(4) + frame[16:], formats=blosc.DECODE_FORMATS)
    empty = next(c[2] for c in CASES if c[0] == "zstd-nbytes0")
    assert blosc.decompress(empty, formats=blosc.DECODE_FORMATS).tobytes() == b""  # no launch


def test_bloscfull_config_and_registration():
    c = blosc.BloscFull(cname="zstd", clevel=3, shuffle=blosc.BITSHUFFLE, blocksize=4096)
    assert c.codec_id == "blosc" and issubclass(blosc.BloscFull, blosc.BloscLZ4)
    assert repr(c) == "BloscFull(cname='zstd', clevel=3, shuffle=BITSHUFFLE, blocksize=4096)"
    assert c.get_config() == blosc.BloscLZ4("zstd", 3, blosc.BITSHUFFLE, 4096).get_config()
    assert blosc.BloscFull.from_config({k: v for k, v in c.get_config().items() if k != "id"}) == c
    assert eval(repr(c), {"BloscFull": blosc.BloscFull, "BITSHUFFLE": blosc.BITSHUFFLE}) == c
    before = dict(codec_registry)
    assert "blosc" not in before  # nothing is registered on import
    try:
        blosc.register()
        assert type(get_codec({"id": "blosc"})) is blosc.Blosc
        blosc.register(full=True)
        assert type(get_codec({"id": "blosc"})) is blosc.BloscLZ4
        blosc.register(full=True, zstd=True)
        got = get_codec({"id": "blosc", "cname": "zstd", "clevel": 1, "shuffle": 1})
        assert type(got) is blosc.BloscFull and got == blosc.BloscFull("zstd", 1, 1)
        with pytest.raises(ValueError, match="full=True"):
            blosc.register(zstd=True)
        assert set(codec_registry) == set(before) | {"blosc"}
    finally:
        codec_registry.pop("blosc", None)
    assert dict(codec_registry) == before


def test_new_entry_points_are_bound():
    assert {"mc_blosc_decode_batch_z", "mc_blosc_decode_batch_z_workspace", "mc_blosc_encode_batch_z",
            "mc_blosc_encode_batch_z_workspace"} <= set(_native.EXPORTED)
    assert len(_native._SIGNATURES["mc_blosc_decode_batch_z"]) == 13
    assert len(_native._SIGNATURES["mc_blosc_encode_batch_z"]) == 11


# ---------------------------------------------------------------------------
# encode, cname='zstd': the host model (the bytes the kernels must give)
# ---------------------------------------------------------------------------
FIXTURE_CONFIGS = [dict(clevel=1, shuffle=gen.SHUFFLE, blocksize=0),  # codec.07's
                   dict(clevel=1, shuffle=gen.NOSHUFFLE, blocksize=0), dict(clevel=1, shuffle=gen.BITSHUFFLE, blocksize=0),
                   dict(clevel=1, shuffle=gen.SHUFFLE, blocksize=256), dict(clevel=1, shuffle=gen.SHUFFLE, blocksize=4096)]


def _fixture_arrays():
    return [np.load(os.path.join(gen.FIXTURE_BLOSC, "array.%02d.npy" % j), allow_pickle=False) for j in range(13)]


@pytest.fixture(scope="module")
def encoded_fixture_arrays():
    """[(array index, config, array bytes, host model's frame)]: made once."""
    out = []
    for j, arr in enumerate(_fixture_arrays()):
        raw = arr.tobytes(order="A")
        for config in FIXTURE_CONFIGS:
            out.append((j, config, raw, gen.host_encode(raw, arr.dtype.itemsize, **config)))
    assert len(out) == 65
    return out


def test_host_encoded_frames_decode_with_the_host_model(encoded_fixture_arrays):
    compressed = 0
    for j, config, raw, frame in encoded_fixture_arrays:
        assert frame[:2] == b"\x02\x01" and frame[2] >> 5 == gen.FMT_ZSTD and frame[2] & 0x10, (j, config)
        assert int.from_bytes(frame[12:16], "little") == len(frame) <= len(raw) + 16
        assert gen.host_array_bytes(frame) == raw, (j, config)
        compressed += not frame[2] & 2
    assert compressed >= 40  # most of the fixture's arrays compress: the decode is not of stored frames alone


def test_host_encoded_streams_decode_with_the_scalar_zstd_decoder(encoded_fixture_arrays):
    """Every stream on its own through tests/native_zstd's build of the scalar
    decoder (the `zstd` codec's model), the container walked here in Python."""
    from tests import zstd_gen as zg

    streams = 0
    for j, config, raw, frame in encoded_fixture_arrays:
        if frame[2] & 2:
            continue
        parts = []
        for stream, share in gen.streams_of(frame):
            if len(stream) == share:
                parts.append(stream)
                continue
            assert len(stream) < share
            rc, got = zg.host_decode(stream, share)[:2]
            assert rc == 0 and len(got) == share, (j, config, rc)
            parts.append(got)
            streams += 1
        flags, ts, bs = frame[2], frame[3], int.from_bytes(frame[8:12], "little")
        assert bgen.unfilter(b"".join(parts), flags, ts, bs) == raw, (j, config)
    assert streams >= 100


def test_host_encoded_streams_decode_with_libzstd(encoded_fixture_arrays):
    from tests import zstd_gen as zg

    lib = zg.load_lib()
    if lib is None:
        pytest.skip("libzstd.so.1 does not load here")
    for j, config, raw, frame in encoded_fixture_arrays:
        if frame[2] & 2:
            continue
        parts = []
        for stream, share in gen.streams_of(frame):
            got, err = (stream, None) if len(stream) == share else lib.decompress(stream, share)
            assert err is None and len(got) == share, (j, config, err)
            parts.append(got)
        flags, ts, bs = frame[2], frame[3], int.from_bytes(frame[8:12], "little")
        assert bgen.unfilter(b"".join(parts), flags, ts, bs) == raw, (j, config)


def test_host_encoded_header_equals_the_recent_cblosc_fixture(encoded_fixture_arrays):
    fixture = {j: frame for j, frame, _want in gen.fixture_frames(7)}
    seen = 0
    for j, config, _raw, frame in encoded_fixture_arrays:
        if j >= 9 and config == FIXTURE_CONFIGS[0]:
            assert frame[:12] == fixture[j][:12], j
            seen += 1
    assert seen == 4


@pytest.mark.parametrize("case", gen.encode_cases(), ids=lambda c: c[0])
def test_host_encode_cases_meet_their_condition(case):
    """The payloads of the GPU suite's encode list, with the host model alone:
    a case named compressible has no raw stream and is below half its input."""
    name, x, kw, compressible = case
    frame = gen.host_encode(x, x.dtype.itemsize, **kw)
    assert len(frame) <= x.nbytes + 16
    if x.nbytes:
        assert gen.host_array_bytes(frame) == x.tobytes()
    stored = bool(frame[2] & 2) or x.nbytes == 0
    streams = [] if stored else gen.streams_of(frame)
    raw = sum(len(s) == share for s, share in streams)
    if compressible:
        assert not stored and raw == 0 and 2 * len(frame) < x.nbytes
    if name == "raw-between":
        assert raw == 1 and len(streams) == 3 and len(streams[1][0]) == streams[1][1]
    if name in ("all-noise", "clevel0", "nbytes1"):
        assert frame[2] & 2 and len(frame) == x.nbytes + 16
    if name == "blocks3x65536+5":
        assert streams[0][1] == 3 * 65536 + 5


# ---------------------------------------------------------------------------
# sanitized stand-alone run
# ---------------------------------------------------------------------------
def test_sanitized_mutation_run(tmp_path):
    """The ASan + UBSan build of the host model, as a process of its own, over
    the 26 fixture frames, the committed cases (each with the bytes or the
    code it must give) and a few hundred mutations of each small one: it exits
    0 only if everything matched and every mutation was decoded within bounds
    or refused."""
    exe = os.path.join(gen.HOSTCHECK_DIR, "blosc_z_hostcheck_main")
    assert os.path.exists(exe), "build with __graft_entry__.build() (make -C tests/native_blosc_z)"
    for k, (name, _fname, frame, _data, code, _bad) in enumerate(CASES):
        path = tmp_path / f"{k:02d}-{name}.frame"
        path.write_bytes(frame)
        if code:
            (tmp_path / (path.name + ".code")).write_text(str(code))
        else:
            rc, filtered, _info = gen.host_decode(frame)
            assert rc == 0
            (tmp_path / (path.name + ".out")).write_bytes(filtered)
    fixtures = [os.path.join(gen.FIXTURE_BLOSC, "codec.%02d" % c) for c in (6, 7)]
    # bounds and undefined behaviour are the point; the leak checker needs ptrace rights some hosts withhold
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    run = subprocess.run([exe, *fixtures, str(tmp_path)], capture_output=True, text=True, timeout=600, env=env)
    assert run.returncode == 0, run.stdout + run.stderr
    nbad = len(gen.malformed_cases())
    assert "failures 0" in run.stdout, run.stdout
    assert "frames %d accepted %d refused %d " % (26 + len(CASES), 26 + len(CASES) - nbad, nbad) in run.stdout, run.stdout
