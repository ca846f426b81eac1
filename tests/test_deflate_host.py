"""zlib / gzip encode, CPU side: the scalar model of csrc/mc_deflate.h (compiled
for the host by tests/native_deflate) on the shared case list -- every frame
through the stdlib, through the project's scalar inflate model and through the
independent Python walker of tests/inflate_gen.py; sizes, bound and block types;
the parse's limits; the fixed bytes; the ``numcodecs_amd.deflate`` surface; the
checks that need no GPU; and the sanitized stand-alone run."""

import gzip as _gzip
import os
import struct
import subprocess
import zlib as _zlib

import numpy as np
import pytest

import numcodecs_amd
from numcodecs_amd import _deflate, _native, codec_registry, deflate, get_codec
from numcodecs_amd import gzip as ngzip
from numcodecs_amd import zlib as nzlib
from tests import deflate_gen as dg
from tests import inflate_gen as ig
from tests.test_boundary import _header_functions

CASES = dg.chunk_cases()


@pytest.fixture(scope="module")
def encoded():
    """{(name, container): (data, frame, segment records)} of the whole list, once."""
    out = {}
    for name, data in CASES:
        for container in ("zlib", "gzip"):
            frame, segs, need = dg.host_encode(data, container)
            assert frame is not None and need == len(frame), name
            out[name, container] = (data, frame, segs)
    return out


def _stdlib(container, frame):
    return _zlib.decompress(frame) if container == "zlib" else _gzip.decompress(frame)


# ---- decoders ---------------------------------------------------------------------
@pytest.mark.parametrize("container", ["zlib", "gzip"])
def test_every_frame_decodes(encoded, container):
    for name, data in CASES:
        _d, frame, _s = encoded[name, container]
        assert _stdlib(container, frame) == data, name
        rc, out, word, consumed = ig.host_decode(container, frame)
        assert rc == 0 and out == data and word == len(data) and consumed == len(frame), name


def test_the_walker_accepts_every_table(encoded):
    """Bit by bit, with none of the product's code; the gzip frame carries the same DEFLATE bytes."""
    types = set()
    for name, data in CASES:
        _d, frame, segs = encoded[name, "zlib"]
        out, census, end = ig.walk(frame, 2)
        assert out == data and end == len(frame) - 4, name
        assert census["max_len"] <= 258 and census["max_dist"] <= 32768 and census["max_code"] <= 15, name
        assert encoded[name, "gzip"][1][10:-8] == frame[2:-4], name
        types |= census["types"]
        # one block per compressed segment, two per full stored one, and a marker after each compressed non-final one
        want = sum((2 if s["bytes"] == dg.SEGMENT + 10 else 1) if s["type"] == dg.STORED else 1 for s in segs)
        want += sum(1 for s in segs[:-1] if s["type"] != dg.STORED)
        assert census["blocks"] == want, name
    assert types == {0, 1, 2}


# ---- sizes ------------------------------------------------------------------------
def test_sizes_bound_and_block_types(encoded):
    seen = {}
    for (name, container), (data, frame, segs) in encoded.items():
        head, trail = (2, 4) if container == "zlib" else (10, 8)
        assert len(frame) <= dg.host_bound(len(data), container) == _deflate.bound(len(data), dg.CONTAINERS[container])
        assert len(frame) == head + trail + int(segs["bytes"].sum()), name
        assert len(segs) == -(-len(data) // dg.SEGMENT)
        at = head
        for k, s in enumerate(segs):
            nk = min(dg.SEGMENT, len(data) - k * dg.SEGMENT)
            cost = [int(c) for c in s["cost"]]
            assert all(c % 8 == 0 for c in cost) and cost[0] == 8 * (nk + 5 * -(-nk // 65535)), name
            assert s["type"] == min(range(3), key=lambda t: (cost[t], t)), (name, k, cost)  # ties: stored, then fixed
            assert 8 * s["bytes"] == cost[s["type"]] and s["off"] == at, name
            at += int(s["bytes"])
            if container == "zlib":  # (the gzip frame carries the same blocks)
                seen.setdefault(name, []).append(int(s["type"]))
    assert seen["stored70000"] == [dg.STORED, dg.STORED]
    assert seen["low3"] == [dg.FIXED] and seen["low1"] == [dg.FIXED]
    assert seen["skewed70000"] == [dg.DYNAMIC, dg.DYNAMIC]
    assert seen["mix3"] == [dg.DYNAMIC, dg.STORED, dg.DYNAMIC]
    assert {t for ts in seen.values() for t in ts} == {dg.STORED, dg.FIXED, dg.DYNAMIC}


def test_a_short_slot_is_refused_and_untouched(encoded):
    for name in ("low13", "stored70000", "mix3"):
        data, frame, _s = encoded[name, "zlib"]
        got, _segs, need = dg.host_encode(data, "zlib", cap=len(frame) - 1)  # asserts that nothing was written
        assert got is None and need == len(frame), name
        assert dg.host_encode(data, "zlib", cap=len(frame))[0] == frame, name
    assert dg.host_encode(b"", "zlib")[0] is None  # the empty frame is the host's (below)


def test_compression_actually_happens(encoded):
    n = 1 << 20
    frame, segs, _need = dg.host_encode(bytes(n), "zlib")
    assert _zlib.decompress(frame) == bytes(n)
    print("zeros:", len(frame), "zlib level 1:", len(_zlib.compress(bytes(n), 1)))
    assert len(frame) < n // 100
    data, frame, _s = encoded["shuffled-floats", "zlib"]
    print("shuffled floats:", len(frame), "of", len(data), "zlib level 1:", len(_zlib.compress(data, 1)))
    assert len(frame) < len(data)


def test_level_0_is_stored(encoded):
    for name in ("low13", "low65537", "run70000"):
        data = dict(CASES)[name]
        frame, segs, _need = dg.host_encode(data, "gzip", level=0)
        assert (segs["type"] == dg.STORED).all() and len(frame) == dg.host_bound(len(data), "gzip"), name
        assert _gzip.decompress(frame) == data, name


# ---- the parse ----------------------------------------------------------------------
def test_pair_split_rule():
    lib = dg.hostlib()
    for L in list(range(4, 1600)) + [65535, 65536]:
        pieces = [lib.hd_deflate_piece(L, j) for j in range(lib.hd_deflate_npairs(L))]
        assert sum(pieces) == L and min(pieces) >= 3 and max(pieces) <= 258, L
        assert len(pieces) == -(-L // 258), L
    assert [lib.hd_deflate_piece(259, j) for j in range(2)] == [256, 3]
    assert [lib.hd_deflate_piece(518, j) for j in range(3)] == [258, 257, 3]
    for length in range(3, 259):
        s = lib.hd_deflate_len_sym(length)
        assert ig.LEN_BASE[s] <= length < ig.LEN_BASE[s] + (1 << ig.LEN_EXTRA[s]) and (s == 28) == (length == 258)
    for dist in list(range(1, 600)) + [4096, 4097, 24576, 24577, 32767, 32768]:
        s = lib.hd_deflate_dist_sym(dist)
        assert ig.DIST_BASE[s] <= dist < ig.DIST_BASE[s] + (1 << ig.DIST_EXTRA[s]), dist


def test_parse_limits():
    by = dict(CASES)
    for n in (258, 259, 260, 261, 516, 517):
        seqs, tail, hist = dg.host_parse(by["run%d" % n])
        assert seqs == [(1, n - 1, 1)] and tail == 0, n  # one literal, then the run at distance 1, to the last byte
        assert hist[7] == 1 and hist[256] == 1 and hist[288] == -(-(n - 1) // 258)
    seqs, tail, _h = dg.host_parse(by["run70000"][:65536])
    assert seqs == [(1, 65535, 1)] and tail == 0
    far = {p: max((d for _l, _m, d in dg.host_parse(by["period%d" % p])[0]), default=0) for p in (32767, 32768, 32769)}
    assert far[32767] == 32767 and far[32768] == 32768
    assert far[32769] < 32769  # the limit: that period is out of reach
    for name in ("low13", "low65536", "skewed70000", "seam-runs"):
        seg = by[name][:65536]
        seqs, tail, hist = dg.host_parse(seg)
        assert len(seqs) <= len(seg) // 4 and sum(l + m for l, m, _d in seqs) + tail == len(seg), name
        assert all(m >= 4 and 1 <= d <= 32768 for _l, m, d in seqs), name
        assert hist[:256].sum() == sum(l for l, _m, _d in seqs) + tail and hist[256] == 1, name
    seqs, tail, hist = dg.host_parse(b"abc")
    assert seqs == [] and tail == 3 and (hist == np.bincount([97, 98, 99, 256], minlength=320)).all()


def test_code_lengths():
    rng = np.random.default_rng(4)
    fib = [1, 1]
    while len(fib) < 30:
        fib.append(fib[-1] + fib[-2])
    sets = [(np.array(fib + [0] * 256), 15), (np.array(fib[:19]), 7), (np.zeros(30, int), 15), (np.ones(286, int), 15),
            (np.eye(1, 30, 5, dtype=int)[0] * 9, 15), (np.eye(1, 30, 0, dtype=int)[0], 15)]
    sets += [(rng.integers(0, 50, 286) * (rng.random(286) < 0.6), 15) for _ in range(20)]
    sets += [(rng.integers(0, 300, 19) * (rng.random(19) < 0.7), 7) for _ in range(20)]
    for freq, maxbits in sets:
        lens = dg.host_code_lengths(freq, maxbits)
        used = lens[lens > 0].astype(int)
        assert lens.max() <= maxbits and len(used) >= 2 and (lens[np.asarray(freq) > 0] > 0).all()
        assert (2.0 ** -used).sum() == 1.0  # exact: powers of two
        # forced codes go to the lowest unused symbols; a more frequent symbol never has the longer code
        if (np.asarray(freq) > 0).sum() < 2:
            assert set(np.flatnonzero(lens)) == set(np.flatnonzero(freq)) | set(
                np.flatnonzero(np.asarray(freq) == 0)[:2 - int((np.asarray(freq) > 0).sum())])
        order = np.lexsort((np.arange(len(freq)), freq))
        order = order[np.asarray(freq)[order] > 0]
        assert (np.diff(lens[order].astype(int)) <= 0).all()
    assert dg.host_code_lengths(fib + [0] * 256, 15).max() == 15 and dg.host_code_lengths(fib[:19], 7).max() == 7


# ---- fixed bytes ---------------------------------------------------------------------
def test_container_bytes(encoded):
    for name, data in CASES:
        z, gz = encoded[name, "zlib"][1], encoded[name, "gzip"][1]
        assert z[:2] == b"\x78\x01" and z[-4:] == struct.pack(">I", _zlib.adler32(data)), name
        assert gz[:10] == bytes([0x1F, 0x8B, 8, 0, 0, 0, 0, 0, 4, 255]), name
        assert gz[-8:] == struct.pack("<II", _zlib.crc32(data), len(data)), name


def test_empty_frame_and_levels():
    assert _deflate.empty_frame(_deflate.ZLIB) == bytes.fromhex("7801030000000001") == _zlib.compress(b"", 1)
    gz = _deflate.empty_frame(_deflate.GZIP)
    assert len(gz) == 20 == _deflate.bound(0, _deflate.GZIP) and _gzip.decompress(gz) == b""
    assert _deflate.bound(0, _deflate.ZLIB) == 8 == dg.host_bound(0, "zlib")
    for n in (1, 65535, 65536, 65537, (1 << 30) - 1):
        assert _deflate.bound(n, 0) == dg.host_bound(n, "zlib") and _deflate.bound(n, 1) == dg.host_bound(n, "gzip")
    for level in (-1, 0, 1, 5, 9):
        _zlib.compress(b"", level)
        assert _deflate.check_level(level) == (0 if level == 0 else 1)
    for level in (-2, 10, 100):
        with pytest.raises(_zlib.error, match="Bad compression level") as std:
            _zlib.compress(b"", level)
        for codec in (deflate.Zlib(level), deflate.GZip(level)):  # accepted by the constructor, refused at encode time
            with pytest.raises(_zlib.error) as got:
                codec.encode(b"abc")
            assert str(got.value) == str(std.value)


# ---- surface ----------------------------------------------------------------------------
def test_class_surface():
    assert set(deflate.__all__) == {"Zlib", "GZip", "compress", "compress_many", "register"}
    assert "deflate" in numcodecs_amd.__all__ and numcodecs_amd.deflate is deflate
    z, gz = deflate.Zlib(), deflate.GZip(level=4)
    assert issubclass(deflate.Zlib, nzlib.Zlib) and issubclass(deflate.GZip, ngzip.GZip)
    assert repr(z) == "Zlib(level=1)" and repr(gz) == "GZip(level=4)"
    assert z.get_config() == {"id": "zlib", "level": 1} and gz.get_config() == {"id": "gzip", "level": 4}
    assert deflate.Zlib.codec_id == "zlib" and deflate.GZip.codec_id == "gzip"
    assert deflate.Zlib.from_config({"level": 3}) == deflate.Zlib(3)
    assert deflate.Zlib.decode is nzlib.Zlib.decode and deflate.GZip.decode is ngzip.GZip.decode
    # the decode-only modules are as they were
    assert set(nzlib.__all__) == {"Zlib", "decompress", "decompress_many", "register"}
    assert set(ngzip.__all__) == {"GZip", "decompress", "decompress_many", "register"}
    with pytest.raises(NotImplementedError, match=r"numcodecs\.Zlib"):
        nzlib.Zlib().encode(b"abc")
    with pytest.raises(NotImplementedError, match=r"numcodecs\.GZip"):
        ngzip.GZip().encode(b"abc")


def test_registration_is_on_request():
    before = dict(codec_registry)
    assert "zlib" not in before and "gzip" not in before
    try:
        deflate.register()
        assert type(get_codec({"id": "zlib", "level": 4})) is deflate.Zlib
        assert type(get_codec({"id": "gzip", "level": 2})) is deflate.GZip
        assert set(codec_registry) == set(before) | {"zlib", "gzip"}
        nzlib.register()  # and the decode-only modules still register their own classes
        assert type(get_codec({"id": "zlib"})) is nzlib.Zlib
    finally:
        codec_registry.pop("zlib", None)
        codec_registry.pop("gzip", None)
    assert dict(codec_registry) == before


class _Sized:
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


def test_argument_checks_need_no_device(monkeypatch):
    assert deflate.compress_many([]) == []
    with pytest.raises(ValueError, match="^container must be 'zlib' or 'gzip'"):
        deflate.compress(b"abc", container="raw")
    with pytest.raises(ValueError, match="^outs must have one entry per buffer$"):
        deflate.compress_many([b"abc"], outs=[None, None])
    with pytest.raises(ValueError, match="^destination buffer too small; expected at least 14, got 13$"):
        deflate.compress_many([b"abc"], outs=[np.zeros(13, np.uint8)])
    with pytest.raises(_zlib.error, match="Bad compression level"):
        deflate.compress_many([b"abc"], level=10)
    # the empty buffer never reaches the device
    assert deflate.compress(b"").tobytes() == _zlib.compress(b"", 1)
    assert _gzip.decompress(deflate.compress(b"", container="gzip").tobytes()) == b""
    out = np.zeros(30, np.uint8)
    got = deflate.compress_many([b""], "gzip", outs=[out])[0]
    assert got.base is out and got.tobytes() == _deflate.empty_frame(_deflate.GZIP)
    monkeypatch.setattr(_deflate._frames, "flat_bytes", lambda buf, limit: buf)
    monkeypatch.setattr(_deflate, "is_device_tensor", lambda x: False)
    with pytest.raises(ValueError, match=r"2\*\*30 bytes and above are not supported on the GPU; got 1073741824$"):
        deflate.compress_many([_Sized(10), _Sized(1 << 30)])


def test_header_and_binding_name_the_entry_points():
    new = {"mc_deflate_encode_workspace", "mc_deflate_encode_batch"}
    names = set(_header_functions())
    assert new <= names and names == set(_native.EXPORTED)
    assert _native.lib.mc_abi_version() == 2
    assert _native.lib.mc_deflate_encode_workspace(3, 10, 5000) >= 5000 * 8 + 10 * (48 + 1280 + 352) + 3 * 4
    assert _native.lib.mc_deflate_encode_workspace(3, 10, 5000) < 5000 * 8 + 11 * 2048  # 2 bytes per input byte + per segment
    assert _deflate._RECORD.itemsize == 40 == dg.hostlib().hd_deflate_record_bytes()
    assert dg.SEG.itemsize == 48 == dg.hostlib().hd_deflate_seg_bytes()


# ---- the sanitized stand-alone run -------------------------------------------------
def test_sanitized_run():
    """The ASan + UBSan build of the scalar encoder, as a process of its own (no
    LD_PRELOAD): every generated case into a heap buffer of exactly the bound,
    nothing past the returned size touched, inflated back into exactly n bytes."""
    exe = os.path.join(dg.HOST_DIR, "deflate_hostcheck_main")
    assert os.path.exists(exe), "build with __graft_entry__.build() (make -C tests/native_deflate)"
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "failures 0" in run.stdout, run.stdout
