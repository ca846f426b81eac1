"""zlib / gzip decode, CPU side: the census of the case list by the independent
Python walker of tests/inflate_gen.py; the product's scalar model
(csrc/mc_inflate.h, compiled for the host by tests/native_inflate) against the
stdlib for every case, valid or invalid; its count-only mode; the reference's
fixture frames; the ``numcodecs_amd.zlib`` / ``numcodecs_amd.gzip`` surface; the
checks that need no GPU; and the sanitized stand-alone run."""

import gzip as _gzip
import os
import subprocess
import zlib as _zlib

import numpy as np
import pytest

import numcodecs_amd
from numcodecs_amd import _inflate, _native, codec_registry, get_codec
from numcodecs_amd import gzip as ngzip
from numcodecs_amd import zlib as nzlib
from tests import inflate_gen as g
from tests.helpers import FIXTURE
from tests.test_boundary import _header_functions

VALID = g.valid_cases()
INVALID = g.invalid_cases()


def test_case_list_is_the_issues():
    """What the generated and hand-built streams are there for really is in
    them: counted by the walker, which also decodes every one of them."""
    census = {}
    for name, container, frame, data in VALID:
        if container != "zlib":
            continue
        out, c, end = g.walk(frame, 2)
        assert out == data and end == len(frame) - 4, name
        census[name] = c
        print(name, c)
    types = set().union(*(c["types"] for c in census.values()))
    assert types == {0, 1, 2}
    assert max(c["max_code"] for c in census.values()) == 15 == census["fibonacci"]["max_code"]
    assert census["fibonacci"]["blocks"] == 8
    assert max(c["max_dist"] for c in census.values()) == 32768 == census["far-32768"]["max_dist"]
    assert max(c["max_len"] for c in census.values()) == 258
    assert census["random-block-x3"]["max_dist"] == 32500 and census["random-block-x3"]["max_len"] == 258
    assert census["zeros100000"]["overlaps"] == 388 and census["zeros100000"]["max_dist"] == 1
    assert census["rle-runs"]["max_dist"] == 1 and census["rle-runs"]["max_len"] == 258
    assert census["repeat-crosses-hlit"]["crossing"] == 1
    assert census["stored70000"] ["types"] == {0} and census["stored70000"]["blocks"] == 2
    assert census["random70000"]["types"] == {0} and census["random70000"]["blocks"] == 5
    assert census["fixed5000"]["types"] == {1}
    assert census["full-flush"]["types"] == {0, 2}
    assert census["empty-stored-then-fixed"]["types"] == {0, 1}
    assert [len(d) for n, c, _f, d in VALID if n.startswith("smooth") and c == "zlib"] == \
        [0, 1, 63, 64, 65, 257, 258, 259, 32767, 32768, 32769]
    names = {n for n, _c, _f in INVALID}
    assert len(INVALID) == 13 * 2 + 4 + 7 and len(names) == 13 + 4 + 7
    # a gzip frame with every optional header field, and one with padding
    by = {n: f for n, c, f, _d in VALID if c == "gzip"}
    assert by["gzip-fname-fextra-fcomment"][3] == 4 | 8 | 16 and by["gzip-zero-padding"].endswith(bytes(7))


@pytest.mark.parametrize("container", ["zlib", "gzip"])
def test_model_agrees_with_the_stdlib_on_valid_cases(container):
    for name, c, frame, data in VALID:
        if c != container:
            continue
        assert g.stdlib_decode(c, frame) == ("ok", data), name
        rc, counted = g.host_count(c, frame)  # the count-only mode: the same size
        assert (rc, counted) == (0, len(data)), name
        rc, out, word, consumed = g.host_decode(c, frame)
        assert rc == 0 and out == data and word == len(data), name
        assert consumed == len(frame) - (7 if name == "gzip-zero-padding" else 0), name
        if data:  # one byte less: refused, nothing past the capacity written (host_decode checks the guard)
            assert g.host_decode(c, frame, len(data) - 1)[0] == _inflate.E_CAPACITY, name


def _expected_exception(container, code):
    """The exception class the product raises for a device code."""
    return type(_inflate._exception(g.CONTAINERS[container], code, 0, 0, None))


@pytest.mark.parametrize("container", ["zlib", "gzip"])
def test_model_agrees_with_the_stdlib_on_invalid_cases(container):
    for name, c, frame in INVALID:
        if c != container:
            continue
        rc, out, word, _consumed = g.host_decode(c, frame)
        std = g.stdlib_decode(c, frame)
        if name == "gzip-two-members":  # the one stated exception: the stdlib concatenates
            assert std[0] == "ok" and rc == _inflate.E_GZ_MEMBER and out == std[1][:3000]
            assert _expected_exception(c, rc) is NotImplementedError
            continue
        assert std[0] == "error" and rc != 0, name
        exc = _inflate._exception(g.CONTAINERS[c], rc, word, 0, None)
        assert type(exc) is std[1], (name, rc, std)
        if c == "zlib":
            assert str(exc) == std[2], (name, rc)
        assert g.host_count(c, frame)[1] == len(out), name  # counted and produced agree up to the fault


@pytest.mark.parametrize("container", ["zlib", "gzip"])
def test_model_agrees_with_the_stdlib_on_corrupted_frames(container):
    frame, data, muts = g.corruption_frames(container)
    assert g.host_decode(container, frame)[:2] == (0, data)
    rejected = 0
    for k, m in enumerate(muts):
        std = g.stdlib_decode(container, m)
        rc, out, word, _c = g.host_decode(container, m)
        assert (rc == 0) == (std[0] == "ok"), k
        if rc == 0:
            assert out == std[1], k
        else:
            rejected += 1
            exc = _inflate._exception(g.CONTAINERS[container], rc, word, 0, None)
            assert type(exc) is std[1], (k, rc, std)
            if container == "zlib":
                assert str(exc) == std[2], (k, rc)
    print(container, "rejected", rejected, "of", len(muts))


@pytest.mark.parametrize("container", ["zlib", "gzip"])
def test_fixture_frames_decode_through_the_host_model(container):
    fx = g.fixture_frames(container)
    assert len(fx) == 78
    for i, j, raw, frame in fx:
        assert g.stdlib_decode(container, frame) == ("ok", raw), (i, j)
        rc, out, _w, consumed = g.host_decode(container, frame)
        assert rc == 0 and out == raw and consumed == len(frame), (i, j)


def test_container_edges():
    assert g.host_decode("zlib", b"")[0] == _inflate.E_TRUNCATED and g.stdlib_decode("zlib", b"")[1] is _zlib.error
    assert g.host_decode("gzip", b"")[:2] == (0, b"") and g.stdlib_decode("gzip", b"") == ("ok", b"")
    assert g.host_decode("gzip", b"\x1f")[0] == _inflate.E_GZ_MAGIC and g.stdlib_decode("gzip", b"\x1f")[1] is _gzip.BadGzipFile
    assert g.host_decode("gzip", b"\x1f\x8b\x08")[0] == _inflate.E_TRUNCATED
    assert g.stdlib_decode("gzip", b"\x1f\x8b\x08")[1] is EOFError
    for cmf, code in ((0x77, _inflate.E_METHOD), (0x88, _inflate.E_WINDOW)):
        flg = 31 - (cmf << 8) % 31
        frame = bytes([cmf, flg]) + bytes(8)
        rc, _o, word, _c = g.host_decode("zlib", frame)
        std = g.stdlib_decode("zlib", frame)
        assert rc == code and str(_inflate._exception(0, rc, word, 0, None)) == std[2]
    # reserved gzip flag bits: GzipFile ignores them, and so do the rules here
    d = g.smooth(100)
    frame = g.gzip_wrap(g.raw_deflate(d), d, flags=0xE0)
    assert g.stdlib_decode("gzip", frame) == ("ok", d) and g.host_decode("gzip", frame)[:2] == (0, d)
    # FHCRC is skipped, not verified
    frame = g.gzip_wrap(g.raw_deflate(d), d, flags=2, extra=b"\x12\x34")
    assert g.stdlib_decode("gzip", frame) == ("ok", d) and g.host_decode("gzip", frame)[:2] == (0, d)
    # bytes after a zlib trailer are ignored
    frame = g.zlib_wrap(g.raw_deflate(d), d)
    assert g.stdlib_decode("zlib", frame + b"junk") == ("ok", d)
    rc, out, _w, consumed = g.host_decode("zlib", frame + b"junk")
    assert (rc, out, consumed) == (0, d, len(frame))


# ---- the surface, no GPU needed --------------------------------------------
def test_class_surface():
    z, gz = nzlib.Zlib(), ngzip.GZip()
    assert repr(z) == "Zlib(level=1)" and repr(gz) == "GZip(level=1)"
    assert z.get_config() == {"id": "zlib", "level": 1} and gz.get_config() == {"id": "gzip", "level": 1}
    assert nzlib.Zlib(level=9).get_config() == {"id": "zlib", "level": 9} and repr(ngzip.GZip(5)) == "GZip(level=5)"
    assert nzlib.Zlib.from_config({"level": 3}) == nzlib.Zlib(3) != z
    assert nzlib.Zlib.codec_id == "zlib" and ngzip.GZip.codec_id == "gzip"
    assert set(nzlib.__all__) == {"Zlib", "decompress", "decompress_many", "register"}
    assert set(ngzip.__all__) == {"GZip", "decompress", "decompress_many", "register"}
    assert {"zlib", "gzip"} <= set(numcodecs_amd.__all__)
    assert numcodecs_amd.zlib is nzlib and numcodecs_amd.gzip is ngzip
    assert nzlib._zlib is _zlib and ngzip._gzip is _gzip  # the stdlib modules, not these
    with pytest.raises(NotImplementedError, match=r"numcodecs\.Zlib"):
        z.encode(b"abc")
    with pytest.raises(NotImplementedError, match=r"numcodecs\.GZip"):
        gz.encode(b"abc")


def test_registration_is_on_request():
    before = dict(codec_registry)
    assert "zlib" not in before and "gzip" not in before
    try:
        nzlib.register()
        ngzip.register()
        assert type(get_codec({"id": "zlib", "level": 4})) is nzlib.Zlib
        assert get_codec({"id": "gzip", "level": 2}) == ngzip.GZip(2)
        assert set(codec_registry) == set(before) | {"zlib", "gzip"}
    finally:
        codec_registry.pop("zlib", None)
        codec_registry.pop("gzip", None)
    assert dict(codec_registry) == before
    assert numcodecs_amd.register_with_numcodecs.__doc__  # unchanged: neither codec is in its list


class _Sized:
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


def test_argument_checks_need_no_device(monkeypatch):
    frame = np.frombuffer(g.zlib_wrap(g.raw_deflate(b"abc" * 50), b"abc" * 50), np.uint8)
    for mod in (nzlib, ngzip):
        assert mod.decompress_many([]) == []
        with pytest.raises(ValueError, match="^outs must have one entry per frame$"):
            mod.decompress_many([frame], [None, None])
        with pytest.raises(ValueError, match="^sizes must have one entry per frame$"):
            mod.decompress_many([frame], sizes=[1, 2])
        with pytest.raises(ValueError, match="^sizes must not be negative$"):
            mod.decompress_many([frame], sizes=[-1])
        with pytest.raises(ValueError, match=r"2\*\*30 bytes and above are not supported on the GPU; got 1073741824$"):
            mod.decompress_many([frame], sizes=[1 << 30])
        ro = np.zeros(150, np.uint8)
        ro.flags.writeable = False
        with pytest.raises(ValueError, match="^destination buffer is read-only$"):
            mod.decompress(frame, ro)
        with pytest.raises(ValueError, match="^destination buffer too small; expected at least 200, got 150$"):
            mod.decompress_many([frame], [np.zeros(150, np.uint8)], sizes=[200])
    with pytest.raises(ValueError, match="^container must be"):
        _inflate.decompress_many([frame], 2)
    # a frame of 2**30 bytes (no such buffer is made: the flattening step only reports the length)
    monkeypatch.setattr(_inflate._frames, "flat_bytes", lambda buf, limit: buf)
    monkeypatch.setattr(_inflate, "is_device_tensor", lambda x: False)
    with pytest.raises(ValueError, match=r"2\*\*30 bytes and above are not supported on the GPU; got 1073741829$"):
        nzlib.decompress_many([_Sized(10), _Sized((1 << 30) + 5)])


def test_header_and_binding_name_the_entry_points():
    new = {"mc_inflate_workspace", "mc_inflate_size_batch", "mc_inflate_decode_batch"}
    names = set(_header_functions())
    assert new <= names and names == set(_native.EXPORTED)
    assert _native.lib.mc_abi_version() == 2
    assert _native.lib.mc_inflate_workspace(10) >= 10 * (32 + 4)
    assert _inflate._RECORD.itemsize == 32 == g.hostlib().hi_inflate_record_bytes()
    assert g.hostlib().hi_inflate_tables_bytes() + 32768 <= 40 * 1024  # four workgroups share a CU's 160 KiB


def test_every_code_has_its_exception():
    for code in range(1, 26):
        for container in (0, 1):
            exc = _inflate._exception(container, code, 0, 0, 10)
            assert isinstance(exc, (_zlib.error, _gzip.BadGzipFile, EOFError, NotImplementedError, ValueError)), code
    for code, text in _inflate._ZLIB_TEXT.items():
        assert str(_inflate._exception(0, code, 0, 0, None)) == "Error -3 while decompressing data: " + text


# ---- the sanitized stand-alone run -----------------------------------------
def test_sanitized_run(tmp_path):
    """The ASan + UBSan build of the scalar model, as a process of its own (no
    LD_PRELOAD): every case and the 156 fixture frames from exactly sized heap
    copies into exactly sized destinations, then truncations and byte changes
    of them."""
    exe = os.path.join(g.HOST_DIR, "inflate_hostcheck_main")
    assert os.path.exists(exe), "build with __graft_entry__.build() (make -C tests/native_inflate)"
    n = refused = 0
    for k, (name, c, frame, data) in enumerate(VALID):
        (tmp_path / f"v{k:03d}-{name}.{c}").write_bytes(frame)
        (tmp_path / f"v{k:03d}-{name}.{c}.out").write_bytes(data)
        n += 1
    for k, (name, c, frame) in enumerate(INVALID):
        if name == "gzip-two-members":  # refused here, accepted by the stdlib: in the tests above
            continue
        (tmp_path / f"x{k:03d}-{name}.{c}").write_bytes(frame)
        n += 1
        refused += 1
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    run = subprocess.run([exe, str(tmp_path), os.path.join(FIXTURE, "zlib"), os.path.join(FIXTURE, "gzip")],
                         capture_output=True, text=True, timeout=600, env=env)
    assert run.returncode == 0, run.stdout + run.stderr
    assert f"frames {n + 156} accepted {n - refused + 156} refused {refused} " in run.stdout, run.stdout
    assert "failures 0" in run.stdout, run.stdout
