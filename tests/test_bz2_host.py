"""bz2 decode, CPU side: the census of the case list by the independent Python
walker of tests/bz2_gen.py; the product's scalar model (csrc/mc_bz2.h, compiled
for the host by tests/native_bz2) against the stdlib for every case, valid or
invalid; its count-only mode; the reference's fixture frames; the
``numcodecs_amd.bz2`` surface; the checks that need no GPU; and the sanitized
stand-alone run."""

import bz2 as _bz2
import os
import subprocess

import numpy as np
import pytest

import numcodecs_amd
from numcodecs_amd import _bz2 as impl
from numcodecs_amd import _native, codec_registry, get_codec
from numcodecs_amd import bz2 as nbz2
from tests import bz2_gen as g
from tests import bz2_write as bw
from tests.helpers import FIXTURE, check_config
from tests.test_boundary import _header_functions

VALID = g.valid_cases()
INVALID = g.invalid_cases()


def test_case_list_is_the_issues():
    """What the generated and hand-built streams are there for really is in
    them: counted by the walker, which also decodes every one of them."""
    census = {}
    for name, frame, data in VALID:
        out, c = g.walk(frame)
        assert out == data, name
        assert c["end"] == len(frame) - {"trailing-xyz": 3, "trailing-zeros": 7, "trailing-BZh0": 7}.get(name, 0), name
        census[name] = c
    blocks = {n: c["blocks"] for n, c in census.items()}
    assert blocks["empty"] == [] and len(VALID[0][2]) == 0
    assert [blocks[n][0]["nblock"] for n in ("one-byte", "plain-63", "plain-64", "plain-65", "plain-255")] == [1, 63, 64, 65, 255]
    assert blocks["one-value"][0]["counts"] == {46} and blocks["all-256"][0]["nblock"] == 256
    for r, counts in ((3, set()), (4, {0}), (5, {1}), (255, {251}), (256, {251}), (259, {251, 0}), (260, {251, 1})):
        for place in ("straddle", "end"):
            assert blocks[f"run-{r}-{place}"][0]["counts"] == counts, (r, place)
        if r >= 4:
            assert blocks[f"run-{r}-straddle"][0]["straddles"]
        if r in (4, 5, 255, 259, 260):
            assert blocks[f"run-{r}-end"][0]["count_ends_block"]
    assert blocks["run-5-straddle"][0]["count_is_byte"]  # a count byte equal to the run's byte
    assert blocks["zeros100000"][0]["counts"] == {251, 36} and blocks["zeros100000"][0]["nblock"] == 1965
    assert [blocks[f"tables-{k}"][0]["tables"] for k in (2, 3, 4, 5, 6)] == [2, 3, 4, 5, 6]
    assert [len(blocks[f"random-{n}"]) for n in (99980, 99981, 99982)] in ([1, 1, 2], [1, 2, 2])
    three = blocks["random-250000-l1"]
    assert len(three) == 3 and any(b["start_bit"] % 8 for b in three[1:]) and len(VALID[[v[0] for v in VALID].index("random-250000-l1")][1]) > 250000
    nine = blocks["random-250000-l9"]
    assert len(nine) == 1 and nine[0]["nblock"] >= 250000 and census["random-250000-l9"]["level"] == 9
    assert blocks["writer-len20"][0]["max_code"] == 20
    assert blocks["writer-orig0"][0]["orig"] == 0
    last = blocks["writer-orig-last"][0]
    assert last["orig"] == last["nblock"] - 1
    assert blocks["writer-small"][0]["nblock"] < 64
    assert blocks["writer-surplus-selectors"][0]["nsel"] == 18010 > 18002
    assert blocks["writer-six-tables"][0]["tables_used"] == {0, 1, 2, 3, 4, 5}
    assert len(blocks["writer-two-blocks"]) == 2 and blocks["writer-two-blocks"][1]["start_bit"] % 8
    for name, lo in (("writer-two-cycles-small", 300), ("writer-two-cycles", 5000)):
        b = blocks[name][0]
        assert b["nblock"] == lo and 2 <= b["cycle"] <= lo // 2, name
    assert all(b["cycle"] == b["nblock"] for n, bl in blocks.items() if not n.startswith("writer-two-cycles") for b in bl)
    names = [n for n, _f in INVALID]
    assert len(set(names)) == len(names) and len([n for n in names if n.startswith("cut-")]) >= 60
    assert set(g.DEPARTURES) <= set(names)


def test_model_agrees_with_the_stdlib_on_valid_cases():
    for name, frame, data in VALID:
        assert g.stdlib_decode(frame) == ("ok", data), name
        rc, counted, _w = g.host_count(frame)  # the count-only mode: the same size
        assert (rc, counted) == (0, len(data)), name
        rc, out, word = g.host_decode(frame)
        assert rc == 0 and out == data, name
        if data:  # one byte less: refused, nothing past the capacity written (host_decode checks the guard)
            assert g.host_decode(frame, len(data) - 1)[0] == impl.E_CAPACITY, name


def test_model_agrees_with_the_stdlib_on_invalid_cases():
    classes = set()
    for name, frame in INVALID:
        rc, _out, word = g.host_decode(frame)
        assert g.host_count(frame)[0] == rc, name  # the count-only mode gives the same verdict
        if name in g.DEPARTURES:
            assert rc == g.DEPARTURES[name] and type(impl._exception(rc, word, 0, None)) is NotImplementedError, name
            continue
        std = g.stdlib_decode(frame)
        assert std[0] == "error" and rc != 0, (name, rc, std)
        exc = impl._exception(rc, word, 0, None)
        assert type(exc) is std[1] and str(exc) == std[2], (name, rc, std)
        classes.add(std[1])
    assert classes == {OSError, ValueError}
    # the stdlib decodes what the departures refuse, or judges it otherwise
    assert g.stdlib_decode(dict(INVALID)["second-stream"]) == ("ok", g.plain(100) * 2)
    assert g.stdlib_decode(dict(INVALID)["second-stream-prefix"])[1] is ValueError


def test_model_agrees_with_the_stdlib_on_corrupted_frames():
    """Single-byte changes all over a two-table and a six-table stream."""
    rejected = total = 0
    for base in ("tables-2", "tables-6", "run-259-straddle"):
        frame = dict((n, f) for n, f, _d in VALID)[base]
        for at in range(0, len(frame), max(1, len(frame) // 150)):
            for flip in (0x01, 0x10, 0x80):
                m = bytearray(frame)
                m[at] ^= flip
                std = g.stdlib_decode(m)
                rc, out, word = g.host_decode(bytes(m))
                total += 1
                if rc in (impl.E_RANDOMISED, impl.E_FURTHER):
                    continue
                assert (rc == 0) == (std[0] == "ok"), (base, at, flip, rc, std[:2])
                if rc == 0:
                    assert out == std[1], (base, at, flip)
                else:
                    rejected += 1
                    exc = impl._exception(rc, word, 0, None)
                    assert type(exc) is std[1] and str(exc) == std[2], (base, at, flip, rc, std)
    assert rejected > total // 2


def test_fixture_frames_decode_through_the_host_model():
    fx = g.fixture_frames()
    assert len(fx) == 52
    for i, j, raw, frame in fx:
        assert g.stdlib_decode(frame) == ("ok", raw), (i, j)
        rc, out, _w = g.host_decode(frame)
        assert rc == 0 and out == raw, (i, j)


def test_edges():
    assert g.host_decode(b"")[:2] == (0, b"") and g.stdlib_decode(b"") == ("ok", b"")
    for frame in (b"B", b"BZ", b"BZh", b"BZh9"):  # shorter than the header, or nothing behind it: truncated
        assert g.host_decode(frame)[0] == impl.E_TRUNCATED and g.stdlib_decode(frame)[1] is ValueError, frame
    assert g.host_decode(b"X")[0] == 1 and g.stdlib_decode(b"X")[1] is OSError
    assert g.host_decode(b"BZh0")[0] == 2 and g.stdlib_decode(b"BZh0")[1] is OSError
    # the CRC pieces the wave's fold is made of
    lib = g.hostlib()
    data = g.noise(1000, 9)
    assert lib.hb_bz2_crc(data, len(data)) == bw.crc32_bz(data)
    a, b = data[:611], data[611:]
    # crc register of a || b = register(a) * x^(8 |b|) + raw(b): what a step of 64 bytes does with 64 lanes
    reg = lib.hb_bz2_crc(a, len(a)) ^ 0xFFFFFFFF
    raw = 0
    for k, byte in enumerate(b):
        raw ^= lib.hb_bz2_gfmul(lib.hb_bz2_mulx(byte << 24, 8), lib.hb_bz2_mulx(1, 8 * (len(b) - 1 - k)))
    assert (lib.hb_bz2_gfmul(reg, lib.hb_bz2_mulx(1, 8 * len(b))) ^ raw) ^ 0xFFFFFFFF == bw.crc32_bz(data)


# ---- the surface, no GPU needed --------------------------------------------
def test_class_surface():
    z = nbz2.BZ2()
    assert repr(z) == "BZ2(level=1)" and z.get_config() == {"id": "bz2", "level": 1}
    assert nbz2.BZ2(level=9).get_config() == {"id": "bz2", "level": 9} and repr(nbz2.BZ2(5)) == "BZ2(level=5)"
    assert nbz2.BZ2.from_config({"level": 3}) == nbz2.BZ2(3) != z
    assert nbz2.BZ2.codec_id == "bz2"
    assert nbz2.__all__ == ["BZ2", "decompress", "decompress_many", "register"]
    assert "bz2" in numcodecs_amd.__all__ and numcodecs_amd.bz2 is nbz2
    assert nbz2._bz2 is _bz2  # the stdlib module, not this one
    with pytest.raises(NotImplementedError, match=r"numcodecs\.BZ2"):
        z.encode(b"abc")


def test_registration_is_on_request():
    before = dict(codec_registry)
    assert "bz2" not in before
    try:
        nbz2.register()
        assert type(get_codec({"id": "bz2", "level": 4})) is nbz2.BZ2
        assert get_codec({"id": "bz2", "level": 2}) == nbz2.BZ2(2)
        assert set(codec_registry) == set(before) | {"bz2"}
        check_config(nbz2.BZ2(7))
    finally:
        codec_registry.pop("bz2", None)
    assert dict(codec_registry) == before


class _Sized:
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


def test_argument_checks_need_no_device(monkeypatch):
    frame = np.frombuffer(_bz2.compress(b"abc" * 50), np.uint8)
    assert nbz2.decompress_many([]) == []
    with pytest.raises(ValueError, match="^outs must have one entry per frame$"):
        nbz2.decompress_many([frame], [None, None])
    with pytest.raises(ValueError, match="^sizes must have one entry per frame$"):
        nbz2.decompress_many([frame], sizes=[1, 2])
    with pytest.raises(ValueError, match="^sizes must not be negative$"):
        nbz2.decompress_many([frame], sizes=[-1])
    with pytest.raises(ValueError, match=r"2\*\*30 bytes and above are not supported on the GPU; got 1073741824$"):
        nbz2.decompress_many([frame], sizes=[1 << 30])
    ro = np.zeros(150, np.uint8)
    ro.flags.writeable = False
    with pytest.raises(ValueError, match="^destination buffer is read-only$"):
        nbz2.decompress(frame, ro)
    with pytest.raises(ValueError, match="^destination buffer too small; expected at least 200, got 150$"):
        nbz2.decompress_many([frame], [np.zeros(150, np.uint8)], sizes=[200])
    # a frame of 2**30 bytes (no such buffer is made: the flattening step only reports the length)
    monkeypatch.setattr(impl._frames, "flat_bytes", lambda buf, limit: buf)
    monkeypatch.setattr(impl, "is_device_tensor", lambda x: False)
    with pytest.raises(ValueError, match=r"2\*\*30 bytes and above are not supported on the GPU; got 1073741829$"):
        nbz2.decompress_many([_Sized(10), _Sized((1 << 30) + 5)])


def test_header_and_binding_name_the_entry_points():
    new = {"mc_bz2_workspace", "mc_bz2_size_batch", "mc_bz2_decode_batch"}
    names = set(_header_functions())
    assert new <= names and names == set(_native.EXPORTED)
    assert _native.lib.mc_abi_version() == 2
    unit = 5 * 100000
    # per resident wave, not per frame: 8192 level-9 frames ask for no more than 768 waves' worth
    assert _native.lib.mc_bz2_workspace(8192, 9) <= 768 * 9 * unit + 8192 * 32 + 4096
    assert _native.lib.mc_bz2_workspace(10, 1) >= 10 * (unit + 32)
    assert _native.lib.mc_bz2_workspace(10, 3) - _native.lib.mc_bz2_workspace(10, 1) == 10 * 2 * unit
    assert impl._RECORD.itemsize == 32 == g.hostlib().hb_bz2_record_bytes()
    assert 3 * (g.hostlib().hb_bz2_tables_bytes() + 2 * 4 * 2049 + 64) <= 160 * 1024  # three workgroups share a CU's LDS


def test_every_code_has_its_exception():
    for code in range(1, 22):
        exc = impl._exception(code, 0, 0, 10)
        assert isinstance(exc, (OSError, ValueError, NotImplementedError)), code
    assert str(impl._exception(4, 0, 0, None)) == "Invalid data stream"
    assert str(impl._exception(impl.E_TRUNCATED, 0, 0, None)) == "Compressed data ended before the end-of-stream marker was reached"
    assert str(impl._exception(impl.E_CAPACITY, 0, 3, 10)) == "frame 3 decodes to more than the 10 bytes given for it"


# ---- the sanitized stand-alone run -----------------------------------------
def test_sanitized_run(tmp_path):
    """The ASan + UBSan build of the scalar model, as a process of its own (no
    LD_PRELOAD): every case and the 52 fixture frames from exactly sized heap
    copies into exactly sized destinations, then truncations and byte changes
    of them."""
    exe = os.path.join(g.HOST_DIR, "bz2_hostcheck_main")
    assert os.path.exists(exe), "build with __graft_entry__.build() (make -C tests/native_bz2)"
    n = refused = 0
    for k, (name, frame, data) in enumerate(VALID):
        (tmp_path / f"v{k:03d}-{name}.bz2").write_bytes(frame)
        (tmp_path / f"v{k:03d}-{name}.bz2.out").write_bytes(data)
        n += 1
    for k, (name, frame) in enumerate(INVALID):
        (tmp_path / f"x{k:03d}-{name}.bz2").write_bytes(frame)
        n += 1
        refused += 1
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    run = subprocess.run([exe, str(tmp_path), os.path.join(FIXTURE, "bz2")], capture_output=True, text=True,
                         timeout=600, env=env)
    assert run.returncode == 0, run.stdout + run.stderr
    assert f"frames {n + 52} accepted {n - refused + 52} refused {refused} " in run.stdout, run.stdout
    assert "failures 0" in run.stdout, run.stdout
