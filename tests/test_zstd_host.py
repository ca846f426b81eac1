"""zstd decode, CPU side: the census of the case list by the independent header
walker of tests/zstd_gen.py; the product's scalar model (csrc/mc_zstd.h,
compiled for the host by tests/native_zstd) against the recorded libzstd 1.4.8
results for every case, valid or invalid, and for every single-byte corruption
and truncation of two short frames; its count-only mode; the reference's
fixture frames; the same comparisons live where libzstd loads; the
``numcodecs_amd.zstd`` surface; the checks that need no GPU; and the sanitized
stand-alone run."""

import collections
import hashlib
import os
import subprocess

import numpy as np
import pytest

import numcodecs_amd
from numcodecs_amd import _native, _zstd, codec_registry, get_codec
from numcodecs_amd import zstd as nzstd
from tests import zstd_gen as g
from tests.test_boundary import _header_functions

VALID = g.valid_cases()
INVALID = g.invalid_cases()
LIB = g.load_lib()
needs_lib = pytest.mark.skipif(LIB is None, reason="libzstd.so.1 does not load here")
CODES = {n: getattr(g, n) for n in ("E_HEADER", "E_EMPTY", "E_DICT", "E_MEMBER", "E_CORRUPT", "E_SRCSIZE",
                                    "E_CAPACITY", "E_CHECK", "E_SIZE")}


def test_case_list_is_the_issues():
    """What the generated and hand-built frames are there for really is in
    them, by the header walker (frame, block, literals and sequences headers;
    no entropy decoding)."""
    census = {name: g.walk(frame) for name, frame, _s, _n in VALID}
    assert [n for n, *_ in VALID] == [s[0] for s in g.lib_specs()] + [h[0] for h in g.hand_cases()]
    for name, frame, _s, size in VALID:
        c = census[name]
        assert c["end"] == len(frame), name
        assert c["content"] in (None, size), name

    def blocks(name):
        return census[name]["blocks"]

    def types(name):
        return [b["type"] for b in blocks(name)]

    assert types("rle_blocks") == [2, 1, 1]
    assert types("raw_two_blocks") == [0, 0]
    # treeless literals in a frame of >= 10 blocks with a window of 2^19, with and without a declared size
    for name in ("sine_treeless", "sine_treeless_nosize"):
        assert census[name]["window"] == 1 << 19 and len(blocks(name)) >= 10, name
        assert sum(b["lit_type"] == 3 for b in blocks(name)) >= 2, name
    assert census["sine_treeless"]["content"] == 1200000 and census["sine_treeless_nosize"]["content"] is None
    assert census["sine_treeless"]["checksum"] == 1 and census["sine_treeless_nosize"]["window_descriptor"] is not None
    # Huffman literals and no sequences
    assert [(b["lit_type"], b["nseq"]) for b in blocks("sine_zero_sequences")] == [(2, 0)]
    # repeat mode beside the other three, and a frame longer than any LDS ring whose end copies its start
    modes = collections.Counter(m for b in blocks("repeat_mode") for m in b.get("modes", ()))
    assert modes[3] >= 50 and modes[2] >= 1 and modes[0] >= 1, modes
    assert census["repeat_far"]["content"] == (1 << 20) + 8192
    assert g.data_of("repeat_far")[:4096] == g.data_of("repeat_far")[-4096:]
    # a 3-byte sequence count
    big = [b for b in blocks("seq_count_3_bytes") if b.get("nseq_bytes") == 3]
    assert len(big) == 1 and big[0]["nseq"] >= 0x7F00
    assert len(blocks("blocks_293")) == 293 and census["blocks_293"]["window"] == 1024
    assert all(b["size"] <= 1024 + 3 for b in blocks("blocks_293"))
    b = blocks("one_stream_direct")[0]
    assert (b["lit_type"], b["streams"], b["weights"]) == (2, 1, "direct")
    every = [b for n in census for b in blocks(n) if b["type"] == 2]
    assert {b["lit_type"] for b in every} == {0, 1, 2, 3}
    assert {b["streams"] for b in every if b["lit_type"] >= 2} == {1, 4}
    assert {b.get("weights") for b in every if b["lit_type"] == 2} == {"fse", "direct"}
    assert {m for b in every for m in b.get("modes", ())} == {0, 1, 2, 3}
    assert {b["nseq_bytes"] for b in every} == {1, 2, 3}
    assert {census[n]["fcs_bytes"] for n in census} == {0, 1, 2, 4, 8}
    assert {census[n]["checksum"] for n in census} == {0, 1}
    params = {n: s[2] for n, s in zip([s[0] for s in g.lib_specs()], g.lib_specs())}
    assert min(p["level"] for p in params.values()) < 0 and max(p["level"] for p in params.values()) == 19
    assert tuple(size for name, _f, _s, size in VALID if name.startswith("len_")) == g.LENGTHS == (
        1, 63, 64, 65, 255, 256, 257, 65535, 65536, 65537, 131071, 131072, 131073)
    # by hand: RLE literals and raw literals in every size format with no sequences, an RLE block, a mantissa
    assert [(b["lit_type"], b["nseq"]) for b in blocks("hand_rle_literals")] == [(1, 0)]
    for sf in range(4):
        b = blocks("hand_raw_literals_sf%d" % sf)[0]
        assert (b["lit_type"], b["lit_sf"], b["nseq"]) == (0, sf, 0)
    assert types("hand_rle_block") == [1]
    assert census["hand_window_mantissa"]["window_descriptor"] & 7 and census["hand_window_mantissa"]["window"] == 2816
    assert blocks("hand_rle_mode_sequence")[0]["modes"] == (1, 1, 1)
    names = [n for n, _f, _m in INVALID]
    assert sum(n.startswith("cut_") for n in names) >= 8  # every structural boundary of a checksummed frame
    assert {"bad_magic", "reserved_bit", "block_type_3", "raw_block_over_128k", "rle_block_over_window",
            "dictionary_id", "content_size_0", "declared_larger", "declared_smaller", "flipped_checksum",
            "offset_beyond_output", "skippable_first", "two_frames", "junk_after"} <= set(names)


def test_data_formulas_are_pinned():
    for name, _frame, sha, size in VALID:
        data = g.data_of(name)
        assert len(data) == size and hashlib.sha256(data).hexdigest() == sha, name


def test_model_decodes_the_fixture_frames():
    fx = g.fixture_frames()
    assert len(fx) == 130
    for i, j, raw, frame in fx:
        assert g.host_count(frame) == (0, len(raw)), (i, j)
        rc, out, word = g.host_decode(frame)
        assert rc == 0 and out == raw and word == len(raw), (i, j)


def test_model_decodes_the_valid_cases():
    for name, frame, sha, size in VALID:
        assert g.host_count(frame) == (0, size), name  # the count-only mode: the same size
        rc, out, word = g.host_decode(frame)
        assert rc == 0 and len(out) == size == word and hashlib.sha256(out).hexdigest() == sha, name
        rc, out, _w = g.host_decode(frame, size - 1)  # one byte less: refused, nothing written behind it
        assert rc == g.E_CAPACITY, name


def _exception(code, word, declared):
    return _zstd._exception(code, word, 0, 10 if declared else None)


def test_model_rejects_the_invalid_cases_as_the_reference_does():
    for name, frame, meta in INVALID:
        declared = _zstd.declared_size(frame)  # the capacity the product gives the frame
        rc, out, word = g.host_decode(frame, 1 << 20 if declared is None else declared)
        assert rc == CODES[meta["expect"]], (name, rc)
        exc = _exception(rc, word, True)
        want = g.expected_exception(meta)
        if want is None:
            # the stated exceptions: the reference skips or concatenates (E_MEMBER); libzstd's one-shot call
            # does not look at Block_Maximum_Size, the RFC and the reference's streaming path do
            assert meta["expect"] in ("E_MEMBER", "E_CORRUPT") and meta["note"], name
            assert type(exc) is (NotImplementedError if rc == g.E_MEMBER else RuntimeError), name
            continue
        assert (type(exc), str(exc)) == want, (name, rc)


@pytest.mark.parametrize("kind", ["checksummed", "plain"])
def test_bounded_corruption_against_the_recorded_libzstd(kind):
    frame, name, verdicts = g.mutation_record(kind)
    assert len(frame) <= 700 and len(verdicts) == 3 * len(frame)
    cap = 4 * len(g.data_of(name)) + 1024
    accepted_more = []
    for (what, at, m), (rwhat, rat, ok, info) in zip(g.mutations(frame), verdicts):
        assert (what, at) == (rwhat, rat)
        rc, out, _w = g.host_decode(m, cap)
        if ok:  # what libzstd accepted the model accepts, with the same bytes
            assert rc == 0 and hashlib.sha256(out).hexdigest()[:16] + ":%d" % len(out) == info, (what, at, rc)
        elif rc == 0:
            accepted_more.append((what, at))
    # what libzstd refused the model refuses: no exception for the checksummed frame, and none needed for the
    # plain one (a mutation the model accepted against libzstd would have to be named here, with its rule)
    assert accepted_more == [], accepted_more


@needs_lib
def test_live_libzstd_agrees_with_the_record():
    for name, frame, sha, size in VALID:
        got, err = LIB.decompress(frame, size)
        assert err is None and hashlib.sha256(got).hexdigest() == sha, name
    for name, frame, meta in INVALID:
        v = LIB.verdict(frame, cap=1 << 20)
        assert v["stage"] == meta["verdict"]["stage"], name
    for i, j, raw, frame in g.fixture_frames():
        assert LIB.decompress(frame, len(raw)) == (raw, None), (i, j)


@needs_lib
@pytest.mark.parametrize("kind", ["checksummed", "plain"])
def test_bounded_corruption_against_live_libzstd(kind):
    frame, name, _v = g.mutation_record(kind)
    cap = 4 * len(g.data_of(name)) + 1024
    for what, at, m in g.mutations(frame):
        v = LIB.verdict(m, cap=cap)
        rc, out, _w = g.host_decode(m, cap)
        if v["stage"] in ("ok", "count"):
            assert rc == 0 and out == LIB.last, (what, at, rc)
        else:
            assert rc != 0, (what, at, v)


def test_header_edges():
    assert g.host_decode(b"", 10)[0] == g.E_HEADER
    assert g.host_decode(b"\x28\xb5\x2f", 10)[0] == g.E_HEADER
    # window: 2^31 is the largest; the exponent byte above it is refused
    data = b"x" * 10
    ok = g.frame_header(None, window=(21 << 3)) + g.block(0, data, True)
    assert g.host_decode(ok, 10)[:2] == (0, data)
    assert g.host_decode(g.frame_header(None, window=(22 << 3)) + g.block(0, data, True), 10)[0] == g.E_HEADER
    # the 2-byte Frame_Content_Size adds 256
    rc, hdr = g.host_open(g.frame_header(300) + g.block(0, b"y" * 300, True))
    assert rc == 0 and hdr[0] == 300 and hdr[4] == 300
    # XXH64 of the model against the plain one, across the 32-byte stripes and the tails
    for n in (0, 1, 3, 4, 7, 8, 31, 32, 33, 63, 64, 100, 1000):
        d = g.noise(n, 40 + n)
        assert g.hostlib().hz_xxh64(d, n) == g.xxh64(d), n


# ---- the surface, no GPU needed --------------------------------------------
def test_class_surface():
    z = nzstd.Zstd()
    assert repr(z) == "Zstd(level=0)" and repr(nzstd.Zstd(5, checksum=True)) == "Zstd(level=5)"
    assert z.get_config() == {"id": "zstd", "level": 0, "checksum": False}
    assert nzstd.Zstd(level=9, checksum=True).get_config() == {"id": "zstd", "level": 9, "checksum": True}
    assert nzstd.Zstd.from_config({"level": 3}) == nzstd.Zstd(3) != z
    assert nzstd.Zstd.codec_id == "zstd"
    assert (nzstd.Zstd.default_level(), nzstd.Zstd.min_level(), nzstd.Zstd.max_level()) == (3, -131072, 22)
    assert set(nzstd.__all__) == {"Zstd", "decompress", "decompress_many", "register"}
    assert "zstd" in numcodecs_amd.__all__ and numcodecs_amd.zstd is nzstd
    with pytest.raises(NotImplementedError, match=r"numcodecs\.Zstd"):
        z.encode(b"abc")


def test_registration_is_on_request():
    before = dict(codec_registry)
    assert "zstd" not in before
    try:
        nzstd.register()
        assert type(get_codec({"id": "zstd", "level": 4})) is nzstd.Zstd
        assert set(codec_registry) == set(before) | {"zstd"}
    finally:
        codec_registry.pop("zstd", None)
    assert dict(codec_registry) == before


class _Sized:
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


def test_argument_checks_need_no_device(monkeypatch):
    by = {n: f for n, f, _s, _z in VALID}
    frame = np.frombuffer(by["small_plain"], np.uint8)      # declares 1100 bytes
    nosize = np.frombuffer(by["small_nosize"], np.uint8)
    assert nzstd.decompress_many([]) == []
    with pytest.raises(ValueError, match="^outs must have one entry per frame$"):
        nzstd.decompress_many([frame], [None, None])
    with pytest.raises(ValueError, match="^sizes must have one entry per frame$"):
        nzstd.decompress_many([frame], sizes=[1, 2])
    with pytest.raises(ValueError, match="^sizes must not be negative$"):
        nzstd.decompress_many([frame], sizes=[-1])
    with pytest.raises(ValueError, match=r"2\*\*30 bytes and above are not supported on the GPU; got 1073741824$"):
        nzstd.decompress_many([nosize], sizes=[1 << 30])
    ro = np.zeros(1100, np.uint8)
    ro.flags.writeable = False
    with pytest.raises(ValueError, match="^destination buffer is read-only$"):
        nzstd.decompress(frame, ro)
    with pytest.raises(ValueError, match="^destination buffer too small; expected at least 1100, got 150$"):
        nzstd.decompress(frame, np.zeros(150, np.uint8))
    with pytest.raises(ValueError, match="^destination buffer too small; expected at least 200, got 150$"):
        nzstd.decompress_many([nosize], [np.zeros(150, np.uint8)], sizes=[200])
    assert _zstd.declared_size(by["small_plain"]) == 1100 and _zstd.declared_size(by["small_nosize"]) is None
    assert _zstd.declared_size(by["hand_fcs_8_bytes"]) == 300 and _zstd.declared_size(b"\x28\xb5") is None
    for name, f, _s, size in VALID:
        assert _zstd.declared_size(f[:18]) == g.walk(f)["content"], name
    monkeypatch.setattr(_zstd._frames, "flat_bytes", lambda buf, limit: buf)
    monkeypatch.setattr(_zstd, "is_device_tensor", lambda x: False)
    with pytest.raises(ValueError, match=r"2\*\*30 bytes and above are not supported on the GPU; got 1073741829$"):
        nzstd.decompress_many([_Sized(10), _Sized((1 << 30) + 5)])


def test_header_and_binding_name_the_entry_points():
    new = {"mc_zstd_workspace", "mc_zstd_size_batch", "mc_zstd_decode_batch"}
    names = set(_header_functions())
    assert new <= names and names == set(_native.EXPORTED)
    assert _native.lib.mc_abi_version() == 2
    assert _native.lib.mc_zstd_workspace(10) >= 10 * (48 + 131072)
    assert _zstd._RECORD.itemsize == 32 == g.hostlib().hz_record_bytes()
    assert g.hostlib().hz_tables_bytes() + 65536 <= 80 * 1024  # two workgroups share a CU's 160 KiB


def test_every_code_has_its_exception():
    with open(os.path.join(g.GOLDEN, "zstd_cases.json")) as fh:
        import json
        meta = json.load(fh)
    recorded = {c["verdict"]["error"] for c in meta["invalid"]} | \
        {e for m in meta["mutations"].values() for e in m["errors"]}
    for code in range(1, 11):
        exc = _exception(code, 0, True)
        assert isinstance(exc, (RuntimeError, NotImplementedError, ValueError)), code
    assert isinstance(_exception(g.E_CAPACITY, 0, False), ValueError)
    for code, text in _zstd._LIB_TEXT.items():  # every text is one libzstd gave the generator
        assert text in recorded and str(_exception(code, 0, True)) == "Zstd decompression error: " + text, code


# ---- the sanitized stand-alone run -----------------------------------------
def test_sanitized_run(tmp_path):
    """The ASan + UBSan build of the scalar model, as a process of its own (no
    LD_PRELOAD): every case and the 130 fixture frames from exactly sized heap
    copies into exactly sized destinations, then truncations and byte changes
    of them."""
    exe = os.path.join(g.HOST_DIR, "zstd_hostcheck_main")
    assert os.path.exists(exe), "build with __graft_entry__.build() (make -C tests/native_zstd)"
    n = refused = 0
    for k, (name, frame, _sha, _size) in enumerate(VALID):
        (tmp_path / f"v{k:03d}-{name}.zst").write_bytes(frame)
        (tmp_path / f"v{k:03d}-{name}.zst.out").write_bytes(g.data_of(name))
        n += 1
    for k, (name, frame, _meta) in enumerate(INVALID):
        (tmp_path / f"x{k:03d}-{name}.zst").write_bytes(frame)
        n += 1
        refused += 1
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    run = subprocess.run([exe, str(tmp_path), g.FIXTURE], capture_output=True, text=True, timeout=600, env=env)
    assert run.returncode == 0, run.stdout + run.stderr
    assert f"frames {n + 130} accepted {n - refused + 130} refused {refused} " in run.stdout, run.stdout
    assert "failures 0" in run.stdout, run.stdout
