"""Zstd encode, CPU side: the scalar model of csrc/mc_zstd_enc.h (compiled for
the host by tests/native_zstd_enc) on the shared case list -- every frame
through the project's scalar decoder, through libzstd where it loads and
through the independent header walker of tests/zstd_gen.py; the census of the
forms the rules can write; exact sizes and the bound; the normalisation and the
count writer against the decoder's reader; the ``numcodecs_amd.zstd_enc``
surface; the checks that need no GPU; and the sanitized stand-alone run."""

import os
import subprocess

import numpy as np
import pytest

import numcodecs_amd
from numcodecs_amd import _native, _zstd_enc, codec_registry, get_codec, zstd_enc
from numcodecs_amd import zstd as nzstd
from tests import zstd_enc_gen as eg
from tests import zstd_gen as zg
from tests.test_boundary import _header_functions

CASES = eg.chunk_cases()
LIB = zg.load_lib()


@pytest.fixture(scope="module")
def encoded():
    """{(name, checksum): (data, frame, segment records)} of the whole list, once."""
    out = {}
    for name, data in CASES:
        for checksum in (False, True):
            frame, segs, need = eg.host_encode(data, checksum)
            assert frame is not None and need == len(frame), name
            out[name, checksum] = (data, frame, segs)
    return out


# ---- decoders ---------------------------------------------------------------------
@pytest.mark.parametrize("checksum", [False, True])
def test_every_frame_decodes_with_the_host_model(encoded, checksum):
    for name, data in CASES:
        _d, frame, _s = encoded[name, checksum]
        rc, out, word = zg.host_decode(frame)
        assert rc == 0 and out == data and word == len(data), name


@pytest.mark.parametrize("checksum", [False, True])
def test_every_frame_decodes_with_libzstd(encoded, checksum):
    if LIB is None:
        pytest.skip("libzstd.so.1 does not load here: its verdict on the frames is not taken")
    for name, data in CASES:
        _d, frame, _s = encoded[name, checksum]
        v = LIB.verdict(frame)
        assert v == {"stage": "ok", "error": None, "size": len(data)} and LIB.last == data, (name, v)


def _walked(encoded):
    for (name, checksum), (data, frame, segs) in encoded.items():
        yield name, checksum, data, frame, segs, zg.walk(frame)


def test_the_walker_reads_every_header(encoded):
    for name, checksum, data, frame, segs, c in _walked(encoded):
        n = len(data)
        assert c["end"] == len(frame) and c["content"] == n and c["dict_id"] == 0 and c["checksum"] == checksum, name
        if n <= 65536:
            assert c["single"] == 1 and c["fcs_bytes"] == (1 if n <= 255 else 2) and c["window_descriptor"] is None, name
        else:
            assert c["single"] == 0 and c["fcs_bytes"] == 4 and c["window_descriptor"] == 0x30, name
            assert c["window"] == 65536, name
        if checksum:
            assert frame[-4:] == (zg.xxh64(data) & 0xFFFFFFFF).to_bytes(4, "little"), name
        assert len(c["blocks"]) == len(segs) == -(-n // eg.SEGMENT), name
        for k, (b, s) in enumerate(zip(c["blocks"], segs)):
            nk = min(eg.SEGMENT, n - k * eg.SEGMENT)
            assert b["type"] == s["type"] and b["last"] == (k + 1 == len(segs)), name
            assert b["size"] == (s["bytes"] - 3 if b["type"] == eg.COMPRESSED else nk), name
            if b["type"] != eg.COMPRESSED:
                continue
            assert b["lit_type"] == s["lit_form"] and b["streams"] == s["streams"] and b["regen"] == s["nlit"], name
            assert b["nseq"] == s["nseq"] and b["nseq_bytes"] <= 2, name
            assert {"direct": eg.W_DIRECT, "fse": eg.W_FSE}.get(b.get("weights"), eg.W_NONE) == s["wdesc"], name
            if b["nseq"]:
                assert b["modes"] == tuple(s["mode"]), name
            # the smallest Size_Format that holds both sizes
            if b["lit_type"] == eg.RAW:
                assert b["lit_sf"] in ((0, 2) if b["regen"] < 32 else (1,) if b["regen"] < 4096 else (3,)), name
            else:
                big = max(b["regen"], b["lit_comp"])
                assert b["lit_sf"] == (0 if b["streams"] == 1 else 1 if big < 1024 else 2 if big < 16384 else 3), name
                assert (b["streams"] == 1) == (b["regen"] < 256), name


def test_census_of_the_forms(encoded):
    """The list reaches every form the rules can write (in blocks that are written)."""
    blocks, lits, streams, weights, reps, headers = set(), set(), set(), set(), 0, set()
    modes = [set(), set(), set()]
    for name, checksum, data, frame, segs, c in _walked(encoded):
        headers.add((c["single"], c["fcs_bytes"]))
        for b, s in zip(c["blocks"], segs):
            blocks.add(b["type"])
            if b["type"] != eg.COMPRESSED:
                continue
            lits.add(b["lit_type"])
            streams.add(b["streams"])
            weights.add(b.get("weights"))
            reps += int(s["nrep"])
            if b["nseq"]:
                for w in range(3):
                    modes[w].add(b["modes"][w])
    assert blocks == {eg.RAW, eg.RLE, eg.COMPRESSED}
    assert lits == {eg.RAW, eg.COMPRESSED}  # RLE literals cannot occur (csrc/mc_zstd_enc.h) and are not in the rules
    assert streams == {0, 1, 4} and weights == {None, "direct", "fse"}
    assert all(m == {eg.PREDEFINED, eg.RLE_MODE, eg.FSE} for m in modes), modes  # no Repeat_Mode
    assert reps > 0
    assert headers == {(1, 1), (1, 2), (0, 4)}
    by = {name: segs for (name, ck), (_d, _f, segs) in encoded.items() if not ck}
    assert by["wide-skewed"][0]["wdesc"] == eg.W_FSE and by["narrow"][0]["wdesc"] == eg.W_DIRECT
    assert by["one-offset"][0]["nrep"] > 100
    assert list(by["noise70000"]["type"]) == [eg.RAW, eg.RAW] and list(by["run70000"]["type"]) == [eg.RLE, eg.RLE]
    assert list(by["run65537"]["type"]) == [eg.RLE, eg.RAW]  # a last block of one byte: the tie goes to raw
    assert list(by["mix3"]["type"]) == [eg.COMPRESSED, eg.RAW, eg.COMPRESSED]
    assert by["period65535"][0]["nseq"] == 0 and by["period65536"][0]["nseq"] == 0
    assert by["offset65532"][0]["nseq"] == 2 and by["offset65532"][0]["type"] == eg.COMPRESSED  # the run, the far word
    assert by["offset65532"][0]["nlit"] == 5 and by["offset65532"][0]["bytes"] < 40


# ---- sizes ------------------------------------------------------------------------
def test_exact_sizes_and_the_bound(encoded):
    assert eg.host_encode(b"a")[0] == bytes.fromhex("28b52ffd20010900 0061".replace(" ", ""))
    assert _zstd_enc.empty_frame(False) == bytes.fromhex("28b52ffd2000010000")
    assert _zstd_enc.empty_frame(True) == bytes.fromhex("28b52ffd2400010000") + (zg.xxh64(b"") & 0xFFFFFFFF).to_bytes(4, "little")
    if LIB is not None:  # libzstd's own bytes for both
        assert LIB.compress(b"a") == eg.host_encode(b"a")[0] and LIB.compress(b"") == _zstd_enc.empty_frame(False)
        assert LIB.compress(b"", checksum=1) == _zstd_enc.empty_frame(True)
    assert eg.host_encode(b"")[0] is None  # the empty frame is the host's
    assert len(eg.host_encode(bytes(65536))[0]) == 11
    assert len(eg.host_encode(bytes(70000))[0]) == 18 and len(eg.host_encode(bytes(70000), True)[0]) == 22
    assert len(encoded["noise70000", False][1]) == 70016 == _zstd_enc.bound(70000, False)
    for (name, checksum), (data, frame, segs) in encoded.items():
        n = len(data)
        assert len(frame) <= eg.host_bound(n, checksum) == _zstd_enc.bound(n, checksum), name
        head = 6 if n <= 255 else 7 if n <= 65536 else 10
        assert len(frame) == head + int(segs["bytes"].sum()) + 4 * checksum, name
        at = head
        for k, s in enumerate(segs):
            nk = min(eg.SEGMENT, n - k * eg.SEGMENT)
            assert s["off"] == at, name
            at += int(s["bytes"])
            sizes = [3 + nk, 4 if s["same"] else None, None]
            content = int(s["lit_bytes"]) + int(s["seq_bytes"])
            if content < nk:
                sizes[2] = 3 + content
            best = min((t for t in range(3) if sizes[t] is not None), key=lambda t: (sizes[t], t))
            assert s["type"] == best and s["bytes"] == sizes[best], (name, k, sizes)
    for n in (0, 1, 255, 256, 65536, 65537, (1 << 30) - 1):
        for ck in (False, True):
            assert _zstd_enc.bound(n, ck) == eg.host_bound(n, ck), n


def test_a_short_slot_is_refused_and_untouched(encoded):
    for name in ("low13", "noise70000", "mix3"):
        data, frame, _s = encoded[name, True]
        got, _segs, need = eg.host_encode(data, True, cap=len(frame) - 1)  # asserts that nothing was written
        assert got is None and need == len(frame), name
        assert eg.host_encode(data, True, cap=len(frame))[0] == frame, name


def test_compression_actually_happens(encoded):
    n = 1 << 20
    frame = eg.host_encode(bytes(n))[0]
    assert len(frame) == 10 + 4 * 16
    data, frame, _s = encoded["shuffled-floats", False]
    print("shuffled floats:", len(frame), "of", len(data))
    assert len(frame) < 0.8 * len(data)


# ---- the FSE pieces ------------------------------------------------------------------
def test_normalisation_and_count_description():
    rng = np.random.default_rng(3)
    sets = [(np.array([1, 1] + [0] * 34), 9), (np.array([5000] + [1] * 35), 9), (np.ones(53, int), 9),
            (np.array([0, 0, 7, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 9]), 8),
            (np.array([3, 0, 0, 250, 2, 0, 0, 0, 0, 0, 0, 0]), 6)]
    sets += [(rng.integers(0, 400, 36) * (rng.random(36) < 0.5), 9) for _ in range(30)]
    sets += [(rng.integers(0, 30, 12) * (rng.random(12) < 0.6), 6) for _ in range(30)]
    for hist, max_log in sets:
        hist = np.asarray(hist)
        if (hist > 0).sum() < 2:
            continue
        norm, log = eg.host_normalise(hist, max_log)
        used = int((hist > 0).sum())
        assert max(5, int(np.ceil(np.log2(used)))) <= log <= max_log, hist
        assert log == min(max_log, max(5, int(np.ceil(np.log2(used))), int(np.floor(np.log2(hist.sum()))))), hist
        assert norm.sum() == 1 << log and ((norm > 0) == (hist > 0)).all() and norm.min() >= 0, (hist, norm)
        desc = eg.host_write_counts(norm, log)
        # the decoder's reader (through a hand-made FSE-mode sequences header would need a frame; read it here)
        assert _read_counts(desc, max_log, len(hist) - 1) == (list(norm[:np.flatnonzero(norm)[-1] + 1]), log, len(desc)), hist


def _read_counts(buf, max_log, max_sym):
    """RFC 8878 4.1.1, from the text: (counts, accuracy log, bytes)."""
    bits = int.from_bytes(buf + bytes(8), "little")
    pos = 4
    log = (bits & 15) + 5
    assert log <= max_log
    remaining, counts = (1 << log) + 1, []
    while remaining > 1 and len(counts) <= max_sym:
        nb = remaining.bit_length()           # bits to hold 0 ... remaining
        v = (bits >> pos) & ((1 << nb) - 1)
        low = (1 << nb) - 1 - remaining       # values below it take nb - 1 bits
        if (v & ((1 << (nb - 1)) - 1)) < low:
            v &= (1 << (nb - 1)) - 1
            pos += nb - 1
        else:
            if v >= (1 << (nb - 1)):
                v -= low
            pos += nb
        count = v - 1
        assert count >= 0, "no 'less than one' counts"
        remaining -= count
        counts.append(count)
        if count == 0:
            while True:
                r = (bits >> pos) & 3
                pos += 2
                counts += [0] * r
                if r != 3:
                    break
    assert remaining == 1 and (pos + 7) // 8 <= len(buf)
    return counts, log, (pos + 7) // 8


def test_length_codes():
    lib = eg.hostlib()
    ll_base = list(range(16)) + [16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384,
                                 32768, 65536]
    ll_bits = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
    ml_base = list(range(3, 35)) + [35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195,
                                    16387, 32771, 65539]
    ml_bits = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
    for v in list(range(0, 300)) + [4095, 4096, 65535, 65536]:
        c = lib.hze_ll_code(v)
        assert ll_base[c] <= v < ll_base[c] + (1 << ll_bits[c]), v
    for v in list(range(3, 300)) + [4098, 4099, 65535, 65536]:
        c = lib.hze_ml_code(v)
        assert ml_base[c] <= v < ml_base[c] + (1 << ml_bits[c]), v


# ---- surface ----------------------------------------------------------------------------
def test_class_surface():
    assert set(zstd_enc.__all__) == {"Zstd", "compress", "compress_many", "register"}
    assert "zstd_enc" in numcodecs_amd.__all__ and numcodecs_amd.zstd_enc is zstd_enc
    z = zstd_enc.Zstd(level=5, checksum=True)
    assert issubclass(zstd_enc.Zstd, nzstd.Zstd) and zstd_enc.Zstd.codec_id == "zstd"
    assert repr(z) == "Zstd(level=5)" == repr(nzstd.Zstd(level=5, checksum=True))
    assert z.get_config() == {"id": "zstd", "level": 5, "checksum": True} == nzstd.Zstd(5, True).get_config()
    assert zstd_enc.Zstd().get_config() == nzstd.Zstd().get_config()
    assert zstd_enc.Zstd.from_config({"level": 3}) == zstd_enc.Zstd(3)
    assert zstd_enc.Zstd.decode is nzstd.Zstd.decode
    # the decode-only module is as it was
    assert set(nzstd.__all__) == {"Zstd", "decompress", "decompress_many", "register"}
    with pytest.raises(NotImplementedError, match=r"numcodecs\.Zstd"):
        nzstd.Zstd().encode(b"abc")


def test_registration_is_on_request():
    before = dict(codec_registry)
    assert "zstd" not in before
    try:
        zstd_enc.register()
        assert type(get_codec({"id": "zstd", "level": 4})) is zstd_enc.Zstd
        assert set(codec_registry) == set(before) | {"zstd"}
        nzstd.register()  # and the decode-only module still registers its own class
        assert type(get_codec({"id": "zstd"})) is nzstd.Zstd
    finally:
        codec_registry.pop("zstd", None)
    assert dict(codec_registry) == before


class _Sized:
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


def test_argument_checks_need_no_device(monkeypatch):
    assert zstd_enc.compress_many([]) == []
    for level in (-131072, 0, 22, 100):  # libzstd clamps; every level is the one parse
        assert zstd_enc.compress(b"", level=level).tobytes() == _zstd_enc.empty_frame(False)
        assert zstd_enc.Zstd(level).encode(b"").tobytes() == _zstd_enc.empty_frame(False)
    for level in ("3", 3.0, None):
        with pytest.raises(TypeError):
            zstd_enc.compress_many([b"abc"], level=level)
    with pytest.raises(ValueError, match="^outs must have one entry per buffer$"):
        zstd_enc.compress_many([b"abc"], outs=[None, None])
    with pytest.raises(ValueError, match="^destination buffer too small; expected at least 12, got 11$"):
        zstd_enc.compress_many([b"abc"], outs=[np.zeros(11, np.uint8)])
    with pytest.raises(ValueError, match="^destination buffer too small; expected at least 16, got 15$"):
        zstd_enc.compress_many([b"abc"], checksum=True, outs=[np.zeros(15, np.uint8)])
    # the empty buffer never reaches the device
    assert zstd_enc.compress(b"", checksum=True).tobytes() == _zstd_enc.empty_frame(True)
    out = np.zeros(30, np.uint8)
    got = zstd_enc.compress_many([b""], outs=[out])[0]
    assert got.base is out and got.tobytes() == _zstd_enc.empty_frame(False)
    # the decoder refuses that frame, as the reference's does
    rc, _out, _w = zg.host_decode(_zstd_enc.empty_frame(False), 0)
    assert rc == zg.E_EMPTY
    if LIB is not None:
        assert LIB.verdict(_zstd_enc.empty_frame(False))["stage"] == "empty"
    monkeypatch.setattr(_zstd_enc._frames, "flat_bytes", lambda buf, limit: buf)
    monkeypatch.setattr(_zstd_enc, "is_device_tensor", lambda x: False)
    with pytest.raises(ValueError, match=r"2\*\*30 bytes and above are not supported on the GPU; got 1073741824$"):
        zstd_enc.compress_many([_Sized(10), _Sized(1 << 30)])


def test_header_and_binding_name_the_entry_points():
    new = {"mc_zstd_encode_workspace", "mc_zstd_encode_batch"}
    names = set(_header_functions())
    assert new <= names and names == set(_native.EXPORTED)
    assert _native.lib.mc_abi_version() == 2
    ws = _native.lib.mc_zstd_encode_workspace(3, 10, 5000)  # callable without a GPU
    assert 5000 * 20 + 10 * (64 + 1664 + 680) + 3 * 4 <= ws < 5000 * 20 + 11 * 4096
    assert _zstd_enc._RECORD.itemsize == 40 == eg.hostlib().hze_record_bytes()
    assert eg.SEG.itemsize == 64 == eg.hostlib().hze_seg_bytes()


# ---- the sanitized stand-alone run -------------------------------------------------
def test_sanitized_run():
    """The ASan + UBSan build of the scalar encoder, as a process of its own (no
    preloaded runtime): every generated case into a heap buffer of exactly the
    bound, nothing past the returned size touched, decoded back into exactly n
    bytes by csrc/mc_zstd.h's scalar decoder."""
    exe = os.path.join(eg.HOST_DIR, "zstd_enc_hostcheck_main")
    assert os.path.exists(exe), "build with __graft_entry__.build() (make -C tests/native_zstd_enc)"
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "failures 0" in run.stdout, run.stdout
