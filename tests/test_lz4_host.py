"""The `lz4` codec, CPU side: the product's scalar stitched encoder
(csrc/mc_lz4_codec.h, compiled for the host by tests/native_lz4codec) against
three independent decoders, both size bounds, the segmentation loss against
the whole-chunk encoder, the reference's fixture frames through the host
scalar decoder, the ``numcodecs_amd.lz4`` surface, and the sanitized
stand-alone run."""

import ctypes
import os
import subprocess

import numpy as np
import pytest

import numcodecs_amd
from numcodecs_amd import _native, codec_registry, get_codec, lz4
from oracle import blosc as oblosc
from tests import blosc_enc_gen as eg
from tests import lz4_gen as lg
from tests.helpers import FIXTURE
from tests.test_boundary import _header_functions


def _liblz4():
    try:
        lib = ctypes.CDLL("liblz4.so.1")
    except OSError:
        return None
    lib.LZ4_decompress_safe.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_int]
    lib.LZ4_decompress_safe.restype = ctypes.c_int
    lib.LZ4_compress_default.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_int]
    lib.LZ4_compress_default.restype = ctypes.c_int
    return lib


CASES = lg.chunk_cases()


@pytest.fixture(scope="module")
def frames():
    return {name: lg.host_frame(data) for name, data in CASES}


def test_case_list_is_the_issues():
    names = [n for n, _d in CASES]
    assert len(names) == len(set(names)) == 11 + 2 + 12
    assert [len(d) for n, d in CASES if n.startswith("low")] == \
        [1, 12, 13, 64, 65535, 65536, 65537, 65536 + 12, 65536 + 13, 131072, 200001]
    assert {int(n[4:]) for n in names if n.startswith("seam")} == {5, 11, 12, 14, 15, 16, 266, 267, 268, 521, 522, 523}
    mix = dict(CASES)["mix"]
    assert len(mix) > 3 * lg.SEGMENT and 70000 % lg.SEGMENT and 120001 % lg.SEGMENT and 150012 % lg.SEGMENT


# ---- the model's frames decode through three decoders ----------------------
@pytest.mark.parametrize("name", [n for n, _d in CASES])
def test_model_frame_decodes(frames, name):
    data = dict(CASES)[name]
    frame = frames[name]
    n = len(data)
    assert frame[:4] == n.to_bytes(4, "little")
    block = frame[4:]
    assert oblosc.lz4_block_decompress(block, n) == data            # the oracle's decoder
    rc, back = lg.host_decode(frame)                                # mc_lz4.h's scalar decoder, behind the plan
    assert rc == 0 and back == data
    if n >= 13:
        eg.parse_block(block, n)  # the block format's end rules


def test_model_frames_against_liblz4(frames):
    lib = _liblz4()
    if lib is None:
        pytest.skip("liblz4.so.1 is not on this machine")
    for name, data in CASES:
        block = frames[name][4:]
        out = ctypes.create_string_buffer(max(len(data), 1))
        assert lib.LZ4_decompress_safe(block, out, len(block), len(data)) == len(data), name
        assert out.raw[:len(data)] == data, name


def test_empty_buffer_is_the_hosts():
    """Length 0: the 5 zero bytes, as liblz4 writes them, with no device."""
    got = lz4.compress(b"")
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.tobytes() == bytes(5) == lg.host_frame(b"")
    assert lz4.compress_many([b"", np.zeros(0, "f4")])[1].tobytes() == bytes(5)
    assert lg.codeclib().hl_lz4c_encode_chunk(b"", 0, None, 0) == 0  # the model refuses it
    lib = _liblz4()
    if lib is not None:
        buf = ctypes.create_string_buffer(16)
        assert lib.LZ4_compress_default(b"", buf, 0, 16) == 1 and buf.raw[0] == 0


def test_expected_shapes(frames):
    """What the crafted inputs are there for really happens."""
    data = dict(CASES)
    for name in ("low1", "low12"):  # no match possible: one literal run
        assert frames[name][4:] == bytes([len(data[name]) << 4]) + data[name]
    # the carry crosses the whole middle segment: one literal run holds all its noise
    seqs = eg.parse_block(frames["noise-middle"][4:], len(data["noise-middle"]))
    assert max(s[0] for s in seqs) >= lg.SEGMENT + 5
    # matches never cross a segment boundary
    for name in ("low131072", "low200001", "mix", "noise-middle"):
        pos = 0
        for lit, off, ml in eg.parse_block(frames[name][4:], len(data[name])):
            pos += lit
            if off is not None:
                assert (pos - off) // lg.SEGMENT == pos // lg.SEGMENT == (pos + ml - 1) // lg.SEGMENT, (name, pos)
            pos += ml


def test_seam_heads_cross_the_extension_thresholds(frames):
    """The stitched head's literal run is tail + 4 bytes (lz4_gen.seam_case):
    9 and 15 straddle the first extension byte, 270 the second, 525 the third."""
    heads = {}
    for t in lg.SEAM_TAILS:
        pos = 0
        for lit, _off, ml in eg.parse_block(frames[f"seam{t}"][4:], 2 * lg.SEGMENT):
            if pos < lg.SEGMENT < pos + lit:
                heads[t] = lit
                assert pos == lg.SEGMENT - t  # the run starts where the first segment's tail does
            pos += lit + ml
    print(heads)
    assert heads == {t: t + 4 for t in lg.SEAM_TAILS}
    ext = lambda v: (v - 15) // 255 + 1 if v >= 15 else 0  # noqa: E731
    assert [ext(heads[t]) for t in lg.SEAM_TAILS] == [0, 1, 1, 1, 1, 1, 2, 2, 2, 3, 3, 3]
    assert [ext(t) for t in lg.SEAM_TAILS] == [0, 0, 0, 0, 1, 1, 1, 1, 1, 2, 2, 2]  # the tail's own run, removed


# ---- the two size bounds ---------------------------------------------------
def test_size_bounds(frames):
    """The stitched block is never larger than the sum of the segments encoded
    as independent blocks, and at most n + n / 255 + 2 bytes; the frame fits
    the reference's 4 + LZ4_compressBound(n) slot (host_frame encodes into
    exactly that and checks the guard bytes behind it)."""
    extra = [("noise200001", lg._noise(200001, 9)), ("noise65536", lg._noise(65536, 10)), ("noise13", lg._noise(13, 11))]
    for name, data in CASES + extra + lg.loss_cases():
        n = len(data)
        block = lg.host_block(data)
        seg_sum = lg.codeclib().hl_lz4c_segment_sum(data, n)
        print(f"{name}: n {n} block {len(block)} segments {seg_sum} bound {lg.block_bound(n)}")
        assert len(block) <= seg_sum, name
        assert len(block) <= lg.block_bound(n) == n + n // 255 + 2, name
        assert 4 + len(block) <= lg.frame_slot(n) == 4 + n + n // 255 + 16, name
        # one byte less than the block needs: refused, nothing written
        small = np.full(len(block) + lg.GUARD, 0xA5, np.uint8)
        assert lg.codeclib().hl_lz4c_encode_chunk(data, n, small.ctypes.data, len(block) - 1) == 0, name
        assert (small == 0xA5).all(), name
    # pure noise meets the second bound within the closing run's extension bytes
    n = 200001
    assert len(lg.host_block(extra[0][1])) == 1 + ((n - 15) // 255 + 1) + n <= lg.block_bound(n)


# ---- segmentation loss -----------------------------------------------------
# stitched size / mc_lz4_encode_stream over the WHOLE chunk, 256 KiB each,
# measured on the CPU (the table of DESIGN.md §6b); the ratio to liblz4 is
# recorded there too and is not bounded (its finder differs by input size).
LOSS_MEASURED = {
    "payload": 1.0033, "smooth-f4-plane0": 1.0000, "smooth-f4-plane1": 1.0000, "smooth-f4-plane2": 1.0010,
    "smooth-f4-plane3": 1.0142, "noise-f4-plane3": 1.0064, "walk-i4-plane0": 1.0000, "walk-i4-plane1": 1.0113,
    "zeros": 1.0260, "text": 1.0018,
}


def test_segmentation_loss():
    """Each ratio at most its measured value + 0.02 (rounding only, not a target)."""
    lib = _liblz4()
    seen = {}
    for name, data in lg.loss_cases():
        n = len(data)
        assert n == 262144
        stitched = len(lg.host_block(data))
        tmp = np.zeros(n, np.uint8)
        whole = eg.enclib().he_lz4_encode_stream(data, n, tmp.ctypes.data, n)
        whole = whole or 1 + ((n - 15) // 255 + 1) + n  # not smaller: one literal run
        seen[name] = stitched / whole
        line = f"{name}: stitched {stitched} whole {whole} ratio {seen[name]:.4f}"
        if lib is not None:
            buf = ctypes.create_string_buffer(n + n // 255 + 16)
            ref = lib.LZ4_compress_default(data, buf, n, len(buf))
            line += f" liblz4 {ref} ratio {stitched / ref:.4f}"
        print(line)
    assert set(seen) == set(LOSS_MEASURED)
    for name, r in seen.items():
        assert r <= LOSS_MEASURED[name] + 0.02, (name, r)


# ---- the reference's fixture frames ----------------------------------------
def test_fixture_frames_decode_through_the_host_decoder():
    fx = lg.fixture_frames()
    assert len(fx) == 91 and len({i for i, _j, _r, _f in fx}) == 13 and len({j for _i, j, _r, _f in fx}) == 7
    for i, j, raw, frame in fx:
        rc, back = lg.host_decode(frame)
        assert rc == 0 and back == raw, (i, j, rc)
        assert oblosc.lz4_block_decompress(frame[4:], len(raw)) == raw, (i, j)


def test_host_decoder_rejects_malformed_frames():
    data = lg.low_entropy(3000, 1)
    frame = lg.host_frame(data)
    assert lg.host_decode(frame[:3])[0] == -1
    assert lg.host_decode(bytes(4) + frame[4:])[0] == -2
    assert lg.host_decode((0x80000000).to_bytes(4, "little") + frame[4:])[0] == -2
    assert lg.host_decode(frame[:4])[0] == 4  # MC_LZ4_E_TRUNCATED: no block at all
    assert lg.host_decode((3001).to_bytes(4, "little") + frame[4:])[0] == 10  # MC_LZ4_E_SIZE
    assert lg.host_decode((2999).to_bytes(4, "little") + frame[4:])[0] in (6, 9)  # literal / match leaves the destination
    assert lg.host_decode(frame[:-1])[0] > 0
    assert lg.host_decode((1 << 30).to_bytes(4, "little") + frame[4:])[0] == 12  # MC_LZ4_E_TABLE: the plan refuses 2**30


# ---- the surface, no GPU needed --------------------------------------------
def test_class_surface():
    c = lz4.LZ4()
    assert repr(c) == "LZ4(acceleration=1)" and lz4.DEFAULT_ACCELERATION == 1
    assert c.get_config() == {"id": "lz4", "acceleration": 1}
    z = lz4.LZ4(acceleration=7)
    assert repr(z) == "LZ4(acceleration=7)" and z.get_config() == {"id": "lz4", "acceleration": 7}
    cfg = z.get_config()
    assert cfg.pop("id") == "lz4"
    assert lz4.LZ4.from_config(cfg) == z and z != c and c == lz4.LZ4()
    assert lz4.LZ4.codec_id == "lz4" and lz4.LZ4.max_buffer_size == 0x7E000000
    assert lz4.LZ4(acceleration=-3).get_config() == {"id": "lz4", "acceleration": -3}  # kept as given
    assert set(lz4.__all__) == {"LZ4", "DEFAULT_ACCELERATION", "compress", "compress_many", "decompress",
                                "decompress_many", "register"}
    assert "lz4" in numcodecs_amd.__all__ and numcodecs_amd.lz4 is lz4
    for doc in (lz4.LZ4.__doc__, lz4.compress_many.__doc__, lz4.__doc__):  # acceleration changes nothing: said so
        assert "no levels" in " ".join(doc.split())


def test_acceleration_is_accepted_and_ignored():
    for acc in (-5, 0, 1, 9, 65537):  # <= 0 means 1, as in the reference; nothing else changes either
        assert lz4.compress(b"", acc).tobytes() == bytes(5)
        assert lz4.LZ4(acceleration=acc).encode(np.zeros(0, "u1")).tobytes() == bytes(5)
    with pytest.raises((TypeError, ValueError)):
        lz4.compress(b"", "fast")


def test_registration_is_on_request():
    before = dict(codec_registry)
    assert "lz4" not in before
    try:
        lz4.register()
        got = get_codec({"id": "lz4", "acceleration": 3})
        assert type(got) is lz4.LZ4 and got == lz4.LZ4(3)
        assert set(codec_registry) == set(before) | {"lz4"}
    finally:
        codec_registry.pop("lz4", None)
    assert dict(codec_registry) == before


class _Sized:
    """A buffer that only claims its size: the checks under test come before
    anything looks at the bytes."""

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


def test_decode_errors_need_no_device(monkeypatch):
    frame = np.frombuffer(lg.host_frame(lg.low_entropy(500, 2)), np.uint8)
    with pytest.raises(ValueError, match="^bad input data$") as e:
        lz4.decompress(b"\x01\x00\x00")
    assert e.value.frame_errors == {0: (-1, 0)}
    with pytest.raises(ValueError, match="^bad input data$"):
        lz4.decompress(b"")
    for word in (0, -1, -(2**31)):
        with pytest.raises(RuntimeError, match="^LZ4 decompression error: invalid input data$"):
            lz4.decompress(word.to_bytes(4, "little", signed=True) + frame[4:].tobytes())
    with pytest.raises(RuntimeError, match="^LZ4 decompression error: invalid input data$"):
        lz4.LZ4().decode(bytes(5))  # the empty buffer's frame: the reference refuses it too
    with pytest.raises(ValueError, match="^destination buffer too small; expected at least 500, got 499$"):
        lz4.decompress(frame, np.zeros(499, np.uint8))
    ro = np.zeros(500, np.uint8)
    ro.flags.writeable = False
    with pytest.raises(ValueError, match="^destination buffer is read-only$"):
        lz4.decompress(frame, ro)
    with pytest.raises(RuntimeError, match="^LZ4 decompression error: -4$"):
        lz4.decompress(frame[:4])  # a size word and no block
    # a batch names its bad frames
    with pytest.raises(RuntimeError, match="invalid input data") as e:
        lz4.decompress_many([frame, bytes(8), frame, bytes(5)])
    assert e.value.frame_errors == {1: (-1, 0), 3: (-1, 0)}
    with pytest.raises(ValueError, match="^outs must have one entry per frame$"):
        lz4.decompress_many([frame], [None, None])
    assert lz4.decompress_many([]) == [] and lz4.compress_many([]) == []
    # the 2**30 limit, decode side: a size word of 2**30 (no such buffer is made)
    big = (1 << 30).to_bytes(4, "little") + frame[4:].tobytes()
    with pytest.raises(ValueError, match=r"^LZ4 chunks of 2\*\*30 bytes and above are not supported"):
        lz4.decompress(big)
    assert (1 << 30) <= lz4.LZ4.max_buffer_size
    # ensure_contiguous_ndarray's own limit (the limit itself would need 2 GiB)
    monkeypatch.setattr(lz4.LZ4, "max_buffer_size", 1000)
    with pytest.raises(ValueError, match="^Codec does not support buffers of > 1000 bytes$"):
        lz4.compress(np.zeros(1001, np.uint8))
    with pytest.raises(ValueError, match="^Codec does not support buffers of > 1000 bytes$"):
        lz4.decompress(np.zeros(1001, np.uint8))


def test_encode_limit_needs_no_device(monkeypatch):
    """2**30 bytes and above are refused before any launch.  The buffer is not
    made: the flattening step is replaced by one that reports the length."""
    monkeypatch.setattr(lz4, "_flat_bytes", lambda buf: buf)
    monkeypatch.setattr(lz4, "is_device_tensor", lambda x: False)
    with pytest.raises(ValueError, match=r"^LZ4 chunks of 2\*\*30 bytes and above are not supported on the GPU; got 1073741824$"):
        lz4.compress_many([_Sized(1 << 30)])
    with pytest.raises(ValueError, match=r"2\*\*30"):
        lz4.compress_many([_Sized(10), _Sized((1 << 30) + 5)])


def test_header_and_binding_name_the_entry_points():
    new = {"mc_lz4_encode_workspace", "mc_lz4_encode_batch", "mc_lz4_decode_workspace", "mc_lz4_decode_batch"}
    names = set(_header_functions())
    assert new <= names and names == set(_native.EXPORTED)
    assert _native.lib.mc_abi_version() == 2
    assert _native.lib.mc_lz4_encode_workspace(3, 10, 1000) >= 1000 + (7 * 10 + 3 * 3) * 4
    assert _native.lib.mc_lz4_decode_workspace(10) >= 10 * 32
    assert lz4._ENC_RECORD.itemsize == 40 and lz4._DEC_RECORD.itemsize == 32


# ---- the sanitized stand-alone run -----------------------------------------
def test_sanitized_run(tmp_path):
    """The ASan + UBSan build of the scalar stitched encoder and the scalar
    decoder, as a process of its own (no LD_PRELOAD): the shared inputs and 120
    generated ones into heap buffers of exactly the bound's size and back, the
    91 fixture frames and mutations of them into exactly sized destinations."""
    exe = os.path.join(lg.CODEC_DIR, "lz4codec_hostcheck_main")
    assert os.path.exists(exe), "build with __graft_entry__.build() (make -C tests/native_lz4codec)"
    for k, (name, data) in enumerate(CASES):
        (tmp_path / f"{k:02d}-{name}.bin").write_bytes(data)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    run = subprocess.run([exe, str(tmp_path), os.path.join(FIXTURE, "lz4")], capture_output=True, text=True,
                         timeout=600, env=env)
    assert run.returncode == 0, run.stdout + run.stderr
    assert f"chunks {len(CASES) + 120} files {len(CASES)} frames 91 " in run.stdout and "failures 0" in run.stdout, \
        run.stdout
