"""bz2 encode without a GPU: the scalar model of csrc/mc_bz2_enc.h (compiled
for the host by tests/native_bz2_enc) over the shared case list, read back by
the stdlib and by the project's scalar bunzip model; the block count, the level
digit and the bound; the model's sort against a naive rotation sort; the
refused short destination; the ``numcodecs_amd.bz2_enc`` surface and the checks
that need no GPU; and the sanitized stand-alone run."""

import bz2
import os
import subprocess

import numpy as np
import pytest

from numcodecs_amd import _bz2_enc, bz2_enc
from numcodecs_amd import bz2 as nbz2
from numcodecs_amd.registry import codec_registry, get_codec
from tests import bz2_enc_gen as g
from tests import bz2_gen, bz2_write

CASES = g.case_levels()
IDS = ["%s-L%d" % (name, level) for name, _d, level in CASES]
END_MAGIC = 0x177245385090
BLOCK_MAGIC = 0x314159265359


@pytest.mark.parametrize("name,data,level", CASES, ids=IDS)
def test_model_frames_decode(name, data, level):
    frame, err, census = g.host_encode(data, level)
    assert err == 0 and frame is not None
    assert frame[:3] == b"BZh" and frame[3] == 0x30 + level
    assert bz2.decompress(frame) == data
    e, got, blocks = bz2_gen.host_decode(frame, len(data))  # the project's scalar bunzip model
    assert e == 0 and got == data
    assert census["blocks"] == blocks == -(-len(data) // g.seg(level))
    assert len(frame) <= g.host_bound(len(data), level)
    assert g.host_bound(len(data), level) == _bz2_enc.bound(len(data), level)
    assert g.hostlib().hb_bz2e_seg(level) == g.seg(level) == _bz2_enc.segment(level)


def test_bound_formula_agrees_at_the_seams():
    for level in range(1, 10):
        s = g.seg(level)
        for n in (0, 1, 3, 4, 5, s - 1, s, s + 1, 2 * s, 2 * s + 7, (1 << 30) - 1):
            assert g.host_bound(n, level) == _bz2_enc.bound(n, level), (n, level)
    assert g.hostlib().hb_bz2e_chunk_bytes() == _bz2_enc._RECORD.itemsize


def _smaller_rotations(pre):
    n = len(pre)
    doubled = pre + pre
    first = doubled[:n]
    return sum(1 for i in range(n) if doubled[i:i + n] < first)


def test_sort_equals_the_naive_rotation_sort():
    seen = 0
    for name, data, _levels in g.chunk_cases():
        if not 0 < len(data) <= 3000:
            continue
        pre = g.host_rle1(data)
        assert pre == bz2_write.rle1(data), name
        col, orig, rounds = g.host_bwt(pre)
        want_col, _want_orig = bz2_write.bwt(pre)
        assert col == want_col, name
        assert orig == _smaller_rotations(pre), name  # equal rotations: the definition, not the sort's tie order
        assert rounds <= max(1, (len(pre) - 1).bit_length()), name
        seen += 1
    assert seen > 40


def test_doubling_depth_is_bounded_on_zeros():
    pre = g.host_rle1(bytes(1 << 20))
    _col, orig, rounds = g.host_bwt(pre[:g.seg(9) // 255 * 5])
    assert rounds <= 17 and orig == 0


def test_zeros_and_shuffled_floats_compress(capsys):
    zeros = bytes(1 << 20)
    for level in (1, 9):
        frame, _e, _c = g.host_encode(zeros, level)
        with capsys.disabled():
            print("\nbz2 encode: 1 MiB zeros L%d: %d bytes, bz2.compress %d" % (level, len(frame), len(bz2.compress(zeros, level))))
        assert len(frame) < len(zeros) // 100
    floats = g.shuffled_floats()
    frame, _e, _c = g.host_encode(floats, 1)
    with capsys.disabled():
        print("bz2 encode: shuffled floats %d: %d bytes, bz2.compress %d" % (len(floats), len(frame), len(bz2.compress(floats, 1))))
    assert len(frame) < len(floats)


def test_noise_stays_under_the_bound_and_mixed_uses_more_tables():
    noise = dict((n, d) for n, d, _l in g.chunk_cases())["noise"]
    frame, _e, census = g.host_encode(noise, 1)
    # the code stage writes the smaller of the refined tables and the fallback: never above the fallback's bound
    assert len(frame) <= g.host_bound(len(noise), 1)
    assert census["bits"] <= 48 + 32 + 25 + 16 + 256 + 18 + -(-(len(noise) * 5 // 4 + 1) // 50) + 526 + 9 * (len(noise) * 5 // 4 + 1)
    mixed = dict((n, d) for n, d, _l in g.chunk_cases())["mixed"]
    _frame, _e, census = g.host_encode(mixed, 1)
    assert census["multi_table"] == 1 and census["fallback"] == 0


def test_fallback_is_taken_where_it_is_smaller():
    taken = sum(g.host_encode(d, lv)[2]["fallback"] for _n, d, lv in CASES if 0 < len(d) < 300)
    assert taken > 0


@pytest.mark.parametrize("name", ["len1", "run260", "ab33", "nsym600", "mixed", "text159975"])
def test_short_destination_is_refused_untouched(name):
    data = dict((n, d) for n, d, _l in g.chunk_cases())[name]
    frame, _e, _c = g.host_encode(data, 1)
    short, err, _c = g.host_encode(data, 1, cap=len(frame) - 1)  # host_encode asserts the buffer is untouched
    assert short is None and err == _bz2_enc.E_SPACE
    exact, err, _c = g.host_encode(data, 1, cap=len(frame))
    assert err == 0 and exact == frame


# ---- the surface ---------------------------------------------------------------------
def test_class_config_repr_and_register():
    c = bz2_enc.BZ2(level=5)
    assert isinstance(c, nbz2.BZ2) and c.codec_id == "bz2"
    assert c.get_config() == {"id": "bz2", "level": 5} == nbz2.BZ2(level=5).get_config()
    assert repr(c) == repr(nbz2.BZ2(level=5))
    before = codec_registry.get("bz2")
    try:
        codec_registry.pop("bz2", None)
        import importlib
        importlib.reload(bz2_enc)
        assert "bz2" not in codec_registry  # nothing on import
        bz2_enc.register()
        assert codec_registry["bz2"] is bz2_enc.BZ2
        assert isinstance(get_codec({"id": "bz2", "level": 3}), bz2_enc.BZ2)
    finally:
        codec_registry.pop("bz2", None)
        if before is not None:
            codec_registry["bz2"] = before


@pytest.mark.parametrize("level", [0, 10, -1, 100, 1.5, "1", None])
def test_level_errors_are_the_stdlibs(level):
    with pytest.raises(Exception) as want:
        bz2.compress(b"", level)
    with pytest.raises(type(want.value)) as got:
        bz2_enc.compress_many([b"abc"], level)
    assert str(got.value) == str(want.value)
    with pytest.raises(type(want.value)):
        bz2_enc.BZ2(level=level).encode(b"abc")


class _Sized:
    """Stands for a buffer of n bytes that is never touched."""

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


def test_chunk_limit(monkeypatch):
    monkeypatch.setattr(_bz2_enc._frames, "flat_bytes", lambda buf, limit: buf)
    monkeypatch.setattr(_bz2_enc, "is_device_tensor", lambda x: False)
    with pytest.raises(ValueError, match=r"2\*\*30 bytes and above are not supported on the GPU; got 1073741824$"):
        bz2_enc.compress_many([_Sized(10), _Sized(1 << 30)])


def test_outs_must_match():
    with pytest.raises(ValueError, match="one entry per buffer"):
        bz2_enc.compress_many([b"a", b"b"], outs=[None])
    assert bz2_enc.compress_many([]) == []


@pytest.mark.parametrize("level", range(1, 10))
def test_empty_frame_is_the_stdlibs(level):
    want = bz2.compress(b"", level)
    assert _bz2_enc.empty_frame(level) == want
    got = bz2_enc.compress(b"", level)  # no launch: works without a GPU
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.tobytes() == want
    out = np.full(_bz2_enc.bound(0, level) + 2, 0xA5, np.uint8)
    got = bz2_enc.compress_many([b""], level, outs=[out])[0]
    assert got.tobytes() == want and out[len(want):].tolist() == [0xA5, 0xA5]
    assert bz2_enc.BZ2(level).encode(np.zeros(0, np.uint8)).tobytes() == want


def test_decode_only_class_still_refuses_to_encode():
    with pytest.raises(NotImplementedError, match="encode with numcodecs.BZ2"):
        nbz2.BZ2().encode(b"abc")


def test_sanitized_standalone_run(tmp_path):
    exe = os.path.join(g.HOST_DIR, "bz2_enc_hostcheck_main")
    assert os.path.exists(exe), "build with __graft_entry__.build() (make -C tests/native_bz2_enc)"
    blocks = 0
    for k, (name, data, level) in enumerate(CASES):
        (tmp_path / ("c%03d-%s.%d.bin" % (k, name, level))).write_bytes(data)
        blocks += -(-len(data) // g.seg(level))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    run = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=600, env=env)
    assert run.returncode == 0, run.stdout + run.stderr
    assert ("cases %d blocks %d " % (len(CASES), blocks)) in run.stdout and run.stdout.rstrip().endswith("failures 0"), run.stdout
