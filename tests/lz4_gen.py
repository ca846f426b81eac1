"""Test-side helpers for the `lz4` codec tests -- TEST INFRASTRUCTURE ONLY.

* the host build of the product's scalar stitched encoder, decode plan and
  scalar decoder (tests/native_lz4codec) through ctypes: :func:`host_frame`
  (the exact model of the GPU encoder), :func:`host_decode`;
* the inputs the CPU and the GPU suites share.
"""

import ctypes
import os

import numpy as np

from tests import blosc_gen as gen

CODEC_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native_lz4codec", "_build")
SEGMENT = 65536
GUARD = 64
SEAM_TAILS = (5, 11, 12, 14, 15, 16, 266, 267, 268, 521, 522, 523)
_lib = None


def codeclib():
    global _lib
    if _lib is None:
        path = os.path.join(CODEC_DIR, "liblz4codec_hostcheck.so")
        assert os.path.exists(path), "build with __graft_entry__.build() (make -C tests/native_lz4codec)"
        lib = ctypes.CDLL(path)
        sz, vp, cp = ctypes.c_size_t, ctypes.c_void_p, ctypes.c_char_p
        for name in ("hl_lz4c_encode_chunk", "hl_lz4c_encode_frame"):
            getattr(lib, name).argtypes = [cp, sz, vp, sz]
            getattr(lib, name).restype = sz
        lib.hl_lz4c_segment_sum.argtypes = [cp, sz]
        lib.hl_lz4c_segment_sum.restype = sz
        for name in ("hl_lz4c_block_bound", "hl_lz4c_frame_slot"):
            getattr(lib, name).argtypes = [sz]
            getattr(lib, name).restype = sz
        lib.hl_lz4c_decode_frame.argtypes = [cp, sz, vp, sz, ctypes.POINTER(ctypes.c_uint32)]
        lib.hl_lz4_decode_block.argtypes = [cp, sz, vp, sz]
        _lib = lib
    return _lib


def block_bound(n):
    """The stitched block's bound, n + n / 255 + 2."""
    return n + n // 255 + 2


def frame_slot(n):
    """The reference's slot: 4 + LZ4_compressBound(n)."""
    return 4 + n + n // 255 + 16


def host_block(data: bytes) -> bytes:
    """The stitched LZ4 block the model writes for `data` (non-empty) into a
    buffer of exactly the bound's size; guard bytes behind it must survive."""
    data = bytes(data)
    n, cap = len(data), block_bound(len(data))
    assert codeclib().hl_lz4c_block_bound(n) == cap
    out = np.full(cap + GUARD, 0xA5, np.uint8)
    cs = codeclib().hl_lz4c_encode_chunk(data, n, out.ctypes.data, cap)
    assert (out[cap:] == 0xA5).all(), "the scalar encoder wrote past its bound"
    assert 0 < cs <= cap, (cs, cap)
    return out[:cs].tobytes()


def host_frame(data: bytes) -> bytes:
    """The frame the product writes for `data`: the 5 zero bytes for an empty
    buffer (the Python layer's), else the host model's frame."""
    data = bytes(data)
    n = len(data)
    if n == 0:
        return bytes(5)
    cap = frame_slot(n)
    assert codeclib().hl_lz4c_frame_slot(n) == cap
    out = np.full(cap + GUARD, 0xA5, np.uint8)
    fl = codeclib().hl_lz4c_encode_frame(data, n, out.ctypes.data, cap)
    assert (out[cap:] == 0xA5).all(), "the scalar encoder wrote past its slot"
    assert 4 < fl <= cap, (fl, cap)
    frame = out[:fl].tobytes()
    assert frame[:4] == n.to_bytes(4, "little") and frame[4:] == host_block(data)
    return frame


def host_decode(frame: bytes):
    """(code, bytes or None) of the host plan + scalar decoder: code 0, a
    negative host error (-1 short, -2 size word <= 0) or a positive mc_lz4_error."""
    frame = bytes(frame)
    usize = ctypes.c_uint32(0)
    rc = codeclib().hl_lz4c_decode_frame(frame, len(frame), None, 0, ctypes.byref(usize))
    if rc != -3:  # not "destination too small": decided without one
        return rc, None
    out = np.full(usize.value + GUARD, 0xA5, np.uint8)
    rc = codeclib().hl_lz4c_decode_frame(frame, len(frame), out.ctypes.data, usize.value, ctypes.byref(usize))
    assert (out[usize.value:] == 0xA5).all(), "the scalar decoder wrote past the destination"
    return rc, (out[:usize.value].tobytes() if rc == 0 else None)


def _noise(n, seed, nonzero=False):
    rng = np.random.default_rng(seed)
    return rng.integers(1 if nonzero else 0, 256, n, dtype=np.uint8).tobytes()


def _text(n, seed):
    rng = np.random.default_rng(seed)
    words = [b"block", b"stream", b"shuffle", b"frame", b"wave", b"lane", b"offset", b"literal", b"match", b"the",
             b"of", b"and", b"a", b"codec", b"chunk"]
    return b" ".join(words[k] for k in rng.integers(0, len(words), n // 3 + 8))[:n]


def low_entropy(n, seed):
    """n bytes over a three-letter alphabet: matches everywhere."""
    return np.random.default_rng(seed).integers(0, 3, n, dtype=np.uint8).tobytes()


def seam_case(tail):
    """Two segments: zeros followed by `tail` non-zero noise bytes up to the
    first segment's end (its closing literals: exactly `tail` bytes), then 3
    non-zero noise bytes and zeros.  The second segment's first match is found
    in its second window and extended back to position 4 (position 3 is the
    first zero, position 2 is not one), so its first literal run is 4 bytes
    and the stitched head carries tail + 4 literals."""
    return bytes(SEGMENT - tail) + _noise(tail, 100 + tail, True) + _noise(3, 200 + tail, True) + bytes(SEGMENT - 3)


LENGTHS = (1, 12, 13, 64, 65535, 65536, 65537, 65536 + 12, 65536 + 13, 131072, 200001)


def chunk_cases():
    """(name, bytes): the inputs of the issue's list (length 0 is the host's)."""
    cases = [(f"low{n}", low_entropy(n, 300 + n % 97)) for n in LENGTHS]
    cases.append(("mix", _noise(70000, 1) + bytes(50001) + _noise(30011, 2) + _text(80003, 3)))
    cases.append(("noise-middle", low_entropy(SEGMENT, 4) + _noise(SEGMENT, 5) + low_entropy(SEGMENT - 1234, 6)))
    cases += [(f"seam{t}", seam_case(t)) for t in SEAM_TAILS]
    return cases


def loss_cases():
    """(name, 256 KiB of bytes): the inputs of the segmentation-loss table --
    tools/probe_blosc_*.py's float32 signals (N(0,1) and its cumulative sum /
    64) as byte planes, an int32 random walk's low planes, and the rest."""
    rng = np.random.default_rng(0)
    n = 262144
    noise = rng.standard_normal(n).astype("<f4")
    smooth = np.cumsum(noise / 64).astype("<f4")
    walk = (np.cumsum(rng.integers(-20, 21, n)) + 100000).astype("<i4")
    planes = lambda a: np.frombuffer(a.tobytes(), np.uint8).reshape(n, 4).T  # noqa: E731
    cases = [("payload", gen._payload(n, 5))]
    cases += [(f"smooth-f4-plane{k}", planes(smooth)[k].tobytes()) for k in range(4)]
    cases.append(("noise-f4-plane3", planes(noise)[3].tobytes()))
    cases += [(f"walk-i4-plane{k}", planes(walk)[k].tobytes()) for k in (0, 1)]
    cases += [("zeros", bytes(n)), ("text", _text(n, 7))]
    return cases


def fixture_frames():
    """[(array index, config index, array bytes, frame)] of the reference's lz4 fixture set."""
    from tests.helpers import fixture_cases

    out, index = [], {}
    for arr, j, _config, frame in fixture_cases("lz4"):
        raw = arr.tobytes(order="A")
        i = index.setdefault((arr.dtype.str, arr.shape, raw), len(index))
        out.append((i, j, raw, frame))
    return out
