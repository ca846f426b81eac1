"""The shared case list of the bz2 encode tests (CPU and GPU) and the ctypes
binding of the host model (tests/native_bz2_enc: csrc/mc_bz2_enc.h's scalar
encoder, the bytes the kernels have to reproduce).  Every case is small; the
largest is one level-9 block."""

import ctypes
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_DIR = os.path.join(ROOT, "tests", "native_bz2_enc", "_build")

_CACHE = {}


def seg(level):
    """S(level): the input bytes of one block."""
    return 80000 * level - 16


def noise(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def text_like(n, seed=3):
    """Words of a small vocabulary: long repeats, a skewed alphabet."""
    rng = np.random.default_rng(seed)
    words = [bytes(rng.integers(97, 123, int(k), dtype=np.uint8)) for k in rng.integers(2, 9, 60)]
    out = b" ".join(words[int(i)] for i in rng.integers(0, 60, n // 4 + 8))
    return out[:n]


def shuffled_floats(nbytes=65536 + 4096):
    """A smooth float32 series after Shuffle(4) (the deflate list's case)."""
    rng = np.random.default_rng(1)
    x = (np.cumsum(rng.standard_normal(nbytes // 4)) / 64).astype(np.float32)
    return x.view(np.uint8).reshape(-1, 4).T.copy().tobytes()


def distinct(k, seed=11):
    """k bytes whose column gives about k symbols: no zero runs to speak of."""
    rng = np.random.default_rng(seed + k)
    return rng.integers(0, 256, k, dtype=np.uint8).tobytes()


def zero_run_case(r):
    """A block whose column holds a zero run of about r: a run of r + 1 equal
    rotations' predecessors comes from r + 1 copies of one byte pair context."""
    return b"q" + b"xy" * (r + 1) + b"z"


def chunk_cases():
    """[(name, data, levels)]: the issue's list."""
    if "cases" in _CACHE:
        return _CACHE["cases"]
    s1 = seg(1)
    one = (1,)
    cases = [("len%d" % n, bytes(range(65, 65 + n)), (1, 9)) for n in (0, 1, 2, 3, 4, 5)]
    cases += [("run%d" % n, b"\x07" * n, one) for n in (3, 4, 5, 255, 256, 259, 260, 1000)]
    cases.append(("run-straddle", noise(s1 - 100, 41) + b"\x33" * 300 + noise(50, 42), one))
    cases.append(("alpha256", bytes(range(256)) * 3 + noise(700, 43), one))
    cases.append(("alpha1", b"\x00" * 3, one))
    cases += [("ab%d" % k, b"ab" * k, one) for k in (1, 2, 33, 1000)]
    cases += [("abc%d" % k, b"abc" * k, one) for k in (1, 5, 700)]
    cases.append(("zeros1M", bytes(1 << 20), (1, 9)))
    cases += [("nsym%d" % k, distinct(k), one) for k in (46, 47, 48, 49, 50, 51, 52)]
    for t in (200, 600, 1200, 2400):
        cases += [("nsym%d" % k, distinct(k), one) for k in (t - 4, t - 3, t - 2, t - 1, t, t + 1)]
    cases += [("zrun%d" % r, zero_run_case(r), one) for r in (1, 2, 3, 4, 7, 8, 15, 16, 31, 32, 63, 64, 127, 128, 1023, 1024)]
    cases += [("text%d" % n, text_like(n), (1, 5, 9) if n > seg(5) else (1,) if n <= s1 else (1, 5))
              for n in (s1 - 1, s1, s1 + 1, 2 * s1 + 7)]
    cases.append(("noise", noise(70000, 2), one))
    cases.append(("mixed", text_like(30000, 5) + noise(30000, 6), one))
    cases.append(("shuffled-floats", shuffled_floats(), one))
    cases.append(("full9", text_like(seg(9) // 2, 7) + shuffled_floats(seg(9) - seg(9) // 2 + 3)[:seg(9) - seg(9) // 2], (9,)))
    _CACHE["cases"] = cases
    return cases


def case_levels():
    """[(name, data, level)], one entry per level at which the case differs."""
    return [(name, data, level) for name, data, levels in chunk_cases() for level in levels]


# ---- the host model (tests/native_bz2_enc) -----------------------------------------
def hostlib():
    if "lib" not in _CACHE:
        lib = ctypes.CDLL(os.path.join(HOST_DIR, "libbz2_enc_hostcheck.so"))
        lib.hb_bz2e_encode.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint,
                                       ctypes.c_void_p]
        lib.hb_bz2e_encode.restype = ctypes.c_int
        lib.hb_bz2e_bound.argtypes = [ctypes.c_uint64, ctypes.c_uint]
        lib.hb_bz2e_bound.restype = ctypes.c_uint64
        lib.hb_bz2e_seg.argtypes = [ctypes.c_uint]
        lib.hb_bz2e_seg.restype = ctypes.c_uint
        lib.hb_bz2e_rle1.argtypes = [ctypes.c_char_p, ctypes.c_uint, ctypes.c_void_p]
        lib.hb_bz2e_rle1.restype = ctypes.c_uint
        lib.hb_bz2e_bwt.argtypes = [ctypes.c_char_p, ctypes.c_uint, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint)]
        lib.hb_bz2e_bwt.restype = ctypes.c_uint
        lib.hb_bz2e_chunk_bytes.restype = ctypes.c_size_t
        _CACHE["lib"] = lib
    return _CACHE["lib"]


def host_bound(n, level):
    return int(hostlib().hb_bz2e_bound(n, level))


def host_encode(data, level, cap=None):
    """(frame bytes or None when refused, error code, census) of the model
    encoding into `cap` bytes (default: the bound); asserts that nothing at or
    past the returned size was touched, and nothing at all when refused."""
    cap = host_bound(len(data), level) if cap is None else cap
    buf = np.full(cap + 64, 0xA5, np.uint8)
    out = np.zeros(6, np.uint64)
    err = int(hostlib().hb_bz2e_encode(bytes(data), len(data), buf.ctypes.data, cap, level, out.ctypes.data))
    size = int(out[0])
    assert (buf[size:] == 0xA5).all(), "the model wrote past the size it returned"
    census = dict(zip(("blocks", "fallback", "multi_table", "rounds_max", "bits"), (int(v) for v in out[1:])))
    return (buf[:size].tobytes() if size else None), err, census


def host_frame(data, level):
    """The model's frame, cached: the GPU suite compares against it."""
    key = (level, data)
    if key not in _CACHE:
        frame, err, _census = host_encode(data, level)
        assert err == 0 and frame is not None
        _CACHE[key] = frame
    return _CACHE[key]


def host_rle1(data):
    out = np.zeros(len(data) * 5 // 4 + 8, np.uint8)
    n = hostlib().hb_bz2e_rle1(bytes(data), len(data), out.ctypes.data)
    return out[:n].tobytes()


def host_bwt(block):
    """(column, origPtr, doubling rounds) of the model's sort."""
    col = np.zeros(len(block), np.uint8)
    rounds = ctypes.c_uint(0)
    orig = hostlib().hb_bz2e_bwt(bytes(block), len(block), col.ctypes.data, ctypes.byref(rounds))
    return col.tobytes(), int(orig), int(rounds.value)
