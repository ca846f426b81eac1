"""The shared case list of the deflate tests (CPU and GPU) and the ctypes
binding of the host model (tests/native_deflate: csrc/mc_deflate.h's scalar
encoder, the bytes the kernels have to reproduce).  Sizes are the smallest
that reach each rule of the format."""

import ctypes
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_DIR = os.path.join(ROOT, "tests", "native_deflate", "_build")
ZLIB, GZIP = 0, 1
CONTAINERS = {"zlib": ZLIB, "gzip": GZIP}
STORED, FIXED, DYNAMIC = 0, 1, 2
SEGMENT = 65536

SEG = np.dtype([("nseq", "<u4"), ("tail_lit", "<u4"), ("type", "<u4"), ("bytes", "<u4"), ("cost", "<u4", (3,)),
                ("hlit", "<u4"), ("hdist", "<u4"), ("hclen", "<u4"), ("off", "<u4"), ("reserved", "<u4")])

_CACHE = {}


def low_entropy(n, seed=5):
    """A slow walk over a few byte values: short matches, skewed literals."""
    rng = np.random.default_rng(seed)
    return (np.cumsum(rng.integers(-1, 2, n)) % 7).astype(np.uint8).tobytes()


def noise(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def skewed(n, seed=9):
    """Bytes drawn from a skewed 40-symbol distribution (no structure to match)."""
    rng = np.random.default_rng(seed)
    p = 0.8 ** np.arange(40)
    return (rng.choice(40, n, p=p / p.sum()) * 5).astype(np.uint8).tobytes()


def smooth_f32(nbytes, seed=1):
    rng = np.random.default_rng(seed)
    return (np.cumsum(rng.standard_normal(nbytes // 4)) / 64).astype(np.float32)


def shuffled_floats(nbytes=65536 + 4096):
    """A smooth float32 series after Shuffle(4)."""
    x = smooth_f32(nbytes)
    return x.view(np.uint8).reshape(-1, 4).T.copy().tobytes()


def periodic(period, n=65536, seed=21):
    base = noise(period, seed + period)
    return (base * (n // period + 1))[:n]


def seam_runs():
    """Runs of one byte that cross the 65536 seam, between noise."""
    out = bytearray(noise(65536 - 300, 31))
    out += b"\x11" * 700            # 300 bytes before the seam, 400 after
    out += noise(100, 32)
    out += b"\x22" * (65536 - 400 - 100 + 259)  # to the next seam and 259 past it
    out += noise(50, 33)
    return bytes(out)


def chunk_cases():
    """[(name, data)]: the issue's list."""
    if "cases" in _CACHE:
        return _CACHE["cases"]
    cases = [("low%d" % n, low_entropy(n)) for n in (1, 3, 12, 13, 64, 65535, 65536, 65537, 131072, 200001)]
    cases.append(("stored70000", noise(70000, 2)))
    cases.append(("skewed70000", skewed(70000)))
    cases.append(("shuffled-floats", shuffled_floats()))
    cases += [("run%d" % n, b"\x07" * n) for n in (258, 259, 260, 261, 516, 517, 70000)]
    cases.append(("seam-runs", seam_runs()))
    cases += [("period%d" % p, periodic(p)) for p in (32767, 32768, 32769)]
    cases.append(("mix3", low_entropy(65536, 6) + noise(65536, 7) + skewed(40000, 8)))
    _CACHE["cases"] = cases
    return cases


# ---- the host model (tests/native_deflate) ---------------------------------------
def hostlib():
    if "lib" not in _CACHE:
        lib = ctypes.CDLL(os.path.join(HOST_DIR, "libdeflate_hostcheck.so"))
        lib.hd_deflate_bound.argtypes = [ctypes.c_size_t, ctypes.c_uint]
        lib.hd_deflate_bound.restype = ctypes.c_size_t
        lib.hd_deflate_encode.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t,
                                          ctypes.c_uint, ctypes.c_uint, ctypes.c_void_p,
                                          ctypes.POINTER(ctypes.c_uint64)]
        lib.hd_deflate_encode.restype = ctypes.c_size_t
        lib.hd_deflate_parse.argtypes = [ctypes.c_char_p, ctypes.c_uint, ctypes.c_void_p,
                                         ctypes.POINTER(ctypes.c_uint), ctypes.c_void_p]
        lib.hd_deflate_parse.restype = ctypes.c_uint
        lib.hd_deflate_code_lengths.argtypes = [ctypes.c_void_p, ctypes.c_uint, ctypes.c_uint, ctypes.c_void_p]
        lib.hd_deflate_code_lengths.restype = None
        for name in ("hd_deflate_npairs", "hd_deflate_len_sym", "hd_deflate_dist_sym"):
            getattr(lib, name).argtypes = [ctypes.c_uint]
            getattr(lib, name).restype = ctypes.c_uint
        lib.hd_deflate_piece.argtypes = [ctypes.c_uint, ctypes.c_uint]
        lib.hd_deflate_piece.restype = ctypes.c_uint
        lib.hd_deflate_seg_bytes.restype = ctypes.c_size_t
        lib.hd_deflate_record_bytes.restype = ctypes.c_size_t
        _CACHE["lib"] = lib
    return _CACHE["lib"]


def host_bound(n, container):
    return int(hostlib().hd_deflate_bound(n, CONTAINERS[container]))


def host_encode(data, container, level=1, cap=None):
    """(frame bytes or None when refused, segment records, the size it needs) of
    the model encoding into `cap` bytes (default: the bound); asserts that
    nothing at or past the returned size was touched."""
    c = CONTAINERS[container]
    cap = host_bound(len(data), container) if cap is None else cap
    buf = np.full(cap + 64, 0xA5, np.uint8)
    segs = np.zeros(max(1, -(-len(data) // SEGMENT)), SEG)
    need = ctypes.c_uint64(0)
    size = int(hostlib().hd_deflate_encode(bytes(data), len(data), buf.ctypes.data, cap, c, level, segs.ctypes.data,
                                           ctypes.byref(need)))
    assert (buf[size:] == 0xA5).all(), "the model wrote past the size it returned"
    return (buf[:size].tobytes() if size else None), segs, int(need.value)


def host_frame(data, container, level=1):
    """The model's frame, cached: the GPU suite compares against it."""
    key = (container, level, data)
    if key not in _CACHE:
        frame, _segs, _need = host_encode(data, container, level)
        _CACHE[key] = frame
    return _CACHE[key]


def host_parse(seg):
    """([(literal run, match length, distance)], closing literals, histogram) of one segment."""
    seqs = np.zeros((max(1, len(seg) // 4), 2), "<u4")
    hist = np.zeros(320, "<u4")
    tail = ctypes.c_uint(0)
    n = hostlib().hd_deflate_parse(bytes(seg), len(seg), seqs.ctypes.data, ctypes.byref(tail), hist.ctypes.data)
    return [(int(a) & 0x1FFFF, int(b), (int(a) >> 17) + 1) for a, b in seqs[:n]], int(tail.value), hist


def host_code_lengths(freq, maxbits):
    freq = np.ascontiguousarray(freq, "<u4")
    lens = np.zeros(len(freq), np.uint8)
    hostlib().hd_deflate_code_lengths(freq.ctypes.data, len(freq), maxbits, lens.ctypes.data)
    return lens
