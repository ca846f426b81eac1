"""The shared case list of the zstd encode tests (CPU and GPU) and the ctypes
binding of the host model (tests/native_zstd_enc: csrc/mc_zstd_enc.h's scalar
encoder, the bytes the kernels have to reproduce).  Sizes are the smallest
that reach each rule of the format."""

import ctypes
import os

import numpy as np

from tests import deflate_gen as dg
from tests import zstd_gen as zg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_DIR = os.path.join(ROOT, "tests", "native_zstd_enc", "_build")
SEGMENT = 65536
RAW, RLE, COMPRESSED = 0, 1, 2          # block types and literals forms
PREDEFINED, RLE_MODE, FSE = 0, 1, 2     # modes
W_NONE, W_DIRECT, W_FSE = 0, 1, 2       # the tree description

SEG = np.dtype([("nseq", "<u4"), ("nlit", "<u4"), ("same", "<u4"), ("nrep", "<u4"), ("type", "<u4"), ("bytes", "<u4"),
                ("lit_form", "<u4"), ("streams", "<u4"), ("wdesc", "<u4"), ("mode", "<u4", (3,)), ("lit_bytes", "<u4"),
                ("seq_bytes", "<u4"), ("off", "<u4"), ("reserved", "<u4")])

_CACHE = {}


def wide_skewed(n, seed=41):
    """All 256 byte values, a few of them frequent: more than 128 weights with a
    skewed distribution, no structure to match."""
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 256, n)
    common = rng.integers(0, 9, n) * 29
    return np.where(rng.random(n) < 0.75, common, v).astype(np.uint8).tobytes()


def narrow(n, seed=42):
    """Byte values 0 ... 5, skewed: five weights, which the direct form writes in fewer bytes."""
    rng = np.random.default_rng(seed)
    p = 0.5 ** np.arange(6)
    return rng.choice(6, n, p=p / p.sum()).astype(np.uint8).tobytes()


def one_offset(n, seed=43):
    """Records of 12 bytes: 8 copied from the record before, 4 of noise.  Every
    sequence has offset 12 and literals in front: repeat codes, RLE_Mode on OF,
    on ML and on LL."""
    rng = np.random.default_rng(seed)
    out = np.zeros(n, np.uint8)
    fresh = rng.integers(0, 256, n, dtype=np.uint8)
    for i in range(0, n, 12):
        rec = fresh[i:i + 12].copy()
        if i:
            rec[:min(8, len(rec))] = out[i - 12:i - 12 + min(8, len(rec))]
        out[i:i + len(rec)] = rec
    return out.tobytes()


def varied_sequences(n, seed=44):
    """Noise with copies of varied length at varied distance between literal runs
    of varied length: enough sequences of many codes for FSE-compressed tables."""
    rng = np.random.default_rng(seed)
    out = bytearray(rng.integers(0, 256, 256, dtype=np.uint8).tobytes())
    while len(out) < n:
        out += rng.integers(0, 256, int(rng.integers(0, 40)), dtype=np.uint8).tobytes()
        ln = int(rng.integers(4, 80))
        back = int(rng.integers(ln, min(len(out), 60000)))
        out += out[len(out) - back:len(out) - back + ln]
    return bytes(out[:n])


def chunk_cases():
    """[(name, data)]: the issue's list."""
    if "cases" in _CACHE:
        return _CACHE["cases"]
    cases = [("low%d" % n, dg.low_entropy(n)) for n in (1, 3, 4, 5, 12, 13, 64, 255, 256, 257, 65535, 65536, 65537,
                                                        131072, 200001)]
    cases.append(("noise70000", dg.noise(70000, 2)))
    cases += [("run%d" % n, b"\x07" * n) for n in (1, 2, 70000, 65537)]
    cases.append(("skewed70000", dg.skewed(70000)))
    cases.append(("shuffled-floats", dg.shuffled_floats()))
    cases.append(("seam-runs", dg.seam_runs()))
    cases += [("period%d" % p, dg.periodic(p)) for p in (65535, 65536)]  # one segment: no match at all
    # the longest offset a match can have inside a segment (the hash table still holds position 0: few words went in)
    cases.append(("offset65532", b"ABCD" + bytes(65528) + b"ABCD"))
    cases.append(("mix3", dg.low_entropy(65536, 6) + dg.noise(65536, 7) + dg.skewed(40000, 8)))
    cases += [("mixed70000-%d" % s, zg.mixed(70000, s)) for s in (5, 6)]
    cases.append(("triples", zg.triples()))
    cases.append(("wide-skewed", wide_skewed(20000)))
    cases.append(("wide-skewed-200", wide_skewed(200, 45)))
    cases.append(("narrow", narrow(3000)))
    cases.append(("one-offset", one_offset(6000)))
    cases.append(("varied-sequences", varied_sequences(40000)))
    _CACHE["cases"] = cases
    return cases


# ---- the host model (tests/native_zstd_enc) -----------------------------------------
def hostlib():
    if "lib" not in _CACHE:
        lib = ctypes.CDLL(os.path.join(HOST_DIR, "libzstd_enc_hostcheck.so"))
        sz, vp, u = ctypes.c_size_t, ctypes.c_void_p, ctypes.c_uint
        lib.hze_bound.argtypes, lib.hze_bound.restype = [sz, u], sz
        lib.hze_encode.argtypes = [ctypes.c_char_p, sz, vp, sz, u, vp, ctypes.POINTER(ctypes.c_uint64)]
        lib.hze_encode.restype = sz
        lib.hze_normalise.argtypes, lib.hze_normalise.restype = [vp, u, u, u, vp], u
        lib.hze_write_counts.argtypes, lib.hze_write_counts.restype = [vp, u, u, vp], u
        for name in ("hze_ll_code", "hze_ml_code"):
            getattr(lib, name).argtypes, getattr(lib, name).restype = [u], u
        lib.hze_seg_bytes.restype = lib.hze_record_bytes.restype = sz
        _CACHE["lib"] = lib
    return _CACHE["lib"]


def host_bound(n, checksum):
    return int(hostlib().hze_bound(n, int(bool(checksum))))


def host_encode(data, checksum=False, cap=None):
    """(frame bytes or None when refused, segment records, the size it needs) of
    the model encoding into `cap` bytes (default: the bound); asserts that
    nothing at or past the returned size was touched."""
    cap = host_bound(len(data), checksum) if cap is None else cap
    buf = np.full(cap + 64, 0xA5, np.uint8)
    segs = np.zeros(max(1, -(-len(data) // SEGMENT)), SEG)
    need = ctypes.c_uint64(0)
    size = int(hostlib().hze_encode(bytes(data), len(data), buf.ctypes.data, cap, int(bool(checksum)), segs.ctypes.data,
                                    ctypes.byref(need)))
    assert (buf[size:] == 0xA5).all(), "the model wrote past the size it returned"
    return (buf[:size].tobytes() if size else None), segs, int(need.value)


def host_frame(data, checksum=False):
    """The model's frame, cached: the GPU suite compares against it."""
    key = (bool(checksum), data)
    if key not in _CACHE:
        _CACHE[key] = host_encode(data, checksum)[0]
    return _CACHE[key]


def host_normalise(hist, max_log):
    hist = np.ascontiguousarray(hist, "<u4")
    norm = np.zeros(len(hist), "<i2")
    log = hostlib().hze_normalise(hist.ctypes.data, len(hist), int(hist.sum()), max_log, norm.ctypes.data)
    return norm, int(log)


def host_write_counts(norm, log):
    norm = np.ascontiguousarray(norm, "<i2")
    out = np.zeros(80, np.uint8)
    n = hostlib().hze_write_counts(norm.ctypes.data, len(norm), log, out.ctypes.data)
    return out[:n].tobytes()
