"""Test-side helpers for the Blosc encode tests -- TEST INFRASTRUCTURE ONLY.

* the host build of the product's scalar LZ4 encoder and frame layout
  (tests/native_lz4enc) through ctypes: :func:`encode_stream`,
  :func:`host_frame` (the exact model of the GPU encoder);
* the input streams and frame cases the CPU and the GPU suites share.
"""

import ctypes
import os

import numpy as np

from numcodecs_amd import blosc
from oracle import blosc as oblosc
from tests import blosc_gen as gen

ENC_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native_lz4enc", "_build")
GUARD = 64
_enclib = None


def enclib():
    global _enclib
    if _enclib is None:
        path = os.path.join(ENC_DIR, "libblosc_enc_hostcheck.so")
        assert os.path.exists(path), "build with __graft_entry__.build() (make -C tests/native_lz4enc)"
        lib = ctypes.CDLL(path)
        lib.he_lz4_encode_stream.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t]
        lib.he_lz4_encode_stream.restype = ctypes.c_size_t
        lib.he_blosc_encode.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_size_t,
                                        ctypes.c_size_t, ctypes.c_uint, ctypes.c_void_p, ctypes.c_size_t]
        lib.he_blosc_encode.restype = ctypes.c_long
        _enclib = lib
    return _enclib


def encode_stream(data: bytes):
    """The scalar encoder's output for `data` with cap = len(data): the LZ4
    block, or None when the stream is to be stored raw.  The output buffer is
    followed by guard bytes, which must survive."""
    data = bytes(data)
    n = len(data)
    out = np.full(n + GUARD, 0xA5, np.uint8)
    cs = enclib().he_lz4_encode_stream(data, n, out.ctypes.data, n)
    assert (out[n:] == 0xA5).all(), "the scalar encoder wrote at or past dst + cap"
    if cs == 0:
        return None
    assert cs < n, (cs, n)
    return out[:cs].tobytes()


def resolve_shuffle(shuffle, itemsize):
    if shuffle == blosc.AUTOSHUFFLE:
        return blosc.BITSHUFFLE if itemsize == 1 else blosc.SHUFFLE
    return shuffle


def host_frame(data: bytes, itemsize=1, clevel=5, shuffle=blosc.SHUFFLE, blocksize=blosc.AUTOBLOCKS) -> bytes:
    """The frame the product writes for `data`, by the host build of its
    encoder: the product's own frame parameters, the oracle's filters, the
    shared scalar encoder and layout code."""
    data = bytes(data)
    n = len(data)
    flags, bs, ts, mode = blosc._frame_params(n, itemsize, clevel, resolve_shuffle(shuffle, itemsize), blocksize)
    if n == 0:
        return blosc._header_bytes(flags, ts, 0, bs, 16)
    filtered = oblosc.blosc_filter(data, ts, bs, mode, True) if mode else data
    out = np.full(n + 16 + GUARD, 0xA5, np.uint8)
    cb = enclib().he_blosc_encode(filtered, data, n, ts, bs, flags, out.ctypes.data, n + 16)
    assert (out[n + 16:] == 0xA5).all(), "the host frame encoder wrote past its slot"
    assert 16 < cb <= n + 16, cb
    return out[:cb].tobytes()


# ---------------------------------------------------------------------------
# C1: single streams
# ---------------------------------------------------------------------------
def _rand(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def stream_cases():
    """(name, bytes): the streams of the issue's list."""
    cases = []
    for n in (0, 1, 4, 12, 13, 14, 63, 64, 65, 75, 76, 77, 127, 128, 129, 4096, 70000):
        cases.append((f"payload{n}", gen._payload(n, 1000 + n)))
    cases.append(("zeros140000", bytes(140000)))
    cases.append(("random5000", _rand(5000, 11)))
    far = _rand(66000, 12)
    cases.append(("distance65535", far + far[66000 - 65535:66000 - 65535 + 3000]))
    cases.append(("distance65536", far + far[66000 - 65536:66000 - 65536 + 3000]))
    # (4096 table entries do not remember 66000 random positions: those two end
    # up stored raw.  With zeros in between the far copy is found -- or not.)
    head = _rand(3000, 14)
    cases.append(("findable65535", head + bytes(65535 - 3000) + head + _rand(16, 15)))
    cases.append(("findable65536", head + bytes(65536 - 3000) + head + _rand(16, 15)))
    rep = _rand(64, 13)
    for ll in (14, 15, 16, 269, 270, 271):  # literal runs between repeats of `rep`
        cases.append((f"literals{ll}", rep + _rand(ll, 20 + ll) + rep + _rand(ll, 40 + ll) + rep + _rand(16, 5)))
    for ml in (18, 19, 20, 273, 274, 275):  # a repeat of exactly ml bytes
        a = _rand(ml, 60 + ml)
        cases.append((f"match{ml}", _rand(40, 61) + a + _rand(30, 62) + a + _rand(20, 63)))
    return cases


def parse_block(block: bytes, n: int):
    """Walk an LZ4 block that decodes to n bytes: [(literal length, offset,
    match length)] with offset None for the last sequence.  Asserts the block
    format's rules: offsets 1..65535 within the produced bytes, the last
    sequence literals only with at least 5 of them, no match starting in the
    last 12 bytes nor reaching into the last 5."""
    seqs, i, produced = [], 0, 0
    while True:
        tok = block[i]
        i += 1
        lit = tok >> 4
        if lit == 15:
            while True:
                b = block[i]
                i += 1
                lit += b
                if b != 255:
                    break
        i += lit
        produced += lit
        if i == len(block):
            seqs.append((lit, None, 0))
            assert (tok & 15) == 0
            break
        assert i + 2 <= len(block)
        off = block[i] | (block[i + 1] << 8)
        i += 2
        ml = tok & 15
        if ml == 15:
            while True:
                b = block[i]
                i += 1
                ml += b
                if b != 255:
                    break
        ml += 4
        assert 1 <= off <= 65535 and off <= produced, (off, produced)
        assert produced <= n - 12, "a match starts in the last 12 bytes"
        produced += ml
        assert produced <= n - 5, "a match reaches into the last 5 bytes"
        seqs.append((lit, off, ml))
    assert produced == n
    assert seqs[-1][0] >= 5
    return seqs


# ---------------------------------------------------------------------------
# C2: the eleven input kinds of the size comparison (64 KiB streams)
# ---------------------------------------------------------------------------
def size_cases():
    """The float32 signals are tools/probe_blosc_*.py's (N(0,1) and its
    cumulative sum / 64), cut to 64 Ki elements so that a byte plane is 64 KiB."""
    rng = np.random.default_rng(0)
    n = 65536
    noise = rng.standard_normal(n).astype("<f4")
    smooth = np.cumsum(noise / 64).astype("<f4")
    ints = (np.cumsum(rng.integers(-20, 21, n)) + 100000).astype("<i4")
    words = [b"block", b"stream", b"shuffle", b"frame", b"wave", b"lane", b"offset", b"literal", b"match", b"the",
             b"of", b"and", b"a", b"codec", b"chunk"]
    text = b" ".join(words[k] for k in rng.integers(0, len(words), 20000))[:n]
    planes = lambda a: np.frombuffer(a.tobytes(), np.uint8).reshape(n, 4).T  # noqa: E731
    cases = [("payload64k", gen._payload(n, 5))]
    cases += [(f"smooth-f4-plane{k}", planes(smooth)[k].tobytes()) for k in range(4)]
    cases.append(("noise-f4-plane3", planes(noise)[3].tobytes()))
    cases += [(f"i4-plane{k}", planes(ints)[k].tobytes()) for k in (0, 1)]
    cases += [("zeros64k", bytes(n)), ("text64k", text), ("payload300", gen._payload(300, 6))]
    assert len(cases) == 11
    return cases


# ---------------------------------------------------------------------------
# C3: frames
# ---------------------------------------------------------------------------
# the distinct lz4 configs of the reference's fixture set: (clevel, shuffle, blocksize)
LZ4_CONFIGS = [(5, 1, 0), (0, 1, 0), (1, 0, 0), (9, 2, 0), (5, 1, 256), (1, 0, 256)]


def shape_params():
    """(name, data, itemsize, shuffle, blocksize, clevel): the parameter list of
    blosc_gen.shape_cases() replayed through the encoder (typesizes 1, 2, 3,
    4, 8, 16, 17; split and unsplit; short last block; last block below
    typesize; 13-element bitshuffle block; incompressible; nbytes 0 and 1)."""
    out = []

    def add(name, n, ts, bs, shuffle=gen.NOSHUFFLE, seed=0, clevel=5):
        # byte j of the elements is a slowly varying signal of its own, so that
        # the shuffled streams compress (a plain payload would not: memcpyed)
        # (16 levels: short streams still get smaller)
        base, e = (np.frombuffer(gen._payload(n, seed + n + ts), np.uint8) >> 4).tobytes(), n // ts
        data = np.frombuffer(base, np.uint8)[:e * ts].reshape(ts, e).T.tobytes() + base[e * ts:] if shuffle else base
        out.append((name, data, ts, shuffle, bs, clevel))

    for ts in (1, 2, 3, 4, 8, 16, 17):
        bs = 4096 // ts * ts
        add(f"ts{ts}-split-shuffle", 3 * bs + 5 * ts + 1, ts, bs, gen.SHUFFLE)
        add(f"ts{ts}-unsplit", 2 * 96 * ts + 7, ts, 96 * ts if 96 * ts >= 128 else 128, gen.NOSHUFFLE)
        add(f"ts{ts}-bitshuffle", 2 * bs + 8 * ts, ts, bs, gen.BITSHUFFLE)
    add("bs256", 256 * 5 + 100, 2, 256, gen.SHUFFLE)
    add("bs255x3-ts3", 765 * 3 + 200, 3, 765, gen.SHUFFLE)
    add("bs255-ts3", 255 * 4 + 11, 3, 256, gen.BITSHUFFLE)  # forced 256 -> 255: 85 elements, copied
    add("bs4096-exact", 4096 * 3, 4, 4096, gen.SHUFFLE)
    add("bs64k", 65536 * 2 + 1000, 4, 65536, gen.SHUFFLE)
    add("bs64k-ts1", 65536 + 3000, 1, 65536, gen.BITSHUFFLE)
    add("auto-256k", 262144 + 4 * 77, 4, 0, gen.SHUFFLE)  # automatic blocksize: one block, four 64 KiB streams
    add("short-last", 4096 + 100, 4, 4096, gen.SHUFFLE)
    add("last-below-typesize", 4096 + 3, 8, 4096, gen.SHUFFLE)
    add("bitshuffle-odd-elements", 4096 + 4 * 13, 4, 4096, gen.BITSHUFFLE)  # last block: 13 elements
    add("memcpyed-clevel0", 5000, 4, 4096, gen.SHUFFLE, clevel=0)
    add("nbytes0", 0, 4, 4096, gen.SHUFFLE)
    add("nbytes1", 1, 4, 4096, gen.SHUFFLE)
    out.append(("incompressible", _rand(8192, 7), 4, gen.SHUFFLE, 4096, 5))  # every stream raw: memcpyed
    return out
