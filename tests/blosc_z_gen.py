"""Test-side generators for the Blosc zstd / zlib tests -- TEST
INFRASTRUCTURE ONLY.

* :func:`z_frame`: :func:`blosc_gen.blosc_frame` with another stream writer
  and the format bits of byte 2 rewritten (the header carries no checksum);
* :func:`build_cases`: the case list, made where libzstd loads
  (tests/golden/make_golden_blosc_z.py commits it as
  tests/golden/blosc_z_cases.npz + .json);
* :func:`load_cases`: the committed list, for the CPU and the GPU suite: the
  machines that run them need neither zlib nor libzstd;
* :func:`host_decode` / :func:`host_encode`: the host build of the product's
  walker and scalar decoders, and of its scalar zstd encoder with the Blosc
  layout helpers (tests/native_blosc_z);
* :func:`encode_cases`: the ``cname='zstd'`` encode list of the two suites.

The expected code of a malformed case is written down here from the rule it
breaks (csrc/mc_zstd.h, csrc/mc_inflate.h, csrc/mc_blosc_z.h), not taken from
a decoder.
"""

import ctypes
import json
import os
import struct
import zlib

import numpy as np

from tests import blosc_gen as bg
from tests import inflate_gen as ig
from tests import zstd_gen as zg

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "blosc_z_cases")
FIXTURE_BLOSC = os.path.join(HERE, "golden", "reference_fixture", "blosc")
HOSTCHECK_DIR = os.path.join(HERE, "native_blosc_z", "_build")

FMT_LZ4, FMT_ZLIB, FMT_ZSTD = 1, 3, 4
FORMATS = {"zlib": FMT_ZLIB, "zstd": FMT_ZSTD}
CONTAINER = 64  # MC_BLOSC_Z_CONTAINER: added to an mc_lz4_error of a zstd / zlib frame's container
NOSHUFFLE, SHUFFLE, BITSHUFFLE = bg.NOSHUFFLE, bg.SHUFFLE, bg.BITSHUFFLE


def z_frame(data, fmt, compress, typesize=1, blocksize=None, shuffle=NOSHUFFLE, **kw):
    """A Blosc1 frame of `data` whose streams `compress` writes, with format
    bits `fmt`.  zstd frames always carry the do-not-split bit, as c-blosc's."""
    if fmt == FMT_ZSTD:
        kw["nosplit"] = True
    frame = bytearray(bg.blosc_frame(data, typesize, blocksize, shuffle, compress=compress, **kw))
    frame[2] = (frame[2] & 0x1F) | (fmt << 5)
    return bytes(frame)


def zlib_stream(part):
    return zlib.compress(part, 1)


# ---------------------------------------------------------------------------
# the case list (needs libzstd: run by tests/golden/make_golden_blosc_z.py)
# ---------------------------------------------------------------------------
def build_cases(lib):
    """[(name, format name, frame, array bytes, code, bad stream)]: code 0 for
    a frame that decodes to the array bytes, else the error record's code
    with the stream it names."""
    cases = []

    def zstd_stream(part, **kw):
        kw.setdefault("level", 1)
        return lib.compress(part, **kw)

    writers = {"zlib": zlib_stream, "zstd": zstd_stream}

    def add(name, fname, data, ts, bs, shuffle=NOSHUFFLE, code=0, bad=0, compress=None, **kw):
        frame = z_frame(data, FORMATS[fname], compress or writers[fname], ts, bs, shuffle, **kw)
        cases.append((f"{fname}-{name}", fname, frame, bytes(data), code, bad))
        return frame

    # ---- both formats: the frame shapes ----
    for fname in ("zlib", "zstd"):
        for ts in (1, 3, 4, 8, 17):
            bs = 4096 // ts * ts
            n = 2 * bs + 5 * ts + 1
            add(f"ts{ts}", fname, bg._payload(n, n + ts), ts, bs, SHUFFLE if ts > 1 else BITSHUFFLE)
        add("short-last", fname, bg._payload(4096 + 100, 1), 4, 4096, SHUFFLE)
        add("last-below-typesize", fname, bg._payload(4096 + 3, 2), 8, 4096, SHUFFLE)
        add("raw-stream", fname, bg._payload(4096 * 3, 3), 4, 4096, SHUFFLE,
            raw_streams=(5,) if fname == "zlib" else (1,))
        add("nbytes0", fname, b"", 4, 4096, SHUFFLE)
        add("nbytes1", fname, b"\x5a", 4, 4096, SHUFFLE)
        add("incompressible", fname, zg.noise(8192, 7), 4, 4096, SHUFFLE)  # every stream stored raw
        add("memcpyed", fname, bg._payload(5000, 4), 4, 4096, NOSHUFFLE, memcpyed=True)

    # ---- zstd ----
    sine = zg.sine_f32(320 * 1024, 10, 0.001)
    add("block320k", "zstd", sine, 4, None, NOSHUFFLE)  # three 128 KiB-limit blocks in one frame
    head = zg.noise(4096, 11)
    far = head + zg.quads(100 * 1024, 12) + head + zg.quads(192 * 1024 - 100 * 1024 - 8192, 13)
    add("far-repeat192k", "zstd", far, 1, None, NOSHUFFLE, compress=lambda p: zstd_stream(p, level=19))
    for n in (65535, 65536, 65537):
        add(f"stream{n}", "zstd", zg.mixed(n + 100, n), 1, n, NOSHUFFLE)
    usize = 3000
    rle = bytes([7]) * usize
    add("rle-block", "zstd", rle, 1, None, streams={0: zg.frame_header(usize) + zg.block(1, rle[:1], True, usize)})
    raw = bg._payload(usize, 5)  # (a raw block makes the stream longer than its share: a reader takes it all the same)
    add("raw-block", "zstd", raw, 1, None, streams={0: zg.frame_header(usize) + zg.block(0, raw, True)})
    add("checksum", "zstd", bg._payload(4096 * 2 + 300, 6), 4, 4096, SHUFFLE,
        compress=lambda p: zstd_stream(p, checksum=1))
    add("no-content-size", "zstd", bg._payload(4096 * 2 + 300, 7), 4, 4096, SHUFFLE,
        compress=lambda p: zstd_stream(p, content_size=0))

    # ---- zlib ----
    add("split8", "zlib", bg._payload(8000 * 2 + 24, 8), 8, 8000, SHUFFLE)  # 8 streams per full block
    add("stream96k", "zlib", zg.mixed(96 * 1024, 9), 1, None, NOSHUFFLE,
        compress=lambda p: zlib.compress(p, 6))  # wraps the 32 KiB ring

    def three_kinds(p):  # a stored, a fixed and a dynamic block in one stream
        a, b = len(p) // 3, 2 * len(p) // 3
        c0 = zlib.compressobj(0, zlib.DEFLATED, -15)
        c1 = zlib.compressobj(6, zlib.DEFLATED, -15, 8, zlib.Z_FIXED)
        raw_ = c0.compress(p[:a]) + c0.flush(zlib.Z_FULL_FLUSH) + c1.compress(p[a:b]) + c1.flush(zlib.Z_FULL_FLUSH) + \
            ig.raw_deflate(p[b:], 6)
        return ig.zlib_wrap(raw_, p)

    add("stored-fixed-dynamic", "zlib", zg.mixed(9000, 10) + bytes(3000), 1, None, NOSHUFFLE, compress=three_kinds)

    # ---- malformed: one stream of a good frame replaced ----
    zdata = bg._payload(4096 * 2 + 300, 20)
    zfilt = bg.oblosc.blosc_filter(zdata, 4, 4096, SHUFFLE, True)
    part = zfilt[4096:8192]  # stream 1 of 3
    good = zstd_stream(part)
    window = 0x10  # Window_Descriptor: 4 KiB

    def zbad(name, stream, code):
        add(name, "zstd", zdata, 4, 4096, SHUFFLE, code=code, bad=1, streams={1: stream})

    zbad("bad-cut-short", good[:-3], zg.E_HEADER)                      # the last block leaves the stream
    zbad("bad-magic", bytes([good[0] ^ 1]) + good[1:], zg.E_HEADER)
    zbad("bad-dictionary-id", zg.frame_header(len(part), dict_id=5) + zg.block(0, part, True), zg.E_DICT)
    zbad("bad-content-size", zg.frame_header(len(part) - 1) + zg.block(0, part[:-1], True), zg.E_SIZE)
    zbad("bad-fewer-bytes", zg.frame_header(None, window=window) + zg.block(0, part[:-5], True), zg.E_SIZE)
    zbad("bad-more-bytes", zg.frame_header(None, window=window + 8) + zg.block(0, part + part[:5], True),
         zg.E_CAPACITY)
    summed = zstd_stream(part, checksum=1)
    zbad("bad-checksum", summed[:-1] + bytes([summed[-1] ^ 0xFF]), zg.E_CHECK)
    zbad("bad-second-frame", good + good, zg.E_MEMBER)

    lfilt = zfilt[4096 + 1024:4096 + 2048]  # stream 5 of 9: the second byte plane of block 1
    lgood = zlib_stream(lfilt)

    def lbad(name, stream, code):
        add(name, "zlib", zdata, 4, 4096, SHUFFLE, code=code, bad=5, streams={5: stream})

    lbad("bad-adler", lgood[:-1] + bytes([lgood[-1] ^ 1]), 21)  # MC_INF_E_CHECK
    lbad("bad-truncated", lgood[:-6], 8)                        # MC_INF_E_TRUNCATED
    return cases


def save_cases(cases):
    arrays, meta = {}, []
    for k, (name, fname, frame, data, code, bad) in enumerate(cases):
        arrays[f"frame_{k}"] = np.frombuffer(frame, np.uint8)
        arrays[f"data_{k}"] = np.frombuffer(data, np.uint8)
        meta.append({"name": name, "format": fname, "code": code, "bad_stream": bad})
    np.savez_compressed(GOLDEN + ".npz", **arrays)
    with open(GOLDEN + ".json", "w") as f:
        json.dump({"cases": meta}, f, indent=1)


_cases = None


def load_cases():
    """[(name, format name, frame, array bytes, code, bad stream)] as committed."""
    global _cases
    if _cases is None:
        with open(GOLDEN + ".json") as f:
            meta = json.load(f)["cases"]
        with np.load(GOLDEN + ".npz") as z:
            _cases = [(m["name"], m["format"], z[f"frame_{k}"].tobytes(), z[f"data_{k}"].tobytes(), m["code"],
                       m["bad_stream"]) for k, m in enumerate(meta)]
    return _cases


def valid_cases():
    return [c for c in load_cases() if c[4] == 0]


def malformed_cases():
    return [c for c in load_cases() if c[4] != 0]


# ---------------------------------------------------------------------------
# the reference's fixture frames
# ---------------------------------------------------------------------------
def fixture_frames(codec):
    """[(index, frame, array bytes)] of tests/golden/reference_fixture/blosc/codec.NN."""
    out = []
    d = os.path.join(FIXTURE_BLOSC, "codec.%02d" % codec)
    for j in range(13):
        arr = np.load(os.path.join(FIXTURE_BLOSC, "array.%02d.npy" % j), allow_pickle=False)
        with open(os.path.join(d, "encoded.%02d.dat" % j), "rb") as f:
            out.append((j, f.read(), arr.tobytes(order="A")))
    return out


# ---------------------------------------------------------------------------
# the product's walker + scalar decoders on the host (tests/native_blosc_z)
# ---------------------------------------------------------------------------
HCZ_REJECTED, HCZ_UNSUPPORTED = -1, -2
_hostlib = None


def hostlib():
    global _hostlib
    if _hostlib is None:
        path = os.path.join(HOSTCHECK_DIR, "libblosc_z_hostcheck.so")
        assert os.path.exists(path), "build with __graft_entry__.build() (make -C tests/native_blosc_z)"
        lib = ctypes.CDLL(path)
        lib.hcz_blosc_decode.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t,
                                         ctypes.c_void_p]
        lib.hcz_record_bytes.restype = ctypes.c_size_t
        _hostlib = lib
    return _hostlib


INFO = ("flags", "typesize", "blocksize", "nbytes", "nstreams", "bad_stream", "raw_streams", "format")


def host_decode(frame):
    """(status, still-filtered bytes or None, info) from the host model: status
    0, -1 rejected by the header checks, -2 unsupported compressor, > 0 the
    error record's code."""
    frame = bytes(frame)
    nbytes = struct.unpack("<I", frame[4:8])[0] if len(frame) >= 16 else 0
    cap = min(nbytes, 1 << 24)
    out = np.full(cap + 64, 0xA5, np.uint8)  # 64 guard bytes behind the output
    info = np.zeros(len(INFO), np.int32)
    rc = hostlib().hcz_blosc_decode(frame, len(frame), out.ctypes.data, cap, info.ctypes.data)
    assert (out[cap:] == 0xA5).all(), "the host decoder wrote behind its output"
    return rc, (out[:cap].tobytes() if rc == 0 else None), dict(zip(INFO, info.tolist()))


def host_array_bytes(frame):
    """The frame's array bytes through the host model and the oracle's inverse filter."""
    rc, filtered, info = host_decode(frame)
    assert rc == 0, (rc, info)
    return bg.unfilter(filtered, info["flags"], info["typesize"], info["blocksize"])


# ---------------------------------------------------------------------------
# encode, cname='zstd': the host model and the cases the CPU and GPU suites share
# ---------------------------------------------------------------------------
def streams_of(frame):
    """[(stream bytes, share)] of a compressed frame, by the container's rules."""
    flags, ts = frame[2], frame[3]
    nbytes, bs = struct.unpack("<II", frame[4:12])
    out = []
    for b in range(-(-nbytes // bs)):
        bsize = min(bs, nbytes - b * bs)
        ns = bg.split_streams(flags, ts, bs, bsize)
        p = struct.unpack("<i", frame[16 + 4 * b:20 + 4 * b])[0]
        for _ in range(ns):
            cb = struct.unpack("<i", frame[p:p + 4])[0]
            out.append((frame[p + 4:p + 4 + cb], bsize // ns))
            p += 4 + cb
    return out


def host_encode(data, itemsize=1, clevel=5, shuffle=SHUFFLE, blocksize=0):
    """The Blosc zstd frame of `data` by the host model: the package's frame
    parameters (numcodecs_amd.blosc._frame_params), the oracle's filter, then
    tests/native_blosc_z's scalar encoder and layout."""
    from numcodecs_amd import blosc

    raw = bytes(np.ascontiguousarray(np.frombuffer(memoryview(data), np.uint8)))
    flags, bs, ts, mode = blosc._frame_params(len(raw), itemsize, clevel, shuffle, blocksize, FMT_ZSTD)
    if not raw:
        return bytes([2, 1, flags, ts]) + struct.pack("<III", 0, bs, 16)
    filtered = bg.oblosc.blosc_filter(raw, ts, bs, mode, True) if mode != NOSHUFFLE else raw
    lib = hostlib()
    lib.hcz_blosc_encode.restype = ctypes.c_long
    lib.hcz_blosc_encode.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                     ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t]
    out = np.full(len(raw) + 16 + 64, 0xA5, np.uint8)
    cb = lib.hcz_blosc_encode(filtered, raw, len(raw), ts, bs, flags, out.ctypes.data, len(raw) + 16)
    assert cb >= 16, cb
    assert (out[len(raw) + 16:] == 0xA5).all(), "the host encoder wrote behind its slot"
    return out[:cb].tobytes()


def ramp_f32(n):
    return (np.arange(n, dtype=np.float32) * 0.25 + 3.0)


def encode_cases():
    """[(name, array, keywords of compress(), compressible)]: `compressible`
    cases must come out with no raw stream and below half their input."""
    noise = np.frombuffer(zg.noise(4096, 31), np.uint8)
    comp = np.tile(np.arange(64, dtype=np.uint8), 64)

    def pay(n, seed):
        """n compressible single bytes: the byte planes of a float32 ramp (bg._payload
        stays above half its size under this encoder: confirmed on the CPU)."""
        r = (ramp_f32(n // 4 + 1) + seed).tobytes()
        return np.frombuffer(bg.oblosc.blosc_filter(r, 4, len(r), SHUFFLE, True), np.uint8)[:n].copy()

    return [
        ("blocks4096", pay(4096 * 3 + 100, 40), dict(clevel=5, shuffle=NOSHUFFLE, blocksize=4096), True),
        ("blocks65536", pay(65536 * 2 + 1000, 41), dict(clevel=5, shuffle=NOSHUFFLE, blocksize=65536), True),
        ("blocks65537", pay(65537 * 2 + 1000, 42), dict(clevel=5, shuffle=NOSHUFFLE, blocksize=65537), True),
        ("blocks3x65536+5", pay((3 * 65536 + 5) + 5000, 43), dict(clevel=5, shuffle=NOSHUFFLE, blocksize=3 * 65536 + 5),
         True),
        ("ramp-shuffle", ramp_f32(96 * 1024), dict(clevel=5, shuffle=SHUFFLE), True),
        ("ramp-bitshuffle", ramp_f32(96 * 1024), dict(clevel=9, shuffle=BITSHUFFLE), True),
        ("raw-between", np.concatenate([comp, noise, comp]), dict(clevel=5, shuffle=NOSHUFFLE, blocksize=4096), False),
        ("all-noise", np.frombuffer(zg.noise(3 * 4096 + 7, 33), np.uint8), dict(clevel=5, shuffle=SHUFFLE, blocksize=4096),
         False),
        ("clevel0", ramp_f32(5000), dict(clevel=0, shuffle=SHUFFLE), False),
        ("nbytes0", np.zeros(0, np.float32), dict(clevel=5, shuffle=SHUFFLE), False),
        ("nbytes1", np.full(1, 0x5A, np.uint8), dict(clevel=5, shuffle=SHUFFLE), False),
    ]
