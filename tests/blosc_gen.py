"""Test-side generators for the Blosc decode tests -- TEST INFRASTRUCTURE ONLY.

* :func:`lz4_compress`: a small greedy hash-table LZ4 block compressor;
* :func:`assemble`: an LZ4 block from hand-specified (literals, offset, match
  length) sequences, with the bytes it must decode to;
* :func:`blosc_frame`: a Blosc1 frame writer with controls for typesize,
  blocksize, shuffle mode, the do-not-split bit, forced raw-stored streams and
  hand-made streams.

Written from the published LZ4 block format and the frame rules restated in
oracle/blosc.py; everything it writes is checked against that oracle's walker
(tests/test_blosc_host.py).
"""

import struct

import numpy as np

from oracle import blosc as oblosc

NOSHUFFLE, SHUFFLE, BITSHUFFLE = 0, 1, 2


def _length_bytes(extra: int) -> bytes:
    """The extension bytes of a length whose 4-bit field is 15: `extra` = length - 15."""
    return b"\xff" * (extra // 255) + bytes([extra % 255])


def sequence(literals: bytes, offset=None, match_len=None) -> bytes:
    """One LZ4 sequence; offset None: the last one (literals only)."""
    lit = len(literals)
    ml = 0 if offset is None else match_len - 4
    assert ml >= 0
    tok = (min(lit, 15) << 4) | min(ml, 15)
    out = bytes([tok])
    if lit >= 15:
        out += _length_bytes(lit - 15)
    out += bytes(literals)
    if offset is not None:
        out += struct.pack("<H", offset)
        if ml >= 15:
            out += _length_bytes(ml - 15)
    return out


def assemble(seqs):
    """(stream, decoded) of a list of (literals, offset, match_len) sequences;
    a sequence with offset None ends the stream with its literals."""
    stream, out = b"", bytearray()
    for lits, off, ml in seqs:
        stream += sequence(lits, off, ml)
        out += lits
        if off is not None:
            st = len(out) - off
            assert 0 <= st
            for k in range(ml):
                out.append(out[st + k])
    return stream, bytes(out)


def lz4_compress(data: bytes) -> bytes:
    """Greedy LZ4 block compressor: a dict of the last position of every
    4-byte word, matches extended forward, the block's last 5 bytes literals
    and no match starting in its last 12 bytes (the format's end conditions)."""
    data = bytes(data)
    n = len(data)
    out = bytearray()
    table = {}
    i = anchor = 0
    last_start, match_end = n - 12, n - 5
    while i < last_start:
        key = data[i:i + 4]
        cand = table.get(key)
        table[key] = i
        if cand is None or i - cand > 65535:
            i += 1
            continue
        ml = 4
        while i + ml < match_end and data[cand + ml] == data[i + ml]:
            ml += 1
        out += sequence(data[anchor:i], i - cand, ml)
        i += ml
        anchor = i
    out += sequence(data[anchor:])
    return bytes(out)


def split_streams(flags: int, typesize: int, blocksize: int, bsize: int) -> int:
    split = not (flags & oblosc.BLOSC_NOSPLIT) and bsize == blocksize and typesize <= 16 and bsize // typesize >= 128
    return typesize if split else 1


def blosc_frame(data, typesize=1, blocksize=None, shuffle=NOSHUFFLE, nosplit=False, raw_streams=(),
                memcpyed=False, streams=None, compress=lz4_compress, version=2):
    """A Blosc1 LZ4 frame of `data`.

    blocksize None: one block.  raw_streams: indices (counted over the whole
    frame) of streams to store raw whatever they compress to.  streams: a dict
    {stream index: compressed bytes} of hand-made LZ4 blocks used instead of
    compressing (their decoded size is the caller's business: that is how
    malformed frames are made).  A stream that does not get smaller is stored
    raw, as c-blosc does (cbytes == size means raw)."""
    raw = bytes(np.ascontiguousarray(np.frombuffer(memoryview(data), np.uint8)))
    nbytes = len(raw)
    if blocksize is None:
        blocksize = max(nbytes, 1)
    flags = oblosc.LZ4_FORMAT << 5
    if shuffle == SHUFFLE:
        flags |= oblosc.BLOSC_DOSHUFFLE
    elif shuffle == BITSHUFFLE:
        flags |= oblosc.BLOSC_DOBITSHUFFLE
    if nosplit:
        flags |= oblosc.BLOSC_NOSPLIT
    if memcpyed:
        flags |= oblosc.BLOSC_MEMCPYED
        body = raw
        return bytes([version, 1, flags, typesize]) + struct.pack("<III", nbytes, blocksize, 16 + nbytes) + body
    filtered = oblosc.blosc_filter(raw, typesize, blocksize, shuffle, True) if shuffle and nbytes else raw
    nblocks = (nbytes + blocksize - 1) // blocksize
    starts, body, sidx = [], b"", 0
    pos = 16 + 4 * nblocks
    for b in range(nblocks):
        blk = filtered[b * blocksize:(b + 1) * blocksize]
        ns = split_streams(flags, typesize, blocksize, len(blk))
        assert len(blk) % ns == 0, "a split block must be a multiple of the typesize"
        neb = len(blk) // ns
        starts.append(pos + len(body))
        for j in range(ns):
            part = blk[j * neb:(j + 1) * neb]
            if streams is not None and sidx in streams:
                comp = streams[sidx]
            elif sidx in raw_streams:
                comp = part
            else:
                comp = compress(part)
                if len(comp) >= neb:
                    comp = part
            body += struct.pack("<i", len(comp)) + comp
            sidx += 1
    table = struct.pack(f"<{nblocks}i", *starts)
    cbytes = 16 + len(table) + len(body)
    return bytes([version, 1, flags, typesize]) + struct.pack("<III", nbytes, blocksize, cbytes) + table + body


def stream_frame(stream: bytes, usize: int) -> bytes:
    """A one-block, one-stream frame around a hand-made LZ4 block that is
    meant to decode to `usize` bytes (typesize 1, no shuffle)."""
    assert len(stream) != usize, "cbytes == size would mean stored raw"
    return blosc_frame(bytes(usize), typesize=1, nosplit=True, streams={0: stream})


# ---------------------------------------------------------------------------
# the product's shared plan walker + scalar decoder on the host (tests/native_lz4)
# ---------------------------------------------------------------------------
import ctypes  # noqa: E402
import os  # noqa: E402

HOSTCHECK_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native_lz4", "_build")
HC_REJECTED, HC_UNSUPPORTED = -1, -2
_hostlib = None


def hostlib():
    global _hostlib
    if _hostlib is None:
        path = os.path.join(HOSTCHECK_DIR, "libblosc_hostcheck.so")
        assert os.path.exists(path), "build with __graft_entry__.build() (make -C tests/native_lz4)"
        lib = ctypes.CDLL(path)
        lib.hc_blosc_decode.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t,
                                        ctypes.c_void_p]
        lib.hc_lz4_decode_stream.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t]
        _hostlib = lib
    return _hostlib


def host_decode(frame: bytes):
    """(status, still-filtered bytes or None, info) from the host build of the
    product's walker and decoder: status 0, -1 rejected by the header checks,
    -2 unsupported compressor, > 0 an mc_lz4_error."""
    frame = bytes(frame)
    nbytes = struct.unpack("<I", frame[4:8])[0] if len(frame) >= 16 else 0
    cap = min(nbytes, 1 << 24)
    out = np.full(cap + 64, 0xA5, np.uint8)  # 64 guard bytes behind the output
    info = np.zeros(6, np.int32)
    rc = hostlib().hc_blosc_decode(frame, len(frame), out.ctypes.data, cap, info.ctypes.data)
    assert (out[cap:] == 0xA5).all(), "the host decoder wrote behind its output"
    return rc, (out[:cap].tobytes() if rc == 0 else None), dict(zip(
        ("flags", "typesize", "blocksize", "nbytes", "nstreams", "bad_stream"), info.tolist()))


def unfilter(filtered: bytes, flags: int, typesize: int, blocksize: int) -> bytes:
    """Invert the frame's shuffle with the oracle's per-block filters."""
    if flags & oblosc.BLOSC_MEMCPYED or not filtered:
        return filtered
    if flags & oblosc.BLOSC_DOBITSHUFFLE:
        return oblosc.blosc_filter(filtered, typesize, blocksize, BITSHUFFLE, False)
    if flags & oblosc.BLOSC_DOSHUFFLE and typesize > 1:
        return oblosc.blosc_filter(filtered, typesize, blocksize, SHUFFLE, False)
    return filtered


def oracle_decode(frame: bytes) -> bytes:
    """The frame's array bytes by the oracle's walker and filters alone."""
    flags, ts, bs, blocks = oblosc.frame_filtered_blocks(frame)
    if blocks is None:
        nbytes = struct.unpack("<I", frame[4:8])[0]
        return bytes(frame[16:16 + nbytes])
    return unfilter(b"".join(blocks), flags, ts, bs)


# ---------------------------------------------------------------------------
# the cases the CPU and the GPU suites share
# ---------------------------------------------------------------------------
def _payload(n: int, seed: int) -> bytes:
    """n compressible bytes: a slowly varying signal with repeats and noise."""
    rng = np.random.default_rng(seed)
    base = (np.cumsum(rng.integers(-2, 3, n)) & 0xFF).astype(np.uint8)
    base[rng.integers(0, max(n, 1), n // 16)] = rng.integers(0, 256, n // 16).astype(np.uint8)
    if n > 64:
        base[n // 2:n // 2 + n // 8] = base[:n // 8]  # a long repeat
    return base.tobytes()


def shape_cases():
    """(name, data, frame): the frame shapes of the issue's list."""
    cases = []

    def add(name, n, ts, bs, shuffle=NOSHUFFLE, seed=0, **kw):
        data = _payload(n, seed + n + ts)
        cases.append((name, data, blosc_frame(data, ts, bs, shuffle, **kw)))

    for ts in (1, 2, 3, 4, 8, 16, 17):
        bs = 4096 // ts * ts
        add(f"ts{ts}-split-shuffle", 3 * bs + 5 * ts + 1, ts, bs, SHUFFLE)
        add(f"ts{ts}-nosplit", 2 * bs + 7, ts, bs, NOSHUFFLE, nosplit=True)
        add(f"ts{ts}-bitshuffle", 2 * bs + 8 * ts, ts, bs, BITSHUFFLE)
    add("bs256", 256 * 5 + 100, 2, 256, SHUFFLE)
    add("bs255x3-ts3", 765 * 3 + 200, 3, 765, SHUFFLE)
    add("bs255-ts3", 255 * 4 + 11, 3, 255, BITSHUFFLE)  # 85 elements: no multiple of 8, copied
    add("bs4096-exact", 4096 * 3, 4, 4096, SHUFFLE)
    add("bs64k", 65536 * 2 + 1000, 4, 65536, SHUFFLE)
    add("bs64k-ts1", 65536 + 3000, 1, 65536, BITSHUFFLE)
    add("short-last", 4096 + 100, 4, 4096, SHUFFLE)
    add("last-below-typesize", 4096 + 3, 8, 4096, SHUFFLE)
    add("bitshuffle-odd-elements", 4096 + 4 * 13, 4, 4096, BITSHUFFLE)  # last block: 13 elements
    add("raw-stream", 4096 * 2, 4, 4096, SHUFFLE, raw_streams=(5,))
    add("memcpyed", 5000, 4, 4096, NOSHUFFLE, memcpyed=True)
    add("nbytes0", 0, 4, 4096, SHUFFLE)
    add("nbytes1", 1, 4, 4096, SHUFFLE)
    rnd = np.random.default_rng(7).integers(0, 256, 8192, dtype=np.uint8).tobytes()
    cases.append(("incompressible", rnd, blosc_frame(rnd, 4, 4096, SHUFFLE)))  # every stream stored raw
    return cases


def _abc(n: int, start: int = 0) -> bytes:
    return bytes((start + 7 * k) % 251 for k in range(n))


def sequence_cases():
    """(name, frame, decoded): hand-assembled LZ4 blocks."""
    cases = []

    def add(name, seqs):
        stream, out = assemble(seqs)
        cases.append((name, stream_frame(stream, len(out)), out))

    tail = (b"12345", None, None)
    for off in (1, 2, 3, 4, 7, 8, 63, 64, 65, 255, 256):
        add(f"offset{off}", [(_abc(max(off, 4)), off, 200), (_abc(9, 3), off, 70), tail])
    add("offset65535", [(_abc(65535 + 40), 65535, 300), (_abc(3, 9), 65535, 66000), tail])
    # the match starts inside the literals the preceding sequence just wrote
    # (sequence 3's offset 110 reaches over its 70 literals and sequence 2's 30 match bytes)
    add("match-in-previous-literals", [(_abc(300), 5, 4), (_abc(20, 50), 12, 30), (_abc(70, 9), 110, 140), tail])
    for ml in (4, 18, 19, 19 + 255, 19 + 2 * 255 + 7):
        add(f"matchlen{ml}", [(_abc(100), 37, ml), (b"", 100, ml), (b"", 50, 8), tail])
    for ll in (0, 14, 15, 15 + 255, 15 + 255 + 3):
        add(f"litlen{ll}", [(_abc(40), 40, 10), (_abc(ll, 5), 9, 6), tail])
    add("literals-only", [(_abc(777), None, None)])
    add("zero-literal-end", [(_abc(33), 20, 50), (b"", None, None)])
    add("long-rle-wraps-history", [(b"\x07", 1, 140000), (_abc(5), 3, 70000), tail])
    return cases


def malformed_cases():
    """(name, frame): frames every decoder must reject."""
    data = _payload(4096 * 2 + 300, 3)
    good = blosc_frame(data, 4, 4096, SHUFFLE)
    cases = []

    def patch(frame, at, word):
        return frame[:at] + struct.pack("<I", word) + frame[at + 4:]

    cut = good[:-3]
    cases.append(("truncated-last-stream", patch(cut, 12, len(cut))))
    first = struct.unpack("<i", good[16:20])[0]
    cases.append(("cbytes-word-past-frame", patch(good, first, len(good))))
    cases.append(("bstarts-outside-frame", patch(good, 20, len(good) + 100)))

    def hand(name, stream, usize):
        cases.append((name, stream_frame(stream, usize)))

    hand("offset-zero", sequence(_abc(8), 0, 8) + sequence(b"12345"), 21)
    hand("offset-beyond-produced", sequence(_abc(4), 5, 8) + sequence(b"12345"), 17)
    hand("match-overruns-destination", sequence(_abc(8), 4, 100) + sequence(b"12345"), 50)
    hand("literals-overrun-source", bytes([0xE0]) + b"abcde", 14)
    hand("literals-overrun-destination", sequence(_abc(40)), 20)
    hand("stream-ends-short", assemble([(_abc(20), 10, 20), (b"12345", None, None)])[0], 64)
    cases.append(("header-cbytes-mismatch", patch(good, 12, len(good) + 1)))
    cases.append(("version-not-2", bytes([1]) + good[1:]))
    return cases
