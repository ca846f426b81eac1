"""Inputs of the inflate tests: the case list (streams made by the stdlib's
``zlib.compressobj`` and streams put together bit by bit), a bit writer, and a
plain bit-serial Python inflate walker that also takes a census of what a
stream contains.  The walker shares nothing with the product: it is a third
decoder beside the stdlib and csrc/mc_inflate.h, and the census pins what the
case list is there for (tests/test_inflate_host.py)."""

import ctypes
import gzip as _gzip
import io
import os
import struct
import zlib as _zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_DIR = os.path.join(ROOT, "tests", "native_inflate", "_build")
ZLIB, GZIP = 0, 1
CONTAINERS = {"zlib": ZLIB, "gzip": GZIP}


# ---- data --------------------------------------------------------------------
def smooth(n, seed=1):
    """A smooth byte series: a slow wave plus a little noise."""
    i = np.arange(n)
    rng = np.random.default_rng(seed)
    v = 128 + 90 * np.sin(i / 40.0) + 20 * np.sin(i / 7.0) + rng.integers(0, 3, n)
    return v.astype(np.uint8).tobytes()


def noise(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def runs(n, seed=3):
    rng = np.random.default_rng(seed)
    out = bytearray()
    while len(out) < n:
        out += bytes([int(rng.integers(0, 256))]) * int(rng.integers(1, 900))
    return bytes(out[:n])


def fibonacci_symbols():
    """121 392 bytes whose 24 symbols have Fibonacci counts, shuffled: a Huffman
    code of 15-bit codes (deeper trees are cut at 15 by zlib's length limiter)."""
    fib = [1, 1]
    while len(fib) < 24:
        fib.append(fib[-1] + fib[-2])
    data = np.concatenate([np.full(c, 40 + s, np.uint8) for s, c in enumerate(fib)])
    np.random.default_rng(5).shuffle(data)
    assert len(data) == 121392
    return data.tobytes()


# ---- containers --------------------------------------------------------------
def zlib_wrap(raw, data, cinfo=7):
    cmf = (cinfo << 4) | 8
    flg = 0x80
    flg += 31 - ((cmf << 8) | flg) % 31
    return bytes([cmf, flg]) + raw + struct.pack(">I", _zlib.adler32(data))


def gzip_wrap(raw, data, flags=0, extra=b""):
    return bytes([0x1F, 0x8B, 8, flags]) + bytes(4) + b"\x00\xff" + extra + raw + \
        struct.pack("<II", _zlib.crc32(data), len(data) & 0xFFFFFFFF)


def raw_deflate(data, level=6, wbits=15, strategy=_zlib.Z_DEFAULT_STRATEGY, flush_at=None):
    c = _zlib.compressobj(level, _zlib.DEFLATED, -wbits, 8, strategy)
    if flush_at is None:
        return c.compress(data) + c.flush()
    return c.compress(data[:flush_at]) + c.flush(_zlib.Z_FULL_FLUSH) + c.compress(data[flush_at:]) + c.flush()


# ---- the bit writer ------------------------------------------------------------
class BitWriter:
    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def bits(self, value, count):
        """`count` bits of `value`, lowest first (header fields, extra bits)."""
        self.acc |= (value & ((1 << count) - 1)) << self.n
        self.n += count
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, length):
        """A Huffman code, its first (most significant) bit first."""
        for k in range(length - 1, -1, -1):
            self.bits((code >> k) & 1, 1)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def bytes(self, data):
        assert self.n == 0
        self.out += data

    def done(self):
        self.align()
        return bytes(self.out)


def canonical(lengths):
    """{symbol: (code, length)} of the canonical code with these lengths (0 = unused)."""
    count = [0] * 16
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = {}
    for s, l in enumerate(lengths):
        if l:
            out[s] = (nxt[l], l)
            nxt[l] += 1
    return out


FIXED_LIT = canonical([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
FIXED_DIST = {d: (d, 5) for d in range(32)}
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
             6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def _len_symbol(length):
    i = 28 if length == 258 else max(k for k in range(28) if LEN_BASE[k] <= length)
    return 257 + i, length - LEN_BASE[i], LEN_EXTRA[i]


def _dist_symbol(dist):
    d = max(k for k in range(30) if DIST_BASE[k] <= dist)
    return d, dist - DIST_BASE[d], DIST_EXTRA[d]


def put_symbols(bw, lit, dist, items):
    """items: ints (literal / length symbols / 256 as they are) or ("m", length,
    distance) or ("raw", symbol) for a bare literal/length symbol, ("rawd", code)
    for a bare distance symbol."""
    for it in items:
        if isinstance(it, int):
            bw.code(*lit[it])
        elif it[0] == "m":
            s, x, xb = _len_symbol(it[1])
            bw.code(*lit[s])
            bw.bits(x, xb)
            d, x, xb = _dist_symbol(it[2])
            bw.code(*dist[d])
            bw.bits(x, xb)
        elif it[0] == "raw":
            bw.code(*lit[it[1]])
        elif it[0] == "rawd":
            bw.code(*dist[it[1]])
        elif it[0] == "bits":
            bw.bits(it[1], it[2])


def kraft_lengths(symbols, size):
    """A complete code over `symbols`: `size` lengths."""
    k = len(symbols)
    lens = [0] * size
    if k == 1:
        lens[symbols[0]] = 1
        return lens
    b = (k - 1).bit_length()
    short = (1 << b) - k
    for j, s in enumerate(sorted(symbols)):
        lens[s] = b - 1 if j < short else b
    return lens


def dynamic_header(bw, final, hlit, hdist, cl_ops, cl_lens=None, hclen=19):
    """BFINAL, BTYPE 2, the counts, the code-length code (a complete code over
    the symbols cl_ops uses, or `cl_lens`) and the ops: (symbol,) or (16|17|18, extra)."""
    bw.bits(final, 1)
    bw.bits(2, 2)
    bw.bits(hlit - 257, 5)
    bw.bits(hdist - 1, 5)
    bw.bits(hclen - 4, 4)
    if cl_lens is None:
        used = sorted({op[0] for op in cl_ops})
        if len(used) == 1:
            used.append(1 if used[0] != 1 else 2)  # the code-length code may not be incomplete
        cl_lens = kraft_lengths(used, 19)
    for s in CL_ORDER[:hclen]:
        bw.bits(cl_lens[s], 3)
    cl = canonical(cl_lens)
    for op in cl_ops:
        bw.code(*cl[op[0]])
        if op[0] >= 16:
            bw.bits(op[1], {16: 2, 17: 3, 18: 7}[op[0]])


def ops_for(lens):
    """Code-length ops for a list of lengths: zero runs as 17 / 18, the rest one by one."""
    ops, i = [], 0
    while i < len(lens):
        if lens[i] == 0:
            j = i
            while j < len(lens) and lens[j] == 0 and j - i < 138:
                j += 1
            run = j - i
            if run >= 11:
                ops.append((18, run - 11))
            elif run >= 3:
                ops.append((17, run - 3))
            else:
                ops.extend([(0,)] * run)
            i = j
        else:
            ops.append((lens[i],))
            i += 1
    return ops


def dynamic_block(final, lit_lens, dist_lens, items, cl_ops=None):
    bw = BitWriter()
    cl_ops = ops_for(list(lit_lens) + list(dist_lens)) if cl_ops is None else cl_ops
    dynamic_header(bw, final, len(lit_lens), len(dist_lens), cl_ops)
    put_symbols(bw, canonical(lit_lens), canonical(dist_lens), items)
    return bw


def fixed_block(items, final=1, bw=None):
    bw = bw or BitWriter()
    bw.bits(final, 1)
    bw.bits(1, 2)
    put_symbols(bw, FIXED_LIT, FIXED_DIST, items)
    return bw


def _lits(symbols, n=257):
    lens = [0] * n
    for s, l in symbols.items():
        lens[s] = l
    return lens


# ---- the hand-built streams ---------------------------------------------------
def handbuilt_valid():
    """(name, raw DEFLATE, the bytes it decodes to)."""
    out = []
    lits = noise(32768, 21)
    data = lits + lits[:258] + lits[257:258] * 3
    out.append(("far-32768", fixed_block(list(lits) + [("m", 258, 32768), ("m", 3, 1), 256]).done(), data))
    out.append(("dist-single-code",
                dynamic_block(1, _lits({97: 1, 256: 2, 257: 2}, 258), [1], [97, ("m", 3, 1), 256]).done(), b"aaaa"))
    out.append(("dist-empty", dynamic_block(1, _lits({97: 1, 98: 2, 256: 2}), [0], [97, 98, 98, 97, 256]).done(), b"abba"))
    # lengths: 97 -> 2, 256 -> 2, then ONE 16-repeat of 6 covers 257, 258 and the four distance lengths
    ops = [(18, 97 - 11), (2,), (18, 138 - 11), (18, 20 - 11), (2,), (16, 6 - 3)]
    out.append(("repeat-crosses-hlit",
                dynamic_block(1, _lits({97: 2, 256: 2, 257: 2, 258: 2}, 259), [2, 2, 2, 2],
                              [97, ("m", 3, 1), ("m", 4, 2), 97, ("m", 3, 4), 256], cl_ops=ops).done(),
                b"aaaa" + b"aaaa" + b"a" + b"aaa"))
    out.append(("only-eob", dynamic_block(1, _lits({256: 1}), [0], [256]).done(), b""))
    bw = BitWriter()
    bw.bits(0, 1), bw.bits(0, 2), bw.align(), bw.bytes(b"\x00\x00\xff\xff")
    out.append(("empty-stored-then-fixed", fixed_block(list(b"hello") + [256], bw=bw).done(), b"hello"))
    return out


def handbuilt_invalid_deflate():
    """(name, raw DEFLATE) with one fault each; padded so that the fault, not the
    end of the data, is what a decoder meets."""
    pad = bytes(8)
    out = []
    out.append(("dist-11-after-10", fixed_block(list(b"0123456789") + [("m", 3, 11), 256]).done()))
    out.append(("litlen-286", fixed_block([97, ("raw", 286), 256]).done() + pad))
    out.append(("dist-code-30", fixed_block([97, ("raw", 257), ("rawd", 30), 256]).done() + pad))
    out.append(("length-with-empty-dist",
                dynamic_block(1, _lits({97: 1, 256: 2, 257: 2}, 258), [0], [97, ("raw", 257), ("bits", 0, 8), 256]).done() + pad))
    bw = BitWriter()
    bw.bits(1, 1), bw.bits(0, 2), bw.align(), bw.bytes(b"\x05\x00\xfa\xfe" + b"hello")
    out.append(("stored-len-nlen", bw.done() + pad))
    bw = BitWriter()
    dynamic_header(bw, 1, 257, 1, [(16, 0), (0,)])
    out.append(("repeat-first", bw.done() + pad))
    bw = BitWriter()
    dynamic_header(bw, 1, 257, 1, [(18, 127), (18, 127)])
    out.append(("repeat-past-end", bw.done() + pad))
    out.append(("litlen-oversubscribed", dynamic_block(1, _lits({97: 1, 98: 1, 256: 1}), [1], [97, 256]).done() + pad))
    out.append(("litlen-incomplete", dynamic_block(1, _lits({97: 2, 256: 2}), [1], [97, 256]).done() + pad))
    out.append(("no-eob", dynamic_block(1, _lits({97: 1, 98: 1}), [1], [97, 98]).done() + pad))
    bw = BitWriter()
    bw.bits(1, 1), bw.bits(2, 2), bw.bits(30, 5), bw.bits(0, 5), bw.bits(15, 4)
    out.append(("hlit-287", bw.done() + pad * 4))
    bw = BitWriter()
    bw.bits(1, 1), bw.bits(3, 2)
    out.append(("btype-3", bw.done() + pad))
    bw = BitWriter()
    cl = [0] * 19
    cl[18] = 1
    dynamic_header(bw, 1, 257, 1, [], cl_lens=cl)
    out.append(("codelens-incomplete", bw.done() + pad * 4))
    return out


# ---- the case list ---------------------------------------------------------------
def _stdlib_streams():
    """(name, raw DEFLATE, data, zlib CINFO)."""
    out = []
    for n in (0, 1, 63, 64, 65, 257, 258, 259, 32767, 32768, 32769):
        d = smooth(n)
        out.append((f"smooth{n}", raw_deflate(d, 6), d, 7))
    d = smooth(70000)
    out.append(("stored70000", raw_deflate(d, 0), d, 7))
    out.append(("level1-70000", raw_deflate(d, 1), d, 7))
    out.append(("level9-70000", raw_deflate(d, 9), d, 7))
    out.append(("wbits9-70000", raw_deflate(d, 6, wbits=9), d, 1))
    d = smooth(5000, 2)
    out.append(("fixed5000", raw_deflate(d, 6, strategy=_zlib.Z_FIXED), d, 7))
    d = runs(60000)
    out.append(("rle-runs", raw_deflate(d, 6, strategy=_zlib.Z_RLE), d, 7))
    d = bytes(100000)
    out.append(("zeros100000", raw_deflate(d, 6), d, 7))
    d = noise(32500, 7) * 3
    out.append(("random-block-x3", raw_deflate(d, 9), d, 7))
    d = noise(70000, 8)
    out.append(("random70000", raw_deflate(d, 6), d, 7))
    d = fibonacci_symbols()
    out.append(("fibonacci", raw_deflate(d, 6, strategy=_zlib.Z_HUFFMAN_ONLY), d, 7))
    d = smooth(9000, 4)
    out.append(("full-flush", raw_deflate(d, 6, flush_at=4000), d, 7))
    return out


_CACHE = {}


def valid_cases():
    """[(name, container name, frame, data)]: every stream in both containers."""
    if "valid" not in _CACHE:
        out = []
        streams = _stdlib_streams() + [(n, r, d, 7) for n, r, d in handbuilt_valid()]
        for name, raw, data, cinfo in streams:
            out.append((name, "zlib", zlib_wrap(raw, data, cinfo), data))
            out.append((name, "gzip", gzip_wrap(raw, data), data))
        d = smooth(3000, 6)
        raw = raw_deflate(d)
        extra = struct.pack("<H", 5) + b"extra" + b"name.bin\x00" + b"a comment\x00"
        out.append(("gzip-fname-fextra-fcomment", "gzip", gzip_wrap(raw, d, flags=4 | 8 | 16, extra=extra), d))
        out.append(("gzip-zero-padding", "gzip", gzip_wrap(raw, d) + bytes(7), d))
        _CACHE["valid"] = out
    return _CACHE["valid"]


def invalid_cases():
    """[(name, container name, frame)], one fault each."""
    if "invalid" not in _CACHE:
        out = []
        for name, raw in handbuilt_invalid_deflate():
            out.append((name, "zlib", zlib_wrap(raw, b"")))
            out.append((name, "gzip", gzip_wrap(raw, b"")))
        d = smooth(3000, 6)
        raw = raw_deflate(d)
        z, g = zlib_wrap(raw, d), gzip_wrap(raw, d)
        flg = 0xA0 + 31 - ((0x78 << 8) | 0xA0) % 31
        out.append(("fdict", "zlib", bytes([0x78, flg]) + bytes(4) + z[2:]))
        out.append(("header-check", "zlib", bytes([z[0], z[1] ^ 1]) + z[2:]))
        out.append(("adler-flipped", "zlib", z[:-2] + bytes([z[-2] ^ 0x10]) + z[-1:]))
        out.append(("truncated-5", "zlib", z[:-5]))
        out.append(("gzip-magic", "gzip", b"\x1f\x8c" + g[2:]))
        out.append(("gzip-method", "gzip", g[:2] + b"\x07" + g[3:]))
        out.append(("gzip-crc-flipped", "gzip", g[:-7] + bytes([g[-7] ^ 0x10]) + g[-6:]))
        out.append(("gzip-isize-flipped", "gzip", g[:-3] + bytes([g[-3] ^ 0x10]) + g[-2:]))
        out.append(("gzip-truncated", "gzip", g[:-5]))
        out.append(("gzip-junk", "gzip", g + b"junk"))
        out.append(("gzip-two-members", "gzip", g + g))
        _CACHE["invalid"] = out
    return _CACHE["invalid"]


def corruption_frames(container="zlib", count=200, seed=11):
    """One 4 KiB level-6 frame and `count` seeded single-byte changes of it."""
    d = smooth(4096, 9)
    raw = raw_deflate(d, 6)
    frame = zlib_wrap(raw, d) if container == "zlib" else gzip_wrap(raw, d)
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        at = int(rng.integers(0, len(frame)))
        m = bytearray(frame)
        m[at] ^= int(rng.integers(1, 256))
        out.append(bytes(m))
    return frame, d, out


# ---- the stdlib, as the oracle -------------------------------------------------
def stdlib_decode(container, frame):
    """("ok", bytes) or ("error", exception class, text)."""
    try:
        if container == "zlib":
            return ("ok", _zlib.decompress(frame))
        with _gzip.GzipFile(fileobj=io.BytesIO(frame), mode="rb") as f:
            return ("ok", f.read())
    except (_zlib.error, _gzip.BadGzipFile, EOFError) as e:
        return ("error", type(e), str(e))


# ---- the host model (tests/native_inflate) ---------------------------------------
def hostlib():
    if "lib" not in _CACHE:
        lib = ctypes.CDLL(os.path.join(HOST_DIR, "libinflate_hostcheck.so"))
        lib.hi_inflate.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint, ctypes.c_void_p, ctypes.c_size_t,
                                   ctypes.POINTER(ctypes.c_uint64)]
        lib.hi_inflate.restype = ctypes.c_int
        lib.hi_inflate_tables_bytes.restype = ctypes.c_size_t
        lib.hi_inflate_record_bytes.restype = ctypes.c_size_t
        _CACHE["lib"] = lib
    return _CACHE["lib"]


def host_count(container, frame):
    """(code, bytes counted) of the model's count-only mode."""
    out = (ctypes.c_uint64 * 3)()
    rc = hostlib().hi_inflate(bytes(frame), len(frame), CONTAINERS[container], None, (1 << 30) - 1, out)
    return rc, int(out[0])


def host_decode(container, frame, cap=None):
    """(code, bytes, second word, consumed) of the model decoding into `cap`
    bytes (default: what the count-only mode counted)."""
    if cap is None:
        cap = host_count(container, frame)[1]
    buf = np.full(cap + 64, 0xA5, np.uint8)
    out = (ctypes.c_uint64 * 3)()
    rc = hostlib().hi_inflate(bytes(frame), len(frame), CONTAINERS[container], buf.ctypes.data, cap, out)
    assert (buf[cap:] == 0xA5).all(), "the model wrote past its capacity"
    return rc, buf[:int(out[0])].tobytes(), int(out[1]), int(out[2])


# ---- the walker -------------------------------------------------------------------
class _Bits:
    def __init__(self, data, pos):
        self.data, self.pos = data, 8 * pos

    def bit(self):
        if self.pos >= 8 * len(self.data):
            raise EOFError("walker: out of data")
        b = (self.data[self.pos >> 3] >> (self.pos & 7)) & 1
        self.pos += 1
        return b

    def bits(self, n):
        v = 0
        for k in range(n):
            v |= self.bit() << k
        return v


def _walk_code(br, table):
    code = 0
    for length in range(1, 16):
        code = (code << 1) | br.bit()
        s = table.get((length, code))
        if s is not None:
            return s, length
    raise ValueError("walker: no such code")


def _table(lengths):
    return {(l, c): s for s, (c, l) in canonical(lengths).items()}


def walk(raw, start=0):
    """Inflate the raw DEFLATE data at raw[start:] bit by bit: (bytes, census,
    the byte behind the data).  Census: block types met, the longest code used,
    the largest distance and length, matches whose distance is below their
    length, and 16/17/18 repeats that cross from the literal/length lengths
    into the distance lengths."""
    br = _Bits(raw, start)
    out = bytearray()
    census = {"types": set(), "blocks": 0, "max_code": 0, "max_dist": 0, "max_len": 0, "overlaps": 0, "crossing": 0}
    while True:
        final, btype = br.bit(), br.bits(2)
        census["types"].add(btype)
        census["blocks"] += 1
        if btype == 0:
            br.pos = (br.pos + 7) & ~7
            n, nn = br.bits(16), br.bits(16)
            assert n == nn ^ 0xFFFF
            at = br.pos >> 3
            out += raw[at:at + n]
            assert len(raw) >= at + n
            br.pos += 8 * n
        elif btype in (1, 2):
            if btype == 1:
                lit, dist = _table([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), _table([5] * 32)
            else:
                nlen, ndist, ncode = br.bits(5) + 257, br.bits(5) + 1, br.bits(4) + 4
                cl = [0] * 19
                for s in CL_ORDER[:ncode]:
                    cl[s] = br.bits(3)
                clt = _table(cl)
                lens = []
                while len(lens) < nlen + ndist:
                    s, _l = _walk_code(br, clt)
                    before = len(lens)
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        lens += [lens[-1]] * (3 + br.bits(2))
                    elif s == 17:
                        lens += [0] * (3 + br.bits(3))
                    else:
                        lens += [0] * (11 + br.bits(7))
                    if s >= 16 and before < nlen < len(lens):
                        census["crossing"] += 1
                assert len(lens) == nlen + ndist
                lit, dist = _table(lens[:nlen]), _table(lens[nlen:])
            while True:
                s, l = _walk_code(br, lit)
                census["max_code"] = max(census["max_code"], l)
                if s < 256:
                    out.append(s)
                elif s == 256:
                    break
                else:
                    i = s - 257
                    length = LEN_BASE[i] + br.bits(LEN_EXTRA[i])
                    d, l = _walk_code(br, dist)
                    census["max_code"] = max(census["max_code"], l)
                    distance = DIST_BASE[d] + br.bits(DIST_EXTRA[d])
                    assert distance <= len(out)
                    census["max_dist"] = max(census["max_dist"], distance)
                    census["max_len"] = max(census["max_len"], length)
                    census["overlaps"] += distance < length
                    for _ in range(length):
                        out.append(out[-distance])
        else:
            raise ValueError("walker: block type 3")
        if final:
            break
    return bytes(out), census, (br.pos + 7) >> 3


def data_offset(container, frame):
    """The first DEFLATE byte of a frame whose header is well formed."""
    if container == "zlib":
        return 2
    flags, p = frame[3], 10
    if flags & 4:
        p += 2 + struct.unpack_from("<H", frame, p)[0]
    for bit in (8, 16):
        if flags & bit:
            p = frame.index(0, p) + 1
    if flags & 2:
        p += 2
    return p


def fixture_frames(container):
    """[(array index, codec index, raw bytes, frame)] of the reference's fixtures."""
    from tests.helpers import fixture_cases
    out = []
    for arr, j, _cfg, enc in fixture_cases(container):
        raw = arr.tobytes(order="A")
        out.append((len(out), j, raw, enc))
    return out
