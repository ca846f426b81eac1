"""Inputs of the zstd tests: the data formulas, the case list (frames made by
libzstd through ``ctypes`` and frames put together by hand), a pure-Python
XXH64, and a header walker that reads the frame header, the block headers and
the literals- and sequences-section headers of a frame (no entropy decoding)
and takes a census of what it contains.  The walker shares nothing with the
product, and the census pins what the case list is there for
(tests/test_zstd_host.py).

The frames live in tests/golden/zstd_cases*.npz + zstd_cases.json, written by
tests/golden/make_golden_zstd.py where libzstd is at hand; the data a frame
decodes to is never stored, it comes from the formulas here and is pinned by
its SHA-256 in the json."""

import ctypes
import hashlib
import json
import os
import struct

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_DIR = os.path.join(ROOT, "tests", "native_zstd", "_build")
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURE = os.path.join(GOLDEN, "reference_fixture", "zstd")
NPZ_PARTS = ("zstd_cases.npz", "zstd_cases_2.npz", "zstd_cases_3.npz")
MAGIC = 0xFD2FB528

# csrc/mc_zstd.h mc_zstd_error
E_HEADER, E_EMPTY, E_DICT, E_MEMBER, E_CORRUPT, E_SRCSIZE, E_CAPACITY, E_CHECK, E_SIZE, E_TABLE = range(1, 11)


# ---- data ----------------------------------------------------------------------
def words(seed, n):
    """n 64-bit words of a splitmix64 sequence: the same on every numpy."""
    with np.errstate(over="ignore"):
        z = (np.arange(1, n + 1, dtype=np.uint64) + np.uint64(seed) * np.uint64(0x632BE59BD9B4E019)) \
            * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def noise(n, seed):
    return words(seed, (n + 7) // 8).view(np.uint8)[:n].tobytes()


def quads(n, seed):
    """n bytes in 0..3."""
    return (np.frombuffer(noise(n, seed), np.uint8) & 3).tobytes()


def mixed(n, seed, gap=8):
    """Letters from a skewed alphabet of 41 with short copies of earlier bytes
    between them: Huffman literals and enough sequences for FSE-coded tables."""
    a = np.frombuffer(noise(4 * n + 8, seed), np.uint8).astype(np.int64)
    v = (97 + ((a[:n] & a[n:2 * n]) % 41)).astype(np.uint8)
    out = bytearray(v[:64].tobytes())
    k = 64
    while len(out) < n:
        lit = 3 + int(a[2 * n + k]) % gap
        out += v[k:k + lit].tobytes()
        ln = 4 + int(a[3 * n + k]) % 6
        back = 1 + (int(a[2 * n + k + 1]) * 7 + int(a[3 * n + k + 1])) % (len(out) - ln)
        st = len(out) - back - ln
        if st >= 0:
            out += out[st:st + ln]
        k += lit
    return bytes(out[:n])


def sine_f32(nbytes, keep, step):
    """float32 samples of a sine kept to `keep` mantissa bits."""
    i = np.arange(nbytes // 4, dtype=np.float64)
    mask = np.uint32((0xFFFFFFFF << (23 - keep)) & 0xFFFFFFFF)
    return (np.sin(i * step).astype(np.float32).view(np.uint32) & mask).tobytes()


def far_repeat():
    head = noise(4096, 11)
    return head + quads(1 << 20, 12) + head


def triples():
    """40 000 records of (one of 64 fixed triples, one random byte)."""
    table = np.frombuffer(noise(64 * 3, 13), np.uint8).reshape(64, 3)
    r = np.frombuffer(noise(80000, 14), np.uint8)
    rec = np.empty((40000, 4), np.uint8)
    rec[:, :3] = table[r[:40000] & 63]
    rec[:, 3] = r[40000:]
    return rec.tobytes()


LENGTHS = (1, 63, 64, 65, 255, 256, 257, 65535, 65536, 65537, 131071, 131072, 131073)


def lib_specs():
    """(name, data maker, libzstd parameters) of the frames libzstd makes."""
    specs = [
        ("rle_blocks", lambda: bytes(300000), dict(level=3)),
        ("raw_two_blocks", lambda: noise(200000, 2), dict(level=3)),
        ("sine_treeless", lambda: sine_f32(1200000, 10, 0.001), dict(level=1, checksum=1)),
        ("sine_treeless_nosize", lambda: sine_f32(1200000, 10, 0.001), dict(level=1, content_size=0)),
        ("sine_zero_sequences", lambda: sine_f32(120000, 23, 0.001), dict(level=1)),
        ("repeat_far", far_repeat, dict(level=19)),
        ("repeat_mode", lambda: mixed(60000, 50), dict(level=7, window_log=10)),
        ("seq_count_3_bytes", triples, dict(level=19)),
        ("blocks_293", lambda: quads(300000, 3), dict(level=3, window_log=10)),
        ("one_stream_direct", lambda: quads(5000, 4), dict(level=3)),
        ("negative_1", lambda: mixed(70000, 5), dict(level=-1, checksum=1)),
        ("negative_50", lambda: mixed(70000, 6, 30), dict(level=-50)),
        ("level_9_checksum", lambda: mixed(3000, 7), dict(level=9, checksum=1)),
        ("small_checksum", lambda: mixed(1100, 9), dict(level=3, checksum=1)),
        ("small_plain", lambda: mixed(1100, 8), dict(level=3)),
        ("small_nosize", lambda: mixed(1100, 8), dict(level=3, content_size=0)),
    ]
    for k, n in enumerate(LENGTHS):
        specs.append(("len_%d" % n, (lambda n=n, k=k: mixed(n, 20 + k) if n > 64 else noise(n, 20 + k)), dict(level=3, checksum=k & 1)))
    return specs


# ---- XXH64 -----------------------------------------------------------------------
_M = (1 << 64) - 1
_P1, _P2, _P3, _P4, _P5 = (0x9E3779B185EBCA87, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9, 0x85EBCA77C2B2AE63,
                           0x27D4EB2F165667C5)


def _rotl(x, r):
    return ((x << r) | (x >> (64 - r))) & _M


def _round(acc, v):
    return (_rotl((acc + v * _P2) & _M, 31) * _P1) & _M


def xxh64(data):
    """XXH64 with seed 0, by the book (hand-built frames are short)."""
    n, i = len(data), 0
    if n >= 32:
        acc = [(_P1 + _P2) & _M, _P2, 0, (-_P1) & _M]
        while n - i >= 32:
            for k in range(4):
                acc[k] = _round(acc[k], int.from_bytes(data[i + 8 * k:i + 8 * k + 8], "little"))
            i += 32
        h = (_rotl(acc[0], 1) + _rotl(acc[1], 7) + _rotl(acc[2], 12) + _rotl(acc[3], 18)) & _M
        for k in range(4):
            h = ((h ^ _round(0, acc[k])) * _P1 + _P4) & _M
    else:
        h = _P5
    h = (h + n) & _M
    while n - i >= 8:
        h = (_rotl(h ^ _round(0, int.from_bytes(data[i:i + 8], "little")), 27) * _P1 + _P4) & _M
        i += 8
    if n - i >= 4:
        h = (_rotl(h ^ (int.from_bytes(data[i:i + 4], "little") * _P1 & _M), 23) * _P2 + _P3) & _M
        i += 4
    while i < n:
        h = (_rotl(h ^ (data[i] * _P5 & _M), 11) * _P1) & _M
        i += 1
    h ^= h >> 33
    h = (h * _P2) & _M
    h ^= h >> 29
    h = (h * _P3) & _M
    return h ^ (h >> 32)


# ---- frames by hand -----------------------------------------------------------------
def frame_header(content=None, content_bytes=None, window=None, checksum=False, dict_id=None, reserved=0):
    """window: the Window_Descriptor byte, None for a single segment."""
    single = window is None
    if content is None:
        flag, fcs = 0, b""
        assert not single
    else:
        nb = content_bytes or (1 if content < 256 and single else 2 if 256 <= content < 65792 else 4 if content < 1 << 32 else 8)
        flag = {1: 0, 2: 1, 4: 2, 8: 3}[nb]
        fcs = (content - 256 if nb == 2 else content).to_bytes(nb, "little")
    did = b"" if dict_id is None else struct.pack("<I", dict_id)
    fhd = (flag << 6) | (single << 5) | reserved | (bool(checksum) << 2) | (3 if did else 0)
    return struct.pack("<IB", MAGIC, fhd) + (b"" if single else bytes([window])) + did + fcs


def block(kind, payload, last=False, size=None):
    """kind 0 raw, 1 RLE (payload one byte, `size` the run), 2 compressed, 3 reserved."""
    size = len(payload) if size is None else size
    return ((size << 3) | (kind << 1) | bool(last)).to_bytes(3, "little") + payload


def raw_literals(data, size_format):
    n = len(data)
    if size_format in (0, 2):  # one format: Size_Format's second bit is the size's lowest
        assert n < 32 and (n & 1) == size_format >> 1
        return bytes([n << 3]) + data
    if size_format == 1:
        assert n < 4096
        return ((n << 4) | 4).to_bytes(2, "little") + data
    return ((n << 4) | 12).to_bytes(3, "little") + data


def rle_literals(byte, n):
    return ((n << 4) | 4 | 1).to_bytes(2, "little") + bytes([byte])


def rle_sequence(ll_code, of_code, ml_code, of_bits):
    """A sequences section of one sequence with all three tables in RLE mode: the
    states take no bits, the stream holds the offset's extra bits below the
    final-bit marker (ll_code < 16 and ml_code < 32 take none)."""
    assert ll_code < 16 and ml_code < 32 and of_code < 8
    return bytes([1, 0x54, ll_code, of_code, ml_code, (1 << of_code) | of_bits])


def with_checksum(frame, data):
    return frame + struct.pack("<I", xxh64(data) & 0xFFFFFFFF)


def hand_cases():
    """(name, frame, data) of the valid frames that need no entropy coder."""
    out = []
    lit = bytes(range(65, 65 + 26))
    for sf in range(4):
        data = lit[:20 + sf // 2] if sf in (0, 2) else lit * (3 if sf == 1 else 200)
        body = block(2, raw_literals(data, sf) + b"\x00", last=True)
        out.append(("hand_raw_literals_sf%d" % sf, frame_header(len(data)) + body, data))
    out.append(("hand_rle_literals", frame_header(1000) + block(2, rle_literals(0x5A, 1000) + b"\x00", last=True),
                b"\x5a" * 1000))
    out.append(("hand_rle_block", with_checksum(frame_header(70000, checksum=True) + block(1, b"\x07", True, 70000),
                                                b"\x07" * 70000), b"\x07" * 70000))
    data = noise(1500, 30)
    # Window_Descriptor 0x0B: exponent 1, mantissa 3: 2 KiB + 3 * 256
    out.append(("hand_window_mantissa", frame_header(None, window=0x0B) + block(0, data[:700]) + block(0, data[700:], True),
                data))
    out.append(("hand_fcs_8_bytes", frame_header(300, content_bytes=8) + block(0, data[:300], True), data[:300]))
    # literals "abcd", then a match of 3 at offset 2 (offset code 2: Offset_Value 4 + 1, minus 3)
    seq = raw_literals(b"abcd", 0) + rle_sequence(4, 2, 0, 1)
    out.append(("hand_rle_mode_sequence", frame_header(7) + block(2, seq, True), b"abcdcdc"))
    return out


# ---- libzstd through ctypes ----------------------------------------------------------
class Lib:
    """libzstd, where it loads (no headers, no binding: the few calls by hand)."""

    def __init__(self):
        z = ctypes.CDLL("libzstd.so.1")
        sz, vp = ctypes.c_size_t, ctypes.c_void_p
        for name, res, args in (
            ("ZSTD_createCCtx", vp, []), ("ZSTD_freeCCtx", sz, [vp]),
            ("ZSTD_CCtx_setParameter", sz, [vp, ctypes.c_int, ctypes.c_int]),
            ("ZSTD_compress2", sz, [vp, vp, sz, vp, sz]), ("ZSTD_compressBound", sz, [sz]),
            ("ZSTD_decompress", sz, [vp, sz, vp, sz]), ("ZSTD_isError", ctypes.c_uint, [sz]),
            ("ZSTD_getErrorName", ctypes.c_char_p, [sz]), ("ZSTD_versionNumber", ctypes.c_uint, []),
            ("ZSTD_findFrameCompressedSize", sz, [vp, sz]),
            ("ZSTD_getFrameContentSize", ctypes.c_ulonglong, [vp, sz]),
        ):
            f = getattr(z, name)
            f.restype, f.argtypes = res, args
        self.z = z
        v = z.ZSTD_versionNumber()
        self.version = "%d.%d.%d" % (v // 10000, v // 100 % 100, v % 100)

    def compress(self, data, level=3, checksum=0, content_size=1, window_log=0):
        z = self.z
        c = z.ZSTD_createCCtx()
        try:
            for param, value in ((100, level), (201, checksum), (200, content_size), (101, window_log)):
                r = z.ZSTD_CCtx_setParameter(c, param, value)
                assert not z.ZSTD_isError(r), z.ZSTD_getErrorName(r)
            cap = z.ZSTD_compressBound(len(data))
            dst = ctypes.create_string_buffer(cap)
            r = z.ZSTD_compress2(c, dst, cap, data, len(data))
            assert not z.ZSTD_isError(r), z.ZSTD_getErrorName(r)
            return dst.raw[:r]
        finally:
            z.ZSTD_freeCCtx(c)

    def decompress(self, frame, cap):
        """(bytes, None) or (None, libzstd's error name)."""
        dst = ctypes.create_string_buffer(max(cap, 1))
        r = self.z.ZSTD_decompress(dst, cap, frame, len(frame))
        if self.z.ZSTD_isError(r):
            return None, self.z.ZSTD_getErrorName(r).decode()
        return dst.raw[:r], None

    def verdict(self, frame, cap=None):
        """What the reference's decompress() comes to for this frame: its frame
        walk (ZSTD_findFrameCompressedSize, ZSTD_getFrameContentSize over every
        frame in the buffer), then ZSTD_decompress into the declared size (`cap`
        where none is declared).  {'stage': 'walk' | 'empty' | 'decompress' |
        'count' | 'ok', 'error': libzstd's error name or None, 'size': bytes}
        ('count': libzstd accepted, with another size than `cap`)."""
        z, off, total, unknown = self.z, 0, 0, False
        while off < len(frame):
            rest = frame[off:]
            r = z.ZSTD_findFrameCompressedSize(rest, len(rest))
            if z.ZSTD_isError(r):
                return {"stage": "walk", "error": z.ZSTD_getErrorName(r).decode(), "size": 0}
            c = z.ZSTD_getFrameContentSize(rest, r)
            if c == (1 << 64) - 2:
                return {"stage": "empty", "error": None, "size": 0}
            if c == (1 << 64) - 1:
                unknown = True
                break
            total += c
            off += r
        if not unknown and total == 0:
            return {"stage": "empty", "error": None, "size": 0}
        want = cap if unknown else total
        got, err = self.decompress(frame, want)
        if err:
            return {"stage": "decompress", "error": err, "size": 0}
        self.last = got  # the bytes of an accepted frame
        if len(got) != want:
            return {"stage": "count", "error": None, "size": len(got)}
        return {"stage": "ok", "error": None, "size": len(got)}


def load_lib():
    try:
        return Lib()
    except (OSError, AttributeError):
        return None


# ---- the header walker -----------------------------------------------------------------
def walk(frame):
    """The census of one frame: header fields, and per block its type, sizes, the
    literals-section header and the sequences-section header.  Raises
    ValueError on what it cannot read.  `cuts`: every structural boundary."""
    f = bytes(frame)
    if len(f) < 5 or struct.unpack_from("<I", f)[0] != MAGIC:
        raise ValueError("magic")
    fhd = f[4]
    flag, single, checksum, did_flag = fhd >> 6, (fhd >> 5) & 1, (fhd >> 2) & 1, fhd & 3
    if fhd & 8:
        raise ValueError("reserved")
    p, cuts = 5, [4, 5]
    c = {"single": single, "checksum": checksum, "window_descriptor": None, "window": None, "dict_id": 0}
    if not single:
        c["window_descriptor"] = f[p]
        base = 1 << (10 + (f[p] >> 3))
        c["window"] = base + (base >> 3) * (f[p] & 7)
        p += 1
    nd = (0, 1, 2, 4)[did_flag]
    c["dict_id"] = int.from_bytes(f[p:p + nd], "little")
    p += nd
    nb = (single, 2, 4, 8)[flag]
    c["fcs_bytes"] = nb
    c["content"] = None
    if nb:
        c["content"] = int.from_bytes(f[p:p + nb], "little") + (256 if nb == 2 else 0)
        p += nb
    if single:
        c["window"] = c["content"]
    cuts.append(p)
    blocks = []
    while True:
        if len(f) - p < 3:
            raise ValueError("block header")
        bh = int.from_bytes(f[p:p + 3], "little")
        last, kind, size = bh & 1, (bh >> 1) & 3, bh >> 3
        p += 3
        cuts.append(p)
        b = {"type": kind, "size": size, "last": last}
        held = 1 if kind == 1 else size
        if kind == 3 or len(f) - p < held:
            raise ValueError("block")
        if kind == 2:
            q = p
            lt, sf = f[q] & 3, (f[q] >> 2) & 3
            b["lit_type"], b["lit_sf"] = lt, sf
            if lt < 2:
                lh = 2 if sf == 1 else 3 if sf == 3 else 1
                regen = f[q] >> 3 if lh == 1 else int.from_bytes(f[q:q + lh], "little") >> 4
                comp = regen if lt == 0 else 1
                b["streams"] = 0
            else:
                lh = 3 if sf < 2 else sf + 2
                v = int.from_bytes(f[q:q + lh], "little") >> 4
                bits = (10, 10, 14, 18)[sf]
                regen, comp = v & ((1 << bits) - 1), v >> bits
                b["streams"] = 1 if sf == 0 else 4
                if lt == 2:
                    b["weights"] = "direct" if f[q + lh] >= 128 else "fse"
            b["regen"], b["lit_comp"] = regen, comp
            cuts.append(q + lh)
            q += lh + comp
            cuts.append(q)
            n0 = f[q]
            if n0 < 128:
                nseq, nsb = n0, 1
            elif n0 < 255:
                nseq, nsb = ((n0 - 128) << 8) + f[q + 1], 2
            else:
                nseq, nsb = f[q + 1] + (f[q + 2] << 8) + 0x7F00, 3
            b["nseq"], b["nseq_bytes"] = nseq, nsb
            q += nsb
            if nseq:
                b["modes"] = (f[q] >> 6, (f[q] >> 4) & 3, (f[q] >> 2) & 3)
                q += 1
            cuts.append(q)
        blocks.append(b)
        p += held
        cuts.append(p)
        if last:
            break
    if checksum:
        p += 4
        cuts += [p - 2, p]
    if p > len(f):
        raise ValueError("checksum")
    c["blocks"], c["end"], c["cuts"] = blocks, p, sorted(set(x for x in cuts if x <= len(f)))
    return c


# ---- the stored case list ---------------------------------------------------------------
_store = None


def _load():
    global _store
    if _store is None:
        with open(os.path.join(GOLDEN, "zstd_cases.json")) as fh:
            meta = json.load(fh)
        arrays = {}
        for part in NPZ_PARTS:
            fn = os.path.join(GOLDEN, part)
            if os.path.exists(fn):
                with np.load(fn) as z:
                    arrays.update({k: z[k].tobytes() for k in z.files})
        _store = (meta, arrays)
    return _store


def data_of(name):
    """The bytes valid case `name` decodes to, from its formula."""
    for n, make, _ in lib_specs():
        if n == name:
            return make()
    for n, _, data in hand_cases():
        if n == name:
            return data
    raise KeyError(name)


def valid_cases():
    """[(name, frame, sha256 of the data, its size)] in the stored order."""
    meta, arrays = _load()
    return [(c["name"], arrays["valid__" + c["name"]], c["sha256"], c["size"]) for c in meta["valid"]]


def invalid_cases():
    """[(name, frame, meta)]: meta['expect'] = the mc_zstd_error name the rules
    give, meta['verdict'] = what the reference comes to with libzstd (Lib.verdict)."""
    meta, arrays = _load()
    return [(c["name"], arrays["invalid__" + c["name"]], c) for c in meta["invalid"]]


def mutation_record(kind):
    """The recorded libzstd verdicts of the bounded corruption of frame `kind`
    ('checksummed' / 'plain'): (frame, [(what, position, ok, sha256 or error)])."""
    meta, arrays = _load()
    m = meta["mutations"][kind]
    frame = arrays["valid__" + m["frame"]]
    ok, err = (np.frombuffer(arrays["mut__%s__%s" % (kind, k)], np.uint8) for k in ("ok", "err"))
    shas = arrays["mut__%s__sha" % kind]
    lens = np.frombuffer(arrays["mut__%s__len" % kind], "<u4")
    verdicts, k = [], 0
    for i, (what, at, _m) in enumerate(mutations(frame)):
        if ok[i]:
            verdicts.append((what, at, 1, shas[8 * k:8 * k + 8].hex() + ":%d" % lens[k]))
            k += 1
        else:
            verdicts.append((what, at, 0, m["errors"][err[i]]))
    assert len(verdicts) == len(ok) and k == len(lens)
    return frame, m["frame"], verdicts


def mutations(frame):
    """Every single-byte XOR with 0x01 and 0x80, and every truncation."""
    for at in range(len(frame)):
        for x in (0x01, 0x80):
            m = bytearray(frame)
            m[at] ^= x
            yield ("xor%02x" % x, at, bytes(m))
    for cut in range(len(frame)):
        yield ("cut", cut, frame[:cut])


def sha(data):
    return hashlib.sha256(data).hexdigest()


def build_invalid(valid):
    """(name, frame, expected mc_zstd_error name, note) from the valid frames
    {name: frame}: pure byte surgery."""
    out = []
    base = valid["small_checksum"]
    c = walk(base)
    for cut in c["cuts"]:
        if cut < len(base):
            out.append(("cut_%d" % cut, base[:cut], "E_HEADER", "truncated at a structural boundary"))
    out.append(("cut_last_byte", base[:-1], "E_HEADER", "truncated inside the checksum"))
    out.append(("bad_magic", b"\x29" + base[1:], "E_HEADER", ""))
    m = bytearray(base)
    m[4] |= 8
    out.append(("reserved_bit", bytes(m), "E_HEADER", ""))
    data = noise(600, 31)
    out.append(("block_type_3", frame_header(600) + block(3, data, True), "E_HEADER", ""))
    big = noise(131073, 32)
    out.append(("raw_block_over_128k", frame_header(len(big)) + block(0, big, True), "E_CORRUPT",
                "Block_Maximum_Size (RFC 8878 3.1.1.2.4); libzstd's one-shot call does not look"))
    out.append(("rle_block_over_window", frame_header(None, window=0x00) + block(1, b"\x01", True, 1025), "E_CORRUPT",
                "Block_Maximum_Size = the window of 1 KiB; libzstd's one-shot call does not look"))
    out.append(("dictionary_id", frame_header(600, dict_id=7) + block(0, data, True), "E_DICT", ""))
    out.append(("content_size_0", frame_header(0) + block(0, b"", True), "E_EMPTY", ""))
    out.append(("declared_larger", frame_header(601) + block(0, data, True), "E_SIZE", ""))
    out.append(("declared_smaller", frame_header(599) + block(0, data, True), "E_CAPACITY", ""))
    m = bytearray(base)
    m[-1] ^= 0x10
    out.append(("flipped_checksum", bytes(m), "E_CHECK", ""))
    # literals "abcd", then a match at offset 32 + 0 - 3 = 29 with 4 bytes out
    seq = raw_literals(b"abcd", 0) + rle_sequence(4, 5, 0, 0)
    out.append(("offset_beyond_output", frame_header(7) + block(2, seq, True), "E_CORRUPT", ""))
    out.append(("skippable_first", struct.pack("<II", 0x184D2A53, 4) + b"skip" + valid["small_plain"], "E_MEMBER",
                "the reference would skip it"))
    out.append(("two_frames", valid["small_plain"] + valid["small_checksum"], "E_MEMBER",
                "the reference would concatenate"))
    out.append(("junk_after", valid["small_plain"] + b"\x00\x01\x02", "E_HEADER", ""))
    out.append(("junk_after_long", base + b"junkjunkjunk", "E_HEADER", ""))
    return out


# ---- the host model (tests/native_zstd) ---------------------------------------------------
_hostlib = None


def hostlib():
    global _hostlib
    if _hostlib is None:
        h = ctypes.CDLL(os.path.join(HOST_DIR, "libzstd_hostcheck.so"))
        vp, sz = ctypes.c_void_p, ctypes.c_size_t
        h.hz_decode.argtypes = [vp, sz, vp, sz, vp]
        h.hz_open.argtypes = [vp, sz, vp]
        h.hz_xxh64.argtypes = [vp, sz]
        h.hz_xxh64.restype = ctypes.c_uint64
        h.hz_tables_bytes.restype = h.hz_record_bytes.restype = sz
        _hostlib = h
    return _hostlib


def host_count(frame):
    """(code, bytes counted) of the model's count-only mode."""
    out = (ctypes.c_uint64 * 2)()
    rc = hostlib().hz_decode(bytes(frame), len(frame), None, (1 << 30) - 1, out)
    return rc, int(out[0])


GUARD = 64


def host_decode(frame, cap=None):
    """(code, bytes, second word) of the model, into `cap` bytes (None: what the
    count-only mode finds); asserts that nothing behind the capacity is written."""
    if cap is None:
        cap = host_count(frame)[1]
    dst = ctypes.create_string_buffer(b"\xa5" * (cap + GUARD), cap + GUARD)
    out = (ctypes.c_uint64 * 2)()
    rc = hostlib().hz_decode(bytes(frame), len(frame), dst, cap, out)
    assert dst.raw[cap:] == b"\xa5" * GUARD, "the model wrote behind its capacity"
    assert out[0] <= cap
    return rc, dst.raw[:out[0]], int(out[1])


def host_open(frame):
    out = (ctypes.c_uint64 * 7)()
    rc = hostlib().hz_open(bytes(frame), len(frame), out)
    return rc, [int(x) for x in out]


def fixture_frames():
    """[(array index, codec index, raw bytes, frame)] of the reference's fixture."""
    out = []
    for i in range(13):
        raw = np.load(os.path.join(FIXTURE, "array.%02d.npy" % i), allow_pickle=False)
        raw = raw.tobytes(order="A")
        for j in range(10):
            with open(os.path.join(FIXTURE, "codec.%02d" % j, "encoded.%02d.dat" % i), "rb") as fh:
                out.append((i, j, raw, fh.read()))
    return out


def expected_exception(meta):
    """(class, text) the reference's decompress() comes to for an invalid case,
    from its recorded verdict; None where the reference accepts (the stated
    exceptions: MC_ZSTD_E_MEMBER, Block_Maximum_Size)."""
    v = meta["verdict"]
    if v["stage"] in ("walk", "empty"):
        return RuntimeError, "Zstd decompression error: invalid input data"
    if v["stage"] == "decompress":
        return RuntimeError, "Zstd decompression error: " + v["error"]
    return None
