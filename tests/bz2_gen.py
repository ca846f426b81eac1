"""bz2 decode tests: the case list, the stdlib as judge, the ctypes binding of
the host model (csrc/mc_bz2.h through tests/native_bz2), and a small Python
walker, independent of the product, that decodes every valid case and takes
the census the tests assert (so the list cannot drift away from what it is
there for)."""

import bz2
import ctypes
import os

import numpy as np

from tests import bz2_write as bw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_DIR = os.path.join(ROOT, "tests", "native_bz2", "_build")
_CACHE = {}

# the two documented departures: refused here, decoded (or judged otherwise) by the stdlib
DEPARTURES = {"randomised": 5, "second-stream": 20, "second-stream-prefix": 20, "second-stream-BZh": 20}


# ---- data ---------------------------------------------------------------------
def noise(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def plain(n, seed=0):
    """n bytes with no two equal neighbours."""
    return bytes((37 * i + 11 * seed + (i >> 3)) % 251 for i in range(n))


def _two_cycle_block(n, seed):
    """A last column whose permutation has several cycles, and an origPtr on one
    of at least 2 and at most n // 2 steps from which the block decodes."""
    rng = np.random.default_rng(seed)
    last = bytes(rng.choice(np.frombuffer(b"\x00\x01\x02\x03\x05", np.uint8), n).tolist())
    order = bw.successors(last)
    seen = [False] * n
    for start in range(n):
        if seen[start]:
            continue
        cyc, p = 0, start
        while not seen[p]:
            seen[p] = True
            p = order[p]
            cyc += 1
        if 2 <= cyc <= n // 2 and bw.unrle1(bw.inverse_walk(last, start)[0]) is not None:
            return last, start
    raise AssertionError("no suitable cycle")


# ---- the cases ------------------------------------------------------------------
def _cases():
    if "cases" in _CACHE:
        return _CACHE["cases"]
    valid, invalid, facts = [], [], {}

    def std(name, data, level=1):
        valid.append((name, bz2.compress(data, level), data))

    def crafted(name, blocks, ok, **kw):
        frame, data, f, marks = bw.build(blocks, **kw)
        facts[name] = dict(f, marks=marks)
        if ok:
            valid.append((name, frame, data))
        else:
            invalid.append((name, frame))
        return frame

    std("empty", b"")
    std("one-byte", b"\x07")
    std("one-value", b"\x55" * 50)
    std("all-256", bytes(range(256)))
    for n in (63, 64, 65, 255):
        std(f"plain-{n}", plain(n))
    for r in (3, 4, 5, 255, 256, 259, 260):
        std(f"run-{r}-straddle", plain(61) + b"\x01" * r + plain(30, 1))  # 5 of byte 1: the count equals the byte
        std(f"run-{r}-end", plain(10) + b"\xfb" * r)
    std("zeros100000", bytes(100000))
    for n, k in ((100, 2), (400, 3), (900, 4), (1800, 5), (3000, 6)):
        std(f"tables-{k}", noise(n, k))
    for n in (99980, 99981, 99982):
        std(f"random-{n}", noise(99982, 5)[:n])
    big = noise(250000, 6)
    std("random-250000-l1", big, 1)
    std("random-250000-l9", big, 9)
    a = bz2.compress(plain(100))
    valid.append(("trailing-xyz", a + b"xyz", plain(100)))
    valid.append(("trailing-zeros", a + bytes(7), plain(100)))
    valid.append(("trailing-BZh0", a + b"BZh0abc", plain(100)))

    p19 = bytes((i * 7) % 19 + 60 for i in range(300))
    crafted("writer-len20", [dict(payload=p19, lengths=[bw.chain_lengths(21)] * 2)], True)
    crafted("writer-orig0", [dict(payload=bytes(range(10, 40)))], True)
    crafted("writer-orig-last", [dict(payload=bytes(range(40, 10, -1)))], True)
    crafted("writer-small", [dict(payload=plain(20))], True)
    crafted("writer-surplus-selectors", [dict(payload=plain(100), extra_selectors=18010 - 3)], True)
    crafted("writer-six-tables", [dict(payload=plain(400), ntables=6)], True)
    crafted("writer-two-blocks", [dict(payload=plain(150)), dict(payload=plain(333, 2), ntables=3)], True)
    for name, n in (("writer-two-cycles-small", 300), ("writer-two-cycles", 5000)):
        last, orig = _two_cycle_block(n, n)
        crafted(name, [dict(last=last, orig=orig)], True)

    base = dict(payload=plain(120))
    crafted("base", [base], True)
    nblock = facts["base"]["nblock"]
    alpha = facts["base"]["alpha"]
    for name, kw in (("magic-B", dict(head=b"XZh")), ("magic-Z", dict(head=b"BXh")), ("magic-h", dict(head=b"BZx")),
                     ("level-0", dict(level_byte=0x30)), ("level-colon", dict(level_byte=0x3A)),
                     ("end-magic", dict(end_magic=bw.END_MAGIC ^ 0x100)), ("combined-crc", dict(combined_xor=1))):
        crafted(name, [base], False, **kw)
    wide = [l + 1 for l in bw.default_lengths(alpha)]
    for name, kw in (
            ("block-magic", dict(magic=bw.BLOCK_MAGIC ^ 1)), ("block-magic-first", dict(magic=bw.BLOCK_MAGIC ^ (3 << 40))),
            ("origptr-huge", dict(orig_field=10 + 100000 + 1)), ("origptr-nblock", dict(orig_field=nblock)),
            ("empty-map", dict(empty_map=True)), ("ngroups-1", dict(ngroups_field=1)), ("ngroups-7", dict(ngroups_field=7)),
            ("nselectors-0", dict(nsel_field=0)), ("selector-missing-table", dict(selectors=[0, 2, 1])),
            ("codelen-0", dict(start_len=0)), ("codelen-0-delta", dict(lengths=[[1, 0] + [9] * (alpha - 2)] * 2)),
            ("codelen-21", dict(lengths=[[20, 21] + [9] * (alpha - 2)] * 2)),
            ("oversubscribed", dict(lengths=[[3] * alpha] * 2)),
            ("incomplete-unused-code", dict(lengths=[wide] * 2, eob=False, tail_code=((1 << max(wide)) - 1, max(wide)))),
            ("run-overflow", dict(syms=[bw.RUNB] * 17)), ("run-weight", dict(syms=[bw.RUNA] * 22)),
            ("no-eob", dict(eob=False)), ("groups-exceed-selectors", dict(selectors=[0, 1])),
            ("block-crc", dict(crc_xor=1)), ("randomised", dict(randomised=1))):
        crafted(name, [dict(base, **kw)], False)
    frame = crafted("cuts", [dict(payload=plain(40))], True)
    for cut in range(1, len(frame)):  # every structural boundary and the middle of a symbol among them
        invalid.append((f"cut-{cut:03d}", frame[:cut]))
    long = bz2.compress(big, 1)
    for cut in (len(long) // 3, len(long) // 2, len(long) - 5, len(long) - 1):
        invalid.append((f"cut-long-{cut}", long[:cut]))
    invalid.append(("second-stream", a + a))
    invalid.append(("second-stream-prefix", a + b"BZ"))
    invalid.append(("second-stream-BZh", a + b"BZh"))
    _CACHE["cases"] = (valid, invalid, facts)
    return _CACHE["cases"]


def valid_cases():
    """[(name, frame, data)]"""
    return _cases()[0]


def invalid_cases():
    """[(name, frame)]"""
    return _cases()[1]


def writer_facts():
    return _cases()[2]


def stdlib_decode(frame):
    """("ok", bytes) or ("error", exception class, text)."""
    try:
        return ("ok", bz2.decompress(bytes(frame)))
    except (OSError, ValueError, EOFError) as e:
        return ("error", type(e), str(e))


def fixture_frames():
    """[(array index, codec index, raw bytes, frame)] of the reference's fixtures."""
    from tests.helpers import fixture_cases
    out = []
    for arr, j, _cfg, enc in fixture_cases("bz2"):
        out.append((len(out), j, arr.tobytes(order="A"), enc))
    return out


# ---- the host model -----------------------------------------------------------------
def hostlib():
    if "lib" not in _CACHE:
        lib = ctypes.CDLL(os.path.join(HOST_DIR, "libbz2_hostcheck.so"))
        lib.hb_bz2.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t,
                               ctypes.POINTER(ctypes.c_uint64)]
        lib.hb_bz2.restype = ctypes.c_int
        lib.hb_bz2_crc.argtypes = [ctypes.c_char_p, ctypes.c_size_t]
        lib.hb_bz2_crc.restype = ctypes.c_uint32
        lib.hb_bz2_gfmul.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
        lib.hb_bz2_gfmul.restype = ctypes.c_uint32
        lib.hb_bz2_mulx.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
        lib.hb_bz2_mulx.restype = ctypes.c_uint32
        lib.hb_bz2_tables_bytes.restype = ctypes.c_size_t
        lib.hb_bz2_record_bytes.restype = ctypes.c_size_t
        _CACHE["lib"] = lib
    return _CACHE["lib"]


def host_count(frame):
    """(code, bytes counted, second word) of the model's count-only mode."""
    out = (ctypes.c_uint64 * 2)()
    rc = hostlib().hb_bz2(bytes(frame), len(frame), None, (1 << 30) - 1, out)
    return rc, int(out[0]), int(out[1])


def host_decode(frame, cap=None):
    """(code, bytes, second word) of the model decoding into `cap` bytes
    (default: what the count-only mode counted)."""
    if cap is None:
        cap = host_count(frame)[1]
    buf = np.full(cap + 64, 0xA5, np.uint8)
    out = (ctypes.c_uint64 * 2)()
    rc = hostlib().hb_bz2(bytes(frame), len(frame), buf.ctypes.data, cap, out)
    assert (buf[cap:] == 0xA5).all(), "the model wrote past its capacity"
    return rc, buf[:int(out[0])].tobytes(), int(out[1])


# ---- the walker ------------------------------------------------------------------------
class _Bits:
    def __init__(self, data):
        self.data, self.pos, self.end = bytes(data) + bytes(8), 0, 8 * len(data)

    def peek(self, n):
        byte = self.pos >> 3
        chunk = int.from_bytes(self.data[byte:byte + 8], "big")
        return (chunk >> (64 - (self.pos & 7) - n)) & ((1 << n) - 1)

    def read(self, n):
        if self.pos + n > self.end:
            raise EOFError("walker: out of data")
        v = self.peek(n)
        self.pos += n
        return v


def walk(frame):
    """(bytes, census) of a valid stream; census = {"level", "end" (the byte the
    stream ends at), "blocks": [per block: tables, tables_used, nsel, nblock,
    orig, cycle, max_code, counts (the count bytes met), count_is_byte,
    straddles (a run of four and its count in different 64-byte steps),
    count_ends_block, start_bit]}."""
    assert frame[:3] == b"BZh" and 0x31 <= frame[3] <= 0x39
    br = _Bits(frame)
    br.pos = 32
    out, blocks, combined = bytearray(), [], 0
    while True:
        start_bit = br.pos
        m = br.read(48)
        if m == bw.END_MAGIC:
            break
        assert m == bw.BLOCK_MAGIC
        crc = br.read(32)
        assert br.read(1) == 0
        orig = br.read(24)
        rows, used = br.read(16), []
        for r in range(16):
            if (rows >> (15 - r)) & 1:
                bits = br.read(16)
                used += [16 * r + c for c in range(16) if (bits >> (15 - c)) & 1]
        alpha = len(used) + 2
        ng, nsel = br.read(3), br.read(15)
        order, sels = list(range(ng)), []
        for _ in range(nsel):
            j = 0
            while br.read(1):
                j += 1
            order.insert(0, order.pop(j))
            sels.append(order[0])
        sels = sels[:18002]
        tables = []
        for _t in range(ng):
            curr, lens = br.read(5), []
            for _i in range(alpha):
                while br.read(1):
                    curr += -1 if br.read(1) else 1
                assert 1 <= curr <= 20
                lens.append(curr)
            codes = bw.assign_codes(lens)
            tables.append((min(lens), max(lens), {(l, c): s for s, (l, c) in enumerate(zip(lens, codes))}))
        mtf, col, k, run, weight, tables_used, max_code = list(used), bytearray(), 0, 0, 1, set(), 0
        while True:
            t = sels[k // 50]
            tables_used.add(t)
            mn, mx, d = tables[t]
            p = br.peek(20)
            for zn in range(mn, mx + 1):
                s = d.get((zn, p >> (20 - zn)))
                if s is not None:
                    break
            else:
                raise ValueError("walker: an unused code")
            br.read(zn)
            k += 1
            max_code = max(max_code, zn)
            if s <= 1:
                run += weight << s
                weight <<= 1
                continue
            if run:
                col += bytes([mtf[0]]) * run
                run, weight = 0, 1
            if s == alpha - 1:
                break
            mtf.insert(0, mtf.pop(s - 1))
            col.append(mtf[0])
        n = len(col)
        assert n <= 100000 * (frame[3] - 0x30) and orig < n
        succ = np.argsort(np.frombuffer(bytes(col), np.uint8), kind="stable").tolist()
        pre, p, cycle = bytearray(n), orig, 0
        for q in range(n):
            p = succ[p]
            pre[q] = col[p]
            if p == orig and not cycle:
                cycle = q + 1
        data, i, counts, count_is_byte, straddles, count_ends = bytearray(), 0, set(), False, False, False
        while i < n:
            c, r = pre[i], 1
            while r < 4 and i + r < n and pre[i + r] == c:
                r += 1
            i += r
            if r == 4:
                assert i < n
                counts.add(pre[i])
                count_is_byte |= pre[i] == c
                straddles |= (i - 4) // 64 != i // 64
                count_ends |= i == n - 1
                r += pre[i]
                i += 1
            data += bytes([c]) * r
        assert bw.crc32_bz(data) == crc
        combined = (((combined << 1) | (combined >> 31)) & 0xFFFFFFFF) ^ crc
        out += data
        blocks.append(dict(tables=ng, tables_used=tables_used, nsel=nsel, nblock=n, orig=orig, cycle=cycle,
                           max_code=max_code, counts=counts, count_is_byte=count_is_byte, straddles=straddles,
                           count_ends_block=count_ends, start_bit=start_bit))
    assert br.read(32) == combined
    return bytes(out), dict(level=frame[3] - 0x30, end=(br.pos + 7) // 8, blocks=blocks)
