"""A test-side writer of Zstandard frames (RFC 8878), for the decoder's tests.

Plain Python and numpy; nothing of the product is imported and neither host
model is called.  A frame is written from what the test wants the decoder to
meet: a list of sequences ``(literal-length code, its extra bits, offset code,
its extra bits, match-length code, its extra bits)`` per block, each of the
three tables in a mode given per block (Predefined, RLE, FSE_Compressed from
given normalized counts, Repeat), literals raw / RLE / Huffman (one or four
streams, weights direct or FSE-coded) / treeless, raw and RLE blocks, with or
without Frame_Content_Size and checksum.

  * FSE decode table: the RFC's spread and state numbering (``fse_cells``);
  * count description: the inverse of the RFC's reader (``write_counts``);
  * states: for each symbol, from the last sequence back, the one cell of that
    symbol whose baseline range holds the next state; the reads are written in
    reverse under the final-bit marker (``pack_backward``);
  * expected bytes: the sequence list executed in plain Python with the RFC's
    repeat-offset rules (initial 1, 4, 8; the shift when ll == 0; rep1 - 1);
  * census: what the writer put in, never what a decoder found.

The families of frames the tests run are below (``FAMILIES``, ``cases()``).  Offset
codes of 18 and more need outputs past 256 KB: they stay out, and a cell of an
offset table that holds such a code counts as not enterable.  A literal-length
code 35 or a match-length code 52 with its 16 extra bits all ones would pass
Block_Maximum_Size (131072): those two take the largest extra that fits."""

import collections

import numpy as np

try:
    from tests import zstd_gen as g
except ImportError:  # run as a script beside it (tests/golden/make_golden_zstd_paths.py)
    import zstd_gen as g

LL, OF, ML = 0, 1, 2
LL_BITS = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
LL_BASE = list(range(16)) + [16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384,
                             32768, 65536]
ML_BITS = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
ML_BASE = [c + 3 for c in range(32)] + [35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099,
                                        8195, 16387, 32771, 65539]
DEFAULT = (
    ([4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1], 6),
    ([1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1], 5),
    ([1, 4, 3, 2, 2, 2, 2, 2, 2] + [1] * 37 + [-1] * 7, 6),
)
MAX_LOG = (9, 8, 9)
MAX_SYM = (35, 31, 52)
OF_CODE_LIMIT = 17  # the largest offset code a frame of these sizes can execute
RING = 65536
BLOCK_MAX = 131072


def highbit(v):
    return v.bit_length() - 1


# ---- FSE ---------------------------------------------------------------------------
def fse_cells(norm, log):
    """[(symbol, nbBits, baseline)] of the decode table of `norm` (RFC 8878 4.1.1)."""
    size = 1 << log
    assert sum(abs(c) for c in norm) == size, (sum(abs(c) for c in norm), size)
    sym, high = [0] * size, size - 1
    for s, c in enumerate(norm):
        if c == -1:
            sym[high] = s
            high -= 1
    step, pos = (size >> 1) + (size >> 3) + 3, 0
    for s, c in enumerate(norm):
        for _ in range(max(c, 0)):
            sym[pos] = s
            pos = (pos + step) & (size - 1)
            while pos > high:
                pos = (pos + step) & (size - 1)
    assert pos == 0
    nxt = [1 if c == -1 else c for c in norm]
    cells = []
    for u in range(size):
        s = sym[u]
        ns = nxt[s]
        nxt[s] += 1
        nb = log - highbit(ns)
        cells.append((s, nb, (ns << nb) - size))
    return cells


class Table:
    """One decode table as the writer sees it; `entered` collects the cells a
    written sequence (or weight) was decoded from."""

    def __init__(self, norm, log, mode):
        self.norm, self.log, self.mode = norm, log, mode
        self.cells = fse_cells(norm, log) if mode != "rle" else [(norm, 0, 0)]  # RLE_Mode: `norm` is the symbol
        self.entered = set()
        self.forms, self.zero_runs = set(), []
        self._cover = {}

    def cover(self, sym):
        """next state -> the cell of `sym` whose baseline range holds it."""
        c = self._cover.get(sym)
        if c is None:
            c = [None] * len(self.cells)
            for u, (s, nb, base) in enumerate(self.cells):
                if s == sym:
                    for x in range(base, base + (1 << nb)):
                        assert c[x] is None
                        c[x] = u
            assert None not in c, "symbol %d is not in the table" % sym
            self._cover[sym] = c
        return c

    def first(self, sym):
        for u, (s, _nb, _b) in enumerate(self.cells):
            if s == sym:
                return u
        raise AssertionError("symbol %d is not in the table" % sym)

    def chain(self, symbols, last=None):
        """The cells of `symbols`, chosen from the last one back."""
        out, nxt = [0] * len(symbols), None
        for i in range(len(symbols) - 1, -1, -1):
            u = (self.first(symbols[i]) if last is None else last) if nxt is None else self.cover(symbols[i])[nxt]
            assert self.cells[u][0] == symbols[i]
            out[i] = nxt = u
        self.entered.update(out)
        return out


def rle_table(sym):
    return Table(sym, 0, "rle")


class BitsForward:
    def __init__(self):
        self.acc = self.n = 0

    def put(self, v, k):
        assert 0 <= v < (1 << k)
        self.acc |= v << self.n
        self.n += k

    def bytes(self):
        return self.acc.to_bytes((self.n + 7) // 8, "little")


def write_counts(norm, log, table=None):
    """The FSE table description of `norm`: the inverse of the RFC's reader."""
    size = 1 << log
    assert sum(abs(c) for c in norm) == size and norm[-1] != 0
    w = BitsForward()
    w.put(log - 5, 4)
    remaining, threshold, nb, sym, prev0 = size + 1, size, log + 1, 0, False
    while remaining > 1:
        if prev0:
            z = 0
            while norm[sym + z] == 0:
                z += 1
            if table is not None:
                table.zero_runs.append(z + 1)  # with the zero that raised the flag
            sym += z
            while z >= 3:
                w.put(3, 2)
                z -= 3
            w.put(z, 2)
        count = norm[sym]
        v, low_max = count + 1, (2 * threshold - 1) - remaining
        if v < low_max:
            w.put(v, nb - 1)
            form = "low"
        else:
            w.put(v + low_max if v >= threshold else v, nb)
            form = "high"
        if table is not None:
            table.forms.add(form)
        remaining -= abs(count)
        sym += 1
        prev0 = count == 0
        while remaining < threshold:
            nb -= 1
            threshold >>= 1
    assert sym == len(norm), (sym, len(norm))
    return w.bytes()


def pack_backward(reads):
    """(bytes, marker bit) of a backward bitstream whose reader takes `reads`
    [(value, bits)] in this order, the first one below the final-bit marker."""
    acc = shift = 0
    for v, k in reversed(reads):
        assert 0 <= v < (1 << k) or (k == 0 and v == 0), (v, k)
        acc |= v << shift
        shift += k
    acc |= 1 << shift
    return acc.to_bytes(shift // 8 + 1, "little"), shift % 8


# ---- sequences ---------------------------------------------------------------------
def seq(ll, ml, ov):
    """The 6-tuple of (literal_length, match_length, offset_value); offset_value
    1..3 are the repeat codes, an offset is offset_value - 3."""
    llc = max(c for c in range(36) if LL_BASE[c] <= ll)
    mlc = max(c for c in range(53) if ML_BASE[c] <= ml)
    ofc = highbit(ov)
    assert ll - LL_BASE[llc] < (1 << LL_BITS[llc]) and ml - ML_BASE[mlc] < (1 << ML_BITS[mlc])
    return (llc, ll - LL_BASE[llc], ofc, ov - (1 << ofc), mlc, ml - ML_BASE[mlc])


def nseq_bytes(n, form=None):
    form = form or (1 if n < 128 else 2 if n < 0x7F00 else 3)
    if form == 1:
        assert 0 < n < 128
        return bytes([n])
    if form == 2:
        assert n < 0x7F00
        return bytes([(n >> 8) + 128, n & 255])
    assert n >= 0x7F00
    return b"\xff" + (n - 0x7F00).to_bytes(2, "little")


def _extra_kind(extra, bits):
    return "none" if bits == 0 else "zeros" if extra == 0 else "ones" if extra == (1 << bits) - 1 else "mixed"


# ---- Huffman -----------------------------------------------------------------------
def code_lengths(m, depth):
    """The lengths of a complete prefix code of m symbols whose longest is `depth`."""
    assert depth + 1 <= m <= (1 << depth) or (m, depth) == (2, 1), (m, depth)
    count = collections.Counter(list(range(1, depth)) + [depth, depth])
    n = depth + 1
    while n < m:
        k = min(x for x in count if x < depth and count[x])
        count[k] -= 1
        count[k + 1] += 2
        n += 1
    return sorted(count.elements())


def huf_weights(nsym, depth, present=None, stride=97):
    """`nsym` weights (the last one is the implied one) of a tree of `depth`
    with `present` symbols that have a code (default: all), equal weights
    spread over the symbol numbers by a stride."""
    m = nsym if present is None else present
    lengths = code_lengths(m, depth)
    where = [nsym - 1 - (k * (nsym - 1)) // (m - 1) for k in range(m)] if m > 1 else [nsym - 1]
    assert len(set(where)) == m and max(where) == nsym - 1
    where.sort()
    order = sorted(range(m), key=lambda i: (i * stride) % m)
    weights = [0] * nsym
    for k, i in enumerate(order):
        weights[where[i]] = depth + 1 - lengths[k]
    return weights


def huf_codes(weights):
    """{symbol: (code, bits)} and the tree's depth, by the RFC's ordering."""
    total = sum(1 << (w - 1) for w in weights if w)
    log = highbit(total)
    assert total == 1 << log, total
    codes, pos = {}, 0
    for w in range(1, log + 1):
        for s, x in enumerate(weights):
            if x == w:
                codes[s] = (pos >> (w - 1), log + 1 - w)
                pos += 1 << (w - 1)
    return codes, log


def weights_direct(weights):
    """Tree description of weights[:-1], four bits each."""
    ws = weights[:-1]
    assert 1 <= len(ws) <= 128
    ws = ws + [0] * (len(ws) & 1)
    return bytes([127 + len(weights) - 1]) + bytes((ws[k] << 4) | ws[k + 1] for k in range(0, len(ws), 2))


def weights_fse(weights, wlog, census=None, norm=None):
    """Tree description of weights[:-1], FSE-coded with two interleaved states."""
    ws = weights[:-1]
    n = len(ws)
    assert n >= 2
    if norm is None:
        used = collections.Counter(ws)
        assert len(used) >= 2
        norm = [1 if s in used else 0 for s in range(max(used) + 1)]
        norm[used.most_common(1)[0][0]] += (1 << wlog) - len(used)
    tab = Table(norm, wlog, "fse")
    head = write_counts(norm, wlog, tab)
    chains = [tab.chain(ws[0::2]), tab.chain(ws[1::2])]
    reads = [(chains[0][0], wlog), (chains[1][0], wlog)]
    for i in range(n - 2):
        _s, nb, base = tab.cells[chains[i & 1][i >> 1]]
        reads.append((chains[i & 1][(i >> 1) + 1] - base, nb))
    # the update after weight n - 2 must overrun: no bit is left, and its cell takes at least one
    assert tab.cells[chains[(n - 2) & 1][(n - 2) >> 1]][1] >= 1
    stream, _marker = pack_backward(reads)
    body = head + stream
    assert len(body) < 128, len(body)
    if census is not None:
        census.update(wlog=wlog, end_state=(n - 1) & 1, wtable_symbols=len(norm))
    return bytes([len(body)]) + body


def huf_streams(data, codes, nstreams):
    """([stream bytes], [symbols in each], [marker bit of each])."""
    if nstreams == 1:
        parts = [data]
    else:
        seg = (len(data) + 3) >> 2
        assert 3 * seg <= len(data)
        parts = [data[k * seg:(k + 1) * seg] for k in range(3)] + [data[3 * seg:]]
    packed = [pack_backward([codes[b] for b in p]) for p in parts]
    return [s for s, _m in packed], [len(p) for p in parts], [m for _s, m in packed]


# ---- frames ------------------------------------------------------------------------
Case = collections.namedtuple("Case", "name family frame data census declared")


class FrameWriter:
    def __init__(self):
        self.blocks = []      # (kind, payload, size)
        self.out = bytearray()
        self.rep = [1, 4, 8]
        self.tabs = [None, None, None]
        self.huf = None       # (codes, log) of the last tree
        c = self.census = collections.defaultdict(list)
        c["straddle"], c["rep"] = set(), set()
        c["ll_codes"], c["of_codes"], c["ml_codes"], c["nseq_bytes"], c["modes"] = set(), set(), set(), set(), set()

    # -- blocks that are not compressed
    def raw_block(self, data):
        self._literal_run(len(data), "block")
        self.out += data
        self.blocks.append((0, bytes(data), len(data)))
        self.census["blocks"].append("raw")

    def rle_block(self, byte, n):
        self._literal_run(n, "block")
        self.out += bytes([byte]) * n
        self.blocks.append((1, bytes([byte]), n))
        self.census["blocks"].append("rle")

    def _crosses(self, lo, hi):
        return any(lo < b < hi for b in (RING, 2 * RING))

    def _literal_run(self, n, what):
        if self._crosses(len(self.out), len(self.out) + n):
            self.census["straddle"].add("lit" if what == "lit" else "block")

    # -- literals
    def _literals(self, lit):
        """(section bytes, the literal bytes) of a literals spec."""
        kind = lit[0]
        if kind == "raw":
            data, sf = lit[1], lit[2] if len(lit) > 2 else None
            if sf is None:
                sf = (0 if len(data) % 2 == 0 else 2) if len(data) < 32 else 1 if len(data) < 4096 else 3
            self.census["raw_sf"].append(sf)
            return g.raw_literals(data, sf), data
        if kind == "rle":
            _k, byte, n = lit
            head = bytes([(n << 3) | 1]) if n < 32 else ((n << 4) | 4 | 1).to_bytes(2, "little") if n < 4096 else \
                ((n << 4) | 12 | 1).to_bytes(3, "little")
            return head + bytes([byte]), bytes([byte]) * n
        if kind == "huf":
            _k, data, weights, nstreams, wlog = lit[:5]
            codes, log = huf_codes(weights)
            h = {"log": log, "nweights": len(weights) - 1, "coded": "direct" if wlog is None else "fse", "treeless": False,
                 # the most groups of 64 symbols that symbols of one weight lie in
                 "groups": max(len({s >> 6 for s, w in enumerate(weights) if w == k}) for k in set(weights) - {0})}
            tree = weights_direct(weights) if wlog is None else \
                weights_fse(weights, wlog, h, norm=lit[5] if len(lit) > 5 else None)
            self.huf = (codes, log)
            ltype = 2
        else:
            _k, data, nstreams = lit
            assert kind == "treeless" and self.huf
            codes, log = self.huf
            h = {"log": log, "nweights": None, "coded": None, "treeless": True}
            tree, ltype = b"", 3
        streams, lens, markers = huf_streams(data, codes, nstreams)
        h.update(nstreams=nstreams, regen=len(data), stream_bytes=[len(s) for s in streams], lens=lens, markers=markers,
                 last_bytes=[s[-1] for s in streams])
        self.census["huf"].append(h)
        body = tree + (b"".join(len(s).to_bytes(2, "little") for s in streams[:3]) if nstreams == 4 else b"") + \
            b"".join(streams)
        regen, comp = len(data), len(body)
        if nstreams == 1:
            assert regen < 1024 and comp < 1024, (regen, comp)
            head = (ltype | (regen << 4) | (comp << 14)).to_bytes(3, "little")
        elif regen < 1024 and comp < 1024:
            head = (ltype | 4 | (regen << 4) | (comp << 14)).to_bytes(3, "little")
        elif regen < 16384 and comp < 16384:
            head = (ltype | 8 | (regen << 4) | (comp << 18)).to_bytes(4, "little")
        else:
            head = (ltype | 12 | (regen << 4) | (comp << 22)).to_bytes(5, "little")
        return head + body, bytes(data)

    # -- a compressed block
    def compressed(self, lit, seqs=(), modes=("pre", "pre", "pre"), last_cells=None, nseq_form=None, execute=True,
                   pad=b""):
        section, literals = self._literals(lit)
        self.census["blocks"].append("compressed")
        self.census["lit_kinds"].append(lit[0])
        seqs = list(seqs)
        if not seqs:
            payload = section + b"\x00"
            self._literal_run(len(literals), "lit")
            self.out += literals
            self.census["zero_seq_blocks"].append(len(self.blocks))
        else:
            head = b""
            for which, mode in enumerate(modes):
                col = (0, 2, 4)[which]
                if mode == "pre":
                    self.tabs[which] = Table(*DEFAULT[which], "pre")
                elif mode == "rle":
                    assert len({s[col] for s in seqs}) == 1
                    self.tabs[which] = rle_table(seqs[0][col])
                    head += bytes([seqs[0][col]])
                elif mode == "rep":
                    assert self.tabs[which] is not None
                    self.census["repeat_after"].append((which, self.tabs[which].mode, self.census["blocks"][-2]
                                                        if len(self.census["blocks"]) > 1 else None,
                                                        bool(self.census["zero_seq_blocks"]) and
                                                        self.census["zero_seq_blocks"][-1] == len(self.blocks) - 1))
                else:
                    _m, norm, log = mode
                    t = self.tabs[which] = Table(norm, log, "fse")
                    t.which = which
                    head += write_counts(norm, log, t)
                    self.census["tables"].append(t)
                self.census["modes"].add((which, mode if isinstance(mode, str) else "fse"))
            tabs = self.tabs
            chains = [tabs[w].chain([s[(0, 2, 4)[w]] for s in seqs], None if last_cells is None else last_cells[w])
                      for w in range(3)]
            reads = [(chains[w][0], tabs[w].log) for w in (LL, OF, ML)]
            for i, (llc, lle, ofc, ofe, mlc, mle) in enumerate(seqs):
                reads += [(ofe, ofc), (mle, ML_BITS[mlc]), (lle, LL_BITS[llc])]
                if i + 1 < len(seqs):
                    for w in (LL, ML, OF):
                        _s, nb, base = tabs[w].cells[chains[w][i]]
                        reads.append((chains[w][i + 1] - base, nb))
                self.census["ll_codes"].add((llc, _extra_kind(lle, LL_BITS[llc])))
                self.census["ml_codes"].add((mlc, _extra_kind(mle, ML_BITS[mlc])))
                self.census["of_codes"].add(ofc)
            stream, marker = pack_backward(reads)
            stream = pad + stream
            count = nseq_bytes(len(seqs), nseq_form)
            self.census["nseq_bytes"].add(len(count))
            mode_byte = sum(({"pre": 0, "rle": 1, "rep": 3}[m] if isinstance(m, str) else 2) << (6 - 2 * w)
                            for w, m in enumerate(modes))
            payload = section + count + bytes([mode_byte]) + head
            self.census["bitstreams"].append({"bytes": len(stream), "marker": marker, "block": len(self.blocks),
                                              "at": len(payload)})  # `at`: from the block's start, fixed up in finish()
            payload += stream
            if execute:
                self._execute(seqs, literals)
        assert len(payload) < BLOCK_MAX
        self.blocks.append((2, payload, len(payload)))

    def _execute(self, seqs, literals):
        out, rep, c, lp = self.out, self.rep, self.census, 0
        first_of_block = True
        before = len(out)
        for llc, lle, ofc, ofe, mlc, mle in seqs:
            ll, ml, ov = LL_BASE[llc] + lle, ML_BASE[mlc] + mle, (1 << ofc) + ofe
            assert lp + ll <= len(literals), "literal length beyond the literals"
            self._literal_run(ll, "lit")
            out += literals[lp:lp + ll]
            lp += ll
            if ov > 3:
                offset = ov - 3
                rep[:] = [offset, rep[0], rep[1]]
            else:
                idx = ov - 1 + (ll == 0)
                c["rep"].add((idx, ll == 0))
                if first_of_block:
                    c["rep_first_in_block"].append((len(self.blocks), c["blocks"][-2] if len(c["blocks"]) > 1 else None))
                offset = rep[0] - 1 if idx == 3 else rep[idx]
                assert offset >= 1, "a repeat offset of 0"
                if idx == 1:
                    rep[:] = [offset, rep[0], rep[2]]
                elif idx >= 2:
                    rep[:] = [offset, rep[0], rep[1]]
            first_of_block = False
            pos = len(out)
            assert offset <= pos, ("offset beyond the output", offset, pos)
            form = "global" if offset > RING else "step" if offset >= 64 else "rep"
            c["matches"].append((form, offset, ml, pos))
            if self._crosses(pos, pos + ml):
                c["straddle"].add("match_" + form)
            if self._crosses(pos - offset, pos - offset + min(ml, offset)):
                c["straddle"].add("pattern" if form == "rep" else "src_" + form)
            if offset >= ml:
                out += out[pos - offset:pos - offset + ml]
            else:
                pat = bytes(out[pos - offset:pos])
                out += (pat * (ml // offset + 1))[:ml]
        self._literal_run(len(literals) - lp, "lit")
        out += literals[lp:]
        assert len(out) - before <= BLOCK_MAX, "Block_Maximum_Size"

    # -- the frame
    def finish(self, name, family, declared=True, checksum=False):
        data = bytes(self.out)
        if declared:
            head = g.frame_header(len(data), checksum=checksum)
        else:
            wlog = max(10, (max(len(data), 1) - 1).bit_length())
            head = g.frame_header(None, window=(wlog - 10) << 3, checksum=checksum)
        body, census = bytearray(head), dict(self.census)
        starts = []
        for k, (kind, payload, size) in enumerate(self.blocks):
            body += ((size << 3) | (kind << 1) | (k + 1 == len(self.blocks))).to_bytes(3, "little")
            starts.append(len(body))
            body += payload
        census["bitstreams"] = [dict(b, start=starts[b["block"]] + b["at"]) for b in self.census["bitstreams"]]
        ends_on_stream = bool(self.blocks) and self.blocks[-1][0] == 2 and census["bitstreams"] and \
            census["bitstreams"][-1]["block"] == len(self.blocks) - 1 and not checksum
        census["ends_on_bitstream"] = len(body) % 4 if ends_on_stream else None
        census["checksum"], census["declared"], census["size"] = bool(checksum), declared, len(data)
        if checksum:
            body += (g.xxh64(data) & 0xFFFFFFFF).to_bytes(4, "little")
        return Case(name + ("" if declared else "_nosize"), family, bytes(body), data, census, declared)


def _both(build, name, family, **kw):
    """The frame with and without a declared size (a Window_Descriptor instead)."""
    w = build()
    return [w.finish(name, family, declared=d, **kw) for d in (True, False)]


# ---- the families -------------------------------------------------------------------
MATCH_LENGTHS = (3, 63, 64, 65, 129, 200)
MATCH_WIDE = tuple((o, ln) for o in (64, 65, 127, 128, 255, 256, 257) for ln in (o - 1, o, o + 1))


def family_match_small():
    """One match a frame, every (offset, length) of the list whose frame stays
    within 256 bytes: the ring of 256."""
    out = []
    pairs = [(o, ln) for o in range(1, 64) for ln in MATCH_LENGTHS] + list(MATCH_WIDE)
    for o, ln in pairs:
        if o + ln > 256:
            continue

        def build(o=o, ln=ln):
            w = FrameWriter()
            w.compressed(("raw", g.noise(o, 1000 + o)), [seq(o, ln, o + 3)])
            return w
        out += _both(build, "match_small_o%d_l%d" % (o, ln), "match_small")
    return out


def family_match_big():
    """All of the list, one frame per length (and one for the wide offsets),
    three noise literals between the matches."""
    out = []
    for ln in MATCH_LENGTHS:
        def build(ln=ln):
            w = FrameWriter()
            lits = g.noise(64 + 3 * 63, 1100 + ln)
            w.compressed(("raw", lits), [seq(64 if o == 1 else 3, ln, o + 3) for o in range(1, 64)] +
                         [seq(3, 3, 5)])
            return w
        out += _both(build, "match_big_l%d" % ln, "match_big")

    def wide():
        w = FrameWriter()
        w.compressed(("raw", g.noise(300 + 3 * len(MATCH_WIDE), 1190)),
                     [seq(300 if k == 0 else 3, ln, o + 3) for k, (o, ln) in enumerate(MATCH_WIDE)])
        return w
    return out + _both(wide, "match_big_wide", "match_big")


def family_wrap():
    """What straddles output position 65536 (the ring's wrap), in frames whose
    first bytes are raw blocks."""
    def prefixed(n, seed, then):
        def build():
            w = FrameWriter()
            data = g.noise(n, seed)
            for at in range(0, n, 65000):
                w.raw_block(data[at:at + 65000])
            then(w)
            w.raw_block(g.noise(700, seed + 50))
            return w
        return build
    lit = g.noise(4096, 1201)
    cases = [
        ("wrap_literal_run", prefixed(65530, 1210, lambda w: w.compressed(("raw", lit[:40]), [seq(30, 5, 7)]))),
        ("wrap_match_rep", prefixed(65500, 1211, lambda w: w.compressed(("raw", lit[:12]), [seq(10, 100, 30 + 3)]))),
        ("wrap_match_step", prefixed(65450, 1212, lambda w: w.compressed(("raw", lit[:12]), [seq(10, 200, 100 + 3)]))),
        ("wrap_source", prefixed(65590, 1213, lambda w: w.compressed(("raw", lit[:12]), [seq(10, 80, 100 + 3)]))),
        ("wrap_pattern", prefixed(65536, 1214, lambda w: w.compressed(("raw", lit[:12]), [seq(10, 150, 30 + 3)]))),
        ("wrap_offsets", prefixed(65536, 1215, lambda w: w.compressed(
            ("raw", lit[:80]), [seq(20, 100, 65535 + 3), seq(5, 100, 65536 + 3), seq(5, 100, 65537 + 3),
                                seq(3, 64, 65536 + 3), seq(3, 65, 65537 + 3), seq(3, 130, 65535 + 3)]))),
        ("wrap_global_overlap", prefixed(65536, 1216, lambda w: w.compressed(
            ("raw", lit[:10]), [seq(4, 65600, 65537 + 3), seq(3, 7, 1)]))),
        ("wrap_global_overlap_far", prefixed(70000, 1217, lambda w: w.compressed(
            ("raw", lit[:10]), [seq(4, 70100, 70001 + 3)]))),
        ("wrap_global_across_131072", prefixed(130950, 1218, lambda w: w.compressed(
            ("raw", lit[:60]), [seq(50, 300, 70000 + 3), seq(5, 40, 100000 + 3)]))),
    ]
    out = []
    for name, build in cases:
        out += _both(build, name, "wrap", checksum=name in ("wrap_offsets", "wrap_global_overlap"))
    return out


def _code_seq(llc, lle, ofc, ofe, mlc, mle):
    return (llc, lle, ofc, ofe, mlc, mle)


def family_codes():
    """Every literal-length and match-length code with its extra bits all zeros
    and all ones (predefined tables), and offset codes 0..17."""
    out = []
    ones = lambda bits: (1 << bits) - 1  # noqa: E731

    def ll_small():
        w = FrameWriter()
        seqs = [_code_seq(c, e, 2, 1, 0, 0) for c in range(31) for e in sorted({0, ones(LL_BITS[c])})]
        n = sum(LL_BASE[s[0]] + s[1] for s in seqs)
        w.compressed(("raw", g.noise(n + 10, 1301)), [seq(5, 3, 4)] + seqs)
        return w
    out += _both(ll_small, "codes_ll_0_30", "codes")

    def ml_small():
        w = FrameWriter()
        seqs = [_code_seq(3, 0, 3, c & 3, c, e) for c in range(46) for e in sorted({0, ones(ML_BITS[c])})]
        w.compressed(("raw", g.noise(3 * len(seqs) + 20, 1302)), [seq(20, 3, 9)] + seqs)
        return w
    out += _both(ml_small, "codes_ml_0_45", "codes")
    for c in range(31, 36):
        for kind in ("zeros", "ones"):
            e = 0 if kind == "zeros" else ones(LL_BITS[c])
            if c == 35 and kind == "ones":
                e = BLOCK_MAX - 3 - LL_BASE[35]  # the largest that Block_Maximum_Size leaves room for

            def build(c=c, e=e):
                w = FrameWriter()
                n = LL_BASE[c] + e
                lit = ("raw", g.noise(n, 1310 + c)) if n < 60000 else ("rle", 0x40 + c, n)
                w.compressed(lit, [_code_seq(c, e, 4, 2, 0, 0)])
                return w
            out += _both(build, "codes_ll_%d_%s" % (c, kind), "codes")
    for c in range(46, 53):
        for kind in ("zeros", "ones"):
            e = 0 if kind == "zeros" else ones(ML_BITS[c])
            if c == 52 and kind == "ones":
                e = BLOCK_MAX - 40 - ML_BASE[52]

            def build(c=c, e=e):
                w = FrameWriter()
                w.compressed(("raw", g.noise(40, 1350 + c)), [_code_seq(23, 0, 5, 6, c, e)])  # ll 40, offset 35
                return w
            out += _both(build, "codes_ml_%d_%s" % (c, kind), "codes")

    def offsets():
        w = FrameWriter()
        data = g.noise(131072, 1370)
        w.raw_block(data[:65536])
        w.raw_block(data[65536:])
        seqs = [_code_seq(2, 0, c, e, 2, 0) for c in range(2, OF_CODE_LIMIT + 1)
                for e in sorted({0, ones(c) if c < 17 else 5})]  # code 17 all ones: an offset of 262140
        seqs += [_code_seq(2, 0, 0, 0, 2, 0), _code_seq(2, 0, 1, 0, 2, 0), _code_seq(2, 0, 1, 1, 2, 0)]
        w.compressed(("raw", g.noise(2 * len(seqs), 1371)), seqs)
        return w
    return out + _both(offsets, "codes_of_0_17", "codes")


def family_repeat():
    """The four resolutions of a repeat code with ll > 0 and ll == 0, the initial
    1, 4, 8, a repeat code first in a second block and after raw and RLE blocks."""
    def initial():
        w = FrameWriter()
        # the frame's first repeat codes: rep2 = 4, then rep3 = 8, then rep3 = 1
        w.compressed(("raw", g.noise(40, 1401)), [seq(10, 4, 2), seq(2, 5, 3), seq(3, 6, 3), seq(1, 3, 1)])
        return w

    def all_forms():
        w = FrameWriter()
        s = [seq(30, 4, 20 + 3), seq(2, 4, 11 + 3), seq(2, 4, 5 + 3)]
        s += [seq(2, 5, 1), seq(2, 5, 2), seq(2, 5, 3)]            # ll > 0: rep1, rep2, rep3
        s += [seq(0, 6, 1), seq(0, 6, 2), seq(0, 6, 3)]            # ll == 0: rep2, rep3, rep1 - 1
        s += [seq(1, 7, 2), seq(0, 7, 3), seq(0, 3, 1), seq(4, 9, 3), seq(0, 4, 2)]
        w.compressed(("raw", g.noise(60, 1402)), s)
        w.compressed(("raw", g.noise(9, 1403)), [seq(0, 5, 2), seq(3, 4, 1), seq(0, 4, 3)])  # a repeat code first
        return w

    def after_blocks():
        w = FrameWriter()
        w.compressed(("raw", g.noise(50, 1404)), [seq(40, 4, 33 + 3), seq(2, 4, 17 + 3)])
        w.raw_block(g.noise(100, 1405))
        w.compressed(("raw", g.noise(9, 1406)), [seq(3, 5, 2), seq(0, 5, 1)])
        w.rle_block(0x33, 90)
        w.compressed(("raw", g.noise(9, 1407)), [seq(0, 6, 3), seq(2, 5, 3)])
        w.compressed(("rle", 0x77, 20), [])
        w.compressed(("raw", g.noise(4, 1408)), [seq(2, 6, 2)])
        return w
    out = []
    for name, build in (("repeat_initial", initial), ("repeat_all_forms", all_forms), ("repeat_after_blocks", after_blocks)):
        out += _both(build, name, "repeat")
    return out


# -- tables
def table_counts(which, log, shape):
    """Normalized counts of a table of 1 << log cells with a given shape."""
    size, top = 1 << log, MAX_SYM[which]
    if shape == "one_big":
        return [1, size - 4, 1, 1, 1] if which != OF else [1, 1, size - 4, 1, 1]
    if shape == "uniform":
        n = min(size // 2, (24, 11, 40)[which])
        return [size // n + (k < size % n) for k in range(n)]
    if shape == "neg15":
        if which == OF:  # codes 0..15 only: a larger one needs more history than a block may hold
            return [-1] * 3 + [size - 15] + [-1] * 12
        n = (17, 0, 18)[which]
        rest = size - n
        return [-1] * n + [rest - rest // 2, rest // 2]
    if shape == "zero_runs":
        # zero runs of 1, 2, 3, 4, 6 and 7 between the seven symbols that have cells
        norm, at = [0] * 30, [0, 2, 5, 9, 14, 21, 29]
        share = (size - 2) // 5
        for k, s in enumerate(at):
            norm[s] = -1 if k >= 5 else share
        norm[0] += size - 2 - 5 * share
        return norm
    if shape == "last_max":
        norm = [0] * (top + 1)
        norm[top] = -1
        for s, c in ((0, size - 1 - 6), (1, 3), (3, 2), (6, 1)):
            norm[s] = c
        return norm
    raise KeyError(shape)


SHAPES = ("one_big", "uniform", "neg15", "zero_runs", "last_max")


def _cost(which, sym):
    """The most output bytes a sequence with this code can bring (family_tables keeps the large codes' extras 0)."""
    if which == OF:
        return 0
    base, bits = (LL_BASE[sym], LL_BITS[sym]) if which == LL else (ML_BASE[sym], ML_BITS[sym])
    return base if base >= 4096 else base + (1 << bits) - 1


def _enterable(which, sym):
    return which != OF or sym <= OF_CODE_LIMIT


def _path_to_new_cell(t, w, start, todo, syms, room):
    """The symbols of the shortest way (breadth first, cheap symbols on the way,
    any affordable one at its end) from cell `start` back to a cell not entered yet."""
    cheap = [s for s in syms if _cost(w, s) <= 40]
    last = [s for s in syms if _cost(w, s) <= room - 2000]
    seen, frontier = {start: None}, [start]
    while frontier:
        nxt = []
        for x in frontier:
            for s in last:
                u = t.cover(s)[x]
                if u in todo:
                    path = [s]
                    while seen[x] is not None:
                        x, s0 = seen[x]
                        path.append(s0)
                    return path[::-1]
            for s in cheap:
                u = t.cover(s)[x]
                if u not in seen:
                    seen[u] = (x, s)
                    nxt.append(u)
        frontier = nxt
    return []


def _walk_tables(norms_logs, seed, budget=40000, limit=120000, max_seqs=3000):
    """Blocks of symbol triples [(symbols, last cells)] that between them enter
    every enterable cell of the three tables: from each block's last sequence
    back, the symbol is picked whose cell for the next state is not entered yet.
    A block is closed at `budget` output bytes and never passes `limit`."""
    tabs = [Table(norm, log, "fse") for norm, log in norms_logs]
    todo = [{u for u, c in enumerate(t.cells) if _enterable(w, c[0])} for w, t in enumerate(tabs)]
    syms = [sorted({c[0] for c in t.cells if _enterable(w, c[0])}, key=lambda s: (_cost(w, s), s))
            for w, t in enumerate(tabs)]
    cheap = [[s for s in syms[w] if _cost(w, s) <= 40] for w in range(3)]
    rnd = np.frombuffer(g.noise(1 << 16, seed), np.uint8)
    blocks, r = [], 0
    while any(todo):
        symbols, state, cost = [], [None] * 3, 0
        for w, t in enumerate(tabs):  # the last sequence's cells: any
            u = min(todo[w], key=lambda x: (_cost(w, t.cells[x][0]), x)) if todo[w] else None
            if u is None or cost + _cost(w, t.cells[u][0]) > limit:
                u = t.first(cheap[w][0])
            state[w] = u
            cost += _cost(w, t.cells[u][0])
        last = tuple(state)
        paths = [[], [], []]
        while True:
            symbols.append(tuple(tabs[w].cells[state[w]][0] for w in range(3)))
            for w in range(3):
                todo[w].discard(state[w])
            if cost > budget or len(symbols) >= max_seqs:
                break
            picks = []
            for w, t in enumerate(tabs):
                if not paths[w]:
                    paths[w] = _path_to_new_cell(t, w, state[w], todo[w], syms[w], limit - cost)
                picks.append(paths[w].pop(0) if paths[w] else None)
            if picks == [None, None, None]:  # nothing more this block can enter
                break
            for w, t in enumerate(tabs):
                if picks[w] is not None and cost + _cost(w, picks[w]) > limit - 2000:  # another table took the room
                    picks[w], paths[w] = None, []
                if picks[w] is None:
                    picks[w] = cheap[w][rnd[r % len(rnd)] % len(cheap[w])]
                    r += 1
                cost += _cost(w, picks[w])
                state[w] = t.cover(picks[w])[state[w]]
        blocks.append((symbols[::-1], last))
    return blocks


def family_tables():
    """FSE_Compressed tables of every accuracy log and shape, LL, OF and ML of
    one (log, shape) together in a frame, the sequences chosen so that every
    enterable cell is entered; the later blocks of a frame use Repeat_Mode."""
    out = []
    for k in range(5):
        for shape in SHAPES:
            logs = (5 + k, min(5 + k, 8), 5 + k)
            norms_logs = [(table_counts(w, logs[w], shape), logs[w]) for w in range(3)]

            def build(norms_logs=norms_logs, k=k, shape=shape):
                w = FrameWriter()
                seed = 1500 + 10 * k + SHAPES.index(shape)
                top_of = max(s for s, c in enumerate(norms_logs[OF][0]) if c and s <= OF_CODE_LIMIT)
                w.raw_block(g.noise(max(64, (1 << top_of) * 2), seed))  # at most 64 KiB: history for every offset
                rnd = np.frombuffer(g.noise(1 << 16, seed + 5000), np.uint8).astype(np.int64)
                r = 0
                for b, (symbols, last) in enumerate(_walk_tables(norms_logs, seed)):
                    seqs = []
                    for llc, ofc, mlc in symbols:
                        x = int(rnd[r % 65536]) | int(rnd[(r + 1) % 65536]) << 8 | int(rnd[(r + 2) % 65536]) << 16
                        r += 3
                        lle = x & ((1 << LL_BITS[llc]) - 1)
                        mle = (x >> 3) & ((1 << ML_BITS[mlc]) - 1)
                        if LL_BASE[llc] >= 4096:
                            lle = 0
                        if ML_BASE[mlc] >= 4096:
                            mle = 0
                        ofe = (x >> 5) & ((1 << ofc) - 1)
                        if ofc == 1 and LL_BASE[llc] + lle == 0:
                            ofe = 0  # never rep1 - 1, which may be 0
                        seqs.append((llc, lle, ofc, ofe, mlc, mle))
                    n = sum(LL_BASE[s[0]] + s[1] for s in seqs)
                    lit = ("raw", g.noise(n + 3, seed + 100 + b)) if n < 30000 else ("rle", 0x21 + b, n + 3)
                    modes = tuple(("fse",) + nl for nl in norms_logs) if b == 0 else ("rep", "rep", "rep")
                    if b:  # the tables of block 0 go on: the census of their cells with them
                        keep = list(w.tabs)
                    w.compressed(lit, seqs, modes, last_cells=last)
                    if b:
                        assert w.tabs == keep
                return w
            out += _both(build, "tables_log%d_%s" % (5 + k, shape), "tables")

    def repeat_modes():
        w = FrameWriter()
        lits = g.noise(400, 1590)
        one = [seq(9, 5, 9), seq(3, 4, 20), seq(2, 6, 9), seq(4, 3, 30)]
        w.compressed(("raw", lits[:40]), one, ("pre", "pre", "pre"))
        w.compressed(("raw", lits[40:80]), one, ("rep", "rep", "rep"))           # after Predefined
        same = [seq(3, 5, 20), seq(3, 5, 21), seq(3, 5, 17)]
        w.compressed(("raw", lits[80:100]), same, ("rle", "rle", "rle"))
        w.compressed(("raw", lits[100:120]), same[::-1], ("rep", "rep", "rep"))  # after RLE_Mode
        fse = (("fse", [8, 8, 4, 4, 2, 2, 1, 1, 1, 1], 5), ("fse", [2, 2, 2, 4, 16, 4, 2], 5),
               ("fse", [10, 10, 4, 4, 2, 1, 1], 5))
        w.compressed(("raw", lits[120:160]), one, fse)
        w.compressed(("raw", lits[160:200]), one[::-1], ("rep", "rep", "rep"))   # after FSE_Compressed
        w.compressed(("raw", lits[200:230]), [])                                   # zero sequences
        w.compressed(("raw", lits[230:270]), one, ("rep", "rep", "rep"))         # after a block with none
        w.compressed(("raw", lits[270:310]), one, ("rep", "pre", "rep"))
        return w
    return out + _both(repeat_modes, "tables_repeat_modes", "tables")


# -- Huffman
def _huf_data(weights, n, seed):
    present = np.array([s for s, w in enumerate(weights) if w], np.uint8)
    r = np.frombuffer(g.noise(2 * n, seed), np.uint16).astype(np.int64)
    data = present[r % len(present)]
    k = min(n, len(present))
    data[:k] = present[np.argsort((np.arange(len(present)) * 37) % len(present))][:k]  # every symbol, where there is room
    return data.tobytes()


FOUR_STREAM_SIZES = tuple(n for n in list(range(4, 49)) + [1023, 1024, 1025, 1026, 16383, 16384, 16385, 16386, 59, 71]
                          if 3 * ((n + 3) >> 2) <= n)  # every size but 5; at 6 and 9 the fourth stream is its marker alone
ONE_STREAM_SIZES = tuple(range(1, 41)) + (1022, 1023)


def family_huffman():
    out = []
    trees = []  # (name, weights, wlog)
    for n in (1, 2, 64, 65, 127, 128):
        depth = {1: 1, 2: 2}.get(n, 8 if n < 127 else 9)
        trees.append(("direct_%d" % n, huf_weights(n + 1, depth), None))
    for n in (129, 200, 255):
        for wlog in (5, 6):
            trees.append(("fse_%d_log%d" % (n, wlog), huf_weights(n + 1, 9, present=n + 1 if n == 255 else n - 20), wlog))
    trees.append(("depth_11_direct", huf_weights(100, 11, present=40), None))
    trees.append(("depth_11_fse", huf_weights(256, 11, present=150), 6))
    trees.append(("ties_256", huf_weights(256, 10, present=256, stride=61), 6))
    for name, weights, wlog in trees:
        for nstreams in (1, 4):
            def build(weights=weights, wlog=wlog, nstreams=nstreams, name=name):
                w = FrameWriter()
                n = 700 if nstreams == 1 else 3001
                if max(weights) <= 2 and nstreams == 1:
                    n = 333
                data = _huf_data(weights, n, 1600 + len(name))
                w.compressed(("huf", data, weights, nstreams, wlog), [seq(len(data) // 2, 9, 33)])
                return w
            out += _both(build, "huf_%s_%dstream" % (name, nstreams), "huffman")

    def wide_weights_table():
        # an FSE table of more than 64 symbols: only a weights' description can carry one.  Weight values 70 and
        # 71 have cells in it (71 as a "less than 1" symbol); the weights written are 1 and 2
        w = FrameWriter()
        weights = [1, 2, 1, 2, 1, 1, 2, 2, 2, 2, 5]
        norm = [0, 20, 7] + [0] * 67 + [4, -1]
        for nstreams, n in ((1, 200), (4, 901)):
            w.compressed(("huf", _huf_data(weights, n, 1650 + n), weights, nstreams, 5, norm), [seq(n // 3, 5, 20)])
        return w
    out += _both(wide_weights_table, "huf_weights_table_72_symbols", "huffman")
    small = huf_weights(12, 4)

    def one_stream_sizes():
        w = FrameWriter()
        for n in ONE_STREAM_SIZES:
            w.compressed(("huf", _huf_data(small, n, 1700 + n), small, 1, None), [])
        return w
    out += _both(one_stream_sizes, "huf_one_stream_sizes", "huffman")
    mid = huf_weights(40, 7)

    def four_stream_sizes():
        w = FrameWriter()
        for n in FOUR_STREAM_SIZES:
            w.compressed(("huf", _huf_data(mid, n, 1800 + n), mid, 4, None), [] if n & 1 else [seq(n - 1, 4, 6)])
        return w
    out += _both(four_stream_sizes, "huf_four_stream_sizes", "huffman")

    def markers():
        # symbol 0 has a code of one bit: 8 k of it end on a byte (the stream's last byte is exactly 1), 8 k + 7
        # put the marker on the top bit of the last byte
        w = FrameWriter()
        tree = [2, 1, 1]
        for data in (b"\0" * 7, b"\0" * 8, b"\0" * 15, b"\0" * 16, b"\1\2\0", b"\2" * 4 + b"\0" * 7):
            w.compressed(("huf", data, tree, 1, None), [])
        for n in (28, 32, 60, 64):  # four streams of 7, 8, 15, 16
            w.compressed(("huf", b"\0" * n, tree, 4, None), [])
        w.compressed(("huf", b"\0" * 7 + b"\1" * 7 + b"\2" * 4 + b"\0" * 10, tree, 4, None), [])
        return w
    out += _both(markers, "huf_markers", "huffman")

    def treeless():
        w = FrameWriter()
        w.compressed(("huf", _huf_data(mid, 500, 1950), mid, 4, None), [seq(100, 5, 50)])
        w.compressed(("raw", g.noise(33, 1951)), [seq(10, 4, 1)])
        w.compressed(("rle", 0x6B, 70), [seq(9, 4, 2)])
        w.raw_block(g.noise(10, 1952))
        w.rle_block(0x11, 12)
        w.compressed(("treeless", _huf_data(mid, 300, 1953), 1), [seq(10, 4, 3)])
        w.compressed(("treeless", _huf_data(mid, 1500, 1954), 4), [seq(700, 30, 900)])
        return w
    return out + _both(treeless, "huf_treeless", "huffman")


# -- the bit window
WINDOW_LENGTHS = tuple(range(240, 253)) + tuple(range(484, 497))


def family_bits():
    """Sequence bitstreams around the window's stride of 61 dwords, at every
    start alignment; a long one; every marker position; frames of every length
    modulo 4 that end on their bitstream."""
    out = []
    for nbytes in WINDOW_LENGTHS:
        for align in range(4):
            def build(nbytes=nbytes, align=align):
                # RLE_Mode tables take no state bits: offset code 8 makes a sequence exactly one byte of the
                # stream, so nbytes - 1 sequences and the marker make nbytes bytes
                w = FrameWriter()
                n = nbytes - 1
                rnd = g.noise(n, 2100 + nbytes + align)
                # the first block leaves 512 + align bytes of history; the second starts with no literals
                w.compressed(("raw", g.noise(512 + align, 2000 + nbytes), 1), [])
                w.compressed(("raw", g.noise(align, 2050 + nbytes), 1),
                             [_code_seq(0, 0, 8, rnd[i], 0, 0) for i in range(n)], ("rle", "rle", "rle"))
                return w
            out += _both(build, "bits_%d_align%d" % (nbytes, align), "bits")

    def long_stream():
        w = FrameWriter()
        rnd = np.frombuffer(g.noise(4 * 1200, 2200), np.uint8).astype(np.int64).reshape(-1, 4)
        seqs = [seq(int(a) % 19, 3 + int(b) % 40, 4 + (int(c) | int(d) << 8) % 300) for a, b, c, d in rnd]
        seqs[0] = seq(310, 5, 9)
        n = sum(LL_BASE[s[0]] + s[1] for s in seqs)
        w.compressed(("raw", g.noise(n, 2201)), seqs)
        return w
    out += _both(long_stream, "bits_long_stream", "bits", checksum=True)
    for ofc in range(2, 10):
        for extra in range(4):
            def build(ofc=ofc, extra=extra):
                # one sequence, no state bits: ofc offset bits, 10 of the literal length and the marker; `extra` literals move the frame's end
                w = FrameWriter()
                llc, lle, _c, _e, mlc, mle = seq(1100, 10, 4)
                w.compressed(("raw", g.noise(1100 + extra, 2300 + ofc), 1),
                             [(llc, lle, ofc, (1 << ofc) - 1, mlc, mle)], ("rle", "rle", "rle"))
                return w
            out += _both(build, "bits_marker_of%d_len%d" % (ofc, extra), "bits")

    def three_byte_count():
        w = FrameWriter()
        n = 0x7F00 + 5
        rnd = g.noise(n, 2400)
        w.compressed(("raw", g.noise(600, 2401)), [seq(600, 3, 5)] +
                     [_code_seq(0, 0, 8, rnd[i], 0, 0) for i in range(n - 1)], ("pre", "pre", "pre"))
        return w
    return out + _both(three_byte_count, "bits_three_byte_count", "bits")


XXH_LENGTHS = (1, 3, 4, 7, 8, 31, 32, 33, 63, 64, 511, 512, 513, 543, 544, 545, 1023, 1024, 1055)


def family_xxh64():
    out = []
    for n in XXH_LENGTHS:
        def build(n=n):
            w = FrameWriter()
            w.raw_block(g.noise(n, 2500 + n))
            return w
        out += _both(build, "xxh64_%d" % n, "xxh64", checksum=True)
    return out


FAMILIES = (("match_small", family_match_small), ("match_big", family_match_big), ("wrap", family_wrap),
            ("codes", family_codes), ("repeat", family_repeat), ("tables", family_tables),
            ("huffman", family_huffman), ("bits", family_bits), ("xxh64", family_xxh64))
_cases = None


def cases():
    """Every valid frame of every family, built once a process."""
    global _cases
    if _cases is None:
        _cases = [c for _name, make in FAMILIES for c in make()]
        assert len({c.name for c in _cases}) == len(_cases)
    return _cases


def family(name):
    return [c for c in cases() if c.family == name]


VALID_TWINS = []  # (name of an invalid case, its frame without the fault, the bytes it decodes to)


# ---- invalid frames -------------------------------------------------------------------
def invalid_cases():
    """[(name, frame, capacity, note)]: one fault each.  What the decoder must say
    is the host model's verdict; the note says where libzstd 1.4.8 is laxer."""
    out = []
    del VALID_TWINS[:]

    def frame(blocks, size):
        w = FrameWriter()
        w.blocks = blocks
        w.out = bytearray(size)
        return w.finish("x", "invalid", declared=False).frame  # no declared size: the fault is the only one

    def one_block(lit, seqs, modes=("pre", "pre", "pre"), size=64, **kw):
        w = FrameWriter()
        w.compressed(lit, seqs, modes, execute=False, **kw)
        return frame(w.blocks, size)
    lits = g.noise(64, 2600)
    out.append(("rep1_minus_1_is_0", one_block(("raw", lits[:10]), [seq(0, 4, 3)]), 64,
                ""))
    out.append(("literal_length_beyond", one_block(("raw", lits[:5]), [seq(10, 4, 4)]), 64, ""))
    deep = list(range(11, 0, -1)) + [1, 12]  # 2^11 before the implied weight: a complete code of 12 bits
    w = FrameWriter()
    w.compressed(("huf", bytes([12, 5, 0, 12]), deep, 1, None), [])
    out.append(("weights_past_depth_11", frame(w.blocks, 4), 64,
                "libzstd accepts a code of 12 bits; the RFC's limit is 11"))
    blk = bytes([127 + 3, (2 << 4) | 2, 1 << 4]) + b"\x01"
    sec = (2 | (1 << 4) | (len(blk) << 14)).to_bytes(3, "little") + blk
    out.append(("odd_weight_1_count", frame([(2, sec + b"\x00", len(sec) + 1)], 1), 64,
                "weights 2, 2, 1: what is left of the power of two is no power of two, so no last weight mends "
                "the odd count"))
    w = FrameWriter()
    mid = huf_weights(40, 7)
    w.compressed(("huf", _huf_data(mid, 100, 2601), mid, 4, None), [])
    payload = bytearray(w.blocks[0][1])
    tree = len(weights_direct(mid))
    l2 = int.from_bytes(payload[3 + tree + 2:3 + tree + 4], "little")
    l3 = int.from_bytes(payload[3 + tree + 4:3 + tree + 6], "little")
    payload[3 + tree + 2:3 + tree + 4] = (0).to_bytes(2, "little")        # the second stream: empty
    payload[3 + tree + 4:3 + tree + 6] = (l2 + l3).to_bytes(2, "little")
    out.append(("four_streams_one_empty", frame([(2, bytes(payload), len(payload))], 100), 128, ""))
    w = FrameWriter()
    w.compressed(("raw", lits[:30]), [seq(8, 4, 9), seq(3, 4, 9)],
                 (("fse", [8, 8, 4, 4, 2, 2, 1, 1, 1, 1], 5), "pre", "pre"))
    payload = bytearray(w.blocks[0][1])
    at = len(g.raw_literals(lits[:30], 0)) + 2  # the literals, the count, the modes: the description's first byte
    assert payload[at] & 15 == 0
    payload[at] |= 5  # Accuracy_Log 10
    out.append(("accuracy_log_10", frame([(2, bytes(payload), len(payload))], 38), 64, ""))
    many = [0, 20, 8] + [0] * 67 + [4]  # the weights' alphabet up to symbol 70: two passes of the wave builder
    for name, wts in (("weights_fse_71_symbols", [1, 2, 1, 70, 1, 1, 2, 2, 2, 2]), ("", [1, 2, 1, 2, 1, 1, 2, 2, 2, 2])):
        blk = weights_fse(wts + [5], 5, norm=many) + b"\x03"  # symbol 10, the implied weight 5: the code '1'
        sec = (2 | (1 << 4) | (len(blk) << 14)).to_bytes(3, "little") + blk
        if name:
            out.append((name, frame([(2, sec + b"\x00", len(sec) + 1)], 1), 64, ""))
        else:
            VALID_TWINS.append(("weights_fse_71_symbols", frame([(2, sec + b"\x00", len(sec) + 1)], 1), b"\x0a"))
    out.append(("bitstream_byte_left_over", one_block(("raw", lits[:10]), [seq(6, 4, 9)], ("rle", "rle", "rle"),
                                                      pad=b"\x00"), 64, ""))
    return out
