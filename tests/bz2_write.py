"""A bzip2 block writer for what the stdlib's encoder never emits: a chosen
number of Huffman tables, chosen code lengths and selectors, surplus selectors,
a chosen origPtr or last column (so a permutation of several cycles), the
randomised bit, wrong CRCs, and field values no encoder writes.  A naive
rotation sort is enough at the sizes the tests use.  The CRC of a block is the
CRC of what the writer's own inverse walk (exactly nblock steps from origPtr)
and RLE1 undo give, so a crafted block is a valid stream whenever the format
allows it."""

import zlib

BLOCK_MAGIC, END_MAGIC = 0x314159265359, 0x177245385090
RUNA, RUNB = 0, 1
_REV = bytes(int(f"{b:08b}"[::-1], 2) for b in range(256))


def crc32_bz(data):
    """CRC-32 with polynomial 0x04c11db7, MSB first: zlib's, bit-reflected."""
    c = zlib.crc32(bytes(data).translate(_REV))
    return int(f"{c:032b}"[::-1], 2)


class BitWriter:
    def __init__(self):
        self.v, self.n, self.marks = 0, 0, {}

    def write(self, value, nbits):
        self.v = (self.v << nbits) | (value & ((1 << nbits) - 1))
        self.n += nbits

    def mark(self, name):
        self.marks[name] = self.n

    def bytes(self):
        pad = -self.n % 8
        return ((self.v << pad).to_bytes((self.n + pad) // 8, "big")) if self.n else b""


def rle1(data):
    out, i, n = bytearray(), 0, len(data)
    while i < n:
        j = i
        while j < n and data[j] == data[i] and j - i < 255:
            j += 1
        run = j - i
        out += bytes([data[i]]) * min(run, 4)
        if run >= 4:
            out.append(run - 4)
        i = j
    return bytes(out)


def unrle1(pre):
    """The RLE1 undo of `pre`, or None where it ends with a count byte due."""
    out, i, n = bytearray(), 0, len(pre)
    while i < n:
        c, run = pre[i], 1
        while run < 4 and i + run < n and pre[i + run] == c:
            run += 1
        i += run
        if run == 4:
            if i >= n:
                return None
            run += pre[i]
            i += 1
        out += bytes([c]) * run
    return bytes(out)


def bwt(pre):
    n = len(pre)
    doubled = pre + pre
    rots = sorted(range(n), key=lambda i: doubled[i:i + n])
    return bytes(pre[(i - 1) % n] for i in rots), rots.index(0)


def successors(last):
    """order[j] = the index in `last` of the j-th byte of the sorted column."""
    return sorted(range(len(last)), key=lambda i: (last[i], i))


def inverse_walk(last, orig):
    """What exactly len(last) steps from orig visit, and the length of orig's cycle."""
    order = successors(last)
    out, p, cycle = bytearray(), orig, 0
    for k in range(len(last)):
        p = order[p]
        out.append(last[p])
        if p == orig and not cycle:
            cycle = k + 1
    return bytes(out), cycle


def mtf_symbols(last, used):
    lst, syms, zeros = list(used), [], 0

    def flush():
        nonlocal zeros
        while zeros:
            syms.append(RUNA if zeros & 1 else RUNB)
            zeros = (zeros - 1) >> 1
    for b in last:
        j = lst.index(b)
        if j == 0:
            zeros += 1
            continue
        flush()
        syms.append(j + 1)
        lst.insert(0, lst.pop(j))
    flush()
    return syms


def default_lengths(alpha):
    """A complete code of two adjacent lengths."""
    k = max(1, (alpha - 1).bit_length())
    short = (1 << k) - alpha
    return [k - 1] * short + [k] * (alpha - short) if k > 1 else [1] * alpha


def chain_lengths(alpha):
    """Lengths 1, 2, 3, ... with the last two alike, held to 20: complete up
    to 21 symbols, incomplete (but usable) beyond."""
    return [min(i + 1, 20) for i in range(alpha - 1)] + [min(alpha - 1, 20)]


def assign_codes(lengths):
    codes, vec = [0] * len(lengths), 0
    for n in range(min(lengths), max(lengths) + 1):
        for i, l in enumerate(lengths):
            if l == n:
                codes[i] = vec
                vec += 1
        vec <<= 1
    return codes


def write_block(w, payload=None, *, last=None, orig=None, orig_field=None, ntables=2, lengths=None, selectors=None,
                extra_selectors=0, nsel_field=None, ngroups_field=None, randomised=0, crc_xor=0, syms=None, eob=True,
                tail_code=None, start_len=None, empty_map=False, magic=BLOCK_MAGIC):
    """One block into BitWriter `w`: (its CRC as written, the bytes it decodes to, facts)."""
    if last is None:
        last, orig = bwt(rle1(payload))
    pre, cycle = inverse_walk(last, orig)
    data = unrle1(pre)
    crc = crc32_bz(data or b"") ^ crc_xor
    w.mark("magic")
    w.write(magic, 48)
    w.mark("crc")
    w.write(crc, 32)
    w.mark("randomised")
    w.write(randomised, 1)
    w.mark("orig")
    w.write(orig if orig_field is None else orig_field, 24)
    w.mark("map")
    used = sorted(set(last))
    if empty_map:
        w.write(0, 16)
    else:
        rows = sorted({b >> 4 for b in used})
        w.write(sum(1 << (15 - r) for r in rows), 16)
        for r in rows:
            w.write(sum(1 << (15 - (b & 15)) for b in used if b >> 4 == r), 16)
    alpha = len(used) + 2
    if syms is None:
        syms = mtf_symbols(last, used)
    syms = list(syms) + ([alpha - 1] if eob else [])
    lengths = lengths or [default_lengths(alpha)] * ntables
    need = -(-len(syms) // 50)
    sel = list(selectors) if selectors is not None else [k % ntables for k in range(need)]
    sel_all = sel + [0] * extra_selectors
    w.mark("ngroups")
    w.write(ntables if ngroups_field is None else ngroups_field, 3)
    w.mark("nsel")
    w.write(len(sel_all) if nsel_field is None else nsel_field, 15)
    w.mark("selectors")
    order = list(range(8))
    for s in sel_all:
        j = order.index(s)
        w.write(((1 << j) - 1) << 1, j + 1)
        order.insert(0, order.pop(j))
    w.mark("lengths")
    for t in range(ntables):
        curr = lengths[t][0] if start_len is None else start_len
        w.write(curr, 5)
        for l in lengths[t]:
            while curr < l:
                w.write(0b10, 2)
                curr += 1
            while curr > l:
                w.write(0b11, 2)
                curr -= 1
            w.write(0, 1)
    w.mark("symbols")
    codes = [assign_codes(l) for l in lengths]
    for k, s in enumerate(syms):
        t = sel[min(k // 50, len(sel) - 1)] if sel else 0
        t = t if t < ntables else 0
        w.write(codes[t][s], lengths[t][s])
        if k == len(syms) // 2:
            w.mark("mid")
    if tail_code:
        w.write(*tail_code)
    w.mark("end")
    facts = {"nblock": len(last), "orig": orig, "cycle": cycle, "nsym": len(syms), "alpha": alpha}
    return crc, data or b"", facts


def build(blocks, level=1, head=b"BZh", level_byte=None, end_magic=END_MAGIC, combined_xor=0):
    """(stream, the bytes it decodes to, the last block's facts, the bit offsets
    of the last block's fields) for a list of write_block keyword dicts."""
    w = BitWriter()
    for b in head:
        w.write(b, 8)
    w.write(0x30 + level if level_byte is None else level_byte, 8)
    combined, out, facts = 0, b"", {}
    for spec in blocks:
        crc, data, facts = write_block(w, **spec)
        combined = (((combined << 1) | (combined >> 31)) & 0xFFFFFFFF) ^ crc
        out += data
    w.mark("end_magic")
    w.write(end_magic, 48)
    w.mark("combined")
    w.write(combined ^ combined_xor, 32)
    return w.bytes(), out, facts, dict(w.marks)
