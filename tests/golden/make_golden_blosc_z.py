"""Generate tests/golden/blosc_z_cases.npz and blosc_z_cases.json: the Blosc
frames with zlib and zstd streams of tests/blosc_z_gen.build_cases(), their
streams written by the standard library's ``zlib`` and by libzstd through
``ctypes`` (tests/zstd_gen.Lib), each with the array bytes it decodes to or
the code it must be refused with.

Every valid frame is decoded here with those two libraries alone (the frame
walk is the oracle's), and the replaced stream of every malformed frame is
shown to be refused by its library -- or, where the library alone accepts it
(a declared or decoded size other than the share, a second frame), to give
another size than the share.

Run where libzstd.so.1 loads:

    python tests/golden/make_golden_blosc_z.py

Fixtures are data, not program text.
"""

import os
import struct
import sys
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import blosc_gen as bg  # noqa: E402
from tests import blosc_z_gen as g  # noqa: E402
from tests import zstd_gen as zg  # noqa: E402

lib = zg.Lib()
assert lib.version == "1.4.8", lib.version


def streams_of(frame):
    """[(stream bytes, share)] of a compressed frame, by the container's rules."""
    flags, ts, nbytes, bs = frame[2], frame[3], *struct.unpack("<II", frame[4:12])
    nblocks = -(-nbytes // bs)
    out = []
    for b in range(nblocks):
        bsize = min(bs, nbytes - b * bs)
        ns = bg.split_streams(flags, ts, bs, bsize)
        p = struct.unpack("<i", frame[16 + 4 * b:20 + 4 * b])[0]
        for _ in range(ns):
            cb = struct.unpack("<i", frame[p:p + 4])[0]
            out.append((frame[p + 4:p + 4 + cb], bsize // ns))
            p += 4 + cb
    return out


def decode_stream(fname, stream, share):
    """The stream's bytes by its library, or None where the library refuses it."""
    if len(stream) == share:
        return stream
    if fname == "zlib":
        try:
            return zlib.decompress(stream)
        except zlib.error:
            return None
    got, _err = lib.decompress(stream, max(share, 1) + 64)
    return got


cases = g.build_cases(lib)
names = [c[0] for c in cases]
assert len(set(names)) == len(names)
for name, fname, frame, data, code, bad in cases:
    flags, ts, nbytes, bs = frame[2], frame[3], *struct.unpack("<II", frame[4:12])
    assert nbytes == len(data) and struct.unpack("<I", frame[12:16])[0] == len(frame), name
    if flags & 2 or nbytes == 0:
        assert code == 0 and frame[16:16 + nbytes] == data, name
        continue
    parts = streams_of(frame)
    assert max(share for _s, share in parts) <= 320 * 1024, name
    decoded = [decode_stream(fname, s, share) for s, share in parts]
    if code == 0:
        assert all(d is not None and len(d) == share for d, (_s, share) in zip(decoded, parts)), name
        assert bg.unfilter(b"".join(decoded), flags, ts, bs) == data, name
    else:
        for k, (d, (_s, share)) in enumerate(zip(decoded, parts)):
            assert (d is None or len(d) != share) == (k == bad), (name, k)
g.save_cases(cases)
size = os.path.getsize(g.GOLDEN + ".npz")
assert size < 1 << 20, size
print(len(cases), "cases,", size, "bytes")
