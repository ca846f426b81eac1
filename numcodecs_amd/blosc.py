"""Blosc on the GPU (reference: src/numcodecs/blosc.pyx:211-326, 448-509).

Decompression: Blosc1 frames whose compressor is LZ4 / LZ4HC, and memcpyed
(stored) frames, become device-resident arrays -- decompressed by
csrc/mc_blosc_dec.hip (one plan launch and one decode launch for a whole
batch of frames) and unshuffled by ``mc_blosc_filter`` (one launch per frame
that carries a shuffle flag).  Frames compressed with zlib or zstd are decoded
too when the call allows them -- ``formats=DECODE_FORMATS`` on
:func:`decompress` / :func:`decompress_many`, or :class:`BloscFull` -- by
csrc/mc_blosc_dec_z.hip: one plan launch and one decode launch per format
present in the batch, which may mix all of them.  Every zstd stream is one
Zstandard frame and every zlib stream one zlib frame; they are held to the
stand-alone ``zstd`` / ``zlib`` decoders' rules (no dictionary, one frame per
stream, content checksum and Adler-32 verified) and must produce exactly
their share of the block.  The default, ``formats=("lz4",)``, refuses them
with NotImplementedError as before.

Compression (:func:`compress`, :func:`compress_many`, :class:`BloscLZ4`):
buffers become Blosc1 LZ4 frames -- shuffled by ``mc_blosc_filter`` (one
launch per shuffled frame) and compressed, laid out and gathered by
csrc/mc_blosc_enc.hip (three launches for a whole batch).  The frames are
valid Blosc1 LZ4 frames that any Blosc reader decodes; they are not byte-equal
to c-blosc's (the match finder differs).  With ``cname='zstd'`` and
``formats=ENCODE_FORMATS`` (or :class:`BloscFull`) every block becomes one
Zstandard frame through the ``zstd`` encoder's own kernels, and the same
layout and gather kernels assemble the container (eight launches for a whole
batch).  Compression with the other Blosc compressors (blosclz, lz4hc,
snappy, zlib) and decompression of blosclz and snappy frames are not built:
DESIGN.md §7.  The
stand-alone ``lz4`` codec is :mod:`numcodecs_amd.lz4`.

The 16-byte frame header is read on the host: version, versionlz, flags,
typesize, then nbytes, blocksize, cbytes as little-endian u32.  For frames
that are already on the device this costs one small device-to-host copy
(one gathered copy for a whole batch).  Everything after the header --
``bstarts``, the streams' ``cbytes`` words, every LZ4 sequence -- is read and
validated on the device (csrc/mc_lz4.h); a violation comes back in a
per-frame error record and raises ``RuntimeError('error during blosc
decompression: -1')``, the reference's text with c-blosc's generic code.

``Blosc`` is the decode-only class (its ``encode`` raises); ``BloscLZ4`` is
the full codec for lz4; ``BloscFull`` is ``BloscLZ4`` that also decodes zlib
and zstd frames and encodes zstd ones.  None is registered on import: call :func:`register`.

Staging a batch's inputs, placing its outputs and handing results back is
:mod:`numcodecs_amd._frames`, shared with the ``lz4`` codec; the rest is Blosc's.
"""

import numpy as np
import torch

from . import _frames
from ._native import check, lib
from .abc import Codec
from .blosc_shuffle import AUTOBLOCKS, AUTOSHUFFLE, BITSHUFFLE, NOSHUFFLE, SHUFFLE
from .compat import ensure_contiguous_ndarray, is_device_tensor, upload
from .registry import register_codec

__all__ = ["Blosc", "BloscLZ4", "BloscFull", "DECODE_FORMATS", "ENCODE_FORMATS", "NOSHUFFLE", "SHUFFLE", "BITSHUFFLE", "AUTOSHUFFLE", "AUTOBLOCKS", "cbuffer_sizes",
           "compress", "compress_many", "decompress", "decompress_many", "register"]

_HEADER = 16
_F_SHUFFLE, _F_MEMCPYED, _F_BITSHUFFLE, _F_NOSPLIT = 0x1, 0x2, 0x4, 0x10
_FORMAT_LZ4, _FORMAT_ZLIB, _FORMAT_ZSTD = 1, 3, 4
_FORMAT_NAMES = {0: "blosclz", 1: "lz4", 2: "snappy", 3: "zlib", 4: "zstd"}
_FORMAT_CODES = {"lz4": _FORMAT_LZ4, "zlib": _FORMAT_ZLIB, "zstd": _FORMAT_ZSTD}
# the Blosc compressors a call may be allowed to use (its ``formats``); lz4 covers lz4hc frames
DECODE_FORMATS = ("lz4", "zlib", "zstd")
ENCODE_FORMATS = ("lz4", "zstd")
_MAX_BLOCKSIZE = (1 << 30) - 1  # mc_blosc_decode_batch refuses more (c-blosc's own limit is lower)
_ERROR_TEXT = "error during blosc decompression: -1"

# one record of mc_blosc_decode_batch's frame table (include/mcodec.h)
_FRAME_RECORD = np.dtype([("src_off", "<u8"), ("src_len", "<u8"), ("dst", "<u8"), ("nbytes", "<u4"),
                          ("blocksize", "<u4"), ("typesize", "<u4"), ("flags", "<u4"), ("block_base", "<u4"),
                          ("stream_base", "<u4")])
assert _FRAME_RECORD.itemsize == 48
# ... and of mc_blosc_decode_batch_z's: the same, then the frame's place in the literals area
_FRAME_RECORD_Z = np.dtype(_FRAME_RECORD.descr + [("lit_off", "<u8")])
assert _FRAME_RECORD_Z.itemsize == 56


def _decode_error(frame_errors):
    """The reference's RuntimeError; ``frame_errors`` maps the index of each
    rejected frame to (code, stream): code -1 for a failed host check, else
    the device error record's: mc_lz4_error (csrc/mc_lz4.h) for an lz4 frame;
    for a zstd / zlib frame mc_zstd_error (csrc/mc_zstd.h) / mc_inf_error
    (csrc/mc_inflate.h) for a violation inside a stream, and 64 + mc_lz4_error
    for one of the container (csrc/mc_blosc_z.h)."""
    exc = RuntimeError(_ERROR_TEXT)
    exc.frame_errors = dict(frame_errors)
    return exc


def _parse_header(hdr) -> tuple:
    """(version, flags, typesize, nbytes, blocksize, cbytes) of 16 header bytes."""
    h = bytes(hdr)
    return (h[0], h[2], h[3], int.from_bytes(h[4:8], "little"), int.from_bytes(h[8:12], "little"),
            int.from_bytes(h[12:16], "little"))


def _flat_bytes(buf):
    """`buf` as flat uint8 (blosc.pyx:499), within ``Blosc.max_buffer_size``."""
    return _frames.flat_bytes(buf, Blosc.max_buffer_size)


def cbuffer_sizes(source):
    """(nbytes, cbytes, blocksize) of a Blosc frame, from its header
    (blosc.pyx:177-196).  A device-resident frame costs a 16-byte copy."""
    src = _flat_bytes(source)
    if len(src) < _HEADER:
        raise _decode_error({0: (-1, 0)})
    hdr = src[:_HEADER].cpu().numpy() if is_device_tensor(src) else src[:_HEADER]
    _v, _f, _ts, nbytes, blocksize, cbytes = _parse_header(hdr)
    return nbytes, cbytes, blocksize


def _nstreams(flags, typesize, nbytes, blocksize):
    """(blocks, streams, largest stream) of a frame: csrc/mc_lz4.h's rules."""
    nblocks = -(-nbytes // blocksize)
    last = nbytes - (nblocks - 1) * blocksize
    if flags & _F_MEMCPYED:
        return nblocks, nblocks, min(blocksize, nbytes)
    split = not (flags & _F_NOSPLIT) and typesize <= 16 and blocksize // typesize >= 128
    if not split:
        return nblocks, nblocks, min(blocksize, nbytes)
    full = nblocks if last == blocksize else nblocks - 1
    longest = max(blocksize // typesize if full else 0, last if full < nblocks else 0)
    return nblocks, full * typesize + (nblocks - full), longest


def _mode(flags, typesize):
    """The filter a frame's bytes still carry once its streams are decoded."""
    if flags & _F_MEMCPYED:
        return NOSHUFFLE
    if flags & _F_BITSHUFFLE:
        return BITSHUFFLE
    return SHUFFLE if flags & _F_SHUFFLE and typesize > 1 else NOSHUFFLE


def _check_formats(formats, allowed, what):
    """``formats`` as a set of names out of ``allowed``: ValueError otherwise."""
    names = (formats,) if isinstance(formats, str) else tuple(formats)
    for name in names:
        if name not in allowed:
            raise ValueError(f"bad Blosc format for {what}: {name!r}; expected names out of {allowed}")
    return set(names)


def decompress_many(frames, outs=None, *, formats=("lz4",)):
    """Decompress a list of Blosc frames with one plan launch and one decode
    launch for all of them (plus one unshuffle launch per shuffled frame).

    ``formats`` names the Blosc compressors the call may meet, out of
    :data:`DECODE_FORMATS`; memcpyed frames are always decoded.  A frame of
    another compressor raises NotImplementedError before any launch.  A batch
    that holds a zlib or zstd frame (and may hold lz4 and memcpyed ones beside
    it) takes one plan launch and one decode launch per format present.

    Each frame is a host buffer or a device tensor; each result is a flat
    uint8 numpy array or device tensor accordingly.  ``outs`` may give, per
    frame, None or a destination (device tensor or writable host buffer) of
    at least ``nbytes`` bytes, which is filled and returned in place of a new
    array.  A malformed frame raises ``RuntimeError('error during blosc
    decompression: -1')`` whose ``frame_errors`` names the rejected frames."""
    allowed = {_FORMAT_CODES[name] for name in _check_formats(formats, DECODE_FORMATS, "decompression")}
    frames = list(frames)
    nf = len(frames)
    outs = [None] * nf if outs is None else list(outs)
    if len(outs) != nf:
        raise ValueError("outs must have one entry per frame")
    if nf == 0:
        return []
    srcs = [_flat_bytes(f) for f in frames]
    on_dev = [is_device_tensor(s) for s in srcs]
    device = _frames.batch_device(srcs, on_dev, outs, "frames")
    lengths = [int(len(s)) for s in srcs]
    short = {i: (-1, 0) for i in range(nf) if lengths[i] < _HEADER}
    if short:
        raise _decode_error(short)
    headers = [_parse_header(h) for h in _frames.read_prefixes(srcs, on_dev, _HEADER)]

    # ---- host checks (before anything is launched) ----
    bad, unsupported = {}, None
    for i, (version, flags, typesize, nbytes, blocksize, cbytes) in enumerate(headers):
        if (version != 2 or cbytes != lengths[i] or typesize < 1 or nbytes > Blosc.max_buffer_size
                or (nbytes > 0 and not 1 <= blocksize <= _MAX_BLOCKSIZE)):
            bad[i] = (-1, 0)
        elif not flags & _F_MEMCPYED and flags >> 5 not in allowed and unsupported is None:
            unsupported = flags >> 5
    if bad:
        raise _decode_error(bad)
    if unsupported is not None:
        name = _FORMAT_NAMES.get(unsupported, f"format {unsupported}")
        can = " / ".join({_FORMAT_LZ4: "lz4 / lz4hc", _FORMAT_ZLIB: "zlib", _FORMAT_ZSTD: "zstd"}[f] for f in sorted(allowed))
        hint = "" if allowed >= set(_FORMAT_CODES.values()) or unsupported not in _FORMAT_CODES.values() else \
            "; allow more with formats=DECODE_FORMATS"
        raise NotImplementedError(f"Blosc frames compressed with {name!r} are not decoded on the GPU "
                                  f"(only {can} and memcpyed frames are{hint})" if allowed != {_FORMAT_LZ4} else
                                  f"Blosc frames compressed with {name!r} are not decoded on the GPU "
                                  "(only lz4 / lz4hc and memcpyed frames are)")
    sizes = [h[3] for h in headers]
    out_raw = [None if o is None else _frames.out_bytes(o, sizes[i]) for i, o in enumerate(outs)]
    _frames.check_out_device(out_raw, device)

    live = [i for i in range(nf) if sizes[i] > 0]
    results = [None] * nf
    for i in range(nf):
        if sizes[i] == 0:  # nothing to decode: no launch
            if out_raw[i] is not None:
                results[i] = outs[i]
            else:
                results[i] = torch.empty(0, dtype=torch.uint8, device=device) if on_dev[i] else np.empty(0, np.uint8)
    if not live:
        return results

    with _frames.launching(device) as (device, st):
        src_all, offsets = _frames.stage_packed(srcs, lengths, on_dev, device)
        own, own_off, final = _frames.place(live, sizes, out_raw, device)
        # frames that still need the inverse shuffle decode into a temporary first
        shuffled = [i for i in live if _mode(headers[i][1], headers[i][2]) != NOSHUFFLE]
        tmp_off, tmp_total = _frames.slot_map(shuffled, [sizes[i] for i in shuffled])
        tmp = torch.empty(tmp_total, dtype=torch.uint8, device=device)
        # a batch with a zlib or zstd frame goes through mc_blosc_decode_batch_z; memcpyed frames count as lz4
        fmt = {i: _FORMAT_LZ4 if headers[i][1] & _F_MEMCPYED else headers[i][1] >> 5 for i in live}
        mixed = any(f != _FORMAT_LZ4 for f in fmt.values())
        table = np.zeros(len(live), dtype=_FRAME_RECORD_Z if mixed else _FRAME_RECORD)
        nblocks = nstreams = lit_bytes = 0
        longest = {_FORMAT_LZ4: 0, _FORMAT_ZLIB: 0, _FORMAT_ZSTD: 0}
        for k, i in enumerate(live):
            _v, flags, typesize, nbytes, blocksize, _c = headers[i]
            b, s, m = _nstreams(flags, typesize, nbytes, blocksize)
            dst = tmp.data_ptr() + tmp_off[i] if i in tmp_off else final[i].data_ptr()
            rec = (offsets[i], lengths[i], dst, nbytes, blocksize, typesize, flags, nblocks, nstreams)
            if mixed:
                rec += (lit_bytes,)
                if fmt[i] == _FORMAT_ZSTD:  # the literals of its streams: nbytes bytes (include/mcodec.h)
                    lit_bytes += -(-nbytes // 16) * 16
            table[k] = rec
            nblocks, nstreams, longest[fmt[i]] = nblocks + b, nstreams + s, max(longest[fmt[i]], m)
        if nblocks > 2**31 - 1 or nstreams > 2**31 - 1:
            raise ValueError("too many Blosc blocks in one batch")
        table_d = upload(table.view(np.uint8), device)
        err = torch.empty(2 * len(live), dtype=torch.int32, device=device)
        if mixed:
            ws_bytes = lib.mc_blosc_decode_batch_z_workspace(nstreams, lit_bytes)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
            check(lib.mc_blosc_decode_batch_z(src_all.data_ptr(), table_d.data_ptr(), len(live), nblocks, nstreams,
                                              longest[_FORMAT_LZ4], longest[_FORMAT_ZLIB], longest[_FORMAT_ZSTD],
                                              lit_bytes, ws.data_ptr(), ws_bytes, err.data_ptr(), st),
                  "mc_blosc_decode_batch_z")
        else:
            ws_bytes = lib.mc_blosc_decode_workspace(nstreams)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
            check(lib.mc_blosc_decode_batch(src_all.data_ptr(), table_d.data_ptr(), len(live), nblocks, nstreams,
                                            longest[_FORMAT_LZ4], ws.data_ptr(), ws_bytes, err.data_ptr(), st),
                  "mc_blosc_decode_batch")
        for i in shuffled:  # one unshuffle launch per frame (a known limit: DESIGN.md §6b)
            _v, flags, typesize, nbytes, blocksize, _c = headers[i]
            check(lib.mc_blosc_filter(tmp.data_ptr() + tmp_off[i], final[i].data_ptr(), nbytes, typesize,
                                      blocksize, _mode(flags, typesize), 0, st), "mc_blosc_filter")
        codes = err.cpu().numpy().reshape(-1, 2)  # waits for the stream
        if codes[:, 0].any():
            raise _decode_error({live[k]: (int(c), int(s)) for k, (c, s) in enumerate(codes) if c})
        _frames.hand_back(results, own, own_off, final, live, sizes, outs, out_raw, on_dev)
    return results


def decompress(source, dest=None, *, formats=("lz4",)):
    """Decompress one Blosc frame (blosc.pyx:274-326): a host buffer gives a
    uint8 numpy array, a device tensor a uint8 device tensor; ``dest``, when
    given, is filled and returned.  ``formats``: see :func:`decompress_many`."""
    return decompress_many([source], [dest], formats=formats)[0]


# ---------------------------------------------------------------------------
# compression
# ---------------------------------------------------------------------------
_COMPRESSORS = ["blosclz", "lz4", "lz4hc", "snappy", "zlib", "zstd"]
_MAX_OVERHEAD = 16  # the reference's BLOSC_MAX_OVERHEAD: a frame never exceeds nbytes + 16
_MIN_BLOCKSIZE = 128
_L1 = 32768
_ZSTD_SEGMENT = 65536  # csrc/mc_zstd_enc.h: MC_ZE_SEGMENT

# one record of mc_blosc_encode_batch's frame table (include/mcodec.h)
_ENC_RECORD = np.dtype([("src", "<u8"), ("raw", "<u8"), ("dst", "<u8"), ("scratch_off", "<u8"), ("nbytes", "<u4"),
                        ("blocksize", "<u4"), ("typesize", "<u4"), ("flags", "<u4"), ("block_base", "<u4"),
                        ("stream_base", "<u4")])
assert _ENC_RECORD.itemsize == 56


def _splits(typesize, blocksize):
    """Would a full block of this size be split into typesize streams?"""
    return typesize <= 16 and blocksize // typesize >= 128


def _blocksize(nbytes, typesize, clevel, blocksize, split=True):
    """The frame's blocksize (nbytes >= 1).

    Forced (``blocksize`` != AUTOBLOCKS): at least 128, at most nbytes, rounded
    down to a multiple of typesize -- 255 for typesize 3 and blocksize 256, as
    in the reference's fixture frames.

    Automatic: c-blosc is absent here (an empty submodule of the reference), so
    the rule is pinned only by those fixtures and by numcodecs' documented
    defaults.  A buffer below 32 KiB (the L1 size c-blosc assumes) is one
    block.  Otherwise 32 KiB is scaled by clevel (0: 1/4, 1: 1/2, 2: 1, 3: 2,
    4-5: 4, 6-9: 8); then, if clevel > 0 and blocks of that size would be
    split into typesize streams, the size is meant per stream: it is clamped
    to 256 KiB, multiplied by typesize and clamped to 64 KiB .. 1 MiB.  The
    result is at most nbytes and a multiple of typesize: 512 KiB for a 1 MiB
    float32 chunk at clevel 5, 8000 for the fixtures' 8000-byte arrays.
    ``split=False`` (zstd: its blocks are never split) leaves the split clause
    out: 128 KiB for that chunk."""
    if blocksize != AUTOBLOCKS:
        bs = max(int(blocksize), _MIN_BLOCKSIZE)
    elif nbytes < _L1:
        bs = nbytes
    else:
        num, den = {0: (1, 4), 1: (1, 2), 2: (1, 1), 3: (2, 1), 4: (4, 1), 5: (4, 1)}.get(clevel, (8, 1))
        bs = _L1 * num // den
        if clevel > 0 and split and _splits(typesize, bs):
            bs = min(bs, 256 * 1024) * typesize
            bs = min(max(bs, 64 * 1024), 1024 * 1024)
    bs = min(bs, nbytes)
    if bs > typesize:
        bs = bs // typesize * typesize
    return bs


def _frame_params(nbytes, itemsize, clevel, shuffle, blocksize, fmt=_FORMAT_LZ4):
    """(flags, blocksize, typesize, filter mode) of the frame of an
    ``nbytes``-byte buffer: version 2, versionlz 1, format bits 1 (lz4) or 4
    (zstd); bit 0 / bit 2 name the shuffle; bit 4 (do-not-split) is set exactly
    when a full block would not be split (typesize > 16 or blocksize / typesize
    < 128), and always for zstd, as c-blosc sets it: one stream per block;
    bit 1 (memcpyed) when clevel is 0.  A typesize above 255 is written as 1,
    as c-blosc does.  ``shuffle`` is already resolved (no AUTOSHUFFLE)."""
    typesize = itemsize if itemsize <= 255 else 1
    flags = fmt << 5
    if fmt == _FORMAT_ZSTD:
        flags |= _F_NOSPLIT
    if shuffle == SHUFFLE:
        flags |= _F_SHUFFLE
    elif shuffle == BITSHUFFLE:
        flags |= _F_BITSHUFFLE
    if nbytes == 0:  # the 16-byte frame: no block, blocksize 1
        return flags, 1, typesize, NOSHUFFLE
    bs = _blocksize(nbytes, typesize, clevel, blocksize, split=fmt != _FORMAT_ZSTD)
    if not _splits(typesize, bs):
        flags |= _F_NOSPLIT
    if clevel == 0:
        flags |= _F_MEMCPYED
    mode = NOSHUFFLE if clevel == 0 or (shuffle == SHUFFLE and typesize == 1) else shuffle
    return flags, bs, typesize, mode


def _header_bytes(flags, typesize, nbytes, blocksize, cbytes):
    return bytes([2, 1, flags, typesize]) + int(nbytes).to_bytes(4, "little") + \
        int(blocksize).to_bytes(4, "little") + int(cbytes).to_bytes(4, "little")


def _check_compress_args(cname, clevel, shuffle, typesize, formats=("lz4",)):
    """The host checks of :func:`compress`, before any buffer is looked at;
    returns the format bits of ``cname``."""
    allowed = _check_formats(formats, ENCODE_FORMATS, "compression")
    name = cname.decode("ascii") if isinstance(cname, (bytes, bytearray)) else cname
    if name not in _COMPRESSORS:
        raise ValueError("bad compressor or compressor not supported: %r; expected one of %s" % (name, _COMPRESSORS))
    if name not in allowed:
        only = " and ".join(repr(n) for n in ENCODE_FORMATS if n in allowed)  # the default: "only 'lz4' is", as before
        raise NotImplementedError(f"Blosc compression with {name!r} is not built in numcodecs_amd (only {only} "
                                  f"{'is' if len(allowed) == 1 else 'are'})")
    if isinstance(typesize, int) and typesize < 1:
        raise ValueError(f"Cannot use typesize {typesize} less than 1.")
    if shuffle not in (AUTOSHUFFLE, NOSHUFFLE, SHUFFLE, BITSHUFFLE):
        raise ValueError("invalid shuffle argument; expected -1, 0, 1 or 2, found %r" % shuffle)
    if not 0 <= int(clevel) <= 9:
        raise RuntimeError("error during blosc compression: -10")  # c-blosc's code for a bad clevel
    return _FORMAT_CODES[name]


def compress_many(sources, cname="lz4", clevel=5, shuffle=SHUFFLE, blocksize=AUTOBLOCKS, typesize=None, *,
                  formats=("lz4",)):
    """Compress a list of buffers to Blosc1 LZ4 frames with three launches for
    all of them (plus one shuffle launch per shuffled frame), or, with
    ``cname='zstd'`` and ``formats=ENCODE_FORMATS``, to Blosc1 zstd frames with
    eight: the chunk table, the Zstandard encoder's parse / code / layout /
    emit, the bridge to the streams' sizes, then the same layout and gather.

    A zstd frame is version 2, versionlz 1, format bits 4 with the do-not-split
    bit always set: one stream per block, every stream one Zstandard frame (64
    KiB segments, Frame_Content_Size declared, no checksum; no matches across
    segments) or, where that would not be smaller than the block, the block's
    bytes stored raw.  The frames are valid for any Blosc reader and byte-equal
    to the host model (tests/native_blosc_z); they are not c-blosc's bytes.
    The automatic blocksize is this package's rule without the split clause;
    above 32 KiB it is not claimed to equal c-blosc's (its source is absent
    and no fixture pins it).

    Each source is a host buffer or a device tensor.  A device tensor gives a
    uint8 device tensor of exactly ``cbytes`` bytes (a view of the frame's
    ``nbytes + 16``-byte slot), a host buffer a uint8 numpy array.  The
    results' lengths are data dependent, so every call reads the frames'
    ``cbytes`` back: one small device-to-host copy and a stream wait per batch.

    ``clevel`` 0 stores the data (memcpyed frames); 1-9 only change the
    automatic blocksize: the match finder has no levels.  ``typesize`` defaults
    to each buffer's itemsize.  Checks of the arguments and sizes come before
    any launch and raise the same on a machine without a GPU.  ``formats``
    names the Blosc compressors the call may use, out of
    :data:`ENCODE_FORMATS`; another name is a ValueError, and a ``cname``
    outside ``formats`` (zstd by default; blosclz, lz4hc, snappy and zlib
    always) raises NotImplementedError."""
    fmt = _check_compress_args(cname, clevel, shuffle, typesize, formats)
    clevel = int(clevel)
    sources = list(sources)
    nf = len(sources)
    if nf == 0:
        return []
    srcs, params = [], []
    for buf in sources:
        arr = ensure_contiguous_ndarray(buf, Blosc.max_buffer_size)
        itemsize = typesize if isinstance(typesize, int) else \
            (arr.element_size() if isinstance(arr, torch.Tensor) else arr.dtype.itemsize)
        mode = shuffle if shuffle != AUTOSHUFFLE else (BITSHUFFLE if itemsize == 1 else SHUFFLE)
        flat = _flat_bytes(arr)
        srcs.append(flat)
        params.append(_frame_params(int(len(flat)), itemsize, clevel, mode, blocksize, fmt))
    on_dev = [is_device_tensor(s) for s in srcs]
    device = _frames.batch_device(srcs, on_dev, what="buffers")
    lengths = [int(len(s)) for s in srcs]
    if any(p[1] > _MAX_BLOCKSIZE for p in params):
        raise ValueError("Blosc block sizes of 2**30 bytes and above are not supported")

    live = [i for i in range(nf) if lengths[i] > 0]
    results = [None] * nf
    for i in range(nf):
        if lengths[i] == 0:  # the 16-byte frame, written on the host
            flags, bs, ts, _m = params[i]
            head = np.frombuffer(_header_bytes(flags, ts, 0, bs, _HEADER), np.uint8).copy()
            results[i] = upload(head, device) if on_dev[i] else head
    if not live:
        return results

    with _frames.launching(device) as (device, st):
        raw = _frames.stage_aligned(srcs, live, on_dev, device)
        # slots: the output (nbytes + 16), a shuffled frame's filtered copy and the compress kernel's scratch (nbytes)
        out_off, out_total = _frames.slot_map(live, [lengths[i] + _MAX_OVERHEAD for i in live])
        shuffled = [i for i in live if params[i][3] != NOSHUFFLE]
        tmp_off, tmp_total = _frames.slot_map(shuffled, [lengths[i] for i in shuffled])
        packed = [i for i in live if not params[i][0] & _F_MEMCPYED]
        scr_off, scr_total = _frames.slot_map(packed, [lengths[i] for i in packed])
        out = torch.empty(out_total, dtype=torch.uint8, device=device)
        tmp = torch.empty(tmp_total, dtype=torch.uint8, device=device)
        table = np.zeros(len(live), dtype=_ENC_RECORD)
        # zstd: every block is one chunk of the Zstandard encoder; its segments (64 KiB) and sequence records (one
        # per 4 bytes) are counted per frame here, per block on the device.  clevel 0 takes the lz4 entry point.
        zstd = fmt == _FORMAT_ZSTD and clevel > 0
        bases = np.zeros((len(live), 2), dtype=np.uint32)
        nblocks = nstreams = nsegs = nseqs = 0
        for k, i in enumerate(live):
            flags, bs, ts, mode = params[i]
            src_ptr = raw[i].data_ptr()
            if i in tmp_off:  # one shuffle launch per frame (a known limit: DESIGN.md §6b)
                src_ptr = tmp.data_ptr() + tmp_off[i]
                check(lib.mc_blosc_filter(raw[i].data_ptr(), src_ptr, lengths[i], ts, bs, mode, 1, st),
                      "mc_blosc_filter")
            b, s, _m = _nstreams(flags, ts, lengths[i], bs)
            table[k] = (src_ptr, raw[i].data_ptr(), out.data_ptr() + out_off[i], scr_off.get(i, 0), lengths[i], bs,
                        ts, flags, nblocks, nstreams)
            nblocks, nstreams = nblocks + b, nstreams + s
            if zstd:
                bases[k] = (nsegs, nseqs)
                last = lengths[i] - (b - 1) * bs
                nsegs += (b - 1) * -(-bs // _ZSTD_SEGMENT) + -(-last // _ZSTD_SEGMENT)
                nseqs += (b - 1) * -(-bs // 4) + -(-last // 4)
                if nseqs > 2**32 - 1:
                    raise ValueError("a Blosc zstd batch holds less than 16 GiB")
        if nblocks > 2**31 - 1 or nstreams > 2**31 - 1:
            raise ValueError("too many Blosc blocks in one batch")
        table_d = upload(table.view(np.uint8), device)
        cbytes_d = torch.empty(len(live), dtype=torch.int32, device=device)
        if zstd:
            bases_d = upload(bases.view(np.uint8).reshape(-1), device)
            ws_bytes = lib.mc_blosc_encode_batch_z_workspace(nstreams, nsegs, nseqs, scr_total)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
            check(lib.mc_blosc_encode_batch_z(None, table_d.data_ptr(), bases_d.data_ptr(), len(live), nblocks, nsegs,
                                              nseqs, ws.data_ptr(), ws_bytes, cbytes_d.data_ptr(), st),
                  "mc_blosc_encode_batch_z")
        else:
            ws_bytes = lib.mc_blosc_encode_workspace(nstreams, scr_total)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
            check(lib.mc_blosc_encode_batch(None, table_d.data_ptr(), len(live), nblocks, nstreams, ws.data_ptr(),
                                            ws_bytes, cbytes_d.data_ptr(), st), "mc_blosc_encode_batch")
        cbytes = cbytes_d.cpu().numpy().view(np.uint32).tolist()  # waits for the stream
        for k, i in enumerate(live):
            if not _HEADER < cbytes[k] <= lengths[i] + _MAX_OVERHEAD:
                raise RuntimeError("error during blosc compression: %d" % (cbytes[k] if cbytes[k] else -1))
        _frames.hand_back_encoded(results, out, out_off, cbytes, live, on_dev)
    return results


def compress(source, cname, clevel, shuffle=SHUFFLE, blocksize=AUTOBLOCKS, typesize=None, *, formats=("lz4",)):
    """Compress one buffer to a Blosc1 LZ4 frame (blosc.pyx:211-326): a device
    tensor gives a uint8 device tensor, a host buffer a uint8 numpy array.  See
    :func:`compress_many` for the one read-back per call."""
    return compress_many([source], cname, clevel, shuffle, blocksize, typesize, formats=formats)[0]


_shuffle_repr = ["AUTOSHUFFLE", "NOSHUFFLE", "SHUFFLE", "BITSHUFFLE"]


class Blosc(Codec):
    """The Blosc meta-compressor's codec (numcodecs id ``blosc``), decode
    only: same constructor, config and repr as the reference (blosc.pyx:448-509).
    ``decode`` handles lz4 / lz4hc and memcpyed frames on the GPU; ``encode``
    raises NotImplementedError (compression is not built)."""

    codec_id = "blosc"
    NOSHUFFLE = NOSHUFFLE
    SHUFFLE = SHUFFLE
    BITSHUFFLE = BITSHUFFLE
    AUTOSHUFFLE = AUTOSHUFFLE
    max_buffer_size = 2**31 - 1

    def __init__(self, cname="lz4", clevel=5, shuffle=SHUFFLE, blocksize=AUTOBLOCKS, typesize=None):
        if isinstance(typesize, int) and typesize < 1:
            raise ValueError(f"Cannot use typesize {typesize} less than 1.")
        self.cname = cname
        self._cname_bytes = cname.encode("ascii") if isinstance(cname, str) else cname
        self.clevel = clevel
        self.shuffle = shuffle
        self.blocksize = blocksize
        self._typesize = typesize

    def encode(self, buf):
        raise NotImplementedError("Blosc compression is not built in numcodecs_amd (decode only); "
                                  "encode with numcodecs.Blosc")

    def decode(self, buf, out=None):
        return decompress(buf, out)

    def __repr__(self):
        return "%s(cname=%r, clevel=%r, shuffle=%s, blocksize=%s)" % (
            type(self).__name__, self.cname, self.clevel, _shuffle_repr[self.shuffle + 1], self.blocksize)


class BloscLZ4(Blosc):
    """The full ``blosc`` codec for ``cname='lz4'``: same constructor, config
    and id as :class:`Blosc`, ``decode`` inherited, ``encode`` compressing on
    the GPU (:func:`compress`).  ``clevel`` 0 stores the data; 1-9 only change
    the automatic blocksize.  Another ``cname`` decodes but raises
    NotImplementedError on ``encode``."""

    def encode(self, buf):
        return compress(buf, self._cname_bytes, self.clevel, self.shuffle, self.blocksize, self._typesize)


class BloscFull(BloscLZ4):
    """The ``blosc`` codec with every format this package decodes: same
    constructor, config, repr form and id as :class:`BloscLZ4`.  ``decode``
    takes lz4 / lz4hc, zlib, zstd and memcpyed frames
    (:data:`DECODE_FORMATS`); ``encode`` uses :data:`ENCODE_FORMATS`: it writes
    lz4 and zstd frames (:func:`compress_many`), and another ``cname`` raises
    NotImplementedError on ``encode``."""

    def encode(self, buf):
        return compress(buf, self._cname_bytes, self.clevel, self.shuffle, self.blocksize, self._typesize,
                        formats=ENCODE_FORMATS)

    def decode(self, buf, out=None):
        return decompress(buf, out, formats=DECODE_FORMATS)


def register(full=False, zstd=False):
    """Register :class:`Blosc` (decode only) or, with ``full=True``,
    :class:`BloscLZ4` under ``'blosc'`` in this package's ``codec_registry``
    (never done on import, and never in numcodecs' own registry: by default a
    decode-only class must not replace the reference's codec).
    ``register(full=True, zstd=True)`` registers :class:`BloscFull`, which
    also decodes zlib and zstd frames; ``zstd=True`` needs ``full=True``."""
    if zstd and not full:
        raise ValueError("register(zstd=True) needs full=True: BloscFull is a full codec")
    register_codec(BloscFull if zstd else BloscLZ4 if full else Blosc)
