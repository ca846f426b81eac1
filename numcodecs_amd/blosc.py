"""Blosc on the GPU (reference: src/numcodecs/blosc.pyx:211-326, 448-509).

Decompression: Blosc1 frames whose compressor is LZ4 / LZ4HC, and memcpyed
(stored) frames, become device-resident arrays -- decompressed by
csrc/mc_blosc_dec.hip (one plan launch and one decode launch for a whole
batch of frames) and unshuffled by ``mc_blosc_filter`` (one launch per frame
that carries a shuffle flag).

Compression (:func:`compress`, :func:`compress_many`, :class:`BloscLZ4`):
buffers become Blosc1 LZ4 frames -- shuffled by ``mc_blosc_filter`` (one
launch per shuffled frame) and compressed, laid out and gathered by
csrc/mc_blosc_enc.hip (three launches for a whole batch).  The frames are
valid Blosc1 LZ4 frames that any Blosc reader decodes; they are not byte-equal
to c-blosc's (the match finder differs).  The other Blosc compressors
(blosclz, lz4hc, snappy, zlib, zstd) are not built: DESIGN.md §7.  The
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
the full codec.  Neither is registered on import: call :func:`register`.
"""

import numpy as np
import torch

from . import _native
from ._native import check, lib
from .abc import Codec
from .blosc_shuffle import AUTOBLOCKS, AUTOSHUFFLE, BITSHUFFLE, NOSHUFFLE, SHUFFLE
from .compat import device_out, download, ensure_contiguous_ndarray, is_device_tensor, upload
from .registry import register_codec

__all__ = ["Blosc", "BloscLZ4", "NOSHUFFLE", "SHUFFLE", "BITSHUFFLE", "AUTOSHUFFLE", "AUTOBLOCKS", "cbuffer_sizes",
           "compress", "compress_many", "decompress", "decompress_many", "register"]

_HEADER = 16
_F_SHUFFLE, _F_MEMCPYED, _F_BITSHUFFLE, _F_NOSPLIT = 0x1, 0x2, 0x4, 0x10
_FORMAT_LZ4 = 1
_FORMAT_NAMES = {0: "blosclz", 1: "lz4", 2: "snappy", 3: "zlib", 4: "zstd"}
_MAX_BLOCKSIZE = (1 << 30) - 1  # mc_blosc_decode_batch refuses more (c-blosc's own limit is lower)
_ERROR_TEXT = "error during blosc decompression: -1"
_ALIGN = 256

# one record of mc_blosc_decode_batch's frame table (include/mcodec.h)
_FRAME_RECORD = np.dtype([("src_off", "<u8"), ("src_len", "<u8"), ("dst", "<u8"), ("nbytes", "<u4"),
                          ("blocksize", "<u4"), ("typesize", "<u4"), ("flags", "<u4"), ("block_base", "<u4"),
                          ("stream_base", "<u4")])
assert _FRAME_RECORD.itemsize == 48


def _decode_error(frame_errors):
    """The reference's RuntimeError; ``frame_errors`` maps the index of each
    rejected frame to (code, stream): code -1 for a failed host check, else
    the device error record's (csrc/mc_lz4.h)."""
    exc = RuntimeError(_ERROR_TEXT)
    exc.frame_errors = dict(frame_errors)
    return exc


def _parse_header(hdr) -> tuple:
    """(version, flags, typesize, nbytes, blocksize, cbytes) of 16 header bytes."""
    h = bytes(hdr)
    return (h[0], h[2], h[3], int.from_bytes(h[4:8], "little"), int.from_bytes(h[8:12], "little"),
            int.from_bytes(h[12:16], "little"))


def _flat_bytes(buf):
    """`buf` as flat uint8: a device tensor stays one, anything else becomes a
    numpy view (ensure_contiguous_ndarray semantics, blosc.pyx:499)."""
    arr = ensure_contiguous_ndarray(buf, Blosc.max_buffer_size)
    if is_device_tensor(arr):
        return arr.view(torch.uint8) if arr.numel() else arr.new_empty(0, dtype=torch.uint8)
    return arr.view(np.uint8)


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


def _out_bytes(out, nbytes):
    """A caller's `out` as flat uint8 (device tensor or numpy), size-checked."""
    flat = ensure_contiguous_ndarray(device_out(out))
    if is_device_tensor(flat):
        raw = flat.view(torch.uint8) if flat.numel() else flat.new_empty(0, dtype=torch.uint8)
        have = raw.numel()
    else:
        if not flat.flags.writeable:
            raise ValueError("destination buffer is read-only")
        raw = flat.view(np.uint8)
        have = raw.nbytes
    if have < nbytes:
        raise ValueError("destination buffer too small; expected at least %s, got %s" % (nbytes, have))
    return raw


def decompress_many(frames, outs=None):
    """Decompress a list of Blosc frames with one plan launch and one decode
    launch for all of them (plus one unshuffle launch per shuffled frame).

    Each frame is a host buffer or a device tensor; each result is a flat
    uint8 numpy array or device tensor accordingly.  ``outs`` may give, per
    frame, None or a destination (device tensor or writable host buffer) of
    at least ``nbytes`` bytes, which is filled and returned in place of a new
    array.  A malformed frame raises ``RuntimeError('error during blosc
    decompression: -1')`` whose ``frame_errors`` names the rejected frames."""
    frames = list(frames)
    nf = len(frames)
    outs = [None] * nf if outs is None else list(outs)
    if len(outs) != nf:
        raise ValueError("outs must have one entry per frame")
    if nf == 0:
        return []
    srcs = [_flat_bytes(f) for f in frames]
    on_dev = [is_device_tensor(s) for s in srcs]
    device = next((s.device for s, d in zip(srcs, on_dev) if d), None)
    for o in outs:
        if device is None and o is not None and is_device_tensor(device_out(o)):
            device = device_out(o).device
    if any(d and s.device != device for s, d in zip(srcs, on_dev)):
        raise ValueError("all frames of a batch must be on one device")

    # ---- the frames' bytes as one device buffer, and their offsets in it ----
    lengths = [int(len(s)) for s in srcs]
    offsets = [0] * nf
    pieces, pos = [], 0
    host_idx = [i for i in range(nf) if not on_dev[i]]
    if host_idx:
        for i in host_idx:
            offsets[i] = pos
            pos += lengths[i]
    for i in range(nf):
        if on_dev[i]:
            offsets[i] = pos
            pos += lengths[i]

    # ---- headers: host frames directly, device frames by one gathered copy ----
    headers = [None] * nf
    short = {i: (-1, 0) for i in range(nf) if lengths[i] < _HEADER}
    if short:
        raise _decode_error(short)
    for i in host_idx:
        headers[i] = _parse_header(srcs[i][:_HEADER])
    dev_idx = [i for i in range(nf) if on_dev[i]]
    if dev_idx:
        heads = torch.cat([srcs[i][:_HEADER] for i in dev_idx]).cpu().numpy().reshape(-1, _HEADER)
        for k, i in enumerate(dev_idx):
            headers[i] = _parse_header(heads[k])

    # ---- host checks (before anything is launched) ----
    bad, unsupported = {}, None
    for i, (version, flags, typesize, nbytes, blocksize, cbytes) in enumerate(headers):
        if (version != 2 or cbytes != lengths[i] or typesize < 1 or nbytes > Blosc.max_buffer_size
                or (nbytes > 0 and not 1 <= blocksize <= _MAX_BLOCKSIZE)):
            bad[i] = (-1, 0)
        elif not flags & _F_MEMCPYED and flags >> 5 != _FORMAT_LZ4 and unsupported is None:
            unsupported = flags >> 5
    if bad:
        raise _decode_error(bad)
    if unsupported is not None:
        name = _FORMAT_NAMES.get(unsupported, f"format {unsupported}")
        raise NotImplementedError(f"Blosc frames compressed with {name!r} are not decoded on the GPU "
                                  "(only lz4 / lz4hc and memcpyed frames are)")
    out_raw = [None if o is None else _out_bytes(o, headers[i][3]) for i, o in enumerate(outs)]
    if any(is_device_tensor(o) and o.device != device for o in out_raw if o is not None) and device is not None:
        raise ValueError("out must be on the same device as the frames")

    live = [i for i in range(nf) if headers[i][3] > 0]
    results = [None] * nf
    for i in range(nf):
        if headers[i][3] == 0:  # nothing to decode: no launch
            if out_raw[i] is not None:
                results[i] = outs[i]
            elif on_dev[i]:
                results[i] = torch.empty(0, dtype=torch.uint8, device=device)
            else:
                results[i] = np.empty(0, dtype=np.uint8)
    if not live:
        return results

    _native.require_device()
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    from ._ops import _guard, stream

    with _guard(torch.empty(0, dtype=torch.uint8, device=device)):
        if host_idx:
            blob = np.concatenate([srcs[i] for i in host_idx]) if len(host_idx) > 1 else srcs[host_idx[0]]
            pieces.append(upload(np.ascontiguousarray(blob), device))
        pieces.extend(srcs[i] for i in dev_idx)
        src_all = pieces[0] if len(pieces) == 1 else torch.cat(pieces)

        # ---- where each frame's bytes go: its final place, and -- for frames
        # that still need the inverse shuffle -- a temporary before that
        def _mode(flags, typesize):
            if flags & _F_MEMCPYED:
                return NOSHUFFLE
            if flags & _F_BITSHUFFLE:
                return BITSHUFFLE
            return SHUFFLE if flags & _F_SHUFFLE and typesize > 1 else NOSHUFFLE

        own_off, own_total, tmp_off, tmp_total = {}, 0, {}, 0
        for i in live:
            nbytes = headers[i][3]
            if not is_device_tensor(out_raw[i]):
                own_off[i] = own_total
                own_total += -(-nbytes // _ALIGN) * _ALIGN
            if _mode(headers[i][1], headers[i][2]) != NOSHUFFLE:
                tmp_off[i] = tmp_total
                tmp_total += -(-nbytes // _ALIGN) * _ALIGN
        own = torch.empty(own_total, dtype=torch.uint8, device=device)
        tmp = torch.empty(tmp_total, dtype=torch.uint8, device=device)
        final = {i: (own[own_off[i]:own_off[i] + headers[i][3]] if i in own_off else out_raw[i][:headers[i][3]])
                 for i in live}

        table = np.zeros(len(live), dtype=_FRAME_RECORD)
        nblocks = nstreams = longest = 0
        for k, i in enumerate(live):
            _v, flags, typesize, nbytes, blocksize, _c = headers[i]
            b, s, m = _nstreams(flags, typesize, nbytes, blocksize)
            dst = tmp.data_ptr() + tmp_off[i] if i in tmp_off else final[i].data_ptr()
            table[k] = (offsets[i], lengths[i], dst, nbytes, blocksize, typesize, flags, nblocks, nstreams)
            nblocks, nstreams, longest = nblocks + b, nstreams + s, max(longest, m)
        if nblocks > 2**31 - 1 or nstreams > 2**31 - 1:
            raise ValueError("too many Blosc blocks in one batch")
        table_d = upload(table.view(np.uint8), device)
        ws_bytes = lib.mc_blosc_decode_workspace(nstreams)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
        err = torch.empty(2 * len(live), dtype=torch.int32, device=device)
        st = stream(src_all)
        check(lib.mc_blosc_decode_batch(src_all.data_ptr(), table_d.data_ptr(), len(live), nblocks, nstreams,
                                        longest, ws.data_ptr(), ws_bytes, err.data_ptr(), st),
              "mc_blosc_decode_batch")
        for i in tmp_off:  # one unshuffle launch per frame (a known limit: DESIGN.md §6b)
            _v, flags, typesize, nbytes, blocksize, _c = headers[i]
            check(lib.mc_blosc_filter(tmp.data_ptr() + tmp_off[i], final[i].data_ptr(), nbytes, typesize, blocksize,
                                      _mode(flags, typesize), 0, st), "mc_blosc_filter")
        codes = err.cpu().numpy().reshape(-1, 2)  # waits for the stream
        if codes[:, 0].any():
            raise _decode_error({live[k]: (int(c), int(s)) for k, (c, s) in enumerate(codes) if c})
        host_all = download(own) if any(not on_dev[i] or isinstance(out_raw[i], np.ndarray) for i in own_off) \
            else None
        for i in live:
            nbytes = headers[i][3]
            if is_device_tensor(out_raw[i]):
                results[i] = outs[i]
            elif out_raw[i] is not None:  # a host destination
                out_raw[i][:nbytes] = host_all[own_off[i]:own_off[i] + nbytes]
                results[i] = outs[i]
            elif on_dev[i]:
                results[i] = final[i]
            else:
                results[i] = host_all[own_off[i]:own_off[i] + nbytes]
    return results


def decompress(source, dest=None):
    """Decompress one Blosc frame (blosc.pyx:274-326): a host buffer gives a
    uint8 numpy array, a device tensor a uint8 device tensor; ``dest``, when
    given, is filled and returned."""
    return decompress_many([source], [dest])[0]


# ---------------------------------------------------------------------------
# compression
# ---------------------------------------------------------------------------
_COMPRESSORS = ["blosclz", "lz4", "lz4hc", "snappy", "zlib", "zstd"]
_MAX_OVERHEAD = 16  # the reference's BLOSC_MAX_OVERHEAD: a frame never exceeds nbytes + 16
_MIN_BLOCKSIZE = 128
_L1 = 32768

# one record of mc_blosc_encode_batch's frame table (include/mcodec.h)
_ENC_RECORD = np.dtype([("src", "<u8"), ("raw", "<u8"), ("dst", "<u8"), ("scratch_off", "<u8"), ("nbytes", "<u4"),
                        ("blocksize", "<u4"), ("typesize", "<u4"), ("flags", "<u4"), ("block_base", "<u4"),
                        ("stream_base", "<u4")])
assert _ENC_RECORD.itemsize == 56


def _splits(typesize, blocksize):
    """Would a full block of this size be split into typesize streams?"""
    return typesize <= 16 and blocksize // typesize >= 128


def _blocksize(nbytes, typesize, clevel, blocksize):
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
    float32 chunk at clevel 5, 8000 for the fixtures' 8000-byte arrays."""
    if blocksize != AUTOBLOCKS:
        bs = max(int(blocksize), _MIN_BLOCKSIZE)
    elif nbytes < _L1:
        bs = nbytes
    else:
        num, den = {0: (1, 4), 1: (1, 2), 2: (1, 1), 3: (2, 1), 4: (4, 1), 5: (4, 1)}.get(clevel, (8, 1))
        bs = _L1 * num // den
        if clevel > 0 and _splits(typesize, bs):
            bs = min(bs, 256 * 1024) * typesize
            bs = min(max(bs, 64 * 1024), 1024 * 1024)
    bs = min(bs, nbytes)
    if bs > typesize:
        bs = bs // typesize * typesize
    return bs


def _frame_params(nbytes, itemsize, clevel, shuffle, blocksize):
    """(flags, blocksize, typesize, filter mode) of the frame of an
    ``nbytes``-byte buffer: version 2, versionlz 1, format bits 1 (lz4); bit 0
    / bit 2 name the shuffle; bit 4 (do-not-split) is set exactly when a full
    block would not be split (typesize > 16 or blocksize / typesize < 128);
    bit 1 (memcpyed) when clevel is 0.  A typesize above 255 is written as 1,
    as c-blosc does.  ``shuffle`` is already resolved (no AUTOSHUFFLE)."""
    typesize = itemsize if itemsize <= 255 else 1
    flags = _FORMAT_LZ4 << 5
    if shuffle == SHUFFLE:
        flags |= _F_SHUFFLE
    elif shuffle == BITSHUFFLE:
        flags |= _F_BITSHUFFLE
    if nbytes == 0:  # the 16-byte frame: no block, blocksize 1
        return flags, 1, typesize, NOSHUFFLE
    bs = _blocksize(nbytes, typesize, clevel, blocksize)
    if not _splits(typesize, bs):
        flags |= _F_NOSPLIT
    if clevel == 0:
        flags |= _F_MEMCPYED
    mode = NOSHUFFLE if clevel == 0 or (shuffle == SHUFFLE and typesize == 1) else shuffle
    return flags, bs, typesize, mode


def _header_bytes(flags, typesize, nbytes, blocksize, cbytes):
    return bytes([2, 1, flags, typesize]) + int(nbytes).to_bytes(4, "little") + \
        int(blocksize).to_bytes(4, "little") + int(cbytes).to_bytes(4, "little")


def _check_compress_args(cname, clevel, shuffle, typesize):
    """The host checks of :func:`compress`, before any buffer is looked at."""
    name = cname.decode("ascii") if isinstance(cname, (bytes, bytearray)) else cname
    if name not in _COMPRESSORS:
        raise ValueError("bad compressor or compressor not supported: %r; expected one of %s" % (name, _COMPRESSORS))
    if name != "lz4":
        raise NotImplementedError(f"Blosc compression with {name!r} is not built in numcodecs_amd (only 'lz4' is)")
    if isinstance(typesize, int) and typesize < 1:
        raise ValueError(f"Cannot use typesize {typesize} less than 1.")
    if shuffle not in (AUTOSHUFFLE, NOSHUFFLE, SHUFFLE, BITSHUFFLE):
        raise ValueError("invalid shuffle argument; expected -1, 0, 1 or 2, found %r" % shuffle)
    if not 0 <= int(clevel) <= 9:
        raise RuntimeError("error during blosc compression: -10")  # c-blosc's code for a bad clevel


def compress_many(sources, cname="lz4", clevel=5, shuffle=SHUFFLE, blocksize=AUTOBLOCKS, typesize=None):
    """Compress a list of buffers to Blosc1 LZ4 frames with three launches for
    all of them (plus one shuffle launch per shuffled frame).

    Each source is a host buffer or a device tensor.  A device tensor gives a
    uint8 device tensor of exactly ``cbytes`` bytes (a view of the frame's
    ``nbytes + 16``-byte slot), a host buffer a uint8 numpy array.  The
    results' lengths are data dependent, so every call reads the frames'
    ``cbytes`` back: one small device-to-host copy and a stream wait per batch.

    ``clevel`` 0 stores the data (memcpyed frames); 1-9 only change the
    automatic blocksize: the match finder has no levels.  ``typesize`` defaults
    to each buffer's itemsize.  Checks of the arguments and sizes come before
    any launch and raise the same on a machine without a GPU."""
    _check_compress_args(cname, clevel, shuffle, typesize)
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
        params.append(_frame_params(int(len(flat)), itemsize, clevel, mode, blocksize))
    on_dev = [is_device_tensor(s) for s in srcs]
    device = next((s.device for s, d in zip(srcs, on_dev) if d), None)
    if any(d and s.device != device for s, d in zip(srcs, on_dev)):
        raise ValueError("all buffers of a batch must be on one device")
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

    _native.require_device()
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    from ._ops import _guard, stream

    with _guard(torch.empty(0, dtype=torch.uint8, device=device)):
        # ---- the inputs on the device: host buffers by one upload ----
        host_idx = [i for i in live if not on_dev[i]]
        raw = {i: srcs[i] for i in live if on_dev[i]}
        if host_idx:
            offs = np.cumsum([0] + [-(-lengths[i] // _ALIGN) * _ALIGN for i in host_idx])
            blob = np.zeros(int(offs[-1]), np.uint8)
            for k, i in enumerate(host_idx):
                blob[offs[k]:offs[k] + lengths[i]] = srcs[i]
            blob_d = upload(blob, device)
            for k, i in enumerate(host_idx):
                raw[i] = blob_d[int(offs[k]):int(offs[k]) + lengths[i]]

        # ---- slots: the output (nbytes + 16 each), the filtered copy of a
        # shuffled frame, and the compress kernel's scratch (nbytes each)
        def _up(n):
            return -(-n // _ALIGN) * _ALIGN

        out_off, tmp_off, scr_off = {}, {}, {}
        out_total = tmp_total = scr_total = 0
        for i in live:
            out_off[i], out_total = out_total, out_total + _up(lengths[i] + _MAX_OVERHEAD)
            if params[i][3] != NOSHUFFLE:
                tmp_off[i], tmp_total = tmp_total, tmp_total + _up(lengths[i])
            if not params[i][0] & _F_MEMCPYED:
                scr_off[i], scr_total = scr_total, scr_total + _up(lengths[i])
        out = torch.empty(out_total, dtype=torch.uint8, device=device)
        tmp = torch.empty(tmp_total, dtype=torch.uint8, device=device)
        st = stream(out)
        table = np.zeros(len(live), dtype=_ENC_RECORD)
        nblocks = nstreams = 0
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
        if nblocks > 2**31 - 1 or nstreams > 2**31 - 1:
            raise ValueError("too many Blosc blocks in one batch")
        table_d = upload(table.view(np.uint8), device)
        ws_bytes = lib.mc_blosc_encode_workspace(nstreams, scr_total)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
        cbytes_d = torch.empty(len(live), dtype=torch.int32, device=device)
        check(lib.mc_blosc_encode_batch(None, table_d.data_ptr(), len(live), nblocks, nstreams, ws.data_ptr(),
                                        ws_bytes, cbytes_d.data_ptr(), st), "mc_blosc_encode_batch")
        cbytes = cbytes_d.cpu().numpy().view(np.uint32)  # waits for the stream
        for k, i in enumerate(live):
            if not _HEADER < cbytes[k] <= lengths[i] + _MAX_OVERHEAD:
                raise RuntimeError("error during blosc compression: %d" % (cbytes[k] if cbytes[k] else -1))
        host_all = download(out) if host_idx else None
        for k, i in enumerate(live):
            lo, hi = out_off[i], out_off[i] + int(cbytes[k])
            results[i] = out[lo:hi] if on_dev[i] else host_all[lo:hi]
    return results


def compress(source, cname, clevel, shuffle=SHUFFLE, blocksize=AUTOBLOCKS, typesize=None):
    """Compress one buffer to a Blosc1 LZ4 frame (blosc.pyx:211-326): a device
    tensor gives a uint8 device tensor, a host buffer a uint8 numpy array.  See
    :func:`compress_many` for the one read-back per call."""
    return compress_many([source], cname, clevel, shuffle, blocksize, typesize)[0]


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


def register(full=False):
    """Register :class:`Blosc` (decode only) or, with ``full=True``,
    :class:`BloscLZ4` under ``'blosc'`` in this package's ``codec_registry``
    (never done on import, and never in numcodecs' own registry: by default a
    decode-only class must not replace the reference's codec)."""
    register_codec(BloscLZ4 if full else Blosc)
