"""Blosc decompression on the GPU (reference: src/numcodecs/blosc.pyx:274-326,
448-509): Blosc1 frames whose compressor is LZ4 / LZ4HC, and memcpyed
(stored) frames, become device-resident arrays -- decompressed by
csrc/mc_blosc_dec.hip (one plan launch and one decode launch for a whole
batch of frames) and unshuffled by ``mc_blosc_filter`` (one launch per frame
that carries a shuffle flag).  Compression is not built, and neither are the
other Blosc compressors (blosclz, snappy, zlib, zstd): DESIGN.md §7.

The 16-byte frame header is read on the host: version, versionlz, flags,
typesize, then nbytes, blocksize, cbytes as little-endian u32.  For frames
that are already on the device this costs one small device-to-host copy
(one gathered copy for a whole batch).  Everything after the header --
``bstarts``, the streams' ``cbytes`` words, every LZ4 sequence -- is read and
validated on the device (csrc/mc_lz4.h); a violation comes back in a
per-frame error record and raises ``RuntimeError('error during blosc
decompression: -1')``, the reference's text with c-blosc's generic code.

``Blosc`` is not registered on import (it cannot encode, so it must not
shadow a full codec silently): call :func:`register`.
"""

import numpy as np
import torch

from . import _native
from ._native import check, lib
from .abc import Codec
from .blosc_shuffle import AUTOBLOCKS, AUTOSHUFFLE, BITSHUFFLE, NOSHUFFLE, SHUFFLE
from .compat import device_out, download, ensure_contiguous_ndarray, is_device_tensor, upload
from .registry import register_codec

__all__ = ["Blosc", "NOSHUFFLE", "SHUFFLE", "BITSHUFFLE", "AUTOSHUFFLE", "AUTOBLOCKS", "cbuffer_sizes",
           "decompress", "decompress_many", "register"]

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


def register():
    """Register :class:`Blosc` under ``'blosc'`` in this package's
    ``codec_registry`` (never done on import, and never in numcodecs' own
    registry: a decode-only class must not replace the reference's codec)."""
    register_codec(Blosc)
