"""Batched inflate on the GPU: what :mod:`.zlib` and :mod:`.gzip` share.

A frame's decoded size is not written in a zlib stream, and gzip's ISIZE is a
claim to check, not to trust.  So a frame that comes with a destination or a
size takes three launches per batch (plan, decode, check: csrc/mc_inflate.hip)
and one read-back of the error and produced words; a frame with neither first
goes through the sizing launch (the same DEFLATE chain with no stores), which
adds one launch pair and one small read-back per batch, and its destination is
allocated from that.  One frame is one serial chain on one wave: throughput
comes from the batch.

Exceptions are the stdlib's own classes with ``frame_errors`` attached
({frame index: (code, second word)}, the device error record of
csrc/mc_inflate.h; code -1 for a host check): ``zlib.error`` for every
rejected zlib frame, with the text ``zlib.decompress`` gives for the
condition; for gzip ``gzip.BadGzipFile`` (magic, method, CRC, length, junk),
``EOFError`` (truncation), ``zlib.error`` (a fault inside the DEFLATE data) and
``NotImplementedError`` for a further member, which the reference would
concatenate.  Output that does not fit a given destination or size is a
``ValueError``.

Staging, placing and handing back is :mod:`numcodecs_amd._frames`."""

import gzip as _gzip
import zlib as _zlib

import numpy as np
import torch

from . import _frames
from ._native import check, lib
from .compat import is_device_tensor, upload

ZLIB, GZIP = 0, 1
_MAX_BYTES = 1 << 30  # csrc/mc_inflate.h MC_INF_MAX_BYTES: frames and outputs are shorter
_MAX_BUFFER = 0x7FFFFFFF

# one record of the frame table (include/mcodec.h)
_RECORD = np.dtype([("src_off", "<u8"), ("src_len", "<u8"), ("dst", "<u8"), ("capacity", "<u4"), ("container", "<u4")])
assert _RECORD.itemsize == 32

# csrc/mc_inflate.h mc_inf_error
E_HEADER, E_METHOD, E_WINDOW, E_DICT, E_GZ_MAGIC, E_GZ_METHOD, E_GZ_FLAGS, E_TRUNCATED = range(1, 9)
E_CAPACITY, E_CHECK, E_LENGTH, E_GZ_JUNK, E_GZ_MEMBER, E_TABLE = 20, 21, 22, 23, 24, 25

# zlib's message for each condition (inflate.c), as zlib.decompress words it
_ZLIB_TEXT = {
    E_HEADER: "incorrect header check",
    E_METHOD: "unknown compression method",
    E_WINDOW: "invalid window size",
    9: "invalid block type",
    10: "invalid stored block lengths",
    11: "too many length or distance symbols",
    12: "invalid code lengths set",
    13: "invalid bit length repeat",
    14: "invalid literal/lengths set",
    15: "invalid distances set",
    16: "invalid code -- missing end-of-block",
    17: "invalid literal/length code",
    18: "invalid distance code",
    19: "invalid distance too far back",
    E_CHECK: "incorrect data check",
}
_EOF_TEXT = "Compressed file ended before the end-of-stream marker was reached"


def _too_long(n):
    return ValueError("zlib / gzip frames and outputs of 2**30 bytes and above are not supported on the GPU; got %d" % n)


def _exception(container, code, word, frame, capacity):
    """The stdlib's exception for error record (code, word) of frame `frame`."""
    if code == E_CAPACITY:
        if capacity is None:
            return _too_long(_MAX_BYTES)
        if container == GZIP:
            return ValueError("Unable to fit data into `out`")
        return ValueError("frame %d decodes to more than the %d bytes given for it" % (frame, capacity))
    if code == E_TABLE:
        return ValueError("frame %d: the frame record is out of range" % frame)
    if container == GZIP:
        if code == E_TRUNCATED:
            return EOFError(_EOF_TEXT)
        if code == E_GZ_MAGIC:
            return _gzip.BadGzipFile("Not a gzipped file")
        if code == E_GZ_METHOD:
            return _gzip.BadGzipFile("Unknown compression method")
        if code == E_CHECK:
            return _gzip.BadGzipFile("CRC check failed: computed %s" % hex(word & 0xFFFFFFFF))
        if code == E_LENGTH:
            return _gzip.BadGzipFile("Incorrect length of data produced")
        if code == E_GZ_JUNK:
            return _gzip.BadGzipFile("Not a gzipped file (trailing bytes after the member)")
        if code == E_GZ_MEMBER:
            return NotImplementedError("gzip frames of more than one member are not supported on the GPU")
    if code == E_TRUNCATED:
        return _zlib.error("Error -5 while decompressing data: incomplete or truncated stream")
    if code == E_DICT:
        return _zlib.error("Error 2 while decompressing data")
    return _zlib.error("Error -3 while decompressing data: %s" % _ZLIB_TEXT.get(code, "code %d" % code))


def _raise(container, errors, capacities):
    first = min(errors)
    exc = _exception(container, *errors[first], first, capacities.get(first))
    exc.frame_errors = dict(errors)
    raise exc


def _records(codes):
    """{index: (code, second word)} of the non-zero rows of a device error record."""
    return {i: (int(c), int(w)) for i, (c, w) in enumerate(codes) if c}


def inflate_many(frames, container, outs=None, sizes=None):
    """(results, produced): see :func:`decompress_many`; `produced[i]` is the
    number of bytes frame i decoded to."""
    frames = list(frames)
    nf = len(frames)
    outs = [None] * nf if outs is None else list(outs)
    sizes = [None] * nf if sizes is None else list(sizes)
    if len(outs) != nf:
        raise ValueError("outs must have one entry per frame")
    if len(sizes) != nf:
        raise ValueError("sizes must have one entry per frame")
    if container not in (ZLIB, GZIP):
        raise ValueError("container must be 0 (zlib) or 1 (gzip)")
    if nf == 0:
        return [], []
    srcs = [_frames.flat_bytes(f, _MAX_BUFFER) for f in frames]
    on_dev = [is_device_tensor(s) for s in srcs]
    device = _frames.batch_device(srcs, on_dev, outs, "frames")
    lengths = [int(len(s)) for s in srcs]
    for n in lengths:
        if n >= _MAX_BYTES:
            raise _too_long(n)
    out_raw = [None if o is None else _frames.out_bytes(o, 0) for o in outs]
    caps = [None] * nf  # the capacity a caller gave: the destination's bytes, or the size
    for i in range(nf):
        if sizes[i] is not None:
            caps[i] = int(sizes[i])
            if caps[i] < 0:
                raise ValueError("sizes must not be negative")
            if out_raw[i] is not None and len(out_raw[i]) < caps[i]:
                raise ValueError("destination buffer too small; expected at least %s, got %s" % (caps[i], len(out_raw[i])))
        elif out_raw[i] is not None:
            caps[i] = int(len(out_raw[i]))
        if caps[i] is not None and caps[i] >= _MAX_BYTES:
            raise _too_long(caps[i])
    _frames.check_out_device(out_raw, device)

    results = [None] * nf
    with _frames.launching(device) as (device, st):
        src_all, offsets = _frames.stage_packed(srcs, lengths, on_dev, device)
        if src_all.numel() == 0:  # nothing but empty frames: the kernels still want an address
            src_all = torch.zeros(16, dtype=torch.uint8, device=device)
        table = np.zeros(nf, dtype=_RECORD)
        for i in range(nf):
            table[i] = (offsets[i], lengths[i], 0, 0, container)
        ws_bytes = lib.mc_inflate_workspace(nf)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)

        # ---- the sizing pass, for the frames that came with neither a destination nor a size ----
        unsized = [i for i in range(nf) if caps[i] is None]
        given = {i: caps[i] for i in range(nf) if caps[i] is not None}
        if unsized:
            sub_d = upload(np.ascontiguousarray(table[unsized]).view(np.uint8), device)
            words = torch.empty(3 * len(unsized), dtype=torch.int32, device=device)  # sizes, then the error record
            check(lib.mc_inflate_size_batch(src_all.data_ptr(), sub_d.data_ptr(), len(unsized), ws.data_ptr(), ws_bytes,
                                            words.data_ptr(), words.data_ptr() + 4 * len(unsized), st),
                  "mc_inflate_size_batch")
            host = words.cpu().numpy()  # waits for the stream
            counted = host[:len(unsized)].view(np.uint32).tolist()
            errors = _records(host[len(unsized):].reshape(-1, 2))
            if errors:  # raised before anything is decoded
                _raise(container, {unsized[k]: v for k, v in errors.items()}, given)
            for k, i in enumerate(unsized):
                caps[i] = counted[k]

        # ---- plan + decode + check ----
        live = range(nf)
        own, own_off, final = _frames.place(live, caps, out_raw, device)
        for i in live:
            table[i]["dst"] = final[i].data_ptr() if caps[i] else 0
            table[i]["capacity"] = caps[i]
        table_d = upload(table.view(np.uint8), device)
        words = torch.empty(3 * nf, dtype=torch.int32, device=device)  # produced, then the error record
        check(lib.mc_inflate_decode_batch(src_all.data_ptr(), table_d.data_ptr(), nf, max(caps), ws.data_ptr(), ws_bytes,
                                          words.data_ptr(), words.data_ptr() + 4 * nf, st), "mc_inflate_decode_batch")
        host = words.cpu().numpy()  # waits for the stream
        produced = host[:nf].view(np.uint32).tolist()
        errors = _records(host[nf:].reshape(-1, 2))
        if errors:
            _raise(container, errors, given)
        _frames.hand_back(results, own, own_off, final, live, produced, outs, out_raw, on_dev)
        for i in live:  # a size was an upper bound: the result is what was produced
            if outs[i] is None and on_dev[i] and produced[i] != caps[i]:
                results[i] = results[i][:produced[i]]
    return results, produced


def decompress_many(frames, container, outs=None, sizes=None):
    """Inflate a list of zlib (``container=0``) or gzip (``container=1``)
    frames, one wave per frame.

    Each frame is a host buffer or a device tensor; each result is a flat uint8
    numpy array or device tensor accordingly.  ``outs`` may give, per frame,
    None or a destination (device tensor or writable host buffer), which is
    filled from its start and returned in place of a new array; ``sizes`` may
    give, per frame, None or the number of bytes the frame decodes to at most.
    A frame with either skips the sizing launch; one that decodes to more
    raises ``ValueError``.  Host frames go up in one upload and host results
    come down in one download.  Errors: see the module's text."""
    return inflate_many(frames, container, outs, sizes)[0]
