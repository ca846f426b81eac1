"""LZ4 on the GPU (reference: src/numcodecs/lz4.pyx).

A frame is a 4-byte little-endian size followed by ONE LZ4 block for the
whole chunk.  An empty buffer encodes to the 5 bytes ``00 00 00 00 00`` (the
size word and a single zero token), written on the host with no launch.

Compression (:func:`compress`, :func:`compress_many`, :class:`LZ4`): a chunk
is cut into 64 KiB segments, each compressed by one wave with the Blosc
encoder's match finder, and the segments' sequences are stitched into one
valid block (csrc/mc_lz4_codec.h states the rules; csrc/mc_lz4_codec.hip runs
them: three launches for a whole batch).  Any LZ4 reader decodes the frames;
they are not byte-equal to liblz4's (the match finder differs, and matches do
not cross 64 KiB segment boundaries).  ``acceleration`` is accepted and kept in
the config, and ``<= 0`` means 1, as in the reference; it does not change the
match finder, which has no levels (the same as Blosc's ``clevel`` here).

Decompression: the 4-byte size word is read on the host -- for frames that are
already on the device this costs one small gathered device-to-host copy per
batch -- then one plan launch and one decode launch handle the whole batch, one
wave per chunk.  One block is one serial chain, so a single large chunk decodes
at one wave's speed: throughput comes from the batch.

The device decoder handles streams below 2**30 bytes, so both directions raise
``ValueError`` for a chunk of 2**30 bytes or more: the encoder never writes
what the decoder here cannot read.  ``LZ4.max_buffer_size`` keeps the
reference's value.

The codec is not registered on import: call :func:`register`.

Staging a batch's inputs, placing its outputs and handing results back is
:mod:`numcodecs_amd._frames`, shared with Blosc; the rest is the codec's own.
"""

import numpy as np
import torch

from . import _frames
from ._native import check, lib
from .abc import Codec
from .compat import is_device_tensor, upload
from .registry import register_codec

__all__ = ["LZ4", "DEFAULT_ACCELERATION", "compress", "compress_many", "decompress", "decompress_many", "register"]

DEFAULT_ACCELERATION = 1
_HEADER = 4
_MAX_CHUNK = 1 << 30  # csrc/mc_lz4.h MC_LZ4_MAX_USIZE: the device decoder's streams are shorter
_SEGMENT = 65536      # csrc/mc_lz4_codec.h MC_LZ4C_SEGMENT
_EMPTY_FRAME = bytes(5)
_E_SIZE = 10          # csrc/mc_lz4.h MC_LZ4_E_SIZE: the block ended short of the size word
_E_TRUNCATED = 4      # MC_LZ4_E_TRUNCATED

# one record of mc_lz4_encode_batch's / mc_lz4_decode_batch's chunk table (include/mcodec.h)
_ENC_RECORD = np.dtype([("src", "<u8"), ("dst", "<u8"), ("scratch_off", "<u8"), ("nbytes", "<u4"), ("dst_cap", "<u4"),
                        ("seg_base", "<u4"), ("reserved", "<u4")])
_DEC_RECORD = np.dtype([("src_off", "<u8"), ("src_len", "<u8"), ("dst", "<u8"), ("usize", "<u4"), ("reserved", "<u4")])
assert _ENC_RECORD.itemsize == 40 and _DEC_RECORD.itemsize == 32


def _frame_slot(n):
    """The reference's destination size: 4 + LZ4_compressBound(n)."""
    return _HEADER + n + n // 255 + 16


def _flat_bytes(buf):
    """`buf` as flat uint8 (lz4.pyx:219), within ``LZ4.max_buffer_size``."""
    return _frames.flat_bytes(buf, LZ4.max_buffer_size)


def _too_long(n):
    return ValueError("LZ4 chunks of 2**30 bytes and above are not supported on the GPU; got %d" % n)


def compress_many(sources, acceleration=DEFAULT_ACCELERATION):
    """Compress a list of buffers to ``lz4`` frames with three launches for all
    of them.

    Each source is a host buffer or a device tensor.  A device tensor gives a
    uint8 device tensor of exactly the frame's length (a view of its slot), a
    host buffer a uint8 numpy array; host inputs go up in one upload.  The
    results' lengths are data dependent, so every call reads the frames'
    lengths back: one small device-to-host copy and a stream wait per batch.

    ``acceleration`` is checked and otherwise unused: the match finder has no
    levels.  Checks of the arguments and sizes come before any launch and
    raise the same on a machine without a GPU."""
    acceleration = int(acceleration)
    if acceleration <= 0:
        acceleration = DEFAULT_ACCELERATION
    srcs = [_flat_bytes(s) for s in sources]
    nf = len(srcs)
    if nf == 0:
        return []
    on_dev = [is_device_tensor(s) for s in srcs]
    device = _frames.batch_device(srcs, on_dev, what="buffers")
    lengths = [int(len(s)) for s in srcs]
    for n in lengths:
        if n >= _MAX_CHUNK:
            raise _too_long(n)

    live = [i for i in range(nf) if lengths[i] > 0]
    results = [None] * nf
    for i in range(nf):
        if lengths[i] == 0:  # the size word and one zero token, written on the host
            head = np.frombuffer(_EMPTY_FRAME, np.uint8).copy()
            results[i] = upload(head, device) if on_dev[i] else head
    if not live:
        return results

    with _frames.launching(device) as (device, st):
        raw = _frames.stage_aligned(srcs, live, on_dev, device)
        # ---- slots: the frame (the reference's bound) and the scratch (nbytes) ----
        out_off, out_total = _frames.slot_map(live, [_frame_slot(lengths[i]) for i in live])
        scr_off, scr_total = _frames.slot_map(live, [lengths[i] for i in live])
        table = np.zeros(len(live), dtype=_ENC_RECORD)
        nsegs = 0
        for k, i in enumerate(live):
            n = lengths[i]
            table[k] = (raw[i].data_ptr(), out_off[i], scr_off[i], n, _frame_slot(n), nsegs, 0)
            nsegs += -(-n // _SEGMENT)
        if nsegs > 2**31 - 1:
            raise ValueError("too many LZ4 segments in one batch")
        out = torch.empty(out_total, dtype=torch.uint8, device=device)
        table["dst"] += out.data_ptr()
        table_d = upload(table.view(np.uint8), device)
        ws_bytes = lib.mc_lz4_encode_workspace(len(live), nsegs, scr_total)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
        cbytes_d = torch.empty(len(live), dtype=torch.int32, device=device)
        check(lib.mc_lz4_encode_batch(None, table_d.data_ptr(), len(live), nsegs, ws.data_ptr(), ws_bytes,
                                      cbytes_d.data_ptr(), st), "mc_lz4_encode_batch")
        cbytes = cbytes_d.cpu().numpy().view(np.uint32).tolist()  # waits for the stream
        for k, i in enumerate(live):
            if not _HEADER < cbytes[k] <= _frame_slot(lengths[i]):
                raise RuntimeError("LZ4 compression error: %d" % (cbytes[k] if cbytes[k] else -1))
        _frames.hand_back_encoded(results, out, out_off, cbytes, live, on_dev)
    return results


def compress(source, acceleration=DEFAULT_ACCELERATION):
    """Compress one buffer to an ``lz4`` frame (lz4.pyx:44-114): a device
    tensor gives a uint8 device tensor, a host buffer a uint8 numpy array.
    See :func:`compress_many` for ``acceleration`` (accepted, no effect on the
    match finder) and the one read-back per call."""
    return compress_many([source], acceleration)[0]


def _decode_error(message, frame_errors, kind=RuntimeError):
    """The reference's exception; ``frame_errors`` maps the index of each
    rejected frame to (code, bytes produced): code -1 for a failed host check,
    else the device error record's (csrc/mc_lz4.h)."""
    exc = kind(message)
    exc.frame_errors = dict(frame_errors)
    return exc


def _device_error_text(code, produced, usize):
    if code == _E_SIZE:
        return "LZ4 decompression error: expected to decompress %s, got %s" % (usize, produced)
    return "LZ4 decompression error: -%d" % code


def decompress_many(frames, outs=None):
    """Decompress a list of ``lz4`` frames with one plan launch and one decode
    launch for all of them, one wave per frame.

    Each frame is a host buffer or a device tensor; each result is a flat
    uint8 numpy array or device tensor accordingly.  ``outs`` may give, per
    frame, None or a destination (device tensor or writable host buffer) of at
    least the frame's size word in bytes, which is filled and returned in place
    of a new array.  Errors are the reference's (lz4.pyx:117-193); a malformed
    block raises ``RuntimeError('LZ4 decompression error: -<code>')`` with the
    device error code of csrc/mc_lz4.h (liblz4's own numbers depend on the
    position and are not reproduced), and the exception's ``frame_errors``
    names the rejected frames of the batch."""
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
        raise _decode_error("bad input data", short, ValueError)
    sizes = _frames.read_prefixes(srcs, on_dev, _HEADER).view("<i4").ravel().tolist()

    # ---- host checks (before anything is launched) ----
    bad = {i: (-1, 0) for i in range(nf) if sizes[i] <= 0}
    if bad:
        raise _decode_error("LZ4 decompression error: invalid input data", bad)
    bad = {i: (_E_TRUNCATED, 0) for i in range(nf) if lengths[i] == _HEADER}  # no block at all
    if bad:
        raise _decode_error(_device_error_text(_E_TRUNCATED, 0, 0), bad)
    out_raw = [None if o is None else _frames.out_bytes(o, sizes[i]) for i, o in enumerate(outs)]
    for n in sizes:
        if n >= _MAX_CHUNK:
            raise _too_long(n)
    _frames.check_out_device(out_raw, device)

    live = range(nf)  # an empty buffer's frame is refused above: every frame is decoded
    results = [None] * nf
    with _frames.launching(device) as (device, st):
        src_all, offsets = _frames.stage_packed(srcs, lengths, on_dev, device)
        own, own_off, final = _frames.place(live, sizes, out_raw, device)
        table = np.zeros(nf, dtype=_DEC_RECORD)
        for i in live:
            table[i] = (offsets[i], lengths[i], final[i].data_ptr(), sizes[i], 0)
        table_d = upload(table.view(np.uint8), device)
        ws_bytes = lib.mc_lz4_decode_workspace(nf)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
        err = torch.empty(2 * nf, dtype=torch.int32, device=device)
        check(lib.mc_lz4_decode_batch(src_all.data_ptr(), table_d.data_ptr(), nf, max(sizes), ws.data_ptr(), ws_bytes,
                                      err.data_ptr(), st), "mc_lz4_decode_batch")
        codes = err.cpu().numpy().reshape(-1, 2)  # waits for the stream
        if codes[:, 0].any():
            errors = {i: (int(c), int(m)) for i, (c, m) in enumerate(codes) if c}
            first = min(errors)
            raise _decode_error(_device_error_text(*errors[first], sizes[first]), errors)
        _frames.hand_back(results, own, own_off, final, live, sizes, outs, out_raw, on_dev)
    return results


def decompress(source, dest=None):
    """Decompress one ``lz4`` frame (lz4.pyx:117-193): a host buffer gives a
    uint8 numpy array, a device tensor a uint8 device tensor; ``dest``, when
    given, is filled and returned."""
    return decompress_many([source], [dest])[0]


class LZ4(Codec):
    """The ``lz4`` codec (numcodecs id ``lz4``): same constructor, config and
    repr as the reference (lz4.pyx:197-230), both directions on the GPU.

    ``acceleration`` is kept in the config and ``<= 0`` means 1, as in the
    reference, but it does not change the match finder, which has no levels.
    Chunks of 2**30 bytes and above raise ``ValueError``."""

    codec_id = "lz4"
    max_buffer_size = 0x7E000000

    def __init__(self, acceleration=DEFAULT_ACCELERATION):
        self.acceleration = acceleration

    def encode(self, buf):
        return compress(buf, self.acceleration)

    def decode(self, buf, out=None):
        return decompress(buf, out)

    def __repr__(self):
        return "%s(acceleration=%r)" % (type(self).__name__, self.acceleration)


def register():
    """Register :class:`LZ4` under ``'lz4'`` in this package's
    ``codec_registry`` (never done on import, and never in numcodecs' own
    registry)."""
    register_codec(LZ4)
