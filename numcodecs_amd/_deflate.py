"""Batched deflate on the GPU: the binding :mod:`.deflate` is built on.

A batch mixes host buffers and device tensors.  Host inputs go up in one
upload; four launches (parse, code, layout, emit: csrc/mc_deflate.hip) encode
every chunk of the batch; the frames' sizes are data dependent, so each call
reads them back once (one small device-to-host copy and a stream wait), and
results are trimmed to their size.  Every output slot holds
:func:`bound` bytes, which no frame exceeds.  An empty buffer's frame is
written on the host with no launch.

Staging, placing and handing back is :mod:`numcodecs_amd._frames`."""

import zlib as _zlib

import numpy as np
import torch

from . import _frames
from ._native import check, lib
from .compat import download, is_device_tensor, upload

ZLIB, GZIP = 0, 1
CONTAINERS = {"zlib": ZLIB, "gzip": GZIP}
_MAX_CHUNK = 1 << 30  # csrc/mc_deflate.h MC_DFL_MAX_BYTES
_SEGMENT = 65536      # MC_DFL_SEGMENT
_MAX_BUFFER = 0x7FFFFFFF
E_SPACE, E_TABLE = 1, 2  # MC_DFL_E_*

# one record of mc_deflate_encode_batch's chunk table (include/mcodec.h)
_RECORD = np.dtype([("src", "<u8"), ("dst", "<u8"), ("nbytes", "<u4"), ("dst_cap", "<u4"), ("seg_base", "<u4"),
                    ("container", "<u4"), ("level", "<u4"), ("seq_base", "<u4")])
assert _RECORD.itemsize == 40

_GZIP_HEADER = bytes([0x1F, 0x8B, 8, 0, 0, 0, 0, 0, 4, 255])  # MTIME 0, XFL 4, OS 255
_ZLIB_HEADER = bytes([0x78, 0x01])


def _box(container):
    return (10, 8) if container == GZIP else (2, 4)


def bound(n, container):
    """csrc/mc_deflate.h mc_deflate_bound: the container's bytes plus, per 64 KiB
    segment, n_k + 5 * ceil(n_k / 65535); no frame of `n` bytes exceeds it."""
    head, trail = _box(container)
    if n == 0:
        return head + 2 + trail
    full, rest = divmod(n, _SEGMENT)
    return head + trail + full * (_SEGMENT + 10) + (rest + 5 * -(-rest // 65535) if rest else 0)


def empty_frame(container):
    """The frame of an empty buffer: the header, a final fixed block holding
    only end-of-block (03 00) and the trailer."""
    if container == GZIP:
        return _GZIP_HEADER + b"\x03\x00" + bytes(8)
    return _ZLIB_HEADER + b"\x03\x00" + b"\x00\x00\x00\x01"


def check_level(level):
    """-1 and 0 ... 9 pass; anything else raises what ``zlib.compress(b"", level)``
    raises (``zlib.error``: Bad compression level).  Returns the record's level
    word: 0 for stored blocks, 1 for the one parse."""
    _zlib.compress(b"", level)
    return 0 if level == 0 else 1


def _too_long(n):
    return ValueError("zlib / gzip chunks of 2**30 bytes and above are not supported on the GPU; got %d" % n)


def compress_many(bufs, container, level=1, outs=None):
    """Deflate a list of buffers into frames of `container` (ZLIB or GZIP).

    Each buffer is a host buffer or a device tensor: a host buffer gives a uint8
    numpy array, a device tensor a uint8 device tensor, both of exactly the
    frame's length.  ``outs`` may give, per buffer, None or a destination (device
    tensor or writable host buffer) of at least ``bound(n, container)`` bytes,
    which is filled from its start; the result is then its first frame-length
    bytes.  Checks of the arguments come before any launch and raise the same on
    a machine without a GPU."""
    level_word = check_level(level)
    if container not in (ZLIB, GZIP):
        raise ValueError("container must be 'zlib' or 'gzip'")
    bufs = list(bufs)
    nf = len(bufs)
    outs = [None] * nf if outs is None else list(outs)
    if len(outs) != nf:
        raise ValueError("outs must have one entry per buffer")
    if nf == 0:
        return []
    srcs = [_frames.flat_bytes(b, _MAX_BUFFER) for b in bufs]
    on_dev = [is_device_tensor(s) for s in srcs]
    device = _frames.batch_device(srcs, on_dev, outs, "buffers")
    lengths = [int(len(s)) for s in srcs]
    for n in lengths:
        if n >= _MAX_CHUNK:
            raise _too_long(n)
    bounds = [bound(n, container) for n in lengths]
    out_raw = [None if o is None else _frames.out_bytes(o, bounds[i]) for i, o in enumerate(outs)]
    _frames.check_out_device(out_raw, device)

    results = [None] * nf
    live = [i for i in range(nf) if lengths[i] > 0]
    empties = [i for i in range(nf) if lengths[i] == 0]
    if not live:
        for i in empties:
            results[i] = _hand_empty(container, out_raw[i], on_dev[i], device)
        return results

    with _frames.launching(device) as (device, st):
        raw = _frames.stage_aligned(srcs, live, on_dev, device)
        own, own_off, final = _frames.place(live, bounds, out_raw, device)
        table = np.zeros(len(live), dtype=_RECORD)
        nsegs = nseqs = 0  # a chunk's segments, and its sequence records: one per 4 bytes at most
        for k, i in enumerate(live):
            n = lengths[i]
            if nseqs + -(-n // 4) > 2**32 - 1:
                raise ValueError("a deflate batch holds less than 16 GiB")
            table[k] = (raw[i].data_ptr(), final[i].data_ptr(), n, bounds[i], nsegs, container, level_word, nseqs)
            nsegs += -(-n // _SEGMENT)
            nseqs += -(-n // 4)
        table_d = upload(table.view(np.uint8), device)
        ws_bytes = lib.mc_deflate_encode_workspace(len(live), nsegs, nseqs)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
        words = torch.empty(3 * len(live), dtype=torch.int32, device=device)  # sizes, then the error record
        check(lib.mc_deflate_encode_batch(None, table_d.data_ptr(), len(live), nsegs, nseqs, ws.data_ptr(), ws_bytes,
                                          words.data_ptr(), words.data_ptr() + 4 * len(live), st),
              "mc_deflate_encode_batch")
        back = words.cpu().numpy()  # the one read-back; waits for the stream
        sizes = back[:len(live)].view(np.uint32).tolist()
        err = back[len(live):].reshape(-1, 2)
        for k, i in enumerate(live):
            head, trail = _box(container)
            if err[k, 0] or not head + trail < sizes[k] <= bounds[i]:
                raise RuntimeError("deflate error %d on buffer %d (frame size %d)" % (err[k, 0], i, sizes[k]))
        host_all = None
        for k, i in enumerate(live):
            size = sizes[k]
            if is_device_tensor(out_raw[i]):
                results[i] = out_raw[i][:size]
            elif out_raw[i] is None and on_dev[i]:
                results[i] = final[i][:size]
            else:
                host_all = download(own) if host_all is None else host_all
                piece = host_all[own_off[i]:own_off[i] + size]
                if out_raw[i] is None:
                    results[i] = piece
                else:  # a host destination
                    out_raw[i][:size] = piece
                    results[i] = out_raw[i][:size]
        for i in empties:
            results[i] = _hand_empty(container, out_raw[i], on_dev[i], device)
    return results


def _hand_empty(container, out, src_on_dev, device):
    frame = np.frombuffer(empty_frame(container), np.uint8).copy()
    if out is None:
        return upload(frame, device) if src_on_dev else frame
    if is_device_tensor(out):
        out[:len(frame)] = upload(frame, out.device)
    else:
        out[:len(frame)] = frame
    return out[:len(frame)]
