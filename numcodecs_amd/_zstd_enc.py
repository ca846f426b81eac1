"""Batched Zstandard encode on the GPU: the binding :mod:`.zstd_enc` is built on.

A batch mixes host buffers and device tensors.  Host inputs go up in one
upload; four launches (parse, code, layout, emit: csrc/mc_zstd_enc.hip) encode
every chunk of the batch; the frames' sizes are data dependent, so each call
reads them back once (one small device-to-host copy and a stream wait), and
results are trimmed to their size.  Every output slot holds :func:`bound`
bytes, which no frame exceeds.  An empty buffer's frame is written on the host
with no launch.

Staging, placing and handing back is :mod:`numcodecs_amd._frames`."""

import numpy as np
import torch

from . import _frames
from ._native import check, lib
from .compat import download, is_device_tensor, upload

_MAX_CHUNK = 1 << 30  # csrc/mc_zstd_enc.h MC_ZE_MAX_BYTES
_SEGMENT = 65536      # MC_ZE_SEGMENT
_MAX_BUFFER = 0x7FFFFFFF
E_SPACE, E_TABLE = 1, 2  # MC_ZE_E_*
F_CHECKSUM = 1           # MC_ZE_F_CHECKSUM

# one record of mc_zstd_encode_batch's chunk table (include/mcodec.h)
_RECORD = np.dtype([("src", "<u8"), ("dst", "<u8"), ("nbytes", "<u4"), ("dst_cap", "<u4"), ("seg_base", "<u4"),
                    ("seq_base", "<u4"), ("flags", "<u4"), ("reserved", "<u4")])
assert _RECORD.itemsize == 40

_EMPTY = bytes.fromhex("28b52ffd2000010000")                    # libzstd's own bytes
_EMPTY_CHECKSUM = bytes.fromhex("28b52ffd240001000099e9d851")  # and the low half of XXH64 of nothing


def _header(n):
    return 6 if n <= 255 else 7 if n <= _SEGMENT else 10


def bound(n, checksum=False):
    """csrc/mc_zstd_enc.h mc_zstd_enc_bound: the all-raw frame (the frame
    header, 3 bytes per 64 KiB segment, the data, 4 for the checksum); no frame
    of `n` bytes exceeds it."""
    return _header(n) + 3 * max(1, -(-n // _SEGMENT)) + n + (4 if checksum else 0)


def empty_frame(checksum=False):
    """The frame of an empty buffer: a single-segment header declaring 0 bytes
    and one last raw block of size 0 (and the checksum of nothing)."""
    return _EMPTY_CHECKSUM if checksum else _EMPTY


def check_level(level):
    """Any int passes (libzstd clamps a level out of range; all levels take the
    one parse); anything else raises ``TypeError`` as the reference's ``int
    level`` does."""
    if isinstance(level, bool) or not isinstance(level, (int, np.integer)):
        raise TypeError("an integer is required for the zstd level, not %s" % type(level).__name__)
    return int(level)


def _too_long(n):
    return ValueError("zstd chunks of 2**30 bytes and above are not supported on the GPU; got %d" % n)


def compress_many(bufs, level=0, checksum=False, outs=None):
    """Encode a list of buffers into Zstandard frames.

    Each buffer is a host buffer or a device tensor: a host buffer gives a uint8
    numpy array, a device tensor a uint8 device tensor, both of exactly the
    frame's length.  ``outs`` may give, per buffer, None or a destination (device
    tensor or writable host buffer) of at least ``bound(n, checksum)`` bytes,
    which is filled from its start; the result is then its first frame-length
    bytes.  Checks of the arguments come before any launch and raise the same on
    a machine without a GPU."""
    check_level(level)
    checksum = bool(checksum)
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
    bounds = [bound(n, checksum) for n in lengths]
    out_raw = [None if o is None else _frames.out_bytes(o, bounds[i]) for i, o in enumerate(outs)]
    _frames.check_out_device(out_raw, device)

    results = [None] * nf
    live = [i for i in range(nf) if lengths[i] > 0]
    empties = [i for i in range(nf) if lengths[i] == 0]
    if not live:
        for i in empties:
            results[i] = _hand_empty(checksum, out_raw[i], on_dev[i], device)
        return results

    with _frames.launching(device) as (device, st):
        raw = _frames.stage_aligned(srcs, live, on_dev, device)
        own, own_off, final = _frames.place(live, bounds, out_raw, device)
        table = np.zeros(len(live), dtype=_RECORD)
        nsegs = nseqs = 0  # a chunk's segments, and its sequence records: one per 4 bytes at most
        for k, i in enumerate(live):
            n = lengths[i]
            if nseqs + -(-n // 4) > 2**32 - 1:
                raise ValueError("a zstd batch holds less than 16 GiB")
            table[k] = (raw[i].data_ptr(), final[i].data_ptr(), n, bounds[i], nsegs, nseqs,
                        F_CHECKSUM if checksum else 0, 0)
            nsegs += -(-n // _SEGMENT)
            nseqs += -(-n // 4)
        table_d = upload(table.view(np.uint8), device)
        ws_bytes = lib.mc_zstd_encode_workspace(len(live), nsegs, nseqs)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
        words = torch.empty(3 * len(live), dtype=torch.int32, device=device)  # sizes, then the error record
        check(lib.mc_zstd_encode_batch(None, table_d.data_ptr(), len(live), nsegs, nseqs, ws.data_ptr(), ws_bytes,
                                       words.data_ptr(), words.data_ptr() + 4 * len(live), st),
              "mc_zstd_encode_batch")
        back = words.cpu().numpy()  # the one read-back; waits for the stream
        sizes = back[:len(live)].view(np.uint32).tolist()
        err = back[len(live):].reshape(-1, 2)
        for k, i in enumerate(live):
            if err[k, 0] or not _header(lengths[i]) + 3 < sizes[k] <= bounds[i]:
                raise RuntimeError("zstd encode error %d on buffer %d (frame size %d)" % (err[k, 0], i, sizes[k]))
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
            results[i] = _hand_empty(checksum, out_raw[i], on_dev[i], device)
    return results


def _hand_empty(checksum, out, src_on_dev, device):
    frame = np.frombuffer(empty_frame(checksum), np.uint8).copy()
    if out is None:
        return upload(frame, device) if src_on_dev else frame
    if is_device_tensor(out):
        out[:len(frame)] = upload(frame, out.device)
    else:
        out[:len(frame)] = frame
    return out[:len(frame)]
