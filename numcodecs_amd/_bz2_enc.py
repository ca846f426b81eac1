"""Batched bzip2 encode on the GPU: the binding :mod:`.bz2_enc` is built on.

A batch mixes host buffers and device tensors.  Host inputs go up in one
upload; five launches (prepare, sort, code, layout, emit: csrc/mc_bz2_enc.hip)
encode every chunk of the batch at one level; the frames' sizes are data
dependent, so each call reads them back once (one small device-to-host copy
and a stream wait), and results are trimmed to their size.  Every output slot
holds :func:`bound` bytes, which no frame exceeds.  An empty buffer's frame is
written on the host with no launch.

Staging, placing and handing back is :mod:`numcodecs_amd._frames`."""

import bz2 as _bz2

import numpy as np
import torch

from . import _frames
from ._native import check, lib
from .compat import download, is_device_tensor, upload

_MAX_CHUNK = 1 << 30  # csrc/mc_bz2_enc.h MC_BZ2E_MAX_BYTES
_MAX_BUFFER = 0x7FFFFFFF
E_SPACE, E_TABLE = 1, 2  # MC_BZ2E_E_*

# one record of mc_bz2_encode_batch's chunk table (include/mcodec.h)
_RECORD = np.dtype([("src", "<u8"), ("dst", "<u8"), ("nbytes", "<u4"), ("dst_cap", "<u4"), ("block_base", "<u4"),
                    ("reserved", "<u4")])
assert _RECORD.itemsize == 32

_END = bytes([0x17, 0x72, 0x45, 0x38, 0x50, 0x90])


def segment(level):
    """csrc/mc_bz2_enc.h mc_bz2e_seg: the input bytes of one block."""
    return 80000 * level - 16


def _block_bits(nk):
    nmtf = nk + nk // 4 + 1
    return 48 + 32 + 1 + 24 + 16 + 256 + 3 + 15 + -(-nmtf // 50) + 2 * (5 + 258) + 9 * nmtf


def bound(n, level):
    """csrc/mc_bz2_enc.h mc_bz2_enc_bound: per block the cost of the
    equal-length fallback at the most symbols RLE1 can give, plus the stream
    header, the end magic and the stream CRC; no frame of `n` bytes exceeds it."""
    full, rest = divmod(n, segment(level))
    bits = 32 + 80 + full * _block_bits(segment(level)) + (_block_bits(rest) if rest else 0)
    return (bits + 7) // 8


def empty_frame(level):
    """The frame of an empty buffer: the stream header, the end magic and a
    zero stream CRC (what the stdlib writes too)."""
    return b"BZh" + bytes([0x30 + level]) + _END + bytes(4)


def check_level(level):
    """1 ... 9 pass; anything else raises what ``bz2.compress(b"", level)``
    raises."""
    _bz2.compress(b"", level)
    return int(level)


def _too_long(n):
    return ValueError("bz2 chunks of 2**30 bytes and above are not supported on the GPU; got %d" % n)


def compress_many(bufs, level=1, outs=None):
    """Encode a list of buffers into bzip2 streams at `level`.

    Each buffer is a host buffer or a device tensor: a host buffer gives a uint8
    numpy array, a device tensor a uint8 device tensor, both of exactly the
    frame's length.  ``outs`` may give, per buffer, None or a destination (device
    tensor or writable host buffer) of at least ``bound(n, level)`` bytes, which
    is filled from its start; the result is then its first frame-length bytes.
    Checks of the arguments come before any launch and raise the same on a
    machine without a GPU."""
    level = check_level(level)
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
    bounds = [bound(n, level) for n in lengths]
    out_raw = [None if o is None else _frames.out_bytes(o, bounds[i]) for i, o in enumerate(outs)]
    _frames.check_out_device(out_raw, device)

    results = [None] * nf
    live = [i for i in range(nf) if lengths[i] > 0]
    empties = [i for i in range(nf) if lengths[i] == 0]
    if not live:
        for i in empties:
            results[i] = _hand_empty(level, out_raw[i], on_dev[i], device)
        return results

    with _frames.launching(device) as (device, st):
        raw = _frames.stage_aligned(srcs, live, on_dev, device)
        own, own_off, final = _frames.place(live, bounds, out_raw, device)
        table = np.zeros(len(live), dtype=_RECORD)
        nblocks = 0
        seg = segment(level)
        for k, i in enumerate(live):
            n = lengths[i]
            table[k] = (raw[i].data_ptr(), final[i].data_ptr(), n, min(bounds[i], 0xFFFFFFFF), nblocks, 0)
            nblocks += -(-n // seg)
        if nblocks > 0x7FFFFFFF:
            raise ValueError("a bz2 batch holds less than 2**31 blocks")
        max_chunk = max(lengths)
        table_d = upload(table.view(np.uint8), device)
        ws_bytes = lib.mc_bz2_encode_workspace(len(live), nblocks, max_chunk, level)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
        words = torch.empty(3 * len(live), dtype=torch.int32, device=device)  # sizes, then the error record
        check(lib.mc_bz2_encode_batch(table_d.data_ptr(), len(live), nblocks, max_chunk, level, ws.data_ptr(), ws_bytes,
                                      words.data_ptr(), words.data_ptr() + 4 * len(live), st),
              "mc_bz2_encode_batch")
        back = words.cpu().numpy()  # the one read-back; waits for the stream
        sizes = back[:len(live)].view(np.uint32).tolist()
        err = back[len(live):].reshape(-1, 2)
        for k, i in enumerate(live):
            if err[k, 0] or not 14 < sizes[k] <= bounds[i]:
                raise RuntimeError("bz2 encode error %d on buffer %d (frame size %d)" % (err[k, 0], i, sizes[k]))
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
            results[i] = _hand_empty(level, out_raw[i], on_dev[i], device)
    return results


def _hand_empty(level, out, src_on_dev, device):
    frame = np.frombuffer(empty_frame(level), np.uint8).copy()
    if out is None:
        return upload(frame, device) if src_on_dev else frame
    if is_device_tensor(out):
        out[:len(frame)] = upload(frame, out.device)
    else:
        out[:len(frame)] = frame
    return out[:len(frame)]
