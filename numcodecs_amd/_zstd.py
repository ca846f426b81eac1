"""Batched Zstandard decode on the GPU: what :mod:`.zstd` runs on.

A frame may state the size it decodes to (Frame_Content_Size); that is read on
the host from the header bytes (for device frames from one small read-back of
the batch's heads) and is the frame's capacity, as the reference passes it to
``ZSTD_decompress``.  A frame that comes with a destination, a size or a
declared size takes three launches per batch (plan, decode, check:
csrc/mc_zstd.hip) and one read-back of the error and produced words; a frame
with none of them first goes through the sizing launch (headers, literal sizes
and the sequences' lengths, no Huffman decode and no stores), which adds one
launch pair and one small read-back per batch.  One frame is one serial chain
on one wave: throughput comes from the batch.

Exceptions follow the reference's ``decompress()`` (src/numcodecs/zstd.pyx),
with ``frame_errors`` attached ({frame index: (code, second word)}, the device
error record of csrc/mc_zstd.h): ``RuntimeError('Zstd decompression error:
...')`` with ``invalid input data`` for what its frame walk refuses and for a
declared size of 0, and libzstd's own text (as ``ZSTD_getErrorName`` of libzstd
1.4.8 gives it; tests/golden/zstd_cases.json) for what ``ZSTD_decompress``
refuses; ``ValueError`` for a destination smaller than the declared size; and
``NotImplementedError`` for a second or a skippable frame, which the reference
would concatenate or skip.

Staging, placing and handing back is :mod:`numcodecs_amd._frames`."""

import numpy as np
import torch

from . import _frames
from ._inflate import _RECORD, _records
from ._native import check, lib
from .compat import is_device_tensor, upload

_MAX_BYTES = 1 << 30  # csrc/mc_zstd.h MC_ZSTD_MAX_BYTES: frames and outputs are shorter
_MAX_BUFFER = 0x7FFFFFFF
_MAGIC = 0xFD2FB528
_HEAD = 18  # the longest frame header

# csrc/mc_zstd.h mc_zstd_error
E_HEADER, E_EMPTY, E_DICT, E_MEMBER, E_CORRUPT, E_SRCSIZE, E_CAPACITY, E_CHECK, E_SIZE, E_TABLE = range(1, 11)

_PREFIX = "Zstd decompression error: "
_INVALID = "invalid input data"
# ZSTD_getErrorName's texts (libzstd 1.4.8)
_LIB_TEXT = {
    E_DICT: "Dictionary mismatch",
    E_CORRUPT: "Corrupted block detected",
    E_SRCSIZE: "Src size is incorrect",
    E_CAPACITY: "Destination buffer is too small",
    E_CHECK: "Restored data doesn't match checksum",
    E_SIZE: "Corrupted block detected",
}


def _too_long(n):
    return ValueError("zstd frames and outputs of 2**30 bytes and above are not supported on the GPU; got %d" % n)


def declared_size(head):
    """The Frame_Content_Size the header bytes `head` declare, None when there
    is none (or no complete Zstandard header: the device names that error)."""
    h = bytes(head[:_HEAD])
    if len(h) < 5 or int.from_bytes(h[:4], "little") != _MAGIC:
        return None
    fhd = h[4]
    flag, single = fhd >> 6, (fhd >> 5) & 1
    nb = (single, 2, 4, 8)[flag]
    if nb == 0 or (fhd & 8):
        return None
    p = 5 + (1 - single) + (0, 1, 2, 4)[fhd & 3]
    if len(h) < p + nb:
        return None
    return int.from_bytes(h[p:p + nb], "little") + (256 if nb == 2 else 0)


def _exception(code, word, frame, capacity):
    """The reference's exception for error record (code, word) of frame `frame`."""
    if code in (E_HEADER, E_EMPTY):
        return RuntimeError(_PREFIX + _INVALID)
    if code == E_MEMBER:
        return NotImplementedError("zstd input of more than one frame (or with a skippable frame) is not supported "
                                   "on the GPU")
    if code == E_TABLE:
        return ValueError("frame %d: the frame record is out of range" % frame)
    if code == E_CAPACITY and capacity is None:
        return _too_long(_MAX_BYTES)
    return RuntimeError(_PREFIX + _LIB_TEXT.get(code, "code %d" % code))


def _raise(errors, capacities):
    first = min(errors)
    exc = _exception(*errors[first], first, capacities.get(first))
    exc.frame_errors = dict(errors)
    raise exc


def _heads(srcs, on_dev, lengths, device):
    """The first bytes of every frame, on the host: one read-back for the device frames."""
    heads = [None] * len(srcs)
    dev = [i for i in range(len(srcs)) if on_dev[i]]
    if dev:
        pad = torch.zeros((len(dev), _HEAD), dtype=torch.uint8, device=srcs[dev[0]].device)
        for k, i in enumerate(dev):
            m = min(_HEAD, lengths[i])
            pad[k, :m] = srcs[i][:m]
        host = pad.cpu().numpy()
        for k, i in enumerate(dev):
            heads[i] = host[k, :min(_HEAD, lengths[i])].tobytes()
    for i in range(len(srcs)):
        if heads[i] is None:
            heads[i] = bytes(memoryview(srcs[i])[:_HEAD])
    return heads


def decode_many(frames, outs=None, sizes=None):
    """(results, produced): see :func:`numcodecs_amd.zstd.decompress_many`;
    `produced[i]` is the number of bytes frame i decoded to."""
    frames = list(frames)
    nf = len(frames)
    outs = [None] * nf if outs is None else list(outs)
    sizes = [None] * nf if sizes is None else list(sizes)
    if len(outs) != nf:
        raise ValueError("outs must have one entry per frame")
    if len(sizes) != nf:
        raise ValueError("sizes must have one entry per frame")
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
    heads = _heads(srcs, on_dev, lengths, device)
    caps = [None] * nf     # the capacity: the declared size, the size given, or the destination's bytes
    exact = [False] * nf   # the capacity is the destination's alone: the frame must fill it
    for i in range(nf):
        declared = declared_size(heads[i])
        have = None if out_raw[i] is None else int(len(out_raw[i]))
        if sizes[i] is not None and int(sizes[i]) < 0:
            raise ValueError("sizes must not be negative")
        if declared is not None:
            if declared >= _MAX_BYTES:
                raise _too_long(declared)
            caps[i] = declared
            for room in (have, None if sizes[i] is None else int(sizes[i])):
                if room is not None and room < declared:
                    raise ValueError("destination buffer too small; expected at least %s, got %s" % (declared, room))
        elif sizes[i] is not None:
            caps[i] = int(sizes[i])
            if have is not None and have < caps[i]:
                raise ValueError("destination buffer too small; expected at least %s, got %s" % (caps[i], have))
        elif have is not None:
            caps[i] = have
            exact[i] = True
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
            table[i] = (offsets[i], lengths[i], 0, 0, 0)
        ws_bytes = lib.mc_zstd_workspace(nf)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)

        # ---- the sizing pass, for the frames with no destination, no size and no declared size ----
        unsized = [i for i in range(nf) if caps[i] is None]
        given = {i: caps[i] for i in range(nf) if caps[i] is not None}
        refused = {}
        if unsized:
            sub_d = upload(np.ascontiguousarray(table[unsized]).view(np.uint8), device)
            words = torch.empty(3 * len(unsized), dtype=torch.int32, device=device)  # sizes, then the error record
            check(lib.mc_zstd_size_batch(src_all.data_ptr(), sub_d.data_ptr(), len(unsized), ws.data_ptr(), ws_bytes,
                                         words.data_ptr(), words.data_ptr() + 4 * len(unsized), st),
                  "mc_zstd_size_batch")
            host = words.cpu().numpy()  # waits for the stream
            counted = host[:len(unsized)].view(np.uint32).tolist()
            # a frame refused here is named with the batch's other rejected frames, after the decode
            refused = {unsized[k]: v for k, v in _records(host[len(unsized):].reshape(-1, 2)).items()}
            for k, i in enumerate(unsized):
                caps[i] = 0 if i in refused else counted[k]

        # ---- plan + decode + check ----
        live = range(nf)
        own, own_off, final = _frames.place(live, caps, out_raw, device)
        for i in live:
            table[i]["dst"] = final[i].data_ptr() if caps[i] else 0
            table[i]["capacity"] = caps[i]
        table_d = upload(table.view(np.uint8), device)
        words = torch.empty(3 * nf, dtype=torch.int32, device=device)  # produced, then the error record
        check(lib.mc_zstd_decode_batch(src_all.data_ptr(), table_d.data_ptr(), nf, max(caps), ws.data_ptr(), ws_bytes,
                                       words.data_ptr(), words.data_ptr() + 4 * nf, st), "mc_zstd_decode_batch")
        host = words.cpu().numpy()  # waits for the stream
        produced = host[:nf].view(np.uint32).tolist()
        errors = _records(host[nf:].reshape(-1, 2))
        errors.update(refused)
        if errors:
            _raise(errors, given)
        for i in live:  # no size anywhere but the destination's: the reference wants it filled
            if exact[i] and produced[i] != caps[i]:
                exc = RuntimeError(_PREFIX + "expected to decompress %s, got %s" % (caps[i], produced[i]))
                exc.frame_errors = {i: (-1, produced[i])}
                raise exc
        _frames.hand_back(results, own, own_off, final, live, produced, outs, out_raw, on_dev)
        for i in live:  # a size was an upper bound: the result is what was produced
            if outs[i] is None and on_dev[i] and produced[i] != caps[i]:
                results[i] = results[i][:produced[i]]
    return results, produced
