"""Batched bzip2 decode on the GPU: what :mod:`.bz2` launches.

The decoded size is written nowhere in a bzip2 stream, and because the RLE1
stage depends on byte order it is known only after the inverse BWT.  So a frame
that comes with a destination or a size takes two launches per batch (plan,
decode: csrc/mc_bz2.hip) and one read-back of the error and produced words; a
frame with neither first goes through the sizing launch (the same chain with
no output stores), which adds one launch pair and one small read-back per
batch, and its destination is allocated from that.  The workspace is per
resident wave, not per frame: 5 bytes x 100000 x the batch's highest level
(read here from the frames' fourth bytes) for each of at most 768 waves, which
take frames from a counter.

Exceptions are the stdlib's own classes with ``frame_errors`` attached
({frame index: (code, second word)}, the device error record of
csrc/mc_bz2.h): ``OSError("Invalid data stream")`` for every rejected stream,
``ValueError`` with the stdlib's text for truncation, ``ValueError`` for output
that does not fit a given destination or size, and ``NotImplementedError`` for
the two departures: a block with the randomised bit set, and a further stream
behind the first.

Staging, placing and handing back is :mod:`numcodecs_amd._frames`."""

import numpy as np
import torch

from . import _frames
from ._native import check, lib
from .compat import is_device_tensor, upload

_MAX_BYTES = 1 << 30  # csrc/mc_bz2.h MC_BZ2_MAX_BYTES: frames and outputs are shorter
_MAX_BUFFER = 0x7FFFFFFF

# one record of the frame table (include/mcodec.h)
_RECORD = np.dtype([("src_off", "<u8"), ("src_len", "<u8"), ("dst", "<u8"), ("capacity", "<u4"), ("reserved", "<u4")])
assert _RECORD.itemsize == 32

# csrc/mc_bz2.h mc_bz2_error
E_TRUNCATED, E_RANDOMISED, E_CAPACITY, E_FURTHER, E_TABLE = 3, 5, 19, 20, 21

# The block size (symbols) from which the inverse BWT goes multi-start; 0: the
# library's measured default (csrc/mc_bz2.hip MC_BZ2_MULTI_MIN).  Another value
# is for an A/B run of the two forms.
MULTI_MIN = 0

_EOF_TEXT = "Compressed data ended before the end-of-stream marker was reached"


def _too_long(n):
    return ValueError("bz2 frames and outputs of 2**30 bytes and above are not supported on the GPU; got %d" % n)


def _exception(code, word, frame, capacity):
    """The stdlib's exception for error record (code, word) of frame `frame`."""
    if code == E_CAPACITY:
        if capacity is None:
            return _too_long(_MAX_BYTES)
        return ValueError("frame %d decodes to more than the %d bytes given for it" % (frame, capacity))
    if code == E_TABLE:
        return ValueError("frame %d: the frame record is out of range" % frame)
    if code == E_TRUNCATED:
        return ValueError(_EOF_TEXT)
    if code == E_RANDOMISED:
        return NotImplementedError("bz2 blocks with the randomised bit set are not supported on the GPU")
    if code == E_FURTHER:
        return NotImplementedError("bz2 frames of more than one stream are not supported on the GPU")
    return OSError("Invalid data stream")


def _raise(errors, capacities):
    first = min(errors)
    exc = _exception(*errors[first], first, capacities.get(first))
    exc.frame_errors = dict(errors)
    raise exc


def _records(codes):
    """{index: (code, second word)} of the non-zero rows of a device error record."""
    return {i: (int(c), int(w)) for i, (c, w) in enumerate(codes) if c}


def _max_level(srcs, on_dev, lengths):
    """The highest level digit among the frames' headers (1 where none is readable)."""
    idx = [i for i, n in enumerate(lengths) if n >= 4]
    if not idx:
        return 1
    heads = _frames.read_prefixes([srcs[i] for i in idx], [on_dev[i] for i in idx], 4)
    digits = heads[:, 3].astype(np.int64) - ord("0")
    digits = digits[(digits >= 1) & (digits <= 9)]
    return int(digits.max()) if len(digits) else 1


def bunzip_many(frames, outs=None, sizes=None):
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
        level = _max_level(srcs, on_dev, lengths)
        src_all, offsets = _frames.stage_packed(srcs, lengths, on_dev, device)
        if src_all.numel() == 0:  # nothing but empty frames: the kernels still want an address
            src_all = torch.zeros(16, dtype=torch.uint8, device=device)
        table = np.zeros(nf, dtype=_RECORD)
        for i in range(nf):
            table[i] = (offsets[i], lengths[i], 0, 0, 0)
        ws_bytes = lib.mc_bz2_workspace(nf, level)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)

        # ---- the sizing pass, for the frames that came with neither a destination nor a size ----
        unsized = [i for i in range(nf) if caps[i] is None]
        given = {i: caps[i] for i in range(nf) if caps[i] is not None}
        if unsized:
            sub_d = upload(np.ascontiguousarray(table[unsized]).view(np.uint8), device)
            words = torch.empty(3 * len(unsized), dtype=torch.int32, device=device)  # sizes, then the error record
            check(lib.mc_bz2_size_batch(src_all.data_ptr(), sub_d.data_ptr(), len(unsized), level, MULTI_MIN, ws.data_ptr(), ws_bytes,
                                        words.data_ptr(), words.data_ptr() + 4 * len(unsized), st), "mc_bz2_size_batch")
            host = words.cpu().numpy()  # waits for the stream
            counted = host[:len(unsized)].view(np.uint32).tolist()
            errors = _records(host[len(unsized):].reshape(-1, 2))
            if errors:  # raised before anything is decoded
                _raise({unsized[k]: v for k, v in errors.items()}, given)
            for k, i in enumerate(unsized):
                caps[i] = counted[k]

        # ---- plan + decode ----
        live = range(nf)
        own, own_off, final = _frames.place(live, caps, out_raw, device)
        for i in live:
            table[i]["dst"] = final[i].data_ptr() if caps[i] else 0
            table[i]["capacity"] = caps[i]
        table_d = upload(table.view(np.uint8), device)
        words = torch.empty(3 * nf, dtype=torch.int32, device=device)  # produced, then the error record
        check(lib.mc_bz2_decode_batch(src_all.data_ptr(), table_d.data_ptr(), nf, level, MULTI_MIN, ws.data_ptr(), ws_bytes,
                                      words.data_ptr(), words.data_ptr() + 4 * nf, st), "mc_bz2_decode_batch")
        host = words.cpu().numpy()  # waits for the stream
        produced = host[:nf].view(np.uint32).tolist()
        errors = _records(host[nf:].reshape(-1, 2))
        if errors:
            _raise(errors, given)
        _frames.hand_back(results, own, own_off, final, live, produced, outs, out_raw, on_dev)
        for i in live:  # a size was an upper bound: the result is what was produced
            if outs[i] is None and produced[i] != caps[i]:
                results[i] = results[i][:produced[i]]
    return results, produced


def decompress_many(frames, outs=None, sizes=None):
    """Decode a list of bzip2 streams, a resident wave per frame.

    Each frame is a host buffer or a device tensor; each result is a flat uint8
    numpy array or device tensor accordingly.  ``outs`` may give, per frame,
    None or a destination (device tensor or writable host buffer), which is
    filled from its start and returned in place of a new array; ``sizes`` may
    give, per frame, None or the number of bytes the frame decodes to at most.
    A frame with either skips the sizing launch; one that decodes to more
    raises ``ValueError``.  Host frames go up in one upload and host results
    come down in one download.  Errors: see the module's text."""
    return bunzip_many(frames, outs, sizes)[0]
