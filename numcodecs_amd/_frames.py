"""What the four ``*_many`` calls of :mod:`.blosc` and :mod:`.lz4` do around their
own table records and launches.  A batch mixes host buffers and device tensors;
per call there is one upload of the host inputs, one gathered copy of the
frames' prefixes (only when a frame is on the device) and one download (only
when a result belongs on the host).  Decode inputs are packed end to end, host
frames first; encode inputs and all output slots start at multiples of ``ALIGN``."""

from contextlib import contextmanager

import numpy as np
import torch

from . import _native
from ._ops import _guard, stream
from .compat import device_out, download, ensure_contiguous_ndarray, is_device_tensor, upload

ALIGN = 256


def up(n):
    """`n` rounded up to a multiple of ALIGN."""
    return -(-n // ALIGN) * ALIGN


def slots(sizes):
    """(offsets, total) of slots of `sizes` bytes one after another, each at a
    multiple of ALIGN; a size of 0 takes no space."""
    offsets, total = [], 0
    for n in sizes:
        offsets.append(total)
        total += -(-n // ALIGN) * ALIGN  # up(n), spelled out: this loop runs per frame of every call
    return offsets, total


def slot_map(keys, sizes):
    """({key: offset}, total) of :func:`slots` for `sizes`, one per key."""
    offsets, total = slots(sizes)
    return dict(zip(keys, offsets)), total


def flat_bytes(buf, max_buffer_size):
    """`buf` as flat uint8, a device tensor or a numpy view (ensure_contiguous_ndarray semantics)."""
    arr = ensure_contiguous_ndarray(buf, max_buffer_size)
    if is_device_tensor(arr):
        return arr.view(torch.uint8) if arr.numel() else arr.new_empty(0, dtype=torch.uint8)
    return arr.view(np.uint8)


def out_bytes(out, nbytes):
    """A caller's `out` as flat uint8 (device tensor or numpy), size-checked."""
    raw = flat_bytes(device_out(out), None)
    if not is_device_tensor(raw) and not raw.flags.writeable:
        raise ValueError("destination buffer is read-only")
    if len(raw) < nbytes:
        raise ValueError("destination buffer too small; expected at least %s, got %s" % (nbytes, len(raw)))
    return raw


def batch_device(srcs, on_dev, outs=(), what="frames"):
    """The batch's device: the first device source's, else the first device
    destination's, else None.  A source on another device is refused."""
    device = next((s.device for s, d in zip(srcs, on_dev) if d), None)
    for o in outs:
        if device is None and o is not None and is_device_tensor(device_out(o)):
            device = device_out(o).device
    if any(d and s.device != device for s, d in zip(srcs, on_dev)):
        raise ValueError(f"all {what} of a batch must be on one device")
    return device


def check_out_device(out_raw, device):
    """Destinations (as :func:`out_bytes` gave them) are on the batch's device."""
    if any(is_device_tensor(o) and o.device != device for o in out_raw if o is not None) and device is not None:
        raise ValueError("out must be on the same device as the frames")


def read_prefixes(srcs, on_dev, n):
    """The first `n` bytes of every frame (each at least that long) as the rows
    of one uint8 array: host frames directly, device frames by one gathered copy."""
    dev_idx = [i for i, d in enumerate(on_dev) if d]
    if dev_idx:
        rows = torch.cat([srcs[i][:n] for i in dev_idx]).cpu().numpy().reshape(-1, n)
        if len(dev_idx) == len(srcs):  # the usual batch: the gathered copy is the answer
            return rows
    heads = np.empty((len(srcs), n), np.uint8)
    if dev_idx:
        heads[dev_idx] = rows
    for i, d in enumerate(on_dev):
        if not d:
            heads[i] = srcs[i][:n]
    return heads


@contextmanager
def launching(device):
    """The launch preamble: requires a HIP device and makes `device` (None: the
    current one) current; yields it and torch's current hipStream_t on it."""
    _native.require_device()
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    anchor = torch.empty(0, dtype=torch.uint8, device=device)
    with _guard(anchor):
        yield device, stream(anchor)


def packed_offsets(lengths, on_dev):
    """Each frame's offset in the packed source buffer: host frames first, then
    device frames, both in index order, end to end."""
    offsets, pos = [0] * len(lengths), 0
    for i in sorted(range(len(lengths)), key=on_dev.__getitem__):  # a stable sort: False first
        offsets[i] = pos
        pos += lengths[i]
    return offsets


def stage_packed(srcs, lengths, on_dev, device):
    """(src_all, offsets): the frames' bytes as one device buffer laid out by :func:`packed_offsets`.
    Host frames go up in one upload; a single piece is concatenated neither on the host nor on the device."""
    host = [s for s, d in zip(srcs, on_dev) if not d]
    pieces = []
    if host:
        blob = np.concatenate(host) if len(host) > 1 else host[0]
        pieces.append(upload(np.ascontiguousarray(blob), device))
    pieces.extend(s for s, d in zip(srcs, on_dev) if d)
    src_all = pieces[0] if len(pieces) == 1 else torch.cat(pieces)
    return src_all, packed_offsets(lengths, on_dev)


def place(live, sizes, out_raw, device):
    """(own, own_off, final) for the frames `live` of `sizes[i]` bytes: a caller's device tensor is decoded
    into in place, every other frame gets the slot `own_off[i]` of `own`; `final[i]` is frame i's device bytes."""
    own_off, total = {}, 0
    for i in live:
        if not is_device_tensor(out_raw[i]):
            own_off[i] = total
            total += up(sizes[i])
    own = torch.empty(total, dtype=torch.uint8, device=device)
    final = {i: (own[own_off[i]:own_off[i] + sizes[i]] if i in own_off else out_raw[i][:sizes[i]]) for i in live}
    return own, own_off, final


def hand_back(results, own, own_off, final, live, sizes, outs, out_raw, on_dev):
    """Fill `results[i]` for the decoded frames `live`: a given destination as
    the caller passed it (a host one is filled here), else the source's kind of
    array.  `own` is downloaded once, and only when a result needs the host."""
    host_all = None
    for i in live:
        if is_device_tensor(out_raw[i]):
            results[i] = outs[i]
        elif out_raw[i] is None and on_dev[i]:
            results[i] = final[i]
        else:
            host_all = download(own) if host_all is None else host_all
            piece = host_all[own_off[i]:own_off[i] + sizes[i]]
            if out_raw[i] is None:
                results[i] = piece
            else:  # a host destination
                out_raw[i][:sizes[i]] = piece
                results[i] = outs[i]


def stage_aligned(srcs, live, on_dev, device):
    """{i: device bytes of buffer i} for `live`: device buffers as they are,
    host buffers through one zero-filled blob with ALIGN-ed offsets, one upload."""
    raw = {i: srcs[i] for i in live if on_dev[i]}
    host_idx = [i for i in live if not on_dev[i]]
    if host_idx:
        offs, total = slots([len(srcs[i]) for i in host_idx])
        blob = np.zeros(total, np.uint8)
        for o, i in zip(offs, host_idx):
            blob[o:o + len(srcs[i])] = srcs[i]
        blob_d = upload(blob, device)
        raw.update((i, blob_d[o:o + len(srcs[i])]) for o, i in zip(offs, host_idx))
    return raw


def hand_back_encoded(results, out, out_off, cbytes, live, on_dev):
    """Fill `results[i]` for the encoded buffers `live`: the first `cbytes[k]`
    (ints) bytes of slot `out_off[i]` of `out`, as a device view for a device source
    and from one download of `out` for the host sources, if there are any."""
    host_all = None
    for k, i in enumerate(live):
        if host_all is None and not on_dev[i]:
            host_all = download(out)
        lo, hi = out_off[i], out_off[i] + cbytes[k]
        results[i] = out[lo:hi] if on_dev[i] else host_all[lo:hi]
