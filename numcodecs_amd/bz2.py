"""BZ2 on the GPU, decode only (reference: src/numcodecs/bz2.py).

A frame is one bzip2 stream: ``BZh`` and a level digit, blocks that follow one
another at bit granularity, the end magic and the combined CRC.
:func:`decompress_many` decodes a batch with a resident wave per frame
(csrc/mc_bz2.hip; the rules are csrc/mc_bz2.h's, which follow libbz2 1.0.8 as
``bz2.decompress`` wraps it): trailing bytes that do not begin a stream are
ignored.  Two things the stdlib decodes are refused with
``NotImplementedError``: a block with the randomised bit set (no encoder since
bzip2 0.9.5 writes one) and a further stream behind the first (trailing bytes
that begin with ``BZh1``..``BZh9`` or are a proper prefix of that).  A rejected
frame raises ``OSError("Invalid data stream")``, a truncated one ``ValueError``
with the stdlib's text, both with ``frame_errors`` naming the batch's rejected
frames; see :mod:`numcodecs_amd._bz2` for the launches and read-backs per batch.

Encoding stays on the host: :meth:`BZ2.encode` raises ``NotImplementedError``
(use ``numcodecs.BZ2``; its frames decode here).

The codec is not registered on import: call :func:`register`.
"""

import bz2 as _bz2  # noqa: F401  (the stdlib module: the judge of what this one accepts)

from . import _bz2 as _impl
from .abc import Codec
from .registry import register_codec

__all__ = ["BZ2", "decompress", "decompress_many", "register"]


def decompress_many(frames, outs=None, sizes=None):
    """Decode a list of bzip2 streams (:func:`numcodecs_amd._bz2.decompress_many`):
    host buffers give uint8 numpy arrays, device tensors uint8 device tensors;
    ``outs[i]`` is filled and returned, ``sizes[i]`` skips the sizing launch."""
    return _impl.decompress_many(frames, outs, sizes)


def decompress(source, dest=None):
    """Decode one bzip2 stream; ``dest``, when given, is filled from its start
    and returned."""
    return decompress_many([source], [dest])[0]


class BZ2(Codec):
    """The ``bz2`` codec (numcodecs id ``bz2``): same constructor, config and
    repr as the reference; decode on the GPU, encode not implemented."""

    codec_id = "bz2"

    def __init__(self, level=1):
        self.level = level

    def encode(self, buf):
        raise NotImplementedError("bzip2 compression is not implemented on the GPU; encode with numcodecs.BZ2")

    def decode(self, buf, out=None):
        results, produced = _impl.bunzip_many([buf], [out])
        if out is not None:
            want = len(_impl._frames.out_bytes(out, 0))
            if produced[0] != want:  # the reference copies into `out`, which must be of the very size
                raise ValueError("frame decodes to %d bytes, `out` holds %d" % (produced[0], want))
        return results[0]


def register():
    """Register :class:`BZ2` under ``'bz2'`` in this package's
    ``codec_registry`` (never done on import, and never in numcodecs' own
    registry)."""
    register_codec(BZ2)
