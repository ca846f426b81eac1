"""Zlib on the GPU, decode only (reference: src/numcodecs/zlib.py).

A frame is an RFC 1950 zlib stream: 2 header bytes, DEFLATE data, a 4-byte
big-endian Adler-32.  :func:`decompress_many` inflates a batch with one wave per
frame (csrc/mc_inflate.hip; the rules are csrc/mc_inflate.h's, which follow
``zlib.decompress``): bytes after the trailer are ignored, a preset dictionary
is refused.  A rejected frame raises ``zlib.error`` with the stdlib's text for
the condition and ``frame_errors`` naming the batch's rejected frames; see
:mod:`numcodecs_amd._inflate` for the launches and read-backs per batch.

Encoding stays on the host: :meth:`Zlib.encode` raises ``NotImplementedError``
(use ``numcodecs.Zlib``; its frames decode here).

The codec is not registered on import: call :func:`register`.
"""

import zlib as _zlib  # noqa: F401  (the stdlib module: the exceptions raised here are its own)

from . import _inflate
from .abc import Codec
from .registry import register_codec

__all__ = ["Zlib", "decompress", "decompress_many", "register"]


def decompress_many(frames, outs=None, sizes=None):
    """Inflate a list of zlib frames (:func:`numcodecs_amd._inflate.decompress_many`
    with the zlib container): host buffers give uint8 numpy arrays, device
    tensors uint8 device tensors; ``outs[i]`` is filled and returned,
    ``sizes[i]`` skips the sizing launch."""
    return _inflate.decompress_many(frames, _inflate.ZLIB, outs, sizes)


def decompress(source, dest=None):
    """Inflate one zlib frame; ``dest``, when given, is filled from its start
    and returned."""
    return decompress_many([source], [dest])[0]


class Zlib(Codec):
    """The ``zlib`` codec (numcodecs id ``zlib``): same constructor, config and
    repr as the reference; decode on the GPU, encode not implemented."""

    codec_id = "zlib"

    def __init__(self, level=1):
        self.level = level

    def encode(self, buf):
        raise NotImplementedError("deflate is not implemented on the GPU; encode with numcodecs.Zlib")

    def decode(self, buf, out=None):
        results, produced = _inflate.inflate_many([buf], _inflate.ZLIB, [out])
        if out is not None:
            want = len(_inflate._frames.out_bytes(out, 0))
            if produced[0] != want:  # the reference copies into `out`, which must be of the very size
                raise ValueError("frame decodes to %d bytes, `out` holds %d" % (produced[0], want))
        return results[0]


def register():
    """Register :class:`Zlib` under ``'zlib'`` in this package's
    ``codec_registry`` (never done on import, and never in numcodecs' own
    registry)."""
    register_codec(Zlib)
