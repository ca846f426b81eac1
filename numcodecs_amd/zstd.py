"""Zstd on the GPU, decode only (reference: src/numcodecs/zstd.pyx).

A frame is one RFC 8878 Zstandard frame.  :func:`decompress_many` decodes a
batch with one wave per frame (csrc/mc_zstd.hip; the rules are
csrc/mc_zstd.h's, which follow libzstd's ``ZSTD_decompress`` where the RFC
leaves a choice).  Refused: a dictionary, a second or a skippable frame in the
same buffer (``NotImplementedError``: the reference would concatenate or skip),
frames and outputs of 2**30 bytes and above.  A rejected frame raises the
reference's ``RuntimeError`` with its text for the condition and
``frame_errors`` naming the batch's rejected frames; see
:mod:`numcodecs_amd._zstd` for the launches and read-backs per batch.

This module is decode only: :meth:`Zstd.encode` raises ``NotImplementedError``
(use ``numcodecs.Zstd``; its frames decode here).  The write side on the GPU
is :mod:`numcodecs_amd.zstd_enc`, whose ``Zstd`` is this class with ``encode``
added.

The codec is not registered on import: call :func:`register`.
"""

from . import _zstd
from .abc import Codec
from .registry import register_codec

__all__ = ["Zstd", "decompress", "decompress_many", "register"]

DEFAULT_CLEVEL = 0


def decompress_many(frames, outs=None, sizes=None):
    """Decode a list of Zstandard frames, one wave per frame.

    Each frame is a host buffer or a device tensor; each result is a flat uint8
    numpy array or device tensor accordingly.  ``outs`` may give, per frame,
    None or a destination (device tensor or writable host buffer), which is
    filled from its start and returned in place of a new array; ``sizes`` may
    give, per frame, None or the number of bytes the frame decodes to at most.
    A frame that declares its size, or comes with either, skips the sizing
    launch.  Host frames go up in one upload and host results come down in one
    download.  Errors: see :mod:`numcodecs_amd._zstd`."""
    return _zstd.decode_many(frames, outs, sizes)[0]


def decompress(source, dest=None):
    """Decode one Zstandard frame; ``dest``, when given, is filled from its
    start and returned.  A frame that declares no size must fill ``dest``."""
    return decompress_many([source], [dest])[0]


class Zstd(Codec):
    """The ``zstd`` codec (numcodecs id ``zstd``): same constructor, config and
    repr as the reference; decode on the GPU, encode not implemented."""

    codec_id = "zstd"

    def __init__(self, level=DEFAULT_CLEVEL, checksum=False):
        self.level = level
        self.checksum = checksum

    def encode(self, buf):
        raise NotImplementedError("zstd compression is not implemented on the GPU; encode with numcodecs.Zstd")

    def decode(self, buf, out=None):
        return decompress(buf, out)

    def __repr__(self):
        return "%s(level=%r)" % (type(self).__name__, self.level)

    # libzstd's own answers (1.4.8 and later): there is no libzstd here to ask
    @classmethod
    def default_level(cls):
        """The default compression level of libzstd."""
        return 3

    @classmethod
    def min_level(cls):
        """The minimum compression level of libzstd."""
        return -131072

    @classmethod
    def max_level(cls):
        """The maximum compression level of libzstd."""
        return 22


def register():
    """Register :class:`Zstd` under ``'zstd'`` in this package's
    ``codec_registry`` (never done on import, and never in numcodecs' own
    registry)."""
    register_codec(Zstd)
