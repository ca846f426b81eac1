"""Zstd on the GPU, the write side (reference: src/numcodecs/zstd.pyx compress).

:func:`compress_many` turns a batch of buffers into Zstandard (RFC 8878)
frames with four launches (csrc/mc_zstd_enc.hip; the format is
csrc/mc_zstd_enc.h's).  A chunk is cut into independent 64 KiB segments; one
wave per segment finds the matches (the deflate encoder's window-of-64 finder
with the distance limit lifted to the segment), Huffman-codes the literals,
FSE-codes the sequences and writes whichever of a raw, an RLE and a compressed
block is smallest.  Any Zstandard decoder reads the frames (they declare their
content size, as the reference's ``decode`` needs); they are not byte-equal to
libzstd's (another match finder, no matches or repeat offsets across segments,
no treeless literals, no repeat-mode tables).  They depend on the input alone.

``level``: any int is accepted and all levels take the one parse (libzstd
clamps a level out of range without raising, so the reference accepts them
too); a non-int raises ``TypeError``.  ``checksum=True`` appends the content
checksum.  Chunks of 2**30 bytes and above raise ``ValueError``.  No frame is
longer than ``numcodecs_amd._zstd_enc.bound(n, checksum)``.

:class:`Zstd` is the decode-only class of :mod:`.zstd` with ``encode`` added:
same ``codec_id``, config and repr.  Nothing is registered on import:
:func:`register` puts it under ``'zstd'`` in this package's registry.  The
decode-only module stays as it is."""

from . import _zstd_enc
from . import zstd as _zstd_mod
from .registry import register_codec

__all__ = ["Zstd", "compress", "compress_many", "register"]


def compress_many(bufs, level=0, checksum=False, outs=None):
    """Encode a list of buffers into Zstandard frames with four launches for
    all of them: host buffers give uint8 numpy arrays, device tensors uint8
    device tensors, each of exactly its frame's length.  ``outs[i]``, when
    given, holds at least ``_zstd_enc.bound(n, checksum)`` bytes, is filled
    from its start, and its first frame-length bytes are returned.  One
    read-back of the frames' sizes per call."""
    return _zstd_enc.compress_many(bufs, level, checksum, outs)


def compress(buf, level=0, checksum=False):
    """Encode one buffer into a Zstandard frame (see :func:`compress_many`)."""
    return compress_many([buf], level, checksum)[0]


class Zstd(_zstd_mod.Zstd):
    """The ``zstd`` codec with both directions on the GPU:
    :class:`numcodecs_amd.zstd.Zstd` (same constructor, config, repr and decode)
    plus ``encode``."""

    def encode(self, buf):
        return compress(buf, self.level, self.checksum)


def register():
    """Register :class:`Zstd` under ``'zstd'`` in this package's
    ``codec_registry`` (never done on import, and never in numcodecs' own
    registry)."""
    register_codec(Zstd)
