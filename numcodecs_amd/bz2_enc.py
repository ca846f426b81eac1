"""BZ2 on the GPU, the write side (reference: src/numcodecs/bz2.py encode).

:func:`compress_many` turns a batch of buffers into bzip2 streams with five
launches (csrc/mc_bz2_enc.hip; the format is csrc/mc_bz2_enc.h's).  A chunk is
cut into independent input segments of ``80000 * level - 16`` bytes; each
becomes one block: RLE1, a forward Burrows-Wheeler transform (a workgroup per
block sorts the rotations by prefix doubling, bounded at ceil(log2 n) rounds
whatever the data), move-to-front with zero runs, and Huffman coding with up
to six tables refined as libbz2 refines them, or equal-length codes where that
is smaller.  ``bz2.decompress`` and any bzip2 decoder read the frames; they are
not byte-equal to libbz2's (another block fill, other code lengths).  They
depend on the input and the level alone.

``level``: 1 ... 9 sets the block size, as in bzip2; anything else raises what
``bz2.compress(b"", level)`` raises, before any launch.  Chunks of 2**30 bytes
and above raise ``ValueError``.  No frame is longer than
``numcodecs_amd._bz2_enc.bound(n, level)``.

:class:`BZ2` is the decode-only class of :mod:`.bz2` with ``encode`` added:
same ``codec_id``, config and repr.  Nothing is registered on import:
:func:`register` puts it under ``'bz2'`` in this package's registry.  The
decode-only module stays as it is."""

from . import _bz2_enc
from . import bz2 as _bz2_mod
from .registry import register_codec

__all__ = ["BZ2", "compress", "compress_many", "register"]


def compress_many(bufs, level=1, outs=None):
    """Encode a list of buffers into bzip2 streams with five launches for all
    of them: host buffers give uint8 numpy arrays, device tensors uint8 device
    tensors, each of exactly its frame's length.  ``outs[i]``, when given,
    holds at least ``_bz2_enc.bound(n, level)`` bytes, is filled from its
    start, and its first frame-length bytes are returned.  One read-back of the
    frames' sizes per call."""
    return _bz2_enc.compress_many(bufs, level, outs)


def compress(buf, level=1):
    """Encode one buffer into a bzip2 stream (see :func:`compress_many`)."""
    return compress_many([buf], level)[0]


class BZ2(_bz2_mod.BZ2):
    """The ``bz2`` codec with both directions on the GPU:
    :class:`numcodecs_amd.bz2.BZ2` (same constructor, config, repr and decode)
    plus ``encode``."""

    def encode(self, buf):
        return compress(buf, self.level)


def register():
    """Register :class:`BZ2` under ``'bz2'`` in this package's
    ``codec_registry`` (never done on import, and never in numcodecs' own
    registry)."""
    register_codec(BZ2)
