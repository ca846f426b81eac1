"""Deflate on the GPU: the write side of the ``zlib`` and ``gzip`` codecs
(reference: src/numcodecs/zlib.py, gzip.py).

:func:`compress_many` turns a batch of buffers into zlib (RFC 1950) or gzip
(RFC 1952) frames with four launches (csrc/mc_deflate.hip; the format is
csrc/mc_deflate.h's).  A chunk is cut into independent 64 KiB segments; one
wave per segment finds the matches (the LZ4 encoder's window-of-64 finder with
DEFLATE's limits), builds dynamic Huffman codes for what it found, and writes
whichever of a stored, a fixed-Huffman and a dynamic-Huffman block is smallest.
Any inflater decodes the frames; they are not byte-equal to zlib's (another
match finder, no matches across segments, no 16/17/18 repeat codes in the code
description).  They depend on the input alone: a gzip frame carries MTIME 0
where the reference writes the wall clock.

``level`` follows the stdlib's rules: -1 and 1 ... 9 all take the one parse (the
finder has no levels), 0 writes stored blocks, anything else raises, at encode
time, what ``zlib.compress(b"", level)`` raises.  Chunks of 2**30 bytes and
above raise ``ValueError``.  No frame is longer than
``numcodecs_amd._deflate.bound(n, container)``.

:class:`Zlib` and :class:`GZip` are the decode-only classes of :mod:`.zlib`
and :mod:`.gzip` with ``encode`` added: same ``codec_id``, config and repr.
Nothing is registered on import: :func:`register` puts both under ``'zlib'``
and ``'gzip'`` in this package's registry.  The decode-only modules stay as
they are."""

from . import _deflate
from . import gzip as _gzip_mod
from . import zlib as _zlib_mod
from .registry import register_codec

__all__ = ["Zlib", "GZip", "compress", "compress_many", "register"]


def _container(container):
    try:
        return _deflate.CONTAINERS[container]
    except (KeyError, TypeError):
        raise ValueError("container must be 'zlib' or 'gzip', not %r" % (container,)) from None


def compress_many(bufs, container="zlib", level=1, outs=None):
    """Deflate a list of buffers into ``container`` frames with four launches
    for all of them: host buffers give uint8 numpy arrays, device tensors uint8
    device tensors, each of exactly its frame's length.  ``outs[i]``, when
    given, holds at least ``_deflate.bound(n, container)`` bytes, is filled from
    its start, and its first frame-length bytes are returned.  One read-back of
    the frames' sizes per call."""
    return _deflate.compress_many(bufs, _container(container), level, outs)


def compress(buf, container="zlib", level=1):
    """Deflate one buffer into a ``container`` frame (see :func:`compress_many`)."""
    return compress_many([buf], container, level)[0]


class Zlib(_zlib_mod.Zlib):
    """The ``zlib`` codec with both directions on the GPU: :class:`numcodecs_amd.zlib.Zlib`
    (same constructor, config, repr and decode) plus ``encode``."""

    def encode(self, buf):
        return compress(buf, "zlib", self.level)


class GZip(_gzip_mod.GZip):
    """The ``gzip`` codec with both directions on the GPU: :class:`numcodecs_amd.gzip.GZip`
    (same constructor, config, repr and decode) plus ``encode``.  MTIME is 0."""

    def encode(self, buf):
        return compress(buf, "gzip", self.level)


def register():
    """Register :class:`Zlib` under ``'zlib'`` and :class:`GZip` under
    ``'gzip'`` in this package's ``codec_registry`` (never done on import, and
    never in numcodecs' own registry)."""
    register_codec(Zlib)
    register_codec(GZip)
