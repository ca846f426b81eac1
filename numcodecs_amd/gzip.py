"""GZip on the GPU, decode only (reference: src/numcodecs/gzip.py).

A frame is one RFC 1952 gzip member: a 10-byte header (FEXTRA, FNAME, FCOMMENT
and FHCRC skipped, their CRC not verified, as ``GzipFile`` does not verify it),
DEFLATE data, a little-endian CRC-32 and ISIZE.  :func:`decompress_many`
inflates a batch with one wave per frame (csrc/mc_inflate.hip; the rules are
csrc/mc_inflate.h's, which follow ``GzipFile.read``): zero bytes after the
trailer are padding, an empty frame is an empty result.  Errors are the
stdlib's classes: ``gzip.BadGzipFile`` (magic, method, CRC, length, trailing
junk), ``EOFError`` (truncation), ``zlib.error`` (a fault inside the DEFLATE
data), each with ``frame_errors`` naming the batch's rejected frames.

A stated limit: a frame of more than one member raises
``NotImplementedError`` (the reference concatenates the members).

Encoding stays on the host: :meth:`GZip.encode` raises ``NotImplementedError``
(use ``numcodecs.GZip``; its frames decode here).

The codec is not registered on import: call :func:`register`.
"""

import gzip as _gzip  # noqa: F401  (the stdlib module: the exceptions raised here are its own)

from . import _inflate
from .abc import Codec
from .registry import register_codec

__all__ = ["GZip", "decompress", "decompress_many", "register"]


def decompress_many(frames, outs=None, sizes=None):
    """Inflate a list of gzip frames (:func:`numcodecs_amd._inflate.decompress_many`
    with the gzip container): host buffers give uint8 numpy arrays, device
    tensors uint8 device tensors; ``outs[i]`` is filled and returned,
    ``sizes[i]`` skips the sizing launch."""
    return _inflate.decompress_many(frames, _inflate.GZIP, outs, sizes)


def decompress(source, dest=None):
    """Inflate one gzip frame; ``dest``, when given, is filled from its start
    and returned."""
    return decompress_many([source], [dest])[0]


class GZip(Codec):
    """The ``gzip`` codec (numcodecs id ``gzip``): same constructor, config and
    repr as the reference; decode on the GPU, encode not implemented.  As in
    the reference, a frame that decodes to more than ``out`` holds raises
    ``ValueError("Unable to fit data into `out`")``; fewer bytes are accepted
    and ``out`` is returned."""

    codec_id = "gzip"

    def __init__(self, level=1):
        self.level = level

    def encode(self, buf):
        raise NotImplementedError("deflate is not implemented on the GPU; encode with numcodecs.GZip")

    def decode(self, buf, out=None):
        return decompress(buf, out)


def register():
    """Register :class:`GZip` under ``'gzip'`` in this package's
    ``codec_registry`` (never done on import, and never in numcodecs' own
    registry)."""
    register_codec(GZip)
