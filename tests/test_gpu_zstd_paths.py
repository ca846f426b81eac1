"""GPU zstd decode over the frames written for the code paths that exist only
on the device (tests/zstd_write.py; csrc/mc_zstd.hip: the bit window, the
ballot-and-scan table builders, the four-lane Huffman decode, the three forms
of the match copy through the LDS ring, the striped XXH64).  Every family goes
through the raw binding ``mc_zstd_decode_batch`` in one or two launches, with
guard bytes behind each output: byte-equal to the bytes the writer got from
executing its own sequence list, ``produced`` equal, nothing written behind
it.  The frames that declare no size also go through ``_zstd.decode_many`` by
its three routes.  The invalid frames: the error record equals the host
model's.  What each family holds is asserted on the CPU
(tests/test_zstd_paths_host.py)."""

import pytest
import torch

from numcodecs_amd import _zstd
from tests import zstd_gen as g
from tests import zstd_write as zw
from tests.test_gpu_zstd import _compare_with_host_model, _dev, _device_records  # the raw binding's helpers

pytestmark = pytest.mark.gpu

GUARD = 33  # the capacity passes the largest output by this much: odd, so the outputs lie at every alignment


def _decode_and_compare(cases, cap, device):
    assert cases and max(len(c.data) for c in cases) <= cap
    codes, _words, produced, outs = _device_records([c.frame for c in cases], cap, device)
    for i, c in enumerate(cases):
        n = len(c.data)
        assert codes[i] == 0 and produced[i] == n, (c.name, codes[i], produced[i], n)
        assert outs[i][:n] == c.data, c.name  # the writer's bytes, not a decoder's
        assert outs[i][n:] == b"\xa5" * (cap - n), c.name  # nothing behind what was produced


def _family(name, device, cap=None):
    cases = zw.family(name)
    _decode_and_compare(cases, cap or max(len(c.data) for c in cases) + GUARD, device)


def test_match_forms_in_the_ring_of_256(device):
    _family("match_small", device, cap=256)  # a batch capacity of at most 256: the smallest ring


def test_match_forms_in_the_ring_of_65536(device):
    _decode_and_compare(zw.family("match_small") + zw.family("match_big"), 65536 + GUARD, device)


def test_what_straddles_the_rings_wrap(device):
    _family("wrap", device)


def test_every_length_and_offset_code(device):
    _family("codes", device)


def test_repeat_offsets(device):
    _family("repeat", device)


def test_fse_tables_every_cell_entered(device):
    _family("tables", device)


def test_huffman_trees_and_stream_lengths(device):
    _family("huffman", device)


def test_bit_window_strides_and_alignments(device):
    _family("bits", device)


def test_xxh64_lengths(device):
    _family("xxh64", device)
    # a wrong checksum is told: the word is the one the device computed
    cases = zw.family("xxh64")
    bad = [c.frame[:-1] + bytes([c.frame[-1] ^ 0x40]) for c in cases]
    codes, words, produced, _outs = _device_records(bad, 1100, device)
    for i, c in enumerate(cases):
        assert (codes[i], words[i], produced[i]) == (g.E_CHECK, g.xxh64(c.data) & 0xFFFFFFFF, len(c.data)), c.name


def test_frames_without_a_declared_size_three_ways(device):
    cases = [c for c in zw.cases() if not c.declared]
    assert len(cases) == len(zw.cases()) // 2
    frames = [_dev(c.frame, device) for c in cases]
    sizes = [len(c.data) for c in cases]

    def same(got):
        for c, out in zip(cases, got):
            assert out.numel() == len(c.data) and out.cpu().numpy().tobytes() == c.data, c.name
    got, produced = _zstd.decode_many(frames)  # the sizing pass
    assert produced == sizes
    same(got)
    got, produced = _zstd.decode_many(frames, sizes=[z + 5 for z in sizes])
    assert produced == sizes
    same(got)
    outs = [torch.full((z,), 0xA5, dtype=torch.uint8, device=device) for z in sizes]
    got, produced = _zstd.decode_many(frames, outs=outs)
    assert produced == sizes and all(o is given for o, given in zip(got, outs))
    same(got)


def test_invalid_frames_error_records_equal_the_host_models(device):
    # (only after the sanitized stand-alone run over these frames is clean: tests/test_zstd_paths_host.py)
    _compare_with_host_model([f for _n, f, _cap, _note in zw.invalid_cases()], 128, device)
