"""The split access policy (| 1024 default-policy stores, | 2048 default-policy
loads) and the tile order of one chunk (bits 12-14: 2^(k+2) virtual rows) of
the five large-chunk Shuffle kernels, through the lab entry points with an
explicit variant word: encodes against the oracle's bytes, decodes against the
input, every output between two 4 KiB sentinels that must stay untouched.
Then the default path of one chunk just over 64 MiB through the public API."""

import functools

import numpy as np
import pytest
import torch

import oracle
from numcodecs_amd import BitRound, Shuffle, batch
from tests.helpers import lab_lib

pytestmark = pytest.mark.gpu

V_NO_NT, V_ST_PLAIN, V_LD_PLAIN, V_VROWS_SHIFT = 8, 1024, 2048, 12
POLICIES = (0, V_ST_PLAIN, V_LD_PLAIN, V_ST_PLAIN | V_LD_PLAIN, V_NO_NT | V_ST_PLAIN, V_NO_NT | V_LD_PLAIN)
R32, R256 = 3 << V_VROWS_SHIFT, 6 << V_VROWS_SHIFT
NTILES = (1, 31, 32, 33, 67, 128)
GUARD = 4096
SENTINEL = 0xC7

# kernel -> (es, encode, layout word, tile bytes, BitRound keepbits or None)
KERNELS = {
    "k_shuffle_enc<4,QMUL8>": (4, 1, 1 | 512, 128 << 10, None),
    "k_shuffle_enc<4,QMUL4>": (4, 1, 1 | 128, 64 << 10, None),
    "k_bitround_shuffle4_planes<0,QMUL4>": (4, 1, 1 | 128, 64 << 10, 20),
    "k_bitround_shuffle4_planes<1,QMUL4>": (4, 1, 1 | 128, 64 << 10, 10),
    "k_bitround_shuffle4_planes<2,QMUL4>": (4, 1, 1 | 128, 64 << 10, 3),
    "k_shuffle4_dec_pair<QMUL2>": (4, 0, 5 | 16, 32 << 10, None),
    "k_shuffle8_enc_pair<NV4>": (8, 1, 5, 16 << 10, None),
    "k_shuffle8_dec_pair<NV8>": (8, 0, 5 | 16, 32 << 10, None),
}


@functools.lru_cache(maxsize=None)
def _case(es, nbytes, keepbits):
    """(plain bytes, encoded bytes) of one size, both on the host, computed once"""
    rng = np.random.default_rng(nbytes * 31 + es)
    x = rng.integers(0, 256, nbytes, dtype=np.uint8)
    if keepbits is None:
        return x, oracle.nporacle.shuffle(x, es)
    with np.errstate(all="ignore"):
        rounded = oracle.nporacle.bitround_encode(x.view("<f4"), keepbits)
    return x, oracle.nporacle.shuffle(rounded, 4)


def _guarded(nbytes, device):
    buf = torch.full((nbytes + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device=device)
    return buf, buf[GUARD: GUARD + nbytes]


def _guards_intact(buf, nbytes):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + nbytes:] == SENTINEL).all())


def _run(lib, kernel, word, src, dst, nbytes, st):
    es, enc, _, _, keep = KERNELS[kernel]
    if keep is None:
        return lib.mc_lab_shuffle_variant(src.data_ptr(), dst.data_ptr(), nbytes, es, enc, word, 0, st)
    return lib.mc_lab_bitround_shuffle_variant(src.data_ptr(), dst.data_ptr(), nbytes // 4, 4, keep, word, 0, st)


def _check(lib, device, kernel, nbytes, words):
    es, enc, layout, _, keep = KERNELS[kernel]
    st = torch.cuda.current_stream().cuda_stream
    plain, encoded = _case(es, nbytes, keep)
    src = torch.from_numpy(encoded if not enc else plain).to(device)
    want = torch.from_numpy(plain if not enc else encoded).to(device)
    for bits in words:
        buf, dst = _guarded(nbytes, device)
        assert _run(lib, kernel, layout | bits, src, dst, nbytes, st) == 0, (kernel, nbytes, bits)
        assert torch.equal(dst, want), (kernel, nbytes, bits)
        assert _guards_intact(buf, nbytes), (kernel, nbytes, bits)


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_policy_and_order_bits(device, kernel):
    lib = lab_lib()
    es, _, layout, tile, _ = KERNELS[kernel]
    # 32 virtual rows on tile counts around the row count, each with 4 tail elements
    for ntiles in NTILES:
        _check(lib, device, kernel, ntiles * tile + 4 * es, [R32 | p for p in POLICIES[:4]])
    # every policy x every order the dispatch accepts, 67 tiles + tail
    every = [p | (k << V_VROWS_SHIFT) for p in POLICIES for k in range(7)]
    _check(lib, device, kernel, 67 * tile + 4 * es, every)
    # more rows than tiles
    _check(lib, device, kernel, 33 * tile + 4 * es, [R256 | p for p in POLICIES[:4]])
    # order code 7 names no row count
    st = torch.cuda.current_stream().cuda_stream
    x = torch.zeros(tile, dtype=torch.uint8, device=device)
    y = torch.zeros(tile, dtype=torch.uint8, device=device)
    assert _run(lib, kernel, layout | (7 << V_VROWS_SHIFT), x, y, tile, st) != 0


@pytest.mark.parametrize("es,enc,layout", [(4, 1, 1 | 512), (4, 0, 5 | 16), (8, 1, 5), (8, 0, 5 | 16)])
def test_batch_ignores_order_bits(device, es, enc, layout):
    """3 chunks at a stride above the chunk bytes: the order bits change nothing"""
    lib = lab_lib()
    st = torch.cuda.current_stream().cuda_stream
    nchunks, nbytes, pad = 3, 9 * (128 << 10) + 4 * es, 4096
    stride = nbytes + pad
    rng = np.random.default_rng(7)
    plain = rng.integers(0, 256, (nchunks, nbytes), dtype=np.uint8)
    encoded = np.stack([oracle.nporacle.shuffle(plain[c], es) for c in range(nchunks)])
    src_np, want_np = (plain, encoded) if enc else (encoded, plain)
    src = torch.full((nchunks, stride), SENTINEL, dtype=torch.uint8, device=device)
    src[:, :nbytes] = torch.from_numpy(src_np).to(device)
    want = torch.from_numpy(want_np).to(device)
    outs = []
    for bits in (0, R32, R256 | V_ST_PLAIN, R32 | V_LD_PLAIN):
        buf = torch.full((GUARD + nchunks * stride + GUARD,), SENTINEL, dtype=torch.uint8, device=device)
        dst = buf[GUARD: GUARD + nchunks * stride].view(nchunks, stride)
        rc = lib.mc_lab_shuffle_batch_variant(src.data_ptr(), stride, dst.data_ptr(), stride, nchunks, nbytes, es,
                                              enc, layout | bits, 0, st)
        assert rc == 0, (es, enc, bits)
        assert torch.equal(dst[:, :nbytes], want), (es, enc, bits)
        assert bool((dst[:, nbytes:] == SENTINEL).all()), (es, enc, bits)
        assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all()), (es, enc, bits)
        outs.append(buf)
    for other in outs[1:]:
        assert torch.equal(other, outs[0])


# ---------------------------------------------------------------------------
# the default path: one chunk of 64 MiB + 4 elements, the smallest total at
# which the default schedule is a large-chunk kernel
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("es", [4, 8])
def test_default_large_chunk_shuffle(device, es):
    nbytes = (64 << 20) + 4 * es
    x = np.random.default_rng(es).integers(0, 256, nbytes, dtype=np.uint8)
    xd = torch.from_numpy(x).to(device)
    enc = Shuffle(es).encode(xd)
    assert torch.equal(enc, torch.from_numpy(oracle.nporacle.shuffle(x, es)).to(device)), es
    assert torch.equal(Shuffle(es).decode(enc), xd), es


def test_default_large_chunk_bitround_shuffle(device):
    count = (16 << 20) + 4
    x = np.random.default_rng(3).integers(0, 2**32, count, dtype=np.uint64).astype(np.uint32).view("<f4")
    xd = torch.from_numpy(x.copy()).to(device)
    pipe = batch.FilterPipeline([BitRound(10), Shuffle(4)])
    enc = pipe.encode(xd)
    with np.errstate(all="ignore"):
        rounded = oracle.nporacle.bitround_encode(x.copy(), 10)
    ref = oracle.nporacle.shuffle(rounded, 4)
    assert torch.equal(enc.view(torch.uint8), torch.from_numpy(ref).to(device))
    # BitRound decodes by re-viewing, so the pipeline gives the rounded values back
    dec = pipe.decode(enc)
    dec = dec.cpu().numpy() if torch.is_tensor(dec) else np.asarray(dec)
    assert dec.view(np.uint8).reshape(-1).tobytes() == rounded.view(np.uint8).tobytes()
