"""GPU bz2 decode (numcodecs_amd.bz2; csrc/mc_bz2.hip): the reference's fixture
frames and the generated / hand-built case list of tests/bz2_gen.py through
``decompress_many`` in mixed batches, byte-equal to the stdlib, by all three
routes (the sizing pass, ``sizes=``, device ``outs``) from host and device
inputs; the invalid cases with the host model's code in ``frame_errors``
(tests/native_bz2), the stdlib's exception class and an untouched guard band
behind each destination; both inverse-BWT forms on every block size; the
``out`` rules of the class; a batch of more frames than resident waves.  The
largest input decodes to 250 000 bytes."""

import numpy as np
import pytest
import torch

from numcodecs_amd import _bz2 as impl
from numcodecs_amd import bz2 as nbz2
from tests import bz2_gen as g

pytestmark = pytest.mark.gpu

GUARD = 32


def _dev(data, device):
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).to(device) if len(data) else \
        torch.empty(0, dtype=torch.uint8, device=device)


def _bytes(x):
    return (x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)).tobytes()


def _host(frame):
    return np.frombuffer(frame, np.uint8)


def test_fixture_frames_decode_in_one_call(device):
    fx = g.fixture_frames()
    assert len(fx) == 52
    got = nbz2.decompress_many([_host(f) for _i, _j, _raw, f in fx])
    for (i, j, raw, _f), out in zip(fx, got):
        assert isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.tobytes() == raw, (i, j)
    got = nbz2.decompress_many([_dev(f, device) for _i, _j, _raw, f in fx])
    for (i, j, raw, _f), out in zip(fx, got):
        assert out.is_cuda and out.dtype == torch.uint8 and _bytes(out) == raw, (i, j)


def test_valid_cases_three_ways(device):
    cases = g.valid_cases()
    frames = [_dev(f, device) if k % 2 else _host(f) for k, (_n, f, _d) in enumerate(cases)]  # a mixed batch
    # no sizes: through the sizing pass
    got, produced = impl.bunzip_many(frames)
    for k, ((name, _f, data), out, p) in enumerate(zip(cases, got, produced)):
        assert p == len(data) and _bytes(out) == data, name
        assert torch.is_tensor(out) == bool(k % 2), name
    # sizes= (one of them generous: a size is an upper bound), from host frames
    sizes = [len(d) + (5 if k == 3 else 0) for k, (_n, _f, d) in enumerate(cases)]
    got, produced = impl.bunzip_many([_host(f) for _n, f, _d in cases], sizes=sizes)
    for (name, _f, data), out, p in zip(cases, got, produced):
        assert isinstance(out, np.ndarray) and p == len(data) and out.tobytes() == data, name
    # device outs, with guard bytes behind each
    outs = [torch.full((len(d) + GUARD,), 0xA5, dtype=torch.uint8, device=device) for _n, _f, d in cases]
    got, produced = impl.bunzip_many(frames, outs=[o[:len(d)] for o, (_n, _f, d) in zip(outs, cases)])
    for (name, _f, data), o, p in zip(cases, outs, produced):
        assert p == len(data) and _bytes(o[:len(data)]) == data, name
        assert bool((o[len(data):] == 0xA5).all()), name


@pytest.mark.parametrize("multi_min", [2, 4000000])
def test_both_inverse_bwt_forms_on_every_block_size(device, monkeypatch, multi_min):
    """Multi-start on the smallest blocks (one symbol, fewer than 64, several
    cycles) and the one-lane chase on the largest: the same bytes."""
    monkeypatch.setattr(impl, "MULTI_MIN", multi_min)
    cases = [c for c in g.valid_cases() if multi_min == 2 or c[0] != "random-250000-l9"]
    got = nbz2.decompress_many([_host(f) for _n, f, _d in cases])
    for (name, _f, data), out in zip(cases, got):
        assert out.tobytes() == data, name


def test_invalid_cases(device):
    bad = g.invalid_cases()
    model = {name: g.host_decode(frame) for name, frame in bad}
    assert all(rc for rc, _o, _w in model.values())
    good = [(n, f, d) for n, f, d in g.valid_cases() if len(d) < 10000][:8]
    # one batch, a destination with a guard band for every frame: the model's code and word for each bad frame
    batch, where, sizes = [], {}, []
    for k, (name, frame) in enumerate(bad):
        if k < len(good):
            batch.append(good[k][1])
            sizes.append(len(good[k][2]))
        where[len(batch)] = name
        batch.append(frame)
        sizes.append(g.host_count(frame)[1])
    outs = [torch.full((n + GUARD,), 0xA5, dtype=torch.uint8, device=device) for n in sizes]
    kinds = (OSError, ValueError, NotImplementedError)
    with pytest.raises(kinds) as e:
        nbz2.decompress_many([_dev(f, device) if k % 3 else _host(f) for k, f in enumerate(batch)],
                             outs=[o[:n] for o, n in zip(outs, sizes)])
    assert e.value.frame_errors == {k: (model[name][0], model[name][2]) for k, name in where.items()}
    for k, (o, n) in enumerate(zip(outs, sizes)):
        assert bool((o[n:] == 0xA5).all()), where.get(k, k)
    # without destinations or sizes the sizing pass makes every check and raises before anything is decoded
    with pytest.raises(kinds) as e:
        nbz2.decompress_many([_host(f) for f in batch])
    assert e.value.frame_errors == {k: (model[name][0], model[name][2]) for k, name in where.items()}
    # alone, one frame per code: the stdlib's class and text
    seen = set()
    for name, frame in bad:
        rc = model[name][0]
        if rc in seen and not name.startswith("cut-long"):
            continue
        seen.add(rc)
        if name in g.DEPARTURES:
            with pytest.raises(NotImplementedError) as e:
                nbz2.decompress(_dev(frame, device))
        else:
            std = g.stdlib_decode(frame)
            with pytest.raises(std[1]) as e:
                nbz2.decompress(_dev(frame, device))
            assert type(e.value) is std[1] and str(e.value) == std[2], name
        assert e.value.frame_errors == {0: (rc, model[name][2])}, name
    assert len(seen) >= 15
    # a clean re-call: the good frames still decode
    got = nbz2.decompress_many([_host(f) for _n, f, _d in good])
    for (name, _f, data), out in zip(good, got):
        assert out.tobytes() == data, name


def test_capacity_is_respected(device):
    cases = [(n, f, d) for n, f, d in g.valid_cases() if 0 < len(d) <= 100000]
    outs = [torch.full((len(d) - 1 + GUARD,), 0xA5, dtype=torch.uint8, device=device) for _n, _f, d in cases]
    with pytest.raises(ValueError, match="decodes to more than the") as e:
        nbz2.decompress_many([_host(f) for _n, f, _d in cases], outs=[o[:len(d) - 1] for o, (_n, _f, d) in zip(outs, cases)])
    assert {k: v[0] for k, v in e.value.frame_errors.items()} == {k: impl.E_CAPACITY for k in range(len(cases))}
    for (name, _f, d), o in zip(cases, outs):
        assert bool((o[len(d) - 1:] == 0xA5).all()), name


def test_class_decode_and_out(device):
    import bz2 as _bz2

    data = g.noise(5000, 3) + bytes(700)
    frame = _bz2.compress(data, 3)
    codec = nbz2.BZ2(3)
    assert _bytes(codec.decode(frame)) == data
    out = torch.zeros(len(data), dtype=torch.uint8, device=device)
    assert codec.decode(_dev(frame, device), out=out) is out and _bytes(out) == data
    host_out = np.zeros(len(data), np.uint8)
    assert codec.decode(frame, out=host_out) is host_out and host_out.tobytes() == data
    with pytest.raises(ValueError, match="`out` holds"):
        codec.decode(frame, out=np.zeros(len(data) + 1, np.uint8))
    with pytest.raises(ValueError, match="decodes to more than"):
        codec.decode(frame, out=np.zeros(len(data) - 1, np.uint8))
    assert _bytes(nbz2.decompress(frame, torch.zeros(len(data) + 9, dtype=torch.uint8, device=device))[:len(data)]) == data


def test_more_frames_than_resident_waves(device):
    """1000 level-1 frames: the grid is 768 waves, the rest come off the counter."""
    small = [(n, f, d) for n, f, d in g.valid_cases() if len(d) < 6000 and f[3:4] == b"1"]
    assert len(small) >= 30
    cases = [small[k % len(small)] for k in range(1000)]
    got = nbz2.decompress_many([_host(f) for _n, f, _d in cases])
    for k, ((name, _f, data), out) in enumerate(zip(cases, got)):
        assert out.tobytes() == data, (k, name)
