"""GPU inflate (numcodecs_amd.zlib / numcodecs_amd.gzip; csrc/mc_inflate.hip):
the reference's fixture frames and the generated / hand-built case list of
tests/inflate_gen.py through ``decompress_many``, byte-equal to the stdlib, by
all three routes (the sizing pass, ``sizes=``, device ``outs``); the invalid
cases with the stdlib's exception class (and text, for zlib) and
``frame_errors``; a bounded corruption check against the stdlib; the kernel's
error record against the host model of the same header (tests/native_inflate);
the ``out`` rules of both classes; a 64 x 64 KiB batch.  Each test is one or two
calls; no frame decodes to more than ~130 KB."""

import gzip as _gzip
import zlib as _zlib

import numpy as np
import pytest
import torch

from numcodecs_amd import _inflate
from numcodecs_amd import gzip as ngzip
from numcodecs_amd import zlib as nzlib
from tests import inflate_gen as g

pytestmark = pytest.mark.gpu

MODULES = {"zlib": nzlib, "gzip": ngzip}


def _dev(data, device):
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).to(device) if len(data) else \
        torch.empty(0, dtype=torch.uint8, device=device)


def _bytes(x):
    return (x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)).tobytes()


def _host(frame):
    return np.frombuffer(frame, np.uint8)


@pytest.mark.parametrize("container", ["zlib", "gzip"])
def test_fixture_frames_decode_in_one_call(device, container):
    fx = g.fixture_frames(container)
    assert len(fx) == 78
    mod = MODULES[container]
    got = mod.decompress_many([_host(f) for _i, _j, _raw, f in fx])
    for (i, j, raw, _f), out in zip(fx, got):
        assert isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.tobytes() == raw, (i, j)
    got = mod.decompress_many([_dev(f, device) for _i, _j, _raw, f in fx])
    for (i, j, raw, _f), out in zip(fx, got):
        assert out.is_cuda and out.dtype == torch.uint8 and _bytes(out) == raw, (i, j)


@pytest.mark.parametrize("container", ["zlib", "gzip"])
def test_valid_cases_three_ways(device, container):
    cases = [(n, f, d) for n, c, f, d in g.valid_cases() if c == container]
    assert len(cases) == (28 if container == "zlib" else 30)  # 22 from the stdlib, 6 hand-built, 2 gzip-only
    frames = [_dev(f, device) for _n, f, _d in cases]
    # no sizes: through the sizing pass
    got, produced = _inflate.inflate_many(frames, g.CONTAINERS[container])
    for (name, _f, data), out, p in zip(cases, got, produced):
        assert p == len(data) and _bytes(out) == data, name
    # sizes= (one of them generous: a size is an upper bound), from host frames
    sizes = [len(d) + (5 if k == 3 else 0) for k, (_n, _f, d) in enumerate(cases)]
    got, produced = _inflate.inflate_many([_host(f) for _n, f, _d in cases], g.CONTAINERS[container], sizes=sizes)
    for (name, _f, data), out, p in zip(cases, got, produced):
        assert isinstance(out, np.ndarray) and p == len(data) and out.tobytes() == data, name
    # device outs, with guard bytes behind each
    outs = [torch.full((len(d) + 16,), 0xA5, dtype=torch.uint8, device=device) for _n, _f, d in cases]
    got, produced = _inflate.inflate_many(frames, g.CONTAINERS[container], outs=[o[:len(d)] for o, (_n, _f, d) in zip(outs, cases)])
    for (name, _f, data), o, p in zip(cases, outs, produced):
        assert p == len(data) and _bytes(o[:len(data)]) == data, name
        assert bool((o[len(data):] == 0xA5).all()), name


def _expect(container, frame):
    kind = g.stdlib_decode(container, frame)
    assert kind[0] == "error"
    return kind[1], kind[2]


@pytest.mark.parametrize("container", ["zlib", "gzip"])
def test_invalid_cases(device, container):
    mod = MODULES[container]
    bad = [(n, f) for n, c, f in g.invalid_cases() if c == container]
    good = [(n, f, d) for n, c, f, d in g.valid_cases() if c == container and len(d) < 10000][:6]
    for name, frame in bad:  # each alone: the stdlib's class, and its text for zlib
        if name == "gzip-two-members":  # the stated limit: the stdlib concatenates the members
            with pytest.raises(NotImplementedError) as e:
                mod.decompress(_dev(frame, device))
            assert e.value.frame_errors == {0: (_inflate.E_GZ_MEMBER, 3000)}
            continue
        cls, text = _expect(container, frame)
        with pytest.raises(cls) as e:
            mod.decompress(_dev(frame, device))
        assert type(e.value) is cls, name
        if container == "zlib":
            assert str(e.value) == text, name
        assert set(e.value.frame_errors) == {0}, name
    # mixed into one batch with good frames: frame_errors names exactly the bad ones
    batch, where = [], {}
    for k, (name, frame) in enumerate(bad):
        if k < len(good):
            batch.append(good[k][1])
        where[len(batch)] = name
        batch.append(frame)
    kinds = (_zlib.error, _gzip.BadGzipFile, EOFError, NotImplementedError)
    caps = [g.host_count(container, f)[1] for f in batch]
    with pytest.raises(kinds) as e:  # with sizes: one decode, every bad frame in one record
        mod.decompress_many([_host(f) for f in batch], sizes=caps)
    assert set(e.value.frame_errors) == set(where)
    # without: what the sizing pass finds (header and DEFLATE faults) is raised before anything is decoded
    with pytest.raises(kinds) as e:
        mod.decompress_many([_host(f) for f in batch])
    assert set(e.value.frame_errors) == {k for k in where if g.host_count(container, batch[k])[0]}
    assert 0 < len(e.value.frame_errors) < len(where)
    # a clean re-call: the good frames still decode
    got = mod.decompress_many([_host(f) for _n, f, _d in good])
    for (name, _f, data), out in zip(good, got):
        assert out.tobytes() == data, name


@pytest.mark.parametrize("container", ["zlib", "gzip"])
def test_bounded_corruption_against_the_stdlib(device, container):
    frame, data, muts = g.corruption_frames(container)
    assert len(data) == 4096 and len(muts) == 200
    expect = [g.stdlib_decode(container, m) for m in muts]
    rejected = {k for k, x in enumerate(expect) if x[0] == "error"}
    print(f"{container}: the stdlib rejects {len(rejected)} of {len(muts)}")
    frames = [_host(m) for m in muts]
    errors = {}
    try:
        _inflate.inflate_many(frames, g.CONTAINERS[container])
    except (_zlib.error, _gzip.BadGzipFile, EOFError, NotImplementedError, ValueError) as e:
        errors = e.frame_errors
    assert set(errors) <= rejected, sorted(set(errors) - rejected)  # found by the sizing pass: DEFLATE faults only
    keep = [k for k in range(len(muts)) if k not in errors]
    try:
        got = _inflate.inflate_many([frames[k] for k in keep], g.CONTAINERS[container])[0]
        errors2 = {}
    except (_zlib.error, _gzip.BadGzipFile, EOFError, NotImplementedError, ValueError) as e:
        errors2 = {keep[k]: v for k, v in e.frame_errors.items()}
        got = None
    assert set(errors) | set(errors2) == rejected
    if got is None:  # the frames both accept: bytes equal
        keep = [k for k in keep if k not in errors2]
        got = _inflate.inflate_many([frames[k] for k in keep], g.CONTAINERS[container])[0]
    for k, out in zip(keep, got):
        assert out.tobytes() == expect[k][1], k


def test_error_record_equals_the_host_model(device):
    """Code and second word, for every hand-built case (and the container
    faults), decoded into the capacity the host model counted."""
    for container in ("zlib", "gzip"):
        cases = [(n, f) for n, c, f in g.invalid_cases() if c == container] + \
                [(n, f) for n, c, f, _d in g.valid_cases() if c == container and n in
                 {x[0] for x in g.handbuilt_valid()}]
        caps = [g.host_count(container, f)[1] for _n, f in cases]
        model = [g.host_decode(container, f, cap) for (_n, f), cap in zip(cases, caps)]
        errors = {}
        try:
            produced = _inflate.inflate_many([_dev(f, device) for _n, f in cases], g.CONTAINERS[container], sizes=caps)[1]
        except Exception as e:  # noqa: BLE001  (whatever class the first bad frame maps to)
            errors, produced = e.frame_errors, None
        for k, ((name, _f), (rc, out, word, _cons)) in enumerate(zip(cases, model)):
            if rc:
                assert errors.get(k) == (rc, word - (1 << 32) if word >= (1 << 31) else word), (container, name)
            else:
                assert k not in errors, (container, name)
        assert produced is None or not any(m[0] for m in model)


def test_out_rules_of_both_classes(device):
    d = g.smooth(3000, 6)
    z, gz = g.zlib_wrap(g.raw_deflate(d), d), g.gzip_wrap(g.raw_deflate(d), d)
    for codec, frame in ((nzlib.Zlib(), z), (ngzip.GZip(), gz)):
        assert _bytes(codec.decode(frame)) == d
        assert _bytes(codec.decode(_dev(frame, device))) == d
        out = np.zeros(3000, np.uint8)
        assert codec.decode(frame, out=out) is out and out.tobytes() == d
        out = torch.zeros(750, dtype=torch.float32, device=device)
        assert codec.decode(_dev(frame, device), out=out) is out and _bytes(out.view(torch.uint8)) == d
        with pytest.raises(ValueError) as e:
            codec.decode(frame, out=np.zeros(2999, np.uint8))
        if codec.codec_id == "gzip":
            assert str(e.value) == "Unable to fit data into `out`"
    big = np.full(3100, 7, np.uint8)
    with pytest.raises(ValueError):
        nzlib.Zlib().decode(z, out=big)  # Zlib: the very size
    assert ngzip.GZip().decode(gz, out=big) is big  # GZip: fewer bytes are accepted
    assert big[:3000].tobytes() == d and (big[3000:] == 7).all()
    assert _bytes(ngzip.decompress(b"")) == b""  # an empty gzip frame is an empty result, as GzipFile reads it


def test_batch_of_64_mixed(device):
    rng = np.random.default_rng(17)
    datas, frames = [], []
    for k in range(64):
        kind = k % 4
        d = (g.smooth(65536, 100 + k) if kind == 0 else bytes(65536) if kind == 1 else
             g.noise(65536, 200 + k) if kind == 2 else g.runs(65536, 300 + k))
        level = int(rng.integers(1, 10))
        frames.append(g.zlib_wrap(g.raw_deflate(d, level), d))
        datas.append(d)
    srcs = [(_dev(f, device) if k % 2 else _host(f)) for k, f in enumerate(frames)]
    got = nzlib.decompress_many(srcs)
    for k, (d, out) in enumerate(zip(datas, got)):
        assert (out.is_cuda if k % 2 else isinstance(out, np.ndarray)), k
        assert _bytes(out) == d, k
