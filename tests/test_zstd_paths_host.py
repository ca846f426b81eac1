"""zstd decode, the frames written for the wave-only code paths
(tests/zstd_write.py), CPU side: the census of what the writer put into each
family, item by item; every valid frame through the product's scalar model
(csrc/mc_zstd.h, compiled for the host) and its count-only mode, byte-equal to
the writer's own execution of its sequence list; the same through libzstd where
it loads; the regenerated frames against the hashes and libzstd 1.4.8 verdicts
recorded in tests/golden/zstd_paths.json; the invalid frames' verdicts; and the
sanitized stand-alone run over all of them."""

import collections
import json
import os
import subprocess

import pytest

from tests import zstd_gen as g
from tests import zstd_write as zw

CASES = zw.cases()
INVALID = zw.invalid_cases()
LIB = g.load_lib()
needs_lib = pytest.mark.skipif(LIB is None, reason="libzstd.so.1 does not load here")


def fam(name):
    return [c for c in CASES if c.family == name]


def matches(cases):
    return [m for c in cases for m in c.census["matches"]]


def test_every_frame_has_its_twin_without_a_declared_size():
    by = {c.name: c for c in CASES}
    sized = [c for c in CASES if c.declared]
    assert len(sized) * 2 == len(CASES) == len(by)
    for c in sized:
        twin = by[c.name + "_nosize"]
        assert twin.data == c.data and not twin.declared and twin.frame != c.frame, c.name
        assert g.walk(c.frame)["content"] == len(c.data) and g.walk(twin.frame)["content"] is None, c.name
        assert g.walk(twin.frame)["window"] >= len(c.data), c.name
    assert collections.Counter(c.family for c in CASES) == {
        "match_small": 764, "match_big": 14, "wrap": 18, "codes": 54, "repeat": 6, "tables": 52, "huffman": 70,
        "bits": 276, "xxh64": 38}
    assert max(len(c.data) for c in CASES) <= 205000  # "no frame decodes to more than about 200 KB"


def test_census_match_forms():
    wanted = {(o, ln) for o in range(1, 64) for ln in zw.MATCH_LENGTHS} | set(zw.MATCH_WIDE)
    assert len(wanted) == 63 * 6 + 21
    assert {(o, ln) for o in (64, 65, 127, 128, 255, 256, 257) for ln in (o - 1, o, o + 1)} <= wanted
    small = fam("match_small")
    # the ring of 256: every pair whose frame fits a capacity of 256, one match a frame
    assert all(len(c.data) <= 256 and len(c.census["matches"]) == 1 for c in small)
    assert {(o, ln) for _f, o, ln, _p in matches(small)} == {(o, ln) for o, ln in wanted if o + ln <= 256}
    assert {f for f, *_ in matches(small)} == {"rep", "step"}
    big = fam("match_big")
    assert wanted <= {(o, ln) for _f, o, ln, _p in matches(big)}
    assert all(256 < len(c.data) < 65536 for c in big)
    for o, ln in wanted:  # which form takes it
        forms = {f for f, oo, ll, _p in matches(big) if (oo, ll) == (o, ln)}
        assert forms == {"rep" if o < 64 else "step"}, (o, ln)


def test_census_ring_wrap():
    wrap = {c.name: c for c in fam("wrap")}
    for c in wrap.values():
        assert 66000 <= len(c.data) <= 205000 and c.census["blocks"][0] == "raw", c.name
    s = {n: wrap[n].census["straddle"] for n in wrap}
    assert "lit" in s["wrap_literal_run"]
    assert "match_rep" in s["wrap_match_rep"] and "match_step" in s["wrap_match_step"]
    assert "match_global" in s["wrap_global_across_131072"]
    assert "src_step" in s["wrap_source"] and "match_step" not in s["wrap_source"]
    assert "pattern" in s["wrap_pattern"] and wrap["wrap_pattern"].census["matches"] == [("rep", 30, 150, 65546)]
    offs = collections.Counter((f, o) for f, o, _l, _p in wrap["wrap_offsets"].census["matches"])
    assert offs == {("step", 65535): 2, ("step", 65536): 2, ("global", 65537): 2}
    # the global form copying its own bytes: an offset above the ring with a length above the offset
    for name in ("wrap_global_overlap", "wrap_global_overlap_far"):
        form, offset, length, _pos = wrap[name].census["matches"][0]
        assert form == "global" and offset >= 65537 and length > offset, name
        assert 131000 <= len(wrap[name].data) <= 205000, name  # "about 132 to 200 KB"
    assert wrap["wrap_global_overlap"].census["checksum"] and wrap["wrap_offsets"].census["checksum"]


def test_census_codes():
    cs = fam("codes")
    ll = set().union(*(c.census["ll_codes"] for c in cs))
    ml = set().union(*(c.census["ml_codes"] for c in cs))
    for c in range(36):
        want = {"none"} if zw.LL_BITS[c] == 0 else {"zeros", "ones"} if c < 35 else {"zeros", "mixed"}
        assert want <= {k for cc, k in ll if cc == c}, c
    for c in range(53):
        want = {"none"} if zw.ML_BITS[c] == 0 else {"zeros", "ones"} if c < 52 else {"zeros", "mixed"}
        assert want <= {k for cc, k in ml if cc == c}, c
    # code 35 / 52 with all ones would pass Block_Maximum_Size: the largest that fits
    by = {c.name: c for c in cs}
    assert len(by["codes_ll_35_ones"].data) == zw.BLOCK_MAX == len(by["codes_ml_52_ones"].data)
    assert by["codes_ml_52_ones"].census["matches"][0][2] == zw.BLOCK_MAX - 40
    assert set().union(*(c.census["of_codes"] for c in cs)) >= set(range(18))
    assert max(set().union(*(c.census["of_codes"] for c in CASES))) == zw.OF_CODE_LIMIT == 17  # 18 and more stay out
    offsets = {o for _f, o, _l, _p in by["codes_of_0_17"].census["matches"]}
    assert {(1 << c) - 3 for c in range(2, 18)} <= offsets and {(2 << c) - 4 for c in range(2, 17)} <= offsets


def test_census_repeat_offsets():
    by = {c.name: c for c in fam("repeat")}
    # the initial 1, 4, 8 straight from a frame's start
    assert [o for _f, o, _l, _p in by["repeat_initial"].census["matches"]] == [4, 8, 1, 1]
    assert by["repeat_all_forms"].census["rep"] == {(0, False), (1, False), (2, False), (1, True), (2, True), (3, True)}
    firsts = by["repeat_all_forms"].census["rep_first_in_block"] + by["repeat_after_blocks"].census["rep_first_in_block"]
    assert {prev for _b, prev in firsts} >= {"compressed", "raw", "rle"}
    assert all(b >= 1 for b, _prev in firsts)
    assert by["repeat_after_blocks"].census["blocks"] == ["compressed", "raw", "compressed", "rle", "compressed",
                                                          "compressed", "compressed"]


def test_census_tables():
    by = {c.name: c for c in fam("tables")}
    seen, forms = set(), collections.defaultdict(set)
    for k in range(5):
        for shape in zw.SHAPES:
            c = by["tables_log%d_%s" % (5 + k, shape)]
            tables = c.census["tables"]
            assert [t.which for t in tables] == [zw.LL, zw.OF, zw.ML], c.name
            if shape == "last_max":  # a code 35 and a code 52 cannot share a block: the later blocks use Repeat_Mode
                assert c.census["blocks"].count("compressed") >= 3 and len(c.census["repeat_after"]) >= 6
            for t in tables:
                size = 1 << t.log
                assert t.log == (min(5 + k, 8) if t.which == zw.OF else 5 + k), c.name
                seen.add((t.which, t.log, shape))
                forms[t.which, t.log] |= t.forms
                enterable = {u for u, (s, _nb, _b) in enumerate(t.cells) if t.which != zw.OF or s <= 17}
                # every cell is entered; an offset table's cells of codes above 17 cannot be (none but in last_max
                # and zero_runs, whose symbols 21, 29 and 31 are "less than 1": one cell each)
                assert enterable <= t.entered, (c.name, t.which, sorted(enterable - t.entered))
                assert len(enterable) >= size - (0 if t.which != zw.OF else {"last_max": 1, "zero_runs": 2}.get(shape, 0))
                norm = t.norm
                if shape == "one_big":
                    assert max(norm) == size - 4
                elif shape == "uniform":
                    assert max(norm) - min(norm) <= 1 and len(norm) >= 11
                elif shape == "neg15":
                    assert sum(x == -1 for x in norm) >= 15
                elif shape == "zero_runs":
                    assert sorted(t.zero_runs) == [1, 2, 3, 4, 6, 7]
                else:
                    assert len(norm) - 1 == zw.MAX_SYM[t.which] == (35, 31, 52)[t.which] and norm[-1] == -1
    assert seen == {(w, log, s) for w in range(3) for log in range(5, zw.MAX_LOG[w] + 1) for s in zw.SHAPES}
    assert len(seen) == 14 * 5
    for key, f in forms.items():  # a value on each side of the low/high encoding threshold
        assert f == {"low", "high"}, key
    rm = by["tables_repeat_modes"].census
    after = {(mode, zero) for _w, mode, _prev, zero in rm["repeat_after"]}
    assert after >= {("pre", False), ("rle", False), ("fse", False), ("fse", True)}
    assert rm["zero_seq_blocks"]


def test_census_huffman():
    cs = fam("huffman")
    hs = [h for c in cs for h in c.census["huf"]]
    trees = [h for h in hs if not h["treeless"]]
    assert {h["nweights"] for h in trees if h["coded"] == "direct"} >= {1, 2, 64, 65, 127, 128}
    assert {(h["nweights"], h["wlog"]) for h in trees if h["coded"] == "fse"} >= {
        (n, wl) for n in (129, 200, 255) for wl in (5, 6)}
    ends = {h["nweights"]: h["end_state"] for h in trees if h["coded"] == "fse"}
    assert ends[129] == 0 and ends[200] == 1  # the weights' chain ends on either state
    assert {h["log"] for h in trees} >= {1, 2, 11}
    # more than 64 symbols in an FSE table: only a weights' description can carry that
    assert max(h["wtable_symbols"] for h in trees if h["coded"] == "fse") == 72
    # equal weights on both sides of every 64-symbol boundary
    assert max(h["groups"] for h in trees) == 4
    assert any(h["groups"] == 4 and h["nweights"] == 255 for h in trees)
    one = {h["regen"] for h in hs if h["nstreams"] == 1}
    assert one >= set(range(1, 41)) | {1022, 1023}
    four = {h["regen"] for h in hs if h["nstreams"] == 4}
    # every valid size from 4 to 48: all but 5, whose three shares of 2 pass it; at 6 and 9 the fourth is empty
    assert four >= (set(range(4, 49)) - {5}) | {1023, 1024, 1025, 1026, 16383, 16384, 16385, 16386}
    assert any(h["lens"] == [2, 2, 2, 0] for h in hs) and any(h["lens"] == [3, 3, 3, 0] for h in hs)
    assert {(lane, n % 4) for h in hs if h["nstreams"] == 4 for lane, n in enumerate(h["lens"])} == {
        (lane, r) for lane in range(4) for r in range(4)}
    assert {h["nstreams"] for h in hs if h["regen"] >= 16384} == {4}  # the 5-byte literals header
    marks = [h for c in cs if c.name.startswith("huf_markers") for h in c.census["huf"]]
    assert any(7 in h["markers"] for h in marks) and any(1 in h["last_bytes"] for h in marks)
    assert any(h["nstreams"] == 4 and 7 in h["markers"] for h in marks)
    assert any(h["nstreams"] == 4 and 1 in h["last_bytes"] for h in marks)
    t = [c for c in cs if c.name == "huf_treeless"][0].census
    assert t["lit_kinds"] == ["huf", "raw", "rle", "treeless", "treeless"]
    assert t["blocks"] == ["compressed"] * 3 + ["raw", "rle"] + ["compressed"] * 2
    assert [h["nstreams"] for h in t["huf"] if h["treeless"]] == [1, 4]


def test_census_bit_window():
    cs = fam("bits")
    streams = [(b["bytes"], b["start"] % 4) for c in cs for b in c.census["bitstreams"]]
    assert set(streams) >= {(n, a) for n in list(range(240, 253)) + list(range(484, 497)) for a in range(4)}
    assert max(n for n, _a in streams) > 1500
    assert {b["marker"] for c in cs for b in c.census["bitstreams"]} == set(range(8))
    ends = collections.defaultdict(set)
    for c in cs:
        if c.census["ends_on_bitstream"] is not None:
            assert len(c.frame) % 4 == c.census["ends_on_bitstream"]
            ends[c.declared].add(len(c.frame) % 4)
    assert ends[True] == ends[False] == {0, 1, 2, 3}
    assert set().union(*(c.census["nseq_bytes"] for c in cs)) == {1, 2, 3}
    assert {m for c in cs for m in c.census["modes"]} >= {(w, m) for w in range(3) for m in ("pre", "rle")}


def test_census_literals_blocks_and_counts():
    raw_sf, kinds, blocks, counts = set(), set(), set(), set()
    for c in CASES:
        raw_sf |= set(c.census.get("raw_sf", ()))
        kinds |= set(c.census.get("lit_kinds", ()))
        blocks |= set(c.census["blocks"])
        counts |= c.census["nseq_bytes"]
    assert raw_sf == {0, 1, 2, 3} and kinds == {"raw", "rle", "huf", "treeless"}
    assert blocks == {"raw", "rle", "compressed"} and counts == {1, 2, 3}
    assert max(len(c.census["blocks"]) for c in CASES) >= 9  # several blocks to a frame
    assert {(c.declared, c.census["checksum"]) for c in CASES} == {(d, k) for d in (True, False) for k in (True, False)}


def test_census_xxh64():
    cs = [c for c in fam("xxh64") if c.declared]
    assert tuple(len(c.data) for c in cs) == zw.XXH_LENGTHS == (
        1, 3, 4, 7, 8, 31, 32, 33, 63, 64, 511, 512, 513, 543, 544, 545, 1023, 1024, 1055)
    for c in fam("xxh64"):
        assert c.census["checksum"] and c.census["blocks"] == ["raw"] and g.walk(c.frame)["checksum"] == 1
        assert int.from_bytes(c.frame[-4:], "little") == g.xxh64(c.data) & 0xFFFFFFFF


def test_model_decodes_every_frame_to_the_writers_bytes():
    for c in CASES:
        assert g.host_count(c.frame) == (0, len(c.data)), c.name  # the count-only mode agrees
        rc, out, word = g.host_decode(c.frame, len(c.data))
        assert rc == 0 and out == c.data and word == len(c.data), c.name
    zw.invalid_cases()
    for name, frame, data in zw.VALID_TWINS:  # an invalid case without its fault decodes
        assert g.host_decode(frame, 64)[:2] == (0, data), name


@needs_lib
def test_live_libzstd_decodes_every_frame_to_the_writers_bytes():
    for c in CASES:
        got, err = LIB.decompress(c.frame, len(c.data))
        assert err is None and got == c.data, (c.name, err)


def _record():
    with open(os.path.join(g.GOLDEN, "zstd_paths.json")) as fh:
        return json.load(fh)


def test_regenerated_frames_are_the_ones_libzstd_judged():
    """The frames are not stored: they are written again here, and must be the
    very bytes libzstd 1.4.8 accepted (or judged) when the record was made."""
    rec = _record()
    assert rec["libzstd"] == "1.4.8"
    assert [v["name"] for v in rec["valid"]] == [c.name for c in CASES]
    for v, c in zip(rec["valid"], CASES):
        assert (v["frame"], v["data"], v["verdict"]) == (g.sha(c.frame), g.sha(c.data), "ok"), c.name
    assert [v["name"] for v in rec["invalid"]] == [n for n, *_ in INVALID]
    for v, (name, frame, _cap, _note) in zip(rec["invalid"], INVALID):
        assert v["frame"] == g.sha(frame), name


def test_invalid_frames_one_fault_each():
    rec = {v["name"]: v for v in _record()["invalid"]}
    assert [n for n, *_ in INVALID] == [
        "rep1_minus_1_is_0", "literal_length_beyond", "weights_past_depth_11", "odd_weight_1_count",
        "four_streams_one_empty", "accuracy_log_10", "weights_fse_71_symbols", "bitstream_byte_left_over"]
    for name, frame, cap, note in INVALID:
        assert g.host_count(frame)[0] == g.E_CORRUPT, name
        rc, _out, _word = g.host_decode(frame, cap)
        assert rc == g.E_CORRUPT, name
        # libzstd refuses them too, but for the code of 12 bits (the header of csrc/mc_zstd.h says so)
        laxer = rec[name]["verdict"] in ("ok", "count")
        assert laxer == (name == "weights_past_depth_11") and laxer == note.startswith("libzstd accepts"), name
        if LIB is not None:
            assert LIB.verdict(frame, cap=cap)["stage"] == rec[name]["verdict"], name


def test_sanitized_run_over_the_new_frames(tmp_path):
    """The ASan + UBSan build of the scalar model, as a process of its own (no
    LD_PRELOAD), as tests/test_zstd_host.py runs it: every new frame from an
    exactly sized heap copy into an exactly sized destination, then truncations
    and byte changes of it."""
    exe = os.path.join(g.HOST_DIR, "zstd_hostcheck_main")
    assert os.path.exists(exe), "build with __graft_entry__.build() (make -C tests/native_zstd)"
    for k, c in enumerate(CASES):
        (tmp_path / f"v{k:04d}-{c.name}.zst").write_bytes(c.frame)
        (tmp_path / f"v{k:04d}-{c.name}.zst.out").write_bytes(c.data)
    for k, (name, frame, _cap, _note) in enumerate(INVALID):
        (tmp_path / f"x{k:04d}-{name}.zst").write_bytes(frame)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    run = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=900, env=env)
    assert run.returncode == 0, run.stdout + run.stderr
    n, refused = len(CASES) + len(INVALID), len(INVALID)
    assert f"frames {n} accepted {n - refused} refused {refused} " in run.stdout, run.stdout
    assert "failures 0" in run.stdout, run.stdout
