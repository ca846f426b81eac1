"""The tile order of one large Shuffle chunk (mc_tile_steps / mc_tile_of_step,
csrc/mc_shuffle.h), compiled for the host with ASan + UBSan by
tests/native_tileorder and run as a process of its own: for every ntiles in
1..2048 and every R the variant word can select (and some it cannot), the
visited steps map one-to-one onto [0, ntiles), and R = 1 is the identity."""

import os
import subprocess

EXE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native_tileorder", "_build", "tileorder_main")
ALLOWED_R = (1, 8, 16, 32, 64, 128, 256)


def _run(*rs):
    assert os.path.exists(EXE), "build with __graft_entry__.build() (make -C tests/native_tileorder)"
    p = subprocess.run([EXE, *map(str, rs)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr
    lines = dict(ln.split(" ", 1) for ln in p.stdout.splitlines())
    return lines


def test_allowed_rows_are_bijections():
    lines = _run(*ALLOWED_R)
    assert set(lines) == {f"R={r}" for r in ALLOWED_R}
    for r in ALLOWED_R:
        want = "bijection=ok identity=" + ("ok" if r == 1 else "-")
        assert lines[f"R={r}"] == want, (r, lines)


def test_any_row_count_is_a_bijection():
    # the map does not depend on R being a power of two, nor on R <= ntiles
    rs = (2, 3, 5, 7, 100, 2047, 2048, 2049, 4096)
    lines = _run(*rs)
    for r in rs:
        assert lines[f"R={r}"] == "bijection=ok identity=-", (r, lines)
