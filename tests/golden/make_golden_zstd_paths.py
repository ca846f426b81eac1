"""Generate tests/golden/zstd_paths.json: for every frame tests/zstd_write.py
writes, its name, the SHA-256 of the frame, the SHA-256 of the bytes the writer
expects, and what libzstd (through ``ctypes``, tests/zstd_gen.py's ``Lib``)
made of it: "ok" for a valid frame, checked to decode to the writer's bytes;
``Lib.verdict``'s stage for an invalid one.  The frames themselves are not
stored: the tests write them again and compare the hashes, so a machine
without libzstd still decodes exactly what libzstd judged.

Run where libzstd.so.1 loads:

    python tests/golden/make_golden_zstd_paths.py

Names, hashes and verdicts only."""

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import zstd_gen as g  # noqa: E402
import zstd_write as zw  # noqa: E402

lib = g.Lib()
valid, invalid = [], []
for c in zw.cases():
    got, err = lib.decompress(c.frame, len(c.data))
    assert err is None and got == c.data, (c.name, err)
    valid.append({"name": c.name, "frame": g.sha(c.frame), "data": g.sha(c.data), "verdict": "ok"})
for name, frame, cap, _note in zw.invalid_cases():
    v = lib.verdict(frame, cap=cap)
    invalid.append({"name": name, "frame": g.sha(frame), "verdict": v["stage"], "error": v["error"]})
with open(os.path.join(HERE, "zstd_paths.json"), "w") as fh:
    fh.write('{"libzstd": %s,\n' % json.dumps(lib.version))
    for key, rows in (("invalid", invalid), ("valid", valid)):  # one line per frame
        fh.write(' "%s": [\n  %s\n ]%s\n' % (key, ",\n  ".join(json.dumps(r, sort_keys=True) for r in rows),
                                              "," if key == "invalid" else ""))
    fh.write("}\n")
print("libzstd", lib.version, "valid", len(valid), "invalid", len(invalid))
