"""Generate tests/golden/zstd_cases*.npz and zstd_cases.json: the frames of
the zstd case list (tests/zstd_gen.py), made and judged by libzstd through
``ctypes`` (ZSTD_createCCtx, ZSTD_CCtx_setParameter with 100 = level, 201 =
checksum, 200 = contentSizeFlag, 101 = windowLog, ZSTD_compress2,
ZSTD_decompress, ZSTD_getErrorName):

  * valid:     every frame of zstd_gen.lib_specs() and zstd_gen.hand_cases(),
               checked to decode with libzstd to the formula's bytes, with the
               SHA-256 and the size of those bytes (the bytes are not stored);
  * invalid:   zstd_gen.build_invalid() with what the reference's decompress()
               comes to for each (zstd_gen.Lib.verdict: its frame walk, then
               ZSTD_decompress) and libzstd's error name;
  * mutations: for one checksummed and one plain frame of at most 700 bytes
               with Huffman literals and FSE tables, the same verdict on every
               single-byte XOR with 0x01 and 0x80 and on every truncation, as
               arrays in the npz in the order of zstd_gen.mutations().

Run where libzstd.so.1 loads:

    python tests/golden/make_golden_zstd.py

No file is written larger than 1 MiB: the frames are spread over
zstd_cases.npz, zstd_cases_2.npz, ...  Fixtures are data, not program text.
"""

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import zstd_gen as g  # noqa: E402

LIMIT = 1000000  # bytes of frames per npz part

lib = g.Lib()
arrays, meta = {}, {"libzstd": lib.version, "valid": [], "invalid": [], "mutations": {}}
valid = {}

for name, make, params in g.lib_specs():
    data = make()
    frame = lib.compress(data, **params)
    got, err = lib.decompress(frame, len(data))
    assert err is None and got == data, (name, err)
    valid[name] = frame
    meta["valid"].append({"name": name, "sha256": g.sha(data), "size": len(data), "params": params, "made_by": "libzstd"})
for name, frame, data in g.hand_cases():
    got, err = lib.decompress(frame, len(data))
    assert err is None and got == data, (name, err)
    valid[name] = frame
    meta["valid"].append({"name": name, "sha256": g.sha(data), "size": len(data), "params": None, "made_by": "hand"})
for name, frame in valid.items():
    arrays["valid__" + name] = frame

for name, frame, expect, note in g.build_invalid(valid):
    arrays["invalid__" + name] = frame
    meta["invalid"].append({"name": name, "expect": expect, "note": note, "verdict": lib.verdict(frame, cap=1 << 20)})

for kind, name in (("checksummed", "small_checksum"), ("plain", "small_plain")):
    frame = valid[name]
    c = g.walk(frame)
    b = c["blocks"][0]
    assert len(frame) <= 700 and b["type"] == 2 and b["lit_type"] == 2 and 2 in b["modes"], (name, c)
    assert bool(c["checksum"]) == (kind == "checksummed")
    size = [v["size"] for v in meta["valid"] if v["name"] == name][0]
    ok, err, names, shas, lens = [], [], [], [], []
    for what, at, m in g.mutations(frame):  # the record follows their order
        v = lib.verdict(m, cap=4 * size + 1024)
        ok.append(v["stage"] in ("ok", "count"))
        if ok[-1]:
            err.append(0)
            shas.append(bytes.fromhex(g.sha(lib.last)[:16]))
            lens.append(len(lib.last))
        else:
            text = v["error"] or v["stage"]
            if text not in names:
                names.append(text)
            err.append(names.index(text))
    arrays["mut__%s__ok" % kind] = np.array(ok, np.uint8).tobytes()
    arrays["mut__%s__err" % kind] = np.array(err, np.uint8).tobytes()
    arrays["mut__%s__sha" % kind] = b"".join(shas)
    arrays["mut__%s__len" % kind] = np.array(lens, "<u4").tobytes()
    meta["mutations"][kind] = {"frame": name, "capacity": 4 * size + 1024, "errors": names}

# the parts: first fit in order of size
parts = [[] for _ in g.NPZ_PARTS]
for key in sorted(arrays, key=lambda k: -len(arrays[k])):
    for p in parts:
        if sum(len(arrays[k]) for k in p) + len(arrays[key]) <= LIMIT:
            p.append(key)
            break
    else:
        raise SystemExit("%s (%d bytes) fits no part" % (key, len(arrays[key])))
for fn, keys in zip(g.NPZ_PARTS, parts):
    path = os.path.join(HERE, fn)
    if keys:
        np.savez(path, **{k: np.frombuffer(arrays[k], np.uint8) for k in sorted(keys)})
        assert os.path.getsize(path) <= 1 << 20, fn
    elif os.path.exists(path):
        os.remove(path)
with open(os.path.join(HERE, "zstd_cases.json"), "w") as fh:
    # one line per case
    fh.write('{"libzstd": %s,\n "mutations": %s,\n' % (json.dumps(meta["libzstd"]), json.dumps(meta["mutations"], sort_keys=True)))
    for key in ("invalid", "valid"):
        fh.write(' "%s": [\n  %s\n ]%s\n' % (key, ",\n  ".join(json.dumps(c, sort_keys=True) for c in meta[key]),
                                              "," if key == "invalid" else ""))
    fh.write("}\n")
print("libzstd", lib.version, "valid", len(meta["valid"]), "invalid", len(meta["invalid"]),
      "bytes", sum(len(v) for v in arrays.values()))
