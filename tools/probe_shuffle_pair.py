"""Shuffle of one large chunk: access policy per side and tile order, timed as
the producer -> consumer pair and as cold kernels.

Through tools/lab's mc_lab_shuffle_variant (explicit variant word), on the
stream of _ops.stream, with 4 rotating buffer sets ins / encs / decs laid out
as bench.py::run_step_timing lays them out.  For one chunk of 64, 128, 256 and
512 MiB, es = 4 and es = 8, every candidate is first compared with the default
variant on the whole buffer, then timed with one HIP event pair around CALLS
back-to-back calls, the candidates alternating inside this process for ROUNDS
interleaved rounds (the parent's variant is in every round; its max - min over
the rounds is the noise S):
  (a) pair      encode set i, then decode set i, i rotating (us per pair)
  (b) enc_cold  encode alone on the rotating sets (us per call)
  (c) dec_cold  decode alone on the rotating sets (us per call)
Candidates:
  policy  encode loads / stores and decode loads each nontemporal or
          default-policy (| 2048 loads, | 1024 stores; both = | 8), decode
          stores nontemporal: 8 pairs, 4 encode and 2 decode kernels;
  order   2^k virtual rows (bits 12-14 of the variant word), k = 3..8, on every
          policy for (b) and (c), and on the parent's policy for (a);
  planes  BitRound(10) + Shuffle(4) (mc_lab_bitround_shuffle_variant), (b) only.
Then the odd-size diagnosis: the default kernels on single chunks of 256 MiB
+- 3, 5, 7 encode tiles (128 KiB) against 256 MiB, in ps per byte.

No profiler is involved.  One JSON file (default
profiles/r07/probe_shuffle_pair.json)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from lab.lablib import lab as _lab  # noqa: E402
from numcodecs_amd import _ops  # noqa: E402

V_NO_NT, V_ST_PLAIN, V_LD_PLAIN, V_VROWS_SHIFT = 8, 1024, 2048, 12
# the library's defaults for one chunk >= 64 MiB whose count is a multiple of the tile
BASE = {(4, 1): 1 | 512, (4, 0): 5 | 16, (8, 1): 5, (8, 0): 5 | 16, ("br4", 1): 1 | 128}
SETS = 4


def policy_bits(ld_plain, st_plain):
    if ld_plain and st_plain:
        return V_NO_NT
    return (V_LD_PLAIN if ld_plain else 0) | (V_ST_PLAIN if st_plain else 0)


def pname(ld_plain, st_plain):
    return f"ld_{'plain' if ld_plain else 'nt'}+st_{'plain' if st_plain else 'nt'}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07", "probe_shuffle_pair.json"))
    ap.add_argument("--sizes", default="64,128,256,512", help="chunk MiB")
    ap.add_argument("--es", default="4,8")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=40)
    args = ap.parse_args()
    assert args.rounds >= 7 and args.calls >= 40
    lab = _lab()
    dev = torch.device("cuda:0")
    result = {"rounds": args.rounds, "calls": args.calls, "device": torch.cuda.get_device_name(0), "sizes": {}}

    def shuffle(src, dst, n, es, enc, v, st):
        rc = lab.mc_lab_shuffle_variant(src.data_ptr(), dst.data_ptr(), n, es, enc, v, 0, st)
        assert rc == 0, (es, enc, v, rc)

    def bitround(src, dst, n, v, st):
        rc = lab.mc_lab_bitround_shuffle_variant(src.data_ptr(), dst.data_ptr(), n // 4, 4, 10, v, 0, st)
        assert rc == 0, (v, rc)

    def timed(call, ncalls):
        for i in range(SETS):
            call(i)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(ncalls):
            call(i % SETS)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / ncalls * 1e3  # us per call

    def summarise(times, parent):
        """per candidate: the rounds, median, min; S = parent's max - min; gain = parent median - median"""
        s = max(times[parent]) - min(times[parent])
        pm = statistics.median(times[parent])
        out = {"S_us": round(s, 3), "parent": parent, "candidates": {}}
        for k, v in times.items():
            med = statistics.median(v)
            out["candidates"][k] = {"median_us": round(med, 3), "min_us": round(min(v), 3),
                                    "gain_us": round(pm - med, 3), "rounds_us": [round(x, 3) for x in v]}
        return out

    orders = list(range(0, 7))  # 0 = address order, k: 2^(k+2) virtual rows

    def oname(k):
        return "R1" if k == 0 else f"R{1 << (k + 2)}"

    for es in [int(x) for x in args.es.split(",")]:
        for mib in [int(x) for x in args.sizes.split(",")]:
            n = mib << 20
            g = torch.Generator(device=dev).manual_seed(1234)
            ins = [torch.randn(n // 4, generator=g, device=dev, dtype=torch.float32).view(torch.uint8)
                   for _ in range(SETS)]
            encs = [torch.empty(n, dtype=torch.uint8, device=dev) for _ in range(SETS)]
            decs = [torch.empty(n, dtype=torch.uint8, device=dev) for _ in range(SETS)]
            st = _ops.stream(ins[0])
            benc, bdec = BASE[(es, 1)], BASE[(es, 0)]
            enc_c = {f"{pname(ld, s)}|{oname(k)}": benc | policy_bits(ld, s) | (k << V_VROWS_SHIFT)
                     for ld in (0, 1) for s in (0, 1) for k in orders}
            dec_c = {f"{pname(ld, 0)}|{oname(k)}": bdec | policy_bits(ld, 0) | (k << V_VROWS_SHIFT)
                     for ld in (0, 1) for k in orders}
            parent = f"{pname(0, 0)}|R1"
            pair_c = {}
            for eld in (0, 1):
                for est in (0, 1):
                    for dld in (0, 1):
                        pair_c[f"enc:{pname(eld, est)} dec:{pname(dld, 0)}"] = (
                            enc_c[f"{pname(eld, est)}|R1"], dec_c[f"{pname(dld, 0)}|R1"])
            pair_parent = f"enc:{pname(0, 0)} dec:{pname(0, 0)}"
            for k in orders[1:]:
                e, d = enc_c[f"{pname(0, 0)}|{oname(k)}"], dec_c[f"{pname(0, 0)}|{oname(k)}"]
                pair_c[f"order enc:{oname(k)} dec:R1"] = (e, dec_c[parent])
                pair_c[f"order enc:R1 dec:{oname(k)}"] = (enc_c[parent], d)
                pair_c[f"order enc:{oname(k)} dec:{oname(k)}"] = (e, d)
            br_c = {}
            if es == 4:
                br_c = {f"{pname(ld, s)}|{oname(k)}": BASE[("br4", 1)] | policy_bits(ld, s) | (k << V_VROWS_SHIFT)
                        for ld in (0, 1) for s in (0, 1) for k in orders}

            # every candidate against the default variant (word 0), whole buffer
            ref_enc, tmp = torch.empty_like(encs[0]), torch.empty_like(encs[0])
            shuffle(ins[0], ref_enc, n, es, 1, 0, st)
            identical = True
            for name, v in enc_c.items():
                tmp.fill_(0x5A)
                shuffle(ins[0], tmp, n, es, 1, v, st)
                identical &= bool(torch.equal(tmp, ref_enc))
            for name, v in dec_c.items():
                tmp.fill_(0x5A)
                shuffle(ref_enc, tmp, n, es, 0, v, st)
                identical &= bool(torch.equal(tmp, ins[0]))
            if br_c:
                ref_br = torch.empty_like(encs[0])
                rc = lab.mc_lab_bitround_shuffle_variant(ins[0].data_ptr(), ref_br.data_ptr(), n // 4, 4, 10, 0, 0, st)
                assert rc == 0
                for name, v in br_c.items():
                    tmp.fill_(0x5A)
                    bitround(ins[0], tmp, n, v, st)
                    identical &= bool(torch.equal(tmp, ref_br))
                del ref_br
            del ref_enc, tmp
            assert identical, (es, mib, "a candidate differs from the default variant")

            t_pair = {k: [] for k in pair_c}
            t_enc = {k: [] for k in enc_c}
            t_dec = {k: [] for k in dec_c}
            t_br = {k: [] for k in br_c}
            for i in range(SETS):  # decode inputs for (c)
                shuffle(ins[i], encs[i], n, es, 1, 0, st)
            for rnd in range(args.rounds):
                for name, (ve, vd) in pair_c.items():
                    def step(i, ve=ve, vd=vd):
                        shuffle(ins[i], encs[i], n, es, 1, ve, st)
                        shuffle(encs[i], decs[i], n, es, 0, vd, st)
                    t_pair[name].append(timed(step, args.calls))
                for name, v in enc_c.items():
                    t_enc[name].append(timed(lambda i, v=v: shuffle(ins[i], encs[i], n, es, 1, v, st), args.calls))
                for name, v in dec_c.items():
                    t_dec[name].append(timed(lambda i, v=v: shuffle(encs[i], decs[i], n, es, 0, v, st), args.calls))
            for i in range(SETS):  # the pairs and (c) must have left the inputs in decs
                assert torch.equal(decs[i], ins[i]), (es, mib, i)
            for rnd in range(args.rounds):
                for name, v in br_c.items():
                    t_br[name].append(timed(lambda i, v=v: bitround(ins[i], decs[i], n, v, st), args.calls))
            entry = {"identical": identical, "pair": summarise(t_pair, pair_parent),
                     "enc_cold": summarise(t_enc, parent), "dec_cold": summarise(t_dec, parent)}
            if br_c:
                entry["bitround10_enc_cold"] = summarise(t_br, parent)
            result["sizes"][f"es{es}_{mib}MiB"] = entry
            print(f"es{es} {mib} MiB: pair S {entry['pair']['S_us']} us, parent "
                  f"{entry['pair']['candidates'][pair_parent]['median_us']} us", flush=True)
            del ins, encs, decs
            torch.cuda.empty_cache()

    # odd-size diagnosis: the default kernels, one chunk, count not a power of two
    tile = 128 << 10
    odd = {}
    sizes = [(256 << 20) + k * tile for k in (0, -7, -5, -3, 3, 5, 7)]
    nmax = max(sizes)
    ins = [torch.randint(0, 256, (nmax,), dtype=torch.uint8, device=dev) for _ in range(SETS)]
    outs = [torch.empty(nmax, dtype=torch.uint8, device=dev) for _ in range(SETS)]
    st = _ops.stream(ins[0])
    for es in (4, 8):
        for enc in (1, 0):
            times = {n: [] for n in sizes}
            for rnd in range(args.rounds):
                for n in sizes:
                    times[n].append(timed(lambda i, n=n: shuffle(ins[i], outs[i], n, es, enc, 0, st), args.calls))
            odd[f"es{es}_{'enc' if enc else 'dec'}"] = {
                f"256MiB{(n - (256 << 20)) // tile:+d}tiles": {
                    "median_us": round(statistics.median(t), 3),
                    "ps_per_byte": round(statistics.median(t) * 1e6 / (2 * n), 4),
                    "spread_us": round(max(t) - min(t), 3)} for n, t in times.items()}
    result["odd_size_diagnosis"] = odd
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out, flush=True)


if __name__ == "__main__":
    main()
