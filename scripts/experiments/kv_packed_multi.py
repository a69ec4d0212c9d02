#!/usr/bin/env python3
"""Attention of T query tokens over ONE layer's packed cache [1, 8 kv heads, S, 128] (fp16, 32 query heads: 4 per kv head) at S = 1024, 4096,
16384 and T = 1, 4, 16, fp8_e4m3 and fp4_e2m1 -> profiles/kv_packed_multi.txt:

  (m) PackedKV.attend_multi over the codes (csrc/msq_kv_packed_multi.hip: two launches);
  (p) what the parent commit does for T > 1: PackedKV.dequantize() + scaled_dot_product_attention with the causal mask of the last T tokens;
  (a) at T = 1: PackedKV.attend, the single-token kernel (the parent's path for that length).

Cold: (m) and (a) walk `copies` separate caches in turn, `copies` chosen per size and format so that the CODE planes walked are at least
512 MB in all (twice the 256 MB last-level cache), so that no call finds its bytes in a cache; (p) walks a quarter of them, at least 2: it also
writes and re-reads the 16-bit tensors, 3.9 to 7.5 times the bytes of the codes.  The header of the output states the copies of every row.
The variants are alternated within each repeat; device events around whole rounds; median and range over the repeats.  Needs a GPU.

    python scripts/experiments/kv_packed_multi.py [--out profiles/kv_packed_multi.txt] [--sizes 1024,4096,16384] [--tokens 1,4,16]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import msq  # noqa: E402,F401
from msq import kvpacked  # noqa: E402

HKV, HQ, D = 8, 32, 128


def timed(fns, rounds):
    """ms per call: `rounds` rounds over all of `fns`, device events around the lot"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(rounds):
        for f in fns:
            f()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / (rounds * len(fns))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kv_packed_multi.txt"))
    ap.add_argument("--sizes", default="1024,4096,16384")
    ap.add_argument("--tokens", default="1,4,16")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kv_packed_multi.py needs a GPU")
    dev = torch.device("cuda:0")
    sdpa = torch.nn.functional.scaled_dot_product_attention
    lines = ["# one layer [1, %d kv heads, S, %d] fp16, %d query heads, T query tokens (the cache's last T, causal); ms per call, cold (copies walked in"
             % (HKV, D, HQ), "# turn), median (min .. max) of %d repeats of %d rounds, variants alternated; %s" % (args.repeats, args.rounds, torch.cuda.get_device_name(0)),
             "# %-6s %-9s %-3s %-28s %10s %22s %10s %6s" % ("S", "format", "T", "variant", "ms", "range", "MB codes", "copies")]
    for S in [int(s) for s in args.sizes.split(",")]:
        g = torch.Generator().manual_seed(S)
        K = torch.randn(1, HKV, S, D, generator=g).to(torch.float16).to(dev)
        V = torch.randn(1, HKV, S, D, generator=g).to(torch.float16).to(dev)
        for fmt in ("fp8_e4m3", "fp4_e2m1"):
            copies = max(2, int(512e6 // kvpacked.plane_nbytes(1, HKV, S, D, fmt)) + 1)
            pks = []
            for _ in range(copies):
                pk = kvpacked.PackedKV(1, HKV, D, torch.float16, fmt, gap=32, capacity=S, device=dev)
                pk.append(K, V)
                pks.append(pk)
            nbytes = kvpacked.plane_nbytes(1, HKV, S, D, fmt)
            for T in [int(t) for t in args.tokens.split(",")]:
                q = torch.randn(1, HQ, T, D, generator=g).to(torch.float16).to(dev)
                pos = torch.arange(S, device=dev)[None, :]
                mask = pos <= (S - T + torch.arange(T, device=dev))[:, None]                  # [T, S] bool, True = attend

                def parent(pk):
                    k, v = pk.dequantize()
                    return sdpa(q, k, v, attn_mask=mask, enable_gqa=True)

                variants = [("m attend_multi", [(lambda pk=pk: pk.attend_multi(q)) for pk in pks]),
                            ("p dequantize + sdpa (parent)", [(lambda pk=pk: parent(pk)) for pk in pks[:max(2, copies // 4)]])]
                if T == 1:
                    q1 = q[:, :, 0, :].contiguous()
                    variants.append(("a attend (single-token)", [(lambda pk=pk: pk.attend(q1)) for pk in pks]))
                y, yp = pks[0].attend_multi(q, out_dtype=torch.float32), parent(pks[0]).transpose(1, 2).float()
                gap = float((y - yp).abs().max())
                res = {n: [] for n, _ in variants}
                for n, fns in variants:                            # warm-up
                    timed(fns, 1)
                for _ in range(args.repeats):
                    for n, fns in variants:
                        res[n].append(timed(fns, args.rounds if n[0] != "p" else max(2, args.rounds // 4)))
                med = {n: sorted(v)[len(v) // 2] for n, v in res.items()}
                for n, v in res.items():
                    lines.append("  %-6d %-9s %-3d %-28s %10.4f %10.4f .. %-10.4f %10.2f %6d" % (S, fmt[:3], T, n, med[n], min(v), max(v), nbytes / 1e6,
                                                                                              len(dict(variants)[n])))
                extra = "" if T != 1 else "; attend_multi / attend %.2f" % (med["m attend_multi"] / med["a attend (single-token)"])
                lines.append("  %-6d %-9s %-3d parent / attend_multi %.2f%s; max |attend_multi - parent| %.2e" % (
                    S, fmt[:3], T, med["p dequantize + sdpa (parent)"] / med["m attend_multi"], extra, gap))
            del pks
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
