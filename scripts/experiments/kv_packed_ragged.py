#!/usr/bin/env python3
"""Decode attention of ONE layer over a batch of 8 sequences (8 kv heads, 32 query heads, head_dim 128, fp16; fp8_e4m3 and fp4_e2m1 codes) with
a state row per sequence -> profiles/kv_packed_ragged.txt.  Two readings:

  (a) the price of the per-slot read: every slot at the SAME length (512, 4096, 16384), SlotPackedKV.attend_dev (msq_kv_mx_attn_decode_seq)
      against StaticPackedKV.attend_dev (msq_kv_mx_attn_decode_dev) at B = 8; the capacity is the length + 96 tokens for both;
  (b) what raggedness buys: slots at 512 .. 16384 tokens, mixed, through SlotPackedKV.attend_dev, against what the shared-length cache
      forces for the same batch: a StaticPackedKV with every sequence left-padded to 16384 tokens and a -inf bias over the padding.

Method of kv_packed_decode.py: every variant walks `copies` separate caches in turn (> 1 GB of planes in all) so that no call finds its bytes
in a cache; device events around whole rounds, one warm-up round; the variants alternated inside each repeat; median and range of
`--repeats` repeats.  Needs a GPU (no fallback).

    python scripts/experiments/kv_packed_ragged.py [--out profiles/kv_packed_ragged.txt] [--sizes 512,4096,16384] [--rounds 10] [--repeats 5]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import msq  # noqa: E402,F401
from msq import kvpacked  # noqa: E402

B, HKV, HQ, D = 8, 8, 32, 128
RAGGED = (2048, 16384, 512, 8192, 1024, 4096, 16384, 512)        # 512 .. 16384, mixed: 49152 live tokens against 8 x 16384 padded


def timed(fns, rounds):
    """ms per call: `rounds` rounds over all of `fns`, device events around the lot, one warm-up round"""
    for f in fns:
        f()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(rounds):
        for f in fns:
            f()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / (rounds * len(fns))


def copies_of(cache, n, make):
    """n caches with the bytes and lengths of `cache` (the first is `cache` itself)"""
    out = [cache]
    for _ in range(n - 1):
        c = make()
        for name, t in cache.planes.items():
            c.planes[name].copy_(t)
        c.k_tail.copy_(cache.k_tail); c.v_tail.copy_(cache.v_tail)
        if isinstance(c, kvpacked.SlotPackedKV):
            for b, (p, t) in enumerate(cache.lengths):
                c.set_lengths(b, p, t)
        else:
            c.set_lengths(cache.packed_len, cache.tail_len)
        out.append(c)
    return out


def n_copies(max_len, fmt):
    return max(2, min(16, int(1.05e9 // kvpacked.plane_nbytes(B, HKV, max_len, D, fmt)) + 1))


def alternate(variants, rounds, repeats):
    """{name: [ms, one per repeat]}: inside every repeat each variant is timed once, in turn"""
    res = {n: [] for n, _ in variants}
    for _ in range(repeats):
        for n, fns in variants:
            res[n].append(timed(fns, rounds))
    return res


def fmt_line(tag, v):
    return "  %-58s %10.4f %10.4f .. %-10.4f" % (tag, sorted(v)[len(v) // 2], min(v), max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kv_packed_ragged.txt"))
    ap.add_argument("--sizes", default="512,4096,16384")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kv_packed_ragged.py needs a GPU")
    dev = torch.device("cuda:0")
    S_max = max(RAGGED)
    g = torch.Generator().manual_seed(11)
    K = torch.randn(B, HKV, S_max, D, generator=g).to(torch.float16).to(dev)
    V = torch.randn(B, HKV, S_max, D, generator=g).to(torch.float16).to(dev)
    q = torch.randn(B, HQ, D, generator=g).to(torch.float16).to(dev)
    med = lambda v: sorted(v)[len(v) // 2]
    lines = ["# one layer, B = %d sequences, %d kv heads, %d query heads, head_dim %d, fp16; attend_dev, one query token per sequence; ms per call, cold "
             "(copies walked in turn), median (min .. max) of %d repeats of %d rounds; %s" % (B, HKV, HQ, D, args.repeats, args.rounds, torch.cuda.get_device_name(0)),
             "# (a) every slot at the same length: a state row per sequence (SlotPackedKV) against one shared row (StaticPackedKV)"]
    for S in [int(s) for s in args.sizes.split(",") if s]:
        for fmt in ("fp8_e4m3", "fp4_e2m1"):
            mk_static = lambda: kvpacked.StaticPackedKV(B, HKV, D, torch.float16, fmt, gap=32, max_len=S + 96, device=dev)
            mk_slot = lambda: kvpacked.SlotPackedKV(B, HKV, D, torch.float16, fmt, gap=32, max_len=S + 96, device=dev)
            st, sl = mk_static(), mk_slot()
            st.append(K[:, :, :S], V[:, :, :S])
            for b in range(B):
                sl.prefill(b, K[b:b + 1, :, :S], V[b:b + 1, :, :S])
            assert torch.equal(st.attend_dev(q), sl.attend_dev(q)), "the two caches disagree at equal lengths"
            n = n_copies(S + 96, fmt)
            sts, sls = copies_of(st, n, mk_static), copies_of(sl, n, mk_slot)
            res = alternate((("shared row", [(lambda c=c: c.attend_dev(q)) for c in sts]), ("row per sequence", [(lambda c=c: c.attend_dev(q)) for c in sls])),
                            args.rounds, args.repeats)
            for name, v in res.items():
                lines.append(fmt_line("a  S %-6d %-9s %-18s (%d copies)" % (S, fmt, name, n), v))
            lines.append("  a  S %-6d %-9s row per sequence / shared row = %.3f" % (S, fmt, med(res["row per sequence"]) / med(res["shared row"])))
            del sts, sls, st, sl
            torch.cuda.empty_cache()
    lines.append("# (b) slots at %s tokens (%d live) against every sequence left-padded to %d (%d padded) with a -inf bias; bytes live / padded = %.3f"
                 % (", ".join(str(x) for x in RAGGED), sum(RAGGED), S_max, B * S_max, sum(RAGGED) / (B * S_max)))
    for fmt in ("fp8_e4m3", "fp4_e2m1"):
        mk_static = lambda: kvpacked.StaticPackedKV(B, HKV, D, torch.float16, fmt, gap=32, max_len=S_max + 96, device=dev)
        mk_slot = lambda: kvpacked.SlotPackedKV(B, HKV, D, torch.float16, fmt, gap=32, max_len=S_max + 96, device=dev)
        st, sl = mk_static(), mk_slot()
        Kp, Vp = torch.zeros_like(K), torch.zeros_like(V)
        bias = torch.zeros(B, st.S_cap + st.gap, dtype=torch.float32, device=dev)
        for b, L in enumerate(RAGGED):
            Kp[b, :, S_max - L:], Vp[b, :, S_max - L:] = K[b, :, :L], V[b, :, :L]
            bias[b, :S_max - L] = float("-inf")
            sl.prefill(b, K[b:b + 1, :, :L], V[b:b + 1, :, :L])
        st.append(Kp, Vp)
        del Kp, Vp
        diff = float((st.attend_dev(q, bias, out_dtype=torch.float32) - sl.attend_dev(q, out_dtype=torch.float32)).abs().max())
        n = n_copies(S_max + 96, fmt)
        sts, sls = copies_of(st, n, mk_static), copies_of(sl, n, mk_slot)
        res = alternate((("left-padded + bias", [(lambda c=c: c.attend_dev(q, bias)) for c in sts]), ("ragged", [(lambda c=c: c.attend_dev(q)) for c in sls])),
                        args.rounds, args.repeats)
        for name, v in res.items():
            lines.append(fmt_line("b  %-9s %-18s (%d copies)" % (fmt, name, n), v))
        lines.append("  b  %-9s left-padded / ragged = %.2f (bytes padded / live = %.2f); max |padded - ragged| = %.3e (another split structure: not the same bits)"
                     % (fmt, med(res["left-padded + bias"]) / med(res["ragged"]), B * S_max / sum(RAGGED), diff))
        del sts, sls, st, sl
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
