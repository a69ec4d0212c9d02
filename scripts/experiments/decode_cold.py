#!/usr/bin/env python3
"""Decode (M = 1 ... 16) time of the fused Llama-2-7B projections with COLD weights: every graph walks through enough distinct
copies of the packed weight (>= 1 GB) that neither the L2 nor the 256 MB Infinity Cache can hold them -- what a decode step
over 32 layers sees (a graph replaying ONE weight measures the Infinity Cache instead).
Usage: python scripts/experiments/decode_cold.py [fp8|posit|mx8|mx4|c16|u16|c32|u32|v6|v8] [M ...]
c16 / c32: int2 inliers + fp4 outliers at block 16 / 32 in the compact layout (MSQ-C1, 6.0 / 5.5 bits per weight); u16 / u32: the same weight and
formats in the unified layout (8.25 bits).  When both of a pair are asked for, their time ratio is printed per projection and M, and with
PACK=1 the pack kernels' time for W[16384, 4096] in both layouts.
v6 / v8: the harness default -- int2 / fp4 fake-quant VALUES with blocks of 16 along out_features (axis 0) -- packed by pack_values as kind 8
(MSQ-U6, 6.25 bits per weight) and as kind 5 (MSQ-U1, 8.25).  Asked for together, the two are timed ALTERNATELY (ROUNDS rounds of REPS graph
replays each, default 3 x 100; both graphs are built first) and the median, the spread and the time ratio are printed; PACK=1 adds the wall
time of pack_values for [16384, 4096] in both kinds."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch

import msq
from msq import qlinear

dev = torch.device("cuda:0")
torch.manual_seed(0)
LOWBIT = {"c16": ("compact", 16), "u16": ("unified", 16), "c32": ("compact", 32), "u32": ("unified", 32)}      # int2 / fp4: (layout, block)
VALUES = {"v6": qlinear.PLANE_U6, "v8": qlinear.PLANE_U8}      # axis-0 int2 / fp4 values through pack_values: plane kind
fmts = [a for a in sys.argv[1:] if a in ("fp8", "posit", "mx8", "mx4") or a in LOWBIT or a in VALUES] or ["fp8", "posit"]      # mx8 / mx4: the MX matrix path (e4m3 values / plain MX-FP4 operand)
Ms = [int(a) for a in sys.argv[1:] if a.isdigit()] or [1, 16]
FO = {"fp8": "fp8_e4m3", "posit": "posit8_es1"}


def clone(P):
    c = lambda t: None if t is None else t.clone()
    if isinstance(P, qlinear.MXPackedWeight):
        import copy
        Q = copy.copy(P)
        Q.codes, Q.scales = P.codes.clone(), P.scales.clone()
        return Q
    return qlinear.PackedWeight(c(P.inl), c(P.out), c(P.scl), P.N, P.K, P.block, P.in_kind, P.out_kind, P.n, P.k)


def make_graph(fns):
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for f in fns[:2]:
            f()
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            for f in fns:
                f()
    for _ in range(2):
        g.replay()
    torch.cuda.synchronize()
    return g


def time_graph(g, n, reps):
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        g.replay()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps / n * 1e3


def tgraph(fns, reps=5):
    return time_graph(make_graph(fns), len(fns), reps)


def values_axis0(W):
    """the harness default: int2 inliers / fp4 outliers, blocks of 16 along out_features"""
    return msq.quant.outlier_fakequant(W, 8, 8, "int2", "fp4", 2, 0, 16)["out"]


def values_pair(name, N, K, W, tot):
    """v6 beside v8 on the same values: both graphs first, then alternating timed rounds"""
    rounds, reps = int(os.environ.get("ROUNDS", "3")), int(os.environ.get("REPS", "100"))
    V = values_axis0(W)
    sets = {}
    for f in ("v8", "v6"):
        P0 = qlinear.pack_values(V, (VALUES[f],))
        copies = max(4, int(1.2e9 // P0.nbytes) + 1)
        sets[f] = [P0] + [clone(P0) for _ in range(copies - 1)]
    del V
    for M in Ms:
        X = torch.randn(M, K, device=dev).to(torch.bfloat16)
        assert torch.equal(qlinear.qlinear(X, sets["v6"][0]), qlinear.qlinear(X, sets["v8"][0])), "the two kinds must give the same bits"
        gs = {f: make_graph([(lambda P=P: qlinear.qlinear(X, P)) for P in sets[f]]) for f in ("v8", "v6")}
        ts = {"v8": [], "v6": []}
        for _ in range(rounds):
            for f in ("v8", "v6"):
                ts[f].append(time_graph(gs[f], len(sets[f]), reps))
        med = {f: sorted(ts[f])[len(ts[f]) // 2] for f in ts}
        for f in ("v8", "v6"):
            nb = sets[f][0].nbytes
            tot[(f, M)] = tot.get((f, M), 0.0) + med[f]
            print(f"{name:8s} N{N:6d} K{K:6d} {f:5s} M{M:3d}: {med[f]:6.1f} us (median of {rounds} rounds x {reps} replays, min {min(ts[f]):.1f} max {max(ts[f]):.1f})  "
                  f"{nb/med[f]/1e3:5.0f} GB/s of packed weight ({len(sets[f])} copies, {nb/1e6:.0f} MB each)", flush=True)
        print(f"{name:8s} v6 / v8 M{M:3d}: time ratio {med['v6']/med['v8']:5.3f}  (byte ratio {sets['v6'][0].nbytes/sets['v8'][0].nbytes:5.3f})", flush=True)
        del gs


def pack_values_times(reps=5):
    """wall time of pack_values (allocation, launch, status read-back) for [16384, 4096] axis-0 int2 / fp4 values, both kinds, alternating"""
    import time
    W = torch.randn(16384, 4096, device=dev) * 0.02
    W[torch.rand(16384, 4096, device=dev) < 0.005] *= 16
    V = values_axis0(W)
    del W
    ts = {"v8": [], "v6": []}
    for i in range(reps + 1):
        for f in ("v8", "v6"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            P = qlinear.pack_values(V, (VALUES[f],))
            torch.cuda.synchronize()
            if i:
                ts[f].append((time.perf_counter() - t0) * 1e6)
            assert P.out_kind == VALUES[f]
    for f in ("v8", "v6"):
        print(f"pack_values [16384, 4096] int2/fp4 axis 0, kind {VALUES[f]}: median {sorted(ts[f])[len(ts[f]) // 2]:7.1f} us wall (min {min(ts[f]):.1f} max {max(ts[f]):.1f}, {reps} calls after one warm-up, "
              f"float32 copy of the input, buffer allocation and the status read-back included)", flush=True)


def pack_times(reps=5):
    """device time of pack_weight's launches for W[16384, 4096], int2 / fp4, compact beside unified (same weight, same run)"""
    W = torch.randn(16384, 4096, device=dev) * 0.02
    W[torch.rand(16384, 4096, device=dev) < 0.005] *= 16
    for f in [f for f in fmts if f in LOWBIT]:
        lay, bs = LOWBIT[f]
        ts = []
        for _ in range(reps + 1):
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            P = qlinear._pack(W, 8, 8, "int2", "fp4", 2, bs, "nearest", False, 0, lay)
            e1.record(); torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        print(f"pack W[16384, 4096] int2/fp4 block {bs} {lay:8s}: {min(ts[1:]):7.1f} us (best of {reps}; buffer allocation and the status read-back included), {P.nbytes/1e6:.1f} MB", flush=True)


def main():
    tot = {}
    res = {}
    ONLY = [a for a in os.environ.get("ONLY", "").split(",") if a]
    for (name, N, K) in (("qkv", 12288, 4096), ("o", 4096, 4096), ("gate_up", 22016, 4096), ("down", 4096, 11008)):
        if ONLY and name not in ONLY:
            continue
        W = torch.randn(N, K, device=dev) * 0.02
        W[torch.rand(N, K, device=dev) < 0.005] *= 16
        if "v6" in fmts and "v8" in fmts:
            values_pair(name, N, K, W, tot)
        for f in fmts:
            if f in VALUES and "v6" in fmts and "v8" in fmts:
                continue
            if f in VALUES:
                P0 = qlinear.pack_values(values_axis0(W), (VALUES[f],))
            elif f == "mx8":
                P0 = qlinear.mx_pack_values(msq.quant.outlier_fakequant(W[:, :K // 128 * 128].contiguous(), 8, 8, "fp4_e2m1", "fp8_e4m3", 2, -1, 32)["out"])
            elif f == "mx4":
                P0 = qlinear.mx_pack_weight(W[:, :K // 128 * 128].contiguous())
            elif f in LOWBIT:
                P0 = qlinear.pack_weight(W, 8, 8, "int2", "fp4", 2, LOWBIT[f][1], layout=LOWBIT[f][0])
            else:
                P0 = qlinear.pack_weight(W, 8, 8, "fp4_e2m1", FO[f], 2, 32, layout="unified")
            call = qlinear.qlinear_mx_w4a8 if f in ("mx8", "mx4") else qlinear.qlinear
            copies = max(4, int(1.2e9 // P0.nbytes) + 1)
            Ps = [P0] + [clone(P0) for _ in range(copies - 1)]
            for M in Ms:
                X = torch.randn(M, P0.k, device=dev).to(torch.bfloat16)
                us = tgraph([(lambda P=P: call(X, P)) for P in Ps])
                tot[(f, M)] = tot.get((f, M), 0.0) + us
                res[(name, f, M)] = (us, P0.nbytes)
                print(f"{name:8s} N{N:6d} K{K:6d} {f:5s} M{M:3d}: {us:6.1f} us  {P0.nbytes/us/1e3:5.0f} GB/s of packed weight ({copies} copies, {P0.nbytes/1e6:.0f} MB each)", flush=True)
            del Ps
        for c, u in (("c16", "u16"), ("c32", "u32")):
            for M in Ms:
                if (name, c, M) in res and (name, u, M) in res:
                    (tc, bc), (tu, bu) = res[(name, c, M)], res[(name, u, M)]
                    print(f"{name:8s} {c} / {u} M{M:3d}: time ratio {tc/tu:5.3f}  (byte ratio {bc/bu:5.3f})", flush=True)
        if os.environ.get("DENSE", "0") == "1":
            Wb = W.to(torch.bfloat16)
            copies = max(4, int(1.2e9 // (N * K * 2)) + 1)
            Ws = [Wb] + [Wb.clone() for _ in range(copies - 1)]
            for M in Ms:
                X = torch.randn(M, K, device=dev).to(torch.bfloat16)
                us = tgraph([(lambda w=w: X @ w.t()) for w in Ws])
                print(f"{name:8s} N{N:6d} K{K:6d} dense bf16 hipBLASLt M{M:3d}: {us:6.1f} us  {N*K*2/us/1e3:5.0f} GB/s", flush=True)
            del Ws
        del W
    for k, v in sorted(tot.items()):
        print(f"layer total {k[0]} M{k[1]}: {v:6.1f} us")
    if os.environ.get("PACK", "0") == "1":
        pack_times()
        if "v6" in fmts and "v8" in fmts:
            pack_values_times()


if __name__ == "__main__":
    main()
