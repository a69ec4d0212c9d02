#!/usr/bin/env python3
"""Times the packed mixture-of-experts forward on the Mixtral-8x7B layer shape (H 4096, I 14336, E 8, top-2) against what the project
could do without the grouped kernel and against the dense expert loop:

    (a) moe.QuantExperts.forward                 two launches of k_qgemm_grouped, routing on the device, no host sync
    (b) per-expert loop over qlinear.qlinear     on PackedExperts.expert(e), with the host-side counts it needs (one sync per call)
    (c) the installed MixtralExperts             Python expert loop of transformers on the unpacked bf16 weights

for MSQ-U6 (int2 / fp4, blocks of 16 along out_features) and MSQ-U1 (fp4 / fp8, blocks of 32 along in_features) weights at T = 1, 16, 256,
2048 tokens with a seeded uniform router.  Event timing: `warm` = back-to-back calls after a warm-up of the same shape, `cold` = a 1 GiB
buffer is rewritten in front of every timed call (the packed weights do not come from the Infinity Cache or L2).

    python scripts/experiments/moe_grouped.py               driver: one child process per kind (the weights are built once for its four
                                                            T), each under its own time limit; stops at the first child that fails;
                                                            writes profiles/moe_grouped.txt
    python scripts/experiments/moe_grouped.py --one u6      one kind, one JSON line per T
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

H, I, E, TOPK = 4096, 14336, 8, 2
KINDS = {"u6": ("int2", "fp4", 16, 0, (8,)), "u8": ("fp4_e2m1", "fp8_e4m3", 32, -1, (5,))}
TOKENS = (1, 16, 256, 2048)
HBM_TBS = 8.0


def one(kind, tokens, iters):
    import torch
    import msq
    from msq import moe, qlinear
    from transformers import MixtralConfig
    from transformers.models.mixtral.modeling_mixtral import MixtralExperts

    dev = torch.device("cuda:0")
    fi, fo, bs, axis, kinds = KINDS[kind]
    g = torch.Generator(device=dev).manual_seed(1)

    def values(n, k):
        W = torch.randn(n, k, generator=g, device=dev) * 0.02
        W[torch.rand(n, k, generator=g, device=dev) < 0.01] *= 16
        return msq.quant.outlier_fakequant(W, 8, 8, fi, fo, 2, axis, bs)["out"]

    class Src(torch.nn.Module):
        pass
    src = Src()
    # gate and up halves quantised on their own, as the harness does
    src.gate_up_proj = torch.nn.Parameter(torch.stack([torch.cat([values(I, H), values(I, H)]) for _ in range(E)]), requires_grad=False)
    src.down_proj = torch.nn.Parameter(torch.stack([values(H, I) for _ in range(E)]), requires_grad=False)
    src.act_fn = torch.nn.functional.silu
    q = moe.QuantExperts.from_module(src, kinds=kinds)
    Pg, Pd = q.packed()
    cfg = MixtralConfig(hidden_size=H, intermediate_size=I, num_local_experts=E, num_experts_per_tok=TOPK, num_hidden_layers=1)
    cfg._experts_implementation = "eager"
    with torch.device("meta"):
        dense = MixtralExperts(cfg)
    dense = dense.to_empty(device=dev).to(torch.bfloat16)
    dense.gate_up_proj.data.copy_(src.gate_up_proj.data); dense.down_proj.data.copy_(src.down_proj.data)
    del src
    torch.cuda.empty_cache()

    flush = torch.empty(1 << 30, dtype=torch.uint8, device=dev)
    for T in tokens:
        measure(kind, T, iters, q, Pg, Pd, dense, flush, g)


def measure(kind, T, iters, q, Pg, Pd, dense, flush, g):
    import torch
    from msq import moe, qlinear
    dev = flush.device
    x = torch.randn(T, H, generator=g, device=dev).to(torch.bfloat16)
    idx = torch.stack([torch.randperm(E, generator=g, device=dev)[:TOPK] for _ in range(T)])       # seeded uniform router
    w = torch.rand(T, TOPK, generator=g, device=dev) + 0.1
    w = w / w.sum(-1, keepdim=True)
    hit = sorted(set(idx.reshape(-1).tolist()))
    bytes_step = len(hit) * (Pg.nbytes + Pd.nbytes) // E        # packed bytes a step must read: the experts that have rows, once

    def f_grouped():
        return q(x, idx, w)

    def f_loop():
        # what the parent commit can do: sort on the device, fetch the counts (host sync), one qlinear per expert with rows and projection
        ri, ro, inv = moe.route(idx, E)
        offs = ro.tolist()
        xs = x[ri.long()]
        y = torch.empty(T * TOPK, H, dtype=torch.bfloat16, device=dev)
        for e in range(E):
            lo, hi = offs[e], offs[e + 1]
            if hi > lo:
                gu = qlinear.qlinear(xs[lo:hi], Pg.expert(e), None, torch.bfloat16)
                y[lo:hi] = qlinear.qlinear(torch.nn.functional.silu(gu[:, :I]) * gu[:, I:], Pd.expert(e), None, torch.bfloat16)
        y = y[inv].view(T, TOPK, H)
        return (y[:, 0] * w[:, 0, None] + y[:, 1] * w[:, 1, None]).to(torch.bfloat16)

    def f_dense():
        return dense(x, idx, w)

    def timed(fn, cold):
        ts = []
        for _ in range(iters):
            if cold:
                flush.add_(1)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b) * 1e3)
        ts.sort()
        return ts[len(ts) // 2], ts[0]

    out = dict(kind=kind, T=T, experts_hit=len(hit), packed_bytes_step=bytes_step)
    with torch.no_grad():
        ya, yb = f_grouped(), f_loop()
        out["max_abs_diff_a_vs_b"] = float((ya.float() - yb.float()).abs().max())
        out["max_abs"] = float(yb.float().abs().max())
        for name, fn in (("a_grouped", f_grouped), ("b_loop", f_loop), ("c_dense", f_dense)):
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            out[name + "_warm_us"], out[name + "_warm_min_us"] = timed(fn, False)
            out[name + "_cold_us"], out[name + "_cold_min_us"] = timed(fn, True)
    print(json.dumps(out), flush=True)


def driver(args):
    rows = []
    for kind in args.kinds.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--one", kind, "--iters", str(args.iters)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)
        except subprocess.TimeoutExpired:
            print("step %s ran into its time limit: stopping" % kind, flush=True)
            return write(rows, args, "stopped: %s ran into its time limit" % kind)
        for line in r.stdout.splitlines():
            if line.startswith("{"):
                rows.append(json.loads(line))
                print(line, flush=True)
        if r.returncode != 0:
            print(r.stdout[-2000:], r.stderr[-4000:], flush=True)
            print("step %s failed with status %d: stopping" % (kind, r.returncode), flush=True)
            return write(rows, args, "stopped: %s failed with status %d" % (kind, r.returncode))
    return write(rows, args, None)


def write(rows, args, note):
    L = ["# packed mixture of experts on the Mixtral-8x7B layer shape (H %d, I %d, E %d, top-%d), bf16 activations, one MI355X" % (H, I, E, TOPK),
         "# scripts/experiments/moe_grouped.py: median of %d event-timed calls, microseconds; warm = back to back, cold = 1 GiB rewritten in front of every call" % args.iters,
         "# (a) QuantExperts.forward (k_qgemm_grouped x 2, no host sync)   (b) per-expert loop over qlinear.qlinear with host-side counts   (c) MixtralExperts (bf16, Python loop)",
         "# packed MB = packed bytes of the experts that have rows (what a step must read); %% of 8 TB/s = those bytes / cold time of (a), T <= 16",
         "%-4s %5s %4s %10s | %9s %9s %9s | %9s %9s %9s | %8s | %s" % ("kind", "T", "hit", "packed MB", "a warm", "b warm", "c warm", "a cold", "b cold", "c cold", "% 8 TB/s", "a loses to")]
    for r in rows:
        frac = "%.1f" % (100.0 * r["packed_bytes_step"] / (r["a_grouped_cold_us"] * 1e-6) / (HBM_TBS * 1e12)) if r["T"] <= 16 else "-"
        loses = [n for n, k in (("b", "b_loop"), ("c", "c_dense")) if r[k + "_warm_us"] < r["a_grouped_warm_us"]]
        loses_c = [n for n, k in (("b", "b_loop"), ("c", "c_dense")) if r[k + "_cold_us"] < r["a_grouped_cold_us"]]
        verdict = ("warm: " + ("/".join(loses) or "none")) + ", cold: " + ("/".join(loses_c) or "none")
        L.append("%-4s %5d %4d %10.1f | %9.1f %9.1f %9.1f | %9.1f %9.1f %9.1f | %8s | %s" % (
            r["kind"], r["T"], r["experts_hit"], r["packed_bytes_step"] / 1e6, r["a_grouped_warm_us"], r["b_loop_warm_us"], r["c_dense_warm_us"],
            r["a_grouped_cold_us"], r["b_loop_cold_us"], r["c_dense_cold_us"], frac, verdict))
    if note:
        L.append("# " + note)
    text = "\n".join(L) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)
    return 1 if note else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", metavar="KIND")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--kinds", default="u6,u8")
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "moe_grouped.txt"))
    a = ap.parse_args()
    if a.one:
        one(a.one, TOKENS, a.iters)
    else:
        sys.exit(driver(a))
