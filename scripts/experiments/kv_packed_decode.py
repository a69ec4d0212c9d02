#!/usr/bin/env python3
"""Decode-step attention of ONE layer [1, 32, S, 128] (fp16) at S = 1024, 4096, 16384 -> profiles/kv_packed_decode.txt:

  (a) PackedKV.attend over the codes, fp8_e4m3 and fp4_e2m1 (csrc/msq_kv_packed.hip: two launches);
  (b) what the parent commit does: the fp16 fake-quantised cache (msq.kvcache method "MX") through scaled_dot_product_attention;
  (c) PackedKV.dequantize() + scaled_dot_product_attention: what PackedMXKVCache.update() + any attention costs;
  and the bytes a step reads, with the time msq_read_stream_probe takes over the same number of bytes of the code planes.

Every variant walks `copies` separate caches in turn (> 1 GB in all) so that no step finds its bytes in a cache; device events around
whole rounds, warm-up first.  Needs a GPU (no fallback).

Then the decode STEP of one layer -- append one token, attend -- at S = 512, 4096, 16384 (--step-sizes), fp8 and fp4, three ways:
  (d) eager with host lengths: PackedKV.append + attend, what the parent commit offers;
  (e) eager with device lengths: StaticPackedKV.append + attend_dev, the same Python without length arithmetic in the launches;
  (f) the step of (e) captured in a HIP graph and replayed;
and the attention launch alone at equal lengths, host-length entry against device-length entry (idle blocks are the latter's only extra
cost).  One cache per variant (warm: the step's fixed costs are the subject, not the bytes), windows of 64 steps from length S (two
flushes at gap 32), the lengths reset between windows, the variants alternated within each of `--step-repeats` repeats; median and range.

    python scripts/experiments/kv_packed_decode.py [--out profiles/kv_packed_decode.txt] [--sizes 1024,4096,16384] [--rounds 20]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import msq  # noqa: E402
from msq import _lib, kvcache, kvpacked  # noqa: E402

H, D = 32, 128


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


def _window(fn, steps):
    """ms per step over one window of `steps` calls: device events around the window (host launch time included: the device waits for it)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def step_three_ways(S, fmt, dev, repeats, steps=64):
    """{variant: [ms per step, one per repeat]} for the decode step and the attention launch alone"""
    g = torch.Generator().manual_seed(S + 1)
    K = torch.randn(1, H, S, D, generator=g).to(torch.float16).to(dev)
    V = torch.randn(1, H, S, D, generator=g).to(torch.float16).to(dev)
    q = torch.randn(1, H, D, generator=g).to(torch.float16).to(dev)
    k1 = torch.randn(1, H, 1, D, generator=g).to(torch.float16).to(dev)
    v1 = torch.randn(1, H, 1, D, generator=g).to(torch.float16).to(dev)
    dyn = kvpacked.PackedKV(1, H, D, torch.float16, fmt, gap=32, capacity=S + steps + 32, device=dev)
    dyn.append(K, V)
    sta = kvpacked.StaticPackedKV(1, H, D, torch.float16, fmt, gap=32, max_len=S + steps + 32, device=dev)
    sta.append(K, V)
    cap = kvpacked.StaticPackedKV(1, H, D, torch.float16, fmt, gap=32, max_len=S + steps + 32, device=dev)
    cap.append(K, V)
    P0, T0 = dyn.packed_len, dyn.tail_len

    def reset():
        dyn.packed_len, dyn.tail_len = P0, T0
        sta.set_lengths(P0, T0)
        cap.set_lengths(P0, T0)

    def step_d():
        dyn.append(k1, v1)
        return dyn.attend(q)

    def step_e():
        sta.append(k1, v1)
        return sta.attend_dev(q)

    cap.append(k1, v1)                                           # one eager step: the workspace
    cap.attend_dev(q)
    cap.set_lengths(P0, T0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap.append(k1, v1)
        y = cap.attend_dev(q)
    reset()
    for f in (step_d, step_e, graph.replay):                     # warm-up of every shape the windows use, and a check that the three agree
        for _ in range(steps):
            out = f()
    torch.cuda.synchronize()
    cap.advance_host(steps)
    assert (dyn.packed_len, dyn.tail_len) == sta.sync() == cap.sync(), "the three caches disagree on the lengths"
    assert torch.equal(dyn.attend(q), sta.attend_dev(q)) and torch.equal(dyn.attend(q), cap.attend_dev(q)), "the three caches disagree"
    res = {n: [] for n in ("d eager host lengths", "e eager device lengths", "f graph replay", "attend host-length", "attend device-length")}
    for _ in range(repeats):
        for name, f in (("d eager host lengths", step_d), ("e eager device lengths", step_e), ("f graph replay", graph.replay)):
            reset()
            torch.cuda.synchronize()
            res[name].append(_window(f, steps))
        reset()
        torch.cuda.synchronize()
        res["attend host-length"].append(_window(lambda: sta.attend(q), steps))
        res["attend device-length"].append(_window(lambda: sta.attend_dev(q), steps))
    # the two attention entries as graph replays too: without the host's launch time the kernels themselves are compared
    for name, f in (("attend host-length, replayed", lambda: sta.attend(q)), ("attend device-length, replayed", lambda: sta.attend_dev(q))):
        f()
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            for _ in range(16):
                f()
        gr.replay()
        torch.cuda.synchronize()
        res[name] = [_window(gr.replay, 8) / 16 for _ in range(repeats)]
    del y, out
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kv_packed_decode.txt"))
    ap.add_argument("--sizes", default="1024,4096,16384")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--step-sizes", default="512,4096,16384")
    ap.add_argument("--step-repeats", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kv_packed_decode.py needs a GPU")
    dev = torch.device("cuda:0")
    sdpa = torch.nn.functional.scaled_dot_product_attention
    sink = torch.zeros(4, dtype=torch.uint8, device=dev)
    lines = ["# one layer [1, %d, S, %d] fp16, one query token; ms per step, cold (copies walked in turn); %s" % (H, D, torch.cuda.get_device_name(0)),
             "# %-6s %-22s %10s %12s %10s %14s %12s" % ("S", "variant", "ms", "MB read", "GB/s", "read probe ms", "share")]
    for S in [int(s) for s in args.sizes.split(",")]:
        g = torch.Generator().manual_seed(S)
        K = torch.randn(1, H, S, D, generator=g).to(torch.float16).to(dev)
        V = torch.randn(1, H, S, D, generator=g).to(torch.float16).to(dev)
        q = torch.randn(1, H, D, generator=g).to(torch.float16).to(dev)
        fp16_bytes = 2 * H * S * D * 2
        copies = max(2, min(64, int(1.05e9 // fp16_bytes) + 1))
        rows = []
        # (b) the parent commit: fake-quantised fp16 tensors through sdpa
        Kq, Vq = kvcache.mx_quantize_keys(K), kvcache.mx_quantize_values(V)
        caches = [(Kq.clone(), Vq.clone()) for _ in range(copies)]
        q4 = q[:, :, None, :]
        ms_b = timed([(lambda k=k, v=v: sdpa(q4, k, v)) for k, v in caches], args.rounds)
        rows.append(("b fp16 fake-quant + sdpa", ms_b, fp16_bytes, None))
        del caches
        ref = sdpa(q4.float(), Kq.float(), Vq.float())[:, :, 0, :]
        for fmt in ("fp8_e4m3", "fp4_e2m1"):
            pks = []
            for _ in range(copies):
                pk = kvpacked.PackedKV(1, H, D, torch.float16, fmt, gap=32, capacity=S, device=dev)
                pk.append(K, V)
                pks.append(pk)
            nbytes = kvpacked.plane_nbytes(1, H, S, D, fmt)
            ms_a = timed([(lambda pk=pk: pk.attend(q)) for pk in pks], args.rounds)
            code_bytes = pks[0].planes["k_codes"].numel()

            def probe(pk, blocks, infl):
                for n in ("k_codes", "v_codes"):
                    _lib.check(_lib.lib().msq_read_stream_probe(_lib.ptr(pk.planes[n]), code_bytes, blocks, infl, _lib.ptr(sink),
                                                                _lib.current_stream(dev)), "msq_read_stream_probe")
            rd = min(timed([(lambda pk=pk: probe(pk, blocks, infl)) for pk in pks], args.rounds) for blocks, infl in ((512, 4), (1024, 4), (256, 8)))
            rd = rd * nbytes / (2 * code_bytes)                 # scaled from the two code planes to all four
            rows.append(("a attend %s" % fmt, ms_a, nbytes, rd))
            ms_c = timed([(lambda pk=pk: sdpa(q4, *pk.dequantize())) for pk in pks[:max(2, copies // 4)]], max(2, args.rounds // 4))
            rows.append(("c dequantize + sdpa %s" % fmt[:3], ms_c, nbytes + 2 * fp16_bytes, None))
            if fmt == "fp8_e4m3":                                # the two caches hold different values (MX in-dtype against float32): report, do not gate
                y = pks[0].attend(q, out_dtype=torch.float32)
                lines.append("# S %d: max |attend(fp8) - sdpa(fp16 fake-quant)| = %.3e (max |ref| %.3e)" % (S, float((y - ref).abs().max()), float(ref.abs().max())))
            del pks
        for name, ms, nb, rd in rows:
            lines.append("  %-6d %-22s %10.4f %12.2f %10.1f %14s %12s" % (S, name, ms, nb / 1e6, nb / ms / 1e6, "%.4f" % rd if rd else "-",
                                                                        "%.2f" % (rd / ms) if rd else "-"))
        lines.append("  %-6d byte ratio fp16 / fp8 %.2f, measured (b) / (a fp8) %.2f; fp16 / fp4 %.2f, measured (b) / (a fp4) %.2f" % (
            S, 16 / 8.25, ms_b / rows[1][1], 16 / 4.25, ms_b / rows[3][1]))
    lines.append("#")
    lines.append("# decode step of one layer [1, %d, S, %d] fp16: append one token + attend; ms per step over windows of 64 steps, median (min .. max) of %d repeats" % (H, D, args.step_repeats))
    lines.append("# %-6s %-10s %-32s %10s %22s" % ("S", "format", "variant", "ms", "range"))
    for S in [int(s) for s in args.step_sizes.split(",") if s]:
        for fmt in ("fp8_e4m3", "fp4_e2m1"):
            res = step_three_ways(S, fmt, dev, args.step_repeats)
            med = {n: sorted(v)[len(v) // 2] for n, v in res.items()}
            for n, v in res.items():
                lines.append("  %-6d %-10s %-32s %10.4f %10.4f .. %-10.4f" % (S, fmt, n, med[n], min(v), max(v)))
            lines.append("  %-6d %-10s step: eager host / graph replay %.2f, eager device / graph replay %.2f; attention launch device / host lengths %.3f eager, %.3f replayed" % (
                S, fmt, med["d eager host lengths"] / med["f graph replay"], med["e eager device lengths"] / med["f graph replay"],
                med["attend device-length"] / med["attend host-length"], med["attend device-length, replayed"] / med["attend host-length, replayed"]))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
