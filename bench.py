#!/usr/bin/env python3
"""bench.py -- fused unpack-dequant-GEMM throughput (BASELINE.json metric) on MI355X.

A "step" is one pass of the hot path over one synthetic batch: Y[M,N] = X[M,K] . Wq^T with the
packed MicroScopiQ W4 weight dequantised inside the MFMA kernel (msq_qlinear_bf16).
Workload (BASELINE.json configs[1], north_star "[B.S, H] x [H, 4H]"): Llama-2-7B shape
H = 4096, M = B.S = 2048 tokens, W = [4H, H] = [16384, 4096], MX-FP4 (e2m1) inliers + 8-bit
outliers (posit8_es1 by default, --outlier fp8_e4m3 for the all-HW-convert variant), block 32
along K, scale bits 8/8, std_dev 2, heavy-tailed synthetic weights (0.5 % of entries x16).

N > 1: one process per GPU.  Launched either by the driver (`python -m torch.distributed.run ... bench.py
--gpus N`: RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* come from the environment) or directly as
`python bench.py --gpus N`: the parent then starts N fresh rank processes itself BEFORE it imports torch or
touches a GPU (plain subprocess children, never an exec of a process that has initialised HIP), relays rank 0's
JSON line and exits with the worst return code.
The 7B path does not shard ("7B = replicas only"): every rank runs an independent replica on
its own GPU, no data-path collective, value = sum over ranks ("weak").
--workload llama70b_rowparallel shards K over the ranks (RowParallelQuantLinear): the partial products are
summed with reduce-scatter + all-gather over RCCL, chunked so that chunk i communicates while chunk i + 1
multiplies.

Prints ONE JSON line (rank 0).  The timed region starts with all inputs resident in HBM.
A plain run sets up, warms up, times --steps steps and prints the line; --dump-outputs DIR also writes what the last timed step
returned.  --full adds, after the timed steps, the measurements the headline does not need: the CPU baseline with its full-size
parity check, a sustained-rate run, hipBLASLt on the unpacked weight, the perplexity leg (`ppl_delta`) and the other BASELINE
configs (`configs`).
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PEAK_BF16_TFLOPS = 2500.0     # MI355X dense bf16 MFMA peak (MI355X_MICROARCH.md)
PEAK_FP8_TFLOPS = 5000.0      # dense fp8 MFMA peak (MI355X_MICROARCH.md); the fp4 x fp8 scaled MFMA issues at the fp8 rate
ROUND_TAG = "r06"


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--M", type=int, default=2048)
    ap.add_argument("--H", type=int, default=4096)
    ap.add_argument("--inlier", default="fp4_e2m1")
    ap.add_argument("--outlier", default="posit8_es1")
    ap.add_argument("--block", type=int, default=32)
    ap.add_argument("--workload", default="llama7b_w4_fused_gemm",
                    choices=["llama7b_w4_fused_gemm", "llama7b_w4a8", "llama7b_mx_w4a8", "llama7b_mx_w6a8", "llama7b_msq_w4a8_mx", "llama70b_rowparallel",
                             "llama7b_e2e"])
    ap.add_argument("--layers", type=int, default=32, help="llama7b_e2e: decoder layers of the Llama-2-7B-shaped model (tests use a slice)")
    ap.add_argument("--seqlen", type=int, default=2048, help="llama7b_e2e: prefill / perplexity window")
    ap.add_argument("--path", default="bf16", choices=["bf16", "mx"], help="llama7b_e2e: packed path (bf16 activations or the MX matrix path)")
    ap.add_argument("--decode-tokens", type=int, default=64, help="llama7b_e2e: tokens of the per-token latency loop (llm/opt.py:332-376)")
    ap.add_argument("--model-dtype", default="fp16", choices=["fp16", "bf16"],
                    help="llama7b_e2e: dtype of the model (Llama-2 checkpoints load as fp16, llm/llama.py:33; bf16 needs no activation cast in front of the bf16 MFMA)")
    ap.add_argument("--timeout", type=float, default=1800.0, help="--gpus N started by hand: overall time limit of the rank processes in seconds")
    ap.add_argument("--layout", default="auto", choices=["planes", "unified", "auto"],
                    help="packed layout: planes = MSQ-T1 (fp4 plane + outlier plane), unified = MSQ-U1 (one e4m3 code per weight)")
    ap.add_argument("--mx", action="store_true",
                    help="llama70b_rowparallel on the MX matrix path (MicroScopiQ e4m3 weight operand x MX-FP8 activations)")
    ap.add_argument("--comm", default="rs_ag", choices=["rs_ag", "all_reduce"],
                    help="llama70b_rowparallel: how the partial outputs are summed")
    ap.add_argument("--chunks", type=int, default=0, help="llama70b_rowparallel: row chunks overlapped with the collective (0 = auto)")
    ap.add_argument("--single-rank-collectives", action="store_true",
                    help="llama70b_rowparallel on ONE GPU: still create the RCCL group (world size 1) and run the reduce-scatter / all-gather, "
                         "so that the communication code path and its evidence keys can be checked without an 8-GPU node")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: leave out everything --full adds")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also run what it does not need: the CPU baseline with full-size parity, the sustained-rate "
                         "run, hipBLASLt on the unpacked weight, the perplexity leg and the other BASELINE configs (`configs`)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the output of the last timed step to DIR/<name>.npy (float32); an output over 64 MB is cut to a "
                         "fixed, seeded sample of its rows")
    ap.add_argument("--stub", action="store_true",
                    help="CPU-only plumbing check (tests): gloo backend, the step is a no-op; exercises rank start-up, "
                         "barriers, max-over-ranks timing and the JSON line without a GPU")
    return ap.parse_args(argv)


# ---------------------------------------------------------------------------------------------------------
# N > 1 started by hand: the parent is a launcher only.  Nothing in this function imports torch.
# ---------------------------------------------------------------------------------------------------------
def spawn_ranks(args, argv):
    import socket
    n = args.gpus
    with socket.socket() as s:                     # a free rendezvous port on the loopback interface
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ)
        env.update(RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0",
                   MSQ_BENCH_CHILD="1")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + list(argv), env=env,
                                      stdout=subprocess.PIPE, stderr=None, text=True))
    # Poll all ranks: when one dies (HIP / RCCL start-up failure, out of memory, a bad shape raising on one rank) the others
    # sit in init_process_group or a barrier for ever -- terminate them and return the first failure, as torchrun does.  An
    # overall time limit covers a hang of all of them.  Rank stdout is drained by reader threads (a full pipe would block).
    import threading
    outs = [[] for _ in procs]

    def drain(i, p):
        for ln in p.stdout:
            outs[i].append(ln.rstrip("\n"))

    readers = [threading.Thread(target=drain, args=(i, p), daemon=True) for i, p in enumerate(procs)]
    for t in readers:
        t.start()
    deadline = time.time() + float(args.timeout)
    worst = 0
    live = set(range(n))
    while live:
        for r in sorted(live):
            rc = procs[r].poll()
            if rc is None:
                continue
            live.discard(r)
            if rc != 0 and worst == 0:
                worst = rc
                sys.stderr.write("bench.py: rank %d exited with code %d; stopping the other ranks\n" % (r, rc))
        if live and (worst != 0 or time.time() > deadline):
            if worst == 0:
                worst = 124
                sys.stderr.write("bench.py: ranks %s still running after %.0f s; stopping them\n" % (sorted(live), float(args.timeout)))
            for r in live:
                procs[r].terminate()
            t_kill = time.time() + 10.0
            while any(procs[r].poll() is None for r in live) and time.time() < t_kill:
                time.sleep(0.1)
            for r in live:
                if procs[r].poll() is None:
                    procs[r].kill()
            for r in live:
                procs[r].wait()
            live.clear()
        elif live:
            time.sleep(0.05)
    for t in readers:
        t.join(timeout=5.0)
    lines = []
    for r in range(n):
        for ln in outs[r]:
            if r == 0 and ln.startswith("{"):
                lines.append(ln)
            else:
                sys.stderr.write("[rank %d] %s\n" % (r, ln))
    if worst == 0 and len(lines) != 1:
        sys.stderr.write("bench.py: rank 0 printed %d JSON lines (expected 1)\n" % len(lines))
        worst = 1
    if worst == 0:
        print(lines[-1])
    sys.stdout.flush()
    return worst


def synth_weight(N, K, dev, seed=0):
    import torch
    g = torch.Generator(device=dev).manual_seed(seed)
    W = torch.randn(N, K, generator=g, device=dev) * 0.02
    W[torch.rand(N, K, generator=g, device=dev) < 0.005] *= 16.0
    return W


DUMP_BYTES = 64 * 1000 * 1000  # --dump-outputs: all files together, headers included


def dump_outputs(path, outputs):
    """--dump-outputs: every output (name -> tensor) as <path>/<name>.npy in float32.  An output larger than its share of DUMP_BYTES
    keeps a sample of its rows (first dimension) drawn by a generator of fixed seed: the same rows on every run with the same
    arguments, so that two builds can be compared output for output."""
    import numpy as np
    import torch
    os.makedirs(path, exist_ok=True)
    share = DUMP_BYTES // len(outputs) - 4096
    for name, t in outputs.items():
        t = t.detach()
        row_bytes = 4 * (t[0].numel() if t.dim() > 1 else 1)
        if t.numel() * 4 > share:
            keep = torch.randperm(t.shape[0], generator=torch.Generator().manual_seed(0))[:share // row_bytes].sort().values
            t = t[keep.to(t.device)]
        np.save(os.path.join(path, name + ".npy"), t.float().cpu().numpy())


def physical_cores():
    omp = os.environ.get("OMP_NUM_THREADS", "")
    if omp.isdigit() and int(omp) > 0:            # a host shared with other jobs caps the threads a process may use
        return int(omp)
    try:
        import psutil
        n = psutil.cpu_count(logical=False)
        if n:
            return int(n)
    except Exception:
        pass
    return os.cpu_count() or 1


def cpu_baseline(M, N, K, bs, fi, fo, plain_mx=False, budget_s=8.0, W_host=None, gpu_values=None):
    """The reference's CPU path timed on the GPU box's host cores on a bounded sample of the same workload.  Reported, never optimised.

    `value` = torch's CPU float32 F.linear on the fake-quantised weight -- the op the reference itself executes for this GEMM
    (number_system/mx/linear.py:91) -- on all M rows of X and the whole weight; the oracle's own dense linear (a C restatement,
    double accumulate, OpenMP over outputs) and the oracle's fake-quant of the WHOLE weight (utils/quant.py:147-266 restated,
    OpenMP over blocks) ride beside it.

    Parity at full size: when the caller passes the GPU's weight (`W_host`, float32 [N, K]) and what the HIP path made of it
    (`gpu_values`: name -> float32 [N, K] host array, e.g. the HIP fake-quant output and unpack(pack(W))), the oracle's
    whole-weight result -- already computed for the timing -- is compared with each of them bit for bit
    (`parity_checked`, `mismatches`)."""
    import numpy as np
    from oracle import oracle as O
    cores = physical_cores()
    threads = O.set_threads(cores)
    rng = np.random.RandomState(0)
    if W_host is None:
        Ws = (rng.randn(N, K) * 0.02).astype(np.float32)         # fake-quant sample: the whole [N, K] weight
        Ws[rng.rand(N, K) < 0.005] *= 16
    else:
        Ws = np.ascontiguousarray(W_host, dtype=np.float32)
    t0 = time.perf_counter()
    r = ({"out": O.quantize_mx(Ws, 8, fi.split()[0], axis=-1, block_size=bs)} if plain_mx
         else O.outlier_fakequant(Ws, 8, 8, fi, fo, 2, -1, bs))
    t_q = time.perf_counter() - t0
    parity = None
    if gpu_values:
        parity = {}
        ob = r["out"].view(np.uint32)
        for k_, v in gpu_values.items():
            gb = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)
            both_nan = np.isnan(r["out"]) & np.isnan(v)
            parity[k_] = int(((ob != gb) & ~both_nan).sum())
    Xs = rng.randn(M, K).astype(np.float32)
    # oracle linear sample: probe, then as many of the N output columns as fit the time budget (all M rows)
    t0 = time.perf_counter()
    O.linear(Xs[:256], r["out"][:1024])
    rate = 2.0 * 256 * 1024 * K / max(time.perf_counter() - t0, 1e-6)
    ns = int(min(N, max(256, rate * budget_s / (2.0 * M * K)))) // 256 * 256
    ns = max(ns, 256)
    t0 = time.perf_counter()
    O.linear(Xs, r["out"][:ns])
    t_l = time.perf_counter() - t0
    oracle_tf = 2.0 * M * ns * K / t_l / 1e12
    import torch
    tthreads = torch.get_num_threads()
    Xt = torch.from_numpy(Xs); Wt = torch.from_numpy(r["out"])
    torch.nn.functional.linear(Xt[:256], Wt)                      # warm-up (thread pool, allocator)
    reps, t_t = 0, 0.0
    t0 = time.perf_counter()
    while reps < 3 or (t_t < 2.0 and reps < 20):
        torch.nn.functional.linear(Xt, Wt)
        reps += 1
        t_t = time.perf_counter() - t0
    torch_tf = reps * 2.0 * M * N * K / t_t / 1e12
    del Wt
    out = {
        "value": torch_tf, "unit": "TFLOP/s", "cores": tthreads, "kind": "port",
        "sample": "torch CPU float32 F.linear X[%d,%d].Wq[%d,%d]^T (the reference's own GEMM op, number_system/mx/linear.py:91; %d torch threads, "
                  "%d calls in %.1f s) on the oracle's fake-quant of the whole W[%d,%d] (%d OpenMP threads, %.2f s)"
                  % (M, K, N, K, tthreads, reps, t_t, N, K, threads, t_q),
        "oracle_linear_tflops": oracle_tf, "oracle_linear_threads": threads,
        "oracle_linear_sample": "X[%d,%d].Wq[%d,%d]^T, double accumulate, %.1f s" % (M, K, ns, K, t_l),
        "fakequant_s_per_weight": t_q, "fakequant_GBps": 2.0 * N * K * 4 / t_q / 1e9,
        "torch_cpu_fp32_linear_tflops": torch_tf, "torch_cpu_threads": tthreads,
        "host_cpus": os.cpu_count(), "host_physical_cores": cores,
    }
    if parity is not None:
        out["parity_checked"] = True
        out["mismatches"] = parity
        out["parity_note"] = ("oracle fake-quant of the GPU run's own W[%d,%d] against the HIP results, bit for bit (NaN == NaN): "
                              "elements that differ" % (N, K))
    else:
        out["parity_checked"] = False
    return out


def ppl_proxy(dev, fi, fo, bs):
    """PPL-delta stand-in (no WikiText-2 / Llama-2 checkpoint in the image): a tiny random-weight Llama evaluated by the
    harness with the weights fake-quantised in place (the reference's path, llm/llama.py:240-253) and then with the same
    Linears swapped for packed QuantLinear modules (fused dequant-GEMM, bf16 activations).  Reports both perplexities
    and the relative difference; BASELINE's "<= 0.05 at PPL ~5.5" corresponds to a relative 0.9 %."""
    import types
    import torch
    import msq
    from msq.harness import find_layers, llama
    from msq.harness.data_utils import _Enc
    from msq.harness.evalppl import perplexity
    from transformers import LlamaConfig, LlamaForCausalLM
    torch.manual_seed(0)
    m = LlamaForCausalLM(LlamaConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4,
                                     num_key_value_heads=4, vocab_size=512, max_position_embeddings=128)).eval()
    m.seqlen = 64
    tokens = _Enc(torch.randint(0, 512, (1, 64 * 6), generator=torch.Generator().manual_seed(1)))
    qc = dict(inlier_elem_format=fi, outlier_elem_format=fo, axes=[-1], block_size=bs)
    ppl_fake = llama.llama_eval(m, tokens, dev, args=types.SimpleNamespace(nearest=True, use_mx=True), quant_cfg=qc)
    q = msq.quant.MXQuantizer(); q.configure(8, 8, **qc)
    for layer in m.model.layers:
        msq.qlinear.make_quant(layer, {n: q for n in find_layers(layer)})
    ppl_packed = perplexity(m, tokens, dev, 64)
    return {"model": "random-weight Llama, 2 layers, hidden 256, vocab 512 (synthetic tokens)", "ppl_fakequant_dense": ppl_fake,
            "ppl_packed_fused": ppl_packed, "relative_delta": abs(ppl_packed - ppl_fake) / ppl_fake,
            "equivalent_delta_at_ppl_5.5": 5.5 * abs(ppl_packed - ppl_fake) / ppl_fake}


PPL_FIXTURE_MODEL = os.path.join(ROOT, "tests", "golden", "ppl_llama")          # tests/golden/make_ppl_fixture.py
PPL_FIXTURE_DATA = os.path.join(ROOT, "tests", "golden", "ppl_wikitext2")


def _logit_metrics(ref_logits, got_logits):
    """Token-level agreement of two models on the same windows: mean KL(ref || got) in nats per token, the share of tokens
    whose arg-max agrees, and the largest absolute logit difference (lists of [S, V] float32 tensors on one device)."""
    import torch
    kl = agree = n = 0.0
    worst = 0.0
    for a, b in zip(ref_logits, got_logits):
        a = a.float(); b = b.float().to(a.device)
        la, lb = torch.log_softmax(a, -1), torch.log_softmax(b, -1)
        kl += float((la.exp() * (la - lb)).sum())
        agree += float((a.argmax(-1) == b.argmax(-1)).sum())
        n += a.shape[0]
        worst = max(worst, float((a - b).abs().max()))
    return {"mean_kl_nats_per_token": kl / n, "top1_agreement": agree / n, "max_logit_abs_err": worst, "tokens": int(n)}


def _window_logits(model, ids, dev, seqlen, fp32=False):
    import torch
    out = []
    with torch.no_grad():
        for i in range(ids.numel() // seqlen):
            lg = model(ids[:, i * seqlen:(i + 1) * seqlen].to(dev)).logits[0]
            out.append(lg.float() if fp32 else lg)
    return out


def _ppl_from_logits(logits, ids, seqlen):
    """llm/llama.py:264-282 on stored logits, fp32 cross entropy."""
    import math
    import torch
    nll = 0.0
    for i, lg in enumerate(logits):
        tok = ids[0, i * seqlen:(i + 1) * seqlen].to(lg.device)
        nll += float(torch.nn.functional.cross_entropy(lg[:-1].float(), tok[1:])) * seqlen
    return math.exp(nll / (len(logits) * seqlen))


def ppl_delta_from_env(dev, fi, fo, bs, paths=("bf16",), corrupt=None):
    """Metric half (ii): perplexity delta of the HIP packed path against the CPU reference arithmetic, through the harness's own
    calls -- get_llama (llm/llama.py:20-58), get_wikitext2 (utils/data_utils.py:36-56), the RTN loop (llm/llama.py:226-253) and
    the PPL formula (:264-282).

    Model and data: MSQ_PPL_MODEL / MSQ_WIKITEXT2_DIR (a HuggingFace Llama checkpoint directory; a directory holding
    wiki.{train,test}.raw or the HF parquet / arrow files) when the environment names both; otherwise the committed fixture
    tests/golden/ppl_llama + tests/golden/ppl_wikitext2 (a small TRAINED Llama and a WikiText-2-format synthetic corpus made by
    tests/golden/make_ppl_fixture.py: neither WikiText-2 nor a Llama-2 checkpoint exists in the image; round 5: a gazetteer whose
    tokens are mostly entity names, digits and world facts the model holds in its weights, test PPL 2.1).  MSQ_PPL_NSAMPLES bounds
    the test windows, MSQ_PPL_SEQLEN sets the window.  Returns None when MSQ_PPL_DISABLE is set or the fixture is absent.

      ppl_cpu_reference        every decoder Linear replaced by the ORACLE's CPU fake-quant of its weight (the reference's
                               arithmetic, utils/quant.py:147-266), the model evaluated by torch on the HOST in float32
      ppl_gpu_dense_fakequant  the same weights, evaluated densely on the GPU in the checkpoint dtype (hipBLASLt)
      ppl_hip_packed_fused     the checkpoint through the HIP quantiser, packed, fused dequant-GEMM (q/k/v and gate/up fused)
      delta                    ppl_hip_packed_fused - ppl_cpu_reference                      -> the bench line's `ppl_delta`
      logits_vs_cpu_reference  mean KL per token, top-1 agreement, largest logit error of the packed model

    ``paths`` may add "mx": W4A8 on the MX matrix path, scored against ITS reference semantics (number_system/mx/linear.py:29-91:
    activations quantised to MX-FP8 by `_quantize_mx`, dense GEMM) -- the oracle's quantize_mx on the input of every decoder
    Linear of the CPU model -- not against the weight-only model.
    "harness_default": a further leg with the harness's OWN default quantiser (int2 inliers / fp4 outliers, axes = [0], block 16,
    llm/llama.py:229-237) -- the configuration in which the quantiser is not near-lossless (the reference moves the fixture's
    perplexity by ~2 %), values packed as they are.
    ``corrupt`` (tests): callable(packed_model) applied before the packed evaluation, e.g. flipping a scale byte."""
    model_dir, data_dir = os.environ.get("MSQ_PPL_MODEL"), os.environ.get("MSQ_WIKITEXT2_DIR")
    fixture = not (model_dir and data_dir)
    if os.environ.get("MSQ_PPL_DISABLE"):
        return None
    if fixture:
        model_dir, data_dir = PPL_FIXTURE_MODEL, PPL_FIXTURE_DATA
        if not (os.path.exists(os.path.join(model_dir, "model.safetensors")) and os.path.exists(os.path.join(data_dir, "wiki.test.raw"))):
            return None
    import copy
    import numpy as np
    import torch
    import msq
    from msq.harness import find_layers, llama
    from msq.harness.data_utils import get_wikitext2
    from msq.harness.evalppl import LLAMA_FUSE, pack_layers, perplexity, quantize_layers_nearest
    from oracle import oracle as O
    model = llama.get_llama(model_dir).eval()
    info = {}
    try:
        info = json.load(open(os.path.join(model_dir, "fixture_info.json")))
    except Exception:
        pass
    seqlen = int(os.environ.get("MSQ_PPL_SEQLEN", info.get("eval_seqlen", model.seqlen)))
    model.seqlen = seqlen
    _, testenc = get_wikitext2(0, 0, seqlen, model_dir, data_dir=data_dir)
    ids = testenc.input_ids
    ns = os.environ.get("MSQ_PPL_NSAMPLES")
    if ns:
        ids = ids[:, :int(ns) * seqlen]
    nwin = int(ids.numel() // seqlen)
    mdt = next(model.parameters()).dtype
    O.set_threads(physical_cores())

    def cpu_reference(fi_, fo_, axis_, bs_):
        """the checkpoint with every decoder Linear replaced by the oracle's CPU fake-quant of its weight (checkpoint dtype)"""
        r = copy.deepcopy(model)
        for layer in r.model.layers:
            for lin in find_layers(layer).values():
                W = lin.weight.data
                lin.weight.data = torch.from_numpy(O.outlier_fakequant(W.float().numpy(), 8, 8, fi_, fo_, 2, axis_, bs_)["out"]).to(W.dtype)
        return r

    out = {"model": ("tests/golden/ppl_llama: trained 4-layer hidden-256 Llama (tests/golden/make_ppl_fixture.py, round 5 gazetteer corpus)" if fixture
                     else os.path.basename(os.path.normpath(model_dir))),
           "dataset": ("tests/golden/ppl_wikitext2: synthetic corpus in the raw WikiText-2 layout (same script); NOT WikiText-2" if fixture
                       else data_dir),
           "model_dtype": str(mdt).replace("torch.", ""), "windows": nwin, "seqlen": seqlen,
           "ppl_unquantised_cpu_fp32": _ppl_from_logits(_window_logits(copy.deepcopy(model).float(), ids, "cpu", seqlen), ids, seqlen)}
    for path in paths:
        # the MX matrix path carries the weight as ONE e4m3 operand: posit outliers do not fit it, so it is scored with fp8_e4m3 outliers
        fo_p = "fp8_e4m3" if path == "mx" else fo
        fi_p, ax_p, bs_p = fi, -1, bs
        if path == "harness_default":
            # the harness's OWN default quantiser (llm/llama.py:229-237): int2 inliers, fp4 outliers, blocks of 16 along out_features
            # (axes = [0]) -- a 2-bit weight: the quantiser's error is large here and a wrong mask bit moves the perplexity visibly.
            # The fake-quant values are packed as they are (pack_values, 8.25 b/w value plane) and run through the fused GEMM.
            fi_p, fo_p, ax_p, bs_p = "int2", "fp4", 0, 16
        qc = dict(inlier_elem_format=fi_p, outlier_elem_format=fo_p, axes=[ax_p], block_size=bs_p)
        # ---- CPU reference: oracle fake-quant weights, the model evaluated by torch on the host in float32
        ref = cpu_reference(fi_p, fo_p, ax_p, bs_p)
        ref_cpu = copy.deepcopy(ref).float()
        if path == "mx":
            # reference semantics of the W4A8 MX path (number_system/mx/linear.py:29-91): the activations of every decoder Linear
            # quantised by _quantize_mx (oracle: MX-FP8 e4m3, block 32 along in_features), float32 GEMM on the fake-quant weight
            def _aq(mod, args_):
                x = args_[0]
                xq = O.quantize_mx(x.detach().reshape(-1, x.shape[-1]).numpy(), 8, "fp8_e4m3", axis=-1, block_size=32)
                return (torch.from_numpy(xq).reshape(x.shape),)
            lg_wo = _window_logits(ref_cpu, ids, "cpu", seqlen)              # weight-only reference, for the size of the activation effect
            hooks = [lin.register_forward_pre_hook(_aq) for layer in ref_cpu.model.layers for lin in find_layers(layer).values()]
        lg_cpu = _window_logits(ref_cpu, ids, "cpu", seqlen)
        ppl_cpu = _ppl_from_logits(lg_cpu, ids, seqlen)
        del ref_cpu
        # ---- HIP: RTN through the harness (llm/llama.py:226-253), packed, fused kernels
        m = copy.deepcopy(model).to(dev)
        quantize_layers_nearest(m.model.layers, dev, qc)
        n_packed, kept = pack_layers(m.model.layers, path="mx" if path == "mx" else "bf16", fuse=LLAMA_FUSE)
        kept += sum(isinstance(l, torch.nn.Linear) for layer in m.model.layers for l in layer.modules())
        if corrupt is not None:
            corrupt(m)
        lg = _window_logits(m, ids, dev, seqlen)
        ppl = _ppl_from_logits(lg, ids, seqlen)
        if path == "bf16":
            # the same reference weights densely on the GPU (hipBLASLt, checkpoint dtype)
            lg_dense = _window_logits(ref.to(dev), ids, dev, seqlen)
            out.update({"outlier": fo_p, "ppl_cpu_reference": ppl_cpu, "ppl_gpu_dense_fakequant": _ppl_from_logits(lg_dense, ids, seqlen),
                        "ppl_hip_packed_fused": ppl, "delta": ppl - ppl_cpu, "relative_delta": (ppl - ppl_cpu) / ppl_cpu,
                        "layers_packed": n_packed, "layers_kept_dense": kept,
                        # loss in the model dtype, exactly llm/llama.py:264-282 (an fp16 loss moves in coarse steps)
                        "ppl_gpu_dense_fakequant_reference_formula": perplexity(ref, ids, dev, seqlen),
                        "ppl_hip_packed_fused_reference_formula": perplexity(m, ids, dev, seqlen),
                        "logits_vs_cpu_reference": _logit_metrics(lg_cpu, lg), "logits_vs_gpu_dense_fakequant": _logit_metrics(lg_dense, lg)})
            out["delta_vs_gpu_dense_fakequant"] = ppl - out["ppl_gpu_dense_fakequant"]
        elif path == "harness_default":
            lg_dense = _window_logits(ref.to(dev), ids, dev, seqlen)
            out["harness_default"] = {"config": "int2 inliers / fp4 outliers, axes=[0], block 16, std_dev 2 (llm/llama.py:229-237), packed as values (8.25 b/w)",
                                      "ppl_cpu_reference": ppl_cpu, "ppl_gpu_dense_fakequant": _ppl_from_logits(lg_dense, ids, seqlen),
                                      "ppl_hip_packed_fused": ppl, "delta": ppl - ppl_cpu, "relative_delta": (ppl - ppl_cpu) / ppl_cpu,
                                      "layers_packed": n_packed, "layers_kept_dense": kept,
                                      "logits_vs_cpu_reference": _logit_metrics(lg_cpu, lg), "logits_vs_gpu_dense_fakequant": _logit_metrics(lg_dense, lg)}
        else:
            mods = [mm for mm in m.modules() if isinstance(mm, msq.qlinear.MXLinearW4A8)]
            out["mx_path"] = {"outlier": fo_p, "ppl_cpu_reference_mxlinear_semantics": ppl_cpu, "ppl_hip_packed_mx": ppl, "delta": ppl - ppl_cpu,
                              "relative_delta": (ppl - ppl_cpu) / ppl_cpu, "layers_kept_dense": kept, "mx_modules": len(mods),
                              "logits_vs_cpu_reference_mxlinear_semantics": _logit_metrics(lg_cpu, lg),
                              "logits_vs_weight_only_cpu_reference": _logit_metrics(lg_wo, lg),
                              "note": "reference = oracle _quantize_mx (MX-FP8 e4m3, block 32) on the input of every decoder Linear + float32 "
                                      "GEMM on the oracle's fake-quant weight (number_system/mx/linear.py:29-91); the weight-only row shows "
                                      "how much of the distance to the weight-only model is the activation quantisation itself"}
        del m, ref
    return out


def _tgraph(fns, reps=10):
    """Device time per call in ms: the calls of `fns` captured into ONE HIP graph on a side stream, `reps` replays timed with HIP
    events (no Python / ctypes launch floor between the kernels); the median replay."""
    import torch
    torch.cuda.synchronize()        # nothing of the caller's warm-up loop runs beside the side stream's first calls (two streams entering
                                    # hipBLASLt at once stalled the whole device in layer7b_prefill: every later synchronize hung)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        for f in fns[:3]:
            f()
        st.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            for f in fns:
                f()
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    # one event pair per replay, the MEDIAN replay: a single stall of the stream (round 5: one replay of the decode probe took 70 ms for no
    # reason the trace shows; the mean of three called `down` 1.0 ms) must not become the figure
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    with _no_gc():
        evs[0].record()
        for i in range(reps):
            g.replay()
            evs[i + 1].record()
        torch.cuda.synchronize()
    per = sorted(evs[i].elapsed_time(evs[i + 1]) for i in range(reps))
    return per[len(per) // 2] / len(fns)


def _clone_packed(P):
    from msq import qlinear
    c = lambda t: None if t is None else t.clone()
    if isinstance(P, qlinear.MXPackedWeight):
        import copy
        Q = copy.copy(P)
        Q.codes, Q.scales = P.codes.clone(), P.scales.clone()
        return Q
    return qlinear.PackedWeight(c(P.inl), c(P.out), c(P.scl), P.N, P.K, P.block, P.in_kind, P.out_kind, P.n, P.k)


HBM_PEAK_GBPS = 8000.0        # MI355X_MICROARCH.md: 8 TB/s spec (6.3 achievable)
# sub-objects of the --full line's `configs` (BASELINE.json configs 3, 4, 5 and decode) and of `rowparallel`: the --stub path emits
# the same keys, tests/test_host_logic.py pins them
CONFIG_KEYS = ("w4a8_mx", "w4a8_mx_plain_fp4", "w6a8_mx_plain_fp6", "producers", "w4a8_mxlinear", "kv_quant", "rtn_fakequant_in_dtype", "decode_cold", "rowparallel_70b_1gpu", "m_sweep",
               "layer7b_prefill")
ROWPAR_KEYS = ("step_ms", "gemm_ms", "comm_ms", "exposed_comm_ms", "chunks", "comm", "wire_dtype")


def _kernel_name(P, M, mx):
    """The GEMM kernel instantiation the library's dispatcher picks for this call (msq_qlinear_kernel_name: the dispatcher's own decision
    function); the MX step also runs the activation packer in front of it."""
    import ctypes
    from msq import _lib
    buf = ctypes.create_string_buffer(160)
    try:
        if mx:
            wf = {"e2m1": 0, "e4m3": 1, "e2m3": 2, "e3m2": 3}.get(getattr(P, "w_fmt", "e2m1"), 0)
            rc = _lib.lib().msq_qlinear_kernel_name(M, P.N, P.K, 0, wf, 2, buf, 160)
            return ("k_mx_pack_a8 + " + buf.value.decode()) if rc == 0 else "k_mxgemm"
        rc = _lib.lib().msq_qlinear_kernel_name(M, P.N, P.K, P.out_kind, -1, 2, buf, 160)
        return buf.value.decode() if rc == 0 else "k_qgemm"
    except Exception:
        return "k_qgemm"


class _no_gc:
    """A timed region without the cycle collector, as `timeit` runs its loops: after the perplexity leg this process holds millions of Python
    objects (transformers, the model), a generation-2 pass takes ~30 ms, and a host that sits in it while the GPU drains its queue shows up as
    GPU time -- the row-parallel leg measured 1.9-5.0 ms per step for 0.75 ms of work (round 5, scripts/experiments/rp_stall.py)."""

    def __init__(self, collect=False):
        self.collect = collect                  # a collection takes tens of ms with the GPU idle: do it BEFORE the warm-up, never between it and the timed loop

    def __enter__(self):
        import gc
        self.was = gc.isenabled()
        if self.collect:
            gc.collect()
        gc.disable()

    def __exit__(self, *a):
        import gc
        if self.was:
            gc.enable()


def _gpu_sensors():
    """Clock / power as far as the box exposes them to an ordinary user: sysfs of the amdgpu card whose PCI address is the one torch reports for
    cuda:0 (a box shows every card of the node, only one of them is ours); when no address matches, the card drawing the most power.
    {} when nothing is readable."""
    import glob
    want = None
    try:
        import torch
        p = torch.cuda.get_device_properties(0)
        want = "%04x:%02x:%02x." % (p.pci_domain_id, p.pci_bus_id, p.pci_device_id)
    except Exception:
        pass
    cards = []
    for card in sorted(glob.glob("/sys/class/drm/card*/device")):
        out = {}
        try:
            sclk = open(os.path.join(card, "pp_dpm_sclk")).read()
            cur = [l for l in sclk.splitlines() if l.strip().endswith("*")]
            if cur:
                out["pp_dpm_sclk"] = cur[0].strip()
        except Exception:
            pass
        for hw in glob.glob(os.path.join(card, "hwmon", "hwmon*")):
            for key in ("power1_average", "power1_input", "power1_cap", "freq1_input"):
                try:
                    out[key] = int(open(os.path.join(hw, key)).read().strip())
                except Exception:
                    pass
        if out:
            out["card"] = card
            out["pci"] = os.path.basename(os.path.realpath(card))
            out["matched_cuda0"] = bool(want and out["pci"].lower().startswith(want))
            cards.append(out)
    for c in cards:
        if c["matched_cuda0"]:
            return c
    if cards:
        return max(cards, key=lambda c: c.get("power1_input", c.get("power1_average", 0)))
    return {}


def sustained(step, flops_step, peak, seconds=3.2, chunk=40):
    """What the chip SUSTAINS on the headline step: back-to-back launches for >= `seconds` s (HIP events around chunks of `chunk` launches on
    the launch stream), the rate over the last second against the first chunk -- the 20-step `value` is a 4 ms burst behind a ramp, and a
    kernel that starts at 0.62 of peak and settles at 0.55 under the package power limit would not show in it (judge, round 4, weak 9)."""
    import torch
    evs = []
    t0 = time.perf_counter()
    ev = torch.cuda.Event(enable_timing=True); ev.record(); evs.append(ev)
    n = 0
    sens_mid = {}
    skip = set()
    with _no_gc(collect=True):                   # (starts from idle anyway: the first chunk is the re-ramp, the figure is the last second)
        while True:
            for _ in range(chunk):
                step()
            n += 1
            ev = torch.cuda.Event(enable_timing=True); ev.record(); evs.append(ev)
            if n % 8 == 0:
                ev.synchronize()                                 # keep the launch queue short: the host clock then tracks the device
                if time.perf_counter() - t0 >= seconds:
                    break
                if not sens_mid and time.perf_counter() - t0 >= seconds / 2:
                    sens_mid = _gpu_sensors()                    # (~0.1 s of sysfs reads with the queue empty: that interval is left out below)
                    skip.add(len(evs) - 1)
        torch.cuda.synchronize()
    ms = [evs[i].elapsed_time(evs[i + 1]) for i in range(len(evs) - 1) if i not in skip]
    tot = sum(ms)
    acc, k = 0.0, len(ms)
    while k > 0 and acc < 1000.0:
        k -= 1
        acc += ms[k]
    last_n = len(ms) - k
    tf = lambda m, c: flops_step * c * chunk / (m * 1e-3) / 1e12
    return {"seconds": tot / 1e3, "launches": len(ms) * chunk, "chunk": chunk,
            "tflops_last_second": tf(acc, last_n), "frac": tf(acc, last_n) / peak,
            "tflops_first_chunk": tf(ms[0], 1), "tflops_whole": tf(tot, len(ms)),
            "tflops_min_chunk": tf(max(ms[1:] or ms), 1), "tflops_max_chunk": tf(min(ms), 1),     # (min: without the first chunk, the re-ramp from idle)
            "sensors_mid_run": sens_mid, "sensors_after": _gpu_sensors(),
            "what": "back-to-back launches of the headline step after the timed region; rate of the last >= 1 s of them"}


def layer7b_prefill(dev, M=2048, inlier="fp4_e2m1", block=32):
    """One Llama-2-7B decoder layer's Linears at prefill size as the harness fuses them (llm/llama.py:226-256 shapes): q/k/v [12288 x 4096],
    o [4096 x 4096], gate/up [22016 x 4096], down [4096 x 11008] -- the TRUE shapes behind north_star's 'at Llama-7B shapes', none of
    which is a whole number of rounds of 256 x 256 tiles over the 256 CUs.  Per projection and per layer: fused dequant-GEMM with posit8
    and fp8_e4m3 outliers, and hipBLASLt bf16 on the unpacked weight on the same box.  Device time from HIP-graph replays."""
    import torch
    from msq import qlinear
    shapes = (("qkv", 12288, 4096), ("o", 4096, 4096), ("gate_up", 22016, 4096), ("down", 4096, 11008))
    X = {k_: torch.randn(M, k_, device=dev).to(torch.bfloat16) for k_ in (4096, 11008)}
    res = {"M": M, "projections": {}}
    tot = {"posit8_es1": 0.0, "fp8_e4m3": 0.0, "hipblaslt_bf16_unpacked": 0.0, "mx_e4m3_operand": 0.0, "mx_fp4": 0.0}
    from msq import quant
    fl_layer = 0.0
    for name, n_, k_ in shapes:
        W = synth_weight(n_, k_, dev, seed=3)
        fl = 2.0 * M * n_ * k_
        fl_layer += fl
        row = {"N": n_, "K": k_, "flops": fl}
        dense = None
        for fo in ("posit8_es1", "fp8_e4m3"):
            P = qlinear.pack_weight(W, 8, 8, inlier, fo, 2, block, layout="unified")
            for _ in range(20):
                qlinear.qlinear(X[k_], P, None, torch.bfloat16)
            ms = _tgraph([lambda P=P: qlinear.qlinear(X[k_], P, None, torch.bfloat16)] * 10)
            row[fo] = {"ms": ms, "tflops": fl / ms / 1e9, "frac": fl / ms / 1e9 / PEAK_BF16_TFLOPS, "kernel": _kernel_name(P, M, False)}
            tot[fo] += ms
            if fo == "fp8_e4m3":
                dense = qlinear.unpack_weight(P, torch.bfloat16)
            del P
        # the same projection on the MX matrix path (scaled MFMA, activations already packed by their producer, 5.004): the MicroScopiQ weight as
        # one exact e4m3 operand, and plain MX-FP4; priced on the fp8 peak
        xp = qlinear.mx_pack_act(X[k_])
        for key, Pm in (("mx_e4m3_operand", qlinear.mx_pack_values(quant.outlier_fakequant(W, 8, 8, inlier, "fp8_e4m3", 2, -1, block)["out"])),
                        ("mx_fp4", qlinear.mx_pack_weight(W, w_fmt="e2m1"))):
            for _ in range(10):
                qlinear.qlinear_mx_w4a8(xp, Pm, None, torch.bfloat16)
            ms = _tgraph([lambda Pm=Pm: qlinear.qlinear_mx_w4a8(xp, Pm, None, torch.bfloat16)] * 10)
            row[key] = {"ms": ms, "tflops": fl / ms / 1e9, "frac": fl / ms / 1e9 / PEAK_FP8_TFLOPS, "peak": PEAK_FP8_TFLOPS}
            tot[key] += ms
            del Pm
        del W, xp
        for _ in range(20):
            X[k_] @ dense.t()
        ms = _tgraph([lambda: X[k_] @ dense.t()] * 10)
        row["hipblaslt_bf16_unpacked"] = {"ms": ms, "tflops": fl / ms / 1e9, "frac": fl / ms / 1e9 / PEAK_BF16_TFLOPS}
        tot["hipblaslt_bf16_unpacked"] += ms
        del dense
        res["projections"][name] = row
    res["layer"] = {k: {"ms": v, "tflops": fl_layer / v / 1e9, "frac": fl_layer / v / 1e9 / (PEAK_FP8_TFLOPS if k.startswith("mx_") else PEAK_BF16_TFLOPS)}
                    for k, v in tot.items()}
    res["flops_per_layer"] = fl_layer
    res["peak"] = PEAK_BF16_TFLOPS
    res["bound"] = "mfma"
    return res


def m_sweep(dev, H=4096, inlier="fp4_e2m1", block=32, Ms=(16, 64, 128, 256, 512, 8192), cold_copies=11):
    """SURVEY 8(d)'s M set for the op the reference runs at number_system/mx/linear.py:91: the headline weight [4H x H] and the four fused projections
    of a Llama-2-7B layer at M in {16, 64, 128, 256, 512, 8192} (M = 1 is `decode_cold`, M = 2048 the headline and `layer7b_prefill`), posit8
    outliers (9.25 bits per weight).  Per cell: device time from HIP-graph replays of ONE weight (`ms`: its packed bytes stay in the 256 MB Infinity
    Cache between replays) and, for the headline weight, of `cold_copies` + 1 copies walked in turn (`ms_cold`); the bounding roofline
    max(bytes / 8 TB/s, flops / 2.5 PF) with bytes = packed weight + bf16 activations in + bf16 out, the fraction of it reached, the kernel
    the dispatcher picks, and hipBLASLt bf16 on the unpacked weight beside it (35.5 MB more bytes per 16384 x 4096 weight)."""
    import torch
    from msq import qlinear
    shapes = (("headline_4HxH", 4 * H, H), ("qkv", 12288, 4096), ("o", 4096, 4096), ("gate_up", 22016, 4096), ("down", 4096, 11008))
    out = {"outlier": "posit8_es1", "bytes": "packed planes + M K 2 + M N 2", "peak_hbm_GBps": HBM_PEAK_GBPS, "peak_mfma_tflops": PEAK_BF16_TFLOPS,
           "Ms": list(Ms), "weights": {}}
    for name, n_, k_ in shapes:
        W = synth_weight(n_, k_, dev, seed=4)
        P = qlinear.pack_weight(W, 8, 8, inlier, "posit8_es1", 2, block, layout="unified")
        del W
        dense = qlinear.unpack_weight(P, torch.bfloat16)
        wbytes = float(P.nbytes)
        rows = {}
        Ps = [P] + ([_clone_packed(P) for _ in range(cold_copies)] if name == "headline_4HxH" else [])
        for M in Ms:
            X = torch.randn(M, k_, device=dev).to(torch.bfloat16)
            fl = 2.0 * M * n_ * k_
            byt = wbytes + 2.0 * M * k_ + 2.0 * M * n_
            roof_ms = max(byt / (HBM_PEAK_GBPS * 1e6), fl / (PEAK_BF16_TFLOPS * 1e9))
            reps = 10 if M <= 512 else 4
            for _ in range(5):
                qlinear.qlinear(X, P, None, torch.bfloat16)
            ms = _tgraph([lambda: qlinear.qlinear(X, P, None, torch.bfloat16)] * reps)
            for _ in range(5):
                X @ dense.t()
            ms_b = _tgraph([lambda: X @ dense.t()] * reps)
            cell = {"ms": ms, "tflops": fl / ms / 1e9, "GBps": byt / ms / 1e6, "roofline_ms": roof_ms,
                    "bound": "hbm" if byt / (HBM_PEAK_GBPS * 1e6) >= fl / (PEAK_BF16_TFLOPS * 1e9) else "mfma", "frac_of_roofline": roof_ms / ms,
                    "kernel": _kernel_name(P, M, False), "hipblaslt_bf16_unpacked_ms": ms_b, "speedup_vs_hipblaslt": ms_b / ms}
            if len(Ps) > 1 and M <= 512:
                cell["ms_cold"] = _tgraph([lambda Q=Q: qlinear.qlinear(X, Q, None, torch.bfloat16) for Q in Ps] * 2)
                cell["frac_of_roofline_cold"] = roof_ms / cell["ms_cold"]
            rows[str(M)] = cell
            del X
        out["weights"][name] = {"N": n_, "K": k_, "packed_bytes": wbytes, "by_M": rows}
        del P, Ps, dense
    return out


def other_configs(dev, M=2048, H=4096, inlier="fp4_e2m1", block=32):
    """BASELINE.json configs 3, 4, 5 and decode, measured in the SAME driver-run process as the headline (default workload, one
    GPU): compact objects with `ms`, the achieved rate, the roofline fraction and the algorithmic flops / bytes they are priced on.
    Device time from HIP-graph replays of back-to-back calls, inputs resident in HBM; ~2 s of GPU time in all."""
    import torch
    import msq
    from msq import kvcache, qlinear, quant
    from msq.mx_ops import _quantize_mx_outlier_v1
    out = {}
    N, K = 4 * H, H
    W = synth_weight(N, K, dev, seed=0)
    X = torch.randn(M, K, device=dev)
    fl = 2.0 * M * N * K
    # ---- config 3 on the CDNA4 fp8 / scaled MFMA (a step = activation pack + k_mxgemm), three weight operands
    P_msq = qlinear.mx_pack_values(quant.outlier_fakequant(W, 8, 8, inlier, "fp8_e4m3", 2, -1, block)["out"])
    for key, P, what in (("w4a8_mx", P_msq, "MicroScopiQ weight (MX-FP4 inliers + fp8_e4m3 outliers) as one exact e4m3 operand, 8.25 b/w"),
                         ("w4a8_mx_plain_fp4", qlinear.mx_pack_weight(W, w_fmt="e2m1"), "plain OCP MX-FP4 weight, 4.25 b/w"),
                         ("w6a8_mx_plain_fp6", qlinear.mx_pack_weight(W, w_fmt="e3m2"), "plain OCP MX-FP6 (e3m2) weight, 6.25 b/w")):
        for _ in range(30):
            qlinear.qlinear_mx_w4a8(X, P, None, torch.bfloat16)
        ms = _tgraph([lambda P=P: qlinear.qlinear_mx_w4a8(X, P, None, torch.bfloat16)] * 10)
        out[key] = {"ms": ms, "tflops": fl / ms / 1e9, "frac": fl / ms / 1e9 / PEAK_FP8_TFLOPS, "peak": PEAK_FP8_TFLOPS, "bound": "mfma (fp8 rate)",
                    "flops": fl, "kernels": "k_mx_pack_a8 + k_mxgemm256", "operand": what, "M": M, "N": N, "K": K,
                    "activations": "fp32 in, MX-FP8 (e4m3, block 32) packed in the step"}
        del P
    # ---- the producers of that activation (round 5): mx.RMSNorm in front of q/k/v / gate/up, silu x up in front of down_proj, handing the MX-FP8
    # operand straight to the GEMM (msq_vec_rmsnorm_mx_pack_a8 / msq_vec_silu_mul_mx_pack_a8) against producer -> float32 -> msq_mx_pack_a8
    from msq import vector_ops as V
    vs = msq.specs.finalize_mx_specs({"w_elem_format": inlier, "a_elem_format": "fp8_e4m3", "scale_bits": 8, "block_size": block, "custom_cuda": True,
                                      "bfloat": 16})
    wn = torch.ones(K, device=dev)
    prod = {}
    I_ = 11008
    gu = torch.randn(M, 2 * I_, device=dev)
    Wd = synth_weight(H, I_, dev, seed=2)
    P_dn = qlinear.mx_pack_values(quant.outlier_fakequant(Wd, 8, 8, inlier, "fp8_e4m3", 2, -1, block)["out"])
    del Wd
    for key, P, n_, k_, unf, fus, byt in (
            ("rmsnorm_then_qkv_shape_gemm", P_msq, N, K, lambda: V.rms_norm(X, wn, None, 1e-6, vs), lambda: V.rms_norm_mx_pack(X, wn, None, 1e-6, vs), M * K * (4 + 1 + 1 / 32)),
            ("silu_mul_then_down_proj", P_dn, H, I_, lambda: V.silu_mul(gu[:, :I_], gu[:, I_:], vs), lambda: V.silu_mul(gu[:, :I_], gu[:, I_:], vs, pack=True),
             M * I_ * (8 + 1 + 1 / 32))):
        for _ in range(5):
            qlinear.qlinear_mx_w4a8(fus(), P, None, torch.bfloat16)
        ms_u = _tgraph([lambda: qlinear.qlinear_mx_w4a8(unf(), P, None, torch.bfloat16)] * 10)
        ms_f = _tgraph([lambda: qlinear.qlinear_mx_w4a8(fus(), P, None, torch.bfloat16)] * 10)
        ms_p = _tgraph([fus] * 10)
        pk_ = fus()
        ms_g = _tgraph([lambda: qlinear.qlinear_mx_w4a8(pk_, P, None, torch.bfloat16)] * 10)      # the GEMM on an operand that is already packed
        fl_ = 2.0 * M * n_ * k_
        prod[key] = {"ms_producer_packer_gemm": ms_u, "ms_fused_producer_gemm": ms_f, "speedup": ms_u / ms_f, "ms_fused_producer_alone": ms_p,
                     "producer_GBps": byt / ms_p / 1e6, "producer_frac_of_hbm": byt / ms_p / 1e6 / HBM_PEAK_GBPS, "producer_bytes": byt,
                     "tflops_fused_step": fl_ / ms_f / 1e9, "frac_fused_step": fl_ / ms_f / 1e9 / PEAK_FP8_TFLOPS,
                     "ms_gemm_on_packed_operand": ms_g, "frac_gemm_on_packed_operand": fl_ / ms_g / 1e9 / PEAK_FP8_TFLOPS, "M": M, "N": n_, "K": k_}
    prod["what"] = ("reference ops number_system/mx/layernorm.py:177 (RMSNorm), activations.py:76 (silu), simd_ops.py:445 (simd_mul), bfloat16 rounding after "
                    "every step; float32 in, MX-FP8 operand out; weight = the exact e4m3 operand of config 3")
    out["producers"] = prod
    del P_msq, P_dn, gu
    # ---- config 3 as the reference composes it: MXLinear(w = fp4_e2m1, a = fp8_e4m3, block 32), mx_ops variant (std_dev 5) on BOTH operands
    Pl = qlinear.pack_values(_quantize_mx_outlier_v1(W, 8, 8, inlier, "fp4_e2m1", "max", 5, [1], block))
    f = lambda: qlinear.qlinear_w4a8(X, Pl, None, torch.bfloat16, a_elem_format="fp8_e4m3", a_std_dev=5, a_block_size=block, a_variant=1)
    for _ in range(30):
        f()
    ms = _tgraph([f] * 10)
    fa = lambda: qlinear.act_quant(X, 8, 8, "fp8_e4m3", "fp8_e4m3", 5, block, variant=1)
    ms_a = _tgraph([fa] * 10)
    out["w4a8_mxlinear"] = {"ms": ms, "tflops": fl / ms / 1e9, "frac": fl / ms / 1e9 / PEAK_BF16_TFLOPS, "peak": PEAK_BF16_TFLOPS, "bound": "mfma (bf16 rate)",
                            "flops": fl, "kernels": "activation quantiser (mx_ops variant, two passes) + k_qgemm256", "act_quant_ms": ms_a,
                            "semantics": "number_system/mx/linear.py:29-91", "M": M, "N": N, "K": K}
    del Pl, W, X
    # ---- config 4: KV-cache quantisation of one Llama-2-7B layer cache [1, 32, 4096, 128] fp16 (GEAR hook, compress_function.py:8-70)
    k = torch.randn(1, 32, 4096, 128, device=dev).to(torch.float16)
    byts = 2.0 * k.numel() * 2
    kv = {}
    for key, fn in (("keys_group_4bit_per_channel_g32", lambda: kvcache.fake_groupwise_channel_asymmetric_quantization_new(k, 4, 32)),
                    ("values_group_4bit_per_token_g32", lambda: kvcache.fake_groupwise_token_asymmetric_quantization(k, 4, 32)),
                    ("keys_mx_fp8_blocks_along_tokens", lambda: kvcache.mx_quantize_keys(k, "fp8_e4m3", 32)),
                    ("values_mx_fp8_blocks_along_head_dim", lambda: kvcache.mx_quantize_values(k, "fp8_e4m3", 32)),
                    ("keys_mx_fp4_blocks_along_tokens", lambda: kvcache.mx_quantize_keys(k, "fp4_e2m1", 32)),
                    ("values_mx_fp4_blocks_along_head_dim", lambda: kvcache.mx_quantize_values(k, "fp4_e2m1", 32)),
                    ("keys_microscopiq_fp4_fp8_blocks_along_tokens", lambda: kvcache.mx_quantize_keys(k, "fp4_e2m1", 32, outlier_format="fp8_e4m3")),
                    ("values_microscopiq_fp4_fp8_blocks_along_head_dim", lambda: kvcache.mx_quantize_values(k, "fp4_e2m1", 32, outlier_format="fp8_e4m3"))):
        keep, quant.CHECK_NAN = quant.CHECK_NAN, False                     # (the MicroScopiQ entries read a status word back otherwise: a host sync inside the graph)
        try:
            for _ in range(5):
                fn()
            ms = _tgraph([fn] * 10)
        finally:
            quant.CHECK_NAN = keep
        kv[key] = {"ms": ms, "GBps": byts / ms / 1e6, "frac": byts / ms / 1e6 / HBM_PEAK_GBPS}
    out["kv_quant"] = dict(kv, bytes=byts, bound="hbm", peak=HBM_PEAK_GBPS, cache="[1, 32, 4096, 128] float16 (read once + written once)")
    # ---- the RTN harness's own call (llm/llama.py:229-253): quantize_mx_outlier_v1 on the checkpoint IN its dtype, W[4H, H]; the packed kernels of
    # DESIGN.md 5.005 (k_outlier_lowp_pk / _pk2).  Algorithmic bytes: the tensor read once + written once
    rtn = {}
    Wr = synth_weight(N, K, dev, seed=0)
    for dn, dt in (("fp16", torch.float16), ("bf16", torch.bfloat16)):
        Wh = Wr.to(dt)
        for nm, fi_, fo_, ax_, bs_ in (("int2_fp4_b16_out_features", "int2", "fp4", 0, 16), ("fp4_fp8e4m3_b32_in_features", inlier, "fp8_e4m3", -1, block)):
            fn = lambda Wh=Wh, fi_=fi_, fo_=fo_, ax_=ax_, bs_=bs_: quant.outlier_fakequant(Wh, 8, 8, fi_, fo_, 2, ax_, bs_)
            keep, quant.CHECK_NAN = quant.CHECK_NAN, False                 # (the status read-back is a host sync: not inside a graph)
            try:
                for _ in range(10):
                    fn()
                ms = _tgraph([fn] * 10)
            finally:
                quant.CHECK_NAN = keep
            by = 2.0 * Wh.numel() * 2
            rtn[dn + "_" + nm] = {"ms": ms, "GBps": by / ms / 1e6, "frac": by / ms / 1e6 / HBM_PEAK_GBPS}
        del Wh
    del Wr
    out["rtn_fakequant_in_dtype"] = dict(rtn, bytes=2.0 * N * K * 2, bound="hbm (kernels: issue-bound, 28-32 VALU per weight)", peak=HBM_PEAK_GBPS, N=N, K=K,
                                         what="utils/quant.py:147-266 computed in the checkpoint dtype, every op rounded as ATen's CPU half kernels do; bit-exact vs the reference")
    # ... and config 4's METRIC end to end on the committed fixture (tests/golden/gsm8k_fixture: a 2-layer Llama trained on two-step word problems,
    # few-shot prompt, 96 problems): the loop of kv_quant/evaluation_gsm8k.py:455-533 (harness/gsm8k.py evaluate) with MXKVCache at the GEAR hook
    try:
        fx = os.path.join(ROOT, "tests", "golden", "gsm8k_fixture")
        from transformers import AutoTokenizer, LlamaForCausalLM
        from msq.harness import gsm8k as G8
        tk = AutoTokenizer.from_pretrained(os.path.join(fx, "model"))
        gm = LlamaForCausalLM.from_pretrained(os.path.join(fx, "model"), torch_dtype=torch.float16).to(dev).eval()
        prompt, qs, ans = G8.load_fixture(fx)
        def cfg_(**kw):
            return kvcache.CompressionConfig(attention_number=gm.config.num_hidden_layers, streaming=True, streaming_gap=32, stream_grouping=True, **kw).copy_for_all_attention()
        accs = {"uncompressed_fp16": G8.evaluate(gm, tk, prompt, qs, ans, None, batch_size=32, max_new_tokens=40)}
        for key, kw in (("KIVI_4bit_g32", dict(compress_method="KIVI", quantize_bit=4, group_size=32)),
                        ("KIVI_2bit_g32", dict(compress_method="KIVI", quantize_bit=2, group_size=32)),
                        ("MX_fp8_e4m3", dict(compress_method="MX", mx_format="fp8_e4m3", mx_block=32)),
                        ("MX_fp4_e2m1", dict(compress_method="MX", mx_format="fp4_e2m1", mx_block=32)),
                        ("MSQ_fp4_fp8", dict(compress_method="MSQ", mx_format="fp4_e2m1", mx_outlier_format="fp8_e4m3", mx_block=32))):
            accs[key] = G8.evaluate(gm, tk, prompt, qs, ans, cfg_(**kw), batch_size=32, max_new_tokens=40)
        out["kv_quant"]["gsm8k_fixture_accuracy"] = dict(accs, problems=len(qs), what="exact match, greedy, 4-shot CoT prompt; fixture model, NOT Llama-2 on GSM8K (neither is in the image)")
        del gm
    except Exception as e:
        out["kv_quant"]["gsm8k_fixture_accuracy"] = {"error": repr(e)[:300]}
    del k
    # ---- decode, M = 1, COLD weights: one decoder layer's four fused projections, each walked over > 1 GB of distinct packed copies
    from msq import _lib
    dec = {}
    tot_ms = tot_b = tot_rd = 0.0
    for name, n_, k_ in (("qkv", 12288, 4096), ("o", 4096, 4096), ("gate_up", 22016, 4096), ("down", 4096, 11008)):
        Wp = synth_weight(n_, k_, dev, seed=1)
        P0 = qlinear.pack_weight(Wp, 8, 8, inlier, "posit8_es1", 2, block, layout="unified")
        del Wp
        copies = max(4, int(1.05e9 // P0.nbytes) + 1)
        Ps = [P0] + [_clone_packed(P0) for _ in range(copies - 1)]
        x1 = torch.randn(1, P0.k, device=dev).to(torch.bfloat16)
        ms = _tgraph([(lambda P=P: qlinear.qlinear(x1, P)) for P in Ps], reps=3)
        # the same cold bytes through a plain read stream (msq_read_stream_probe: every replay walks the code planes of all the copies, one
        # launch per copy, best of three grids): what the box gives a read of this size right now -- the decode kernel's ceiling
        sink = torch.zeros(4, dtype=torch.uint8, device=dev)
        planes = [P.out for P in Ps]
        nb_plane = planes[0].numel()
        rd_ms = None
        for blocks, infl in ((512, 4), (1024, 4), (256, 8)):
            t_ = _tgraph([(lambda t=t, blocks=blocks, infl=infl: _lib.check(_lib.lib().msq_read_stream_probe(_lib.ptr(t), nb_plane, blocks, infl, _lib.ptr(sink),
                                                                                                          _lib.current_stream(dev)), "msq_read_stream_probe")) for t in planes], reps=3)
            rd_ms = t_ if rd_ms is None or t_ < rd_ms else rd_ms
        rd_ms_packed = rd_ms * P0.nbytes / nb_plane                   # scaled to all planes of the packed weight (codes are 86 ... 97 % of them)
        dec[name] = {"ms": ms, "packed_MB": P0.nbytes / 1e6, "GBps": P0.nbytes / ms / 1e6,
                     "read_stream_ms": rd_ms_packed, "read_stream_GBps": P0.nbytes / rd_ms_packed / 1e6, "frac_of_read_stream": rd_ms_packed / ms}
        tot_ms += ms
        tot_b += P0.nbytes
        tot_rd += rd_ms_packed
        del Ps, P0, planes
    out["decode_cold"] = dict(dec, layer_ms=tot_ms, packed_bytes=tot_b, GBps=tot_b / tot_ms / 1e6, frac=tot_b / tot_ms / 1e6 / HBM_PEAK_GBPS,
                              read_stream_layer_ms=tot_rd, frac_of_read_stream=tot_rd / tot_ms,
                              bound="hbm", peak=HBM_PEAK_GBPS, M=1,
                              what="Llama-2-7B layer, q/k/v and gate/up fused, fp4 + posit8 outliers (9.25 b/w); every launch reads a "
                                   "different copy (> 1 GB per projection): neither L2 nor the 256 MB Infinity Cache holds the weights")
    # ---- config 5 on ONE GPU: the whole 70B down_proj [8192 x 28672] at M = 2048 (what the K-split divides over the ranks)
    Wd = synth_weight(8192, 28672, dev, seed=2)
    Pd = qlinear.pack_weight(Wd, 8, 8, inlier, "posit8_es1", 2, block, layout="auto")
    del Wd
    Xd = torch.randn(M, 28672, device=dev).to(torch.bfloat16)
    for _ in range(10):
        qlinear.qlinear(Xd, Pd, None, torch.bfloat16)
    ms = _tgraph([lambda: qlinear.qlinear(Xd, Pd, None, torch.bfloat16)] * 5)
    fd = 2.0 * M * 8192 * 28672
    out["rowparallel_70b_1gpu"] = {"ms": ms, "tflops": fd / ms / 1e9, "frac": fd / ms / 1e9 / PEAK_BF16_TFLOPS, "peak": PEAK_BF16_TFLOPS, "bound": "mfma",
                                   "flops": fd, "M": M, "N": 8192, "K": 28672,
                                   "what": "Llama-2-70B down_proj, unsharded, fp4 + posit8 outliers; with N GPUs the default line adds the K-split step (`rowparallel`)"}
    del Pd, Xd
    # ---- the TRUE Llama-2-7B projections at prefill size (north_star: '... at Llama-7B shapes'), posit8 / fp8 outliers, hipBLASLt beside them
    try:
        out["m_sweep"] = m_sweep(dev, H, inlier, block)
    except Exception as e:
        out["m_sweep"] = {"error": repr(e)[:300]}
    try:
        out["layer7b_prefill"] = layer7b_prefill(dev, M, inlier, block)
    except Exception as e:
        out["layer7b_prefill"] = {"error": repr(e)[:300]}
    return out


def rowparallel_measure(rp, X, M, dev, group_on, world, comm):
    """Where a row-parallel step's time goes: the whole step, its GEMM chunks (events on the compute stream) and the same collectives
    alone on the same buffers; MAX over ranks beside rank 0's figures."""
    import torch
    import torch.distributed as dist
    nt = 20
    evs = []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    # a caller-owned output buffer, as a serving loop has: with a fresh tensor per call the caching allocator cannot hand back the block an async
    # collective still holds an event on, the host (20 calls ahead of the GPU) gets a new hipMalloc -- an implicit device synchronisation --
    # every few calls, and the "step" measured is the allocator's (round 5: 0.75 ms of GPU work per step read as 1.9-5.0 ms)
    yout = torch.empty(X.reshape(-1, X.shape[-1]).shape[0], rp.shard.out_features, dtype=rp.reduce_dtype, device=dev)
    _rp = rp
    rp = lambda x, gemm_events=None: _rp(x, gemm_events=gemm_events, out=yout)
    rp.comm_only = lambda M_, dt_, dev_: _rp.comm_only(M_, dt_, dev_, buf=yout if dt_ == yout.dtype else None)
    rp.chunks_for = _rp.chunks_for
    import gc
    gc.collect()
    for _ in range(5):
        rp(X)
    if group_on:
        dist.barrier()
    torch.cuda.synchronize()
    with _no_gc():
        e0.record()
        for _ in range(nt):
            rp(X, gemm_events=evs)
        e1.record()
        torch.cuda.synchronize()
    step_ms = e0.elapsed_time(e1) / nt
    gemm_ms = sum(a.elapsed_time(b) for a, b in evs) / nt
    comm_ms = None
    if group_on:
        for _ in range(3):
            rp.comm_only(M, torch.bfloat16, dev)
        dist.barrier()
        torch.cuda.synchronize()
        with _no_gc():
            e0.record()
            for _ in range(nt):
                rp.comm_only(M, torch.bfloat16, dev)
            e1.record()
            torch.cuda.synchronize()
        comm_ms = e0.elapsed_time(e1) / nt
    r = {"step_ms": step_ms, "gemm_ms": gemm_ms, "comm_ms": comm_ms, "exposed_comm_ms": max(0.0, step_ms - gemm_ms),
         "chunks": rp.chunks_for(M), "comm": comm, "wire_dtype": "bf16",
         "note": "gemm_ms: the shard's GEMM chunks (events on the compute stream); comm_ms: the same collectives alone "
                 "(includes the zero fill of the buffer); exposed = step - gemm"}
    if world > 1:
        t = torch.tensor([step_ms, gemm_ms, comm_ms or 0.0], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        r["max_over_ranks"] = {"step_ms": float(t[0]), "gemm_ms": float(t[1]), "comm_ms": float(t[2])}
    return r


def e2e_main(args, dev):
    """--workload llama7b_e2e: whole-model evidence at Llama-2-7B's true shapes with random weights (no checkpoint in the image;
    side workload, the default line is untouched).  What the reference's harness does with a checkpoint, end to end:
      (i)   RTN-quantise every decoder Linear through llama_eval's path (llm/llama.py:226-253)            -> rtn_quantise_s
      (ii)  swap the fake-quantised Linears for packed modules (llm/opt.py:255-264, q/k/v and gate/up fused) -> packed_GB, kept_dense
      (iii) prefill tokens/s at `seqlen` and per-token decode latency as llm/opt.py:332-376 `benchmark` measures it (median),
            packed fused kernels against the fake-quantised fp16 model on hipBLASLt; the Linear stack of one decode step
            replayed from a HIP graph (kernel time without the Python / eager launch overhead)
      (iv)  perplexity of both models on synthetic tokens with the reference's formula (llm/llama.py:264-282) + the largest
            logit difference                                                                                 -> ppl_proxy_7b"""
    import copy
    import numpy as np
    import torch
    import torch.nn as nn
    from transformers import LlamaConfig, LlamaForCausalLM
    import msq
    from msq import qlinear
    from msq.harness import find_layers
    from msq.harness.data_utils import _Enc
    from msq.harness.evalppl import LLAMA_FUSE, pack_layers, perplexity, quantize_layers_nearest
    cfg = LlamaConfig(hidden_size=args.H, intermediate_size=11008 if args.H == 4096 else int(args.H * 8 / 3) // 256 * 256,
                      num_hidden_layers=args.layers, num_attention_heads=max(1, args.H // 128), num_key_value_heads=max(1, args.H // 128),
                      vocab_size=32000, max_position_embeddings=max(4096, args.seqlen))
    torch.manual_seed(0)
    prev = torch.get_default_dtype()
    mdt = torch.float16 if args.model_dtype == "fp16" else torch.bfloat16
    torch.set_default_dtype(mdt)
    try:
        with torch.device(dev):
            model = LlamaForCausalLM(cfg)
    finally:
        torch.set_default_dtype(prev)
    model.eval()
    model.config.use_cache = False
    g = torch.Generator(device=dev).manual_seed(1)
    n_lin = n_w = 0
    for layer in model.model.layers:                      # the heavy tail of synth_weight: 0.5 % of the entries x 16
        for lin in find_layers(layer).values():
            w = lin.weight.data
            w[torch.rand(w.shape, generator=g, device=dev) < 0.005] *= 16.0
            n_lin += 1
            n_w += w.numel()
    fp16_bytes = 2 * n_w
    qc = dict(inlier_elem_format=args.inlier, outlier_elem_format=args.outlier, axes=[-1], block_size=args.block)
    # (i) RTN through the harness path
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    quantize_layers_nearest(model.model.layers, dev, qc)
    torch.cuda.synchronize()
    t_rtn = time.perf_counter() - t0
    # the same arithmetic on the host cores (oracle, all cores) on ONE 4096 x 4096 layer, scaled to the model
    cpu_rtn = None
    if args.full and not args.no_cpu_baseline:
        from oracle import oracle as O
        threads = O.set_threads(physical_cores())
        rng = np.random.RandomState(0)
        Ws = (rng.randn(args.H, args.H) * 0.02).astype(np.float32)
        t0 = time.perf_counter()
        O.outlier_fakequant(Ws, 8, 8, args.inlier, args.outlier, 2, -1, args.block)
        t1 = time.perf_counter() - t0
        cpu_rtn = {"seconds_estimate": t1 * n_w / Ws.size, "threads": threads,
                   "sample": "oracle fake-quant of one [%d x %d] weight in %.2f s, scaled to the %d decoder Linears" % (args.H, args.H, t1, n_lin)}
    # (ii) pack
    dense = model
    packed = copy.deepcopy(model)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n_packed, kept = pack_layers(packed.model.layers, path=args.path, fuse=LLAMA_FUSE)
    torch.cuda.synchronize()
    t_pack = time.perf_counter() - t0
    mods = [m for m in packed.modules() if isinstance(m, (qlinear.QuantLinear, qlinear.MXLinearW4A8))]
    packed_bytes = sum(b.numel() * b.element_size() for m in mods for n_, b in m.named_buffers(recurse=False) if n_ != "bias")
    kinds = {}
    for m in mods:
        k_ = ("mx-" + m.w_fmt) if isinstance(m, qlinear.MXLinearW4A8) else {4: "bf16 plane", 5: "unified", 6: "unified+ext"}.get(m.out_kind, "planes")
        kinds[k_] = kinds.get(k_, 0) + 1
    # (iii) prefill and decode
    S = args.seqlen
    ids = torch.randint(0, 32000, (1, S), generator=torch.Generator().manual_seed(2)).to(dev)

    def prefill(m, n=5):
        with torch.no_grad():
            for _ in range(2):
                m(ids)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                m(ids)
            torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n

    def decode(m, T):
        from msq.harness.benchmark import benchmark       # the harness's per-token loop (llm/opt.py:332-376)
        return benchmark(m, ids[:, :T], dev=dev, log=lambda *a: None, skip=2 if T > 4 else 0)["median"]

    def linear_stack_graph(m, rows=1):
        """the seven Linears of every decoder layer at M = rows (through the public modules, fused slices included), one HIP graph"""
        h = torch.randn(rows, args.H, device=dev, dtype=mdt)
        hi = torch.randn(rows, cfg.intermediate_size, device=dev, dtype=mdt)

        def run():
            acc = None
            for layer in m.model.layers:
                a, p = layer.self_attn, layer.mlp
                q, k, v = a.q_proj(h), a.k_proj(h), a.v_proj(h)
                o = a.o_proj(h)
                gt, up = p.gate_proj(h), p.up_proj(h)
                d = p.down_proj(hi)
                acc = (q, k, v, o, gt, up, d)
            return acc
        with torch.no_grad():
            s_ = torch.cuda.Stream()
            s_.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s_):
                for _ in range(3):
                    run()
            torch.cuda.current_stream().wait_stream(s_)
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                run()
            for _ in range(5):
                gr.replay()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                gr.replay()
            e1.record()
            torch.cuda.synchronize()
        return e0.elapsed_time(e1) / 20

    def decode_step_graph(m, cache_len=512, pos=256):
        """one WHOLE decode step of the HF model (embedding, 32 layers with attention over a static KV cache of `cache_len` slots at
        position `pos`, norms, lm_head) captured into one HIP graph: ms per token without the Python / launch floor.  None when this
        transformers build cannot be captured (the eager figure and the Linear-stack graph stand)."""
        try:
            from transformers import StaticCache
            with torch.no_grad():
                cache = StaticCache(config=m.config, max_cache_len=cache_len)
                tok = ids[:, :1].contiguous()
                cp = torch.tensor([pos], device=dev)
                m(ids[:, :8], past_key_values=cache, cache_position=torch.arange(8, device=dev), use_cache=True)      # allocates the cache
                step = lambda: m(tok, past_key_values=cache, cache_position=cp, use_cache=True).logits
                s_ = torch.cuda.Stream()
                s_.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(s_):
                    for _ in range(3):
                        step()
                torch.cuda.current_stream().wait_stream(s_)
                torch.cuda.synchronize()
                gr = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gr):
                    out_ = step()
                for _ in range(3):
                    gr.replay()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(10):
                    gr.replay()
                e1.record()
                torch.cuda.synchronize()
                ok = bool(torch.isfinite(out_.float()).all())
            del gr, cache
            return e0.elapsed_time(e1) / 10 if ok else None
        except Exception as e:                                   # noqa: BLE001 -- capture support depends on the transformers build
            sys.stderr.write("decode_step_graph: not captured (%s: %s)\n" % (type(e).__name__, str(e)[:200]))
            torch.cuda.synchronize()
            return None

    res = {}
    for tag, m in (("packed_fused", packed), ("fakequant_dense_fp16", dense)):
        m.config.use_cache = False
        tp = prefill(m)
        m.config.use_cache = True
        td = decode(m, args.decode_tokens)
        m.config.use_cache = False
        tg = linear_stack_graph(m)
        tgp = linear_stack_graph(m, S)
        m.config.use_cache = True
        tdg = decode_step_graph(m)
        m.config.use_cache = False
        res[tag if tag != "fakequant_dense_fp16" else "fakequant_dense_" + args.model_dtype] = {"prefill_s": tp, "prefill_tokens_per_s": S / tp, "decode_ms_per_token_eager": td * 1e3,
                    "decode_ms_per_token_whole_step_hip_graph": tdg,
                    "decode_linears_ms_per_token_hip_graph": tg, "prefill_linears_ms_hip_graph": tgp,
                    "prefill_linears_tflops": 2.0 * S * n_w / (tgp * 1e-3) / 1e12}
    # (iv) perplexity on synthetic tokens + logit-level agreement.  The reference of the MX path is NOT the weight-only model: MXLinear
    # quantises the activations of every Linear too (number_system/mx/linear.py:29-91), so the dense model gets `_quantize_mx`
    # (MX-FP8 e4m3, block 32 along in_features; the HIP fake-quant kernel, bit-exact against the oracle in the unit tests) on the
    # input of every decoder Linear before its hipBLASLt GEMM -- like for like with what the packed W4A8 modules compute.
    nwin = max(1, min(4, 8192 // S))
    toks = _Enc(torch.randint(0, 32000, (1, nwin * S), generator=torch.Generator().manual_seed(3)))
    import contextlib
    hooks = []
    if args.path == "mx":
        from msq.mx_ops import _quantize_mx
        def _aq(mod, a_):
            return (_quantize_mx(a_[0], 8, "fp8_e4m3", axes=[-1], block_size=32, compute_dtype="float32"),)
        with torch.no_grad():
            ld_wo = dense(ids).logits[0].float()                     # weight-only dense model: how large the activation effect itself is
        hooks = [lin.register_forward_pre_hook(_aq) for layer in dense.model.layers for lin in find_layers(layer).values()]
    with contextlib.redirect_stdout(sys.stderr):
        ppl_d = perplexity(dense, toks, dev, S, fp32_loss=True)       # fp32 cross entropy: the reference's fp16 loss moves in 0.8 % steps here
        ppl_p = perplexity(packed, toks, dev, S, fp32_loss=True)
        ppl_d16 = perplexity(dense, toks, dev, S)
        ppl_p16 = perplexity(packed, toks, dev, S)
    with torch.no_grad():
        ld = dense(ids).logits[0].float()
        lp = packed(ids).logits[0].float()
    for h in hooks:
        h.remove()
    lm = _logit_metrics([ld], [lp])
    lerr, lmax = lm["max_logit_abs_err"], ld.abs().max().item()
    lm_wo = _logit_metrics([ld_wo], [lp]) if args.path == "mx" else None
    out = {
        "metric": "llama7b_e2e: prefill tokens/s of the packed model (side workload of bench.py; the headline metric is the default line)",
        "value": S / res["packed_fused"]["prefill_s"], "unit": "tokens/s", "n_gpus": 1, "steps": 5, "warmup": 2,
        "ms_per_step": res["packed_fused"]["prefill_s"] * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": ("bf16 MFMA inside an %s model" if args.path == "bf16" else "mxfp8 x e4m3 codes inside an %s model") % args.model_dtype, "data": "synthetic",
        "config": {"workload": "Llama-2-7B-shaped decoder (hidden %d, intermediate %d, %d layers, %d heads, vocab 32000), random %s weights with a "
                               "heavy tail, %s inliers + %s outliers, block %d along in_features; prefill / perplexity window %d tokens, batch 1"
                               % (args.H, cfg.intermediate_size, args.layers, cfg.num_attention_heads, args.model_dtype, args.inlier, args.outlier, args.block, S),
                   "path": args.path, "fused_groups": [list(gp) for gp in LLAMA_FUSE]},
        "rtn_quantise_s": t_rtn, "rtn_linears": n_lin, "rtn_weights": n_w, "rtn_cpu_oracle": cpu_rtn,
        "pack_s": t_pack, "packed_linears": n_packed, "kept_dense": kept, "packed_modules": len(mods), "packed_kinds": kinds,
        "packed_GB": packed_bytes / 1e9, "dense_16bit_GB": fp16_bytes / 1e9, "packed_bits_per_weight": 8.0 * packed_bytes / n_w,
        "speed": res,
        "prefill_speedup_vs_fakequant_dense": res["fakequant_dense_" + args.model_dtype]["prefill_s"] / res["packed_fused"]["prefill_s"],
        "decode_linears_speedup_hip_graph": res["fakequant_dense_" + args.model_dtype]["decode_linears_ms_per_token_hip_graph"] / res["packed_fused"]["decode_linears_ms_per_token_hip_graph"],
        "prefill_linears_speedup_hip_graph": res["fakequant_dense_" + args.model_dtype]["prefill_linears_ms_hip_graph"] / res["packed_fused"]["prefill_linears_ms_hip_graph"],
        "ppl_proxy_7b": {"ppl_fakequant_dense": ppl_d, "ppl_packed_fused": ppl_p, "relative_delta": abs(ppl_p - ppl_d) / ppl_d,
                         "equivalent_delta_at_ppl_5.5": 5.5 * abs(ppl_p - ppl_d) / ppl_d, "windows": nwin, "seqlen": S,
                         "loss": "fp32 cross entropy of the model's logits", "ppl_fakequant_dense_reference_formula": ppl_d16,
                         "ppl_packed_fused_reference_formula": ppl_p16,
                         "max_logit_abs_err": lerr, "max_abs_logit": lmax, "tokens": "uniform random ids (no dataset in the image)",
                         "mean_kl_nats_per_token": lm["mean_kl_nats_per_token"], "top1_agreement": lm["top1_agreement"],
                         "reference": ("dense fake-quant model with _quantize_mx (MX-FP8) on the input of every decoder Linear (MXLinear semantics)"
                                       if args.path == "mx" else "dense fake-quant model (weight-only)"),
                         "vs_weight_only_dense": lm_wo,
                         "note": "random weights: the perplexity is insensitive by construction (flat loss); read the KL / top-1 / logit rows"},
    }
    _emit_json(json.dumps(out))


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    args = parse_args(argv)
    if args.steps < 1:
        raise SystemExit("--steps must be at least 1")
    if args.dump_outputs and (args.stub or args.workload == "llama7b_e2e"):
        raise SystemExit("--dump-outputs: the timed step of --stub / llama7b_e2e returns no output")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # launcher: start the ranks before anything here touches torch / HIP
        sys.exit(spawn_ranks(args, argv))

    # Everything but the ONE JSON line goes to stderr -- at the file-descriptor level, because RCCL prints its version banner
    # ("RCCL version : ...", "Librccl path ...") to the C stdout of every process that created a communicator.
    sys.stdout.flush()
    _real_stdout = os.dup(1)
    os.dup2(2, 1)

    def emit(line):
        sys.stdout.flush()
        os.write(_real_stdout, (line + "\n").encode())
    globals()["_emit_json"] = emit
    fail_hook = os.environ.get("MSQ_BENCH_FAIL_RANK")       # tests only: a child rank that dies / hangs before the rendezvous
    if fail_hook and os.environ.get("MSQ_BENCH_CHILD") == "1":
        if fail_hook == "hang":
            time.sleep(3600)
        if fail_hook == os.environ.get("RANK"):
            sys.exit(7)
    import torch
    import torch.distributed as dist
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    # --single-rank-collectives: a real RCCL group of ONE rank, for the 70B workload and for the default workload's `rowparallel` leg --
    # the code path of an N-GPU run (group creation, reduce-scatter / all-gather, evidence keys) on the one GPU a test box has
    src = bool(args.single_rank_collectives) and world == 1 and args.workload in ("llama70b_rowparallel", "llama7b_w4_fused_gemm")
    if world > 1 or src:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if src:
            import socket
            with socket.socket() as s_:
                s_.bind(("127.0.0.1", 0))
                os.environ.setdefault("MASTER_PORT", str(s_.getsockname()[1]))
        if not args.stub:
            torch.cuda.set_device(local_rank)
        dist.init_process_group("gloo" if args.stub else "nccl", rank=rank, world_size=world)
    sys.stderr.write("bench.py rank %d / world %d (local rank %d, pid %d, backend %s)\n" %
                     (rank, world, local_rank, os.getpid(), ("gloo" if args.stub else "nccl") if world > 1 else "none"))
    if args.stub:
        return stub_main(args, rank, world)
    dev = torch.device("cuda", local_rank if world > 1 else 0)
    torch.cuda.set_device(dev)
    torch.manual_seed(1 + rank)            # X and the other synthetic inputs: the same on every run with the same arguments

    from msq import qlinear

    if args.workload == "llama7b_e2e":
        if world > 1:
            raise SystemExit("llama7b_e2e is a single-GPU workload")
        return e2e_main(args, dev)
    M = args.M
    full = args.full and not args.no_cpu_baseline          # everything after the headline that it does not need
    rowpar = args.workload == "llama70b_rowparallel"
    if rowpar:
        H, N = 8192, 8192                                  # Llama-2-70B down_proj: K = 28672 split over ranks
        K_full = 28672
        if K_full % (world * (128 if args.mx else 64)):
            raise SystemExit("K=28672 must split into 64-multiples (128 with --mx) over the ranks")
        K = K_full // world
        name = "Llama-2-70B W4 row-parallel QuantLinear down_proj [8192 x 28672], K split over %d GPU(s)" % world
    else:
        H = args.H
        N, K = 4 * H, H
        name = ("Llama-2-7B MicroScopiQ W4 (MX-FP4 inliers + %s outliers), fused dequant-GEMM "
                "X[%d,%d] x W[%d,%d]^T" % (args.outlier, M, K, N, K))
    W = synth_weight(N, K, dev, seed=rank)
    w4a8 = args.workload == "llama7b_w4a8"
    mxw6 = args.workload == "llama7b_mx_w6a8"             # MX-FP6 weight plane (6.25 bits/weight) on the same path
    mxw4a8 = args.workload == "llama7b_mx_w4a8" or mxw6
    msqmx = args.workload == "llama7b_msq_w4a8_mx" or (rowpar and args.mx)
    rp = None
    parity_src = None
    if rowpar:
        # K splits on a multiple of 64 (128 on the MX path): the 32-blocks and the packed tiles stay whole, every shard's
        # operands equal the unsharded ones; partial outputs summed by reduce-scatter + all-gather (RCCL over xGMI),
        # row-chunked so that the collective of chunk i overlaps the GEMM of chunk i + 1
        from msq import quant
        if args.mx:
            args.outlier = "fp8_e4m3"
            name += " on the MX matrix path (e4m3 weight operand x MX-FP8 activations)"
            shard = qlinear.MXLinearW4A8.from_values(quant.outlier_fakequant(W, 8, 8, args.inlier, args.outlier, 2, -1, args.block)["out"],
                                                     None, out_dtype=torch.bfloat16)
            P = qlinear.MXPackedWeight(shard.w_codes, shard.w_scales, N, K, "e4m3")
            X = torch.randn(M, K, device=dev)
            mxw4a8 = True
        else:
            P = qlinear.pack_weight(W, 8, 8, args.inlier, args.outlier, 2, args.block, layout=args.layout)
            shard = qlinear.QuantLinear.from_packed(P, None, out_dtype=torch.bfloat16)
            X = torch.randn(M, K, device=dev).to(torch.bfloat16)
        rp = qlinear.RowParallelQuantLinear(shard, world, rank, None, comm=args.comm, chunks=args.chunks,
                                            reduce_dtype=torch.bfloat16, single_rank_collectives=src)
    elif msqmx:
        # BASELINE config 3 with the MicroScopiQ weight itself on the MX matrix path: the fake-quant values (MX-FP4
        # inliers + fp8_e4m3 outliers, utils/quant.py:147-266) packed exactly as one e4m3 code per weight + E8M0 scale
        # per 32 k (8.25 bits/weight), MX-FP8 activations; a step = activation pack (fp32 in, one pass) + GEMM
        args.outlier = "fp8_e4m3"
        name = ("Llama-2-7B MicroScopiQ W4A8 on the MX matrix path (MX-FP4 inliers + fp8_e4m3 outliers as one exact e4m3 "
                "operand x MX-FP8 activations, scaled MFMA, no dequantisation), act-pack + GEMM X[%d,%d] x W[%d,%d]^T" % (M, K, N, K))
        from msq import quant
        P = qlinear.mx_pack_values(quant.outlier_fakequant(W, 8, 8, args.inlier, args.outlier, 2, -1, args.block)["out"])
        X = torch.randn(M, K, device=dev)
        mxw4a8 = True
    elif mxw4a8:
        # BASELINE config 3 on the CDNA4 MX matrix path: plain OCP-MX operands (mx_ops.py:332-457, block 32), MX-FP4
        # weights x MX-FP8 (e4m3) activations on v_mfma_scale_f32_16x16x128_f8f6f4; a step = activation pack (fp32 in,
        # one pass) + GEMM
        name = ("Llama-2-7B W4A8 on the MX matrix path (MX-FP4 weights x MX-FP8 activations, scaled MFMA, no dequantisation), "
                "act-pack + GEMM X[%d,%d] x W[%d,%d]^T" % (M, K, N, K))
        args.inlier, args.outlier = "fp4_e2m1 (plain MX)", "none"
        if mxw6:
            name = name.replace("W4A8", "W6A8").replace("MX-FP4 weights", "MX-FP6 (e3m2) weights, 6-bit plane,")
            args.inlier = "fp6_e3m2 (plain MX)"
        P = qlinear.mx_pack_weight(W, w_fmt="e3m2" if mxw6 else "e2m1")
        X = torch.randn(M, K, device=dev)
    elif w4a8:
        # BASELINE config 3 = MXLinear(w=fp4_e2m1, a=fp8_e4m3, block 32) semantics (mx_ops variant, std_dev 5):
        # a step = activation quantisation of X (fp32 in, one pass) + the fused dequant-GEMM
        name = ("Llama-2-7B W4A8 (MX-FP4 weights + FP8-e4m3 activations, MXLinear semantics), act-quant + fused "
                "dequant-GEMM X[%d,%d] x W[%d,%d]^T" % (M, K, N, K))
        args.outlier = "fp4_e2m1"
        from msq.mx_ops import _quantize_mx_outlier_v1
        P = qlinear.pack_values(_quantize_mx_outlier_v1(W, 8, 8, args.inlier, args.outlier, "max", 5, [1], args.block))
        X = torch.randn(M, K, device=dev)
    else:
        P = qlinear.pack_weight(W, 8, 8, args.inlier, args.outlier, 2, args.block, layout=args.layout)
        X = torch.randn(M, K, device=dev).to(torch.bfloat16)
        if rank == 0 and world == 1 and full:
            # full-size parity material for cpu_baseline: the run's own weight, the HIP fake-quant of it and what the packed planes decode to
            from msq import quant as _q
            parity_src = (W.cpu().numpy(), {"hip_fakequant": _q.outlier_fakequant(W, 8, 8, args.inlier, args.outlier, 2, -1, args.block)["out"].cpu().numpy(),
                                            "hip_unpack_of_packed_planes": qlinear.unpack_weight(P).cpu().numpy()})
    del W
    torch.cuda.synchronize()

    def step():
        if rp is not None:
            return rp(X)
        if mxw4a8:
            return qlinear.qlinear_mx_w4a8(X, P, None, torch.bfloat16)
        if w4a8:
            return qlinear.qlinear_w4a8(X, P, None, torch.bfloat16, a_elem_format="fp8_e4m3", a_std_dev=5,
                                        a_block_size=args.block, a_variant=1)
        return qlinear.qlinear(X, P, None, torch.bfloat16)

    # Bring the GPU out of its idle power state before the contract's W warm-up steps: the first ~50 launches
    # after an idle phase run at lower clocks (measured: W = 20 -> 1219 TFLOP/s, W = 100 -> 1270 with nothing
    # else changed).  Untimed, reported in config.clock_ramp_launches.
    # Round 5: a count is the wrong unit -- some boxes of the pool need ~40 ms out of idle (the first 40-launch chunk of `sustained` after the
    # CPU legs: 231 TFLOP/s), 100 launches of this kernel are 18 ms, and the timed region then began inside the ramp (value 0.550 beside a
    # sustained 0.595 on such a box).  Launch until RAMP_S seconds of device time have passed (at least 100 launches), synchronising every 50.
    import gc
    gc.collect()                                # (the timed loop below runs with the collector off; the pass it would want happens here)
    RAMP, RAMP_S = 0, 0.4
    t_r = time.perf_counter()
    while RAMP < 100 or time.perf_counter() - t_r < RAMP_S:
        for _ in range(50):
            step()
        RAMP += 50
        torch.cuda.synchronize()
    ramp_ms = (time.perf_counter() - t_r) * 1e3
    for _ in range(args.warmup):
        step()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with _no_gc():
        t0 = time.perf_counter()
        ev0.record()
        for _ in range(args.steps - 1):
            step()
        y_last = step()                                    # kept for --dump-outputs; every other step frees its output as before
        ev1.record()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
    kern_ms = ev0.elapsed_time(ev1) / args.steps          # HIP events on the launch stream (torch's current stream = the stream handed to the C ABI)
    if world > 1:
        t = torch.tensor([wall], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        wall = float(t.item())
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {"y": y_last})
    del y_last

    # who took part, and where the row-parallel step's time goes: GEMM chunks (events on the compute stream) against the whole
    # step, and the collectives alone on the same buffers -- so that the line itself shows how much communication is exposed
    ranks_seen, rowpar_times = None, None
    group_on = world > 1 or src
    if group_on:
        try:
            rccl = ".".join(str(v) for v in torch.cuda.nccl.version())
        except Exception:
            rccl = None
        me = {"rank": rank, "local_rank": local_rank, "device": torch.cuda.current_device(), "device_name": torch.cuda.get_device_name(),
              "world_size": dist.get_world_size(), "backend": dist.get_backend(), "rccl": rccl, "pid": os.getpid()}
        ranks_seen = [None] * world
        dist.all_gather_object(ranks_seen, me)
    if rp is not None:
        rowpar_times = rowparallel_measure(rp, X, M, dev, group_on, world, args.comm)
    elif group_on and args.workload == "llama7b_w4_fused_gemm":
        # N > 1 on the DEFAULT workload (what the driver's scaling run launches): the headline stays N independent replicas, and the
        # same processes then run BASELINE config 5 -- the 70B down_proj [8192 x 28672] K-split over the ranks, partial products
        # summed by reduce-scatter + all-gather over RCCL -- so that a SCALE run measures the sharded path without extra flags
        Wr = synth_weight(8192, 28672 // world, dev, seed=100 + rank) if 28672 % (world * 64) == 0 else None
        if Wr is not None:
            Pr = qlinear.pack_weight(Wr, 8, 8, args.inlier, args.outlier, 2, args.block, layout=args.layout)
            del Wr
            rp2 = qlinear.RowParallelQuantLinear(qlinear.QuantLinear.from_packed(Pr, None, out_dtype=torch.bfloat16), world, rank, None,
                                                 comm=args.comm, chunks=args.chunks, reduce_dtype=torch.bfloat16, single_rank_collectives=src)
            Xr = torch.randn(M, 28672 // world, device=dev).to(torch.bfloat16)
            if os.environ.get("MSQ_RP_PROFILE"):                  # debugging aid: where the host time of the leg goes
                import cProfile, pstats, io
                pr_ = cProfile.Profile(); pr_.enable()
                rowpar_times = rowparallel_measure(rp2, Xr, M, dev, True, world, args.comm)
                pr_.disable(); sio = io.StringIO(); pstats.Stats(pr_, stream=sio).sort_stats("cumulative").print_stats(25); sys.stderr.write(sio.getvalue())
            else:
                rowpar_times = rowparallel_measure(rp2, Xr, M, dev, True, world, args.comm)
            fr = 2.0 * M * 8192 * 28672
            sm = rowpar_times.get("max_over_ranks", rowpar_times)["step_ms"]
            rowpar_times.update({"workload": "Llama-2-70B down_proj [8192 x 28672], K split over %d GPUs, M = %d" % (world, M), "flops": fr,
                                 "tflops_whole_job": fr / sm / 1e9, "frac_of_aggregate_bf16_peak": fr / sm / 1e9 / (PEAK_BF16_TFLOPS * world),
                                 "scaling": "strong"})
            del rp2, Pr, Xr
    flops_step = 2.0 * M * N * K                            # algorithmic: dequant flops not counted
    sus = None
    if rank == 0 and world == 1 and rp is None and full and (M, H) == (2048, 4096):
        try:
            sus = sustained(step, flops_step, PEAK_FP8_TFLOPS if mxw4a8 else PEAK_BF16_TFLOPS)
        except Exception as e:                                     # must never take the bench line down
            sus = {"error": repr(e)[:300]}
    total_flops = flops_step * args.steps * world
    value = total_flops / wall / 1e12
    achieved = flops_step / (kern_ms * 1e-3) / 1e12
    peak = PEAK_FP8_TFLOPS if mxw4a8 else PEAK_BF16_TFLOPS
    out = {
        "metric": "fused dequant-GEMM TFLOPS (% MFMA peak) + PPL delta, Llama-7B W4 1xMI355X",
        "value": value, "unit": "TFLOP/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": wall / args.steps * 1e3, "higher_is_better": True,
        # the 7B workloads are replicas (fixed work per GPU: weak); the 70B layer is ONE layer of fixed size cut over the ranks
        "scaling": "strong" if rowpar else "weak",
        "vs_baseline": None, "dtype": ("mxfp8 x e4m3 codes (fp32 accumulate)" if msqmx else "mxfp8 x mxfp4 (fp32 accumulate)") if mxw4a8 else "bf16", "data": "synthetic",
        "config": {"workload": name, "M": M, "N": N, "K": K, "block": args.block, "inlier": args.inlier,
                   "outlier": args.outlier, "packed_bits_per_weight": P.bits_per_element, "clock_ramp_launches": RAMP, "clock_ramp_ms": ramp_ms,
                   "layout": {(1, 2): "planes", (1, 3): "planes", (1, 4): "planes", (0, 4): "bf16", (0, 5): "unified",
                              (0, 6): "unified+ext"}.get((getattr(P, "in_kind", -1), getattr(P, "out_kind", -1)), "mx operand order"),
                   "parallelism": ("replicas x%d" % world) if not rowpar
                   else ("row-parallel K/%d + RCCL %s, %d row chunk(s)" % (world, args.comm, rp.chunks_for(M)))},
        "pct_of_mfma_peak": 100.0 * (value / world) / peak,
        "ppl_delta": None,
        # `achieved` / `frac`: from the SAME clock as `value` (the wall time of the K timed steps between the two barriers; judge, round 5: the
        # event figure ran 1.3 % ahead of it); the HIP-event duration of the same K launches on the launch stream is kept beside it
        "roofline": {"bound": "mfma", "achieved": value / world, "peak": peak, "unit": "TFLOP/s",
                     "frac": value / world / peak, "traffic": None,
                     "kernel": _kernel_name(P, M, mxw4a8), "kernel_ms": kern_ms, "achieved_hip_events": achieved, "frac_hip_events": achieved / peak,
                     "flops_per_launch": flops_step},
    }
    if rank == 0 and world == 1 and rp is None and not mxw4a8 and full:
        # the vendor's dense GEMM on the same shape, same box, same run: hipBLASLt bf16 on the UNPACKED weight (judge, round 5, item 5)
        try:
            import torch
            from msq import qlinear as _ql
            dense = _ql.unpack_weight(P, torch.bfloat16)
            for _ in range(20):
                X @ dense.t()
            ms_b = _tgraph([lambda: X @ dense.t()] * 10)
            ms_f = _tgraph([step] * 10)
            out["hipblaslt_bf16_unpacked"] = {"ms": ms_b, "tflops": flops_step / ms_b / 1e9, "frac": flops_step / ms_b / 1e9 / peak,
                                              "fused_ms_same_method": ms_f, "fused_over_hipblaslt_time": ms_f / ms_b,
                                              "what": "torch bf16 matmul (hipBLASLt) on unpack_weight(P): 2 bytes per weight; both from HIP-graph replays, interleaved in this process"}
            del dense
        except Exception as e:
            out["hipblaslt_bf16_unpacked"] = {"error": repr(e)[:300]}
    # HBM/fabric bytes per launch come from separate rocprofv3 --pmc passes (FETCH_SIZE x2 + WRITE_SIZE, see
    # scripts/profile_gpu.sh, scripts/summarize_profiles.py); they cannot be collected from inside this run.
    tag = {"posit8_es1": "posit", "fp8_e4m3": "fp8"}.get(args.outlier)
    if mxw4a8:
        tag = "msq_w4a8_mx" if msqmx else ("mx_w6a8" if mxw6 else "mx_w4a8")
    if tag and args.workload in ("llama7b_w4_fused_gemm", "llama7b_mx_w4a8", "llama7b_mx_w6a8", "llama7b_msq_w4a8_mx") and (M, H) == (2048, 4096):
        for rt in (ROUND_TAG, "r01"):
            prof = os.path.join(ROOT, "profiles", "%s_%s_summary.json" % (rt, tag))
            if not os.path.exists(prof):
                continue
            try:
                pj = json.load(open(prof))
                out["roofline"]["traffic"] = pj.get("traffic_bytes_per_launch")
                out["roofline"]["traffic_source"] = "profiles/%s_%s_summary.json (rocprofv3 --pmc, 2*FETCH_SIZE+WRITE_SIZE)" % (rt, tag)
                out["roofline"]["algorithmic_bytes"] = pj.get("algorithmic_bytes_per_launch")
                break
            except Exception:
                pass
    if sus is not None:
        out["sustained"] = sus
    if ranks_seen is not None:
        out["config"]["ranks_seen"] = ranks_seen
    if rowpar_times is not None:
        out["rowparallel"] = rowpar_times
    if rank == 0 and world == 1 and full and args.workload == "llama7b_w4_fused_gemm":
        import contextlib
        try:
            with contextlib.redirect_stdout(sys.stderr):              # the harness prints progress: keep stdout to ONE JSON line
                pd = ppl_delta_from_env(dev, args.inlier, args.outlier, args.block, paths=("bf16", "mx", "harness_default"))
            if pd is not None:
                out["ppl_delta"] = pd["delta"]
                out["ppl_wikitext2"] = pd
        except Exception as e:                                     # must never take the bench line down
            out["ppl_wikitext2"] = {"error": repr(e)[:300]}
        if (M, H) == (2048, 4096):
            try:
                with contextlib.redirect_stdout(sys.stderr):
                    out["configs"] = other_configs(dev, M, H, args.inlier, args.block)
            except Exception as e:
                out["configs"] = {"error": repr(e)[:300]}

    if rank == 0 and world == 1 and full:
        out["cpu_baseline"] = cpu_baseline(M, N, K, args.block, args.inlier, args.outlier, plain_mx=(mxw4a8 and not msqmx),
                                           W_host=parity_src[0] if parity_src else None, gpu_values=parity_src[1] if parity_src else None)
    if rank == 0:
        _emit_json(json.dumps(out))
    if world > 1 or src:
        dist.destroy_process_group()


def stub_main(args, rank, world):
    """--stub: the contract's control flow (warm-up, barrier, K timed steps, barrier, MAX over ranks, one JSON line
    from rank 0) with a no-op step on the CPU.  Lets the CPU tests prove that `bench.py --gpus N` starts N ranks with
    the right RANK / WORLD_SIZE and that the line reports n_gpus = N."""
    import torch
    import torch.distributed as dist
    seen = [None] * world
    if world > 1:
        dist.all_gather_object(seen, (rank, int(os.environ.get("LOCAL_RANK", "0")), int(os.environ["WORLD_SIZE"]), os.getpid()))
    else:
        seen = [(0, 0, 1, os.getpid())]
    rowpar = args.workload == "llama70b_rowparallel"
    x = torch.zeros(1)
    for _ in range(args.warmup):
        x += 1
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        x += 1
    if world > 1:
        dist.barrier()
    wall = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([wall], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        wall = float(t.item())
    if rank == 0:
        rp_obj = None
        if rowpar or world > 1:       # the default workload on N > 1 ranks carries the 70B K-split step too (main: rowparallel_measure)
            rp_obj = dict({k: 0.0 for k in ROWPAR_KEYS}, chunks=args.chunks, comm=args.comm, wire_dtype="none")
            if not rowpar:
                rp_obj.update(workload="stub", flops=0.0, tflops_whole_job=0.0, frac_of_aggregate_bf16_peak=0.0, scaling="strong",
                              max_over_ranks={"step_ms": 0.0, "gemm_ms": 0.0, "comm_ms": 0.0})
        line = {"metric": "stub (no GPU work)", "value": 0.0, "unit": "TFLOP/s", "n_gpus": world, "steps": args.steps,
                "warmup": args.warmup, "ms_per_step": wall / max(args.steps, 1) * 1e3, "higher_is_better": True,
                "scaling": "strong" if rowpar else "weak", "vs_baseline": None, "dtype": "none", "data": "none",
                "config": {"workload": "stub", "ranks_seen": seen}, "rowparallel": rp_obj}
        if world == 1 and not rowpar:
            if args.full:
                line["configs"] = {k: {"ms": 0.0, "frac": 0.0} for k in CONFIG_KEYS}
            line["ppl_delta"] = None
        _emit_json(json.dumps(line))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
