"""SURVEY 8 row f3, the PACKED MX KV cache (msq.kvpacked, csrc/msq_kv_packed.hip).

Pack / unpack: the planes decode to the float32 `_quantize_mx` values bit for bit (oracle and package) at head_dim 32 .. 256, the V planes of an fp8 cache at
head_dim 128 are the bytes of mx_pack_act, a pack touches only its own token range, a planted Inf raises MSQ_STATUS_NAN.
Attention: float64 softmax attention over dequantize().double() -- the exact values the codes hold, so quantisation error is not in the
comparison -- is the reference.  The float32 output may be off by at most 4 x the error of torch's float32 math-backend SDPA on the same
dequantised tensors against the same reference (floor 2^-20 max|ref|: the factor covers another summation order, the split and combine and an
exp2-based exponential; a dropped group, a wrong scale byte or a wrong nibble is thousands of times larger); the half output is the float32
output rounded; a planted dominant token exercises every rescale path of the online softmax; a left-padding bias; repeatability.
Cache: the tensors PackedMXKVCache hands back at every step of prefill 70 + 30 tokens, and the logits of a seeded 2-layer Llama decoded over
the codes against sdpa over the same cache type, bounded by the sdpa / eager gap on that cache.  Every test prints its figures (pytest -s)."""
import math

import numpy as np
import pytest
import torch

from gpu_common import dev, eq, planted

pytestmark = pytest.mark.gpu

FMTS = ("fp8_e4m3", "fp4_e2m1")
DTYPES = (torch.float16, torch.bfloat16)
B, HKV = 2, 2
_cache = {}


def _rand(shape, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(dtype)


def _planes(kp, Bv, H, S_cap, D, fmt, fill=0):
    return {n: torch.full(s, fill, dtype=torch.uint8, device=dev()) for n, s in kp.plane_shapes(Bv, H, S_cap, D, fmt).items()}


# ---------------------------------------------------------------------------------------------------------------------
# pack / unpack
# ---------------------------------------------------------------------------------------------------------------------
def _pack_inputs(T, D, along_tokens):
    """float32 inputs [B, HKV, T, D]: randn x per-channel scales over 2^-8 .. 2^8, and gpu_common.planted blocks laid along the quantised axis
    (maxima a few ulps under a power of two: the Python-path exponent cases)"""
    key = ("in", T, D, along_tokens)
    if key not in _cache:
        g = torch.Generator().manual_seed(7 + T + D)
        x = torch.randn(B, HKV, T, D, generator=g) * torch.exp2(torch.rand(D, generator=g) * 16 - 8)
        if along_tokens:
            p = torch.from_numpy(planted(B * HKV * D, T, 11 + D)).reshape(B, HKV, D, T).transpose(2, 3).contiguous()
        else:
            p = torch.from_numpy(planted(B * HKV * T, D, 13 + D)).reshape(B, HKV, T, D)
        _cache[key] = (x, p)
    return _cache[key]


@pytest.mark.parametrize("along_tokens", [1, 0])
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("D", [32, 64, 96, 128, 160, 256])
def test_unpack_of_pack_is_quantize_mx_f32(msq, O, D, fmt, along_tokens):
    kp = msq.kvpacked
    T, S_cap = 64, 96
    axis = 2 if along_tokens else 3
    cn, sn = ("k_codes", "k_scales") if along_tokens else ("v_codes", "v_scales")
    rnd, pl = _pack_inputs(T, D, along_tokens)
    cases = [("randn f32", rnd), ("planted f32", pl)] + [("randn %s" % dt, rnd.to(dt)) for dt in DTYPES]
    for name, x in cases:
        P = _planes(kp, B, HKV, S_cap, D, fmt)
        kp.mx_pack(x.to(dev()), P[cn], P[sn], 32, fmt, along_tokens, check_status=True)
        got = kp.mx_unpack(P[cn], P[sn], 32, T, D, torch.float32, fmt, along_tokens).cpu().numpy()
        want = O.quantize_mx(x.float().numpy(), 8, fmt, axis=axis, block_size=32)
        assert eq(got, want), (name, "oracle", int((got != want).sum()))
        pkg = msq.mx_ops._quantize_mx(x.float().to(dev()), 8, fmt, axes=[axis], block_size=32).cpu().numpy()
        assert eq(got, pkg), (name, "package")
        for dt in DTYPES:                                        # an unpack rounds once to the cache dtype
            h = kp.mx_unpack(P[cn], P[sn], 32, T, D, dt, fmt, along_tokens)
            assert eq(h.float().cpu().numpy(), torch.from_numpy(want).to(dt).float().numpy()), (name, dt)


def test_v_planes_of_fp8_are_mx_pack_act_bytes(msq):
    kp = msq.kvpacked
    T, D = 64, 128
    rnd, pl = _pack_inputs(T, D, 0)
    for x in (rnd, pl, rnd.to(torch.float16), rnd.to(torch.bfloat16)):
        P = _planes(kp, B, HKV, T, D, "fp8_e4m3")
        kp.mx_pack(x.to(dev()), P["v_codes"], P["v_scales"], 0, "fp8_e4m3", False)
        codes, scales = msq.qlinear.mx_pack_act(x.to(dev()).reshape(B * HKV * T, D))
        assert torch.equal(P["v_codes"].reshape(-1, D), codes) and torch.equal(P["v_scales"].reshape(-1, D // 32), scales)


# head_dim 64 keeps the ids it had before the other head dims were added
@pytest.mark.parametrize("fmt,D", [pytest.param(f, d, id=f if d == 64 else "%s-D%d" % (f, d)) for d in (64, 32, 96, 256) for f in FMTS])
def test_pack_touches_only_its_token_range(msq, fmt, D):
    kp = msq.kvpacked
    S_cap, pos, T = 160, 64, 32
    x = _rand((B, HKV, T, D), 3, torch.bfloat16).to(dev())
    P = _planes(kp, B, HKV, S_cap, D, fmt, fill=0xA5)
    kp.mx_pack(x, P["k_codes"], P["k_scales"], pos, fmt, True)
    kp.mx_pack(x, P["v_codes"], P["v_scales"], pos, fmt, False)
    for n in ("k_codes", "v_codes", "v_scales"):
        keep = torch.cat([P[n][:, :, :pos], P[n][:, :, pos + T:]], dim=2)
        assert bool((keep == 0xA5).all()), n
    keep = torch.cat([P["k_scales"][:, :, :pos // 32], P["k_scales"][:, :, (pos + T) // 32:]], dim=2)
    assert bool((keep == 0xA5).all())
    Q = _planes(kp, B, HKV, T, D, fmt)                           # and the range itself holds what a pack at 0 of a fresh plane holds
    kp.mx_pack(x, Q["k_codes"], Q["k_scales"], 0, fmt, True)
    kp.mx_pack(x, Q["v_codes"], Q["v_scales"], 0, fmt, False)
    for n in ("k_codes", "v_codes", "v_scales"):
        assert torch.equal(P[n][:, :, pos:pos + T], Q[n])
    assert torch.equal(P["k_scales"][:, :, pos // 32:(pos + T) // 32], Q["k_scales"])


@pytest.mark.parametrize("along_tokens", [1, 0])
def test_planted_inf_raises_status_nan(msq, along_tokens):
    kp = msq.kvpacked
    x = _rand((B, HKV, 32, 64), 5, torch.float16)
    x[1, 0, 7, 33] = float("inf")
    P = _planes(kp, B, HKV, 32, 64, "fp8_e4m3")
    cn, sn = ("k_codes", "k_scales") if along_tokens else ("v_codes", "v_scales")
    with pytest.raises(msq._lib.MsqError, match="MSQ_STATUS_NAN"):
        kp.mx_pack(x.to(dev()), P[cn], P[sn], 0, "fp8_e4m3", along_tokens, check_status=True)
    kp.mx_pack(x[:1].to(dev()), P[cn][:1], P[sn][:1], 0, "fp8_e4m3", along_tokens, check_status=True)   # sequence 0 is finite


# ---------------------------------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------------------------------
def _filled(kp, K, V, fmt, gap=32):
    pk = kp.PackedKV(K.shape[0], K.shape[1], K.shape[3], K.dtype, fmt, gap=gap, capacity=32, device=dev())
    pk.append(K, V)
    return pk


def _reference(pk, q, bias, scaling):
    """float64 softmax attention over the values the cache holds; a row whose every position is masked gives zeros.
    Returns (ref [B, Hq, D] float64, the logits [B, Hq, S] float64, rows that are fully masked [B])"""
    kd, vd = pk.dequantize()
    G = q.shape[1] // kd.shape[1]
    k64 = kd.double().repeat_interleave(G, dim=1)
    v64 = vd.double().repeat_interleave(G, dim=1)
    logits = torch.einsum("bhd,bhsd->bhs", q.double(), k64) * scaling
    if bias is not None:
        logits = logits + bias.double()[:, None, :]
    dead = torch.isinf(logits).all(dim=2).all(dim=1)
    w = torch.softmax(logits, dim=2)
    w = torch.where(torch.isnan(w), torch.zeros_like(w), w)
    return torch.einsum("bhs,bhsd->bhd", w, v64), logits, dead


def _torch_f32(pk, q, bias, scaling):
    """torch's float32 math-backend SDPA on the same dequantised tensors"""
    from torch.nn.attention import SDPBackend, sdpa_kernel
    kd, vd = pk.dequantize()
    G = q.shape[1] // kd.shape[1]
    k32, v32 = kd.float().repeat_interleave(G, dim=1), vd.float().repeat_interleave(G, dim=1)
    mask = None if bias is None else bias[:, None, None, :].float()
    with sdpa_kernel(SDPBackend.MATH):
        y = torch.nn.functional.scaled_dot_product_attention(q.float()[:, :, None, :], k32, v32, attn_mask=mask, scale=scaling)
    return y[:, :, 0, :]


def _check(pk, q, bias, tag):
    """the float32 bound and the half-output identity of one call; returns (err, err_torch)"""
    scaling = q.shape[2] ** -0.5
    ref, _, dead = _reference(pk, q, bias, scaling)
    out32 = pk.attend(q, bias, scaling, out_dtype=torch.float32)
    live = ~dead
    assert bool((out32[dead] == 0).all()), (tag, "a fully masked row must give zeros")
    th = _torch_f32(pk, q, bias, scaling)
    err = float((out32.double() - ref)[live].abs().max())
    err_t = float((th.double() - ref)[live].abs().max())
    floor = 2.0 ** -20 * float(ref[live].abs().max())
    print("%-60s err %.3e torch %.3e floor %.3e" % (tag, err, err_t, floor))
    assert err <= max(4 * err_t, floor), (tag, err, err_t, floor)
    outh = pk.attend(q, bias, scaling)
    assert outh.dtype == q.dtype and torch.equal(outh, out32.to(q.dtype)), (tag, "half output != rounded float32 output")
    return err, err_t


def _split_tokens(kp, Hq, D):
    return kp.attn_plan(B, Hq, HKV, D, 4096, 0)[1]


def _left_pad_bias(total):
    """sequence 1: the first 40 positions are -inf (left padding)"""
    bias = torch.zeros(B, total, dtype=torch.float32, device=dev())
    bias[1, :40] = float("-inf")
    return bias


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("Hq", [4, 16])
@pytest.mark.parametrize("D", [64, 128])
def test_attend_against_float64(msq, D, Hq, dtype, fmt):
    kp = msq.kvpacked
    st = _split_tokens(kp, Hq, D)
    assert st % 32 == 0 and kp.attn_plan(B, Hq, HKV, D, st + 32, 0)[0] == 2 and kp.attn_plan(B, Hq, HKV, D, 2 * st, 0)[0] == 2
    for S in (0, 32, 96, st + 32, 2 * st):                       # one group past a split boundary; an exact multiple of the split size
        for tail in (0, 1, 31):
            if S + tail == 0:
                continue
            total = S + tail
            K = _rand((B, HKV, total, D), 100 + total, dtype).to(dev())
            V = _rand((B, HKV, total, D), 200 + total, dtype).to(dev())
            q = _rand((B, Hq, D), 300 + total, dtype).to(dev())
            pk = _filled(kp, K, V, fmt)
            assert (pk.packed_len, pk.tail_len) == (S, tail)
            for bias in (None, _left_pad_bias(total)):
                _check(pk, q, bias, "D %d Hq %d %s %s S %d tail %d %s" % (D, Hq, str(dtype)[6:], fmt, S, tail, "bias" if bias is not None else "-"))


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("D,Hq", [(64, 16), (128, 4)])
def test_rescale_paths_with_a_dominant_token(msq, D, Hq, dtype, fmt):
    """one token whose logit exceeds all others by more than 30, in the first split, in the last split, in the tail"""
    kp = msq.kvpacked
    st = _split_tokens(kp, Hq, D)
    S, tail = st + 32, 31
    total = S + tail
    for where, t in (("first split", 5), ("last split", S - 3), ("tail", total - 1)):
        K = _rand((B, HKV, total, D), 400, dtype)
        V = _rand((B, HKV, total, D), 401, dtype)
        q = _rand((B, Hq, D), 402, dtype)
        sign = torch.where(_rand((D,), 403) >= 0, 1.0, -1.0)
        q = (q.float().abs() * sign).to(dtype)                   # every query head leans the same way ...
        K[:, :, t, :] = (8.0 * sign).to(dtype)                   # ... and one key points there
        pk = _filled(kp, K.to(dev()), V.to(dev()), fmt)
        q = q.to(dev())
        _, logits, _ = _reference(pk, q, None, D ** -0.5)
        others = torch.cat([logits[:, :, :t], logits[:, :, t + 1:]], dim=2)
        assert float((logits[:, :, t] - others.max(dim=2).values).min()) > 30, where
        _check(pk, q, None, "dominant token in the %s: D %d Hq %d %s %s" % (where, D, Hq, str(dtype)[6:], fmt))


@pytest.mark.parametrize("fmt", FMTS)
def test_repeatable_and_independent_of_the_batch(msq, fmt):
    kp = msq.kvpacked
    D, Hq = 128, 16
    st = _split_tokens(kp, Hq, D)
    total = 2 * st + 32 + 31
    K = _rand((B, HKV, total, D), 500, torch.float16).to(dev())
    V = _rand((B, HKV, total, D), 501, torch.float16).to(dev())
    q = _rand((B, Hq, D), 502, torch.float16).to(dev())
    bias = _left_pad_bias(total)
    pk = _filled(kp, K, V, fmt)
    first = pk.attend(q, bias, out_dtype=torch.float32)
    for _ in range(20):
        assert torch.equal(pk.attend(q, bias, out_dtype=torch.float32), first)
    one = _filled(kp, K[:1].contiguous(), V[:1].contiguous(), fmt)
    assert torch.equal(one.attend(q[:1].contiguous(), bias[:1].contiguous(), out_dtype=torch.float32)[0], first[0])


# ---------------------------------------------------------------------------------------------------------------------
# cache
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_cache_returns_quantised_prefix_and_exact_tail(msq, dtype, fmt):
    kp = msq.kvpacked
    D, gap, n0, steps = 64, 32, 70, 30
    K = _rand((B, HKV, n0 + steps, D), 600, dtype).to(dev())
    V = _rand((B, HKV, n0 + steps, D), 601, dtype).to(dev())
    qf = lambda t, ax: msq.mx_ops._quantize_mx(t.float(), 8, fmt, axes=[ax], block_size=32).to(dtype)
    cache = kp.PackedMXKVCache(1, fmt, gap=gap, capacity=64)

    def expect(n, P):
        return (torch.cat([qf(K[:, :, :P], 2), K[:, :, P:n]], dim=2), torch.cat([qf(V[:, :, :P], 3), V[:, :, P:n]], dim=2))

    k, v = cache.update(K[:, :, :n0], V[:, :, :n0], 0)
    ek, ev = expect(n0, 64)
    assert eq(k.float().cpu().numpy(), ek.float().cpu().numpy()) and eq(v.float().cpu().numpy(), ev.float().cpu().numpy())
    for i in range(steps):
        cached = n0 + i
        k, v = cache.update(K[:, :, cached:cached + 1], V[:, :, cached:cached + 1], 0)
        P = 96 if cached >= 96 else 64                           # the tail of 32 is packed when the 97th token arrives
        ek, ev = expect(cached + 1, P)
        pk = cache.layers[0].packed
        assert (pk.packed_len, pk.len, cache.get_seq_length()) == (P, cached + 1, cached + 1)
        assert k.dtype == dtype and tuple(k.shape) == (B, HKV, cached + 1, D)
        assert eq(k.float().cpu().numpy(), ek.float().cpu().numpy()), ("K", cached)
        assert eq(v.float().cpu().numpy(), ev.float().cpu().numpy()), ("V", cached)
    pk = cache.layers[0].packed
    assert pk.capacity == 128                                    # grown once, in whole groups: 64 -> 128
    bits = 8.25 if fmt == "fp8_e4m3" else 4.25
    assert pk.bits_per_element == bits
    assert pk.nbytes == int(2 * B * HKV * pk.capacity * D * bits / 8) + 2 * B * HKV * gap * D * 2


def test_model_logits_over_the_codes(msq):
    """A seeded 2-layer Llama (hidden 256, 4 heads, 2 kv heads, head_dim 64, bf16): 40 greedy steps from a 70-token prompt over a
    PackedMXKVCache.  The tokens are the greedy tokens of the sdpa run, fed to all three runs so that the per-step logits are comparable.
    Per step: max |logits(msq_packed_kv) - logits(sdpa)| <= 4 max |logits(eager) - logits(sdpa)| -- sdpa and eager are two existing
    implementations over identical dequantised tensors, so their gap is the spread that reassociation alone produces."""
    from transformers import LlamaConfig, LlamaForCausalLM
    kp = msq.kvpacked
    torch.manual_seed(0)
    cfg = LlamaConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2, head_dim=64,
                      vocab_size=256, max_position_embeddings=256)
    cfg._attn_implementation = "sdpa"
    model = LlamaForCausalLM(cfg).to(torch.bfloat16).to(dev()).eval()
    prompt = torch.randint(0, 256, (1, 70), generator=torch.Generator().manual_seed(1)).to(dev())

    def run(impl, tokens=None):
        cache = kp.PackedMXKVCache(2, "fp8_e4m3", gap=32)
        if impl == kp.ATTENTION_NAME:
            kp.use_packed_attention(model, cache)
        else:
            model.config._attn_implementation = impl
            for m in model.modules():
                if hasattr(m, "_msq_packed_layer"):
                    del m._msq_packed_layer
        logits, toks, ids = [], [], prompt
        with torch.no_grad():
            for step in range(41):
                out = model(input_ids=ids, past_key_values=cache, use_cache=True)
                lg = out.logits[:, -1, :].float()
                logits.append(lg)
                nxt = lg.argmax(dim=-1, keepdim=True) if tokens is None else tokens[step]
                toks.append(nxt)
                ids = nxt
        assert cache.get_seq_length() == 70 + 40
        return logits, toks

    ls, toks = run("sdpa")
    le, _ = run("eager", toks)
    lf, _ = run(kp.ATTENTION_NAME, toks)
    assert model.config._attn_implementation == kp.ATTENTION_NAME
    worst = 0.0
    for step in range(41):
        df = float((lf[step] - ls[step]).abs().max())
        de = float((le[step] - ls[step]).abs().max())
        print("step %2d  |packed - sdpa| %.4e  |eager - sdpa| %.4e" % (step, df, de))
        assert df <= 4 * de, (step, df, de)
        worst = max(worst, df)
    assert math.isfinite(worst)
