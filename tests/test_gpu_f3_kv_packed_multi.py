"""SURVEY 8 row f3, the packed MX KV cache with MORE THAN ONE query token (msq.kvpacked.PackedKV.attend_multi / crop,
csrc/msq_kv_packed_multi.hip).

Attention: float64 causal attention over dequantize().double() -- the exact values the codes hold -- is the reference.  The float32 output may
be off by at most 2^-16 max|V dequantised| of the call: the probabilities enter the second product as hi + lo bf16 parts, 16 significant
bits, so every weight is off by at most 2^-17 relative, the output is a convex combination of V rows, and a factor 2 covers the float32
accumulation and the exponentials.  K, V and q enter exactly, so nothing else is rounded before an fp32 accumulator.  (A single bf16 P misses
this bound by an order of magnitude; torch's half-precision SDPA too.)  Every case prints the kernel's error beside those of torch's float32
math-backend SDPA and of its half-precision SDPA on the same tensors (pytest -s).  The half output is the float32 output rounded once; an
explicit [B, T, len] causal bias gives the bits of causal=True; a fully masked row gives zeros.
Row independence: a (token, head) row of a T-token call has the bits of the single-token call on that token; 20 repeats and another batch
size give the same bits.  A planted dominant token exercises every rescale path.  crop: dequantize() of the kept tokens and the planes before
packed_len do not change.  Model: a seeded 2-layer Llama fed in chunks of 4 tokens over the codes against sdpa on the same cache type, and a
rejected draft taken back."""
import math

import pytest
import torch

from gpu_common import dev

pytestmark = pytest.mark.gpu

FMTS = ("fp8_e4m3", "fp4_e2m1")
DTYPES = (torch.float16, torch.bfloat16)
B, HKV = 2, 2
NEG = float("-inf")


def _rand(shape, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(dtype)


def _filled(kp, K, V, fmt, gap=32):
    pk = kp.PackedKV(K.shape[0], K.shape[1], K.shape[3], K.dtype, fmt, gap=gap, capacity=32, device=dev())
    pk.append(K, V)
    return pk


def _split_tokens(kp, Hq, D):
    return kp.attn_plan(B, Hq, HKV, D, 4096, 0)[1]


def _causal_bias(Bv, T, total):
    """[B, T, total] float32: query t sees the positions <= total - T + t"""
    pos = torch.arange(total, device=dev())[None, :]
    lim = (total - T + torch.arange(T, device=dev()))[:, None]
    b = torch.zeros(T, total, dtype=torch.float32, device=dev()).masked_fill_(pos > lim, NEG)
    return b[None].expand(Bv, T, total).contiguous()


def _left_pad_bias(total):
    """sequence 1: the first 40 positions are -inf (left padding); a shorter cache is masked altogether"""
    bias = torch.zeros(B, total, dtype=torch.float32, device=dev())
    bias[1, :40] = NEG
    return bias


def _full_bias(q, total, bias, causal):
    """the additive [B, T, total] float32 mask a call amounts to"""
    Bv, T = q.shape[0], q.shape[2]
    full = _causal_bias(Bv, T, total) if causal else torch.zeros(Bv, T, total, dtype=torch.float32, device=dev())
    if bias is not None:
        full = full + (bias[:, None, :] if bias.ndim == 2 else bias)
    return full


def _reference(pk, q, full, scaling):
    """float64 attention over the values the cache holds.  Returns (ref [B, T, Hq, D] float64, logits [B, Hq, T, S], fully masked rows
    [B, T, Hq], max |V|)"""
    kd, vd = pk.dequantize()
    G = q.shape[1] // kd.shape[1]
    k64, v64 = kd.double().repeat_interleave(G, dim=1), vd.double().repeat_interleave(G, dim=1)
    logits = torch.einsum("bhtd,bhsd->bhts", q.double(), k64) * scaling + full.double()[:, None]
    dead = torch.isinf(logits).all(dim=3)
    w = torch.softmax(logits, dim=3)
    w = torch.where(torch.isnan(w), torch.zeros_like(w), w)
    return torch.einsum("bhts,bhsd->bthd", w, v64), logits, dead.permute(0, 2, 1), float(vd.float().abs().max())


def _torch_sdpa(pk, q, full, scaling, dtype):
    """torch's math-backend SDPA on the same dequantised tensors, in `dtype`; [B, T, Hq, D]"""
    from torch.nn.attention import SDPBackend, sdpa_kernel
    kd, vd = pk.dequantize()
    G = q.shape[1] // kd.shape[1]
    k, v = kd.to(dtype).repeat_interleave(G, dim=1), vd.to(dtype).repeat_interleave(G, dim=1)
    with sdpa_kernel(SDPBackend.MATH):
        y = torch.nn.functional.scaled_dot_product_attention(q.to(dtype), k, v, attn_mask=full[:, None].to(dtype), scale=scaling)
    return y.transpose(1, 2)


def _check(pk, q, bias, causal, tag, ratios=None):
    """the float32 bound, the zeros of masked rows and the half-output identity of one call; returns the float32 output"""
    scaling = q.shape[3] ** -0.5
    full = _full_bias(q, pk.len, bias, causal)
    ref, _, dead, vmax = _reference(pk, q, full, scaling)
    out32 = pk.attend_multi(q, bias, causal=causal, scaling=scaling, out_dtype=torch.float32)
    assert tuple(out32.shape) == (q.shape[0], q.shape[2], q.shape[1], q.shape[3]) and out32.dtype == torch.float32
    assert bool((out32[dead] == 0).all()), (tag, "a fully masked row must give zeros")
    live = ~dead
    bound = 2.0 ** -16 * vmax
    if bool(live.any()):
        err = float((out32.double() - ref)[live].abs().max())
        e32 = float((_torch_sdpa(pk, q, full, scaling, torch.float32).double() - ref)[live].abs().max())
        e16 = float((_torch_sdpa(pk, q, full, scaling, q.dtype).double() - ref)[live].abs().max())
        print("%-66s err %.3e bound %.3e (%.3f) torch f32 %.3e half %.3e" % (tag, err, bound, err / bound, e32, e16))
        if ratios is not None:
            ratios.append(err / bound)
        assert err <= bound, (tag, err, bound)
    outh = pk.attend_multi(q, bias, causal=causal, scaling=scaling)
    assert outh.dtype == q.dtype and torch.equal(outh, out32.to(q.dtype)), (tag, "half output != rounded float32 output")
    return out32


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("Hq", [4, 16])
@pytest.mark.parametrize("D", [64, 128])
def test_attend_multi_against_float64(msq, D, Hq, dtype, fmt):
    kp = msq.kvpacked
    st = _split_tokens(kp, Hq, D)
    assert st % 32 == 0 and kp.attn_plan(B, Hq, HKV, D, st + 32, 0)[0] == 2 and kp.attn_plan(B, Hq, HKV, D, 2 * st, 0)[0] == 2
    ratios = []
    for S, tail in ((0, 17), (32, 0), (96, 1), (st + 32, 31), (2 * st, 0)):      # at (96, 1) the causal edge of T = 5 cuts through a packed group
        total = S + tail
        K = _rand((B, HKV, total, D), 100 + total, dtype).to(dev())
        V = _rand((B, HKV, total, D), 200 + total, dtype).to(dev())
        pk = _filled(kp, K, V, fmt)
        assert (pk.packed_len, pk.tail_len) == (S, tail)
        for T in (2, 5, 17):                                     # at G = 8, T = 17 is 136 rows: three row tiles, the last part-filled
            q = _rand((B, Hq, T, D), 300 + total + T, dtype).to(dev())
            tag = "D %d Hq %d %s %s S %d tail %d T %d" % (D, Hq, str(dtype)[6:], fmt, S, tail, T)
            causal = _check(pk, q, None, True, tag + " causal", ratios)
            _check(pk, q, _left_pad_bias(total), True, tag + " causal + padding", ratios)
            explicit = _check(pk, q, _causal_bias(B, T, total), False, tag + " [B, T, len] bias", ratios)
            assert torch.equal(explicit, causal), (tag, "an explicit causal bias must give the bits of causal=True")
    print("worst err / bound: %.4f" % max(ratios))


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_a_row_has_the_bits_of_its_single_token_call(msq, dtype, fmt):
    """the project's rule: a row's result is the same bits alone or among others, from run to run and whatever it is batched with"""
    kp = msq.kvpacked
    D, Hq, T = 128, 16, 17
    st = _split_tokens(kp, Hq, D)
    total = st + 32 + 31
    K = _rand((B, HKV, total, D), 500, dtype).to(dev())
    V = _rand((B, HKV, total, D), 501, dtype).to(dev())
    q = _rand((B, Hq, T, D), 502, dtype).to(dev())
    pk = _filled(kp, K, V, fmt)
    first = pk.attend_multi(q, out_dtype=torch.float32)
    for t in range(T):
        bias = torch.zeros(B, total, dtype=torch.float32, device=dev())
        bias[:, total - T + t + 1:] = NEG
        one = pk.attend_multi(q[:, :, t:t + 1].contiguous(), bias, out_dtype=torch.float32)
        assert torch.equal(one[:, 0], first[:, t]), t
    for _ in range(20):
        assert torch.equal(pk.attend_multi(q, out_dtype=torch.float32), first)
    single = _filled(kp, K[:1].contiguous(), V[:1].contiguous(), fmt)
    assert torch.equal(single.attend_multi(q[:1].contiguous(), out_dtype=torch.float32)[0], first[0])


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("D,Hq", [(64, 16), (128, 4)])
def test_rescale_paths_with_a_dominant_token(msq, D, Hq, dtype, fmt):
    """one token whose logit exceeds all others by more than 30, in the first split, in the last split, in the tail"""
    kp = msq.kvpacked
    st = _split_tokens(kp, Hq, D)
    S, tail, T = st + 32, 31, 5
    total = S + tail
    for where, t in (("first split", 5), ("last split", S - 3), ("tail", total - T - 1)):
        K = _rand((B, HKV, total, D), 400, dtype)
        V = _rand((B, HKV, total, D), 401, dtype)
        q = _rand((B, Hq, T, D), 402, dtype)
        sign = torch.where(_rand((D,), 403) >= 0, 1.0, -1.0)
        q = (q.float().abs() * sign).to(dtype)                   # every query row leans the same way ...
        K[:, :, t, :] = (8.0 * sign).to(dtype)                   # ... and one key points there
        pk = _filled(kp, K.to(dev()), V.to(dev()), fmt)
        q = q.to(dev())
        _, logits, _, _ = _reference(pk, q, _full_bias(q, total, None, True), D ** -0.5)
        others = torch.cat([logits[..., :t], logits[..., t + 1:]], dim=3)
        assert float((logits[..., t] - others.max(dim=3).values).min()) > 30, where
        _check(pk, q, None, True, "dominant token in the %s: D %d Hq %d %s %s" % (where, D, Hq, str(dtype)[6:], fmt))


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("static", [False, True], ids=["dynamic", "static"])
def test_crop_keeps_the_bits_of_the_kept_tokens(msq, static, fmt):
    kp = msq.kvpacked
    D, Hq, dtype = 64, 4, torch.bfloat16
    K = _rand((B, HKV, 100, D), 600, dtype).to(dev())
    V = _rand((B, HKV, 100, D), 601, dtype).to(dev())
    if static:
        pk = kp.StaticPackedKV(B, HKV, D, dtype, fmt, gap=32, max_len=128, device=dev())
        pk.append(K, V)
    else:
        pk = _filled(kp, K, V, fmt)
    assert (pk.packed_len, pk.tail_len) == (96, 4)
    k0, v0 = pk.dequantize()
    planes0 = {n: p.clone() for n, p in pk.planes.items()}
    for n, want in ((98, (96, 2)), (70, (64, 6)), (64, (64, 0)), (0, (0, 0))):
        pk.crop(n)
        assert (pk.packed_len, pk.tail_len) == want and pk.len == n
        if static:
            assert pk.sync() == want and pk.state.tolist()[2] == 0
        k, v = pk.dequantize()
        assert torch.equal(k, k0[:, :, :n]) and torch.equal(v, v0[:, :, :n]), n
        P = pk.packed_len
        for name in ("k_codes", "v_codes", "v_scales"):
            assert torch.equal(pk.planes[name][:, :, :P], planes0[name][:, :, :P]), (n, name)
        assert torch.equal(pk.planes["k_scales"][:, :, :P // 32], planes0["k_scales"][:, :, :P // 32]), n
        if n:
            q = _rand((B, Hq, 5, D), 602 + n, dtype).to(dev())
            _check(pk, q, None, True, "after crop(%d) %s %s" % (n, "static" if static else "dynamic", fmt))
    with pytest.raises(msq._lib.MsqError):
        pk.attend_multi(_rand((B, Hq, 2, D), 1, dtype).to(dev()))            # the cache is empty
    pk.append(K[:, :, :40], V[:, :, :40])                        # and it goes on from there
    assert (pk.packed_len, pk.tail_len) == (32, 8)
    assert torch.equal(pk.dequantize()[0][:, :, :32], k0[:, :, :32])          # the packed group; the 8 tail tokens are unquantised again


def test_model_chunks_and_a_rejected_draft(msq, monkeypatch):
    """The seeded 2-layer Llama of test_gpu_f3_kv_packed.py (hidden 256, 4 heads, 2 kv heads, head_dim 64, bf16) over an fp8 PackedMXKVCache:
    a 70-token prompt, then ten chunks of 4 tokens.  Per chunk: max |logits(msq_packed_kv, max_query_tokens=8) - logits(sdpa)| <=
    4 max |logits(eager) - logits(sdpa)| -- the project's bound: sdpa and eager are two implementations over identical dequantised tensors.
    With the default max_query_tokens the chunks go to sdpa.  A rejected draft: append 4, crop 2, append 2 others."""
    from transformers import LlamaConfig, LlamaForCausalLM
    kp = msq.kvpacked
    torch.manual_seed(0)
    cfg = LlamaConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2, head_dim=64,
                      vocab_size=256, max_position_embeddings=256)
    cfg._attn_implementation = "sdpa"
    model = LlamaForCausalLM(cfg).to(torch.bfloat16).to(dev()).eval()
    g = torch.Generator().manual_seed(1)
    prompt = torch.randint(0, 256, (1, 70), generator=g).to(dev())
    chunks = [torch.randint(0, 256, (1, 4), generator=g).to(dev()) for _ in range(10)]
    calls = []
    real = kp.PackedKV.attend_multi

    def spy(self, q, *a, **kw):
        calls.append(int(q.shape[2]))
        return real(self, q, *a, **kw)

    monkeypatch.setattr(kp.PackedKV, "attend_multi", spy)

    def setup(impl, **kw):
        cache = kp.PackedMXKVCache(2, "fp8_e4m3", gap=32)
        if impl == kp.ATTENTION_NAME:
            kp.use_packed_attention(model, cache, **kw)
        else:
            model.config._attn_implementation = impl
            for m in model.modules():
                if hasattr(m, "_msq_packed_layer"):
                    del m._msq_packed_layer
        return cache

    def feed(cache, ids):
        with torch.no_grad():
            return model(input_ids=ids, past_key_values=cache, use_cache=True).logits.float()

    def run(impl, **kw):
        cache = setup(impl, **kw)
        feed(cache, prompt)
        out = [feed(cache, c) for c in chunks]
        assert cache.get_seq_length() == 70 + 40
        return out

    ls = run("sdpa")
    le = run("eager")
    assert calls == []
    ld = run(kp.ATTENTION_NAME)                                  # the default: query lengths above 1 still go to sdpa
    assert calls == [] and len(ld) == 10
    lf = run(kp.ATTENTION_NAME, max_query_tokens=8)
    assert calls == [4] * 20                                     # ten chunks, two layers; the 70-token prompt went to sdpa
    for i in range(10):
        df, de = float((lf[i] - ls[i]).abs().max()), float((le[i] - ls[i]).abs().max())
        print("chunk %2d  |packed - sdpa| %.4e  |eager - sdpa| %.4e" % (i, df, de))
        assert df <= 4 * de, (i, df, de)
        assert math.isfinite(df)

    # a rejected draft: 4 draft tokens, the last `reject` taken back, then 2 others; against a run whose draft differed in its last two (rejected)
    # tokens.  70 + 4 tokens, 2 rejected: the crop stays in the tail (packed 64, tail 10 -> 8).  94 + 4 tokens cross a gap boundary (packed 96,
    # tail 2); 3 rejected: PackedKVLayer.crop goes into the packed part (n = 95 < 96: packed 64, the tail = the unpacked codes 64 .. 95)
    long_prompt = torch.cat([prompt, chunks[2], chunks[3], chunks[4], chunks[5], chunks[6], chunks[7]], dim=1)
    assert long_prompt.shape[1] == 94

    def draft_round(start, draft, reject, before, after):
        cache = setup(kp.ATTENTION_NAME, max_query_tokens=8)
        feed(cache, start)
        feed(cache, draft)
        n = start.shape[1] + 4
        pk = cache.layers[0].packed
        assert cache.get_seq_length() == n and (pk.packed_len, pk.tail_len) == before
        cache.crop(-reject)
        assert cache.get_seq_length() == n - reject and (pk.packed_len, pk.tail_len) == after
        return feed(cache, chunks[1][:, :2]), cache

    other = chunks[0].clone()
    other[:, 2:] = (other[:, 2:] + 1) % 256
    for start, reject, before, after in ((prompt, 2, (64, 10), (64, 8)), (long_prompt, 3, (96, 2), (64, 31))):
        la, ca = draft_round(start, chunks[0], reject, before, after)
        lb, cb = draft_round(start, other, reject, before, after)
        assert torch.equal(la, lb), (reject, float((la - lb).abs().max()))
        for x, y in zip(ca.layers, cb.layers):
            (kx, vx), (ky, vy) = x.packed.dequantize(), y.packed.dequantize()
            assert torch.equal(kx, ky) and torch.equal(vx, vy)
