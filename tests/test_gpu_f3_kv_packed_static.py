"""SURVEY 8 row f3, the packed MX KV cache with the lengths on the device (msq.kvpacked.StaticPackedKV, msq_kv_mx_append_dev /
msq_kv_mx_attn_decode_dev).

The reference throughout is the host-length path of the parent commit (PackedKV.append / attend, tests/test_gpu_f3_kv_packed.py checks it
against float64): the device-length entries promise the SAME BITS for equal cache contents, so every comparison is torch.equal -- of the
attention output at every step of a captured and replayed decode step, of the code / scale planes and tails after the flushes, and of a small
model's logits.  Also: the empty cache, the overflow that drops a token and says so, a planted Inf that surfaces through sync()."""
import pytest
import torch

from gpu_common import dev

pytestmark = pytest.mark.gpu

FMTS = ("fp8_e4m3", "fp4_e2m1")
DTYPES = (torch.float16, torch.bfloat16)
B, HKV = 2, 2
NAN, OVERFLOW = 1, 8


def _rand(shape, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(dtype)


def _left_pad_bias(width):
    """sequence 1: the first 40 positions are -inf (left padding); `width` may exceed the length: the rest is never read"""
    bias = torch.zeros(B, width, dtype=torch.float32, device=dev())
    bias[1, :40] = float("-inf")
    return bias


def _same_planes(st, dyn, upto):
    for n in ("k_codes", "v_codes", "v_scales"):
        assert torch.equal(st.planes[n][:, :, :upto], dyn.planes[n][:, :, :upto]), n
    assert torch.equal(st.planes["k_scales"][:, :, :upto // 32], dyn.planes["k_scales"][:, :, :upto // 32])


# ---------------------------------------------------------------------------------------------------------------------
# 1. the captured step against the eager dynamic cache
# ---------------------------------------------------------------------------------------------------------------------
def _captured_against_dynamic(kp, D, Hq, dtype, fmt, with_bias):
    n0, steps = 120, 50
    K = _rand((B, HKV, n0 + steps, D), 700 + D, dtype).to(dev())
    V = _rand((B, HKV, n0 + steps, D), 701 + D, dtype).to(dev())
    Q = _rand((steps, B, Hq, D), 702 + D, dtype).to(dev())
    dyn = kp.PackedKV(B, HKV, D, dtype, fmt, gap=32, capacity=32, device=dev())
    st = kp.StaticPackedKV(B, HKV, D, dtype, fmt, gap=32, max_len=256, device=dev())
    for c in (dyn, st):
        c.append(K[:, :, :n0], V[:, :, :n0])
        assert (c.packed_len, c.tail_len) == (96, 24)
    assert st.S_cap == 256 and st.sync() == (96, 24)
    bias = _left_pad_bias(288) if with_bias else None            # S_cap + gap wide: used in place, the same buffer at every length
    k_in = torch.zeros(B, HKV, 1, D, dtype=dtype, device=dev())
    v_in, q_in = torch.zeros_like(k_in), torch.zeros(B, Hq, D, dtype=dtype, device=dev())
    st.append(k_in, v_in)                                        # one eager step allocates the workspace ...
    st.attend_dev(q_in, bias)
    st.set_lengths(96, 24)                                       # ... and is undone: its token sits in a slot the first real step overwrites
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        st.append(k_in, v_in)
        y = st.attend_dev(q_in, bias)
    st.set_lengths(96, 24)                                       # capturing ran the Python (the mirror moved), not the kernels
    for i in range(steps):
        t = n0 + i
        k_in.copy_(K[:, :, t:t + 1]); v_in.copy_(V[:, :, t:t + 1]); q_in.copy_(Q[i])
        graph.replay()
        st.advance_host(1)
        dyn.append(K[:, :, t:t + 1], V[:, :, t:t + 1])
        want = dyn.attend(Q[i], None if bias is None else bias[:, :dyn.len].contiguous())
        assert torch.equal(y, want), ("step", i, "len", dyn.len, float((y.float() - want.float()).abs().max()))
        assert (st.packed_len, st.tail_len) == (dyn.packed_len, dyn.tail_len)
    assert (dyn.packed_len, dyn.tail_len) == (160, 10)           # the flushes at 128 and 160 tokens, one split -> two
    assert kp.attn_plan(B, Hq, HKV, D, 128, 0)[0] == 1 and kp.attn_plan(B, Hq, HKV, D, 160, 0)[0] == 2
    assert st.sync() == (160, 10) and st.state.tolist() == [160, 10, 0, 0]
    _same_planes(st, dyn, 160)
    assert torch.equal(st.k_tail, dyn.k_tail) and torch.equal(st.v_tail, dyn.v_tail)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("Hq", [4, 16])
@pytest.mark.parametrize("D", [64, 128])
def test_captured_step_equals_the_eager_dynamic_cache(msq, D, Hq, dtype, fmt):
    _captured_against_dynamic(msq.kvpacked, D, Hq, dtype, fmt, False)


def test_captured_step_with_a_left_padding_bias(msq):
    _captured_against_dynamic(msq.kvpacked, 128, 16, torch.bfloat16, "fp4_e2m1", True)


def test_capture_needs_the_workspace_first(msq):
    kp = msq.kvpacked
    st = kp.StaticPackedKV(B, HKV, 64, torch.float16, "fp8_e4m3", max_len=64, device=dev())
    q = torch.zeros(B, 4, 64, dtype=torch.float16, device=dev())
    kv = torch.zeros(B, HKV, 4, 64, dtype=torch.float16, device=dev())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                # both refusals come back before anything is launched into the capture
        q.zero_()                                                # (one node of our own: the graph is not empty)
        with pytest.raises(msq._lib.MsqError, match="eager"):
            st.attend_dev(q)
        with pytest.raises(msq._lib.MsqError, match="captur"):
            st.append(kv, kv)
    assert (st.packed_len, st.tail_len) == (0, 0)


# ---------------------------------------------------------------------------------------------------------------------
# 2. eager: the device-length entry equals the host-length entry bit for bit
# ---------------------------------------------------------------------------------------------------------------------
def _dev_equals_host(st, q, tag):
    width = st.S_cap + st.gap
    for bias in (None, _left_pad_bias(width)):
        hb = None if bias is None else bias[:, :st.len].contiguous()
        for od in (torch.float32, None):
            got, want = st.attend_dev(q, bias, out_dtype=od), st.attend(q, hb, out_dtype=od)
            assert got.dtype == want.dtype and torch.equal(got, want), (tag, "bias" if bias is not None else "-", od)
    if st.len < width:                                           # a bias of exactly the length is copied into a buffer of the full width
        assert torch.equal(st.attend_dev(q, _left_pad_bias(st.len)), st.attend(q, _left_pad_bias(st.len))), (tag, "narrow bias")


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("Hq", [4, 16])
@pytest.mark.parametrize("D", [64, 128])
def test_attend_dev_equals_attend(msq, D, Hq, dtype, fmt):
    kp = msq.kvpacked
    for S in (0, 32, 96, 160, 256):
        for tail in (0, 1, 31):
            if S + tail == 0:
                continue
            total = S + tail
            K = _rand((B, HKV, total, D), 100 + total, dtype).to(dev())
            V = _rand((B, HKV, total, D), 200 + total, dtype).to(dev())
            q = _rand((B, Hq, D), 300 + total, dtype).to(dev())
            st = kp.StaticPackedKV(B, HKV, D, dtype, fmt, gap=32, max_len=256, device=dev())
            st.append(K, V)
            assert st.sync() == (S, tail)
            _dev_equals_host(st, q, "D %d Hq %d %s %s S %d tail %d" % (D, Hq, str(dtype)[6:], fmt, S, tail))


def test_attend_dev_equals_attend_beyond_8192_tokens(msq):
    """257 groups: the groups per split go from 4 to 8 and the splits from 64 to 33, under a grid of 64"""
    kp = msq.kvpacked
    S, tail = 8224, 5
    assert kp.attn_plan(1, 1, 1, 64, 8192, 0)[:2] == (64, 128) and kp.attn_plan(1, 1, 1, 64, S, tail)[:2] == (33, 256)
    assert kp.attn_plan_cap(1, 1, 1, 64, S, 32)[0] == 64
    K = _rand((1, 1, S + tail, 64), 800, torch.float16).to(dev())
    V = _rand((1, 1, S + tail, 64), 801, torch.float16).to(dev())
    q = _rand((1, 1, 64), 802, torch.float16).to(dev())
    st = kp.StaticPackedKV(1, 1, 64, torch.float16, "fp4_e2m1", gap=32, max_len=S, device=dev())
    st.append(K, V)
    assert st.sync() == (S, tail)
    for bias in (None, torch.zeros(1, S + 32, dtype=torch.float32, device=dev())):
        if bias is not None:
            bias[0, 100:8000] = float("-inf")
        hb = None if bias is None else bias[:, :S + tail].contiguous()
        assert torch.equal(st.attend_dev(q, bias, out_dtype=torch.float32), st.attend(q, hb, out_dtype=torch.float32))


# ---------------------------------------------------------------------------------------------------------------------
# 3. - 5. the empty cache, overflow, status
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("D,Hq", [(64, 16), (128, 4)])
def test_empty_cache_gives_zeros_and_one_token_gives_its_value(msq, D, Hq, fmt):
    kp = msq.kvpacked
    st = kp.StaticPackedKV(B, HKV, D, torch.float16, fmt, gap=32, max_len=64, device=dev())
    q = _rand((B, Hq, D), 900, torch.float16).to(dev())
    for bias in (None, _left_pad_bias(96)):
        out = st.attend_dev(q, bias, out_dtype=torch.float32)
        assert tuple(out.shape) == (B, Hq, D) and bool((out == 0).all())
    k, v = (_rand((B, HKV, 1, D), 901 + i, torch.float16).to(dev()) for i in range(2))
    st.append(k, v)
    assert st.sync() == (0, 1)
    out = st.attend_dev(q, out_dtype=torch.float32)
    want = v[:, :, 0, :].double().repeat_interleave(Hq // HKV, dim=1)            # softmax over one token is 1
    err, floor = float((out.double() - want).abs().max()), 2.0 ** -20 * float(want.abs().max())
    print("one token: err %.3e floor %.3e" % (err, floor))
    assert err <= floor
    assert torch.equal(out, st.attend(q, out_dtype=torch.float32))


@pytest.mark.parametrize("fmt", FMTS)
def test_overflow_drops_the_token_and_raises_the_status(msq, fmt):
    kp = msq.kvpacked
    D = 64
    st = kp.StaticPackedKV(B, HKV, D, torch.bfloat16, fmt, gap=32, max_len=64, device=dev())
    K, V = _rand((B, HKV, 96, D), 910, torch.bfloat16).to(dev()), _rand((B, HKV, 96, D), 911, torch.bfloat16).to(dev())
    st.append(K[:, :, :95], V[:, :, :95])                        # prefill: 64 packed (the capacity), 31 in the tail ...
    st.append(K[:, :, 95:], V[:, :, 95:])                        # ... and the token that fills the tail: nothing left to flush into
    assert st.sync() == (64, 32)
    k, v = (_rand((B, HKV, 1, D), 912 + i, torch.bfloat16).to(dev()) for i in range(2))
    before = {n: t.clone() for n, t in st.planes.items()}
    tails = (st.k_tail.clone(), st.v_tail.clone())
    with pytest.raises(msq._lib.MsqError, match="overflow"):
        st.append(k, v)                                          # the mirror knows: refused before any launch
    assert st.state.tolist() == [64, 32, 0, 0]
    st._append_dev(k, v)                                         # the C entry, as a replayed graph would reach it
    assert st.state.tolist() == [64, 32, OVERFLOW, 0]
    for n, t in before.items():
        assert torch.equal(st.planes[n], t), n
    assert torch.equal(st.k_tail, tails[0]) and torch.equal(st.v_tail, tails[1])
    with pytest.raises(msq._lib.MsqError, match="MSQ_STATUS_OVERFLOW"):
        st.sync()
    assert (st.packed_len, st.tail_len) == (64, 32)
    st.set_lengths(32, 32)                                       # roll back one group: the status is cleared and the flush fits again
    st.append(k, v)
    assert st.sync() == (64, 1) and torch.equal(st.k_tail[:, :, :1], k)


def test_planted_inf_in_the_tail_raises_status_nan_at_its_flush(msq):
    kp = msq.kvpacked
    D = 64
    K, V = _rand((B, HKV, 33, D), 920, torch.float16), _rand((B, HKV, 33, D), 921, torch.float16)
    K[1, 0, 7, 33] = float("inf")
    K, V = K.to(dev()), V.to(dev())
    st = kp.StaticPackedKV(B, HKV, D, torch.float16, "fp8_e4m3", gap=32, max_len=64, device=dev())
    st.append(K[:, :, :31], V[:, :, :31])
    st.append(K[:, :, 31:32], V[:, :, 31:32])
    assert st.sync() == (0, 32)                                  # in the tail an Inf is just a value
    st.append(K[:, :, 32:33], V[:, :, 32:33])                    # the flush packs it
    assert st.state.tolist() == [32, 1, NAN, 0]
    with pytest.raises(msq._lib.MsqError, match="MSQ_STATUS_NAN"):
        st.sync()


# ---------------------------------------------------------------------------------------------------------------------
# 6. a model over the static cache
# ---------------------------------------------------------------------------------------------------------------------
def test_model_logits_equal_the_dynamic_packed_cache(msq):
    """The seeded 2-layer Llama of test_gpu_f3_kv_packed.py::test_model_logits_over_the_codes, 40 greedy steps from a 70-token prompt over the
    codes: PackedMXKVCache(max_len=128) (device append, attend_dev) gives the logits of the dynamic packed cache bit for bit."""
    from transformers import LlamaConfig, LlamaForCausalLM
    kp = msq.kvpacked
    torch.manual_seed(0)
    cfg = LlamaConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2, head_dim=64,
                      vocab_size=256, max_position_embeddings=256)
    cfg._attn_implementation = "sdpa"
    model = LlamaForCausalLM(cfg).to(torch.bfloat16).to(dev()).eval()
    prompt = torch.randint(0, 256, (1, 70), generator=torch.Generator().manual_seed(1)).to(dev())

    def run(cache, tokens=None):
        kp.use_packed_attention(model, cache)
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

    ld, toks = run(kp.PackedMXKVCache(2, "fp8_e4m3", gap=32))
    static = kp.PackedMXKVCache(2, "fp8_e4m3", gap=32, max_len=128)
    ls, _ = run(static, toks)
    for layer in static.layers:
        assert isinstance(layer.packed, kp.StaticPackedKV) and layer.packed.sync() == (96, 14)
    for step in range(41):
        assert torch.equal(ls[step], ld[step]), (step, float((ls[step] - ld[step]).abs().max()))
