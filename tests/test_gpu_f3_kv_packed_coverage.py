"""SURVEY 8 row f3, the packed MX KV cache at the arguments the other four test_gpu_f3_kv_packed*.py files never launch (msq.kvpacked,
csrc/msq_kv_packed.hip, csrc/msq_kv_packed_multi.hip).  Those files run gap 32, 2 kv heads with 2 or 8 query heads each,
head_dim 64 / 128, the default scaling, a bias of 0 / -inf and randn inputs.  Here:

  1. GQA ratios     G = Hq / Hkv in {1, 3, 4, 5, 6, 7} with Hkv in {1, 2, 3} and B in {1, 3}: the GMAX = 1 and GMAX = 4 instantiations of the decode
                    kernel, G < GMAX, the rg / G, rg % G row map of the MFMA kernel at G that is no power of two; host, _dev and _seq forms
  2. gap 64 / 96    more than one chunk of 32 tail tokens (tc > 0) in both attention kernels, a full tail, the device flush of tail_cap / 32 = 2
                    K groups (shared state row and a row per slot), overflow at gap 64
  3. finite bias    an ALiBi-shaped bias with a slope per sequence and scaling != head_dim^-0.5: fmaf(dot, scaling, bias) against
                    (dot + bias) * scaling; a [B, T, len] bias whose rows differ by more than the causal edge
  4. scale bytes    K, V and q scaled by exact powers of two per channel / token group / (token, channel block), so that neighbouring E8M0 bytes
                    differ while the logits stay those of the randn case; compared per block of 32 output channels
  5. pack / unpack  blocks of zeros, one non-zero element, the ends of the fp16 / bf16 range; PackedKV at head_dim 96 and 256
  6. row tiles      exactly 16, 32 and 64 rows of attend_multi and one more, 256 rows, T = 1, T = len

The rules are those of the files beside this one, not new ones.  The reference is float64 attention over dequantize().double() -- the exact values
the codes hold.  Decode (attend, attend_dev): the float32 output is within max(4 x the error of torch's float32 math-backend SDPA against the same
reference, 2^-20 max|ref|) (test_gpu_f3_kv_packed.py).  attend_multi: within 2^-16 max|V dequantised| (the per-row derivation at the top of
test_gpu_f3_kv_packed_multi.py: it depends on neither G, T nor the gap).  A half output is the float32 output rounded once, a fully masked row is
zeros, and the device-length forms give the bits of the host-length form.  Every test prints its figures (pytest -s); what a test needs to hold on
the inputs (a logit lead, the logit range, the count of distinct scale bytes) is asserted before the kernel runs."""
import numpy as np
import pytest
import torch

from gpu_common import dev, eq

pytestmark = pytest.mark.gpu

FMTS = ("fp8_e4m3", "fp4_e2m1")
F16, BF16 = torch.float16, torch.bfloat16
DTYPES = (F16, BF16)
NEG = float("-inf")
OVERFLOW = 8                                                     # include/msq.h MSQ_STATUS_OVERFLOW
PLANES = ("k_codes", "k_scales", "v_codes", "v_scales")


def _dn(dtype):
    return str(dtype)[6:]


def _rand(shape, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(dtype)


def _kvq(Bv, Hkv, Hq, total, D, dtype, seed, T=None):
    """K, V [B, Hkv, total, D] and q [B, Hq, D] (or [B, Hq, T, D]) on the device"""
    K = _rand((Bv, Hkv, total, D), seed, dtype).to(dev())
    V = _rand((Bv, Hkv, total, D), seed + 1, dtype).to(dev())
    q = _rand((Bv, Hq, D) if T is None else (Bv, Hq, T, D), seed + 2, dtype).to(dev())
    return K, V, q


def _feed(cache, K, V, singles=0):
    """all but the last `singles` tokens in one append, those one at a time (the way a tail gets full)"""
    n = K.shape[2] - singles
    if n:
        cache.append(K[:, :, :n], V[:, :, :n])
    for i in range(n, K.shape[2]):
        cache.append(K[:, :, i:i + 1], V[:, :, i:i + 1])
    return cache


def _filled(kp, K, V, fmt, gap=32, singles=0):
    return _feed(kp.PackedKV(K.shape[0], K.shape[1], K.shape[3], K.dtype, fmt, gap=gap, capacity=32, device=dev()), K, V, singles)


def _split_tokens(kp, Bv, Hq, Hkv, D):
    """the tokens of one split: st + 32 packed tokens are one group past a split boundary"""
    st = kp.attn_plan(Bv, Hq, Hkv, D, 4096, 0)[1]
    assert st % 32 == 0 and kp.attn_plan(Bv, Hq, Hkv, D, st + 32, 0)[0] == 2
    return st


def _pad_bias(Bv, width):
    """the last sequence: the first 40 positions are -inf (left padding); a shorter cache is masked altogether"""
    bias = torch.zeros(Bv, width, dtype=torch.float32, device=dev())
    bias[Bv - 1, :40] = NEG
    return bias


def _alibi_bias(Bv, width, lens, pad=True):
    """-slope_b x (len_b - 1 - pos), a slope per sequence, as float32; with pad the last sequence's first 40 positions are -inf.  `lens`: one length
    or one per sequence; positions at or beyond a sequence's length hold 0 (a wide bias of the device-length forms: never read)"""
    lens = [lens] * Bv if isinstance(lens, int) else list(lens)
    pos = torch.arange(width, dtype=torch.float32, device=dev())
    rows = []
    for b in range(Bv):
        slope = 0.05 * 2.0 ** b
        rows.append(torch.where(pos < lens[b], -slope * (lens[b] - 1 - pos), torch.zeros_like(pos)))
    bias = torch.stack(rows)
    if pad:
        bias[Bv - 1, :40] = NEG
    return bias


def _block_max(x, D):
    """max |x| per block of 32 channels (the last axis), over everything else: [D / 32]"""
    return x.abs().reshape(-1, D // 32, 32).amax(dim=(0, 2))


# ---------------------------------------------------------------------------------------------------------------------
# the float64 references and the two bounds
# ---------------------------------------------------------------------------------------------------------------------
def _reference(pk, q, bias, scaling):
    """one query token: (ref [B, Hq, D] float64, logits [B, Hq, S], fully masked rows [B, Hq])"""
    kd, vd = pk.dequantize()
    G = q.shape[1] // kd.shape[1]
    k64, v64 = kd.double().repeat_interleave(G, dim=1), vd.double().repeat_interleave(G, dim=1)
    logits = torch.einsum("bhd,bhsd->bhs", q.double(), k64) * scaling
    if bias is not None:
        logits = logits + bias.double()[:, None, :]
    dead = torch.isinf(logits).all(dim=2)
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


def _check(pk, q, bias, tag, scaling=None, per_block=False):
    """PackedKV.attend: the float32 bound (per_block: held for every block of 32 output channels on its own), the zeros of masked rows and the
    half-output identity; returns the float32 output"""
    D = q.shape[2]
    scaling = D ** -0.5 if scaling is None else scaling
    ref, _, dead = _reference(pk, q, bias, scaling)
    out32 = pk.attend(q, bias, scaling, out_dtype=torch.float32)
    assert tuple(out32.shape) == tuple(q.shape) and out32.dtype == torch.float32
    assert bool((out32[dead] == 0).all()), (tag, "a fully masked row must give zeros")
    live = ~dead
    if bool(live.any()):
        th = _torch_f32(pk, q, bias, scaling)
        e, et, r = (out32.double() - ref)[live], (th.double() - ref)[live], ref[live]
        if per_block:
            err, err_t, floor = _block_max(e, D), _block_max(et, D), 2.0 ** -20 * _block_max(r, D)
            bound = torch.maximum(4 * err_t, floor)
            print("%-72s err/bound per block %s" % (tag, " ".join("%.3e/%.3e" % (float(a), float(b)) for a, b in zip(err, bound))))
            assert bool((err <= bound).all()), (tag, err.tolist(), err_t.tolist(), floor.tolist())
        else:
            err, err_t, floor = float(e.abs().max()), float(et.abs().max()), 2.0 ** -20 * float(r.abs().max())
            bound = max(4 * err_t, floor)
            print("%-72s err %.3e torch %.3e floor %.3e (err / bound %.3f)" % (tag, err, err_t, floor, err / bound))
            assert err <= bound, (tag, err, err_t, floor)
    else:
        print("%-72s every row masked: zeros" % tag)
    outh = pk.attend(q, bias, scaling)
    assert outh.dtype == q.dtype and torch.equal(outh, out32.to(q.dtype)), (tag, "half output != rounded float32 output")
    return out32


def _causal_bias(Bv, T, total):
    """[B, T, total] float32: query t sees the positions <= total - T + t"""
    pos = torch.arange(total, device=dev())[None, :]
    lim = (total - T + torch.arange(T, device=dev()))[:, None]
    b = torch.zeros(T, total, dtype=torch.float32, device=dev()).masked_fill_(pos > lim, NEG)
    return b[None].expand(Bv, T, total).contiguous()


def _full_bias(q, total, bias, causal):
    """the additive [B, T, total] float32 mask a call amounts to"""
    Bv, T = q.shape[0], q.shape[2]
    full = _causal_bias(Bv, T, total) if causal else torch.zeros(Bv, T, total, dtype=torch.float32, device=dev())
    if bias is not None:
        full = full + (bias[:, None, :] if bias.ndim == 2 else bias)
    return full


def _reference_multi(pk, q, full, scaling):
    """T query tokens: (ref [B, T, Hq, D] float64, logits [B, Hq, T, S], fully masked rows [B, T, Hq], V dequantised)"""
    kd, vd = pk.dequantize()
    G = q.shape[1] // kd.shape[1]
    k64, v64 = kd.double().repeat_interleave(G, dim=1), vd.double().repeat_interleave(G, dim=1)
    logits = torch.einsum("bhtd,bhsd->bhts", q.double(), k64) * scaling + full.double()[:, None]
    dead = torch.isinf(logits).all(dim=3)
    w = torch.softmax(logits, dim=3)
    w = torch.where(torch.isnan(w), torch.zeros_like(w), w)
    return torch.einsum("bhts,bhsd->bthd", w, v64), logits, dead.permute(0, 2, 1), vd


def _check_multi(pk, q, bias, causal, tag, scaling=None, per_block=False):
    """PackedKV.attend_multi: the bound 2^-16 max|V dequantised| (per_block: every block of 32 output channels against the maximum of ITS channels of V),
    the zeros of masked rows and the half-output identity; returns the float32 output"""
    D = q.shape[3]
    scaling = D ** -0.5 if scaling is None else scaling
    ref, _, dead, vd = _reference_multi(pk, q, _full_bias(q, pk.len, bias, causal), scaling)
    out32 = pk.attend_multi(q, bias, causal=causal, scaling=scaling, out_dtype=torch.float32)
    assert tuple(out32.shape) == (q.shape[0], q.shape[2], q.shape[1], D) and out32.dtype == torch.float32
    assert bool((out32[dead] == 0).all()), (tag, "a fully masked row must give zeros")
    live = ~dead
    if bool(live.any()):
        e = (out32.double() - ref)[live]
        if per_block:
            err, bound = _block_max(e, D), 2.0 ** -16 * _block_max(vd.double(), D)
            print("%-72s err/bound per block %s" % (tag, " ".join("%.3e/%.3e" % (float(a), float(b)) for a, b in zip(err, bound))))
            assert bool((err <= bound).all()), (tag, err.tolist(), bound.tolist())
        else:
            err, bound = float(e.abs().max()), 2.0 ** -16 * float(vd.float().abs().max())
            print("%-72s err %.3e bound %.3e (err / bound %.3f)" % (tag, err, bound, err / bound))
            assert err <= bound, (tag, err, bound)
    else:
        print("%-72s every row masked: zeros" % tag)
    outh = pk.attend_multi(q, bias, causal=causal, scaling=scaling)
    assert outh.dtype == q.dtype and torch.equal(outh, out32.to(q.dtype)), (tag, "half output != rounded float32 output")
    return out32


def _lengths(kp, Bv, Hq, Hkv, D):
    st = _split_tokens(kp, Bv, Hq, Hkv, D)
    return ((0, 5), (96, 1), (st + 32, 31))


def _slots(kp, lens, Hkv, D, dtype, fmt, seed, gap=32, max_len=256):
    """a SlotPackedKV whose slot b holds lens[b] = (packed, tail) tokens, one PackedKV(B = 1) per slot fed the same tokens (a full tail: all but one
    token, then one), and the tokens"""
    sl = kp.SlotPackedKV(len(lens), Hkv, D, dtype, fmt, gap=gap, max_len=max_len, device=dev())
    refs, toks = [], []
    for b, (p, t) in enumerate(lens):
        K, V = (_rand((1, Hkv, p + t + 1, D), seed + 10 * b + i, dtype).to(dev()) for i in range(2))      # one token to spare: the next step's
        ref = kp.PackedKV(1, Hkv, D, dtype, fmt, gap=gap, capacity=32, device=dev())
        at = 0
        for n in ([p + t - 1, 1] if t == gap else [p + t]):
            sl.prefill(b, K[:, :, at:at + n], V[:, :, at:at + n])
            ref.append(K[:, :, at:at + n], V[:, :, at:at + n])
            at += n
        assert sl.lengths[b] == (ref.packed_len, ref.tail_len) == (p, t), b
        refs.append(ref); toks.append((K, V))
    assert sl.sync() == [tuple(x) for x in lens]
    return sl, refs, toks


def _ref_rows(refs, q, bias, scaling, out_dtype):
    """row b: slot b's own cache attends alone (host lengths, B = 1)"""
    return torch.cat([r.attend(q[b:b + 1], None if bias is None else bias[b:b + 1, :r.len].contiguous(), scaling, out_dtype=out_dtype)
                      for b, r in enumerate(refs)], dim=0)


# ---------------------------------------------------------------------------------------------------------------------
# 1. GQA ratios: G in {1, 3, 4, 5, 6, 7}
# ---------------------------------------------------------------------------------------------------------------------
GQA = [pytest.param(hkv, hq, b, dt, id="hkv%d-hq%d-b%d-%s" % (hkv, hq, b, _dn(dt)))
       for hkv, hq, b, dts in ((1, 1, 3, (F16,)), (3, 3, 1, (BF16,)),                  # G = 1: GMAX = 1 (multi-head attention)
                               (1, 3, 3, DTYPES), (2, 8, 1, DTYPES),                   # G = 3, 4: GMAX = 4
                               (1, 5, 1, (BF16,)), (2, 12, 3, (F16,)), (1, 7, 3, (BF16,)))   # G = 5, 6, 7: GMAX = 8, G < GMAX
       for dt in dts]


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Hkv,Hq,Bv,dtype", GQA)
def test_gqa_attend_against_float64_and_attend_dev(msq, Hkv, Hq, Bv, dtype, D, fmt):
    """PackedKV.attend against float64, and StaticPackedKV.attend_dev (same tokens, same lengths) with the bits of attend"""
    kp = msq.kvpacked
    for S, tail in _lengths(kp, Bv, Hq, Hkv, D):
        total = S + tail
        K, V, q = _kvq(Bv, Hkv, Hq, total, D, dtype, 1000 + total + Hq)
        pk = _filled(kp, K, V, fmt)
        st = _feed(kp.StaticPackedKV(Bv, Hkv, D, dtype, fmt, gap=32, max_len=S + 32, device=dev()), K, V)
        assert (pk.packed_len, pk.tail_len) == (S, tail) and st.sync() == (S, tail)
        for bias in (None, _pad_bias(Bv, total)):
            tag = "G %d Hkv %d B %d D %d %s %s S %d tail %d %s" % (Hq // Hkv, Hkv, Bv, D, _dn(dtype), fmt, S, tail, "bias" if bias is not None else "-")
            out32 = _check(pk, q, bias, tag)
            wide = None if bias is None else _pad_bias(Bv, st.S_cap + st.gap)
            assert torch.equal(st.attend_dev(q, wide, out_dtype=torch.float32), out32), (tag, "attend_dev != attend")
            assert torch.equal(st.attend_dev(q, wide), out32.to(dtype)), (tag, "attend_dev != attend (half)")


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Hkv,Hq,Bv,dtype", GQA)
def test_gqa_ragged_slots_equal_every_slots_own_cache(msq, Hkv, Hq, Bv, dtype, D, fmt):
    """SlotPackedKV.attend_dev on three slots of different lengths (Bv does not enter: the slots are the batch)"""
    kp = msq.kvpacked
    lens = _lengths(kp, 1, Hq, Hkv, D)
    sl, refs, _ = _slots(kp, lens, Hkv, D, dtype, fmt, 1100 + Hq, max_len=lens[2][0] + 32)
    q = _rand((3, Hq, D), 1101 + Hq, dtype).to(dev())
    bias = torch.zeros(3, sl.S_cap + sl.gap, dtype=torch.float32, device=dev())
    bias[1, 3:50] = NEG
    bias[2, 100:140] = NEG
    for bs in (None, bias):
        for od in (torch.float32, None):
            got, want = sl.attend_dev(q, bs, out_dtype=od), _ref_rows(refs, q, bs, None, od)
            assert got.dtype == want.dtype and torch.equal(got, want), (lens, "bias" if bs is not None else "-", od)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Hkv,Hq,Bv,dtype", GQA)
def test_gqa_attend_multi_against_float64(msq, Hkv, Hq, Bv, dtype, D, fmt):
    kp = msq.kvpacked
    for S, tail in _lengths(kp, Bv, Hq, Hkv, D):
        total = S + tail
        for T in (2, 5):
            K, V, q = _kvq(Bv, Hkv, Hq, total, D, dtype, 1200 + total + Hq + T, T)
            pk = _filled(kp, K, V, fmt)
            tag = "G %d Hkv %d B %d D %d %s %s S %d tail %d T %d" % (Hq // Hkv, Hkv, Bv, D, _dn(dtype), fmt, S, tail, T)
            _check_multi(pk, q, None, True, tag + " causal")
            _check_multi(pk, q, _pad_bias(Bv, total), True, tag + " causal + padding")


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("Hkv,Hq,D", [(2, 6, 128), (1, 5, 64)], ids=["G3", "G5"])
def test_gqa_row_has_the_bits_of_its_single_token_call(msq, Hkv, Hq, D, dtype, fmt):
    """the claim of the kernel header at G that is no power of two: a row's bits do not depend on the rows it is computed with (T = 17 is 51 and 85
    rows: row tiles of 64 that a token's G rows straddle; T = 1 is one tile of 16)"""
    kp = msq.kvpacked
    Bv, T = 2, 17
    total = _split_tokens(kp, Bv, Hq, Hkv, D) + 32 + 31
    K, V, q = _kvq(Bv, Hkv, Hq, total, D, dtype, 1300 + Hq, T)
    pk = _filled(kp, K, V, fmt)
    first = pk.attend_multi(q, out_dtype=torch.float32)
    for t in range(T):
        bias = torch.zeros(Bv, total, dtype=torch.float32, device=dev())
        bias[:, total - T + t + 1:] = NEG
        one = pk.attend_multi(q[:, :, t:t + 1].contiguous(), bias, out_dtype=torch.float32)
        assert torch.equal(one[:, 0], first[:, t]), t
    single = _filled(kp, K[:1].contiguous(), V[:1].contiguous(), fmt)
    assert torch.equal(single.attend_multi(q[:1].contiguous(), out_dtype=torch.float32)[0], first[0])


# ---------------------------------------------------------------------------------------------------------------------
# 2. gap = 64 and 96: tail chunks after the first, a full tail, the device flush of two K groups
# ---------------------------------------------------------------------------------------------------------------------
GAP_STATES = ((64, 0, 33), (64, 64, 32), (64, 64, 63), (64, 128, 64), (96, 96, 65), (96, 96, 96))     # (gap, S, tail); a full tail by single appends
SHAPES = [pytest.param(64, 8, F16, "fp8_e4m3", id="64-8-f16-fp8"), pytest.param(128, 4, BF16, "fp4_e2m1", id="128-4-bf16-fp4"),
          pytest.param(64, 4, BF16, "fp8_e4m3", id="64-4-bf16-fp8"), pytest.param(128, 16, F16, "fp4_e2m1", id="128-16-f16-fp4")]
B, HKV = 2, 2


@pytest.mark.parametrize("gap,S,tail", GAP_STATES)
@pytest.mark.parametrize("D,Hq,dtype,fmt", SHAPES)
def test_wide_gap_attend_and_attend_multi_against_float64(msq, D, Hq, dtype, fmt, gap, S, tail):
    kp = msq.kvpacked
    total = S + tail
    K, V, q = _kvq(B, HKV, Hq, total, D, dtype, 2000 + total + gap)
    pk = _filled(kp, K, V, fmt, gap=gap, singles=5 if tail == gap else 0)
    assert (pk.packed_len, pk.tail_len, pk.k_tail.shape[2]) == (S, tail, gap)
    tag = "gap %d S %d tail %d D %d Hq %d %s %s" % (gap, S, tail, D, Hq, _dn(dtype), fmt)
    for bias in (None, _pad_bias(B, total)):
        bt = " padding" if bias is not None else ""
        _check(pk, q, bias, tag + bt)
        for T in (3, 17):
            qm = _rand((B, Hq, T, D), 2001 + total + T, dtype).to(dev())
            _check_multi(pk, qm, bias, True, tag + " T %d%s" % (T, bt))


@pytest.mark.parametrize("D,Hq,dtype,fmt", SHAPES)
def test_wide_gap_dominant_token_in_the_second_and_third_tail_chunk(msq, D, Hq, dtype, fmt):
    """one token whose logit exceeds all others by more than 30, in tail tokens 32 .. 63 and 64 .. 95 of a full tail of 96"""
    kp = msq.kvpacked
    gap, S, tail, T = 96, 96, 96, 5
    total = S + tail
    for where, t in (("second tail chunk", S + 40), ("third tail chunk", S + 80)):
        K = _rand((B, HKV, total, D), 2100, dtype)
        V = _rand((B, HKV, total, D), 2101, dtype)
        sign = torch.where(_rand((D,), 2103) >= 0, 1.0, -1.0)
        q = (_rand((B, Hq, D), 2102, dtype).float().abs() * sign).to(dtype).to(dev())        # every query row leans the same way ...
        qm = (_rand((B, Hq, T, D), 2104, dtype).float().abs() * sign).to(dtype).to(dev())
        K[:, :, t, :] = (8.0 * sign).to(dtype)                                               # ... and one key points there
        pk = _filled(kp, K.to(dev()), V.to(dev()), fmt, gap=gap, singles=2)
        assert (pk.packed_len, pk.tail_len) == (S, tail) and t < total - T
        _, logits, _ = _reference(pk, q, None, D ** -0.5)
        others = torch.cat([logits[..., :t], logits[..., t + 1:]], dim=2)
        assert float((logits[..., t] - others.max(dim=2).values).min()) > 30, where
        _, logits, _, _ = _reference_multi(pk, qm, _full_bias(qm, total, None, True), D ** -0.5)
        others = torch.cat([logits[..., :t], logits[..., t + 1:]], dim=3)
        assert float((logits[..., t] - others.max(dim=3).values).min()) > 30, where
        tag = "dominant token in the %s: D %d Hq %d %s %s" % (where, D, Hq, _dn(dtype), fmt)
        _check(pk, q, None, tag)
        _check_multi(pk, qm, None, True, tag + " T %d" % T)


@pytest.mark.parametrize("S", [0, 64])
@pytest.mark.parametrize("D,Hq,dtype,fmt", SHAPES)
def test_attend_multi_over_a_full_tail_of_32(msq, D, Hq, dtype, fmt, S):
    """tail_len == gap: the state between the append that fills the tail and the one that flushes it"""
    kp = msq.kvpacked
    total = S + 32
    K = _rand((B, HKV, total, D), 2200 + S, dtype).to(dev())
    V = _rand((B, HKV, total, D), 2201 + S, dtype).to(dev())
    pk = _filled(kp, K, V, fmt, singles=3)
    assert (pk.packed_len, pk.tail_len) == (S, 32)
    for T in (1, 5, 32):
        q = _rand((B, Hq, T, D), 2202 + T, dtype).to(dev())
        for bias in (None, _pad_bias(B, total)):
            _check_multi(pk, q, bias, True, "full tail: S %d D %d Hq %d %s %s T %d%s" % (S, D, Hq, _dn(dtype), fmt, T, " padding" if bias is not None else ""))


def _same_planes(pa, pb, upto, sa=slice(None)):
    """the first `upto` tokens of two sets of planes (sa: the slots of pa to look at)"""
    for n in ("k_codes", "v_codes", "v_scales"):
        assert torch.equal(pa[n][sa, :, :upto], pb[n][:, :, :upto]), n
    assert torch.equal(pa["k_scales"][sa, :, :upto // 32], pb["k_scales"][:, :, :upto // 32]), "k_scales"


@pytest.mark.parametrize("D,Hq,dtype,fmt", SHAPES)
def test_gap64_captured_step_flushes_two_k_groups(msq, D, Hq, dtype, fmt):
    """StaticPackedKV(gap=64): one captured step replayed 140 times from an empty cache, against the eager PackedKV(gap=64) fed the same tokens.  The
    device flush packs tail_cap / 32 = 2 K groups and moves packed_len by 64: after either flush the planes and the state are the host pack's."""
    kp = msq.kvpacked
    steps, gap = 140, 64
    K = _rand((B, HKV, steps, D), 2300 + D, dtype).to(dev())
    V = _rand((B, HKV, steps, D), 2301 + D, dtype).to(dev())
    Q = _rand((steps, B, Hq, D), 2302 + D, dtype).to(dev())
    dyn = kp.PackedKV(B, HKV, D, dtype, fmt, gap=gap, capacity=32, device=dev())
    st = kp.StaticPackedKV(B, HKV, D, dtype, fmt, gap=gap, max_len=192, device=dev())
    assert st.S_cap == 192 and tuple(st.k_tail.shape) == (B, HKV, gap, D)
    bias = _pad_bias(B, 256) if fmt == "fp4_e2m1" else None      # S_cap + gap wide: used in place, the same buffer at every length
    k_in = torch.zeros(B, HKV, 1, D, dtype=dtype, device=dev())
    v_in, q_in = torch.zeros_like(k_in), torch.zeros(B, Hq, D, dtype=dtype, device=dev())
    st.append(k_in, v_in)                                        # one eager step allocates the workspace ...
    st.attend_dev(q_in, bias)
    st.set_lengths(0, 0)                                         # ... and is undone: its token sits in the slot the first real step overwrites
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        st.append(k_in, v_in)
        y = st.attend_dev(q_in, bias)
    st.set_lengths(0, 0)                                         # capturing ran the Python (the mirror moved), not the kernels
    flushes = []
    for i in range(steps):
        k_in.copy_(K[:, :, i:i + 1]); v_in.copy_(V[:, :, i:i + 1]); q_in.copy_(Q[i])
        graph.replay()
        st.advance_host(1)
        dyn.append(K[:, :, i:i + 1], V[:, :, i:i + 1])
        want = dyn.attend(Q[i], None if bias is None else bias[:, :dyn.len].contiguous())
        assert torch.equal(y, want), ("step", i, "len", dyn.len, float((y.float() - want.float()).abs().max()))
        assert (st.packed_len, st.tail_len) == (dyn.packed_len, dyn.tail_len)
        if dyn.packed_len and dyn.tail_len == 1:                 # this step flushed
            flushes.append(i)
            assert st.sync() == (dyn.packed_len, 1) and st.state.tolist() == [dyn.packed_len, 1, 0, 0]
            _same_planes(st.planes, dyn.planes, dyn.packed_len)
    assert flushes == [64, 128] and st.sync() == (128, 12)
    _same_planes(st.planes, dyn.planes, 128)
    assert torch.equal(st.k_tail, dyn.k_tail) and torch.equal(st.v_tail, dyn.v_tail)


@pytest.mark.parametrize("fmt", FMTS)
def test_gap64_overflow_drops_the_129th_token(msq, fmt):
    kp = msq.kvpacked
    D = 64
    st = kp.StaticPackedKV(B, HKV, D, BF16, fmt, gap=64, max_len=64, device=dev())
    K, V = _rand((B, HKV, 128, D), 2400, BF16).to(dev()), _rand((B, HKV, 128, D), 2401, BF16).to(dev())
    _feed(st, K, V, singles=2)                                   # 64 packed (the capacity) and a full tail of 64: nothing left to flush into
    assert st.S_cap == 64 and st.sync() == (64, 64)
    k, v = (_rand((B, HKV, 1, D), 2402 + i, BF16).to(dev()) for i in range(2))
    before = {n: t.clone() for n, t in st.planes.items()}
    tails = (st.k_tail.clone(), st.v_tail.clone())
    with pytest.raises(msq._lib.MsqError, match="overflow"):
        st.append(k, v)                                          # the mirror knows: refused before any launch
    assert st.state.tolist() == [64, 64, 0, 0]
    st._append_dev(k, v)                                         # the C entry, as a replayed graph would reach it
    assert st.state.tolist() == [64, 64, OVERFLOW, 0]
    for n, t in before.items():
        assert torch.equal(st.planes[n], t), n
    assert torch.equal(st.k_tail, tails[0]) and torch.equal(st.v_tail, tails[1])
    with pytest.raises(msq._lib.MsqError, match="MSQ_STATUS_OVERFLOW"):
        st.sync()
    assert (st.packed_len, st.tail_len) == (64, 64)


@pytest.mark.parametrize("D,Hq,dtype,fmt", SHAPES)
def test_gap64_slots_one_captured_step_in_which_only_the_middle_slot_flushes(msq, D, Hq, dtype, fmt):
    kp = msq.kvpacked
    gap, lens = 64, ((0, 40), (64, 64), (128, 1))
    k_in = torch.zeros(3, HKV, 1, D, dtype=dtype, device=dev())
    v_in, q_in = torch.zeros_like(k_in), torch.zeros(3, Hq, D, dtype=dtype, device=dev())
    sl = kp.SlotPackedKV(3, HKV, D, dtype, fmt, gap=gap, max_len=192, device=dev())
    sl.append(k_in, v_in)                                        # the eager step that allocates the workspace runs on the EMPTY slots: at the
    sl.attend_dev(q_in)                                          # lengths below it would flush the middle slot for real
    for b in range(3):
        sl.reset(b)
    refs, toks = [], []
    for b, (p, t) in enumerate(lens):
        Kb, Vb = (_rand((1, HKV, p + t + 1, D), 2500 + 10 * b + i, dtype).to(dev()) for i in range(2))
        ref = kp.PackedKV(1, HKV, D, dtype, fmt, gap=gap, capacity=32, device=dev())
        at = 0
        for n in ([p + t - 1, 1] if t == gap else [p + t]):
            sl.prefill(b, Kb[:, :, at:at + n], Vb[:, :, at:at + n]); ref.append(Kb[:, :, at:at + n], Vb[:, :, at:at + n])
            at += n
        refs.append(ref); toks.append((Kb, Vb))
    assert sl.sync() == [tuple(x) for x in lens] and [(r.packed_len, r.tail_len) for r in refs] == [tuple(x) for x in lens]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sl.append(k_in, v_in)
        y = sl.attend_dev(q_in)
    for b, (p, t) in enumerate(lens):
        sl.set_lengths(b, p, t)                                  # capturing ran the Python (the mirror moved), not the kernels
    before = {n: t.clone() for n, t in sl.planes.items()}
    q = _rand((3, Hq, D), 2550, dtype).to(dev())
    for b, (p, t) in enumerate(lens):
        k_in[b].copy_(toks[b][0][0, :, p + t:p + t + 1]); v_in[b].copy_(toks[b][1][0, :, p + t:p + t + 1])
    q_in.copy_(q)
    graph.replay()
    sl.advance_host(1)
    after = [(0, 41), (128, 1), (128, 2)]
    assert sl.lengths == after and sl.state.tolist() == [[p, t, 0, 0] for p, t in after] and sl.sync() == after
    for b, (p, t) in enumerate(lens):
        r = refs[b]
        r.append(toks[b][0][:, :, p + t:p + t + 1], toks[b][1][:, :, p + t:p + t + 1])
        assert (r.packed_len, r.tail_len) == after[b]
        assert torch.equal(y[b:b + 1], r.attend(q[b:b + 1])), ("slot", b)
        _same_planes(sl.planes, r.planes, r.packed_len, slice(b, b + 1))
        assert torch.equal(sl.k_tail[b:b + 1, :, :r.tail_len], r.k_tail[:, :, :r.tail_len]) and torch.equal(sl.v_tail[b:b + 1, :, :r.tail_len], r.v_tail[:, :, :r.tail_len]), b
    for n in PLANES:                                             # slots 0 and 2 did not flush: not a byte of their planes moved
        assert torch.equal(sl.planes[n][0], before[n][0]) and torch.equal(sl.planes[n][2], before[n][2]), n
        assert not torch.equal(sl.planes[n][1], before[n][1]), n


# ---------------------------------------------------------------------------------------------------------------------
# 3. a finite bias and scaling != head_dim^-0.5
# ---------------------------------------------------------------------------------------------------------------------
BIAS_SHAPES = [pytest.param(64, 8, F16, "fp8_e4m3", id="64-8-f16-fp8"), pytest.param(128, 16, BF16, "fp4_e2m1", id="128-16-bf16-fp4"),
               pytest.param(64, 16, BF16, "fp8_e4m3", id="64-16-bf16-fp8"), pytest.param(128, 8, F16, "fp4_e2m1", id="128-8-f16-fp4")]


def _scalings(D):
    return (0.5 * D ** -0.5, 0.25)


@pytest.mark.parametrize("D,Hq,dtype,fmt", BIAS_SHAPES)
def test_alibi_bias_and_scaling_decode(msq, D, Hq, dtype, fmt):
    """fmaf(dot, scaling, bias): a kernel that scaled the bias too, or took another sequence's row, is off by whole logits.  The static and the
    per-slot form take the same bias at width S_cap + gap and give the bits of attend."""
    kp = msq.kvpacked
    st = _split_tokens(kp, B, Hq, HKV, D)
    for S, tail in ((96, 1), (st + 32, 31)):
        total = S + tail
        K, V, q = _kvq(B, HKV, Hq, total, D, dtype, 3000 + total)
        pk = _filled(kp, K, V, fmt)
        sk = _feed(kp.StaticPackedKV(B, HKV, D, dtype, fmt, gap=32, max_len=S + 32, device=dev()), K, V)
        bias, wide = _alibi_bias(B, total, total), _alibi_bias(B, sk.S_cap + sk.gap, total)
        assert torch.equal(wide[:, :total], bias) and bool(torch.isfinite(bias[0]).all()) and float(bias[0].min()) < -4
        for scaling in _scalings(D):
            out32 = _check(pk, q, bias, "ALiBi: D %d Hq %d %s %s S %d tail %d scaling %.4f" % (D, Hq, _dn(dtype), fmt, S, tail, scaling), scaling)
            assert torch.equal(sk.attend_dev(q, wide, scaling, out_dtype=torch.float32), out32), "attend_dev != attend"
    lens = ((0, 5), (96, 1), (st + 32, 31))
    sl, refs, _ = _slots(kp, lens, HKV, D, dtype, fmt, 3050, max_len=st + 64)
    q = _rand((3, Hq, D), 3051, dtype).to(dev())
    wide = _alibi_bias(3, sl.S_cap + sl.gap, [p + t for p, t in lens])
    for scaling in _scalings(D):
        for od in (torch.float32, None):
            assert torch.equal(sl.attend_dev(q, wide, scaling, out_dtype=od), _ref_rows(refs, q, wide, scaling, od)), ("slots", scaling, od)


@pytest.mark.parametrize("D,Hq,dtype,fmt", BIAS_SHAPES)
def test_alibi_bias_and_scaling_multi(msq, D, Hq, dtype, fmt):
    """the [B, len] form, and a [B, T, len] bias whose rows differ by more than the causal edge (ALiBi + 0.01 t cos(pos), held as float32: the
    reference adds exactly those values), with causal=True on top and with causal=False"""
    kp = msq.kvpacked
    st, T = _split_tokens(kp, B, Hq, HKV, D), 5
    for S, tail in ((96, 1), (st + 32, 31)):
        total = S + tail
        K, V, q = _kvq(B, HKV, Hq, total, D, dtype, 3100 + total, T)
        pk = _filled(kp, K, V, fmt)
        bias = _alibi_bias(B, total, total)
        pos = torch.arange(total, dtype=torch.float32, device=dev())
        rows = (bias[:, None, :] + (0.01 * torch.arange(T, dtype=torch.float32, device=dev()))[None, :, None] * torch.cos(pos)[None, None, :]).contiguous()
        assert rows.dtype == torch.float32 and tuple(rows.shape) == (B, T, total) and float((rows[0, T - 1] - rows[0, 0]).abs().max()) > 0.03
        for scaling in _scalings(D):
            tag = "ALiBi: D %d Hq %d %s %s S %d tail %d T %d scaling %.4f" % (D, Hq, _dn(dtype), fmt, S, tail, T, scaling)
            _check_multi(pk, q, bias, True, tag + " [B, len]", scaling)
            _check_multi(pk, q, rows, True, tag + " [B, T, len] causal", scaling)
            _check_multi(pk, q, rows, False, tag + " [B, T, len]", scaling)


# ---------------------------------------------------------------------------------------------------------------------
# 4. distinct scale bytes
# ---------------------------------------------------------------------------------------------------------------------
def _scaled_inputs(Hq, total, D, dtype, seed, T=None):
    """K = randn x 2^(e_c + u_g), q = randn x 2^(-e_c), V = randn x 2^f: e_c in -6 .. 6 per channel, u_g in {-1, 0, 1} per group of 32 tokens, f in
    -6 .. 6 per (token, block of 32 channels) -- exact powers of two on the values the cache dtype holds, so q . k is that of the randn tensors times
    2^u_g.  Returns (K, V, q, K0, q0) on the host; K0, q0: the unscaled tensors of the same seed."""
    g = torch.Generator().manual_seed(seed)
    K0 = torch.randn(B, HKV, total, D, generator=g).to(dtype)
    V0 = torch.randn(B, HKV, total, D, generator=g).to(dtype)
    q0 = torch.randn(*((B, Hq, D) if T is None else (B, Hq, T, D)), generator=g).to(dtype)
    ng = (total + 31) // 32
    e_c = torch.randint(-6, 7, (D,), generator=g).float()
    u_g = torch.randint(-1, 2, (ng,), generator=g).float().repeat_interleave(32)[:total]
    f = torch.randint(-6, 7, (B, HKV, total, D // 32), generator=g).float().repeat_interleave(32, dim=3)
    K = (K0.float() * torch.exp2(e_c[None, None, None, :] + u_g[None, None, :, None])).to(dtype)
    V = (V0.float() * torch.exp2(f)).to(dtype)
    q = (q0.float() * torch.exp2(-e_c)).to(dtype)
    return K, V, q, K0, q0


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("Hq", [8, 16], ids=["G4", "G8"])
@pytest.mark.parametrize("D", [64, 128])
def test_distinct_scale_bytes(msq, D, Hq, dtype, fmt):
    """neighbouring channels of K and neighbouring (token, block) entries of V carry different E8M0 bytes: a wrong byte of the eight a lane
    holds, or another block's V scale, is off by powers of two"""
    kp = msq.kvpacked
    S, tail, T = _split_tokens(kp, B, Hq, HKV, D) + 32, 31, 5
    total, G = S + tail, Hq // HKV
    for Tq in (None, T):
        K, V, q, K0, q0 = _scaled_inputs(Hq, total, D, dtype, 4000 + D + Hq, Tq)
        # on the host, before anything is launched: the logits stay in the range of the randn case, and the scale planes will hold many bytes
        eins = "bhd,bhsd->bhs" if Tq is None else "bhtd,bhsd->bhts"
        lg = torch.einsum(eins, q.double(), K.double().repeat_interleave(G, dim=1)) * D ** -0.5
        lg0 = torch.einsum(eins, q0.double(), K0.double().repeat_interleave(G, dim=1)) * D ** -0.5
        assert float(lg.abs().max()) <= 2 * float(lg0.abs().max()), (float(lg.abs().max()), float(lg0.abs().max()))
        kexp = torch.floor(torch.log2(K[:, :, :S].float().abs().reshape(B, HKV, S // 32, 32, D).amax(dim=3)))
        vexp = torch.floor(torch.log2(V[:, :, :S].float().abs().reshape(B, HKV, S, D // 32, 32).amax(dim=4)))
        assert len(torch.unique(kexp)) >= 8 and len(torch.unique(vexp)) >= 8
        pk = _filled(kp, K.to(dev()), V.to(dev()), fmt)
        assert (pk.packed_len, pk.tail_len) == (S, tail)
        nk, nv = (len(torch.unique(pk.planes[n][:, :, :S // g])) for n, g in (("k_scales", 32), ("v_scales", 1)))
        ks = pk.planes["k_scales"][:, :, :S // 32]
        print("D %d Hq %d %s %s: %d distinct K scale bytes, %d distinct V scale bytes, %.0f %% of neighbouring K channels differ"
              % (D, Hq, _dn(dtype), fmt, nk, nv, 100 * float((ks[..., 1:] != ks[..., :-1]).float().mean())))
        assert nk >= 8 and nv >= 8
        tag = "scale bytes: D %d Hq %d %s %s S %d tail %d" % (D, Hq, _dn(dtype), fmt, S, tail)
        if Tq is None:
            _check(pk, q.to(dev()), None, tag, per_block=True)
        else:
            _check_multi(pk, q.to(dev()), None, True, tag + " T %d" % T, per_block=True)


# ---------------------------------------------------------------------------------------------------------------------
# 5. pack / unpack: the ends of the range, head dims other than 64 / 128
# ---------------------------------------------------------------------------------------------------------------------
def _edge_blocks():
    """[(name, block of 32 float32 values)]: the block maximum sits at element 5 (either sign), the rest is randn x 0.3 x the maximum"""
    def around(top, seed, sign=1.0):
        rs = np.random.RandomState(seed)
        x = (rs.randn(32) * 0.3).astype(np.float32) * np.float32(top)
        x[5] = np.float32(sign * top)
        return x
    one = np.zeros(32, np.float32); one[7] = 1.0
    tiny = np.zeros(32, np.float32); tiny[31] = -2.0 ** -20
    bf16_max = float(np.uint32(0x7F7F0000).view(np.float32))
    return [("all zero", np.zeros(32, np.float32)), ("zero but one element", one), ("zero but one small negative element", tiny),
            ("fp16 max", around(65504.0, 1)), ("-fp16 max", around(65504.0, 2, -1.0)),
            ("bf16 max", around(bf16_max, 3)), ("-bf16 max", around(bf16_max, 4, -1.0)),
            ("fp16 smallest normal", around(2.0 ** -14, 5)), ("fp16 subnormal", around(3 * 2.0 ** -24, 6)), ("fp16 smallest subnormal", around(2.0 ** -24, 7)),
            ("bf16 smallest normal", around(2.0 ** -126, 8)), ("bf16 subnormal", around(3 * 2.0 ** -133, 9)), ("bf16 smallest subnormal", around(2.0 ** -133, 10))]


def _edge_matrix():
    """the edge blocks, then randn blocks: ([64 blocks, 32] float32, the names)"""
    blocks = _edge_blocks()
    rs = np.random.RandomState(77)
    rows = [b for _, b in blocks] + [rs.randn(32).astype(np.float32) for _ in range(64 - len(blocks))]
    return np.stack(rows), [n for n, _ in blocks] + ["randn"] * (64 - len(blocks))


def _as_tensor(m, along_tokens):
    """[64 blocks, 32] -> [1, 1, 32, 64]: the blocks along the tokens (one per channel) or along head_dim (two per token)"""
    return np.ascontiguousarray(m.T.reshape(1, 1, 32, 64) if along_tokens else m.reshape(1, 1, 32, 64))


def _per_block(a, along_tokens):
    """[1, 1, 32, 64] -> [64 blocks, 32]"""
    a = np.asarray(a, np.float32).reshape(32, 64)
    return a.T if along_tokens else a.reshape(64, 32)


@pytest.mark.parametrize("along_tokens", [1, 0])
@pytest.mark.parametrize("fmt", FMTS)
def test_pack_of_edge_blocks_is_quantize_mx_f32(msq, O, fmt, along_tokens):
    """zeros, one non-zero element, the largest finite and the smallest normal / subnormal values of fp16 and bf16: unpack(pack(x)) against the
    oracle and against the package's float32 route (kvpacked.py: the definition of the bytes), bit for bit; as float32 and held in the dtype
    that can hold them"""
    kp = msq.kvpacked
    axis = 2 if along_tokens else 3
    cn, sn = ("k_codes", "k_scales") if along_tokens else ("v_codes", "v_scales")
    m, names = _edge_matrix()
    for dt in (torch.float32, F16, BF16):
        # the blocks at the ends of bf16's range overflow or flush in an fp16 tensor: zeros there (an Inf would raise MSQ_STATUS_NAN)
        keep = np.array([dt != F16 or "bf16" not in n for n in names])
        x = torch.from_numpy(_as_tensor(m * keep[:, None].astype(np.float32), along_tokens)).to(dt)
        want = O.quantize_mx(x.float().numpy(), 8, fmt, axis=axis, block_size=32)          # on the host, before anything is launched
        assert np.isfinite(want).all()
        P = {n: torch.zeros(s, dtype=torch.uint8, device=dev()) for n, s in kp.plane_shapes(1, 1, 32, 64, fmt).items()}
        kp.mx_pack(x.to(dev()), P[cn], P[sn], 0, fmt, along_tokens, check_status=True)
        got = kp.mx_unpack(P[cn], P[sn], 0, 32, 64, torch.float32, fmt, along_tokens).cpu().numpy()
        pkg = msq.mx_ops._quantize_mx(x.float().to(dev()), 8, fmt, axes=[axis], block_size=32).cpu().numpy()
        gb, wb, pb = _per_block(got, along_tokens), _per_block(want, along_tokens), _per_block(pkg, along_tokens)
        for i, n in enumerate(names[:len(_edge_blocks())]):
            if keep[i]:
                print("%-9s %-5s %s %-36s max|x| %.6e -> %.6e  kernel == package %s, == oracle %s, oracle == package %s"
                      % (fmt, _dn(dt), "K" if along_tokens else "V", n, float(np.abs(_per_block(x.float().numpy(), along_tokens)[i]).max()),
                         float(np.abs(gb[i]).max()), eq(gb[i], pb[i]), eq(gb[i], wb[i]), eq(wb[i], pb[i])))
        bad = [n for i, n in enumerate(names) if not eq(gb[i], pb[i])]
        assert not bad, ("kernel != package", _dn(dt), bad)
        bad = [n for i, n in enumerate(names) if not eq(gb[i], wb[i])]
        assert not bad, ("kernel != oracle", _dn(dt), bad)
        assert (got[np.asarray(x.float().numpy()) == 0] == 0).all(), "a zero must stay a zero"
        for odt in DTYPES:                                       # an unpack rounds once to the cache dtype
            h = kp.mx_unpack(P[cn], P[sn], 0, 32, 64, odt, fmt, along_tokens)
            assert eq(h.float().cpu().numpy(), torch.from_numpy(want).to(odt).float().numpy()), (_dn(dt), odt)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("D", [96, 256])
def test_cache_at_head_dims_without_an_attention_kernel(msq, O, D, dtype, fmt):
    """PackedKV at head_dim 96 and 256 (append, dequantize, crop work at every multiple of 32 up to 256; the attention kernels exist for 64 and
    128): after 70 + 30 single tokens dequantize() is the oracle's quantised prefix followed by the exact tail, crop keeps the bits of the kept
    tokens, attend and attend_multi raise"""
    kp = msq.kvpacked
    n0, steps = 70, 30
    K = _rand((B, HKV, n0 + steps, D), 5000 + D, dtype).to(dev())
    V = _rand((B, HKV, n0 + steps, D), 5001 + D, dtype).to(dev())
    qf = lambda t, ax: torch.from_numpy(O.quantize_mx(t.float().cpu().numpy(), 8, fmt, axis=ax, block_size=32)).to(dtype).to(dev())
    qk, qv = qf(K[:, :, :96], 2), qf(V[:, :, :96], 3)
    pk = kp.PackedKV(B, HKV, D, dtype, fmt, gap=32, capacity=64, device=dev())
    for n in [n0] + [1] * steps:
        at = pk.len
        pk.append(K[:, :, at:at + n], V[:, :, at:at + n])
        P = 96 if pk.len > 96 else 64                            # the tail of 32 is packed when the 97th token arrives
        assert (pk.packed_len, pk.len) == (P, at + n)
        k, v = pk.dequantize()
        assert k.dtype == dtype and tuple(k.shape) == (B, HKV, at + n, D)
        assert eq(k.float().cpu().numpy(), torch.cat([qk[:, :, :P], K[:, :, P:at + n]], dim=2).float().cpu().numpy()), ("K", at + n)
        assert eq(v.float().cpu().numpy(), torch.cat([qv[:, :, :P], V[:, :, P:at + n]], dim=2).float().cpu().numpy()), ("V", at + n)
    assert pk.capacity == 128
    for Hq in (HKV, 4 * HKV):
        with pytest.raises(msq._lib.MsqError, match="head_dim must be 64 or 128"):
            pk.attend(_rand((B, Hq, D), 1, dtype).to(dev()))
        with pytest.raises(msq._lib.MsqError, match="head_dim must be 64 or 128"):
            pk.attend_multi(_rand((B, Hq, 3, D), 2, dtype).to(dev()))
    k0, v0 = pk.dequantize()
    planes0 = {n: p.clone() for n, p in pk.planes.items()}
    for n, want in ((98, (96, 2)), (70, (64, 6)), (64, (64, 0)), (33, (32, 1)), (0, (0, 0))):
        pk.crop(n)
        assert (pk.packed_len, pk.tail_len) == want and pk.len == n
        if n:
            k, v = pk.dequantize()
            assert torch.equal(k, k0[:, :, :n]) and torch.equal(v, v0[:, :, :n]), n
        _same_planes(pk.planes, planes0, pk.packed_len)


# ---------------------------------------------------------------------------------------------------------------------
# 6. row-tile edges of attend_multi
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,dtype,fmt", [(128, F16, "fp8_e4m3"), (64, BF16, "fp4_e2m1")], ids=["128-f16-fp8", "64-bf16-fp4"])
@pytest.mark.parametrize("T,G", [(16, 1), (17, 1), (32, 1), (11, 3), (16, 4), (13, 5), (32, 8), (1, 8)],
                         ids=["16rows", "17rows", "32rows", "33rows", "64rows", "65rows", "256rows", "T1-8rows"])
def test_row_tile_edges_against_float64(msq, T, G, D, dtype, fmt):
    """nr = 1 up to 16 rows, 2 up to 32, 4 beyond; 65 rows are two row tiles, 256 are four full ones"""
    kp = msq.kvpacked
    Hq = G * HKV
    st = _split_tokens(kp, B, Hq, HKV, D)
    for S, tail in ((96, 1), (st + 32, 31)):
        total = S + tail
        K, V, q = _kvq(B, HKV, Hq, total, D, dtype, 6000 + total + T * G, T)
        pk = _filled(kp, K, V, fmt)
        tag = "%d rows: T %d G %d D %d %s %s S %d tail %d" % (T * G, T, G, D, _dn(dtype), fmt, S, tail)
        _check_multi(pk, q, None, True, tag)
        _check_multi(pk, q, _pad_bias(B, total), True, tag + " padding")


@pytest.mark.parametrize("D,Hq,dtype,fmt", SHAPES)
def test_as_many_query_tokens_as_the_cache_holds(msq, D, Hq, dtype, fmt):
    """T == len: query 0 sees exactly one position, its own"""
    kp = msq.kvpacked
    for S, tail, singles in ((32, 0, 0), (0, 32, 3), (0, 5, 0)):
        T = total = S + tail
        K, V, q = _kvq(B, HKV, Hq, total, D, dtype, 6100 + total + S, T)
        pk = _filled(kp, K, V, fmt, singles=singles)
        assert (pk.packed_len, pk.tail_len) == (S, tail)
        out = _check_multi(pk, q, None, True, "T == len: D %d Hq %d %s %s S %d tail %d" % (D, Hq, _dn(dtype), fmt, S, tail))
        _, logits, _, vd = _reference_multi(pk, q, _full_bias(q, total, None, True), D ** -0.5)
        assert int(torch.isfinite(logits[:, :, 0]).sum()) == B * Hq and bool(torch.isfinite(logits[:, :, 0, 0]).all())
        first = vd[:, :, 0].float().repeat_interleave(Hq // HKV, dim=1)               # softmax over one position is 1: query 0 returns V of token 0
        assert float((out[:, 0] - first).abs().max()) <= 2.0 ** -16 * float(vd.float().abs().max())
