"""SURVEY 8 row f3, the packed MX KV cache with a state row per sequence (msq.kvpacked.SlotPackedKV, msq_kv_mx_append_seq /
msq_kv_mx_attn_decode_seq).

The yardstick throughout is the code that is already tested: an independent PackedKV(B = 1) per slot, fed that slot's tokens
(tests/test_gpu_f3_kv_packed.py checks it against float64, and shows that a sequence's bits do not depend on its batch).  The per-sequence
entries promise the SAME BITS for every slot, so every comparison is torch.equal -- no tolerance.  Fixed setup: 3 slots, 2 kv heads, max_len
288: msq_kv_mx_attn_plan_cap gives a grid of 3 splits of 128 tokens, so slots with 96, 160 and 256 packed tokens have 1, 2 and 2 live splits
under it -- rows of different live counts in one workspace."""
import pytest
import torch

from gpu_common import dev

pytestmark = pytest.mark.gpu

FMTS = ("fp8_e4m3", "fp4_e2m1")
DTYPES = (torch.float16, torch.bfloat16)
B, HKV, MAX_LEN, GAP = 3, 2, 288, 32
WIDTH = MAX_LEN + GAP                                            # 320: the bias width
NAN, OVERFLOW, IDLE = 1, 8, 1
TRIPLES = (((0, 0), (0, 1), (32, 0)), ((96, 1), (160, 31), (256, 0)), ((0, 17), (256, 32), (96, 0)))
PLANES = ("k_codes", "k_scales", "v_codes", "v_scales")


def _rand(shape, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(dtype)


def _chunks(p, t):
    """token counts of the appends that leave a cache at p packed + t tail tokens (a full tail: all but one token, then one)"""
    n = p + t
    if n == 0:
        return []
    return [n - 1, 1] if t == GAP else [n]


def _fill(kp, lens, D, dtype, fmt, seed, max_len=MAX_LEN, order=None):
    """a SlotPackedKV whose slot b holds sequence order[b] at lens[order[b]], and one PackedKV(B = 1) per SEQUENCE fed the same tokens"""
    order = list(range(len(lens))) if order is None else order
    sl = kp.SlotPackedKV(len(lens), HKV, D, dtype, fmt, gap=GAP, max_len=max_len, device=dev())
    refs = [kp.PackedKV(1, HKV, D, dtype, fmt, gap=GAP, capacity=32, device=dev()) for _ in lens]
    for slot, s in enumerate(order):
        p, t = lens[s]
        K, V = (_rand((1, HKV, max(p + t, 1), D), seed + 10 * s + i, dtype).to(dev()) for i in range(2))
        at = 0
        for n in _chunks(p, t):
            sl.prefill(slot, K[:, :, at:at + n], V[:, :, at:at + n])
            refs[s].append(K[:, :, at:at + n], V[:, :, at:at + n])
            at += n
        assert sl.lengths[slot] == (refs[s].packed_len, refs[s].tail_len) == (p, t), (slot, s)
    assert sl.sync() == [tuple(lens[s]) for s in order]
    return sl, refs


def _bias():
    bias = torch.zeros(B, WIDTH, dtype=torch.float32, device=dev())
    bias[0, 5:40] = float("-inf")
    bias[1, 0:3] = float("-inf")                                 # a slot of one token: every position masked, zeros
    bias[2, 100:130] = float("-inf")
    return bias


def _ref_rows(refs, q, bias, out_dtype, order=None):
    """row b: the reference cache of slot b's sequence attends alone (host lengths, B = 1); an empty one gives zeros"""
    rows = []
    for slot in range(q.shape[0]):
        r = refs[slot if order is None else order[slot]]
        if r.len == 0:
            rows.append(torch.zeros(1, q.shape[1], q.shape[2], dtype=out_dtype or q.dtype, device=q.device))
        else:
            rows.append(r.attend(q[slot:slot + 1], None if bias is None else bias[slot:slot + 1, :r.len].contiguous(), out_dtype=out_dtype))
    return torch.cat(rows, dim=0)


# ---------------------------------------------------------------------------------------------------------------------
# 1. ragged attention
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("Hq", [4, 16])
@pytest.mark.parametrize("D", [64, 128])
def test_ragged_attention_equals_every_slots_own_cache(msq, D, Hq, dtype, fmt):
    kp = msq.kvpacked
    assert kp.attn_plan_cap(B, Hq, HKV, D, MAX_LEN, GAP)[0] == 3 and [kp.attn_plan(1, Hq, HKV, D, s, 0)[0] for s in (96, 160, 256)] == [1, 2, 2]
    for ti, lens in enumerate(TRIPLES):
        sl, refs = _fill(kp, lens, D, dtype, fmt, 1000 * ti + D)
        q = _rand((B, Hq, D), 77 + ti, dtype).to(dev())
        for bias in (None, _bias()):
            for od in (torch.float32, None):
                got, want = sl.attend_dev(q, bias, out_dtype=od), _ref_rows(refs, q, bias, od)
                assert got.dtype == want.dtype and torch.equal(got, want), (lens, "bias" if bias is not None else "-", od)
        for b, (p, t) in enumerate(lens):
            if p + t == 0:
                assert bool((sl.attend_dev(q, out_dtype=torch.float32)[b] == 0).all()), "the empty slot gives zeros"


def test_ragged_attention_against_float64(msq):
    """the middle triple once more against float64 attention over dequantize(slot).double(), with the bound of test_gpu_f3_kv_packed.py:
    4 x the error of torch's float32 math-backend SDPA on the same tensors, floor 2^-20 max|ref|"""
    from torch.nn.attention import SDPBackend, sdpa_kernel
    kp = msq.kvpacked
    D, Hq, G = 128, 16, 16 // HKV
    sl, _ = _fill(kp, TRIPLES[1], D, torch.float16, "fp8_e4m3", 4242)
    q = _rand((B, Hq, D), 78, torch.float16).to(dev())
    out = sl.attend_dev(q, out_dtype=torch.float32)
    for b in range(B):
        kd, vd = sl.dequantize(b)
        assert kd.shape[2] == sum(TRIPLES[1][b])
        k64, v64 = kd.double().repeat_interleave(G, dim=1), vd.double().repeat_interleave(G, dim=1)
        ref = torch.einsum("bhs,bhsd->bhd", torch.softmax(torch.einsum("bhd,bhsd->bhs", q[b:b + 1].double(), k64) * D ** -0.5, dim=2), v64)
        with sdpa_kernel(SDPBackend.MATH):
            th = torch.nn.functional.scaled_dot_product_attention(q[b:b + 1].float()[:, :, None, :], k64.float(), v64.float(), scale=D ** -0.5)[:, :, 0, :]
        err, err_t = float((out[b:b + 1].double() - ref).abs().max()), float((th.double() - ref).abs().max())
        floor = 2.0 ** -20 * float(ref.abs().max())
        print("slot %d len %3d: err %.3e torch %.3e floor %.3e" % (b, kd.shape[2], err, err_t, floor))
        assert err <= max(4 * err_t, floor), (b, err, err_t, floor)


# ---------------------------------------------------------------------------------------------------------------------
# 2. - 4. one captured step: replays, slot reuse, idle
# ---------------------------------------------------------------------------------------------------------------------
class _Step:
    """slots at 20, 95 and 150 tokens and ONE HIP graph of append + attend_dev (one stream, a linear chain); replay(i) feeds token i of every
    live sequence to the graph and to the references' eager step and compares every live slot's output row"""

    def __init__(self, kp, D, Hq, dtype, fmt, sentinel=False, steps=60):
        self.kp, self.D, self.Hq, self.dtype, self.fmt = kp, D, Hq, dtype, fmt
        starts = (20, 95, 150)
        self.sl = kp.SlotPackedKV(B, HKV, D, dtype, fmt, gap=GAP, max_len=MAX_LEN, device=dev())
        if sentinel:
            for t in self.sl.planes.values():
                t.fill_(0xA5)
        self.refs, self.K, self.V, self.at = [], [], [], []
        for b, n in enumerate(starts):
            self._new_sequence(b, n, steps, 500 + b)
        self.Q = _rand((steps, B, Hq, D), 599, dtype).to(dev())
        self.k_in = torch.zeros(B, HKV, 1, D, dtype=dtype, device=dev())
        self.v_in, self.q_in = torch.zeros_like(self.k_in), torch.zeros(B, Hq, D, dtype=dtype, device=dev())
        self.live = [True] * B
        before = self.sl.lengths
        self.sl.append(self.k_in, self.v_in)                     # one eager step allocates the workspace ...
        self.sl.attend_dev(self.q_in)
        for b, (p, t) in enumerate(before):
            self.sl.set_lengths(b, p, t)                         # ... and is undone: its token sits in a tail slot the first real step overwrites
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.sl.append(self.k_in, self.v_in)
            self.y = self.sl.attend_dev(self.q_in)
        for b, (p, t) in enumerate(before):
            self.sl.set_lengths(b, p, t)                         # capturing ran the Python (the mirror moved), not the kernels
        self.i = 0

    def _new_sequence(self, b, n, steps, seed):
        K, V = (_rand((1, HKV, n + steps, self.D), seed + 50 * i, self.dtype).to(dev()) for i in range(2))
        ref = self.kp.PackedKV(1, HKV, self.D, self.dtype, self.fmt, gap=GAP, capacity=32, device=dev())
        ref.append(K[:, :, :n], V[:, :, :n])
        self.sl.prefill(b, K[:, :, :n], V[:, :, :n])
        if b < len(self.refs):
            self.refs[b], self.K[b], self.V[b], self.at[b] = ref, K, V, n
        else:
            self.refs.append(ref); self.K.append(K); self.V.append(V); self.at.append(n)

    def replay(self, n=1):
        for _ in range(n):
            for b in range(B):
                if self.live[b]:
                    self.k_in[b].copy_(self.K[b][0, :, self.at[b]:self.at[b] + 1]); self.v_in[b].copy_(self.V[b][0, :, self.at[b]:self.at[b] + 1])
            self.q_in.copy_(self.Q[self.i])
            self.graph.replay()
            self.sl.advance_host(1)
            for b in range(B):
                if not self.live[b]:
                    assert bool((self.y[b] == 0).all()), ("an idle slot's rows are zeros", self.i, b)
                    continue
                r, a = self.refs[b], self.at[b]
                r.append(self.K[b][:, :, a:a + 1], self.V[b][:, :, a:a + 1])
                self.at[b] += 1
                want = r.attend(self.Q[self.i][b:b + 1])
                assert torch.equal(self.y[b:b + 1], want), ("replay", self.i, "slot", b, "len", r.len, float((self.y[b:b + 1].float() - want.float()).abs().max()))
                assert self.sl.lengths[b] == (r.packed_len, r.tail_len), (self.i, b)
            self.i += 1

    def same_bytes(self, b):
        r, sl = self.refs[b], self.sl
        P = r.packed_len
        for n in ("k_codes", "v_codes", "v_scales"):
            assert torch.equal(sl.planes[n][b:b + 1, :, :P], r.planes[n][:, :, :P]), (b, n)
        assert torch.equal(sl.planes["k_scales"][b:b + 1, :, :P // 32], r.planes["k_scales"][:, :, :P // 32]), b
        assert torch.equal(sl.k_tail[b:b + 1, :, :r.tail_len], r.k_tail[:, :, :r.tail_len]) and torch.equal(sl.v_tail[b:b + 1, :, :r.tail_len], r.v_tail[:, :, :r.tail_len]), b


@pytest.mark.parametrize("D,Hq,dtype,fmt", [(64, 4, torch.float16, "fp8_e4m3"), (128, 16, torch.bfloat16, "fp4_e2m1"),
                                            (64, 16, torch.bfloat16, "fp8_e4m3"), (128, 4, torch.float16, "fp4_e2m1")],
                         ids=["64-4-f16-fp8", "128-16-bf16-fp4", "64-16-bf16-fp8", "128-4-f16-fp4"])
def test_captured_step_replays_over_slots_that_flush_at_different_steps(msq, D, Hq, dtype, fmt):
    kp = msq.kvpacked
    s = _Step(kp, D, Hq, dtype, fmt)
    s.replay(50)
    assert s.sl.lengths == [(64, 6), (128, 17), (192, 8)]        # flushes at replays 13 / 45, 2 / 34 and 11 / 43; slot 2 went from 1 split to 2
    assert kp.attn_plan(1, Hq, HKV, D, 128, 0)[0] == 1 and kp.attn_plan(1, Hq, HKV, D, 160, 0)[0] == 2
    assert s.sl.sync() == [(64, 6), (128, 17), (192, 8)] and s.sl.state.tolist() == [[64, 6, 0, 0], [128, 17, 0, 0], [192, 8, 0, 0]]
    for b in range(B):
        s.same_bytes(b)
        assert torch.equal(s.sl.k_tail[b:b + 1], s.refs[b].k_tail) and torch.equal(s.sl.v_tail[b:b + 1], s.refs[b].v_tail), b


def test_slot_reuse_under_the_same_graph(msq):
    s = _Step(msq.kvpacked, 128, 16, torch.float16, "fp8_e4m3", sentinel=True)
    sl = s.sl
    s.replay(10)
    assert sl.lengths == [(0, 30), (96, 9), (128, 32)]
    before = {n: t.clone() for n, t in sl.planes.items()}
    tails = (sl.k_tail.clone(), sl.v_tail.clone())
    rows = sl.state.clone()
    sl.reset(1)
    assert sl.state.tolist()[1] == [0, 0, 0, 0]
    s._new_sequence(1, 70, 60, 900)                              # a fresh reference, and prefill(1, ...) of the new 70-token prompt, eagerly
    assert sl.lengths[1] == (64, 6) and sl.state.tolist() == [rows[0].tolist(), [64, 6, 0, 0], rows[2].tolist()]
    for n in PLANES:
        g = 32 if n == "k_scales" else 1
        assert torch.equal(sl.planes[n][0], before[n][0]) and torch.equal(sl.planes[n][2], before[n][2]), n       # slots 0 and 2: every byte
        assert torch.equal(sl.planes[n][1, :, 64 // g:], before[n][1, :, 64 // g:]), n                            # slot 1 beyond its new length
        assert bool((sl.planes[n][1, :, 96 // g:] == 0xA5).all()), n                                              # ... the sentinel no one has written
        assert not torch.equal(sl.planes[n][1, :, :64 // g], before[n][1, :, :64 // g]), n
    for t, t0 in zip((sl.k_tail, sl.v_tail), tails):
        assert torch.equal(t[0], t0[0]) and torch.equal(t[2], t0[2]) and torch.equal(t[1, :, 6:], t0[1, :, 6:])
    s.replay(20)                                                 # the SAME graph
    assert sl.lengths == [(32, 18), (64, 26), (160, 20)] and sl.sync() == sl.lengths
    for b in range(B):
        s.same_bytes(b)


def test_idle_slot_is_left_alone_and_resumes(msq):
    s = _Step(msq.kvpacked, 64, 4, torch.bfloat16, "fp4_e2m1")
    sl = s.sl
    s.replay(1)                                                  # slot 1: 64 + 32, a full tail: the next token would flush it
    assert sl.lengths[1] == (64, 32)
    sl.set_idle(1)
    s.live[1] = False
    before = {n: t[1].clone() for n, t in sl.planes.items()}
    tails = (sl.k_tail[1].clone(), sl.v_tail[1].clone())
    s.replay(5)                                                  # checks that slot 1's output rows are zeros and that the others advance
    assert sl.state.tolist() == [[0, 26, 0, 0], [64, 32, 0, IDLE], [128, 28, 0, 0]] and sl.lengths[1] == (64, 32)
    for n in PLANES:
        assert torch.equal(sl.planes[n][1], before[n]), n
    assert torch.equal(sl.k_tail[1], tails[0]) and torch.equal(sl.v_tail[1], tails[1])
    sl.set_idle(1, False)
    s.live[1] = True
    s.replay(3)                                                  # slot 1 resumes from where it stood: the flush first
    assert sl.sync() == [(0, 29), (96, 3), (128, 31)]
    for b in range(B):
        s.same_bytes(b)


# ---------------------------------------------------------------------------------------------------------------------
# 5. - 7. overflow of one slot, status per slot, crop
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
def test_overflow_of_one_slot_leaves_it_alone_and_the_others_advance(msq, fmt):
    kp, D = msq.kvpacked, 64
    sl, refs = _fill(kp, ((64, 32), (0, 5), (32, 1)), D, torch.bfloat16, fmt, 3100, max_len=64)
    assert sl.S_cap == 64
    k, v = (_rand((B, HKV, 1, D), 3200 + i, torch.bfloat16).to(dev()) for i in range(2))
    before = {n: t.clone() for n, t in sl.planes.items()}
    tails = (sl.k_tail.clone(), sl.v_tail.clone())
    sl.append(k, v)                                              # the C entry: two live slots have room, so the mirror does not refuse
    assert sl.state.tolist() == [[64, 32, OVERFLOW, 0], [0, 6, 0, 0], [32, 2, 0, 0]]
    assert sl.lengths == [(64, 32), (0, 6), (32, 2)]
    for n, t in before.items():
        assert torch.equal(sl.planes[n], t), n                   # no slot flushed, and the full one was not touched
    assert torch.equal(sl.k_tail[0], tails[0][0]) and torch.equal(sl.v_tail[0], tails[1][0])
    assert torch.equal(sl.k_tail[1, :, 5:6], k[1]) and torch.equal(sl.v_tail[2, :, 1:2], v[2])
    for b in (1, 2):
        refs[b].append(k[b:b + 1], v[b:b + 1])
    q = _rand((B, 4, D), 3300, torch.bfloat16).to(dev())
    assert torch.equal(sl.attend_dev(q), _ref_rows(refs, q, None, None))          # the full slot still attends over what it holds
    with pytest.raises(msq._lib.MsqError, match=r"slot 0: MSQ_STATUS_OVERFLOW"):
        sl.sync()
    assert sl.sync(raise_on_status=False) == ([(64, 32), (0, 6), (32, 2)], [OVERFLOW, 0, 0])
    sl.reset(0)
    assert sl.state.tolist()[0] == [0, 0, 0, 0] and sl.sync() == [(0, 0), (0, 6), (32, 2)]


def test_planted_inf_raises_status_nan_in_its_own_slot_only(msq):
    kp, D = msq.kvpacked, 64
    sl = kp.SlotPackedKV(B, HKV, D, torch.float16, "fp8_e4m3", gap=GAP, max_len=64, device=dev())
    K, V = _rand((B, HKV, 33, D), 3400, torch.float16), _rand((B, HKV, 33, D), 3401, torch.float16)
    K[1, 0, 7, 33] = float("inf")
    K, V = K.to(dev()), V.to(dev())
    for b in range(B):
        sl.prefill(b, K[b:b + 1, :, :31], V[b:b + 1, :, :31])
    sl.append(K[:, :, 31:32], V[:, :, 31:32])
    assert sl.state.tolist() == [[0, 32, 0, 0]] * 3              # in the tail an Inf is just a value
    sl.append(K[:, :, 32:33], V[:, :, 32:33])                    # every slot flushes; slot 1 packs the Inf
    assert sl.state.tolist() == [[32, 1, 0, 0], [32, 1, NAN, 0], [32, 1, 0, 0]]
    with pytest.raises(msq._lib.MsqError, match=r"slot 1: MSQ_STATUS_NAN"):
        sl.sync()


def test_crop_one_slot_keeps_its_bits_and_the_others_bytes(msq):
    kp, D = msq.kvpacked, 128
    sl, _ = _fill(kp, ((96, 4), (64, 6), (32, 8)), D, torch.float16, "fp4_e2m1", 3500)
    k0, v0 = sl.dequantize(1)
    assert tuple(k0.shape) == (1, HKV, 70, D)
    others = {n: t.clone() for n, t in sl.planes.items()}
    tails, rows = (sl.k_tail.clone(), sl.v_tail.clone()), sl.state.clone()
    for n, want in ((66, (64, 2)), (50, (32, 18)), (32, (32, 0))):           # into the tail, into the packed part, onto a group boundary
        sl.crop(1, n)
        assert sl.lengths[1] == want and sl.state.tolist()[1] == [want[0], want[1], 0, 0]
        k, v = sl.dequantize(1)
        assert torch.equal(k, k0[:, :, :n]) and torch.equal(v, v0[:, :, :n]), n
        for b in (0, 2):
            assert sl.state.tolist()[b] == rows[b].tolist()
            for name, t in others.items():
                assert torch.equal(sl.planes[name][b], t[b]), (n, b, name)
            assert torch.equal(sl.k_tail[b], tails[0][b]) and torch.equal(sl.v_tail[b], tails[1][b])
    with pytest.raises(msq._lib.MsqError):
        sl.crop(1, 33)


# ---------------------------------------------------------------------------------------------------------------------
# 8. repeatability
# ---------------------------------------------------------------------------------------------------------------------
def test_repeated_runs_and_permuted_slots_give_identical_bits(msq):
    kp, D, Hq = msq.kvpacked, 128, 16
    sl, _ = _fill(kp, TRIPLES[1], D, torch.bfloat16, "fp8_e4m3", 3600)
    q = _rand((B, Hq, D), 3601, torch.bfloat16).to(dev())
    bias = _bias()
    first = sl.attend_dev(q, bias, out_dtype=torch.float32).clone()
    for _ in range(19):
        assert torch.equal(sl.attend_dev(q, bias, out_dtype=torch.float32), first)
    order = [2, 0, 1]                                            # the same three sequences in other slots
    perm, _ = _fill(kp, TRIPLES[1], D, torch.bfloat16, "fp8_e4m3", 3600, order=order)
    assert perm.lengths == [TRIPLES[1][s] for s in order]
    got = perm.attend_dev(q[order].contiguous(), bias[order].contiguous(), out_dtype=torch.float32)
    assert torch.equal(got, first[order])
