"""Packed MX KV cache with a state row per sequence, host side (no GPU): the argument checks of msq_kv_mx_append_seq /
msq_kv_mx_attn_decode_seq that come back before any launch, and the per-slot host mirror of msq.kvpacked.SlotPackedKV on a stub whose "device"
is a list of rows moved by the rule of include/msq.h (as in test_kv_packed_static_host.py)."""
import pytest
import torch

from kv_packed_stubs import _msq, _tokens, dynamic_stub as _dynamic_stub

FP8, FP4 = 5, 8
BAD_ARG, UNSUPPORTED = -1, -2
PTR = 4096                                                       # a non-null, 16-byte aligned "pointer" for entries that return before they look
OVERFLOW, NAN, IDLE = 8, 1, 1


def test_append_seq_and_decode_seq_argument_errors():
    lib = _msq()._lib.lib()
    app = lambda **kw: lib.msq_kv_mx_append_seq(*[kw.get(k, d) for k, d in (
        ("k", None), ("v", None), ("dtype", 1), ("kc", None), ("ks", None), ("vc", None), ("vs", None), ("S_cap", 128), ("kt", None), ("vt", None),
        ("tail_cap", 32), ("state", PTR), ("B", 3), ("H", 2), ("D", 64), ("fmt", FP8), ("stream", None))])
    full = dict(k=PTR, v=PTR, kc=PTR, ks=PTR, vc=PTR, vs=PTR, kt=PTR, vt=PTR)
    assert app(state=None) == BAD_ARG and b"msq_kv_mx_append_seq: null state" in lib.msq_last_error()
    assert app(state=PTR + 4, **full) == BAD_ARG and b"aligned" in lib.msq_last_error()              # a misaligned state
    assert app(S_cap=100) == BAD_ARG and b"S_cap" in lib.msq_last_error()
    assert app(S_cap=0) == BAD_ARG
    assert app(tail_cap=48) == BAD_ARG and b"tail_cap" in lib.msq_last_error()
    assert app(tail_cap=0) == BAD_ARG
    assert app(D=48) == UNSUPPORTED and app(D=288) == UNSUPPORTED and b"head_dim" in lib.msq_last_error()
    assert app(dtype=0) == UNSUPPORTED and app(dtype=3) == UNSUPPORTED           # the tail is f16 or bf16
    assert app(fmt=6) == UNSUPPORTED
    assert app(B=0) == BAD_ARG
    assert app(B=65536) == UNSUPPORTED and b"slots" in lib.msq_last_error()      # the slot is a grid axis
    assert app() == BAD_ARG and b"null buffer" in lib.msq_last_error()
    assert app(**dict(full, vt=PTR + 8)) == BAD_ARG and b"aligned" in lib.msq_last_error()

    dec = lambda **kw: lib.msq_kv_mx_attn_decode_seq(*[kw.get(k, d) for k, d in (
        ("q", None), ("q_dtype", 1), ("kc", None), ("ks", None), ("vc", None), ("vs", None), ("S_cap", 128), ("kt", None), ("vt", None),
        ("tail_cap", 32), ("state", PTR), ("bias", None), ("bias_stride", 0), ("out", None), ("out_dtype", 0), ("B", 3), ("Hq", 8), ("Hkv", 2),
        ("D", 128), ("fmt", FP8), ("scaling", 0.125), ("ws", None), ("ws_bytes", 1 << 24), ("stream", None))])
    bufs = dict(q=PTR, out=PTR, ws=PTR, kt=PTR, vt=PTR, kc=PTR, ks=PTR, vc=PTR, vs=PTR)
    assert dec(state=None) == BAD_ARG and b"msq_kv_mx_attn_decode_seq: null state" in lib.msq_last_error()
    assert dec(state=PTR + 8, **bufs) == BAD_ARG and b"aligned" in lib.msq_last_error()
    assert dec(bias=PTR, bias_stride=159) == BAD_ARG and b"bias_stride" in lib.msq_last_error()      # < S_cap + tail_cap
    assert dec(bias=PTR, bias_stride=160) == BAD_ARG and b"null buffer" in lib.msq_last_error()      # wide enough: on to the buffers
    assert dec(S_cap=100) == BAD_ARG and b"S_cap" in lib.msq_last_error()
    assert dec(tail_cap=40) == BAD_ARG and b"tail_cap" in lib.msq_last_error()
    assert dec(D=48) == UNSUPPORTED and b"head_dim" in lib.msq_last_error()
    assert dec(Hq=32) == UNSUPPORTED                                             # 16 query heads per kv head
    assert dec(Hq=9) == BAD_ARG
    assert dec(fmt=6) == UNSUPPORTED and dec(q_dtype=0) == UNSUPPORTED and dec(out_dtype=2) == UNSUPPORTED
    assert dec(ws_bytes=3 * 8 * 1 * 130 * 4 - 1, **bufs) == BAD_ARG and b"workspace" in lib.msq_last_error()     # plan_cap's size, less one byte
    assert dec() == BAD_ARG and b"null buffer" in lib.msq_last_error()
    # the entries the bodies are shared with still speak under their own names
    assert lib.msq_kv_mx_append_dev(None, None, 1, None, None, None, None, 128, None, None, 32, None, 2, 2, 64, FP8, None) == BAD_ARG
    assert b"msq_kv_mx_append_dev: null state" in lib.msq_last_error()


# ---------------------------------------------------------------------------------------------------------------------
# the per-slot mirror, on stubs
# ---------------------------------------------------------------------------------------------------------------------
def _slot_stub(B, gap, max_len):
    kp = _msq().kvpacked

    class View(kp._SlotView):
        def __init__(self, owner, slot):
            super().__init__(owner, slot)
            self.owner, self.slot = owner, slot

        def _check_kv(self, k, v):
            pass

        def _pack(self, k, v, pos):
            assert k.shape[0] == 1 and k.shape[2] % 32 == 0 and pos % 32 == 0 and pos + k.shape[2] <= self.capacity
            self.owner.log[self.slot].append((pos, k[0, 0, :, 0].tolist()))

    class Stub(kp.SlotPackedKV):
        """storage on the host; the device state is a list of rows that _append_dev moves by the rule of include/msq.h, per slot"""
        _VIEW = View

        def _check_device(self):
            pass

        def _alloc_planes(self):
            self.planes, self.capacity = {}, self.S_cap

        def _alloc_state(self):
            self.dev = [[0, 0, 0, 0] for _ in range(self.B)]
            self.writes, self.launches, self.capturing = [0] * self.B, 0, False

        def _write_row(self, slot, what):
            p, t = self._lens[slot]
            flags = IDLE if self._idle[slot] else 0
            if what == "lengths":
                self.dev[slot][:2] = [p, t]
            elif what == "flags":
                self.dev[slot][3] = flags
            else:
                self.dev[slot] = [p, t, 0, flags]
            self.writes[slot] += 1

        def _read_state(self):
            return [list(r) for r in self.dev]

        def _capturing(self):
            return self.capturing

        def _check_kv(self, k, v):
            pass

        def _append_dev(self, k, v):
            self.launches += 1
            for b, row in enumerate(self.dev):
                p, t = row[:2]
                if row[3] & IDLE:
                    continue
                if t == self.gap:
                    if p + self.gap > self.S_cap:
                        row[2] |= OVERFLOW
                        continue
                    self.log[b].append((p, self.k_tail[b, 0, :, 0].tolist()))
                    p, t = p + self.gap, 0
                self.k_tail[b, :, t:t + 1] = k[b]
                self.v_tail[b, :, t:t + 1] = v[b]
                row[:2] = [p, t + 1]

    s = Stub(B, 1, 32, torch.float16, "fp8_e4m3", gap=gap, max_len=max_len, device="cpu")
    s.log = [[] for _ in range(B)]
    return s


def _step_tokens(values):
    """one token per slot, slot b's holding values[b]"""
    t = torch.tensor(values, dtype=torch.float16).reshape(-1, 1, 1, 1).expand(len(values), 1, 1, 32).contiguous()
    return t, t.clone()


@pytest.mark.parametrize("gap", [32, 64])
def test_per_slot_mirror_follows_independent_dynamic_caches(gap):
    starts = (0, 1, gap - 1, 2 * gap + 7)                        # different starting lengths: the slots flush at different steps
    B = len(starts)
    sl = _slot_stub(B, gap, 8 * gap)
    dyn = [_dynamic_stub(gap) for _ in starts]
    for b, p in enumerate(starts):
        if p:
            sl.prefill(b, *_tokens(1000 * b, 1000 * b + p))
            dyn[b].append(*_tokens(1000 * b, 1000 * b + p))
    assert sl.writes == [int(p > 0) for p in starts] and sl.launches == 0         # one state-row write per prefilled slot, no launch
    assert sl.lengths == [(d.packed_len, d.tail_len) for d in dyn] == [(p - p % gap, p % gap) for p in starts]
    for i in range(100):
        sl.append(*_step_tokens([1000 * b + starts[b] + i for b in range(B)]))
        for b, d in enumerate(dyn):
            d.append(*_tokens(1000 * b + starts[b] + i, 1000 * b + starts[b] + i + 1))
        assert sl.lengths == [(d.packed_len, d.tail_len) for d in dyn], (gap, i)
        assert [r[:3] for r in sl.dev] == [[p, t, 0] for p, t in sl.lengths], (gap, i)    # the mirror never left the device's side of the rule
    assert sl.launches == 100
    for b, d in enumerate(dyn):
        assert sl.log[b] == d.log, b                             # every slot packed what its own dynamic cache packed, where it did
        assert sl.k_tail[b, 0, :d.tail_len, 0].tolist() == d.k_tail[0, 0, :d.tail_len, 0].tolist()
    adv = _slot_stub(B, gap, 8 * gap)
    for b, p in enumerate(starts):
        adv.set_lengths(b, p - p % gap, p % gap)
    adv.advance_host(100)                                        # 100 replays later: the same lengths, in one step and without a launch
    adv.advance_host(0)
    assert adv.lengths == sl.lengths and adv.launches == 0
    assert sl.sync() == sl.lengths == [(d.packed_len, d.tail_len) for d in dyn]


def test_prefill_reset_and_idle_touch_one_slot():
    sl = _slot_stub(3, 32, 128)
    sl.prefill(1, *_tokens(0, 70))
    assert sl.lengths == [(0, 0), (64, 6), (0, 0)] and sl.dev == [[0, 0, 0, 0], [64, 6, 0, 0], [0, 0, 0, 0]]
    assert sl.log == [[], [(0, [float(i) for i in range(64)])], []]
    assert sl.k_tail[1, 0, :6, 0].tolist() == [64.0, 65.0, 66.0, 67.0, 68.0, 69.0] and not sl.k_tail[0].any() and not sl.k_tail[2].any()
    sl.prefill(1, *_tokens(70, 100))                             # a second prompt chunk joins the tail first: the timing rule of PackedKV.append
    assert sl.lengths[1] == (96, 4) and sl.log[1][1] == (64, [float(i) for i in range(64, 96)])
    sl.dev[1][2] = NAN
    sl.set_idle(1)
    assert sl.dev[1] == [96, 4, NAN, IDLE]                       # the flag alone is written
    sl.append(*_step_tokens([1, 2, 3]))
    sl.advance_host(3)                                           # ... and advance_host skips the idle slot too
    assert sl.lengths == [(0, 4), (96, 4), (0, 4)] and sl.dev[1] == [96, 4, NAN, IDLE] and sl.dev[0][:2] == [0, 1]
    sl.set_idle(1, False)
    assert sl.dev[1] == [96, 4, NAN, 0]
    lengths, statuses = sl.sync(raise_on_status=False)
    assert statuses == [0, NAN, 0] and lengths == [(0, 1), (96, 4), (0, 1)]
    with pytest.raises(_msq()._lib.MsqError, match=r"slot 1: MSQ_STATUS_NAN"):
        sl.sync()
    sl.set_idle(2)
    sl.reset(1)
    sl.reset(2)                                                  # lengths 0, status 0, not idle
    assert sl.dev[1] == [0, 0, 0, 0] and sl.dev[2] == [0, 0, 0, 0] and sl.lengths == [(0, 1), (0, 0), (0, 0)] and sl.sync() == sl.lengths
    Err = _msq()._lib.MsqError
    for bad in (-1, 3):
        with pytest.raises(Err, match="slot"):
            sl.reset(bad)
    with pytest.raises(Err):
        sl.prefill(0, *_tokens(0, 32 * 5))                       # 160 packed tokens into a slot of 128
    assert sl.lengths[0] == (0, 1) and sl.dev[0][:2] == [0, 1]


def test_crop_one_slot():
    sl = _slot_stub(2, 32, 128)
    sl.prefill(0, *_tokens(0, 70))
    sl.prefill(1, *_tokens(0, 40))
    sl.crop(0, 66)
    assert sl.lengths == [(64, 2), (32, 8)] and sl.dev[0][:2] == [64, 2] and sl.writes == [2, 1]
    with pytest.raises(_msq()._lib.MsqError):
        sl.crop(1, 41)
    assert sl.lengths[1] == (32, 8)


@pytest.mark.parametrize("gap", [32, 64])
def test_one_full_slot_does_not_stop_the_others_and_all_full_is_refused(gap):
    Err = _msq()._lib.MsqError
    sl = _slot_stub(3, gap, 2 * gap)
    sl.prefill(0, *_tokens(0, 3 * gap - 1))
    sl.append(*_step_tokens([7, 8, 9]))                          # slot 0's tail fills up: 2 gap packed + a full tail is all it holds
    assert sl.lengths == [(2 * gap, gap), (0, 1), (0, 1)] and sl.launches == 1
    sl.append(*_step_tokens([7, 8, 9]))                          # slot 0 overflows: launched all the same, its mirror stays, the others move
    assert sl.launches == 2 and sl.lengths == [(2 * gap, gap), (0, 2), (0, 2)]
    assert sl.dev == [[2 * gap, gap, OVERFLOW, 0], [0, 2, 0, 0], [0, 2, 0, 0]]
    with pytest.raises(Err, match=r"slot 0: MSQ_STATUS_OVERFLOW"):
        sl.sync()
    assert sl.sync(raise_on_status=False) == ([(2 * gap, gap), (0, 2), (0, 2)], [OVERFLOW, 0, 0])
    sl.advance_host(5)                                           # the full slot stays where the device leaves it
    assert sl.lengths == [(2 * gap, gap), (0, 7), (0, 7)]
    sl.set_lengths(1, 0, 2)
    sl.set_lengths(2, 0, 2)
    sl.set_idle(1)
    sl.set_idle(2)                                               # the only live slot is the full one: refused before any launch
    with pytest.raises(Err, match="overflow"):
        sl.append(*_step_tokens([7, 8, 9]))
    with pytest.raises(Err, match="overflow"):
        sl.advance_host(1)
    assert sl.launches == 2 and sl.lengths == [(2 * gap, gap), (0, 2), (0, 2)]
    sl.reset(0)                                                  # the server retires the one full slot: its status is cleared
    assert sl.dev[0] == [0, 0, 0, 0] and sl.sync() == [(0, 0), (0, 2), (0, 2)]
    sl.append(*_step_tokens([7, 8, 9]))
    assert sl.lengths == [(0, 1), (0, 2), (0, 2)] and sl.launches == 3
    sl.set_idle(0)                                               # every slot idle: nothing is live, nothing overflows, the launch is a no-op
    sl.append(*_step_tokens([7, 8, 9]))
    assert sl.lengths == [(0, 1), (0, 2), (0, 2)] and [r[:2] for r in sl.dev] == [[0, 1], [0, 2], [0, 2]]
    # advance_host stops a slot exactly where the device does: 3 gap tokens fit
    a = _slot_stub(2, gap, 2 * gap)
    a.set_lengths(1, gap, 5)
    a.advance_host(3 * gap)
    assert a.lengths == [(2 * gap, gap), (2 * gap, gap)]


def test_capture_time_refusals_and_the_names_that_are_not_offered():
    msq = _msq()
    Err = msq._lib.MsqError
    sl = _slot_stub(2, 32, 128)
    sl.prefill(0, *_tokens(0, 40))
    sl.capturing = True
    for call in (lambda: sl.prefill(1, *_tokens(0, 8)), lambda: sl.reset(0), lambda: sl.set_idle(0), lambda: sl.crop(0, 3),
                 lambda: sl.set_lengths(0, 0, 0)):
        with pytest.raises(Err, match="captur"):
            call()
    sl.append(*_step_tokens([1, 2]))                             # the single-token step is the captured path
    assert sl.lengths == [(32, 9), (0, 1)] and sl.writes == [1, 0]
    with pytest.raises(Err, match="eager"):
        sl.attend_dev(_FakeCuda(2, 4, 32))                       # no workspace yet: it would have to be allocated during capture
    sl.capturing = False
    with pytest.raises(Err, match="one token per slot"):
        sl.append(torch.zeros(2, 1, 4, 32, dtype=torch.float16), torch.zeros(2, 1, 4, 32, dtype=torch.float16))
    for name in ("attend", "attend_multi", "update", "get_seq_length"):
        with pytest.raises(Err, match="one shared host length, and transformers batches by left padding"):
            getattr(sl, name)(torch.zeros(2, 4, 32))
    with pytest.raises(Err, match="per slot"):
        sl.len
    assert msq.SlotPackedKV is msq.kvpacked.SlotPackedKV and issubclass(msq.SlotPackedKV, msq.kvpacked.StaticPackedKV)


class _FakeCuda(torch.Tensor):
    """a CPU tensor that claims to live on the device: attend_dev's checks in front of the workspace run without one"""
    @staticmethod
    def __new__(cls, *shape):
        return torch.Tensor._make_subclass(cls, torch.zeros(*shape, dtype=torch.float16))

    is_cuda = True


def test_workspace_is_plan_caps_and_cpu_tensors_are_refused():
    msq = _msq()
    kp, Err = msq.kvpacked, msq._lib.MsqError
    with pytest.raises(Err):
        kp.SlotPackedKV(2, 2, 64, torch.float16, max_len=64, device="cpu")
    sl = _slot_stub(3, 32, 288)
    with pytest.raises(Err):
        sl.attend_dev(torch.zeros(3, 4, 32, dtype=torch.float16))                 # a CPU tensor
    with pytest.raises(Err, match="W >= 320"):
        sl.attend_dev(torch.zeros(3, 4, 32, dtype=torch.float16), bias=torch.zeros(3, 319))
    # the workspace the class allocates is plan_cap's: B Hq max_splits (D + 2) floats, 3 splits of 128 tokens at 288
    ms, wb = kp.attn_plan_cap(3, 16, 2, 128, 288, 32)
    assert (ms, wb) == (3, 3 * 16 * 3 * 130 * 4) and kp.attn_plan(3, 16, 2, 128, 288, 0)[:2] == (3, 128)
    assert [kp.attn_plan(1, 16, 2, 128, s, 0)[0] for s in (96, 160, 256)] == [1, 2, 2]
    lib = msq._lib.lib()
    args = [PTR, 1, PTR, PTR, PTR, PTR, 288, PTR, PTR, 32, PTR, None, 0, PTR, 0, 3, 16, 2, 128, FP8, 0.125, PTR]
    assert lib.msq_kv_mx_attn_decode_seq(*args, wb - 1, None) == BAD_ARG and b"workspace" in lib.msq_last_error()
