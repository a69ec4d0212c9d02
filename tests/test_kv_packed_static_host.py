"""Packed MX KV cache with the lengths on the device, host side (no GPU): msq_kv_mx_attn_plan_cap against the per-length
plan, the argument checks of the three new C entries that come back before any launch (null buffers, as in test_kv_packed_host.py), and the
host mirror of msq.kvpacked.StaticPackedKV on a stub that records packs and device appends instead of launching them."""
import ctypes as C

import pytest
import torch

from kv_packed_stubs import _msq, _tokens, dynamic_stub as _dynamic_stub, static_stub as _static_stub

FP8, FP4 = 5, 8
BAD_ARG, UNSUPPORTED = -1, -2
PTR = 4096                                                       # a non-null, 16-byte aligned "pointer" for entries that return before they look


def _plan_splits(lib, B, Hq, Hkv, D, S):
    ns = C.c_int(-1)
    assert lib.msq_kv_mx_attn_plan(B, Hq, Hkv, D, S, 0 if S else 1, C.byref(ns), None, None) == 0
    return ns.value


def _plan_cap(lib, B, Hq, Hkv, D, S_cap, tail_cap):
    ms, wb = C.c_int(-1), C.c_int64(-1)
    rc = lib.msq_kv_mx_attn_plan_cap(B, Hq, Hkv, D, S_cap, tail_cap, C.byref(ms), C.byref(wb))
    return rc, ms.value, wb.value


def test_plan_cap_is_the_largest_plan_up_to_the_capacity():
    lib = _msq()._lib.lib()
    B, Hq, Hkv, D = 2, 8, 2, 128
    running, seen = _plan_splits(lib, B, Hq, Hkv, D, 0), set()
    dips = 0
    for S_cap in range(32, 16384 + 1, 32):
        ns = _plan_splits(lib, B, Hq, Hkv, D, S_cap)
        dips += ns < running                                     # n_splits is not monotone: plan(S_cap) alone would be too small
        running = max(running, ns)                               # max over every S <= S_cap, so >= each of them with equality for one
        rc, ms, wb = _plan_cap(lib, B, Hq, Hkv, D, S_cap, 32)
        assert rc == 0 and ms == running and ms <= 64, (S_cap, ms, running)
        assert wb == B * Hq * ms * (D + 2) * 4, S_cap
        seen.add(ms)
    assert dips > 0 and max(seen) == 64 and len(seen) > 4
    # a function of the capacity alone, like the plan; any output pointer may be null
    assert _plan_cap(lib, 1, 32, 32, 64, 4096, 64)[1] == _plan_cap(lib, B, Hq, Hkv, D, 4096, 32)[1]
    assert _plan_cap(lib, 3, 16, 4, 64, 9000 // 32 * 32, 32)[2] == 3 * 16 * 64 * 66 * 4
    assert lib.msq_kv_mx_attn_plan_cap(B, Hq, Hkv, D, 4096, 32, None, None) == 0
    assert _msq().kvpacked.attn_plan_cap(B, Hq, Hkv, D, 96, 32) == (1, B * Hq * 1 * (D + 2) * 4)
    assert _plan_cap(lib, B, Hq, Hkv, D, 0, 32)[1] == 1          # planes of no tokens: the tail-only split


def test_plan_cap_argument_errors():
    msq = _msq()
    lib = msq._lib.lib()
    assert _plan_cap(lib, 2, 8, 2, 48, 256, 32)[0] == UNSUPPORTED and b"head_dim" in lib.msq_last_error()
    assert _plan_cap(lib, 2, 32, 2, 128, 256, 32)[0] == UNSUPPORTED              # 16 query heads per kv head
    assert _plan_cap(lib, 2, 9, 2, 128, 256, 32)[0] == BAD_ARG                   # Hq % Hkv
    assert _plan_cap(lib, 0, 8, 2, 128, 256, 32)[0] == BAD_ARG
    assert _plan_cap(lib, 2, 8, 2, 128, 250, 32)[0] == BAD_ARG and b"S_cap" in lib.msq_last_error()
    assert _plan_cap(lib, 2, 8, 2, 128, 256, 48)[0] == BAD_ARG and b"tail_cap" in lib.msq_last_error()
    assert _plan_cap(lib, 2, 8, 2, 128, 256, 0)[0] == BAD_ARG
    with pytest.raises(msq._lib.MsqError):
        msq.kvpacked.attn_plan_cap(2, 8, 2, 128, 250, 32)


def test_append_dev_and_decode_dev_argument_errors():
    lib = _msq()._lib.lib()
    app = lambda **kw: lib.msq_kv_mx_append_dev(*[kw.get(k, d) for k, d in (
        ("k", None), ("v", None), ("dtype", 1), ("kc", None), ("ks", None), ("vc", None), ("vs", None), ("S_cap", 128), ("kt", None), ("vt", None),
        ("tail_cap", 32), ("state", PTR), ("B", 2), ("H", 2), ("D", 64), ("fmt", FP8), ("stream", None))])
    assert app(state=None) == BAD_ARG and b"null state" in lib.msq_last_error()
    assert app(S_cap=100) == BAD_ARG and b"S_cap" in lib.msq_last_error()
    assert app(S_cap=0) == BAD_ARG
    assert app(tail_cap=48) == BAD_ARG and b"tail_cap" in lib.msq_last_error()
    assert app(tail_cap=0) == BAD_ARG
    assert app(D=48) == UNSUPPORTED and app(D=288) == UNSUPPORTED and b"head_dim" in lib.msq_last_error()
    assert app(dtype=0) == UNSUPPORTED and app(dtype=3) == UNSUPPORTED           # the tail is f16 or bf16
    assert app(fmt=6) == UNSUPPORTED
    assert app(B=0) == BAD_ARG
    assert app() == BAD_ARG and b"null buffer" in lib.msq_last_error()           # every size is fine: the buffers are looked at last
    assert app(k=PTR, v=PTR, kc=PTR, ks=PTR, vc=PTR, vs=PTR, kt=PTR, vt=PTR + 8) == BAD_ARG and b"aligned" in lib.msq_last_error()

    dec = lambda **kw: lib.msq_kv_mx_attn_decode_dev(*[kw.get(k, d) for k, d in (
        ("q", None), ("q_dtype", 1), ("kc", None), ("ks", None), ("vc", None), ("vs", None), ("S_cap", 128), ("kt", None), ("vt", None),
        ("tail_cap", 32), ("state", PTR), ("bias", None), ("bias_stride", 0), ("out", None), ("out_dtype", 0), ("B", 2), ("Hq", 8), ("Hkv", 2),
        ("D", 128), ("fmt", FP8), ("scaling", 0.125), ("ws", None), ("ws_bytes", 1 << 24), ("stream", None))])
    assert dec(state=None) == BAD_ARG and b"null state" in lib.msq_last_error()
    assert dec(bias=PTR, bias_stride=159) == BAD_ARG and b"bias_stride" in lib.msq_last_error()      # < S_cap + tail_cap
    assert dec(bias=PTR, bias_stride=160) == BAD_ARG and b"null buffer" in lib.msq_last_error()      # wide enough: on to the buffers
    assert dec(bias_stride=0) == BAD_ARG and b"null buffer" in lib.msq_last_error()                  # no bias: the stride is not looked at
    assert dec(S_cap=100) == BAD_ARG and b"S_cap" in lib.msq_last_error()
    assert dec(tail_cap=40) == BAD_ARG and b"tail_cap" in lib.msq_last_error()
    assert dec(D=48) == UNSUPPORTED and b"head_dim" in lib.msq_last_error()
    assert dec(Hq=32) == UNSUPPORTED                                             # 16 query heads per kv head
    assert dec(Hq=9) == BAD_ARG
    assert dec(fmt=6) == UNSUPPORTED and dec(q_dtype=0) == UNSUPPORTED and dec(out_dtype=2) == UNSUPPORTED
    assert dec(q=PTR, out=PTR, ws=PTR, kt=PTR, vt=PTR, kc=PTR, ks=PTR, vc=PTR, vs=PTR, ws_bytes=64) == BAD_ARG and b"workspace" in lib.msq_last_error()
    assert dec() == BAD_ARG and b"null buffer" in lib.msq_last_error()


# ---------------------------------------------------------------------------------------------------------------------
# the host mirror, on stubs
# ---------------------------------------------------------------------------------------------------------------------
def test_capacity_is_max_len_rounded_up_to_the_gap():
    for gap, max_len, cap in ((32, 256, 256), (32, 250, 256), (64, 130, 192), (64, 64, 64), (32, 1, 32)):
        s = _static_stub(gap, max_len)
        assert (s.S_cap, s.capacity, s.packed_len, s.tail_len) == (cap, cap, 0, 0)
        assert tuple(s.k_tail.shape) == (1, 1, gap, 32)
    Err = _msq()._lib.MsqError
    for bad in (dict(gap=48, max_len=256), dict(gap=32, max_len=0)):
        with pytest.raises(Err):
            _static_stub(**bad)


@pytest.mark.parametrize("gap", [32, 64])
def test_mirror_follows_the_dynamic_cache_and_advance_host(gap):
    for p, n in ((0, 1), (0, 3 * gap + 5), (1, gap), (gap - 1, 2), (gap, 1), (gap, gap + 1), (70, 30), (2 * gap + 7, 2 * gap), (3 * gap, 3 * gap)):
        dyn, st, adv = _dynamic_stub(gap), _static_stub(gap, 8 * gap), _static_stub(gap, 8 * gap)
        if p:
            for s in (dyn, st, adv):
                s.append(*_tokens(0, p))                         # the parent's host path + one write of the lengths
            assert (st.writes, st.launches) == ((1, 0) if p > 1 else (0, 1))      # one token is the device append even as the first call
        assert (st.packed_len, st.tail_len) == (dyn.packed_len, dyn.tail_len) == (p - p % gap, p % gap)
        for i in range(n):
            dyn.append(*_tokens(p + i, p + i + 1))
            st.append(*_tokens(p + i, p + i + 1))
            assert (st.packed_len, st.tail_len) == (dyn.packed_len, dyn.tail_len), (gap, p, i)
            assert st.dev[:3] == [st.packed_len, st.tail_len, 0], (gap, p, i)          # the mirror never left the device's side of the rule
        assert st.launches == n + (p == 1) and st.writes == (p > 1) and st.log == dyn.log
        assert st.k_tail[0, 0, :st.tail_len, 0].tolist() == dyn.k_tail[0, 0, :dyn.tail_len, 0].tolist()
        adv.advance_host(n)                                      # n replays later: the same lengths, in one step and without a launch
        assert (adv.packed_len, adv.tail_len) == (st.packed_len, st.tail_len) and adv.launches == (p == 1)
        adv.advance_host(0)
        assert (adv.packed_len, adv.tail_len) == (st.packed_len, st.tail_len)
        assert st.sync() == (dyn.packed_len, dyn.tail_len)


@pytest.mark.parametrize("gap", [32, 64])
def test_overflow_is_refused_exactly_when_a_full_tail_cannot_be_flushed(gap):
    Err = _msq()._lib.MsqError
    s = _static_stub(gap, 2 * gap)                               # S_cap = 2 gap: 3 gap tokens fit (2 gap packed + a full tail)
    s.append(*_tokens(0, 2 * gap + gap - 1))
    assert (s.packed_len, s.tail_len) == (2 * gap, gap - 1)
    s.append(*_tokens(0, 1))                                     # the tail fills up: nothing to flush yet
    assert (s.packed_len, s.tail_len, s.launches) == (2 * gap, gap, 1)
    with pytest.raises(Err, match="overflow"):
        s.append(*_tokens(0, 1))                                 # packed_len + gap > S_cap with a full tail
    assert (s.packed_len, s.tail_len, s.launches) == (2 * gap, gap, 1) and s.dev[:3] == [2 * gap, gap, 0]      # refused before any launch
    with pytest.raises(Err):
        s.advance_host(1)
    s._append_dev(*_tokens(0, 1))                                # what a replay would do: the device refuses too, and says so
    assert s.dev[:3] == [2 * gap, gap, 8]
    with pytest.raises(Err, match="MSQ_STATUS_OVERFLOW"):
        s.sync()
    s.set_lengths(gap, gap)                                      # roll back: the status is cleared, one flush fits again
    assert s.dev == [gap, gap, 0, 0] and s.sync() == (gap, gap)
    s.append(*_tokens(0, 1))
    assert (s.packed_len, s.tail_len) == (2 * gap, 1)
    # advance_host refuses at the same token
    a = _static_stub(gap, 2 * gap)
    a.advance_host(3 * gap)
    assert (a.packed_len, a.tail_len) == (2 * gap, gap)
    b = _static_stub(gap, 2 * gap)
    with pytest.raises(Err):
        b.advance_host(3 * gap + 1)
    assert (b.packed_len, b.tail_len) == (0, 0)
    with pytest.raises(Err):
        _static_stub(gap, 2 * gap).append(*_tokens(0, 3 * gap))  # a prefill that needs 3 gap packed tokens
    for bad in ((gap + 1, 0), (3 * gap, 0), (gap, gap + 1), (-gap, 0)):
        with pytest.raises(Err):
            s.set_lengths(*bad)


def test_sync_reports_nan_and_multi_token_append_refuses_capture():
    Err = _msq()._lib.MsqError
    s = _static_stub(32, 128)
    s.append(*_tokens(0, 40))
    s.dev[2] = 1
    with pytest.raises(Err, match="MSQ_STATUS_NAN"):
        s.sync()
    s.capturing = True
    with pytest.raises(Err, match="captur"):
        s.append(*_tokens(40, 44))
    s.append(*_tokens(40, 41))                                   # a single token is the captured path
    assert (s.packed_len, s.tail_len) == (32, 9)


def test_static_entries_refuse_cpu_tensors():
    msq = _msq()
    kp, Err = msq.kvpacked, msq._lib.MsqError
    with pytest.raises(Err):
        kp.StaticPackedKV(1, 2, 64, torch.float16, max_len=64, device="cpu")
    x = torch.zeros(1, 2, 1, 64, dtype=torch.float16)
    cache = kp.PackedMXKVCache(2, max_len=64)
    with pytest.raises(Err):
        cache.update(x, x, 0)
    assert cache.get_seq_length() == 0
    with pytest.raises(Err):
        kp.PackedMXKVCache(2, max_len=0)
    s = _static_stub(32, 64)
    with pytest.raises(Err):
        s.attend_dev(torch.zeros(1, 4, 32, dtype=torch.float16))
    with pytest.raises(Err):
        s.attend(torch.zeros(1, 4, 32, dtype=torch.float16))
