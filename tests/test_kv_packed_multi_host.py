"""Packed MX KV cache, more than one query token, host side (no GPU): the workspace of msq_kv_mx_attn_multi against the plan
of the single-token entry, the argument errors that come back before any launch (C entry and msq.kvpacked.PackedKV.attend_multi), and the
lengths PackedKV.crop / StaticPackedKV.crop leave, on the stubs of the other host tests (storage on the host, a log instead of launches)."""
import ctypes as C

import pytest
import torch

from kv_packed_stubs import _msq, _tokens, dynamic_stub, static_stub

FP8, FP4 = 5, 8
BAD_ARG, UNSUPPORTED = -1, -2


def _dynamic_stub(gap):
    return dynamic_stub(gap, keep_tokens=True)                   # _pack keeps the tokens it is given so that _unpack can hand them back


def _static_stub(gap, max_len):
    return static_stub(gap, max_len, keep_tokens=True)


def test_workspace_is_the_plan_times_the_query_tokens():
    msq = _msq()
    lib, kp = msq._lib.lib(), msq.kvpacked
    for S in (0, 32, 96, 4096, 8192 + 32, 16384):
        for tail in (0, 1, 31):
            for T in (1, 2, 17, 32):
                if T > S + tail:
                    assert lib.msq_kv_mx_attn_multi_workspace_bytes(2, 8, 2, 128, T, S, tail) == BAD_ARG
                    continue
                ns, _, wb1 = kp.attn_plan(2, 8, 2, 128, S, tail)
                wb = lib.msq_kv_mx_attn_multi_workspace_bytes(2, 8, 2, 128, T, S, tail)
                assert wb == 2 * 8 * T * ns * (128 + 2) * 4 == T * wb1, (S, tail, T)
    assert lib.msq_kv_mx_attn_multi_workspace_bytes(1, 32, 8, 64, 4, 64, 3) == 32 * 4 * 1 * 66 * 4


def test_c_entry_argument_errors_before_any_launch():
    lib = _msq()._lib.lib()
    call = lambda **kw: lib.msq_kv_mx_attn_multi(*[kw.get(k, d) for k, d in (
        ("q", None), ("q_dtype", 1), ("kc", None), ("ks", None), ("vc", None), ("vs", None), ("S_packed", 64), ("S_cap", 64), ("kt", None),
        ("vt", None), ("tail_len", 3), ("tail_cap", 32), ("bias", None), ("bias_stride", 0), ("causal", 1), ("out", None), ("out_dtype", 0),
        ("B", 2), ("Hq", 8), ("Hkv", 2), ("D", 128), ("T", 4), ("fmt", FP8), ("scaling", 0.125), ("ws", None), ("ws_bytes", 1 << 24),
        ("stream", None))])
    assert call(T=0) == BAD_ARG and b"T must" in lib.msq_last_error()
    assert call(T=33) == BAD_ARG and b"T must" in lib.msq_last_error()
    assert call(T=32, S_packed=0, S_cap=0, tail_len=17) == BAD_ARG and b"T exceeds" in lib.msq_last_error()      # T > len
    assert call(Hq=32) == UNSUPPORTED and b"8 query heads" in lib.msq_last_error()                                # G = 16
    assert call(D=48) == UNSUPPORTED and call(Hq=9) == BAD_ARG
    assert call(S_packed=0, tail_len=0) == BAD_ARG
    assert call(S_packed=96) == BAD_ARG and b"S_cap" in lib.msq_last_error()
    assert call(tail_len=33) == BAD_ARG
    assert call(fmt=6) == UNSUPPORTED and call(q_dtype=0) == UNSUPPORTED and call(out_dtype=2) == UNSUPPORTED
    one = C.c_float(0.0)
    assert call(bias=C.cast(C.pointer(one), C.c_void_p), bias_stride=66) == BAD_ARG and b"bias_row_stride_t" in lib.msq_last_error()
    assert call() == BAD_ARG and b"null buffer" in lib.msq_last_error()               # every size is fine: the buffers are looked at last
    assert lib.msq_kv_mx_attn_multi_workspace_bytes(2, 8, 2, 128, 0, 64, 3) == BAD_ARG
    assert lib.msq_kv_mx_attn_multi_workspace_bytes(2, 32, 2, 128, 4, 64, 3) == UNSUPPORTED


def _tail(s):
    return s.k_tail[0, 0, :s.tail_len, 0].tolist()


@pytest.mark.parametrize("gap", [32, 64])
def test_crop_lengths(gap):
    Err = _msq()._lib.MsqError
    s = _dynamic_stub(gap)
    s.append(*_tokens(0, 200))
    P = 200 - 200 % gap
    assert (s.packed_len, s.tail_len) == (P, 200 - P)
    for bad in (-1, 201):
        with pytest.raises(Err, match="crop"):
            s.crop(bad)
    s.crop(200)                                                  # nothing to do
    assert (s.packed_len, s.tail_len, s.unpacks) == (P, 200 - P, [])
    s.crop(P + 3)                                                # inside the tail: only tail_len changes
    assert (s.packed_len, s.tail_len, s.unpacks) == (P, 3, []) and _tail(s) == [float(P), P + 1.0, P + 2.0]
    s.crop(P)                                                    # the boundary itself
    assert (s.packed_len, s.tail_len, s.unpacks) == (P, 0, [])
    n = P - gap - 7                                              # into the packed part: whole gaps stay packed, the rest is unpacked into the tail
    s.crop(n)
    assert (s.packed_len, s.tail_len, s.len) == (n - n % gap, n % gap, n) and s.packed_len % gap == 0
    assert s.unpacks == [(n - n % gap, n % gap)] and _tail(s) == [float(i) for i in range(n - n % gap, n)]
    s.append(*_tokens(n, n + 1))                                 # the cache goes on from there
    assert (s.len, s.tail_len) == (n + 1, n % gap + 1)
    s.crop(gap)                                                  # a multiple of the gap: nothing to unpack
    assert (s.packed_len, s.tail_len) == (gap, 0) and len(s.unpacks) == 1
    s.crop(0)
    assert (s.packed_len, s.tail_len, s.len) == (0, 0, 0) and len(s.unpacks) == 1
    s.append(*_tokens(0, 5))
    assert (s.packed_len, s.tail_len) == (0, 5)


@pytest.mark.parametrize("gap", [32, 64])
def test_static_crop_writes_the_device_state(gap):
    Err = _msq()._lib.MsqError
    s = _static_stub(gap, 256)
    s.append(*_tokens(0, 100))
    P = 100 - 100 % gap
    w = s.writes
    s.crop(98)
    assert (s.packed_len, s.tail_len) == (P, 98 - P) and s.dev[:2] == [P, 98 - P] and s.writes == w + 1
    s.crop(P - 10)
    n = P - 10
    assert (s.packed_len, s.tail_len) == (n - n % gap, n % gap) and s.sync() == (n - n % gap, n % gap)
    assert _tail(s) == [float(i) for i in range(n - n % gap, n)]
    s.capturing = True
    with pytest.raises(Err, match="captured"):
        s.crop(1)
    with pytest.raises(Err, match="captured|CUDA"):
        s.attend_multi(torch.zeros(1, 4, 2, 32, dtype=torch.float16))
    s.capturing = False
    s.crop(0)
    assert s.sync() == (0, 0)


def test_attend_multi_argument_errors():
    msq = _msq()
    Err = msq._lib.MsqError
    s = _dynamic_stub(32)
    s.append(*_tokens(0, 40))
    q = lambda T, D=32, dt=torch.float16: torch.zeros(1, 4, T, D, dtype=dt)
    with pytest.raises(Err, match="query tokens"):
        s.attend_multi(q(0))
    with pytest.raises(Err, match="query tokens"):
        s.attend_multi(q(33))
    s.crop(3)
    with pytest.raises(Err, match="the cache holds 3"):
        s.attend_multi(q(4))                                     # T > len
    s.append(*_tokens(3, 40))
    with pytest.raises(Err, match="expected q"):
        s.attend_multi(q(4, D=64))
    with pytest.raises(Err, match="expected q"):
        s.attend_multi(q(4, dt=torch.bfloat16))
    with pytest.raises(Err, match="expected q"):
        s.attend_multi(torch.zeros(1, 4, 32, dtype=torch.float16))
    with pytest.raises(Err, match="out_dtype"):
        s.attend_multi(q(4), out_dtype=torch.bfloat16)
    for shape in ((1, 39), (1, 4, 41), (1, 3, 40), (2, 40)):     # a bias of the wrong width / token count / batch
        with pytest.raises(Err, match="bias must be"):
            s.attend_multi(q(4), bias=torch.zeros(shape))
    with pytest.raises(Err, match="CUDA"):                       # every argument is fine: CPU tensors, no fallback
        s.attend_multi(q(4), bias=torch.zeros(1, 4, 40))
    with pytest.raises(Err, match="CUDA"):
        s.attend_multi(q(4))


def test_use_packed_attention_checks_max_query_tokens():
    msq = _msq()
    for bad in (0, 33):
        with pytest.raises(msq._lib.MsqError, match="max_query_tokens"):
            msq.kvpacked.use_packed_attention(torch.nn.Linear(2, 2), None, max_query_tokens=bad)
