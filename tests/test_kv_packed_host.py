"""Packed MX KV cache, host side (no GPU): the plane sizes of DESIGN.md 4, the launch plan of the decode kernel (msq_kv_mx_attn_plan: host
arithmetic of libmsq_hip.so), the argument checks of the C entries that come back before any launch, and the timing rule of
msq.kvpacked.PackedKV on a stub that records the pack calls instead of launching them."""
import ctypes as C

import pytest
import torch

from kv_packed_stubs import _msq, _tokens, dynamic_stub as _stub

FP8, FP4 = 5, 8
BAD_ARG, UNSUPPORTED = -1, -2


@pytest.mark.parametrize("fmt,code_bits", [("fp8_e4m3", 8), ("fp4_e2m1", 4)])
@pytest.mark.parametrize("B,H,S,D", [(1, 32, 4096, 128), (2, 2, 96, 64), (3, 8, 32, 256)])
def test_plane_sizes(fmt, code_bits, B, H, S, D):
    kp = _msq().kvpacked
    shp = kp.plane_shapes(B, H, S, D, fmt)
    assert shp["k_codes"] == shp["v_codes"] == (B, H, S, D * code_bits // 8)
    assert shp["k_scales"] == (B, H, S // 32, D)
    assert shp["v_scales"] == (B, H, S, D // 32)
    elems = 2 * B * H * S * D
    assert kp.plane_nbytes(B, H, S, D, fmt) * 8 == elems * (code_bits + 0.25)        # 8.25 / 4.25 bits per element, against 16
    for bad in ((B, H, S + 1, D), (B, H, S, 48), (B, H, S, 288)):
        with pytest.raises(_msq()._lib.MsqError):
            kp.plane_shapes(*bad, fmt)
    with pytest.raises(_msq()._lib.MsqError):
        kp.plane_shapes(B, H, S, D, "fp6_e3m2")


def _plan(lib, B, Hq, Hkv, D, S, tail):
    ns, st, wb = C.c_int(-1), C.c_int(-1), C.c_int64(-1)
    rc = lib.msq_kv_mx_attn_plan(B, Hq, Hkv, D, S, tail, C.byref(ns), C.byref(st), C.byref(wb))
    return rc, ns.value, st.value, wb.value


def test_plan_covers_every_packed_token_once():
    lib = _msq()._lib.lib()
    seen_sizes = set()
    for S in range(0, 4096 + 1, 32):
        for tail in (0, 1, 31, 32):
            if S + tail == 0:
                assert _plan(lib, 2, 8, 2, 128, S, tail)[0] == BAD_ARG
                continue
            rc, ns, st, wb = _plan(lib, 2, 8, 2, 128, S, tail)
            assert rc == 0 and ns >= 1 and st > 0 and st % 32 == 0, (S, tail)
            # split s covers s * st .. min((s + 1) * st, S): whole groups of 32, no gap, no overlap, no empty split but the tail-only one
            edges = [min(s * st, S) for s in range(ns + 1)]
            assert edges[0] == 0 and edges[-1] == S and (ns - 1) * st < max(S, 1) and ns * st >= S, (S, tail, ns, st)
            assert all(b > a and (b - a) % 32 == 0 for a, b in zip(edges, edges[1:])) or S == 0
            if S == 0:
                assert ns == 1
            assert wb == 2 * 8 * ns * (128 + 2) * 4
            assert lib.msq_kv_mx_attn_workspace_bytes(2, 8, 2, 128, S, tail) == wb
            # the splits are a function of S alone: a sequence gives the same bits whatever it is batched with
            assert _plan(lib, 1, 32, 32, 64, S, tail)[1:3] == (ns, st) and _plan(lib, 2, 8, 2, 128, S, 0 if S else 1)[1:3] == (ns, st)
            seen_sizes.add(ns)
    assert len(seen_sizes) > 4 and max(seen_sizes) <= 64


def test_plan_and_decode_argument_errors():
    msq = _msq()
    lib = msq._lib.lib()
    assert _plan(lib, 2, 8, 2, 48, 64, 0)[0] == UNSUPPORTED                 # head_dim 48
    assert b"head_dim" in lib.msq_last_error()
    assert _plan(lib, 2, 32, 2, 128, 64, 0)[0] == UNSUPPORTED               # 16 query heads per kv head
    assert _plan(lib, 2, 9, 2, 128, 64, 0)[0] == BAD_ARG                    # Hq % Hkv
    assert _plan(lib, 2, 8, 2, 128, 0, 0)[0] == BAD_ARG                     # empty cache
    assert b"empty" in lib.msq_last_error()
    assert _plan(lib, 2, 8, 2, 128, 40, 0)[0] == BAD_ARG                    # S_packed % 32
    assert lib.msq_kv_mx_attn_workspace_bytes(2, 8, 2, 48, 64, 0) == UNSUPPORTED
    with pytest.raises(msq._lib.MsqError):
        msq.kvpacked.attn_plan(2, 8, 2, 128, 0, 0)
    assert msq.kvpacked.attn_plan(2, 8, 2, 128, 64, 3)[0] == 1

    dec = lambda **kw: lib.msq_kv_mx_attn_decode(*[kw.get(k, d) for k, d in (
        ("q", None), ("q_dtype", 1), ("kc", None), ("ks", None), ("vc", None), ("vs", None), ("S_packed", 64), ("S_cap", 64), ("kt", None),
        ("vt", None), ("tail_len", 3), ("tail_cap", 32), ("bias", None), ("out", None), ("out_dtype", 0), ("B", 2), ("Hq", 8), ("Hkv", 2),
        ("D", 128), ("fmt", FP8), ("scaling", 0.125), ("ws", None), ("ws_bytes", 1 << 20), ("stream", None))])
    assert dec(D=48) == UNSUPPORTED
    assert dec(Hq=32) == UNSUPPORTED
    assert dec(S_packed=0, tail_len=0) == BAD_ARG and b"empty" in lib.msq_last_error()
    assert dec(S_packed=96) == BAD_ARG and b"S_cap" in lib.msq_last_error()          # S_packed > S_cap
    assert dec(tail_len=33) == BAD_ARG
    assert dec(fmt=6) == UNSUPPORTED and dec(q_dtype=0) == UNSUPPORTED and dec(out_dtype=2) == UNSUPPORTED
    assert dec() == BAD_ARG and b"null buffer" in lib.msq_last_error()               # every shape is fine: the buffers are looked at last


def test_pack_and_unpack_argument_errors():
    lib = _msq()._lib.lib()
    pack = lambda **kw: lib.msq_kv_mx_pack(*[kw.get(k, d) for k, d in (
        ("x", None), ("dtype", 1), ("codes", None), ("scales", None), ("B", 2), ("H", 2), ("T", 32), ("D", 64), ("S_cap", 128), ("pos", 64),
        ("fmt", FP8), ("along", 1), ("status", None), ("stream", None))])
    assert pack(pos=48) == BAD_ARG and b"pos" in lib.msq_last_error()
    assert pack(T=40) == BAD_ARG and b"T must" in lib.msq_last_error()
    assert pack(D=48) == UNSUPPORTED and pack(D=288) == UNSUPPORTED
    assert pack(pos=128) == BAD_ARG                                                   # pos + T > S_cap
    assert pack(S_cap=100) == BAD_ARG and pack(fmt=4) == UNSUPPORTED and pack(dtype=3) == UNSUPPORTED
    assert pack(T=0) == 0                                                             # nothing to do: no buffer is looked at
    assert pack() == BAD_ARG and b"null buffer" in lib.msq_last_error()
    unpack = lambda **kw: lib.msq_kv_mx_unpack(*[kw.get(k, d) for k, d in (
        ("codes", None), ("scales", None), ("out", None), ("dtype", 1), ("B", 2), ("H", 2), ("D", 64), ("S_cap", 128), ("pos", 64), ("T", 32),
        ("fmt", FP4), ("along", 0), ("stream", None))])
    assert unpack(D=48) == UNSUPPORTED and unpack(pos=100) == BAD_ARG and unpack(T=0) == 0
    assert unpack() == BAD_ARG and b"null buffer" in lib.msq_last_error()


def test_timing_rule_prefill_70_then_30_tokens():
    """packed lengths 64, 64, ..., 96 exactly when the hook of msq.kvcache (streaming, stream_grouping, gap 32) would compress"""
    s = _stub(32)
    s.append(*_tokens(0, 70))
    assert (s.packed_len, s.tail_len, s.len) == (64, 6, 70)
    assert s.log == [(0, [float(i) for i in range(64)])]
    packed = []
    for i in range(30):
        cached = 70 + i
        hook_compresses = cached % 32 == 0                       # kvcache.MXKVLayer.update: `elif cached % gap == 0`
        before = s.packed_len
        s.append(*_tokens(cached, cached + 1))
        assert (s.packed_len != before) == hook_compresses, cached
        packed.append(s.packed_len)
        assert s.len == cached + 1 and s.tail_len == s.len - s.packed_len
        assert s.k_tail[0, 0, :s.tail_len, 0].tolist() == [float(t) for t in range(s.packed_len, s.len)]
    assert packed == [64] * 26 + [96] * 4
    assert s.log[1] == (64, [float(i) for i in range(64, 96)]) and len(s.log) == 2


def test_timing_rule_other_appends():
    s = _stub(64)                                                # a gap of two groups
    for i in range(64):
        s.append(*_tokens(i, i + 1))
    assert (s.packed_len, s.tail_len) == (0, 64) and s.log == []     # a full tail is packed by the NEXT token
    s.append(*_tokens(64, 65))
    assert (s.packed_len, s.tail_len) == (64, 1) and s.log == [(0, [float(i) for i in range(64)])]
    s.append(*_tokens(65, 200))                                  # a later multi-token append: the tail joins the new tokens
    assert (s.packed_len, s.tail_len) == (192, 8)
    assert s.log[1] == (64, [float(i) for i in range(64, 192)])
    assert s.k_tail[0, 0, :8, 0].tolist() == [float(i) for i in range(192, 200)]
    s = _stub(32)
    s.append(*_tokens(0, 31))                                    # shorter than a group: nothing to pack
    assert (s.packed_len, s.tail_len) == (0, 31) and s.log == []
    s.append(*_tokens(31, 33))
    assert (s.packed_len, s.tail_len) == (32, 1)


def test_every_entry_refuses_cpu_tensors():
    msq = _msq()
    kp, Err = msq.kvpacked, msq._lib.MsqError
    with pytest.raises(Err):
        kp.PackedKV(1, 2, 64, torch.float16, device="cpu")
    with pytest.raises(Err):
        kp.PackedKV(1, 2, 64, torch.float16, gap=48, device="cpu")
    x = torch.zeros(1, 2, 32, 64, dtype=torch.float16)
    codes, scales = torch.zeros(1, 2, 32, 64, dtype=torch.uint8), torch.zeros(1, 2, 1, 64, dtype=torch.uint8)
    with pytest.raises(Err):
        kp.mx_pack(x, codes, scales, 0, "fp8_e4m3", True)
    with pytest.raises(Err):
        kp.mx_unpack(codes, scales, 0, 32, 64, torch.float16, "fp8_e4m3", True)
    cache = kp.PackedMXKVCache(2)
    with pytest.raises(Err):
        cache.update(x, x, 0)
    s = _stub(32)
    with pytest.raises(Err):
        s.attend(torch.zeros(1, 4, 32, dtype=torch.float16))
