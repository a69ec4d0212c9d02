"""SURVEY 8 row N2, compact layout MSQ-C1 (include/msq.h): the fused dequant-GEMM on a compact weight at every M -- k_qgemv_u (single-launch
wide decode), k_qgemv (+ k_splitk_reduce) and k_qgemm3 (with and without split-K workspace) -- against the CPU oracle's linear on small
shapes and against a dense bf16 product of the unpacked weight on the Llama-2-7B projections."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from gpu_common import dev, weights

pytestmark = pytest.mark.gpu

DECODE, GEMM128 = 0, 1


def _choice(msq, M, N, K):
    return msq._lib.lib().msq_qlinear_kernel_choice(M, N, K, 7, -1)


def _name(msq, M, N, K, y_dtype=0):
    buf = C.create_string_buffer(128)
    assert msq._lib.lib().msq_qlinear_kernel_name(M, N, K, 7, -1, y_dtype, buf, 128) == 0
    return buf.value.decode()


@pytest.mark.parametrize("fi,fo,bs", [("int2", "fp4", 16), ("fp4_e2m1", "fp4_e2m1", 32)])
@pytest.mark.parametrize("M", [1, 16, 24, 40, 64, 65, 300, 513])
def test_compact_fused_gemm_vs_oracle_linear(msq, O, fi, fo, bs, M):
    """Same K, same accumulation as legacy_gpu_parity.py::test_fused_gemm_vs_oracle_linear: its bounds (fp32 accumulation of K = 512
    products against the oracle's double: 2e-5 max|y| + 1e-6; one bf16 rounding on top: 2^-8 max|y| + 1e-6)."""
    g = torch.Generator().manual_seed(2)
    W = torch.randn(256, 512, generator=g) * 0.02
    W[torch.rand(256, 512, generator=g) < 0.01] *= 20
    X = torch.randn(M, 512, generator=g).to(torch.bfloat16)
    bias = torch.randn(256, generator=g)
    P = msq.qlinear.pack_weight(W.to(dev()), 8, 8, fi, fo, 2, bs, layout="compact")
    assert (P.in_kind, P.out_kind) == (1, 7)
    Wq = O.outlier_fakequant(W.numpy(), 8, 8, fi, fo, 2, -1, bs)["out"]
    ref = O.linear(X.float().numpy(), Wq, bias.numpy())
    y = msq.qlinear.qlinear(X.to(dev()), P, bias.to(dev()), torch.float32).cpu().numpy()
    e32 = float(np.abs(y - ref).max())
    yb = msq.qlinear.qlinear(X.to(dev()), P, bias.to(dev()), torch.bfloat16).float().cpu().numpy()
    e16 = float(np.abs(yb - ref).max())
    print("M %d %s/%s/%d: f32 err %.3e (bound %.3e), bf16 err %.3e (bound %.3e)" % (
        M, fi, fo, bs, e32, 2e-5 * np.abs(ref).max() + 1e-6, e16, 2.0 ** -8 * np.abs(ref).max() + 1e-6))
    assert e32 <= 2e-5 * np.abs(ref).max() + 1e-6
    assert e16 <= 2.0 ** -8 * np.abs(ref).max() + 1e-6
    yh = msq.qlinear.qlinear(X.to(dev()), P, bias.to(dev()), torch.float16).float().cpu().numpy()
    assert np.abs(yh - ref).max() <= 2.0 ** -8 * np.abs(ref).max() + 1e-6          # fp16 rounds finer than bf16


def _dense_check(msq, P, Wb, M, seed, family, name_prefix, workspace=True):
    """qlinear against a dense bf16 matmul on the unpacked bf16 weight (an independent library kernel, fp32 accumulation, one rounding
    to bf16): within one bf16 ulp of the result scale, the criterion of test_full_size_properties for the same comparison."""
    N, K = P.N, P.K
    assert _choice(msq, M, N, K) == family, (M, N, K)
    assert _name(msq, M, N, K).startswith(name_prefix), _name(msq, M, N, K)
    g = torch.Generator(device=dev()).manual_seed(seed)
    X = torch.randn(M, K, generator=g, device=dev()).to(torch.bfloat16)
    ref = (X @ Wb.t()).float()
    if workspace:
        y = msq.qlinear.qlinear(X, P, None, torch.float32)
    else:                                                    # no split-K workspace: the single-pass form of the same kernel
        from msq._lib import check, current_stream, lib, ptr
        y = torch.empty(M, N, dtype=torch.float32, device=dev())
        check(lib().msq_qlinear_bf16(ptr(X), ptr(P.inl), ptr(P.out), ptr(P.scl), None, ptr(y), 0, M, N, K, P.block, P.in_kind, P.out_kind,
                                     None, 0, current_stream(dev())), "msq_qlinear_bf16")
    err, scale = float((y - ref).abs().max()), float(ref.abs().max())
    print("N %d K %d M %d %s: err %.3e, bound %.3e" % (N, K, M, name_prefix, err, 2.0 ** -8 * scale + 1e-6))
    assert err <= 2.0 ** -8 * scale + 1e-6
    return X, y


@pytest.mark.parametrize("N,K", [(12288, 4096), (22016, 4096)])
def test_wide_decode_on_the_fused_projections(msq, N, K):
    """fused q/k/v and gate/up, int2 / fp4 block 16, M = 1, 16, 32: k_qgemv_u<7, ...>, one launch"""
    W = weights(N, K, 21).to(dev())
    P = msq.qlinear.pack_weight(W, 8, 8, "int2", "fp4", 2, 16, layout="compact")
    assert P.nbytes == N * K * 6 // 8
    Wb = msq.qlinear.unpack_weight(P, torch.bfloat16)
    assert torch.equal(Wb.float(), msq.quant.outlier_fakequant(W, 8, 8, "int2", "fp4", 2, -1, 16)["out"])
    for M in (1, 16, 32):
        X, y = _dense_check(msq, P, Wb, M, 100 + M, DECODE, "k_qgemv_u<7, ")
        if M == 16:                                          # run to run: 20 launches, identical bits
            for _ in range(20):
                assert torch.equal(msq.qlinear.qlinear(X, P, None, torch.float32), y)


@pytest.mark.parametrize("N,K", [(4096, 4096), (4096, 11008)])
def test_decode_and_gemm_on_the_4096_wide_projections(msq, N, K):
    """o and down: k_qgemv + k_splitk_reduce at M = 1, 16; [4096, 4096] also k_qgemm3 at M = 128, 2048 (with / without workspace)
    and at M = 300 twenty times"""
    W = weights(N, K, 22).to(dev())
    P = msq.qlinear.pack_weight(W, 8, 8, "int2", "fp4", 2, 16, layout="compact")
    Wb = msq.qlinear.unpack_weight(P, torch.bfloat16)
    for M in (1, 16):
        _dense_check(msq, P, Wb, M, 200 + M, DECODE, "k_qgemv<1, 7, ")
    if K == 4096:
        for M in (128, 2048):
            _dense_check(msq, P, Wb, M, 300 + M, GEMM128, "k_qgemm3<1, 7, ")
            _dense_check(msq, P, Wb, M, 300 + M, GEMM128, "k_qgemm3<1, 7, ", workspace=False)
        X, y = _dense_check(msq, P, Wb, 300, 77, GEMM128, "k_qgemm3<1, 7, ")
        for _ in range(20):
            assert torch.equal(msq.qlinear.qlinear(X, P, None, torch.float32), y)


def test_fp16_activations_at_decode_sizes(msq):
    """as test_decode_kernels_take_fp16_activations for the other kinds: M = 8, fp16 x == x.to(bfloat16), bit for bit"""
    torch.manual_seed(58)
    for N, K in ((4096, 4096), (16384, 1024)):
        W = weights(N, K, 12).to(dev())
        x = (torch.randn(8, K, device=dev()) * 2).half()
        x[0, 0] = 65504.0; x[7, 1] = 6e-8
        b = torch.randn(N, device=dev())
        for bs in (16, 32):
            P = msq.qlinear.pack_weight(W, 8, 8, "int2", "fp4", 2, bs, layout="compact")
            for od in (torch.float16, torch.float32, torch.bfloat16):
                assert torch.equal(msq.qlinear.qlinear(x, P, b, od), msq.qlinear.qlinear(x.to(torch.bfloat16), P, b, od)), (N, bs, od)


def test_w4a8_on_a_compact_weight(msq):
    W = weights(512, 1024, 31).to(dev())
    P = msq.qlinear.pack_weight(W, 8, 8, "int2", "fp4", 2, 16, layout="compact")
    b = torch.randn(512, device=dev())
    for M in (4, 200):
        x = torch.randn(M, 1024, device=dev())
        xq, st = msq.qlinear.act_quant(x, 8, 8, "fp8_e4m3", "fp8_e4m3", 2, 32)
        assert int(st.item()) == 0
        assert torch.equal(msq.qlinear.qlinear_w4a8(x, P, b, torch.float32, check_status=True), msq.qlinear.qlinear(xq, P, b, torch.float32))
        xb = x.to(torch.bfloat16)                            # the bfloat16-activation entry ends in the same dispatcher
        xq2, _ = msq.qlinear.act_quant(xb, 8, 8, "fp8_e4m3", "fp8_e4m3", 2, 32)
        assert torch.equal(msq.qlinear.qlinear_w4a8(xb, P, b, torch.float32), msq.qlinear.qlinear(xq2, P, b, torch.float32))


def test_modules_and_graph_capture(msq, O):
    """QuantLinear.from_linear / fuse_projections / RowParallelQuantLinear with layout="compact"; one decode step (M = 1) of the
    module captured in a HIP graph replays to the eager result, also after the input buffer has been rewritten."""
    from msq.qlinear import QuantLinear, RowParallelQuantLinear, fuse_projections
    from msq.quant import MXQuantizer
    q = MXQuantizer()
    q.configure(8, 8, "int2", "fp4", "max", 2, [-1], 16)
    g = torch.Generator().manual_seed(9)
    lin = torch.nn.Linear(512, 768, bias=True)
    with torch.no_grad():
        lin.weight.copy_(weights(768, 512, 41))
    Wq = O.outlier_fakequant(lin.weight.detach().numpy(), 8, 8, "int2", "fp4", 2, -1, 16)["out"]
    lin = lin.to(dev())
    m = QuantLinear.from_linear(lin, q, layout="compact", compute_dtype="float32")
    assert m.layout == "compact" and (m.in_kind, m.out_kind) == (1, 7)
    assert (m.dequantize().cpu().numpy() == Wq).all()
    with pytest.raises(msq._lib.MsqError):
        QuantLinear.from_linear(copy.deepcopy(lin).to(torch.bfloat16), q, layout="compact")          # in-dtype packing is out of scope
    x = torch.randn(1, 512, generator=g).to(torch.bfloat16).to(dev())
    with torch.no_grad():
        eager = m(x).clone()
        ref = O.linear(x.float().cpu().numpy(), Wq, lin.bias.detach().float().cpu().numpy())
        assert np.abs(eager.float().cpu().numpy() - ref).max() <= 2.0 ** -8 * np.abs(ref).max() + 1e-6
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(3):
                m(x)
        torch.cuda.current_stream().wait_stream(s)
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            y = m(x)
        for _ in range(3):
            gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(y, eager)
        x2 = torch.randn(1, 512, generator=g).to(torch.bfloat16).to(dev())
        eager2 = m(x2).clone()
        x.copy_(x2)
        gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(y, eager2)

    class Att(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.q_proj, self.k_proj, self.v_proj = (torch.nn.Linear(512, 256, bias=False) for _ in range(3))
    att = Att().to(dev())
    Ws = [l.weight.detach().clone() for l in (att.q_proj, att.k_proj, att.v_proj)]
    fused = fuse_projections(att, ["q_proj", "k_proj", "v_proj"], q, layout="compact")
    assert fused.proj.layout == "compact" and fused.proj.out_kind == 7
    xx = torch.randn(5, 512, device=dev()).to(torch.bfloat16)
    with torch.no_grad():
        outs = [att.q_proj(xx), att.k_proj(xx), att.v_proj(xx)]
    Wf = fused.proj.dequantize()
    for i, (Wi, yi) in enumerate(zip(Ws, outs)):             # every row is quantised as it would be alone: the same values
        Wo = O.outlier_fakequant(Wi.cpu().numpy(), 8, 8, "int2", "fp4", 2, -1, 16)["out"]
        assert (Wf[256 * i:256 * (i + 1)].cpu().numpy() == Wo).all()
        ref = O.linear(xx.float().cpu().numpy(), Wo)
        assert np.abs(yi.float().cpu().numpy() - ref).max() <= 2.0 ** -8 * np.abs(ref).max() + 1e-6
    rp = RowParallelQuantLinear.from_linear(lin, q, 1, 0, layout="compact")
    assert rp.shard.layout == "compact"
    with torch.no_grad():
        assert torch.equal(rp(x).to(torch.bfloat16), m(x))   # the same kernel: the fp32 sum, rounded once
