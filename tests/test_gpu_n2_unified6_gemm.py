"""SURVEY 8 row N2, six-bit unified layout MSQ-U6 (include/msq.h): the fused dequant-GEMM on a U6 weight at every M -- k_qgemv_u (single-launch
wide decode), k_qgemv (+ k_splitk_reduce) and k_qgemm3 (with and without split-K workspace) -- against the CPU oracle's linear on small
shapes, against a dense bf16 product of the unpacked weight on the wide shapes, and bit for bit against the same values packed as MSQ-U1
wherever both run the same kernel.  The weights are packed from fake-quant VALUES (pack_values), blocks along out_features included."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from gpu_common import dev, weights
from test_gpu_n1_unified6_pack import fits_u6

pytestmark = pytest.mark.gpu

DECODE, GEMM128 = 0, 1
U6, U8 = 8, 5


def _choice(msq, M, N, K, kind=U6):
    return msq._lib.lib().msq_qlinear_kernel_choice(M, N, K, kind, -1)


def _name(msq, M, N, K, kind=U6, y_dtype=0):
    buf = C.create_string_buffer(128)
    assert msq._lib.lib().msq_qlinear_kernel_name(M, N, K, kind, -1, y_dtype, buf, 128) == 0
    return buf.value.decode()


def _values(msq, N, K, seed, axis=0, fi="int2", fo="fp4", bs=16):
    """fake-quant values on the device (the HIP quantiser the a6 tests pin to the oracle), checked against the layout's rule on the CPU"""
    V = msq.quant.outlier_fakequant(weights(N, K, seed).to(dev()), 8, 8, fi, fo, 2, axis, bs)["out"]
    assert fits_u6(V[:1024].cpu().numpy()) == 0
    return V


@pytest.mark.parametrize("fi,fo,bs,axis", [("int2", "fp4", 16, 0), ("fp4_e2m1", "fp4_e2m1", 32, -1)])
@pytest.mark.parametrize("M", [1, 16, 24, 40, 64, 65, 300, 513])
def test_unified6_fused_gemm_vs_oracle_linear(msq, O, fi, fo, bs, axis, M):
    """Same K, same accumulation as legacy_gpu_parity.py::test_fused_gemm_vs_oracle_linear: its bounds (fp32 accumulation of K = 512
    products against the oracle's double: 2e-5 max|y| + 1e-6; one bf16 / fp16 rounding on top: 2^-8 max|y| + 1e-6)."""
    g = torch.Generator().manual_seed(2)
    W = torch.randn(256, 512, generator=g) * 0.02
    W[torch.rand(256, 512, generator=g) < 0.01] *= 20
    X = torch.randn(M, 512, generator=g).to(torch.bfloat16)
    bias = torch.randn(256, generator=g)
    Wq = O.outlier_fakequant(W.numpy(), 8, 8, fi, fo, 2, axis, bs)["out"]
    assert fits_u6(Wq) == 0
    P = msq.qlinear.pack_values(torch.from_numpy(Wq).to(dev()), (U6,))
    assert (P.in_kind, P.out_kind) == (0, U6)
    ref = O.linear(X.float().numpy(), Wq, bias.numpy())
    y = msq.qlinear.qlinear(X.to(dev()), P, bias.to(dev()), torch.float32).cpu().numpy()
    e32 = float(np.abs(y - ref).max())
    yb = msq.qlinear.qlinear(X.to(dev()), P, bias.to(dev()), torch.bfloat16).float().cpu().numpy()
    e16 = float(np.abs(yb - ref).max())
    print("M %d %s/%s/%d axis %d: f32 err %.3e (bound %.3e), bf16 err %.3e (bound %.3e)" % (
        M, fi, fo, bs, axis, e32, 2e-5 * np.abs(ref).max() + 1e-6, e16, 2.0 ** -8 * np.abs(ref).max() + 1e-6))
    assert e32 <= 2e-5 * np.abs(ref).max() + 1e-6
    assert e16 <= 2.0 ** -8 * np.abs(ref).max() + 1e-6
    yh = msq.qlinear.qlinear(X.to(dev()), P, bias.to(dev()), torch.float16).float().cpu().numpy()
    assert np.abs(yh - ref).max() <= 2.0 ** -8 * np.abs(ref).max() + 1e-6


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


def _same_kernel_but_kind(msq, M, N, K):
    """do the MSQ-U1 and the MSQ-U6 weight of this shape run instantiations that differ in the kind parameter only?"""
    n5, n8 = _name(msq, M, N, K, U8), _name(msq, M, N, K, U6)
    m5, m8 = re.fullmatch(r"(k_qgemv_u<)5(, .*)", n5), re.fullmatch(r"(k_qgemv_u<)8(, .*)", n8)
    if m5 and m8:
        return m5.groups() == m8.groups()
    m5, m8 = re.fullmatch(r"(k_qgemv<0, )5(, .*)", n5), re.fullmatch(r"(k_qgemv<0, )8(, .*)", n8)
    return bool(m5 and m8 and m5.groups() == m8.groups())


@pytest.mark.parametrize("N,K", [(8448, 1024), (12288, 4096)])
def test_wide_decode_and_same_bits_as_u1(msq, N, K):
    """more than 128 strips (8448 x 1024: 132 strips, the smallest grid that takes k_qgemv_u, two tiles per wave; the fused q/k/v shape), axis-0
    int2 / fp4 values, M = 1, 16, 32: k_qgemv_u<8, ...>, one launch; the MSQ-U1 weight of the same values runs the same kernel for its own kind
    and must give the same bits (the decode yields the same bf16 weights, summed in the same order)"""
    V = _values(msq, N, K, 21)
    P = msq.qlinear.pack_values(V, (U6,))
    P5 = msq.qlinear.pack_values(V, (U8,))
    assert P.nbytes == N * K * 25 // 32 and P.out_kind == U6 and P5.out_kind == U8
    Wb = msq.qlinear.unpack_weight(P, torch.bfloat16)
    assert torch.equal(Wb.float(), V)
    for M in (1, 16, 32):
        X, y = _dense_check(msq, P, Wb, M, 100 + M, DECODE, "k_qgemv_u<8, ")
        assert _same_kernel_but_kind(msq, M, N, K), (_name(msq, M, N, K, U8), _name(msq, M, N, K, U6))
        for od in (torch.float32, torch.bfloat16):
            assert torch.equal(msq.qlinear.qlinear(X, P, None, od), msq.qlinear.qlinear(X, P5, None, od)), (M, od)
        if M == 16:                                          # run to run: 20 launches, identical bits
            for _ in range(20):
                assert torch.equal(msq.qlinear.qlinear(X, P, None, torch.float32), y)


def test_decode_and_gemm_on_the_4096_wide_projection(msq):
    """[4096, 4096]: k_qgemv + k_splitk_reduce at M = 1, 16; k_qgemm3 at M = 128, 2048 (with / without workspace) and at M = 300 twenty times"""
    N = K = 4096
    V = _values(msq, N, K, 22)
    P = msq.qlinear.pack_values(V, (U6,))
    P5 = msq.qlinear.pack_values(V, (U8,))
    Wb = msq.qlinear.unpack_weight(P, torch.bfloat16)
    assert torch.equal(Wb.float(), V)
    for M in (1, 16):
        X, y = _dense_check(msq, P, Wb, M, 200 + M, DECODE, "k_qgemv<0, 8, ")
        if _same_kernel_but_kind(msq, M, N, K):
            assert torch.equal(y, msq.qlinear.qlinear(X, P5, None, torch.float32)), M
    for M in (128, 2048):
        _dense_check(msq, P, Wb, M, 300 + M, GEMM128, "k_qgemm3<0, 8, ")
        _dense_check(msq, P, Wb, M, 300 + M, GEMM128, "k_qgemm3<0, 8, ", workspace=False)
    X, y = _dense_check(msq, P, Wb, 300, 77, GEMM128, "k_qgemm3<0, 8, ")
    for _ in range(20):
        assert torch.equal(msq.qlinear.qlinear(X, P, None, torch.float32), y)


def test_fp16_activations_at_decode_sizes(msq):
    """as test_decode_kernels_take_fp16_activations for the other kinds: M = 8, fp16 x == x.to(bfloat16), bit for bit"""
    torch.manual_seed(58)
    for N, K in ((4096, 4096), (16384, 1024)):
        P = msq.qlinear.pack_values(_values(msq, N, K, 12), (U6,))
        x = (torch.randn(8, K, device=dev()) * 2).half()
        x[0, 0] = 65504.0; x[7, 1] = 6e-8
        b = torch.randn(N, device=dev())
        for od in (torch.float16, torch.float32, torch.bfloat16):
            assert torch.equal(msq.qlinear.qlinear(x, P, b, od), msq.qlinear.qlinear(x.to(torch.bfloat16), P, b, od)), (N, od)


def test_w4a8_on_a_unified6_weight(msq):
    P = msq.qlinear.pack_values(_values(msq, 512, 1024, 31), (U6,))
    assert P.out_kind == U6
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
    """QuantLinear.from_dense / fuse_projections(quantizer=None) with kinds=(8, 5, 6, 4) on axis-0 fake-quantised Linears, QuantLinear.from_linear
    and RowParallelQuantLinear with layout="unified6"; one decode step (M = 1) of the module captured in a HIP graph replays to the eager
    result, also after the input buffer has been rewritten."""
    from msq.qlinear import QuantLinear, RowParallelQuantLinear, fuse_projections
    from msq.quant import MXQuantizer
    KINDS = (8, 5, 6, 4)
    g = torch.Generator().manual_seed(9)
    lin = torch.nn.Linear(512, 768, bias=True)
    Wq = O.outlier_fakequant(weights(768, 512, 41).numpy(), 8, 8, "int2", "fp4", 2, 0, 16)["out"]      # the harness default: blocks along out_features
    assert fits_u6(Wq) == 0
    with torch.no_grad():
        lin.weight.copy_(torch.from_numpy(Wq))
    lin = lin.to(dev())
    m = QuantLinear.from_dense(lin, kinds=KINDS)
    assert m.layout == "unified6" and (m.in_kind, m.out_kind) == (0, U6)
    assert (m.dequantize().cpu().numpy() == Wq).all()
    assert QuantLinear.from_dense(lin).out_kind == U8                 # the default is unchanged
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
    att = Att()
    Wos = [O.outlier_fakequant(weights(256, 512, 50 + i).numpy(), 8, 8, "int2", "fp4", 2, 0, 16)["out"] for i in range(3)]
    with torch.no_grad():
        for l, Wo in zip((att.q_proj, att.k_proj, att.v_proj), Wos):
            l.weight.copy_(torch.from_numpy(Wo))
    att = att.to(dev())
    fused = fuse_projections(att, ["q_proj", "k_proj", "v_proj"], None, kinds=KINDS)
    assert fused.proj.layout == "unified6" and fused.proj.out_kind == U6
    xx = torch.randn(5, 512, device=dev()).to(torch.bfloat16)
    with torch.no_grad():
        outs = [att.q_proj(xx), att.k_proj(xx), att.v_proj(xx)]
    Wf = fused.proj.dequantize()
    for i, (Wo, yi) in enumerate(zip(Wos, outs)):
        assert (Wf[256 * i:256 * (i + 1)].cpu().numpy() == Wo).all()
        ref = O.linear(xx.float().cpu().numpy(), Wo)
        assert np.abs(yi.float().cpu().numpy() - ref).max() <= 2.0 ** -8 * np.abs(ref).max() + 1e-6
    # quantise + pack through the modules: blocks along in_features
    q = MXQuantizer()
    q.configure(8, 8, "int2", "fp4", "max", 2, [-1], 16)
    lin2 = torch.nn.Linear(512, 768, bias=True)
    with torch.no_grad():
        lin2.weight.copy_(weights(768, 512, 41))
    Wq2 = O.outlier_fakequant(lin2.weight.detach().numpy(), 8, 8, "int2", "fp4", 2, -1, 16)["out"]
    lin2 = lin2.to(dev())
    m2 = QuantLinear.from_linear(lin2, q, layout="unified6")
    assert m2.layout == "unified6" and (m2.in_kind, m2.out_kind) == (0, U6) and (m2.dequantize().cpu().numpy() == Wq2).all()
    rp = RowParallelQuantLinear.from_linear(lin2, q, 1, 0, layout="unified6")
    assert rp.shard.layout == "unified6"
    with torch.no_grad():
        assert torch.equal(rp(x).to(torch.bfloat16), m2(x))  # the same kernel: the fp32 sum, rounded once
