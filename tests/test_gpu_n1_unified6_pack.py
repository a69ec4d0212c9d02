"""SURVEY 8 row N1, six-bit unified layout MSQ-U6 (include/msq.h): values -> planes -> values against the CPU oracle's fake-quant values, the
reference-made goldens (RTN along axis 0, GPTQ outputs) and planted boundary groups, bit for bit.

Every input is first checked on the CPU with `fits_u6`, the layout's own rule written out here, so a pass cannot come from an input the
format could not hold (and a refusal is checked against the same rule)."""
import os

import numpy as np
import pytest
import torch

from gpu_common import G, dev, eq, weights

pytestmark = pytest.mark.gpu

U6, U8 = 8, 5
CFGS = [("int2", "fp4", 16), ("int2", "fp4", 32), ("fp4_e2m1", "fp4_e2m1", 16), ("int2", "int2", 16)]


def fits_u6(values):
    """Number of (row, 32-k group) pairs of a 2-D array that MSQ-U6 cannot hold.  Per group: su = floor(log2(max|v|)) - 8, + 1 if
    max|v| 2^-su > 448, clamped to >= -126 (the scale rule of the MSQ-U1 packer); the group fits iff every |v| 2^-su is 0, a normal e4m3
    value (2^-6 ... 448) whose mantissa is 1 or 1.5, or exactly 2^-7 (the one e4m3 subnormal whose code has its two low bits clear)."""
    V = np.asarray(values, np.float64)
    n, k = V.shape
    V = np.pad(V, ((0, 0), (0, (-k) % 32))).reshape(n, -1, 32)
    finite = np.isfinite(V).all(-1)
    A = np.abs(np.where(np.isfinite(V), V, 0.0))
    mx = A.max(-1)
    su = np.zeros(mx.shape)
    nz = mx > 0
    su[nz] = np.floor(np.log2(mx[nz])) - 8
    su[nz & (mx * np.exp2(-su) > 448)] += 1
    su = np.maximum(su, -126)
    t = A * np.exp2(-su)[..., None]
    m, e = np.frexp(t)                                       # t = m 2^e, m in [0.5, 1)
    normal = ((m == 0.5) | (m == 0.75)) & (e - 1 >= -6) & (t <= 448)
    ok = ((t == 0) | normal | (t == 2.0 ** -7)).all(-1) & finite & (su <= 127)
    return int((~ok).sum())


def _small():
    """the 256 x 512 matrix of test_unified_pack_unpack_equals_fakequant (an all-zero group included)"""
    g = torch.Generator().manual_seed(1)
    W = torch.randn(256, 512, generator=g) * 0.02
    W[torch.rand(256, 512, generator=g) < 0.01] *= 20
    W[5, 64:96] = 0
    return W


def _roundtrip(msq, V, kinds=(U6,)):
    """pack_values(V) -> (PackedWeight, f32 unpack, bf16 unpack as float)"""
    P = msq.qlinear.pack_values(torch.from_numpy(np.ascontiguousarray(V, dtype=np.float32)).to(dev()), kinds)
    return P, msq.qlinear.unpack_weight(P, torch.float32).cpu().numpy(), msq.qlinear.unpack_weight(P, torch.bfloat16).float().cpu().numpy()


_ORACLE = {}


def _oracle_values(O, which, fi, fo, bs, axis):
    key = (which, fi, fo, bs, axis)
    if key not in _ORACLE:
        W = _small() if which == "small" else weights(1024, 1024, 3)
        _ORACLE[key] = O.outlier_fakequant(W.numpy(), 8, 8, fi, fo, 2, axis, bs)["out"]
    return _ORACLE[key]


@pytest.mark.parametrize("axis", [0, -1])
@pytest.mark.parametrize("fi,fo,bs", CFGS)
@pytest.mark.parametrize("which", ["small", "weights1024"])
def test_pack_values_unpack_equals_oracle(msq, O, which, fi, fo, bs, axis):
    V = _oracle_values(O, which, fi, fo, bs, axis)
    assert fits_u6(V) == 0
    P, f32, bf16 = _roundtrip(msq, V)
    assert (P.in_kind, P.out_kind, P.block) == (0, U6, 32) and P.bits_per_element == 6.25
    assert eq(f32, V) and eq(bf16, V)
    assert not np.signbit(f32[f32 == 0]).any()


def test_off_grid_shape(msq, O):
    V = O.outlier_fakequant(weights(300, 200, 11).numpy(), 8, 8, "int2", "fp4", 2, 0, 16)["out"]
    assert fits_u6(V) == 0
    P, f32, bf16 = _roundtrip(msq, V)
    assert (P.n, P.k, P.N, P.K) == (300, 200, 512, 256) and P.out_kind == U6
    assert f32.shape == (300, 200) and eq(f32, V) and eq(bf16, V)


def test_reference_goldens_along_axis_0(msq):
    """every 2-D int2 / fp4, block 16, axis 0 case of the reference-made golden (the harness default configuration): seven"""
    z = np.load(os.path.join(G, "outlier_fakequant.npz"))
    found = 0
    for key in sorted(k[4:] for k in z.keys() if k.startswith("out|int2_fp4_bs16_ax0|")):
        V = z["out|" + key]
        if V.ndim != 2:
            continue
        found += 1
        assert fits_u6(V) == 0, key
        P, f32, bf16 = _roundtrip(msq, V)
        assert P.out_kind == U6 and eq(f32, V) and eq(bf16, V), key
    print("reference goldens packed into MSQ-U6: %d" % found)
    assert found == 7


def test_gptq_goldens(msq):
    z, ze = np.load(os.path.join(G, "gptq.npz")), np.load(os.path.join(G, "gptq_exact.npz"))
    for name, V in (("gptq Q", z["Q"]), ("single", ze["single_int2_fp4|Q"]), ("multi", ze["multi_int2_fp4|Q"])):
        assert fits_u6(V) == 0, name
        P, f32, bf16 = _roundtrip(msq, V)
        assert P.out_kind == U6 and eq(f32, V) and eq(bf16, V), name
    V = ze["single_fp4_fp8|Q"]                               # e4m3 outliers: three mantissa bits
    assert fits_u6(V) > 0
    with pytest.raises(msq._lib.MsqError):
        _roundtrip(msq, V)
    P, f32, _ = _roundtrip(msq, V, (U6, 5, 6, 4))
    assert P.out_kind == U8 and eq(f32, V)


def _planted(x, s=-10):
    V = np.zeros((64, 64), np.float32)
    V[3, 32], V[3, 41] = 256.0 * 2.0 ** s, x * 2.0 ** s       # one 32-k group: its maximum 256 2^s (scale 2^s) and x 2^s
    return V


def test_planted_boundary(msq):
    V = _planted(2.0 ** -7)
    assert fits_u6(V) == 0
    P, f32, bf16 = _roundtrip(msq, V)
    assert P.out_kind == U6 and eq(f32, V) and eq(bf16, V)
    for x in (1.5 * 2.0 ** -8, 2.0 ** -9):                   # e4m3 subnormals 011 and 001: the low bits carry them
        V = _planted(x)
        assert fits_u6(V) == 1
        with pytest.raises(msq._lib.MsqError):
            _roundtrip(msq, V)
        P, f32, _ = _roundtrip(msq, V, (U6, U8))
        assert P.out_kind == U8 and eq(f32, V)
    V = _planted(1.5)
    V[3, 33] = -0.0
    V[10, 5] = -0.0
    assert fits_u6(V) == 0
    P, f32, bf16 = _roundtrip(msq, V)
    assert P.out_kind == U6 and eq(f32, V) and not np.signbit(f32[f32 == 0]).any() and not np.signbit(bf16[bf16 == 0]).any()
    V = _planted(1.5)
    V[3, 40] = np.nan
    with pytest.raises(AssertionError, match="NaN"):
        _roundtrip(msq, V)


def test_fused_quantise_and_pack(msq, O):
    W = _small()
    Vo = O.outlier_fakequant(W.numpy(), 8, 8, "int2", "fp4", 2, -1, 16)["out"]
    assert fits_u6(Vo) == 0
    P = msq.qlinear.pack_weight(W.to(dev()), 8, 8, "int2", "fp4", 2, 16, layout="unified6")
    assert (P.in_kind, P.out_kind, P.block) == (0, U6, 16) and P.bits_per_element == 6.25
    assert eq(msq.qlinear.unpack_weight(P, torch.float32).cpu().numpy(), Vo)
    assert eq(msq.qlinear.unpack_weight(P, torch.bfloat16).float().cpu().numpy(), Vo)
    for dt in (torch.float16, torch.bfloat16):               # quantised in its own dtype, packed from the values (the case MSQ-C1 refuses)
        Wh = W.to(dt).to(dev())
        Vh = msq.quant.outlier_fakequant(Wh, 8, 8, "int2", "fp4", 2, -1, 16)["out"]
        assert Vh.dtype == dt and fits_u6(Vh.float().cpu().numpy()) == 0
        Ph = msq.qlinear.pack_weight(Wh, 8, 8, "int2", "fp4", 2, 16, layout="unified6")
        assert (Ph.in_kind, Ph.out_kind) == (0, U6)
        assert torch.equal(msq.qlinear.unpack_weight(Ph, torch.float32), Vh.float())
    Err = msq._lib.MsqError
    Wd = W.to(dev())
    with pytest.raises(Err, match="unified6"):
        msq.qlinear.pack_weight(Wd, 8, 8, "fp4_e2m1", "fp8_e4m3", 2, 16, layout="unified6")
    with pytest.raises(Err, match="unified6"):
        msq.qlinear.pack_weight(Wd.half(), 8, 8, "fp4_e2m1", "fp8_e4m3", 2, 16, layout="unified6")
    with pytest.raises(Err, match="unified6"):
        msq.qlinear.pack_weight(Wd, 8, 8, "int2", "fp4", 2, 16, round="floor", layout="unified6")
    with pytest.raises(Err, match="unified6"):
        msq.qlinear.pack_weight(Wd, 8, 8, "int2", "fp4", 2, 16, variant=1, layout="unified6")
    # the other layouts select what they selected
    Pa = msq.qlinear.pack_weight(Wd, 8, 8, "int2", "fp4", 2, 16, layout="auto")
    Pp = msq.qlinear.pack_weight(Wd, 8, 8, "int2", "fp4", 2, 16, layout="planes")
    Pc = msq.qlinear.pack_weight(Wd, 8, 8, "int2", "fp4", 2, 16, layout="compact")
    assert (Pa.in_kind, Pa.out_kind) == (0, 5) and (Pp.in_kind, Pp.out_kind) == (1, 2) and (Pc.in_kind, Pc.out_kind) == (1, 7)
    assert msq.qlinear.pack_values(torch.from_numpy(Vo).to(dev())).out_kind == 5          # the default kinds are unchanged


def test_whole_size_once(msq):
    """[16384, 4096] on the device, the harness default (int2 / fp4, block 16 along out_features)"""
    N, K = 16384, 4096
    V = msq.quant.outlier_fakequant(weights(N, K).to(dev()), 8, 8, "int2", "fp4", 2, 0, 16)["out"]
    assert fits_u6(V[:2048].cpu().numpy()) == 0              # (the CPU predicate on an eighth of the rows; the unpack below covers all)
    P = msq.qlinear.pack_values(V, (U6,))
    assert P.nbytes == N * K * 25 // 32 and (P.in_kind, P.out_kind) == (0, U6)
    assert torch.equal(msq.qlinear.unpack_weight(P, torch.float32), V)
    assert torch.equal(msq.qlinear.unpack_weight(P, torch.bfloat16).float(), V)
