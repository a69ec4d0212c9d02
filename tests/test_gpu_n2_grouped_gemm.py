"""SURVEY 8 row N2, mixture of experts: the grouped fused dequant-GEMM k_qgemm_grouped (msq.moe.grouped_qlinear) -- one activation batch
times several packed weights chosen per row -- against the CPU oracle's linear per expert on small shapes (fewer K-tiles than waves, an
uneven share, one tile per wave), its exact properties (run to run, a row alone or among others or in another order, rows beyond the routed
count untouched, pack / unpack), and one wide shape against a dense bf16 product of the unpacked weights."""
import functools

import numpy as np
import pytest
import torch

from gpu_common import dev, weights
from test_gpu_n1_unified6_pack import fits_u6

pytestmark = pytest.mark.gpu

U8, U8X, U6 = 5, 6, 8
E, N = 4, 256
FAMILIES = {                       # inlier / outlier format, block, axis, plane kind
    "u6": ("int2", "fp4", 16, 0, U6),
    "u8": ("fp4_e2m1", "fp8_e4m3", 32, -1, U8),
    "u8x": ("fp4_e2m1", "posit8_es1", 32, -1, U8X),
}
COUNTS = ([0, 1, 63, 0], [64, 65, 0, 129], [0, 0, 0, 5], [300, 0, 0, 0], [1, 1, 1, 1])


@functools.lru_cache(maxsize=None)
def _values(family, K):
    """oracle fake-quant values [E, N, K] (another seed per expert), computed once per (family, K)"""
    from oracle import oracle as O
    fi, fo, bs, axis, kind = FAMILIES[family]
    V = np.stack([O.outlier_fakequant(weights(N, K, 1000 + 17 * e + K).numpy(), 8, 8, fi, fo, 2, axis, bs)["out"] for e in range(E)])
    if kind == U6:
        assert fits_u6(V.reshape(E * N, K)) == 0
    return V


@functools.lru_cache(maxsize=None)
def _packed(family, K):
    import msq
    kind = FAMILIES[family][4]
    PE = msq.moe.pack_expert_values(torch.from_numpy(_values(family, K)).to(dev()), (kind,) if kind == U6 else (U8, U8X))
    assert (PE.in_kind, PE.out_kind, PE.E, PE.N, PE.K) == (0, kind, E, N, K)
    return PE


def _offsets(counts):
    return torch.tensor([0] + list(np.cumsum(counts)), dtype=torch.int32, device=dev())


def _expert_of_rows(counts):
    return np.repeat(np.arange(len(counts)), counts)


@pytest.mark.parametrize("K", [256, 448, 512])
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_grouped_gemm_vs_oracle_linear(msq, O, family, K):
    """bounds of test_unified6_fused_gemm_vs_oracle_linear: fp32 accumulation of K <= 512 products against the oracle's double
    (2e-5 max|ref| + 1e-6), one bf16 / fp16 rounding on top (2^-8 max|ref| + 1e-6)"""
    V, PE = _values(family, K), _packed(family, K)
    g = torch.Generator().manual_seed(3 + K)
    bias = torch.randn(E, N, generator=g)
    for ci, counts in enumerate(COUNTS):
        R = sum(counts)
        ex = _expert_of_rows(counts)
        Xbig = torch.randn(R + 37, K, generator=g).to(torch.bfloat16)
        ridx = torch.randint(0, R + 37, (R,), generator=g).to(torch.int32)
        off = _offsets(counts)
        for gather in (True, False):
            Xrows = Xbig[ridx.long()] if gather else Xbig[:R]
            xf = Xrows.float().numpy()
            for with_bias in (True, False):
                ref = np.zeros((R, N), np.float64)
                for e in range(E):
                    sel = ex == e
                    if sel.any():
                        ref[sel] = O.linear(xf[sel], V[e], bias[e].numpy() if with_bias else None)
                scale = float(np.abs(ref).max())
                x_dev = Xbig.to(dev()) if gather else Xbig[:R].to(dev())
                kw = dict(row_index=ridx.to(dev()) if gather else None, bias=bias.to(dev()) if with_bias else None)
                y = msq.moe.grouped_qlinear(x_dev, PE, off, out_dtype=torch.float32, **kw).cpu().numpy()
                e32 = float(np.abs(y - ref).max())
                print("%s K %d counts %s gather %d bias %d: f32 err %.3e (bound %.3e)" % (family, K, counts, gather, with_bias, e32, 2e-5 * scale + 1e-6))
                assert y.shape == (R, N) and e32 <= 2e-5 * scale + 1e-6
                if gather and with_bias:
                    for od in (torch.bfloat16, torch.float16):
                        y16 = msq.moe.grouped_qlinear(x_dev, PE, off, out_dtype=od, **kw)
                        assert y16.dtype == od
                        e16 = float(np.abs(y16.float().cpu().numpy() - ref).max())
                        print("    %s err %.3e (bound %.3e)" % (od, e16, 2.0 ** -8 * scale + 1e-6))
                        assert e16 <= 2.0 ** -8 * scale + 1e-6


@pytest.mark.parametrize("family,K", [("u6", 448), ("u8x", 512), ("u8", 256)])
def test_same_bits_every_run_and_for_a_row_alone(msq, family, K):
    counts = [64, 65, 0, 129]
    R, ex = sum(counts), _expert_of_rows(counts)
    PE = _packed(family, K)
    g = torch.Generator().manual_seed(11)
    X = torch.randn(R + 9, K, generator=g).to(torch.bfloat16).to(dev())
    ridx = torch.randint(0, R + 9, (R,), generator=g).to(torch.int32).to(dev())
    off = _offsets(counts)
    y = msq.moe.grouped_qlinear(X, PE, off, ridx, out_dtype=torch.float32)
    for _ in range(20):                                          # (a) run to run
        assert torch.equal(msq.moe.grouped_qlinear(X, PE, off, ridx, out_dtype=torch.float32), y)
    # (b) every row recomputed in a call that holds that row alone (same expert): the same bits
    alone = torch.empty_like(y)
    for r in range(R):
        o1 = torch.zeros(E + 1, dtype=torch.int32)
        o1[ex[r] + 1:] = 1
        alone[r:r + 1] = msq.moe.grouped_qlinear(X, PE, o1.to(dev()), ridx[r:r + 1], out_dtype=torch.float32)
    assert torch.equal(alone, y)
    # ... and with the same rows presented in another order inside every expert
    perm = np.concatenate([np.random.RandomState(5 + e).permutation(np.nonzero(ex == e)[0]) for e in range(E)])
    perm_t = torch.from_numpy(perm).to(dev())
    y2 = msq.moe.grouped_qlinear(X, PE, off, ridx[perm_t].contiguous(), out_dtype=torch.float32)
    assert torch.equal(y2, y[perm_t])
    yb = msq.moe.grouped_qlinear(X, PE, off, ridx, out_dtype=torch.bfloat16)
    assert torch.equal(yb, y.to(torch.bfloat16))                 # the 16-bit epilogue rounds the same fp32 sums once


@pytest.mark.parametrize("od", [torch.float32, torch.bfloat16])
def test_rows_beyond_the_routed_count_are_not_written(msq, od):
    """(c) `rows` is the capacity; row_offsets[E] says how many rows exist: the 5 unused rows and 8 guard rows keep the sentinel"""
    K, counts, cap = 256, [70, 0, 3, 60], 138
    PE = _packed("u6", K)
    X = torch.randn(cap, K, generator=torch.Generator().manual_seed(2)).to(torch.bfloat16).to(dev())
    off = _offsets(counts)
    assert int(off[-1]) == cap - 5
    buf = torch.full((cap + 8, N), -768.0, dtype=od, device=dev())
    y = msq.moe.grouped_qlinear(X, PE, off, out_dtype=od, out=buf[:cap], rows=cap)
    assert y.data_ptr() == buf.data_ptr()
    assert bool((buf[cap - 5:] == -768.0).all())
    assert torch.equal(buf[:cap - 5], msq.moe.grouped_qlinear(X[:cap - 5], PE, off, out_dtype=od))
    assert not bool((buf[:cap - 5] == -768.0).all(dim=1).any())


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_pack_unpack_and_expert_views(msq, O, family):
    K = 512
    V, PE = _values(family, K), _packed(family, K)
    assert np.array_equal(msq.moe.unpack_experts(PE).cpu().numpy(), V)                      # (d) exact
    assert torch.equal(msq.moe.unpack_experts(PE, torch.bfloat16).float().cpu(), torch.from_numpy(V))
    if family == "u6":
        assert PE.nbytes == E * N * K * 25 // 32 and PE.bits_per_element == 6.25          # (e)
    x = torch.randn(40, K, generator=torch.Generator().manual_seed(8)).to(torch.bfloat16)
    for e in range(E):
        P = PE.expert(e)
        assert P.out.data_ptr() == PE.out[e].data_ptr()                                    # a view, not a copy
        ref = O.linear(x.float().numpy(), V[e])
        y = msq.qlinear.qlinear(x.to(dev()), P, None, torch.float32).cpu().numpy()
        assert np.abs(y - ref).max() <= 2e-5 * np.abs(ref).max() + 1e-6


def test_pack_expert_values_picks_one_kind_for_the_stack(msq):
    Vx = torch.from_numpy(_values("u8x", 256)).to(dev())
    assert msq.moe.pack_expert_values(Vx).out_kind == U8X
    mixed = torch.from_numpy(_values("u8", 256).copy()).to(dev())
    assert msq.moe.pack_expert_values(mixed).out_kind == U8
    mixed[2] = Vx[2]                                             # ONE expert needs the extension bit: the whole stack takes it
    assert msq.moe.pack_expert_values(mixed).out_kind == U8X
    with pytest.raises(msq._lib.MsqError):
        msq.moe.pack_expert_values(mixed, (U8,))
    bad = mixed.clone(); bad[1, 3, 5] = float("nan")
    with pytest.raises(AssertionError):
        msq.moe.pack_expert_values(bad)
    PB = msq.moe.pack_expert_values(mixed, (4,))                 # a kind the grouped kernel does not read: refused, never a dense fall-back
    assert PB.out_kind == 4
    with pytest.raises(msq._lib.MsqError):
        msq.moe.grouped_qlinear(torch.zeros(4, 256, dtype=torch.bfloat16, device=dev()), PB, _offsets([1, 1, 1, 1]))


def test_wide_shape_vs_dense_bf16(msq):
    """E = 8, N = 2048, K = 1024, MSQ-U6: against x_e @ W_e^T on the unpacked bf16 weights (an independent library kernel, fp32
    accumulation): within one bf16 ulp of the result scale, the criterion of _dense_check"""
    Ew, Nw, Kw, counts = 8, 2048, 1024, [0, 3, 0, 17, 1, 0, 70, 2]
    V = torch.stack([msq.quant.outlier_fakequant(weights(Nw, Kw, 60 + e).to(dev()), 8, 8, "int2", "fp4", 2, 0, 16)["out"] for e in range(Ew)])
    assert fits_u6(V[:, :128].reshape(-1, Kw).cpu().numpy()) == 0
    PE = msq.moe.pack_expert_values(V, (U6,))
    assert PE.out_kind == U6 and PE.nbytes == Ew * Nw * Kw * 25 // 32
    Wb = msq.moe.unpack_experts(PE, torch.bfloat16)
    assert torch.equal(Wb.float(), V)
    R = sum(counts)
    g = torch.Generator(device=dev()).manual_seed(4)
    X = torch.randn(R + 11, Kw, generator=g, device=dev()).to(torch.bfloat16)
    ridx = torch.randint(0, R + 11, (R,), generator=g, device=dev()).to(torch.int32)
    off = torch.tensor([0] + list(np.cumsum(counts)), dtype=torch.int32, device=dev())
    y = msq.moe.grouped_qlinear(X, PE, off, ridx, out_dtype=torch.float32)
    ref = torch.empty_like(y)
    lo = 0
    for e, m in enumerate(counts):
        ref[lo:lo + m] = (X[ridx[lo:lo + m].long()] @ Wb[e].t()).float()
        lo += m
    err, scale = float((y - ref).abs().max()), float(ref.abs().max())
    print("wide: err %.3e, bound %.3e" % (err, 2.0 ** -8 * scale + 1e-6))
    assert err <= 2.0 ** -8 * scale + 1e-6
