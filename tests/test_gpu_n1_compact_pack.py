"""SURVEY 8 row N1, compact layout MSQ-C1 (include/msq.h): pack -> unpack against the CPU oracle's fake-quant values, bit for bit.

Every comparison is against the oracle (or the HIP fake-quant that the a6 tests pin to it); before packing, each input is checked
against the layout's code model FROM THE ORACLE'S OWN mask / e_in / e_out, so a pass cannot come from an input the format could not hold."""
import json
import os

import numpy as np
import pytest
import torch

from gpu_common import G, dev, eq, weights

pytestmark = pytest.mark.gpu

CFGS = [("int2", "fp4", 16), ("int2", "fp4", 32), ("fp4_e2m1", "fp4_e2m1", 16), ("fp4_e2m1", "fp4_e2m1", 32), ("int2", "int2", 16)]
E2M1 = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])


def _small():
    """the 256 x 512 matrix of test_unified_pack_unpack_equals_fakequant (an all-zero group included)"""
    g = torch.Generator().manual_seed(1)
    W = torch.randn(256, 512, generator=g) * 0.02
    W[torch.rand(256, 512, generator=g) < 0.01] *= 20
    W[5, 64:96] = 0
    return W


def _fits_code_model(o, bs):
    """every value == e2m1 * 2^(mask ? e_out - e_in : e_in), scale bytes inside 1..254 (blocks along the last axis): misfit count"""
    out = np.asarray(o["out"], np.float64)
    mask = np.asarray(o["mask"]).astype(bool)
    e_in = np.repeat(np.asarray(o["e_in"], np.float64).reshape(out.shape[0], -1), bs, axis=1)[:, :out.shape[1]]
    e_out = np.repeat(np.asarray(o["e_out"], np.float64).reshape(out.shape[0], -1), bs, axis=1)[:, :out.shape[1]]
    code = np.abs(out) / np.exp2(np.where(mask, e_out - e_in, e_in))
    bad = ~np.isin(code, E2M1)
    bi, bo = e_in + 127, e_out - e_in + 127
    bad |= (bi < 1) | (bi > 254) | (mask & (out != 0) & ((bo < 1) | (bo > 254)))
    return int(bad.sum())


@pytest.mark.parametrize("fi,fo,bs", CFGS)
@pytest.mark.parametrize("which", ["small", "weights1024"])
def test_compact_pack_unpack_equals_oracle(msq, O, fi, fo, bs, which):
    W = _small() if which == "small" else weights(1024, 1024, 3)
    o = O.outlier_fakequant(W.numpy(), 8, 8, fi, fo, 2, -1, bs)
    assert _fits_code_model(o, bs) == 0
    P = msq.qlinear.pack_weight(W.to(dev()), 8, 8, fi, fo, 2, bs, layout="compact")
    assert (P.in_kind, P.out_kind) == (1, 7)
    assert P.bits_per_element == (6.0 if bs == 16 else 5.5)
    assert eq(msq.qlinear.unpack_weight(P, torch.float32).cpu().numpy(), o["out"])
    assert eq(msq.qlinear.unpack_weight(P, torch.bfloat16).float().cpu().numpy(), o["out"])


def test_reference_goldens_that_fit_the_layout(msq):
    """int2 / fp4 cases of the reference-made golden whose blocks run along the last axis with block 16 or 32, round nearest.
    The golden file holds NONE (its int2 / fp4 case runs along axis 0): found = 0, the oracle cases above carry the parity."""
    z = np.load(os.path.join(G, "outlier_fakequant.npz"))
    meta = json.load(open(os.path.join(G, "outlier_fakequant_meta.json")))
    e2m1 = ("int2", "fp4", "fp4_e2m1")
    found = 0
    for key, m in sorted(meta.items()):
        if "assert" in m:
            continue
        isb, osb, ifmt, ofmt, sd, ax, bs, rnd = m["cfg"]
        A = z["in|%s" % key.split("|")[1]]
        if not (ifmt in e2m1 and ofmt in e2m1 and bs in (16, 32) and rnd == "nearest" and A.ndim == 2 and [a % A.ndim for a in ax] == [A.ndim - 1]):
            continue
        found += 1
        P = msq.qlinear.pack_weight(torch.from_numpy(np.ascontiguousarray(A)).to(dev()), isb, osb, ifmt, ofmt, sd, bs, layout="compact")
        assert eq(msq.qlinear.unpack_weight(P).cpu().numpy(), z["out|%s" % key]), key
    print("reference goldens that fit the compact layout: %d" % found)
    assert found == 0


@pytest.mark.parametrize("bs", [16, 32])
def test_off_grid_shape(msq, O, bs):
    W = weights(300, 200, 11)
    o = O.outlier_fakequant(W.numpy(), 8, 8, "int2", "fp4", 2, -1, bs)
    assert _fits_code_model(o, bs) == 0
    P = msq.qlinear.pack_weight(W.to(dev()), 8, 8, "int2", "fp4", 2, bs, layout="compact")
    assert (P.n, P.k, P.N, P.K) == (300, 200, 512, 256)
    Wu = msq.qlinear.unpack_weight(P, torch.float32)
    assert tuple(Wu.shape) == (300, 200) and eq(Wu.cpu().numpy(), o["out"])


def test_limits(msq):
    Err = msq._lib.MsqError
    W = weights(256, 256, 5).to(dev())
    with pytest.raises(Err, match="compact"):
        msq.qlinear.pack_weight(W, 8, 8, "int2", "fp8_e4m3", 2, 16, layout="compact")
    with pytest.raises(Err, match="compact"):
        msq.qlinear.pack_weight(W, 8, 8, "int2", "fp4", 2, 64, layout="compact")
    for dt in (torch.float16, torch.bfloat16):
        with pytest.raises(Err, match="float32"):
            msq.qlinear.pack_weight(W.to(dt), 8, 8, "int2", "fp4", 2, 16, layout="compact", compute_dtype="input")
        P = msq.qlinear.pack_weight(W.to(dt), 8, 8, "int2", "fp4", 2, 16, layout="compact", compute_dtype="float32")
        assert (P.in_kind, P.out_kind) == (1, 7)
    with pytest.raises(Err, match="compact"):                     # other roundings are not built for the layout
        msq.qlinear.pack_weight(W, 8, 8, "int2", "fp4", 2, 16, round="floor", layout="compact")
    with pytest.raises(Err, match="compact"):
        msq.qlinear.pack_weight(W, 8, 8, "int2", "fp4", 2, 16, variant=1, layout="compact")
    # the other layouts select what they selected
    Pa = msq.qlinear.pack_weight(W, 8, 8, "int2", "fp4", 2, 16, layout="auto")
    Pp = msq.qlinear.pack_weight(W, 8, 8, "int2", "fp4", 2, 16, layout="planes")
    assert (Pa.in_kind, Pa.out_kind) == (0, 5) and (Pp.in_kind, Pp.out_kind) == (1, 2)


def test_whole_size_once(msq):
    N, K = 16384, 4096
    g = torch.Generator(device=dev()).manual_seed(3)
    W = torch.randn(N, K, generator=g, device=dev()) * 0.02
    W[torch.rand(N, K, generator=g, device=dev()) < 0.01] *= 16
    P = msq.qlinear.pack_weight(W, 8, 8, "int2", "fp4", 2, 16, layout="compact")
    assert P.nbytes == N * K * 6 // 8 and (P.in_kind, P.out_kind) == (1, 7)
    Wq = msq.quant.outlier_fakequant(W, 8, 8, "int2", "fp4", 2, -1, 16)["out"]
    assert torch.equal(msq.qlinear.unpack_weight(P, torch.float32), Wq)
    assert torch.equal(msq.qlinear.unpack_weight(P, torch.bfloat16).float(), Wq)
