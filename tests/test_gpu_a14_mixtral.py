"""SURVEY 8 row A14, mixture of experts (`get_llama(model_type="mixtral")`): the RTN harness quantises every expert's gate / up / down
weight of a Mixtral whose experts are stacked 3-D parameters, pack_layers swaps the experts for moe.QuantExperts (two grouped fused
dequant-GEMMs per block), the packed module computes what the dense fake-quantised experts compute, and one decode step through it is
captured in a HIP graph and replayed with another routing."""
import numpy as np
import pytest
import torch

from gpu_common import dev
from test_gpu_n1_unified6_pack import fits_u6

pytestmark = pytest.mark.gpu

KINDS = (8, 5, 6)                                               # MSQ-U6 first, then MSQ-U1 without / with the extension bit
H, NE, TOPK = 256, 4, 2


def _tiny_mixtral(intermediate=256, seed=0):
    from transformers import MixtralConfig, MixtralForCausalLM
    cfg = MixtralConfig(hidden_size=H, intermediate_size=intermediate, num_hidden_layers=1, num_attention_heads=4, num_key_value_heads=2,
                        num_local_experts=NE, num_experts_per_tok=TOPK, vocab_size=128, max_position_embeddings=64)
    torch.manual_seed(seed)
    model = MixtralForCausalLM(cfg).eval()
    model.config._experts_implementation = "eager"               # the dense yardstick is the expert module's own forward (the Python loop)
    model.model.layers[0].mlp.experts.config._experts_implementation = "eager"
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():                                        # the stacked parameters explicitly: BASELINE-style weights, 1 % outliers
        moe = model.model.layers[0].mlp
        for p in (moe.experts.gate_up_proj, moe.experts.down_proj):
            w = torch.randn(p.shape, generator=g) * 0.02
            w[torch.rand(p.shape, generator=g) < 0.01] *= 16
            p.copy_(w)
        moe.gate.weight.copy_(torch.randn(moe.gate.weight.shape, generator=g) * 0.5)
    return model.to(dev())


def _experts(model):
    return model.model.layers[0].mlp.experts


@pytest.mark.parametrize("intermediate", [256, 72])
def test_quantize_layers_nearest_reaches_the_experts(msq, O, intermediate):
    """every expert's gate half, up half and down weight is quantised as its own 2-D weight (int2 / fp4, blocks of 16 along out_features);
    intermediate 72: the halves are no multiple of the block, a block over the stacked [2I, H] weight would straddle gate and up"""
    from msq.harness.evalppl import quantize_layers_nearest
    model = _tiny_mixtral(intermediate)
    ex, router = _experts(model), model.model.layers[0].mlp.gate
    gu0, dn0, r0 = ex.gate_up_proj.detach().cpu().numpy().copy(), ex.down_proj.detach().cpu().numpy().copy(), router.weight.detach().clone()
    quantize_layers_nearest(model.model.layers, dev())
    gu1, dn1 = ex.gate_up_proj.detach().cpu().numpy(), ex.down_proj.detach().cpu().numpy()
    fq = lambda w: O.outlier_fakequant(np.ascontiguousarray(w), 8, 8, "int2", "fp4", 2, 0, 16)["out"]
    I = intermediate
    for e in range(NE):
        assert np.array_equal(gu1[e, :I], fq(gu0[e, :I])), ("gate", e)
        assert np.array_equal(gu1[e, I:], fq(gu0[e, I:])), ("up", e)
        assert np.array_equal(dn1[e], fq(dn0[e])), ("down", e)
        assert not np.array_equal(gu1[e], gu0[e]) and not np.array_equal(dn1[e], dn0[e])
    assert torch.equal(router.weight.detach(), r0)               # the router is left alone


def _quantized_pair():
    from msq.harness.evalppl import quantize_layers_nearest
    dense, packed = _tiny_mixtral(), _tiny_mixtral()
    for m in (dense, packed):
        quantize_layers_nearest(m.model.layers, dev())
    return dense, packed


def _routing(T, seed, experts=None):
    g = torch.Generator().manual_seed(seed)
    pool = list(range(NE)) if experts is None else list(experts)
    idx = torch.stack([torch.tensor(pool)[torch.randperm(len(pool), generator=g)[:TOPK]] for _ in range(T)])
    w = torch.rand(T, TOPK, generator=g) + 0.1
    return idx.to(dev()), (w / w.sum(-1, keepdim=True)).to(dev())


def test_quant_experts_module(msq):
    from msq.moe import QuantExperts, grouped_qlinear, route
    dense, _ = _quantized_pair()
    ex = _experts(dense)
    assert fits_u6(ex.gate_up_proj.data.reshape(-1, H).cpu().numpy()) == 0
    q = QuantExperts.from_module(ex, kinds=KINDS)
    assert q.out_kind == 8 and (q.num_experts, q.hidden_dim, q.intermediate_dim) == (NE, H, 256) and q.act_fn is ex.act_fn
    Wg, Wd = q.dequantize()
    assert torch.equal(Wg, ex.gate_up_proj.data.float()) and torch.equal(Wd, ex.down_proj.data.float())
    assert QuantExperts.from_module(ex).out_kind == 5            # the default kinds: MSQ-U1
    T = 48
    x = torch.randn(T, H, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16).to(dev())
    idx, w = _routing(T, 2)
    with torch.no_grad():
        y = q(x, idx, w)
        assert y.shape == x.shape and y.dtype == x.dtype
        # state_dict round trip into a fresh module
        fresh = QuantExperts(NE, H, 256, ex.act_fn, 8, 8, device=dev())
        assert set(fresh.state_dict()) == set(q.state_dict()) and len(q.state_dict()) == 6
        fresh.load_state_dict(q.state_dict())
        assert torch.equal(fresh(x, idx, w), y)
        # (i) the manual composition, bit for bit
        Pg, Pd = q.packed()
        ri, ro, inv = route(idx, NE)
        gu = grouped_qlinear(x, Pg, ro, ri, out_dtype=torch.bfloat16)
        hmid = ex.act_fn(gu[:, :256]) * gu[:, 256:]
        yd = grouped_qlinear(hmid, Pd, ro, out_dtype=torch.bfloat16)[inv].view(T, TOPK, H)
        manual = (yd[:, 0] * w[:, 0, None] + yd[:, 1] * w[:, 1, None]).to(torch.bfloat16)
        assert torch.equal(manual, y)
        # (ii) accuracy: float64 on the CPU, same weights, same routing; yardstick = the installed dense expert loop in bf16 on the GPU
        ref = torch.zeros(T, H, dtype=torch.float64)
        xd, Wg64, Wd64, w64, idc = x.double().cpu(), Wg.double().cpu(), Wd.double().cpu(), w.double().cpu(), idx.cpu()
        for t in range(T):
            for j in range(TOPK):
                e = int(idc[t, j])
                a = Wg64[e] @ xd[t]
                ref[t] += w64[t, j] * (Wd64[e] @ (torch.nn.functional.silu(a[:256]) * a[256:]))
        from transformers.models.mixtral.modeling_mixtral import MixtralExperts
        import copy
        cfg = copy.deepcopy(dense.config)
        cfg._experts_implementation = "eager"                    # the module's own forward: the Python loop over the experts that have rows
        dm = MixtralExperts(cfg).to(dev()).to(torch.bfloat16)
        dm.gate_up_proj.data.copy_(Wg); dm.down_proj.data.copy_(Wd)
        d_dense = float((dm(x, idx, w).double().cpu() - ref).abs().max())
        d_packed = float((y.double().cpu() - ref).abs().max())
        print("experts forward, T = 48: max |ref| %.3e, dense bf16 loop err %.3e, packed module err %.3e" % (float(ref.abs().max()), d_dense, d_packed))
        assert d_packed <= 2 * d_dense + 1e-6


def test_packed_experts_in_the_model_and_pack_layers(msq, tmp_path):
    from msq import checkpoint
    from msq.harness.evalppl import pack_expert_modules, pack_layers
    from msq.moe import QuantExperts
    dense, packed = _quantized_pair()
    assert pack_expert_modules(packed.model.layers, kinds=KINDS) == 1
    q = _experts(packed)
    assert isinstance(q, QuantExperts) and q.out_kind == 8
    assert not any(isinstance(m, msq.qlinear.QuantLinear) for m in packed.modules())       # attention stays dense: identical router inputs
    assert pack_expert_modules(packed.model.layers, kinds=KINDS) == 0
    x = torch.randint(0, 128, (2, 24), generator=torch.Generator().manual_seed(4)).to(dev())
    with torch.no_grad():
        yd, yp = dense(x).logits.float(), packed(x).logits.float()
    err, scale = (yd - yp).abs().max().item(), yd.abs().max().item()
    print("experts only packed, logits: max err %.3e, max |dense| %.3e, bound %.3e" % (err, scale, 2e-2 * scale))
    assert err <= 2e-2 * scale
    # pack_layers: the experts and the four attention Linears
    _, both = _quantized_pair()
    assert pack_layers(both.model.layers, kinds=KINDS + (4,)) == (4, 0)
    assert isinstance(_experts(both), QuantExperts) and _experts(both).out_kind == 8
    assert sum(isinstance(m, msq.qlinear.QuantLinear) for m in both.modules()) == 4
    with torch.no_grad():
        assert torch.isfinite(both(x).logits).all()
    with pytest.raises(msq._lib.MsqError, match="experts"):
        checkpoint.save_packed(both, str(tmp_path / "m.safetensors"))
    # a model without expert modules: what pack_layers returned before
    from test_gpu_a14_unified6_harness import _tiny_llama
    from msq.harness.evalppl import LLAMA_FUSE, quantize_layers_nearest
    llama = _tiny_llama()
    quantize_layers_nearest(llama.model.layers, dev())
    assert pack_layers(llama.model.layers, fuse=LLAMA_FUSE, kinds=(8, 5, 6, 4)) == (14, 0)


@pytest.mark.parametrize("T", [1, 4])
def test_decode_step_in_a_hip_graph(msq, T):
    """QuantExperts.forward has no host sync: captured, replayed, and replayed again after input AND routing buffers were overwritten with
    a routing that uses an expert which had no rows at capture"""
    from msq.moe import QuantExperts
    dense, _ = _quantized_pair()
    q = QuantExperts.from_module(_experts(dense), kinds=KINDS)
    g = torch.Generator().manual_seed(20 + T)
    x = torch.randn(T, H, generator=g).to(torch.bfloat16).to(dev())
    idx, w = _routing(T, 30 + T, experts=(0, 2, 3))              # expert 1 has no rows
    with torch.no_grad():
        eager = q(x, idx, w).clone()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(3):
                q(x, idx, w)
        torch.cuda.current_stream().wait_stream(s)
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            y = q(x, idx, w)
        for _ in range(3):
            gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(y, eager)
        x2 = torch.randn(T, H, generator=g).to(torch.bfloat16).to(dev())
        idx2, w2 = _routing(T, 40 + T, experts=(1, 2) if T == 1 else (0, 1, 2, 3))
        idx2[0] = torch.tensor([1, 3])                           # expert 1 gets rows now
        eager2 = q(x2, idx2, w2).clone()
        assert not torch.equal(eager2, eager)
        x.copy_(x2); idx.copy_(idx2); w.copy_(w2)
        gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(y, eager2)
