"""SURVEY 8 row A14, six-bit unified layout MSQ-U6: the harness default configuration (int2 inliers / fp4 outliers, blocks of 16 along
out_features, RTN) packed through pack_layers(kinds=(8, 5, 6, 4)): every layer lands in MSQ-U6, 6.25 / 8.25 of the default result's bytes,
and the model computes what the dense fake-quantised model computes."""
import pytest
import torch

from gpu_common import dev
from test_gpu_n1_unified6_pack import fits_u6

pytestmark = pytest.mark.gpu


def _tiny_llama():
    """the two-layer decoder stack the a14 tests build"""
    from transformers import LlamaConfig, LlamaForCausalLM
    cfg = LlamaConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4,
                      num_key_value_heads=4, vocab_size=512, max_position_embeddings=128)
    torch.manual_seed(0)
    return LlamaForCausalLM(cfg).eval().to(dev())


def _packed_bytes(msq, model):
    return sum(l._packed().nbytes for l in model.modules() if isinstance(l, msq.qlinear.QuantLinear))


def test_pack_layers_with_the_six_bit_kind(msq):
    from msq.harness import find_layers
    from msq.harness.evalppl import LLAMA_FUSE, pack_layers, quantize_layers_nearest
    dense, a, b = _tiny_llama(), _tiny_llama(), _tiny_llama()
    for m in (dense, a, b):
        quantize_layers_nearest(m.model.layers, dev())            # DEFAULT_QUANT: int2 / fp4, axes=[0], block 16
    for layer in dense.model.layers:
        for name, lin in find_layers(layer).items():
            assert fits_u6(lin.weight.data.float().cpu().numpy()) == 0, name
    assert pack_layers(a.model.layers, fuse=LLAMA_FUSE) == (14, 0)
    assert pack_layers(b.model.layers, fuse=LLAMA_FUSE, kinds=(8, 5, 6, 4)) == (14, 0)
    qa = [l for l in a.modules() if isinstance(l, msq.qlinear.QuantLinear)]
    qb = [l for l in b.modules() if isinstance(l, msq.qlinear.QuantLinear)]
    assert len(qa) == len(qb) == 8
    assert all(l.out_kind == 5 for l in qa)                         # without `kinds`: what pack_layers did before
    assert all(l.out_kind == 8 and l.layout == "unified6" for l in qb)
    assert _packed_bytes(msq, b) * 33 == _packed_bytes(msq, a) * 25  # 6.25 / 8.25
    att_d, att_b = dense.model.layers[0].self_attn, b.model.layers[0].self_attn
    Wf = att_b.q_proj.shared().proj.dequantize()
    for i, n in enumerate(("q_proj", "k_proj", "v_proj")):
        assert torch.equal(Wf[256 * i:256 * (i + 1)], getattr(att_d, n).weight.data.float())
    x = torch.randint(0, 512, (2, 24), generator=torch.Generator().manual_seed(4)).to(dev())
    with torch.no_grad():
        yd, yb = dense(x).logits.float(), b(x).logits.float()
    err, scale = (yd - yb).abs().max().item(), yd.abs().max().item()
    print("logits: max err %.3e, max |dense| %.3e, bound %.3e" % (err, scale, 2e-2 * scale))
    # the same weights; bf16 activations and another summation order: the bound test_fused_projections_same_values_fewer_launches uses
    # on the logits and test_pack_layers_in_half_precision_model on the perplexity against the dense fake-quantised model (2 %)
    assert err <= 2e-2 * scale
