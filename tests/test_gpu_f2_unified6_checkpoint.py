"""SURVEY 8 row F2, six-bit unified layout MSQ-U6: a model with one U6 layer (packed from axis-0 fake-quant values) and one unified layer
survives save / load (header version 4, layout "unified6", kinds (0, 8)) and computes the same bits afterwards; without the U6 layer the
same model is written as version 2."""
import pytest
import torch

from gpu_common import dev, weights
from test_gpu_n1_unified6_pack import fits_u6

pytestmark = pytest.mark.gpu


class Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.a = torch.nn.Linear(512, 768, bias=True)
        self.b = torch.nn.Linear(768, 256, bias=False)

    def forward(self, x):
        return self.b(torch.nn.functional.relu(self.a(x)))


def test_unified6_checkpoint_roundtrip(msq, tmp_path):
    from msq import checkpoint
    from msq.qlinear import QuantLinear
    from msq.quant import MXQuantizer
    src = Net()
    with torch.no_grad():
        src.a.weight.copy_(weights(768, 512, 61)); src.b.weight.copy_(weights(256, 768, 62))
    src = src.to(dev())
    Va = msq.quant.outlier_fakequant(src.a.weight.data, 8, 8, "int2", "fp4", 2, 0, 16)["out"]      # the harness default: blocks along out_features
    assert fits_u6(Va.cpu().numpy()) == 0
    dense_a = torch.nn.Linear(512, 768, bias=True).to(dev())
    with torch.no_grad():
        dense_a.weight.copy_(Va); dense_a.bias.copy_(src.a.bias)
    qb = MXQuantizer()
    qb.configure(8, 8, "fp4_e2m1", "fp8_e4m3", "max", 2, [-1], 32)
    src.a = QuantLinear.from_dense(dense_a, kinds=(8, 5, 6, 4))
    src.b = QuantLinear.from_linear(src.b, qb, layout="unified")
    assert (src.a.in_kind, src.a.out_kind) == (0, 8) and src.b.out_kind == 5
    assert torch.equal(src.a.dequantize(), Va)
    x = torch.randn(7, 512, device=dev()).to(torch.bfloat16)
    with torch.no_grad():
        y0 = src(x)
    path = str(tmp_path / "unified6.safetensors")
    hdr = checkpoint.save_packed(src, path)
    assert hdr["version"] == 4 and checkpoint.read_header(path)["version"] == 4
    la = hdr["layers"]["a"]
    assert (la["layout"], la["in_kind"], la["out_kind"], la["block_size"]) == ("unified6", 0, 8, 32)
    assert hdr["layers"]["b"]["layout"] == "unified"
    dst = Net().to(dev())
    checkpoint.load_packed(dst, path)
    assert isinstance(dst.a, QuantLinear) and dst.a.layout == "unified6" and (dst.a.in_kind, dst.a.out_kind) == (0, 8)
    for k, v in src.state_dict().items():
        assert torch.equal(v, dst.state_dict()[k]), k
    with torch.no_grad():
        assert torch.equal(dst(x), y0)
    assert torch.equal(dst.a.dequantize(), Va)
    # the same model without the U6 layer is still written as version 2
    src.a = QuantLinear.from_dense(dense_a)
    assert src.a.out_kind == 5
    assert checkpoint.save_packed(src, str(tmp_path / "unified.safetensors"))["version"] == 2
