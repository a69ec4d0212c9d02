"""SURVEY 8 row F2, compact layout MSQ-C1: a model with one compact and one unified layer survives save / load (header version 3,
layout "compact", kinds (1, 7)) and computes the same bits afterwards."""
import pytest
import torch

from gpu_common import dev, weights

pytestmark = pytest.mark.gpu


class Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.a = torch.nn.Linear(512, 768, bias=True)
        self.b = torch.nn.Linear(768, 256, bias=False)

    def forward(self, x):
        return self.b(torch.nn.functional.relu(self.a(x)))


def test_compact_checkpoint_roundtrip(msq, tmp_path):
    from msq import checkpoint
    from msq.qlinear import QuantLinear
    from msq.quant import MXQuantizer
    src = Net()
    with torch.no_grad():
        src.a.weight.copy_(weights(768, 512, 61)); src.b.weight.copy_(weights(256, 768, 62))
    src = src.to(dev())
    qa, qb = MXQuantizer(), MXQuantizer()
    qa.configure(8, 8, "int2", "fp4", "max", 2, [-1], 16)
    qb.configure(8, 8, "fp4_e2m1", "fp8_e4m3", "max", 2, [-1], 32)
    src.a = QuantLinear.from_linear(src.a, qa, layout="compact", compute_dtype="float32")
    src.b = QuantLinear.from_linear(src.b, qb, layout="unified")
    assert (src.a.in_kind, src.a.out_kind) == (1, 7) and src.b.out_kind == 5
    x = torch.randn(7, 512, device=dev()).to(torch.bfloat16)
    with torch.no_grad():
        y0 = src(x)
    path = str(tmp_path / "compact.safetensors")
    hdr = checkpoint.save_packed(src, path)
    assert hdr["version"] == 3 and checkpoint.read_header(path)["version"] == 3
    la = hdr["layers"]["a"]
    assert (la["layout"], la["in_kind"], la["out_kind"], la["block_size"]) == ("compact", 1, 7, 16)
    assert hdr["layers"]["b"]["layout"] == "unified"
    dst = Net().to(dev())
    checkpoint.load_packed(dst, path)
    assert isinstance(dst.a, QuantLinear) and dst.a.layout == "compact" and (dst.a.in_kind, dst.a.out_kind) == (1, 7)
    for k, v in src.state_dict().items():
        assert torch.equal(v, dst.state_dict()[k]), k
    with torch.no_grad():
        assert torch.equal(dst(x), y0)
    # a model without a compact layer is still written as version 2
    src.a = QuantLinear.from_linear(Net().a.to(dev()), qa, layout="planes")
    assert checkpoint.save_packed(src, str(tmp_path / "planes.safetensors"))["version"] == 2
