"""Compact packed layout MSQ-C1 (include/msq.h: one e2m1 nibble + one select bit per weight + two E8M0 bytes per block), host logic
only: plane kinds, exact sizes (6.0 / 5.5 bits per weight), the kernel families the dispatcher names for it, the Python surface and
the checkpoint writer's version rule.  No GPU, no launch."""
import ctypes as C
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FP4, SEL, UNSUPPORTED = 1, 7, -2
DECODE, GEMM128 = 0, 1


@pytest.fixture(scope="module")
def msq():
    import __graft_entry__ as ge
    if not os.path.exists(os.path.join(ROOT, "microscopiq-llm-quantization_amd", "libmsq_hip.so")):
        ge.build()
    import msq as m
    return m


def _kinds(msq, fi, fo, layout=2):
    ik, ok = C.c_int(-1), C.c_int(-1)
    rc = msq._lib.lib().msq_packed_kinds_layout(msq.formats.format_id(fi), msq.formats.format_id(fo), layout, C.byref(ik), C.byref(ok))
    return rc, ik.value, ok.value


@pytest.mark.parametrize("fi", ["int2", "fp4_e2m1"])
@pytest.mark.parametrize("fo", ["fp4_e2m1", "int2"])
def test_kinds_of_the_eligible_formats(msq, fi, fo):
    assert _kinds(msq, fi, fo) == (0, FP4, SEL)
    assert msq.qlinear.packed_kinds(fi, fo, layout="compact") == (FP4, SEL)
    assert msq.qlinear.packed_kinds(fi, fo, layout=msq.qlinear.LAYOUT_COMPACT) == (FP4, SEL)
    assert (msq.qlinear.LAYOUT_COMPACT, msq.qlinear.PLANE_SEL) == (2, 7)


@pytest.mark.parametrize("fi,fo", [("fp4_e2m1", "fp8_e4m3"), ("int2", "posit8_es1"), ("fp4_e2m1", "int4"), ("int2", "fp8_e5m2"),
                                   ("fp6_e3m2", "fp4_e2m1"), ("fp6_e2m3", "int2")])
def test_other_formats_are_refused_with_a_message(msq, fi, fo):
    rc, _, _ = _kinds(msq, fi, fo)
    assert rc == UNSUPPORTED
    assert len(msq._lib.lib().msq_last_error()) > 0
    with pytest.raises(msq._lib.MsqError):
        msq.qlinear.packed_kinds(fi, fo, layout="compact")


def test_the_other_layouts_select_what_they_selected(msq):
    assert _kinds(msq, "int2", "fp4_e2m1", 0)[1:] == (1, 2) and _kinds(msq, "int2", "fp4_e2m1", 1)[1:] == (0, 5)
    assert msq.qlinear.packed_kinds("int2", "fp4", "planes") == (1, 2) and msq.qlinear.packed_kinds("int2", "fp4", "unified") == (0, 5)


@pytest.mark.parametrize("N,K", [(4096, 4096), (16384, 4096), (4096, 11008)])
@pytest.mark.parametrize("block,bits", [(16, 6.0), (32, 5.5)])
def test_sizes_are_exact(msq, N, K, block, bits):
    ib, ob, sb, wb = msq.qlinear.packed_sizes(N, K, block, FP4, SEL)
    tiles = N * K // 4096
    assert (ib, ob, sb) == (tiles * 2048, tiles * 512, 2 * N * K // block)
    assert 8.0 * (ib + ob + sb) / (N * K) == bits


@pytest.mark.parametrize("block", [8, 64, 128])
def test_other_blocks_are_refused(msq, block):
    z = C.c_int64()
    rc = msq._lib.lib().msq_packed_sizes(4096, 4096, block, FP4, SEL, C.byref(z), C.byref(z), C.byref(z), C.byref(z))
    assert rc == UNSUPPORTED and len(msq._lib.lib().msq_last_error()) > 0


@pytest.mark.parametrize("N,K", [(12288, 4096), (22016, 4096), (4096, 4096), (4096, 11008)])
def test_kernel_families(msq, N, K):
    """decode kernels up to 32 rows, the 128-row GEMM with split-K above; never a kernel that is not built for the kind"""
    lib = msq._lib.lib()
    for M in (1, 16, 32):
        assert lib.msq_qlinear_kernel_choice(M, N, K, SEL, -1) == DECODE, (M, N, K)
    for M in (128, 2048):
        assert lib.msq_qlinear_kernel_choice(M, N, K, SEL, -1) == GEMM128, (M, N, K)
    for M in (1, 8, 16, 17, 32, 33, 48, 64, 65, 100, 128, 129, 256, 300, 512, 1024, 2048, 4096):
        assert lib.msq_qlinear_kernel_choice(M, N, K, SEL, -1) in (DECODE, GEMM128), (M, N, K)
    buf = C.create_string_buffer(128)
    assert lib.msq_qlinear_kernel_name(16, N, K, SEL, -1, 2, buf, 128) == 0
    assert buf.value.decode().startswith("k_qgemv_u<7, " if N > 8192 else "k_qgemv<1, 7, "), buf.value
    assert lib.msq_qlinear_kernel_name(2048, N, K, SEL, -1, 2, buf, 128) == 0
    assert buf.value.decode().startswith("k_qgemm3<1, 7, "), buf.value


def test_checkpoint_version_rule(msq, tmp_path):
    """A file that holds a compact layer is written as version 3 and loads back; a file without one is version 2 as before."""
    from msq import checkpoint
    from msq.qlinear import QuantLinear

    class Net(torch.nn.Module):
        def __init__(self, packed, lay_b):
            super().__init__()
            if packed:
                self.a = QuantLinear(128, 256, True, 32, "fp4_e2m1", "fp8_e4m3", layout="unified")
                self.b = QuantLinear(256, 512, True, 16, "int2", "fp4_e2m1", layout=lay_b)
            else:
                self.a, self.b = torch.nn.Linear(128, 256), torch.nn.Linear(256, 512)

    g = torch.Generator().manual_seed(0)
    for lay_b, version in (("compact", 3), ("planes", 2)):
        src = Net(True, lay_b)
        for m in (src.a, src.b):
            for buf in (m.inl_plane, m.out_plane, m.scale_plane):
                if buf.numel():
                    buf.copy_(torch.randint(0, 256, buf.shape, generator=g, dtype=torch.uint8))
        path = str(tmp_path / ("m_%s.safetensors" % lay_b))
        hdr = checkpoint.save_packed(src, path)
        assert hdr["version"] == version and checkpoint.read_header(path)["version"] == version
        assert hdr["layers"]["b"]["layout"] == lay_b
        if lay_b == "compact":
            assert (hdr["layers"]["b"]["in_kind"], hdr["layers"]["b"]["out_kind"]) == (FP4, SEL)
            assert src.b.inl_plane.numel() + src.b.out_plane.numel() + src.b.scale_plane.numel() == 256 * 512 * 6 // 8
        dst = Net(False, lay_b)
        checkpoint.load_packed(dst, path)
        assert isinstance(dst.b, QuantLinear) and dst.b.layout == lay_b and (dst.b.in_kind, dst.b.out_kind) == (src.b.in_kind, src.b.out_kind)
        for k, v in src.state_dict().items():
            assert torch.equal(v, dst.state_dict()[k]), k
