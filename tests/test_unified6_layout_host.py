"""Six-bit unified layout MSQ-U6 (include/msq.h: the top six bits of the MSQ-U1 code of every weight + MSQ-U1's scale plane), host logic
only: plane kinds, exact sizes (6.25 bits per weight), the kernel families and instantiations the dispatcher names for the kind, the
Python surface and the checkpoint writer's version rule.  No GPU, no launch."""
import ctypes as C
import json
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NONE, U6, UNSUPPORTED, BAD_ARG = 0, 8, -2, -1
DECODE, GEMM128 = 0, 1
MS = (1, 8, 16, 17, 32, 33, 48, 64, 65, 100, 128, 129, 256, 300, 512, 1024, 2048, 4096)


@pytest.fixture(scope="module")
def msq():
    import __graft_entry__ as ge
    if not os.path.exists(os.path.join(ROOT, "microscopiq-llm-quantization_amd", "libmsq_hip.so")):
        ge.build()
    import msq as m
    return m


def _kinds(msq, fi, fo, layout=3):
    ik, ok = C.c_int(-1), C.c_int(-1)
    rc = msq._lib.lib().msq_packed_kinds_layout(msq.formats.format_id(fi), msq.formats.format_id(fo), layout, C.byref(ik), C.byref(ok))
    return rc, ik.value, ok.value


@pytest.mark.parametrize("fi,fo", [("int2", "fp4_e2m1"), ("fp4_e2m1", "fp4_e2m1"), ("int2", "int2")])
def test_kinds_of_the_eligible_formats(msq, fi, fo):
    assert _kinds(msq, fi, fo) == (0, NONE, U6)
    assert msq.qlinear.packed_kinds(fi, fo, layout="unified6") == (NONE, U6)
    assert msq.qlinear.packed_kinds(fi, fo, layout=msq.qlinear.LAYOUT_UNIFIED6) == (NONE, U6)
    assert (msq.qlinear.LAYOUT_UNIFIED6, msq.qlinear.PLANE_U6) == (3, 8)
    assert msq.qlinear._layout_of(msq.qlinear.PLANE_U6) == "unified6"


@pytest.mark.parametrize("fi,fo", [("fp4_e2m1", "fp8_e4m3"), ("int2", "posit8_es1"), ("fp6_e3m2", "fp4_e2m1"), ("fp4_e2m1", "int4")])
def test_other_formats_are_refused_with_a_message(msq, fi, fo):
    rc, _, _ = _kinds(msq, fi, fo)
    assert rc == UNSUPPORTED
    assert len(msq._lib.lib().msq_last_error()) > 0
    with pytest.raises(msq._lib.MsqError):
        msq.qlinear.packed_kinds(fi, fo, layout="unified6")


def test_the_other_layouts_select_what_they_selected(msq):
    assert _kinds(msq, "int2", "fp4_e2m1", 0)[1:] == (1, 2) and _kinds(msq, "int2", "fp4_e2m1", 1)[1:] == (0, 5)
    assert _kinds(msq, "int2", "fp4_e2m1", 2)[1:] == (1, 7)
    assert _kinds(msq, "fp4_e2m1", "fp8_e4m3", 1)[1:] == (0, 5) and _kinds(msq, "fp4_e2m1", "posit8_es1", 1)[1:] == (0, 6)
    assert msq.qlinear.packed_kinds("int2", "fp4", "planes") == (1, 2) and msq.qlinear.packed_kinds("int2", "fp4", "unified") == (0, 5)
    assert msq.qlinear.packed_kinds("int2", "fp4", "compact") == (1, 7)


@pytest.mark.parametrize("N,K", [(4096, 4096), (16384, 4096), (4096, 11008)])
def test_sizes_are_exact(msq, N, K):
    ib, ob, sb, wb = msq.qlinear.packed_sizes(N, K, 32, NONE, U6)
    tiles = N * K // 4096
    assert ib + ob + sb == tiles * (3072 + 128) and sb == tiles * 128 and wb == 0
    assert (ib + ob + sb) * 8 == N * K * 25 // 4 and 8.0 * (ib + ob + sb) / (N * K) == 6.25


def test_an_inlier_plane_kind_is_refused(msq):
    z = C.c_int64()
    rc = msq._lib.lib().msq_packed_sizes(4096, 4096, 32, 1, U6, C.byref(z), C.byref(z), C.byref(z), C.byref(z))
    assert rc in (UNSUPPORTED, BAD_ARG) and len(msq._lib.lib().msq_last_error()) > 0


@pytest.mark.parametrize("N,K", [(12288, 4096), (22016, 4096), (4096, 4096), (4096, 11008)])
def test_kernel_families(msq, N, K):
    """decode kernels or the 128-row GEMM (k_qgemm3, split-K where it pays), never a kernel that is not built for the kind; the names are
    those of the instantiations the dispatcher launches"""
    lib = msq._lib.lib()
    for M in (1, 16, 32):
        assert lib.msq_qlinear_kernel_choice(M, N, K, U6, -1) == DECODE, (M, N, K)
    for M in (128, 2048):
        assert lib.msq_qlinear_kernel_choice(M, N, K, U6, -1) == GEMM128, (M, N, K)
    for M in MS:
        assert lib.msq_qlinear_kernel_choice(M, N, K, U6, -1) in (DECODE, GEMM128), (M, N, K)
        assert lib.msq_qlinear_kernel_choice(M, N, K, U6, -1) == lib.msq_qlinear_kernel_choice(M, N, K, 7, -1), (M, N, K)   # routed as MSQ-C1 is
    buf = C.create_string_buffer(128)
    assert lib.msq_qlinear_kernel_name(16, N, K, U6, -1, 2, buf, 128) == 0
    assert buf.value.decode().startswith("k_qgemv_u<8, " if N > 8192 else "k_qgemv<0, 8, "), buf.value
    assert lib.msq_qlinear_kernel_name(2048, N, K, U6, -1, 2, buf, 128) == 0
    assert buf.value.decode().startswith("k_qgemm3<0, 8, "), buf.value


def test_checkpoint_version_rule(msq, tmp_path):
    """version 4 with a unified6 layer (compact layers may ride along), 3 with compact only, 2 otherwise; a version-4 header without a
    unified6 layer is refused with the version in the message"""
    from msq import checkpoint
    from msq.qlinear import QuantLinear

    class Net(torch.nn.Module):
        def __init__(self, packed, lay_b, lay_c):
            super().__init__()
            if packed:
                self.a = QuantLinear(128, 256, True, 32, "fp4_e2m1", "fp8_e4m3", layout="unified")
                self.b = QuantLinear(256, 512, True, 16, "int2", "fp4_e2m1", layout=lay_b)
                self.c = QuantLinear(512, 256, False, 16, "int2", "fp4_e2m1", layout=lay_c)
            else:
                self.a, self.b, self.c = torch.nn.Linear(128, 256), torch.nn.Linear(256, 512), torch.nn.Linear(512, 256, bias=False)

    g = torch.Generator().manual_seed(0)
    for lay_b, lay_c, version in (("unified6", "planes", 4), ("unified6", "compact", 4), ("compact", "planes", 3), ("planes", "unified", 2)):
        src = Net(True, lay_b, lay_c)
        for m in (src.a, src.b, src.c):
            for buf in (m.inl_plane, m.out_plane, m.scale_plane):
                if buf.numel():
                    buf.copy_(torch.randint(0, 256, buf.shape, generator=g, dtype=torch.uint8))
        path = str(tmp_path / ("m_%s_%s.safetensors" % (lay_b, lay_c)))
        hdr = checkpoint.save_packed(src, path)
        assert hdr["version"] == version and checkpoint.read_header(path)["version"] == version
        assert hdr["layers"]["b"]["layout"] == lay_b
        if lay_b == "unified6":
            assert (hdr["layers"]["b"]["in_kind"], hdr["layers"]["b"]["out_kind"]) == (NONE, U6)
            assert src.b.inl_plane.numel() + src.b.out_plane.numel() + src.b.scale_plane.numel() == 256 * 512 * 25 // 32
        dst = Net(False, lay_b, lay_c)
        checkpoint.load_packed(dst, path)
        assert isinstance(dst.b, QuantLinear) and dst.b.layout == lay_b and (dst.b.in_kind, dst.b.out_kind) == (src.b.in_kind, src.b.out_kind)
        for k, v in src.state_dict().items():
            assert torch.equal(v, dst.state_dict()[k]), k
    # a "version 4" header that holds no unified6 layer comes from some other definition of that number
    from safetensors.torch import save_file
    src = Net(True, "compact", "planes")
    hdr = checkpoint.save_packed(src, str(tmp_path / "v3.safetensors"))
    hdr["version"] = 4
    bad = str(tmp_path / "v4_without.safetensors")
    save_file({k: v.contiguous() for k, v in src.state_dict().items()}, bad, metadata={"msq": json.dumps(hdr)})
    with pytest.raises(msq._lib.MsqError, match="version 4"):
        checkpoint.read_header(bad)
    m = QuantLinear.empty_single_plane(256, 512, False, out_kind=8)
    assert m.layout == "unified6" and (m.in_kind, m.out_kind) == (NONE, U6)
