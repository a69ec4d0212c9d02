"""Packed mixture of experts, host side (no GPU): the router-to-rows map `msq.moe.route` on CPU tensors, the launch plan of the grouped fused
dequant-GEMM (msq_qlinear_grouped_plan: host arithmetic of libmsq_hip.so) against a brute force over the splits of the rows, and the
harness's duck-typed `find_experts` on a tiny Mixtral built from a config."""
import ctypes as C
import itertools
import random

import pytest
import torch

U8, U8X, U6 = 5, 6, 8
UNSUPPORTED = -2


def _msq():
    import msq
    msq._lib.lib()
    return msq


@pytest.mark.parametrize("T", [1, 7, 64])
@pytest.mark.parametrize("E", [4, 8])
def test_route_on_cpu_tensors(T, E):
    moe = _msq().moe
    k = 2
    g = torch.Generator().manual_seed(100 * T + E)
    idx = torch.stack([torch.randperm(E, generator=g)[:k] for _ in range(T)])
    if T == 64:
        idx[idx == 1] = 2                                     # an expert without rows in the middle
    row_index, row_offsets, inverse = moe.route(idx, E)
    assert row_index.dtype == torch.int32 and row_offsets.dtype == torch.int32 and inverse.dtype == torch.int64
    assert tuple(row_index.shape) == (T * k,) and tuple(row_offsets.shape) == (E + 1,) and tuple(inverse.shape) == (T * k,)
    counts = torch.bincount(idx.reshape(-1), minlength=E)
    assert row_offsets.tolist() == [0] + torch.cumsum(counts, 0).tolist()
    flat = idx.reshape(-1)
    for e in range(E):
        lo, hi = int(row_offsets[e]), int(row_offsets[e + 1])
        if counts[e] == 0:
            assert lo == hi                                  # equal consecutive offsets
        pos = [p for p in range(T * k) if flat[p] == e]       # flat (token, slot) positions of the expert, ascending
        assert row_index[lo:hi].tolist() == [p // k for p in pos]
        assert [int(inverse[p]) for p in pos] == list(range(lo, hi))
    # row_index and inverse are consistent: sorted row inverse[t, j] reads token t and belongs to expert idx[t, j]
    assert sorted(inverse.tolist()) == list(range(T * k))
    for t in range(T):
        for j in range(k):
            r = int(inverse[t * k + j])
            assert int(row_index[r]) == t and int(row_offsets[idx[t, j]]) <= r < int(row_offsets[idx[t, j] + 1])


def _plan(lib, rows, E, N=256, K=256, kind=U6):
    rt, ts, nb = C.c_int(-1), C.c_int(-1), C.c_int64(-1)
    rc = lib.msq_qlinear_grouped_plan(rows, E, N, K, kind, C.byref(rt), C.byref(ts), C.byref(nb))
    return rc, rt.value, ts.value, nb.value


def _splits(rows, E):
    """every split of `rows` into E counts, or a seeded sample of 2000 (corner splits included) where there are too many"""
    import math
    if math.comb(rows + E - 1, E - 1) <= 30000:
        for cuts in itertools.combinations_with_replacement(range(rows + 1), E - 1):
            edges = (0,) + cuts + (rows,)
            yield [edges[i + 1] - edges[i] for i in range(E)]
        return
    rnd = random.Random(1000 * rows + E)
    yield [rows] + [0] * (E - 1)
    yield [1] * (E - 1) + [rows - (E - 1)]                      # E - 1 part-filled tiles and the rest
    yield [rows // E + (1 if i < rows % E else 0) for i in range(E)]
    for _ in range(2000):
        edges = [0] + sorted(rnd.randint(0, rows) for _ in range(E - 1)) + [rows]
        yield [edges[i + 1] - edges[i] for i in range(E)]


@pytest.mark.parametrize("E", [1, 3, 8])
@pytest.mark.parametrize("rows", [0, 1, 63, 64, 65, 200])
def test_grouped_plan_bounds_every_split(rows, E):
    lib = _msq()._lib.lib()
    for kind in (U8, U8X, U6):
        rc, rt, slots, blocks = _plan(lib, rows, E, 512, 256, kind)
        assert rc == 0 and rt > 0 and rt % 16 == 0
        assert blocks == (512 // 64) * slots
    ceil = lambda a: (a + rt - 1) // rt
    worst = 0
    for m in _splits(rows, E):
        assert sum(m) == rows and len(m) == E
        worst = max(worst, sum(ceil(v) for v in m))
    assert worst <= slots <= ceil(rows) + E, (rows, E, worst, slots)


def test_grouped_plan_refuses_other_kinds_and_shapes():
    msq = _msq()
    lib = msq._lib.lib()
    for kind in (1, 2, 3, 4, 7):                                 # fp4 / fp8 / bf8 (MSQ-T1 planes), bf16, select bits
        assert _plan(lib, 64, 4, 256, 256, kind)[0] == UNSUPPORTED, kind
    assert _plan(lib, 64, 4, 320, 256)[0] == UNSUPPORTED         # N % 256
    assert _plan(lib, 64, 4, 256, 96)[0] == UNSUPPORTED          # K % 64
    assert b"grouped" in lib.msq_last_error()
    assert _plan(lib, 64, 4, 256, 256)[0] == 0
    with pytest.raises(msq._lib.MsqError):
        msq.moe.grouped_plan(64, 4, 256, 256, 7)


def test_grouped_entry_validates_before_any_launch():
    """argument checks of msq_qlinear_grouped_bf16 that need no device: kinds, shapes, null buffers, strides; zero rows is a no-op"""
    lib = _msq()._lib.lib()
    call = lambda **kw: lib.msq_qlinear_grouped_bf16(*[kw.get(k, d) for k, d in (
        ("X", None), ("x_rows", 4), ("row_index", None), ("row_offsets", None), ("inl", None), ("out", None), ("scl", None), ("inl_stride", 0),
        ("out_stride", 0), ("scl_stride", 0), ("bias", None), ("Y", None), ("y_dtype", 2), ("rows", 4), ("E", 4), ("N", 256), ("K", 256),
        ("block", 32), ("in_kind", 0), ("out_kind", U6), ("stream", None))])
    for ik, ok in ((1, 2), (1, 3), (1, 7), (0, 4), (1, U8)):     # MSQ-T1 planes, select bits, bf16 plane, an inlier plane beside a unified kind
        assert call(in_kind=ik, out_kind=ok) == UNSUPPORTED, (ik, ok)
    assert call(N=320) == UNSUPPORTED and call(K=96) == UNSUPPORTED and call(y_dtype=3) == UNSUPPORTED
    assert call(rows=0) == 0                                     # nothing to do: no buffer is looked at
    assert call() == -1                                          # null buffers
    assert b"null buffer" in lib.msq_last_error()


def _tiny(kind):
    if kind == "mixtral":
        from transformers import MixtralConfig, MixtralForCausalLM
        cfg = MixtralConfig(hidden_size=256, intermediate_size=256, num_hidden_layers=1, num_attention_heads=4, num_key_value_heads=2,
                            num_local_experts=4, num_experts_per_tok=2, vocab_size=128, max_position_embeddings=64)
        return MixtralForCausalLM(cfg)
    from transformers import LlamaConfig, LlamaForCausalLM
    cfg = LlamaConfig(hidden_size=256, intermediate_size=256, num_hidden_layers=1, num_attention_heads=4, num_key_value_heads=2,
                      vocab_size=128, max_position_embeddings=64)
    return LlamaForCausalLM(cfg)


def test_find_experts_is_duck_typed():
    _msq()
    from msq.harness.modelutils import find_experts, find_layers
    mix = _tiny("mixtral")
    found = [find_experts(layer) for layer in mix.model.layers]
    assert [len(f) for f in found] == [1]
    (name, mod), = found[0].items()
    assert name.endswith("experts") and tuple(mod.gate_up_proj.shape) == (4, 512, 256) and tuple(mod.down_proj.shape) == (4, 256, 256)
    assert find_experts(mix.model.layers[0], name="model.layers.0") == {"model.layers.0." + name: mod}
    assert len(find_layers(mix.model.layers[0])) == 4            # the attention projections: the experts and the router are no nn.Linear
    assert all(find_experts(layer) == {} for layer in _tiny("llama").model.layers)
