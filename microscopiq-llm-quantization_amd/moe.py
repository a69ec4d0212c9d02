"""Packed mixture of experts: the expert weights of a Mixtral-style block (the `w1` / `w3` / `w2` Linears the reference's harness
quantises one by one, llm/llama.py:37-40 with ``model_type="mixtral"``) as stacked packed planes, multiplied by ONE grouped fused
dequant-GEMM launch per projection (csrc/msq_gemm_grouped.hip: k_qgemm_grouped).

    route            top-k expert indices -> rows sorted by expert (torch ops only, no host sync: capturable in a HIP graph)
    PackedExperts    stacked planes [E, bytes] of E weights of one shape and one plane kind; ``expert(e)`` is a PackedWeight view
    grouped_qlinear  Y[r] = X[row_index[r]] . W_e(r)^T for rows sorted by expert
    QuantExperts     drop-in for a module with 3-D ``gate_up_proj`` / ``down_proj`` parameters and an ``act_fn``

The per-expert row counts never reach the host: the launch geometry comes from the row capacity (tokens * top_k) and E alone, so a
decode step through a router can be captured and replayed with another routing.  Nothing here falls back to a dense path."""
import ctypes as C

import torch
import torch.nn as nn

from ._lib import MsqError, check, current_stream, lib, ptr
from .qlinear import (_YD, K_MULT, N_MULT, PLANE_NONE, PLANE_U8, PLANE_U8X, PackedWeight, _cast_f16_bf16, _ceil_to, _pad2d, _pad_k,
                      pack_weight, packed_sizes, unpack_weight)


def route(top_k_index, num_experts):
    """[T, k] expert indices -> (row_index int32 [T*k], row_offsets int32 [E+1], inverse int64 [T*k]).

    Sorted row r holds token ``row_index[r]``; expert e owns the rows ``row_offsets[e] .. row_offsets[e+1]``; inside an expert the rows
    ascend by (token, k-slot) (stable sort of the flat [T, k] positions); ``inverse[t * k + j]`` is the sorted row of slot j of token t.
    An index outside 0 .. E-1 sorts behind ``row_offsets[E]``: the grouped GEMM does not compute it.  No ``.item()``, no ``nonzero``."""
    if top_k_index.ndim != 2:
        raise MsqError("route: top_k_index must be [tokens, top_k]")
    k = top_k_index.shape[1]
    flat = top_k_index.reshape(-1).to(torch.int64)
    flat = torch.where((flat < 0) | (flat >= num_experts), torch.full_like(flat, num_experts), flat)
    vals, order = torch.sort(flat, stable=True)
    row_index = torch.div(order, k, rounding_mode="floor").to(torch.int32)
    # first sorted row whose expert is >= e, e = 0 .. E: the cumulative bincount without bincount's host sync
    edges = torch.arange(num_experts + 1, device=flat.device, dtype=torch.int64)
    row_offsets = torch.searchsorted(vals, edges).to(torch.int32)
    inverse = torch.empty_like(order)
    inverse.scatter_(0, order, torch.arange(order.numel(), device=order.device, dtype=torch.int64))
    return row_index, row_offsets, inverse


class PackedExperts:
    """Stacked packed planes of E weights [n, k] of one plane kind: ``inl`` / ``out`` / ``scl`` are uint8 [E, bytes] (or None), row e
    being exactly the planes pack_values / pack_weight build for expert e alone.  ``N`` / ``K`` are the padded dimensions."""

    def __init__(self, inl, out, scl, E, N, K, block, in_kind, out_kind, n=None, k=None):
        self.inl, self.out, self.scl = inl, out, scl
        self.E, self.N, self.K, self.block, self.in_kind, self.out_kind = int(E), N, K, block, in_kind, out_kind
        self.n, self.k = (N if n is None else int(n)), (K if k is None else int(k))

    @property
    def nbytes(self):
        return sum(int(t.numel()) for t in (self.inl, self.out, self.scl) if t is not None)

    @property
    def bits_per_element(self):
        return 8.0 * self.nbytes / (self.E * self.n * self.k)

    def expert(self, e):
        """PackedWeight VIEW of expert e (no copy): qlinear.qlinear and unpack_weight take it."""
        if not 0 <= e < self.E:
            raise MsqError("PackedExperts.expert: %d is outside 0 .. %d" % (e, self.E - 1))
        pick = lambda t: None if t is None else t[e]
        return PackedWeight(pick(self.inl), pick(self.out), pick(self.scl), self.N, self.K, self.block, self.in_kind, self.out_kind, self.n, self.k)


def _empty_planes(E, N, K, block, in_kind, out_kind, dev):
    ib, ob, sb, _ = packed_sizes(N, K, block, in_kind, out_kind)
    mk = lambda b: torch.empty(E, b, dtype=torch.uint8, device=dev) if b else None
    return mk(ib), mk(ob), mk(sb)


def pack_expert_values(Wq, kinds=(PLANE_U8, PLANE_U8X)):
    """Pack a stack [E, n, k] that already holds fake-quant values into the first single-plane kind of `kinds` that holds EVERY expert
    exactly (one kind per stack, one stride).  Nothing is rounded; padding as pack_values (256 x 64 grid)."""
    if not Wq.is_cuda:
        raise MsqError("pack_expert_values needs a CUDA/HIP tensor (no CPU fallback)")
    if Wq.ndim != 3:
        raise MsqError("pack_expert_values expects a 3-D [experts, out_features, in_features] tensor")
    E, n, k = Wq.shape
    N, K = _ceil_to(n, N_MULT), _ceil_to(k, K_MULT)
    dev = Wq.device
    status = torch.zeros(E, dtype=torch.int32, device=dev)
    for ok in kinds:
        inl, out, scl = _empty_planes(E, N, K, 32, PLANE_NONE, ok, dev)
        status.zero_()
        for e in range(E):
            Wf = _pad2d(Wq[e].detach().contiguous().float(), N_MULT, K_MULT)
            check(lib().msq_pack_values(ptr(Wf), ptr(None if inl is None else inl[e]), ptr(out[e]), ptr(None if scl is None else scl[e]),
                                        ptr(status[e:e + 1]), N, K, PLANE_NONE, ok, current_stream(dev)), "msq_pack_values")
        st = status.tolist()
        if any(s & 1 for s in st):
            raise AssertionError("pack_values: the tensor contains NaN / Inf")
        if not any(st):
            return PackedExperts(inl, out, scl, E, N, K, 32, PLANE_NONE, ok, n, k)
    raise MsqError("pack_expert_values: no plane kind of %r holds every expert exactly" % (tuple(kinds),))


def pack_experts(W, layout="unified", **quantizer_kwargs):
    """Quantise (blocks along in_features) and pack every expert of W [E, n, k] as qlinear.pack_weight does for one weight; the experts
    must end in ONE plane kind (a stack has one stride): MsqError otherwise."""
    if W.ndim != 3:
        raise MsqError("pack_experts expects a 3-D [experts, out_features, in_features] tensor")
    Ps = [pack_weight(W[e], layout=layout, **quantizer_kwargs) for e in range(W.shape[0])]
    P0 = Ps[0]
    if any((P.in_kind, P.out_kind, P.block) != (P0.in_kind, P0.out_kind, P0.block) for P in Ps):
        raise MsqError("pack_experts: the experts do not share one plane kind under layout %r; name a layout every expert fits" % (layout,))
    stack = lambda ts: None if ts[0] is None else torch.stack(ts)
    return PackedExperts(stack([P.inl for P in Ps]), stack([P.out for P in Ps]), stack([P.scl for P in Ps]), len(Ps), P0.N, P0.K, P0.block,
                         P0.in_kind, P0.out_kind, P0.n, P0.k)


def unpack_experts(PE, dtype=torch.float32):
    """Dense dequantised stack [E, n, k] (exact in f32 and bf16)."""
    return torch.stack([unpack_weight(PE.expert(e), dtype) for e in range(PE.E)])


def grouped_plan(rows, E, N, K, out_kind):
    """(row_tile, tile_slots, blocks) of the grouped kernel for a row capacity: host arithmetic only."""
    rt, ts, nb = C.c_int(), C.c_int(), C.c_int64()
    check(lib().msq_qlinear_grouped_plan(rows, E, N, K, out_kind, C.byref(rt), C.byref(ts), C.byref(nb)), "msq_qlinear_grouped_plan")
    return rt.value, ts.value, nb.value


def grouped_qlinear(x, PE, row_offsets, row_index=None, bias=None, out_dtype=torch.bfloat16, out=None, rows=None):
    """y[r] = x[row_index[r]] . W_e(r)^T (+ bias[e(r)]) for rows sorted by expert: expert e owns rows row_offsets[e] .. row_offsets[e+1].

    x [x_rows, k] (cast to bf16); row_offsets int32 [E + 1] and row_index int32 [rows] (None: row r reads x[r]) on x's device; ``rows`` is
    the CAPACITY of the result (default: len(row_index), or x_rows) -- rows at and beyond row_offsets[E] are left as they are."""
    if not x.is_cuda:
        raise MsqError("grouped_qlinear needs CUDA/HIP tensors (no CPU fallback)")
    if x.ndim != 2 or x.shape[1] != PE.k:
        raise MsqError("grouped_qlinear: x must be [rows, %d]" % PE.k)
    dev = x.device
    if row_offsets.device != dev or row_offsets.dtype != torch.int32 or row_offsets.numel() != PE.E + 1 or not row_offsets.is_contiguous():
        raise MsqError("grouped_qlinear: row_offsets must be a contiguous int32 [%d] tensor on %s" % (PE.E + 1, dev))
    if row_index is not None and (row_index.device != dev or row_index.dtype != torch.int32 or row_index.ndim != 1 or not row_index.is_contiguous()):
        raise MsqError("grouped_qlinear: row_index must be a contiguous 1-D int32 tensor on %s" % (dev,))
    cap = int(row_index.numel()) if row_index is not None else int(x.shape[0])
    rows = cap if rows is None else int(rows)
    if rows < 0 or rows > cap:
        raise MsqError("grouped_qlinear: rows = %d exceeds the %d rows that %s provides" % (rows, cap, "row_index" if row_index is not None else "x"))
    if out_dtype not in _YD:
        raise MsqError("grouped_qlinear: out_dtype must be float32, float16 or bfloat16")
    for t in (PE.inl, PE.out, PE.scl):
        if t is not None and (t.device != dev or not t.is_contiguous()):
            raise MsqError("grouped_qlinear: the packed planes must be contiguous and on %s" % (dev,))
    if x.dtype == torch.float16:
        xb = _cast_f16_bf16(x)
    else:
        xb = x if x.dtype == torch.bfloat16 else x.to(torch.bfloat16)
    xb = _pad_k(xb, PE.K).contiguous()
    padded_n = PE.n != PE.N
    want = (rows, PE.n)
    if out is not None and (tuple(out.shape) != want or out.dtype != out_dtype or not out.is_contiguous() or out.device != dev):
        raise MsqError("grouped_qlinear: out must be a contiguous [%d, %d] %s tensor on %s" % (rows, PE.n, out_dtype, dev))
    if padded_n:
        y = torch.empty(rows, PE.N, dtype=out_dtype, device=dev) if out is None else torch.nn.functional.pad(out, (0, PE.N - PE.n))
    else:
        y = torch.empty(rows, PE.N, dtype=out_dtype, device=dev) if out is None else out
    b = None
    if bias is not None:
        if tuple(bias.shape) != (PE.E, PE.n) or bias.device != dev:
            raise MsqError("grouped_qlinear: bias must be [%d, %d] on %s" % (PE.E, PE.n, dev))
        b = bias.detach().float()
        b = (torch.nn.functional.pad(b, (0, PE.N - PE.n)) if padded_n else b).contiguous()
    stride = lambda t: 0 if t is None else int(t.stride(0))
    check(lib().msq_qlinear_grouped_bf16(ptr(xb), xb.shape[0], ptr(row_index), ptr(row_offsets), ptr(PE.inl), ptr(PE.out), ptr(PE.scl),
                                         stride(PE.inl), stride(PE.out), stride(PE.scl), ptr(b), ptr(y), _YD[out_dtype], rows, PE.E,
                                         PE.N, PE.K, PE.block, PE.in_kind, PE.out_kind, current_stream(dev)), "msq_qlinear_grouped_bf16")
    if padded_n:
        if out is not None:
            out.copy_(y[:, :PE.n]); y = out
        else:
            y = y[:, :PE.n].contiguous()
    return y


def is_expert_module(m):
    """duck type of a stacked-experts module: 3-D ``gate_up_proj`` [E, 2I, H] and ``down_proj`` [E, H, I] parameters"""
    gu, dn = getattr(m, "gate_up_proj", None), getattr(m, "down_proj", None)
    return isinstance(gu, nn.Parameter) and isinstance(dn, nn.Parameter) and gu.ndim == 3 and dn.ndim == 3


class QuantExperts(nn.Module):
    """Packed stand-in for a stacked-experts module (transformers' ``MixtralExperts``): the two weight stacks live as packed planes
    (registered buffers: state_dict round-trips them), the forward runs two grouped fused dequant-GEMMs around ``act_fn(gate) * up``.
    Deterministic (no index_add_, no atomics), no host sync."""

    _PLANES = ("inl", "out", "scl")

    def __init__(self, num_experts, hidden_dim, intermediate_dim, act_fn, gate_up_kind=PLANE_U8, down_kind=None, device=None):
        super().__init__()
        self.num_experts, self.hidden_dim, self.intermediate_dim, self.act_fn = int(num_experts), int(hidden_dim), int(intermediate_dim), act_fn
        self.gate_up_kind, self.down_kind = int(gate_up_kind), int(gate_up_kind if down_kind is None else down_kind)
        for stack, (n, k), kind in (("gate_up", (2 * self.intermediate_dim, self.hidden_dim), self.gate_up_kind),
                                    ("down", (self.hidden_dim, self.intermediate_dim), self.down_kind)):
            sizes = packed_sizes(_ceil_to(n, N_MULT), _ceil_to(k, K_MULT), 32, PLANE_NONE, kind)[:3]
            for nm, b in zip(self._PLANES, sizes):
                self.register_buffer("%s_%s" % (stack, nm), torch.zeros(self.num_experts, b, dtype=torch.uint8, device=device))

    @property
    def out_kind(self):
        """plane kind of the stacks (a pair when gate_up and down differ)"""
        return self.gate_up_kind if self.gate_up_kind == self.down_kind else (self.gate_up_kind, self.down_kind)

    @classmethod
    def from_module(cls, experts, kinds=None):
        """Pack the (already fake-quantised) values of a module with 3-D ``gate_up_proj`` / ``down_proj`` parameters and an ``act_fn``;
        ``kinds``: the plane kinds pack_expert_values tries per stack, in order (None = its default)."""
        if not is_expert_module(experts) or not hasattr(experts, "act_fn"):
            raise MsqError("QuantExperts.from_module: the module needs 3-D gate_up_proj / down_proj parameters and an act_fn")
        gu, dn = experts.gate_up_proj.data, experts.down_proj.data
        E, I2, H = gu.shape
        if I2 % 2 or tuple(dn.shape) != (E, H, I2 // 2):
            raise MsqError("QuantExperts.from_module: gate_up_proj [E, 2I, H] and down_proj [E, H, I] do not match")
        kw = {} if kinds is None else {"kinds": tuple(kinds)}
        Pg, Pd = pack_expert_values(gu, **kw), pack_expert_values(dn, **kw)
        m = cls(E, H, I2 // 2, experts.act_fn, Pg.out_kind, Pd.out_kind, device=gu.device)
        for stack, P in (("gate_up", Pg), ("down", Pd)):
            for nm in cls._PLANES:
                t = getattr(P, nm)
                if t is not None:
                    setattr(m, "%s_%s" % (stack, nm), t)      # adopts the planes (a registered buffer is replaced, not copied)
        return m

    def _packed(self, stack):
        n, k, kind = ((2 * self.intermediate_dim, self.hidden_dim, self.gate_up_kind) if stack == "gate_up"
                      else (self.hidden_dim, self.intermediate_dim, self.down_kind))
        pl = [getattr(self, "%s_%s" % (stack, nm)) for nm in self._PLANES]
        pl = [t if t.shape[1] else None for t in pl]
        return PackedExperts(pl[0], pl[1], pl[2], self.num_experts, _ceil_to(n, N_MULT), _ceil_to(k, K_MULT), 32, PLANE_NONE, kind, n, k)

    def packed(self):
        """(gate_up, down) as PackedExperts views of the module's buffers"""
        return self._packed("gate_up"), self._packed("down")

    @property
    def nbytes(self):
        return sum(P.nbytes for P in self.packed())

    def dequantize(self, dtype=torch.float32):
        """the two dense stacks (gate_up [E, 2I, H], down [E, H, I])"""
        Pg, Pd = self.packed()
        return unpack_experts(Pg, dtype), unpack_experts(Pd, dtype)

    def forward(self, hidden_states, top_k_index, top_k_weights):
        T, k = top_k_index.shape
        I, H = self.intermediate_dim, self.hidden_dim
        dt = hidden_states.dtype if hidden_states.dtype in _YD else torch.bfloat16
        Pg, Pd = self.packed()
        row_index, row_offsets, inverse = route(top_k_index, self.num_experts)
        gu = grouped_qlinear(hidden_states.reshape(-1, H), Pg, row_offsets, row_index, out_dtype=dt)          # [T k, 2 I]: the gather is fused in
        h = self.act_fn(gu[:, :I]) * gu[:, I:]
        y = torch.zeros(T * k, H, dtype=dt, device=h.device)          # rows of an index outside 0 .. E-1 are not computed: they contribute zero
        grouped_qlinear(h, Pd, row_offsets, out_dtype=dt, out=y)
        y = y.index_select(0, inverse).view(T, k, H)
        w = top_k_weights.to(torch.promote_types(dt, top_k_weights.dtype))
        acc = y[:, 0] * w[:, 0, None]
        for j in range(1, k):                                             # summed in slot order: the same bits every run
            acc = acc + y[:, j] * w[:, j, None]
        return acc.to(hidden_states.dtype)


def pack_expert_modules(layers, kinds=None):
    """Swap every stacked-experts module on the GPU below `layers` (a module or an iterable of modules) for
    ``QuantExperts.from_module(..., kinds=kinds)``; returns the number of modules swapped."""
    roots = [layers] if isinstance(layers, nn.Module) else list(layers)
    count = 0
    for root in roots:
        for name, m in list(root.named_modules()):
            if not name or isinstance(m, QuantExperts) or not is_expert_module(m) or not m.gate_up_proj.is_cuda:
                continue
            parent = root
            parts = name.split(".")
            for p_ in parts[:-1]:
                parent = getattr(parent, p_)
            setattr(parent, parts[-1], QuantExperts.from_module(m, kinds=kinds))
            count += 1
    return count
