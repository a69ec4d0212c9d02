"""Packed MX KV cache with fused single-token decode attention.

``msq.kvcache.MXKVCache`` fake-quantises K and V in place and keeps them as fp16 / bf16 tensors: the accuracy of an MX cache at the footprint
of an unquantised one.  Here the cache IS the codes: plain OCP-MX (no MicroScopiQ outliers) e4m3 or e2m1 codes + E8M0 scale bytes on the
axes ``mx_quantize_keys`` / ``mx_quantize_values`` use (K: blocks of 32 consecutive tokens of one channel, V: blocks of 32 consecutive
head_dim entries of one token), 8.25 / 4.25 bits per element against 16, and the decode step's attention reads the codes
(csrc/msq_kv_packed.hip).  The bytes are defined by the float32 route of ``_quantize_mx``: a half-precision cache is read as the float32
values it holds and an unpack rounds once to the cache dtype -- not the in-dtype fp16 arithmetic of the "MX" method of msq.kvcache, whose
results are not always code x 2^e (parity table).

  PackedKV            one layer's storage (planes + a tail of tokens that do not fill a group yet), independent of transformers
  PackedMXKVCache     a transformers Cache whose layers wrap PackedKV; update() returns dequantize(), so any attention works
  use_packed_attention registers the attention function "msq_packed_kv" and ties a model's attention modules to the cache's layers

Not built: lengths held on the device / HIP-graph capture of a step, paged or block-table caches, prefill attention over the codes,
MicroScopiQ outlier caches, more than one query token.  Every entry raises MsqError on CPU tensors: there is no CPU fallback."""
import ctypes as C

import torch

from ._lib import MsqError, check, current_stream, lib, ptr

_DT = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
_FMT = {"fp8_e4m3": 5, "fp4_e2m1": 8, "fp4": 8}                  # include/msq.h MSQ_FMT_*
_CODE_BITS = {5: 8, 8: 4}
GROUP = 32                                                       # the MX block: tokens of a K block, channels of a V block
ATTENTION_NAME = "msq_packed_kv"


def _fmt_id(elem_format):
    try:
        return _FMT[str(elem_format).lower()]
    except KeyError:
        raise MsqError("packed KV cache: elem_format must be fp8_e4m3 or fp4_e2m1, not %r" % (elem_format,)) from None


def plane_shapes(B, Hkv, S_cap, D, elem_format):
    """Shapes (uint8) of the four planes of one layer: the table of DESIGN.md 4."""
    fid = _fmt_id(elem_format)
    if S_cap % GROUP or S_cap < 0:
        raise MsqError("packed KV cache: the capacity must be a multiple of 32")
    if D % GROUP or not 0 < D <= 256:
        raise MsqError("packed KV cache: head_dim must be a multiple of 32, at most 256")
    cd = D * _CODE_BITS[fid] // 8
    return {"k_codes": (B, Hkv, S_cap, cd), "k_scales": (B, Hkv, S_cap // GROUP, D),
            "v_codes": (B, Hkv, S_cap, cd), "v_scales": (B, Hkv, S_cap, D // GROUP)}


def plane_nbytes(B, Hkv, S_cap, D, elem_format):
    n = 0
    for shp in plane_shapes(B, Hkv, S_cap, D, elem_format).values():
        n += shp[0] * shp[1] * shp[2] * shp[3]
    return n


def attn_plan(B, Hq, Hkv, D, S_packed, tail_len):
    """(n_splits, split_tokens, workspace_bytes) of the decode kernel: host arithmetic of libmsq_hip.so, no device.  Split s covers the
    packed tokens s * split_tokens .. min((s + 1) * split_tokens, S_packed); the last one also takes the tail."""
    ns, st, wb = C.c_int(-1), C.c_int(-1), C.c_int64(-1)
    check(lib().msq_kv_mx_attn_plan(B, Hq, Hkv, D, S_packed, tail_len, C.byref(ns), C.byref(st), C.byref(wb)), "msq_kv_mx_attn_plan")
    return ns.value, st.value, wb.value


def _need_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise MsqError("the packed KV cache needs CUDA/HIP tensors (no CPU fallback)")


def _status(status, who):
    if status is not None and int(status.item()) & 1:
        raise MsqError(who + ": MSQ_STATUS_NAN (a block holds Inf / NaN)")


def mx_pack(x, codes, scales, pos, elem_format, along_tokens, check_status=False):
    """x [B, H, T, D] (f32 / f16 / bf16) -> tokens pos .. pos + T of a code plane and its scale plane (in place).  T % 32 == 0,
    pos % 32 == 0.  along_tokens: the K form (blocks of 32 tokens of a channel), else the V form (blocks of 32 channels of a token)."""
    _need_cuda(x, codes, scales)
    if x.ndim != 4 or x.dtype not in _DT:
        raise MsqError("mx_pack: expected a [batch, heads, tokens, head_dim] tensor of float32, float16 or bfloat16")
    B, H, T, D = x.shape
    x = x.contiguous()
    if x.data_ptr() % 16:
        x = x.clone()
    status = torch.zeros(1, dtype=torch.int32, device=x.device) if check_status else None
    check(lib().msq_kv_mx_pack(ptr(x), _DT[x.dtype], ptr(codes), ptr(scales), B, H, T, D, codes.shape[2], int(pos), _fmt_id(elem_format),
                               int(bool(along_tokens)), ptr(status), current_stream(x.device)), "msq_kv_mx_pack")
    _status(status, "mx_pack")


def mx_unpack(codes, scales, pos, T, D, dtype, elem_format, along_tokens):
    """tokens pos .. pos + T of a code plane -> [B, H, T, D] in `dtype` (one rounding of code x 2^(scale - 127))."""
    _need_cuda(codes, scales)
    if dtype not in _DT:
        raise MsqError("mx_unpack: dtype must be float32, float16 or bfloat16")
    B, H, S_cap = codes.shape[:3]
    out = torch.empty(B, H, T, D, dtype=dtype, device=codes.device)
    check(lib().msq_kv_mx_unpack(ptr(codes), ptr(scales), ptr(out), _DT[dtype], B, H, D, S_cap, int(pos), int(T), _fmt_id(elem_format),
                                 int(bool(along_tokens)), current_stream(codes.device)), "msq_kv_mx_unpack")
    return out


class PackedKV:
    """One attention layer's K / V as packed planes + a tail.

    Timing rule (the hook of msq.kvcache with streaming=True, stream_grouping=True): after a multi-token append the first
    ``len - len % gap`` tokens are packed and the rest is the tail; on a single-token append, a tail that holds exactly ``gap`` tokens
    is packed first, then the token joins the tail."""

    def __init__(self, B, Hkv, D, dtype, elem_format="fp8_e4m3", gap=32, capacity=256, device="cuda"):
        if gap <= 0 or gap % GROUP:
            raise MsqError("PackedKV: gap must be a positive multiple of 32")
        if dtype not in (torch.float16, torch.bfloat16):
            raise MsqError("PackedKV: the cache dtype must be float16 or bfloat16")
        self.fmt_id = _fmt_id(elem_format)
        plane_shapes(B, Hkv, 0, D, elem_format)                   # head_dim check
        self.B, self.Hkv, self.D, self.dtype, self.elem_format, self.gap = int(B), int(Hkv), int(D), dtype, elem_format, int(gap)
        self.device = torch.device(device)
        self._check_device()
        self.packed_len = self.tail_len = self.capacity = 0
        self.planes = None
        self._ws = None
        self._alloc_tail()
        self._reserve(max(int(capacity), GROUP))

    # ---- storage (overridden by the host test's stub) ------------------------------------------------------------------------------
    def _check_device(self):
        if self.device.type != "cuda":
            raise MsqError("the packed KV cache needs a CUDA/HIP device (no CPU fallback)")

    def _alloc_tail(self):
        self.k_tail = torch.zeros(self.B, self.Hkv, self.gap, self.D, dtype=self.dtype, device=self.device)
        self.v_tail = torch.zeros_like(self.k_tail)

    def _reserve(self, need):
        """capacity >= need, grown in whole groups by reallocate-and-copy"""
        if need <= self.capacity:
            return
        cap = max((need + GROUP - 1) // GROUP * GROUP, 2 * self.capacity)
        new = {n: torch.zeros(s, dtype=torch.uint8, device=self.device)
               for n, s in plane_shapes(self.B, self.Hkv, cap, self.D, self.elem_format).items()}
        if self.planes is not None and self.packed_len:
            P = self.packed_len
            for n in ("k_codes", "v_codes", "v_scales"):
                new[n][:, :, :P] = self.planes[n][:, :, :P]
            new["k_scales"][:, :, :P // GROUP] = self.planes["k_scales"][:, :, :P // GROUP]
        self.planes, self.capacity = new, cap

    def _pack(self, k, v, pos):
        mx_pack(k, self.planes["k_codes"], self.planes["k_scales"], pos, self.elem_format, True)
        mx_pack(v, self.planes["v_codes"], self.planes["v_scales"], pos, self.elem_format, False)

    def _tail_put(self, k, v, at):
        n = k.shape[2]
        self.k_tail[:, :, at:at + n] = k
        self.v_tail[:, :, at:at + n] = v

    def _tail_get(self):
        return self.k_tail[:, :, :self.tail_len], self.v_tail[:, :, :self.tail_len]

    # ---- the cache ------------------------------------------------------------------------------------------------------------------
    @property
    def len(self):
        return self.packed_len + self.tail_len

    def __len__(self):
        return self.len

    def _check_kv(self, k, v):
        _need_cuda(k, v)
        want = (self.B, self.Hkv, self.D)
        if k.ndim != 4 or v.shape != k.shape or (k.shape[0], k.shape[1], k.shape[3]) != want or k.dtype != self.dtype or v.dtype != self.dtype:
            raise MsqError("PackedKV.append: expected k, v [%d, %d, T, %d] of %s" % (self.B, self.Hkv, self.D, self.dtype))

    def append(self, k, v):
        self._check_kv(k, v)
        T = k.shape[2]
        if T == 0:
            return
        if T == 1:
            if self.tail_len == self.gap:                        # the last `gap` tokens are complete: pack them, then take the token
                tk, tv = self._tail_get()
                self._reserve(self.packed_len + self.gap)
                self._pack(tk, tv, self.packed_len)
                self.packed_len += self.gap
                self.tail_len = 0
            self._tail_put(k, v, self.tail_len)
            self.tail_len += 1
            return
        if self.tail_len:
            tk, tv = self._tail_get()
            k, v = torch.cat([tk, k], dim=2), torch.cat([tv, v], dim=2)
        total = self.packed_len + k.shape[2]
        npk = total - total % self.gap - self.packed_len         # packed_len is a multiple of gap, so this is one too
        if npk > 0:
            self._reserve(self.packed_len + npk)
            self._pack(k[:, :, :npk], v[:, :, :npk], self.packed_len)
            self.packed_len += npk
        self.tail_len = 0
        rest = k.shape[2] - max(npk, 0)
        if rest:
            self._tail_put(k[:, :, max(npk, 0):], v[:, :, max(npk, 0):], 0)
            self.tail_len = rest

    def dequantize(self):
        """K and V as [B, Hkv, len, D] in the cache dtype: the unpacked part followed by the tail."""
        P = self.packed_len
        tk, tv = self._tail_get()
        if P == 0:
            return tk.clone(), tv.clone()
        k = mx_unpack(self.planes["k_codes"], self.planes["k_scales"], 0, P, self.D, self.dtype, self.elem_format, True)
        v = mx_unpack(self.planes["v_codes"], self.planes["v_scales"], 0, P, self.D, self.dtype, self.elem_format, False)
        if self.tail_len:
            k, v = torch.cat([k, tk], dim=2), torch.cat([v, tv], dim=2)
        return k, v

    def attend(self, q, bias=None, scaling=None, out_dtype=None):
        """softmax(scaling q K^T + bias) V for one query token per sequence, over the codes and the tail (the fused kernel).
        q [B, Hq, D] (or [B, Hq, 1, D]) in the cache dtype; bias [B, len] float32 (may hold -inf) or None; returns [B, Hq, D] in
        out_dtype (the q dtype or float32)."""
        _need_cuda(q, bias)
        if q.ndim == 4 and q.shape[2] == 1:
            q = q[:, :, 0, :]
        if q.ndim != 3 or q.shape[0] != self.B or q.shape[2] != self.D or q.dtype != self.dtype:
            raise MsqError("PackedKV.attend: expected q [%d, Hq, %d] of %s" % (self.B, self.D, self.dtype))
        Hq = q.shape[1]
        out_dtype = q.dtype if out_dtype is None else out_dtype
        if out_dtype not in (q.dtype, torch.float32):
            raise MsqError("PackedKV.attend: out_dtype must be the q dtype or float32")
        q = q.contiguous()
        if q.data_ptr() % 16:
            q = q.clone()
        if bias is not None:
            if tuple(bias.shape) != (self.B, self.len):
                raise MsqError("PackedKV.attend: bias must be [%d, %d]" % (self.B, self.len))
            bias = bias.to(torch.float32).contiguous()
        scaling = float(self.D) ** -0.5 if scaling is None else float(scaling)
        need = lib().msq_kv_mx_attn_workspace_bytes(self.B, Hq, self.Hkv, self.D, self.packed_len, self.tail_len)
        if need < 0:
            check(int(need), "msq_kv_mx_attn_workspace_bytes")
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(int(need), dtype=torch.uint8, device=self.device)
        out = torch.empty(self.B, Hq, self.D, dtype=out_dtype, device=self.device)
        p = self.planes
        check(lib().msq_kv_mx_attn_decode(ptr(q), _DT[q.dtype], ptr(p["k_codes"]), ptr(p["k_scales"]), ptr(p["v_codes"]), ptr(p["v_scales"]),
                                          self.packed_len, self.capacity, ptr(self.k_tail), ptr(self.v_tail), self.tail_len, self.gap,
                                          ptr(bias), ptr(out), _DT[out_dtype], self.B, Hq, self.Hkv, self.D, self.fmt_id, scaling,
                                          ptr(self._ws), self._ws.numel(), current_stream(self.device)), "msq_kv_mx_attn_decode")
        return out

    @property
    def bits_per_element(self):
        """of the packed part: code bits + one scale byte per 32 elements"""
        return _CODE_BITS[self.fmt_id] + 8.0 / GROUP

    @property
    def nbytes(self):
        """device bytes held: the four planes at the current capacity + the tail buffers"""
        esz = 2
        return plane_nbytes(self.B, self.Hkv, self.capacity, self.D, self.elem_format) + 2 * self.B * self.Hkv * self.gap * self.D * esz


def _make_layer_class():
    from transformers.cache_utils import CacheLayerMixin

    class PackedKVLayer(CacheLayerMixin):
        """One attention layer of PackedMXKVCache.  ``fused`` (set by use_packed_attention): a single-token update hands back the new
        token's K / V only -- the tied attention function reads the codes and never looks at them -- instead of dequantize()."""
        is_sliding = False
        is_compileable = False

        def __init__(self, elem_format="fp8_e4m3", gap=32, capacity=256):
            super().__init__()
            self.elem_format, self.gap, self.capacity = elem_format, gap, capacity
            self.packed = None
            self.fused = False

        def lazy_initialization(self, key_states, value_states=None):
            _need_cuda(key_states)
            B, H, _, D = key_states.shape
            self.dtype, self.device = key_states.dtype, key_states.device
            self.packed = PackedKV(B, H, D, key_states.dtype, self.elem_format, self.gap, self.capacity, key_states.device)
            self.keys = self.values = None
            self.is_initialized = True

        def update(self, key_states, value_states, *args, **kwargs):
            if not self.is_initialized:
                self.lazy_initialization(key_states, value_states)
            self.packed.append(key_states, value_states)
            if self.fused and key_states.shape[2] == 1:
                return key_states, value_states
            return self.packed.dequantize()

        def get_seq_length(self):
            return self.packed.len if self.packed is not None else 0

        def get_mask_sizes(self, query_length):
            return self.get_seq_length() + query_length, 0

        def get_max_cache_shape(self):
            return -1

        def get_max_length(self):
            return -1

        def reset(self):
            if self.packed is not None:
                self.packed.packed_len = self.packed.tail_len = 0

    return PackedKVLayer


def PackedMXKVCache(num_layers, elem_format="fp8_e4m3", gap=32, capacity=256):
    """A transformers Cache (``past_key_values=PackedMXKVCache(n)``) whose layers hold packed MX planes."""
    from transformers.cache_utils import Cache
    layer_cls = _make_layer_class()
    _fmt_id(elem_format)
    if gap <= 0 or gap % GROUP:
        raise MsqError("PackedMXKVCache: gap must be a positive multiple of 32")
    return Cache(layers=[layer_cls(elem_format, gap, capacity) for _ in range(num_layers)])


def _packed_attention_forward(module, query, key, value, attention_mask, dropout=0.0, scaling=None, **kwargs):
    from transformers.integrations.sdpa_attention import sdpa_attention_forward
    layer = getattr(module, "_msq_packed_layer", None)
    if layer is None or layer.packed is None or query.shape[2] != 1:
        return sdpa_attention_forward(module, query, key, value, attention_mask, dropout=dropout, scaling=scaling, **kwargs)
    bias = None
    if attention_mask is not None:
        if attention_mask.ndim != 4 or attention_mask.shape[1] != 1 or attention_mask.shape[2] != 1:
            raise MsqError("msq_packed_kv: expected a [B, 1, 1, S] attention mask at query length 1")
        am = attention_mask[:, 0, 0, :]
        if am.dtype == torch.bool:                               # the sdpa mask convention: True = attend
            bias = torch.zeros(am.shape, dtype=torch.float32, device=am.device).masked_fill_(~am, float("-inf"))
        else:
            bias = am.to(torch.float32)
        if bias.shape[0] != query.shape[0]:
            bias = bias.expand(query.shape[0], -1)
    out = layer.packed.attend(query[:, :, 0, :], bias, scaling)
    return out.unsqueeze(1), None                                # [B, 1, Hq, D], the layout the attention interface returns


def use_packed_attention(model, cache):
    """Decode steps of `model` attend over the codes of `cache` (a PackedMXKVCache): registers the attention function "msq_packed_kv",
    ties every attention module to its cache layer (the registered function is not handed past_key_values: the module attribute is the
    link) and selects the function in the model's config.  Query lengths above 1 go to sdpa on the dequantised tensors."""
    from transformers import AttentionInterface
    from transformers.masking_utils import AttentionMaskInterface, sdpa_mask
    AttentionInterface.register(ATTENTION_NAME, _packed_attention_forward)
    AttentionMaskInterface.register(ATTENTION_NAME, sdpa_mask)
    tied = 0
    for m in model.modules():
        idx = getattr(m, "layer_idx", None)
        if idx is None or not hasattr(m, "q_proj") or not hasattr(m, "k_proj"):
            continue
        if idx >= len(cache.layers) or not hasattr(cache.layers[idx], "packed"):
            raise MsqError("use_packed_attention: the cache has no packed layer %d" % idx)
        m._msq_packed_layer = cache.layers[idx]
        cache.layers[idx].fused = True
        tied += 1
    if not tied:
        raise MsqError("use_packed_attention: no attention module (layer_idx + q_proj / k_proj) found in the model")
    model.config._attn_implementation = ATTENTION_NAME
    return model
