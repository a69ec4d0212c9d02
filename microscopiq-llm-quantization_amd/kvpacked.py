"""Packed MX KV cache with fused single-token decode attention.

``msq.kvcache.MXKVCache`` fake-quantises K and V in place and keeps them as fp16 / bf16 tensors: the accuracy of an MX cache at the footprint
of an unquantised one.  Here the cache IS the codes: plain OCP-MX (no MicroScopiQ outliers) e4m3 or e2m1 codes + E8M0 scale bytes on the
axes ``mx_quantize_keys`` / ``mx_quantize_values`` use (K: blocks of 32 consecutive tokens of one channel, V: blocks of 32 consecutive
head_dim entries of one token), 8.25 / 4.25 bits per element against 16, and the decode step's attention reads the codes
(csrc/msq_kv_packed.hip).  The bytes are defined by the float32 route of ``_quantize_mx``: a half-precision cache is read as the float32
values it holds and an unpack rounds once to the cache dtype -- not the in-dtype fp16 arithmetic of the "MX" method of msq.kvcache, whose
results are not always code x 2^e (parity table).

  PackedKV            one layer's storage (planes + a tail of tokens that do not fill a group yet), independent of transformers
  StaticPackedKV      the same with a fixed capacity and the lengths in device memory: a decode step -- append(k, v), then
                      attend_dev(q) -- launches the same kernels with the same arguments at every length, so it can be captured in a HIP
                      graph and replayed; the host keeps a mirror of the lengths that every Python call advances without a device read
  SlotPackedKV        StaticPackedKV with a state row PER SEQUENCE: B slots with lengths of their own, so a ragged batch needs
                      no left padding, and a slot can be reset and prefilled again between replays of ONE captured step while the others go on
  PackedMXKVCache     a transformers Cache whose layers wrap PackedKV; update() returns dequantize(), so any attention works
  use_packed_attention registers the attention function "msq_packed_kv" and ties a model's attention modules to the cache's layers

Query lengths 2 .. 32: ``PackedKV.attend_multi`` is causal attention of the LAST T tokens the cache holds over the codes on
the matrix cores (csrc/msq_kv_packed_multi.hip) -- a few draft tokens to verify, a short chunk of new tokens -- and ``PackedKV.crop`` takes
rejected tokens back.  ``use_packed_attention(model, cache, max_query_tokens=T)`` routes those lengths to it.

Not built: paged or block-table caches (SlotPackedKV keeps planes [B, Hkv, S_cap, ..]: a slot reserves max_len tokens; per-sequence lengths
are the prerequisite for paging, not paging), a transformers Cache over SlotPackedKV (transformers batches by left padding on one shared
length), prefill attention over the codes (more than 32 query tokens go to sdpa on the dequantised tensors),
MicroScopiQ outlier caches, a device-length or per-sequence form of attend_multi and a device-side multi-token append (both run on the host
mirror's lengths and cannot be captured), capture of a whole transformers model (its mask and position plumbing is not ours: PackedMXKVCache(max_len=...)
runs eagerly).  Every entry raises MsqError on CPU tensors: there is no CPU fallback.

Head dims: mx_pack / mx_unpack and PackedKV's append / dequantize / crop take every head_dim that is a multiple of 32 up to 256 (pack / unpack
are pinned to the oracle at 32, 64, 96, 128, 160 and 256, the cache at 64, 96 and 256); the attention kernels exist for 64 and 128, and attend /
attend_dev / attend_multi raise MsqError (head_dim must be 64 or 128) before any launch elsewhere.

GPU tests (tests/test_gpu_f3_kv_packed*.py; DESIGN.md 5.013 maps kernel instantiations to tests):
  test_gpu_f3_kv_packed.py           pack / unpack against the oracle, attend against float64 (gap 32, 2 or 8 query heads per kv head), a model
  test_gpu_f3_kv_packed_static.py    attend_dev and the captured step, bit-equal to the host-length path; overflow, status
  test_gpu_f3_kv_packed_multi.py     attend_multi against float64, row independence, crop, a model fed in chunks
  test_gpu_f3_kv_packed_slots.py     ragged slots, slot reuse, idle slots, bit-equal to every slot's own cache
  test_gpu_f3_kv_packed_coverage.py  1, 3, 4, 5, 6 and 7 query heads per kv head (1 and 3 kv heads), gap 64 / 96 (tail chunks after the first,
                                     a full tail, the device flush of two K groups), an ALiBi bias with scaling != head_dim^-0.5, scale
                                     bytes that differ between neighbours, blocks at the ends of the fp16 / bf16 range, head_dim 96 / 256,
                                     the row-tile boundaries of attend_multi and T == len"""
import ctypes as C

import torch

from ._lib import MsqError, check, current_stream, lib, ptr

_DT = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
_FMT = {"fp8_e4m3": 5, "fp4_e2m1": 8, "fp4": 8}                  # include/msq.h MSQ_FMT_*
_CODE_BITS = {5: 8, 8: 4}
GROUP = 32                                                       # the MX block: tokens of a K block, channels of a V block
MAX_QUERY_TOKENS = 32                                            # of attend_multi (msq_kv_mx_attn_multi)
ATTENTION_NAME = "msq_packed_kv"
STATUS_NAN, STATUS_OVERFLOW = 1, 8                               # include/msq.h MSQ_STATUS_*
SLOT_IDLE = 1                                                    # include/msq.h MSQ_KV_SLOT_IDLE: bit 0 of a state row's flags word


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


def _check_gap(who, gap):
    if gap <= 0 or gap % GROUP:
        raise MsqError(who + ": gap must be a positive multiple of 32")


def _status_names(status):
    """the bits of a state's status word by name"""
    names = [n for bit, n in ((STATUS_OVERFLOW, "MSQ_STATUS_OVERFLOW"), (STATUS_NAN, "MSQ_STATUS_NAN")) if status & bit]
    if status & ~(STATUS_OVERFLOW | STATUS_NAN):
        names.append("status %d" % status)
    return names


def _step_lengths(p, t, n, S_cap, gap):
    """(packed_len, tail_len, taken) after n single-token appends to a cache at (p, t): the rule of PackedKV.append in closed form.  A cache
    holds S_cap packed tokens + a full tail and stays there: taken < n tells that it filled up."""
    taken = max(0, min(n, S_cap + gap - (p + t)))
    if taken > 0:
        flushes = (t + taken - 1) // gap
        p, t = p + flushes * gap, t + taken - flushes * gap
    return p, t, taken


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
        _check_gap("PackedKV", gap)
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
        self._ws_multi = None                                    # attend_multi's workspace
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

    def _unpack(self, pos, T):
        """K and V of the packed tokens pos .. pos + T in the cache dtype"""
        k = mx_unpack(self.planes["k_codes"], self.planes["k_scales"], pos, T, self.D, self.dtype, self.elem_format, True)
        v = mx_unpack(self.planes["v_codes"], self.planes["v_scales"], pos, T, self.D, self.dtype, self.elem_format, False)
        return k, v

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
        tk, tv = self._tail_get()
        if self.packed_len == 0:
            return tk.clone(), tv.clone()
        k, v = self._unpack(0, self.packed_len)
        if self.tail_len:
            k, v = torch.cat([k, tk], dim=2), torch.cat([v, tv], dim=2)
        return k, v

    def _prep_q(self, who, q, ndim, out_dtype, scaling):
        """what the attention entries do with q before anything else: q [B, Hq, D] (ndim 3; [B, Hq, 1, D] is taken too) or [B, Hq, T, D]
        (ndim 4) in the cache dtype -> (q contiguous and 16-byte aligned, out_dtype, scaling) with their defaults filled in"""
        if ndim == 3 and q.ndim == 4 and q.shape[2] == 1:
            q = q[:, :, 0, :]
        if q.ndim != ndim or q.shape[0] != self.B or q.shape[-1] != self.D or q.dtype != self.dtype:
            raise MsqError("%s: expected q [%d, Hq, %s%d] of %s" % (who, self.B, "T, " if ndim == 4 else "", self.D, self.dtype))
        out_dtype = q.dtype if out_dtype is None else out_dtype
        if out_dtype not in (q.dtype, torch.float32):
            raise MsqError(who + ": out_dtype must be the q dtype or float32")
        q = q.contiguous()
        if q.data_ptr() % 16:
            q = q.clone()
        return q, out_dtype, float(self.D) ** -0.5 if scaling is None else float(scaling)

    def attend(self, q, bias=None, scaling=None, out_dtype=None):
        """softmax(scaling q K^T + bias) V for one query token per sequence, over the codes and the tail (the fused kernel).
        q [B, Hq, D] (or [B, Hq, 1, D]) in the cache dtype; bias [B, len] float32 (may hold -inf) or None; returns [B, Hq, D] in
        out_dtype (the q dtype or float32)."""
        _need_cuda(q, bias)
        q, out_dtype, scaling = self._prep_q("PackedKV.attend", q, 3, out_dtype, scaling)
        Hq = q.shape[1]
        if bias is not None:
            if tuple(bias.shape) != (self.B, self.len):
                raise MsqError("PackedKV.attend: bias must be [%d, %d]" % (self.B, self.len))
            bias = bias.to(torch.float32).contiguous()
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

    def _capturing(self):
        return False

    def crop(self, n):
        """keep the first n tokens (0 <= n <= len): dequantize() of those is the same bits before and after.  n in the tail: tail_len
        changes.  n < packed_len: packed_len := n - n % gap and the tail becomes the unpacked codes packed_len .. n (the values dequantize()
        gave for them); the planes before packed_len are not touched."""
        n = int(n)
        if not 0 <= n <= self.len:
            raise MsqError("PackedKV.crop: n must be 0 .. %d (the cached length), not %d" % (self.len, n))
        if self._capturing():
            raise MsqError("PackedKV.crop runs on host lengths and cannot be captured")
        if n >= self.packed_len:
            self.tail_len = n - self.packed_len
            return
        packed = n - n % self.gap
        rest = n - packed
        if rest:
            k, v = self._unpack(packed, rest)
            self._tail_put(k, v, 0)
        self.packed_len, self.tail_len = packed, rest

    def attend_multi(self, q, bias=None, causal=True, scaling=None, out_dtype=None):
        """softmax(scaling q K^T + bias + causal) V for the LAST T tokens the cache holds (append first, then attend), 1 <= T <= 32, over the
        codes and the tail (csrc/msq_kv_packed_multi.hip).  q [B, Hq, T, D] in the cache dtype; with causal, query t sees the positions
        <= len - T + t; bias float32 (may hold -inf) [B, len] (one row for every t) or [B, T, len], or None; returns [B, T, Hq, D] in
        out_dtype (the q dtype or float32).  A row whose every position is masked gives zeros."""
        q, out_dtype, scaling = self._prep_q("PackedKV.attend_multi", q, 4, out_dtype, scaling)
        Hq, T = int(q.shape[1]), int(q.shape[2])
        if not 1 <= T <= MAX_QUERY_TOKENS:
            raise MsqError("PackedKV.attend_multi: 1 .. %d query tokens, not %d" % (MAX_QUERY_TOKENS, T))
        if T > self.len:
            raise MsqError("PackedKV.attend_multi: %d query tokens but the cache holds %d (append first: the query tokens are the cache's last T)"
                           % (T, self.len))
        stride_t = 0
        if bias is not None:
            if tuple(bias.shape) == (self.B, T, self.len):
                stride_t = self.len
            elif tuple(bias.shape) != (self.B, self.len):
                raise MsqError("PackedKV.attend_multi: bias must be [%d, %d] or [%d, %d, %d]" % (self.B, self.len, self.B, T, self.len))
        _need_cuda(q, bias)
        if self._capturing():
            raise MsqError("PackedKV.attend_multi runs on host lengths and cannot be captured")
        if bias is not None:
            bias = bias.to(torch.float32).contiguous()
        need = lib().msq_kv_mx_attn_multi_workspace_bytes(self.B, Hq, self.Hkv, self.D, T, self.packed_len, self.tail_len)
        if need < 0:
            check(int(need), "msq_kv_mx_attn_multi_workspace_bytes")
        ws = self._ws_multi
        if ws is None or ws.numel() < need:
            ws = self._ws_multi = torch.empty(int(need), dtype=torch.uint8, device=self.device)
        out = torch.empty(self.B, T, Hq, self.D, dtype=out_dtype, device=self.device)
        p = self.planes
        check(lib().msq_kv_mx_attn_multi(ptr(q), _DT[q.dtype], ptr(p["k_codes"]), ptr(p["k_scales"]), ptr(p["v_codes"]), ptr(p["v_scales"]),
                                         self.packed_len, self.capacity, ptr(self.k_tail), ptr(self.v_tail), self.tail_len, self.gap,
                                         ptr(bias), stride_t, int(bool(causal)), ptr(out), _DT[out_dtype], self.B, Hq, self.Hkv, self.D, T,
                                         self.fmt_id, scaling, ptr(ws), ws.numel(), current_stream(self.device)), "msq_kv_mx_attn_multi")
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


def attn_plan_cap(B, Hq, Hkv, D, S_cap, tail_cap):
    """(max_splits, workspace_bytes) of the device-length decode entry for planes of S_cap tokens: the largest n_splits of attn_plan over
    every S_packed <= S_cap (host arithmetic)."""
    ms, wb = C.c_int(-1), C.c_int64(-1)
    check(lib().msq_kv_mx_attn_plan_cap(B, Hq, Hkv, D, S_cap, tail_cap, C.byref(ms), C.byref(wb)), "msq_kv_mx_attn_plan_cap")
    return ms.value, wb.value


class StaticPackedKV(PackedKV):
    """PackedKV with planes allocated once for `max_len` tokens (rounded up to a multiple of `gap`) and the lengths held on the device:
    ``state`` = int32[4] {packed_len, tail_len, status, 0}.

    A single-token ``append`` and ``attend_dev`` read the lengths from ``state`` inside their kernels; their launches do not depend on the
    lengths, so the pair can be captured in a HIP graph (one stream, a linear chain) and replayed.  ``packed_len`` / ``tail_len`` are the
    host's mirror: every Python call advances them arithmetically, never by a device read.  A replay does not go through Python: call
    ``advance_host(n)`` after n replayed steps, or ``sync()`` to read the state back (which also raises on a status bit).  A warm-up before
    capture moves the lengths like any other step: undo it with ``set_lengths``."""

    _APPEND_ENTRY, _ATTN_ENTRY = "msq_kv_mx_append_dev", "msq_kv_mx_attn_decode_dev"      # SlotPackedKV: the _seq entries, the same arguments

    def __init__(self, B, Hkv, D, dtype, elem_format="fp8_e4m3", gap=32, max_len=256, device="cuda"):
        _check_gap("StaticPackedKV", gap)
        if max_len <= 0:
            raise MsqError("StaticPackedKV: max_len must be positive")
        self.S_cap = (int(max_len) + gap - 1) // gap * gap
        self._ws_dev = {}                                        # Hq -> workspace: never replaced, a captured graph holds its address
        self._bias_pad = None
        super().__init__(B, Hkv, D, dtype, elem_format, gap, self.S_cap, device)
        self._alloc_state()

    # ---- storage and launches (overridden by the host test's stub) -----------------------------------------------------------------
    def _reserve(self, need):
        if need > self.S_cap:
            raise MsqError("StaticPackedKV: %d packed tokens exceed the capacity of %d" % (need, self.S_cap))
        if self.planes is None:
            self._alloc_planes()

    def _alloc_planes(self):
        self.planes = {n: torch.zeros(s, dtype=torch.uint8, device=self.device)
                       for n, s in plane_shapes(self.B, self.Hkv, self.S_cap, self.D, self.elem_format).items()}
        self.capacity = self.S_cap

    def _alloc_state(self):
        self.state = torch.zeros(4, dtype=torch.int32, device=self.device)

    def _write_state(self, clear_status=False):
        """one host-to-device copy: the mirror's lengths (and, with clear_status, zeros for the status word)"""
        if clear_status:
            self.state.copy_(torch.tensor([self.packed_len, self.tail_len, 0, 0], dtype=torch.int32))
        else:
            self.state[:2].copy_(torch.tensor([self.packed_len, self.tail_len], dtype=torch.int32))

    def _read_state(self):
        return self.state.tolist()                               # one device-to-host copy

    def _capturing(self):
        return torch.cuda.is_current_stream_capturing()

    def _append_dev(self, k, v):
        k, v = k.contiguous(), v.contiguous()
        if k.data_ptr() % 16 or v.data_ptr() % 16:
            if self._capturing():
                raise MsqError("StaticPackedKV.append: k and v must be 16-byte aligned during capture")
            k, v = k.clone(), v.clone()
        p = self.planes
        check(getattr(lib(), self._APPEND_ENTRY)(ptr(k), ptr(v), _DT[self.dtype], ptr(p["k_codes"]), ptr(p["k_scales"]), ptr(p["v_codes"]),
                                                 ptr(p["v_scales"]), self.S_cap, ptr(self.k_tail), ptr(self.v_tail), self.gap, ptr(self.state),
                                                 self.B, self.Hkv, self.D, self.fmt_id, current_stream(self.device)), self._APPEND_ENTRY)

    # ---- the cache ------------------------------------------------------------------------------------------------------------------
    def _after_steps(self, n):
        """the mirror's lengths after n single-token appends; raises when the cache cannot take all n"""
        p, t, taken = _step_lengths(self.packed_len, self.tail_len, n, self.S_cap, self.gap)
        if taken < n:
            raise MsqError("StaticPackedKV: %d more token(s) overflow the capacity of %d packed tokens (MSQ_STATUS_OVERFLOW on the device)"
                           % (n, self.S_cap))
        return p, t

    def advance_host(self, n=1):
        """apply n single-token steps to the host mirror (after n replays of a captured step); no device access"""
        self.packed_len, self.tail_len = self._after_steps(int(n))

    def append(self, k, v):
        self._check_kv(k, v)
        T = k.shape[2]
        if T == 0:
            return
        if T == 1:
            after = self._after_steps(1)                         # raises before any launch when the mirror knows the cache is full
            self._append_dev(k, v)
            self.packed_len, self.tail_len = after
            return
        if self._capturing():
            raise MsqError("StaticPackedKV.append: a multi-token append runs on host lengths and cannot be captured")
        super().append(k, v)
        self._write_state()

    def _check_lengths(self, who, packed_len, tail_len):
        packed_len, tail_len = int(packed_len), int(tail_len)
        if packed_len < 0 or packed_len % self.gap or packed_len > self.S_cap or not 0 <= tail_len <= self.gap:
            raise MsqError(who + ".set_lengths: packed_len must be a multiple of gap within the capacity, tail_len within the tail")
        return packed_len, tail_len

    def set_lengths(self, packed_len, tail_len):
        """mirror and device state := (packed_len, tail_len), status cleared: restore after a warm-up, roll back"""
        self.packed_len, self.tail_len = self._check_lengths("StaticPackedKV", packed_len, tail_len)
        self._write_state(clear_status=True)

    def crop(self, n):
        """PackedKV.crop, then the device state takes the mirror's lengths (one host-to-device copy).  n is counted on the MIRROR: after graph
        replays call advance_host(steps) or sync() first, or the state is overwritten with lengths that are behind the device's."""
        super().crop(n)
        self._write_state()

    def sync(self):
        """read the device state back (one copy): the mirror takes its lengths; a status bit raises MsqError (set_lengths clears it)"""
        packed_len, tail_len, status, _ = self._read_state()
        self.packed_len, self.tail_len = int(packed_len), int(tail_len)
        if status:
            raise MsqError("StaticPackedKV: " + " | ".join(_status_names(status)) + " (overflow: an append found the cache full and dropped the "
                           "token; nan: a packed block holds Inf / NaN; set_lengths clears it)")
        return self.packed_len, self.tail_len

    def attend_dev(self, q, bias=None, scaling=None, out_dtype=None):
        """attend() with the lengths read from the device state by the kernels: the same bits as attend() at equal lengths, zeros for an
        empty cache.  bias [B, W] float32, indexed by the absolute token position; W >= S_cap + gap is used in place (entries at or beyond
        the length are never read; this is the form to capture), a narrower one must be [B, len] of the mirror and is copied into a buffer
        of that width first.  The workspace is allocated on the first call for a given Hq: run one eager call before capturing."""
        _need_cuda(q, bias)
        q, out_dtype, scaling = self._prep_q("StaticPackedKV.attend_dev", q, 3, out_dtype, scaling)
        Hq = q.shape[1]
        capturing = self._capturing()
        width = self.S_cap + self.gap
        if bias is not None:
            if bias.ndim != 2 or bias.shape[0] != self.B:
                raise MsqError("StaticPackedKV.attend_dev: bias must be [%d, W]" % self.B)
            if bias.shape[1] >= width:
                if bias.dtype != torch.float32 or not bias.is_contiguous():
                    bias = bias.to(torch.float32).contiguous()
            else:
                if bias.shape[1] != self.len:
                    raise MsqError("StaticPackedKV.attend_dev: bias must be [%d, %d] (the length) or at least %d wide" % (self.B, self.len, width))
                if self._bias_pad is None:
                    if capturing:
                        raise MsqError("StaticPackedKV.attend_dev: pass a bias at least %d wide during capture" % width)
                    self._bias_pad = torch.zeros(self.B, width, dtype=torch.float32, device=self.device)
                self._bias_pad[:, :bias.shape[1]] = bias
                bias = self._bias_pad
        ws = self._ws_dev.get(Hq)
        if ws is None:
            if capturing:
                raise MsqError("StaticPackedKV.attend_dev: the workspace is not allocated yet: run one eager attend_dev call before capturing")
            ws = self._ws_dev[Hq] = torch.empty(attn_plan_cap(self.B, Hq, self.Hkv, self.D, self.S_cap, self.gap)[1], dtype=torch.uint8,
                                                device=self.device)
        out = torch.empty(self.B, Hq, self.D, dtype=out_dtype, device=self.device)
        p = self.planes
        check(getattr(lib(), self._ATTN_ENTRY)(ptr(q), _DT[q.dtype], ptr(p["k_codes"]), ptr(p["k_scales"]), ptr(p["v_codes"]), ptr(p["v_scales"]),
                                               self.S_cap, ptr(self.k_tail), ptr(self.v_tail), self.gap, ptr(self.state), ptr(bias),
                                               bias.shape[1] if bias is not None else 0, ptr(out), _DT[out_dtype], self.B, Hq, self.Hkv,
                                               self.D, self.fmt_id, scaling, ptr(ws), ws.numel(), current_stream(self.device)),
              self._ATTN_ENTRY)
        return out


class _SlotView(PackedKV):
    """One slot of a SlotPackedKV as a PackedKV of batch 1 over that slot's (contiguous) slice of the planes and the tail: no storage of its
    own, the lengths copied from the owner's mirror.  The host paths of PackedKV -- append by the timing rule, crop, dequantize -- run on it
    unchanged, and msq_kv_mx_pack sees B = 1."""

    def __init__(self, owner, slot):
        self.B, self.Hkv, self.D, self.dtype = 1, owner.Hkv, owner.D, owner.dtype
        self.elem_format, self.fmt_id, self.gap, self.device = owner.elem_format, owner.fmt_id, owner.gap, owner.device
        self.capacity = owner.S_cap
        self.packed_len, self.tail_len = owner._lens[slot]
        self.planes = {n: t[slot:slot + 1] for n, t in owner.planes.items()}
        self.k_tail, self.v_tail = owner.k_tail[slot:slot + 1], owner.v_tail[slot:slot + 1]
        self._ws = self._ws_multi = None

    def _reserve(self, need):
        if need > self.capacity:
            raise MsqError("SlotPackedKV: %d packed tokens exceed a slot's capacity of %d" % (need, self.capacity))


_NO_SHARED_LENGTH = ("SlotPackedKV: attend, attend_multi and the transformers Cache wrapper are not offered on this class: both run on one "
                     "shared host length, and transformers batches by left padding (use append / attend_dev, and prefill per slot)")


class SlotPackedKV(StaticPackedKV):
    """StaticPackedKV for a RAGGED batch: B slots of `max_len` tokens, ``state`` = int32[B, 4] with one row
    {packed_len, tail_len, status, flags} per slot (flags bit 0: the slot is idle).

    ``append(k, v)`` ([B, Hkv, 1, D]: one token for every slot that is not idle) and ``attend_dev(q)`` read every slot's own row inside their
    kernels, with launches that depend on no length: the pair is captured once and replayed for ever, and between replays a slot is emptied
    (``reset``), filled with a new prompt (``prefill``, the host path on that slot's slice of the planes), parked (``set_idle``) or cut
    (``crop``) while the others go on.  ``lengths`` is the host's mirror per slot, advanced arithmetically (``advance_host`` after replays);
    ``sync()`` reads the state back.  A slot that is full keeps its bytes and lengths and reports MSQ_STATUS_OVERFLOW in its own status word;
    the others advance."""

    _APPEND_ENTRY, _ATTN_ENTRY = "msq_kv_mx_append_seq", "msq_kv_mx_attn_decode_seq"
    _VIEW = _SlotView                                            # overridden by the host test's stub

    def __init__(self, B, Hkv, D, dtype, elem_format="fp8_e4m3", gap=32, max_len=256, device="cuda"):
        self._lens = [(0, 0)] * int(B)                           # the mirror: (packed_len, tail_len) per slot
        self._idle = [False] * int(B)
        super().__init__(B, Hkv, D, dtype, elem_format, gap, max_len, device)

    # ---- storage (overridden by the host test's stub) ------------------------------------------------------------------------------
    def _alloc_state(self):
        self.state = torch.zeros(self.B, 4, dtype=torch.int32, device=self.device)

    def _write_row(self, slot, what):
        """one host-to-device copy into slot's state row: "lengths" (words 0 .. 1), "flags" (word 3) or "all" (status cleared too)"""
        p, t = self._lens[slot]
        flags = SLOT_IDLE if self._idle[slot] else 0
        if what == "lengths":
            self.state[slot, :2].copy_(torch.tensor([p, t], dtype=torch.int32))
        elif what == "flags":
            self.state[slot, 3:].copy_(torch.tensor([flags], dtype=torch.int32))
        else:
            self.state[slot].copy_(torch.tensor([p, t, 0, flags], dtype=torch.int32))

    # ---- the mirror ----------------------------------------------------------------------------------------------------------------
    @property
    def lengths(self):
        """[(packed_len, tail_len)] per slot, from the host mirror"""
        return list(self._lens)

    @property
    def len(self):
        raise MsqError("SlotPackedKV has a length per slot: use lengths")

    def __bool__(self):                                          # not __len__, which has no one answer here
        return True

    def _slot(self, slot):
        slot = int(slot)
        if not 0 <= slot < self.B:
            raise MsqError("SlotPackedKV: slot must be 0 .. %d, not %d" % (self.B - 1, slot))
        return slot

    def _slot_after(self, slot, n):
        """(lengths of the slot after n single-token steps, does it take all n): a slot holds S_cap packed tokens + a full tail and stays there"""
        p, t, taken = _step_lengths(*self._lens[slot], n, self.S_cap, self.gap)
        return (p, t), taken == n

    def _steps(self, n, who):
        live = [b for b in range(self.B) if not self._idle[b]]
        after = {b: self._slot_after(b, n) for b in live}
        if n > 0 and live and not any(ok for _, ok in after.values()):
            raise MsqError("SlotPackedKV.%s: %d more token(s) overflow every live slot (capacity %d packed tokens; MSQ_STATUS_OVERFLOW on the "
                           "device)" % (who, n, self.S_cap))
        return after

    def advance_host(self, n=1):
        """apply n single-token steps to the mirror of every slot that is not idle (after n replays); a slot that fills up stops where the
        device stops (its status word reports the overflow); refused when every live slot would overflow.  No device access."""
        for b, (lens, _) in self._steps(int(n), "advance_host").items():
            self._lens[b] = lens

    def append(self, k, v):
        """one token [B, Hkv, 1, D] for every slot that is not idle (an idle slot's row of k, v is ignored); can be captured.  Refused before
        launching only if EVERY live slot would overflow; otherwise an overflowing slot's mirror stays and its device status reports it."""
        self._check_kv(k, v)
        if k.shape[2] != 1:
            raise MsqError("SlotPackedKV.append takes one token per slot, [%d, %d, 1, %d]: more tokens go to one slot through prefill(slot, k, v)"
                           % (self.B, self.Hkv, self.D))
        after = self._steps(1, "append")
        self._append_dev(k, v)
        for b, (lens, _) in after.items():
            self._lens[b] = lens

    def _host_only(self, who):
        if self._capturing():
            raise MsqError("SlotPackedKV.%s writes a state row from the host and cannot be captured (call it between replays)" % who)

    def prefill(self, slot, k, v):
        """append T tokens k, v [1, Hkv, T, D] to ONE slot on the host path, by the timing rule of PackedKV.append (msq_kv_mx_pack on the
        slot's slice of the planes with B = 1, the rest into the slot's tail rows), then one host-to-device copy of the slot's lengths.
        The other slots' bytes and rows are not touched.  Refused during capture."""
        slot = self._slot(slot)
        self._host_only("prefill")
        view = self._VIEW(self, slot)
        view.append(k, v)
        self._lens[slot] = (view.packed_len, view.tail_len)
        self._write_row(slot, "lengths")

    def reset(self, slot):
        """slot := empty: lengths 0, status 0, not idle (one host-to-device copy); its bytes stay and are overwritten by what comes next"""
        slot = self._slot(slot)
        self._host_only("reset")
        self._lens[slot], self._idle[slot] = (0, 0), False
        self._write_row(slot, "all")

    def set_idle(self, slot, idle=True):
        """an idle slot takes no token, keeps its lengths and bytes, raises no status, and its rows of attend_dev are zeros"""
        slot = self._slot(slot)
        self._host_only("set_idle")
        self._idle[slot] = bool(idle)
        self._write_row(slot, "flags")

    def set_lengths(self, slot, packed_len, tail_len):
        """mirror and state row of one slot := (packed_len, tail_len), status cleared: restore after a warm-up, roll back"""
        slot = self._slot(slot)
        self._host_only("set_lengths")
        self._lens[slot] = self._check_lengths("SlotPackedKV", packed_len, tail_len)
        self._write_row(slot, "all")

    def crop(self, slot, n):
        """PackedKV.crop on one slot (n counted on the MIRROR), then that slot's state row takes the lengths"""
        slot = self._slot(slot)
        self._host_only("crop")
        view = self._VIEW(self, slot)
        view.crop(n)
        self._lens[slot] = (view.packed_len, view.tail_len)
        self._write_row(slot, "lengths")

    def dequantize(self, slot):
        """one slot's K and V as [1, Hkv, len, D] in the cache dtype"""
        return self._VIEW(self, self._slot(slot)).dequantize()

    def sync(self, raise_on_status=True):
        """read the state back (one copy): the mirror takes every slot's lengths and idle flag.  Returns the list of lengths; a status bit
        raises MsqError naming the slot(s) and bit(s) -- or, with raise_on_status=False, returns (lengths, statuses) so that a server can
        retire the one full slot (reset(slot) clears its status)."""
        rows = self._read_state()
        self._lens = [(int(r[0]), int(r[1])) for r in rows]
        self._idle = [bool(int(r[3]) & SLOT_IDLE) for r in rows]
        statuses = [int(r[2]) for r in rows]
        if not raise_on_status:
            return self.lengths, statuses
        bad = ["slot %d: %s" % (b, " | ".join(_status_names(st))) for b, st in enumerate(statuses) if st]
        if bad:
            raise MsqError("SlotPackedKV: " + "; ".join(bad) + " (overflow: an append found the slot full and dropped its token; nan: a packed "
                           "block holds Inf / NaN; reset(slot) clears it)")
        return self.lengths

    def attend_dev(self, q, bias=None, scaling=None, out_dtype=None):
        """row b = softmax(scaling q[b] K_b^T + bias[b]) V_b over slot b's OWN tokens (its lengths read from its state row by the kernels):
        the bits PackedKV.attend gives for that sequence alone; zeros for an empty or idle slot.  bias [B, W] float32 with W >= S_cap + gap,
        indexed by the absolute token position, or None: a ragged batch needs no padding bias.  Can be captured after one eager call."""
        if bias is not None and (bias.ndim != 2 or bias.shape[0] != self.B or bias.shape[1] < self.S_cap + self.gap):
            raise MsqError("SlotPackedKV.attend_dev: bias must be [%d, W] with W >= %d (S_cap + gap): the slots have no common length"
                           % (self.B, self.S_cap + self.gap))
        return super().attend_dev(q, bias, scaling, out_dtype)

    # ---- not offered ---------------------------------------------------------------------------------------------------------------
    def attend(self, *args, **kwargs):
        raise MsqError(_NO_SHARED_LENGTH)

    def attend_multi(self, *args, **kwargs):
        raise MsqError(_NO_SHARED_LENGTH)

    def update(self, *args, **kwargs):                           # the transformers cache-layer protocol
        raise MsqError(_NO_SHARED_LENGTH)

    def get_seq_length(self, *args, **kwargs):
        raise MsqError(_NO_SHARED_LENGTH)


def _make_layer_class():
    from transformers.cache_utils import CacheLayerMixin

    class PackedKVLayer(CacheLayerMixin):
        """One attention layer of PackedMXKVCache.  ``fused`` (set by use_packed_attention): a single-token update hands back the new
        token's K / V only -- the tied attention function reads the codes and never looks at them -- instead of dequantize()."""
        is_sliding = False
        is_compileable = False

        def __init__(self, elem_format="fp8_e4m3", gap=32, capacity=256, max_len=None):
            super().__init__()
            self.elem_format, self.gap, self.capacity, self.max_len = elem_format, gap, capacity, max_len
            self.packed = None
            self.fused = False
            self.fused_max_q = 1                                 # use_packed_attention(max_query_tokens=...): query lengths up to this are fused

        def lazy_initialization(self, key_states, value_states=None):
            _need_cuda(key_states)
            B, H, _, D = key_states.shape
            self.dtype, self.device = key_states.dtype, key_states.device
            if self.max_len is None:
                self.packed = PackedKV(B, H, D, key_states.dtype, self.elem_format, self.gap, self.capacity, key_states.device)
            else:                                                # fixed capacity, lengths on the device: a one-token update is the device append
                self.packed = StaticPackedKV(B, H, D, key_states.dtype, self.elem_format, self.gap, self.max_len, key_states.device)
            self.keys = self.values = None
            self.is_initialized = True

        def update(self, key_states, value_states, *args, **kwargs):
            if not self.is_initialized:
                self.lazy_initialization(key_states, value_states)
            self.packed.append(key_states, value_states)
            if self.fused and 1 <= key_states.shape[2] <= self.fused_max_q:
                return key_states, value_states
            return self.packed.dequantize()

        def crop(self, max_length):
            """keep the first max_length tokens (negative: drop that many from the end), as transformers' DynamicLayer.crop"""
            if self.packed is None:
                return
            if max_length < 0:
                max_length = self.packed.len - abs(max_length)
            if self.packed.len <= max_length:
                return
            self.packed.crop(max(int(max_length), 0))

        def get_seq_length(self):
            return self.packed.len if self.packed is not None else 0

        def get_mask_sizes(self, query_length):
            return self.get_seq_length() + query_length, 0

        def get_max_cache_shape(self):
            return -1

        def get_max_length(self):
            return -1

        def reset(self):
            if isinstance(self.packed, StaticPackedKV):
                self.packed.set_lengths(0, 0)
            elif self.packed is not None:
                self.packed.packed_len = self.packed.tail_len = 0

    return PackedKVLayer


def PackedMXKVCache(num_layers, elem_format="fp8_e4m3", gap=32, capacity=256, max_len=None):
    """A transformers Cache (``past_key_values=PackedMXKVCache(n)``) whose layers hold packed MX planes.  With ``max_len`` the layers are
    StaticPackedKV (fixed capacity, lengths on the device): a one-token update() is the device append, get_seq_length() comes from the host
    mirror without a sync, and the tied attention function calls attend_dev."""
    from transformers.cache_utils import Cache
    layer_cls = _make_layer_class()
    _fmt_id(elem_format)
    _check_gap("PackedMXKVCache", gap)
    if max_len is not None and max_len <= 0:
        raise MsqError("PackedMXKVCache: max_len must be positive")
    return Cache(layers=[layer_cls(elem_format, gap, capacity, max_len) for _ in range(num_layers)])


def _mask_bias(am, B):
    """an sdpa mask slice (bool: True = attend, or additive) -> a float32 bias over B sequences"""
    if am.dtype == torch.bool:
        bias = torch.zeros(am.shape, dtype=torch.float32, device=am.device).masked_fill_(~am, float("-inf"))
    else:
        bias = am.to(torch.float32)
    if bias.shape[0] != B:
        bias = bias.expand(B, *bias.shape[1:])
    return bias


def _packed_attention_forward(module, query, key, value, attention_mask, dropout=0.0, scaling=None, **kwargs):
    from transformers.integrations.sdpa_attention import sdpa_attention_forward
    layer = getattr(module, "_msq_packed_layer", None)
    T = query.shape[2]
    if layer is not None and layer.packed is not None and 2 <= T <= getattr(layer, "fused_max_q", 1):
        bias = None                                              # no mask: the T tokens are the cache's last T, causal among themselves
        if attention_mask is not None:
            if attention_mask.ndim != 4 or attention_mask.shape[1] != 1 or attention_mask.shape[2] != T:
                raise MsqError("msq_packed_kv: expected a [B, 1, %d, S] attention mask at query length %d" % (T, T))
            bias = _mask_bias(attention_mask[:, 0], query.shape[0])
        return layer.packed.attend_multi(query, bias, causal=bias is None, scaling=scaling), None      # [B, T, Hq, D]
    if layer is None or layer.packed is None or T != 1:
        return sdpa_attention_forward(module, query, key, value, attention_mask, dropout=dropout, scaling=scaling, **kwargs)
    bias = None
    if attention_mask is not None:
        if attention_mask.ndim != 4 or attention_mask.shape[1] != 1 or attention_mask.shape[2] != 1:
            raise MsqError("msq_packed_kv: expected a [B, 1, 1, S] attention mask at query length 1")
        bias = _mask_bias(attention_mask[:, 0, 0, :], query.shape[0])
    if isinstance(layer.packed, StaticPackedKV):                 # lengths from the device state; bias_stride = the mask length
        out = layer.packed.attend_dev(query[:, :, 0, :], bias, scaling)
    else:
        out = layer.packed.attend(query[:, :, 0, :], bias, scaling)
    return out.unsqueeze(1), None                                # [B, 1, Hq, D], the layout the attention interface returns


def use_packed_attention(model, cache, max_query_tokens=1):
    """Decode steps of `model` attend over the codes of `cache` (a PackedMXKVCache): registers the attention function "msq_packed_kv",
    ties every attention module to its cache layer (the registered function is not handed past_key_values: the module attribute is the
    link) and selects the function in the model's config.  Query lengths 2 .. max_query_tokens (at most 32) go to attend_multi (a
    [B, 1, T, S] mask becomes its [B, T, S] bias, no mask means causal); longer ones -- with the default of 1, every length above 1 -- go
    to sdpa on the dequantised tensors."""
    max_query_tokens = int(max_query_tokens)
    if not 1 <= max_query_tokens <= MAX_QUERY_TOKENS:
        raise MsqError("use_packed_attention: max_query_tokens must be 1 .. %d" % MAX_QUERY_TOKENS)
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
        cache.layers[idx].fused_max_q = max_query_tokens
        tied += 1
    if not tied:
        raise MsqError("use_packed_attention: no attention module (layer_idx + q_proj / k_proj) found in the model")
    model.config._attn_implementation = ATTENTION_NAME
    return model
