// msq_kv_packed_common.h -- what the two attention translation units of the packed MX KV cache share (msq_kv_packed.hip: one query token,
// msq_kv_packed_multi.hip: 1 .. 32 query tokens on the matrix cores): the scalar helpers, the code-to-float conversion, the token-split plan,
// the readers of the device-held lengths, the split-combine kernel and the host checks of the attention entries.  One statement of each;
// everything sits in an anonymous namespace, so each unit keeps its own internal copy and its own kernel instantiations.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/msq.h"
#include "msq_device.h"

extern "C" void msq_set_error_(const char* msg);      // msq_quant.hip: the message msq_last_error() returns

namespace {

using namespace msq;

typedef float v2f_t __attribute__((ext_vector_type(2)));

constexpr float LOG2E = 1.44269504088896340736f;
MSQ_D float ex(float x) { return __builtin_amdgcn_exp2f(x * LOG2E); }                 // e^x; e^-inf = 0
MSQ_D float e8m0_f32(uint32_t sb) { return sb ? u2f(sb << 23) : u2f(0x00400000u); }   // 2^(sb - 127)
MSQ_D float neg_inf() { return -__builtin_inff(); }

// value of a code pair: the scaled convert at scale 1, then the exact power of two (scale byte 255: the block held Inf / NaN)
MSQ_D float apply_e8m0(float v, int sb) { return sb == 255 ? u2f(0x7FC00000u) : __builtin_ldexpf(v, sb - 127); }

// the two values of a word of a 16-bit tensor (low half first); half_lo / half_hi: the dtype as an argument (1 f16, 2 bf16)
MSQ_D float bf16_lo(uint32_t w) { return u2f(w << 16); }
MSQ_D float bf16_hi(uint32_t w) { return u2f(w & 0xFFFF0000u); }
MSQ_D float f16_lo(uint32_t w) { return (float)__builtin_bit_cast(_Float16, (uint16_t)(w & 0xFFFFu)); }
MSQ_D float f16_hi(uint32_t w) { return (float)__builtin_bit_cast(_Float16, (uint16_t)(w >> 16)); }
MSQ_D float half_lo(uint32_t w, int dt) { return dt == 1 ? f16_lo(w) : bf16_lo(w); }
MSQ_D float half_hi(uint32_t w, int dt) { return dt == 1 ? f16_hi(w) : bf16_hi(w); }

// channel pair j (0 .. 3) of 8 codes of one token (8 consecutive channels: e2m1 in c0, e4m3 in c0 and c1) x the scale operand `sc`.  The
// converts take the pair's position as an immediate, hence the ladder.
template <bool FP4> MSQ_D v2f_t cvt_pair(uint32_t c0, uint32_t c1, float sc, int j) {
    if (FP4) {
        if (j == 0) return __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(c0, sc, 0);
        else if (j == 1) return __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(c0, sc, 1);
        else if (j == 2) return __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(c0, sc, 2);
        else return __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(c0, sc, 3);
    } else {
        if ((j & 1) == 0) return __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(j < 2 ? c0 : c1, sc, false);
        else return __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(j < 2 ? c0 : c1, sc, true);
    }
}
// all 8 codes -> 4 float pairs
template <bool FP4> MSQ_D void cvt8(uint32_t c0, uint32_t c1, float sc, float (&f)[8]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const v2f_t v = cvt_pair<FP4>(c0, c1, sc, j);
        f[2 * j] = v[0]; f[2 * j + 1] = v[1];
    }
}

// Token splits of the attention kernels: a function of the packed groups alone (not of the batch or the head count), so a sequence gives the
// same bits whatever it is batched with.  A split is a whole number of groups of 32, a multiple of 4 groups (one per wave), at most 64 splits.
// The one statement of the rule: the host plan and the device-length kernels both call it.
struct AttnPlan { int nsplit, gps; };
MSQ_HD AttnPlan attn_split_plan(int64_t ng) {
    int64_t gps = (ng + 63) / 64;
    gps = (gps + 3) / 4 * 4;
    if (gps < 4) gps = 4;
    AttnPlan p;
    p.gps = (int)gps;
    p.nsplit = ng ? (int)((ng + gps - 1) / gps) : 1;
    return p;
}
// what split `split` of the plan covers: npk packed groups from group g0 on, then ntc chunks of 32 tail tokens.  Reference outputs on purpose:
// a returned aggregate reschedules the prologue of every kernel that calls this
MSQ_D void split_range(int split, int nsplit, int gps, int S_packed, int tail_len, int& g0, int& npk, int& ntc) {
    const int ngroups = S_packed / 32;
    g0 = split * gps;
    const int g1 = (g0 + gps < ngroups) ? g0 + gps : ngroups;
    npk = g1 > g0 ? g1 - g0 : 0;
    ntc = (split == nsplit - 1) ? (tail_len + 31) / 32 : 0;      // the last split also takes the tail, 32 tokens at a time
}

// ---- device-held lengths: state = int32[4] {packed_len, tail_len, status, 0} of one layer, read by every block of a launch
// and changed only by k_kvp_advance, a launch of its own behind every reader on the stream.
// What a single-token append does in the state it finds: 0 nothing (the cache is full, or the state is not one this library wrote),
// 1 the token goes to tail slot `slot`, 2 the full tail is packed at token `pos` first and the token goes to slot 0.
// UNIFORM = false (the advance of the per-sequence form, one lane per slot): `state` differs between the lanes, a per-lane read.
template <bool UNIFORM = true>
MSQ_D int append_step(const int* state, int64_t S_cap, int tail_cap, int& pos, int& slot) {
    const int pl = UNIFORM ? __builtin_amdgcn_readfirstlane(state[0]) : state[0], tl = UNIFORM ? __builtin_amdgcn_readfirstlane(state[1]) : state[1];
    pos = pl; slot = tl;
    if (pl < 0 || pl % 32 || pl > S_cap || tl < 0 || tl > tail_cap) return 0;
    if (tl < tail_cap) return 1;
    if ((int64_t)pl + tail_cap > S_cap) return 0;
    slot = 0;
    return 2;
}
// SEQ: `row` is the state row of the ONE slot this block works for (the slot is a grid axis, so the read is wave-uniform
// like the shared row's).  3: the slot is idle (flags bit 0): nothing is written, the lengths stay and no status is raised.
MSQ_D int append_step_seq(const int* row, int64_t S_cap, int tail_cap, int& pos, int& slot) {
    if (__builtin_amdgcn_readfirstlane(row[3]) & MSQ_KV_SLOT_IDLE) { pos = 0; slot = 0; return 3; }
    return append_step(row, S_cap, tail_cap, pos, slot);
}
// the lengths a device-length launch works with: whatever the state holds, cut to the planes and the tail it was given
MSQ_D void dev_lengths(const int* state, int64_t S_cap, int tail_cap, int& S_packed, int& tail_len) {
    int pl = __builtin_amdgcn_readfirstlane(state[0]), tl = __builtin_amdgcn_readfirstlane(state[1]);
    pl = pl < 0 ? 0 : (pl > S_cap ? (int)S_cap : pl);
    S_packed = pl & ~31;
    tail_len = tl < 0 ? 0 : (tl > tail_cap ? tail_cap : tl);
}
// SEQ: the lengths of the slot whose state row is `row`; an idle slot counts as empty (its output rows are zeros)
MSQ_D void seq_lengths(const int* row, int64_t S_cap, int tail_cap, int& S_packed, int& tail_len) {
    dev_lengths(row, S_cap, tail_cap, S_packed, tail_len);
    if (__builtin_amdgcn_readfirstlane(row[3]) & MSQ_KV_SLOT_IDLE) { S_packed = 0; tail_len = 0; }
}

// the splits of one output row in ascending order; a row whose every position is masked gives zeros.  The host-length form (DEV = false):
// the row is blockIdx.x -- b * Hq + hq for one query token, (b * T + t) * Hq + hq for T -- and `state` / `S_cap` are not looked at.
// DEV: the number of live splits comes from the state, as in k_kvp_attn_split
// SEQ: the grid is (Hq, B), `nsplit` arrives as the row stride (max_splits) and the live count comes from the sequence's own state row
// ODT: 0 float32, 1 f16, 2 bf16
template <int D, int ODT, bool DEV = false, bool SEQ = false>
__global__ void __launch_bounds__(D)
k_kvp_attn_combine(const float* __restrict__ ws, void* __restrict__ out, int nsplit, const int* state, int64_t S_cap) {
    const int wstride = nsplit;
    if (DEV) {
        int S_packed, tail_len;
        if (SEQ) seq_lengths(state + 4 * (int64_t)blockIdx.y, S_cap, 0, S_packed, tail_len);
        else dev_lengths(state, S_cap, 0, S_packed, tail_len);
        nsplit = attn_split_plan(S_packed / 32).nsplit;
    }
    const int d = threadIdx.x;
    const int64_t row = SEQ ? (int64_t)blockIdx.y * gridDim.x + blockIdx.x : (int64_t)blockIdx.x;
    const float* p = ws + row * (SEQ ? wstride : nsplit) * (D + 2);
    float mn = neg_inf();
    for (int s = 0; s < nsplit; ++s) mn = __builtin_fmaxf(mn, p[s * (D + 2) + D]);
    const float mm = (mn == neg_inf()) ? 0.f : mn;
    float num = 0.f, den = 0.f;
    for (int s = 0; s < nsplit; ++s) {
        const float f = ex(p[s * (D + 2) + D] - mm);
        num += p[s * (D + 2) + d] * f; den += p[s * (D + 2) + D + 1] * f;
    }
    const float y = den > 0.f ? num / den : 0.f;
    if (ODT == 0) reinterpret_cast<float*>(out)[row * D + d] = y;
    else if (ODT == 1) reinterpret_cast<uint16_t*>(out)[row * D + d] = __builtin_bit_cast(uint16_t, (_Float16)y);
    else reinterpret_cast<uint16_t*>(out)[row * D + d] = __builtin_bit_cast(uint16_t, (__bf16)y);
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------------
inline int kvp_fail(int code, const char* msg) { msq_set_error_(msg); return code; }
// "<entry>: <what>" as the message msq_last_error() returns
inline int kvp_fail_in(int code, const char* who, const char* what) {
    char msg[256];
    snprintf(msg, sizeof(msg), "%s: %s", who, what);
    return kvp_fail(code, msg);
}

// the checks of the sizes every attention entry starts with + the plan
inline int attn_plan(int64_t B, int Hq, int Hkv, int D, int64_t S_packed, int64_t tail_len, AttnPlan* p) {
    if (B <= 0 || Hq <= 0 || Hkv <= 0 || S_packed < 0 || tail_len < 0) return kvp_fail(MSQ_ERR_BAD_ARG, "msq_kv_mx_attn: sizes must be positive");
    if (Hq % Hkv) return kvp_fail(MSQ_ERR_BAD_ARG, "msq_kv_mx_attn: Hq must be a multiple of Hkv");
    if (Hq / Hkv > 8) return kvp_fail(MSQ_ERR_UNSUPPORTED, "msq_kv_mx_attn: at most 8 query heads per kv head");
    if (D != 64 && D != 128) return kvp_fail(MSQ_ERR_UNSUPPORTED, "msq_kv_mx_attn: head_dim must be 64 or 128");
    if (S_packed % 32) return kvp_fail(MSQ_ERR_BAD_ARG, "msq_kv_mx_attn: S_packed must be a multiple of 32");
    if (S_packed + tail_len == 0) return kvp_fail(MSQ_ERR_BAD_ARG, "msq_kv_mx_attn: the cache is empty");
    if (S_packed > (int64_t)1 << 30 || tail_len > (int64_t)1 << 20 || B > 65535 || Hkv > 65535)
        return kvp_fail(MSQ_ERR_UNSUPPORTED, "msq_kv_mx_attn: sizes beyond the launch grid");
    *p = attn_split_plan(S_packed / 32);
    return MSQ_OK;
}

// the nine pointers AttnArgs and MultiArgs begin with
template <class ARGS>
void set_attn_buffers(ARGS& A, const void* q, const void* k_codes, const void* k_scales, const void* v_codes, const void* v_scales, const void* k_tail,
                      const void* v_tail, const float* bias, void* workspace) {
    A.q = q; A.kc = (const uint8_t*)k_codes; A.ks = (const uint8_t*)k_scales; A.vc = (const uint8_t*)v_codes; A.vs = (const uint8_t*)v_scales;
    A.kt = k_tail; A.vt = v_tail; A.bias = bias; A.ws = (float*)workspace;
}

// What the three attention entries check after the sizes, on the pointers set_attn_buffers stored: the formats, then `own` -- the entry's own
// checks of lengths, strides and state (all MSQ_ERR_BAD_ARG; the message of the first that failed, or null) --, then the buffers, which are
// looked at last.  planes / tail: does a launch read them (a host-length entry: the length is not 0).  state: null for a host-length entry.
template <class ARGS>
int check_attn_common(const char* who, const ARGS& A, const void* out, const void* state, int elem_fmt, int q_dtype, int out_dtype, const char* own,
                      bool planes, bool tail, int64_t workspace_bytes, int64_t need, const char* workspace_what) {
    if (elem_fmt != MSQ_FMT_FP8_E4M3 && elem_fmt != MSQ_FMT_FP4_E2M1) return kvp_fail_in(MSQ_ERR_UNSUPPORTED, who, "elem_fmt must be fp8_e4m3 or fp4_e2m1");
    if (q_dtype != 1 && q_dtype != 2) return kvp_fail_in(MSQ_ERR_UNSUPPORTED, who, "q and the tail must be f16 (1) or bf16 (2)");
    if (out_dtype != 0 && out_dtype != q_dtype) return kvp_fail_in(MSQ_ERR_UNSUPPORTED, who, "out must be float32 or the q dtype");
    if (own) return kvp_fail_in(MSQ_ERR_BAD_ARG, who, own);
    if (!A.q || !out || !A.ws) return kvp_fail_in(MSQ_ERR_BAD_ARG, who, "null buffer");
    if (planes && (!A.kc || !A.ks || !A.vc || !A.vs)) return kvp_fail_in(MSQ_ERR_BAD_ARG, who, "null buffer (planes)");
    if (tail && (!A.kt || !A.vt)) return kvp_fail_in(MSQ_ERR_BAD_ARG, who, "null buffer (tail)");
    if (workspace_bytes < need) return kvp_fail_in(MSQ_ERR_BAD_ARG, who, workspace_what);
    if ((((uintptr_t)A.q | (uintptr_t)A.kc | (uintptr_t)A.ks | (uintptr_t)A.vc | (uintptr_t)A.kt | (uintptr_t)A.vt | (uintptr_t)A.ws | (uintptr_t)state) & 15) != 0)
        return kvp_fail_in(MSQ_ERR_BAD_ARG, who, "buffers must be 16-byte aligned");      // v_scales, bias and out are read / written one element at a time
    return MSQ_OK;
}

}  // namespace
