// msq_kv_packed.hip -- the PACKED MX KV cache: plain OCP-MX codes + E8M0 scale bytes instead of fake-quantised
// half-precision tensors, and single-token decode attention that reads the codes.
//
// Planes of one attention layer (B sequences, H kv heads, S_cap tokens, head_dim D; KIVI's axes, the ones msq.kvcache.mx_quantize_keys /
// mx_quantize_values use):
//   K codes  [B, H, S_cap, D] bytes (e4m3) or [B, H, S_cap, D / 2] bytes (e2m1, even d in the low nibble)
//   K scales [B, H, S_cap / 32, D] bytes      one block = 32 consecutive TOKENS of one channel
//   V codes  as K codes
//   V scales [B, H, S_cap, D / 32] bytes      one block = 32 consecutive head_dim entries of one token
// decode(code) * 2^(scale - 127) == _quantize_mx(x.float(), 8, fmt, axes=[axis], block_size=32) bit for bit: the float32 Python-path
// arithmetic of msq_mx.hip k_mx_pack (shared exponent floor(torch.log2(max)), round half away through the sticky bit, e4m3 clamped first).
//
// Attention: out = softmax(scaling q K^T + bias) V for ONE query token per sequence over the packed tokens 0 .. S_packed and then the
// tail (tokens that do not fill a group yet, kept in the cache dtype).  A block owns one (sequence, kv head, token split) and serves every
// query head of the group, so a code byte is read once per group; a lane owns 8 consecutive channels of one token (K and V of the same
// token: one address pattern), D / 8 lanes share a token.  fp32 dot products, fp32 online softmax kept PER LANE over the tokens the lane
// has seen (no cross-lane traffic in the loop beyond the dot product's butterfly), merged across the lanes of a wave by shuffles and
// across the four waves through LDS in a fixed order; every split writes (acc[D], m, l) to the workspace and a second launch combines the
// splits in ascending order.  No atomics, no flags, no block waits on another: equal inputs give equal bits.
//
// Lengths on the device: msq_kv_mx_append_dev / msq_kv_mx_attn_decode_dev read {packed_len, tail_len} from an int32[4] state
// in device memory instead of taking them as launch arguments, with grids fixed by the capacity, so that a decode step can be captured in a
// HIP graph.  They are further instantiations of the kernels below (template switches DEVPOS / DEV): the host-length forms are unchanged.
//
// Lengths per sequence: msq_kv_mx_append_seq / msq_kv_mx_attn_decode_seq take state = int32[B][4], one row
// {packed_len, tail_len, status, flags} per slot, so the sequences of a batch differ in length and a slot can be emptied and refilled between
// replays of one captured step.  A third template switch (SEQ) beside DEVPOS / DEV: the slot sits on a grid axis of its own in every kernel, so
// a block works for one slot and its state read stays wave-uniform; the host-length and the shared-row forms are unchanged.
#include "msq_kv_packed_common.h"
#include "msq_mx_pack_core.h"

using namespace msq;

namespace {

typedef short v2s_t __attribute__((ext_vector_type(2)));

template <int DT> MSQ_D float ld_any(const void* p, int64_t i) {
    if (DT == 0) return reinterpret_cast<const float*>(p)[i];
    const uint16_t h = reinterpret_cast<const uint16_t*>(p)[i];
    return DT == 1 ? (float)__builtin_bit_cast(_Float16, h) : u2f((uint32_t)h << 16);
}
template <int DT> MSQ_D void st_pair(void* p, int64_t i, float v0, float v1) {      // i even
    if (DT == 0) { *reinterpret_cast<float2*>(reinterpret_cast<float*>(p) + i) = make_float2(v0, v1); return; }
    uint32_t w;
    if (DT == 1) w = (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)v0) | ((uint32_t)__builtin_bit_cast(uint16_t, (_Float16)v1) << 16);
    else w = (uint32_t)__builtin_bit_cast(uint16_t, (__bf16)v0) | ((uint32_t)__builtin_bit_cast(uint16_t, (__bf16)v1) << 16);
    *reinterpret_cast<uint32_t*>(reinterpret_cast<uint16_t*>(p) + i) = w;
}

// One MX block of 32 float32 values -> codes (e4m3: 8 words, element i in byte i; e2m1: 4 words, element i in nibble i) + the scale byte:
// the arithmetic of msq_mx.hip k_mx_pack (activations / weights, flush_fp32_subnorms = 0) on a register array.
template <bool FP4>
MSQ_D void mx_block32(const float (&a)[32], uint32_t (&cw)[FP4 ? 4 : 8], int& sb, int& status) {
    uint32_t mag = 0u;
#pragma unroll
    for (int b = 0; b < 32; ++b) { const uint32_t t = f2u(a[b]) & 0x7FFFFFFFu; mag = t > mag ? t : mag; }
    sb = mx_scale_byte(biased_exp_py(mag), FP4 ? 2 : 8, status);
    const float s_op = u2f((uint32_t)sb << 23);                  // the converts read the exponent field only
    const float bound = __builtin_ldexpf(448.f, sb - 127);       // e4m3 max_norm x scale (exact)
    const uint32_t qb = half_away_quirk_bits(sb - 127 - (FP4 ? 2 : 10));
#pragma unroll
    for (int p = 0; p < 16; ++p) {
        float x0 = sticky_half_away(a[2 * p], qb), x1 = sticky_half_away(a[2 * p + 1], qb);
        if (FP4) {
            uint32_t w = (p & 3) ? cw[p >> 2] : 0u;
            if ((p & 3) == 0) w = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w, x0, x1, s_op, 0);
            else if ((p & 3) == 1) w = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w, x0, x1, s_op, 1);
            else if ((p & 3) == 2) w = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w, x0, x1, s_op, 2);
            else w = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w, x0, x1, s_op, 3);
            cw[p >> 2] = w;
        } else {
            x0 = __builtin_amdgcn_fmed3f(x0, -bound, bound); x1 = __builtin_amdgcn_fmed3f(x1, -bound, bound);   // e4m3 does not saturate
            v2s_t cur = __builtin_bit_cast(v2s_t, (p & 1) ? cw[p >> 1] : 0u);
            if ((p & 1) == 0) cur = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(cur, x0, x1, s_op, false);
            else cur = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(cur, x0, x1, s_op, true);
            cw[p >> 1] = __builtin_bit_cast(uint32_t, cur);
        }
    }
}

// ---- pack, K form: one lane per (b h, token group, channel), channel fastest: 32 strided reads, coalesced across the lanes
// DEVPOS (both pack kernels): the flush of msq_kv_mx_append_dev.  `in` is the tail [B H, T = tail_cap, D]; the position comes from `state`, the
// launch does nothing unless the tail is full and fits, and the status bits go to state[2].
// SEQ (with DEVPOS): the grid is (blocks of ONE slot, B); `total` counts one slot's lanes, blockIdx.y is the slot, `state` is [B][4] and the block
// reads its slot's row: a slot whose tail is full flushes to its own packed_len and raises its own status word, the others return.
template <int DT, bool FP4, bool DEVPOS = false, bool SEQ = false>
__global__ void __launch_bounds__(256)
k_kvp_pack_k(const void* __restrict__ in, uint8_t* __restrict__ codes, uint8_t* __restrict__ scales, int64_t total, int64_t T, int D,
             int64_t S_cap, int64_t pos, int* status_flag, int* state) {
    if (DEVPOS) {
        int p, slot;
        if (SEQ) state += 4 * (int64_t)blockIdx.y;
        if ((SEQ ? append_step_seq(state, S_cap, (int)T, p, slot) : append_step(state, S_cap, (int)T, p, slot)) != 2) return;
        pos = p; status_flag = state + 2;
    }
    const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = t0 < total;                                   // total is even and so is D: a nibble pair is live or dead as one
    const int64_t t = live ? t0 : 0;
    const int64_t ng = T / 32;
    const int d = (int)(t % D);
    const int64_t tg = (t / D) % ng, bh = t / ((int64_t)D * ng) + (SEQ ? (int64_t)blockIdx.y * (total / ((int64_t)D * ng)) : 0);
    float a[32];
#pragma unroll
    for (int i = 0; i < 32; ++i) a[i] = ld_any<DT>(in, (bh * T + tg * 32 + i) * D + d);
    uint32_t cw[FP4 ? 4 : 8];
    int sb, status = 0;
    mx_block32<FP4>(a, cw, sb, status);
    const int64_t row0 = bh * S_cap + pos + tg * 32;
    if (FP4) {
        uint32_t ow[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) ow[j] = (uint32_t)__shfl_xor((int)cw[j & 3], 1, 64);     // the odd neighbour's nibbles
        if (live && !(d & 1)) {
#pragma unroll
            for (int i = 0; i < 32; ++i) {
                const uint32_t lo = (cw[(i >> 3) & 3] >> (4 * (i & 7))) & 0xFu, hi = (ow[i >> 3] >> (4 * (i & 7))) & 0xFu;
                codes[(row0 + i) * (D / 2) + (d >> 1)] = (uint8_t)(lo | (hi << 4));
            }
        }
    } else if (live) {
#pragma unroll
        for (int i = 0; i < 32; ++i) codes[(row0 + i) * D + d] = (uint8_t)((cw[(i >> 2) & (FP4 ? 3 : 7)] >> (8 * (i & 3))) & 0xFFu);
    }
    if (live) scales[(bh * (S_cap / 32) + pos / 32 + tg) * D + d] = (uint8_t)sb;
    if (live && status && status_flag) atomicOr(status_flag, status);
}

// ---- pack, V form: one lane per (b h, token, block of 32 channels): 16-byte reads and stores
template <int DT, bool FP4, bool DEVPOS = false, bool SEQ = false>
__global__ void __launch_bounds__(256)
k_kvp_pack_v(const void* __restrict__ in, uint8_t* __restrict__ codes, uint8_t* __restrict__ scales, int64_t total, int64_t T, int D,
             int64_t S_cap, int64_t pos, int* status_flag, int* state) {
    if (DEVPOS) {
        int p, slot;
        if (SEQ) state += 4 * (int64_t)blockIdx.y;
        if ((SEQ ? append_step_seq(state, S_cap, (int)T, p, slot) : append_step(state, S_cap, (int)T, p, slot)) != 2) return;
        pos = p; status_flag = state + 2;
    }
    int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    if (SEQ) t += (int64_t)blockIdx.y * total;                      // total: the lanes of one slot
    const int nb = D / 32;
    const int blk = (int)(t % nb);
    const int64_t row = t / nb, bh = row / T, tok = row % T;
    float a[32];
    if (DT == 0) {
        const float4* s4 = reinterpret_cast<const float4*>(reinterpret_cast<const float*>(in) + row * D + blk * 32);
#pragma unroll
        for (int k = 0; k < 8; ++k) { const float4 v = s4[k]; a[4 * k] = v.x; a[4 * k + 1] = v.y; a[4 * k + 2] = v.z; a[4 * k + 3] = v.w; }
    } else {
        const uint4* s8 = reinterpret_cast<const uint4*>(reinterpret_cast<const uint16_t*>(in) + row * D + blk * 32);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint4 v = s8[k];
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) { a[8 * k + 2 * j] = half_lo(w[j], DT); a[8 * k + 2 * j + 1] = half_hi(w[j], DT); }
        }
    }
    uint32_t cw[FP4 ? 4 : 8];
    int sb, status = 0;
    mx_block32<FP4>(a, cw, sb, status);
    const int64_t dst = bh * S_cap + pos + tok;
    if (FP4) {
        *reinterpret_cast<uint4*>(codes + dst * (D / 2) + blk * 16) = make_uint4(cw[0], cw[1], cw[2], cw[3]);
    } else {
        uint4* o = reinterpret_cast<uint4*>(codes + dst * D + blk * 32);
        o[0] = make_uint4(cw[0], cw[1], cw[2], cw[3]);
        o[1] = make_uint4(cw[FP4 ? 0 : 4], cw[FP4 ? 1 : 5], cw[FP4 ? 2 : 6], cw[FP4 ? 3 : 7]);
    }
    scales[dst * nb + blk] = (uint8_t)sb;
    if (status && status_flag) atomicOr(status_flag, status);
}

// ---- unpack: one lane per (b h, token, channel pair)
template <int DT, bool FP4>
__global__ void __launch_bounds__(256)
k_kvp_unpack(const uint8_t* __restrict__ codes, const uint8_t* __restrict__ scales, void* __restrict__ out, int64_t total, int64_t T, int D,
             int64_t S_cap, int64_t pos, int along_tokens) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int hd = D / 2;
    const int dp = (int)(t % hd);
    const int64_t tok = (t / hd) % T, bh = t / ((int64_t)hd * T);
    const int64_t src = bh * S_cap + pos + tok;
    v2f_t v;
    if (FP4) v = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4((uint32_t)codes[src * hd + dp], 1.0f, 0);
    else v = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8((uint32_t)*reinterpret_cast<const uint16_t*>(codes + src * D + 2 * dp), 1.0f, false);
    int s0, s1;
    if (along_tokens) {
        const uint8_t* sp = scales + (bh * (S_cap / 32) + (pos + tok) / 32) * D + 2 * dp;
        s0 = sp[0]; s1 = sp[1];
    } else {
        s0 = s1 = scales[src * (D / 32) + (2 * dp) / 32];
    }
    st_pair<DT>(out, (bh * T + tok) * D + 2 * dp, apply_e8m0(v[0], s0), apply_e8m0(v[1], s1));
}

// =====================================================================================================================
// decode attention
// =====================================================================================================================
struct AttnArgs {
    const void* q; const uint8_t* kc; const uint8_t* ks; const uint8_t* vc; const uint8_t* vs; const void* kt; const void* vt;
    const float* bias; float* ws;
    int Hq, G, nsplit, gps, S_packed, tail_len, tail_cap;
    int64_t S_cap;
    float scaling;
    const int* state; int bias_stride;            // the device-length forms (DEV; SEQ: state is [B][4]): lengths from state, bias rows of bias_stride floats
};

// one group of NP tokens per lane: the scores sc[p][g] are in hand; fold them into the lane's running (m, l), rescale acc once, and leave the
// probabilities in sc
template <int NP, int GMAX>
MSQ_D void softmax_fold(float (&sc)[NP][GMAX], float (&m)[GMAX], float (&l)[GMAX], float (&acc)[GMAX][8]) {
#pragma unroll
    for (int g = 0; g < GMAX; ++g) {
        float mn = m[g];
#pragma unroll
        for (int p = 0; p < NP; ++p) mn = __builtin_fmaxf(mn, sc[p][g]);
        const float mm = (mn == neg_inf()) ? 0.f : mn;              // everything masked so far: e^(-inf - 0) = 0, never inf - inf
        const float a = ex(m[g] - mm);
        float ls = l[g] * a;
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[g][j] *= a;
#pragma unroll
        for (int p = 0; p < NP; ++p) { sc[p][g] = ex(sc[p][g] - mm); ls += sc[p][g]; }
        l[g] = ls; m[g] = mn;
    }
}

// DEV: the grid is (max_splits of the capacity, Hkv, B); every block reads the lengths from A.state, derives the plan a host-length launch at
// those lengths gets and returns when its split does not exist, so the live blocks do what that launch's blocks do, bit for bit.
// SEQ (with DEV): A.state is [B][4] and the block reads the row of ITS sequence, so the plan is per slot; the partials of a (sequence, query
// head) are gridDim.x = max_splits apart in the workspace whatever the slot's live splits (rows of different live counts must not overlap).
template <int D, bool FP4, int GMAX, int QDT, bool DEV = false, bool SEQ = false>
__global__ void __launch_bounds__(256)
k_kvp_attn_split(const AttnArgs A) {
    constexpr int LPT = D / 8, TP = 64 / LPT, NP = 32 / TP;          // lanes per token, tokens per pass of a wave, passes per group of 32
    constexpr int CB = FP4 ? 4 : 8;                                   // code bytes of a lane's 8 channels
    __shared__ float red[4][GMAX][D + 2];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int c = lane % LPT, ts = lane / LPT;
    const int split = blockIdx.x, hk = blockIdx.y, b = blockIdx.z;
    const int G = A.G, Hkv = A.Hq / G;
    const int64_t bh = (int64_t)b * Hkv + hk;
    int S_packed = A.S_packed, tail_len = A.tail_len, nsplit = A.nsplit, gps = A.gps;
    if (DEV) {
        if (SEQ) seq_lengths(A.state + 4 * (int64_t)b, A.S_cap, A.tail_cap, S_packed, tail_len);
        else dev_lengths(A.state, A.S_cap, A.tail_cap, S_packed, tail_len);
        const AttnPlan pl = attn_split_plan(S_packed / 32);
        nsplit = pl.nsplit; gps = pl.gps;
        if (split >= nsplit) return;
    }
    const int stot = DEV ? A.bias_stride : S_packed + tail_len;      // floats of a bias row

    float q[GMAX][8];
#pragma unroll
    for (int g = 0; g < GMAX; ++g) {
        uint4 raw = make_uint4(0u, 0u, 0u, 0u);
        if (g < G) raw = *reinterpret_cast<const uint4*>(reinterpret_cast<const uint16_t*>(A.q) + ((int64_t)b * A.Hq + hk * G + g) * D + c * 8);
        const uint32_t w[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) { q[g][2 * j] = half_lo(w[j], QDT); q[g][2 * j + 1] = half_hi(w[j], QDT); }
    }
    float m[GMAX], l[GMAX], acc[GMAX][8];
#pragma unroll
    for (int g = 0; g < GMAX; ++g) {
        m[g] = neg_inf(); l[g] = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[g][j] = 0.f;
    }

    int g0, npk, ntc;
    split_range(split, nsplit, gps, S_packed, tail_len, g0, npk, ntc);

    for (int it = wv; it < npk + ntc; it += 4) {
        float sc[NP][GMAX];
        if (it < npk) {                                               // ---- a packed group
            const int gi = g0 + it;
            const uint8_t* ksp = A.ks + (bh * (A.S_cap / 32) + gi) * D + c * 8;
            const uint2 ksr = *reinterpret_cast<const uint2*>(ksp);
            uint32_t kr[NP][2], vr[NP][2], vsb[NP];
            float bv[NP];
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const int tok = gi * 32 + p * TP + ts;
                const int64_t row = bh * A.S_cap + tok;
                if (FP4) {
                    kr[p][0] = *reinterpret_cast<const uint32_t*>(A.kc + row * (D / 2) + c * CB); kr[p][1] = 0u;
                    vr[p][0] = *reinterpret_cast<const uint32_t*>(A.vc + row * (D / 2) + c * CB); vr[p][1] = 0u;
                } else {
                    const uint2 kk = *reinterpret_cast<const uint2*>(A.kc + row * D + c * CB); kr[p][0] = kk.x; kr[p][1] = kk.y;
                    const uint2 vv = *reinterpret_cast<const uint2*>(A.vc + row * D + c * CB); vr[p][0] = vv.x; vr[p][1] = vv.y;
                }
                vsb[p] = A.vs[row * (D / 32) + c / 4];
                bv[p] = A.bias ? A.bias[(int64_t)b * stot + tok] : 0.f;
            }
            float ksf[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) ksf[j] = e8m0_f32(((j < 4 ? ksr.x : ksr.y) >> (8 * (j & 3))) & 0xFFu);
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                float kf[8];
#pragma unroll
                for (int j = 0; j < 4; ++j) {                         // channel pairs: the K scales differ inside a pair, so scale 1 and an exact multiply
                    v2f_t v;
                    if (FP4) {
                        if (j == 0) v = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(kr[p][0], 1.0f, 0);
                        else if (j == 1) v = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(kr[p][0], 1.0f, 1);
                        else if (j == 2) v = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(kr[p][0], 1.0f, 2);
                        else v = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(kr[p][0], 1.0f, 3);
                    } else {
                        if ((j & 1) == 0) v = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(kr[p][j >> 1], 1.0f, false);
                        else v = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(kr[p][j >> 1], 1.0f, true);
                    }
                    kf[2 * j] = v[0] * ksf[2 * j]; kf[2 * j + 1] = v[1] * ksf[2 * j + 1];
                }
#pragma unroll
                for (int g = 0; g < GMAX; ++g) {
                    float dot = 0.f;
#pragma unroll
                    for (int j = 0; j < 8; ++j) dot = __builtin_fmaf(q[g][j], kf[j], dot);
#pragma unroll
                    for (int o = 1; o < LPT; o <<= 1) dot += __shfl_xor(dot, o, 64);
                    sc[p][g] = __builtin_fmaf(dot, A.scaling, bv[p]);
                }
            }
            softmax_fold<NP, GMAX>(sc, m, l, acc);
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const float vsc = u2f(vsb[p] << 23);                  // a V block lies along head_dim: the pair shares the scale operand
                float vf[8];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    v2f_t v;
                    if (FP4) {
                        if (j == 0) v = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(vr[p][0], vsc, 0);
                        else if (j == 1) v = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(vr[p][0], vsc, 1);
                        else if (j == 2) v = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(vr[p][0], vsc, 2);
                        else v = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(vr[p][0], vsc, 3);
                    } else {
                        if ((j & 1) == 0) v = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(vr[p][j >> 1], vsc, false);
                        else v = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(vr[p][j >> 1], vsc, true);
                    }
                    vf[2 * j] = v[0]; vf[2 * j + 1] = v[1];
                }
#pragma unroll
                for (int g = 0; g < GMAX; ++g)
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[g][j] = __builtin_fmaf(sc[p][g], vf[j], acc[g][j]);
            }
        } else {                                                      // ---- 32 tokens of the tail (cache dtype = the query's)
            const int tc = it - npk;
            uint4 kr[NP], vr[NP];
            float bv[NP];
            bool ok[NP];
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const int j = tc * 32 + p * TP + ts;
                ok[p] = j < tail_len;
                kr[p] = make_uint4(0u, 0u, 0u, 0u); vr[p] = make_uint4(0u, 0u, 0u, 0u); bv[p] = 0.f;
                if (ok[p]) {
                    const int64_t e = (bh * A.tail_cap + j) * D + c * 8;
                    kr[p] = *reinterpret_cast<const uint4*>(reinterpret_cast<const uint16_t*>(A.kt) + e);
                    vr[p] = *reinterpret_cast<const uint4*>(reinterpret_cast<const uint16_t*>(A.vt) + e);
                    if (A.bias) bv[p] = A.bias[(int64_t)b * stot + S_packed + j];
                }
            }
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const uint32_t w[4] = {kr[p].x, kr[p].y, kr[p].z, kr[p].w};
                float kf[8];
#pragma unroll
                for (int j = 0; j < 4; ++j) { kf[2 * j] = half_lo(w[j], QDT); kf[2 * j + 1] = half_hi(w[j], QDT); }
#pragma unroll
                for (int g = 0; g < GMAX; ++g) {
                    float dot = 0.f;
#pragma unroll
                    for (int j = 0; j < 8; ++j) dot = __builtin_fmaf(q[g][j], kf[j], dot);
#pragma unroll
                    for (int o = 1; o < LPT; o <<= 1) dot += __shfl_xor(dot, o, 64);
                    sc[p][g] = ok[p] ? __builtin_fmaf(dot, A.scaling, bv[p]) : neg_inf();
                }
            }
            softmax_fold<NP, GMAX>(sc, m, l, acc);
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const uint32_t w[4] = {vr[p].x, vr[p].y, vr[p].z, vr[p].w};       // zeros where the token does not exist
                float vf[8];
#pragma unroll
                for (int j = 0; j < 4; ++j) { vf[2 * j] = half_lo(w[j], QDT); vf[2 * j + 1] = half_hi(w[j], QDT); }
#pragma unroll
                for (int g = 0; g < GMAX; ++g)
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[g][j] = __builtin_fmaf(sc[p][g], vf[j], acc[g][j]);
            }
        }
    }

    // the TP token subsets of the wave -> lanes 0 .. LPT - 1
#pragma unroll
    for (int o = LPT; o < 64; o <<= 1) {
#pragma unroll
        for (int g = 0; g < GMAX; ++g) {
            const float mo = __shfl_xor(m[g], o, 64), lo = __shfl_xor(l[g], o, 64);
            const float mn = __builtin_fmaxf(m[g], mo);
            const float mm = (mn == neg_inf()) ? 0.f : mn;
            const float a = ex(m[g] - mm), bb = ex(mo - mm);
            l[g] = l[g] * a + lo * bb;
#pragma unroll
            for (int j = 0; j < 8; ++j) { const float ao = __shfl_xor(acc[g][j], o, 64); acc[g][j] = acc[g][j] * a + ao * bb; }
            m[g] = mn;
        }
    }
    if (ts == 0) {
#pragma unroll
        for (int g = 0; g < GMAX; ++g) {
#pragma unroll
            for (int j = 0; j < 8; ++j) red[wv][g][c * 8 + j] = acc[g][j];
            if (c == 0) { red[wv][g][D] = m[g]; red[wv][g][D + 1] = l[g]; }
        }
    }
    __syncthreads();
    // the four waves, in wave order -> the split's partial (acc[D], m, l) of every query head of the group
    for (int idx = threadIdx.x; idx < G * D; idx += 256) {
        const int g = idx / D, d = idx % D;
        float mn = neg_inf();
#pragma unroll
        for (int w = 0; w < 4; ++w) mn = __builtin_fmaxf(mn, red[w][g][D]);
        const float mm = (mn == neg_inf()) ? 0.f : mn;
        float num = 0.f, den = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) { const float f = ex(red[w][g][D] - mm); num += red[w][g][d] * f; den += red[w][g][D + 1] * f; }
        float* o = A.ws + ((((int64_t)b * A.Hq + hk * G + g) * (SEQ ? (int)gridDim.x : nsplit)) + split) * (D + 2);
        o[d] = num;
        if (d == 0) { o[D] = mn; o[D + 1] = den; }
    }
}

// ---- the single-token append of the device-length cache (msq_kv_mx_append_dev), after the flush: one lane per 16 bytes of the token
// SEQ: the grid is (blocks of one slot, B) and `total` one slot's lanes, as in the pack kernels; an idle or full slot takes no token
template <bool SEQ = false>
__global__ void __launch_bounds__(256)
k_kvp_tail_put(const uint4* __restrict__ k_new, const uint4* __restrict__ v_new, uint4* __restrict__ k_tail, uint4* __restrict__ v_tail, int64_t total,
               int dv, int64_t S_cap, int tail_cap, const int* state) {
    int pos, slot;
    if (SEQ) {
        state += 4 * (int64_t)blockIdx.y;
        const int step = append_step_seq(state, S_cap, tail_cap, pos, slot);
        if (step == 0 || step == 3) return;
    } else if (append_step(state, S_cap, tail_cap, pos, slot) == 0) return;
    int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    if (SEQ) t += (int64_t)blockIdx.y * total;
    const int64_t bh = t / dv, dst = (bh * tail_cap + slot) * dv + t % dv;       // k_new / v_new [B H, 1, D], the tail [B H, tail_cap, D]
    k_tail[dst] = k_new[t];
    v_tail[dst] = v_new[t];
}

// ... and the lengths: one lane, a launch of its own behind every kernel that read the old ones
// SEQ: one lane per slot (a per-lane read of the slot's row, plain stores to it): a full slot or one with an invalid row gets
// MSQ_STATUS_OVERFLOW in its OWN status word and keeps its lengths, an idle slot is left alone, the others move.  nslots: B (SEQ only).
template <bool SEQ = false>
__global__ void __launch_bounds__(64)
k_kvp_advance(int* state, int64_t S_cap, int tail_cap, int nslots) {
    if (SEQ) {
        const int b = blockIdx.x * 64 + threadIdx.x;
        if (b >= nslots) return;
        int* row = state + 4 * (int64_t)b;
        if (row[3] & MSQ_KV_SLOT_IDLE) return;
        int pos, slot;
        const int step = append_step<false>(row, S_cap, tail_cap, pos, slot);
        if (step == 0) { row[2] = row[2] | MSQ_STATUS_OVERFLOW; return; }
        if (step == 2) row[0] = pos + tail_cap;
        row[1] = slot + 1;
        return;
    }
    if (threadIdx.x) return;
    int pos, slot;
    const int step = append_step(state, S_cap, tail_cap, pos, slot);
    if (step == 0) { atomicOr(state + 2, MSQ_STATUS_OVERFLOW); return; }
    if (step == 2) state[0] = pos + tail_cap;
    state[1] = slot + 1;
}

// the two launches of a decode call (DEV: the device-length form, grid_x = the capacity's max_splits; SEQ: a state row per sequence)
template <bool DEV, bool SEQ = false>
int attn_launch(const AttnArgs& A, int q_dtype, void* out, int out_dtype, int64_t B, int Hkv, int D, bool f4, int grid_x, hipStream_t st, const char* fail) {
    const dim3 grid((unsigned)grid_x, (unsigned)Hkv, (unsigned)B), blk(256);
    const int gm = A.G <= 1 ? 1 : (A.G <= 2 ? 2 : (A.G <= 4 ? 4 : 8));
#define MSQ_KVA(DV, F4, GM, QD) hipLaunchKernelGGL((k_kvp_attn_split<DV, F4, GM, QD, DEV, SEQ>), grid, blk, 0, st, A)
#define MSQ_KVA_Q(DV, F4, GM) do { if (q_dtype == 1) MSQ_KVA(DV, F4, GM, 1); else MSQ_KVA(DV, F4, GM, 2); } while (0)
#define MSQ_KVA_G(DV, F4) do { if (gm == 1) MSQ_KVA_Q(DV, F4, 1); else if (gm == 2) MSQ_KVA_Q(DV, F4, 2); else if (gm == 4) MSQ_KVA_Q(DV, F4, 4); else MSQ_KVA_Q(DV, F4, 8); } while (0)
#define MSQ_KVA_F(DV) do { if (f4) MSQ_KVA_G(DV, true); else MSQ_KVA_G(DV, false); } while (0)
    if (D == 64) MSQ_KVA_F(64); else MSQ_KVA_F(128);
#undef MSQ_KVA_F
#undef MSQ_KVA_G
#undef MSQ_KVA_Q
#undef MSQ_KVA
    if (hipGetLastError() != hipSuccess) return kvp_fail(MSQ_ERR_LAUNCH, fail);
    const dim3 cgrid = SEQ ? dim3((unsigned)A.Hq, (unsigned)B) : dim3((unsigned)(B * A.Hq));
#define MSQ_KVC1(DV, OD) hipLaunchKernelGGL((k_kvp_attn_combine<DV, OD, DEV, SEQ>), cgrid, dim3(DV), 0, st, (const float*)A.ws, out, SEQ ? grid_x : A.nsplit, A.state, A.S_cap)
#define MSQ_KVC(DV) do { if (out_dtype == 0) MSQ_KVC1(DV, 0); else if (out_dtype == 1) MSQ_KVC1(DV, 1); else MSQ_KVC1(DV, 2); } while (0)
    if (D == 64) MSQ_KVC(64); else MSQ_KVC(128);
#undef MSQ_KVC
#undef MSQ_KVC1
    return hipGetLastError() == hipSuccess ? MSQ_OK : kvp_fail(MSQ_ERR_LAUNCH, fail);
}

// msq_kv_mx_attn_decode_dev (SEQ = false: state int32[4]) and msq_kv_mx_attn_decode_seq (SEQ = true: state int32[B][4]): the same checks, the
// same grid of the split kernel
template <bool SEQ>
int attn_decode_state(const char* who, const void* q, int q_dtype, const void* k_codes, const void* k_scales, const void* v_codes, const void* v_scales,
                      int64_t S_cap, const void* k_tail, const void* v_tail, int64_t tail_cap, const int* state, const float* bias,
                      int64_t bias_stride, void* out, int out_dtype, int64_t B, int Hq, int Hkv, int D, int elem_fmt, float scaling,
                      void* workspace, int64_t workspace_bytes, void* stream) {
    int ms = 0;
    int64_t need = 0;
    const int rc = msq_kv_mx_attn_plan_cap(B, Hq, Hkv, D, S_cap, tail_cap, &ms, &need);
    if (rc != MSQ_OK) return rc;
    AttnArgs A;
    set_attn_buffers(A, q, k_codes, k_scales, v_codes, v_scales, k_tail, v_tail, bias, workspace);
    // the tail is read at whatever length the state holds: a null one is refused with q, out and the workspace
    const char* own = !state ? "null state"
                    : (bias && (bias_stride < S_cap + tail_cap || bias_stride > 0x7FFFFFFF)) ? "bias_stride must be at least S_cap + tail_cap"
                    : (!k_tail || !v_tail) ? "null buffer" : nullptr;
    const int bad = check_attn_common(who, A, out, state, elem_fmt, q_dtype, out_dtype, own, S_cap != 0, false, workspace_bytes, need,
                                      "workspace too small (msq_kv_mx_attn_plan_cap)");
    if (bad != MSQ_OK) return bad;
    A.Hq = Hq; A.G = Hq / Hkv; A.nsplit = 0; A.gps = 0; A.S_packed = 0; A.tail_len = 0; A.tail_cap = (int)tail_cap;
    A.S_cap = S_cap; A.scaling = scaling; A.state = state; A.bias_stride = (int)bias_stride;
    char fail[96];
    snprintf(fail, sizeof(fail), "%s: launch failed", who);
    return attn_launch<true, SEQ>(A, q_dtype, out, out_dtype, B, Hkv, D, elem_fmt == MSQ_FMT_FP4_E2M1, ms, (hipStream_t)stream, fail);
}

// msq_kv_mx_append_dev (SEQ = false) and msq_kv_mx_append_seq (SEQ = true: the slot is the grids' y axis, the advance has one lane per slot)
template <bool SEQ>
int append_state(const char* who, const void* k_new, const void* v_new, int dtype, void* k_codes, void* k_scales, void* v_codes, void* v_scales,
                 int64_t S_cap, void* k_tail, void* v_tail, int64_t tail_cap, int* state, int64_t B, int64_t H, int64_t D, int elem_fmt, void* stream) {
    if (B <= 0 || H <= 0) return kvp_fail_in(MSQ_ERR_BAD_ARG, who, "sizes must be positive");
    if (elem_fmt != MSQ_FMT_FP8_E4M3 && elem_fmt != MSQ_FMT_FP4_E2M1) return kvp_fail_in(MSQ_ERR_UNSUPPORTED, who, "elem_fmt must be fp8_e4m3 or fp4_e2m1");
    if (dtype != 1 && dtype != 2) return kvp_fail_in(MSQ_ERR_UNSUPPORTED, who, "the cache dtype must be f16 (1) or bf16 (2)");
    if (D <= 0 || D % 32 || D > 256) return kvp_fail_in(MSQ_ERR_UNSUPPORTED, who, "head_dim must be a multiple of 32, at most 256");
    if (S_cap <= 0 || S_cap % 32 || S_cap > (int64_t)1 << 30) return kvp_fail_in(MSQ_ERR_BAD_ARG, who, "S_cap must be a positive multiple of 32, at most 2^30");
    if (tail_cap <= 0 || tail_cap % 32 || tail_cap > (int64_t)1 << 20) return kvp_fail_in(MSQ_ERR_BAD_ARG, who, "tail_cap must be a positive multiple of 32");
    if (SEQ && B > 65535) return kvp_fail_in(MSQ_ERR_UNSUPPORTED, who, "at most 65535 slots (the slot is a grid axis)");
    if (!state) return kvp_fail_in(MSQ_ERR_BAD_ARG, who, "null state");
    if (!k_new || !v_new || !k_codes || !k_scales || !v_codes || !v_scales || !k_tail || !v_tail) return kvp_fail_in(MSQ_ERR_BAD_ARG, who, "null buffer");
    if ((((uintptr_t)k_new | (uintptr_t)v_new | (uintptr_t)k_codes | (uintptr_t)v_codes | (uintptr_t)k_tail | (uintptr_t)v_tail | (uintptr_t)state) & 15) != 0)
        return kvp_fail_in(MSQ_ERR_BAD_ARG, who, "buffers must be 16-byte aligned");
    // SEQ: the totals count ONE slot's lanes and the slot is blockIdx.y
    const int64_t nb = SEQ ? 1 : B, ny = SEQ ? B : 1;
    const int64_t tot_k = nb * H * (tail_cap / 32) * D, tot_v = nb * H * tail_cap * (D / 32), tot_p = nb * H * (D / 8);
    if ((tot_k + 255) / 256 > 0x7FFFFFFF || (tot_v + 255) / 256 > 0x7FFFFFFF) return kvp_fail_in(MSQ_ERR_UNSUPPORTED, who, "tensor too large for one launch");
    hipStream_t st = (hipStream_t)stream;
    const bool f4 = elem_fmt == MSQ_FMT_FP4_E2M1;
    const dim3 blk(256), gk((unsigned)((tot_k + 255) / 256), (unsigned)ny), gv((unsigned)((tot_v + 255) / 256), (unsigned)ny), gp((unsigned)((tot_p + 255) / 256), (unsigned)ny);
    char fail[96];
    snprintf(fail, sizeof(fail), "%s: launch failed", who);
    // four launches, every grid a function of (B, H, D, tail_cap) alone: the flush (K form, V form: no-ops unless the tail is full and fits), the
    // token into its slot, and the one thread (SEQ: one lane per slot) that moves the lengths once every reader of the old ones is done
#define MSQ_KVF(K, DTV, F4, G, TAIL, C, SC, TOT) hipLaunchKernelGGL((K<DTV, F4, true, SEQ>), G, blk, 0, st, (const void*)TAIL, (uint8_t*)C, (uint8_t*)SC, TOT, tail_cap, (int)D, S_cap, (int64_t)0, (int*)nullptr, state)
#define MSQ_KVF_DT(K, F4, G, TAIL, C, SC, TOT) do { if (dtype == 1) MSQ_KVF(K, 1, F4, G, TAIL, C, SC, TOT); else MSQ_KVF(K, 2, F4, G, TAIL, C, SC, TOT); } while (0)
    if (f4) { MSQ_KVF_DT(k_kvp_pack_k, true, gk, k_tail, k_codes, k_scales, tot_k); MSQ_KVF_DT(k_kvp_pack_v, true, gv, v_tail, v_codes, v_scales, tot_v); }
    else { MSQ_KVF_DT(k_kvp_pack_k, false, gk, k_tail, k_codes, k_scales, tot_k); MSQ_KVF_DT(k_kvp_pack_v, false, gv, v_tail, v_codes, v_scales, tot_v); }
#undef MSQ_KVF_DT
#undef MSQ_KVF
    if (hipGetLastError() != hipSuccess) return kvp_fail(MSQ_ERR_LAUNCH, fail);
    hipLaunchKernelGGL(k_kvp_tail_put<SEQ>, gp, blk, 0, st, (const uint4*)k_new, (const uint4*)v_new, (uint4*)k_tail, (uint4*)v_tail, tot_p, (int)(D / 8), S_cap,
                       (int)tail_cap, (const int*)state);
    hipLaunchKernelGGL(k_kvp_advance<SEQ>, dim3(SEQ ? (unsigned)((B + 63) / 64) : 1u), dim3(64), 0, st, state, S_cap, (int)tail_cap, (int)B);
    return hipGetLastError() == hipSuccess ? MSQ_OK : kvp_fail(MSQ_ERR_LAUNCH, fail);
}

}  // namespace

extern "C" {

int msq_kv_mx_pack(const void* in, int dtype, void* codes, void* scales, int64_t B, int64_t H, int64_t T, int64_t D, int64_t S_cap,
                   int64_t pos, int elem_fmt, int along_tokens, int* status_flag, void* stream) {
    if (B < 0 || H < 0 || T < 0) return kvp_fail(MSQ_ERR_BAD_ARG, "msq_kv_mx_pack: negative size");
    if (elem_fmt != MSQ_FMT_FP8_E4M3 && elem_fmt != MSQ_FMT_FP4_E2M1) return kvp_fail(MSQ_ERR_UNSUPPORTED, "msq_kv_mx_pack: elem_fmt must be fp8_e4m3 or fp4_e2m1");
    if (dtype < 0 || dtype > 2) return kvp_fail(MSQ_ERR_UNSUPPORTED, "msq_kv_mx_pack: dtype must be 0 (f32), 1 (f16) or 2 (bf16)");
    if (D <= 0 || D % 32 || D > 256) return kvp_fail(MSQ_ERR_UNSUPPORTED, "msq_kv_mx_pack: head_dim must be a multiple of 32, at most 256");
    if (S_cap <= 0 || S_cap % 32) return kvp_fail(MSQ_ERR_BAD_ARG, "msq_kv_mx_pack: S_cap must be a positive multiple of 32");
    if (T % 32) return kvp_fail(MSQ_ERR_BAD_ARG, "msq_kv_mx_pack: T must be a multiple of 32");
    if (pos < 0 || pos % 32) return kvp_fail(MSQ_ERR_BAD_ARG, "msq_kv_mx_pack: pos must be a multiple of 32");
    if (pos + T > S_cap) return kvp_fail(MSQ_ERR_BAD_ARG, "msq_kv_mx_pack: pos + T exceeds S_cap");
    if (B * H * T == 0) return MSQ_OK;
    if (!in || !codes || !scales) return kvp_fail(MSQ_ERR_BAD_ARG, "msq_kv_mx_pack: null buffer");
    if ((((uintptr_t)in | (uintptr_t)codes) & 15) != 0) return kvp_fail(MSQ_ERR_BAD_ARG, "msq_kv_mx_pack: buffers must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const bool f4 = elem_fmt == MSQ_FMT_FP4_E2M1;
    const int64_t total = along_tokens ? B * H * (T / 32) * D : B * H * T * (D / 32);
    if ((total + 255) / 256 > 0x7FFFFFFF) return kvp_fail(MSQ_ERR_UNSUPPORTED, "msq_kv_mx_pack: tensor too large for one launch");
    const dim3 grid((unsigned)((total + 255) / 256)), blk(256);
#define MSQ_KVP(K, DTV, F4) hipLaunchKernelGGL((K<DTV, F4>), grid, blk, 0, st, in, (uint8_t*)codes, (uint8_t*)scales, total, T, (int)D, S_cap, pos, status_flag, (int*)nullptr)
#define MSQ_KVP_DT(K, F4) do { if (dtype == 0) MSQ_KVP(K, 0, F4); else if (dtype == 1) MSQ_KVP(K, 1, F4); else MSQ_KVP(K, 2, F4); } while (0)
    if (along_tokens) { if (f4) MSQ_KVP_DT(k_kvp_pack_k, true); else MSQ_KVP_DT(k_kvp_pack_k, false); }
    else { if (f4) MSQ_KVP_DT(k_kvp_pack_v, true); else MSQ_KVP_DT(k_kvp_pack_v, false); }
#undef MSQ_KVP_DT
#undef MSQ_KVP
    return hipGetLastError() == hipSuccess ? MSQ_OK : kvp_fail(MSQ_ERR_LAUNCH, "msq_kv_mx_pack: launch failed");
}

int msq_kv_mx_unpack(const void* codes, const void* scales, void* out, int dtype, int64_t B, int64_t H, int64_t D, int64_t S_cap,
                     int64_t pos, int64_t T, int elem_fmt, int along_tokens, void* stream) {
    if (B < 0 || H < 0 || T < 0) return kvp_fail(MSQ_ERR_BAD_ARG, "msq_kv_mx_unpack: negative size");
    if (elem_fmt != MSQ_FMT_FP8_E4M3 && elem_fmt != MSQ_FMT_FP4_E2M1) return kvp_fail(MSQ_ERR_UNSUPPORTED, "msq_kv_mx_unpack: elem_fmt must be fp8_e4m3 or fp4_e2m1");
    if (dtype < 0 || dtype > 2) return kvp_fail(MSQ_ERR_UNSUPPORTED, "msq_kv_mx_unpack: dtype must be 0 (f32), 1 (f16) or 2 (bf16)");
    if (D <= 0 || D % 32 || D > 256) return kvp_fail(MSQ_ERR_UNSUPPORTED, "msq_kv_mx_unpack: head_dim must be a multiple of 32, at most 256");
    if (S_cap <= 0 || S_cap % 32) return kvp_fail(MSQ_ERR_BAD_ARG, "msq_kv_mx_unpack: S_cap must be a positive multiple of 32");
    if (pos < 0 || pos + T > S_cap) return kvp_fail(MSQ_ERR_BAD_ARG, "msq_kv_mx_unpack: pos + T exceeds S_cap");
    if (B * H * T == 0) return MSQ_OK;
    if (!codes || !scales || !out) return kvp_fail(MSQ_ERR_BAD_ARG, "msq_kv_mx_unpack: null buffer");
    if ((((uintptr_t)out | (uintptr_t)codes) & 15) != 0) return kvp_fail(MSQ_ERR_BAD_ARG, "msq_kv_mx_unpack: buffers must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const bool f4 = elem_fmt == MSQ_FMT_FP4_E2M1;
    const int64_t total = B * H * T * (D / 2);
    if ((total + 255) / 256 > 0x7FFFFFFF) return kvp_fail(MSQ_ERR_UNSUPPORTED, "msq_kv_mx_unpack: tensor too large for one launch");
    const dim3 grid((unsigned)((total + 255) / 256)), blk(256);
#define MSQ_KVU(DTV, F4) hipLaunchKernelGGL((k_kvp_unpack<DTV, F4>), grid, blk, 0, st, (const uint8_t*)codes, (const uint8_t*)scales, out, total, T, (int)D, S_cap, pos, along_tokens ? 1 : 0)
#define MSQ_KVU_DT(F4) do { if (dtype == 0) MSQ_KVU(0, F4); else if (dtype == 1) MSQ_KVU(1, F4); else MSQ_KVU(2, F4); } while (0)
    if (f4) MSQ_KVU_DT(true); else MSQ_KVU_DT(false);
#undef MSQ_KVU_DT
#undef MSQ_KVU
    return hipGetLastError() == hipSuccess ? MSQ_OK : kvp_fail(MSQ_ERR_LAUNCH, "msq_kv_mx_unpack: launch failed");
}

int msq_kv_mx_attn_plan(int64_t B, int Hq, int Hkv, int D, int64_t S_packed, int64_t tail_len, int* n_splits, int* split_tokens,
                        int64_t* workspace_bytes) {
    AttnPlan p;
    const int rc = attn_plan(B, Hq, Hkv, D, S_packed, tail_len, &p);
    if (rc != MSQ_OK) return rc;
    if (n_splits) *n_splits = p.nsplit;
    if (split_tokens) *split_tokens = p.gps * 32;
    if (workspace_bytes) *workspace_bytes = B * Hq * (int64_t)p.nsplit * (D + 2) * (int64_t)sizeof(float);
    return MSQ_OK;
}

int64_t msq_kv_mx_attn_workspace_bytes(int64_t B, int Hq, int Hkv, int D, int64_t S_packed, int64_t tail_len) {
    int64_t bytes = 0;
    const int rc = msq_kv_mx_attn_plan(B, Hq, Hkv, D, S_packed, tail_len, nullptr, nullptr, &bytes);
    return rc != MSQ_OK ? (int64_t)rc : bytes;
}

int msq_kv_mx_attn_decode(const void* q, int q_dtype, const void* k_codes, const void* k_scales, const void* v_codes, const void* v_scales,
                          int64_t S_packed, int64_t S_cap, const void* k_tail, const void* v_tail, int64_t tail_len, int64_t tail_cap,
                          const float* bias, void* out, int out_dtype, int64_t B, int Hq, int Hkv, int D, int elem_fmt, float scaling,
                          void* workspace, int64_t workspace_bytes, void* stream) {
    AttnPlan p;
    const int rc = attn_plan(B, Hq, Hkv, D, S_packed, tail_len, &p);
    if (rc != MSQ_OK) return rc;
    AttnArgs A;
    set_attn_buffers(A, q, k_codes, k_scales, v_codes, v_scales, k_tail, v_tail, bias, workspace);
    const char* own = (S_cap < 0 || S_cap % 32 || S_packed > S_cap) ? "S_packed exceeds S_cap (a multiple of 32)"
                    : tail_len > tail_cap ? "tail_len exceeds tail_cap" : nullptr;
    const int bad = check_attn_common("msq_kv_mx_attn_decode", A, out, nullptr, elem_fmt, q_dtype, out_dtype, own, S_packed != 0, tail_len != 0, workspace_bytes,
                                      B * Hq * (int64_t)p.nsplit * (D + 2) * (int64_t)sizeof(float), "workspace too small (msq_kv_mx_attn_workspace_bytes)");
    if (bad != MSQ_OK) return bad;
    A.Hq = Hq; A.G = Hq / Hkv; A.nsplit = p.nsplit; A.gps = p.gps; A.S_packed = (int)S_packed; A.tail_len = (int)tail_len; A.tail_cap = (int)tail_cap;
    A.S_cap = S_cap; A.scaling = scaling; A.state = nullptr; A.bias_stride = 0;
    return attn_launch<false>(A, q_dtype, out, out_dtype, B, Hkv, D, elem_fmt == MSQ_FMT_FP4_E2M1, p.nsplit, (hipStream_t)stream, "msq_kv_mx_attn_decode: launch failed");
}

int msq_kv_mx_attn_plan_cap(int64_t B, int Hq, int Hkv, int D, int64_t S_cap, int64_t tail_cap, int* max_splits, int64_t* workspace_bytes) {
    AttnPlan p;
    const int rc = attn_plan(B, Hq, Hkv, D, 0, 1, &p);           // the checks of the sizes that do not depend on a length
    if (rc != MSQ_OK) return rc;
    if (S_cap < 0 || S_cap % 32 || S_cap > (int64_t)1 << 30) return kvp_fail(MSQ_ERR_BAD_ARG, "msq_kv_mx_attn_plan_cap: S_cap must be a multiple of 32, at most 2^30");
    if (tail_cap <= 0 || tail_cap % 32 || tail_cap > (int64_t)1 << 20) return kvp_fail(MSQ_ERR_BAD_ARG, "msq_kv_mx_attn_plan_cap: tail_cap must be a positive multiple of 32");
    // n_splits is not monotone in the length (above 8192 tokens a longer cache may take fewer, larger splits), so this is the maximum over
    // every length the planes can hold; 64 is the rule's ceiling, reached at 8192 tokens at the latest
    int ms = 1;
    for (int64_t ng = 1; ng <= S_cap / 32 && ms < 64; ++ng) { const int n = attn_split_plan(ng).nsplit; ms = n > ms ? n : ms; }
    if (max_splits) *max_splits = ms;
    if (workspace_bytes) *workspace_bytes = B * Hq * (int64_t)ms * (D + 2) * (int64_t)sizeof(float);
    return MSQ_OK;
}

int msq_kv_mx_attn_decode_dev(const void* q, int q_dtype, const void* k_codes, const void* k_scales, const void* v_codes, const void* v_scales,
                              int64_t S_cap, const void* k_tail, const void* v_tail, int64_t tail_cap, const int* state, const float* bias,
                              int64_t bias_stride, void* out, int out_dtype, int64_t B, int Hq, int Hkv, int D, int elem_fmt, float scaling,
                              void* workspace, int64_t workspace_bytes, void* stream) {
    return attn_decode_state<false>("msq_kv_mx_attn_decode_dev", q, q_dtype, k_codes, k_scales, v_codes, v_scales, S_cap, k_tail, v_tail, tail_cap, state, bias,
                                    bias_stride, out, out_dtype, B, Hq, Hkv, D, elem_fmt, scaling, workspace, workspace_bytes, stream);
}

int msq_kv_mx_append_dev(const void* k_new, const void* v_new, int dtype, void* k_codes, void* k_scales, void* v_codes, void* v_scales,
                         int64_t S_cap, void* k_tail, void* v_tail, int64_t tail_cap, int* state, int64_t B, int64_t H, int64_t D, int elem_fmt,
                         void* stream) {
    return append_state<false>("msq_kv_mx_append_dev", k_new, v_new, dtype, k_codes, k_scales, v_codes, v_scales, S_cap, k_tail, v_tail, tail_cap, state, B, H, D,
                               elem_fmt, stream);
}

int msq_kv_mx_attn_decode_seq(const void* q, int q_dtype, const void* k_codes, const void* k_scales, const void* v_codes, const void* v_scales,
                              int64_t S_cap, const void* k_tail, const void* v_tail, int64_t tail_cap, const int* state, const float* bias,
                              int64_t bias_stride, void* out, int out_dtype, int64_t B, int Hq, int Hkv, int D, int elem_fmt, float scaling,
                              void* workspace, int64_t workspace_bytes, void* stream) {
    return attn_decode_state<true>("msq_kv_mx_attn_decode_seq", q, q_dtype, k_codes, k_scales, v_codes, v_scales, S_cap, k_tail, v_tail, tail_cap, state, bias,
                                   bias_stride, out, out_dtype, B, Hq, Hkv, D, elem_fmt, scaling, workspace, workspace_bytes, stream);
}

int msq_kv_mx_append_seq(const void* k_new, const void* v_new, int dtype, void* k_codes, void* k_scales, void* v_codes, void* v_scales,
                         int64_t S_cap, void* k_tail, void* v_tail, int64_t tail_cap, int* state, int64_t B, int64_t H, int64_t D, int elem_fmt,
                         void* stream) {
    return append_state<true>("msq_kv_mx_append_seq", k_new, v_new, dtype, k_codes, k_scales, v_codes, v_scales, S_cap, k_tail, v_tail, tail_cap, state, B, H, D,
                              elem_fmt, stream);
}

}  // extern "C"
