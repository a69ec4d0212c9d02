// msq_kv_packed_multi.hip -- causal attention of 1 .. 32 query tokens over the PACKED MX KV cache: the MFMA form of
// msq_kv_packed.hip's single-token kernel.  The planes, the tail and the token splits are that file's; nothing here writes the cache.
//
// The T query tokens are the LAST T tokens the cache holds.  The T * G (token, head of the group) pairs of one kv head are the ROWS; a block
// owns (sequence, kv head, token split, row tile of at most 64 rows), its four waves take every fourth group of 32 tokens, so a code byte is
// fetched once per row tile.  Per group of 32 tokens a wave computes, with v_mfma_f32_16x16x32_bf16 (lane l: c = l & 15, h = l >> 4):
//   S^T = K Q^T   A = K: a lane's 8 consecutive code bytes of token c are its fragment (channels 8h .. 8h + 7 of a k step of 32), decoded
//                 to bf16 WITH the channel's E8M0 scale (exact: at most 4 significant bits, bf16 has float32's exponent range);
//                 B = Q^T from an LDS image (a bf16 q as it is, an fp16 q split exactly into hi + lo bf16: two MFMAs).
//                 C: lane (c, h) holds tokens 4h .. 4h + 3 of both 16-token halves for query row c -- 8 scores of ONE row per lane.
//   softmax       fp32, online, per row: the row sits on the 4 lanes c, c + 16, c + 32, c + 48 (two shuffles for the maximum); the -inf guards of
//                 msq_kv_packed.hip's softmax_fold.  P = hi + lo bf16 (16 significant bits).
//   O^T = V^T P^T the C registers of S^T are already the B fragment of P^T in the token order k = 8h + j -> token 4h + j (j < 4), 16 + 4h + j - 4;
//                 A = V^T in the same order: V is decoded to bf16 with its scale (exact) into a wave-private LDS tile [token][D] and read back
//                 transposed (ds_read_b64_tr_b16: lanes 16h .. 16h + 15 take tokens 4h .. 4h + 3 of 16 channels).  C: lane (c, h) holds channels
//                 4h .. 4h + 3 of every 16 for query row c: the running maximum of a row and its accumulators share a lane.
// Tail tokens are in the cache dtype: bf16 goes straight in; fp16 uses the _f16 form of the same MFMA (q as it is, P = hi + lo fp16).
// The waves merge through LDS in wave order, every split writes (acc[D], m, l) per row to the workspace, a second launch combines the splits
// in ascending order.  No atomics, no flags, no block waits on another: equal inputs give equal bits, and a row's bits do not depend on the
// rows it is computed with.
#include "msq_kv_packed_common.h"

using namespace msq;

namespace {

typedef float v4f_t __attribute__((ext_vector_type(4)));
typedef short v4s_t __attribute__((ext_vector_type(4)));
typedef __bf16 v8bf_t __attribute__((ext_vector_type(8)));
typedef _Float16 v8h_t __attribute__((ext_vector_type(8)));

// two float32 values that ARE bf16 values (low 16 bits zero) -> one packed word
MSQ_D uint32_t pk_top(float lo, float hi) { return (f2u(lo) >> 16) | (f2u(hi) & 0xFFFF0000u); }
MSQ_D uint32_t pk_bf16(float lo, float hi) {
    return (uint32_t)__builtin_bit_cast(uint16_t, (__bf16)lo) | ((uint32_t)__builtin_bit_cast(uint16_t, (__bf16)hi) << 16);
}
MSQ_D uint32_t pk_f16(float lo, float hi) {
    return (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)lo) | ((uint32_t)__builtin_bit_cast(uint16_t, (_Float16)hi) << 16);
}

template <bool F16> MSQ_D v4f_t mma(const uint4 a, const uint4 b, const v4f_t c) {
    if (F16) return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(v8h_t, a), __builtin_bit_cast(v8h_t, b), c, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(v8bf_t, a), __builtin_bit_cast(v8bf_t, b), c, 0, 0, 0);
}

// LDS traffic inside ONE wave (the V tile is wave-private): the stores are done and visible before the transposed reads, the reads are done
// before the next group's stores.  DS operations of a wave complete in order; this keeps the compiler from moving them across.
MSQ_D void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

struct MultiArgs {
    const void* q; const uint8_t* kc; const uint8_t* ks; const uint8_t* vc; const uint8_t* vs; const void* kt; const void* vt;
    const float* bias; float* ws;
    int Hq, G, T, nsplit, gps, S_packed, tail_len, tail_cap, ntiles, causal;
    int64_t S_cap, bias_bstride, bias_tstride;
    float scaling;
};

// scores of one group of 32 tokens (S[n][s]: row tile n, token half s, C layout) -> online softmax -> O^T += V^T P^T from the wave's V tile.
// pos0: the absolute position of the group's first token; lim[n]: the last position row n * 16 + c may see (-1: none).
template <bool F16, int NR, int D>
MSQ_D void fold_group(v4f_t (&S)[NR][2], float (&m)[NR], float (&l)[NR], v4f_t (&O)[NR][D / 16], const int (&lim)[NR],
                      const float* const (&brow)[NR], bool has_bias, bool bias_per_row, int len, int pos0, float scaling,
                      const unsigned char* vtile, int vstr, int lane) {
    const int c = lane & 15, h = lane >> 4;
    float bv[2][4];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int pos = pos0 + s * 16 + 4 * h + r;
            bv[s][r] = (has_bias && !bias_per_row && pos < len) ? brow[0][pos] : 0.f;
        }
    uint4 ph[NR], pl[NR];
#pragma unroll
    for (int n = 0; n < NR; ++n) {
        float sc[8];
        float mx = neg_inf();
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int pos = pos0 + s * 16 + 4 * h + r;
                const bool see = pos <= lim[n];
                float bb = bv[s][r];
                if (has_bias && bias_per_row) bb = see ? brow[n][pos] : 0.f;
                const float x = see ? __builtin_fmaf(S[n][s][r], scaling, bb) : neg_inf();
                sc[4 * s + r] = x;
                mx = __builtin_fmaxf(mx, x);
            }
        mx = __builtin_fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = __builtin_fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float mn = __builtin_fmaxf(m[n], mx);
        const float mm = (mn == neg_inf()) ? 0.f : mn;                // everything masked so far: e^(-inf - 0) = 0, never inf - inf
        const float a = ex(m[n] - mm);
        float ls = l[n] * a;
#pragma unroll
        for (int dc = 0; dc < D / 16; ++dc) O[n][dc] *= a;
        float hi[8], lo[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float p = ex(sc[j] - mm);
            ls += p;
            hi[j] = F16 ? (float)(_Float16)p : (float)(__bf16)p;
            lo[j] = p - hi[j];                                        // exact
        }
        l[n] = ls; m[n] = mn;
        if (F16) {
            ph[n] = make_uint4(pk_f16(hi[0], hi[1]), pk_f16(hi[2], hi[3]), pk_f16(hi[4], hi[5]), pk_f16(hi[6], hi[7]));
            pl[n] = make_uint4(pk_f16(lo[0], lo[1]), pk_f16(lo[2], lo[3]), pk_f16(lo[4], lo[5]), pk_f16(lo[6], lo[7]));
        } else {
            ph[n] = make_uint4(pk_top(hi[0], hi[1]), pk_top(hi[2], hi[3]), pk_top(hi[4], hi[5]), pk_top(hi[6], hi[7]));
            pl[n] = make_uint4(pk_bf16(lo[0], lo[1]), pk_bf16(lo[2], lo[3]), pk_bf16(lo[4], lo[5]), pk_bf16(lo[6], lo[7]));
        }
    }
    // lane 4q + p of a 16-lane group gives the address of token row q, columns 4p .. 4p + 3 of the block; lane i receives column i
    const unsigned char* va = vtile + (4 * h + (c >> 2)) * vstr + (c & 3) * 8;
#pragma unroll
    for (int dc = 0; dc < D / 16; ++dc) {
        const v4s_t a0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s_t*)(va + dc * 32));
        const v4s_t a1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s_t*)(va + dc * 32 + 16 * vstr));
        const uint2 w0 = __builtin_bit_cast(uint2, a0), w1 = __builtin_bit_cast(uint2, a1);
        const uint4 af = make_uint4(w0.x, w0.y, w1.x, w1.y);
#pragma unroll
        for (int n = 0; n < NR; ++n) {
            O[n][dc] = mma<F16>(af, ph[n], O[n][dc]);
            O[n][dc] = mma<F16>(af, pl[n], O[n][dc]);
        }
    }
}

// grid (n_splits, Hkv * ntiles, B).  NR: 16-row tiles of a block's row tile (1, 2 or 4)
template <int D, bool FP4, int QDT, int NR>
__global__ void __launch_bounds__(256)
k_kvp_attn_multi_split(const MultiArgs A) {
    constexpr bool QH = QDT == 1;                                     // fp16: q images hi, lo (bf16) and the fp16 values (for the tail)
    constexpr int KS = D / 32, DC = D / 16, ROWS = NR * 16;
    constexpr int QSTR = D * 2 + 16, VSTR = D * 2 + 32;               // bytes of a row of a q image / of the V tile (bank spread, 16-byte aligned)
    constexpr int NQ = QH ? 3 : 1;
    constexpr int QIMG = ROWS * QSTR, VTILE = 32 * VSTR;
    constexpr int RSTR = D + 4;                                       // floats of a row of the merge image: acc[D], m, l
    constexpr int LOOP_BYTES = NQ * QIMG + 4 * VTILE, RED_BYTES = 4 * ROWS * RSTR * 4;
    constexpr int LPT = D / 8, TP = 64 / LPT, NP = 32 / TP;           // the V tile's load pattern: lanes per token, tokens per pass, passes
    __shared__ __attribute__((aligned(16))) unsigned char smem[LOOP_BYTES > RED_BYTES ? LOOP_BYTES : RED_BYTES];

    // the split's range (split_range below).  Declared first on purpose: where these three sit among the locals decides the order in which the
    // compiler initialises m and l of the one-tile kernels, and here their instructions stay what they were
    int g0, npk, ntc;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int c = lane & 15, h = lane >> 4;
    const int split = blockIdx.x, hk = blockIdx.y / A.ntiles, tile = blockIdx.y % A.ntiles, b = blockIdx.z;
    const int G = A.G, T = A.T, Hkv = A.Hq / G, nrows = T * G;
    const int64_t bh = (int64_t)b * Hkv + hk;
    const int S_packed = A.S_packed, tail_len = A.tail_len, len = S_packed + tail_len;

    // ---- q -> LDS: row r of the tile is (token, head) = ((tile * ROWS + r) / G, (tile * ROWS + r) % G); rows beyond T * G are zeros
    for (int idx = threadIdx.x; idx < ROWS * (D / 8); idx += 256) {
        const int row = idx / (D / 8), ch = idx % (D / 8);
        const int rg = tile * ROWS + row;
        uint4 raw = make_uint4(0u, 0u, 0u, 0u);
        if (rg < nrows) {
            const int t = rg / G, g = rg % G;
            raw = *reinterpret_cast<const uint4*>(reinterpret_cast<const uint16_t*>(A.q) + (((int64_t)b * A.Hq + hk * G + g) * T + t) * D + ch * 8);
        }
        unsigned char* dst = smem + row * QSTR + ch * 16;
        if (QH) {
            const uint32_t w[4] = {raw.x, raw.y, raw.z, raw.w};
            uint32_t wh[4], wl[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float x0 = f16_lo(w[j]), x1 = f16_hi(w[j]);
                const float h0 = (float)(__bf16)x0, h1 = (float)(__bf16)x1;
                wh[j] = pk_top(h0, h1);
                wl[j] = pk_top(x0 - h0, x1 - h1);                     // at most 4 significant bits are left: a bf16 value
            }
            *reinterpret_cast<uint4*>(dst) = make_uint4(wh[0], wh[1], wh[2], wh[3]);
            *reinterpret_cast<uint4*>(dst + QIMG) = make_uint4(wl[0], wl[1], wl[2], wl[3]);
            *reinterpret_cast<uint4*>(dst + 2 * QIMG) = raw;
        } else {
            *reinterpret_cast<uint4*>(dst) = raw;
        }
    }
    __syncthreads();

    int lim[NR];
    const float* brow[NR];
#pragma unroll
    for (int n = 0; n < NR; ++n) {
        const int rg = tile * ROWS + n * 16 + c;
        const int t = rg < nrows ? rg / G : 0;
        lim[n] = rg < nrows ? (A.causal ? len - T + t : len - 1) : -1;
        brow[n] = A.bias ? A.bias + (int64_t)b * A.bias_bstride + (int64_t)t * A.bias_tstride : nullptr;
    }
    const bool has_bias = A.bias != nullptr, bias_per_row = A.bias_tstride != 0;

    float m[NR], l[NR];
    v4f_t O[NR][DC];
#pragma unroll
    for (int n = 0; n < NR; ++n) {
        m[n] = neg_inf(); l[n] = 0.f;
#pragma unroll
        for (int dc = 0; dc < DC; ++dc) O[n][dc] = v4f_t{0.f, 0.f, 0.f, 0.f};
    }

    split_range(split, A.nsplit, A.gps, S_packed, tail_len, g0, npk, ntc);
    unsigned char* vtile = smem + NQ * QIMG + wv * VTILE;
    const unsigned char* qfrag = smem + c * QSTR + h * 16;                // + n * 16 * QSTR + ks * 64: the B fragment of row n * 16 + c
    const int vc8 = lane % LPT, vts = lane / LPT;

    for (int it = wv; it < npk + ntc; it += 4) {
        v4f_t S[NR][2];
#pragma unroll
        for (int n = 0; n < NR; ++n) { S[n][0] = v4f_t{0.f, 0.f, 0.f, 0.f}; S[n][1] = v4f_t{0.f, 0.f, 0.f, 0.f}; }
        if (it < npk) {                                               // ---- a packed group
            const int gi = g0 + it;
            uint32_t kr[2][KS][2], vr[NP][2], vsb[NP];
            uint2 ksr[KS];
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                ksr[ks] = *reinterpret_cast<const uint2*>(A.ks + (bh * (A.S_cap / 32) + gi) * D + ks * 32 + h * 8);
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const int64_t row = bh * A.S_cap + gi * 32 + s * 16 + c;
                    if (FP4) {
                        kr[s][ks][0] = *reinterpret_cast<const uint32_t*>(A.kc + row * (D / 2) + ks * 16 + h * 4); kr[s][ks][1] = 0u;
                    } else {
                        const uint2 kk = *reinterpret_cast<const uint2*>(A.kc + row * D + ks * 32 + h * 8);
                        kr[s][ks][0] = kk.x; kr[s][ks][1] = kk.y;
                    }
                }
            }
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const int64_t row = bh * A.S_cap + gi * 32 + p * TP + vts;
                if (FP4) {
                    vr[p][0] = *reinterpret_cast<const uint32_t*>(A.vc + row * (D / 2) + vc8 * 4); vr[p][1] = 0u;
                } else {
                    const uint2 vv = *reinterpret_cast<const uint2*>(A.vc + row * D + vc8 * 8); vr[p][0] = vv.x; vr[p][1] = vv.y;
                }
                vsb[p] = A.vs[row * (D / 32) + vc8 / 4];
            }
            // K -> bf16 fragments: the scales differ inside a channel pair, so scale 1 and an exact multiply
            uint4 kf[2][KS];
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                float ksf[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) ksf[j] = e8m0_f32(((j < 4 ? ksr[ks].x : ksr[ks].y) >> (8 * (j & 3))) & 0xFFu);
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    float f[8];
                    cvt8<FP4>(kr[s][ks][0], kr[s][ks][1], 1.0f, f);
#pragma unroll
                    for (int j = 0; j < 8; ++j) f[j] *= ksf[j];
                    kf[s][ks] = make_uint4(pk_top(f[0], f[1]), pk_top(f[2], f[3]), pk_top(f[4], f[5]), pk_top(f[6], f[7]));
                }
            }
            // V -> bf16, the wave's tile [token][D]: a V block lies along head_dim, the 8 channels share the scale operand
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                float f[8];
                cvt8<FP4>(vr[p][0], vr[p][1], u2f(vsb[p] << 23), f);
                *reinterpret_cast<uint4*>(vtile + (p * TP + vts) * VSTR + vc8 * 16) =
                    make_uint4(pk_top(f[0], f[1]), pk_top(f[2], f[3]), pk_top(f[4], f[5]), pk_top(f[6], f[7]));
            }
#pragma unroll
            for (int n = 0; n < NR; ++n)
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    const uint4 qh = *reinterpret_cast<const uint4*>(qfrag + n * 16 * QSTR + ks * 64);
                    S[n][0] = mma<false>(kf[0][ks], qh, S[n][0]);
                    S[n][1] = mma<false>(kf[1][ks], qh, S[n][1]);
                    if (QH) {
                        const uint4 ql = *reinterpret_cast<const uint4*>(qfrag + QIMG + n * 16 * QSTR + ks * 64);
                        S[n][0] = mma<false>(kf[0][ks], ql, S[n][0]);
                        S[n][1] = mma<false>(kf[1][ks], ql, S[n][1]);
                    }
                }
            wave_lds_sync();
            fold_group<false, NR, D>(S, m, l, O, lim, brow, has_bias, bias_per_row, len, gi * 32, A.scaling, vtile, VSTR, lane);
        } else {                                                      // ---- 32 tokens of the tail (cache dtype = the query's)
            const int tc = it - npk;
            uint4 kf[2][KS];
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int j = tc * 32 + s * 16 + c;
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    kf[s][ks] = make_uint4(0u, 0u, 0u, 0u);
                    if (j < tail_len)
                        kf[s][ks] = *reinterpret_cast<const uint4*>(reinterpret_cast<const uint16_t*>(A.kt) + (bh * A.tail_cap + j) * D + ks * 32 + h * 8);
                }
            }
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const int j = tc * 32 + p * TP + vts;
                uint4 vv = make_uint4(0u, 0u, 0u, 0u);                // zeros where the token does not exist
                if (j < tail_len) vv = *reinterpret_cast<const uint4*>(reinterpret_cast<const uint16_t*>(A.vt) + (bh * A.tail_cap + j) * D + vc8 * 8);
                *reinterpret_cast<uint4*>(vtile + (p * TP + vts) * VSTR + vc8 * 16) = vv;
            }
#pragma unroll
            for (int n = 0; n < NR; ++n)
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    const uint4 qv = *reinterpret_cast<const uint4*>(qfrag + (QH ? 2 * QIMG : 0) + n * 16 * QSTR + ks * 64);
                    S[n][0] = mma<QH>(kf[0][ks], qv, S[n][0]);
                    S[n][1] = mma<QH>(kf[1][ks], qv, S[n][1]);
                }
            wave_lds_sync();
            fold_group<QH, NR, D>(S, m, l, O, lim, brow, has_bias, bias_per_row, len, S_packed + tc * 32, A.scaling, vtile, VSTR, lane);
        }
        wave_lds_sync();
    }

    // a row's l is spread over its 4 lanes
#pragma unroll
    for (int n = 0; n < NR; ++n) {
        l[n] += __shfl_xor(l[n], 16, 64);
        l[n] += __shfl_xor(l[n], 32, 64);
    }
    __syncthreads();                                                  // every wave is done with the q images and its V tile
    float* red = reinterpret_cast<float*>(smem);                      // [4 waves][ROWS][RSTR]
#pragma unroll
    for (int n = 0; n < NR; ++n) {
        float* rr = red + ((wv * ROWS) + n * 16 + c) * RSTR;
#pragma unroll
        for (int dc = 0; dc < DC; ++dc) *reinterpret_cast<float4*>(rr + dc * 16 + 4 * h) = make_float4(O[n][dc][0], O[n][dc][1], O[n][dc][2], O[n][dc][3]);
        if (h == 0) { rr[D] = m[n]; rr[D + 1] = l[n]; }
    }
    __syncthreads();
    // the four waves, in wave order -> the split's partial (acc[D], m, l) of every row of the tile
    for (int idx = threadIdx.x; idx < ROWS * D; idx += 256) {
        const int row = idx / D, d = idx % D;
        const int rg = tile * ROWS + row;
        if (rg >= nrows) continue;
        float mn = neg_inf();
#pragma unroll
        for (int w = 0; w < 4; ++w) mn = __builtin_fmaxf(mn, red[(w * ROWS + row) * RSTR + D]);
        const float mm = (mn == neg_inf()) ? 0.f : mn;
        float num = 0.f, den = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const float* rr = red + (w * ROWS + row) * RSTR;
            const float f = ex(rr[D] - mm);
            num += rr[d] * f; den += rr[D + 1] * f;
        }
        const int t = rg / G, g = rg % G;
        float* o = A.ws + (((((int64_t)b * T + t) * A.Hq + hk * G + g) * A.nsplit) + split) * (D + 2);
        o[d] = num;
        if (d == 0) { o[D] = mn; o[D + 1] = den; }
    }
}

// the checks of the sizes + the plan (the single-token entry's, a function of S_packed alone)
int multi_plan(int64_t B, int Hq, int Hkv, int D, int T, int64_t S_packed, int64_t tail_len, AttnPlan* p) {
    if (T < 1 || T > 32) return kvp_fail(MSQ_ERR_BAD_ARG, "msq_kv_mx_attn_multi: T must be 1 .. 32");
    const int rc = attn_plan(B, Hq, Hkv, D, S_packed, tail_len, p);
    if (rc != MSQ_OK) return rc;
    if (T > S_packed + tail_len) return kvp_fail(MSQ_ERR_BAD_ARG, "msq_kv_mx_attn_multi: T exceeds the cached length (the query tokens are the cache's last T)");
    return MSQ_OK;
}

}  // namespace

extern "C" {

int64_t msq_kv_mx_attn_multi_workspace_bytes(int64_t B, int Hq, int Hkv, int D, int T, int64_t S_packed, int64_t tail_len) {
    AttnPlan p;
    const int rc = multi_plan(B, Hq, Hkv, D, T, S_packed, tail_len, &p);
    return rc != MSQ_OK ? (int64_t)rc : B * Hq * (int64_t)T * p.nsplit * (D + 2) * (int64_t)sizeof(float);
}

int msq_kv_mx_attn_multi(const void* q, int q_dtype, const void* k_codes, const void* k_scales, const void* v_codes, const void* v_scales,
                         int64_t S_packed, int64_t S_cap, const void* k_tail, const void* v_tail, int64_t tail_len, int64_t tail_cap,
                         const float* bias, int64_t bias_row_stride_t, int causal, void* out, int out_dtype, int64_t B, int Hq, int Hkv, int D,
                         int T, int elem_fmt, float scaling, void* workspace, int64_t workspace_bytes, void* stream) {
    AttnPlan p;
    const int rc = multi_plan(B, Hq, Hkv, D, T, S_packed, tail_len, &p);
    if (rc != MSQ_OK) return rc;
    const int ns = p.nsplit;
    const int64_t len = S_packed + tail_len;
    MultiArgs A;
    set_attn_buffers(A, q, k_codes, k_scales, v_codes, v_scales, k_tail, v_tail, bias, workspace);
    const char* own = (S_cap < 0 || S_cap % 32 || S_packed > S_cap) ? "S_packed exceeds S_cap (a multiple of 32)"
                    : tail_len > tail_cap ? "tail_len exceeds tail_cap"
                    : (bias && bias_row_stride_t != 0 && bias_row_stride_t < len) ? "bias_row_stride_t must be 0 (rows [B, len]) or at least len (rows [B, T, stride])"
                    : nullptr;
    const int bad = check_attn_common("msq_kv_mx_attn_multi", A, out, nullptr, elem_fmt, q_dtype, out_dtype, own, S_packed != 0, tail_len != 0, workspace_bytes,
                                      B * Hq * (int64_t)T * ns * (D + 2) * (int64_t)sizeof(float), "workspace too small (msq_kv_mx_attn_multi_workspace_bytes)");
    if (bad != MSQ_OK) return bad;
    const int G = Hq / Hkv, nrows = T * G;
    const int nr = nrows <= 16 ? 1 : (nrows <= 32 ? 2 : 4);          // 16-row tiles of a block: at most 64 rows per row tile
    const int ntiles = (nrows + nr * 16 - 1) / (nr * 16);
    if ((int64_t)Hkv * ntiles > 65535) return kvp_fail(MSQ_ERR_UNSUPPORTED, "msq_kv_mx_attn_multi: sizes beyond the launch grid");
    if (B * Hq * (int64_t)T > 0x7FFFFFFF) return kvp_fail(MSQ_ERR_UNSUPPORTED, "msq_kv_mx_attn_multi: sizes beyond the launch grid");
    A.Hq = Hq; A.G = G; A.T = T; A.nsplit = ns; A.gps = p.gps; A.S_packed = (int)S_packed; A.tail_len = (int)tail_len; A.tail_cap = (int)tail_cap;
    A.ntiles = ntiles; A.causal = causal ? 1 : 0;
    A.S_cap = S_cap; A.bias_tstride = bias ? bias_row_stride_t : 0; A.bias_bstride = bias_row_stride_t ? (int64_t)T * bias_row_stride_t : len;
    A.scaling = scaling;
    hipStream_t st = (hipStream_t)stream;
    const bool f4 = elem_fmt == MSQ_FMT_FP4_E2M1;
    const dim3 grid((unsigned)ns, (unsigned)(Hkv * ntiles), (unsigned)B), blk(256);
#define MSQ_KVM(DV, F4, QD, NRV) hipLaunchKernelGGL((k_kvp_attn_multi_split<DV, F4, QD, NRV>), grid, blk, 0, st, A)
#define MSQ_KVM_N(DV, F4, QD) do { if (nr == 1) MSQ_KVM(DV, F4, QD, 1); else if (nr == 2) MSQ_KVM(DV, F4, QD, 2); else MSQ_KVM(DV, F4, QD, 4); } while (0)
#define MSQ_KVM_Q(DV, F4) do { if (q_dtype == 1) MSQ_KVM_N(DV, F4, 1); else MSQ_KVM_N(DV, F4, 2); } while (0)
#define MSQ_KVM_F(DV) do { if (f4) MSQ_KVM_Q(DV, true); else MSQ_KVM_Q(DV, false); } while (0)
    if (D == 64) MSQ_KVM_F(64); else MSQ_KVM_F(128);
#undef MSQ_KVM_F
#undef MSQ_KVM_Q
#undef MSQ_KVM_N
#undef MSQ_KVM
    if (hipGetLastError() != hipSuccess) return kvp_fail(MSQ_ERR_LAUNCH, "msq_kv_mx_attn_multi: launch failed");
    const dim3 cgrid((unsigned)(B * Hq * T));
#define MSQ_KVMC1(DV, OD) hipLaunchKernelGGL((k_kvp_attn_combine<DV, OD>), cgrid, dim3(DV), 0, st, (const float*)workspace, out, ns, (const int*)nullptr, (int64_t)0)
#define MSQ_KVMC(DV) do { if (out_dtype == 0) MSQ_KVMC1(DV, 0); else if (out_dtype == 1) MSQ_KVMC1(DV, 1); else MSQ_KVMC1(DV, 2); } while (0)
    if (D == 64) MSQ_KVMC(64); else MSQ_KVMC(128);
#undef MSQ_KVMC
#undef MSQ_KVMC1
    return hipGetLastError() == hipSuccess ? MSQ_OK : kvp_fail(MSQ_ERR_LAUNCH, "msq_kv_mx_attn_multi: launch failed");
}

}  // extern "C"
