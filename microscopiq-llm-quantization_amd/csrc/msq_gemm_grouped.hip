// msq_gemm_grouped.hip -- k_qgemm_grouped: ONE activation batch times SEVERAL packed weights chosen per row (mixture of experts; the expert
// Linears w1 / w3 / w2 the reference's harness quantises one by one, llm/llama.py:37-40 with model_type "mixtral").  For R routed rows sorted by
// expert
//     Y[r, :] = X[row_index[r], :] . W_e(r)^T (+ bias[e(r), :]),     e(r) = the expert whose range [row_offsets[e], row_offsets[e + 1]) holds r
// in one launch whose geometry is a function of the CAPACITY `rows` and E alone (msq_qlinear_grouped_plan): the per-expert counts stay on
// the device, so a decode step with a router in it can be captured in a HIP graph.
//
// Form: the per-wave stream of k_qgemm_sk form 1 (msq_gemm_stream.hip).  A block = one 64-row tile of ONE expert x one 64-column strip x all of
// K; its eight waves take the K-tiles kg, kg + 8, ... (every wave a 64 x 64 fp32 accumulator tile), the eight partial tiles meet in LDS and are
// summed in the fixed order of the waves.  The packed planes of expert e are exactly what msq_pack_values / msq_outlier_pack write for one
// [N, K] weight, at base + e * stride: per-expert buffer descriptors, nothing re-packed, kinds MSQ-U1 / U1X / U6 through HalfRegs /
// load_half_buf / convert_quarter.  The activation tile of a K-tile goes through registers into the wave's PRIVATE two-buffer LDS ring
// (buffer_load_b128 -> ds_write_b128 -> ds_read_b128 of one wave execute in order: no LDS-DMA, hence no barrier in the K-loop); its source
// rows come from row_index (the gather of the routed tokens is fused in) and are clamped to the expert's last row.
//
// Block -> (expert, row tile): the grid is strips x tile_slots, tile_slots >= sum_e ceil(m_e / 64) for EVERY split of `rows` into E counts
// (floor((rows - j) / 64) + j with j = min(E, rows)).  Every wave scans row_offsets with scalar loads (offsets clamped to [previous, rows]: a
// malformed table cannot take a store out of Y) until its slot falls into an expert; a slot beyond the last used one returns at once, and an
// expert without rows owns no slot: none of its bytes are read.  Every block owns its output tile: no flags, no atomics, no workspace, nothing
// waits on another block.
//
// Summation order: the K-tiles of an output element are added in an order that depends on (expert, strip) alone -- the walk starts at tile
// rot(expert, strip) and wraps, wave kg adds its tiles in walk order, the eight partial sums are added kg ascending.  A row's result is the same
// bits whether it is computed alone or among others, in whichever row tile and at whichever position, and from run to run.
// What bounds it: at decode sizes the packed bytes of the experts that have rows (read once); with many rows per expert every 64-row tile
// re-reads its strip's packed bytes and its own activation rows out of L2 -- (2 x 64 + packed bytes per 64 k) K bytes per block at the ~70 GB/s
// one CU pulls from L2 (MI355X_MICROARCH.md, "Indexed rows").
#include <stdio.h>
#include <stdlib.h>
#include <atomic>

#include "msq_gemm_common.h"

extern "C" void msq_set_error_(const char* msg);

namespace {

constexpr int G_MF = 4;            // 16-row fragments per block: 64 rows
constexpr int G_KG = 8;            // waves = k-groups per block
constexpr int G_BM = 16 * G_MF;
constexpr int G_A_TILE = G_BM * BK * 2;      // bytes of one activation tile
constexpr int G_PPW = G_BM / 8;              // 1 KiB staging pieces (8 rows) per tile

// one half-step of a wave (k_qgemm_sk's): MFMAs of the current weight fragments against the four activation fragments at `rd` (+ 2048 per
// fragment), the next half-step's fragments converted two quarters per fragment row behind them
template <int OUT_KIND>
MSQ_D void g_half_step(f32x4_t (&acc)[G_MF][4], const u32x4_t (&wf_use)[4], u32x4_t (&wf_make)[4],
                       const HalfRegs<MSQ_PLANE_NONE, OUT_KIND>& pk, const u32x4_t& sc, int kf_make, const char* rd) {
    bf16x8_t xf[3];
    xf[0] = *reinterpret_cast<const bf16x8_t*>(rd);
    xf[1] = *reinterpret_cast<const bf16x8_t*>(rd + 2048);
#pragma unroll
    for (int mf = 0; mf < G_MF; ++mf) {
        if (mf + 2 < G_MF) xf[(mf + 2) % 3] = *reinterpret_cast<const bf16x8_t*>(rd + (mf + 2) * 2048);
#pragma unroll
        for (int nf = 0; nf < 4; ++nf)
            acc[mf][nf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, wf_use[nf]), xf[mf % 3], acc[mf][nf], 0, 0, 0);
        convert_quarter<MSQ_PLANE_NONE, OUT_KIND>(wf_make, pk, sc, kf_make, mf * 2);
        convert_quarter<MSQ_PLANE_NONE, OUT_KIND>(wf_make, pk, sc, kf_make, mf * 2 + 1);
        __builtin_amdgcn_sched_barrier(0);
    }
}

template <int OUT_KIND> struct GSet {
    HalfRegs<MSQ_PLANE_NONE, OUT_KIND> h0, h1;
    u32x4_t sc;
};

template <int OUT_KIND, typename YT>
__global__ void __launch_bounds__(64 * G_KG, 1)
k_qgemm_grouped(const uint16_t* __restrict__ X, int x_rows, const int32_t* __restrict__ row_index, const int32_t* __restrict__ row_offsets,
                const uint8_t* __restrict__ inl_planes, const uint8_t* __restrict__ out_planes, const uint8_t* __restrict__ scl_planes,
                int64_t inl_stride, int64_t out_stride, int64_t scl_stride, const float* __restrict__ bias, YT* __restrict__ Y,
                int rows, int E, int N, int K, int tile_slots, int y16) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int IN_KIND = MSQ_PLANE_NONE;
    const int tid = threadIdx.x, lane = tid & 63;
    const int kg = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 15, g = lane >> 4;
    const int NTB = N / TILE_N;
    const int bid = (int)blockIdx.x;
    int slot, strip;
    if ((NTB & 7) == 0) {                                        // the row tiles of a strip on ONE XCD, back to back: an expert's packed bytes come from HBM once
        const int xcd = bid & 7, i = bid >> 3;
        slot = i % tile_slots; strip = (i / tile_slots) * 8 + xcd;
    } else { slot = bid % tile_slots; strip = bid / tile_slots; }

    // ---- (expert, row tile) of this block: a wave-uniform scan of row_offsets (scalar loads)
    int ex = -1, r0 = 0, r_end = 0;
    {
        int prev = 0, s = slot;
        for (int e = 0; e < E; ++e) {
            int hi = row_offsets[e + 1];
            hi = hi > prev ? hi : prev;
            hi = hi < rows ? hi : rows;
            const int t = (hi - prev + G_BM - 1) / G_BM;
            if (s < t) { ex = e; r0 = prev + s * G_BM; r_end = hi; break; }
            s -= t; prev = hi;
        }
    }
    ex = sgpr(ex);
    if (ex < 0) return;                                          // slot beyond the last used one (the whole block: nothing has been staged, no barrier passed)
    r0 = sgpr(r0); r_end = sgpr(r_end);

    const int KT = K / BK;
    const int nt = sgpr((kg < KT) ? (KT - kg + G_KG - 1) / G_KG : 0);   // tiles of this wave: kg, kg + 8, ... of the rotated walk
    char* const smem_g = smem + kg * (2 * G_A_TILE);

    const int64_t ntiles = (int64_t)(N / TILE_N) * KT;
    PlaneRsrc pr;
    pr.inl = make_rsrc(inl_planes ? inl_planes + (int64_t)ex * inl_stride : nullptr,
                       OUT_KIND == MSQ_PLANE_U6 ? ntiles * 2 * 1024 : (OUT_KIND == MSQ_PLANE_U8X ? ntiles * 2 * 256 : 0));
    pr.out = make_rsrc(out_planes + (int64_t)ex * out_stride, OUT_KIND == MSQ_PLANE_U6 ? ntiles * 2 * 512 : ntiles * 4 * 1024);
    constexpr int SCLB = SclBytes<OUT_KIND>::n;
    pr.scl = make_rsrc(scl_planes + (int64_t)ex * scl_stride, ntiles * 16 * SCLB);
    const int lane16 = lane * 16;
    const int scl_lane_off = (lane & 15) * SCLB;
    const uint32_t tile_row32 = (uint32_t)sgpr(strip * KT);
    const int i_last = sgpr(nt > 0 ? nt - 1 : 0);
    // the walk over K starts at a tile that is a function of (expert, strip) ONLY -- never of the slot, the row tile or the block index: every row
    // of an expert sums its K-tiles in the same order wherever it sits.  (Blocks that run side by side read different tiles and DRAM pages.)
    const int rot = sgpr((int)(((uint32_t)ex * 40503u + (uint32_t)strip * 5u) % (uint32_t)KT));
    auto kt_of = [&](int i) -> int {
        const int ic = i < i_last ? i : i_last;                  // branch-free tail: re-load the last tile
        int kt = kg + ic * G_KG; kt = kt < KT ? kt : KT - 1;     // (kg >= KT: a wave without tiles re-reads tile KT - 1 and multiplies nothing)
        kt += rot;
        return kt >= KT ? kt - KT : kt;
    };
    auto load_set = [&](GSet<OUT_KIND>& t, int i) {
        const uint32_t tile = tile_row32 + (uint32_t)kt_of(i);
        load_half_buf<IN_KIND, OUT_KIND>(t.h0, pr, lane16, tile * 2u);
        load_half_buf<IN_KIND, OUT_KIND>(t.h1, pr, lane16, tile * 2u + 1u);
        const u32x2_t v = __builtin_bit_cast(u32x2_t, __builtin_amdgcn_raw_buffer_load_b64(pr.scl, scl_lane_off, tile * (16u * SCLB), 0));
        t.sc = u32x4_t{v[0], v[1], 0u, 0u};
    };

    // activation staging: piece p = rows 8 p .. 8 p + 7 of the tile; lane l fetches row 8 p + l / 8, source chunk (l & 7) ^ ((row >> 1) & 7): the
    // LDS image stays lane-linear, fragment reads are conflict-free.  Source row: row_index[r] of the routed row r, r clamped to the expert's
    // last row (rows past it are computed and not stored), the index itself clamped into X.
    const __amdgpu_buffer_rsrc_t xr = make_rsrc(X, (int64_t)x_rows * K * 2);
    int aoff[G_PPW];
#pragma unroll
    for (int p = 0; p < G_PPW; ++p) {
        const int row = p * 8 + (lane >> 3);
        const int chunk = (lane & 7) ^ ((row >> 1) & 7);
        int r = r0 + row; r = r < r_end ? r : r_end - 1;
        int tok = row_index ? row_index[r] : r;
        tok = tok < 0 ? 0 : (tok < x_rows ? tok : x_rows - 1);
        aoff[p] = (int)(uint32_t)(((int64_t)tok * K + chunk * 8) * 2);
    }
    u32x4_t xs[G_PPW];
    auto xload = [&](int i) {
        const uint32_t koff = (uint32_t)kt_of(i) * (BK * 2);
#pragma unroll
        for (int p = 0; p < G_PPW; ++p) xs[p] = __builtin_bit_cast(u32x4_t, __builtin_amdgcn_raw_buffer_load_b128(xr, aoff[p], koff, 0));
    };
    auto xwrite = [&](int buf) {
#pragma unroll
        for (int p = 0; p < G_PPW; ++p) *reinterpret_cast<u32x4_t*>(smem_g + buf * G_A_TILE + p * 1024 + lane16) = xs[p];
    };
    const int sw = (c >> 1) & 7;
    const int rd0 = c * 128 + (((0 + g) ^ sw) << 4);
    const int rd1 = c * 128 + (((4 + g) ^ sw) << 4);

    f32x4_t acc[G_MF][4];
#pragma unroll
    for (int i = 0; i < G_MF; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    // four packed tile sets in flight per wave; the activation rows of tile i + 2 are requested in front of the packed loads of tile i + 4
    // (vmcnt is in-order) and written to LDS a tile later, into the buffer tile i was read from
    GSet<OUT_KIND> sA, sB, sC, sD;
    u32x4_t wfA[4], wfB[4];
    xload(0);
    load_set(sA, 0);
    load_set(sB, 1);
    load_set(sC, 2);
    load_set(sD, 3);
    __builtin_amdgcn_s_waitcnt(0);
    xwrite(0); xload(1);
#pragma unroll
    for (int q = 0; q < 8; ++q) convert_quarter<IN_KIND, OUT_KIND>(wfA, sA.h0, sA.sc, 0, q);
    int buf = 0;
#define G_TILE(I, CUR, NXT)                                                                                        \
    {                                                                                                              \
        const char* abase = smem_g + buf * G_A_TILE;                                                               \
        g_half_step<OUT_KIND>(acc, wfA, wfB, CUR.h1, CUR.sc, 1, abase + rd0);                                      \
        keep_live(NXT.h0); keep_live4(NXT.sc);         /* hipcc's vmcnt wait for tile i + 1's planes lands here */  \
        g_half_step<OUT_KIND>(acc, wfB, wfA, NXT.h0, NXT.sc, 0, abase + rd1);                                      \
        xwrite(buf ^ 1);                               /* tile i + 1 (requested a tile ago) into the buffer tile i - 1 was read from */ \
        __builtin_amdgcn_sched_barrier(0);                                                                         \
        xload((I) + 2);                                                                                            \
        __builtin_amdgcn_sched_barrier(0);                                                                         \
        load_set(CUR, (I) + 4);                                                                                    \
        __builtin_amdgcn_sched_barrier(0);                                                                         \
        buf ^= 1;                                                                                                  \
    }
    {
        int i = 0;
        for (; i + 3 < nt; i += 4) {
            G_TILE(i, sA, sB)
            G_TILE(i + 1, sB, sC)
            G_TILE(i + 2, sC, sD)
            G_TILE(i + 3, sD, sA)
        }
        if (i < nt) {
            G_TILE(i, sA, sB)
            if (i + 1 < nt) {
                G_TILE(i + 1, sB, sC)
                if (i + 2 < nt) G_TILE(i + 2, sC, sD)
            }
        }
    }
#undef G_TILE

    // ---- the eight partial tiles meet in LDS: red[wave][quad (mf, nf)][lane] float4 (conflict-free), summed in the order of the waves; wave kg
    // reduces and stores fragment row kg / 2, quad pair (kg & 1) * 2
    __builtin_amdgcn_s_waitcnt(0x0070);                          // vmcnt(0) lgkmcnt(0): nothing of this wave reads or fills its ring any more
    __builtin_amdgcn_s_barrier();
    float4* red = reinterpret_cast<float4*>(smem);
    const int n_base = strip * TILE_N;
    const int colp = (g & 1) ? 16 + (g - 1) * 4 : g * 4;         // 16-bit outputs: this lane's 8 columns inside the unit's 32 after the swap (store_wave_tile_direct_)
#pragma unroll
    for (int mf = 0; mf < G_MF; ++mf)
#pragma unroll
        for (int nf = 0; nf < 4; ++nf) {
            const f32x4_t& a4 = acc[mf][nf];
            red[(kg * (G_MF * 4) + mf * 4 + nf) * 64 + lane] = make_float4(a4[0], a4[1], a4[2], a4[3]);
        }
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __builtin_amdgcn_s_barrier();
    const int mf = kg >> 1, a = (kg & 1) * 2;
    const float* bias_e = bias ? bias + (int64_t)ex * N : nullptr;
    f32x4_t s[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        float4 t = red[(0 * (G_MF * 4) + mf * 4 + a + q) * 64 + lane];
#pragma unroll
        for (int k2 = 1; k2 < G_KG; ++k2) {
            const float4 p = red[(k2 * (G_MF * 4) + mf * 4 + a + q) * 64 + lane];
            t.x += p.x; t.y += p.y; t.z += p.z; t.w += p.w;
        }
        s[q] = f32x4_t{t.x, t.y, t.z, t.w};
        if (bias_e) {
            const float4 b = *reinterpret_cast<const float4*>(bias_e + n_base + (a + q) * 16 + g * 4);
            s[q][0] += b.x; s[q][1] += b.y; s[q][2] += b.z; s[q][3] += b.w;
        }
    }
    const int m = r0 + mf * 16 + c;                              // routed row of this lane: stored only inside the expert's own range (r_end <= rows)
    char* rowp = reinterpret_cast<char*>(Y) + ((int64_t)m * N + n_base) * (int64_t)sizeof(YT);
    if (sizeof(YT) == 4) {
#pragma unroll
        for (int q = 0; q < 2; ++q)
            if (m < r_end) *reinterpret_cast<float4*>(rowp + ((a + q) * 16 + g * 4) * 4) = make_float4(s[q][0], s[q][1], s[q][2], s[q][3]);
    } else {
        uint32_t d[2][2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            if (y16) {
                f16x2_t lo, hi;
                lo[0] = (_Float16)s[q][0]; lo[1] = (_Float16)s[q][1]; hi[0] = (_Float16)s[q][2]; hi[1] = (_Float16)s[q][3];
                d[q][0] = __builtin_bit_cast(uint32_t, lo); d[q][1] = __builtin_bit_cast(uint32_t, hi);
            } else {
                bf16x2_t lo, hi;
                lo[0] = (__bf16)s[q][0]; lo[1] = (__bf16)s[q][1]; hi[0] = (__bf16)s[q][2]; hi[1] = (__bf16)s[q][3];
                d[q][0] = __builtin_bit_cast(uint32_t, lo); d[q][1] = __builtin_bit_cast(uint32_t, hi);
            }
        }
        const auto x0 = __builtin_amdgcn_permlane16_swap(d[0][0], d[1][0], false, false);
        const auto x1 = __builtin_amdgcn_permlane16_swap(d[0][1], d[1][1], false, false);
        const u32x4_t o = {x0[0], x1[0], x0[1], x1[1]};
        if (m < r_end) *reinterpret_cast<u32x4_t*>(rowp + (a * 16 + colp) * 2) = o;
    }
}

struct DevOnceG { std::atomic<uint64_t> mask{0}; };
inline bool attr_needed_g(const DevOnceG& o) {
    int d = 0;
    if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= 64) return true;
    return !(o.mask.load(std::memory_order_acquire) & (1ull << d));
}
inline void attr_done_g(DevOnceG& o) {
    int d = 0;
    if (hipGetDevice(&d) == hipSuccess && d >= 0 && d < 64) o.mask.fetch_or(1ull << d, std::memory_order_release);
}

int fail_g(int code, const char* msg) { msq_set_error_(msg); return code; }

}  // namespace

extern "C" int msq_qlinear_grouped_plan(int64_t rows, int E, int64_t N, int64_t K, int out_kind, int* row_tile, int* tile_slots, int64_t* blocks) {
    if (rows < 0 || E < 1) return fail_g(MSQ_ERR_BAD_ARG, "msq_qlinear_grouped_plan: rows must be >= 0 and E >= 1");
    if (out_kind != MSQ_PLANE_U8 && out_kind != MSQ_PLANE_U8X && out_kind != MSQ_PLANE_U6)
        return fail_g(MSQ_ERR_UNSUPPORTED, "msq_qlinear_grouped_plan: the grouped GEMM reads the unified planes only (MSQ_PLANE_U8 / _U8X / _U6 with in_kind NONE)");
    if (N <= 0 || K <= 0 || (N % BN) || (K % BK))
        return fail_g(MSQ_ERR_UNSUPPORTED, "msq_qlinear_grouped_plan: N must be a positive multiple of 256 and K of 64");
    if (rows > (1 << 30) || N > (1 << 30) || K > (1 << 30) || E > 65536) return fail_g(MSQ_ERR_UNSUPPORTED, "msq_qlinear_grouped_plan: dimension too large");
    // sum_e ceil(m_e / 64) over every split of `rows` into E counts: j experts with a part-filled last tile hold at least j rows, the whole
    // tiles share the other rows - j: floor((rows - j) / 64) + j, largest at j = min(E, rows)
    const int64_t j = rows < E ? rows : E;
    const int64_t slots = (rows - j) / G_BM + j;
    const int64_t nblk = slots * (N / TILE_N);
    if (nblk > 0x7FFFFFFFll) return fail_g(MSQ_ERR_UNSUPPORTED, "msq_qlinear_grouped_plan: grid too large; split the rows on the host");
    if (row_tile) *row_tile = G_BM;
    if (tile_slots) *tile_slots = (int)slots;
    if (blocks) *blocks = nblk;
    return MSQ_OK;
}

extern "C" int msq_qlinear_grouped_bf16(const void* X, int64_t x_rows, const int32_t* row_index, const int32_t* row_offsets,
                                        const void* inl_planes, const void* out_planes, const void* scale_planes,
                                        int64_t inl_stride, int64_t out_stride, int64_t scale_stride, const float* bias, void* Y, int y_dtype,
                                        int64_t rows, int E, int64_t N, int64_t K, int block, int in_kind, int out_kind, void* stream) {
    if (in_kind != MSQ_PLANE_NONE)
        return fail_g(MSQ_ERR_UNSUPPORTED, "msq_qlinear_grouped_bf16: the grouped GEMM reads the unified planes only (in_kind NONE with MSQ_PLANE_U8 / _U8X / _U6)");
    int slots = 0;
    int64_t nblk = 0;
    int rc = msq_qlinear_grouped_plan(rows, E, N, K, out_kind, nullptr, &slots, &nblk);
    if (rc) return rc;
    int64_t ib = 0, ob = 0, sb = 0;
    rc = msq_packed_sizes(N, K, block, in_kind, out_kind, &ib, &ob, &sb, nullptr);
    if (rc) return rc;
    if (y_dtype != 0 && y_dtype != 1 && y_dtype != 2) return fail_g(MSQ_ERR_UNSUPPORTED, "msq_qlinear_grouped_bf16: y_dtype must be 0 (f32), 1 (fp16) or 2 (bf16)");
    if (rows == 0) return MSQ_OK;
    if (!X || !Y || !row_offsets || !out_planes || !scale_planes || (ib > 0 && !inl_planes))
        return fail_g(MSQ_ERR_BAD_ARG, "msq_qlinear_grouped_bf16: null buffer");
    if (x_rows < 1) return fail_g(MSQ_ERR_BAD_ARG, "msq_qlinear_grouped_bf16: X has no rows");
    if (out_stride < ob || scale_stride < sb || (ib > 0 && inl_stride < ib) || (out_stride & 3) || (scale_stride & 3) || (ib > 0 && (inl_stride & 3)))
        return fail_g(MSQ_ERR_BAD_ARG, "msq_qlinear_grouped_bf16: an expert stride is smaller than one expert's plane (msq_packed_sizes) or not a multiple of 4 bytes");
    if (x_rows * K * 2 > 0xFFFFFFFFll || ib > 0xFFFFFFFFll || ob > 0xFFFFFFFFll || sb > 0xFFFFFFFFll)
        return fail_g(MSQ_ERR_UNSUPPORTED, "msq_qlinear_grouped_bf16: activations (x_rows*K*2 bytes) and every expert's planes must stay below 4 GiB");
    const dim3 grid((unsigned)nblk), blk(64 * G_KG);
    const size_t lds = (size_t)G_KG * 2 * G_A_TILE;              // = the eight partial tiles of the reduction (8 x 16 KiB)
    const int y16 = (y_dtype == 1) ? 1 : 0;
    hipStream_t st = (hipStream_t)stream;
#define G_LAUNCH(OK, YT)                                                                                               \
    do { static DevOnceG once_;                                                                                        \
         if (attr_needed_g(once_)) { (void)hipFuncSetAttribute((const void*)k_qgemm_grouped<OK, YT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); attr_done_g(once_); } \
         hipLaunchKernelGGL((k_qgemm_grouped<OK, YT>), grid, blk, lds, st, (const uint16_t*)X, (int)x_rows, row_index, row_offsets,          \
                            (const uint8_t*)inl_planes, (const uint8_t*)out_planes, (const uint8_t*)scale_planes, inl_stride, out_stride,    \
                            scale_stride, bias, (YT*)Y, (int)rows, E, (int)N, (int)K, slots, y16); } while (0)
#define G_KIND(OK) do { if (y_dtype == 0) G_LAUNCH(OK, float); else G_LAUNCH(OK, uint16_t); } while (0)
    if (out_kind == MSQ_PLANE_U8) G_KIND(MSQ_PLANE_U8);
    else if (out_kind == MSQ_PLANE_U8X) G_KIND(MSQ_PLANE_U8X);
    else G_KIND(MSQ_PLANE_U6);
#undef G_KIND
#undef G_LAUNCH
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { char b[200]; snprintf(b, sizeof(b), "msq_qlinear_grouped_bf16(k_qgemm_grouped): %s", hipGetErrorString(e)); return fail_g(MSQ_ERR_LAUNCH, b); }
    return MSQ_OK;
}
