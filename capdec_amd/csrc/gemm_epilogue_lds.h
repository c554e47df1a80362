// Coalesced GEMM epilogues: the accumulators of a wavefront go through an LDS transposition before they leave the CU.
//
// Why (round 4, per-block phase stamps: profiles/r4_gemm_pp.txt): in the TR accumulator layout a lane owns four consecutive columns of ONE row, so a
// float4 store instruction of the direct epilogues (gemm_epilogue.h) touches 64 different rows -- 64
// partly written 128-byte lines per instruction, ~600 cycles each: a 256 x 256 tile took 17-20 us to store (a quarter of
// its whole time at 25 000 rows; most of a 625-caption launch's fixed cost), the packed outputs (8-byte pieces) more.
// Here every wavefront writes a 32-row block of its tile into its own LDS slab [32][W + 4] fp32 (16 ds_write_b128 at
// most), reads it back row-major -- consecutive lanes hold consecutive 16 bytes of a row -- applies bias / activation /
// residual there (bias is per column: loaded once per lane; the residual is read as coalesced as the result is written)
// and stores whole row segments: W = 64 columns -> 4 rows x 256 B per instruction.  The packed f16x2 output leaves as
// 16-byte pieces that tile 256-byte runs of a plane, the K / V third of the decode-step qkv projection as whole 256-byte
// keys / values.  No block barrier: a slab is private to its wavefront (the ring must be idle: the main loops end with
// vmcnt(0) + s_barrier).
#pragma once
#include "gemm_epilogue.h"

namespace capdec {

struct EpiArgs {
    float *C = nullptr;
    int ldc = 0, M = 0, N = 0, m0 = 0, n0 = 0;
    const float *bias = nullptr;
    const float *resid = nullptr;      // fp32 residual [M, ldr] (C path)
    int ldr = 0, act = CAPDEC_ACT_NONE;
    float scale = 1.0f;
    char *packed = nullptr;            // packed f16x2 / x1 output (K of the next GEMM = N)
    const char *resid_pk = nullptr;    // packed residual of the output's format
    int fmt = PK_F16X2;
    const QkvScatter *sc = nullptr;    // decode-step qkv projection: K / V thirds straight into the cache
};

template <int TJ> struct EpiSlab {
    static constexpr int W = TJ * 32, LD = W + 4;                 // floats; LD % 32 == 4: conflict-free 16-byte row writes
    static constexpr int BYTES = 32 * LD * 4;
};

template <int ACT> __device__ __forceinline__ float act_const(float v) {
    if constexpr (ACT == CAPDEC_ACT_TANH) return tanhf(v);
    else if constexpr (ACT == CAPDEC_ACT_RELU) return fmaxf(v, 0.f);
    else if constexpr (ACT == CAPDEC_ACT_GELU_NEW) {
        const float c2 = 2.0f * 0.7978845608028654f;
        const float u2 = v * (c2 + (c2 * 0.044715f) * v * v);
        return __fdividef(v, 1.f + __expf(-u2));
    } else if constexpr (ACT == CAPDEC_ACT_QUICK_GELU) return __fdividef(v, 1.f + __expf(-1.702f * v));   // (rcp + mul like gelu_new above: an IEEE division is ~10 VALU instructions per element of a K = 512 tile whose MFMAs take less time than its epilogue)
    else return v;
}
template <int ACT> __device__ __forceinline__ float post_resid_const(float v) {
    if constexpr (ACT == CAPDEC_ACT_RESID_RELU) return fmaxf(v, 0.f);
    else return v;
}

// rows of the 32-row block per pass and passes per block when a lane owns Q consecutive quads (4 Q columns) of a row
template <int TJ, int Q> struct EpiWalk {
    static constexpr int LPR = TJ * 8 / Q;                        // lanes per row
    static constexpr int PASSES = (32 * LPR + 63) / 64;
};

// One wavefront: acc[i][j] (TR layout; WAVE_M / WAVE_N = the wavefront's block coordinates in units of its tile) ->
// slab -> out.  MODE 0: fp32 C (+ bias, activation, residual); 1: packed output (+ packed residual); 2: qkv scatter.
// AHEAD (MODE 0 and 2, a lane's column the same in every pass): the lane's bias quad and, MODE 0, the residual quads of
// all its TI x PASSES pieces are requested BEFORE the transposition instead of inside each store pass, where a pass's
// residual load sat behind the previous pass's stores on the wavefront's memory counter -- TI x PASSES x 4 registers, so
// only for the 2 x 2 tile, whose cross-term accumulators are dead by then.  Addresses of pieces past M or N are clamped
// into the matrix (loaded, never used): no branch per load.  The arithmetic of a piece is unchanged.
template <int TI, int TJ, int MODE, int ACT, bool AHEAD = false>
__device__ __forceinline__ void epilogue_lds_wave(const f32x16 (&acc)[TI][TJ], float *slab, int row0, int col0,
                                                  const EpiArgs &a) {
    using S = EpiSlab<TJ>;
    const int lane = threadIdx.x & 63, half = lane >> 5, l32 = lane & 31;
    constexpr int Q = MODE == 1 ? 2 : 1;                           // packed output: 8 columns (one 16-byte piece) per lane
    using Wk = EpiWalk<TJ, Q>;
    constexpr bool PRE = AHEAD && MODE != 1;
    static_assert(!PRE || (64 % Wk::LPR == 0 && Wk::PASSES * 64 == 32 * Wk::LPR), "AHEAD: one column per lane, whole passes");
    float4 bq = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 rq[PRE && MODE == 0 ? TI * Wk::PASSES : 1];
    if constexpr (PRE) {
        const int colc = min(col0 + (lane % Wk::LPR) * 4, a.N - 4);
        if (a.bias) bq = *reinterpret_cast<const float4 *>(a.bias + colc);
        if constexpr (MODE == 0) {
            if (a.resid) {
#pragma unroll
                for (int i = 0; i < TI; ++i)
#pragma unroll
                    for (int p = 0; p < Wk::PASSES; ++p) {
                        const int rowc = min(row0 + i * 32 + (p * 64 + lane) / Wk::LPR, a.M - 1);
                        rq[i * Wk::PASSES + p] = *reinterpret_cast<const float4 *>(a.resid + (size_t)rowc * a.ldr + colc);
                    }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < TI; ++i) {
        // ---- accumulators -> slab (row l32, four consecutive columns per quad)
#pragma unroll
        for (int j = 0; j < TJ; ++j)
#pragma unroll
            for (int g = 0; g < 4; ++g)
                *reinterpret_cast<float4 *>(slab + l32 * S::LD + j * 32 + 8 * g + 4 * half) = acc_quad(acc[i][j], g);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // ---- slab -> memory, row-major
#pragma unroll
        for (int p = 0; p < Wk::PASSES; ++p) {
            const int idx = p * 64 + lane;
            const int rl = idx / Wk::LPR, cq = idx - rl * Wk::LPR;  // row in the block, piece in the row
            const int row = row0 + i * 32 + rl, col = col0 + cq * (4 * Q);
            const bool live = (Wk::PASSES * 64 == 32 * Wk::LPR || rl < 32) && row < a.M && col < a.N;
            if (!live) continue;
            float4 v[Q];
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                v[q] = *reinterpret_cast<const float4 *>(slab + rl * S::LD + cq * (4 * Q) + 4 * q);
                v[q].x *= a.scale; v[q].y *= a.scale; v[q].z *= a.scale; v[q].w *= a.scale;
                if (a.bias) {
                    float4 b;
                    if constexpr (PRE) b = bq;
                    else b = *reinterpret_cast<const float4 *>(a.bias + col + 4 * q);
                    v[q].x += b.x; v[q].y += b.y; v[q].z += b.z; v[q].w += b.w;
                }
                v[q].x = act_const<ACT>(v[q].x); v[q].y = act_const<ACT>(v[q].y);
                v[q].z = act_const<ACT>(v[q].z); v[q].w = act_const<ACT>(v[q].w);
            }
            if constexpr (MODE == 0) {
                if (a.resid) {
                    float4 r4;
                    if constexpr (PRE) r4 = rq[i * Wk::PASSES + p];
                    else r4 = *reinterpret_cast<const float4 *>(a.resid + (size_t)row * a.ldr + col);
                    v[0].x = post_resid_const<ACT>(v[0].x + r4.x); v[0].y = post_resid_const<ACT>(v[0].y + r4.y);
                    v[0].z = post_resid_const<ACT>(v[0].z + r4.z); v[0].w = post_resid_const<ACT>(v[0].w + r4.w);
                }
                *reinterpret_cast<float4 *>(a.C + (size_t)row * a.ldc + col) = v[0];
            } else if constexpr (MODE == 2) {
                const QkvScatter &sc = *a.sc;
                if (col < sc.d) {
                    *reinterpret_cast<float4 *>(a.C + (size_t)row * a.ldc + col) = v[0];
                } else {
                    const int cap = row / sc.beam, b = row - cap * sc.beam;
                    const size_t srow = (size_t)(sc.cmap ? sc.cmap[cap] : cap) * sc.beam + b;
                    float *cache = col >= 2 * sc.d ? sc.vc : sc.kc;
                    const int hc = col - (col >= 2 * sc.d ? 2 * sc.d : sc.d), head = hc >> 6;
                    const size_t el = ((srow * sc.heads + head) * sc.ctx + sc.pos) * 64 + (hc & 63);
                    if (sc.bf16) {
                        bf16x4 t;
                        t[0] = (__bf16)v[0].x; t[1] = (__bf16)v[0].y; t[2] = (__bf16)v[0].z; t[3] = (__bf16)v[0].w;
                        *reinterpret_cast<bf16x4 *>(reinterpret_cast<__bf16 *>(cache) + el) = t;
                    } else
                        *reinterpret_cast<float4 *>(cache + el) = v[0];
                }
            } else {
                // one 16-byte half of a (row, k-step) chunk per plane: k-step = col / 16, half = (col / 8) & 1, swizzled
                // by bit 3 of the row like x3_group_offset
                const int nk_out = a.N >> 4, ks = col >> 4, hf = (col >> 3) & 1, r7 = row & 127;
                const size_t blk = (size_t)(row >> 7) * nk_out + ks;
                const int inrow = r7 * X3_ROW_B + ((hf ^ ((r7 >> 3) & 1)) << 4);
                if (a.resid_pk) {
#pragma unroll
                    for (int q = 0; q < Q; ++q) {
                        const float4 rr = x3_load_quad(a.resid_pk, nk_out, row, ks, 2 * hf + q, a.fmt);
                        v[q].x = post_resid_const<ACT>(v[q].x + rr.x); v[q].y = post_resid_const<ACT>(v[q].y + rr.y);
                        v[q].z = post_resid_const<ACT>(v[q].z + rr.z); v[q].w = post_resid_const<ACT>(v[q].w + rr.w);
                    }
                }
                if (a.fmt == PK_F16X2) {
                    f16x4 h0, l0, h1, l1;
                    split2h(v[0], h0, l0);
                    split2h(v[1], h1, l1);
                    char *pp = a.packed + blk * H2_BLOCK_B + inrow;
                    f16x8 hh, ll;
#pragma unroll
                    for (int e = 0; e < 4; ++e) { hh[e] = h0[e]; hh[4 + e] = h1[e]; ll[e] = l0[e]; ll[4 + e] = l1[e]; }
                    *reinterpret_cast<f16x8 *>(pp) = hh;
                    *reinterpret_cast<f16x8 *>(pp + X3_PLANE_B) = ll;
                } else {      // one-plane formats
                    x3_store_quad(a.packed, nk_out, row, ks, 2 * hf, v[0], a.fmt);
                    x3_store_quad(a.packed, nk_out, row, ks, 2 * hf + 1, v[1], a.fmt);
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}

template <int TI, int TJ> __device__ __forceinline__ void epilogue_slab_fill(const f32x16 (&acc)[TI][TJ], float *slab, int i) {
    using S = EpiSlab<TJ>;
    const int lane = threadIdx.x & 63, half = lane >> 5, l32 = lane & 31;
#pragma unroll
    for (int j = 0; j < TJ; ++j)
#pragma unroll
        for (int g = 0; g < 4; ++g)
            *reinterpret_cast<float4 *>(slab + l32 * S::LD + j * 32 + 8 * g + 4 * half) = acc_quad(acc[i][j], g);
}
__device__ __forceinline__ void epilogue_slab_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Section 10 of DESIGN.md: the vector-ALU work between two tiles.  The two walks below produce what epilogue_lds_wave
// produces -- the same values to the same addresses -- for the cases the decode step runs 24 times per step; what differs
// is what a lane does per piece besides the arithmetic of its values.

// MODE 1, two-plane output without a packed residual, of a wavefront block that lies wholly inside [0, M) x [0, N) and
// starts at a multiple of 32 rows (195 of 196 row tiles at 25 000 rows).  A lane's column is the same in every pass: its
// k-step, its half and its bias are taken once.  Its rows advance by 64 / LPR per pass inside one 128-row block of the
// plane: the block offset is taken once per 32 rows, the pass offset and the swizzle bit (bit 3 of the row) are constants of
// the unrolled loop.  No `live` test, no clamped address.  Saturated quads are summed in a register and posted once; a pass
// in which no lane saturates (every pass of a healthy checkpoint) skips the clamp, which is the identity there.
template <int TI, int TJ, int ACT>
__device__ __forceinline__ void epilogue_lds_wave_h2_interior(const f32x16 (&acc)[TI][TJ], float *slab, int row0, int col0,
                                                              const EpiArgs &a) {
    using S = EpiSlab<TJ>;
    using Wk = EpiWalk<TJ, 2>;
    static_assert(64 % Wk::LPR == 0 && Wk::PASSES * 64 == 32 * Wk::LPR, "one column per lane, whole passes");
    constexpr int RPP = 64 / Wk::LPR;                              // rows per pass
    const int lane = threadIdx.x & 63;
    const int rl0 = lane / Wk::LPR, cq = lane % Wk::LPR;
    const int col = col0 + cq * 8;
    const int nk_out = a.N >> 4, ks = col >> 4, hf = (col >> 3) & 1;
    const bool has_bias = a.bias != nullptr;
    float4 b0 = make_float4(0.f, 0.f, 0.f, 0.f), b1 = b0;
    if (has_bias) {
        b0 = *reinterpret_cast<const float4 *>(a.bias + col);
        b1 = *reinterpret_cast<const float4 *>(a.bias + col + 4);
    }
    const float *sp = slab + rl0 * S::LD + cq * 8;
    unsigned int nsat = 0;
#pragma unroll
    for (int i = 0; i < TI; ++i) {
        epilogue_slab_fill<TI, TJ>(acc, slab, i);
        epilogue_slab_sync();
        const int rb = row0 + i * 32;                              // a multiple of 32
        char *pb = a.packed + ((size_t)(rb >> 7) * nk_out + ks) * H2_BLOCK_B + ((rb & 96) + rl0) * X3_ROW_B;
#pragma unroll
        for (int p = 0; p < Wk::PASSES; ++p) {
            float4 v[2];
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                v[q] = *reinterpret_cast<const float4 *>(sp + p * RPP * S::LD + 4 * q);
                v[q].x *= a.scale; v[q].y *= a.scale; v[q].z *= a.scale; v[q].w *= a.scale;
                if (has_bias) {
                    const float4 b = q ? b1 : b0;
                    v[q].x += b.x; v[q].y += b.y; v[q].z += b.z; v[q].w += b.w;
                }
                v[q].x = act_const<ACT>(v[q].x); v[q].y = act_const<ACT>(v[q].y);
                v[q].z = act_const<ACT>(v[q].z); v[q].w = act_const<ACT>(v[q].w);
            }
            const unsigned int sat0 = h2_saturates(v[0]), sat1 = h2_saturates(v[1]);
            nsat += sat0 + sat1;
            f16x4 h0, l0, h1, l1;
            if (__builtin_amdgcn_ballot_w64((sat0 | sat1) != 0u)) {      // wave-uniform; rare by construction
                split2h<false>(v[0], h0, l0);
                split2h<false>(v[1], h1, l1);
            } else {                                                     // nothing to clamp in the whole pass
                split2h<false, false>(v[0], h0, l0);
                split2h<false, false>(v[1], h1, l1);
            }
            const int sw = ((p * RPP + rl0) >> 3) & 1;             // bit 3 of the row (rb adds multiples of 32)
            char *pp = pb + p * RPP * X3_ROW_B + ((hf ^ sw) << 4);
            f16x8 hh, ll;
#pragma unroll
            for (int e = 0; e < 4; ++e) { hh[e] = h0[e]; hh[4 + e] = h1[e]; ll[e] = l0[e]; ll[4 + e] = l1[e]; }
            *reinterpret_cast<f16x8 *>(pp) = hh;
            *reinterpret_cast<f16x8 *>(pp + X3_PLANE_B) = ll;
        }
        epilogue_slab_sync();
    }
    h2_post_saturated(nsat);
}

// MODE 2 (qkv scatter) with one column per lane.  Everything that depends on the column alone -- q or K / V, the cache,
// the head and the offset inside a cached row -- is taken once per tile.  A lane's rows advance by 64 / LPR per piece
// through the whole tile: one division gives (caption, beam) of its first row, the rest follow by addition.  With a
// caption map, the lane's TI x PASSES entries are requested BEFORE the transposition (as the bias is) instead of each one
// in front of its store; entries of rows past M are clamped into the map (loaded, never used).
template <int TI, int TJ, bool INTERIOR>
__device__ __forceinline__ void epilogue_lds_wave_qkv(const f32x16 (&acc)[TI][TJ], float *slab, int row0, int col0,
                                                      const EpiArgs &a) {
    using S = EpiSlab<TJ>;
    using Wk = EpiWalk<TJ, 1>;
    static_assert(64 % Wk::LPR == 0 && Wk::PASSES * 64 == 32 * Wk::LPR, "one column per lane, whole passes");
    constexpr int RPP = 64 / Wk::LPR, NP = TI * Wk::PASSES;
    const QkvScatter &sc = *a.sc;
    const int lane = threadIdx.x & 63;
    const int rl0 = lane / Wk::LPR, cq = lane % Wk::LPR;
    const int col = col0 + cq * 4;
    const bool col_live = INTERIOR || col < a.N;
    float4 bq = make_float4(0.f, 0.f, 0.f, 0.f);
    const bool has_bias = a.bias != nullptr;
    if (has_bias) bq = *reinterpret_cast<const float4 *>(a.bias + (INTERIOR ? col : min(col, a.N - 4)));
    const bool is_q = col < sc.d, is_v = col >= 2 * sc.d;
    float *cache = is_v ? sc.vc : sc.kc;
    const int hc = col - (is_v ? 2 * sc.d : sc.d), head = hc >> 6;
    const size_t cell = ((size_t)head * sc.ctx + sc.pos) * 64 + (hc & 63);      // inside a cached row
    const size_t row_el = (size_t)sc.heads * sc.ctx * 64;                        // elements per cached row
    const int beam = sc.beam, step_q = RPP / beam, step_r = RPP - step_q * beam;
    const int cap0 = (row0 + rl0) / beam, b0 = (row0 + rl0) - cap0 * beam;
    int cm[NP];                                                                  // the cache caption of every piece
    {
        const int cap_last = (a.M - 1) / beam;
        int cap = cap0, b = b0;
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            cm[k] = sc.cmap ? sc.cmap[INTERIOR ? cap : min(cap, cap_last)] : cap;
            cap += step_q; b += step_r;
            if (b >= beam) { b -= beam; ++cap; }
        }
    }
    const float *sp = slab + rl0 * S::LD + cq * 4;
    int b = b0;
#pragma unroll
    for (int i = 0; i < TI; ++i) {
        epilogue_slab_fill<TI, TJ>(acc, slab, i);
        epilogue_slab_sync();
#pragma unroll
        for (int p = 0; p < Wk::PASSES; ++p) {
            const int row = row0 + i * 32 + p * RPP + rl0;
            const int bcur = b;
            b += step_r;
            if (b >= beam) b -= beam;
            if (!INTERIOR && !(col_live && row < a.M)) continue;
            float4 v = *reinterpret_cast<const float4 *>(sp + p * RPP * S::LD);
            v.x *= a.scale; v.y *= a.scale; v.z *= a.scale; v.w *= a.scale;
            if (has_bias) { v.x += bq.x; v.y += bq.y; v.z += bq.z; v.w += bq.w; }
            if (is_q) {
                *reinterpret_cast<float4 *>(a.C + (size_t)row * a.ldc + col) = v;
            } else {
                const size_t srow = (size_t)cm[i * Wk::PASSES + p] * beam + bcur;
                const size_t el = srow * row_el + cell;
                if (sc.bf16) {
                    bf16x4 t;
                    t[0] = (__bf16)v.x; t[1] = (__bf16)v.y; t[2] = (__bf16)v.z; t[3] = (__bf16)v.w;
                    *reinterpret_cast<bf16x4 *>(reinterpret_cast<__bf16 *>(cache) + el) = t;
                } else
                    *reinterpret_cast<float4 *>(cache + el) = v;
            }
        }
        epilogue_slab_sync();
    }
}

// wave-uniform: the wavefront's TI x 32 rows and TJ x 32 columns lie inside the matrix and start at a multiple of 32 rows
template <int TI, int TJ>
__device__ __forceinline__ bool epilogue_interior(int row0, int col0, const EpiArgs &a) {
    return (row0 & 31) == 0 && row0 + TI * 32 <= a.M && col0 + TJ * 32 <= a.N;
}

// the activation code becomes a compile-time constant of the element loops (one switch per tile, not per element)
template <int TI, int TJ, int MODE, bool AHEAD = false>
__device__ __forceinline__ void epilogue_lds_dispatch(const f32x16 (&acc)[TI][TJ], float *slab, int row0, int col0,
                                                      const EpiArgs &a) {
    if constexpr (MODE == 1 && 64 % EpiWalk<TJ, 2>::LPR == 0 && EpiWalk<TJ, 2>::PASSES * 64 == 32 * EpiWalk<TJ, 2>::LPR) {
        if (a.fmt == PK_F16X2 && !a.resid_pk && epilogue_interior<TI, TJ>(row0, col0, a)) {
            switch (a.act) {
                case CAPDEC_ACT_GELU_NEW: epilogue_lds_wave_h2_interior<TI, TJ, CAPDEC_ACT_GELU_NEW>(acc, slab, row0, col0, a); break;
                case CAPDEC_ACT_QUICK_GELU: epilogue_lds_wave_h2_interior<TI, TJ, CAPDEC_ACT_QUICK_GELU>(acc, slab, row0, col0, a); break;
                case CAPDEC_ACT_RELU: epilogue_lds_wave_h2_interior<TI, TJ, CAPDEC_ACT_RELU>(acc, slab, row0, col0, a); break;
                case CAPDEC_ACT_TANH: epilogue_lds_wave_h2_interior<TI, TJ, CAPDEC_ACT_TANH>(acc, slab, row0, col0, a); break;
                default: epilogue_lds_wave_h2_interior<TI, TJ, CAPDEC_ACT_NONE>(acc, slab, row0, col0, a); break;   // (RESID_RELU acts on a residual only)
            }
            return;
        }
    }
    switch (a.act) {
        case CAPDEC_ACT_GELU_NEW: epilogue_lds_wave<TI, TJ, MODE, CAPDEC_ACT_GELU_NEW, AHEAD>(acc, slab, row0, col0, a); break;
        case CAPDEC_ACT_QUICK_GELU: epilogue_lds_wave<TI, TJ, MODE, CAPDEC_ACT_QUICK_GELU, AHEAD>(acc, slab, row0, col0, a); break;
        case CAPDEC_ACT_RELU: epilogue_lds_wave<TI, TJ, MODE, CAPDEC_ACT_RELU, AHEAD>(acc, slab, row0, col0, a); break;
        case CAPDEC_ACT_TANH: epilogue_lds_wave<TI, TJ, MODE, CAPDEC_ACT_TANH, AHEAD>(acc, slab, row0, col0, a); break;
        case CAPDEC_ACT_RESID_RELU: epilogue_lds_wave<TI, TJ, MODE, CAPDEC_ACT_RESID_RELU, AHEAD>(acc, slab, row0, col0, a); break;
        default: epilogue_lds_wave<TI, TJ, MODE, CAPDEC_ACT_NONE, AHEAD>(acc, slab, row0, col0, a); break;
    }
}

// block-level entry: G supplies WN, TI, TJ (wavefront w owns tile (w / WN, w % WN)); smem = the block's idle ring, at
// least NW * EpiSlab<TJ>::BYTES
template <class G, bool AHEAD = false>
__device__ __forceinline__ void epilogue_lds(const f32x16 (&acc)[G::TI][G::TJ], char *smem, const EpiArgs &a) {
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wm = wave / G::WN, wn = wave % G::WN;
    float *slab = reinterpret_cast<float *>(smem + wave * EpiSlab<G::TJ>::BYTES);
    const int row0 = a.m0 + wm * G::TI * 32, col0 = a.n0 + wn * G::TJ * 32;
    if (a.packed) epilogue_lds_dispatch<G::TI, G::TJ, 1>(acc, slab, row0, col0, a);
    else if (a.sc && a.sc->kc) {
        if constexpr (AHEAD) {
            if (epilogue_interior<G::TI, G::TJ>(row0, col0, a)) epilogue_lds_wave_qkv<G::TI, G::TJ, true>(acc, slab, row0, col0, a);
            else epilogue_lds_wave_qkv<G::TI, G::TJ, false>(acc, slab, row0, col0, a);
        } else
            epilogue_lds_wave<G::TI, G::TJ, 2, CAPDEC_ACT_NONE, AHEAD>(acc, slab, row0, col0, a);
    } else epilogue_lds_dispatch<G::TI, G::TJ, 0, AHEAD>(acc, slab, row0, col0, a);
}

}  // namespace capdec
