// The launch plan of a packed GEMM: which kernel, how many K slices, how many blocks, how large the split-K workspace.
// gemm_plan() is the ONE place where these are decided -- a pure host function of the shape, a few flags and the Tuning (no
// statics, no environment, no HIP), so its rules are tested on any machine (tests/test_gemm_plan.py).  gemm_dispatch.hip
// computes the plan once per launch, sizes the workspace from it and hands it to the launcher, which only checks its
// arguments and launches what the plan names.
#pragma once
#include <algorithm>
#include <cstddef>

#include "config.h"

namespace capdec {

// operand formats (the values of PackFmt, bf16x3.h)
constexpr int PLAN_BF16X3 = 0, PLAN_F16X2 = 1, PLAN_BF16X1 = 2, PLAN_F16X1 = 3;
constexpr int PLAN_BK = 16;                    // k per k-step (X3_BK)
// blocks the chip runs at a time, per kernel family: 256 CUs x the blocks of that family a CU holds
constexpr int PLAN_CUS = 256;
constexpr int PLAN_SLOTS_PP = PLAN_CUS;        // ping-pong: ONE 8-wavefront block per CU
constexpr int PLAN_SLOTS_H2W = 2 * PLAN_CUS;   // wide tiles (and the 128 x 128 two-plane kernel by default: Tuning::h2_persist)
// one-plane vec4 kernel: ring of 3, THREE blocks per CU where the two-plane kernel has two (measured +3 % at 25 000 rows,
// +1.3 % on the greedy bf16 workload against two) -- 768 slots at the default h2_persist of 512
constexpr int PLAN_X1_VEC4_BLOCKS_NUM = 3, PLAN_X1_VEC4_BLOCKS_DEN = 2;

enum GemmKernel {
    GK_H2P, GK_H2P_SPLITK,       // 128 x 128, two fp16 planes (gemm_f16x2.hip)
    GK_X1, GK_X1_SPLITK,         // 128 x 128, one 16-bit plane (gemm_f16x2.hip)
    GK_X3P, GK_X3P_SPLITK,       // 128 x 128, three bf16 planes (gemm_bf16x3.hip)
    GK_H2W,                      // wide tile, one accumulator set (gemm_h2w.hip)
    GK_PP, GK_PP_SPLITK,         // ping-pong (gemm_pp.hip)
};

struct GemmPlanIn {
    int fmt = PLAN_F16X2;        // operand format of both operands
    int M = 0, N = 0, K = 0;     // K % 64 == 0
    bool vec4 = false;           // float4 epilogue possible: N % 4 == 0 and 16-byte aligned C / bias / residual rows (gemm_vec4)
    bool wide_ok = false;        // two-plane: B is a weight with max |w| < 16 (the single-accumulator kernels are exact)
    bool invariant = false;      // batch-invariant mode: no planner, no split-K
    bool split_ok = false;       // the caller lets this launch split K (gemm_dispatch.hip then attaches the workspace)
    bool packed_out = false, resid_packed = false, scatter = false;      // GemmEpilogue: packed_out, resid_packed, qkv_scatter
    const Tuning *tune = nullptr;
};

struct GemmPlan {
    int kernel = GK_H2P;
    int geo = 0;                 // 0 = 128 x 128; 2 = W256x128, 8 = W128x192 (gemm_h2w.hip); 10 = P256x128, 14 = P256x192s (gemm_pp.hip)
    int bm = 128, bn = 128;      // block tile
    int threads = 256;
    int ns = 0;                  // ring depth where it is a template argument (0: it is not)
    bool vec4 = false;           // float4 epilogue (a template argument of the 128 x 128 kernels)
    int S = 1;                   // K slices
    int grid = 0;                // blocks
    size_t ws_bytes = 0;         // S * M * N * 4 when S > 1
};

inline int plan_tiles(int M, int N, int bm, int bn) { return ((M + bm - 1) / bm) * ((N + bn - 1) / bn); }

// K slices of the 128 x 128 kernels for a [M, N, K] problem (1 = no split).  Two under-filled regimes (the chip runs 512 blocks
// at a time):
//  (a) M <= 512 rows (at most four tile rows: the decode of small batches): S depends on K ONLY -- the largest divisor of
//      the k-step count that leaves >= 8 (an even number of) k-steps per slice -- so a row's result is bit-identical for
//      every batch size in this regime;
//  (b) larger M whose grid is still at most HALF of the chip (<= 256 tiles: the N = 768 projections at a few thousand
//      rows, e.g. 625 captions x beam 5 = 3125 rows -> 150 tiles): the largest S with tiles x S <= 512 and >= 16 (even)
//      k-steps per slice.  mlp.c_proj (K = 3072, 150 tiles walking 192 k-steps each): 58 -> ~35 us.
// Across a regime / S boundary the fp32 summation order of a row changes (round-off level; the unsplit regime above is
// again batch-size independent).  CAPDEC_SPLITK=0 disables both, CAPDEC_SPLITK_MID=0 only (b).
// (Tried and removed: cutting only the tiles of the last, partly filled round of a > 512-tile grid into K-slices inside
//  the same launch, summed by the last piece to arrive at a per-tile counter.  Device-scope fences cost an L2 write-back +
//  invalidate per piece; with sc1 write-through dumps instead, the dump + arrival + re-read still cost more than the
//  round they save: 3125 x 3072 x 768: 55 -> 68 us, 25000 x 768 x 3072: 393 -> 440 us.  DESIGN.md section 5.)
// (Also decode.hip's condition for the qkv scatter epilogue, which needs an unsplit launch: this rule says 1.)
inline int plan_splitk_128(int M, int N, int K, const Tuning &t) {
    const int nk = K / PLAN_BK;
    if (!t.splitk || N % 4 != 0) return 1;
    int best = 1;
    if (M <= 512) {
        for (int s = 2; s <= nk / 8; ++s)
            if (nk % s == 0 && (nk / s) % 2 == 0) best = s;
        return best;
    }
    if (!t.splitk_mid) return 1;
    const int tiles = plan_tiles(M, N, 128, 128);
    if (tiles > PLAN_CUS) return 1;
    for (int s = 2; s <= nk / 16 && tiles * s <= 2 * PLAN_CUS; ++s)
        if (nk % s == 0 && (nk / s) % 2 == 0) best = s;
    return best;
}

inline void plan_pp_tile(int geo, int &bm, int &bn) {
    bm = 256;
    bn = geo == 14 ? 192 : 128;
}

// K slices for a ping-pong launch (1 = none): grids of at most a third of the CUs are cut along K -- the largest S with
// tiles x S <= 256 that divides the k-steps and leaves >= 8 per slice.  (625 captions x beam 5 = 3125 rows: the N = 768
// projections are 78 tiles of 256 x 128 -> S = 3, 234 blocks.)
// (M <= 512 -- the small-batch regime whose results must not depend on the batch size -- is never cut here: the planner
//  does not use these kernels there, and a FORCED geometry, CAPDEC_H2W >= 10, then runs unsplit whatever M is)
inline int plan_splitk_pp(int geo, int M, int N, int K) {
    int bm, bn;
    plan_pp_tile(geo, bm, bn);
    const int tiles = plan_tiles(M, N, bm, bn), nk = K / PLAN_BK;
    if (N % 4 != 0 || tiles * 3 > PLAN_SLOTS_PP || M <= 512) return 1;
    int best = 1;
    for (int s = 2; tiles * s <= PLAN_SLOTS_PP && s <= nk / 8; ++s)
        if (nk % s == 0) best = s;
    return best;
}

// Which kernel for an f16x2 GEMM [M, N, K] of more than 512 rows: 0 = the 128 x 128 / wide-tile kernels, else a ping-pong
// geometry.  The chip runs these GEMMs at its power limit (sustained launches of the old and the new structure reach the
// same k-steps per second per CU: profiles/r4_gemm_pp.txt), so the ping-pong kernels are used only where they were MEASURED
// faster inside the decode loop: mid-size launches (513 .. 8191 rows, about one round), with the tile whose grid fills the
// 256 CUs best -- 256 x 192 for mlp.c_fc (3125 rows: 208 blocks instead of 400 half-speed ones), 256 x 128 cut along K for
// the N = 768 projections.  Large launches (>= 8192 rows, several rounds) stay with the 128 x 128 kernels: inside the
// 5000-caption decode loop a 256 x 256 tile came out 2 % slower than they are.
inline int plan_pp_geo(int M, int N, int K, bool wide_ok, bool can_split) {
    if (M >= 8192) return 0;
    auto blocks_pp = [&](int geo) {
        int bm, bn;
        plan_pp_tile(geo, bm, bn);
        return (long)plan_tiles(M, N, bm, bn) * (can_split ? plan_splitk_pp(geo, M, N, K) : 1);
    };
    // one round of blocks that fills >= 75 % of the CUs: prefer the larger tile
    if (wide_ok && N >= 2048) {
        const long b14 = blocks_pp(14);
        if (b14 <= PLAN_SLOTS_PP && b14 >= 192 && N % 192 == 0) return 14;
    }
    const long b10 = blocks_pp(10);
    if (b10 <= PLAN_SLOTS_PP && b10 >= 192 && N <= 1024) return 10;
    return 0;
}

// Which kernel for an f16x2 GEMM [M, N] whose grid is not split along K: 0 = the 128 x 128 two-accumulator kernel, else a
// wide-tile geometry.  Estimated time = (full rounds of 512 blocks + what the partly filled last round costs) x tile area /
// relative loop efficiency; a block alone on its CU runs ~1.64x faster than one of a pair (measured: one block per CU =
// 0.82 of two), so a last round of <= 256 tiles costs 0.61.  The wide tiles only win where they remove a round: at 25 000
// rows the estimates tie (measured: within +-3 %, profiles/r3_gemm_geometries.txt) and the 128 x 128 kernel stays; at a few
// thousand rows mlp.c_fc (600 tiles of 128x128 = 1.17 rounds) takes the 128x192 tile (400 tiles, one round).
inline int plan_h2w_geo(int M, int N) {
    auto cost = [&](int bm, int bn, double eff) {
        const long tiles = plan_tiles(M, N, bm, bn);
        const long full = tiles / PLAN_SLOTS_H2W, rem = tiles % PLAN_SLOTS_H2W;
        const double rounds = (double)full + (rem == 0 ? 0.0 : rem <= PLAN_CUS ? 0.61 : 1.0);
        return rounds * bm * bn / eff;
    };
    const double c0 = cost(128, 128, 1.0), c8 = cost(128, 192, 1.04), c2 = cost(256, 128, 1.05);
    int best = 0;
    double cb = c0 * 0.97;                       // the wide kernel must be worth >= 3 %
    if (c8 < cb) { best = 8; cb = c8; }
    if (c2 < cb) { best = 2; cb = c2; }
    return best;
}

// Persistent form: at most `slots` blocks, block b walks tiles b, b + grid, ... -- for grids of up to four rounds, where the
// partly filled last round matters (625 captions: mlp.c_fc 600 tiles, 80 -> 70 us inside the decode loop); larger grids keep
// one block per tile (the dispatcher balances them: within noise either way at 25 000 rows).  slots == 0: never
inline int plan_persistent_grid(int tiles, int slots) {
    return (slots > 0 && tiles <= 4 * slots) ? std::min(tiles, slots) : tiles;
}

inline GemmPlan gemm_plan(const GemmPlanIn &in) {
    const Tuning &t = *in.tune;
    const int M = in.M, N = in.N, K = in.K;
    GemmPlan p;
    p.vec4 = in.vec4;
    auto finish = [&](int kernel, int split_kernel, int S, int slots) {
        const int tiles = plan_tiles(M, N, p.bm, p.bn);
        p.S = S;
        p.kernel = S > 1 ? split_kernel : kernel;
        p.grid = S > 1 ? tiles * S : plan_persistent_grid(tiles, slots);
        p.ws_bytes = S > 1 ? (size_t)S * M * N * sizeof(float) : 0;
        return p;
    };
    // a split launch sums raw fp32 partial tiles in a reduce pass with a float4 epilogue that knows neither the packed
    // residual nor the qkv scatter; the batch-invariant mode never splits
    const bool can_split = in.split_ok && in.vec4 && !in.invariant && !in.resid_packed && !in.scatter;
    const int S128 = can_split ? plan_splitk_128(M, N, K, t) : 1;
    if (in.fmt == PLAN_BF16X3) return finish(GK_X3P, GK_X3P_SPLITK, S128, 0);
    if (in.fmt != PLAN_F16X2) {
        // (Round 5 measured the ping-pong tiles of gemm_pp.hip under one-plane operands -- 256 x 256 / 256 x 192 / 256 x 128,
        //  rings of 4-5 and of 5-6 stages -- against this kernel inside the decode loop: 12-15 % SLOWER per launch at 5000
        //  rows, 25 % at 25 000 (profiles/r5_x1_pingpong_ab.txt); the variant was removed again.)
        // a slice is a whole, even number of two-k-step stages
        const int S = (S128 > 1 && (K / PLAN_BK / S128) % 4 == 0) ? S128 : 1;
        p.ns = S > 1 ? 4 : in.vec4 ? 3 : 4;
        const int slots = in.vec4 ? t.h2_persist * PLAN_X1_VEC4_BLOCKS_NUM / PLAN_X1_VEC4_BLOCKS_DEN : t.h2_persist;
        return finish(GK_X1, GK_X1_SPLITK, S, slots);
    }
    // ---- two fp16 planes: ping-pong, then split-K, then wide tile, then the (persistent) 128 x 128 kernel.  Everything but
    // the last needs the float4 epilogue; the batch-invariant mode takes the last whatever M is
    const bool wide_ok = in.wide_ok && !in.invariant;
    if (in.vec4 && !in.invariant) {
        // ping-pong: forced (CAPDEC_H2W >= 10) or where the planner expects a gain (mid-size launches; the small-batch regime
        // M <= 512 keeps its batch-size independent split-K)
        const bool can_split_pp = can_split && !in.packed_out;
        int geo = 0;
        if (t.h2w >= 10) geo = (t.h2w == 10 || wide_ok) ? t.h2w : 0;
        else if (t.h2w == 1 && t.pp && M > 512) geo = plan_pp_geo(M, N, K, wide_ok, can_split_pp);
        if (geo) {
            p.geo = geo;
            plan_pp_tile(geo, p.bm, p.bn);
            p.threads = 512;
            p.ns = geo == 14 ? 4 : 5;
            return finish(GK_PP, GK_PP_SPLITK, can_split_pp ? plan_splitk_pp(geo, M, N, K) : 1, PLAN_SLOTS_PP);
        }
    }
    p.ns = 4;
    if (S128 > 1) return finish(GK_H2P, GK_H2P_SPLITK, S128, 0);
    if (in.vec4 && wide_ok && t.h2w >= 1 && t.h2w < 10 && !in.scatter) {      // wide single-accumulator tiles where they remove a round
        const int geo = t.h2w >= 2 ? t.h2w : plan_h2w_geo(M, N);
        if (geo) {
            p.geo = geo;
            p.bm = geo == 2 ? 256 : 128;
            p.bn = geo == 2 ? 128 : 192;
            p.ns = geo == 2 ? 3 : 4;
            return finish(GK_H2W, GK_H2W, 1, PLAN_SLOTS_H2W);
        }
    }
    return finish(GK_H2P, GK_H2P_SPLITK, 1, t.h2_persist);      // CAPDEC_H2_PERSIST=<blocks> (0 = one block per tile)
}

}  // namespace capdec
