// Round 4: the fp32-accurate three-product GEMM (format PK_F16X2, see gemm_f16x2.hip) as ONE 8-wavefront block per CU
// whose two wavefronts per SIMD alternate between a load phase and a matrix phase ("ping-pong"):
//     C[M,N] = epi( A[M,K] . Bt[N,K]^T )
//
// Why: the round-2 / round-3 kernels put two INDEPENDENT 4-wavefront blocks on a CU.  Each wavefront interleaves its own
// fragment reads and LDS-DMA pieces with its MFMAs and meets the other three wavefronts of its block at an s_barrier every
// k-step, while its SIMD partner -- a wavefront of the other block, at an arbitrary phase -- competes for the same matrix
// pipe: the SQ counters show that pipe busy 50-54 % of the cycles and the waves parked or issue-stalled the rest of the
// time, with random and with zero operands, capped and uncapped clocks alike (profiles/r3_pmc_sq_gemm.txt).  Here the two
// wavefronts of a SIMD belong to the SAME block and are kept half a k-step apart by the block's own barriers: while one
// group of four wavefronts issues nothing but MFMAs (at raised priority), the other group issues the ds_reads of its next
// fragments and its share of the LDS-DMA pieces; at the barrier they swap roles.  The matrix pipe of every SIMD is handed
// from one wavefront to the other without either of them having to hide its own memory operations under its own MFMAs.
// (The CDNA4 guide's plain-HIP bf16 GEMM template is built the same way; this is that structure for the two-plane
//  operands and the three products of the f16x2 scheme, with the packed tile-major operands of bf16x3.h.)
//
// Geometry (PGeo): WM x WN = 8 wavefronts, wave tile TI x TJ blocks of 32 x 32; wavefronts 0-3 form group 0, 4-7 group 1
// (the hardware places wavefront w and w + 4 of a block on the same SIMD).  A stage of the LDS ring holds one k-step
// (16 k, both planes) of the block tile's A and B rows in 1 KB pieces (32 rows x 32 B of one plane), chunk-major like
// gemm_h2w.hip; the ring has NS stages and the DMA runs D = NS - 2 k-steps ahead.
//
// Timeline (half-phases h, one s_barrier between consecutive ones; group 0 is at LOAD(kt) when h = 2 kt, group 1 when
// h = 2 kt + 1, each group's MMA(kt) is the half-phase after its LOAD(kt)):
//   LOAD(kt): ds_read the fragments of tile kt from stage kt % NS; send this wavefront's pieces of tile kt + D to stage
//             (kt + D) % NS; s_waitcnt vmcnt(PPW (D - 1))  -- this wavefront's pieces of tile kt + 1 have landed.
//   MMA(kt):  s_waitcnt lgkmcnt(0); s_setprio 1; the 3 TI TJ MFMAs of tile kt; s_setprio 0.
// Read-after-DMA: a fragment read of tile kt + 1 (group 0: h = 2 kt + 2, group 1: h = 2 kt + 3) comes after every
// wavefront's counted wait for that tile (group 0: end of h = 2 kt, group 1: end of h = 2 kt + 1) AND a barrier.
// DMA-after-read: stage (kt + D) % NS last held tile kt + D - NS, whose last reads (group 1, h = 2 (kt + D - NS) + 1) were
// retired by the lgkmcnt(0) at the start of h = 2 (kt + D - NS) + 2; the earliest overwrite is group 0's at h = 2 kt, and
// 2 (kt + D - NS) + 2 < 2 kt  <=>  D <= NS - 2.
#include <algorithm>
#include <cstdlib>

#include "bf16x3.h"
#include "gemm_epilogue_lds.h"
#include "gemm_packed.h"

namespace capdec {

template <int WM_, int WN_, int TI_, int TJ_, int NS_, bool TWOACC_>
struct PGeo {
    static constexpr int WM = WM_, WN = WN_, TI = TI_, TJ = TJ_, NS = NS_;
    static constexpr bool TWOACC = TWOACC_;       // two accumulator sets (any weights) / one (weights with max |w| < 16)
    static constexpr int NW = WM * WN, THREADS = 64 * NW, MINW = 2;
    static constexpr int BM = WM * TI * 32, BN = WN * TJ * 32;
    static constexpr int CA = BM / 32, CB = BN / 32;
    static constexpr int PIECES = 2 * (CA + CB), PPW = (PIECES + NW - 1) / NW;   // (a remainder is padded with duplicates)
    static constexpr int STAGE_B = PIECES * 1024;
    static constexpr int SMEM_B = NS * STAGE_B;
    static constexpr int D = NS - 2;
    static_assert(NW == 8, "two groups of four wavefronts");
    static_assert(D >= 1 && PPW * D < 64, "ring depth / vmcnt range");
    static_assert(SMEM_B <= 160 * 1024, "LDS");
};

// acc (and ac for TWOACC) in the TR layout of gemm_epilogue.h when TR, the plain MFMA layout otherwise
// (ks0, nks: the k-steps [ks0, ks0 + nks) of the product -- split-K; nks < 0: all of them)
template <class G, bool TR>
__device__ __forceinline__ void pp_mainloop(const _Float16 *__restrict__ Apk, const _Float16 *__restrict__ Bpk, int K,
                                            int tm, int tn, int chunksA, int chunksB, char *smem,
                                            f32x16 (&acc)[G::TI][G::TJ], f32x16 (&ac)[G::TWOACC ? G::TI : 1][G::TWOACC ? G::TJ : 1],
                                            int ks0 = 0, int nks = -1) {
    constexpr int TI = G::TI, TJ = G::TJ, NS = G::NS, PPW = G::PPW, SB = G::STAGE_B, D = G::D;
    const int t = threadIdx.x;
    const int lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int wm = wave / G::WN, wn = wave % G::WN, grp = wave >> 2;
    const int half = lane >> 5, l32 = lane & 31;
    const int nkf = K / X3_BK;                     // k-steps of the whole K (panel stride)
    const int nk = nks < 0 ? nkf : nks;            // k-steps of THIS block
    // ---- LDS-DMA: piece p of a stage = plane (p & 1) of chunk (p >> 1); chunks 0 .. CA-1 = the A rows of the block tile,
    // CA .. CA+CB-1 its B rows.  Global chunk g of a packed operand = piece (g & 3) of each plane of its 128-row tile g >> 2.
    const char *src[PPW];
    int dofs[PPW];
#pragma unroll
    for (int e = 0; e < PPW; ++e) {
        const int p = min(wave * PPW + e, G::PIECES - 1), c = p >> 1, pl = p & 1;
        const bool isA = c < G::CA;
        const int g = isA ? min(tm * G::CA + c, chunksA - 1) : min(tn * G::CB + (c - G::CA), chunksB - 1);
        const char *base = reinterpret_cast<const char *>(isA ? Apk : Bpk);
        src[e] = base + ((size_t)(g >> 2) * nkf + ks0) * H2_BLOCK_B + pl * X3_PLANE_B + (g & 3) * 1024 + lane * 16;
        dofs[e] = p * 1024;
    }
#define P_DMA(stage, ks_)                                                                                        \
    {                                                                                                            \
        _Pragma("unroll") for (int e = 0; e < PPW; ++e)                                                          \
            __builtin_amdgcn_global_load_lds((glb_void *)(src[e] + (size_t)(ks_) * H2_BLOCK_B),                 \
                                             (lds_void *)(smem + (stage) * SB + dofs[e]), 16, 0, 0);           \
    }
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < TJ; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    if constexpr (G::TWOACC) {
#pragma unroll
        for (int i = 0; i < TI; ++i)
#pragma unroll
            for (int j = 0; j < TJ; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) ac[i][j][r] = 0.f;
    }
    const int swz = ((half ^ ((l32 >> 3) & 1)) << 4);
    const int a_rd = (2 * wm * TI) * 1024 + l32 * X3_ROW_B + swz;                  // chunk wm TI + i, plane p: + (2 i + p) KB
    const int b_rd = (2 * (G::CA + wn * TJ)) * 1024 + l32 * X3_ROW_B + swz;
    f16x8 fa[TI][2], fb[TJ][2];
#define P_READ(stage)                                                                                            \
    {                                                                                                            \
        const char *rs = smem + (stage) * SB;                                                                    \
        _Pragma("unroll") for (int j = 0; j < TJ; ++j) {                                                         \
            fb[j][0] = *reinterpret_cast<const f16x8 *>(rs + b_rd + (2 * j) * 1024);                             \
            fb[j][1] = *reinterpret_cast<const f16x8 *>(rs + b_rd + (2 * j + 1) * 1024);                         \
        }                                                                                                        \
        _Pragma("unroll") for (int i = 0; i < TI; ++i) {                                                         \
            fa[i][0] = *reinterpret_cast<const f16x8 *>(rs + a_rd + (2 * i) * 1024);                             \
            fa[i][1] = *reinterpret_cast<const f16x8 *>(rs + a_rd + (2 * i + 1) * 1024);                         \
        }                                                                                                        \
    }
#define P_MM1(x, y, c) __builtin_amdgcn_mfma_f32_32x32x16_f16(x, y, c, 0, 0, 0)
#define P_MM(x, y, c) (TR ? P_MM1(y, x, c) : P_MM1(x, y, c))
#define P_BARRIER()                          \
    asm volatile("" ::: "memory");           \
    __builtin_amdgcn_s_barrier();            \
    asm volatile("" ::: "memory");           \
    __builtin_amdgcn_sched_barrier(0);

    // prologue: tiles 0 .. D-1 in flight, tile 0 landed everywhere; group 1 then waits one barrier more (half a k-step)
#pragma unroll
    for (int s = 0; s < D; ++s) P_DMA(s, min(s, nk - 1))
    __builtin_amdgcn_s_waitcnt(waitcnt_imm(PPW * (D - 1), 15));
    P_BARRIER()
    if (grp == 1) { P_BARRIER() }
    int s0 = 0, sd = D % NS;                     // kt % NS, (kt + D) % NS
    for (int kt = 0; kt < nk; ++kt) {
        // ---- LOAD(kt)
        P_READ(s0)
        P_DMA(sd, min(kt + D, nk - 1))
        asm volatile("" ::: "memory");
        __builtin_amdgcn_s_waitcnt(waitcnt_imm(PPW * (D - 1), 15));
        P_BARRIER()
        // ---- MMA(kt)
        __builtin_amdgcn_s_waitcnt(waitcnt_imm(63, 0));
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(1);
        if constexpr (G::TWOACC) {
#pragma unroll
            for (int i = 0; i < TI; ++i)
#pragma unroll
                for (int j = 0; j < TJ; ++j) ac[i][j] = P_MM(fa[i][1], fb[j][0], ac[i][j]);
#pragma unroll
            for (int i = 0; i < TI; ++i)
#pragma unroll
                for (int j = 0; j < TJ; ++j) acc[i][j] = P_MM(fa[i][0], fb[j][0], acc[i][j]);
#pragma unroll
            for (int i = 0; i < TI; ++i)
#pragma unroll
                for (int j = 0; j < TJ; ++j) ac[i][j] = P_MM(fa[i][0], fb[j][1], ac[i][j]);
        } else {
            f16x8 bs[TJ];
#pragma unroll
            for (int j = 0; j < TJ; ++j) bs[j] = fb[j][0] * (_Float16)H2_LO_SCALE;
            // term-major over the whole wave tile: an accumulator comes up again only after TI TJ other MFMAs
#pragma unroll
            for (int i = 0; i < TI; ++i)
#pragma unroll
                for (int j = 0; j < TJ; ++j) acc[i][j] = P_MM(fa[i][1], fb[j][0], acc[i][j]);
#pragma unroll
            for (int i = 0; i < TI; ++i)
#pragma unroll
                for (int j = 0; j < TJ; ++j) acc[i][j] = P_MM(fa[i][0], bs[j], acc[i][j]);
#pragma unroll
            for (int i = 0; i < TI; ++i)
#pragma unroll
                for (int j = 0; j < TJ; ++j) acc[i][j] = P_MM(fa[i][0], fb[j][1], acc[i][j]);
        }
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_sched_barrier(0);
        P_BARRIER()
        s0 = s0 + 1 == NS ? 0 : s0 + 1;
        sd = sd + 1 == NS ? 0 : sd + 1;
    }
    if (grp == 0) { P_BARRIER() }
    __builtin_amdgcn_s_waitcnt(waitcnt_imm(0, 15));            // clamped tail pieces must land before the ring is reused
    P_BARRIER()
#undef P_DMA
#undef P_READ
#undef P_MM1
#undef P_MM
#undef P_BARRIER
}

template <class G>
__device__ __forceinline__ void pp_join(f32x16 (&am)[G::TI][G::TJ], const f32x16 (&ac)[G::TWOACC ? G::TI : 1][G::TWOACC ? G::TJ : 1]) {
    if constexpr (G::TWOACC) {
#pragma unroll
        for (int i = 0; i < G::TI; ++i)
#pragma unroll
            for (int j = 0; j < G::TJ; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) am[i][j][r] = fmaf(ac[i][j][r], 1.0f / H2_LO_SCALE, am[i][j][r]);
    }
}

// persistent form: grid = min(tiles, CUs) blocks, block b walks tiles b, b + grid, ...
template <class G>
__global__ __launch_bounds__(G::THREADS, G::MINW) void gemm_pp_kernel(const _Float16 *__restrict__ Apk,
                                                                     const _Float16 *__restrict__ Bpk, float *C, int ldc,
                                                                     int M, int N, int K, const float *__restrict__ bias,
                                                                     const float *resid, int ldr, int act, int tiles_m,
                                                                     int tiles_n, char *packed_out, float scale, QkvScatter sc) {
    __shared__ __attribute__((aligned(16))) char smem[G::SMEM_B];
    const int ntiles = tiles_m * tiles_n;
    const int chunksA = ((M + 127) >> 7) * 4, chunksB = ((N + 127) >> 7) * 4;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        int tm, tn;
        tile_coords(tiles_m, tiles_n, tm, tn, tile);
        f32x16 acc[G::TI][G::TJ], ac[G::TWOACC ? G::TI : 1][G::TWOACC ? G::TJ : 1];
        pp_mainloop<G, true>(Apk, Bpk, K, tm, tn, chunksA, chunksB, smem, acc, ac);
        pp_join<G>(acc, ac);
        EpiArgs ea;
        ea.C = C; ea.ldc = ldc; ea.M = M; ea.N = N; ea.m0 = tm * G::BM; ea.n0 = tn * G::BN;
        ea.bias = bias; ea.act = act; ea.scale = scale; ea.ldr = ldr;
        ea.packed = packed_out;
        if (packed_out) ea.resid_pk = reinterpret_cast<const char *>(resid);      // (with packed_out, `resid` is PACKED)
        else ea.resid = resid;
        ea.sc = &sc;
        epilogue_lds<G>(acc, smem, ea);
        slab_release(tile + (int)gridDim.x < ntiles);
    }
}

// split-K for grids that leave most CUs idle (the N = 768 projections of a few thousand rows): block b = (tile, slice)
// walks k-steps [slice nks, (slice + 1) nks) and writes its raw fp32 partial tile to part[slice][M][N]; the slices are
// summed in a fixed order by launch_splitk_reduce (gemm_bf16x3.hip), which applies the epilogue -- and the LayerNorm that
// follows, when there is one
template <class G>
__global__ __launch_bounds__(G::THREADS, G::MINW) void gemm_pp_splitk_kernel(const _Float16 *__restrict__ Apk,
                                                                            const _Float16 *__restrict__ Bpk, float *part,
                                                                            int M, int N, int K, int tiles_m, int tiles_n,
                                                                            int S, float scale) {
    __shared__ __attribute__((aligned(16))) char smem[G::SMEM_B];
    const int ntiles = tiles_m * tiles_n;
    const int slice = blockIdx.x / ntiles;
    int tm, tn;
    tile_coords(tiles_m, tiles_n, tm, tn, blockIdx.x - slice * ntiles);
    const int nks = K / X3_BK / S;
    f32x16 acc[G::TI][G::TJ], ac[G::TWOACC ? G::TI : 1][G::TWOACC ? G::TJ : 1];
    pp_mainloop<G, true>(Apk, Bpk, K, tm, tn, ((M + 127) >> 7) * 4, ((N + 127) >> 7) * 4, smem, acc, ac, slice * nks, nks);
    pp_join<G>(acc, ac);
    EpiArgs ea;
    ea.C = part + (size_t)slice * M * N; ea.ldc = N; ea.M = M; ea.N = N; ea.m0 = tm * G::BM; ea.n0 = tn * G::BN;
    ea.scale = scale;
    epilogue_lds<G>(acc, smem, ea);
}

using P256x128 = PGeo<4, 2, 2, 2, 5, true>;       // 8 waves x (64 x 64), two accumulator sets, 24 KB stages, 120 KB
using P256x192s = PGeo<4, 2, 2, 3, 4, false>;     // 8 waves x (64 x 96), ONE accumulator set (two would spill), 28 KB stages, 112 KB
// (A 256 x 256 one-set tile won the isolated micro-benchmark -- +12 % on mlp.c_fc at 25 000 rows -- and lost 2 % inside the
//  decode loop; the remedy its phase stamps suggested, storing tile i while tile i + 1's MFMAs run, needs a second set of 128
//  accumulator registers or 256 KB of LDS to park them.  It, the one-set 256 x 128 and the 128 x 256 forms are gone:
//  profiles/r4_gemm_pp.txt, docs/rounds.md.)

template <class G>
static int launch_pp(hipStream_t st, const void *Apacked, const void *Bpacked, float *C, int ldc, int M, int N, int K,
                     const GemmEpilogue &epi, const GemmPlan &plan, const PackedArgs &a) {
    CAPDEC_CHECK(plan.bm == G::BM && plan.bn == G::BN && plan.threads == G::THREADS && plan.ns == G::NS,
                 "gemm_pp: the plan names another geometry");
    const int tiles_m = (M + G::BM - 1) / G::BM, tiles_n = (N + G::BN - 1) / G::BN;
    const float kscale = G::TWOACC ? 1.0f : 1.0f / H2_LO_SCALE;      // (single-set geometries scale the result by 2^-11)
    if (plan.S > 1) {
        hipLaunchKernelGGL((gemm_pp_splitk_kernel<G>), dim3(plan.grid), dim3(G::THREADS), 0, st, (const _Float16 *)Apacked,
                           (const _Float16 *)Bpacked, a.part, M, N, K, tiles_m, tiles_n, plan.S, kscale);
        CAPDEC_HIP(hipGetLastError());
        return launch_splitk_reduce(st, a.part, plan.S, M, N, epi, C, ldc, PK_F16X2);
    }
    hipLaunchKernelGGL((gemm_pp_kernel<G>), dim3(plan.grid), dim3(G::THREADS), 0, st, (const _Float16 *)Apacked,
                       (const _Float16 *)Bpacked, C, ldc, M, N, K, epi.bias, a.resid, epi.ldr, epi.act, tiles_m, tiles_n,
                       (char *)epi.packed_out, kscale, a.sc);
    CAPDEC_HIP(hipGetLastError());
    return 0;
}

// plan.geo: 10 = 256x128 (two accumulator sets), 14 = 256x192 (one set: weights with |w| < 16), chosen by gemm_plan.h
int launch_gemm_pp(hipStream_t st, const void *Apacked, const void *Bpacked, float *C, int ldc, int M, int N, int K,
                   const GemmEpilogue &epi, const GemmPlan &plan) {
    PackedArgs a;
    CAPDEC_TRY(packed_args("gemm_f16x2p", epi, plan, C, ldc, M, N, K, &a));
    CAPDEC_CHECK(plan.vec4, "gemm_pp: needs the float4 epilogue");
    if (plan.geo == 10) return launch_pp<P256x128>(st, Apacked, Bpacked, C, ldc, M, N, K, epi, plan, a);
    CAPDEC_CHECK(plan.geo == 14, "gemm_pp: unknown geometry");
    return launch_pp<P256x192s>(st, Apacked, Bpacked, C, ldc, M, N, K, epi, plan, a);
}

CAPDEC_SAT_ACCESSOR(sat_count_gemm_pp)

}  // namespace capdec
