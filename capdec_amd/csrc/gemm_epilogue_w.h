// The lm_head epilogue of the wide-tile GEMM kernel (gemm_h2w.hip): a wavefront owns TI x TJ blocks of 32 x 32 of the
// block tile; G supplies WN (wavefronts along N), TI, TJ, BM / BN / NW / SMEM_B.  (The plain outputs of the wide tiles
// leave through the coalesced epilogue of gemm_epilogue_lds.h, which replaced round 3's direct stores.)
#pragma once
#include "gemm_epilogue.h"

namespace capdec {

// lm_head epilogue on a G::BM x 128 block tile (non-TR accumulator layout: acc[i][j][r] = C[wm TI 32 + i 32 + (r & 3) +
// 8 (r >> 2) + 4 (lane >> 5)][wn TJ 32 + j 32 + (lane & 31)]): the logits go through LDS in slabs of 128 rows (66 KB,
// re-using the ring) and leave as per-(row, 128-column tile) max, sum exp(x - max) and top-k (value, column) -- the
// arithmetic and the tie rules of epilogue_topk (gemm_epilogue.h), so the merge kernel sees the same partial lists
// whichever tile height produced them.
// KSEL = 0: max and sum exp only (the sparse lm_head's first pass: the candidates come from a later pass over the few tiles
// that can hold them, decode.hip: lm_head_select) -- the same bits as with any other KSEL.
// GROUPED (that later pass, gemm_h2w_topk_grouped_kernel): the block's rows are rows m0 .. M-1 of a gathered operand, row
// `row` of it writes its KSEL candidates to list slot_of[row]; max and sum exp are not written again.
template <class G, int KSEL, bool GROUPED = false>
__device__ __forceinline__ void epilogue_topk_w(const f32x16 (&acc)[G::TI][G::TJ], float scale, float *Ct, int M, int N,
                                                int m0, int n0, int tn, int tiles_n, float *tile_max, float *tile_sum,
                                                float *cand_val, int *cand_idx, const int *slot_of = nullptr) {
    static_assert(G::BN == 128 && G::NW == 4 && G::SMEM_B >= 128 * CT_LD * 4, "top-k epilogue: 128-column tiles, 4 waves");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave / G::WN, wn = wave % G::WN, half = lane >> 5, l32 = lane & 31;
    const int grp = lane >> 4, sub = lane & 15;
    constexpr int SLABS = G::BM / 128, WROWS = G::TI * 32;       // rows of one wavefront's tile
    for (int hh = 0; hh < SLABS; ++hh) {
        if ((wm * WROWS) / 128 == hh) {
            const int r0 = (wm * WROWS) % 128;
#pragma unroll
            for (int i = 0; i < G::TI; ++i)
#pragma unroll
                for (int j = 0; j < G::TJ; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int row = r0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                        Ct[row * CT_LD + (wn * G::TJ + j) * 32 + l32] = acc[i][j][r] * scale;
                    }
        }
        __syncthreads();
        for (int it = 0; it < 8; ++it) {
            const int rl = wave * 32 + it * 4 + grp;              // row within the slab
            const int row = m0 + hh * 128 + rl;
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int cl = sub + 16 * j;
                v[j] = (n0 + cl < N) ? Ct[rl * CT_LD + cl] : -INFINITY;
            }
            float mx = v[0];
#pragma unroll
            for (int j = 1; j < 8; ++j) mx = fmaxf(mx, v[j]);
            mx = row16_max(mx);
            float se = 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) se += __expf(v[j] - mx);
            se = row16_sum(se);
            if constexpr (GROUPED) {
                const size_t tbase = row < M ? (size_t)slot_of[row] : 0;
                row_tile_topk<KSEL>(v, mx, sub, n0, row < M, tbase, cand_val, cand_idx);
            } else {
                const size_t tbase = (size_t)row * tiles_n + tn;
                if (row < M && sub == 0) {
                    tile_max[tbase] = mx;
                    tile_sum[tbase] = se;
                }
                row_tile_topk<KSEL>(v, mx, sub, n0, row < M, tbase, cand_val, cand_idx);
            }
        }
        __syncthreads();
    }
}

}  // namespace capdec
