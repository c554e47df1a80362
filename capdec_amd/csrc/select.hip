// Token selection: merge of the lm_head per-tile candidates, greedy step, and the beam-search
// bookkeeping of reference gpt2_prefix_eval.py:78-108 (one wavefront per caption; all
// per-caption state lives in a few hundred bytes, so these kernels are launch-latency sized).
// The tie rule, the lane lists, the winner-pops round and the tile logsumexp come from row_select.h; the three merge
// kernels are entry points over merge_tile_lists.
// The beam kernels are beam_state.h's stage / commit around the plain candidate tournament; beam_finalize_kernel also ends
// the constrained beam.
#include "beam_state.h"

namespace capdec {

// ---- merge: one wavefront per row; the row's KOUT best of its tiles' KIN-entry lists [ntiles, KIN] -> out_val / out_idx
// [KOUT].  Returns, for the callers that flag rows, the row's KOUT-th winner and the best LAST-kept candidate among this
// lane's tiles (what bounds their hidden ones).  Only the k = 3 kernel reads them; they are register arithmetic without
// side effects, so where the result is ignored the compiler drops the tracking.
struct MergeTail {
    float kth_v; int kth_i;
    float last_v; int last_i;
};
template <int KIN, int KOUT>
__device__ __forceinline__ MergeTail merge_tile_lists(const float *__restrict__ cand_val, const int *__restrict__ cand_idx,
                                                      int ntiles, int lane, float *__restrict__ out_val,
                                                      int *__restrict__ out_idx) {
    LaneTopk<KOUT> best;
    best.clear();
    MergeTail t{-INFINITY, 0x7fffffff, -INFINITY, 0x7fffffff};
    for (int tile = lane; tile < ntiles; tile += 64) {
#pragma unroll
        for (int kk = 0; kk < KIN; ++kk) {
            const float v = cand_val[(size_t)tile * KIN + kk];
            const int i = cand_idx[(size_t)tile * KIN + kk];
            if (kk == KIN - 1 && better(v, i, t.last_v, t.last_i)) { t.last_v = v; t.last_i = i; }
            best.push(v, i);
        }
    }
#pragma unroll
    for (int r = 0; r < KOUT; ++r) {
        best.pop_best(t.kth_v, t.kth_i);
        if (lane == 0) { out_val[r] = t.kth_v; out_idx[r] = t.kth_i; }
    }
    return t;
}

// per row, logsumexp over tiles and the global top-k of the per-tile top-k lists
template <int KSEL>
__global__ __launch_bounds__(256) void topk_merge_kernel(const float *__restrict__ tile_max,
                                                         const float *__restrict__ tile_sum,
                                                         const float *__restrict__ cand_val,
                                                         const int *__restrict__ cand_idx, int rows, int ntiles,
                                                         float *__restrict__ lse, float *__restrict__ top_val,
                                                         int *__restrict__ top_idx) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const size_t base = (size_t)row * ntiles;
    const float l = tile_logsumexp(tile_max + base, tile_sum + base, ntiles, lane);
    if (lane == 0) lse[row] = l;
    merge_tile_lists<KSEL, KSEL>(cand_val + base * KSEL, cand_idx + base * KSEL, ntiles, lane, top_val + (size_t)row * KSEL,
                                 top_idx + (size_t)row * KSEL);
}

// ---- k = 3 per tile in, top 5 out, with the "may hide a fourth" flag (common.h)
__global__ __launch_bounds__(256) void topk_merge_k3_kernel(const float *__restrict__ tile_max, const float *__restrict__ tile_sum,
                                                            const float *__restrict__ cand_val, const int *__restrict__ cand_idx,
                                                            int rows, int ntiles, float *__restrict__ lse,
                                                            float *__restrict__ top_val, int *__restrict__ top_idx,
                                                            int *__restrict__ flag_rows, int *__restrict__ flag_count,
                                                            int *__restrict__ flag_total) {
    constexpr int KIN = 3, KOUT = 5;
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const size_t base = (size_t)row * ntiles;
    const float l = tile_logsumexp(tile_max + base, tile_sum + base, ntiles, lane);
    if (lane == 0) lse[row] = l;
    const MergeTail t = merge_tile_lists<KIN, KOUT>(cand_val + base * KIN, cand_idx + base * KIN, ntiles, lane,
                                                    top_val + (size_t)row * KOUT, top_idx + (size_t)row * KOUT);
    // A tile's hidden candidates are all worse than its third kept one, so they can only matter if that third one is
    // STRICTLY better than the row's fifth (if it IS the fifth, or worse, nothing hidden can pass it)
    const bool mine = better(t.last_v, t.last_i, t.kth_v, t.kth_i);
    if (__ballot(mine) != 0ull && lane == 0) {
        flag_rows[atomicAdd(flag_count, 1)] = row;
        atomicAdd(flag_total, 1);
    }
}

int launch_topk_merge_k3(hipStream_t st, const float *tile_max, const float *tile_sum, const float *cand_val,
                         const int *cand_idx, int rows, int ntiles, float *lse, float *top_val, int *top_idx,
                         int *flag_rows, int *flag_count, int *flag_total) {
    if (rows <= 0) return 0;
    hipLaunchKernelGGL(topk_merge_k3_kernel, dim3((rows + 3) / 4), dim3(256), 0, st, tile_max, tile_sum, cand_val, cand_idx,
                       rows, ntiles, lse, top_val, top_idx, flag_rows, flag_count, flag_total);
    CAPDEC_HIP(hipGetLastError());
    return 0;
}

// ---- the second pass's merge: compact row i (k = 5 lists) -> top 5 of row out_rows[i]; persistent over *count_dev rows
__global__ __launch_bounds__(256) void topk_merge_rows_kernel(const float *__restrict__ cand_val, const int *__restrict__ cand_idx,
                                                              const int *__restrict__ count_dev, const int *__restrict__ out_rows,
                                                              int ntiles, float *__restrict__ top_val, int *__restrict__ top_idx) {
    constexpr int KSEL = 5;
    const int lane = threadIdx.x & 63;
    const int n = *count_dev;
    for (int row = blockIdx.x * 4 + (threadIdx.x >> 6); row < n; row += gridDim.x * 4) {
        const size_t base = (size_t)row * ntiles;
        const size_t orow = (size_t)out_rows[row];
        merge_tile_lists<KSEL, KSEL>(cand_val + base * KSEL, cand_idx + base * KSEL, ntiles, lane, top_val + orow * KSEL,
                                     top_idx + orow * KSEL);
    }
}

int launch_topk_merge_rows(hipStream_t st, const float *cand_val, const int *cand_idx, const int *count_dev,
                           const int *out_rows, int rows_cap, int ntiles, float *top_val, int *top_idx) {
    if (rows_cap <= 0) return 0;
    hipLaunchKernelGGL(topk_merge_rows_kernel, dim3(std::min((rows_cap + 3) / 4, 1024)), dim3(256), 0, st, cand_val, cand_idx,
                       count_dev, out_rows, ntiles, top_val, top_idx);
    CAPDEC_HIP(hipGetLastError());
    return 0;
}

// ---- the sparse lm_head (decode.hip: lm_head_select): the first pass left max and sum exp per (row, tile) and NO candidates.
// With T5 the fifth largest of a row's tile maxima, every element of the row's top 5 lies in a tile with max >= T5 (an
// element of any other tile is strictly below five elements, the maxima of five tiles): without ties at T5 five tiles of
// all.  One wavefront per row, the row's tile maxima in registers (lane l holds tiles l + 64 j): logsumexp as the merge
// kernels take it; T5 by at most five rounds of "largest value below the last one, and how many tiles hold it"; then the
// tiles with max >= T5 in ascending order -> row_tiles[row][0 .. row_cnt[row]).  A row with more than LM_SPARSE_CAP such
// tiles (exact ties at T5) or a tile maximum that is not finite joins flag_rows, as a row of the three-candidate merge does
// (row_cnt = 0): the full second pass computes it.
constexpr int LM_SEL_MAXJ = 16;     // tiles per lane: <= 1024 column tiles
__global__ __launch_bounds__(256) void lm_tile_select_kernel(const float *__restrict__ tile_max, const float *__restrict__ tile_sum,
                                                             int rows, int ntiles, float *__restrict__ lse,
                                                             int *__restrict__ row_cnt, int *__restrict__ row_tiles,
                                                             int *__restrict__ flag_rows, int *__restrict__ flag_count,
                                                             int *__restrict__ flag_total) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const size_t base = (size_t)row * ntiles;
    const float l = tile_logsumexp(tile_max + base, tile_sum + base, ntiles, lane);
    if (lane == 0) lse[row] = l;
    const int nj = (ntiles + 63) >> 6;
    float mv[LM_SEL_MAXJ];
    bool bad = false;
#pragma unroll
    for (int j = 0; j < LM_SEL_MAXJ; ++j) {
        mv[j] = -INFINITY;
        if (j < nj) {
            const int t = lane + 64 * j;
            if (t < ntiles) {
                mv[j] = tile_max[base + t];
                bad |= !(__builtin_fabsf(mv[j]) < INFINITY);
            }
        }
    }
    float t5 = INFINITY;
    int have = 0;
    for (int r = 0; r < 5 && have < 5; ++r) {
        float lm = -INFINITY;
#pragma unroll
        for (int j = 0; j < LM_SEL_MAXJ; ++j)
            if (j < nj) lm = fmaxf(lm, mv[j] < t5 ? mv[j] : -INFINITY);
        t5 = wave_max(lm);
#pragma unroll
        for (int j = 0; j < LM_SEL_MAXJ; ++j)
            if (j < nj) have += __popcll(__ballot(mv[j] == t5));
    }
    if (__any(bad) || have > LM_SPARSE_CAP) {      // (have = tiles with max >= T5 when no maximum is -inf or NaN)
        if (lane == 0) {
            row_cnt[row] = 0;
            flag_rows[atomicAdd(flag_count, 1)] = row;
            atomicAdd(flag_total, 1);
        }
        return;
    }
    int pos = 0;
#pragma unroll
    for (int j = 0; j < LM_SEL_MAXJ; ++j) {
        if (j < nj) {
            const bool sel = mv[j] >= t5;
            const unsigned long long m = __ballot(sel);
            if (sel) row_tiles[(size_t)row * LM_SPARSE_CAP + pos + __popcll(m & ((1ull << lane) - 1ull))] = lane + 64 * j;
            pos += __popcll(m);
        }
    }
    if (lane == 0) row_cnt[row] = have;
}

// Pairs per tile, and later every pair's place in its tile's bucket: one THREAD per row, a block's 1024 rows first meet in
// an LDS histogram, so that a tile takes one global integer atomic per block and not one per pair (the first vocabulary
// tiles collect a large share of all pairs).  PLACE = false: tile_cnt[t] += the block's pairs of tile t.  PLACE = true
// (after the scan): the block reserves its share of every bucket and writes slot_of[tile_off[t] + place] = row *
// LM_SPARSE_CAP + s for its pairs.  The order inside a bucket differs from run to run; nothing reads it.
template <bool PLACE>
__global__ __launch_bounds__(1024) void lm_pair_bucket_kernel(const int *__restrict__ row_cnt, const int *__restrict__ row_tiles,
                                                              int rows, int ntiles, int *__restrict__ tile_acc,
                                                              const int *__restrict__ tile_off, int *__restrict__ slot_of) {
    __shared__ int hist[1024];
    const int t = threadIdx.x, row = blockIdx.x * 1024 + t;
    hist[t] = 0;
    __syncthreads();
    const int n = row < rows ? row_cnt[row] : 0;
    int tile[LM_SPARSE_CAP], place[LM_SPARSE_CAP];
#pragma unroll
    for (int s = 0; s < LM_SPARSE_CAP; ++s) {
        tile[s] = 0;
        place[s] = 0;
        if (s < n) {
            tile[s] = row_tiles[(size_t)row * LM_SPARSE_CAP + s];
            place[s] = atomicAdd(&hist[tile[s]], 1);
        }
    }
    __syncthreads();
    if (t < ntiles && hist[t] > 0) {
        const int b = atomicAdd(tile_acc + t, hist[t]);
        if (PLACE) hist[t] = tile_off[t] + b;
    }
    if (!PLACE) return;
    __syncthreads();
#pragma unroll
    for (int s = 0; s < LM_SPARSE_CAP; ++s)
        if (s < n) slot_of[hist[tile[s]] + place[s]] = row * LM_SPARSE_CAP + s;
}

// One block: the pair counts per tile -> tile_off (where a tile's bucket starts in the pair list), the grouped launch's
// block table (one entry per 256 pairs of a bucket: tile, first pair, pairs) and its length, cleared cursors for the
// placement, and the rows each slice of the full second pass takes.
__global__ __launch_bounds__(1024) void lm_bucket_scan_kernel(const int *__restrict__ tile_cnt, int ntiles, int *__restrict__ tile_cur,
                                                              int *__restrict__ tile_off, int *__restrict__ nblk,
                                                              int *__restrict__ blk_tab, const int *__restrict__ flag_count,
                                                              int *__restrict__ slice_cnt, int slice_rows, int nslices) {
    __shared__ int s_rows[1024], s_blk[1024];
    const int t = threadIdx.x;
    const int c = t < ntiles ? tile_cnt[t] : 0;
    const int blks = (c + 255) >> 8;
    s_rows[t] = c;
    s_blk[t] = blks;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {                       // inclusive scan of both
        const int a = t >= o ? s_rows[t - o] : 0, b = t >= o ? s_blk[t - o] : 0;
        __syncthreads();
        s_rows[t] += a;
        s_blk[t] += b;
        __syncthreads();
    }
    if (t < ntiles) {
        const int off = s_rows[t] - c, b0 = s_blk[t] - blks;
        tile_off[t] = off;
        tile_cur[t] = 0;
        for (int b = 0; b < blks; ++b) {
            blk_tab[3 * (b0 + b)] = t;
            blk_tab[3 * (b0 + b) + 1] = off + 256 * b;
            blk_tab[3 * (b0 + b) + 2] = min(256, c - 256 * b);
        }
    }
    if (t == 1023) *nblk = s_blk[1023];
    if (t < nslices) slice_cnt[t] = max(0, min(slice_rows, *flag_count - t * slice_rows));
}

// The row's top 5 of the (<= LM_SPARSE_CAP x 5) candidates its pairs brought back (list slot row * LM_SPARSE_CAP + s), under
// the tie rule; whatever order the pairs were computed in.  Rows of the full second pass (row_cnt = 0) are not touched.
__global__ __launch_bounds__(256) void lm_sparse_merge_kernel(const float *__restrict__ cand_val, const int *__restrict__ cand_idx,
                                                              const int *__restrict__ row_cnt, int rows,
                                                              float *__restrict__ top_val, int *__restrict__ top_idx) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int n = row_cnt[row];
    if (n == 0) return;
    LaneTopk<1> best;
    best.clear();
    if (lane < n * 5) best.push(cand_val[(size_t)row * LM_SPARSE_CAP * 5 + lane], cand_idx[(size_t)row * LM_SPARSE_CAP * 5 + lane]);
#pragma unroll
    for (int r = 0; r < 5; ++r) {
        float gv;
        int gi;
        best.pop_best(gv, gi);
        if (lane == 0) { top_val[(size_t)row * 5 + r] = gv; top_idx[(size_t)row * 5 + r] = gi; }
    }
}

// s.tile_cnt zeroed by the caller; leaves lse, the pairs bucketed by tile in s.slot_of, the block table and the slice counts
int launch_lm_tile_select(hipStream_t st, const float *tile_max, const float *tile_sum, int rows, int ntiles, float *lse,
                          const SparseLm &s, int *flag_rows, int *flag_count, int *flag_total) {
    if (rows <= 0) return 0;
    CAPDEC_CHECK(ntiles >= 5 && ntiles <= 64 * LM_SEL_MAXJ, "lm_tile_select: 5 .. 1024 column tiles");
    const dim3 rb((rows + 1023) / 1024);
    hipLaunchKernelGGL(lm_tile_select_kernel, dim3((rows + 3) / 4), dim3(256), 0, st, tile_max, tile_sum, rows, ntiles, lse,
                       s.row_cnt, s.row_tiles, flag_rows, flag_count, flag_total);
    hipLaunchKernelGGL(lm_pair_bucket_kernel<false>, rb, dim3(1024), 0, st, s.row_cnt, s.row_tiles, rows, ntiles, s.tile_cnt,
                       (const int *)nullptr, (int *)nullptr);
    hipLaunchKernelGGL(lm_bucket_scan_kernel, dim3(1), dim3(1024), 0, st, s.tile_cnt, ntiles, s.tile_cur, s.tile_off, s.nblk,
                       s.blk_tab, flag_count, s.slice_cnt, s.slice_rows, LM_HARD_SLICES);
    hipLaunchKernelGGL(lm_pair_bucket_kernel<true>, rb, dim3(1024), 0, st, s.row_cnt, s.row_tiles, rows, ntiles, s.tile_cur,
                       s.tile_off, s.slot_of);
    CAPDEC_HIP(hipGetLastError());
    return 0;
}

int launch_lm_sparse_merge(hipStream_t st, const float *cand_val, const int *cand_idx, const int *row_cnt, int rows,
                           float *top_val, int *top_idx) {
    if (rows <= 0) return 0;
    hipLaunchKernelGGL(lm_sparse_merge_kernel, dim3((rows + 3) / 4), dim3(256), 0, st, cand_val, cand_idx, row_cnt, rows, top_val,
                       top_idx);
    CAPDEC_HIP(hipGetLastError());
    return 0;
}

int launch_topk_merge(hipStream_t st, const float *tile_max, const float *tile_sum, const float *cand_val,
                      const int *cand_idx, int rows, int ntiles, int k, float *lse, float *top_val, int *top_idx) {
    if (rows <= 0) return 0;
    dim3 grid((rows + 3) / 4), block(256);
    CAPDEC_TRY(with_topk_k(k, "topk_merge", [&](auto KS) {
        hipLaunchKernelGGL(topk_merge_kernel<KS>, grid, block, 0, st, tile_max, tile_sum, cand_val, cand_idx, rows, ntiles,
                           lse, top_val, top_idx);
    }));
    CAPDEC_HIP(hipGetLastError());
    return 0;
}

// ---- greedy: reference gpt2_prefix_eval.py:177-188 (argmax; stop on '.' or id 764)
// (k candidates per row: k = 1 normally; teacher forcing -- forced != nullptr -- feeds forced[row, step] as the next
//  token instead of the arg-max and, with k = 2, records (top-1 logit, top-2 logit, logsumexp) of every step)
__global__ void greedy_step_kernel(GreedyState s, const int *__restrict__ top_idx, int rows, int step, int k,
                                   const int *__restrict__ forced, const float *__restrict__ top_val,
                                   const float *__restrict__ lse, float *__restrict__ stats) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;       // activation row (compact)
    if (r >= rows) return;
    const int row = s.cmap ? s.cmap[r] : r;                    // caption
    const int tok = top_idx[(size_t)r * k];
    if (stats) {
        float *o = stats + ((size_t)row * s.T + step) * 3;
        o[0] = top_val[(size_t)r * k];
        o[1] = k > 1 ? top_val[(size_t)r * k + 1] : -INFINITY;
        o[2] = lse[r];
    }
    if (forced) {                                              // teacher forcing: nothing stops, every step is recorded
        s.next_tok[row] = forced[(size_t)row * s.T + step];
        s.ids[(size_t)row * s.T + step] = tok;
        s.lens[row] = step + 1;
        atomicAdd(s.alive_count, 1);
        return;
    }
    // The next step embeds next_tok of EVERY row that is still in the batch, finished captions included (until the next
    // compaction), so it is written before `done` is looked at.  greedy_emit stores the same value again: redundant here,
    // needed by the sampling kernel, which leaves before any store when the caption is done.  Keep this order.
    s.next_tok[row] = tok;
    if (s.done[row]) return;
    greedy_emit(s, row, step, tok, 0.f);
}

int launch_greedy_step(hipStream_t st, const GreedyState &s, const int *top_idx, int rows, int step, int k,
                       const int *forced, const float *top_val, const float *lse, float *stats) {
    if (rows <= 0) return 0;
    hipLaunchKernelGGL(greedy_step_kernel, dim3((rows + 255) / 256), dim3(256), 0, st, s, top_idx, rows, step, k, forced,
                       top_val, lse, stats);
    CAPDEC_HIP(hipGetLastError());
    return 0;
}

// ---- beam step 0: reference gpt2_prefix_eval.py:78-88,105-108
// one wavefront per caption; top_val/top_idx/lse are per CAPTION row here (prefill last position)
__global__ __launch_bounds__(64) void beam_init_kernel(BeamState s, const float *__restrict__ lse,
                                                       const float *__restrict__ top_val,
                                                       const int *__restrict__ top_idx, int beam, int k, int T,
                                                       int stop_id) {
    const int cap = blockIdx.x, b = threadIdx.x;
    bool stop = true;
    if (b < beam) {
        const float logp = top_val[(size_t)cap * k + b] - lse[cap];   // log softmax
        stop = beam_init_slot(s, (size_t)cap * beam + b, T, top_idx[(size_t)cap * k + b], logp, stop_id);
    }
    beam_init_done(s, cap, stop);
}

int launch_beam_init(hipStream_t st, const BeamState &s, const float *lse, const float *top_val, const int *top_idx,
                     int ncap, int beam, int k, int T, int stop_id) {
    CAPDEC_CHECK(beam >= 1 && beam <= BEAM_MAX && k >= beam, "beam: beam size must be in 1..8");
    if (ncap <= 0) return 0;
    hipLaunchKernelGGL(beam_init_kernel, dim3(ncap), dim3(64), 0, st, s, lse, top_val, top_idx, beam, k, T, stop_id);
    CAPDEC_HIP(hipGetLastError());
    return 0;
}

// ---- beam step i >= 1: reference gpt2_prefix_eval.py:89-108.
// lane c < beam*k is candidate (b = c / k, j = c % k).  fp32 arithmetic in the reference's order:
//   scores_sum = scores + logp; seq += ~stopped; avg = scores_sum / seq; top-beam of avg over the
//   flattened [beam * V]; scores = avg * seq[src].
__global__ __launch_bounds__(64) void beam_step_kernel(BeamState s, const float *__restrict__ lse,
                                                       const float *__restrict__ top_val,
                                                       const int *__restrict__ top_idx, int beam, int k, int T, int ctx,
                                                       int step, int pos_cur, int vocab, int stop_id,
                                                       const int *__restrict__ cmap) {
    __shared__ BeamStepLds L;
    const int lane = threadIdx.x;
    const int cap = cmap ? cmap[blockIdx.x] : blockIdx.x;       // state (tokens, scores, anc ...) by original caption
    if (s.done[cap]) return;
    const size_t cb0 = (size_t)cap * beam;
    const size_t ab0 = (size_t)blockIdx.x * beam;               // lm_head outputs by (compact) activation row
    beam_stage(s, L, cap, beam, T, ctx, step, pos_cur);
    __syncthreads();
    // candidate of this lane
    float key = -INFINITY;
    int flat = 0x7fffffff, ctok = 0, cb = 0;
    if (lane < beam * k) {
        cb = lane / k;
        const int j = lane - cb * k;
        const size_t row = cb0 + cb, arow = ab0 + cb;
        if (L.st_old[cb]) {
            if (j == 0) { ctok = 0; key = (s.scores[row] + 0.0f) / L.seq_new[cb]; }
        } else {
            ctok = top_idx[arow * k + j];
            const float logp = top_val[arow * k + j] - lse[arow];
            key = (s.scores[row] + logp) / L.seq_new[cb];
        }
        if (key > -INFINITY || (L.st_old[cb] && j == 0)) flat = cb * vocab + ctok;
        if (s.diverge && j != 0) { key = -INFINITY; flat = 0x7fffffff; }      // measurement only: each beam keeps its own lineage
    }
    for (int r = 0; r < beam; ++r) {
        float gv = key;
        int gi = flat;
        wave_best(gv, gi);
        if (gi == flat && gv == key && flat != 0x7fffffff) {   // winner (flat indices are unique)
            L.w_src[r] = cb; L.w_tok[r] = ctok; L.w_key[r] = key;
            key = -INFINITY; flat = 0x7fffffff;
        }
    }
    __syncthreads();
    beam_commit(s, L, cap, beam, T, ctx, step, pos_cur, stop_id);
}

int launch_beam_step(hipStream_t st, const BeamState &s, const float *lse, const float *top_val, const int *top_idx,
                     int ncap, int beam, int k, int T, int ctx, int step, int pos_cur, int vocab, int stop_id,
                     const int *cmap) {
    CAPDEC_TRY(beam_step_checks("beam", beam, T, ctx, step, pos_cur, vocab));
    CAPDEC_CHECK(beam * k <= 64, "beam: beam*k must fit one wavefront");
    if (ncap <= 0) return 0;
    hipLaunchKernelGGL(beam_step_kernel, dim3(ncap), dim3(64), beam_step_lds(beam, T, ctx), st, s, lse, top_val, top_idx,
                       beam, k, T, ctx, step, pos_cur, vocab, stop_id, cmap);
    CAPDEC_HIP(hipGetLastError());
    return 0;
}

// ---- end of generate_beam: scores /= seq_lengths; order = argsort(desc) (reference :110-114).  With a constraint state
// (con_state [ncap, beam], constrained.hip) the rows are ordered by (phrases met, scores / seq, slot) and met [ncap, beam]
// (may be nullptr) receives their met masks; without one every slot has met nothing and the order is (score desc, slot asc).
// (the phrase counts travel by shuffle, not through LDS)
__global__ __launch_bounds__(64) void beam_finalize_kernel(BeamState s, const int *__restrict__ con_state, int beam, int T,
                                                           int *__restrict__ ids, int *__restrict__ lens,
                                                           float *__restrict__ scores, int *__restrict__ order,
                                                           int *__restrict__ met) {
    __shared__ float f[BEAM_MAX];
    __shared__ int rank_of[BEAM_MAX];
    const int cap = blockIdx.x, lane = threadIdx.x;
    const size_t cb0 = (size_t)cap * beam;
    float fl = 0.f;
    int cst = 0;
    if (lane < beam) {
        f[lane] = fl = s.scores[cb0 + lane] / s.seq[cb0 + lane];
        if (con_state) cst = con_state[cb0 + lane];
    }
    __syncthreads();
    const int nmet = __popc(con_met(cst));
    int rank = 0;
    for (int o = 0; o < beam; ++o) {
        const int no = __shfl(nmet, o, 64);
        const bool ahead = no != nmet ? no > nmet : (f[o] > fl || (f[o] == fl && o < lane));
        if (o != lane && ahead) ++rank;
    }
    if (lane < beam) {
        rank_of[lane] = rank;
        scores[cb0 + rank] = fl;
        lens[cb0 + rank] = (int)s.seq[cb0 + lane];
        if (order) order[cb0 + rank] = lane;
        if (met) met[cb0 + rank] = con_met(cst);
    }
    __syncthreads();
    for (int i = lane; i < beam * T; i += 64) {
        const int b = i / T, t = i - b * T;
        ids[(cb0 + rank_of[b]) * T + t] = s.tokens[(cb0 + b) * T + t];
    }
}

int launch_beam_finalize(hipStream_t st, const BeamState &s, int ncap, int beam, int T, int *ids, int *lens,
                         float *scores, int *order, const int *con_state, int *met) {
    if (ncap <= 0) return 0;
    CAPDEC_CHECK(beam >= 1 && beam <= BEAM_MAX && (con_state || !met), "beam finalize: beam size must be in 1..8");
    hipLaunchKernelGGL(beam_finalize_kernel, dim3(ncap), dim3(64), 0, st, s, con_state, beam, T, ids, lens, scores, order, met);
    CAPDEC_HIP(hipGetLastError());
    return 0;
}

// ---- finished-caption compaction: the captions that still generate, in ascending order.  One block; every
// 1024-caption slab is ranked with a wavefront ballot + a 16-entry scan of the wavefront totals.
__global__ __launch_bounds__(1024) void compact_alive_kernel(const uint8_t *__restrict__ done, int ncap,
                                                             int *__restrict__ cmap, int *__restrict__ count) {
    __shared__ int wtot[16];
    __shared__ int base;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (t == 0) base = 0;
    __syncthreads();
    for (int c0 = 0; c0 < ncap; c0 += 1024) {
        const int c = c0 + t;
        const bool alive = c < ncap && !done[c];
        const unsigned long long m = __ballot(alive);
        const int before = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wtot[wave] = __popcll(m);
        __syncthreads();
        int off = base;
        for (int w = 0; w < wave; ++w) off += wtot[w];
        if (alive) cmap[off + before] = c;
        __syncthreads();
        if (t == 0) {
            int tot = 0;
            for (int w = 0; w < 16; ++w) tot += wtot[w];
            base += tot;
        }
        __syncthreads();
    }
    if (t == 0) *count = base;
}

int launch_compact_alive(hipStream_t st, const uint8_t *done, int ncap, int *cmap, int *count) {
    if (ncap <= 0) return 0;
    hipLaunchKernelGGL(compact_alive_kernel, dim3(1), dim3(1024), 0, st, done, ncap, cmap, count);
    CAPDEC_HIP(hipGetLastError());
    return 0;
}

// ---- token cross-entropy of a logits matrix (the loss of the train step's forward: reference train.py:349 /
// GPT2LMHeadModel's `labels=`): nll[row] = logsumexp(logits[row]) - logits[row][label[row]], one wavefront per row
// (max, then sum of exp(x - max): the order torch's log_softmax uses), rows whose label == ignore_index contribute
// nothing; the mean over the counted rows is taken by ONE block in a fixed order (deterministic).
__global__ __launch_bounds__(256) void token_nll_kernel(const float *__restrict__ logits, int ld, const int *__restrict__ labels,
                                                        int rows, int V, int ignore_index, float *__restrict__ nll) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lab = labels[row];
    if (lab == ignore_index) { if (lane == 0) nll[row] = -1.f; return; }     // -1 = not counted
    // a label outside [0, V) that is not ignore_index is an ERROR in torch's cross_entropy (and in the reference's
    // train.py:350 / GPT2LMHeadModel labels path): a wrong tokenizer or vocabulary must not yield a plausible mean over
    // fewer rows -- the row becomes NaN, so the loss is NaN (capdec.h)
    if (lab < 0 || lab >= V) { if (lane == 0) nll[row] = nanf(""); return; }
    const float *x = logits + (size_t)row * ld;
    float mx = -INFINITY;
    for (int c = lane; c < V; c += 64) mx = fmaxf(mx, x[c]);
    mx = wave_max(mx);
    float se = 0.f;
    for (int c = lane; c < V; c += 64) se += expf(x[c] - mx);
    se = wave_sum(se);
    if (lane == 0) nll[row] = (mx + logf(se)) - x[lab];
}
__global__ __launch_bounds__(256) void nll_mean_kernel(const float *__restrict__ nll, int rows, float *__restrict__ out) {
    __shared__ double part[256];
    __shared__ int cnt[256];
    double s = 0.0;
    int n = 0;
    for (int r = threadIdx.x; r < rows; r += 256) {
        const float v = nll[r];
        if (v >= 0.f || v != v) { s += (double)v; ++n; }          // (a NaN loss must stay visible)
    }
    part[threadIdx.x] = s;
    cnt[threadIdx.x] = n;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) { part[threadIdx.x] += part[threadIdx.x + o]; cnt[threadIdx.x] += cnt[threadIdx.x + o]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = cnt[0] > 0 ? (float)(part[0] / cnt[0]) : nanf("");    // torch: mean over nothing = nan
}
int launch_cross_entropy_mean(hipStream_t st, const float *logits, int ld, const int *labels, int rows, int V,
                              int ignore_index, float *nll_ws, float *out) {
    if (rows <= 0) return 0;
    hipLaunchKernelGGL(token_nll_kernel, dim3((rows + 3) / 4), dim3(256), 0, st, logits, ld, labels, rows, V, ignore_index, nll_ws);
    hipLaunchKernelGGL(nll_mean_kernel, dim3(1), dim3(256), 0, st, nll_ws, rows, out);
    CAPDEC_HIP(hipGetLastError());
    return 0;
}

}  // namespace capdec
