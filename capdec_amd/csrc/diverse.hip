// Diverse (group) beam search (Vijayakumar et al. 2016) on the beam decode: the winner selection of select.hip's
// beam_init_kernel / beam_step_kernel run per GROUP of Bg = beam / groups slots (capdec_decode_beam_groups; the contract:
// include/capdec.h); staging, write-back and the limits are the shared ones of beam_state.h.  Slots g*Bg .. (g+1)*Bg-1 of a caption form group g; within a step the groups are processed in order,
// and a token that h hypotheses of the earlier groups took AT THIS STEP (from sources that were not stopped) costs a row of
// a later group lambda * h of its log-prob.  Everything around these two kernels is the plain beam's: the fused lm_head +
// per-tile top-k with k = beam candidates per row, the ancestor-table attention (the ancestor bytes hold caption-level
// slots), compaction, chunking, beam_finalize_kernel.
//
// Why k = beam candidates per row are still enough (the [rows, vocab] logits stay unmaterialised):
//   1. at most B - Bg tokens are penalised for any group (the earlier groups selected at most B - Bg hypotheses);
//   2. a row's unpenalised top-B list therefore holds at least Bg unpenalised tokens;
//   3. each of those is >= every token outside the list, penalised or not (the penalty only lowers a value);
//   4. the list is built with ties to the smaller column, the tie rule of the selection;
//   5. so the row's best Bg after the penalty -- all a group can take from one row -- are inside the list it already has.
//
// Rounding: lp_pen = lp - lambda * (float)cnt is one multiplication and one subtraction, each rounded (no fma), so cnt = 0
// leaves lp as it is and groups = 1 is the plain beam bit for bit.  `scores` accumulates the PENALISED values (the classic
// algorithm); BeamState::logp carries the unpenalised sum next to it.  BeamState::diverge is not honoured here.
#include "beam_state.h"

namespace capdec {

__device__ __forceinline__ float penalised(float lp, float lambda, int cnt) {
    return __fsub_rn(lp, __fmul_rn(lambda, (float)cnt));
}

// ---- step 0: one logits row per caption (prefill last position).  lane j < k holds the row's j-th candidate; group g takes
// the best Bg of lp - lambda * cnt, cnt = how many slots of the groups before it took the token.  Ties go to the earlier
// place in the row's list (larger logit, then smaller token), so that with one group the slots are the list's first `beam`
// entries in order: beam_init_kernel
__global__ __launch_bounds__(64) void group_beam_init_kernel(BeamState s, const float *__restrict__ lse,
                                                             const float *__restrict__ top_val,
                                                             const int *__restrict__ top_idx, int beam, int groups,
                                                             float lambda, int k, int T, int stop_id) {
    __shared__ int w_tok[BEAM_MAX];
    const int cap = blockIdx.x, lane = threadIdx.x;
    const int bg = beam / groups;
    int tok = 0x7fffffff;
    float lp = -INFINITY;
    if (lane < k) {
        tok = top_idx[(size_t)cap * k + lane];
        lp = top_val[(size_t)cap * k + lane] - lse[cap];          // log softmax
    }
    if (lane < BEAM_MAX) w_tok[lane] = -1;
    __syncthreads();
    bool stop = true;
    for (int g = 0; g < groups; ++g) {
        int cnt = 0;
        for (int r = 0; r < g * bg; ++r) cnt += w_tok[r] == tok;
        float key = lane < k ? penalised(lp, lambda, cnt) : -INFINITY;
        int idx = key > -INFINITY ? lane : 0x7fffffff;
        for (int r = 0; r < bg; ++r) {
            float gv = key;
            int gi = idx;
            wave_best(gv, gi);
            if (gi == idx && gv == key && idx != 0x7fffffff) {     // winner (list places are unique)
                const int slot = g * bg + r;
                w_tok[slot] = tok;
                s.logp[(size_t)cap * beam + slot] = lp;
                if (!beam_init_slot(s, (size_t)cap * beam + slot, T, tok, key, stop_id)) stop = false;
                key = -INFINITY; idx = 0x7fffffff;
            }
        }
        __syncthreads();                                           // the next group reads this group's w_tok
    }
    beam_init_done(s, cap, stop);
}

int launch_group_beam_init(hipStream_t st, const BeamState &s, const float *lse, const float *top_val, const int *top_idx,
                           int ncap, int beam, int groups, float diversity, int k, int T, int stop_id) {
    CAPDEC_CHECK(beam >= 1 && beam <= BEAM_MAX && k >= beam && k <= 64, "beam groups: beam size must be in 1..8");
    CAPDEC_CHECK(groups >= 1 && groups <= beam && beam % groups == 0, "beam groups: groups must divide the beam size");
    CAPDEC_CHECK(s.logp, "beam groups: no log-prob accumulator");
    if (ncap <= 0) return 0;
    hipLaunchKernelGGL(group_beam_init_kernel, dim3(ncap), dim3(64), 0, st, s, lse, top_val, top_idx, beam, groups, diversity,
                       k, T, stop_id);
    CAPDEC_HIP(hipGetLastError());
    return 0;
}

// ---- step i >= 1: beam_state.h's stage and commit around the group loop.  lane c < beam*k is candidate (b = c / k,
// j = c % k) and belongs to group b / Bg; w_src / w_tok of the slots already filled this step are the (token, live) table of
// the penalty.  B winner rounds per step, as in the plain beam: Bg per group, in which only that group's lanes compete.
__global__ __launch_bounds__(64) void group_beam_step_kernel(BeamState s, const float *__restrict__ lse,
                                                             const float *__restrict__ top_val,
                                                             const int *__restrict__ top_idx, int beam, int groups,
                                                             float lambda, int k, int T, int ctx, int step, int pos_cur,
                                                             int vocab, int stop_id, const int *__restrict__ cmap) {
    __shared__ struct : BeamStepLds { float w_lp[BEAM_MAX], lp_old[BEAM_MAX]; } L;     // + the winners' and the old slots' log-probs
    const int lane = threadIdx.x;
    const int cap = cmap ? cmap[blockIdx.x] : blockIdx.x;       // state (tokens, scores, anc ...) by original caption
    if (s.done[cap]) return;
    const int bg = beam / groups;
    const size_t cb0 = (size_t)cap * beam;
    const size_t ab0 = (size_t)blockIdx.x * beam;               // lm_head outputs by (compact) activation row
    beam_stage(s, L, cap, beam, T, ctx, step, pos_cur);
    if (lane < beam) L.lp_old[lane] = s.logp[cb0 + lane];
    if (lane < BEAM_MAX) { L.w_src[lane] = lane < beam ? lane : 0; L.w_tok[lane] = 0; L.w_key[lane] = -INFINITY; L.w_lp[lane] = 0.0f; }
    __syncthreads();
    // candidate of this lane
    int ctok = 0, cb = 0, j = 0;
    float lp = 0.0f, sc = 0.0f;
    const bool cand = lane < beam * k;
    if (cand) {
        cb = lane / k;
        j = lane - cb * k;
        sc = s.scores[cb0 + cb];
        if (!L.st_old[cb]) {
            ctok = top_idx[(ab0 + cb) * k + j];
            lp = top_val[(ab0 + cb) * k + j] - lse[ab0 + cb];
        }
    }
    const int grp = cb / bg;
    for (int g = 0; g < groups; ++g) {
        float key = -INFINITY;
        int flat = 0x7fffffff;
        if (cand && grp == g) {
            if (L.st_old[cb]) {
                if (j == 0) key = (sc + 0.0f) / L.seq_new[cb];     // the single candidate: neither penalised nor counted
            } else {
                int cnt = 0;
                for (int r = 0; r < g * bg; ++r) cnt += (L.w_tok[r] == ctok) & !L.st_old[L.w_src[r]];
                key = (sc + penalised(lp, lambda, cnt)) / L.seq_new[cb];
            }
            if (key > -INFINITY || (L.st_old[cb] && j == 0)) flat = cb * vocab + ctok;
        }
        for (int r = 0; r < bg; ++r) {
            float gv = key;
            int gi = flat;
            wave_best(gv, gi);
            if (gi == flat && gv == key && flat != 0x7fffffff) {   // winner (flat indices are unique)
                const int slot = g * bg + r;
                L.w_src[slot] = cb; L.w_tok[slot] = ctok; L.w_key[slot] = key; L.w_lp[slot] = L.st_old[cb] ? 0.0f : lp;
                key = -INFINITY; flat = 0x7fffffff;
            }
        }
        __syncthreads();                                           // the next group (and the commit) reads the winners
    }
    if (lane < beam) s.logp[cb0 + lane] = L.lp_old[L.w_src[lane]] + L.w_lp[lane];
    beam_commit(s, L, cap, beam, T, ctx, step, pos_cur, stop_id);
}

int launch_group_beam_step(hipStream_t st, const BeamState &s, const float *lse, const float *top_val, const int *top_idx,
                           int ncap, int beam, int groups, float diversity, int k, int T, int ctx, int step, int pos_cur,
                           int vocab, int stop_id, const int *cmap) {
    CAPDEC_TRY(beam_step_checks("beam groups", beam, T, ctx, step, pos_cur, vocab));
    CAPDEC_CHECK(beam * k <= 64, "beam groups: beam*k must fit one wavefront");
    CAPDEC_CHECK(groups >= 1 && groups <= beam && beam % groups == 0, "beam groups: groups must divide the beam size");
    CAPDEC_CHECK(s.logp, "beam groups: no log-prob accumulator");
    if (ncap <= 0) return 0;
    hipLaunchKernelGGL(group_beam_step_kernel, dim3(ncap), dim3(64), beam_step_lds(beam, T, ctx), st, s, lse, top_val, top_idx,
                       beam, groups, diversity, k, T, ctx, step, pos_cur, vocab, stop_id, cmap);
    CAPDEC_HIP(hipGetLastError());
    return 0;
}

// ---- the unpenalised sums in the order beam_finalize_kernel returned the rows
__global__ void group_beam_logp_kernel(const float *__restrict__ logp, const int *__restrict__ order, int rows, int beam,
                                       float *__restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows) return;
    const int cap = i / beam;
    const int slot = order[i];
    out[i] = logp[(size_t)cap * beam + (slot >= 0 && slot < beam ? slot : 0)];
}

int launch_group_beam_logp(hipStream_t st, const BeamState &s, int ncap, int beam, const int *order, float *logp_out) {
    if (ncap <= 0) return 0;
    const int rows = ncap * beam;
    hipLaunchKernelGGL(group_beam_logp_kernel, dim3((rows + 255) / 256), dim3(256), 0, st, s.logp, order, rows, beam, logp_out);
    CAPDEC_HIP(hipGetLastError());
    return 0;
}

}  // namespace capdec
