// The bookkeeping every beam-step kernel shares (select.hip: plain; diverse.hip: groups; constrained.hip: phrases): the
// limits and the launch geometry, the staging of the state a step permutes in place, and the commit of the step's winners.
// A step kernel is  beam_stage -> its own candidates and winner selection -> beam_commit;  a step-0 kernel hands every
// slot to beam_init_slot and ends in beam_init_done.  ONE definition of each: the ancestor permutation, the kv_stat count
// and the done / alive_count epilogue are what keeps the variants equal to each other where their contracts say so
// (groups = 1 and no phrases are the plain beam bit for bit).  One wavefront per caption throughout.
#pragma once
#include "row_select.h"

namespace capdec {

constexpr int BEAM_T_MAX = 1024;    // max entry_length
constexpr int BEAM_CTX_MAX = 1024;  // max context (prefix + generated): GPT-2's n_positions, the reference's only limit
constexpr int BEAM_MAX = 8;         // (a step stages beam x (T ints + ctx bytes) of state in dynamic LDS: <= 40 KB)
static_assert(CON_BEAM_MAX == BEAM_MAX, "a constrained row's list holds one place per beam slot");

// ---- launch side: the checks of a step launcher, and the dynamic LDS its kernel stages into
inline int beam_step_checks(const char *what, int beam, int T, int ctx, int step, int pos_cur, int vocab) {
    CAPDEC_CHECK(beam >= 1 && beam <= BEAM_MAX, std::string(what) + ": beam size must be in 1..8");
    CAPDEC_CHECK(T <= BEAM_T_MAX && ctx <= BEAM_CTX_MAX && step >= 1 && step < T && pos_cur >= 0 && pos_cur < ctx,
                 std::string(what) + ": entry_length / context too long");
    CAPDEC_CHECK((long long)beam * vocab < 0x7fffffffLL, std::string(what) + ": beam*vocab overflows int");
    return 0;
}
inline size_t beam_step_lds(int beam, int T, int ctx) {
    return (size_t)beam * T * sizeof(int) + (((size_t)beam * ctx + 3) & ~(size_t)3);
}

// ---- the constraint state of a slot in one int: met in bits 0..3, cur + 1 in bits 4..6 (0: none), pos in bits 8..10
__device__ __forceinline__ int con_pack(int met, int cur, int pos) { return met | ((cur + 1) << 4) | (pos << 8); }
__device__ __forceinline__ int con_met(int st) { return st & 15; }
__device__ __forceinline__ int con_cur(int st) { return ((st >> 4) & 7) - 1; }
__device__ __forceinline__ int con_pos(int st) { return (st >> 8) & 7; }

// ---- a step's LDS: the winners (slot r continues slot w_src[r] with token w_tok[r] at key w_key[r]), which the variant's
// selection fills, and the old slots' state; the token histories and ancestor bytes the step permutes sit in dynamic LDS
struct BeamStepLds {
    int w_src[BEAM_MAX], w_tok[BEAM_MAX];
    float w_key[BEAM_MAX], seq_new[BEAM_MAX];
    uint8_t st_old[BEAM_MAX];
};
struct BeamOld {
    int *tok;          // [beam][T]
    uint8_t *anc;      // [beam][ctx]
};
__device__ __forceinline__ BeamOld beam_old(int beam, int T) {
    extern __shared__ int beam_dyn[];
    return {beam_dyn, reinterpret_cast<uint8_t *>(beam_dyn + beam * T)};
}

// stage the state of caption `cap` that is permuted in place: `step` tokens and pos_cur ancestor bytes per slot, the
// stopped flags and the lengths after this step.  The caller's barrier follows (after whatever else it stages).
__device__ __forceinline__ void beam_stage(const BeamState &s, BeamStepLds &L, int cap, int beam, int T, int ctx, int step,
                                           int pos_cur) {
    const int lane = threadIdx.x;
    const size_t cb0 = (size_t)cap * beam;
    const BeamOld old = beam_old(beam, T);
    for (int i = lane; i < beam * step; i += 64) {
        const int b = i / step, t = i - b * step;
        old.tok[b * T + t] = s.tokens[(cb0 + b) * T + t];
    }
    for (int i = lane; i < beam * pos_cur; i += 64) {
        const int b = i / pos_cur, p = i - b * pos_cur;
        old.anc[b * ctx + p] = s.anc[(cb0 + b) * ctx + p];
    }
    if (lane < beam) {
        const bool stp = s.stopped[cb0 + lane];
        L.st_old[lane] = stp;
        L.seq_new[lane] = s.seq[cb0 + lane] + (stp ? 0.0f : 1.0f);
    }
}

// write the permuted state (the caller's barrier stands between the winners and this): seq, scores = key * seq, stopped,
// next_tok and the new token of every slot, its source's history and ancestor bytes with the source appended, kv_stat,
// done / alive_count.  What a variant carries on top it writes itself, beside the call.
__device__ __forceinline__ void beam_commit(const BeamState &s, const BeamStepLds &L, int cap, int beam, int T, int ctx,
                                            int step, int pos_cur, int stop_id) {
    const int lane = threadIdx.x;
    const size_t cb0 = (size_t)cap * beam;
    const BeamOld old = beam_old(beam, T);
    bool stop = true;
    if (lane < beam) {
        const int src = L.w_src[lane], tok = L.w_tok[lane];
        const float sq = L.seq_new[src];
        s.seq[cb0 + lane] = sq;
        s.scores[cb0 + lane] = L.w_key[lane] * sq;
        stop = L.st_old[src] || tok == stop_id;
        s.stopped[cb0 + lane] = stop;
        s.next_tok[cb0 + lane] = tok;
        s.tokens[(cb0 + lane) * T + step] = tok;
    }
    for (int i = lane; i < beam * step; i += 64) {
        const int b = i / step, t = i - b * step;
        s.tokens[(cb0 + b) * T + t] = old.tok[L.w_src[b] * T + t];
    }
    for (int i = lane; i < beam * (pos_cur + 1); i += 64) {
        const int b = i / (pos_cur + 1), p = i - b * (pos_cur + 1);
        s.anc[(cb0 + b) * ctx + p] = (p < pos_cur) ? old.anc[L.w_src[b] * ctx + p] : (uint8_t)L.w_src[b];
    }
    if (s.kv_stat) {     // distinct slots the NEXT step's attention reads at each of its pos_cur + 1 cached positions
        int cnt = 0;
        for (int p = lane; p <= pos_cur; p += 64) {
            unsigned seen = 0;
            for (int b = 0; b < beam; ++b)
                seen |= 1u << ((p < pos_cur) ? old.anc[L.w_src[b] * ctx + p] : (uint8_t)L.w_src[b]);
            cnt += __popc(seen);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
        if (lane == 0) { s.kv_stat[2 * cap] += (unsigned)cnt; s.kv_stat[2 * cap + 1] += (unsigned)(pos_cur + 1); }
    }
    const bool all = __all(stop);              // the caption's loop breaks when every slot has stopped
    if (lane == 0) {
        if (all) s.done[cap] = 1;
        else atomicAdd(s.alive_count, 1);
    }
}

// step 0: slot cb (= caption * beam + slot) starts with `tok` at `score`; -> whether it stopped at once
__device__ __forceinline__ bool beam_init_slot(const BeamState &s, size_t cb, int T, int tok, float score, int stop_id) {
    s.tokens[cb * T] = tok;
    s.scores[cb] = score;
    s.seq[cb] = 1.0f;
    const bool stop = tok == stop_id;
    s.stopped[cb] = stop;
    s.next_tok[cb] = tok;
    return stop;
}

// step 0 ends: `stop` of every lane (true where it holds no slot) -> done / alive_count
__device__ __forceinline__ void beam_init_done(const BeamState &s, int cap, bool stop) {
    const bool all = __all(stop);
    if (threadIdx.x == 0) {
        s.done[cap] = all;
        if (!all) atomicAdd(s.alive_count, 1);
    }
}

}  // namespace capdec
