// Lexically constrained beam search (Anderson et al. 2017) by dynamic beam allocation (Post & Vilar 2018) on the beam decode
// (capdec_decode_beam_constrained; the contract: include/capdec.h).  Every caption carries up to CON_PHRASES phrases of up to
// CON_LEN tokens that must all occur in it; every beam slot carries (met, cur, pos) -- the phrases matched, the one in
// progress and how far -- next to tokens / seq / scores / stopped.  A step differs from the plain beam's in three places:
//   * the stop token is banned while a row's phrases are not all met;
//   * a candidate belongs to the BANK of the state it leads to (tokens of phrases matched so far), and the `beam` slots are
//     handed out round-robin over the non-empty banks, highest first, each visit taking the bank's best remaining candidate;
//   * the end sorts by (phrases met, score).
// Everything else is the plain beam's: the key (scores + lp) / seq_new, the tie rule, the ancestor-table attention,
// compaction, chunking.  The logits are always materialised (decode.hip: lm_head_rows_forced), so that the logits of a
// row's special tokens come from the same arithmetic as its list.
//
// Why a short list per row is still exact:
//   1. from one row, every token outside S(state) -- the next token of cur and the first tokens of the unmet phrases, at
//      most CON_SPECIAL = 5 -- leads to the same state (met, none, 0), hence to ONE bank;
//   2. the selection takes at most `beam` candidates in all, so at most `beam` from that bank, and within a bank a
//      candidate is only ever taken after every better candidate of the bank: of the row's tokens outside S only its best
//      `beam` can be taken;
//   3. the tokens of S are read individually, whatever their rank;
//   4. the list is built with ties to the smaller column, the tie rule of the selection;
//   5. so a row's list is S followed by its best `beam` tokens outside S: at most 8 x 13 = 104 candidates per caption, two
//      per lane of one wavefront.
// With no phrases S is empty, nothing is banned, there is one bank, and the round-robin takes the best `beam` in order:
// the plain beam bit for bit (the row pass is the one logits_select_kernel runs: row_select.h's logits_row_pass; staging,
// write-back and the end are the plain beam's own code: beam_state.h and select.hip's beam_finalize_kernel).
// BeamState::diverge is not honoured here.
#include "beam_state.h"

namespace capdec {

namespace {

constexpr int CON_THREADS = 256;
constexpr int CON_NONE = 0x7fffffff;

// (a slot's state packed into one int: beam_state.h)  ph: the caption's phrase table, CON_PHRASES x CON_LEN ints
__device__ __forceinline__ int con_len(const int *ph, int c) {
    int n = 0;
    while (n < CON_LEN && ph[c * CON_LEN + n] >= 0) ++n;
    return n;
}
__device__ __forceinline__ int con_count(const int *ph) {       // phrases of the caption: its leading non-empty rows
    int n = 0;
    while (n < CON_PHRASES && ph[n * CON_LEN] >= 0) ++n;
    return n;
}
__device__ __forceinline__ int con_adv(const int *ph, int st, int t) {
    int met = con_met(st);
    const int cur = con_cur(st), pos = con_pos(st);
    if (cur >= 0 && ph[cur * CON_LEN + pos] == t) {
        if (pos + 1 == con_len(ph, cur)) return con_pack(met | (1 << cur), -1, 0);
        return con_pack(met, cur, pos + 1);
    }
    const int np = con_count(ph);
    for (int c = 0; c < np; ++c) {
        if (((met >> c) & 1) || ph[c * CON_LEN] != t) continue;
        if (con_len(ph, c) == 1) return con_pack(met | (1 << c), -1, 0);
        return con_pack(met, c, 1);
    }
    return con_pack(met, -1, 0);
}
__device__ __forceinline__ int con_bank(const int *ph, int st) {
    int b = con_pos(st);
    const int met = con_met(st);
    for (int c = 0; c < CON_PHRASES; ++c)
        if ((met >> c) & 1) b += con_len(ph, c);
    return b;
}

// The round-robin over the banks by one wavefront.  A lane offers up to two candidates (key, flat index, bank; flat CON_NONE:
// none; flat indices are unique).  -> won0 / won1: the slot the lane's candidate took, or -1.
__device__ __forceinline__ void con_round_robin(float k0, int f0, int b0, float k1, int f1, int b1, int beam, int &won0,
                                                int &won1) {
    won0 = won1 = -1;
    unsigned present = (f0 != CON_NONE ? 1u << b0 : 0u) | (f1 != CON_NONE ? 1u << b1 : 0u);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) present |= (unsigned)__shfl_xor((int)present, o, 64);
    int taken = 0;
    while (taken < beam && present) {
        unsigned pass = present;
        while (pass && taken < beam) {
            const int b = 31 - __clz(pass);
            pass &= ~(1u << b);
            // the lane's better candidate in this bank, then the wavefront's
            float v = -INFINITY;
            int i = CON_NONE, q = -1;
            if (f0 != CON_NONE && b0 == b) { v = k0; i = f0; q = 0; }
            if (f1 != CON_NONE && b1 == b && (q < 0 || better(k1, f1, v, i))) { v = k1; i = f1; q = 1; }
            float gv = v;
            int gi = i;
            wave_best(gv, gi);
            if (gi == CON_NONE) { present &= ~(1u << b); continue; }     // the bank is used up
            if (q == 0 && gi == f0) { won0 = taken; f0 = CON_NONE; }
            if (q == 1 && gi == f1) { won1 = taken; f1 = CON_NONE; }
            ++taken;
        }
    }
}

// ---- logsumexp, the special tokens' values and the best K tokens outside them, one pass over the row: row_select.h's
// logits_row_pass (what logits_select_kernel runs) under the policy below.  Row r of the launch is activation row row0 + r:
// caption (row0 + r) / rpc through cmap, slot (row0 + r) % rpc; state == nullptr (step 0): the empty state.
struct RowForced {                      // the stop token banned while phrases are unmet; the special tokens kept off the list
    static constexpr bool filtered = true;
    int ban, s0, s1, s2, s3, s4;
    bool any;                           // (false: -1 everywhere, no special token)
    __device__ __forceinline__ bool excluded(int j) const {
        return any && (j == s0 || j == s1 || j == s2 || j == s3 || j == s4);
    }
};
template <int K>
__global__ __launch_bounds__(CON_THREADS) void logits_select_forced_kernel(const float *__restrict__ logits, int ld, int V,
                                                                           int row0, float inv_temp,
                                                                           const int *__restrict__ phrases,
                                                                           const int *__restrict__ state,
                                                                           const int *__restrict__ cmap, int rpc, int beam,
                                                                           int stop_id, float *__restrict__ lse,
                                                                           float *__restrict__ top_val,
                                                                           int *__restrict__ top_idx) {
    __shared__ int ph[CON_PHRASES * CON_LEN];
    __shared__ int sp[CON_SPECIAL + 1];                          // the special tokens (-1: unused place), then the ban flag
    const int tid = threadIdx.x;
    const size_t r = blockIdx.x;
    const float *x = logits + r * ld;
    const int R = row0 + (int)r;
    const int cap = cmap ? cmap[R / rpc] : R / rpc;
    if (tid < CON_PHRASES * CON_LEN) ph[tid] = phrases[(size_t)cap * CON_PHRASES * CON_LEN + tid];
    __syncthreads();
    if (tid == 0) {
        const int st = state ? state[(size_t)cap * beam + R % rpc] : 0;
        const int met = con_met(st), cur = con_cur(st), np = con_count(ph);
        sp[0] = cur >= 0 ? ph[cur * CON_LEN + con_pos(st)] : -1;
        for (int c = 0; c < CON_PHRASES; ++c) {
            int t = (c < np && !((met >> c) & 1)) ? ph[c * CON_LEN] : -1;
            for (int q = 0; q <= c; ++q)
                if (sp[q] == t) t = -1;                          // a token has one place: the first
            sp[1 + c] = t;
        }
        sp[CON_SPECIAL] = met != (1 << np) - 1;
    }
    __syncthreads();
    RowForced pol;
    pol.s0 = sp[0]; pol.s1 = sp[1]; pol.s2 = sp[2]; pol.s3 = sp[3]; pol.s4 = sp[4];
    pol.any = (pol.s0 & pol.s1 & pol.s2 & pol.s3 & pol.s4) >= 0;
    pol.ban = sp[CON_SPECIAL] ? stop_id : -1;
    // the special tokens at their fixed places (a phrase never holds the stop token: the ban does not reach them)
    if (tid < CON_SPECIAL) {
        const int t = sp[tid];
        top_idx[r * CON_LIST + tid] = t;
        top_val[r * CON_LIST + tid] = t >= 0 ? x[t] * inv_temp : -INFINITY;
    }
    logits_row_pass<K, CON_THREADS>(x, V, inv_temp, pol, lse + r, top_val + r * CON_LIST + CON_SPECIAL,
                                    top_idx + r * CON_LIST + CON_SPECIAL);
}

// ---- step 0: one logits row per caption (prefill last position), the empty state.  lane p < CON_LIST holds place p of the
// row's list.
__global__ __launch_bounds__(64) void constrained_beam_init_kernel(BeamState s, ConstraintState cs,
                                                                   const float *__restrict__ lse,
                                                                   const float *__restrict__ top_val,
                                                                   const int *__restrict__ top_idx, int beam, int T,
                                                                   int vocab, int stop_id) {
    __shared__ int ph[CON_PHRASES * CON_LEN];
    __shared__ int w_tok[BEAM_MAX], w_cst[BEAM_MAX];
    __shared__ float w_key[BEAM_MAX];
    const int cap = blockIdx.x, lane = threadIdx.x;
    if (lane < CON_PHRASES * CON_LEN) ph[lane] = cs.phrases[(size_t)cap * CON_PHRASES * CON_LEN + lane];
    if (lane < BEAM_MAX) { w_tok[lane] = 0; w_cst[lane] = 0; w_key[lane] = -INFINITY; }
    __syncthreads();
    float key = -INFINITY;
    int flat = CON_NONE, nst = 0, bank = 0;
    if (lane < CON_SPECIAL + beam) {
        const int tok = top_idx[(size_t)cap * CON_LIST + lane];
        if ((unsigned)tok < (unsigned)vocab) {
            key = top_val[(size_t)cap * CON_LIST + lane] - lse[cap];      // log softmax
            if (key > -INFINITY) {
                flat = tok;
                nst = con_adv(ph, 0, tok);
                bank = con_bank(ph, nst);
            }
        }
    }
    int won, none;
    con_round_robin(key, flat, bank, -INFINITY, CON_NONE, 0, beam, won, none);
    if (won >= 0) { w_tok[won] = flat; w_cst[won] = nst; w_key[won] = key; }
    __syncthreads();
    bool stop = true;
    if (lane < beam) {
        const size_t cb = (size_t)cap * beam + lane;
        stop = beam_init_slot(s, cb, T, w_tok[lane], w_key[lane], stop_id);
        cs.state[cb] = w_cst[lane];
    }
    beam_init_done(s, cap, stop);
}

// ---- step i >= 1: beam_state.h's stage and commit around the states, the banks and the round-robin.  Candidate
// c < beam * CON_LIST is (b = c / CON_LIST, place p = c % CON_LIST); a lane holds candidates lane and lane + 64.
__global__ __launch_bounds__(64) void constrained_beam_step_kernel(BeamState s, ConstraintState cs,
                                                                   const float *__restrict__ lse,
                                                                   const float *__restrict__ top_val,
                                                                   const int *__restrict__ top_idx, int beam, int T,
                                                                   int ctx, int step, int pos_cur, int vocab, int stop_id,
                                                                   const int *__restrict__ cmap) {
    __shared__ struct : BeamStepLds {                           // + the phrases, the winners' and the old slots' states, the old scores
        int ph[CON_PHRASES * CON_LEN];
        int w_cst[BEAM_MAX], cst_old[BEAM_MAX];
        float sc_old[BEAM_MAX];
    } L;
    const int lane = threadIdx.x;
    const int cap = cmap ? cmap[blockIdx.x] : blockIdx.x;       // state (tokens, scores, anc ...) by original caption
    if (s.done[cap]) return;
    const size_t cb0 = (size_t)cap * beam;
    const size_t ab0 = (size_t)blockIdx.x * beam;               // lm_head outputs by (compact) activation row
    beam_stage(s, L, cap, beam, T, ctx, step, pos_cur);
    if (lane < CON_PHRASES * CON_LEN) L.ph[lane] = cs.phrases[(size_t)cap * CON_PHRASES * CON_LEN + lane];
    if (lane < BEAM_MAX) {
        const int b = lane < beam ? lane : 0;
        L.sc_old[lane] = s.scores[cb0 + b];
        L.cst_old[lane] = cs.state[cb0 + b];
        L.w_src[lane] = b; L.w_tok[lane] = 0; L.w_key[lane] = -INFINITY; L.w_cst[lane] = L.cst_old[lane];
    }
    __syncthreads();
    // the two candidates of this lane
    float key[2];
    int flat[2], ctok[2], csrc[2], nst[2], bank[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int c = lane + 64 * q;
        key[q] = -INFINITY; flat[q] = CON_NONE; ctok[q] = 0; nst[q] = 0; bank[q] = 0;
        const int cb = c / CON_LIST, p = c - cb * CON_LIST;
        csrc[q] = cb;
        if (cb >= beam || p >= CON_SPECIAL + beam) continue;
        if (L.st_old[cb]) {                                        // the single candidate: token 0, log-prob 0, the state stays
            if (p != 0) continue;
            key[q] = (L.sc_old[cb] + 0.0f) / L.seq_new[cb];
            flat[q] = cb * vocab;
            nst[q] = L.cst_old[cb];
        } else {
            const size_t arow = ab0 + cb;
            const int tok = top_idx[arow * CON_LIST + p];
            if ((unsigned)tok >= (unsigned)vocab) continue;      // an unused place
            const float logp = top_val[arow * CON_LIST + p] - lse[arow];
            const float k = (L.sc_old[cb] + logp) / L.seq_new[cb];
            if (!(k > -INFINITY)) continue;
            key[q] = k;
            ctok[q] = tok;
            flat[q] = cb * vocab + tok;
            nst[q] = con_adv(L.ph, L.cst_old[cb], tok);
        }
        bank[q] = con_bank(L.ph, nst[q]);
    }
    int won0, won1;
    con_round_robin(key[0], flat[0], bank[0], key[1], flat[1], bank[1], beam, won0, won1);
    if (won0 >= 0) { L.w_src[won0] = csrc[0]; L.w_tok[won0] = ctok[0]; L.w_key[won0] = key[0]; L.w_cst[won0] = nst[0]; }
    if (won1 >= 0) { L.w_src[won1] = csrc[1]; L.w_tok[won1] = ctok[1]; L.w_key[won1] = key[1]; L.w_cst[won1] = nst[1]; }
    __syncthreads();
    if (lane < beam) cs.state[cb0 + lane] = L.w_cst[lane];
    beam_commit(s, L, cap, beam, T, ctx, step, pos_cur, stop_id);
}

}  // namespace

int launch_logits_select_forced(hipStream_t st, const float *logits, int ld, int rows, int row0, int V, int beam,
                                float inv_temp, const ConstraintState &cs, const int *cmap, int step, int stop_id,
                                float *lse, float *top_val, int *top_idx) {
    if (rows <= 0) return 0;
    CAPDEC_CHECK(ld >= V && ld % 4 == 0 && V >= beam && cs.phrases && cs.state, "logits_select_forced: bad geometry");
    const int *state = step == 0 ? nullptr : cs.state;          // step 0: one row per caption, the empty state
    const int rpc = step == 0 ? 1 : beam;
    CAPDEC_TRY(with_topk_k(beam, "logits_select_forced", [&](auto KS) {
        hipLaunchKernelGGL(logits_select_forced_kernel<KS>, dim3(rows), dim3(CON_THREADS), 0, st, logits, ld, V, row0,
                           inv_temp, cs.phrases, state, cmap, rpc, beam, stop_id, lse, top_val, top_idx);
    }));
    CAPDEC_HIP(hipGetLastError());
    return 0;
}

int launch_constrained_beam_init(hipStream_t st, const BeamState &s, const ConstraintState &cs, const float *lse,
                                 const float *top_val, const int *top_idx, int ncap, int beam, int T, int vocab, int stop_id) {
    CAPDEC_CHECK(beam >= 1 && beam <= BEAM_MAX, "constrained beam: beam size must be in 1..8");
    CAPDEC_CHECK(cs.phrases && cs.state, "constrained beam: no constraint state");
    if (ncap <= 0) return 0;
    hipLaunchKernelGGL(constrained_beam_init_kernel, dim3(ncap), dim3(64), 0, st, s, cs, lse, top_val, top_idx, beam, T, vocab,
                       stop_id);
    CAPDEC_HIP(hipGetLastError());
    return 0;
}

int launch_constrained_beam_step(hipStream_t st, const BeamState &s, const ConstraintState &cs, const float *lse,
                                 const float *top_val, const int *top_idx, int ncap, int beam, int T, int ctx, int step,
                                 int pos_cur, int vocab, int stop_id, const int *cmap) {
    CAPDEC_TRY(beam_step_checks("constrained beam", beam, T, ctx, step, pos_cur, vocab));
    CAPDEC_CHECK(cs.phrases && cs.state, "constrained beam: no constraint state");
    if (ncap <= 0) return 0;
    hipLaunchKernelGGL(constrained_beam_step_kernel, dim3(ncap), dim3(64), beam_step_lds(beam, T, ctx), st, s, cs, lse, top_val,
                       top_idx, beam, T, ctx, step, pos_cur, vocab, stop_id, cmap);
    CAPDEC_HIP(hipGetLastError());
    return 0;
}

}  // namespace capdec
