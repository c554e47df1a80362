// Contrastive search (Su et al. 2022; `penalty_alpha` / `top_k` of transformers) on the beam layout
// (capdec_decode_contrastive; the contract: include/capdec.h).  It is the one decode that reads hidden states: every
// caption keeps hist [ctx, d], ln_f of each position of its chosen path, L2-normalised.  A step is
//   1. the lm_head over ONE row per caption -- the residual row of the candidate chosen last (ContrastState::sel, compact
//      like the activations) -> the K best tokens v_c, their logits and the row's logsumexp: greedy's head, not beam's;
//   2. the K candidates through gpt2_body as K beam rows (row = caption * K + c) that attend to the chosen path's K/V
//      through the ancestor table;
//   3. contrast_select_kernel: ln_f + normalise of the K rows, max cosine against the `pos` history rows, score, arg-max,
//      then everything the next step needs -- token, length, done, alive count, anc[all K rows][pos] = winner (the winner's
//      K/V at `pos` becomes the path's), the history row `pos`, the winner's residual row.
// The [K, pos] similarities live in registers and LDS only.  Chunking, compaction and the adaptive poll are decode.hip's.
#include "context.h"

namespace capdec {

constexpr int CS_WAVES = 4;

// one wavefront: out[0..d) = ln_f(x) / max(||ln_f(x)||, 1e-12) (out: LDS or global; every lane re-reads only what it wrote)
__device__ __forceinline__ void lnf_unit_row(const float *__restrict__ x, const float *__restrict__ w,
                                             const float *__restrict__ b, float eps, int d, float *out, int lane) {
    float s = 0.f;
    for (int e = lane; e < d; e += WAVE) s += x[e];
    const float mean = wave_sum(s) / (float)d;
    float v = 0.f;
    for (int e = lane; e < d; e += WAVE) { const float t = x[e] - mean; v += t * t; }
    const float rstd = 1.0f / sqrtf(wave_sum(v) / (float)d + eps);
    float n2 = 0.f;
    for (int e = lane; e < d; e += WAVE) {
        const float y = (x[e] - mean) * rstd * w[e] + b[e];
        out[e] = y;
        n2 += y * y;
    }
    const float inv = 1.0f / fmaxf(sqrtf(wave_sum(n2)), 1e-12f);
    for (int e = lane; e < d; e += WAVE) out[e] *= inv;
}

// ---- prefill: one wavefront per prefix row
__global__ __launch_bounds__(64 * CS_WAVES) void contrast_prefill_kernel(ContrastState s, const float *__restrict__ h,
                                                                         const float *__restrict__ lnw,
                                                                         const float *__restrict__ lnb, float eps, int ncap,
                                                                         int P) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * CS_WAVES + (threadIdx.x >> 6);
    if (row >= ncap * P) return;
    const int cap = row / P, p = row - cap * P, d = s.d;
    const float *x = h + (size_t)row * d;
    lnf_unit_row(x, lnw, lnb, eps, d, s.hist + ((size_t)cap * s.ctx + p) * d, lane);
    if (p == P - 1)
        for (int e = lane; e < d; e += WAVE) s.last[(size_t)cap * d + e] = s.sel[(size_t)cap * d + e] = x[e];
}

int launch_contrast_prefill(hipStream_t st, const ContrastState &s, const float *h, const float *lnw, const float *lnb,
                            float eps, int ncap, int P) {
    if (ncap <= 0) return 0;
    hipLaunchKernelGGL(contrast_prefill_kernel, dim3((ncap * P + CS_WAVES - 1) / CS_WAVES), dim3(64 * CS_WAVES), 0, st, s, h,
                       lnw, lnb, eps, ncap, P);
    CAPDEC_HIP(hipGetLastError());
    return 0;
}

// ---- one selection: a block of four wavefronts per live caption.  The wavefronts share the K candidate vectors through
// LDS and take the history rows j = wave, wave + 4, ...: a row is read once (float4 per lane), gives K dot products, each
// reduced over the wavefront; the running maxima stay in registers until the four wavefronts' are joined.
template <int K>
__global__ __launch_bounds__(64 * CS_WAVES) void contrast_select_kernel(ContrastState s, const float *__restrict__ h,
                                                                        const float *__restrict__ lnw,
                                                                        const float *__restrict__ lnb, float eps,
                                                                        const float *__restrict__ lse,
                                                                        const float *__restrict__ top_val,
                                                                        const int *__restrict__ top_idx, float alpha,
                                                                        int step, int pos, const int *__restrict__ cmap) {
    // all LDS is dynamic (a static array in front would move the base off the 16 bytes the float4 reads need):
    // [K][d] the candidates, ln_f'ed and normalised | [CS_WAVES][K] the wavefronts' maxima | the winner
    extern __shared__ __attribute__((aligned(16))) float cs_cand[];
    float(*wmax)[K] = reinterpret_cast<float(*)[K]>(cs_cand + (size_t)K * s.d);
    int &win = *reinterpret_cast<int *>(cs_cand + (size_t)K * s.d + CS_WAVES * K);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int act = blockIdx.x, cap = cmap ? cmap[act] : act;            // activation rows are compact, the state is not
    if (s.done[cap]) return;
    const int d = s.d, nv = d >> 2;
    const float *rows = h + (size_t)act * K * d;
    for (int c = wave; c < K; c += CS_WAVES) lnf_unit_row(rows + (size_t)c * d, lnw, lnb, eps, d, cs_cand + c * d, lane);
    __syncthreads();
    float mx[K];
#pragma unroll
    for (int c = 0; c < K; ++c) mx[c] = -INFINITY;
    const float *H = s.hist + (size_t)cap * s.ctx * d;
    for (int j = wave; j < pos; j += CS_WAVES) {
        const float4 *hr = reinterpret_cast<const float4 *>(H + (size_t)j * d);
        float dot[K];
#pragma unroll
        for (int c = 0; c < K; ++c) dot[c] = 0.f;
        for (int e = lane; e < nv; e += WAVE) {
            const float4 hv = hr[e];
#pragma unroll
            for (int c = 0; c < K; ++c) {
                const float4 cv = reinterpret_cast<const float4 *>(cs_cand + c * d)[e];
                dot[c] += hv.x * cv.x + hv.y * cv.y + hv.z * cv.z + hv.w * cv.w;
            }
        }
#pragma unroll
        for (int c = 0; c < K; ++c) mx[c] = fmaxf(mx[c], wave_sum(dot[c]));
    }
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < K; ++c) wmax[wave][c] = mx[c];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int w = 0;
        float best = -INFINITY, bp = 0.f, bs = 0.f;
        const float l = lse[act];
        for (int c = 0; c < K; ++c) {
            float sim = wmax[0][c];
            for (int q = 1; q < CS_WAVES; ++q) sim = fmaxf(sim, wmax[q][c]);
            const float p = expf(top_val[(size_t)act * K + c] - l);
            const float score = __fsub_rn(__fmul_rn(1.0f - alpha, p), __fmul_rn(alpha, sim));
            if (c == 0 || score > best) { best = score; w = c; bp = p; bs = sim; }      // a tie keeps the lower c
        }
        const int tok = top_idx[(size_t)act * K + w];
        s.ids[(size_t)cap * s.T + step] = tok;
        s.lens[cap] = step + 1;
        if (s.trace) {
            s.trace[((size_t)cap * s.T + step) * 2] = bp;
            s.trace[((size_t)cap * s.T + step) * 2 + 1] = bs;
        }
        if (tok == s.stop_id || tok == s.alt_stop_id) s.done[cap] = 1;
        else atomicAdd(s.alive_count, 1);
        win = w;
    }
    __syncthreads();
    const int w = win;
    if (threadIdx.x < K) s.anc[((size_t)cap * K + threadIdx.x) * s.ctx + pos] = (uint8_t)w;
    const float4 *src = reinterpret_cast<const float4 *>(rows + (size_t)w * d);
    const float4 *unit = reinterpret_cast<const float4 *>(cs_cand + w * d);
    float4 *hn = reinterpret_cast<float4 *>(s.hist + ((size_t)cap * s.ctx + pos) * d);
    float4 *la = reinterpret_cast<float4 *>(s.last + (size_t)cap * d), *se = reinterpret_cast<float4 *>(s.sel + (size_t)act * d);
    for (int e = threadIdx.x; e < nv; e += 64 * CS_WAVES) {
        hn[e] = unit[e];
        la[e] = se[e] = src[e];
    }
}

int launch_contrast_select(hipStream_t st, const ContrastState &s, const float *h, const float *lnw, const float *lnb,
                           float eps, const float *lse, const float *top_val, const int *top_idx, int nact, int K,
                           float alpha, int step, int pos, const int *cmap) {
    CAPDEC_CHECK(s.d % 4 == 0 && (size_t)K * s.d * 4 <= 48 * 1024, "contrastive: model width too large for the candidates in LDS");
    CAPDEC_CHECK(step >= 0 && step < s.T && pos >= 1 && pos < s.ctx, "contrastive: step or position out of range");
    if (nact <= 0) return 0;
    CAPDEC_TRY(with_topk_k(K, "contrastive", [&](auto kc) {
        constexpr int KC = decltype(kc)::value;
        hipLaunchKernelGGL(contrast_select_kernel<KC>, dim3(nact), dim3(64 * CS_WAVES),
                           ((size_t)KC * s.d + CS_WAVES * KC + 4) * 4, st, s, h, lnw, lnb, eps, lse, top_val, top_idx, alpha,
                           step, pos, cmap);
    }));
    CAPDEC_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------- the driver: decode_chunk's loop, one
// position later -- every emitted token is chosen AFTER its own candidate pass, so step t feeds position P + t
static int contrastive_chunk(capdec_ctx *c, const float *prefix, int nc, const DecodeCall &a, int K, float alpha,
                             float *trace) {
    const Gpt2 &g = c->gpt;
    const int d = g.d, P = a.P, T = a.T, ctx = P + T, rows = nc * K;
    const bool proc = processors_on(c, false);
    KvCache kv;
    CAPDEC_TRY(ensure_kv(c, kv, rows, ctx));
    kv.fixed_variant = c->batch_invariant;
    kv.prefix_len = P;
    CAPDEC_TRY(ensure_body_ws(c, std::max(nc * P, rows), d));
    CAPDEC_TRY(c->alive.ensure(sizeof(int)));
    CAPDEC_TRY(c->done.ensure((size_t)nc));
    CAPDEC_TRY(c->anc.ensure((size_t)rows * ctx));
    CAPDEC_TRY(c->cs_hist.ensure((size_t)nc * ctx * d * 4));
    CAPDEC_TRY(c->cs_last.ensure((size_t)nc * d * 4));
    CAPDEC_TRY(c->cs_sel.ensure((size_t)nc * d * 4));
    CAPDEC_TRY(c->cmap.ensure(((size_t)nc + 1) * 4));
    ContrastState s;
    s.ids = a.ids; s.lens = a.lens; s.trace = trace;
    s.done = c->done.as<uint8_t>();
    s.anc = c->anc.as<uint8_t>();
    s.alive_count = c->alive.as<int>();
    s.hist = c->cs_hist.as<float>(); s.last = c->cs_last.as<float>(); s.sel = c->cs_sel.as<float>();
    s.T = T; s.ctx = ctx; s.d = d; s.stop_id = a.stop_id; s.alt_stop_id = a.alt_stop_id;
    GreedyState gs;             // what lm_head_rows reads of it: the compaction in force
    gs.ids = a.ids; gs.lens = a.lens; gs.T = T; gs.stop_id = a.stop_id; gs.alt_stop_id = a.alt_stop_id;
    CAPDEC_HIP(hipMemsetAsync(a.ids, 0, (size_t)nc * T * 4, c->stream));
    CAPDEC_HIP(hipMemsetAsync(a.lens, 0, (size_t)nc * 4, c->stream));
    if (trace) CAPDEC_HIP(hipMemsetAsync(trace, 0, (size_t)nc * T * 2 * 4, c->stream));
    CAPDEC_HIP(hipMemsetAsync(s.done, 0, (size_t)nc, c->stream));
    CAPDEC_HIP(hipMemsetAsync(s.anc, 0, (size_t)rows * ctx, c->stream));

    // ---- prefill: positions 0..P-1 (their K/V shared by the K rows as for beams), the history of the prefix
    { ProfScope ps(c, F_EMBED); CAPDEC_TRY(launch_embed_prefix(c->stream, prefix, g.wpe, c->h.as<float>(), nc, P, 0, d)); }
    StepShape sp{};
    sp.prefill = true;
    sp.ncap = nc;
    sp.P = P;
    sp.beam = K;
    CAPDEC_TRY(gpt2_body(c, sp, kv));
    { ProfScope ps(c, F_CONTRAST); CAPDEC_TRY(launch_contrast_prefill(c->stream, s, c->h.as<float>(), g.lnfw, g.lnfb, g.eps, nc, P)); }

    // ---- steps 0..T-1 (poll cadence and compaction: decode_chunk)
    int na = nc, next_poll = 1, backoff = 1, last_alive = nc + 1;
    const int *cmap = nullptr;
    for (int t = 0; t < T; ++t) {
        if (t >= next_poll) {
            int alive = 0;
            CAPDEC_TRY(poll_alive(c, &alive));
            if (alive == 0) break;
            const int rows_now = alive * K;
            const int base = rows_now >= 8192 ? 1 : rows_now >= 2048 ? 2 : rows_now >= 512 ? 4 : 8;
            backoff = alive < last_alive ? 1 : std::min(8, backoff * 2);
            last_alive = alive;
            next_poll = t + std::min(8, std::max(base, backoff));
            if (c->compact && alive <= na - std::max(1, na / 32)) {
                ProfScope ps(c, F_SELECT);
                CAPDEC_TRY(launch_compact_alive(c->stream, s.done, nc, c->cmap.as<int>(), c->cmap.as<int>() + nc));
                na = alive;
                cmap = c->cmap.as<int>();
                c->stat_compactions += 1;
                CAPDEC_TRY(launch_gather_rows(c->stream, s.last, cmap, s.sel, na, d));      // the lm_head's rows follow
            }
        }
        const int pos = P + t, arows = na * K;
        c->stat_steps = std::max(c->stat_steps, t + 1);
        c->stat_row_steps += arows;
        if ((int)c->stat_step_rows.size() < t + 1) c->stat_step_rows.resize(t + 1, 0);
        c->stat_step_rows[t] += arows;
        CAPDEC_HIP(hipMemsetAsync(c->alive.p, 0, sizeof(int), c->stream));
        gs.cmap = cmap;
        if (proc) CAPDEC_TRY(lm_head_rows(c, s.sel, d, na, K, 1.0f, a, gs, true, t, 1, a.ids));
        else CAPDEC_TRY(lm_head_select(c, s.sel, d, na, K, 1.0f));
        {   // the candidate lists are laid out like the activation rows: [na, K]
            ProfScope ps(c, F_EMBED);
            CAPDEC_TRY(launch_embed_tokens(c->stream, c->topi.as<int>(), g.wte, g.wpe + (size_t)pos * d, c->h.as<float>(),
                                           arows, d));
        }
        StepShape sd{};
        sd.prefill = false;
        sd.rows = arows;
        sd.beam = K;
        sd.L = pos + 1;
        sd.anc = s.anc;
        sd.anc_stride = ctx;
        sd.cmap = cmap;
        CAPDEC_TRY(gpt2_body(c, sd, kv));
        ProfScope ps(c, F_CONTRAST);
        CAPDEC_TRY(launch_contrast_select(c->stream, s, c->h.as<float>(), g.lnfw, g.lnfb, g.eps, c->lse.as<float>(),
                                          c->topv.as<float>(), c->topi.as<int>(), na, K, alpha, t, pos, cmap));
    }
    return 0;
}

}  // namespace capdec

using namespace capdec;

extern "C" int capdec_decode_contrastive(capdec_ctx *c, const float *prefix, int n, int P, int top_k, float penalty_alpha,
                                         int stop_id, int alt_stop_id, int entry_length, int32_t *ids, int32_t *lens,
                                         float *trace) {
    CAPDEC_CHECK(c && (n == 0 || (prefix && ids && lens)), "decode_contrastive: null argument");
    CAPDEC_CHECK(c->gpt.loaded, "decode_contrastive: GPT-2 weights not loaded");
    CAPDEC_CHECK(top_k >= 1 && top_k <= 8, "decode_contrastive: top_k must be in 1..8");
    CAPDEC_CHECK(penalty_alpha >= 0.f && penalty_alpha <= 1.f, "decode_contrastive: penalty_alpha must be in [0, 1]");
    const int T = entry_length;
    CAPDEC_CHECK(n >= 0 && P >= 1 && T >= 1, "decode_contrastive: bad sizes");
    CAPDEC_CHECK((long long)P + T <= c->gpt.n_pos, "decode_contrastive: prefix + entry_length exceeds n_positions");
    CAPDEC_CHECK((long long)P + T <= 1024, "decode_contrastive: context > 1024 not supported");
    CAPDEC_CHECK(c->gpt.d / c->gpt.n_head == 64, "decode_contrastive: head_dim must be 64");
    CAPDEC_CHECK(c->gpt.vocab >= top_k, "decode_contrastive: vocabulary smaller than top_k");
    CAPDEC_CHECK(c->proc_bias_n == 0 || c->proc_bias_n == c->gpt.vocab,
                 "decode_contrastive: the logit bias was set for another vocabulary");
    CAPDEC_HIP(hipSetDevice(c->device));
    c->stat_steps = 0;
    c->stat_compactions = 0;
    c->stat_chunks = 0;
    c->stat_row_steps = 0;
    c->stat_step_rows.clear();
    c->stat_kv_slots = c->stat_kv_pos = 0.0;
    c->kvstat_n = 0;
    if (n == 0) return 0;
    const int ctx = P + T, d = c->gpt.d;
    const int chunk = chunk_captions(c, n, top_k, ctx, (size_t)ctx * d * 4);       // the history counts against the budget
    c->stat_chunks = (n + chunk - 1) / chunk;
    CAPDEC_TRY(c->lmflag.ensure(((size_t)chunk + 2) * 4));      // (lm_head_select's second-pass bookkeeping, as decode_common)
    CAPDEC_HIP(hipMemsetAsync(c->lmflag.p, 0, 2 * sizeof(int), c->stream));
    c->lmflag_live = false;
    c->k3_off = false;
    c->k3_rows = 0;
    DecodeCall a;
    a.P = P; a.stop_id = stop_id; a.alt_stop_id = alt_stop_id; a.T = T;
    for (int c0 = 0; c0 < n; c0 += chunk) {
        const int nc = std::min(chunk, n - c0);
        a.ids = ids + (size_t)c0 * T;
        a.lens = lens + c0;
        a.cap_off = c0;
        CAPDEC_TRY(contrastive_chunk(c, prefix + (size_t)c0 * P * d, nc, a, top_k, penalty_alpha,
                                     trace ? trace + (size_t)c0 * T * 2 : nullptr));
    }
    CAPDEC_HIP(hipStreamSynchronize(c->stream));
    return 0;
}
