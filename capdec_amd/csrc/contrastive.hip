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
// The [K, pos] similarities live in registers and LDS only.  The step loop is decode.hip's decode_steps, from step 0 with K
// rows per caption; after a compaction the lm_head's rows (sel) are gathered again through the new map.  Call checks,
// per-call reset and chunking are decode.hip's too.
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

    // ---- steps 0..T-1: K rows per caption; after a compaction the lm_head's rows follow the new map
    const StepLoop loop{nc, 0, T, K, s.done, nc};
    auto gather_sel = [&](int *cmap, int na) -> int { return launch_gather_rows(c->stream, s.last, cmap, s.sel, na, d); };
    return decode_steps(c, loop, gather_sel, [&](int t, int na, const int *cmap) -> int {
        const int pos = P + t, arows = na * K;
        gs.cmap = cmap;
        if (proc) CAPDEC_TRY(lm_head_rows(c, s.sel, d, na, K, 1.0f, a, gs, true, t, 1, a.ids));
        else CAPDEC_TRY(lm_head_select(c, s.sel, d, na, K, 1.0f));
        {   // the candidate lists are laid out like the activation rows: [na, K]
            ProfScope ps(c, F_EMBED);
            CAPDEC_TRY(launch_embed_tokens(c->stream, c->topi.as<int>(), g.wte, g.wpe + (size_t)pos * d, c->h.as<float>(),
                                           arows, d));
        }
        CAPDEC_TRY(gpt2_step(c, kv, arows, K, pos + 1, s.anc, cmap));
        ProfScope ps(c, F_CONTRAST);
        return launch_contrast_select(c->stream, s, c->h.as<float>(), g.lnfw, g.lnfb, g.eps, c->lse.as<float>(),
                                      c->topv.as<float>(), c->topi.as<int>(), na, K, alpha, t, pos, cmap);
    });
}

}  // namespace capdec

using namespace capdec;

extern "C" int capdec_decode_contrastive(capdec_ctx *c, const float *prefix, int n, int P, int top_k, float penalty_alpha,
                                         int stop_id, int alt_stop_id, int entry_length, int32_t *ids, int32_t *lens,
                                         float *trace) {
    const char *who = "decode_contrastive";
    CAPDEC_CHECK(c && (n == 0 || (prefix && ids && lens)), "decode_contrastive: null argument");
    CAPDEC_TRY(decode_call_checks(c, who, CK_LOADED, n, 0, 0, 0));
    CAPDEC_CHECK(top_k >= 1 && top_k <= 8, "decode_contrastive: top_k must be in 1..8");
    CAPDEC_CHECK(penalty_alpha >= 0.f && penalty_alpha <= 1.f, "decode_contrastive: penalty_alpha must be in [0, 1]");
    const int T = entry_length;
    CAPDEC_TRY(decode_call_checks(c, who, CK_SIZES | CK_CONTEXT | CK_HEAD_DIM, n, P, T, (long long)P + T));
    CAPDEC_CHECK(c->gpt.vocab >= top_k, "decode_contrastive: vocabulary smaller than top_k");
    CAPDEC_TRY(decode_call_checks(c, who, CK_BIAS, n, P, T, 0));
    // every emitted token is chosen AFTER its own candidate pass: the context is one position longer than the plain decode's,
    // and step 0 is a loop step.  The history counts against the KV budget; the lm_head sees one row per caption.
    const int ctx = P + T, d = c->gpt.d;
    int chunk = 0;
    CAPDEC_TRY(decode_call_begin(c, n, 0, 0, top_k, ctx, (size_t)ctx * d * 4, 1, &chunk));
    if (n == 0) return 0;
    DecodeCall call;
    call.P = P; call.stop_id = stop_id; call.alt_stop_id = alt_stop_id; call.T = T;
    call.ids = ids; call.lens = lens;
    for (int c0 = 0; c0 < n; c0 += chunk)
        CAPDEC_TRY(contrastive_chunk(c, prefix + (size_t)c0 * P * d, std::min(chunk, n - c0), chunk_call(call, c0), top_k,
                                     penalty_alpha, trace ? trace + (size_t)c0 * T * 2 : nullptr));
    CAPDEC_HIP(hipStreamSynchronize(c->stream));
    return 0;
}
