// Classifier-free guidance on the greedy and the beam decode (capdec_decode_guided; the contract: include/capdec.h).
// Every caption is decoded twice in lock-step: from its own prefix (the cond half) and from a negative prefix (the neg
// half), both fed the same tokens.  A chunk of nc captions runs as 2 nc captions of `beam` rows -- caption j and its partner
// nc + j -- through the unchanged embedding, body, KV cache and ancestor-table attention.  A step is
//   1. the body over the 2 * na * beam activation rows: the alive captions, then their partners (the compaction map lists
//      them in that order);
//   2. lm_head_rows (decode.hip) with the partner rows -- per block of cond rows: the materialised logits of the block and
//      of its partner block, guided_combine_kernel (g = gamma * log_softmax(cond) + (1 - gamma) * log_softmax(neg), written
//      over the cond rows), the logits processors and the one-pass selection on the cond rows (process.hip);
//   3. decode_advance: the greedy / beam step kernel of select.hip on the na * beam cond rows -- the state (decode_state
//      with two halves) lives with the cond half only;
//   4. guided_mirror_kernel: the partner rows get their captions' next tokens and, for beam, the re-ordered ancestor rows.
// The step loop is decode.hip's decode_steps: 2 * beam rows per caption, a compaction map of 2 nc slots, and the partner map
// as what follows a compaction.  Call checks, per-call reset and chunking are decode.hip's too; this file keeps the four
// kernels, the prefill of both halves and the body of a step.
#include "context.h"
#include "row_select.h"

namespace capdec {

namespace {

constexpr int GD_THREADS = 256, GD_WAVES = GD_THREADS / WAVE;

// (max, sum exp(x - max)) of the lanes' partials -> the row's logsumexp, the same value in every thread: the wavefront's DPP
// tree, then the wavefronts in index order (logits_select_kernel's order)
__device__ __forceinline__ float block_logsumexp(float m, float s, float *wm, float *ws) {
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    const float M = wave_max(m);
    const float t = wave_sum(m > -INFINITY ? s * expf(m - M) : 0.f);
    if (lane == 0) { wm[wave] = M; ws[wave] = t; }
    __syncthreads();
    float Mb = wm[0];
#pragma unroll
    for (int w = 1; w < GD_WAVES; ++w) Mb = fmaxf(Mb, wm[w]);
    float S = 0.f;
#pragma unroll
    for (int w = 0; w < GD_WAVES; ++w) S += wm[w] > -INFINITY ? ws[w] * expf(wm[w] - Mb) : 0.f;
    return Mb + logf(S);
}

__device__ __forceinline__ void online4(float &m, float &s, const float4 q) {
    online_rescale(m, s, fmaxf(fmaxf(q.x, q.y), fmaxf(q.z, q.w)));
    if (m > -INFINITY) s += ((expf(q.x - m) + expf(q.y - m)) + expf(q.z - m)) + expf(q.w - m);
}

// g = gamma * (l - lse_c) + (1 - gamma) * (u - lse_u), every operation rounded on its own (equal rows: g = c up to the
// rounding of the two products)
__device__ __forceinline__ float guide(float l, float u, float lc, float lu, float gamma, float omg) {
    return __fadd_rn(__fmul_rn(gamma, __fsub_rn(l, lc)), __fmul_rn(omg, __fsub_rn(u, lu)));
}

// One workgroup per (cond, neg) row pair of materialised logits [rows, ld]: one pass for the two (max, sum exp) pairs, one
// pass -- the pair's 2 x V floats come from L2 -- that writes g over the cond row.  16-byte accesses (rows are 16-byte
// aligned: ld is a multiple of 4); the ld - V pad columns are never read or written.
__global__ __launch_bounds__(GD_THREADS) void guided_combine_kernel(float *__restrict__ cond, const float *__restrict__ neg,
                                                                    int ld, int V, float gamma) {
    __shared__ float wm[2][GD_WAVES], ws[2][GD_WAVES];
    const int r = blockIdx.x, tid = threadIdx.x;
    float *x = cond + (size_t)r * ld;
    const float *y = neg + (size_t)r * ld;
    const int V4 = V & ~3;
    float mc = -INFINITY, sc = 0.f, mu = -INFINITY, su = 0.f;
    for (int j = tid * 4; j < V4; j += GD_THREADS * 4) {
        online4(mc, sc, *reinterpret_cast<const float4 *>(x + j));
        online4(mu, su, *reinterpret_cast<const float4 *>(y + j));
    }
    for (int j = V4 + tid; j < V; j += GD_THREADS) {
        const float a = x[j], b = y[j];
        online_rescale(mc, sc, a);
        if (mc > -INFINITY) sc += expf(a - mc);
        online_rescale(mu, su, b);
        if (mu > -INFINITY) su += expf(b - mu);
    }
    const float lc = block_logsumexp(mc, sc, wm[0], ws[0]);
    const float lu = block_logsumexp(mu, su, wm[1], ws[1]);
    const float omg = 1.0f - gamma;
    for (int j = tid * 4; j < V4; j += GD_THREADS * 4) {
        const float4 a = *reinterpret_cast<const float4 *>(x + j);
        const float4 b = *reinterpret_cast<const float4 *>(y + j);
        *reinterpret_cast<float4 *>(x + j) = make_float4(guide(a.x, b.x, lc, lu, gamma, omg), guide(a.y, b.y, lc, lu, gamma, omg),
                                                         guide(a.z, b.z, lc, lu, gamma, omg), guide(a.w, b.w, lc, lu, gamma, omg));
    }
    for (int j = V4 + tid; j < V; j += GD_THREADS) x[j] = guide(x[j], y[j], lc, lu, gamma, omg);
}

// The partner rows follow their captions: block i takes alive caption cap = cmap[i] and copies, for each of its `beam` rows,
// next_tok and the first `npos` ancestor bytes (the beam step has just re-ordered them: slots are caption-relative, so the
// partner's table is a copy) to the rows of caption ncap + cap.  anc == nullptr (greedy): tokens only.
__global__ __launch_bounds__(64) void guided_mirror_kernel(int *__restrict__ next_tok, uint8_t *__restrict__ anc, int ncap,
                                                           int beam, int ctx, int npos, const int *__restrict__ cmap) {
    const int cap = cmap ? cmap[blockIdx.x] : blockIdx.x, lane = threadIdx.x;
    const size_t src = (size_t)cap * beam, dst = ((size_t)ncap + cap) * beam;
    if (lane < beam) next_tok[dst + lane] = next_tok[src + lane];
    if (!anc) return;
    for (int i = lane; i < beam * npos; i += 64) {
        const int b = i / npos, p = i - b * npos;
        anc[(dst + b) * ctx + p] = anc[(src + b) * ctx + p];
    }
}

// cmap[na + i] = cmap[i] + ncap: the partners of the alive captions, in the same order, behind them
__global__ void guided_partner_map_kernel(int *__restrict__ cmap, int na, int ncap) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < na) cmap[na + i] = cmap[i] + ncap;
}

// h[(c, i)] = neg[(c, i)] + wpe[i] for the n captions' negative prefixes; cap_nv = float4s between two captions' prefixes
// (0: one prefix serves all)
__global__ void guided_embed_neg_kernel(const float *__restrict__ neg, size_t cap_nv, const float *__restrict__ wpe,
                                        float *__restrict__ h, int n, int P, int nv) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * P * nv) return;
    const int c = i % nv, p = (i / nv) % P, cap = i / (nv * P);
    const float4 a = reinterpret_cast<const float4 *>(neg)[cap * cap_nv + (size_t)p * nv + c];
    const float4 w = reinterpret_cast<const float4 *>(wpe + (size_t)p * nv * 4)[c];
    reinterpret_cast<float4 *>(h)[i] = make_float4(a.x + w.x, a.y + w.y, a.z + w.z, a.w + w.w);
}

}  // namespace

int launch_guided_combine(hipStream_t st, float *cond, const float *neg, int ld, int rows, int V, float gamma) {
    if (rows <= 0) return 0;
    CAPDEC_CHECK(ld >= V && ld % 4 == 0 && (((uintptr_t)cond | (uintptr_t)neg) & 15) == 0, "guided_combine: bad geometry");
    hipLaunchKernelGGL(guided_combine_kernel, dim3(rows), dim3(GD_THREADS), 0, st, cond, neg, ld, V, gamma);
    CAPDEC_HIP(hipGetLastError());
    return 0;
}

namespace {

int launch_guided_mirror(hipStream_t st, int *next_tok, uint8_t *anc, int nact, int ncap, int beam, int ctx, int npos,
                         const int *cmap) {
    if (nact <= 0) return 0;
    CAPDEC_CHECK(beam >= 1 && beam <= 64 && npos >= 0 && npos <= ctx, "guided_mirror: bad geometry");
    hipLaunchKernelGGL(guided_mirror_kernel, dim3(nact), dim3(64), 0, st, next_tok, anc, ncap, beam, ctx, npos, cmap);
    CAPDEC_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------- the driver: both halves through decode_steps
int guided_chunk(capdec_ctx *c, const float *prefix, const float *neg, size_t neg_stride, int nc, const DecodeCall &a,
                 float gamma) {
    const Gpt2 &g = c->gpt;
    const int d = g.d, P = a.P, T = a.T, beam = a.beam, ctx = P + T - 1;
    const int k = beam;                             // candidates kept per cond row
    const float inv_temp = 1.0f / (a.temperature > 0.f ? a.temperature : 1.0f);
    const bool proc = processors_on(c, false);
    DecodeState s;
    CAPDEC_TRY(decode_state(c, nc, a, 2, &s));

    // the guided selection over R cond rows (partners at hn), the step kernel of the decode on the cond half, then the mirror:
    // ncap_act captions are in the batch, npos ancestor positions are valid after the step
    auto select_and_advance = [&](const float *hc, const float *hn, int ldh, int R, int step, int hbeam, const int *cmap,
                                  int ncap_act, int npos) -> int {
        s.gs.cmap = cmap;
        CAPDEC_TRY(lm_head_rows(c, hc, ldh, R, k, inv_temp, a, s.gs, proc, step, hbeam, s.hist, hn, gamma));
        CAPDEC_TRY(decode_advance(c, a, s, R, step, k, cmap));
        ProfScope ps(c, F_GUIDED);
        return launch_guided_mirror(c->stream, c->next_tok.as<int>(), s.anc, ncap_act, nc, beam, ctx, npos, cmap);
    };

    // ---- step 0: prefill both prefixes (captions 0..nc-1 and their partners nc..2nc-1), logits of the last prefix rows
    float *h = c->h.as<float>();
    {
        ProfScope ps(c, F_EMBED);
        CAPDEC_TRY(launch_embed_prefix(c->stream, prefix, g.wpe, h, nc, P, 0, d));
        const int tot = nc * P * (d / 4);
        hipLaunchKernelGGL(guided_embed_neg_kernel, dim3((tot + 255) / 256), dim3(256), 0, c->stream, neg, neg_stride / 4,
                           g.wpe, h + (size_t)nc * P * d, nc, P, d / 4);
        CAPDEC_HIP(hipGetLastError());
    }
    StepShape sp{};
    sp.prefill = true;
    sp.ncap = 2 * nc;
    sp.P = P;
    sp.beam = beam;
    CAPDEC_TRY(gpt2_body(c, sp, s.kv));
    CAPDEC_TRY(select_and_advance(h + (size_t)(P - 1) * d, h + ((size_t)nc * P + P - 1) * d, P * d, nc, 0, 1, nullptr, nc, 0));

    // ---- steps 1..T-1: 2 * beam rows per caption (rows are counted as launched, both halves); a new compaction map gets
    // the partners of its captions listed behind them
    const StepLoop loop{nc, 1, T, 2 * beam, c->done.as<uint8_t>(), 2 * nc};
    auto partners = [&](int *cmap, int na) -> int {
        hipLaunchKernelGGL(guided_partner_map_kernel, dim3((na + 255) / 256), dim3(256), 0, c->stream, cmap, na, nc);
        CAPDEC_HIP(hipGetLastError());
        return 0;
    };
    CAPDEC_TRY(decode_steps(c, loop, partners, [&](int i, int na, const int *cmap) -> int {
        const int pos = P + i - 1;   // position of the token fed this step
        const int arows = na * beam; // cond rows; the step launches 2 * arows
        {
            ProfScope ps(c, F_EMBED);
            CAPDEC_TRY(launch_embed_tokens(c->stream, c->next_tok.as<int>(), g.wte, g.wpe + (size_t)pos * d, h, 2 * arows, d,
                                           cmap, beam));
        }
        CAPDEC_TRY(gpt2_step(c, s.kv, 2 * arows, beam, pos + 1, s.anc, cmap));
        return select_and_advance(h, h + (size_t)arows * d, d, arows, i, beam, cmap, na, pos + 1);
    }));
    if (!a.greedy) {
        ProfScope ps(c, F_SELECT);
        CAPDEC_TRY(launch_beam_finalize(c->stream, s.bs, nc, beam, T, a.ids, a.lens, a.scores, a.order));
    }
    return 0;
}

}  // namespace

}  // namespace capdec

using namespace capdec;

extern "C" int capdec_decode_guided(capdec_ctx *c, const float *prefix, const float *neg_prefix, int neg_n, int n, int P,
                                    int beam, float guidance_scale, int stop_id, int alt_stop_id, int entry_length,
                                    float temperature, int32_t *ids, int32_t *lens, float *scores, int32_t *order) {
    const int T = entry_length;
    CAPDEC_CHECK(c, "decode_guided: null context");
    CAPDEC_CHECK(guidance_scale >= 1.0f && guidance_scale <= 3.0e38f, "decode_guided: guidance_scale must be finite and >= 1");
    CAPDEC_CHECK(beam >= 1 && beam <= 8, "decode_guided: beam size must be in 1..8");
    CAPDEC_CHECK(n >= 0 && (neg_n == 1 || neg_n == n), "decode_guided: neg_n must be 1 or n");
    CAPDEC_CHECK(n == 0 || (prefix && neg_prefix && ids && lens && (beam == 1 || scores)), "decode_guided: null argument");
    if (guidance_scale == 1.0f)         // off: the plain call, no negative rows
        return beam == 1 ? capdec_decode_greedy(c, prefix, n, P, stop_id, alt_stop_id, T, ids, lens)
                         : capdec_decode_beam(c, prefix, n, P, beam, stop_id, T, temperature, ids, lens, scores, order);
    const char *who = "decode_guided";
    CAPDEC_TRY(decode_call_checks(c, who, CK_LOADED | CK_SIZES | CK_CONTEXT | CK_HEAD_DIM, n, P, T, (long long)P + T - 1));
    CAPDEC_CHECK(c->gpt.vocab >= beam, "decode_guided: vocabulary smaller than the beam");
    CAPDEC_TRY(decode_call_checks(c, who, CK_BIAS, n, P, T, 0));
    const int d = c->gpt.d, ctx = P + T - 1;
    // a caption and its partner share a chunk: the partner's K/V counts against the budget as much again.  (The fused
    // lm_head never runs here.)
    const size_t kv_per_cap = (size_t)beam * ctx * d * 2 * (c->gemm_mode == GEMM_BF16 ? 2 : 4) * c->gpt.n_layer;
    int chunk = 0;
    CAPDEC_TRY(decode_call_begin(c, n, 1, beam > 1 ? n : 0, beam, ctx, kv_per_cap, 0, &chunk));
    if (n == 0) return 0;
    DecodeCall call;
    call.P = P; call.beam = beam; call.greedy = beam == 1; call.stop_id = stop_id; call.alt_stop_id = beam == 1 ? alt_stop_id : -1;
    call.T = T; call.temperature = temperature;
    call.ids = ids; call.lens = lens; call.scores = scores; call.order = order;
    const size_t neg_stride = neg_n == 1 ? 0 : (size_t)P * d;
    for (int c0 = 0; c0 < n; c0 += chunk)
        CAPDEC_TRY(guided_chunk(c, prefix + (size_t)c0 * P * d, neg_prefix + (size_t)c0 * neg_stride, neg_stride,
                                std::min(chunk, n - c0), chunk_call(call, c0), guidance_scale));
    CAPDEC_HIP(hipStreamSynchronize(c->stream));
    return 0;
}
