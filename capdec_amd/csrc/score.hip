// capdec_score: teacher-forced log-probabilities of GIVEN captions, with the [rows, vocab] logits never in HBM.
//
// Contract (include/capdec.h; tests/score_def.py restates it in fp64).  Caption r has prefix rows prefix[r] [P, d], token
// ids tok[r, 0..L) and a length len[r] in 0..L.  The model input is cat(prefix[r], wte(tok[r, :len[r]-1])) + wpe, and for
// i < len[r]
//     logp[r, i] = s[tok[r, i]] - logsumexp(s),   s = logits at position P-1+i, times 1 / temperature
// (`logits[:, P-1:-1]` against `tokens` of reference train.py:349; the `softmax().log()` of generate_beam; the logp of
// capdec_decode_sample).  Positions i >= len[r] get 0; a label equal to ignore_id gets 0 and is not counted (-1: none);
// sum[r] / count[r] are taken over the counted positions; top1[r, i] is the arg-max id.  An id outside [0, V) is never an
// address: as an input it looks up row 0 and taints the caption from the position it feeds on (logp NaN, sum NaN), as a
// label it gives NaN at its own position.  len[r] = 0 is legal (sum 0, count 0).
//
// Path, per chunk (a run of whole captions in input order; nc captions x S = P + Lc - 1 positions <= CAPDEC_SCORE_ROWS, Lc the
// chunk's own longest len):
//   score_embed_kernel    h[c, p] = (p < P ? prefix[c, p] : wte[tok[c, p - P]]) + wpe[p]; positions past a caption's own
//                         inputs lie behind the causal mask of every row that is scored, so they need no attention mask
//   gpt2_body             the decode loop's prefill, unchanged (beam 1)
//   launch_gather_rows    the R = sum(len) scored rows (c, P-1+i) of h -> [R, d]
//   lm_head_select, k = 1 ln_f + the fused lm_head + merge, exactly as greedy decode runs them -> lse [R], topi [R]
//   label_logit_kernel    the one value per row the fused head does not keep: ln_f(row) . wte[label]
//   score_finish_kernel   logp = logit / temperature - lse, ignore_id, taint, scatter to [n, L], per-caption sum / count
// Per scored row the head moves ~6 KB here (the row of h, one row of wte) against 201 KB of fp32 logits at GPT-2's vocabulary.
#include <climits>

#include "context.h"

namespace capdec {

namespace {

constexpr int SC_MAXV = 4;       // float4s per lane: d <= 1024 (launch_layernorm's limit)

__global__ void score_embed_kernel(const float *__restrict__ prefix, const int *__restrict__ tok,
                                   const int *__restrict__ lens, const float *__restrict__ wte,
                                   const float *__restrict__ wpe, float *__restrict__ h, int *__restrict__ bad, int nc, int P,
                                   int S, int L, int V, int nv) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nc * S * nv) return;
    const int c = i % nv, p = (i / nv) % S, r = i / (nv * S);
    float4 a;
    if (p < P) {
        a = reinterpret_cast<const float4 *>(prefix)[((size_t)r * P + p) * nv + c];
    } else {
        const int j = p - P;                         // j <= S - 1 - P = Lc - 2 <= L - 2: inside the caption's row of `tok`
        int t = tok[(size_t)r * L + j];
        if (t < 0 || t >= V) {                       // never an address; a real input (not padding) taints positions > j
            if (c == 0 && j < lens[r] - 1) atomicMin(&bad[r], j + 1);
            t = 0;
        }
        a = reinterpret_cast<const float4 *>(wte)[(size_t)t * nv + c];
    }
    const float4 w = reinterpret_cast<const float4 *>(wpe)[(size_t)p * nv + c];
    reinterpret_cast<float4 *>(h)[i] = make_float4(a.x + w.x, a.y + w.y, a.z + w.z, a.w + w.w);
}

// how the lm_head GEMM of the mode sees an operand (bf16x3.h: x3_store_quad), so that logit - lse mixes no two precisions
enum ScoreRound { SR_NONE = 0, SR_BF16 = 1, SR_F16 = 2, SR_CLAMP = 3 };
__device__ __forceinline__ float score_round(float v, int mode) {
    if (mode == SR_BF16) return (float)(__bf16)v;
    if (mode == SR_F16) return (float)(_Float16)h2_clamp(v);
    if (mode == SR_CLAMP) return h2_clamp(v);
    return v;
}

// logit[row] = ln_f(x[row]) . wte[label of row]: one wavefront per scored row, the row and the label's embedding in
// registers (3 float4 per lane each at d = 768), LayerNorm as launch_layernorm computes it, the dot product in fp32 in a
// fixed order (a lane's float4s in index order, then the wavefront's tree).  NaN for a label outside [0, V).
__global__ __launch_bounds__(256) void label_logit_kernel(const float *__restrict__ x, const int *__restrict__ target,
                                                          const int *__restrict__ tok, const float *__restrict__ lnw,
                                                          const float *__restrict__ lnb, float eps,
                                                          const float *__restrict__ wte, float *__restrict__ logit, int R,
                                                          int d, int V, int mode) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= R) return;
    const float *xr = x + (size_t)row * d;
    const int nv = d >> 2;
    float4 v[SC_MAXV];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < SC_MAXV; ++i) {
        const int idx = lane + 64 * i;
        if (idx < nv) {
            v[i] = reinterpret_cast<const float4 *>(xr)[idx];
            s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
        } else {
            v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    const float mean = wave_sum(s) / (float)d;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < SC_MAXV; ++i) {
        const int idx = lane + 64 * i;
        if (idx < nv) {
            const float a = v[i].x - mean, bb = v[i].y - mean, c = v[i].z - mean, e = v[i].w - mean;
            q += (a * a + bb * bb) + (c * c + e * e);
        }
    }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)d + eps);
    const int label = tok[target[row]];
    const bool ok = label >= 0 && label < V;                     // (uniform over the wavefront)
    const float *wr = wte + (size_t)(ok ? label : 0) * d;
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < SC_MAXV; ++i) {
        const int idx = lane + 64 * i;
        if (idx < nv) {
            const float4 ww = reinterpret_cast<const float4 *>(lnw)[idx];
            const float4 bb = reinterpret_cast<const float4 *>(lnb)[idx];
            const float4 e = reinterpret_cast<const float4 *>(wr)[idx];
            const float ox = score_round((v[i].x - mean) * rstd * ww.x + bb.x, mode);
            const float oy = score_round((v[i].y - mean) * rstd * ww.y + bb.y, mode);
            const float oz = score_round((v[i].z - mean) * rstd * ww.z + bb.z, mode);
            const float ow = score_round((v[i].w - mean) * rstd * ww.w + bb.w, mode);
            acc += (ox * score_round(e.x, mode) + oy * score_round(e.y, mode)) +
                   (oz * score_round(e.z, mode) + ow * score_round(e.w, mode));
        }
    }
    acc = wave_sum(acc);
    if (lane == 0) logit[row] = ok ? acc : __builtin_nanf("");
}

// One wavefront per caption of the chunk: logp of its len positions (compact rows off .. off + len), scattered to
// [n, L]; sum and count over a lane's positions in order, then the wavefront's tree -- the same order whatever the chunk.
__global__ __launch_bounds__(256) void score_finish_kernel(const float *__restrict__ logit, const float *__restrict__ lse,
                                                           const int *__restrict__ topi, const int *__restrict__ tok,
                                                           const int *__restrict__ lens, const int *__restrict__ roff,
                                                           const int *__restrict__ bad, int base, int nc, int L, int V,
                                                           int ignore_id, float inv_temp, float *__restrict__ logp,
                                                           float *__restrict__ sum, int *__restrict__ count,
                                                           int *__restrict__ top1) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= nc) return;
    const int len = lens[r], off = roff[r] - base, from = bad[r];
    float s = 0.f, cnt = 0.f;
    for (int i = lane; i < len; i += WAVE) {
        const int label = tok[(size_t)r * L + i];
        float lp = 0.f;
        if (!(ignore_id != -1 && label == ignore_id)) {
            lp = (i >= from || label < 0 || label >= V) ? __builtin_nanf("") : logit[off + i] * inv_temp - lse[off + i];
            s += lp;
            cnt += 1.f;
        }
        logp[(size_t)r * L + i] = lp;
        if (top1) top1[(size_t)r * L + i] = topi[off + i];
    }
    s = wave_sum(s);
    cnt = wave_sum(cnt);                                         // (<= 1024: exact)
    if (lane == 0) {
        if (sum) sum[r] = s;
        if (count) count[r] = (int)cnt;
    }
}

struct ScoreChunk { int c0, nc, Lc, r0, R; };      // captions c0 .. c0 + nc, padded to Lc tokens; scored rows r0 .. r0 + R of the call

struct ScoreArgs {
    const float *prefix;
    const int *tokens;
    int n, P, L, ignore_id;
    float inv_temp;
    float *logp, *sum;
    int *count, *top1;
};

// `plan` (host; it must outlive the upload): [lens n | first scored row of each caption n | row of h (within its chunk) of
// every scored row | its index in [n, L]]
int score_run(capdec_ctx *c, const ScoreArgs &a, const std::vector<ScoreChunk> &chunks, const std::vector<int> &plan, int Rtot) {
    const Gpt2 &g = c->gpt;
    const int d = g.d, n = a.n, P = a.P, L = a.L;
    CAPDEC_HIP(hipMemsetAsync(a.logp, 0, (size_t)n * L * 4, c->stream));
    if (a.top1) CAPDEC_HIP(hipMemsetAsync(a.top1, 0, (size_t)n * L * 4, c->stream));
    CAPDEC_TRY(c->s_plan.ensure(plan.size() * 4));
    CAPDEC_HIP(hipMemcpyAsync(c->s_plan.p, plan.data(), plan.size() * 4, hipMemcpyHostToDevice, c->stream));
    const int *d_lens = c->s_plan.as<int>(), *d_roff = d_lens + n, *d_hrow = d_roff + n, *d_target = d_hrow + Rtot;
    int maxR = 1, maxnc = 1;
    for (const ScoreChunk &k : chunks) {
        maxR = std::max(maxR, k.R);
        maxnc = std::max(maxnc, k.nc);
    }
    CAPDEC_TRY(c->s_rows.ensure((size_t)maxR * d * 4));
    CAPDEC_TRY(c->s_logit.ensure((size_t)maxR * 4));
    CAPDEC_TRY(c->s_bad.ensure((size_t)maxnc * 4));
    const int mode = c->gemm_mode == GEMM_BF16 ? SR_BF16 : c->gemm_mode == GEMM_F16 ? SR_F16
                     : c->gemm_mode == GEMM_F16X2 ? SR_CLAMP : SR_NONE;
    for (const ScoreChunk &k : chunks) {
        const int S = P + k.Lc - 1, M = k.nc * S;
        const int *tok = a.tokens + (size_t)k.c0 * L;
        int *bad = c->s_bad.as<int>();
        CAPDEC_HIP(hipMemsetAsync(bad, 0x7f, (size_t)k.nc * 4, c->stream));      // (0x7f7f7f7f: past every position)
        if (k.R > 0) {
            CAPDEC_CHECK((size_t)M * (d / 4) < (size_t)INT_MAX, "score: CAPDEC_SCORE_ROWS too large");
            KvCache kv;
            CAPDEC_TRY(ensure_kv(c, kv, k.nc, S));
            kv.fixed_variant = c->batch_invariant;
            CAPDEC_TRY(ensure_body_ws(c, M, d));
            {
                ProfScope ps(c, F_EMBED);
                const int tot = M * (d / 4);
                hipLaunchKernelGGL(score_embed_kernel, dim3((tot + 255) / 256), dim3(256), 0, c->stream,
                                   a.prefix + (size_t)k.c0 * P * d, tok, d_lens + k.c0, g.wte, g.wpe, c->h.as<float>(), bad, k.nc,
                                   P, S, L, g.vocab, d / 4);
                CAPDEC_HIP(hipGetLastError());
            }
            StepShape sp{};
            sp.prefill = true;
            sp.ncap = k.nc;
            sp.P = S;
            sp.beam = 1;
            CAPDEC_TRY(gpt2_body(c, sp, kv));
            float *rows = c->s_rows.as<float>();
            { ProfScope ps(c, F_EMBED); CAPDEC_TRY(launch_gather_rows(c->stream, c->h.as<float>(), d_hrow + k.r0, rows, k.R, d)); }
            CAPDEC_TRY(lm_head_select(c, rows, d, k.R, 1, a.inv_temp));
            ProfScope ps(c, F_SELECT);
            hipLaunchKernelGGL(label_logit_kernel, dim3((k.R + 3) / 4), dim3(256), 0, c->stream, rows, d_target + k.r0, a.tokens,
                               g.lnfw, g.lnfb, g.eps, g.wte, c->s_logit.as<float>(), k.R, d, g.vocab, mode);
            CAPDEC_HIP(hipGetLastError());
        }
        ProfScope ps(c, F_SELECT);
        hipLaunchKernelGGL(score_finish_kernel, dim3((k.nc + 3) / 4), dim3(256), 0, c->stream, c->s_logit.as<float>(),
                           c->lse.as<float>(), c->topi.as<int>(), tok, d_lens + k.c0, d_roff + k.c0, bad, k.r0, k.nc, L, g.vocab,
                           a.ignore_id, a.inv_temp, a.logp + (size_t)k.c0 * L, a.sum ? a.sum + k.c0 : nullptr,
                           a.count ? a.count + k.c0 : nullptr, a.top1 ? a.top1 + (size_t)k.c0 * L : nullptr);
        CAPDEC_HIP(hipGetLastError());
    }
    return 0;
}

}  // namespace

}  // namespace capdec

using namespace capdec;

extern "C" int capdec_score(capdec_ctx *c, const float *prefix, const int32_t *tokens, const int32_t *h_lens, int n, int P,
                            int L, int ignore_id, float temperature, float *logp, float *sum, int32_t *count, int32_t *top1) {
    CAPDEC_CHECK(c && c->gpt.loaded, "score: GPT-2 weights not loaded");
    CAPDEC_CHECK(n == 0 || (prefix && tokens && logp), "score: null argument");
    CAPDEC_CHECK(n >= 0 && P >= 1 && L >= 1, "score: bad sizes");
    CAPDEC_CHECK(P + L - 1 <= c->gpt.n_pos, "score: prefix + caption length exceeds n_positions");
    CAPDEC_CHECK(P + L - 1 <= 1024, "score: context > 1024 not supported");
    CAPDEC_CHECK(c->gpt.d / c->gpt.n_head == 64, "score: head_dim must be 64");
    CAPDEC_CHECK(c->gpt.d % 4 == 0 && c->gpt.d <= 256 * SC_MAXV, "score: unsupported width");
    CAPDEC_CHECK(temperature == temperature, "score: temperature is NaN");
    CAPDEC_HIP(hipSetDevice(c->device));
    c->stat_score_chunks = 0;
    if (n == 0) return 0;
    int maxlen = 1;
    long long total = 0;
    for (int r = 0; r < n; ++r) {
        const int len = h_lens ? h_lens[r] : L;
        CAPDEC_CHECK(len >= 0 && len <= L, "score: a caption length outside 0..L");
        maxlen = std::max(maxlen, len);
        total += len;
    }
    CAPDEC_CHECK((long long)n * L < INT_MAX / 4, "score: too many tokens for one call");
    const int Rtot = (int)total;
    // ---- the plan: chunks of whole captions in input order.  Batch-invariant mode pads every chunk to the call's longest
    // caption: the prefill attention picks its kernel by the sequence length, which must then not depend on the chunking.
    std::vector<ScoreChunk> chunks;
    std::vector<int> plan((size_t)2 * n + 2 * (size_t)Rtot);
    int *p_lens = plan.data(), *p_roff = p_lens + n, *p_hrow = p_roff + n, *p_target = p_hrow + Rtot;
    const long long cap = std::max(1, c->tune.score_rows);
    ScoreChunk cur{0, 0, c->batch_invariant ? maxlen : 1, 0, 0};
    int row = 0;
    for (int r = 0; r < n; ++r) {
        const int len = h_lens ? h_lens[r] : L;
        const int Lc = std::max(cur.Lc, len);
        if (cur.nc > 0 && (long long)(cur.nc + 1) * (P + Lc - 1) > cap) {
            chunks.push_back(cur);
            cur = ScoreChunk{r, 0, c->batch_invariant ? maxlen : 1, row, 0};
        }
        cur.Lc = std::max(cur.Lc, len);
        cur.nc += 1;
        cur.R += len;
        p_lens[r] = len;
        p_roff[r] = row;
        row += len;
    }
    chunks.push_back(cur);
    for (const ScoreChunk &k : chunks) {
        const int S = P + k.Lc - 1;
        for (int r = k.c0; r < k.c0 + k.nc; ++r)
            for (int i = 0; i < p_lens[r]; ++i) {
                p_hrow[p_roff[r] + i] = (r - k.c0) * S + P - 1 + i;
                p_target[p_roff[r] + i] = r * L + i;
            }
    }
    c->stat_score_chunks = (int)chunks.size();
    const ScoreArgs a{prefix, tokens, n, P, L, ignore_id, 1.0f / (temperature > 0.f ? temperature : 1.0f), logp, sum, count, top1};
    const int rc = score_run(c, a, chunks, plan, Rtot);
    // (the plan is uploaded from this call's own memory: nothing may still be reading it when the call returns)
    if (hipStreamSynchronize(c->stream) != hipSuccess && rc == 0) {
        set_error("score: hipStreamSynchronize failed");
        return 1;
    }
    return rc;
}
