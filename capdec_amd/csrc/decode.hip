// The KV-cached batched decode: the pre-LN block stack (GPT-2, and the CLIP towers that run on the same stack), the fused
// lm_head + candidate selection, the one step loop of every decode (decode_steps: alive-count polls on decode_sched.h's
// schedule, finished-caption compaction, the statistics) and the greedy / beam / sampling drivers on it -- host-side
// orchestration only: every operation is a launcher of common.h enqueued on the context's stream.  (The mapping networks:
// mapper.hip.)  A call's constants travel in one DecodeCall.  A driver is the prefill, the body of a step handed to
// decode_steps, and the finalisation; the guided decode (guided.hip) and the contrastive search (contrastive.hip) are two
// more such drivers and start their calls with the same decode_call_checks / decode_call_begin / chunk_call.  Here every
// step, the prefill's included, ends in select_and_advance, which picks the lm_head route (lm_head_select: fused, logits
// never in HBM; lm_head_rows: materialised, for the logits processors, the sampling decode and the guided decode) and then
// advances the greedy or the beam state (decode_advance).
#include "context.h"
#include "decode_sched.h"

namespace capdec {

int ensure_body_ws(capdec_ctx *c, int M, int d) {
    CAPDEC_TRY(c->h.ensure((size_t)M * d * 4));
    CAPDEC_TRY(c->x.ensure((size_t)M * d * 4));
    CAPDEC_TRY(c->qkv.ensure((size_t)M * 3 * d * 4));
    CAPDEC_TRY(c->att.ensure((size_t)M * d * 4));
    CAPDEC_TRY(c->ff.ensure((size_t)M * 4 * d * 4));
    return 0;
}

// h [M, d] (in c->h) -> h after all blocks (final LN NOT applied).  The same pre-LN block serves
// GPT-2 (gelu_new, causal, KV cache kept for the decode steps) and the CLIP towers (QuickGELU, attention straight from
// the qkv activations, nothing cached; the vision tower is not causal).
int stack_body(capdec_ctx *c, const StackCfg &g, const StepShape &s, const KvCache &kv) {
    const int d = g.d, M = s.prefill ? s.ncap * s.P : s.rows;
    float *h = c->h.as<float>(), *x = c->x.as<float>(), *qkv = c->qkv.as<float>(), *att = c->att.as<float>(),
          *ff = c->ff.as<float>();
    // packed chain (bf16x3 mode): LN1 -> [packed] -> qkv GEMM -> attention -> [packed] -> c_proj (+h) -> LN2 ->
    // [packed] -> fc GEMM + act -> [packed] -> mlp c_proj (+h): every GEMM operand moves by LDS-DMA, and the
    // attention / MLP intermediates never exist in fp32 in HBM.
    const bool chain = use_packed_a(c, d) && c->pack_chain;
    const bool kv_direct = c->tune.kv_direct;
    void *apk = nullptr, *fpk = nullptr;
    if (chain) {
        CAPDEC_TRY(c->apk.ensure(x3_packed_bytes_host(M, d)));
        CAPDEC_TRY(c->fpk.ensure(x3_packed_bytes_host(M, 4 * d)));
        apk = c->apk.p;
        fpk = c->fpk.p;
    }
    int ln1_ready = 0;      // xpk already holds this layer's LN1(h): fused into the previous layer's mlp c_proj reduce
    for (int l = 0; l < g.n_layer; ++l) {
        const Gpt2Layer &w = (*g.layers)[l];
        const int kl = g.keep_kv ? l : 0;
        // decode steps in the default mode: K / V of the new token go from the qkv GEMM's epilogue straight into the cache
        // (QkvScatter) when that GEMM runs unsplit -- the attention then reads them like any other position
        QkvScatter sc;
            // (the scatter epilogue is float4-only: a host whose c_attn bias is not 16-byte aligned keeps the other path)
        // (round 5: also in bf16 mode -- the one-plane qkv GEMM rounds K / V to bf16 as it writes them into the bf16 cache)
        const bool mode_ok = (c->gemm_mode == GEMM_F16X2 && !kv.bf16) || (c->gemm_mode == GEMM_BF16 && kv.bf16);
        const bool scatter = kv_direct && !s.prefill && g.keep_kv && mode_ok && use_packed_a(c, d) && w.bqkv &&
                             (((uintptr_t)w.bqkv | (uintptr_t)qkv) & 15) == 0 &&
                             d % GEMM_BN == 0 && (s.beam == 1 || s.beam == 5) &&
                             (c->batch_invariant || plan_splitk_128(M, 3 * d, d, c->tune) == 1);
        if (scatter) {
            sc.kc = reinterpret_cast<float *>(kv.bf16 ? (void *)kv.kp<__bf16>(kl) : (void *)kv.kp<float>(kl));
            sc.vc = reinterpret_cast<float *>(kv.bf16 ? (void *)kv.vp<__bf16>(kl) : (void *)kv.vp<float>(kl));
            sc.cmap = s.cmap;
            sc.beam = s.beam; sc.heads = kv.heads; sc.ctx = kv.ctx; sc.pos = s.L - 1; sc.d = d;
            sc.bf16 = kv.bf16;
        }
        if (use_packed_a(c, d)) {
            CAPDEC_TRY(ln_gemm_packed(c, h, d, w.ln1w, w.ln1b, g.eps, w.wqkv, qkv, 3 * d, M, 3 * d, d, w.bqkv, CAPDEC_ACT_NONE,
                                      nullptr, ln1_ready != 0, scatter ? &sc : nullptr));
            ln1_ready = 0;
        } else {
            { ProfScope ps(c, F_LN); CAPDEC_TRY(launch_layernorm(c->stream, h, d, w.ln1w, w.ln1b, g.eps, x, d, M, d)); }
            CAPDEC_TRY(gemm(c, x, d, w.wqkv, d, qkv, 3 * d, M, 3 * d, d, w.bqkv, CAPDEC_ACT_NONE));
        }
        if (s.prefill) {
            ProfScope ps(c, F_ATTN_PRE);
            if (g.keep_kv)      // the towers never decode: only GPT-2 needs its prefix K/V in the cache
                CAPDEC_TRY(launch_kv_scatter_prefill(c->stream, qkv, kv, kl, s.ncap, s.P, s.beam));
            CAPDEC_TRY(launch_attn_prefill(c->stream, qkv, kv, kl, s.ncap, s.P, s.beam, att, g.causal, apk, pack_fmt(c)));
        } else {
            ProfScope ps(c, F_ATTN_DEC);
            CAPDEC_TRY(launch_attn_decode(c->stream, qkv, kv, kl, s.rows, s.beam, s.L, s.anc, s.anc_stride, att, apk, s.cmap, pack_fmt(c),
                                          scatter));
        }
        int ln2_ready = 0;
        if (chain) {
            const NextLn n2{w.ln2w, w.ln2b, g.eps, &ln2_ready};
            CAPDEC_TRY(gemm_packed(c, apk, w.wproj, h, d, M, d, d, w.bproj, CAPDEC_ACT_NONE, h, d, nullptr, &n2));
        } else {
            CAPDEC_TRY(gemm(c, att, d, w.wproj, d, h, d, M, d, d, w.bproj, CAPDEC_ACT_NONE, h, d));
        }
        if (chain) {
            CAPDEC_TRY(ln_gemm_packed(c, h, d, w.ln2w, w.ln2b, g.eps, w.wfc, ff, 4 * d, M, 4 * d, d, w.bfc, g.act, fpk,
                                      ln2_ready != 0));
            // the LayerNorm after mlp c_proj is the NEXT layer's ln_1 (the final ln_f runs on its own: it may see strided rows)
            const bool has_next = l + 1 < g.n_layer;
            const NextLn n1{has_next ? (*g.layers)[l + 1].ln1w : nullptr, has_next ? (*g.layers)[l + 1].ln1b : nullptr, g.eps,
                            &ln1_ready};
            CAPDEC_TRY(gemm_packed(c, fpk, w.wproj2, h, d, M, d, 4 * d, w.bproj2, CAPDEC_ACT_NONE, h, d, nullptr,
                                   has_next ? &n1 : nullptr));
            continue;
        }
        if (use_packed_a(c, d)) {
            CAPDEC_TRY(ln_gemm_packed(c, h, d, w.ln2w, w.ln2b, g.eps, w.wfc, ff, 4 * d, M, 4 * d, d, w.bfc, g.act));
        } else {
            { ProfScope ps(c, F_LN); CAPDEC_TRY(launch_layernorm(c->stream, h, d, w.ln2w, w.ln2b, g.eps, x, d, M, d)); }
            CAPDEC_TRY(gemm(c, x, d, w.wfc, d, ff, 4 * d, M, 4 * d, d, w.bfc, g.act));
        }
        CAPDEC_TRY(gemm(c, ff, 4 * d, w.wproj2, 4 * d, h, d, M, d, 4 * d, w.bproj2, CAPDEC_ACT_NONE, h, d));
    }
    return 0;
}

int gpt2_body(capdec_ctx *c, const StepShape &s, const KvCache &kv) {
    const Gpt2 &g = c->gpt;
    StackCfg cfg{&g.layers, g.n_layer, g.d, g.eps, CAPDEC_ACT_GELU_NEW, true, true};
    return stack_body(c, cfg, s, kv);
}

// The sparse route of lm_head_select (k = 5, the wide two-plane kernel, >= LM_SPARSE_MIN_TILES column tiles): the first pass
// keeps NO candidates, only max and sum exp per (row, tile), which the logsumexp needs anyway.  A row's top 5 lie in the tiles
// whose maximum reaches the row's fifth largest tile maximum -- five tiles of 393 unless maxima tie exactly -- so those
// (row, tile) pairs alone are computed again with the k = 5 epilogue: bucketed by tile, one grouped launch that reads the
// pairs' packed rows where the LayerNorm left them, one merge per row.  A recomputed logit has the bits of the first pass (same kernel geometry and order), so
// the result is the k = 5 result.  Rows with more than LM_SPARSE_CAP pairs or a tile maximum that is not finite take the
// full second pass of the three-candidate route instead, through the same flag list and counters; it runs in
// LM_HARD_SLICES slices so that its partial lists need room for a fraction of the rows only.
static int lm_head_sparse(capdec_ctx *c, const float *h0, int ldh, int R, float inv_temp) {
    const Gpt2 &g = c->gpt;
    const int d = g.d, nt = gemm_tiles_n(g.vocab), k = 5;
    const int slice = (R + LM_HARD_SLICES - 1) / LM_HARD_SLICES;
    const int bcap = SparseLm::blocks_cap(R, nt);
    CAPDEC_TRY(c->tmax.ensure((size_t)R * nt * 4));
    CAPDEC_TRY(c->tsum.ensure((size_t)R * nt * 4));
    CAPDEC_TRY(c->lse.ensure((size_t)R * 4));
    CAPDEC_TRY(c->topv.ensure((size_t)R * k * 4));
    CAPDEC_TRY(c->topi.ensure((size_t)R * k * 4));
    // candidate lists: one per pair, then (the pairs' merge has run) one per (row of a slice, tile)
    const size_t lists = std::max((size_t)R * LM_SPARSE_CAP, (size_t)slice * nt);
    CAPDEC_TRY(c->cval.ensure(lists * k * 4));
    CAPDEC_TRY(c->cidx.ensure(lists * k * 4));
    CAPDEC_TRY(c->lmflag.ensure(((size_t)R + 2) * 4));
    CAPDEC_TRY(c->xpk2.ensure(x3_packed_bytes_host(slice, d)));
    CAPDEC_TRY(c->lmsp.ensure(((size_t)3 * nt + 1 + LM_HARD_SLICES + 3 * (size_t)bcap + R + 2 * (size_t)R * LM_SPARSE_CAP) * 4));
    SparseLm s;
    s.tile_cnt = c->lmsp.as<int>();
    s.tile_cur = s.tile_cnt + nt;
    s.tile_off = s.tile_cur + nt;
    s.nblk = s.tile_off + nt;
    s.slice_cnt = s.nblk + 1;
    s.blk_tab = s.slice_cnt + LM_HARD_SLICES;
    s.row_cnt = s.blk_tab + 3 * (size_t)bcap;
    s.row_tiles = s.row_cnt + R;
    s.slot_of = s.row_tiles + (size_t)R * LM_SPARSE_CAP;
    s.slice_rows = slice;
    const TopkOut o{c->tmax.as<float>(), c->tsum.as<float>(), c->cval.as<float>(), c->cidx.as<int>()};
    float *topv = c->topv.as<float>();
    int *topi = c->topi.as<int>();
    int *cnt = c->lmflag.as<int>(), *total = cnt + 1, *rows = cnt + 2;
    bool k3 = false;
    CAPDEC_TRY(ln_gemm_topk(c, h0, ldh, g.lnfw, g.lnfb, g.eps, g.wte, R, g.vocab, d, k, inv_temp, o, false, &k3, /*no_cand=*/true));
    {
        ProfScope ps(c, F_SELECT);
        CAPDEC_HIP(hipMemsetAsync(cnt, 0, sizeof(int), c->stream));
        CAPDEC_HIP(hipMemsetAsync(s.tile_cnt, 0, (size_t)nt * sizeof(int), c->stream));
        CAPDEC_TRY(launch_lm_tile_select(c->stream, o.tile_max, o.tile_sum, R, nt, c->lse.as<float>(), s, rows, cnt, total));
    }
    {
        ProfScope ps(c, F_LMHEAD_2ND);
        CAPDEC_TRY(gemm_topk_grouped(c, c->xpk.p, g.wte, s, bcap, g.vocab, d, inv_temp, o.cand_val, o.cand_idx));
    }
    {
        ProfScope ps(c, F_SELECT);
        CAPDEC_TRY(launch_lm_sparse_merge(c->stream, o.cand_val, o.cand_idx, s.row_cnt, R, topv, topi));
    }
    // the flagged rows: gather, k = 5 kernel over every tile, merge -- per slice (tile_max / tile_sum and the pairs' lists are
    // dead by now: their buffers take the slices' partial lists)
    ProfScope ps(c, F_LMHEAD_2ND);
    for (int sl = 0; sl < LM_HARD_SLICES && sl * slice < R; ++sl) {
        const int cap = std::min(slice, R - sl * slice);
        const int *n_dev = s.slice_cnt + sl, *src = rows + (size_t)sl * slice;
        CAPDEC_TRY(launch_gather_packed_rows(c->stream, c->xpk.p, d, src, n_dev, cap, c->xpk2.p, pack_fmt(c)));
        CAPDEC_TRY(gemm_topk_dev(c, c->xpk2.p, g.wte, n_dev, g.vocab, d, inv_temp, o));
        CAPDEC_TRY(launch_topk_merge_rows(c->stream, o.cand_val, o.cand_idx, n_dev, src, cap, nt, topv, topi));
    }
    c->lmflag_live = true;
    c->k3_rows += R;
    return 0;
}

// ln_f over `R` rows of h (row stride ldh floats, starting at h0) then the fused lm_head:
// -> lse [R], topv/topi [R, k]
int lm_head_select(capdec_ctx *c, const float *h0, int ldh, int R, int k, float inv_temp) {
    const Gpt2 &g = c->gpt;
    const int d = g.d, nt = gemm_tiles_n(g.vocab);
    const bool k3_ok = c->tune.lmhead_k3 && k == 5 && !c->k3_off;
    const int sparse = c->tune.lmhead_sparse;       // (2: from the wide tile's first row, tests)
    if (k3_ok && sparse && (sparse >= 2 || R >= LM_SPARSE_MIN_ROWS) && nt >= LM_SPARSE_MIN_TILES && nt <= 1024) {
        bool wide = false;
        CAPDEC_TRY(lm_head_wide_tile(c, g.wte, R, g.vocab, d, &wide));
        if (wide) return lm_head_sparse(c, h0, ldh, R, inv_temp);
    }
    TopkOut o;
    CAPDEC_TRY(topk_workspace(c, R, nt, k, &o));
    CAPDEC_TRY(c->topv.ensure((size_t)R * k * 4));
    CAPDEC_TRY(c->topi.ensure((size_t)R * k * 4));
    // Beam search (k = 5) may keep THREE candidates per (row, 128-column tile) -- two selection rounds fewer in every tile's
    // epilogue.  The merge then knows exactly which rows that can have been too few for (some tile's third candidate is
    // still strictly better than the row's fifth: with 393 tiles a rare event) and those rows alone go through the k = 5
    // kernel again, compacted; the result is the k = 5 result.
    bool k3 = false;
    CAPDEC_TRY(ln_gemm_topk(c, h0, ldh, g.lnfw, g.lnfb, g.eps, g.wte, R, g.vocab, d, k, inv_temp, o, k3_ok, &k3));
    if (k3) {
        CAPDEC_TRY(c->lmflag.ensure(((size_t)R + 2) * 4));
        CAPDEC_TRY(c->xpk2.ensure(x3_packed_bytes_host(R, d)));
        int *cnt = c->lmflag.as<int>(), *total = cnt + 1, *rows = cnt + 2;
        {
            ProfScope ps(c, F_SELECT);
            CAPDEC_HIP(hipMemsetAsync(cnt, 0, sizeof(int), c->stream));
            CAPDEC_TRY(launch_topk_merge_k3(c->stream, o.tile_max, o.tile_sum, o.cand_val, o.cand_idx, R, nt,
                                            c->lse.as<float>(), c->topv.as<float>(), c->topi.as<int>(), rows, cnt, total));
        }
        // the second pass: gather (the packed LayerNorm output sits in c->xpk), k = 5 kernel over the device-side row count,
        // merge (the partial lists of the first pass are dead once its merge has run: their buffers are reused)
        ProfScope ps(c, F_LMHEAD_2ND);
        CAPDEC_TRY(launch_gather_packed_rows(c->stream, c->xpk.p, d, rows, cnt, R, c->xpk2.p, pack_fmt(c)));
        CAPDEC_TRY(gemm_topk_dev(c, c->xpk2.p, g.wte, cnt, g.vocab, d, inv_temp, o));
        CAPDEC_TRY(launch_topk_merge_rows(c->stream, o.cand_val, o.cand_idx, cnt, rows, R, nt, c->topv.as<float>(),
                                          c->topi.as<int>()));
        c->lmflag_live = true;
        c->k3_rows += R;
        return 0;
    }
    ProfScope ps(c, F_SELECT);
    return launch_topk_merge(c->stream, o.tile_max, o.tile_sum, o.cand_val, o.cand_idx, R, nt, k, c->lse.as<float>(),
                             c->topv.as<float>(), c->topi.as<int>());
}

// ln_f over `R` rows of h (row stride ldh floats, starting at h0) then the plain lm_head GEMM over wte:
// -> logits fp32 [R, ld]  (the full rows: capdec_gpt2_logits and the sampling decode; greedy / beam never materialise them)
int lm_head_logits(capdec_ctx *c, const float *h0, int ldh, int R, float *logits, int ld) {
    const Gpt2 &g = c->gpt;
    const int d = g.d;
    if (use_packed_a(c, d))   // same operand path as the decode loop's fused lm_head (bf16 mode: bf16 operands)
        return ln_gemm_packed(c, h0, ldh, g.lnfw, g.lnfb, g.eps, g.wte, logits, ld, R, g.vocab, d, nullptr, CAPDEC_ACT_NONE);
    CAPDEC_TRY(c->xl.ensure((size_t)R * d * 4));
    { ProfScope ps(c, F_LN); CAPDEC_TRY(launch_layernorm(c->stream, h0, ldh, g.lnfw, g.lnfb, g.eps, c->xl.as<float>(), d, R, d)); }
    return gemm(c, c->xl.as<float>(), d, g.wte, d, logits, ld, R, g.vocab, d, nullptr, CAPDEC_ACT_NONE);
}

// Does this call run the logits processors (capdec_set_logits_processors / capdec_set_logit_bias)?  top_k counts in the
// sampling decode only.
bool processors_on(const capdec_ctx *c, bool sampling) {
    const LogitsProc &p = c->proc;
    return p.theta != 1.0f || p.ngram > 0 || p.min_len > 0 || c->proc_bias_n > 0 || (sampling && p.top_k > 0);
}

// One step over `R` activation rows through materialised logits, tune.sample_rows rows at a time (the fp32 logits of 5000
// rows of GPT-2's vocabulary are 1 GB): lm_head_logits, with `proc` the processors in place (process.hip), then
//   greedy, beam  the one-pass selection at the block's offset into c->lse / c->topv / c->topi: what lm_head_select
//                 leaves, the step kernels follow unchanged
//   sampling      top_k where it removes something, the nucleus-sampling kernel (it writes what launch_greedy_step
//                 writes, into gs), the logp shift under top_k.
// hn (the guided decode): the rows' partners, same stride -- a block's partner logits go behind the block's own in the
// scratch, and the combine (guided.hip) writes gamma * log_softmax(own) + (1 - gamma) * log_softmax(partner) over the own
// rows in front of the processors.
// hist: the rows' histories [captions, beam, T] -- `ids` or BeamState::tokens; `step` entries of each are read.
int lm_head_rows(capdec_ctx *c, const float *h0, int ldh, int R, int k, float inv_temp, const DecodeCall &a,
                 const GreedyState &gs, bool proc, int step, int beam, const int *hist, const float *hn, float gamma) {
    const int V = c->gpt.vocab, ld = pad64(V), blk = std::min(R, std::max(1, c->tune.sample_rows));
    const LogitsProc &p = c->proc;
    const float *bias = c->proc_bias_n > 0 ? c->pbias.as<float>() : nullptr;
    const bool cut = proc && a.sample && p.top_k > 0 && p.top_k < V;
    CAPDEC_TRY(c->slogits.ensure((size_t)(hn ? 2 : 1) * blk * ld * 4));
    if (!a.sample) {
        CAPDEC_TRY(c->lse.ensure((size_t)R * 4));
        CAPDEC_TRY(c->topv.ensure((size_t)R * k * 4));
        CAPDEC_TRY(c->topi.ensure((size_t)R * k * 4));
    } else if (cut && a.logp) {
        CAPDEC_TRY(c->pcorr.ensure((size_t)blk * 4));
    }
    float *lg = c->slogits.as<float>(), *lgn = lg + (size_t)blk * ld;
    float *corr = cut && a.logp ? c->pcorr.as<float>() : nullptr;
    for (int r0 = 0; r0 < R; r0 += blk) {
        const int nr = std::min(blk, R - r0);
        CAPDEC_TRY(lm_head_logits(c, h0 + (size_t)r0 * ldh, ldh, nr, lg, ld));
        if (hn) {
            CAPDEC_TRY(lm_head_logits(c, hn + (size_t)r0 * ldh, ldh, nr, lgn, ld));
            ProfScope ps(c, F_GUIDED);
            CAPDEC_TRY(launch_guided_combine(c->stream, lg, lgn, ld, nr, V, gamma));
        }
        ProfScope ps(c, F_SELECT);
        if (proc)
            CAPDEC_TRY(launch_logits_process(c->stream, lg, ld, nr, r0, V, gs.cmap, beam, hist, a.T, step, p, bias, a.stop_id,
                                             a.alt_stop_id));
        if (!a.sample) {
            CAPDEC_TRY(launch_logits_select(c->stream, lg, ld, nr, V, k, inv_temp, c->lse.as<float>() + r0,
                                            c->topv.as<float>() + (size_t)r0 * k, c->topi.as<int>() + (size_t)r0 * k));
            continue;
        }
        if (cut) CAPDEC_TRY(launch_logits_topk(c->stream, lg, ld, nr, V, p.top_k, inv_temp, corr));
        CAPDEC_TRY(launch_sample_top_p(c->stream, gs, lg, ld, nr, r0, V, inv_temp, a.top_p, a.seed, a.u, a.cap_off, step));
        if (corr) CAPDEC_TRY(launch_logp_shift(c->stream, corr, nr, r0, gs.cmap, gs.lens, step, a.T, a.logp));
    }
    return 0;
}

// lm_head_rows for the constrained beam search (constrained.hip), which always takes this route: per block of rows the
// logits, with `proc` the processors in place, then the one-pass selection that bans the stop token while the row's phrases
// are unmet and leaves the row's list -- its special tokens' places, then its best `beam` others -- CON_LIST entries per row
// at the block's offset into c->lse / c->topv / c->topi.
static int lm_head_rows_forced(capdec_ctx *c, const float *h0, int ldh, int R, float inv_temp, const DecodeCall &a,
                               const DecodeState &s, bool proc, int step, const int *cmap) {
    const int V = c->gpt.vocab, ld = pad64(V), blk = std::min(R, std::max(1, c->tune.sample_rows));
    const float *bias = c->proc_bias_n > 0 ? c->pbias.as<float>() : nullptr;
    CAPDEC_TRY(c->slogits.ensure((size_t)blk * ld * 4));
    CAPDEC_TRY(c->lse.ensure((size_t)R * 4));
    CAPDEC_TRY(c->topv.ensure((size_t)R * CON_LIST * 4));
    CAPDEC_TRY(c->topi.ensure((size_t)R * CON_LIST * 4));
    float *lg = c->slogits.as<float>();
    for (int r0 = 0; r0 < R; r0 += blk) {
        const int nr = std::min(blk, R - r0);
        CAPDEC_TRY(lm_head_logits(c, h0 + (size_t)r0 * ldh, ldh, nr, lg, ld));
        ProfScope ps(c, F_SELECT);
        if (proc)
            CAPDEC_TRY(launch_logits_process(c->stream, lg, ld, nr, r0, V, cmap, step == 0 ? 1 : a.beam, s.hist, a.T, step,
                                             c->proc, bias, a.stop_id, a.alt_stop_id));
        CAPDEC_TRY(launch_logits_select_forced(c->stream, lg, ld, nr, r0, V, a.beam, inv_temp, s.cs, cmap, step, a.stop_id,
                                               c->lse.as<float>() + r0, c->topv.as<float>() + (size_t)r0 * CON_LIST,
                                               c->topi.as<int>() + (size_t)r0 * CON_LIST));
    }
    return 0;
}

// geometry only (the CLIP towers attend straight from the qkv activations and never touch a cache)
void kv_geometry(KvCache &kv, int rows, int ctx, int heads, int hd) {
    kv.rows = rows;
    kv.heads = heads;
    kv.ctx = ctx;
    kv.hd = hd;
    kv.k = kv.v = nullptr;
}
int ensure_kv(capdec_ctx *c, KvCache &kv, int rows, int ctx, int heads, int hd, int layers) {
    const Gpt2 &g = c->gpt;
    kv.rows = rows;
    kv.heads = heads ? heads : g.n_head;
    kv.ctx = ctx;
    kv.hd = hd ? hd : g.d / g.n_head;
    kv.bf16 = c->gemm_mode == GEMM_BF16;      // BASELINE configs[1]: bf16 weights / GEMM operands / KV cache
    const size_t bytes = kv.layer_stride() * (layers ? layers : g.n_layer) * kv.elem_bytes();
    CAPDEC_TRY(c->kc.ensure(bytes));
    CAPDEC_TRY(c->vc.ensure(bytes));
    kv.k = c->kc.p;
    kv.v = c->vc.p;
    return 0;
}

int poll_alive(capdec_ctx *c, int *alive) {
    CAPDEC_HIP(hipMemcpyAsync(c->alive_host, c->alive.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    const bool watch = c->lmflag_live && !c->k3_off;
    if (watch) CAPDEC_HIP(hipMemcpyAsync(c->alive_host + 1, c->lmflag.as<int>() + 1, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    CAPDEC_HIP(hipStreamSynchronize(c->stream));
    *alive = *c->alive_host;
    // a vocabulary that clusters a row's best candidates inside one 128-column tile sends many rows through the lm_head's
    // second pass: past the break-even the rest of the call keeps k candidates per tile (same results either way)
    if (watch && c->k3_rows > 0 && (double)c->alive_host[1] * 1000.0 > (double)c->tune.lmhead_k3_max * (double)c->k3_rows) c->k3_off = true;
    return 0;
}

// captions per chunk so that the fp32 KV cache fits the budget: the configured budget (capdec_set_kv_budget, default
// 192 GiB), clamped to 85 % of what the device can still give (free memory + what the KV buffers already hold), so
// a GPU that is partly occupied -- torch's caching allocator, the CLIP towers, a smaller part -- gets smaller chunks
// instead of a failed hipMalloc.  extra_per_cap: bytes a caption keeps next to its K/V (the contrastive search's history)
int chunk_captions(capdec_ctx *c, int n, int beam, int ctx, size_t extra_per_cap) {
    const Gpt2 &g = c->gpt;
    const size_t per_cap = (size_t)beam * ctx * g.d * 2 * (c->gemm_mode == GEMM_BF16 ? 2 : 4) * g.n_layer + extra_per_cap;
    size_t budget = c->kv_budget, free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
        const size_t avail = (size_t)((double)(free_b + c->kc.cap + c->vc.cap) * 0.85);
        budget = std::min(budget, avail);
    }
    size_t m = budget / std::max<size_t>(per_cap, 1);
    m = std::max<size_t>(m, 1);
    return (int)std::min<size_t>(m, (size_t)n);
}

// ---------------------------------------------------------------------------- what every decode entry point shares
// The checks common to the entry points, `who` in front of every message.  An entry point asks for them in the groups its own
// checks sit between (`which`: CK_*); ctx: the last position the call reaches + 1.
int decode_call_checks(capdec_ctx *c, const char *who, int which, int n, int P, int T, long long ctx) {
    const std::string w = std::string(who) + ": ";
    if (which & CK_LOADED) CAPDEC_CHECK(c && c->gpt.loaded, w + "GPT-2 weights not loaded");
    if (which & CK_SIZES) CAPDEC_CHECK(n >= 0 && P >= 1 && T >= 1, w + "bad sizes");
    if (which & CK_CONTEXT) {
        CAPDEC_CHECK(ctx <= c->gpt.n_pos, w + "prefix + entry_length exceeds n_positions");
        // (a context that counts the last token too -- contrastive search -- bounds entry_length with it)
        CAPDEC_CHECK(ctx <= 1024 && T <= 1024,
                     w + (ctx == (long long)P + T ? "context > 1024 not supported" : "context or entry_length > 1024 not supported"));
    }
    if (which & CK_HEAD_DIM) CAPDEC_CHECK(c->gpt.d / c->gpt.n_head == 64, w + "head_dim must be 64");
    if (which & CK_BIAS)
        CAPDEC_CHECK(c->proc_bias_n == 0 || c->proc_bias_n == c->gpt.vocab, w + "the logit bias was set for another vocabulary");
    return 0;
}

// The per-call reset and plan: the statistics (steps0: what the prefill's selection counts as -- 1, or 0 where step 0 is a
// loop step), the K/V-slot counters of kvstat_caps captions (0: greedy), the captions per chunk under the KV budget
// (chunk_captions) -> *chunk, the lm_head's second-pass bookkeeping ([count, total, rows...], lm_head_select) sized once for
// the largest step of lm_rows_per_cap rows per caption, total zeroed (0: the fused lm_head never runs, poll_alive has
// nothing to watch).  n == 0: the reset alone, *chunk = 0.
int decode_call_begin(capdec_ctx *c, int n, int steps0, int kvstat_caps, int rows_per_caption, int ctx, size_t extra_per_cap,
                      int lm_rows_per_cap, int *chunk) {
    CAPDEC_HIP(hipSetDevice(c->device));
    c->stat_steps = n > 0 ? steps0 : 0;
    c->stat_compactions = 0;
    c->stat_chunks = 0;
    c->stat_row_steps = 0;
    c->stat_step_rows.clear();
    c->stat_kv_slots = c->stat_kv_pos = 0.0;
    c->kvstat_n = 0;
    *chunk = 0;
    if (n == 0) return 0;
    if (kvstat_caps > 0) {
        CAPDEC_TRY(c->kvstat.ensure((size_t)kvstat_caps * 2 * sizeof(unsigned)));
        CAPDEC_HIP(hipMemsetAsync(c->kvstat.p, 0, (size_t)kvstat_caps * 2 * sizeof(unsigned), c->stream));
        c->kvstat_n = kvstat_caps;
    }
    *chunk = chunk_captions(c, n, rows_per_caption, ctx, extra_per_cap);
    c->stat_chunks = (n + *chunk - 1) / *chunk;
    if (lm_rows_per_cap > 0) {
        CAPDEC_TRY(c->lmflag.ensure(((size_t)*chunk * lm_rows_per_cap + 2) * 4));
        CAPDEC_HIP(hipMemsetAsync(c->lmflag.p, 0, 2 * sizeof(int), c->stream));
    }
    c->lmflag_live = false;
    c->k3_off = false;
    c->k3_rows = 0;
    return 0;
}

// a call's constants for the chunk that starts at caption c0
DecodeCall chunk_call(const DecodeCall &call, int c0) {
    const int T = call.T, beam = call.beam;
    DecodeCall a = call;
    a.ids += (size_t)c0 * beam * T;
    a.lens += (size_t)c0 * beam;
    if (a.scores) a.scores += (size_t)c0 * beam;
    if (a.order) a.order += (size_t)c0 * beam;
    if (a.forced) a.forced += (size_t)c0 * T;
    if (a.stats) a.stats += (size_t)c0 * T * 3;
    if (a.u) a.u += (size_t)c0 * T;
    if (a.logp) a.logp += (size_t)c0 * T;
    if (a.glogp) a.glogp += (size_t)c0 * beam;
    if (a.phrases) a.phrases += (size_t)c0 * CON_PHRASES * CON_LEN;
    if (a.met) a.met += (size_t)c0 * beam;
    a.cap_off = c0;
    return a;
}

// The workspaces and the greedy or the beam state of a chunk of nc captions, zeroed.  halves = 2 (the guided decode): every
// caption has a partner nc captions further on -- twice the K/V rows, next_tok, ancestor rows and body workspace; the state
// proper lives with the first half alone.
int decode_state(capdec_ctx *c, int nc, const DecodeCall &a, int halves, DecodeState *s) {
    const int T = a.T, ctx = a.P + T - 1, rows = nc * a.beam;
    CAPDEC_TRY(ensure_kv(c, s->kv, halves * rows, ctx));
    s->kv.fixed_variant = c->batch_invariant;
    s->kv.prefix_len = a.P;
    CAPDEC_TRY(ensure_body_ws(c, halves * std::max(nc * a.P, rows), c->gpt.d));
    CAPDEC_TRY(c->next_tok.ensure((size_t)halves * rows * 4));
    CAPDEC_TRY(c->alive.ensure(sizeof(int)));
    CAPDEC_TRY(c->done.ensure((size_t)rows));
    BeamState &bs = s->bs;
    GreedyState &gs = s->gs;
    if (!a.greedy) {
        CAPDEC_TRY(c->tokens.ensure((size_t)rows * T * 4));
        CAPDEC_TRY(c->scores.ensure((size_t)rows * 4));
        CAPDEC_TRY(c->seq.ensure((size_t)rows * 4));
        CAPDEC_TRY(c->stopped.ensure((size_t)rows));
        CAPDEC_TRY(c->anc.ensure((size_t)halves * rows * ctx));
        bs.tokens = c->tokens.as<int>();
        bs.scores = c->scores.as<float>();
        bs.seq = c->seq.as<float>();
        bs.stopped = c->stopped.as<uint8_t>();
        bs.done = c->done.as<uint8_t>();
        bs.anc = c->anc.as<uint8_t>();
        bs.next_tok = c->next_tok.as<int>();
        bs.alive_count = c->alive.as<int>();
        if (a.groups > 0) {
            CAPDEC_TRY(c->glogp.ensure((size_t)rows * 4));
            bs.logp = c->glogp.as<float>();
        }
        if (a.phrases) {            // the chunk's phrases by chunk-local caption, every slot in the empty state
            CAPDEC_TRY(c->cstate.ensure((size_t)rows * 4));
            s->cs.phrases = a.phrases;
            s->cs.state = c->cstate.as<int>();
            CAPDEC_HIP(hipMemsetAsync(s->cs.state, 0, (size_t)rows * 4, c->stream));
        }
        // (distinct-K/V-slot statistic: this chunk's slice of the per-call array decode_call_begin zeroed; nothing is read
        //  back here -- capdec_decode_counters sums it when somebody asks)
        bs.kv_stat = c->kvstat.p ? c->kvstat.as<unsigned>() + (size_t)a.cap_off * 2 : nullptr;
        CAPDEC_HIP(hipMemsetAsync(bs.tokens, 0, (size_t)rows * T * 4, c->stream));
        CAPDEC_HIP(hipMemsetAsync(bs.anc, 0, (size_t)halves * rows * ctx, c->stream));
    } else {
        gs.ids = a.ids;
        gs.lens = a.lens;
        gs.done = c->done.as<uint8_t>();
        gs.next_tok = c->next_tok.as<int>();
        gs.alive_count = c->alive.as<int>();
        gs.logp = a.logp;
        gs.T = T;
        gs.stop_id = a.stop_id;
        gs.alt_stop_id = a.alt_stop_id;
        CAPDEC_HIP(hipMemsetAsync(a.ids, 0, (size_t)nc * T * 4, c->stream));
        CAPDEC_HIP(hipMemsetAsync(a.lens, 0, (size_t)nc * 4, c->stream));
        if (a.logp) CAPDEC_HIP(hipMemsetAsync(a.logp, 0, (size_t)nc * T * 4, c->stream));
    }
    CAPDEC_HIP(hipMemsetAsync(c->done.p, 0, (size_t)rows, c->stream));
    CAPDEC_HIP(hipMemsetAsync(c->alive.p, 0, sizeof(int), c->stream));
    s->hist = a.greedy ? a.ids : bs.tokens;
    s->anc = a.greedy ? nullptr : bs.anc;
    return 0;
}

// The step kernel of the decode over what the lm_head left for the R rows (c->lse / c->topv / c->topi, k per row): greedy,
// or the beam / group-beam bookkeeping -- its first form at step 0, where a caption is one row.
int decode_advance(capdec_ctx *c, const DecodeCall &a, const DecodeState &s, int R, int step, int k, const int *cmap) {
    const int P = a.P, T = a.T, beam = a.beam, ctx = P + T - 1, V = c->gpt.vocab;
    ProfScope ps(c, F_SELECT);
    const float *lse = c->lse.as<float>(), *topv = c->topv.as<float>();
    const int *topi = c->topi.as<int>();
    if (a.greedy) return launch_greedy_step(c->stream, s.gs, topi, R, step, k, a.forced, topv, lse, a.stats);
    if (a.phrases) {                // (the lists are lm_head_rows_forced's: CON_LIST places per row)
        if (step == 0) return launch_constrained_beam_init(c->stream, s.bs, s.cs, lse, topv, topi, R, beam, T, V, a.stop_id);
        return launch_constrained_beam_step(c->stream, s.bs, s.cs, lse, topv, topi, R / beam, beam, T, ctx, step, P + step - 1, V,
                                            a.stop_id, cmap);
    }
    if (a.groups > 0) {
        if (step == 0)
            return launch_group_beam_init(c->stream, s.bs, lse, topv, topi, R, beam, a.groups, a.diversity, k, T, a.stop_id);
        return launch_group_beam_step(c->stream, s.bs, lse, topv, topi, R / beam, beam, a.groups, a.diversity, k, T, ctx, step,
                                      P + step - 1, V, a.stop_id, cmap);
    }
    if (step == 0) return launch_beam_init(c->stream, s.bs, lse, topv, topi, R, beam, k, T, a.stop_id);
    return launch_beam_step(c->stream, s.bs, lse, topv, topi, R / beam, beam, k, T, ctx, step, P + step - 1, V, a.stop_id, cmap);
}

// GPT-2's blocks over the `rows` activation rows of one decode step at context length L (c->h in place)
int gpt2_step(capdec_ctx *c, const KvCache &kv, int rows, int beam, int L, const uint8_t *anc, const int *cmap) {
    StepShape sd{};
    sd.prefill = false;
    sd.rows = rows;
    sd.beam = beam;
    sd.L = L;
    sd.anc = anc;
    sd.anc_stride = kv.ctx;
    sd.cmap = cmap;
    return gpt2_body(c, sd, kv);
}

// ---------------------------------------------------------------------------- the step loop
// Steps l.first .. l.T - 1 of a chunk of l.nc captions, each l.rows_per_caption activation rows: everything between "the
// first selection has run" and "every caption is done or T is reached".  Finished captions (l.done: stop token on every
// beam) are dropped from the batch at the poll points (decode_sched.h says when): the compaction map lists the na captions
// still generating, the activations of a step are the rows of those captions only, while KV cache / ancestor table / state
// keep their original rows.  The map has l.map_slots slots, the device-side count behind them.  The drivers plug in
//   after_compact(cmap, na)   what else has to follow a new map (may be empty)
//   step(i, na, cmap)         the body of step i over the na captions of cmap (nullptr: all of them, in order)
int decode_steps(capdec_ctx *c, const StepLoop &l, const AfterCompact &after_compact, const StepFn &step) {
    CAPDEC_TRY(c->cmap.ensure(((size_t)l.map_slots + 1) * 4));
    PollSchedule sched(l.nc);
    int na = l.nc;
    const int *cmap = nullptr;
    for (int i = l.first; i < l.T; ++i) {
        if (sched.due(i)) {
            int alive = 0;
            CAPDEC_TRY(poll_alive(c, &alive));
            if (alive == 0) break;
            sched.polled(i, alive, l.rows_per_caption);
            if (c->compact && compaction_pays(na, alive)) {
                ProfScope ps(c, F_SELECT);
                int *m = c->cmap.as<int>();
                CAPDEC_TRY(launch_compact_alive(c->stream, l.done, l.nc, m, m + l.map_slots));
                na = alive;
                cmap = m;
                c->stat_compactions += 1;
                if (after_compact) CAPDEC_TRY(after_compact(m, na));
            }
        }
        const int arows = na * l.rows_per_caption, s = i - l.first;
        c->stat_steps = std::max(c->stat_steps, i + 1);
        c->stat_row_steps += arows;
        if ((int)c->stat_step_rows.size() <= s) c->stat_step_rows.resize(s + 1, 0);     // (chunks of one call add up step by step)
        c->stat_step_rows[s] += arows;
        CAPDEC_HIP(hipMemsetAsync(c->alive.p, 0, sizeof(int), c->stream));
        CAPDEC_TRY(step(i, na, cmap));
    }
    return 0;
}

// ---------------------------------------------------------------------------- the plain drivers: greedy, beam, sampling
static int decode_chunk(capdec_ctx *c, const float *prefix, int nc, const DecodeCall &a) {
    const Gpt2 &g = c->gpt;
    const int d = g.d, P = a.P, T = a.T, beam = a.beam;
    const int k = (a.greedy && a.stats) ? 2 : beam;   // candidates kept per row (teacher-forced statistics: top-2)
    const float inv_temp = 1.0f / (a.temperature > 0.f ? a.temperature : 1.0f);
    const bool proc = !a.forced && processors_on(c, a.sample);      // (teacher forcing ignores the processors)
    DecodeState s;
    CAPDEC_TRY(decode_state(c, nc, a, 1, &s));
    s.bs.diverge = c->diverge;

    // Select and advance: the lm_head route of this call over the R rows of h at h0 (row stride ldh), then the step
    // kernel of the decode.  hbeam: rows per caption for the history lookup; cmap: the compaction in force.
    auto select_and_advance = [&](const float *h0, int ldh, int R, int step, int hbeam, const int *cmap) -> int {
        s.gs.cmap = cmap;
        if (a.phrases) CAPDEC_TRY(lm_head_rows_forced(c, h0, ldh, R, inv_temp, a, s, proc, step, cmap));
        else if (proc || a.sample) CAPDEC_TRY(lm_head_rows(c, h0, ldh, R, k, inv_temp, a, s.gs, proc, step, hbeam, s.hist));
        else CAPDEC_TRY(lm_head_select(c, h0, ldh, R, k, inv_temp));
        if (a.sample) return 0;                         // (the sampling kernel has advanced the state)
        return decode_advance(c, a, s, R, step, k, cmap);
    };

    // ---- step 0: prefill the prefix (positions 0..P-1), logits of the last prefix row
    { ProfScope ps(c, F_EMBED); CAPDEC_TRY(launch_embed_prefix(c->stream, prefix, g.wpe, c->h.as<float>(), nc, P, 0, d)); }
    StepShape sp{};
    sp.prefill = true;
    sp.ncap = nc;
    sp.P = P;
    sp.beam = beam;
    CAPDEC_TRY(gpt2_body(c, sp, s.kv));
    // (one row per caption and an empty history: nothing is read through `hist` yet)
    CAPDEC_TRY(select_and_advance(c->h.as<float>() + (size_t)(P - 1) * d, P * d, nc, 0, 1, nullptr));
    // ---- steps 1..T-1: one token per row per step
    const StepLoop loop{nc, 1, T, beam, c->done.as<uint8_t>(), nc};
    CAPDEC_TRY(decode_steps(c, loop, nullptr, [&](int i, int na, const int *cmap) -> int {
        const int pos = P + i - 1;   // position of the token fed this step
        const int arows = na * beam;
        {
            ProfScope ps(c, F_EMBED);
            CAPDEC_TRY(launch_embed_tokens(c->stream, c->next_tok.as<int>(), g.wte, g.wpe + (size_t)pos * d,
                                           c->h.as<float>(), arows, d, cmap, beam));
        }
        CAPDEC_TRY(gpt2_step(c, s.kv, arows, beam, pos + 1, s.anc, cmap));
        return select_and_advance(c->h.as<float>(), d, arows, i, beam, cmap);
    }));
    if (!a.greedy) {
        ProfScope ps(c, F_SELECT);
        CAPDEC_TRY(launch_beam_finalize(c->stream, s.bs, nc, beam, T, a.ids, a.lens, a.scores, a.order, s.cs.state, a.met));  // (both null without phrases)
        if (a.glogp) CAPDEC_TRY(launch_group_beam_logp(c->stream, s.bs, nc, beam, a.order, a.glogp));
    }
    return 0;
}

static int decode_common(capdec_ctx *c, const float *prefix, int n, const DecodeCall &call) {
    const int P = call.P, T = call.T, beam = call.beam, ctx = P + T - 1;
    CAPDEC_TRY(decode_call_checks(c, "decode", CK_LOADED | CK_SIZES | CK_CONTEXT, n, P, T, (long long)P + T - 1));
    CAPDEC_CHECK(beam >= 1 && beam <= 8, "decode: beam size must be in 1..8");
    CAPDEC_TRY(decode_call_checks(c, "decode", CK_HEAD_DIM | (call.forced ? 0 : CK_BIAS), n, P, T, ctx));
    int chunk = 0;
    CAPDEC_TRY(decode_call_begin(c, n, 1, call.greedy ? 0 : n, beam, ctx, 0, beam, &chunk));
    for (int c0 = 0; c0 < n; c0 += chunk)
        CAPDEC_TRY(decode_chunk(c, prefix + (size_t)c0 * P * c->gpt.d, std::min(chunk, n - c0), chunk_call(call, c0)));
    if (n > 0) CAPDEC_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

}  // namespace capdec

using namespace capdec;

extern "C" {

int capdec_gpt2_logits(capdec_ctx *c, const float *embeds, int n, int L, int all_positions, float *logits) {
    CAPDEC_CHECK(c && c->gpt.loaded, "gpt2_logits: GPT-2 weights not loaded");
    CAPDEC_CHECK(embeds && logits && n >= 1 && L >= 1 && L <= 1024 && L <= c->gpt.n_pos, "gpt2_logits: bad argument");
    CAPDEC_HIP(hipSetDevice(c->device));
    const Gpt2 &g = c->gpt;
    const int d = g.d;
    KvCache kv;
    CAPDEC_TRY(ensure_kv(c, kv, n, L));
    CAPDEC_TRY(ensure_body_ws(c, n * L, d));
    { ProfScope ps(c, F_EMBED); CAPDEC_TRY(launch_embed_prefix(c->stream, embeds, g.wpe, c->h.as<float>(), n, L, 0, d)); }
    StepShape sp{};
    sp.prefill = true;
    sp.ncap = n;
    sp.P = L;
    sp.beam = 1;
    CAPDEC_TRY(gpt2_body(c, sp, kv));
    const int R = all_positions ? n * L : n;
    const float *h0 = all_positions ? c->h.as<float>() : c->h.as<float>() + (size_t)(L - 1) * d;
    const int ldh = all_positions ? d : L * d;
    return lm_head_logits(c, h0, ldh, R, logits, g.vocab);
}

int capdec_cross_entropy(capdec_ctx *c, const float *logits, int ld, const int32_t *labels, int rows, int vocab,
                         int ignore_index, float *loss) {
    CAPDEC_CHECK(c && loss && (rows == 0 || (logits && labels)), "cross_entropy: null argument");
    CAPDEC_CHECK(rows >= 0 && vocab > 0 && ld >= vocab, "cross_entropy: bad sizes");
    CAPDEC_HIP(hipSetDevice(c->device));
    if (rows == 0) return 0;
    CAPDEC_TRY(c->xl.ensure((size_t)rows * sizeof(float)));
    ProfScope ps(c, F_SELECT);
    return launch_cross_entropy_mean(c->stream, logits, ld, labels, rows, vocab, ignore_index, c->xl.as<float>(), loss);
}

int capdec_wte_lookup(capdec_ctx *c, const int32_t *ids, int n, float *out) {
    CAPDEC_CHECK(c && c->gpt.loaded, "wte_lookup: GPT-2 weights not loaded");
    CAPDEC_HIP(hipSetDevice(c->device));
    ProfScope ps(c, F_EMBED);
    return launch_gather_rows(c->stream, c->gpt.wte, ids, out, n, c->gpt.d);
}

int capdec_decode_greedy(capdec_ctx *c, const float *prefix, int n, int P, int stop_id, int alt_stop_id,
                         int entry_length, int32_t *ids, int32_t *lens) {
    CAPDEC_CHECK(c && (n == 0 || (prefix && ids && lens)), "decode_greedy: null argument");
    DecodeCall a;
    a.P = P; a.stop_id = stop_id; a.alt_stop_id = alt_stop_id; a.T = entry_length;
    a.ids = ids; a.lens = lens;
    return decode_common(c, prefix, n, a);
}

int capdec_decode_greedy_forced(capdec_ctx *c, const float *prefix, int n, int P, int entry_length,
                                const int32_t *forced, int32_t *ids, float *stats) {
    CAPDEC_CHECK(c && (n == 0 || (prefix && forced && ids)), "decode_greedy_forced: null argument");
    DBuf lens;
    CAPDEC_TRY(lens.ensure((size_t)std::max(n, 1) * 4));
    const bool compact = c->compact;
    c->compact = false;                       // every caption runs every step
    DecodeCall a;
    a.P = P; a.T = entry_length;
    a.ids = ids; a.lens = lens.as<int>();
    a.forced = forced; a.stats = stats;
    const int rc = decode_common(c, prefix, n, a);
    c->compact = compact;
    lens.release();
    return rc;
}

int capdec_decode_sample(capdec_ctx *c, const float *prefix, int n, int P, int stop_id, int alt_stop_id, int entry_length,
                         float temperature, float top_p, uint64_t seed, const float *u, int32_t *ids, int32_t *lens,
                         float *logp) {
    CAPDEC_CHECK(top_p == top_p && temperature == temperature, "decode_sample: top_p or temperature is NaN");
    CAPDEC_CHECK(c && (n == 0 || (prefix && ids && lens)), "decode_sample: null argument");
    DecodeCall a;
    a.P = P; a.stop_id = stop_id; a.alt_stop_id = alt_stop_id; a.T = entry_length; a.temperature = temperature;
    a.ids = ids; a.lens = lens;
    a.sample = true; a.top_p = top_p; a.seed = seed; a.u = u; a.logp = logp;
    return decode_common(c, prefix, n, a);
}

int capdec_decode_beam(capdec_ctx *c, const float *prefix, int n, int P, int beam, int stop_id, int entry_length,
                       float temperature, int32_t *ids, int32_t *lens, float *scores, int32_t *order) {
    CAPDEC_CHECK(c && (n == 0 || (prefix && ids && lens && scores)), "decode_beam: null argument");
    CAPDEC_CHECK(c->gpt.loaded && c->gpt.vocab >= beam, "decode_beam: vocabulary smaller than the beam");
    DecodeCall a;
    a.P = P; a.beam = beam; a.greedy = false; a.stop_id = stop_id; a.T = entry_length; a.temperature = temperature;
    a.ids = ids; a.lens = lens; a.scores = scores; a.order = order;
    return decode_common(c, prefix, n, a);
}

int capdec_decode_beam_groups(capdec_ctx *c, const float *prefix, int n, int P, int beam, int groups, float diversity_penalty,
                              int stop_id, int entry_length, float temperature, int32_t *ids, int32_t *lens, float *scores,
                              int32_t *order, float *logp) {
    CAPDEC_CHECK(c && (n == 0 || (prefix && ids && lens && scores)), "decode_beam_groups: null argument");
    CAPDEC_CHECK(beam >= 1 && beam <= 8, "decode_beam_groups: beam size must be in 1..8");
    CAPDEC_CHECK(groups >= 1, "decode_beam_groups: groups must be >= 1");
    CAPDEC_CHECK(groups <= beam, "decode_beam_groups: more groups than beams");
    CAPDEC_CHECK(beam % groups == 0, "decode_beam_groups: groups must divide the beam size");
    CAPDEC_CHECK(diversity_penalty >= 0.f && diversity_penalty <= 3.0e38f,
                 "decode_beam_groups: the diversity penalty must be finite and >= 0");
    CAPDEC_CHECK(c->gpt.loaded && c->gpt.vocab >= beam, "decode_beam_groups: vocabulary smaller than the beam");
    DBuf own_order;             // the log-prob sums are gathered through the order: keep one when the caller wants none
    if (logp && !order && n > 0) {
        CAPDEC_TRY(own_order.ensure((size_t)n * beam * 4));
        order = own_order.as<int32_t>();
    }
    DecodeCall a;
    a.P = P; a.beam = beam; a.greedy = false; a.stop_id = stop_id; a.T = entry_length; a.temperature = temperature;
    a.ids = ids; a.lens = lens; a.scores = scores; a.order = order;
    a.groups = groups; a.diversity = diversity_penalty; a.glogp = logp;
    const int rc = decode_common(c, prefix, n, a);
    own_order.release();
    return rc;
}

int capdec_decode_beam_constrained(capdec_ctx *c, const float *prefix, const int32_t *phrases, int n, int P, int beam,
                                   int stop_id, int entry_length, float temperature, int32_t *ids, int32_t *lens,
                                   float *scores, int32_t *order, int32_t *met) {
    const char *who = "decode_beam_constrained: ";
    CAPDEC_CHECK(beam >= 1 && beam <= 8, "decode_beam_constrained: beam size must be in 1..8");
    CAPDEC_CHECK(c && (n == 0 || (prefix && phrases && ids && lens && scores)), "decode_beam_constrained: null argument");
    CAPDEC_CHECK(c->gpt.loaded && c->gpt.vocab >= beam, "decode_beam_constrained: vocabulary smaller than the beam");
    CAPDEC_CHECK(n >= 0, "decode_beam_constrained: bad sizes");
    if (n > 0) {                    // the phrase tables are read on the host before anything is launched
        CAPDEC_HIP(hipSetDevice(c->device));
        std::vector<int32_t> ph((size_t)n * CON_PHRASES * CON_LEN);
        CAPDEC_HIP(hipMemcpyAsync(ph.data(), phrases, ph.size() * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        CAPDEC_HIP(hipStreamSynchronize(c->stream));
        const int V = c->gpt.vocab;
        for (int r = 0; r < n; ++r) {
            bool empty_seen = false;
            for (int p = 0; p < CON_PHRASES; ++p) {
                const int32_t *w = ph.data() + ((size_t)r * CON_PHRASES + p) * CON_LEN;
                const std::string at = " (caption " + std::to_string(r) + ", phrase " + std::to_string(p) + ")";
                bool end_seen = false;
                for (int q = 0; q < CON_LEN; ++q) {
                    if (w[q] == -1) { end_seen = true; continue; }
                    CAPDEC_CHECK(w[q] >= 0 && w[q] < V, who + std::string("a token id outside the vocabulary") + at);
                    CAPDEC_CHECK(w[q] != stop_id, who + std::string("a phrase holds the stop token") + at);
                    CAPDEC_CHECK(!end_seen, who + std::string("a hole in front of a used place") + at);
                    CAPDEC_CHECK(!empty_seen, who + std::string("a hole in front of a used place: an empty phrase in front") + at);
                }
                if (w[0] == -1) empty_seen = true;
            }
        }
    }
    DecodeCall a;
    a.P = P; a.beam = beam; a.greedy = false; a.stop_id = stop_id; a.T = entry_length; a.temperature = temperature;
    a.ids = ids; a.lens = lens; a.scores = scores; a.order = order;
    a.phrases = phrases; a.met = met;
    return decode_common(c, prefix, n, a);
}


}  // extern "C"
