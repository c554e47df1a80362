// The GEMM dispatch behind every projection of the path: the cache of packed weight planes, which operand format a launch
// takes in the context's precision mode, the LayerNorm -> GEMM and packed-chain forms of the block stack, the fused lm_head
// (LayerNorm -> GEMM -> per-tile top-k), and capdec_gemm_f32 / capdec_gemm_tn_f32 (the test / micro-benchmark hooks onto the
// same launchers).
// Every packed launch goes through launch_packed, which asks gemm_plan() (gemm_plan.h: a pure host function, tested without
// a GPU) for the kernel, tile geometry, split-K slices, grid and workspace size, attaches the workspace and hands the plan
// to the launcher -- nothing about a launch is decided anywhere else.
#include "context.h"

namespace capdec {

// ---------------------------------------------------------------------------- GEMM wrappers
// bf16 planes of an [N, K] fp32 weight matrix: made on first use, dropped whenever weights are reloaded
void drop_planes(capdec_ctx *c) {
    for (auto &kv : c->planes) (void)hipFree(kv.second.p);
    c->planes.clear();
}
void drop_planes_of(capdec_ctx *c, const void *weight) {       // every format cached for this weight
    for (auto it = c->planes.lower_bound({weight, -1}); it != c->planes.end() && it->first.first == weight;) {
        (void)hipFree(it->second.p);
        it = c->planes.erase(it);
    }
}
// packed operand format of the block-stack / lm_head GEMMs in the current mode (bf16x3.h): two fp16 planes (f16x2),
// three bf16 planes (bf16x3), or ONE bf16 / fp16 plane (the reduced-precision modes)
int pack_fmt(const capdec_ctx *c) {
    switch (c->gemm_mode) {
        case GEMM_F16X2: return PK_F16X2;
        case GEMM_BF16: return PK_BF16X1;
        case GEMM_F16: return PK_F16X1;
        default: return PK_BF16X3;
    }
}
int pack_any(capdec_ctx *c, const float *W, int N, int K, int fmt, void *out) {
    if (fmt == PK_F16X2) return launch_pack_planes_h2(c->stream, W, K, N, K, out);
    if (fmt == PK_BF16X3) return launch_pack_planes(c->stream, W, N, K, out);
    return launch_pack_planes_fmt(c->stream, W, K, N, K, out, fmt);
}
// max |w| < 16 ?  (one tiny reduction + a 4-byte read-back, once per cached weight)
static int weight_wide_ok(capdec_ctx *c, const float *W, size_t n, bool *ok) {
    CAPDEC_TRY(c->absmax.ensure(sizeof(unsigned)));
    CAPDEC_TRY(launch_absmax_bits(c->stream, W, n, c->absmax.as<unsigned>()));
    unsigned bits = 0;
    CAPDEC_HIP(hipMemcpyAsync(&bits, c->absmax.p, sizeof(bits), hipMemcpyDeviceToHost, c->stream));
    CAPDEC_HIP(hipStreamSynchronize(c->stream));
    float m;
    memcpy(&m, &bits, sizeof(m));
    *ok = m < 16.0f;
    return 0;
}
int planes_of(capdec_ctx *c, const float *W, int N, int K, bool cache, const void **out, int fmt_override,
                     bool *wide_ok) {
    const int fmt = fmt_override >= 0 ? fmt_override : pack_fmt(c);
    const size_t n = (size_t)N * K, bytes = x3_packed_bytes(N, K, fmt);
    if (wide_ok) *wide_ok = false;
    if (cache) {
        auto it = c->planes.find({W, fmt});
        if (it != c->planes.end()) {
            if (it->second.n == n) {
                *out = it->second.p;
                if (wide_ok) *wide_ok = it->second.wide_ok;
                return 0;
            }
            (void)hipFree(it->second.p);      // same address, different matrix
            c->planes.erase(it);
        }
        bool ok = false;
        if (fmt == PK_F16X2) CAPDEC_TRY(weight_wide_ok(c, W, n, &ok));      // (before the allocation: a failure leaks nothing)
        void *p = nullptr;
        CAPDEC_HIP(hipMalloc(&p, bytes));
        if (pack_any(c, W, N, K, fmt, p)) {
            (void)hipFree(p);
            return 1;
        }
        c->planes[{W, fmt}] = capdec_ctx::Planes{p, n, fmt, ok};
        *out = p;
        if (wide_ok) *wide_ok = ok;
        return 0;
    }
    CAPDEC_TRY(c->x3_tmp.ensure(bytes));
    CAPDEC_TRY(pack_any(c, W, N, K, fmt, c->x3_tmp.p));
    *out = c->x3_tmp.p;
    return 0;
}

int gemm_family(int fmt) { return fmt == PK_F16X2 ? F_GEMM_H2P : fmt == PK_BF16X3 ? F_GEMM_X3P : F_GEMM_BF16P; }

static_assert(PLAN_BF16X3 == PK_BF16X3 && PLAN_F16X2 == PK_F16X2 && PLAN_BF16X1 == PK_BF16X1 && PLAN_F16X1 == PK_F16X1 &&
                  PLAN_BK == X3_BK && GEMM_BM == 128 && GEMM_BN == 128,
              "gemm_plan.h restates these constants");

// C = epilogue(Apk . Bpk^T) with both operands packed in format fmt.  The ONE place where a packed launch is decided:
// gemm_plan() turns the shape, what the epilogue asks for and the caller's permissions into a plan (kernel, K slices, blocks,
// workspace); the workspace is attached here and the launcher of the plan's kernel runs it as it stands.
// split: the caller lets the launch split K; invariant: batch-invariant mode (the unsplit 128 x 128 kernel whatever M is).
// flops: what the profiler books for the launch
static int launch_packed(capdec_ctx *c, int fmt, const void *Apk, const void *Bpk, float *C, int ldc, int M, int N, int K,
                         GemmEpilogue &e, bool split, bool invariant, double flops) {
    e.tune = &c->tune;
    GemmPlanIn in;
    in.fmt = fmt; in.M = M; in.N = N; in.K = K;
    in.vec4 = gemm_vec4(e, C, ldc, N);
    in.wide_ok = e.wide_ok;
    in.invariant = invariant;
    in.split_ok = split && !c->batch_invariant;
    in.packed_out = e.packed_out != nullptr;
    in.resid_packed = e.resid_packed != nullptr;
    in.scatter = e.qkv_scatter != nullptr && e.qkv_scatter->kc != nullptr;
    in.tune = &c->tune;
    const GemmPlan plan = gemm_plan(in);
    if (plan.ws_bytes) {
        CAPDEC_TRY(c->splitk.ensure(plan.ws_bytes));
        e.splitk_ws = c->splitk.p;
    }
    ProfScope ps(c, gemm_family(fmt), flops);
    switch (plan.kernel) {
        case GK_H2W: return launch_gemm_h2w(c->stream, Apk, Bpk, C, ldc, M, N, K, e, plan);
        case GK_PP: case GK_PP_SPLITK: return launch_gemm_pp(c->stream, Apk, Bpk, C, ldc, M, N, K, e, plan);
        case GK_X3P: case GK_X3P_SPLITK: return launch_gemm_bf16x3p(c->stream, Apk, Bpk, C, ldc, M, N, K, e, plan);
        default: return launch_gemm_f16x2p(c->stream, Apk, Bpk, C, ldc, M, N, K, e, fmt, plan);      // (two planes or one)
    }
}

int gemm_native(capdec_ctx *c, const float *A, int lda, const float *Bt, int ldb, float *C, int ldc, int M, int N, int K,
                GemmEpilogue e) {
    e.tune = &c->tune;
    ProfScope ps(c, F_GEMM, 2.0 * M * (double)N * K);
    return launch_gemm_f32(c->stream, A, lda, Bt, ldb, C, ldc, M, N, K, e);
}

int gemm(capdec_ctx *c, const float *A, int lda, const float *Bt, int ldb, float *C, int ldc, int M, int N,
                int K, const float *bias, int act, const float *resid, int ldr, bool weight) {
    GemmEpilogue e;
    e.tune = &c->tune;
    e.bias = bias;
    e.act = act;
    e.resid = resid;
    e.ldr = ldr;
    if ((c->gemm_mode == GEMM_F16X2 || mode_single(c)) && ldb == K && K % 64 == 0 && lda % 4 == 0 && M > 0) {
        // fp32 activations in HBM (mapper, patch embedding, CLIP projections): one packing pass (read 4 B, write 4 B
        // per element), then the packed LDS-DMA kernel -- fp32-accurate (f16x2) also in the reduced-precision modes,
        // whose 16-bit operands are confined to the GPT-2 / CLIP block stacks and the lm_head
        const void *pl = nullptr;
        CAPDEC_TRY(planes_of(c, Bt, N, K, weight, &pl, PK_F16X2, &e.wide_ok));
        CAPDEC_TRY(c->a_tmp.ensure(x3_packed_bytes(M, K, PK_F16X2)));
        { ProfScope ps(c, F_PACK); CAPDEC_TRY(launch_pack_planes_h2(c->stream, A, lda, M, K, c->a_tmp.p)); }
        return launch_packed(c, PK_F16X2, c->a_tmp.p, pl, C, ldc, M, N, K, e, /*split=*/true, c->batch_invariant,
                             2.0 * M * (double)N * K);
    }
    // (bf16 mode: GEMMs whose A operand is fp32 in HBM -- mapper, patch embedding -- keep the split kernel)
    if (c->gemm_mode != GEMM_F32 && ldb == K && K % 64 == 0) {   // other K: native fp32 MFMA
        const void *pl = nullptr;
        CAPDEC_TRY(planes_of(c, Bt, N, K, weight, &pl));
        ProfScope ps(c, F_GEMM_X3, 2.0 * M * (double)N * K);
        return launch_gemm_bf16x3(c->stream, A, lda, pl, C, ldc, M, N, K, e);
    }
    return gemm_native(c, A, lda, Bt, ldb, C, ldc, M, N, K, e);
}

// C [N1, N2] = Xa^T Xb for fp32 Xa [rows, N1], Xb [rows, N2] (row-major, row strides lda / ldb): the weight-gradient product of the train
// step (dW = dY^T X, K = the token rows).  Both operands are packed TRANSPOSED straight from their row-major form
// (launch_pack_planes_h2_t: no fp32 transposed copies), then the two-fp16-plane kernels run with K = rows padded to 64.
int gemm_tn(capdec_ctx *c, const float *Xa, int lda, const float *Xb, int ldb, int rows, int N1, int N2, float *C, int ldc) {
    const int Kp = (rows + 63) / 64 * 64;
    CAPDEC_TRY(c->a_tmp.ensure(x3_packed_bytes(N1, Kp, PK_F16X2)));
    CAPDEC_TRY(c->x3_tmp.ensure(x3_packed_bytes(N2, Kp, PK_F16X2)));
    {
        ProfScope ps(c, F_PACK);
        CAPDEC_TRY(launch_pack_planes_h2_t(c->stream, Xa, lda, rows, N1, Kp, c->a_tmp.p));
        CAPDEC_TRY(launch_pack_planes_h2_t(c->stream, Xb, ldb, rows, N2, Kp, c->x3_tmp.p));
    }
    GemmEpilogue e;
    return launch_packed(c, PK_F16X2, c->a_tmp.p, c->x3_tmp.p, C, ldc, N1, N2, Kp, e, /*split=*/true, c->batch_invariant,
                         2.0 * N1 * (double)N2 * rows);
}

// LayerNorm -> GEMM with the normalised rows handed over as the packed A operand of the mode (never fp32 in HBM)?
// Otherwise the caller runs the fp32-activation path.
bool use_packed_a(capdec_ctx *c, int K) {
    return (mode_single(c) || c->gemm_mode == GEMM_F16X2 || (c->gemm_mode == GEMM_BF16X3 && c->pack_a)) && K % 64 == 0;
}

// C = act(Apk . W^T + bias) + resid with A already packed; packed_out != nullptr: the result is written as the
// packed A operand of the next GEMM instead of fp32 C
// (next_ln: the LayerNorm that follows this GEMM in the block stack; when the launch splits K it is fused into the
//  reduce pass, its packed output lands in c->xpk and *ln_done is set -- see GemmEpilogue)
int gemm_packed(capdec_ctx *c, const void *Apk, const float *W, float *C, int ldc, int M, int N, int K,
                       const float *bias, int act, const float *resid, int ldr,
                       void *packed_out, const NextLn *next_ln, const void *resid_packed,
                       const QkvScatter *qkv_scatter) {
    const void *pl = nullptr;
    GemmEpilogue e;
    e.qkv_scatter = qkv_scatter;
    CAPDEC_TRY(planes_of(c, W, N, K, true, &pl, -1, &e.wide_ok));
    e.bias = bias;
    e.act = act;
    e.resid = resid;
    e.ldr = ldr;
    e.packed_out = packed_out;
    e.resid_packed = resid_packed;
    if (next_ln && next_ln->w && ldc == N && (const void *)Apk != c->xpk.p) {
        CAPDEC_TRY(c->xpk.ensure(x3_packed_bytes_host(M, N)));
        e.ln_w = next_ln->w; e.ln_b = next_ln->b; e.ln_eps = next_ln->eps; e.ln_out = c->xpk.p; e.ln_done = next_ln->done;
    }
    // (no split-K under the qkv scatter; the one-plane kernels split only under CAPDEC_X1_SPLITK)
    const bool split = c->gemm_mode != GEMM_F32 && !qkv_scatter && (!mode_single(c) || c->tune.x1_splitk);
    return launch_packed(c, pack_fmt(c), Apk, pl, C, ldc, M, N, K, e, split, c->batch_invariant, 2.0 * M * (double)N * K);
}

// (ln_ready: c->xpk already holds LayerNorm(h) -- written by the fused split-K reduce of the previous GEMM)
int ln_gemm_packed(capdec_ctx *c, const float *h, int ldh, const float *lnw, const float *lnb, float eps,
                          const float *W, float *C, int ldc, int M, int N, int K, const float *bias, int act,
                          void *packed_out, bool ln_ready, const QkvScatter *qkv_scatter) {
    CAPDEC_TRY(c->xpk.ensure(x3_packed_bytes_host(M, K)));
    if (!ln_ready) {
        ProfScope ps(c, F_LN);
        CAPDEC_TRY(launch_layernorm_packed(c->stream, h, ldh, lnw, lnb, eps, c->xpk.p, M, K, pack_fmt(c)));
    }
    return gemm_packed(c, c->xpk.p, W, C, ldc, M, N, K, bias, act, nullptr, 0, packed_out, nullptr, nullptr, qkv_scatter);
}

int topk_workspace(capdec_ctx *c, int rows, int ntiles, int k, TopkOut *o) {
    CAPDEC_TRY(c->tmax.ensure((size_t)rows * ntiles * 4));
    CAPDEC_TRY(c->tsum.ensure((size_t)rows * ntiles * 4));
    CAPDEC_TRY(c->cval.ensure((size_t)rows * ntiles * k * 4));
    CAPDEC_TRY(c->cidx.ensure((size_t)rows * ntiles * k * 4));
    CAPDEC_TRY(c->lse.ensure((size_t)rows * 4));
    *o = TopkOut{c->tmax.as<float>(), c->tsum.as<float>(), c->cval.as<float>(), c->cidx.as<int>()};
    return 0;
}

// The tile of a fused top-k launch on two fp16 planes: 256 x 128 with one accumulator set once the grid is many rounds deep
// (each W panel is then fetched by half as many row tiles); small row counts keep the 128-row tile (more blocks, the same
// partial lists).  wide_ok: max |w| < 16 (GemmEpilogue::wide_ok).  (CAPDEC_H2W >= 2: forced, tests)
static bool topk_wide_tile(const capdec_ctx *c, bool wide_ok, int M) {
    const int h2w = c->tune.h2w;
    return wide_ok && !c->batch_invariant && ((c->tune.lmhead_wide && h2w >= 1 && M >= 2048) || h2w >= 2);
}

int lm_head_wide_tile(capdec_ctx *c, const float *W, int M, int N, int K, bool *wide) {
    *wide = false;
    if (c->gemm_mode != GEMM_F16X2 || !use_packed_a(c, K)) return 0;
    const void *pl = nullptr;
    bool wide_ok = false;
    CAPDEC_TRY(planes_of(c, W, N, K, true, &pl, -1, &wide_ok));
    *wide = topk_wide_tile(c, wide_ok, M);
    return 0;
}

int ln_gemm_topk(capdec_ctx *c, const float *h, int ldh, const float *lnw, const float *lnb, float eps, const float *W,
                 int M, int N, int K, int k, float inv_temp, const TopkOut &o, bool k3_ok, bool *k3, bool no_cand) {
    const double flops = 2.0 * M * (double)N * K;
    *k3 = false;
    CAPDEC_CHECK(!no_cand || (c->gemm_mode == GEMM_F16X2 && use_packed_a(c, K)), "ln_gemm_topk: only the wide two-plane kernel runs without candidates");
    if (!use_packed_a(c, K)) {
        CAPDEC_TRY(c->xl.ensure((size_t)M * K * 4));
        float *x = c->xl.as<float>();
        { ProfScope ps(c, F_LN); CAPDEC_TRY(launch_layernorm(c->stream, h, ldh, lnw, lnb, eps, x, K, M, K)); }
        if (c->gemm_mode == GEMM_F32) {
            ProfScope ps(c, F_LMHEAD, flops);
            return launch_gemm_f32_topk(c->stream, x, K, W, K, M, N, K, k, inv_temp, o);
        }
        const void *pl = nullptr;
        CAPDEC_TRY(planes_of(c, W, N, K, true, &pl));
        ProfScope ps(c, F_LMHEAD_X3, flops);
        return launch_gemm_bf16x3_topk(c->stream, x, K, pl, M, N, K, k, inv_temp, o);
    }
    CAPDEC_TRY(c->xpk.ensure(x3_packed_bytes_host(M, K)));
    { ProfScope ps(c, F_LN); CAPDEC_TRY(launch_layernorm_packed(c->stream, h, ldh, lnw, lnb, eps, c->xpk.p, M, K, pack_fmt(c))); }
    const void *pl = nullptr;
    bool wide_ok = false;
    CAPDEC_TRY(planes_of(c, W, N, K, true, &pl, -1, &wide_ok));
    if (c->gemm_mode == GEMM_F16X2) {
        ProfScope ps(c, F_LMHEAD_H2, flops);
        if (topk_wide_tile(c, wide_ok, M)) {
            if (no_cand) return launch_gemm_h2w_topk(c->stream, c->xpk.p, pl, M, N, K, 0, inv_temp, o);
            *k3 = k3_ok;
            return launch_gemm_h2w_topk(c->stream, c->xpk.p, pl, M, N, K, *k3 ? 3 : k, inv_temp, o);
        }
        CAPDEC_CHECK(!no_cand, "ln_gemm_topk: only the wide two-plane kernel runs without candidates");
        return launch_gemm_f16x2p_topk(c->stream, c->xpk.p, pl, M, N, K, k, inv_temp, o, PK_F16X2);
    }
    if (mode_single(c)) {
        ProfScope ps(c, F_LMHEAD_BF16, flops);
        *k3 = k3_ok && M >= 2048 && !c->batch_invariant;      // (as for the wide two-plane tile above)
        return launch_gemm_f16x2p_topk(c->stream, c->xpk.p, pl, M, N, K, *k3 ? 3 : k, inv_temp, o, pack_fmt(c));
    }
    ProfScope ps(c, F_LMHEAD_X3, flops);
    return launch_gemm_bf16x3p_topk(c->stream, c->xpk.p, pl, M, N, K, k, inv_temp, o);
}

int gemm_topk_dev(capdec_ctx *c, const void *Apk, const float *W, const int *m_dev, int N, int K, float inv_temp,
                  const TopkOut &o) {
    const void *pl = nullptr;
    CAPDEC_TRY(planes_of(c, W, N, K, true, &pl));
    if (mode_single(c)) return launch_gemm_x1_topk_dev(c->stream, Apk, pl, m_dev, N, K, inv_temp, o, pack_fmt(c));
    return launch_gemm_h2w_topk_dev(c->stream, Apk, pl, m_dev, N, K, inv_temp, o);
}

int gemm_topk_grouped(capdec_ctx *c, const void *Apk, const float *W, const SparseLm &s, int blocks_cap, int N, int K,
                      float inv_temp, float *cand_val, int *cand_idx) {
    CAPDEC_CHECK(c->gemm_mode == GEMM_F16X2, "gemm_topk_grouped: two-plane operands only");
    const void *pl = nullptr;
    CAPDEC_TRY(planes_of(c, W, N, K, true, &pl));
    return launch_gemm_h2w_topk_grouped(c->stream, Apk, pl, s.nblk, s.blk_tab, s.slot_of, LM_SPARSE_SHIFT, blocks_cap, N, K, inv_temp,
                                        cand_val, cand_idx);
}

// gemm()'s rule for fp32 activations: the packed two-fp16-plane path in the f16x2 and the one-plane modes when K % 64 == 0
bool topk_packed_a(const capdec_ctx *c, int K) { return (c->gemm_mode == GEMM_F16X2 || mode_single(c)) && K % 64 == 0; }

int gemm_topk(capdec_ctx *c, const void *A, const float *Bt, bool cache, bool b_small, int M, int N, int K, int k,
              const TopkOut &o, float *lse, float *top_val, int *top_idx) {
    const double flops = 2.0 * M * (double)N * K;
    if (topk_packed_a(c, K)) {
        const void *pl = nullptr;
        bool wide_ok = false;
        CAPDEC_TRY(planes_of(c, Bt, N, K, cache, &pl, PK_F16X2, &wide_ok));
        ProfScope ps(c, F_NEAREST, flops);
        if (topk_wide_tile(c, wide_ok || b_small, M))
            CAPDEC_TRY(launch_gemm_h2w_topk(c->stream, A, pl, M, N, K, k, 1.0f, o));
        else
            CAPDEC_TRY(launch_gemm_f16x2p_topk(c->stream, A, pl, M, N, K, k, 1.0f, o, PK_F16X2));
    } else if (c->gemm_mode != GEMM_F32 && K % 64 == 0) {
        const void *pl = nullptr;
        CAPDEC_TRY(planes_of(c, Bt, N, K, cache, &pl, PK_BF16X3));
        ProfScope ps(c, F_NEAREST, flops);
        CAPDEC_TRY(launch_gemm_bf16x3_topk(c->stream, (const float *)A, K, pl, M, N, K, k, 1.0f, o));
    } else {
        ProfScope ps(c, F_NEAREST, flops);
        CAPDEC_TRY(launch_gemm_f32_topk(c->stream, (const float *)A, K, Bt, K, M, N, K, k, 1.0f, o));
    }
    ProfScope ps(c, F_SELECT);
    return launch_topk_merge(c->stream, o.tile_max, o.tile_sum, o.cand_val, o.cand_idx, M, gemm_tiles_n(N), k, lse, top_val,
                             top_idx);
}

}  // namespace capdec

using namespace capdec;

extern "C" {

int capdec_gemm_f32(capdec_ctx *c, const float *a, int lda, const float *bt, int ldb, float *cc, int ldc, int M, int N,
                    int K, const float *bias, const float *resid, int ldr, int act) {
    CAPDEC_CHECK(c && a && bt && cc, "gemm: null argument");
    CAPDEC_HIP(hipSetDevice(c->device));
    const bool cache = c->tune.hook_cache;   // benchmarking: treat Bt as a resident weight
    const bool packa = c->tune.hook_packa;   // tests / benchmarking: pre-packed A (the LayerNorm -> GEMM path)
    if ((packa || mode_single(c)) && c->gemm_mode != GEMM_F32 && lda == K && ldb == K && K % 64 == 0) {
        const int fmt = pack_fmt(c);
        const void *pa = nullptr, *pb = nullptr;
        if (cache) {
            CAPDEC_TRY(planes_of(c, a, M, K, true, &pa));
        } else {   // tests: always re-pack A (the plane cache is keyed by address, torch recycles addresses)
            CAPDEC_TRY(c->xpk.ensure(x3_packed_bytes_host(M, K)));
            CAPDEC_TRY(pack_any(c, a, M, K, fmt, c->xpk.p));
            pa = c->xpk.p;
        }
        GemmEpilogue e;
        e.bias = bias; e.act = act; e.resid = resid; e.ldr = ldr;
        CAPDEC_TRY(planes_of(c, bt, N, K, cache, &pb, -1, &e.wide_ok));
        // (an uncached B keeps the two-accumulator kernels: measuring max |b| costs a reduction and a stream synchronisation
        //  per call -- paid only when a geometry is FORCED, CAPDEC_H2W >= 2: how the parity tests reach the wide tiles)
        if (!cache && fmt == PK_F16X2 && c->tune.h2w >= 2) CAPDEC_TRY(weight_wide_ok(c, bt, (size_t)N * K, &e.wide_ok));
        // (the hook leaves the planner's geometries on in the batch-invariant mode.  Split-K of the one-plane kernels: under
        //  CAPDEC_HOOK_PACKA the decision of gemm_packed -- CAPDEC_X1_SPLITK -- so that the tests reach their split kernel;
        //  without the flag, the tools/ micro-benchmarks, never)
        const bool split = !mode_single(c) || (packa && c->tune.x1_splitk);
        return launch_packed(c, fmt, pa, pb, cc, ldc, M, N, K, e, split, /*invariant=*/false, 2.0 * M * (double)N * K);
    }
    return gemm(c, a, lda, bt, ldb, cc, ldc, M, N, K, bias, act, resid, ldr, /*weight=*/cache);
}

// test hook onto gemm_tn, the weight-gradient product of the train step, as it stands: no routing of its own
int capdec_gemm_tn_f32(capdec_ctx *c, const float *xa, int lda, const float *xb, int ldb, int rows, int n1, int n2, float *cc,
                       int ldc) {
    CAPDEC_CHECK(c && xa && xb && cc, "gemm_tn: null argument");
    CAPDEC_CHECK(rows > 0 && n1 > 0 && n2 > 0 && lda >= n1 && ldb >= n2 && ldc >= n2, "gemm_tn: bad shape or row stride");
    CAPDEC_HIP(hipSetDevice(c->device));
    return gemm_tn(c, xa, lda, xb, ldb, rows, n1, n2, cc, ldc);
}

}  // extern "C"
