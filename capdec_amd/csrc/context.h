// Internal declarations shared by the translation units behind the C ABI (include/capdec.h): the context, the weight
// containers, the per-family profiler and the host-side pieces each unit exports to the others.
//   capi_context.hip  context lifetime, streams, modes, memory, timers, profiler, decode statistics, the environment knobs
//   weights.hip       capdec_load_* (uploads; Conv1D transposes; BatchNorm folding)
//   gemm_dispatch.hip the GEMM planner: operand planes cache, which kernel / split for a projection and for the fused
//                     lm_head, capdec_gemm_f32
//   decode.hip        the pre-LN block stack, fused lm_head + selection, the one KV-cached step loop (decode_steps; its poll
//                     schedule: decode_sched.h) and what every decode entry point starts with, the greedy / beam / sampling
//                     drivers on them (the sampling kernel itself: sample.hip; the logits processors' kernels: process.hip)
//   guided.hip        capdec_decode_guided: classifier-free guidance, a driver on decode.hip's loop and greedy / beam state
//                     with partner rows (its combine, mirror and partner-map kernels)
//   contrastive.hip   capdec_decode_contrastive: contrastive search, a driver on decode.hip's loop (its selection kernels)
//   score.hip         capdec_score: teacher-forced log-probabilities of given captions (chunk planning, its three kernels)
//   nearest.hip       capdec_nearest_tokens: nearest table rows by cosine similarity (the normalised-wte cache, row blocks)
//   gap_stats.hip     capdec_embed_moments, capdec_group_distances: modality offset and paraphrase spread, fp64 sums
//   clipscore.hip     capdec_clip_score: CLIPScore / RefCLIPScore of candidate captions and their order per image, fp64 sums
//   memory.hip        capdec_memory_*: image embeddings projected onto a support memory of text embeddings (one fused pass)
//   bridger.hip       capdec_bridger_*: the supervised modality bridger (an MLP trained with MSE and SGD with momentum), fp32
//   mapper.hip        the prefix stage and the three mapping networks; the one TransformerLayer forward they and the train
//                     forward share (tlayer_self_front / tlayer_tail)
//   train_*.hip       the train step (train.h): step, mapping networks, shared backward pieces, optimizer + C entry points
//   clip.hip          CLIP ViT-B/32 towers, the ModifiedResNet tower, image preprocessing
//   comm.hip          caption-shard bounds and the RCCL all-gather (librccl dlopen'ed)
#pragma once
#include <rccl/rccl.h>      // types only: the library is dlopen'ed (no link-time dependency on RCCL)

#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <utility>

#include "bf16x3.h"
#include "common.h"
#include "config.h"

namespace capdec {

// ---------------------------------------------------------------------------- device buffers
struct DBuf {   // grow-only device buffer
    void *p = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes) {
        if (bytes <= cap) return 0;
        if (p) CAPDEC_HIP(hipFree(p));
        p = nullptr;
        cap = 0;
        CAPDEC_HIP(hipMalloc(&p, bytes));
        cap = bytes;
        return 0;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    template <class T> T *as() const { return reinterpret_cast<T *>(p); }
};

struct Gpt2Layer {
    float *ln1w, *ln1b, *wqkv, *bqkv, *wproj, *bproj, *ln2w, *ln2b, *wfc, *bfc, *wproj2, *bproj2;
};
struct Gpt2 {
    bool loaded = false;
    int n_layer = 0, n_head = 0, d = 0, vocab = 0, n_pos = 0;
    float eps = 1e-5f;
    float *wte = nullptr, *wpe = nullptr, *lnfw = nullptr, *lnfb = nullptr;
    std::vector<Gpt2Layer> layers;
    std::vector<void *> owned;
};
// One TransformerLayer of the reference (transformer_mapper.py:54-73) at width w: its twelve tensors in checkpoint order
// (TLayerSlot, train.h).  wq is to_queries [w, w], wkv to_keys_values [2w, ref]; both are always valid.
struct TMapLayer {
    float *n1w, *n1b, *wq, *wkv, *wproj, *bproj, *n2w, *n2b, *wfc1, *bfc1, *wfc2, *bfc2;
    // true: TransformerMapper and ref_encoder layers, whose queries, keys and values all read norm1(x): wkv == wq + w * w, so
    // wq is also the fused [3w, w] projection [q | k | v].  false: prefix_decoder layers -- wkv is a matrix of the layer's
    // own (odd = self, keys / values from x itself) or this layer's rows of Mapper::wkv_cross (even = cross)
    bool fused = false;
};
struct Mapper {
    int kind = 0;   // 0 none, 1 mlp, 2 transformer, 3 transformer encoder-decoder (trained only after capdec_train_set_encdec)
    int D = 0, P = 0, d = 768;
    // mlp
    int hidden = 0;
    float *w1 = nullptr, *b1 = nullptr, *w2 = nullptr, *b2 = nullptr;
    // transformer
    int clip_len = 0, n_layers = 0, heads = 8, mlp_hidden = 0;
    float *lin_w = nullptr, *lin_b = nullptr, *prefix_const = nullptr;
    std::vector<TMapLayer> layers;
    // encoder-decoder: `layers` is the ref_encoder (n_layers at width enc_dim, hidden enc_hidden), `dec` the prefix_decoder
    // (2 * n_layers at width d, hidden mlp_hidden; even = cross, odd = self); lin_w is [clip_len * enc_dim, D]
    int enc_dim = 0, enc_hidden = 0;
    std::vector<TMapLayer> dec;
    float *wkv_cross = nullptr;     // [n_layers * 2d, enc_dim]: the cross layers' to_keys_values stacked (one GEMM serves all)
    std::vector<void *> owned;
};

// CLIP tower = the same pre-LN block stack as GPT-2 (fused qkv, 4w MLP) with QuickGELU
struct Tower {
    bool loaded = false;
    int n_layer = 0, n_head = 0, d = 0, embed = 0;
    std::vector<Gpt2Layer> layers;
    std::vector<void *> owned;
    // text
    int ctx = 0, vocab = 0;
    float *tok_emb = nullptr, *pos_emb = nullptr, *lnf_w = nullptr, *lnf_b = nullptr, *proj_t = nullptr;  // proj_t [embed, d]
    // vision
    int image = 0, patch = 0, ntok = 0;
    float *conv_w = nullptr, *cls = nullptr, *ln_pre_w = nullptr, *ln_pre_b = nullptr;
};

// CLIP ModifiedResNet: a convolution with its BatchNorm folded in, as a GEMM operand
struct ConvW {
    float *w = nullptr;      // [cout_p, K]: K = k*k*cin_p in (ky, kx, c) order (first stem conv: 27 real columns, padded to 64)
    float *b = nullptr;      // [cout_p]
    int cin = 0, cout = 0, k = 0, cin_p = 0, cout_p = 0, K = 0;
};
struct ResNet {
    bool loaded = false;
    int image = 0, width = 0, embed = 0, feat = 0, heads = 0, sp = 0;
    int layers[4] = {0, 0, 0, 0};
    ConvW stem[3];
    std::vector<ConvW> blocks;          // 4 per bottleneck (conv1, conv2, conv3, downsample; downsample.w may be null)
    float *pos = nullptr, *wq = nullptr, *bq = nullptr, *wk = nullptr, *bk = nullptr, *wv = nullptr, *bv = nullptr,
          *wc = nullptr, *bc = nullptr;
    std::vector<void *> owned;
};

// The supervised modality bridger (bridger.hip): L Linear layers in nn.Linear layout with ReLU between them, the momentum
// buffers of torch.optim.SGD, the activations the last train step saved, and the loss scalars.
constexpr int BRIDGER_MAX_LAYERS = 16, BRIDGER_MAX_WIDTH = 1024, BRIDGER_MAX_BATCH = 64;
struct BridgerScalars { float last; int pad; double sum; long long steps; double eval_sum; long long eval_batches; };
struct Bridger {
    bool loaded = false;
    int L = 0, dims[BRIDGER_MAX_LAYERS + 1] = {0};
    float *w[BRIDGER_MAX_LAYERS] = {nullptr}, *b[BRIDGER_MAX_LAYERS] = {nullptr};       // W_l [dims[l+1], dims[l]], b_l [dims[l+1]]
    float *vw[BRIDGER_MAX_LAYERS] = {nullptr}, *vb[BRIDGER_MAX_LAYERS] = {nullptr};     // their momentum buffers (0 at load)
    float *act[BRIDGER_MAX_LAYERS] = {nullptr};      // [BRIDGER_MAX_BATCH, dims[l+1]]: post-activation of the last train step
    float *dy[2] = {nullptr, nullptr};               // [BRIDGER_MAX_BATCH, widest]: the gradient flowing down, two in turn
    BridgerScalars *scal = nullptr;                  // device
    int last_batch = 0;                              // rows of the last train step (0: none since the load)
    std::vector<void *> owned;
};

enum Family { F_GEMM = 0, F_LMHEAD, F_ATTN_DEC, F_ATTN_PRE, F_LN, F_EMBED, F_SELECT, F_MAP_ATTN, F_OTHER, F_GEMM_X3,
              F_LMHEAD_X3, F_GEMM_X3P, F_GEMM_BF16P, F_LMHEAD_BF16, F_GEMM_H2P, F_LMHEAD_H2, F_PACK, F_LMHEAD_2ND, F_NEAREST, F_CONTRAST, F_GUIDED, F_COUNT };
extern const char *const kFamilyNames[F_COUNT];
constexpr int PROF_SLOTS = 24;   // capdec_profile_get fills at most this many families (engine.py sizes its arrays by it)
static_assert(F_COUNT <= PROF_SLOTS, "profile arrays too small");
enum GemmMode { GEMM_F32 = 0, GEMM_BF16X3 = 1, GEMM_BF16 = 2, GEMM_F16X2 = 3, GEMM_F16 = 4 };

struct Prof {
    bool on = false;
    int every = 1;                       // time every `every`-th launch of each family (1 = all)
    int64_t calls[PROF_SLOTS] = {0};     // launches seen per family (timed or not)
    struct Rec { int fam; hipEvent_t a, b; double flops; };
    std::vector<Rec> recs;
    std::vector<hipEvent_t> pool;
    double ms[F_COUNT] = {0}, flops[F_COUNT] = {0};
    int64_t launches[F_COUNT] = {0};
};

}  // namespace capdec

using namespace capdec;

namespace capdec { struct TrainState; }      // train.h: saved activations, gradients, AdamW moments of the train step
struct capdec_ctx {
    capdec::Tuning tune;            // the environment knobs, parsed once by capdec_create (config.h)
    int device = 0;
    hipStream_t own_stream = nullptr, stream = nullptr;
    size_t kv_budget = (size_t)192 << 30;
    Gpt2 gpt;
    Mapper map;
    Tower clip_text, clip_vision;
    ResNet clip_resnet;
    DBuf r_a, r_b, r_c, r_d, r_e, r_f, r_col;      // ResNet activation buffers (NHWC) + im2col
    DBuf r_pk1, r_pk2, r_xpk, r_ypk, r_xi, r_idp, r_zero;   // ... packed activations (GEMM / implicit-conv operands), zero rows
    Prof prof;
    int gemm_mode = GEMM_F16X2;
    struct Planes { void *p; size_t n; int fmt; bool wide_ok; };   // wide_ok: max |w| < 16 (see GemmEpilogue::wide_ok)
    std::map<std::pair<const void *, int>, Planes> planes;   // (fp32 weight, PackFmt) -> packed planes: a weight used in two
                                                             // formats (train forward f16x2, decode in a one-plane mode) keeps both
    DBuf x3_tmp, xpk, apk, fpk, a_tmp;   // scratch planes for un-cached matrices; packed LayerNorm output; packed fp32-A
    int stat_steps = 0, stat_compactions = 0;      // last decode call: steps run, compactions done,
    int stat_chunks = 0;                           // ... and the chunks its captions were split into (capdec_decode_chunks)
    long long stat_row_steps = 0;                  // activation rows pushed through the GPT-2 body (prefill excluded)
    std::vector<int> stat_step_rows;               // ... per decode step (capdec_decode_step_rows)
    bool batch_invariant = false;   // capdec_set_batch_invariant: no launch-size dependent summation order (no split-K, pinned kernel variants)
    int diverge = 0;                // measurement: beams never share history (capdec_set_debug_diverge)
    double stat_kv_slots = 0.0, stat_kv_pos = 0.0;   // last beam decode: sums behind capdec_decode_counters (filled lazily)
    bool k3_off = false;                             // this decode call went back to k candidates per tile (poll_alive)
    long long k3_rows = 0;                           // rows of this call's lm_head launches that kept 3 per tile
    bool lmflag_live = false;                        // `lmflag` holds the second-pass row count of the last decode call
    int kvstat_n = 0;                                // captions of the last beam decode whose counters sit in `kvstat`
    bool compact = true;       // decode: drop finished captions from the batch at the poll points (CAPDEC_COMPACT=0: off)
    bool pack_chain = true;    // ... and attention / the fc GEMM epilogue emit the packed A operand of the GEMM that follows
    bool pack_a = true;        // bf16x3 mode: LayerNorm emits the packed A operand, GEMM moves both operands by LDS-DMA
    hipEvent_t t0 = nullptr, t1 = nullptr;
    // workspaces
    DBuf h, x, qkv, att, ff, xl, tmax, tsum, cval, cidx, lse, topv, topi, kc, vc;
    DBuf tokens, scores, seq, stopped, done, anc, next_tok, alive, gids, glens, cmap, kvstat;
    DBuf glogp;            // diverse beam search (capdec_decode_beam_groups): the unpenalised log-prob sums [rows] (BeamState::logp)
    DBuf cstate;           // constrained beam search (capdec_decode_beam_constrained): a slot's (met, cur, pos) [rows] (ConstraintState::state)
    DBuf cs_hist, cs_last, cs_sel;   // contrastive search (contrastive.hip): the L2-normalised ln_f history [captions, ctx, d],
                                     // the chosen candidate's residual row by caption and by compact activation row [captions, d]
    capdec::TrainState *train = nullptr;     // created by the first capdec_train_step, freed by train_release
    int train_scope = 0;                     // capdec_train_set_scope: survives capdec_train_reset and weight reloads
    int train_encdec = 0;                    // capdec_train_set_encdec: the encoder-decoder mapper trains (off: it is refused); survives like the scope
    float train_drop_p = 0.f;                // capdec_train_set_dropout: GPT-2's dropout probability in scope 1 (0 = off)
    unsigned long long train_drop_seed = 0;  // ... key of the Philox keep-mask stream (counter = element, train step)
    DBuf slogits;          // sampling decode, logits processors: fp32 logits of one row block, [min(rows, tune.sample_rows), ld]
                           // (decode.hip: lm_head_rows; the guided decode keeps a block's partner rows behind it: guided.hip)
    DBuf s_plan, s_rows, s_logit, s_bad;   // capdec_score (score.hip): the call's plan [lens | row offsets | h rows | targets], a
                                           // chunk's scored rows of h [R, d], their label logits [R], first tainted position [nc]
    int stat_score_chunks = 0;             // chunks of the last capdec_score call (capdec_score_chunks)
    DBuf wte_n;                            // capdec_nearest_tokens (nearest.hip): the loaded wte with every row L2-normalised, fp32
    bool wte_n_valid = false;              // [vocab, d] -- built on first use, its operand planes cached by planes_of like a weight's;
                                           // dropped with the wte it was made from (drop_wte_norm)
    DBuf n_tab, n_bad;                     // ... a caller's table normalised for one call; [table flag | one flag per row of a block]
    capdec::Bridger bridger;               // bridger.hip: at most one supervised modality bridger
    DBuf br_f0, br_f1, br_ev;              // ... capdec_bridger_forward / _eval: activations of n rows, two in turn; a loss per batch
    DBuf gap_ws, gap_ws2, gap_off;         // gap_stats.hip: fp64 partial sums per slab and their folds; [flag | group offsets]
    DBuf clipscore_off;                    // clipscore.hip: [candidate offsets | reference offsets] of the call
    DBuf mem_n;                            // memory.hip: the support memory, every row L2-normalised, fp32 [rows up to MEM_MTILE, d up
    int mem_rows = 0, mem_d = 0;           // to 128], zero padded (mem_rows == 0: none loaded) -- one per context
    DBuf mem_q, mem_part, mem_bad;         // ... a row block's normalised queries, its per-chunk partials, [flag | one flag per row]
    capdec::LogitsProc proc;               // capdec_set_logits_processors (defaults: every processor off)
    int proc_bias_n = 0;                   // capdec_set_logit_bias: entries of `pbias` (0 = no bias)
    DBuf pbias, pcorr;     // the logit bias [vocab]; a row block's logp shift under top_k (decode.hip: lm_head_rows)
    DBuf lmflag, xpk2;     // fused lm_head with 3 candidates per tile: [count, total, rows...] of the rows whose top 5 need
                           // the exact second pass; their compacted packed A operand (decode.hip: lm_head_select)
    DBuf lmsp;             // sparse lm_head: a step's SparseLm bookkeeping (common.h)
    DBuf m_hid, m_lin, m_seq, m_x, m_qkv, m_att, m_ff;
    DBuf m_kvc;            // encoder-decoder mapper: keys / values of the cross layers, [n * clip_len, n_layers * 2d]
    DBuf t_idx, t_patch, t_pout, p_desc, p_inter, splitk, absmax;
    int *alive_host = nullptr;   // pinned: [captions still generating, second-pass rows so far]
    // caption-shard communicator (RCCL), see capdec_comm_init
    ncclComm_t comm = nullptr;
    int comm_rank = 0, comm_world = 1;
    DBuf g_pad, g_all;
};


namespace capdec {

// ---- capi_context.hip
// ---------------------------------------------------------------------------- profiling
inline hipEvent_t prof_event(capdec_ctx *c) {
    if (!c->prof.pool.empty()) {
        hipEvent_t e = c->prof.pool.back();
        c->prof.pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}
struct ProfScope {
    capdec_ctx *c;
    int idx = -1;
    ProfScope(capdec_ctx *ctx, int fam, double flops = 0.0) : c(ctx) {
        if (!c->prof.on) return;
        if (c->prof.calls[fam]++ % c->prof.every != 0) return;
        Prof::Rec r{fam, prof_event(c), prof_event(c), flops};
        (void)hipEventRecord(r.a, c->stream);
        c->prof.recs.push_back(r);
        idx = (int)c->prof.recs.size() - 1;
    }
    ~ProfScope() {
        if (idx >= 0) (void)hipEventRecord(c->prof.recs[idx].b, c->stream);
    }
};
int prof_collect(capdec_ctx *c);

// ---- train_optim.hip (the train step: train.h)
void train_release(capdec_ctx *c);      // frees the train-step state (a mapper / GPT-2 reload invalidates it)

// ---- comm.hip
void comm_release(capdec_ctx *c);       // destroys the context's communicator, if any

inline int pad64(int c) { return (c + 63) / 64 * 64; }

// ---- weights.hip
int upload(std::vector<void *> &owned, const float *h_src, size_t n, float **out);
int upload_transposed(capdec_ctx *c, std::vector<void *> &owned, const float *h_src, int rows, int cols, float **out);
void free_all(std::vector<void *> &owned);

// ---- gemm_dispatch.hip: the planner
void drop_planes(capdec_ctx *c);
void drop_planes_of(capdec_ctx *c, const void *weight);      // one cached weight (its values changed: train_optim.hip)
int pack_fmt(const capdec_ctx *c);
inline bool mode_single(const capdec_ctx *c) { return c->gemm_mode == GEMM_BF16 || c->gemm_mode == GEMM_F16; }
int pack_any(capdec_ctx *c, const float *W, int N, int K, int fmt, void *out);
int planes_of(capdec_ctx *c, const float *W, int N, int K, bool cache, const void **out, int fmt_override = -1,
              bool *wide_ok = nullptr);
// profiler family of a packed-operand GEMM in format fmt (PK_*: bf16x3.h)
int gemm_family(int fmt);
// C = epilogue(A . Bt^T) on the native fp32 MFMA kernel (the f32 mode, other K; the train step under CAPDEC_TRAIN_F16X2=0)
int gemm_native(capdec_ctx *c, const float *A, int lda, const float *Bt, int ldb, float *C, int ldc, int M, int N, int K,
                GemmEpilogue e = GemmEpilogue());
// C = act(A . Bt^T + bias) + resid with fp32 A in HBM (mapper, patch embedding, projections)
int gemm(capdec_ctx *c, const float *A, int lda, const float *Bt, int ldb, float *C, int ldc, int M, int N, int K,
         const float *bias, int act, const float *resid = nullptr, int ldr = 0, bool weight = true);
// C [N1, N2] = Xa^T Xb (fp32 Xa [rows, N1] / Xb [rows, N2], row strides lda / ldb): weight-gradient products, operands packed transposed
int gemm_tn(capdec_ctx *c, const float *Xa, int lda, const float *Xb, int ldb, int rows, int N1, int N2, float *C, int ldc);
bool use_packed_a(capdec_ctx *c, int K);
struct NextLn { const float *w, *b; float eps; int *done; };
int gemm_packed(capdec_ctx *c, const void *Apk, const float *W, float *C, int ldc, int M, int N, int K, const float *bias,
                int act, const float *resid = nullptr, int ldr = 0, void *packed_out = nullptr,
                const NextLn *next_ln = nullptr, const void *resid_packed = nullptr,
                const QkvScatter *qkv_scatter = nullptr);
int ln_gemm_packed(capdec_ctx *c, const float *h, int ldh, const float *lnw, const float *lnb, float eps, const float *W,
                   float *C, int ldc, int M, int N, int K, const float *bias, int act, void *packed_out = nullptr,
                   bool ln_ready = false, const QkvScatter *qkv_scatter = nullptr);

// The workspace of a fused top-k launch over `rows` rows, `ntiles` column tiles and k candidates per tile: the per-tile
// lists (c->tmax / tsum / cval / cidx) -> *o, and c->lse [rows].  (c->topv / c->topi belong to the caller: not every one
// of them merges into these.)
int topk_workspace(capdec_ctx *c, int rows, int ntiles, int k, TopkOut *o);
// The fused lm_head: LayerNorm of the M rows of h, then LN(h) . W^T (W [N, K]) fused with the per-(row, 128-column tile)
// top-k of the logits * inv_temp into o.  k3_ok: a k = 5 selection may keep three candidates per tile where the kernel
// allows it (the wide two-plane tile; the one-plane kernel from 2048 rows); *k3 reports whether it did -- the rows the
// merge then flags need gemm_topk_dev.  The packed modes leave LN(h) in c->xpk.
int ln_gemm_topk(capdec_ctx *c, const float *h, int ldh, const float *lnw, const float *lnb, float eps, const float *W,
                 int M, int N, int K, int k, float inv_temp, const TopkOut &o, bool k3_ok, bool *k3, bool no_cand = false);
// (no_cand: max and sum exp per (row, tile) only, no candidates -- the sparse route of lm_head_select; it asks first whether
//  a launch of M rows takes the wide two-plane tile, the only kernel with that form: lm_head_wide_tile)
int lm_head_wide_tile(capdec_ctx *c, const float *W, int M, int N, int K, bool *wide);
// ... the sparse route's grouped pass (gemm_h2w.hip: gemm_h2w_topk_grouped_kernel) over the pairs of s, rows read from Apk
int gemm_topk_grouped(capdec_ctx *c, const void *Apk, const float *W, const SparseLm &s, int blocks_cap, int N, int K,
                      float inv_temp, float *cand_val, int *cand_idx);
// ... its exact second pass: k = 5 lists for the *m_dev rows of the packed operand Apk (in the format of the mode)
int gemm_topk_dev(capdec_ctx *c, const void *Apk, const float *W, const int *m_dev, int N, int K, float inv_temp,
                  const TopkOut &o);
// The fused top-k GEMM WITHOUT a LayerNorm in front, fp32-accurate in every mode as gemm() is: the k best columns of every
// row of A . Bt^T (Bt fp32 [N, K]) -> top_val / top_idx [M, k] (descending, equal values in ascending column order) and
// lse [M]; o: the per-tile lists in between.  A is what topk_packed_a(c, K) says: the packed PK_F16X2 operand (modes f16x2,
// bf16, f16 with K % 64 == 0 -> the two-fp16-plane kernels, the 256 x 128 tile from 2048 rows) or fp32 rows of stride K
// (mode bf16x3 with K % 64 == 0 -> its own top-k kernel; otherwise the native fp32 one).  b_small: every |Bt| < 16 is known
// (GemmEpilogue::wide_ok without measuring it).  cache: Bt is a resident matrix whose operand planes may be kept.  Never
// the three-candidate shortcut of ln_gemm_topk; the 128-row tile alone in the batch-invariant mode.
bool topk_packed_a(const capdec_ctx *c, int K);
int gemm_topk(capdec_ctx *c, const void *A, const float *Bt, bool cache, bool b_small, int M, int N, int K, int k,
              const TopkOut &o, float *lse, float *top_val, int *top_idx);

// ---- mapper.hip: the TransformerLayer forward, x -> out on M rows of width w (hidden hid):
//     a1 = norm1(x); qkv = a1 . [q | k | v]^T                                       tlayer_self_front (fused layers)
//     att = attention(...)                                                          the caller's launch: it is what differs
//     mid = x + project(att); a2 = norm2(mid); ff = relu(fc1(a2)); out = mid + fc2(ff)      tlayer_tail (every layer)
// The buffers may alias (inference: x = mid = out, a1 = a2) or be kept per layer (the train forward saves all of them).
// weight: the GEMMs may cache the weights' operand planes (false in the train forward: the weights change every step).
struct TLayerBufs { const float *x; float *a1, *qkv; const float *att; float *mid, *a2, *ff, *out; };
int tlayer_self_front(capdec_ctx *c, const TMapLayer &w, const TLayerBufs &b, int M, int wd, bool weight);
int tlayer_tail(capdec_ctx *c, const TMapLayer &w, const TLayerBufs &b, int M, int wd, int hid, bool weight);

// ---- decode.hip: the block stack (GPT-2 and the CLIP towers run on it)
struct StepShape {
    bool prefill;
    int ncap, P, beam;      // prefill: rows = ncap * P
    int rows, L;            // decode: rows at context length L
    const uint8_t *anc;
    int anc_stride;
    const int *cmap;        // decode after compaction: activation row r -> caption cmap[r / beam] (nullptr: identity)
};
struct StackCfg {
    const std::vector<Gpt2Layer> *layers;
    int n_layer, d;
    float eps;
    int act;
    bool causal, keep_kv;
};
int ensure_body_ws(capdec_ctx *c, int M, int d);
int stack_body(capdec_ctx *c, const StackCfg &g, const StepShape &s, const KvCache &kv);
void kv_geometry(KvCache &kv, int rows, int ctx, int heads, int hd);
// ... the pieces of the decode loop that capdec_score (score.hip) runs as they are: GPT-2's blocks on c->h; ln_f over R rows
// of h (row stride ldh) + the fused lm_head -> c->lse [R], c->topv / c->topi [R, k]; the KV cache of `rows` sequences
int gpt2_body(capdec_ctx *c, const StepShape &s, const KvCache &kv);
int lm_head_select(capdec_ctx *c, const float *h0, int ldh, int R, int k, float inv_temp);
int ensure_kv(capdec_ctx *c, KvCache &kv, int rows, int ctx, int heads = 0, int hd = 0, int layers = 0);
// The constants of one decode call; the extern "C" entry points fill it, chunk_call offsets the pointers per chunk.
struct DecodeCall {
    int P = 0, beam = 1;
    bool greedy = true;         // the greedy family (arg-max, teacher-forced, sampling): beam == 1
    int stop_id = -1, alt_stop_id = -1, T = 0;
    float temperature = 1.0f;
    int *ids = nullptr, *lens = nullptr;        // [n, beam, T], [n, beam]
    float *scores = nullptr;    // [n, beam] (beam)
    int *order = nullptr;       // [n, beam] or nullptr (beam)
    const int *forced = nullptr;    // [n, T] teacher forcing: fed instead of the arg-max (greedy)
    float *stats = nullptr;     // [n, T, 3] or nullptr (teacher forcing)
    // the sampling decode (capdec_decode_sample): the greedy loop with the arg-max replaced by a draw.  The Philox counter
    // is (cap_off + caption, step) and nothing else, so a caption's draws do not depend on the chunking, on the compaction or
    // on the rest of the batch.
    bool sample = false;
    float top_p = 0.f;
    uint64_t seed = 0;
    const float *u = nullptr;   // [n, T] or nullptr (Philox)
    float *logp = nullptr;      // [n, T] or nullptr
    // diverse beam search (capdec_decode_beam_groups): groups > 0 sends the beam bookkeeping to diverse.hip's group kernels
    int groups = 0;
    float diversity = 0.f;
    float *glogp = nullptr;     // [n, beam] or nullptr: the unpenalised log-prob sums, in the returned order
    // constrained beam search (capdec_decode_beam_constrained): `phrases` sends every step through the materialised logits and
    // constrained.hip's selection and bookkeeping kernels
    const int *phrases = nullptr;   // [n, 4, 4]
    int *met = nullptr;         // [n, beam] or nullptr: the met masks, in the returned order
    int cap_off = 0;            // index of the chunk's first caption within the call: the Philox counter's caption offset, and
                                // the offset of the chunk's slice of the per-call K/V-slot statistic (BeamState::kv_stat)
};
// ... and what the drivers of decode.hip, guided.hip and contrastive.hip are built from (decode.hip).  An entry point:
// decode_call_checks (in the groups its own checks sit between), decode_call_begin (the per-call reset, the captions per
// chunk), then per chunk its driver on chunk_call's constants.
enum { CK_LOADED = 1, CK_SIZES = 2, CK_CONTEXT = 4, CK_HEAD_DIM = 8, CK_BIAS = 16 };
int decode_call_checks(capdec_ctx *c, const char *who, int which, int n, int P, int T, long long ctx);
int decode_call_begin(capdec_ctx *c, int n, int steps0, int kvstat_caps, int rows_per_caption, int ctx, size_t extra_per_cap,
                      int lm_rows_per_cap, int *chunk);
DecodeCall chunk_call(const DecodeCall &call, int c0);
int chunk_captions(capdec_ctx *c, int n, int beam, int ctx, size_t extra_per_cap = 0);
// A driver: the prefill and its selection, then decode_steps -- the one step loop: alive-count polls, compaction, statistics
// -- with the body of a step plugged in, then the finalisation.
struct StepLoop {
    int nc, first, T;           // captions of the chunk; steps first .. T - 1 (first: 1, or 0 where the prefill selects nothing)
    int rows_per_caption;       // activation rows per caption: beam, 2 * beam (guided), top_k (contrastive)
    const uint8_t *done;        // [nc] the captions' done flags
    int map_slots;              // caption slots of the compaction map: nc, or 2 nc where partners are listed behind
};
using AfterCompact = std::function<int(int *cmap, int na)>;
using StepFn = std::function<int(int i, int na, const int *cmap)>;
int decode_steps(capdec_ctx *c, const StepLoop &l, const AfterCompact &after_compact, const StepFn &step);
int poll_alive(capdec_ctx *c, int *alive);
// ... the KV cache and the greedy or the beam state of a chunk (halves = 2: with the guided decode's partner rows), and the
// step kernel that advances it
struct DecodeState {
    KvCache kv;
    BeamState bs;
    GreedyState gs;
    const int *hist = nullptr;      // the rows' own histories, for the logits processors: ids (greedy) or bs.tokens
    uint8_t *anc = nullptr;         // bs.anc (nullptr: greedy)
    ConstraintState cs;             // constrained beam search: the chunk's phrases and the slots' states
};
int decode_state(capdec_ctx *c, int nc, const DecodeCall &a, int halves, DecodeState *s);
int decode_advance(capdec_ctx *c, const DecodeCall &a, const DecodeState &s, int R, int step, int k, const int *cmap);
int gpt2_step(capdec_ctx *c, const KvCache &kv, int rows, int beam, int L, const uint8_t *anc, const int *cmap);
// ... whether the call runs the logits processors; the lm_head route through materialised logits (hn, gamma: the guided
// decode's partner rows and scale; its combine kernel: guided.hip); ln_f over R rows of h (row stride ldh) + the plain
// lm_head GEMM -> logits [R, ld]
bool processors_on(const capdec_ctx *c, bool sampling);
int lm_head_rows(capdec_ctx *c, const float *h0, int ldh, int R, int k, float inv_temp, const DecodeCall &a,
                 const GreedyState &gs, bool proc, int step, int beam, const int *hist, const float *hn = nullptr,
                 float gamma = 0.f);
int lm_head_logits(capdec_ctx *c, const float *h0, int ldh, int R, float *logits, int ld);

// ---- guided.hip
int launch_guided_combine(hipStream_t st, float *cond, const float *neg, int ld, int rows, int V, float gamma);

// ---- memory.hip
void memory_release(capdec_ctx *c);     // frees the support memory (capdec_memory_free, capdec_destroy)

// ---- nearest.hip
void drop_wte_norm(capdec_ctx *c);      // the normalised copy of wte and its planes (wte was reloaded or updated)

}  // namespace capdec
