/*
 * capdec.h -- C ABI of libcapdec_hip.so: the MI355X (gfx950) caption hot path of CapDec.
 *
 *   CLIP embedding -> (normalise / noise) -> mapping network -> GPT-2 KV-cached decode
 *   (greedy | beam) -> token ids
 *
 * The reference (DavidHuji/CapDec) is pure Python: its "plugin API" for this path is a set
 * of Python names, not an FFI.  Each entry point below cites the reference interface it
 * replaces (file:line under the reference tree); capdec_amd/ (ctypes) binds exactly these
 * symbols and re-exposes the reference names (MappingType, MLP, TransformerMapper,
 * ClipCaptionModel, generate2, generate_beam, noise_injection).  INTEGRATION.md shows the
 * stub a reference maintainer would add.
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on failure; capdec_last_error() returns
 *     a thread-local message for the last failure on the calling thread.
 *   - one capdec_ctx per GPU / rank, driven by one host thread at a time.
 *   - "h_" pointers are host memory (read during the call), "d_" pointers are device memory
 *     on the context's GPU; bulk data (embeddings in, token ids out) stays on the device.
 *   - all work is enqueued on the context's HIP stream (own stream, or one adopted with
 *     capdec_set_stream); decode calls synchronise that stream before returning.
 *   - tensors are dense row-major fp32 / int32 unless stated.
 */
#ifndef CAPDEC_H
#define CAPDEC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CAPDEC_ABI_VERSION 6   /* 6: capdec_load_mapper_encdec (MappingType.TransformerDecoder; inference only until
                                     capdec_train_set_encdec, added without a new number, turns its training on);
                                     (capdec_decode_sample was added WITHOUT a new number: the addition changes no existing
                                     symbol, and a library built from older sources is refused through capdec_build_id)
                                  5: capdec_set_compact, capdec_decode_step_rows (the workload in which captions stop);
                                  4: train step -- GPT-2's dropouts (capdec_train_set_dropout / _masks), capdec_train_loss, loss == NULL
                                     enqueues without waiting, the scope survives capdec_train_reset;
                                  3: the diverged-beam debug hook left the shipped library (measurement builds only);
                                  2: capdec_profile_get takes the array capacity in *count; batch-invariant mode; decode counters */

typedef struct capdec_ctx capdec_ctx;

/* activation codes for capdec_gemm_f32 (test hook) */
enum { CAPDEC_ACT_NONE = 0, CAPDEC_ACT_TANH = 1, CAPDEC_ACT_RELU = 2, CAPDEC_ACT_GELU_NEW = 3,
       CAPDEC_ACT_QUICK_GELU = 4,
       CAPDEC_ACT_RESID_RELU = 5 /* relu(acc + bias + resid): the tail of a ResNet bottleneck */ };

/* ---- context ------------------------------------------------------------------------ */
int capdec_abi_version(void);
/* hash of the sources this library was compiled from (capdec_amd/build.py:source_hash); the Python host refuses a
 * library whose id differs from the source tree next to it (a stale .so would silently run old kernels) */
const char *capdec_build_id(void);
const char *capdec_last_error(void);
/* replaces `device = CUDA(0); model = model.to(device)` (reference predictions_runner.py:154-155) */
int capdec_create(int device_id, capdec_ctx **out);
void capdec_destroy(capdec_ctx *ctx);
/* enqueue on an external hipStream_t (e.g. torch's current stream).  NULL is a valid handle:
 * HIP's default (null) stream.  capdec_use_own_stream() goes back to the context's private
 * non-blocking stream (the default after capdec_create). */
int capdec_set_stream(capdec_ctx *ctx, void *hip_stream);
int capdec_use_own_stream(capdec_ctx *ctx);
int capdec_synchronize(capdec_ctx *ctx);
/* how the dense projections (GPT-2 / CLIP block stacks, lm_head) run:
 * 3 = "f16x2" (DEFAULT): fp32-accurate -- every fp32 operand is two fp16 planes (a = hi + 2^-11 lo), THREE
 *     v_mfma_f32_32x32x16_f16 per product, fp32 accumulate; error below the rounding noise of an fp32 GEMM, every
 *     parity test (token ids bit-identical to the fp32 reference) passes; GEMM inputs are clamped to +-65504;
 * 1 = "bf16x3": fp32-accurate, three bf16 planes, six v_mfma_f32_32x32x16_bf16 per product (round-1 scheme, A/B);
 * 0 = native fp32 MFMA (v_mfma_f32_32x32x2_f32, exact fma chain);
 * 2 = "bf16" (BASELINE configs[1]): weights and GEMM-input activations rounded to bf16 (RNE) and a bf16 KV cache, ONE
 *     MFMA per product, fp32 accumulate; residual stream, LayerNorm and softmax stay fp32.  Not bit-comparable with
 *     the fp32 reference (teacher-forced tolerance tests, capdec_decode_greedy_forced);
 * 4 = "f16": fp16 GEMM operands, fp32 everything else (KV cache included): the precision class of the reference's
 *     CLIP towers on a GPU (clip.load converts to fp16).
 * In the two 16-bit modes the CLIP towers' attention (every tower sequence up to 128 positions -- the 77-token text tower,
 * the 50-token ViT: the prefill rule `tower || P >= 24` sends them to the fp16 matrix-core kernel) also takes fp16 operands
 * for its two products -- q, k, v and the un-normalised softmax weights, fp32 accumulate, fp32 softmax; GPT-2's attention
 * keeps fp32 operands (bf16 mode: the bf16-rounded K / V of its cache).
 * The mapper, patch-embedding and projection GEMMs are fp32-accurate in every mode.
 * The environment variable CAPDEC_GEMM_MODE=f16x2|bf16x3|f32|bf16|f16 overrides the default at capdec_create (any
 * other value makes capdec_create fail: a typo must not silently select another precision). */
enum { CAPDEC_GEMM_F32 = 0, CAPDEC_GEMM_BF16X3 = 1, CAPDEC_GEMM_BF16 = 2, CAPDEC_GEMM_F16X2 = 3, CAPDEC_GEMM_F16 = 4 };
int capdec_set_gemm_mode(capdec_ctx *ctx, int mode);
int capdec_get_gemm_mode(capdec_ctx *ctx);
/* Batch-invariant mode (default off; CAPDEC_BATCH_INVARIANT=1 sets it at capdec_create).  By default a few kernels
 * pick a variant from the size of the launch -- split-K for under-filled GEMM grids (the K slices are summed in another
 * order than the unsplit loop), the block-tile geometry of a GEMM (one or two accumulator sets), the fused lm_head's
 * tile height, the number of positions the decode attention keeps in flight -- so the fp32 ROUND-OFF
 * of a row depends on how many other rows share its launch: a caption decoded alone, in a 625-caption shard or in a
 * 5000-caption batch can differ in the last bit of a logit, and on a numerical near-tie in a token.  With this mode on,
 * every row goes through the same summation order whatever the batch (unsplit 128x128 GEMMs, pinned kernel variants):
 * results are bit-identical across batch sizes, chunkings and multi-GPU shardings, at the price of under-filled grids
 * for small batches (and they may differ in the last bit from the default mode's). */
int capdec_set_batch_invariant(capdec_ctx *ctx, int on);
/* cap on bytes the decode KV cache may take (captions are processed in chunks that fit);
 * 0 = default (192 GiB of the 288 GB HBM3E) */
int capdec_set_kv_budget(capdec_ctx *ctx, size_t bytes);

/* raw device memory for hosts that do not bring their own allocator (torch is optional) */
int capdec_malloc(capdec_ctx *ctx, size_t bytes, void **d_ptr);
int capdec_free(capdec_ctx *ctx, void *d_ptr);
int capdec_memcpy_h2d(capdec_ctx *ctx, void *d_dst, const void *h_src, size_t bytes);
int capdec_memcpy_d2h(capdec_ctx *ctx, void *h_dst, const void *d_src, size_t bytes);

/* ---- weights -------------------------------------------------------------------------
 * replaces `model.load_state_dict(torch.load(ckpt))` (reference predictions_runner.py:461);
 * layouts are the checkpoint's own: GPT-2 Conv1D matrices [in, out], nn.Linear [out, in]. */
typedef struct capdec_gpt2_layer {
    const float *ln_1_w, *ln_1_b;            /* [d] */
    const float *c_attn_w, *c_attn_b;        /* [d, 3d], [3d] */
    const float *c_proj_w, *c_proj_b;        /* [d, d], [d] */
    const float *ln_2_w, *ln_2_b;            /* [d] */
    const float *c_fc_w, *c_fc_b;            /* [d, 4d], [4d] */
    const float *mlp_c_proj_w, *mlp_c_proj_b;/* [4d, d], [d] */
} capdec_gpt2_layer;

typedef struct capdec_gpt2_weights {
    int n_layer, n_head, n_embd, vocab, n_pos;
    float ln_eps;
    const float *wte;                        /* [vocab, d]  (lm_head is tied to it) */
    const float *wpe;                        /* [n_pos, d] */
    const capdec_gpt2_layer *layers;         /* [n_layer] */
    const float *ln_f_w, *ln_f_b;            /* [d] */
} capdec_gpt2_weights;

/* transformers.GPT2LMHeadModel as owned by ClipCaptionModel.gpt (reference gpt2_prefix.py:162) */
int capdec_load_gpt2(capdec_ctx *ctx, const capdec_gpt2_weights *h_w);

/* MLP mapper: reference gpt2_prefix.py:114-126, sizes (D, d*P/2, d*P) at :167-168 */
int capdec_load_mapper_mlp(capdec_ctx *ctx, int prefix_dim, int prefix_length, int hidden,
                           const float *h_w1, const float *h_b1,   /* [hidden, D], [hidden] */
                           const float *h_w2, const float *h_b2);  /* [d*P, hidden], [d*P] */

typedef struct capdec_tmapper_layer {
    const float *norm1_w, *norm1_b;          /* [d] */
    const float *to_queries_w;               /* [d, d]   (no bias) */
    const float *to_keys_values_w;           /* [2d, d]  (no bias) */
    const float *project_w, *project_b;      /* [d, d], [d] */
    const float *norm2_w, *norm2_b;          /* [d] */
    const float *fc1_w, *fc1_b;              /* [hid, d], [hid] */
    const float *fc2_w, *fc2_b;              /* [d, hid], [d] */
} capdec_tmapper_layer;

typedef struct capdec_tmapper_weights {
    int prefix_dim, prefix_length, clip_length, num_layers, num_heads, d, mlp_hidden;
    const float *linear_w, *linear_b;        /* [clip_length*d, D], [clip_length*d] */
    const float *prefix_const;               /* [P, d] */
    const capdec_tmapper_layer *layers;      /* [num_layers] */
} capdec_tmapper_weights;

/* TransformerMapper: reference transformer_mapper.py:113-127 (8 heads, pre-LN, ReLU MLP) */
int capdec_load_mapper_transformer(capdec_ctx *ctx, const capdec_tmapper_weights *h_w);

typedef struct capdec_edmapper_weights capdec_edmapper_weights;
struct capdec_edmapper_weights {
    int prefix_dim, prefix_length, clip_length, num_layers, num_heads, d;
    int enc_dim;                             /* width of the encoder: 512 in the reference, whatever prefix_dim and d are */
    int enc_mlp_hidden, dec_mlp_hidden;      /* 2 * enc_dim, 2 * d in the reference */
    const float *linear_w, *linear_b;        /* [clip_length*enc_dim, D], [clip_length*enc_dim] */
    const float *prefix_const;               /* [P, d] */
    const capdec_tmapper_layer *enc_layers;  /* [num_layers]: the layer of capdec_tmapper_weights at d = enc_dim, hid = enc_mlp_hidden */
    const capdec_tmapper_layer *dec_layers;  /* [2*num_layers] at d, hid = dec_mlp_hidden; to_keys_values_w is [2d, enc_dim] in the
                                                even layers (cross: keys from the encoder's output) and [2d, d] in the odd
                                                ones (self: keys from the residual stream, which norm1 does NOT touch) */
};

/* TransformerEncoderDecoder: reference transformer_mapper.py:130-145 (MappingType.TransformerDecoder).  Inference only by
 * default: capdec_mapper_forward and everything built on it serve it; capdec_train_step refuses it until
 * capdec_train_set_encdec(ctx, 1) asks for its training. */
int capdec_load_mapper_encdec(capdec_ctx *ctx, const capdec_edmapper_weights *h_w);

/* ---- prefix stage -------------------------------------------------------------------- */
/* `prefix / prefix.norm(2,-1)` then `+ offset` (reference predictions_runner.py:221-224);
 * d_offset [D] may be NULL; normalize=0 mirrors --dont_normalize_prefix.  In place if out==x. */
int capdec_normalize_prefix(capdec_ctx *ctx, const float *d_x, int n, int dim, int normalize,
                            const float *d_offset, float *d_out);

/* noise_injection (reference train.py:27-39): variance==0 -> copy of x (NOT normalised).
 * d_noise [n,dim]: unit-variance draw standing for torch.randn (NULL -> on-device Philox
 * stream seeded by `seed`).  uniform!=0 -> get_uniform_ball_noise (train.py:18-24) using
 * d_noise as the Gaussian direction and d_u [n] as the torch.rand draw (NULL -> Philox). */
int capdec_noise_inject(capdec_ctx *ctx, const float *d_x, int n, int dim, float variance,
                        const float *d_offset, int uniform, int dont_norm, uint64_t seed,
                        const float *d_noise, const float *d_u, float *d_out);

/* `model.clip_project(prefix)` (reference predictions_runner.py:228; gpt2_prefix.py:145-147):
 * d_x [n, D] -> d_out [n, P, d] with whichever mapper is loaded. */
int capdec_mapper_forward(capdec_ctx *ctx, const float *d_x, int n, float *d_out);

/* ---- CLIP ViT-B/32 towers --------------------------------------------------------------
 * replaces `clip.load("ViT-B/32", device, jit=False)` + `encode_text` / `encode_image`
 * (reference embeddings_generator.py:49,86,89; predictions_runner.py:161,218,220).  Pointers are
 * the tensors of an OpenAI CLIP state dict, in its own layouts (nn.Linear / in_proj [out,in];
 * text_projection / visual.proj [width, embed_dim]).  head_dim must be 64 (ViT-B/32: 512/8, 768/12). */
typedef struct capdec_clip_block {
    const float *ln_1_w, *ln_1_b;            /* [w] */
    const float *in_proj_w, *in_proj_b;      /* [3w, w], [3w] */
    const float *out_proj_w, *out_proj_b;    /* [w, w], [w] */
    const float *ln_2_w, *ln_2_b;            /* [w] */
    const float *c_fc_w, *c_fc_b;            /* [4w, w], [4w] */
    const float *c_proj_w, *c_proj_b;        /* [w, 4w], [w] */
} capdec_clip_block;

typedef struct capdec_clip_text_weights {
    int context_length, vocab, width, heads, layers, embed_dim;
    const float *token_embedding;            /* [vocab, w] */
    const float *positional_embedding;       /* [context_length, w] */
    const capdec_clip_block *blocks;         /* [layers] */
    const float *ln_final_w, *ln_final_b;    /* [w] */
    const float *text_projection;            /* [w, embed_dim] */
} capdec_clip_text_weights;

typedef struct capdec_clip_vision_weights {
    int image_size, patch, width, heads, layers, embed_dim;
    const float *conv1_w;                    /* [w, 3, patch, patch] (no bias) */
    const float *class_embedding;            /* [w] */
    const float *positional_embedding;       /* [(image_size/patch)^2 + 1, w] */
    const float *ln_pre_w, *ln_pre_b;        /* [w] */
    const capdec_clip_block *blocks;         /* [layers] */
    const float *ln_post_w, *ln_post_b;      /* [w] */
    const float *proj;                       /* [w, embed_dim] */
} capdec_clip_vision_weights;

int capdec_load_clip_text(capdec_ctx *ctx, const capdec_clip_text_weights *h_w);
int capdec_load_clip_vision(capdec_ctx *ctx, const capdec_clip_vision_weights *h_w);

/* CLIP ModifiedResNet visual tower (`clip.load("RN50x4")`: the reference's DEFAULT image backbone,
 * predictions_runner.py:158,220; embeddings_generator.py:89,113; train.py:445).  One entry per convolution with the
 * BatchNorm that follows it (inference statistics; folded into the convolution at load time).  Host fp32 pointers in
 * the OpenAI state-dict layouts: w [cout, cin, k, k] (k = 1, or 3 with padding 1), bn_* [cout]. */
typedef struct capdec_conv_bn {
    const float *w, *bn_w, *bn_b, *bn_mean, *bn_var;   /* w == NULL: this convolution does not exist (no downsample) */
    int cin, cout, k;
} capdec_conv_bn;
typedef struct capdec_clip_resnet_weights {
    int image_size;        /* 288 for RN50x4 */
    int width;             /* 80 for RN50x4: stage planes width * {1,2,4,8}, attention-pool input 32 * width channels */
    int embed_dim;         /* 640 */
    int layers[4];         /* bottleneck blocks per stage: {4, 6, 10, 6} */
    const capdec_conv_bn *stem;     /* [3]: visual.conv1/bn1 (stride 2), conv2/bn2, conv3/bn3; then AvgPool2d(2) */
    const capdec_conv_bn *blocks;   /* [4 * sum(layers)]: per bottleneck conv1/bn1, conv2/bn2, conv3/bn3, downsample.0/.1;
                                       the first block of stages 2..4 has stride 2 (AvgPool2d(2) after conv2 and in front
                                       of the downsample convolution) */
    const float *positional_embedding;                 /* visual.attnpool.positional_embedding [(S/32)^2 + 1, 32 width] */
    const float *q_w, *q_b, *k_w, *k_b, *v_w, *v_b;    /* attnpool.{q,k,v}_proj: [32w, 32w], [32w] */
    const float *c_w, *c_b;                            /* attnpool.c_proj: [embed_dim, 32w], [embed_dim] */
} capdec_clip_resnet_weights;
/* after this call capdec_clip_encode_image takes [n, 3, image_size, image_size] pixels through the ResNet tower
 * (a ViT tower loaded earlier is replaced, and vice versa).
 * Arithmetic: in the f16x2 / f16 / bf16 modes every activation between the pixels and the attention pool -- the residual
 * stream included -- exists only as a packed GEMM operand of the mode (f16x2: two fp16 planes, 22 significand bits,
 * |x| <= 65504; f16 / bf16: one 16-bit plane, what the reference's fp16 GPU model does), 3x3 convolutions are implicit
 * GEMMs over it; the bf16x3 / f32 modes keep fp32 activations (im2col + GEMM).  Limits: width even with 32 * width a
 * multiple of 64, image_size a multiple of 32 with at most 256 attention-pool tokens (image_size <= 480). */
int capdec_load_clip_resnet(capdec_ctx *ctx, const capdec_clip_resnet_weights *h_weights);
/* `clip_model.encode_text(clip.tokenize(caption))`: d_tokens int32 [n, context_length] (SOT ... EOT,
 * zero padded; the EOT row is found as argmax of the ids) -> d_out [n, embed_dim], NOT normalised */
int capdec_clip_encode_text(capdec_ctx *ctx, const int32_t *d_tokens, int n, float *d_out);
/* `clip_model.encode_image(preprocess(image))`: d_pixels fp32 [n, 3, S, S] already resized /
 * normalised -> d_out [n, embed_dim], NOT normalised */
int capdec_clip_encode_image(capdec_ctx *ctx, const float *d_pixels, int n, float *d_out);

/* ---- GPT-2 --------------------------------------------------------------------------- */
/* `model.gpt(inputs_embeds=x).logits` (reference gpt2_prefix_eval.py:76-77,163-164).
 * d_embeds [n, L, d].  all_positions!=0 -> d_logits [n, L, vocab] (what the reference
 * materialises); 0 -> d_logits [n, vocab], last position only (what it uses). */
int capdec_gpt2_logits(capdec_ctx *ctx, const float *d_embeds, int n, int L, int all_positions,
                       float *d_logits);
/* ---- the train step (reference train.py:344-354) ------------------------------------------------------------------
 * One iteration: d_prefix [batch, D] is the embedding batch AFTER noise_injection (train.py:347; capdec_noise_inject),
 * d_tokens [batch, length] int32 right-padded with 0 as train.ClipCocoDataset pads (:52-63; under the causal mask the
 * padding mask of :348 changes nothing a real position sees).  Computes logits[:, P-1:-1], the loss of :349
 * (cross_entropy with ignore_index = 0: padding AND real tokens with id 0 are skipped; mean over the rest), its gradient
 * with respect to every tensor of the scope (:350), and -- with apply_update != 0 -- one update of transformers-4.24
 * AdamW (:351; betas / eps / weight_decay as passed: the reference's AdamW(params, lr) means 0.9, 0.999, 1e-6, 0.0; bias
 * correction on; `lr` is the scheduler's current value, :352) on the device-resident weights, which the inference entry
 * points then use.  loss != NULL: *loss (host) receives the loss and the call waits for the device; loss == NULL: the
 * call only enqueues (capdec_train_loss reads the loss, and the running sum, later).  An id outside [0, vocab) -- an
 * IndexError in the reference -- makes the loss NaN and leaves every weight and the optimizer untouched.
 * The optimizer state lives in the context; loading a mapper or GPT-2 again, or capdec_train_reset, drops it (the scope
 * and the dropout setting stay).
 *
 * Scope (capdec_train_set_scope): 0 (default) = the mapper, GPT-2 frozen and in eval mode (--only_prefix:
 * ClipCaptionPrefix, train.py:279-287; a deterministic step); 1 = GPT-2 as well -- the reference's DEFAULT run
 * (train.py:326: AdamW(model.parameters()) of a ClipCaptionModel).  Changing the scope starts a fresh optimizer.
 *
 * capdec_train_get copies a tensor of the scope (kind 0) or its gradient from the last step (kind 1, = what
 * loss.backward() leaves in .grad) to d_out (device).  MLP mapper: which = 0 model.0.weight [hidden, D], 1 model.0.bias,
 * 2 model.2.weight [P * d, hidden], 3 model.2.bias.  TransformerMapper: linear.weight, linear.bias, prefix_const, then per
 * layer norm1.weight, norm1.bias, attn.to_queries.weight, attn.to_keys_values.weight, attn.project.weight, .bias,
 * norm2.weight, .bias, mlp.fc1.weight, .bias, mlp.fc2.weight, .bias.  Scope 1 continues with wte (the tied lm_head), wpe,
 * per layer ln_1.weight, ln_1.bias, attn.c_attn.weight, .bias, attn.c_proj.weight, .bias, ln_2.weight, .bias,
 * mlp.c_fc.weight, .bias, mlp.c_proj.weight, .bias, then ln_f.weight, ln_f.bias; Conv1D weights (and their gradients)
 * are returned in the checkpoint's [in, out] layout.
 *
 * The encoder-decoder mapper (capdec_load_mapper_encdec) trains only after capdec_train_set_encdec(ctx, 1): a context
 * setting like the scope -- off at capdec_create, kept by capdec_train_reset and by mapper loads, without effect on the
 * other two mappers.  While off, capdec_train_step and capdec_train_get refuse that mapper ("... is inference-only").  Its
 * 3 + 36 num_layers tensors come in the key order of the reference module's state_dict(): prefix_const; per ref_encoder
 * layer the twelve tensors listed above (at width enc_dim); per prefix_decoder layer (2 num_layers of them) the same twelve,
 * attn.to_keys_values.weight being [2d, enc_dim] in the even (cross) layers and [2d, d] in the odd (self) ones; then
 * linear.weight, linear.bias.  Its attention backward keeps one head's tiles in LDS and has no fallback: with Sq queries
 * and Sk keys of heads hd wide it needs Sq, Sk <= 128 and
 *     (2 max(Sq, Sk) (hd + 1) + 2 Sq (Sk + 1) + 16 (2 hd + Sk)) * 4 <= 153600 bytes
 * for the encoder (clip_length x clip_length, hd = enc_dim / heads = 64), the cross layers (prefix_length x clip_length,
 * hd = 96) and the self layers (prefix_length x prefix_length, hd = 96: at most 90 x 90); a geometry beyond that is refused
 * before the first launch and the context goes on working.  d must be 768 and enc_dim 512. */
int capdec_train_set_encdec(capdec_ctx *ctx, int on);
int capdec_train_step(capdec_ctx *ctx, const float *d_prefix, const int32_t *d_tokens, int batch, int length, float lr,
                      float beta1, float beta2, float eps, float weight_decay, int apply_update, float *loss);
int capdec_train_get(capdec_ctx *ctx, int kind, int which, float *d_out, size_t n);
int capdec_train_reset(capdec_ctx *ctx);
int capdec_train_set_scope(capdec_ctx *ctx, int train_gpt);
/* The loss of the last train step (*last), the sum of the losses and the number of steps since the last reset (the
 * `accumulated_loss` of train.py:356 without a device round trip per step); reset != 0 clears sum and count.  Waits for
 * the device.  Any pointer may be NULL. */
int capdec_train_loss(capdec_ctx *ctx, float *last, double *sum, long long *steps, int reset);
/* GPT-2's dropouts in scope 1 (GPT2Model in train() mode, train.py:321: `drop` after inputs_embeds + position_embeds;
 * per block attn_dropout on the softmax weights, resid_dropout after attn.c_proj, the MLP's dropout after mlp.c_proj;
 * transformers' default embd_pdrop = attn_pdrop = resid_pdrop = 0.1).  p = 0 (default) computes the step of a model whose
 * GPT2Config has them at 0.  Keep-masks come from a Philox4x32-10 stream keyed by `seed` (counter: element group, number
 * of mask streams drawn since the last capdec_train_reset / capdec_train_set_dropout), survivors scaled by 1 / (1 - p)
 * like torch.  Scope 0 never applies dropout (GPT-2 stays in eval mode there).
 * capdec_train_set_dropout_masks injects the keep-masks of the NEXT train step (consumed once; parity tests): one byte per
 * element, 1 = keep, every site of the step concatenated in call order -- embd [B, S, d], then per block attn
 * [B, heads, S, S], resid [B, S, d], mlp [B, S, d], with S = prefix_length + length; n must equal that total.
 * capdec_train_get_dropout_masks copies the mask stream the last step used (same layout) to d_out. */
int capdec_train_set_dropout(capdec_ctx *ctx, float p, uint64_t seed);
int capdec_train_set_dropout_masks(capdec_ctx *ctx, const uint8_t *d_masks, size_t n);
int capdec_train_get_dropout_masks(capdec_ctx *ctx, uint8_t *d_out, size_t n);

/* The loss of the train step's forward (reference train.py:349 `nnf.cross_entropy(logits, tokens, ignore_index=0)`,
 * and GPT2LMHeadModel's shifted `labels=` loss used by gpt2_prefix.py:154): mean over the rows whose label differs
 * from ignore_index of logsumexp(d_logits[row, 0..vocab)) - d_logits[row, label].  d_logits: device fp32 [rows, ld],
 * d_labels: device int32 [rows], d_loss: device fp32 [1] (NaN when no row counts, like torch).  A label outside
 * [0, vocab) other than ignore_index -- an error in torch -- makes the loss NaN instead of being skipped silently. */
int capdec_cross_entropy(capdec_ctx *ctx, const float *d_logits, int ld, const int32_t *d_labels, int rows, int vocab,
                         int ignore_index, float *d_loss);
/* `model.gpt.transformer.wte(ids)` (reference gpt2_prefix_eval.py:105,181): d_out [n, d] */
int capdec_wte_lookup(capdec_ctx *ctx, const int32_t *d_ids, int n, float *d_out);

/* ---- decode -------------------------------------------------------------------------- */
/* generate2, batched (reference gpt2_prefix_eval.py:118-198; top-p filter + argmax == argmax).
 * d_prefix [n, P, d] -> d_ids [n, entry_length] (zero padded), d_lens [n] = number of tokens
 * INCLUDING the stop token.  A row stops at stop_id or alt_stop_id (764 in the reference,
 * :187; pass -1 to disable). */
int capdec_decode_greedy(capdec_ctx *ctx, const float *d_prefix, int n, int P, int stop_id,
                         int alt_stop_id, int entry_length, int32_t *d_ids, int32_t *d_lens);

/* Teacher-forced greedy decode (evaluation / test hook of the reduced-precision modes, where free-running sequences
 * of two bf16 pipelines diverge by construction): the token fed at step i is d_forced[r, i] (int32 [n, entry_length],
 * e.g. the ids an fp32 run produced) instead of the arg-max; d_ids [n, entry_length] receives the arg-max of every
 * step, d_stats (may be NULL) fp32 [n, entry_length, 3] = (top-1 logit, top-2 logit, logsumexp over the vocabulary) of
 * every step.  Same kernels and KV cache as capdec_decode_greedy; nothing stops early. */
int capdec_decode_greedy_forced(capdec_ctx *ctx, const float *d_prefix, int n, int P, int entry_length,
                                const int32_t *d_forced, int32_t *d_ids, float *d_stats);

/* Limits of the decode entry points (the reference has none, gpt2_prefix_eval.py:50-51,118-129; each is checked and
 * reported through capdec_last_error): beam size 1..8; head_dim = 64 (GPT-2 / CLIP ViT-B/32); context prefix_length +
 * entry_length - 1 <= n_positions (<= 1024, GPT-2's own limit; beyond ~400 positions the attention's per-block tables need
 * most of a CU's LDS and run at lower occupancy); n_embd a multiple of 32, <= 1024.  In the default
 * f16x2 GEMM mode GEMM inputs are clamped to +-65504 (fp16's range; LayerNorm / attention / GELU outputs and weights
 * are orders of magnitude below it). */

/* generate_beam, batched (reference gpt2_prefix_eval.py:50-115).  d_prefix [n, P, d] ->
 * d_ids [n, beam, entry_length], d_lens [n, beam] (= int(seq_lengths)), d_scores [n, beam]
 * (= scores / seq_lengths, :110).  Beams are sorted by score descending (:113-114), so
 * d_ids[i][0] is what `generate_beam(...)[0]` decodes (predictions_runner.py:230).
 * d_order [n, beam] (may be NULL) receives the reference's internal beam index of each row. */
int capdec_decode_beam(capdec_ctx *ctx, const float *d_prefix, int n, int P, int beam, int stop_id,
                       int entry_length, float temperature, int32_t *d_ids, int32_t *d_lens,
                       float *d_scores, int32_t *d_order);
/* Diverse (group) beam search (Vijayakumar et al. 2016; `num_beam_groups` / `diversity_penalty` of older transformers)
 * on the beam decode: beam B in 1..8, G groups (1 <= G <= B, B % G == 0, Bg = B / G), diversity_penalty lambda >= 0
 * (finite).  Beam slots g*Bg .. (g+1)*Bg-1 of a caption form group g.  Each group runs capdec_decode_beam's step over its
 * own Bg rows only: its own Bg x vocab candidates, its own top Bg, sources from its own slots.  Within a step the groups of
 * a caption are processed in order 0..G-1:
 *   lp      = the log-softmax of the processed, temperature-scaled logits, exactly as in capdec_decode_beam;
 *   lp_pen  = lp - lambda * (float)cnt[j] for token j of a row of group g that is not stopped, where cnt[j] is the number of
 *             hypotheses that groups < g of the same caption selected AT THIS STEP with token j, counting only selections
 *             whose source beam was not stopped; a stopped row keeps its single candidate (token 0, log-prob 0), which is
 *             neither penalised nor counted;
 *   key     = (scores[row] + lp_pen) / seq_new[row], fp32 in that operation order; the group's Bg winners by the tie rule
 *             of capdec_decode_beam (larger key, then smaller flat index = caption-level slot * vocab + token);
 *   scores[slot] = key * seq_new[src]: the scores accumulate the PENALISED values, as the classic algorithm does;
 *   logp[slot]   = logp[src] + (stopped[src] ? 0 : lp): a second accumulator with the UNPENALISED sum.
 * Step 0 has one logits row per caption: group g takes the best Bg tokens of lp - lambda * cnt, cnt holding what groups
 * < g took at this step (with lambda = 0 all groups start identical).  tokens, seq, stopped, logp and the ancestor table
 * follow the winners' permutation (sources are caption-level slots); a caption is done when every slot of every group is
 * stopped; the end is capdec_decode_beam's: d_scores = scores / seq sorted descending over all B slots, d_order [n, beam]
 * (may be NULL) the slot of each returned row, so a row's group is d_order / Bg; d_logp [n, beam] (may be NULL) the
 * unpenalised sums in the returned order.  groups == 1 is capdec_decode_beam bit for bit, whatever the penalty.  The
 * selection stays exact with `beam` candidates per row (the logits are still not materialised when no processor is set):
 * at most B - Bg tokens are penalised for a group, so a row's unpenalised top-B list holds at least Bg unpenalised
 * tokens, each >= every token outside the list.  Logits processors compose unchanged (they act before the selection; a
 * row's history is its slot's tokens).  capdec_set_debug_diverge is not honoured here.  Errors (capdec_last_error):
 * groups < 1, groups > beam, beam % groups != 0, a negative, infinite or NaN penalty. */
int capdec_decode_beam_groups(capdec_ctx *ctx, const float *d_prefix, int n, int P,
                              int beam, int groups, float diversity_penalty,
                              int stop_id, int entry_length, float temperature,
                              int32_t *d_ids, int32_t *d_lens, float *d_scores,
                              int32_t *d_order,
                              float *d_logp /* [n, beam] or NULL */);
/* Lexically constrained beam search (Anderson et al. 2017) by dynamic beam allocation (Post & Vilar 2018; `force_words_ids`
 * of transformers.generate) on the beam decode: capdec_decode_beam's inputs plus, per caption, phrases that must occur in
 * it.  d_phrases is int32 [n, 4, 4]: caption r has up to 4 phrases of 1..4 token ids each; unused places hold -1; a phrase
 * is the leading non-negative run of its row, a caption's phrases are its leading non-empty rows.  EVERY phrase of a caption
 * must occur in the caption as a contiguous token run (conjunctive constraints).
 * Hypothesis state, following each beam slot through every permutation next to tokens, seq, scores and stopped:
 *   met  bitmask of the phrases fully matched;  cur  the phrase in progress, or none;  pos  tokens of cur already matched,
 *   1..len-1.
 * Transition adv(state, t):
 *   1. if cur is set and phrase[cur][pos] == t: pos += 1; when pos == len, the bit of cur is set in met and cur, pos are
 *      cleared.  Nothing else happens to the state in this case.
 *   2. otherwise cur and pos are cleared -- the progress is lost, there is no back-tracking inside a phrase (as in
 *      transformers' PhrasalConstraint) -- and
 *   3. with c the lowest-index unmet phrase with phrase[c][0] == t, if there is one: len == 1 sets its bit, otherwise
 *      cur = c, pos = 1.
 * bank(state) = sum of len over the met phrases + pos.  The special tokens S(state) are the next token of cur, if any, and
 * the first token of every unmet phrase: at most 5.  Every token outside S leads to the same state (met, none, 0).
 * Per step, for a live row, in this order: the logits processors that are set (steps 1-4 of
 * capdec_set_logits_processors); if the row's met is not complete, l[stop_id] <- -inf (a caption cannot end before its
 * phrases are in it); the division by the temperature; lp = log_softmax.  A stopped row keeps its single candidate (token
 * 0, log-prob 0, state unchanged), as in capdec_decode_beam.  key = (scores[row] + lp) / seq_new[row], fp32 in that
 * operation order: the plain beam's key.
 * Selection per caption: every candidate (row, token) with a finite key belongs to bank bank(adv(state_row, token)).  The
 * non-empty banks are taken in descending order and passed over repeatedly from the highest to the lowest; each visit takes
 * the bank's best remaining candidate (larger key, then smaller flat index = slot * vocab + token); the passes end when
 * `beam` candidates are taken; the slots are filled in the order taken.  Step 0 has one row per caption with the empty
 * state and is selected the same way.  scores[slot] = key * seq_new[src]; tokens, seq, stopped, the state and the ancestor
 * table follow the winners.  A caption is done when every slot is stopped.
 * End: the returned rows are sorted by the number of phrases fully met (descending), then scores / seq (descending), then
 * slot (ascending); d_ids, d_lens, d_scores, d_order as in capdec_decode_beam; d_met [n, beam] (may be NULL) receives each
 * returned row's met mask, so that a caller sees when entry_length ran out before the phrases were in.  With no phrases
 * there is one bank, nothing is banned, and the call is capdec_decode_beam on the same logits route bit for bit.
 * The call always materialises the logits (CAPDEC_SAMPLE_ROWS rows at a time, as the processors do): the special tokens'
 * logits come from the same arithmetic as the rest of the row.  A row's list -- S, then its best `beam` tokens outside S,
 * ties to the smaller column -- is enough for an exact selection: all tokens outside S land in one bank, of which at most
 * `beam` can be taken.  Logits processors and the bias compose (they act before the stop ban); capdec_set_compact,
 * capdec_set_kv_budget, capdec_set_batch_invariant and the GEMM mode are honoured; a caption's result does not depend on
 * the batch size, the chunking or the compaction.  Guidance and beam groups are separate entry points and do not take
 * constraints.  capdec_set_debug_diverge is not honoured here.  Refused before any launch (capdec_last_error): a token id
 * outside the vocabulary, a phrase that holds stop_id, a hole in front of a used place (a used place behind a -1 of its
 * phrase, a phrase behind an empty one), beam outside 1..8. */
int capdec_decode_beam_constrained(capdec_ctx *ctx, const float *d_prefix, const int32_t *d_phrases, int n, int P,
                                   int beam, int stop_id, int entry_length, float temperature,
                                   int32_t *d_ids, int32_t *d_lens, float *d_scores, int32_t *d_order,
                                   int32_t *d_met /* [n, beam] or NULL */);
/* Contrastive search (Su et al. 2022; `penalty_alpha` / `top_k` of transformers.generate): the one decode that reads the
 * model's hidden states.  top_k = K in 1..8, penalty_alpha = a in [0, 1] (finite), prefix_length + entry_length <=
 * min(1024, n_positions) -- one position more than capdec_decode_greedy, because every emitted token is chosen after its
 * own candidate pass.  hid(x) is the ln_f output of the last layer (the vector that multiplies wte; transformers'
 * hidden_states[-1] for GPT-2).  Per caption, with prefix [P, d] and T = entry_length:
 *   prefill  H = [hid of prefix positions 0..P-1], every row divided by max(its L2 norm, 1e-12); last = hid(position P-1);
 *   for t = 0..T-1, pos = P + t:
 *     lg = last . wte^T, with the logits processors that are set (repetition_penalty, no_repeat_ngram_size, min_length,
 *          logit_bias) applied with the caption's chosen ids as history, exactly as in capdec_decode_greedy (the processors'
 *          top_k is sampling-only and ignored; there is no temperature);
 *     candidates v_0..v_{K-1} = the K largest processed logits (larger value, then smaller token); p_c = softmax(lg)[v_c];
 *     every candidate is fed at pos (wte[v_c] + wpe[pos]) and attends to the chosen path's K/V: h_c = hid(...);
 *     sim_c = max over j < pos of cos(h_c, H_j) -- the prefix positions count as context;
 *     score_c = (1 - a) * p_c - a * sim_c in fp32; the winner w = argmax_c score_c, an exact tie going to the lower c;
 *     d_ids[t] = v_w, d_lens = t + 1; the normalised h_w is appended to H, the K/V candidate w wrote at pos becomes the
 *     path's, last = h_w; v_w == stop_id or alt_stop_id finishes the caption (the stop token is part of the output).
 * a = 0 or K = 1 gives capdec_decode_greedy's tokens.  d_ids [n, entry_length] zero padded, d_lens [n]; d_trace (may be
 * NULL) fp32 [n, entry_length, 2] = (p, sim) of the chosen candidate of every emitted token, zero elsewhere.  A caption's
 * result does not depend on chunking, compaction or the other captions (capdec_set_batch_invariant's caveat applies).  The
 * K candidates are K beam rows (row = caption * K + c) on the ancestor-table attention; the lm_head runs on one row per
 * caption; the per-caption history [P + T, d] fp32 counts against the KV budget.  Errors (capdec_last_error): top_k
 * outside 1..8, penalty_alpha outside [0, 1] or NaN, a context that is too long, head_dim other than 64. */
int capdec_decode_contrastive(capdec_ctx *ctx, const float *d_prefix, int n, int P, int top_k, float penalty_alpha,
                              int stop_id, int alt_stop_id, int entry_length,
                              int32_t *d_ids /* [n, T] */, int32_t *d_lens /* [n] */,
                              float *d_trace /* [n, T, 2] or NULL */);
/* Classifier-free guidance (`guidance_scale` of transformers.generate; Kornblith et al. 2023 for captioning) on the greedy
 * (beam == 1) and the beam (beam 2..8) decode.  For caption r: p_r = d_prefix[r] [P, d]; q_r = its negative prefix [P, d],
 * d_neg_prefix[r] (neg_n == n) or d_neg_prefix[0] for every caption (neg_n == 1).  A hypothesis of r after i emitted tokens
 * t_0..t_{i-1} has two contexts, (p_r, t_0..t_{i-1}) and (q_r, t_0..t_{i-1}): the same tokens, only the prefix differs.
 * With l and m the raw fp32 lm_head logits [V] of the two contexts and gamma = guidance_scale:
 *   c_j = l_j - logsumexp(l),  u_j = m_j - logsumexp(m),  g_j = gamma * c_j + (1 - gamma) * u_j
 * (fp32, every operation rounded on its own, in this form: equal rows give g = c up to rounding).  g takes the place of
 * the raw logits in everything that follows, in the existing order: the logits processors that are set (steps 1-4 of
 * capdec_set_logits_processors; the history is the hypothesis's own tokens), the division by the temperature, then the
 * call's rule -- the arg-max for beam == 1 (stop_id / alt_stop_id as in capdec_decode_greedy; the temperature cannot change
 * it), log_softmax and capdec_decode_beam's unchanged bookkeeping otherwise (alt_stop_id is ignored there).  Two consequences:
 *   1. the processors see log-probabilities (all <= 0), not raw logits, as in transformers: repetition_penalty always
 *      multiplies, so gamma -> 1+ with a repetition penalty is not continuous with gamma == 1;
 *   2. unlike transformers' beam search, the guided scores are renormalised (log_softmax of g / temperature) before they
 *      enter the beam sums -- what this library does after its processors anyway.
 * Both logsumexps and everything else per row have a fixed summation order and one workgroup owns one (cond, neg) row pair
 * whatever the launch holds: a caption's result does not depend on the batch size, the row blocks, the chunking or the
 * compaction (capdec_set_batch_invariant's caveat applies to the GEMMs); pad columns of the logits are never touched.
 * guidance_scale == 1 means off: the call IS capdec_decode_greedy / capdec_decode_beam (no negative rows, bit-identical
 * results).  Outputs have the shapes and the meaning of capdec_decode_greedy (beam == 1: d_ids [n, T], d_lens [n];
 * d_scores / d_order unused) and of capdec_decode_beam (d_ids [n, beam, T], d_lens, d_scores [n, beam], d_order [n, beam]
 * or NULL); limits as for those calls, the negative prefix has the same P.  The call honours the logits processors and
 * bias, capdec_set_compact, capdec_set_batch_invariant, capdec_set_kv_budget (a caption and its partner always share a
 * chunk and both count) and the GEMM mode; capdec_decode_stats / _step_rows count rows as launched: both halves.  Every
 * step materialises the logits of at most 2 * CAPDEC_SAMPLE_ROWS rows.  Errors (capdec_last_error, before any launch): a
 * guidance_scale that is NaN, infinite or < 1; neg_n other than 1 or n; beam outside 1..8; a context that is too long;
 * head_dim other than 64. */
int capdec_decode_guided(capdec_ctx *ctx, const float *d_prefix, const float *d_neg_prefix, int neg_n /* 1 or n */,
                         int n, int P, int beam /* 1 = greedy, 2..8 = beam */, float guidance_scale,
                         int stop_id, int alt_stop_id /* greedy only */, int entry_length, float temperature,
                         int32_t *d_ids, int32_t *d_lens, float *d_scores /* beam */,
                         int32_t *d_order /* beam, may be NULL */);
/* Nucleus-sampling decode: the greedy loop with the arg-max replaced by one draw per step.  For a row of logits l, with
 * s = l / (temperature > 0 ? temperature : 1) and p = softmax(s): token j is in the nucleus iff it is the arg-max or the
 * sum of p[i] over all p[i] > p[j] is <= top_p (the filter of reference gpt2_prefix_eval.py:166-175; exactly equal
 * probabilities are treated alike); q = p restricted to the nucleus and renormalised; the token is the first j in ascending
 * id order whose running sum of q exceeds the step's uniform (the last nucleus token if rounding leaves the total below it).
 * top_p <= 0 keeps the arg-max only (= capdec_decode_greedy), top_p >= 1 is plain multinomial sampling.
 * Uniforms: d_u [n, entry_length] in [0, 1) (the convention of capdec_noise_inject's d_noise / d_u), or, when d_u is NULL,
 * the device Philox4x32-10 keyed by (seed, caption index within the call, step) and nothing else: a caption's draws do
 * not depend on the KV budget's chunking, on finished-caption compaction or on the other captions of the batch.
 * d_ids / d_lens as for capdec_decode_greedy (rows stop at stop_id or alt_stop_id; zero padded; lens include the stop
 * token); d_logp (may be NULL) [n, entry_length]: log-probability of each chosen token under the unfiltered,
 * temperature-scaled distribution, 0 after the stop.  Limits and errors as for greedy; a NaN top_p or temperature is an
 * error.  Each step materialises the fp32 logits of at most CAPDEC_SAMPLE_ROWS rows (default 2048) at a time. */
int capdec_decode_sample(capdec_ctx *ctx, const float *d_prefix, int n, int P, int stop_id, int alt_stop_id,
                         int entry_length, float temperature, float top_p, uint64_t seed,
                         const float *d_u,      /* [n, entry_length] or NULL */
                         int32_t *d_ids,        /* [n, entry_length] */
                         int32_t *d_lens,       /* [n] */
                         float *d_logp);        /* [n, entry_length] or NULL */

/* ---- logits processors --------------------------------------------------------------- */
/* Context state, like capdec_set_compact: what the following capdec_decode_greedy / _beam / _sample calls apply to the
 * raw logits l[0..vocab) of every row at every step i, before the division by the temperature.  A row's history
 * g = (g_0 .. g_{i-1}) is what its own hypothesis has generated so far -- the caption's ids (greedy, sampling), that beam's
 * tokens after the previous step's re-ordering (beam); prefix rows and prompt tokens folded into the prefix are not
 * history.  In this order:
 *   1. repetition_penalty theta > 0 (1 = off): for every DISTINCT j in g, l[j] <- l[j] / theta if l[j] > 0 else
 *      l[j] * theta (a token that occurs twice is penalised once);
 *   2. the bias of capdec_set_logit_bias: l <- l + b (entries finite or -inf; -inf bans the token);
 *   3. no_repeat_ngram_size m (0 = off): if i >= m - 1, for every s with g[s .. s+m-2] == g[i-m+1 .. i-1]:
 *      l[g[s+m-1]] <- -inf (m = 1 bans every token of g);
 *   4. min_length (0 = off): if i < min_length, l[stop_id] <- -inf, and l[alt_stop_id] where the call has one;
 *   5. top_k (0 = off; capdec_decode_sample only): j stays iff fewer than top_k entries are strictly greater than l[j]
 *      (ties at the boundary stay), everything else becomes -inf.
 * Then s = l / temperature and the call's own rule runs unchanged: arg-max; log-softmax, the stopped-beam rule and the
 * length-averaged top-k; nucleus + draw.  Beam scores and the sampling d_logp are those of the processed distribution;
 * d_logp's logsumexp runs over the logits after steps 1-4, before top_k and top_p (the convention d_logp has for top_p).
 * With a processor or a bias set, a step materialises the fp32 logits of at most CAPDEC_SAMPLE_ROWS rows at a time, as
 * capdec_decode_sample does; with none set the decode calls run exactly the launches they run without this state.
 * capdec_decode_greedy_forced, capdec_score, capdec_gpt2_logits and the train step IGNORE the processors and the bias.
 * Refused (capdec_last_error; the state is left as it was): theta <= 0, NaN or inf; a negative size.  NULL: none.
 * (Added without a new ABI number, like capdec_decode_sample.) */
typedef struct { float repetition_penalty; int no_repeat_ngram_size; int min_length; int top_k; } capdec_logits_processors;
int capdec_set_logits_processors(capdec_ctx *ctx, const capdec_logits_processors *p);
/* h_bias: HOST array [vocab], validated and uploaded once (NULL: no bias).  Refused: GPT-2 not loaded, vocab not the
 * loaded vocabulary, a NaN or +inf entry, fewer than 1026 finite entries -- a step bans at most entry_length + 1 <= 1025
 * tokens, so a row can always emit one. */
int capdec_set_logit_bias(capdec_ctx *ctx, const float *h_bias, int vocab);

/* ---- scoring ------------------------------------------------------------------------- */
/* Teacher-forced log-probabilities of GIVEN captions; the [rows, vocab] logits never exist in HBM.
 * Caption r has prefix rows d_prefix[r] [P, d], token ids d_tokens[r, 0..L) and a length len[r] in 0..L.  The model input is
 * cat(d_prefix[r], wte(tok[r, :len[r]-1])) + wpe, and for i < len[r]
 *     d_logp[r, i] = s[tok[r, i]] - logsumexp(s),   s = logits at position P-1+i, times 1 / (temperature > 0 ? temperature : 1)
 * -- `logits[:, P-1:-1]` against `tokens` of reference train.py:349, the `softmax().log()` of generate_beam, and the logp
 * capdec_decode_sample reports.
 *   - positions i >= len[r] get d_logp = 0 (and d_top1 = 0);
 *   - a label equal to ignore_id gets d_logp = 0 and is not counted (ignore_id = -1: none; ignore_id = 0 with every len = L is
 *     the train loss's convention);
 *   - d_sum[r] = the sum of d_logp[r, :] over the counted positions, d_count[r] = how many there are;
 *   - d_top1[r, i] (optional) = the arg-max id at that position;
 *   - an id outside [0, vocab) is never used as an address: as an input it looks up row 0, and from the position it feeds on
 *     the caption's d_logp -- and its d_sum -- are NaN; as a label it gives NaN at its own position (capdec_cross_entropy
 *     and the train step treat such ids the same way);
 *   - len[r] = 0 is legal: sum 0, count 0.
 * h_lens is a HOST array ([n]; NULL = every caption has L tokens): the call plans its chunks from the lengths before it
 * launches anything, and a device array would cost a synchronisation per call.  A chunk is a run of whole captions in
 * input order whose padded row count, captions x (P + the chunk's longest len - 1), stays within CAPDEC_SCORE_ROWS (default
 * 16384; at least one caption); a caption's results do not depend on the chunk it lands in beyond the summation order of
 * the GEMMs, and not at all under capdec_set_batch_invariant (every chunk is then padded to the call's longest caption).
 * Limits: those of capdec_gpt2_logits, P + L - 1 <= min(n_positions, 1024); head_dim 64.  A NaN temperature is an error.
 * (Added without a new ABI number, like capdec_decode_sample.) */
int capdec_score(capdec_ctx *ctx, const float *d_prefix /* [n, P, d] */, const int32_t *d_tokens /* [n, L] */,
                 const int32_t *h_lens /* HOST [n], NULL = all L */, int n, int P, int L, int ignore_id,
                 float temperature, float *d_logp /* [n, L] */, float *d_sum /* [n] or NULL */,
                 int32_t *d_count /* [n] or NULL */, int32_t *d_top1 /* [n, L] or NULL */);
/* *chunks = how many chunks the last capdec_score call split its captions into; 0 for an empty call. */
int capdec_score_chunks(capdec_ctx *ctx, int *chunks);

/* ---- prefix interpretation ----------------------------------------------------------- */
/* Nearest rows of a table under cosine similarity; the [rows, table_rows] similarity matrix never exists in HBM.
 * xn = x / max(||x||_2, 1e-12), tn likewise (torch's nnf.normalize); sim[r, j] = <xn[r], tn[j]>.
 * d_ids[r, 0..k) = the k table rows with the largest sim, descending; EQUAL sims in ascending id order; d_sims (may be NULL)
 * their values.  d_table == NULL: the loaded GPT-2's wte [vocab, n_embd] (reference gpt2_prefix_eval.py:248-249, :233-234,
 * with the normalisation of :259-260); table_rows is then ignored.
 *   - Both operands are normalised BEFORE the product, so every GEMM operand lies in [-1, 1]: the norms of trained prefixes
 *     never meet the +-65504 clamp of the fp16-plane operand formats.
 *   - fp32-accurate in every GEMM mode, as the mapper's GEMMs are: modes f16x2, bf16 and f16 run the two-fp16-plane
 *     kernels (d % 64 == 0; other d the native fp32 kernel), mode bf16x3 its own top-k kernel, mode f32 the native one.
 *   - Limits, each refused with capdec_last_error and the context left usable: d a multiple of 32, at most 1024;
 *     1 <= k <= 8 and k <= table_rows; rows >= 0 (rows == 0 succeeds and touches nothing); with d_table == NULL, GPT-2
 *     must be loaded and d == n_embd.  d_x and d_table are 16-byte aligned.
 *   - An all-zero query row has every sim 0 and ids 0..k-1.  A query row holding a NaN or an inf gets d_sims NaN and d_ids
 *     -1 for that row only; no id outside [0, table_rows) is ever written otherwise.  A zero table row has sim 0.  A table
 *     row holding a NaN or an inf makes the call FAIL and write nothing (the normalising pass reads every row anyway).
 *     Defined for norms whose square is a normal fp32 number; beyond that the behaviour is that of fp32 nnf.normalize.
 *   - Rows are processed in blocks of a fixed 16 384 rows (the per-tile candidate lists of 50 257 columns at k = 8 are
 *     28 KB per row).  A row's result does not depend on the other rows beyond what capdec_set_batch_invariant documents
 *     (from 2048 rows a block takes a 256-row tile); with that mode on a row's ids and sims are bit-identical whatever the
 *     batch and the block (the 128-row tile is pinned, as for the lm_head).
 *   - The normalised wte is cached on first use (an fp32 copy plus its operand planes) and dropped by capdec_load_gpt2,
 *     capdec_destroy and every train step that updates wte.  A caller's d_table is normalised on every call, never cached.
 *   - The call enqueues on the context's stream and synchronises before it returns, like the decode calls.
 * (Added without a new ABI number, like capdec_score.) */
int capdec_nearest_tokens(capdec_ctx *ctx, const float *d_x /* [rows, d] */, int rows, int d,
                          const float *d_table /* [table_rows, d] or NULL = wte */, int table_rows,
                          int k, int32_t *d_ids /* [rows, k] */, float *d_sims /* [rows, k] or NULL */);
/* ---- noise variance and modality offset from embeddings -------------------------------- */
/* Column moments of two sets of embeddings, paired row by row: what reference others/modality_offset_calculator.py
 * (get_centers_info, get_variance_info) computes with fp32 torch on the host, and the per-row image-text distance that
 * predictions_runner.py's --ablation_image_dist averages.  With normalize != 0 every row is first divided by its L2 norm
 * (x /= torch.norm(x, dim=1, keepdim=True)).  Rows of d_stats [7, dim]:
 *   0, 1     column means of a and of b
 *   2        column mean of b - a: offset_to_add_in_inference (the training offset is its negative)
 *   3, 4, 5  unbiased column standard deviations (torch.std, divisor n - 1) of a, b and b - a
 *   6        column mean of |b - a|
 * d_pair[i] (may be NULL) = (||b_i - a_i||_2, ||b_i - a_i||_inf) of the (normalised) rows.  d_b == NULL: rows 0 and 3 only,
 * the other rows are set to 0, and d_pair must be NULL.
 *   - Every sum -- row norms, column sums, sums of squares -- is taken in fp64; the outputs are the fp32 roundings.
 *   - Deterministic, no floating-point atomics: rows are split into slabs of a fixed 64 rows, each block writes its slab's
 *     fp64 sums to a workspace of the context, and these are added in slab order (32 consecutive partials at a time, level
 *     by level).  Two calls on the same input return the same bits; a row's d_pair does not depend on n.
 *   - Every input row is read from global memory twice, once by the norm pass and once by the column pass of the same
 *     block.  With several 160-330 KB slabs live per CU the second read is NOT known to hit L2 or the Infinity Cache;
 *     HBM traffic was not measured and may be up to twice the input.
 *   - The deviations come from the sums and the sums of squares, (sum x^2 - (sum x)^2 / n) / (n - 1) in fp64: about
 *     1e-16 (mean / std)^2 of relative error in the variance.  That is nothing for embeddings; a column whose std is below
 *     about 1e-5 of its |mean| loses its digits, and a constant column may return a tiny non-zero std where torch returns 0
 *     (a negative variance is returned as 0).
 *   - Limits, each refused with capdec_last_error and the context left usable: n >= 1 (with n == 1 the standard deviations
 *     are NaN, as in torch); dim a multiple of 4, at most 1024.  d_a and d_b are 16-byte aligned.
 *   - A zero row under normalize gives NaN, and NaN / inf propagate, exactly where the torch expressions give them: through
 *     every statistic that row's side enters and through that row's d_pair.  No address depends on a value.
 *   - The call enqueues on the context's stream and synchronises before it returns.
 * (Added without a new ABI number, like capdec_nearest_tokens.) */
int capdec_embed_moments(capdec_ctx *ctx, const float *d_a /* [n, dim] images */,
                         const float *d_b /* [n, dim] texts, or NULL */, int n, int dim, int normalize,
                         float *d_stats /* [7, dim] */, float *d_pair /* [n, 2] or NULL */);
/* Distances inside groups of rows: reference predictions_runner.py calc_distances_of_ready_embeddings (:32-95) for every
 * image's captions at once.  Group k is the rows d_index[h_offsets[k] .. h_offsets[k + 1]) of d_x (d_index == NULL: those row
 * numbers themselves), so the caller groups by image id without a gather.  Per group of g rows with c = g (g - 1) / 2 pairs,
 * d_out[k, 0..8) (columns 0-3 over the pair differences x_i - x_j; m = the group's mean row):
 *   0  sum ||x_i - x_j||_1 / (W c)
 *   1  sum ||x_i - x_j||_2 / (W c)      (the reference's own normalisation, kept although its comment calls it wrong)
 *   2  sum ||x_i - x_j||_inf / c        (its mean over the images is what --noise_variance stands for)
 *   3  max over the pairs of ||x_i - x_j||_2 / sqrt(W)
 *   4  mean over the rows of ||x_i - m||_2
 *   5  mean over the rows of ||x_i - m||_inf
 *   6  c          7  g
 * g == 1: columns 0-3 and c are 0, and so are the to-centre columns.
 *   - One block per group walks the columns once; sums of |d| and d^2 are taken in fp64, maxima in fp32 (the fp32 rounding of
 *     an exact difference: column 2 of a two-row group is bit-exact); the square roots and divisions are fp64, the outputs
 *     their fp32 roundings.  A NaN propagates into every column it enters.
 *   - Limits, each refused with capdec_last_error before the group kernel is launched, the context left usable:
 *     1 <= g <= 8 (h_offsets ascends strictly, from a value >= 0); W a positive multiple of 4; groups >= 0 (groups == 0
 *     succeeds and touches nothing); every index in [0, rows) -- d_index is checked by a small kernel whose flag the call
 *     reads first; without d_index, h_offsets[groups] <= rows.  No row outside the array is ever read.  d_x is 16-byte
 *     aligned.
 *   - The call enqueues on the context's stream and synchronises before it returns.
 * (Added without a new ABI number, like capdec_nearest_tokens.) */
int capdec_group_distances(capdec_ctx *ctx, const float *d_x /* [rows, W] */, int rows, int W,
                           const int32_t *d_index /* [h_offsets[groups]] row numbers, or NULL = identity */,
                           const int32_t *h_offsets /* HOST [groups + 1], ascending */, int groups,
                           float *d_out /* [groups, 8] */);
/* ---- CLIPScore and the order of candidate captions ------------------------------------- */
/* CLIPScore / RefCLIPScore (Hessel et al., EMNLP 2021) of candidate captions, and their order per image: the comparison
 * after capdec_clip_encode_image / capdec_clip_encode_text that says which of an image's candidates fits it.  Group g (one
 * image, row g of d_img) owns the candidate rows h_offsets[g] .. h_offsets[g + 1] of d_cand, 0 to 64 of them, and the
 * reference rows h_ref_offsets[g] .. h_ref_offsets[g + 1] of d_ref, any number.  All rows are raw tower outputs: nothing is
 * normalised beforehand.  d is 1..2048, any value.  Per candidate c of an image v with references R, d_scores[row, 0..4):
 *   0  cos       = c.v / (||c|| ||v||)
 *   1  clip_s    = w max(cos, 0)                               (w = 2.5 in the paper)
 *   2  ref_sim   = max(0, max over r in R of cos(c, r));       NaN when the group has no references or d_ref is NULL
 *   3  refclip_s = 2 clip_s ref_sim / (clip_s + ref_sim), 0 when both are 0;      NaN when column 2 is NaN
 *   - Every sum (squared norms, dots) is fp64; each column is computed in fp64 and rounded to fp32 once.
 *   - A candidate or image row that holds a NaN or an inf, or is all zero, gives NaN in all four columns.  A reference row of
 *     that kind makes columns 2 and 3 of its whole group NaN, and nothing else.
 *   - d_order[h_offsets[g] + j] is the absolute row number of the j-th best candidate of group g: descending by the fp32 cos
 *     as written to column 0, NaN rows last, equal values (and the NaN rows among themselves) by ascending row.
 *   - A candidate's four values and a group's order depend only on that group's own rows: they are bit-identical whatever
 *     else is in the call and however the groups are arranged.  No atomics.
 *   - One block per image: the image row and the reference rows go through LDS once (the references in slabs of 16 KB), a
 *     wavefront takes each candidate's dots, one wavefront ranks the group.  The [rows, references] similarities never reach
 *     HBM: the algorithmic traffic is (rows + groups + ref_rows) d 4 bytes.  A group whose references need several slabs
 *     reads its candidates once per slab.
 *   - Refused, each with capdec_last_error, nothing launched and no output written, the context left usable: offsets that
 *     descend, do not start at 0 or do not end at rows / ref_rows; a group of more than 64 candidates; d outside 1..2048;
 *     exactly one of d_ref / h_ref_offsets given; a negative count.  groups == 0 or rows == 0 is a valid empty call.
 *   - The call enqueues on the context's stream and synchronises before it returns.
 * (Added without a new ABI number, like capdec_nearest_tokens.) */
int capdec_clip_score(capdec_ctx *ctx, const float *d_cand /* [rows, d] */, int rows, int d,
                      const float *d_img /* [groups, d] */, const int32_t *h_offsets /* HOST [groups + 1] */, int groups,
                      const float *d_ref /* [ref_rows, d] or NULL */, int ref_rows,
                      const int32_t *h_ref_offsets /* HOST [groups + 1] or NULL */, float w,
                      float *d_scores /* [rows, 4] */, int32_t *d_order /* [rows] */);
/* ---- supervised modality bridger ------------------------------------------------------- */
/* Reference others/supervised_embedding_bridger.py: an MLP that maps an image embedding to its caption's text embedding,
 * trained with nn.MSELoss and torch.optim.SGD(momentum) on pairs, applied between the normalisation / offset and clip_project
 * (predictions_runner.py --modality_bridger).  A context owns at most one bridger: L Linear layers in nn.Linear layout,
 * W_l [dims[l + 1], dims[l]] and b_l [dims[l + 1]], ReLU after every layer but the last.  capdec_bridger_load copies the
 * host tensors, zeroes the momentum buffers and the loss scalars, and replaces a bridger loaded before.
 *   - Limits, each refused with capdec_last_error and the context left usable: 1 <= L <= 16; every width a multiple of 4 in
 *     4..1024; train batch 1..64; every call but the load needs a loaded bridger.  Device pointers are 16-byte aligned,
 *     and d_out does not overlap d_x.
 *   - Arithmetic is fp32 with fp32 accumulation.  An output of a layer is four chains of FMAs over the layer's inputs (by
 *     index mod 4, each in index order), added in a fixed order, whatever n is and wherever the row sits: capdec_bridger_forward, _train_step and _eval give a row the same
 *     bits.  No floating-point atomics anywhere: the same call from the same state gives the same bits.
 *   - NaN / inf in the inputs propagate as IEEE arithmetic propagates them; there is no guard (torch has none).
 * capdec_bridger_forward: d_out = MLP(d_x) for n rows (n == 0 succeeds and touches nothing); synchronises.
 * capdec_bridger_train_step: the reference's loop body (:144-153) -- forward, MSELoss over the batch * dims[L] outputs (the
 *   squared differences summed in fp64 in a fixed order, the loss rounded to fp32), backward, and the update of
 *   torch.optim.SGD with dampening 0, no Nesterov, no weight decay: v = momentum * v + g, p -= lr * v (v is 0 after a load:
 *   torch's buf = grad on the first step).  The ReLU derivative is h > 0 on the saved post-activation (0 at 0, as torch).
 *   The weight gradient is never stored: after the first step from a load the momentum buffer IS the gradient, afterwards
 *   g_k = v_k - momentum * v_(k-1).  lr == 0 is legal (the weights stay, v moves).  loss == NULL only enqueues; otherwise
 *   the call waits and returns the step's loss.  2 L + 1 launches.
 * capdec_bridger_train_epoch: the unshuffled, not-drop_last DataLoader over n device-resident rows -- consecutive slices of
 *   `batch` rows, the last one possibly short -- enqueued without a host round trip; bit for bit that sequence of
 *   capdec_bridger_train_step calls.  It does not wait for the device.
 * capdec_bridger_loss: like capdec_train_loss -- the last step's loss, the fp64 sum of the steps' fp32 losses and their
 *   number since the load or the last reset (the epoch's train_loss is sum / steps); waits for the device.
 * capdec_bridger_eval: the validation loop (:165-177) -- the forward over all n rows, MSELoss per consecutive slice of
 *   `batch` >= 1 rows (the last possibly short), the fp64 sum of those fp32 losses in order and their count; synchronises.
 * capdec_bridger_get copies to d_out (device, n floats, which must be the tensor's size): kind 0 a parameter, kind 1 its
 *   momentum buffer (which = 2 l the weight, 2 l + 1 the bias); kind 2 activation `which` of the last train step,
 *   [batch, dims[which + 1]], post-ReLU for hidden layers, which = L - 1 the output.
 * (Added without a new ABI number, like capdec_nearest_tokens.) */
int capdec_bridger_load(capdec_ctx *ctx, int num_layers, const int *h_dims /* HOST [L + 1] */,
                        const float *const *h_w /* HOST [L] pointers to host tensors */, const float *const *h_b);
int capdec_bridger_forward(capdec_ctx *ctx, const float *d_x /* [n, dims[0]] */, int n, float *d_out /* [n, dims[L]] */);
int capdec_bridger_train_step(capdec_ctx *ctx, const float *d_x /* [batch, dims[0]] */, const float *d_y /* [batch, dims[L]] */,
                              int batch, float lr, float momentum, float *loss /* host, or NULL */);
int capdec_bridger_train_epoch(capdec_ctx *ctx, const float *d_x /* [n, dims[0]] */, const float *d_y /* [n, dims[L]] */, int n,
                               int batch, float lr, float momentum);
int capdec_bridger_eval(capdec_ctx *ctx, const float *d_x, const float *d_y, int n, int batch, double *loss_sum,
                        long long *batches);
int capdec_bridger_loss(capdec_ctx *ctx, float *last, double *sum, long long *steps, int reset);
int capdec_bridger_get(capdec_ctx *ctx, int kind, int which, float *d_out, size_t n);
/* ---- projection onto a support memory of text embeddings -------------------------------- */
/* The training-free way across the modality gap (DeCap, Li et al., ICLR 2023): keep the CLIP text embeddings of the training
 * captions as a support memory m [M, d] and replace an image embedding x by its softmax-weighted combination of memory rows,
 *     xn = x / max(||x||, 1e-12)        mn_j = m_j / max(||m_j||, 1e-12)
 *     w  = softmax_j(<xn, mn_j> / temperature)          (0.01 in the paper)
 *     v  = sum_j w_j mn_j               d_out = v / max(||v||, 1e-12)
 * so the result lies in the span of the text embeddings the decoder was trained on.  Also returned, each optional (NULL):
 * d_lse[r] = logsumexp_j(<xn, mn_j> / temperature); d_nearest[r] = argmax_j <xn, mn_j>, the lowest index among bit-equal
 * similarities -- the retrieval baseline; d_max_sim[r] = that similarity.
 *   - One fused pass, flash attention with K = V = the memory: neither the [rows, M] similarities nor the weights reach HBM.
 *   - fp32 arithmetic whatever the context's GEMM mode: both products run on the fp32 matrix instruction (a k-ordered chain
 *     of fp32 FMAs), the exponentials and the sums are fp32.  No fp16 plane holds a similarity or a weight.
 *   - capdec_memory_load normalises every row of d_mem (device, [rows, d]) once and keeps the unit rows in the context, fp32,
 *     d padded to a multiple of 128 -- 1.2 GB for 566 747 x 512 -- for every later call.  One memory per context: a second
 *     load replaces the first, capdec_memory_free and capdec_destroy drop it.  rows 1..4 194 304, d a multiple of 32 in
 *     32..640.  A memory row holding a NaN or an inf makes the load FAIL with the previous memory untouched; an all-zero row
 *     stays a zero row (similarity 0 to everything).
 *   - Deterministic and batch-invariant, no atomics: the memory is split into chunks of a fixed 2048 rows, every chunk is
 *     reduced from a fresh (max, sum, vector) state into a partial in a workspace of the context, and the partials are folded
 *     in chunk order by one formula.  The split depends on the memory alone, so a row's four outputs are bit-identical on
 *     every call, whatever the other rows of the call are.  One query row against a large memory still fills the chip (one
 *     block per chunk).  Query rows are processed in blocks sized so that the partials stay below 256 MiB.
 *   - A query row holding a NaN or an inf gets a NaN d_out row, NaN d_lse and d_max_sim and d_nearest -1; the call succeeds
 *     and the other rows are unaffected.  An all-zero query row has similarity 0 to every row: uniform weights.
 *   - Errors, each with capdec_last_error and the context left usable: no memory loaded, d differs from the memory's,
 *     temperature <= 0 or not finite, rows < 0.  rows == 0 succeeds and touches nothing.
 *   - The calls enqueue on the context's stream and synchronise before they return.
 * (Added without a new ABI number, like capdec_nearest_tokens.) */
int capdec_memory_load(capdec_ctx *ctx, const float *d_mem /* [rows, d] */, int rows, int d);
int capdec_memory_free(capdec_ctx *ctx);
int capdec_memory_project(capdec_ctx *ctx, const float *d_x /* [rows, d] */, int rows, int d, float temperature,
                          float *d_out /* [rows, d] */, float *d_lse /* [rows] or NULL */,
                          int32_t *d_nearest /* [rows] or NULL */, float *d_max_sim /* [rows] or NULL */);
/* Image preprocessing in front of capdec_clip_encode_image: the `preprocess` transform clip.load returns
 * (reference predictions_runner.py:212, embeddings_generator.py:72) = Resize(n_px, BICUBIC) -> CenterCrop(n_px) ->
 * ToTensor -> Normalize(mean, std); stretch != 0 = clip_transform_full (predictions_runner.py:116-122): Resize((n_px,
 * n_px)), no crop.  Bit-identical to PIL's 8-bit bicubic resampler + torch fp32 ToTensor / Normalize.
 * d_rgb: device buffer of concatenated uint8 HWC RGB images; offsets / heights / widths: HOST arrays [n] (byte offset
 * of image i in d_rgb and its size); mean / stdv: HOST float[3]; d_out: device fp32 [n, 3, n_px, n_px]. */
int capdec_preprocess_images(capdec_ctx *ctx, const uint8_t *d_rgb, const int64_t *offsets, const int32_t *heights,
                             const int32_t *widths, int n, int n_px, int stretch, const float *mean,
                             const float *stdv, float *d_out);
/* what the last decode call did: decode steps run (<= entry_length: the loop ends when every caption has stopped),
 * how many times finished captions were compacted out of the batch, and the activation rows pushed through the
 * GPT-2 body after the prefill (n * beam * (steps - 1) without early stopping).  CAPDEC_COMPACT=0 disables compaction. */
int capdec_decode_stats(capdec_ctx *ctx, int *steps, int *compactions, long long *row_steps);
/* finished-caption compaction on / off for the following decode calls (default on; CAPDEC_COMPACT=0 sets it off at
 * capdec_create): with it off every caption stays in the batch until ALL have stopped -- the reference's behaviour per
 * caption is the same either way (reference gpt2_prefix_eval.py:107-109,187-188 stop one caption at a time). */
int capdec_set_compact(capdec_ctx *ctx, int on);
/* rows[i] = activation rows the (i + 1)-th decode step of the last decode call pushed through the GPT-2 body (step 0 is the
 * prefill); *n = how many steps there were (<= entry_length - 1).  At most `cap` entries are written.  With compaction the
 * sequence steps down at the poll points as captions finish; without it it is constant.  The poll cadence is adaptive: every
 * step from 8192 rows, every 2 from 2048, every 4 from 512, every 8 below; a poll that finds no newly finished caption
 * doubles the interval (up to 8), the next one that does resets it. */
int capdec_decode_step_rows(capdec_ctx *ctx, int *rows, int cap, int *n);
/* *chunks = how many chunks the KV budget (capdec_set_kv_budget, clamped to the free device memory) split the captions of
 * the last decode call into; 0 for an empty call.  (Added with capdec_decode_sample, again without a new ABI number.) */
int capdec_decode_chunks(capdec_ctx *ctx, int *chunks);
/* kv_slots_per_position: over the last capdec_decode_beam call, the mean number of DISTINCT K/V cache slots one
 * (caption, position) of the decode attention read (1.0 = all beams of a caption share their whole history, `beam` =
 * none of it): the decode attention loads each distinct slot once, so its HBM traffic -- and its roofline -- scale with
 * this number (0 when no beam decode ran).  saturated_quads: how many 4-element groups of GEMM operands were clamped to
 * the +-65504 range of the fp16-plane formats since the last call (the counter is reset by the call; NaN is not
 * clamped, it propagates) -- nonzero means the fp32-accuracy claim of the default mode does not hold for this
 * checkpoint / input: switch to CAPDEC_GEMM_BF16X3 or CAPDEC_GEMM_F32.  The saturation counter is kept PER DEVICE (one
 * counter per GPU, shared by every context on it): with several contexts on one GPU the call returns -- and resets --
 * the clamps of all of them.  Either pointer may be NULL; the K/V statistic is accumulated on the device and read back
 * (one small copy + a stream synchronisation) only by this call. */
int capdec_decode_counters(capdec_ctx *ctx, double *kv_slots_per_position, long long *saturated_quads);
/* rows: over the last decode call, how many (row, step) pairs of the fused lm_head went through its exact second pass.
 * Beam search needs the 5 best logits of a row; above 2048 rows the fused kernel keeps only 3 per 128-column vocabulary
 * tile, the merge detects every row for which that can have dropped a candidate that matters, and those rows alone are
 * recomputed with 5 per tile (results are identical to keeping 5 everywhere; CAPDEC_LMHEAD_K3=0 does exactly that).  Compare
 * with row_steps of capdec_decode_stats: a checkpoint whose vocabulary clusters its best candidates in one tile pays for
 * the second pass, and this is the number that shows it.  (From 12288 rows the fused kernel keeps no candidates at all and
 * the tiles that can hold a row's 5 best are recomputed instead; the rows counted here are then those whose tile maxima tie
 * beyond 8 tiles or are not finite -- they take the same second pass.  CAPDEC_LMHEAD_SPARSE=0: 3 per tile at every size.) */
int capdec_decode_second_pass_rows(capdec_ctx *ctx, long long *rows);
#ifdef CAPDEC_MEASURE
/* MEASUREMENT BUILDS ONLY (libcapdec_hip_measure.so, compiled with -DCAPDEC_MEASURE; the shipped library does not export
 * it): every beam continues ITSELF (candidates of other parents are ignored), so no two beams of a caption share history
 * after the first step -- the worst-case K/V traffic of the decode attention.  Results are NOT the reference's beam search. */
int capdec_set_debug_diverge(capdec_ctx *ctx, int on);
#endif

/* ---- multi-GPU: caption-batch sharding + ONE gather of the generated ids (RCCL over xGMI) ------------------------
 * The reference has no distributed code: it loops over captions one at a time (predictions_runner.py:194,
 * embeddings_generator.py:58); every caption is independent.  Rank r of R decodes the contiguous block
 * [r * ceil(N/R), (r+1) * ceil(N/R)) of the embedding matrix with replicated weights; the only exchange is an
 * all-gather of int32 token ids / lengths (+ fp32 scores, or fp32 embeddings for the embeddings_generator path),
 * in rank order, so the gathered matrix has the single-GPU layout (and, in batch-invariant mode, the single-GPU
 * bits: by default the fp32 round-off of a row may depend on the size of its launch, see capdec_set_batch_invariant).  One communicator per context; RCCL is
 * dlopen'ed on first use (librccl.so.1), so single-GPU hosts do not need it.  A host without torch distributes the
 * 128-byte id itself (file, socket, MPI, environment ...); capdec_amd/distributed.py can use torch.distributed or
 * this communicator. */
#define CAPDEC_COMM_ID_BYTES 128
/* rank 0: create the communicator id (ncclGetUniqueId) and hand it to every rank */
int capdec_comm_unique_id(char *id /* [CAPDEC_COMM_ID_BYTES] */);
/* every rank, after capdec_create on its own GPU: join (ncclCommInitRank).  nranks == 1 is allowed. */
int capdec_comm_init(capdec_ctx *ctx, int rank, int nranks, const char *id /* [CAPDEC_COMM_ID_BYTES] */);
int capdec_comm_destroy(capdec_ctx *ctx);
/* what RCCL reports for the context's communicator (ncclCommUserRank / ncclCommCount): *rank = 0, *nranks = 1 when the
 * context has none.  A launcher can check that N ranks really joined (bench.py prints it as `rccl_ranks`). */
int capdec_comm_info(capdec_ctx *ctx, int *rank, int *nranks);
/* the shard of rank `rank`: [*lo, *hi) of n_total rows (trailing ranks may get an empty block) */
int capdec_shard_bounds(int n_total, int rank, int nranks, int *lo, int *hi);
/* all-gather of row blocks laid out by capdec_shard_bounds: d_local [n_local, row_elems] 4-byte elements (int32 or
 * fp32) of this rank -> d_global [n_total, row_elems] on every rank (blocks padded to ceil(N/R) rows internally, one
 * ncclAllGather, padding cut off).  Without a communicator (single GPU) it is a device copy and n_local must equal
 * n_total. */
int capdec_gather_rows(capdec_ctx *ctx, const void *d_local, int n_local, int row_elems, int n_total, void *d_global);
/* ids [n_local, T] + lens [n_local] (+ scores [n_local], may be NULL) of this rank's captions -> global arrays */
int capdec_gather_ids(capdec_ctx *ctx, const int32_t *d_ids, const int32_t *d_lens, const float *d_scores, int n_local,
                      int T, int n_total, int32_t *d_ids_global, int32_t *d_lens_global, float *d_scores_global);

/* ---- measurement / test hooks -------------------------------------------------------- */
/* C[M,N] = act(A[M,K] . Bt[N,K]^T + bias[N]) + resid[M,N]; bias / resid may be NULL.
 * The MFMA GEMM every projection above runs on (nn.Linear weights are already [N,K]). */
int capdec_gemm_f32(capdec_ctx *ctx, const float *d_a, int lda, const float *d_bt, int ldb,
                    float *d_c, int ldc, int M, int N, int K, const float *d_bias,
                    const float *d_resid, int ldr, int act);
/* C[n1,n2] = Xa[rows,n1]^T . Xb[rows,n2] (row strides lda / ldb / ldc): the weight-gradient product of the train step
 * (dW = dY^T X, reduction over the token rows), exactly as the train step calls it. */
int capdec_gemm_tn_f32(capdec_ctx *ctx, const float *d_xa, int lda, const float *d_xb, int ldb, int rows, int n1, int n2,
                       float *d_c, int ldc);
/* hipEvent timers on the context's stream -- the reference's Timer (predictions_runner.py:125-150) */
int capdec_timer_start(capdec_ctx *ctx);
int capdec_timer_stop_ms(capdec_ctx *ctx, float *ms);   /* records, synchronises, returns elapsed */
/* per-kernel-family accumulated device time since the last reset (hipEvents around the timed launches).
 * on = 0: off; 1: every launch is timed; N > 1: every N-th launch of each family is timed (sampling: the
 * events of the other launches are skipped, so a timed region is barely perturbed).
 * get: on entry *count = capacity of the caller's arrays (24 is always enough; a smaller capacity than the library
 * has families is an error, never an overflow), on return the number of entries filled; ms / launches / flops cover the TIMED launches
 * (flops: algorithmic FLOPs issued, 0 for non-GEMM families), calls = all launches of the family. */
int capdec_profile_enable(capdec_ctx *ctx, int on);
int capdec_profile_get(capdec_ctx *ctx, int *count, const char **names, float *ms, int64_t *launches,
                       double *flops, int64_t *calls);
int capdec_profile_reset(capdec_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* CAPDEC_H */
