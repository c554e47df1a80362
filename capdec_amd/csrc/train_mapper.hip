// Train step, the mapping networks (train.h): the MLP (reference gpt2_prefix.py:114-126), the TransformerMapper
// (transformer_mapper.py:113-127) and the encoder-decoder mapper (:130-145) -- forward keeping what the backward needs,
// backward into the gradient arena.
#include "train.h"

namespace capdec {

// dx = dy * (1 - y^2), y = tanh(.)
__global__ void tanh_bwd_kernel(const float *__restrict__ y, const float *dy, float *dx, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dx[i] = dy[i] * (1.0f - y[i] * y[i]);
}
// dx = dy where y > 0 (y = relu(.)), else 0
__global__ void relu_bwd_kernel(const float *__restrict__ y, const float *dy, float *dx, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dx[i] = y[i] > 0.f ? dy[i] : 0.f;
}
// TransformerMapper output = rows clip_len.. of the sequence: dseq[b, s] = s >= clip_len ? dout[b, s - clip_len] : 0
__global__ void tmapper_put_kernel(const float *__restrict__ dout, float *__restrict__ dseq, int n, int clip_len, int P, int d) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int S = clip_len + P;
    if (i >= (size_t)n * S * d) return;
    const int c = (int)(i % d), s_ = (int)((i / d) % S), b = (int)(i / ((size_t)d * S));
    dseq[i] = s_ >= clip_len ? dout[((size_t)b * P + (s_ - clip_len)) * d + c] : 0.f;
}
// the sequence's first layer input = cat(linear(x).view(B, clip_len, d), prefix_const): dlin[b, s, :] = dseq[b, s < clip_len],
// g_prefix_const[p, :] = sum_b dseq[b, clip_len + p, :]
__global__ void tmapper_split_grad_kernel(const float *__restrict__ dseq, float *__restrict__ dlin, float *__restrict__ gpc,
                                          int n, int clip_len, int P, int d) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int S = clip_len + P;
    if (i < (size_t)n * clip_len * d) {
        const int c = (int)(i % d), s_ = (int)((i / d) % clip_len), b = (int)(i / ((size_t)d * clip_len));
        dlin[i] = dseq[((size_t)b * S + s_) * d + c];
    }
    if (i < (size_t)P * d) {
        const int c = (int)(i % d), pp = (int)(i / d);
        float a = 0.f;
        for (int b = 0; b < n; ++b) a += dseq[((size_t)b * S + clip_len + pp) * d + c];
        gpc[i] = a;
    }
}

// y += x
__global__ void add_into_kernel(float *__restrict__ y, const float *__restrict__ x, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] += x[i];
}

// ---- the encoder-decoder mapper (mapper.hip: encdec_chunk states its forward).  What is kept: the encoder's layers as the
// TransformerMapper's (t_* buffers, width E; t_seq[L] = ref), the stacked cross keys | values, and per decoder layer the block
// input, norm1 output, queries, attention output, mid residual, norm2 output, relu(fc1) (+ keys | values on the self layers).
// Layer 0 runs on all B P rows (no shared-query shortcut): prefix_const's gradient is then the batch sum of d (decoder input).
int encdec_train_fits(capdec_ctx *c) {
    const Mapper &m = c->map;
    const int C = m.clip_len, P = m.P;
    CAPDEC_CHECK(m.d == 768 && m.d / m.heads == 96 && m.enc_dim == 512 && m.enc_dim / m.heads == 64,
                 "train_step: the encoder-decoder mapper trains at d = 768 (heads of 96) over an encoder of 512 (heads of 64)");
    CAPDEC_CHECK(AttnRect<64>::fits(C, C) && AttnRect<96>::fits(P, C) && AttnRect<96>::fits(P, P),
                 "train_step: the encoder-decoder mapper's attention backward (encoder C x C, cross P x C, self P x P) needs at most "
                 "128 queries and 128 keys and 153600 bytes of LDS per head: prefix_length or clip_length too large (square limit "
                 "90 at heads of 96)");
    return 0;
}

static int encdec_forward_saved(capdec_ctx *c, TrainState &t, const float *x, int B, float *pe) {
    Mapper &m = c->map;
    const int d = m.d, E = m.enc_dim, C = m.clip_len, P = m.P, L = m.n_layers, H = m.heads, hid = m.mlp_hidden, eh = m.enc_hidden;
    const int Me = B * C, Md = B * P, ldc = L * 2 * d;
    const size_t MeE = (size_t)Me * E, Mdd = (size_t)Md * d;
    hipStream_t st = c->stream;
    CAPDEC_TRY(t.t_seq.ensure(MeE * 4 * (L + 1)));
    CAPDEC_TRY(t.t_a1.ensure(MeE * 4 * L));
    CAPDEC_TRY(t.t_qkv.ensure(MeE * 3 * 4 * L));
    CAPDEC_TRY(t.t_att.ensure(MeE * 4 * L));
    CAPDEC_TRY(t.t_mid.ensure(MeE * 4 * L));
    CAPDEC_TRY(t.t_a2.ensure(MeE * 4 * L));
    CAPDEC_TRY(t.t_r.ensure((size_t)Me * eh * 4 * L));
    CAPDEC_TRY(t.d_kvc.ensure((size_t)Me * ldc * 4));
    CAPDEC_TRY(t.d_seq.ensure(Mdd * 4 * 2 * L));
    CAPDEC_TRY(t.d_a1.ensure(Mdd * 4 * 2 * L));
    CAPDEC_TRY(t.d_q.ensure(Mdd * 4 * 2 * L));
    CAPDEC_TRY(t.d_att.ensure(Mdd * 4 * 2 * L));
    CAPDEC_TRY(t.d_mid.ensure(Mdd * 4 * 2 * L));
    CAPDEC_TRY(t.d_a2.ensure(Mdd * 4 * 2 * L));
    CAPDEC_TRY(t.d_r.ensure((size_t)Md * hid * 4 * 2 * L));
    CAPDEC_TRY(t.d_kv.ensure(Mdd * 2 * 4 * L));
    // ---- encoder (current weights everywhere: never the cached planes of an earlier step)
    float *eseq = t.t_seq.as<float>();
    CAPDEC_TRY(gemm(c, x, m.D, m.lin_w, m.D, eseq, C * E, B, C * E, m.D, m.lin_b, CAPDEC_ACT_NONE, nullptr, 0, false));
    for (int l = 0; l < L; ++l) {
        float *qkv = t.t_qkv.as<float>() + MeE * 3 * l, *att = t.t_att.as<float>() + MeE * l;
        const TLayerBufs b{eseq + MeE * l, t.t_a1.as<float>() + MeE * l, qkv, att, t.t_mid.as<float>() + MeE * l,
                           t.t_a2.as<float>() + MeE * l, t.t_r.as<float>() + (size_t)Me * eh * l, eseq + MeE * (l + 1)};
        CAPDEC_TRY(tlayer_self_front(c, m.layers[l], b, Me, E, false));
        { ProfScope ps(c, F_MAP_ATTN); CAPDEC_TRY(launch_attn_cross(st, qkv, 3 * E, (size_t)C * 3 * E, qkv + E, qkv + 2 * E, 3 * E, att, B, C, C, H, E / H)); }
        CAPDEC_TRY(tlayer_tail(c, m.layers[l], b, Me, E, eh, false));
    }
    const float *ref = eseq + MeE * L;
    // ---- decoder
    float *kvc = t.d_kvc.as<float>(), *seq = t.d_seq.as<float>();
    CAPDEC_TRY(gemm(c, ref, E, m.wkv_cross, E, kvc, ldc, Me, ldc, E, nullptr, CAPDEC_ACT_NONE, nullptr, 0, false));
    { ProfScope ps(c, F_OTHER); CAPDEC_TRY(launch_tmapper_concat(st, nullptr, m.prefix_const, seq, B, 0, P, d)); }
    for (int l = 0; l < 2 * L; ++l) {
        const TMapLayer &w = m.dec[l];
        float *h = seq + Mdd * l, *a1 = t.d_a1.as<float>() + Mdd * l, *q = t.d_q.as<float>() + Mdd * l, *att = t.d_att.as<float>() + Mdd * l;
        { ProfScope ps(c, F_LN); CAPDEC_TRY(launch_layernorm(st, h, d, w.n1w, w.n1b, 1e-5f, a1, d, Md, d)); }
        CAPDEC_TRY(gemm(c, a1, d, w.wq, d, q, d, Md, d, d, nullptr, CAPDEC_ACT_NONE, nullptr, 0, false));
        if (l % 2 == 0) {
            const float *kl = kvc + (size_t)(l / 2) * 2 * d;
            ProfScope ps(c, F_MAP_ATTN);
            CAPDEC_TRY(launch_attn_cross(st, q, d, (size_t)P * d, kl, kl + d, ldc, att, B, P, C, H, d / H));
        } else {
            float *kv = t.d_kv.as<float>() + Mdd * 2 * (l / 2);
            CAPDEC_TRY(gemm(c, h, d, w.wkv, d, kv, 2 * d, Md, 2 * d, d, nullptr, CAPDEC_ACT_NONE, nullptr, 0, false));   // the stream itself
            ProfScope ps(c, F_MAP_ATTN);
            CAPDEC_TRY(launch_attn_cross(st, q, d, (size_t)P * d, kv, kv + d, 2 * d, att, B, P, P, H, d / H));
        }
        const TLayerBufs b{h, nullptr, nullptr, att, t.d_mid.as<float>() + Mdd * l, t.d_a2.as<float>() + Mdd * l,
                           t.d_r.as<float>() + (size_t)Md * hid * l, l == 2 * L - 1 ? pe : h + Mdd};
        CAPDEC_TRY(tlayer_tail(c, w, b, Md, d, hid, false));
    }
    return 0;
}

// one layer's backward from d (layer output) in `ds` down to d (attention output) in `datt`; leaves d mid in ds2.
// g(s) = where slot s's gradient goes
template <class G>
static int tlayer_tail_bwd(capdec_ctx *c, TrainState &t, const TMapLayer &w, G g, int M, int wd, int hid, const float *att,
                           const float *mid, const float *a2, const float *r, const float *ds, float *ds2, float *da, float *dr,
                           float *datt, bool ordered) {
    hipStream_t st = c->stream;
    // mlp: out = mid + fc2(relu(fc1(a2)))
    CAPDEC_TRY(linear_dw(c, t, ds, r, M, wd, hid, g(TL_WFC2), g(TL_BFC2), ordered));
    CAPDEC_TRY(linear_dx(c, t, ds, w.wfc2, dr, M, wd, hid));
    hipLaunchKernelGGL(relu_bwd_kernel, grid1((size_t)M * hid), dim3(256), 0, st, r, dr, dr, (size_t)M * hid);
    CAPDEC_TRY(linear_dw(c, t, dr, a2, M, hid, wd, g(TL_WFC1), g(TL_BFC1), ordered));
    CAPDEC_TRY(linear_dx(c, t, dr, w.wfc1, da, M, hid, wd));
    CAPDEC_TRY(ln_bwd(c, mid, w.n2w, da, ds, ds2, M, wd, 1e-5f, g(TL_N2W), g(TL_N2B), ordered));        // ds2 = d mid
    // attention: mid = h + project(att)
    CAPDEC_TRY(linear_dw(c, t, ds2, att, M, wd, wd, g(TL_WPROJ), g(TL_BPROJ), ordered));
    return linear_dx(c, t, ds2, w.wproj, datt, M, wd, wd);
}

static int encdec_backward(capdec_ctx *c, TrainState &t, const float *x, const float *dy, int B) {
    Mapper &m = c->map;
    const int d = m.d, E = m.enc_dim, C = m.clip_len, P = m.P, L = m.n_layers, H = m.heads, hid = m.mlp_hidden, eh = m.enc_hidden;
    const int Me = B * C, Md = B * P, ldc = L * 2 * d;
    const size_t MeE = (size_t)Me * E, Mdd = (size_t)Md * d, big = std::max(MeE, Mdd);
    hipStream_t st = c->stream;
    CAPDEC_TRY(t.t_ds.ensure(big * 4));
    CAPDEC_TRY(t.t_ds2.ensure(big * 4));
    CAPDEC_TRY(t.t_da.ensure(big * 4));
    CAPDEC_TRY(t.t_dr.ensure(std::max((size_t)Me * eh, (size_t)Md * hid) * 4));
    CAPDEC_TRY(t.t_dqkv.ensure(std::max(MeE * 3, Mdd) * 4));
    CAPDEC_TRY(t.t_datt.ensure(big * 4));
    CAPDEC_TRY(t.d_dkv.ensure(Mdd * 2 * 4));
    CAPDEC_TRY(t.d_dkvc.ensure((size_t)Me * ldc * 4));
    CAPDEC_TRY(t.d_dref.ensure(MeE * 4));
    float *ds = t.t_ds.as<float>(), *ds2 = t.t_ds2.as<float>(), *da = t.t_da.as<float>(), *dr = t.t_dr.as<float>(),
          *dq = t.t_dqkv.as<float>(), *datt = t.t_datt.as<float>(), *dkv = t.d_dkv.as<float>(), *dkvc = t.d_dkvc.as<float>(),
          *dref = t.d_dref.as<float>();
    const float *kvc = t.d_kvc.as<float>(), *seq = t.d_seq.as<float>(), *eseq = t.t_seq.as<float>();
    // ---- decoder, last layer first
    const float scale = (float)pow((double)(d / H), -0.5);
    CAPDEC_HIP(hipMemcpyAsync(ds, dy, Mdd * 4, hipMemcpyDeviceToDevice, st));
    for (int l = 2 * L - 1; l >= 0; --l) {
        const TMapLayer &w = m.dec[l];
        auto g = [&](TLayerSlot s) { return t.grad(ed_dec_slot(L, l, s)); };
        const float *h = seq + Mdd * l, *a1 = t.d_a1.as<float>() + Mdd * l, *q = t.d_q.as<float>() + Mdd * l;
        CAPDEC_TRY(tlayer_tail_bwd(c, t, w, g, Md, d, hid, t.d_att.as<float>() + Mdd * l, t.d_mid.as<float>() + Mdd * l,
                                   t.d_a2.as<float>() + Mdd * l, t.d_r.as<float>() + (size_t)Md * hid * l, ds, ds2, da, dr, datt, true));
        if (l % 2 == 0) {       // cross: this layer's column block of the stacked d (keys | values); its products wait for all L
            const float *kl = kvc + (size_t)(l / 2) * 2 * d;
            float *dkl = dkvc + (size_t)(l / 2) * 2 * d;
            ProfScope ps(c, F_MAP_ATTN);
            CAPDEC_TRY(train_attn_rect_bwd(c, q, d, kl, kl + d, ldc, datt, dq, d, dkl, dkl + d, ldc, B, P, C, H, d / H, scale));
        } else {                // self: keys and values read the stream itself -- x gets a second gradient, the weight sees x
            const float *kv = t.d_kv.as<float>() + Mdd * 2 * (l / 2);
            { ProfScope ps(c, F_MAP_ATTN); CAPDEC_TRY(train_attn_rect_bwd(c, q, d, kv, kv + d, 2 * d, datt, dq, d, dkv, dkv + d, 2 * d, B, P, P, H, d / H, scale)); }
            CAPDEC_TRY(linear_dw(c, t, dkv, h, Md, 2 * d, d, g(TL_WKV), nullptr));
        }
        CAPDEC_TRY(linear_dw(c, t, dq, a1, Md, d, d, g(TL_WQ), nullptr));
        CAPDEC_TRY(linear_dx(c, t, dq, w.wq, da, Md, d, d));
        CAPDEC_TRY(ln_bwd(c, h, w.n1w, da, ds2, ds, Md, d, 1e-5f, g(TL_N1W), g(TL_N1B), true));       // ds = d mid + LN'(..)
        if (l % 2 == 1) {
            CAPDEC_TRY(linear_dx(c, t, dkv, w.wkv, da, Md, 2 * d, d));
            hipLaunchKernelGGL(add_into_kernel, grid1(Mdd), dim3(256), 0, st, ds, da, Mdd);            // ... + dkv Wkv
        }
    }
    // prefix_const is the decoder's input in every caption: the batch sum, b = 0 first
    hipLaunchKernelGGL(tmapper_split_grad_kernel, grid1((size_t)P * d), dim3(256), 0, st, ds, (float *)nullptr, t.grad(ED_PREFIX_CONST),
                       B, 0, P, d);
    CAPDEC_HIP(hipGetLastError());
    // every cross layer read `ref`: one product each of the stacked d (keys | values) [B C, L 2d] with wkv_cross and with ref
    // (the L gradients are adjacent in the arena, as the weights are on the device: build_slots)
    CAPDEC_TRY(linear_dw(c, t, dkvc, eseq + MeE * L, Me, ldc, E, t.G.as<float>() + t.ed_cross_off, nullptr));
    CAPDEC_TRY(linear_dx(c, t, dkvc, m.wkv_cross, dref, Me, ldc, E));
    // ---- encoder: the TransformerMapper's layer at width E
    const float escale = (float)pow((double)(E / H), -0.5);
    float *es = dref, *es2 = ds2, *eo = ds;       // d (layer output), d mid, d (layer input)
    for (int l = L - 1; l >= 0; --l) {
        const TMapLayer &w = m.layers[l];
        auto g = [&](TLayerSlot s) { return t.grad(ed_enc_slot(l, s)); };
        const float *h = eseq + MeE * l, *a1 = t.t_a1.as<float>() + MeE * l, *qkv = t.t_qkv.as<float>() + MeE * 3 * l;
        CAPDEC_TRY(tlayer_tail_bwd(c, t, w, g, Me, E, eh, t.t_att.as<float>() + MeE * l, t.t_mid.as<float>() + MeE * l,
                                   t.t_a2.as<float>() + MeE * l, t.t_r.as<float>() + (size_t)Me * eh * l, es, es2, da, dr, datt, true));
        {
            ProfScope ps(c, F_MAP_ATTN);
            CAPDEC_TRY(train_attn_rect_bwd(c, qkv, 3 * E, qkv + E, qkv + 2 * E, 3 * E, datt, dq, 3 * E, dq + E, dq + 2 * E, 3 * E, B, C, C, H,
                                           E / H, escale));
        }
        CAPDEC_TRY(linear_dw(c, t, dq, a1, Me, 3 * E, E, g(TL_WQ), nullptr));       // [to_queries ; to_keys_values]: no bias
        CAPDEC_TRY(linear_dx(c, t, dq, w.wq, da, Me, 3 * E, E));
        CAPDEC_TRY(ln_bwd(c, h, w.n1w, da, es2, eo, Me, E, 1e-5f, g(TL_N1W), g(TL_N1B), true));
        std::swap(es, eo);
    }
    // es = d linear(x) viewed [B, C E]
    return linear_dw(c, t, es, x, B, C * E, m.D, t.grad(ed_lin_w_slot(L)), t.grad(ed_lin_b_slot(L)), true);
}

// ---- the mapper's forward with everything its backward needs; out = pe [B, P d]
int mapper_forward_saved(capdec_ctx *c, TrainState &t, const float *x, int B, float *pe) {
    Mapper &m = c->map;
    const int d = m.d, D = m.D, O = m.P * d;
    hipStream_t st = c->stream;
    if (m.kind == 3) return encdec_forward_saved(c, t, x, B, pe);
    if (m.kind == 1) {
        const int H = m.hidden;
        CAPDEC_TRY(t.hid.ensure((size_t)B * H * 4));
        // (current weights: never the cached planes of an earlier step)
        CAPDEC_TRY(gemm(c, x, D, m.w1, D, t.hid.as<float>(), H, B, H, D, m.b1, CAPDEC_ACT_TANH, nullptr, 0, false));
        return gemm(c, t.hid.as<float>(), H, m.w2, H, pe, O, B, O, H, m.b2, CAPDEC_ACT_NONE, nullptr, 0, false);
    }
    const int S = m.clip_len + m.P, M = B * S, hd = d / m.heads, hid = m.mlp_hidden, nl = m.n_layers;
    const size_t Md = (size_t)M * d;
    CAPDEC_TRY(t.t_lin.ensure((size_t)B * m.clip_len * d * 4));
    CAPDEC_TRY(t.t_seq.ensure(Md * 4 * (nl + 1)));
    CAPDEC_TRY(t.t_a1.ensure(Md * 4 * nl));
    CAPDEC_TRY(t.t_qkv.ensure(Md * 3 * 4 * nl));
    CAPDEC_TRY(t.t_att.ensure(Md * 4 * nl));
    CAPDEC_TRY(t.t_mid.ensure(Md * 4 * nl));
    CAPDEC_TRY(t.t_a2.ensure(Md * 4 * nl));
    CAPDEC_TRY(t.t_r.ensure((size_t)M * hid * 4 * nl));
    float *seq = t.t_seq.as<float>();
    CAPDEC_TRY(gemm(c, x, D, m.lin_w, D, t.t_lin.as<float>(), m.clip_len * d, B, m.clip_len * d, D, m.lin_b, CAPDEC_ACT_NONE,
                    nullptr, 0, false));
    { ProfScope ps(c, F_OTHER); CAPDEC_TRY(launch_tmapper_concat(st, t.t_lin.as<float>(), m.prefix_const, seq, B, m.clip_len, m.P, d)); }
    for (int l = 0; l < nl; ++l) {
        const TMapLayer &w = m.layers[l];
        float *h = seq + Md * l, *hn = seq + Md * (l + 1), *a1 = t.t_a1.as<float>() + Md * l, *qkv = t.t_qkv.as<float>() + Md * 3 * l,
              *att = t.t_att.as<float>() + Md * l, *mid = t.t_mid.as<float>() + Md * l, *a2 = t.t_a2.as<float>() + Md * l,
              *r = t.t_r.as<float>() + (size_t)M * hid * l;
        const TLayerBufs b{h, a1, qkv, att, mid, a2, r, hn};
        CAPDEC_TRY(tlayer_self_front(c, w, b, M, d, false));      // (current weights: never cached planes)
        {
            ProfScope ps(c, F_MAP_ATTN);
            if (hd == 96)       // (block-per-(sample, head) kernel when the head fits the LDS; the inference kernel otherwise)
                CAPDEC_TRY(train_attn_fwd(c, qkv, att, B, S, m.heads, 96, false, (float)pow(96.0, -0.5), nullptr, 1.f));
            else
                CAPDEC_TRY(launch_attn_mapper(st, qkv, 3 * d, qkv + d, qkv + 2 * d, 3 * d, att, B, S, m.heads, hd));
        }
        CAPDEC_TRY(tlayer_tail(c, w, b, M, d, hid, false));
    }
    ProfScope ps(c, F_OTHER);
    return launch_tmapper_take(st, seq + Md * nl, pe, B, m.clip_len, m.P, d);
}

// ---- the mapper's backward: dy [B, P d] = d loss / d pe  ->  every slot's gradient in the arena G
int mapper_backward(capdec_ctx *c, TrainState &t, const float *x, const float *dy, int B) {
    Mapper &m = c->map;
    const int d = m.d, D = m.D, O = m.P * d;
    hipStream_t st = c->stream;
    if (m.kind == 3) return encdec_backward(c, t, x, dy, B);
    if (m.kind == 1) {
        const int H = m.hidden;
        CAPDEC_TRY(t.dhid.ensure((size_t)B * H * 4));
        float *hid = t.hid.as<float>(), *dhid = t.dhid.as<float>();
        CAPDEC_TRY(linear_dw(c, t, dy, hid, B, O, H, t.grad(2), t.grad(3)));
        CAPDEC_TRY(linear_dx(c, t, dy, m.w2, dhid, B, O, H));
        hipLaunchKernelGGL(tanh_bwd_kernel, grid1((size_t)B * H), dim3(256), 0, st, hid, dhid, dhid, (size_t)B * H);
        return linear_dw(c, t, dhid, x, B, H, D, t.grad(0), t.grad(1));
    }
    const int S = m.clip_len + m.P, M = B * S, hid = m.mlp_hidden, nl = m.n_layers, HD = d / m.heads;
    CAPDEC_CHECK(HD == 96 && d == 768, "train: the TransformerMapper backward is instantiated for d = 768, 8 heads of 96");
    const size_t Md = (size_t)M * d;
    CAPDEC_TRY(t.t_ds.ensure(Md * 4));
    CAPDEC_TRY(t.t_ds2.ensure(Md * 4));
    CAPDEC_TRY(t.t_da.ensure(Md * 4));
    CAPDEC_TRY(t.t_dr.ensure((size_t)M * hid * 4));
    CAPDEC_TRY(t.t_dqkv.ensure(Md * 3 * 4));
    CAPDEC_TRY(t.t_datt.ensure(Md * 4));
    CAPDEC_TRY(t.t_dlin.ensure((size_t)B * m.clip_len * d * 4));
    CAPDEC_TRY(t.lse.ensure((size_t)B * m.heads * S * 4));
    CAPDEC_TRY(t.dsum.ensure((size_t)B * m.heads * S * 4));
    float *ds = t.t_ds.as<float>(), *ds2 = t.t_ds2.as<float>(), *da = t.t_da.as<float>(), *dr = t.t_dr.as<float>(),
          *dqkv = t.t_dqkv.as<float>(), *datt = t.t_datt.as<float>(), *dlin = t.t_dlin.as<float>();
    const float *seq = t.t_seq.as<float>();
    const float scale = (float)pow((double)HD, -0.5);
    hipLaunchKernelGGL(tmapper_put_kernel, grid1(Md), dim3(256), 0, st, dy, ds, B, m.clip_len, m.P, d);
    for (int l = nl - 1; l >= 0; --l) {
        const TMapLayer &w = m.layers[l];
        auto g = [&](TLayerSlot s) { return t.grad(tlayer_slot(l, s)); };
        const float *h = seq + Md * l, *a1 = t.t_a1.as<float>() + Md * l, *qkv = t.t_qkv.as<float>() + Md * 3 * l,
                    *att = t.t_att.as<float>() + Md * l, *mid = t.t_mid.as<float>() + Md * l, *a2 = t.t_a2.as<float>() + Md * l,
                    *r = t.t_r.as<float>() + (size_t)M * hid * l;
        CAPDEC_TRY(tlayer_tail_bwd(c, t, w, g, M, d, hid, att, mid, a2, r, ds, ds2, da, dr, datt, false));
        { ProfScope ps(c, F_MAP_ATTN); CAPDEC_TRY(train_attn_bwd(c, t, qkv, datt, dqkv, B, S, m.heads, 96, false, scale, nullptr, 1.f)); }
        CAPDEC_TRY(linear_dw(c, t, dqkv, a1, M, 3 * d, d, g(TL_WQ), nullptr));      // [to_queries ; to_keys_values]: no bias
        CAPDEC_TRY(linear_dx(c, t, dqkv, w.wq, da, M, 3 * d, d));
        CAPDEC_TRY(ln_bwd(c, h, w.n1w, da, ds2, ds, M, d, 1e-5f, g(TL_N1W), g(TL_N1B)));          // ds = d h
    }
    hipLaunchKernelGGL(tmapper_split_grad_kernel, grid1(std::max((size_t)B * m.clip_len * d, (size_t)m.P * d)), dim3(256), 0, st,
                       ds, dlin, t.grad(TM_PREFIX_CONST), B, m.clip_len, m.P, d);
    CAPDEC_HIP(hipGetLastError());
    return linear_dw(c, t, dlin, x, B, m.clip_len * d, D, t.grad(TM_LIN_W), t.grad(TM_LIN_B));
}

}  // namespace capdec
