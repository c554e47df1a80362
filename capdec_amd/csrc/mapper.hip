// From a CLIP embedding to the GPT-2 prefix: the prefix stage (capdec_normalize_prefix, capdec_noise_inject) and the three
// mapping networks behind capdec_mapper_forward -- the MLP, the TransformerMapper and the encoder-decoder mapper.  Every
// transformer among them is a stack of ONE layer (reference transformer_mapper.py:54-73); its forward is stated once here
// (tlayer_self_front, tlayer_tail: context.h) and the train forward (train_mapper.hip) runs the same two functions on
// per-layer saved buffers.  Host-side orchestration only, like decode.hip.
#include "context.h"

namespace capdec {

int tlayer_self_front(capdec_ctx *c, const TMapLayer &w, const TLayerBufs &b, int M, int wd, bool weight) {
    CAPDEC_CHECK(w.fused, "mapper: a layer without the fused [q | k | v] projection has no self front");
    { ProfScope ps(c, F_LN); CAPDEC_TRY(launch_layernorm(c->stream, b.x, wd, w.n1w, w.n1b, 1e-5f, b.a1, wd, M, wd)); }
    return gemm(c, b.a1, wd, w.wq, wd, b.qkv, 3 * wd, M, 3 * wd, wd, nullptr, CAPDEC_ACT_NONE, nullptr, 0, weight);
}

int tlayer_tail(capdec_ctx *c, const TMapLayer &w, const TLayerBufs &b, int M, int wd, int hid, bool weight) {
    CAPDEC_TRY(gemm(c, b.att, wd, w.wproj, wd, b.mid, wd, M, wd, wd, w.bproj, CAPDEC_ACT_NONE, b.x, wd, weight));
    { ProfScope ps(c, F_LN); CAPDEC_TRY(launch_layernorm(c->stream, b.mid, wd, w.n2w, w.n2b, 1e-5f, b.a2, wd, M, wd)); }
    CAPDEC_TRY(gemm(c, b.a2, wd, w.wfc1, wd, b.ff, hid, M, hid, wd, w.bfc1, CAPDEC_ACT_RELU, nullptr, 0, weight));
    return gemm(c, b.ff, hid, w.wfc2, hid, b.out, wd, M, wd, hid, w.bfc2, CAPDEC_ACT_NONE, b.mid, wd, weight);
}

// TransformerEncoderDecoder (reference transformer_mapper.py:130-145): ref = ref_encoder(linear(x) as [n, C, E]);
// out = prefix_decoder(prefix_const for every caption, ref).  Decoder layers alternate: even = cross (keys / values of
// `ref` as it is), odd = self called as layer(x, x): queries from norm1(x), keys / values from x ITSELF -- so the odd
// layers cannot use a fused [q|k|v] projection of one input.
static int encdec_chunk(capdec_ctx *c, const float *x, int n, float *out) {
    Mapper &m = c->map;
    const int d = m.d, E = m.enc_dim, C = m.clip_len, P = m.P, L = m.n_layers, H = m.heads;
    const int Me = n * C, Md = n * P;
    // refused before the first launch (the loader checked the same: a context cannot hold such a mapper)
    CAPDEC_CHECK(attn_cross_lds_bytes(C, C, E / H, 1) <= 160 * 1024 && attn_cross_lds_bytes(P, C, d / H, 1) <= 160 * 1024 &&
                 attn_cross_lds_bytes(P, P, d / H, 1) <= 160 * 1024, "mapper_forward: one head's keys, values and queries exceed 160 KB of LDS");
    const size_t ldc = (size_t)L * 2 * d;
    CAPDEC_TRY(c->m_lin.ensure((size_t)Me * E * 4));
    CAPDEC_TRY(c->m_seq.ensure((size_t)Md * d * 4));
    CAPDEC_TRY(c->m_x.ensure(std::max((size_t)Me * E, (size_t)Md * d) * 4));
    CAPDEC_TRY(c->m_qkv.ensure(std::max((size_t)Me * 3 * E, (size_t)Md * 3 * d) * 4));
    CAPDEC_TRY(c->m_att.ensure(std::max((size_t)Me * E, (size_t)Md * d) * 4));
    CAPDEC_TRY(c->m_ff.ensure(std::max((size_t)Me * m.enc_hidden, (size_t)Md * m.mlp_hidden) * 4));
    CAPDEC_TRY(c->m_kvc.ensure((size_t)Me * ldc * 4));
    CAPDEC_TRY(c->m_hid.ensure((size_t)2 * P * d * 4));
    float *ref = c->m_lin.as<float>(), *seq = c->m_seq.as<float>(), *xn = c->m_x.as<float>(), *qkv = c->m_qkv.as<float>(),
          *att = c->m_att.as<float>(), *ff = c->m_ff.as<float>(), *kvc = c->m_kvc.as<float>(), *q0 = c->m_hid.as<float>();
    // ---- encoder: the TransformerMapper layer at width E on the C rows of linear(x)
    CAPDEC_TRY(gemm(c, x, m.D, m.lin_w, m.D, ref, C * E, n, C * E, m.D, m.lin_b, CAPDEC_ACT_NONE));
    const TLayerBufs eb{ref, xn, qkv, att, ref, xn, ff, ref};       // in place: x = mid = out, one scratch for both norms
    for (int l = 0; l < L; ++l) {
        CAPDEC_TRY(tlayer_self_front(c, m.layers[l], eb, Me, E, true));
        { ProfScope ps(c, F_MAP_ATTN); CAPDEC_TRY(launch_attn_cross(c->stream, qkv, 3 * E, (size_t)C * 3 * E, qkv + E, qkv + 2 * E, 3 * E, att, n, C, C, H, E / H)); }
        CAPDEC_TRY(tlayer_tail(c, m.layers[l], eb, Me, E, m.enc_hidden, true));
    }
    // ---- decoder
    // `ref` is the same for every cross layer: their to_keys_values, stacked at load, run as ONE GEMM (N = L * 2d)
    // (5000 captions, L 4: 23.12 -> 22.75 ms per call against one GEMM per layer, profiles/mapper_encdec_bench.txt)
    CAPDEC_TRY(gemm(c, ref, E, m.wkv_cross, E, kvc, (int)ldc, Me, (int)ldc, E, nullptr, CAPDEC_ACT_NONE));
    // the residual stream starts as prefix_const in every caption (the concat kernel with no CLIP rows never reads `lin`)
    { ProfScope ps(c, F_OTHER); CAPDEC_TRY(launch_tmapper_concat(c->stream, nullptr, m.prefix_const, seq, n, 0, P, d)); }
    float *q = qkv, *kv = qkv + (size_t)Md * d;
    for (int l = 0; l < 2 * L; ++l) {
        const TMapLayer &w = m.dec[l];
        const bool cross = l % 2 == 0;
        const float *ql = q;
        size_t q_cap = (size_t)P * d;
        if (l == 0) {       // ... so layer 0's norm1 and to_queries are caption-independent: P rows, caption stride 0 (22.99 -> 22.75 ms)
            { ProfScope ps(c, F_LN); CAPDEC_TRY(launch_layernorm(c->stream, m.prefix_const, d, w.n1w, w.n1b, 1e-5f, q0 + (size_t)P * d, d, P, d)); }
            CAPDEC_TRY(gemm(c, q0 + (size_t)P * d, d, w.wq, d, q0, d, P, d, d, nullptr, CAPDEC_ACT_NONE));
            ql = q0;
            q_cap = 0;
        } else {
            { ProfScope ps(c, F_LN); CAPDEC_TRY(launch_layernorm(c->stream, seq, d, w.n1w, w.n1b, 1e-5f, xn, d, Md, d)); }
            CAPDEC_TRY(gemm(c, xn, d, w.wq, d, q, d, Md, d, d, nullptr, CAPDEC_ACT_NONE));
        }
        if (cross) {
            const float *kl = kvc + (size_t)(l / 2) * 2 * d;
            { ProfScope ps(c, F_MAP_ATTN); CAPDEC_TRY(launch_attn_cross(c->stream, ql, d, q_cap, kl, kl + d, (int)ldc, att, n, P, C, H, d / H)); }
        } else {
            CAPDEC_TRY(gemm(c, seq, d, w.wkv, d, kv, 2 * d, Md, 2 * d, d, nullptr, CAPDEC_ACT_NONE));   // the stream itself, not norm1 of it
            { ProfScope ps(c, F_MAP_ATTN); CAPDEC_TRY(launch_attn_cross(c->stream, ql, d, q_cap, kv, kv + d, 2 * d, att, n, P, P, H, d / H)); }
        }
        CAPDEC_TRY(tlayer_tail(c, w, TLayerBufs{seq, xn, nullptr, att, seq, xn, ff, l == 2 * L - 1 ? out : seq}, Md, d, m.mlp_hidden, true));
    }
    return 0;
}

static int mapper_chunk(capdec_ctx *c, const float *x, int n, float *out) {
    Mapper &m = c->map;
    const int d = m.d;
    if (m.kind == 3) return encdec_chunk(c, x, n, out);
    if (m.kind == 1) {
        CAPDEC_TRY(c->m_hid.ensure((size_t)n * m.hidden * 4));
        CAPDEC_TRY(gemm(c, x, m.D, m.w1, m.D, c->m_hid.as<float>(), m.hidden, n, m.hidden, m.D, m.b1, CAPDEC_ACT_TANH));
        CAPDEC_TRY(gemm(c, c->m_hid.as<float>(), m.hidden, m.w2, m.hidden, out, m.P * d, n, m.P * d, m.hidden, m.b2,
                        CAPDEC_ACT_NONE));
        return 0;
    }
    const int S = m.clip_len + m.P, M = n * S, hd = d / m.heads;
    CAPDEC_TRY(c->m_lin.ensure((size_t)n * m.clip_len * d * 4));
    CAPDEC_TRY(c->m_seq.ensure((size_t)M * d * 4));
    CAPDEC_TRY(c->m_x.ensure((size_t)M * d * 4));
    CAPDEC_TRY(c->m_qkv.ensure((size_t)M * 3 * d * 4));
    CAPDEC_TRY(c->m_att.ensure((size_t)M * d * 4));
    CAPDEC_TRY(c->m_ff.ensure((size_t)M * m.mlp_hidden * 4));
    float *seq = c->m_seq.as<float>(), *xn = c->m_x.as<float>(), *qkv = c->m_qkv.as<float>(), *att = c->m_att.as<float>();
    CAPDEC_TRY(gemm(c, x, m.D, m.lin_w, m.D, c->m_lin.as<float>(), m.clip_len * d, n, m.clip_len * d, m.D, m.lin_b,
                    CAPDEC_ACT_NONE));
    { ProfScope ps(c, F_OTHER); CAPDEC_TRY(launch_tmapper_concat(c->stream, c->m_lin.as<float>(), m.prefix_const, seq, n, m.clip_len, m.P, d)); }
    const TLayerBufs b{seq, xn, qkv, att, seq, xn, c->m_ff.as<float>(), seq};     // in place: x = mid = out, one scratch for both norms
    for (int l = 0; l < m.n_layers; ++l) {
        CAPDEC_TRY(tlayer_self_front(c, m.layers[l], b, M, d, true));
        { ProfScope ps(c, F_MAP_ATTN); CAPDEC_TRY(launch_attn_mapper(c->stream, qkv, 3 * d, qkv + d, qkv + 2 * d, 3 * d, att, n, S, m.heads, hd)); }
        CAPDEC_TRY(tlayer_tail(c, m.layers[l], b, M, d, m.mlp_hidden, true));
    }
    { ProfScope ps(c, F_OTHER); CAPDEC_TRY(launch_tmapper_take(c->stream, seq, out, n, m.clip_len, m.P, d)); }
    return 0;
}

}  // namespace capdec

using namespace capdec;

extern "C" {

int capdec_normalize_prefix(capdec_ctx *c, const float *x, int n, int dim, int normalize, const float *offset,
                            float *out) {
    CAPDEC_CHECK(c && n >= 0 && dim >= 1 && (n == 0 || (x && out)), "normalize_prefix: bad argument");
    if (n == 0) return 0;
    CAPDEC_HIP(hipSetDevice(c->device));
    ProfScope ps(c, F_OTHER);
    return launch_normalize_prefix(c->stream, x, n, dim, normalize, offset, out);
}

int capdec_noise_inject(capdec_ctx *c, const float *x, int n, int dim, float variance, const float *offset,
                        int uniform, int dont_norm, uint64_t seed, const float *noise, const float *u, float *out) {
    CAPDEC_CHECK(c && n >= 0 && dim >= 1 && (n == 0 || (x && out)), "noise_inject: bad argument");
    CAPDEC_CHECK(variance >= 0.f, "noise_inject: negative variance");
    if (n == 0) return 0;
    CAPDEC_HIP(hipSetDevice(c->device));
    ProfScope ps(c, F_OTHER);
    return launch_noise_inject(c->stream, x, n, dim, variance, offset, uniform, dont_norm, seed, noise, u, out);
}

int capdec_mapper_forward(capdec_ctx *c, const float *x, int n, float *out) {
    CAPDEC_CHECK(c && c->map.kind != 0, "mapper_forward: no mapper loaded");
    CAPDEC_CHECK(n >= 0 && (n == 0 || (x && out)), "mapper_forward: bad argument");
    CAPDEC_HIP(hipSetDevice(c->device));
    const Mapper &m = c->map;
    const int chunk = 8192;
    for (int c0 = 0; c0 < n; c0 += chunk) {
        const int nc = std::min(chunk, n - c0);
        CAPDEC_TRY(mapper_chunk(c, x + (size_t)c0 * m.D, nc, out + (size_t)c0 * m.P * m.d));
    }
    return 0;
}

}  // extern "C"
