// Shared declarations for libcapdec_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/capdec.h"
#include "config.h"
#include "gemm_plan.h"

namespace capdec {

void set_error(const std::string &msg);

#define CAPDEC_HIP(expr)                                                                         \
    do {                                                                                         \
        hipError_t _e = (expr);                                                                  \
        if (_e != hipSuccess) {                                                                  \
            ::capdec::set_error(std::string(#expr) + ": " + hipGetErrorString(_e) + " (" +       \
                                __FILE__ + ":" + std::to_string(__LINE__) + ")");               \
            return 1;                                                                            \
        }                                                                                        \
    } while (0)

#define CAPDEC_CHECK(cond, msg)                                                                  \
    do {                                                                                         \
        if (!(cond)) {                                                                           \
            ::capdec::set_error(std::string(msg) + " [" #cond "]");                              \
            return 1;                                                                            \
        }                                                                                        \
    } while (0)

#define CAPDEC_TRY(expr)                                                                         \
    do {                                                                                         \
        int _r = (expr);                                                                         \
        if (_r) return _r;                                                                       \
    } while (0)

constexpr int WAVE = 64;

// ---- wave-level helpers (64-wide wavefronts) ------------------------------------------
// Cross-lane traffic goes through DPP (data-parallel primitives: a VALU operand modifier), not
// through __shfl (which hipcc lowers to ds_bpermute_b32, an LDS-crossbar round trip per step).
// Within a row of 16 lanes: quad_perm [1,0,3,2] / [2,3,0,1] are the xor-1 / xor-2 butterflies, then
// row_half_mirror (lane i <- 7-i) and row_mirror (lane i <- 15-i) join the two quads and the two
// halves: after the four steps every lane of the row holds the reduction of the row's 16 lanes.
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
template <int CTRL>
__device__ __forceinline__ int dpp_i(int v) {
    return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, true);
}
constexpr int DPP_XOR1 = 0xB1, DPP_XOR2 = 0x4E, DPP_HALF_MIRROR = 0x141, DPP_MIRROR = 0x140;

__device__ __forceinline__ float row16_sum(float v) {
    v += dpp_f<DPP_XOR1>(v);
    v += dpp_f<DPP_XOR2>(v);
    v += dpp_f<DPP_HALF_MIRROR>(v);
    v += dpp_f<DPP_MIRROR>(v);
    return v;
}
__device__ __forceinline__ float row16_max(float v) {
    v = fmaxf(v, dpp_f<DPP_XOR1>(v));
    v = fmaxf(v, dpp_f<DPP_XOR2>(v));
    v = fmaxf(v, dpp_f<DPP_HALF_MIRROR>(v));
    v = fmaxf(v, dpp_f<DPP_MIRROR>(v));
    return v;
}
__device__ __forceinline__ float lane_bcast(float v, int l) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}
// full-wave reductions (all 64 lanes must be active): four row reductions + four scalar reads
__device__ __forceinline__ float wave_sum(float v) {
    v = row16_sum(v);
    return (lane_bcast(v, 0) + lane_bcast(v, 16)) + (lane_bcast(v, 32) + lane_bcast(v, 48));
}
__device__ __forceinline__ float wave_max(float v) {
    v = row16_max(v);
    return fmaxf(fmaxf(lane_bcast(v, 0), lane_bcast(v, 16)), fmaxf(lane_bcast(v, 32), lane_bcast(v, 48)));
}

// Philox4x32-10 counter RNG (Salmon et al.): key = seed, counter = (element index, stream).
__device__ __forceinline__ void philox4x32(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                           uint32_t k1, uint32_t (&o)[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
}

// ---- launch geometry of the f32 MFMA GEMM ----------------------------------------------
constexpr int GEMM_BM = 128, GEMM_BN = 128, GEMM_BK = 32;
constexpr int TOPK_MAX = 8;

// Decode-step qkv projection (f16x2 mode, fp32 KV cache): the K and V thirds of the result go STRAIGHT into the KV cache
// at the position being decoded -- activation row r (caption cmap[r / beam] after compaction) -> cache row
// caption * beam + r % beam, [head][pos][64] -- instead of into the qkv activation buffer, so the attention kernel
// neither re-writes them (154 MB per layer-step at 25 000 rows) nor treats the current token apart: it is simply the
// last cached position.  The q third still goes to C.
struct QkvScatter {
    float *kc = nullptr, *vc = nullptr;     // this layer's K / V cache (fp32; bf16 elements when `bf16` is set)
    const int *cmap = nullptr;
    int beam = 1, heads = 0, ctx = 0, pos = 0, d = 0;
    bool bf16 = false;                      // bf16 mode: the cache holds bf16 -- K / V are rounded (RNE) as they are written
};

// The epilogue of one GEMM.  Families: f32 (native fp32), bf16x3 (fp32 A), the packed-A kernels (bf16x3p / f16x2p / x1 and
// the wide-tile and ping-pong geometries of the two-plane format: gemm_h2w.hip, gemm_pp.hip) and the implicit 3x3
// convolution.  WHAT a packed launch runs -- kernel, K slices, blocks, workspace -- is decided by gemm_plan() (gemm_plan.h)
// alone; gemm_dispatch.hip (launch_packed) computes the plan from this struct and the shape and attaches the workspace.
struct GemmEpilogue {
    const float *bias = nullptr;   // [N]                                       (all)
    const float *resid = nullptr;  // [M, ldr] added after the activation       (all)
    int ldr = 0;
    int act = CAPDEC_ACT_NONE;     //                                           (all)
    void *splitk_ws = nullptr;     // packed-A kernels: workspace [S][M][N] of a plan with S > 1 (GemmPlan::ws_bytes)
    void *packed_out = nullptr;    // bf16x3p / f16x2p / x1 / conv: write act(acc + bias) as the packed A operand (K = N, the
                                   // launch's format) of the next GEMM instead of fp32 C
    const Tuning *tune = nullptr;  // the context's environment knobs (config.h); nullptr = every default
    const QkvScatter *qkv_scatter = nullptr;   // f16x2p / x1, unsplit plans only (see QkvScatter)
    bool wide_ok = false;          // planner input, f16x2p only: the B operand is a weight with max |w| < 16, so its high plane
                                   // can be scaled by 2^11 in fp16 registers (the single-accumulator kernels of gemm_h2w.hip)
    const void *resid_packed = nullptr;   // f16x2p / x1 with packed_out only: residual [M, N] stored as a packed operand of
                                          // the output's format (added after the activation; no split-K then)
    // bf16x3p / f16x2p / x1: optional LayerNorm of the RESULT rows, fused into the split-K reduce pass (only when the launch
    // splits K, C has N = ldc columns and N <= 1024): ln_out receives LayerNorm(C row) as a packed operand (format of the
    // launch); *ln_done is set to 1 when the fusion happened, left untouched otherwise (the caller then runs its own LayerNorm)
    const float *ln_w = nullptr, *ln_b = nullptr;
    float ln_eps = 1e-5f;
    void *ln_out = nullptr;
    int *ln_done = nullptr;
};
// Outputs of the fused lm_head launchers (*_topk, *_topk_dev): per (row, 128-column tile) the max, sum exp(x - max) and the
// k best (value, column) pairs -- [rows, tiles] and [rows, tiles, k]
struct TopkOut {
    float *tile_max, *tile_sum, *cand_val;
    int *cand_idx;
};
// f(std::integral_constant<int, K>()) for the runtime k in 1..TOPK_MAX: one instantiation of a top-k kernel per k
template <int K = 1, class F>
inline int with_topk_k(int k, const char *what, F &&f) {
    if constexpr (K <= TOPK_MAX) {
        if (k != K) return with_topk_k<K + 1>(k, what, f);
        f(std::integral_constant<int, K>());
        return 0;
    }
    CAPDEC_CHECK(false, std::string(what) + ": k must be in 1..8");
    return 1;
}
inline const Tuning &tuning_of(const GemmEpilogue &e) { return e.tune ? *e.tune : default_tuning(); }

// ---- what every packed launcher does before it launches what its plan names
// float4 epilogue when every row segment is 16-byte aligned (always the case on the decode path): a planner input
inline bool gemm_vec4(const GemmEpilogue &epi, const float *C, int ldc, int N) {
    return N % 4 == 0 && ldc % 4 == 0 && ((uintptr_t)C & 15) == 0 &&
           (epi.bias == nullptr || ((uintptr_t)epi.bias & 15) == 0) &&
           (epi.resid == nullptr || (epi.ldr % 4 == 0 && ((uintptr_t)epi.resid & 15) == 0));
}
struct PackedArgs {
    const float *resid = nullptr;      // the kernels' one residual argument: packed with a packed output, else fp32
    QkvScatter sc;
    float *part = nullptr;             // split launches: the workspace [S][M][N]
};
inline int packed_args(const std::string &who, const GemmEpilogue &epi, const GemmPlan &plan, const float *C, int ldc, int M,
                       int N, int K, PackedArgs *a) {
    CAPDEC_CHECK(M > 0 && N > 0 && K > 0 && K % 64 == 0, who + ": K must be a multiple of 64");
    CAPDEC_CHECK(epi.packed_out == nullptr ||
                     (N % 64 == 0 && epi.resid == nullptr && ((uintptr_t)epi.bias & 15) == 0),
                 who + ": packed output needs N % 64 == 0, a 16-byte aligned bias and no residual");
    const bool vec4 = gemm_vec4(epi, C, ldc, N);
    CAPDEC_CHECK(plan.vec4 == vec4 && (plan.S == 1 || epi.splitk_ws), who + ": the plan was made for another launch");
    CAPDEC_CHECK(epi.resid_packed == nullptr || epi.packed_out != nullptr, who + ": a packed residual needs a packed output");
    a->resid = epi.packed_out ? (const float *)epi.resid_packed : epi.resid;
    a->sc = epi.qkv_scatter ? *epi.qkv_scatter : QkvScatter();
    a->part = (float *)epi.splitk_ws;
    const QkvScatter &sc = a->sc;
    CAPDEC_CHECK(!sc.kc || (vec4 && epi.bias && !epi.resid && !epi.packed_out && epi.act == CAPDEC_ACT_NONE && N == 3 * sc.d &&
                            sc.d % GEMM_BN == 0 && plan.S == 1),
                 who + ": the qkv scatter epilogue needs an unsplit, biased, plain [M, 3d] projection");
    return 0;
}

// gemm_f32.hip
int launch_gemm_f32(hipStream_t st, const float *A, int lda, const float *Bt, int ldb, float *C, int ldc,
                    int M, int N, int K, const GemmEpilogue &epi);
// lm_head: logits tile never leaves the CU; per (row, 128-column tile) emits max, sum exp(x - max)
// and the top-k (value, column) pairs.
int launch_gemm_f32_topk(hipStream_t st, const float *A, int lda, const float *Bt, int ldb, int M, int N, int K,
                         int k, float inv_temp, const TopkOut &o);
inline int gemm_tiles_n(int N) { return (N + GEMM_BN - 1) / GEMM_BN; }

// gemm_bf16x3.hip: the same two GEMMs on the bf16 matrix cores with operands split into three bf16
// planes (fp32-accurate, 6 MFMA terms).  Bpacked = tile-major planes made by launch_pack_planes.
size_t packed_planes_bytes(int N, int K);
inline size_t x3_packed_bytes_host(int rows, int K) { return (size_t)((rows + 127) / 128) * 128 * K * 3 * sizeof(uint16_t); }
int launch_pack_planes(hipStream_t st, const float *w, int N, int K, void *out);
int launch_gemm_bf16x3(hipStream_t st, const float *A, int lda, const void *Bpacked, float *C, int ldc, int M, int N,
                       int K, const GemmEpilogue &epi);
int launch_gemm_bf16x3_topk(hipStream_t st, const float *A, int lda, const void *Bpacked, int M, int N, int K, int k,
                            float inv_temp, const TopkOut &o);
// packed-A variants: A already split / tile-major (written by launch_layernorm_packed, launch_pack_planes): both
// operands move by LDS-DMA.  Every packed launcher (here and below) takes the GemmPlan that gemm_plan() made for the launch:
// it checks its arguments against the plan and launches the kernel, slices and blocks the plan names
int launch_gemm_bf16x3p(hipStream_t st, const void *Apacked, const void *Bpacked, float *C, int ldc, int M, int N, int K,
                        const GemmEpilogue &epi, const GemmPlan &plan);
int launch_gemm_bf16x3p_topk(hipStream_t st, const void *Apacked, const void *Bpacked, int M, int N, int K, int k,
                             float inv_temp, const TopkOut &o);
// adds the S partial tiles of a split-K launch in slice order and applies the epilogue (fmt: packed output format)
int launch_splitk_reduce(hipStream_t st, const float *part, int S, int M, int N, const GemmEpilogue &epi, float *C,
                         int ldc, int fmt);
// f16x2 mode (gemm_f16x2.hip): operands as TWO fp16 planes (format PK_F16X2 of bf16x3.h), three MFMAs per product,
// fp32-accurate.  launch_pack_planes_h2 packs an fp32 [N, K] matrix (row stride ldw) -- weights once, fp32 activations
// (mapper, patch embedding) per call.
int launch_pack_planes_h2(hipStream_t st, const float *w, int ldw, int N, int K, void *out);
// ... and the TRANSPOSE of src [rows][cols] (row stride ld) as the packed matrix [cols][Kp] (k = the rows of src, zero-padded to Kp)
int launch_pack_planes_h2_t(hipStream_t st, const float *src, int ld, int rows, int cols, int Kp, void *out);
// fmt: PK_F16X2, or PK_F16X1 / PK_BF16X1 -- the one-plane kernels on the same main loop (32-deep stages, one MFMA per product)
int launch_gemm_f16x2p(hipStream_t st, const void *Apacked, const void *Bpacked, float *C, int ldc, int M, int N, int K,
                       const GemmEpilogue &epi, int fmt, const GemmPlan &plan);
int launch_gemm_f16x2p_topk(hipStream_t st, const void *Apacked, const void *Bpacked, int M, int N, int K, int k,
                            float inv_temp, const TopkOut &o, int fmt);
// round-3 wide-tile kernels with ONE accumulator set (gemm_h2w.hip); plan.geo: 2 = 256x128, 8 = 128x192 (two blocks per CU)
int launch_absmax_bits(hipStream_t st, const float *w, size_t n, unsigned *d_out);
int launch_gemm_h2w(hipStream_t st, const void *Apacked, const void *Bpacked, float *C, int ldc, int M, int N, int K,
                    const GemmEpilogue &epi, const GemmPlan &plan);
int launch_gemm_h2w_topk(hipStream_t st, const void *Apacked, const void *Bpacked, int M, int N, int K, int k,
                         float inv_temp, const TopkOut &o);
// round-4 ping-pong kernels (gemm_pp.hip): ONE 8-wavefront block per CU, the two wavefronts of a SIMD alternate between a
// load phase and a matrix phase; plan.geo: 10 = 256x128 (two accumulator sets), 14 = 256x192 (one set)
int launch_gemm_pp(hipStream_t st, const void *Apacked, const void *Bpacked, float *C, int ldc, int M, int N, int K,
                   const GemmEpilogue &epi, const GemmPlan &plan);
// exact second pass of the fused lm_head (decode.hip): k = 5 lists for the *m_dev rows of a compacted packed A operand
int launch_gemm_h2w_topk_dev(hipStream_t st, const void *Apacked, const void *Bpacked, const int *m_dev, int N, int K,
                             float inv_temp, const TopkOut &o);
int launch_gemm_x1_topk_dev(hipStream_t st, const void *Apacked, const void *Bpacked, const int *m_dev, int N, int K,
                            float inv_temp, const TopkOut &o, int fmt);
// generic packer for any PackFmt (gemm_f16x2.hip); the one-plane formats use it
int launch_pack_planes_fmt(hipStream_t st, const float *w, int ldw, int N, int K, void *out, int fmt);
// LayerNorm whose output goes straight into the packed split-bf16 A format of the next GEMM (d % 16 == 0)
int launch_layernorm_packed(hipStream_t st, const float *x, int ldx, const float *w, const float *b, float eps,
                            void *packed, int rows, int d, int fmt = 0);

// elementwise.hip
int launch_layernorm(hipStream_t st, const float *x, int ldx, const float *w, const float *b, float eps, float *y,
                     int ldy, int rows, int d);
// x / max(||x||_2, 1e-12) per row of x [rows, d] (nnf.normalize in fp32), as a packed GEMM operand of format fmt (`packed`)
// or as fp32 rows (`y`) -- exactly one is non-null.  A row holding a NaN or an inf is written as zeros and reported:
// row_bad[row] = 1 (else 0; may be null), *any_bad |= 1 (may be null)
int launch_l2norm_rows(hipStream_t st, const float *x, void *packed, float *y, int rows, int d, int fmt, int *row_bad,
                       int *any_bad);
int launch_embed_tokens(hipStream_t st, const int *tok, const float *wte, const float *wpe_row, float *h, int rows,
                        int d, const int *cmap = nullptr, int beam = 1);
int launch_embed_prefix(hipStream_t st, const float *prefix, const float *wpe, float *h, int n, int P, int pos0,
                        int d);
int launch_gather_rows(hipStream_t st, const float *table, const int *ids, float *out, int rows, int d);
int launch_normalize_prefix(hipStream_t st, const float *x, int n, int dim, int normalize, const float *offset,
                            float *out);
int launch_noise_inject(hipStream_t st, const float *x, int n, int dim, float variance, const float *offset,
                        int uniform, int dont_norm, uint64_t seed, const float *noise, const float *u, float *out);
int launch_tmapper_concat(hipStream_t st, const float *lin, const float *prefix_const, float *seq, int n,
                          int clip_len, int P, int d);
int launch_tmapper_take(hipStream_t st, const float *seq, float *out, int n, int clip_len, int P, int d);
int launch_transpose(hipStream_t st, const float *in, float *out, int rows, int cols);  // out[c][r] = in[r][c]
// CLIP glue
int launch_clip_text_embed(hipStream_t st, const int *tokens, const float *tok_emb, const float *pos_emb, float *h,
                           int n, int L, int d, int P = 0, const int *perm = nullptr);
int launch_eot_index(hipStream_t st, const int *tokens, int *flat_idx, int n, int L, int flat = 1);   // (flat: n*L +) argmax_t tokens[n,t]
int launch_eot_rows(hipStream_t st, const int *pos, const int *perm, int *rows, int m, int P);
int launch_scatter_rows(hipStream_t st, const float *src, const int *perm, float *dst, int rows, int d);
int launch_im2col_patches(hipStream_t st, const float *pixels, float *patches, int n, int S, int patch);
int launch_vision_assemble(hipStream_t st, const float *patch_out, const float *cls, const float *pos, float *seq,
                           int n, int ntok, int d);

// gemm_f16x2.hip: implicit-GEMM 3x3 convolution (stride 1, padding 1) on the packed-operand main loop: act_pk = the input
// activation [Nimg H W pixels][Cin] as a packed operand of format fmt (f16x2 / f16 / bf16), Bpacked = weights
// [Cout][9 Cin] in (ky, kx, c) order; zeros = a zeroed device buffer of >= (Cin / 16 + 1) * 8 KB (the padding's rows)
int launch_conv3x3_packed(hipStream_t st, const void *act_pk, const void *Bpacked, float *C, int ldc, int Nimg, int H,
                          int W, int Cin, int Cout, const GemmEpilogue &epi, int fmt, const void *zeros, size_t zero_bytes);

// resnet.hip: glue of CLIP's ModifiedResNet tower (NHWC fp32, channels padded to multiples of 64)
int launch_im2col3x3(hipStream_t st, const float *in, float *out, int N, int H, int W, int C, int stride, bool nchw3,
                     int Kp);
// the same straight into the packed GEMM operand of format fmt (PK_*: bf16x3.h): no fp32 im2col matrix in HBM
int launch_im2col3x3_packed(hipStream_t st, const float *in, void *out, int N, int H, int W, int C, int stride, bool nchw3,
                            int Kp, int fmt);
int launch_avgpool2(hipStream_t st, const float *in, float *out, int N, int H, int W, int C);
// AvgPool2d(2) between packed activations [N H W pixels][C] of format fmt; packed rows -> fp32 [M, C]
int launch_avgpool2_packed(hipStream_t st, const void *in, void *out, int N, int H, int W, int C, int fmt);
int launch_unpack_rows(hipStream_t st, const void *in, float *out, int M, int C, int fmt);
int launch_attnpool_tokens(hipStream_t st, const float *feat, const float *pos, float *t, int N, int HW, int C);
int launch_attnpool_attend(hipStream_t st, const float *q, const float *k, const float *v, float *out, int N, int heads,
                           int T, int C);

// attention.hip
struct KvCache {
    void *k = nullptr;   // [layer][phys_row][head][ctx][hd], fp32 -- or bf16 when `bf16` is set (bf16 GEMM mode)
    void *v = nullptr;
    int rows = 0, heads = 0, ctx = 0, hd = 0;
    bool bf16 = false;
    int prefix_len = 0;           // decode: positions [0, prefix_len) of every row live in slot 0 (the CLIP prefix)
    bool fixed_variant = false;   // batch-invariant mode: the launch-size dependent kernel variants are pinned
    size_t layer_stride() const { return (size_t)rows * heads * ctx * hd; }      // elements
    size_t elem_bytes() const { return bf16 ? 2 : 4; }
    template <typename T> T *kp(int layer) const { return reinterpret_cast<T *>(k) + (size_t)layer * layer_stride(); }
    template <typename T> T *vp(int layer) const { return reinterpret_cast<T *>(v) + (size_t)layer * layer_stride(); }
};
// write K/V of `rows` prefill rows (row = caption * P + i) into phys row caption*beam, position i
int launch_kv_scatter_prefill(hipStream_t st, const float *qkv, const KvCache &c, int layer, int ncap, int P,
                              int beam);
// prefill: query row (caption, i) attends cache positions 0..i of phys row caption*beam
int launch_attn_prefill(hipStream_t st, const float *qkv, const KvCache &c, int layer, int ncap, int P, int beam,
                        float *out, bool causal = true, void *packed_out = nullptr, int fmt = 0);
// decode: row r (caption = r / beam) at position L-1: its own k/v come from qkv (and are written to the cache
// at phys row r), positions p < L-1 from phys row caption*beam + anc[r][p] (anc == nullptr -> r itself)
int launch_attn_decode(hipStream_t st, const float *qkv, const KvCache &c, int layer, int rows, int beam, int L,
                       const uint8_t *anc, int anc_stride, float *out, void *packed_out = nullptr,
                       const int *cmap = nullptr, int fmt = 0, bool cur_cached = false);
// (cur_cached: the rows' own K / V are already in the cache at position L-1 -- written by the qkv GEMM's epilogue,
//  QkvScatter -- so the kernel neither reads them from `qkv` nor appends them)
// (cmap != nullptr: finished captions were compacted away -- activation row r belongs to caption cmap[r / beam];
//  KV cache, ancestor table and beam state stay indexed by the original caption)
// (packed_out != nullptr: the attention rows are written as the packed split-bf16 A operand of c_proj, K = d,
//  instead of fp32 `out`)
// TransformerMapper self-attention (no mask): q / k / v rows of n*seq tokens (row strides ldq, ldkv), head-major
int launch_attn_mapper(hipStream_t st, const float *q, int ldq, const float *k, const float *v, int ldkv, float *out,
                       int n, int seq, int heads, int hd);
// Encoder-decoder mapper: nq query rows per caption attend to nkv key / value rows from pointers of their own (row
// strides ldq / ldkv; q_cap_stride = elements between two captions' query blocks, 0 = one block shared by all), out
// [n, nq, heads * hd].  A block serves two (caption, head) units while their LDS need stays below ATTN_CROSS_GROUP_LDS.
constexpr size_t ATTN_CROSS_GROUP_LDS = 26 * 1024;
size_t attn_cross_lds_bytes(int nq, int nkv, int hd, int group);
int launch_attn_cross(hipStream_t st, const float *q, int ldq, size_t q_cap_stride, const float *k, const float *v,
                      int ldkv, float *out, int n, int nq, int nkv, int heads, int hd);

// select.hip
int launch_topk_merge(hipStream_t st, const float *tile_max, const float *tile_sum, const float *cand_val,
                      const int *cand_idx, int rows, int ntiles, int k, float *lse, float *top_val, int *top_idx);
// Three candidates per (row, tile) in, the row's top 5 + logsumexp out; a row one of whose tiles may hide a fourth
// candidate that still matters (the tile's third kept candidate is strictly better than the row's fifth) is appended to
// flag_rows[atomicAdd(flag_count)] -- its top 5 are provisional until the exact second pass has rewritten them
int launch_topk_merge_k3(hipStream_t st, const float *tile_max, const float *tile_sum, const float *cand_val,
                         const int *cand_idx, int rows, int ntiles, float *lse, float *top_val, int *top_idx,
                         int *flag_rows, int *flag_count, int *flag_total);
// the second pass's merge: *count_dev compact rows of k = 5 lists -> top_val / top_idx of rows out_rows[i]
int launch_topk_merge_rows(hipStream_t st, const float *cand_val, const int *cand_idx, const int *count_dev,
                           const int *out_rows, int rows_cap, int ntiles, float *top_val, int *top_idx);
// rows src_rows[i], i < *count_dev, of a packed operand [*, K] (PK_F16X2 or a one-plane format) -> rows i of `out`
int launch_gather_packed_rows(hipStream_t st, const void *packed, int K, const int *src_rows, const int *count_dev,
                              int rows_cap, void *out, int fmt);
// ---- the sparse lm_head (decode.hip: lm_head_select): no candidates from the first pass; per row the (row, tile) PAIRS
// whose tile maximum reaches the row's fifth largest are recomputed with k = 5 by a launch grouped by tile, then merged.
constexpr int LM_SPARSE_SHIFT = 3;
constexpr int LM_SPARSE_CAP = 1 << LM_SPARSE_SHIFT;        // pairs a row may have (five, plus exact ties at the fifth maximum); more: full second pass
constexpr int LM_SPARSE_MIN_TILES = 40;  // below that, five tiles of all are no saving
constexpr int LM_SPARSE_MIN_ROWS = 12288; // rows from which the route pays: +1.5 % at 25 000 rows, -1.1 % at 3125 (its ~13 extra small
                                          // launches cost ~100 us a step, the first pass saves ~18 ns per row: break-even near 7700 rows;
                                          // profiles/lm_head_sparse_ab.txt)
constexpr int LM_HARD_SLICES = 2;       // the full second pass of this route runs in that many slices of its flagged rows
struct SparseLm {        // device bookkeeping of one step (ints)
    int *tile_cnt;       // [ntiles]  pairs per column tile -- zeroed by the caller before launch_lm_tile_select
    int *tile_cur;       // [ntiles]  scatter cursors
    int *tile_off;       // [ntiles]  where a tile's bucket starts in the pair list
    int *nblk;           // [1]       blocks of the grouped launch
    int *slice_cnt;      // [LM_HARD_SLICES]  flagged rows each slice of the full second pass takes
    int *blk_tab;        // [blocks_cap][3]   (tile, first pair, pairs <= 256)
    int *row_cnt;        // [rows]    pairs of a row; 0 = the row takes the full second pass
    int *row_tiles;      // [rows][LM_SPARSE_CAP]  their tiles, ascending
    int *slot_of;        // [rows * LM_SPARSE_CAP]  the pair list, bucketed by tile: candidate list row * LM_SPARSE_CAP + s of a pair
    int slice_rows;      // rows per slice of the full second pass
    static int blocks_cap(int rows, int ntiles) { return (rows * LM_SPARSE_CAP + 255) / 256 + ntiles; }
};
// logsumexp [rows], the pairs of every row, the rows that need the full pass instead (flag_rows as launch_topk_merge_k3);
// then -- three small launches -- the pairs counted per tile, buckets / block table / slice counts, the pairs placed
int launch_lm_tile_select(hipStream_t st, const float *tile_max, const float *tile_sum, int rows, int ntiles, float *lse,
                          const SparseLm &s, int *flag_rows, int *flag_count, int *flag_total);
// the grouped pass (gemm_h2w.hip): block b of blk_tab computes its pairs' rows (slot_of[p] >> slot_shift of Apacked, read in
// place) against its one column tile, k = 5 candidates of pair p -> lists slot_of[p] of cand_val / cand_idx
int launch_gemm_h2w_topk_grouped(hipStream_t st, const void *Apacked, const void *Bpacked, const int *nblk_dev,
                                 const int *blk_tab, const int *slot_of, int slot_shift, int blocks_cap, int N, int K,
                                 float inv_temp, float *cand_val, int *cand_idx);
// top 5 of the candidate lists of a row's pairs -> top_val / top_idx [rows, 5] (rows with row_cnt = 0 untouched)
int launch_lm_sparse_merge(hipStream_t st, const float *cand_val, const int *cand_idx, const int *row_cnt, int rows,
                           float *top_val, int *top_idx);
struct BeamState {
    int *tokens = nullptr;      // [ncap, beam, T]
    float *scores = nullptr;    // [ncap, beam]  running SUM of log-probs (reference `scores`)
    float *seq = nullptr;       // [ncap, beam]  reference `seq_lengths` (fp32)
    uint8_t *stopped = nullptr; // [ncap, beam]
    uint8_t *done = nullptr;    // [ncap]  caption's loop has broken (all beams stopped)
    uint8_t *anc = nullptr;     // [ncap, beam, ctx]
    int *next_tok = nullptr;    // [ncap * beam]
    int *alive_count = nullptr; // [1] captions still running (device counter, polled by the host)
    unsigned *kv_stat = nullptr;   // [ncap, 2] optional: per caption, sum over the decode steps of (distinct K/V slots the
                                   // next step's attention reads, positions it attends to) -- what the attention roofline depends on
    int diverge = 0;               // measurement only: every beam continues ITSELF (worst-case K/V traffic; results differ)
    float *logp = nullptr;      // [ncap, beam]  diverse beam search only (diverse.hip): running sum of the UNPENALISED log-probs
};
int launch_beam_init(hipStream_t st, const BeamState &s, const float *lse, const float *top_val, const int *top_idx,
                     int ncap, int beam, int k, int T, int stop_id);
// pos_cur: the position this step's token was fed at (the step's attention read positions 0 .. pos_cur)
int launch_beam_step(hipStream_t st, const BeamState &s, const float *lse, const float *top_val, const int *top_idx,
                     int ncap, int beam, int k, int T, int ctx, int step, int pos_cur, int vocab, int stop_id,
                     const int *cmap = nullptr);
// rows ordered by (score / seq, slot); with con_state (ConstraintState::state) by (phrases met, score / seq, slot), and
// met [ncap, beam] (may be nullptr) receives the rows' met masks
int launch_beam_finalize(hipStream_t st, const BeamState &s, int ncap, int beam, int T, int *ids, int *lens,
                         float *scores, int *order, const int *con_state = nullptr, int *met = nullptr);
// diverse.hip: diverse (group) beam search -- the beam step run per group of beam / groups slots, with the tokens that the
// earlier groups of the caption took at this step penalised by `diversity` each (the contract: include/capdec.h)
int launch_group_beam_init(hipStream_t st, const BeamState &s, const float *lse, const float *top_val, const int *top_idx,
                           int ncap, int beam, int groups, float diversity, int k, int T, int stop_id);
int launch_group_beam_step(hipStream_t st, const BeamState &s, const float *lse, const float *top_val, const int *top_idx,
                           int ncap, int beam, int groups, float diversity, int k, int T, int ctx, int step, int pos_cur,
                           int vocab, int stop_id, const int *cmap = nullptr);
// logp_out[cap, rank] = s.logp[cap, order[cap, rank]]: the unpenalised sums in the order launch_beam_finalize returned
int launch_group_beam_logp(hipStream_t st, const BeamState &s, int ncap, int beam, const int *order, float *logp_out);
// constrained.hip: lexically constrained beam search by dynamic beam allocation (capdec_decode_beam_constrained; the
// contract: include/capdec.h).  phrases [ncap, 4, 4] (unused places -1), state [ncap, beam]: a slot's (met, cur, pos) packed
// into one int (0: nothing met, nothing in progress), permuted with the rest of the BeamState.
struct ConstraintState {
    const int *phrases = nullptr;   // [ncap, CON_PHRASES, CON_LEN]
    int *state = nullptr;           // [ncap, beam]
};
constexpr int CON_PHRASES = 4, CON_LEN = 4, CON_SPECIAL = CON_PHRASES + 1, CON_BEAM_MAX = 8;
constexpr int CON_LIST = CON_SPECIAL + CON_BEAM_MAX;     // a row's list: the special tokens' places, then its best `beam` others
// logsumexp and the list of every row of materialised logits [rows, ld], one pass: lse [rows]; top_val / top_idx
// [rows, CON_LIST] -- places 0..4 the row's special tokens (top_idx -1: unused), places 5..5+beam-1 its best `beam` tokens
// outside them; the stop token counts as -inf while the row's phrases are not all met.  Logits row r is activation row
// row0 + r and finds its caption and slot through cmap and beam as launch_logits_process finds its history (step 0: one
// row per caption, the empty state).
int launch_logits_select_forced(hipStream_t st, const float *logits, int ld, int rows, int row0, int V, int beam,
                                float inv_temp, const ConstraintState &cs, const int *cmap, int step, int stop_id,
                                float *lse, float *top_val, int *top_idx);
int launch_constrained_beam_init(hipStream_t st, const BeamState &s, const ConstraintState &cs, const float *lse,
                                 const float *top_val, const int *top_idx, int ncap, int beam, int T, int vocab, int stop_id);
int launch_constrained_beam_step(hipStream_t st, const BeamState &s, const ConstraintState &cs, const float *lse,
                                 const float *top_val, const int *top_idx, int ncap, int beam, int T, int ctx, int step,
                                 int pos_cur, int vocab, int stop_id, const int *cmap = nullptr);
// contrastive.hip: contrastive search (capdec_decode_contrastive; the contract: include/capdec.h).  K candidate rows per
// caption in the beam layout (row = caption * K + c); hist [ncap, ctx, d] holds ln_f of every position of the chosen path,
// L2-normalised.
struct ContrastState {
    int *ids = nullptr;         // [ncap, T]
    int *lens = nullptr;        // [ncap]
    uint8_t *done = nullptr;    // [ncap]
    uint8_t *anc = nullptr;     // [ncap, K, ctx]
    int *alive_count = nullptr; // [1] captions still running (device counter, polled by the host)
    float *hist = nullptr;      // [ncap, ctx, d]
    float *last = nullptr;      // [ncap, d] the chosen candidate's residual row (before ln_f), by caption
    float *sel = nullptr;       // [active captions, d] the same, by compact activation row: the next lm_head's input
    float *trace = nullptr;     // [ncap, T, 2] (p, sim) of the chosen candidate, or nullptr
    int T = 0, ctx = 0, d = 0, stop_id = -1, alt_stop_id = -1;
};
// hist[cap][p] = normalise(ln_f(h[cap * P + p])) for the ncap * P prefill rows; last[cap] = sel[cap] = h[cap * P + P - 1]
int launch_contrast_prefill(hipStream_t st, const ContrastState &s, const float *h, const float *lnw, const float *lnb,
                            float eps, int ncap, int P);
// one selection: block i takes the K rows h[i * K ..] of caption cmap[i] fed at position `pos`, their tokens / logits
// top_idx / top_val [i, K] and lse [i], and emits the winner at `step` (see the contract)
int launch_contrast_select(hipStream_t st, const ContrastState &s, const float *h, const float *lnw, const float *lnb,
                           float eps, const float *lse, const float *top_val, const int *top_idx, int nact, int K,
                           float alpha, int step, int pos, const int *cmap);
// The state the greedy family of decodes (arg-max, teacher-forced, sampling) keeps per caption, and the constants of the
// call that its step kernels need
struct GreedyState {
    int *ids = nullptr;         // [ncap, T]
    int *lens = nullptr;        // [ncap]
    uint8_t *done = nullptr;    // [ncap]
    int *next_tok = nullptr;    // [ncap]
    int *alive_count = nullptr; // [1] captions still running (device counter, polled by the host)
    float *logp = nullptr;      // [ncap, T] optional: log-probability of every emitted token (sampling)
    int T = 0, stop_id = -1, alt_stop_id = -1;
    const int *cmap = nullptr;  // after compaction: activation row r -> caption cmap[r] (nullptr: identity)
};
// caption `row` (not done) emits `tok` at `step`
__device__ __forceinline__ void greedy_emit(const GreedyState &s, int row, int step, int tok, float lp) {
    s.next_tok[row] = tok;
    s.ids[(size_t)row * s.T + step] = tok;
    s.lens[row] = step + 1;
    if (s.logp) s.logp[(size_t)row * s.T + step] = lp;
    if (tok == s.stop_id || tok == s.alt_stop_id) s.done[row] = 1;
    else atomicAdd(s.alive_count, 1);
}
// top_idx / top_val [rows, k], lse [rows]: k = 1 normally; forced [ncap, T] (teacher forcing) and stats [ncap, T, 3] may be nullptr
int launch_greedy_step(hipStream_t st, const GreedyState &s, const int *top_idx, int rows, int step, int k = 1,
                       const int *forced = nullptr, const float *top_val = nullptr, const float *lse = nullptr,
                       float *stats = nullptr);
// sample.hip: one nucleus-sampling decode step over materialised logits [rows, ld], the activation rows row0 .. row0 + rows
// of the step -- writes what greedy_step_kernel writes (plus s.logp).  u [captions, T] (nullptr: Philox keyed by (seed,
// cap_off + caption, step)).
int launch_sample_top_p(hipStream_t st, const GreedyState &s, const float *logits, int ld, int rows, int row0, int V,
                        float inv_temp, float top_p, uint64_t seed, const float *u, int cap_off, int step);
// process.hip: the logits processors (capdec_set_logits_processors) over materialised logits [rows, ld], in place; logits
// row r is activation row row0 + r of the step and finds its history -- hist [captions, beam, T], the first `step` entries
// -- through cmap and beam as the greedy / beam step kernels find their rows.  bias [V] or nullptr.
struct LogitsProc {
    float theta = 1.0f;                    // repetition penalty (1 = off)
    int ngram = 0, min_len = 0, top_k = 0; // 0 = off; top_k acts in the sampling decode only
};
int launch_logits_process(hipStream_t st, float *logits, int ld, int rows, int row0, int V, const int *cmap, int beam,
                          const int *hist, int T, int step, const LogitsProc &p, const float *bias, int stop_id,
                          int alt_stop_id);
// ... logsumexp and the k best of every row, one pass: what launch_topk_merge leaves in lse [rows], top_val / top_idx [rows, k]
int launch_logits_select(hipStream_t st, const float *logits, int ld, int rows, int V, int k, float inv_temp, float *lse,
                         float *top_val, int *top_idx);
// ... everything below a row's top_k-th largest value becomes -inf (no launch when top_k <= 0 or top_k >= V); corr [rows]
// (may be nullptr) receives logsumexp(kept) - logsumexp(all) of the scaled row, which launch_logp_shift adds to the logp
// of the rows that emitted a token at `step`
int launch_logits_topk(hipStream_t st, float *logits, int ld, int rows, int V, int top_k, float inv_temp, float *corr);
int launch_logp_shift(hipStream_t st, const float *corr, int rows, int row0, const int *cmap, const int *lens, int step, int T,
                      float *logp);
// mean over the rows with label != ignore_index of logsumexp(logits[row]) - logits[row][label]; nll_ws: rows floats
int launch_cross_entropy_mean(hipStream_t st, const float *logits, int ld, const int *labels, int rows, int V,
                              int ignore_index, float *nll_ws, float *out);
// cmap[0..count) = indices of the captions with done[c] == 0, ascending; *count = how many (one block)
int launch_compact_alive(hipStream_t st, const uint8_t *done, int ncap, int *cmap, int *count);

// operands clamped to the fp16 range since the last reset, per translation unit (bf16x3.h: g_h2_saturated)
unsigned long long sat_count_gemm_f16x2(bool reset);
unsigned long long sat_count_gemm_h2w(bool reset);
unsigned long long sat_count_gemm_pp(bool reset);
unsigned long long sat_count_gemm_bf16x3(bool reset);
unsigned long long sat_count_elementwise(bool reset);
unsigned long long sat_count_attention(bool reset);
unsigned long long sat_count_resnet(bool reset);

// preprocess.hip: PIL-exact bicubic resize + centre crop + ToTensor + Normalize of a batch of uint8 RGB images
struct ImageDesc {
    long long off;     // byte offset of the image (HWC uint8) in the concatenated pixel buffer
    long long ioff;    // byte offset of its [H][n_px][3] intermediate (after the horizontal pass)
    int H, W;          // input size
    int rh, rw;        // size after Resize
    int top, left;     // crop origin inside the resized image
};
int launch_preprocess(hipStream_t st, const uint8_t *rgb, const ImageDesc *desc, int n, int max_h, int n_px,
                      uint8_t *inter, float *out, const float *mean, const float *stdv);

}  // namespace capdec
