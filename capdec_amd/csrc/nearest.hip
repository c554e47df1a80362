// capdec_nearest_tokens: the k table rows nearest to every query row under cosine similarity, with the [rows, table_rows]
// similarity matrix never in HBM -- the "prefix interpretation" of reference gpt2_prefix_eval.py:247-251 (and :233-234) against
// the normalised embedding table of :259-260.
//
// Contract (include/capdec.h; tests/nearest_def.py restates it in fp64).  xn = x / max(||x||_2, 1e-12), tn likewise,
// sim[r, j] = <xn[r], tn[j]>; ids[r, 0..k) = the k largest, descending, equal sims in ascending id order.
//
// Path:
//   launch_l2norm_rows   BOTH operands are normalised before the product (elementwise.hip): every GEMM operand lies in
//                        [-1, 1], whatever the norms of trained prefixes are.  The query rows go straight into the packed A
//                        operand where the mode has one (topk_packed_a); the table becomes fp32 unit rows that planes_of packs.
//   gemm_topk            the fused top-k GEMM of the lm_head without its LayerNorm + launch_topk_merge (gemm_dispatch.hip)
//   nearest_fix_kernel   the rows the normalising pass flagged (a NaN or an inf): ids -1, sims NaN
// in blocks of NEAREST_ROWS query rows (the per-tile candidate lists of 50 257 columns at k = 8 are 28 KB per row).
//
// The table.  d_table == NULL means the loaded GPT-2's wte: its unit rows are kept as an fp32 copy (c->wte_n, built on first
// use) whose operand planes planes_of caches like any weight's; capdec_load_gpt2, capdec_destroy and a train step that
// moves wte drop both (drop_wte_norm).  A caller's table is normalised into c->n_tab on every call and never cached: the
// plane cache is keyed by address, and callers' allocators recycle addresses.
#include "context.h"

namespace capdec {

namespace {

constexpr int NEAREST_ROWS = 16384;      // query rows per block: a compile-time constant, not a knob

__global__ void nearest_fix_kernel(const int *__restrict__ row_bad, int rows, int k, int32_t *__restrict__ ids,
                                   float *__restrict__ sims) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * k || !row_bad[i / k]) return;
    ids[i] = -1;
    if (sims) sims[i] = __builtin_nanf("");
}

// unit rows of `table` -> out (fp32 [n, d]); fails, before anything else runs, when a row holds a NaN or an inf
int normalize_table(capdec_ctx *c, const float *table, int n, int d, float *out) {
    int *flag = c->n_bad.as<int>();
    CAPDEC_HIP(hipMemsetAsync(flag, 0, sizeof(int), c->stream));
    { ProfScope ps(c, F_PACK); CAPDEC_TRY(launch_l2norm_rows(c->stream, table, nullptr, out, n, d, 0, nullptr, flag)); }
    int bad = 0;
    CAPDEC_HIP(hipMemcpyAsync(&bad, flag, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    CAPDEC_HIP(hipStreamSynchronize(c->stream));
    CAPDEC_CHECK(bad == 0, "nearest_tokens: a table row holds a NaN or an inf");
    return 0;
}

int nearest_run(capdec_ctx *c, const float *x, int rows, int d, const float *table, int n, int k, int32_t *ids, float *sims) {
    CAPDEC_TRY(c->n_bad.ensure(((size_t)NEAREST_ROWS + 1) * sizeof(int)));
    const float *tn = nullptr;
    if (!table) {
        if (!c->wte_n_valid) {
            drop_planes_of(c, c->wte_n.p);      // (a grown buffer changes its address)
            CAPDEC_TRY(c->wte_n.ensure((size_t)n * d * 4));
            CAPDEC_TRY(normalize_table(c, c->gpt.wte, n, d, c->wte_n.as<float>()));
            c->wte_n_valid = true;
        }
        tn = c->wte_n.as<float>();
    } else {
        CAPDEC_TRY(c->n_tab.ensure((size_t)n * d * 4));
        CAPDEC_TRY(normalize_table(c, table, n, d, c->n_tab.as<float>()));
        tn = c->n_tab.as<float>();
    }
    const bool packed = topk_packed_a(c, d);
    const int blk = std::min(rows, NEAREST_ROWS), nt = gemm_tiles_n(n);
    if (packed) CAPDEC_TRY(c->xpk.ensure(x3_packed_bytes(blk, d, PK_F16X2)));
    else CAPDEC_TRY(c->xl.ensure((size_t)blk * d * 4));
    TopkOut o;
    CAPDEC_TRY(topk_workspace(c, blk, nt, k, &o));
    if (!sims) CAPDEC_TRY(c->topv.ensure((size_t)blk * k * 4));
    int *row_bad = c->n_bad.as<int>() + 1;
    for (int r0 = 0; r0 < rows; r0 += NEAREST_ROWS) {
        const int nr = std::min(NEAREST_ROWS, rows - r0);
        const float *xb = x + (size_t)r0 * d;
        {
            ProfScope ps(c, F_PACK);
            CAPDEC_TRY(launch_l2norm_rows(c->stream, xb, packed ? c->xpk.p : nullptr, packed ? nullptr : c->xl.as<float>(), nr, d,
                                          PK_F16X2, row_bad, nullptr));
        }
        int32_t *ib = ids + (size_t)r0 * k;
        float *sb = sims ? sims + (size_t)r0 * k : nullptr;
        CAPDEC_TRY(gemm_topk(c, packed ? c->xpk.p : c->xl.p, tn, /*cache=*/!table, /*b_small=*/true, nr, n, d, k, o,
                             c->lse.as<float>(), sb ? sb : c->topv.as<float>(), ib));
        ProfScope ps(c, F_SELECT);
        hipLaunchKernelGGL(nearest_fix_kernel, dim3((nr * k + 255) / 256), dim3(256), 0, c->stream, row_bad, nr, k, ib, sb);
        CAPDEC_HIP(hipGetLastError());
    }
    return 0;
}

}  // namespace

void drop_wte_norm(capdec_ctx *c) {
    drop_planes_of(c, c->wte_n.p);
    c->wte_n_valid = false;
}

}  // namespace capdec

using namespace capdec;

extern "C" int capdec_nearest_tokens(capdec_ctx *c, const float *x, int rows, int d, const float *table, int table_rows, int k,
                                     int32_t *ids, float *sims) {
    CAPDEC_CHECK(c, "nearest_tokens: null context");
    CAPDEC_CHECK(d >= 32 && d % 32 == 0 && d <= 1024, "nearest_tokens: d must be a multiple of 32, at most 1024");
    CAPDEC_CHECK(rows >= 0, "nearest_tokens: negative row count");
    if (!table) {
        CAPDEC_CHECK(c->gpt.loaded, "nearest_tokens: no table given and GPT-2 weights not loaded");
        CAPDEC_CHECK(d == c->gpt.d, "nearest_tokens: d is not the loaded GPT-2's n_embd");
        table_rows = c->gpt.vocab;
    }
    CAPDEC_CHECK(table_rows >= 1, "nearest_tokens: empty table");
    CAPDEC_CHECK(k >= 1 && k <= TOPK_MAX, "nearest_tokens: k must be in 1..8");
    CAPDEC_CHECK(k <= table_rows, "nearest_tokens: k exceeds the table's rows");
    if (rows == 0) return 0;
    CAPDEC_CHECK(x && ids, "nearest_tokens: null argument");
    CAPDEC_CHECK((((uintptr_t)x | (uintptr_t)table) & 15) == 0, "nearest_tokens: x and the table must be 16-byte aligned");
    CAPDEC_HIP(hipSetDevice(c->device));
    const int rc = nearest_run(c, x, rows, d, table, table_rows, k, ids, sims);
    if (hipStreamSynchronize(c->stream) != hipSuccess && rc == 0) {
        set_error("nearest_tokens: hipStreamSynchronize failed");
        return 1;
    }
    return rc;
}
