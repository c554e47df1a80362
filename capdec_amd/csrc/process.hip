// Logits processors over materialised logits (capdec_set_logits_processors / capdec_set_logit_bias): what the decode loop
// runs between the plain lm_head GEMM and the selection when a processor or a bias is set (decode.hip: lm_head_rows).
//
// At step i a row has raw logits l[0..V) (before the division by the temperature) and a history g = (g_0 .. g_{i-1}): the
// tokens its own hypothesis has generated so far -- the caption's `ids` (greedy, sampling) or that beam's row of
// BeamState::tokens after the previous step's re-ordering.  In this order:
//   1. repetition penalty theta: for every DISTINCT j in g, l[j] <- l[j] / theta if l[j] > 0 else l[j] * theta
//   2. bias: l <- l + b (entries finite or -inf)
//   3. no-repeat n-grams of size m: if i >= m - 1, for every s with g[s .. s+m-2] == g[i-m+1 .. i-1]: l[g[s+m-1]] <- -inf
//   4. minimum length: if i < min_length, l[stop_id] <- -inf (and l[alt_stop_id] where the call has one)
//   5. top_k (sampling only): j stays iff fewer than top_k entries are strictly greater than l[j]; the rest become -inf
//
// logits_process_kernel   steps 1-4 in place, one workgroup per row
// logits_select_kernel<K> logsumexp and the K best (value, column) pairs of a row in ONE pass over it (row_select.h's
//                         logits_row_pass with nothing banned and nothing excluded) -- exactly what
//                         launch_topk_merge (select.hip) leaves in lse / top_val / top_idx: values scaled by inv_temp, ties
//                         to the smaller column -- so the greedy / beam step kernels run unchanged behind it
// logits_topk_kernel      step 5 in place: the top_k-th largest value by a count-based bisection over the order-preserving
//                         integer image of the floats; launch_sample_top_p runs unchanged on the row it leaves
//
// Every sum has a fixed order (a lane's elements in index order, the wavefront's DPP tree, the wavefronts in order) and one
// workgroup owns a row whatever the launch holds: a row's result does not depend on the launch size, the row blocks, the
// chunking or the compaction of the batch.  The ld - V pad columns of a row are never read or written.
// The candidate lists, the winner-pops round, the tie rule, order_key and the workgroup reductions are row_select.h's: the
// ones launch_topk_merge and the sampling kernel use.
#include "row_select.h"

namespace capdec {

namespace {

constexpr int PRC_THREADS = 256;
constexpr int PRC_HIST_MAX = 1024;      // entry_length <= 1024 (decode_call_checks)
constexpr int TOPK_THREADS = 1024, TOPK_WAVES = TOPK_THREADS / WAVE;

// history row of logits row r of a block: activation row row0 + r of the step, exactly as greedy_step_kernel (beam == 1)
// and beam_step_kernel find their rows
__device__ __forceinline__ const int *history_of(const int *hist, int row0, int r, const int *cmap, int beam, int T) {
    const int R = row0 + r;
    const int cap = cmap ? cmap[R / beam] : R / beam;
    return hist + ((size_t)cap * beam + R % beam) * T;
}

__global__ __launch_bounds__(PRC_THREADS) void logits_process_kernel(float *__restrict__ logits, int ld, int V, int row0,
                                                                     const int *__restrict__ cmap, int beam,
                                                                     const int *__restrict__ hist, int T, int step,
                                                                     LogitsProc p, const float *__restrict__ bias,
                                                                     int stop_id, int alt_stop_id) {
    __shared__ int g[PRC_HIST_MAX];
    const int r = blockIdx.x, tid = threadIdx.x;
    float *x = logits + (size_t)r * ld;
    const int n = step < PRC_HIST_MAX ? step : PRC_HIST_MAX;         // history length
    if (n > 0) {
        const int *h = history_of(hist, row0, r, cmap, beam, T);
        for (int s = tid; s < n; s += PRC_THREADS) g[s] = h[s];
    }
    __syncthreads();
    // 1. the first occurrence of a token penalises it: one thread per distinct token, so no two threads touch one logit
    if (p.theta != 1.0f) {
        for (int s = tid; s < n; s += PRC_THREADS) {
            const int tok = g[s];
            bool first = (unsigned)tok < (unsigned)V;
            for (int q = 0; q < s && first; ++q) first = g[q] != tok;
            if (first) {
                const float l = x[tok];
                x[tok] = l > 0.f ? l / p.theta : l * p.theta;
            }
        }
    }
    __syncthreads();
    // 2. the bias streams the row (rows and the bias are 16-byte aligned: ld is a multiple of 64)
    if (bias) {
        const int V4 = V & ~3;
        for (int j = tid * 4; j < V4; j += PRC_THREADS * 4) {
            float4 a = *reinterpret_cast<const float4 *>(x + j);
            const float4 b = *reinterpret_cast<const float4 *>(bias + j);
            a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
            *reinterpret_cast<float4 *>(x + j) = a;
        }
        for (int j = V4 + tid; j < V; j += PRC_THREADS) x[j] += bias[j];
    }
    __syncthreads();
    // 3. / 4. the bans (several threads may write the same -inf)
    const int m = p.ngram;
    if (m > 0 && n >= m - 1) {
        for (int s = tid; s + m <= n; s += PRC_THREADS) {
            bool eq = true;
            for (int q = 0; q < m - 1 && eq; ++q) eq = g[s + q] == g[n - m + 1 + q];
            const int tok = g[s + m - 1];
            if (eq && (unsigned)tok < (unsigned)V) x[tok] = -INFINITY;
        }
    }
    if (tid == 0 && step < p.min_len) {
        if ((unsigned)stop_id < (unsigned)V) x[stop_id] = -INFINITY;
        if ((unsigned)alt_stop_id < (unsigned)V) x[alt_stop_id] = -INFINITY;
    }
}

template <int K>
__global__ __launch_bounds__(PRC_THREADS) void logits_select_kernel(const float *__restrict__ logits, int ld, int V,
                                                                    float inv_temp, float *__restrict__ lse,
                                                                    float *__restrict__ top_val, int *__restrict__ top_idx) {
    const size_t r = blockIdx.x;
    logits_row_pass<K, PRC_THREADS>(logits + r * ld, V, inv_temp, RowUnfiltered(), lse + r, top_val + r * K, top_idx + r * K);
}

// tau = the largest key with at least top_k keys >= tau: the top_k-th largest value, built bit by bit from the top (32
// counting passes over the row, which stays in L2).  Entries below it become -inf, ties at the boundary stay.
// corr (may be nullptr): corr[r] = logsumexp(kept) - logsumexp(all) of the temperature-scaled row -- what the sampling
// kernel's logp, taken on the filtered row, lacks to be the log-probability under the distribution before top_k.
__global__ __launch_bounds__(TOPK_THREADS) void logits_topk_kernel(float *__restrict__ logits, int ld, int V, int top_k,
                                                                   float inv_temp, float *__restrict__ corr) {
    __shared__ int cred[2 * TOPK_WAVES];
    __shared__ float fred[2 * TOPK_WAVES];
    const int r = blockIdx.x, tid = threadIdx.x;
    float *x = logits + (size_t)r * ld;
    uint32_t tau = 0u;
    int par = 0;
    for (int bit = 31; bit >= 0; --bit) {
        const uint32_t cand = tau | (1u << bit);
        int cnt = 0;
        for (int j = tid; j < V; j += TOPK_THREADS) cnt += order_key(x[j]) >= cand ? 1 : 0;
        cnt = block_count<TOPK_WAVES>(cnt, cred, par);
        par ^= 1;
        if (cnt >= top_k) tau = cand;
    }
    if (corr) {
        float m = -INFINITY;
        for (int j = tid; j < V; j += TOPK_THREADS) m = fmaxf(m, x[j] * inv_temp);
        m = block_max<TOPK_WAVES>(m, fred, 0);
        float all = 0.f, kept = 0.f;
        for (int j = tid; j < V; j += TOPK_THREADS) {
            const float v = x[j], e = expf(v * inv_temp - m);
            all += e;
            kept += order_key(v) >= tau ? e : 0.f;
        }
        all = block_sum<TOPK_WAVES>(all, fred, 1);
        kept = block_sum<TOPK_WAVES>(kept, fred, 0);
        if (tid == 0) corr[r] = logf(kept) - logf(all);
    }
    __syncthreads();                                             // every read of the row is behind us
    for (int j = tid; j < V; j += TOPK_THREADS)
        if (order_key(x[j]) < tau) x[j] = -INFINITY;
}

// logp of the rows that emitted a token at `step`: from the filtered row's normaliser to the unfiltered one's
__global__ void logp_shift_kernel(const float *__restrict__ corr, int rows, int row0, const int *__restrict__ cmap,
                                  const int *__restrict__ lens, int step, int T, float *__restrict__ logp) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    const int row = cmap ? cmap[row0 + r] : row0 + r;
    if (lens[row] == step + 1) logp[(size_t)row * T + step] += corr[r];
}

}  // namespace

int launch_logits_process(hipStream_t st, float *logits, int ld, int rows, int row0, int V, const int *cmap, int beam,
                          const int *hist, int T, int step, const LogitsProc &p, const float *bias, int stop_id,
                          int alt_stop_id) {
    if (rows <= 0) return 0;
    CAPDEC_CHECK(ld >= V && ld % 4 == 0 && beam >= 1 && step >= 0 && step < T && T <= PRC_HIST_MAX && (step == 0 || hist),
                 "logits_process: bad geometry");
    hipLaunchKernelGGL(logits_process_kernel, dim3(rows), dim3(PRC_THREADS), 0, st, logits, ld, V, row0, cmap, beam, hist, T,
                       step, p, bias, stop_id, alt_stop_id);
    CAPDEC_HIP(hipGetLastError());
    return 0;
}

int launch_logits_select(hipStream_t st, const float *logits, int ld, int rows, int V, int k, float inv_temp, float *lse,
                         float *top_val, int *top_idx) {
    if (rows <= 0) return 0;
    CAPDEC_CHECK(ld >= V && ld % 4 == 0 && V >= k, "logits_select: bad geometry");
    CAPDEC_TRY(with_topk_k(k, "logits_select", [&](auto KS) {
        hipLaunchKernelGGL(logits_select_kernel<KS>, dim3(rows), dim3(PRC_THREADS), 0, st, logits, ld, V, inv_temp, lse, top_val,
                           top_idx);
    }));
    CAPDEC_HIP(hipGetLastError());
    return 0;
}

int launch_logits_topk(hipStream_t st, float *logits, int ld, int rows, int V, int top_k, float inv_temp, float *corr) {
    if (rows <= 0 || top_k <= 0 || top_k >= V) return 0;         // nothing to remove
    CAPDEC_CHECK(ld >= V, "logits_topk: bad geometry");
    hipLaunchKernelGGL(logits_topk_kernel, dim3(rows), dim3(TOPK_THREADS), 0, st, logits, ld, V, top_k, inv_temp, corr);
    CAPDEC_HIP(hipGetLastError());
    return 0;
}

int launch_logp_shift(hipStream_t st, const float *corr, int rows, int row0, const int *cmap, const int *lens, int step, int T,
                      float *logp) {
    if (rows <= 0) return 0;
    hipLaunchKernelGGL(logp_shift_kernel, dim3((rows + 255) / 256), dim3(256), 0, st, corr, rows, row0, cmap, lens, step, T, logp);
    CAPDEC_HIP(hipGetLastError());
    return 0;
}

}  // namespace capdec
