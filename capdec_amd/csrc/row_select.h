// Device primitives for rows of logits, shared by everything that ends a decode step (select.hip, process.hip, sample.hip,
// and through beam_state.h the beam variants): the tie rule, the wavefront's arg-best butterfly, a lane's descending list of
// K candidates, the wavefront round that pops the best of the lanes' heads, the row logsumexp from per-tile partials, the
// online (max, sum exp) rescale, the one pass over a row of materialised logits (logsumexp + its K best, under a policy
// that may ban a column and keep columns off the list), the order-preserving integer image of a float and the workgroup
// reductions.  ONE definition of each: the tie rule and the summation orders written here are what keeps beam results
// equal to the reference's, and results independent of batch, chunking and compaction.
#pragma once
#include "common.h"

namespace capdec {

// the tie rule: larger value, then smaller column
__device__ __forceinline__ bool better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

// the arg-best butterfly: (gv, gi) <- the best of the 64 lanes' pairs, in every lane
__device__ __forceinline__ void wave_best(float &gv, int &gi) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(gv, o, 64);
        const int oi = __shfl_xor(gi, o, 64);
        if (better(ov, oi, gv, gi)) { gv = ov; gi = oi; }
    }
}

// a lane's K best (value, column) pairs, descending under `better`; empty slots are (-inf, 0x7fffffff)
template <int K>
struct LaneTopk {
    float v[K];
    int i[K];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int j = 0; j < K; ++j) { v[j] = -INFINITY; i[j] = 0x7fffffff; }
    }
    __device__ __forceinline__ void push(float cv, int ci) {
        if (!better(cv, ci, v[K - 1], i[K - 1])) return;       // (a shortcut only: nothing below would move)
#pragma unroll
        for (int j = 0; j < K; ++j) {
            if (better(cv, ci, v[j], i[j])) {
                const float tv = v[j]; const int ti = i[j];
                v[j] = cv; i[j] = ci; cv = tv; ci = ti;
            }
        }
    }
    // one round over the wavefront: (gv, gi) = the best of the 64 lanes' heads, in every lane; the lane that held it pops it
    __device__ __forceinline__ void pop_best(float &gv, int &gi) {
        gv = v[0];
        gi = i[0];
        wave_best(gv, gi);
        if (gi == i[0] && gv == v[0]) {
#pragma unroll
            for (int j = 0; j + 1 < K; ++j) { v[j] = v[j + 1]; i[j] = i[j + 1]; }
            v[K - 1] = -INFINITY; i[K - 1] = 0x7fffffff;
        }
    }
};

// logsumexp of a row from its tiles' (max, sum exp(x - max)) pairs, by one wavefront (the same value in every lane)
__device__ __forceinline__ float tile_logsumexp(const float *__restrict__ tile_max, const float *__restrict__ tile_sum,
                                                int ntiles, int lane) {
    float m = -INFINITY;
    for (int t = lane; t < ntiles; t += 64) m = fmaxf(m, tile_max[t]);
    m = wave_max(m);
    float s = 0.f;
    for (int t = lane; t < ntiles; t += 64) s += tile_sum[t] * expf(tile_max[t] - m);
    s = wave_sum(s);
    return m + logf(s);
}

// running (max, sum exp(x - max)) of a lane over one more group of values whose maximum is gm
__device__ __forceinline__ void online_rescale(float &m, float &s, float gm) {
    if (gm > m) {
        s = m > -INFINITY ? s * expf(m - gm) : 0.f;
        m = gm;
    }
}

// ---- one pass of a THREADS-thread workgroup over a row x[0..V) of materialised logits: logsumexp of the row scaled by
// inv_temp -> *lse, and its K best (value, column) pairs under the tie rule -> out_val / out_idx [K], both written by thread
// 0.  Per lane an online (max, sum exp) and a LaneTopk, then K winner-pops rounds per wavefront and thread 0's merge of the
// wavefronts' lists; every sum in a fixed order (a lane's elements in index order, the DPP tree, the wavefronts in order).
// The policy is a compile-time type: `filtered` = false drops the ban and the exclusion from the loop altogether.
struct RowUnfiltered {                  // every column counts and may be listed
    static constexpr bool filtered = false;
    static constexpr int ban = -1;
    __device__ __forceinline__ bool excluded(int) const { return false; }
};
template <int K, int THREADS, class Policy>
__device__ __forceinline__ void logits_row_pass(const float *__restrict__ x, int V, float inv_temp, const Policy &pol,
                                                float *__restrict__ lse, float *__restrict__ out_val,
                                                int *__restrict__ out_idx) {
    constexpr int WAVES = THREADS / WAVE;
    __shared__ float wm[WAVES], ws[WAVES];
    __shared__ float cv[WAVES * K];
    __shared__ int ci[WAVES * K];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    float m = -INFINITY, s = 0.f;
    LaneTopk<K> best;
    best.clear();
    auto offer = [&](float v, int j) {
        if (Policy::filtered && pol.excluded(j)) return;
        best.push(v, j);
    };
    const int V4 = V & ~3;
    for (int j = tid * 4; j < V4; j += THREADS * 4) {
        const float4 q = *reinterpret_cast<const float4 *>(x + j);
        float v0 = q.x * inv_temp, v1 = q.y * inv_temp, v2 = q.z * inv_temp, v3 = q.w * inv_temp;
        if (Policy::filtered && (unsigned)(pol.ban - j) < 4u) {     // the banned column (-1: none) counts as -inf
            if (pol.ban == j) v0 = -INFINITY;
            if (pol.ban == j + 1) v1 = -INFINITY;
            if (pol.ban == j + 2) v2 = -INFINITY;
            if (pol.ban == j + 3) v3 = -INFINITY;
        }
        online_rescale(m, s, fmaxf(fmaxf(v0, v1), fmaxf(v2, v3)));
        if (m > -INFINITY) s += ((expf(v0 - m) + expf(v1 - m)) + expf(v2 - m)) + expf(v3 - m);
        offer(v0, j);
        offer(v1, j + 1);
        offer(v2, j + 2);
        offer(v3, j + 3);
    }
    for (int j = V4 + tid; j < V; j += THREADS) {
        const float v = Policy::filtered && j == pol.ban ? -INFINITY : x[j] * inv_temp;
        online_rescale(m, s, v);
        if (m > -INFINITY) s += expf(v - m);
        offer(v, j);
    }
    // logsumexp: lanes -> wavefront -> workgroup, each in a fixed order
    const float M = wave_max(m);
    const float t = wave_sum(m > -INFINITY ? s * expf(m - M) : 0.f);
    if (lane == 0) { wm[wave] = M; ws[wave] = t; }
    // the wavefront's K best: K rounds of the arg-best butterfly, the lane that held the winner pops it
#pragma unroll
    for (int q = 0; q < K; ++q) {
        float gv;
        int gi;
        best.pop_best(gv, gi);
        if (lane == 0) { cv[wave * K + q] = gv; ci[wave * K + q] = gi; }
    }
    __syncthreads();
    if (tid != 0) return;
    float Mb = wm[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) Mb = fmaxf(Mb, wm[w]);
    float S = 0.f;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) S += wm[w] > -INFINITY ? ws[w] * expf(wm[w] - Mb) : 0.f;
    *lse = Mb + logf(S);
    best.clear();
    for (int q = 0; q < WAVES * K; ++q) best.push(cv[q], ci[q]);
#pragma unroll
    for (int j = 0; j < K; ++j) { out_val[j] = best.v[j]; out_idx[j] = best.i[j]; }
}

// order-preserving integer image of a float (-0 counts as +0: the two compare equal)
__device__ __forceinline__ uint32_t order_key(float f) {
    if (f == 0.f) f = 0.f;
    const uint32_t b = __float_as_uint(f);
    return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}

// Reductions over a workgroup of WAVES wavefronts, the same value in every thread: the wavefront's DPP tree (common.h), then
// the wavefronts in index order.  `red` holds 2 x WAVES entries and successive calls alternate `par`, so that one barrier
// per call is enough.
template <int WAVES>
__device__ __forceinline__ float block_sum(float v, float *red, int par) {
    v = wave_sum(v);
    float *r = red + par * WAVES;
    if ((threadIdx.x & (WAVE - 1)) == 0) r[threadIdx.x / WAVE] = v;
    __syncthreads();
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) t += r[w];
    return t;
}
template <int WAVES>
__device__ __forceinline__ float block_max(float v, float *red, int par) {
    v = wave_max(v);
    float *r = red + par * WAVES;
    if ((threadIdx.x & (WAVE - 1)) == 0) r[threadIdx.x / WAVE] = v;
    __syncthreads();
    float t = r[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) t = fmaxf(t, r[w]);
    return t;
}
template <int WAVES>
__device__ __forceinline__ int block_count(int v, int *red, int par) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    int *r = red + par * WAVES;
    if ((threadIdx.x & (WAVE - 1)) == 0) r[threadIdx.x / WAVE] = v;
    __syncthreads();
    int t = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) t += r[w];
    return t;
}

}  // namespace capdec
