// Device primitives for rows of logits, shared by everything that ends a decode step (select.hip, process.hip, sample.hip):
// the tie rule, a lane's descending list of K candidates, the wavefront round that pops the best of the lanes' heads, the
// row logsumexp from per-tile partials, the online (max, sum exp) rescale, the order-preserving integer image of a float
// and the workgroup reductions.  ONE definition of each: the tie rule and the summation orders written here are what
// keeps beam results equal to the reference's, and results independent of batch, chunking and compaction.
#pragma once
#include "common.h"

namespace capdec {

// the tie rule: larger value, then smaller column
__device__ __forceinline__ bool better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

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
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(gv, o, 64);
            const int oi = __shfl_xor(gi, o, 64);
            if (better(ov, oi, gv, gi)) { gv = ov; gi = oi; }
        }
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
