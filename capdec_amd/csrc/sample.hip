// Nucleus (top-p) sampling over materialised logits: one 1024-thread workgroup owns one row and finishes it.
//
// For a row of logits l[0..V), temperature t and nucleus top_p, with s = l / t and p = softmax(s):
//   token j is in the nucleus iff it is the arg-max or A(j) <= top_p, A(j) = sum of p[i] over p[i] > p[j]
//   (reference gpt2_prefix_eval.py:166-175: sort descending, drop where the cumulative sum BEFORE the token exceeds
//   top_p, never drop the first); q = p restricted to the nucleus, renormalised; the pick is the first j in ascending
//   token-id order whose running sum of q exceeds the uniform u (the last nucleus token when rounding leaves the total
//   below u); logp = s[pick] - logsumexp(s).
//
// The row is read from HBM once: lane `tid` keeps e[i] = exp(s[tid + 1024 i] - max) in registers (50 values at GPT-2's
// vocabulary).  e lies in [0, 1], so its bit pattern is its order-preserving integer image, and the nucleus is
// {e >= tau} with tau the smallest key k for which the mass strictly above k is <= top_p * sum(e): a bisection over the
// 30 significant bits of k, one block reduction per step.  Rows whose arg-max alone carries more than top_p (and every
// row at top_p <= 0) leave after the two opening reductions; rows at top_p >= 1 skip the bisection (tau = 0).
//
// Every sum has a fixed order -- a lane's registers in index order, the wavefront's DPP tree, the 16 wavefronts in order
// (row_select.h: block_sum / block_max), and for the pick the 64-token segments in id order -- and one workgroup owns a row
// whatever the launch holds, so a row's result does not depend on the launch size, the chunking or the compaction of the
// batch.  A pick is written by greedy_emit (common.h), as the arg-max of the greedy step is.
#include "row_select.h"

namespace capdec {

namespace {

constexpr int SMP_THREADS = 1024, SMP_WAVES = SMP_THREADS / WAVE;

// inclusive prefix sum over the 64 lanes of a wavefront, in lane order
__device__ __forceinline__ float wave_scan(float v) {
    const int lane = threadIdx.x & (WAVE - 1);
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const float t = __shfl_up(v, o, WAVE);
        if (lane >= o) v += t;
    }
    return v;
}

// [0, 1) like torch.rand; counter = (caption index within the call, step), stream 2 (0 / 1: the noise injection's)
__device__ __forceinline__ float sample_uniform(uint64_t seed, uint32_t caption, uint32_t step) {
    uint32_t o[4];
    philox4x32(caption, 0u, step, 2u, (uint32_t)seed, (uint32_t)(seed >> 32), o);
    return (float)(o[0] >> 8) * (1.0f / 16777216.0f);
}

// The scaled logit and exp(s - max) of one value.  Every pass of the kernel goes through these two, and they are kept from
// contracting into an fma, so that a value compared with tau in the pick is bit for bit the value tau was found on (and
// the arg-max is exactly 1.0 in every pass) whatever the temperature.
__device__ __forceinline__ float scaled_logit(float x, float inv_temp) {
#pragma clang fp contract(off)
    return x * inv_temp;
}
__device__ __forceinline__ float exp_shifted(float s, float m) {
#pragma clang fp contract(off)
    const float d = s - m;
    return __expf(d);
}

// NV > 0: the row (V <= 1024 NV) lives in registers; NV == 0: any V, every pass re-reads the row (from L2)
template <int NV>
__global__ __launch_bounds__(SMP_THREADS) void sample_top_p_kernel(const float *__restrict__ logits, int ld, int V,
                                                                   int row0, float inv_temp, float top_p, uint64_t seed,
                                                                   const float *__restrict__ u_in, int cap_off, int step,
                                                                   GreedyState o) {
    __shared__ float red[2 * SMP_WAVES];
    __shared__ float seg[(NV > 0 ? NV : 1) * SMP_WAVES];
    __shared__ float pick_rem;
    __shared__ int pick_seg;
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const int row = o.cmap ? o.cmap[row0 + r] : row0 + r;        // caption (logits row r = activation row row0 + r of the step)
    if (o.done[row]) return;                                     // (uniform over the workgroup: nothing below runs)
    const float *x = logits + (size_t)r * ld;
    const int nv = NV > 0 ? NV : (V + SMP_THREADS - 1) / SMP_THREADS;
    float e[NV > 0 ? NV : 1];
    // value i of this lane: the scaled logit before `m` is known, exp(s - m) afterwards
    auto scaled = [&](int i) { const int j = tid + i * SMP_THREADS; return j < V ? scaled_logit(x[j], inv_temp) : -INFINITY; };

    float m = -INFINITY;
    if constexpr (NV > 0) {
#pragma unroll
        for (int i = 0; i < NV; ++i) e[i] = scaled(i);
#pragma unroll
        for (int i = 0; i < NV; ++i) m = fmaxf(m, e[i]);
    } else {
        for (int i = 0; i < nv; ++i) m = fmaxf(m, scaled(i));
    }
    m = block_max<SMP_WAVES>(m, red, 0);
    auto val = [&](int i) {
        if constexpr (NV > 0) return e[i];
        else return exp_shifted(scaled(i), m);
    };
    float s = 0.f, nmax = 0.f;
    if constexpr (NV > 0) {
#pragma unroll
        for (int i = 0; i < NV; ++i) e[i] = exp_shifted(e[i], m);
    }
#pragma unroll
    for (int i = 0; i < nv; ++i) {
        const float v = val(i);
        s += v;
        nmax += v == 1.0f ? 1.f : 0.f;
    }
    const float S = block_sum<SMP_WAVES>(s, red, 1);
    nmax = block_sum<SMP_WAVES>(nmax, red, 0);
    const float bound = top_p * S;                               // nucleus: mass strictly above the token <= bound
    const float lse = m + __logf(S);

    if (nmax == 1.f && !(nmax <= bound)) {                       // the arg-max alone is the nucleus: whatever u is
#pragma unroll
        for (int i = 0; i < nv; ++i)
            if (val(i) == 1.0f) greedy_emit(o, row, step, tid + i * SMP_THREADS, m - lse);
        return;
    }

    // tau = the smallest key whose strictly-greater mass is <= bound (monotone in the key; true at the arg-max's key
    // whenever nmax <= bound -- otherwise the tied arg-maxes are the nucleus)
    uint32_t lo = 0u, hi = 0x3f800000u;                          // keys of e = 0 and e = 1
    if (!(nmax <= bound)) lo = hi;
    else if (bound >= S) hi = 0u;
    int par = 1;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        float a = 0.f;
#pragma unroll
        for (int i = 0; i < nv; ++i) {
            const float v = val(i);
            a += __float_as_uint(v) > mid ? v : 0.f;
        }
        a = block_sum<SMP_WAVES>(a, red, par);
        par ^= 1;
        if (a <= bound) hi = mid;
        else lo = mid + 1;
    }
    const uint32_t tau = lo;

    // ---- the pick: the nucleus mass of every 64-token segment (ids 1024 i + 64 wave + lane: segment 16 i + wave, in id
    // order), a scan over the segments by wavefront 0, then a scan inside the segment the target falls into
    const float uu = u_in ? u_in[(size_t)row * o.T + step] : sample_uniform(seed, (uint32_t)(cap_off + row), (uint32_t)step);
    auto nucleus = [&](int i) { const float v = val(i); return __float_as_uint(v) >= tau ? v : 0.f; };
    if constexpr (NV > 0) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const float w = wave_sum(nucleus(i));
            if (lane == 0) seg[i * SMP_WAVES + wave] = w;
        }
        __syncthreads();
        if (wave == 0) {
            constexpr int NSEG = NV * SMP_WAVES, PER = (NSEG + WAVE - 1) / WAVE;
            float part = 0.f;
            for (int k = 0; k < PER; ++k) {
                const int g = lane * PER + k;
                if (g < NSEG) part += seg[g];
            }
            const float incl = wave_scan(part);
            const float Z = __shfl(incl, WAVE - 1, WAVE);
            const float target = uu * Z;
            float run = incl - part;                             // mass before this lane's first segment
            int found = -1, last = -1;
            float rem = 0.f;
            for (int k = 0; k < PER; ++k) {
                const int g = lane * PER + k;
                if (g >= NSEG) break;
                const float w = seg[g];
                if (w > 0.f) last = g;
                if (found < 0 && w > 0.f && run + w > target) { found = g; rem = target - run; }
                run += w;
            }
            const unsigned long long hit = __ballot(found >= 0);
            if (hit) {
                if (lane == __ffsll((long long)hit) - 1) { pick_seg = found; pick_rem = rem; }
            } else {                                             // rounding left the total at or below the target
                const unsigned long long any = __ballot(last >= 0);
                if (lane == 63 - __clzll((long long)any)) { pick_seg = last; pick_rem = INFINITY; }
            }
        }
        __syncthreads();
        const int g = pick_seg;
        if (wave != (g & (SMP_WAVES - 1))) return;
        const int gi = g / SMP_WAVES;
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i)
            if (i == gi) q = nucleus(i);
        const float incl = wave_scan(q);
        const unsigned long long hit = __ballot(q > 0.f && incl > pick_rem), any = __ballot(q > 0.f);
        const int pl = hit ? __ffsll((long long)hit) - 1 : 63 - __clzll((long long)any);
        if (lane == pl) {
            const int tok = gi * SMP_THREADS + tid;
            greedy_emit(o, row, step, tok, scaled_logit(x[tok], inv_temp) - lse);
        }
    } else {
        // any vocabulary: wavefront 0 walks the row in id order, 64 tokens at a time
        if (wave != 0) return;
        float Z = 0.f;
        for (int j0 = 0; j0 < V; j0 += WAVE) {
            const int j = j0 + lane;
            const float v = j < V ? exp_shifted(scaled_logit(x[j], inv_temp), m) : 0.f;
            Z += wave_sum(__float_as_uint(v) >= tau && j < V ? v : 0.f);
        }
        const float target = uu * Z;
        float run = 0.f;
        int tok = -1, last = -1;
        for (int j0 = 0; j0 < V && tok < 0; j0 += WAVE) {
            const int j = j0 + lane;
            const float v = j < V ? exp_shifted(scaled_logit(x[j], inv_temp), m) : 0.f;
            const float q = __float_as_uint(v) >= tau && j < V ? v : 0.f;
            const float incl = wave_scan(q);
            const unsigned long long hit = __ballot(q > 0.f && run + incl > target), any = __ballot(q > 0.f);
            if (hit) tok = j0 + __ffsll((long long)hit) - 1;
            if (any) last = j0 + 63 - __clzll((long long)any);
            run += __shfl(incl, WAVE - 1, WAVE);
        }
        if (tok < 0) tok = last;
        if (lane == 0 && tok >= 0) greedy_emit(o, row, step, tok, scaled_logit(x[tok], inv_temp) - lse);
    }
}

}  // namespace

int launch_sample_top_p(hipStream_t st, const GreedyState &s, const float *logits, int ld, int rows, int row0, int V,
                        float inv_temp, float top_p, uint64_t seed, const float *u, int cap_off, int step) {
    if (rows <= 0) return 0;
    const dim3 grid(rows), block(SMP_THREADS);
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, block, 0, st, logits, ld, V, row0, inv_temp, top_p, seed, u, cap_off, step, s);
    };
    if (V <= 2 * SMP_THREADS) launch(sample_top_p_kernel<2>);
    else if (V <= 50 * SMP_THREADS) launch(sample_top_p_kernel<50>);
    else launch(sample_top_p_kernel<0>);
    CAPDEC_HIP(hipGetLastError());
    return 0;
}

}  // namespace capdec
