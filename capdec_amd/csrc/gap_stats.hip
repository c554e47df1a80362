// capdec_embed_moments / capdec_group_distances: the two estimates CapDec's training takes from data -- the modality offset
// (reference others/modality_offset_calculator.py) and the spread of the embeddings of captions that describe one image,
// whose per-entry maximum is what --noise_variance stands for (reference predictions_runner.py:32-95, :235-251).
//
// Contract (include/capdec.h; tests/gap_stats_def.py restates it in fp64).  Every sum -- the row norms, the column sums, the
// sums of squares -- is taken in fp64; the outputs are the fp32 roundings.
//
// capdec_embed_moments
//   gap_moments_kernel   one block per slab of GAP_SLAB rows.  Norm pass: a wave per row, the row in registers, 1 / ||row|| into
//                        LDS (and the row's ||b - a||_2, ||b - a||_inf into d_pair).  Column pass: a thread per four columns
//                        reads the slab's rows from global memory a SECOND time (whether a cache serves that read was not measured) and adds
//                        [sum a, sum a^2, sum b, sum b^2, sum (b-a)^2, sum |b-a|] in fp64; the block's sums go to the workspace
//                        [slab][6][dim].  No atomics: a row's contribution does not depend on n.
//   gap_fold_kernel      adds the partials of GAP_FOLD consecutive slabs, in slab order; repeated until at most GAP_FOLD are left
//   gap_finish_kernel    adds those in order and writes the seven rows of d_stats
// capdec_group_distances
//   gap_index_kernel     flags an index outside [0, rows): the call reads the flag and refuses before the next launch
//   gap_group_kernel<g>  one block per group of g <= 8 rows (the host sorts the groups by size): a thread holds its column's g values, the g (g - 1) / 2 pair
//                        accumulators (sum |d| and sum d^2 in fp64, max |d| in fp32 -- the fp32 rounding of the exact
//                        difference, and rounding is monotonic) and the g to-centre accumulators in registers; one walk
//                        over the columns, then a wave butterfly and an in-order sum of the block's waves (one wave up to
//                        2048 columns, four beyond).
// No address depends on a value: the index array is checked before it is used, and NaN / inf only ever flow through arithmetic.
#include "context.h"

namespace capdec {

namespace {

constexpr int GAP_THREADS = 256;
constexpr int GAP_SLAB = 64;                       // rows per slab: a compile-time constant, not a knob
constexpr int GAP_MAX_DIM = 4 * GAP_THREADS;       // a thread of the column pass owns four columns
constexpr int GAP_FOLD = 32;                       // partials added per thread of one fold
constexpr int GAP_MAX_G = 8, GAP_MAX_PAIRS = GAP_MAX_G * (GAP_MAX_G - 1) / 2;
constexpr int GAP_NARROW_W = 2048;                 // group rows up to this width are walked by one wave, wider ones by four: the
                                                   // reduction across a block costs as much for 640 columns as for 30 720

// butterfly: every lane ends with the same bits (a + b == b + a at every step)
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o, WAVE);
    return v;
}
__device__ __forceinline__ float wave_max_f32(float v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, WAVE));
    return v;
}
__device__ __forceinline__ float comp(const float4 &v, int e) { return e == 0 ? v.x : e == 1 ? v.y : e == 2 ? v.z : v.w; }
__device__ __forceinline__ double sumsq(const float4 &v, double s) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const double x = comp(v, e);
        s = fma(x, x, s);
    }
    return s;
}

// ---------------------------------------------------------------------------- moments
template <bool HAS_B, bool PAIR>
__global__ __launch_bounds__(GAP_THREADS) void gap_moments_kernel(const float *__restrict__ a, const float *__restrict__ b, int n,
                                                                  int dim, int normalize, double *__restrict__ part,
                                                                  float *__restrict__ pair) {
    constexpr int NS = HAS_B ? 6 : 2;
    __shared__ double s_inv[2][GAP_SLAB];
    const int r0 = blockIdx.x * GAP_SLAB, nr = min(GAP_SLAB, n - r0);
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    const int q = dim >> 2;                         // float4 per row, <= GAP_THREADS
    // ---- norm pass: wave-uniform loop, every lane reaches every shuffle
    for (int r = wave; r < nr; r += GAP_THREADS / WAVE) {
        const float4 *pa = reinterpret_cast<const float4 *>(a + (size_t)(r0 + r) * dim);
        const float4 *pb = HAS_B ? reinterpret_cast<const float4 *>(b + (size_t)(r0 + r) * dim) : nullptr;
        float4 va[4], vb[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int j = lane + WAVE * k;
            va[k] = j < q ? pa[j] : make_float4(0.f, 0.f, 0.f, 0.f);
            vb[k] = HAS_B && j < q ? pb[j] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        double ia = 1.0, ib = 1.0;
        if (normalize) {                            // a zero row: 1 / 0 = inf, and 0 * inf = NaN as torch's 0 / 0
            double sa = 0.0, sb = 0.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                sa = sumsq(va[k], sa);
                if (HAS_B) sb = sumsq(vb[k], sb);
            }
            ia = 1.0 / sqrt(wave_sum_f64(sa));
            if (HAS_B) ib = 1.0 / sqrt(wave_sum_f64(sb));
        }
        if (lane == 0) {
            s_inv[0][r] = ia;
            s_inv[1][r] = ib;
        }
        if (PAIR) {
            double s2 = 0.0;
            float mx = 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (lane + WAVE * k < q) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const double d = (double)comp(vb[k], e) * ib - (double)comp(va[k], e) * ia;
                        s2 = fma(d, d, s2);
                        mx = fmaxf(mx, (float)fabs(d));
                    }
                }
            }
            s2 = wave_sum_f64(s2);
            mx = wave_max_f32(mx);
            if (lane == 0) {                        // fmaxf drops a NaN; the sum of squares keeps it
                pair[2 * (size_t)(r0 + r)] = (float)sqrt(s2);
                pair[2 * (size_t)(r0 + r) + 1] = s2 != s2 ? __builtin_nanf("") : mx;
            }
        }
    }
    __syncthreads();
    // ---- column pass
    const int t = threadIdx.x;
    if (t >= q) return;
    double S[NS][4];
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int e = 0; e < 4; ++e) S[s][e] = 0.0;
#pragma unroll 4
    for (int r = 0; r < nr; ++r) {
        const float4 xa = reinterpret_cast<const float4 *>(a + (size_t)(r0 + r) * dim)[t];
        const double ia = s_inv[0][r];
        if constexpr (HAS_B) {
            const float4 xb = reinterpret_cast<const float4 *>(b + (size_t)(r0 + r) * dim)[t];
            const double ib = s_inv[1][r];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double an = (double)comp(xa, e) * ia, bn = (double)comp(xb, e) * ib, d = bn - an;
                S[0][e] += an;
                S[1][e] = fma(an, an, S[1][e]);
                S[2][e] += bn;
                S[3][e] = fma(bn, bn, S[3][e]);
                S[4][e] = fma(d, d, S[4][e]);
                S[5][e] += fabs(d);
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double an = (double)comp(xa, e) * ia;
                S[0][e] += an;
                S[1][e] = fma(an, an, S[1][e]);
            }
        }
    }
    double *p = part + (size_t)blockIdx.x * NS * dim + 4 * t;
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int e = 0; e < 4; ++e) p[(size_t)s * dim + e] = S[s][e];
}

// out[g][e] = sum over the slabs [g * GAP_FOLD, min(count, (g + 1) * GAP_FOLD)) of in[slab][e], in slab order
__global__ __launch_bounds__(GAP_THREADS) void gap_fold_kernel(const double *__restrict__ in, int count, int width,
                                                               double *__restrict__ out) {
    const int e = blockIdx.y * GAP_THREADS + threadIdx.x;
    if (e >= width) return;
    const int s0 = blockIdx.x * GAP_FOLD, s1 = min(count, s0 + GAP_FOLD);
    double acc = 0.0;
    for (int s = s0; s < s1; ++s) acc += in[(size_t)s * width + e];
    out[(size_t)blockIdx.x * width + e] = acc;
}

__device__ __forceinline__ float unbiased_std(double sq, double sum, int n) {
    if (n < 2) return __builtin_nanf("");           // torch.std of one row
    const double v = (sq - sum * sum / n) / (n - 1);
    return (float)sqrt(v < 0.0 ? 0.0 : v);          // (a NaN stays: the comparison is false)
}

__global__ __launch_bounds__(GAP_THREADS) void gap_finish_kernel(const double *__restrict__ part, int count, int n, int dim,
                                                                 int has_b, float *__restrict__ stats) {
    const int c = blockIdx.x * GAP_THREADS + threadIdx.x;
    if (c >= dim) return;
    const int ns = has_b ? 6 : 2;
    double S[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int g = 0; g < count; ++g)
        for (int s = 0; s < ns; ++s) S[s] += part[((size_t)g * ns + s) * dim + c];
    stats[c] = (float)(S[0] / n);
    stats[3 * dim + c] = unbiased_std(S[1], S[0], n);
    const double sd = S[2] - S[0];
    stats[dim + c] = has_b ? (float)(S[2] / n) : 0.f;
    stats[2 * dim + c] = has_b ? (float)(sd / n) : 0.f;
    stats[4 * dim + c] = has_b ? unbiased_std(S[3], S[2], n) : 0.f;
    stats[5 * dim + c] = has_b ? unbiased_std(S[4], sd, n) : 0.f;
    stats[6 * dim + c] = has_b ? (float)(S[5] / n) : 0.f;
}

int moments_run(capdec_ctx *c, const float *a, const float *b, int n, int dim, int normalize, float *stats, float *pair) {
    const int ns = b ? 6 : 2, width = ns * dim;
    const int slabs = (n - 1) / GAP_SLAB + 1, folded = (slabs + GAP_FOLD - 1) / GAP_FOLD;      // (no n + 63: n may be INT_MAX)
    CAPDEC_TRY(c->gap_ws.ensure((size_t)slabs * width * sizeof(double)));
    CAPDEC_TRY(c->gap_ws2.ensure((size_t)folded * width * sizeof(double)));
    double *cur = c->gap_ws.as<double>(), *other = c->gap_ws2.as<double>();
    ProfScope ps(c, F_OTHER);
    const dim3 grid(slabs), block(GAP_THREADS);
    if (b && pair) hipLaunchKernelGGL((gap_moments_kernel<true, true>), grid, block, 0, c->stream, a, b, n, dim, normalize, cur, pair);
    else if (b) hipLaunchKernelGGL((gap_moments_kernel<true, false>), grid, block, 0, c->stream, a, b, n, dim, normalize, cur, pair);
    else hipLaunchKernelGGL((gap_moments_kernel<false, false>), grid, block, 0, c->stream, a, b, n, dim, normalize, cur, pair);
    CAPDEC_HIP(hipGetLastError());
    int count = slabs;
    while (count > GAP_FOLD) {                      // the two buffers take turns: every level is smaller than the one before
        const int next = (count + GAP_FOLD - 1) / GAP_FOLD;
        hipLaunchKernelGGL(gap_fold_kernel, dim3(next, (width + GAP_THREADS - 1) / GAP_THREADS), block, 0, c->stream, cur, count,
                           width, other);
        CAPDEC_HIP(hipGetLastError());
        std::swap(cur, other);
        count = next;
    }
    hipLaunchKernelGGL(gap_finish_kernel, dim3((dim + GAP_THREADS - 1) / GAP_THREADS), block, 0, c->stream, cur, count, n, dim,
                       b ? 1 : 0, stats);
    CAPDEC_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------- group distances
__global__ void gap_index_kernel(const int32_t *__restrict__ index, int lo, int hi, int rows, int *__restrict__ flag) {
    const int i = lo + blockIdx.x * blockDim.x + threadIdx.x;
    if (i < hi && (index[i] < 0 || index[i] >= rows)) *flag = 1;
}

struct GroupLds {
    double d[GAP_THREADS / WAVE][2 * GAP_MAX_PAIRS + GAP_MAX_G];
    float f[GAP_THREADS / WAVE][GAP_MAX_PAIRS + GAP_MAX_G];
};

template <int G>
__device__ __forceinline__ void gap_group(const float *__restrict__ x, int W, const int32_t *__restrict__ index, int o0,
                                          float *__restrict__ out, GroupLds &lds) {
    constexpr int NP = G * (G - 1) / 2, NPA = NP > 0 ? NP : 1;
    const float4 *row[G];
#pragma unroll
    for (int i = 0; i < G; ++i) row[i] = reinterpret_cast<const float4 *>(x + (size_t)(index ? index[o0 + i] : o0 + i) * W);
    double s1[NPA], s2[NPA], c2[G];
    float mx[NPA], cm[G];
#pragma unroll
    for (int p = 0; p < NPA; ++p) s1[p] = s2[p] = 0.0, mx[p] = 0.f;
#pragma unroll
    for (int i = 0; i < G; ++i) c2[i] = 0.0, cm[i] = 0.f;
    for (int j = threadIdx.x; j < (W >> 2); j += blockDim.x) {
        float4 v[G];
#pragma unroll
        for (int i = 0; i < G; ++i) v[i] = row[i][j];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            double f[G], m = 0.0;
#pragma unroll
            for (int i = 0; i < G; ++i) {
                f[i] = comp(v[i], e);
                m += f[i];
            }
            m /= G;
#pragma unroll
            for (int i = 0; i < G; ++i) {
                const double dc = f[i] - m;
                c2[i] = fma(dc, dc, c2[i]);
                cm[i] = fmaxf(cm[i], (float)fabs(dc));
            }
            int p = 0;
#pragma unroll
            for (int i = 0; i < G; ++i)
#pragma unroll
                for (int k = i + 1; k < G; ++k, ++p) {
                    const double d = fabs(f[i] - f[k]);          // exact: both are fp32 values
                    s1[p] += d;
                    s2[p] = fma(d, d, s2[p]);
                    mx[p] = fmaxf(mx[p], (float)d);
                }
        }
    }
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        s1[p] = wave_sum_f64(s1[p]);
        s2[p] = wave_sum_f64(s2[p]);
        mx[p] = wave_max_f32(mx[p]);
    }
#pragma unroll
    for (int i = 0; i < G; ++i) {
        c2[i] = wave_sum_f64(c2[i]);
        cm[i] = wave_max_f32(cm[i]);
    }
    if (lane == 0) {
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            lds.d[wave][2 * p] = s1[p];
            lds.d[wave][2 * p + 1] = s2[p];
            lds.f[wave][p] = mx[p];
        }
#pragma unroll
        for (int i = 0; i < G; ++i) {
            lds.d[wave][2 * NP + i] = c2[i];
            lds.f[wave][NP + i] = cm[i];
        }
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const float nan = __builtin_nanf("");
    const int waves = blockDim.x / WAVE;
    auto sum_d = [&](int k) {                       // the waves' sums in wave order
        double v = lds.d[0][k];
        for (int w = 1; w < waves; ++w) v += lds.d[w][k];
        return v;
    };
    auto max_f = [&](int k) {
        float v = lds.f[0][k];
        for (int w = 1; w < waves; ++w) v = fmaxf(v, lds.f[w][k]);
        return v;
    };
    double l1 = 0.0, l2 = 0.0, linf = 0.0, best = 0.0, ctr2 = 0.0, ctrinf = 0.0;
    for (int p = 0; p < NP; ++p) {
        const double q = sum_d(2 * p + 1), nrm = sqrt(q);
        l1 += sum_d(2 * p);
        l2 += nrm;
        linf += q != q ? nan : max_f(p);            // fmaxf drops a NaN; the sum of squares keeps it
        best = (nrm > best || nrm != nrm) ? nrm : best;
    }
    for (int i = 0; i < G; ++i) {
        const double q = sum_d(2 * NP + i);
        ctr2 += sqrt(q);
        ctrinf += q != q ? nan : max_f(NP + i);
    }
    const double wc = (double)W * NP;
    out[0] = NP ? (float)(l1 / wc) : 0.f;
    out[1] = NP ? (float)(l2 / wc) : 0.f;
    out[2] = NP ? (float)(linf / NP) : 0.f;
    out[3] = NP ? (float)(best / sqrt((double)W)) : 0.f;
    out[4] = (float)(ctr2 / G);
    out[5] = (float)(ctrinf / G);
    out[6] = (float)NP;
    out[7] = (float)G;
}

// One instantiation per group size, so that a group of five does not pay for the registers of a group of eight: the host sorts
// the group numbers by size (gids) and launches each size present over its share of them.
template <int G>
__global__ __launch_bounds__(GAP_THREADS) void gap_group_kernel(const float *__restrict__ x, int W, const int32_t *__restrict__ index,
                                                                const int32_t *__restrict__ offsets,
                                                                const int32_t *__restrict__ gids, float *__restrict__ out) {
    __shared__ GroupLds lds;
    const int k = gids[blockIdx.x];
    gap_group<G>(x, W, index, offsets[k], out + 8 * (size_t)k, lds);
}

template <int G>
int launch_groups(capdec_ctx *c, int count, const float *x, int W, const int32_t *index, const int32_t *offsets,
                  const int32_t *gids, float *out) {
    hipLaunchKernelGGL(gap_group_kernel<G>, dim3(count), dim3(W <= GAP_NARROW_W ? WAVE : GAP_THREADS), 0, c->stream, x, W, index,
                       offsets, gids, out);
    CAPDEC_HIP(hipGetLastError());
    return 0;
}

// h_offsets was checked by the caller: every group has 1..GAP_MAX_G rows.  c->gap_off: [flag | offsets | group numbers by size]
int groups_run(capdec_ctx *c, const float *x, int rows, int W, const int32_t *index, const int32_t *h_offsets, int groups,
               float *out) {
    CAPDEC_TRY(c->gap_off.ensure((2 * (size_t)groups + 2) * sizeof(int32_t)));
    int *flag = c->gap_off.as<int>();
    int32_t *offsets = c->gap_off.as<int32_t>() + 1, *gids = offsets + groups + 1;
    if (index) {
        const int lo = h_offsets[0], hi = h_offsets[groups];
        CAPDEC_HIP(hipMemsetAsync(flag, 0, sizeof(int), c->stream));
        hipLaunchKernelGGL(gap_index_kernel, dim3((unsigned)(((size_t)(hi - lo) + 255) / 256)), dim3(256), 0, c->stream, index, lo, hi,
                           rows, flag);
        CAPDEC_HIP(hipGetLastError());
        int bad = 0;
        CAPDEC_HIP(hipMemcpyAsync(&bad, flag, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        CAPDEC_HIP(hipStreamSynchronize(c->stream));
        CAPDEC_CHECK(bad == 0, "group_distances: an index lies outside [0, rows)");
    }
    int start[GAP_MAX_G + 2] = {0};
    for (int k = 0; k < groups; ++k) ++start[h_offsets[k + 1] - h_offsets[k] + 1];
    for (int g = 1; g <= GAP_MAX_G + 1; ++g) start[g] += start[g - 1];      // start[g] = groups smaller than g
    std::vector<int32_t> by_size(groups);
    {
        int next[GAP_MAX_G + 1];
        for (int g = 1; g <= GAP_MAX_G; ++g) next[g] = start[g];
        for (int k = 0; k < groups; ++k) by_size[next[h_offsets[k + 1] - h_offsets[k]]++] = k;
    }
    CAPDEC_HIP(hipMemcpyAsync(offsets, h_offsets, ((size_t)groups + 1) * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    CAPDEC_HIP(hipMemcpyAsync(gids, by_size.data(), (size_t)groups * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    CAPDEC_HIP(hipStreamSynchronize(c->stream));      // by_size is pageable and leaves scope with this function
    ProfScope ps(c, F_OTHER);
    for (int g = 1; g <= GAP_MAX_G; ++g) {
        const int count = start[g + 1] - start[g];
        if (!count) continue;
        const int32_t *ids = gids + start[g];
        switch (g) {
            case 1: CAPDEC_TRY(launch_groups<1>(c, count, x, W, index, offsets, ids, out)); break;
            case 2: CAPDEC_TRY(launch_groups<2>(c, count, x, W, index, offsets, ids, out)); break;
            case 3: CAPDEC_TRY(launch_groups<3>(c, count, x, W, index, offsets, ids, out)); break;
            case 4: CAPDEC_TRY(launch_groups<4>(c, count, x, W, index, offsets, ids, out)); break;
            case 5: CAPDEC_TRY(launch_groups<5>(c, count, x, W, index, offsets, ids, out)); break;
            case 6: CAPDEC_TRY(launch_groups<6>(c, count, x, W, index, offsets, ids, out)); break;
            case 7: CAPDEC_TRY(launch_groups<7>(c, count, x, W, index, offsets, ids, out)); break;
            default: CAPDEC_TRY(launch_groups<8>(c, count, x, W, index, offsets, ids, out)); break;
        }
    }
    return 0;
}

}  // namespace

}  // namespace capdec

using namespace capdec;

extern "C" int capdec_embed_moments(capdec_ctx *c, const float *a, const float *b, int n, int dim, int normalize, float *stats,
                                    float *pair) {
    CAPDEC_CHECK(c, "embed_moments: null context");
    CAPDEC_CHECK(n >= 1, "embed_moments: n must be at least 1");
    CAPDEC_CHECK(dim >= 4 && dim % 4 == 0 && dim <= GAP_MAX_DIM, "embed_moments: dim must be a multiple of 4, at most 1024");
    CAPDEC_CHECK(a && stats, "embed_moments: null argument");
    CAPDEC_CHECK(b || !pair, "embed_moments: d_pair needs d_b");
    CAPDEC_CHECK((((uintptr_t)a | (uintptr_t)b) & 15) == 0, "embed_moments: d_a and d_b must be 16-byte aligned");
    CAPDEC_HIP(hipSetDevice(c->device));
    const int rc = moments_run(c, a, b, n, dim, normalize, stats, pair);
    if (hipStreamSynchronize(c->stream) != hipSuccess && rc == 0) {
        set_error("embed_moments: hipStreamSynchronize failed");
        return 1;
    }
    return rc;
}

extern "C" int capdec_group_distances(capdec_ctx *c, const float *x, int rows, int W, const int32_t *index,
                                      const int32_t *h_offsets, int groups, float *out) {
    CAPDEC_CHECK(c, "group_distances: null context");
    CAPDEC_CHECK(groups >= 0, "group_distances: negative group count");
    CAPDEC_CHECK(rows >= 0, "group_distances: negative row count");
    CAPDEC_CHECK(W >= 4 && W % 4 == 0, "group_distances: W must be a positive multiple of 4");
    if (groups == 0) return 0;
    CAPDEC_CHECK(x && h_offsets && out, "group_distances: null argument");
    CAPDEC_CHECK(((uintptr_t)x & 15) == 0, "group_distances: d_x must be 16-byte aligned");
    CAPDEC_CHECK(h_offsets[0] >= 0, "group_distances: negative offset");
    for (int k = 0; k < groups; ++k) {
        CAPDEC_CHECK(h_offsets[k + 1] > h_offsets[k], "group_distances: offsets must ascend (every group has at least one row)");
        CAPDEC_CHECK(h_offsets[k + 1] - h_offsets[k] <= GAP_MAX_G, "group_distances: a group has more than 8 rows");
    }
    CAPDEC_CHECK(index || h_offsets[groups] <= rows, "group_distances: the offsets run past the rows");
    CAPDEC_HIP(hipSetDevice(c->device));
    const int rc = groups_run(c, x, rows, W, index, h_offsets, groups, out);
    if (hipStreamSynchronize(c->stream) != hipSuccess && rc == 0) {
        set_error("group_distances: hipStreamSynchronize failed");
        return 1;
    }
    return rc;
}
