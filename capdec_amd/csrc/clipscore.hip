// capdec_clip_score: CLIPScore / RefCLIPScore (Hessel et al., EMNLP 2021) of candidate captions against their image and its
// reference captions, and the candidates' order per image -- what sample-and-rerank needs after the two towers (clip.hip).
//
// Contract (include/capdec.h; tests/clip_score_def.py restates it in fp64).  Every sum -- the squared norms, the dots -- is
// taken in fp64; the four columns are computed in fp64 and rounded to fp32 once.
//
//   clip_score_kernel    one block of four waves per image.  The image row goes to LDS once (zero padded to a multiple of four
//                        columns); the group's reference rows follow in slabs of CS_REF_FLOATS (16 KB: five rows up to 816
//                        columns; two at 2048), each slab's squared norms taken by a wave per row.  Then a wave per candidate:
//                        the row from global memory into registers (lane l holds the float4s l, l + 64, ...: at most eight),
//                        its squared norm and its dot with the image (first slab only) and with every reference row of the
//                        slab from LDS, each a per-lane fp64 FMA chain and a wave butterfly; the running maximum of the
//                        reference cosines stays in LDS between slabs.  A group whose references need more than one slab
//                        reads its candidates once per slab (from L2, as a rule).  Last, wave 0 with a lane per candidate
//                        forms the four columns and ranks the candidates by counting, through wave shuffles, the lanes that
//                        come before its own.
// A lane's share of a row and the order of its chain depend on d alone -- the float4 path (d % 4 == 0, 16-byte aligned
// pointers) and the scalar path read the same elements into the same places -- so a candidate's bits depend on nothing but
// its group's rows.  No atomics; no address depends on a value (the offsets are checked on the host before the launch).
#include "context.h"

namespace capdec {

namespace {

constexpr int CS_THREADS = 256, CS_WAVES = CS_THREADS / WAVE;
constexpr int CS_MAX_D = 2048, CS_MAX_G = 64;
constexpr int CS_K = CS_MAX_D / (4 * WAVE);         // float4s of a row a lane holds
constexpr int CS_REF_FLOATS = 4096;                 // a slab of reference rows in LDS
constexpr int CS_REF_ROWS = 32;                     // ... and at most that many rows (narrow d)

// butterfly: every lane ends with the same bits (a + b == b + a at every step)
__device__ __forceinline__ double cs_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o, WAVE);
    return v;
}
__device__ __forceinline__ double cs_dot(const float4 &a, const float4 &b, double s) {
    s = fma((double)a.x, (double)b.x, s);
    s = fma((double)a.y, (double)b.y, s);
    s = fma((double)a.z, (double)b.z, s);
    return fma((double)a.w, (double)b.w, s);
}
// a squared norm of a usable row: not zero, and no NaN or inf went into it (fp64 cannot overflow on 2048 fp32 squares)
__device__ __forceinline__ bool cs_good(double ss) { return ss > 0.0 && ss < __builtin_inf(); }

// columns 4 i .. 4 i + 3 of a row of d columns, zeros past the end (i < ceil(d / 4))
template <bool VEC>
__device__ __forceinline__ float4 cs_load4(const float *__restrict__ row, int i, int d) {
    if constexpr (VEC) {
        return reinterpret_cast<const float4 *>(row)[i];
    } else {
        const int e = 4 * i;
        float4 v;
        v.x = row[e];
        v.y = e + 1 < d ? row[e + 1] : 0.f;
        v.z = e + 2 < d ? row[e + 2] : 0.f;
        v.w = e + 3 < d ? row[e + 3] : 0.f;
        return v;
    }
}

template <bool VEC>
__global__ __launch_bounds__(CS_THREADS) void clip_score_kernel(const float *__restrict__ cand, int d, const float *__restrict__ img,
                                                                const int32_t *__restrict__ offsets, const float *__restrict__ ref,
                                                                const int32_t *__restrict__ ref_offsets, float w,
                                                                float *__restrict__ scores, int32_t *__restrict__ order) {
    __shared__ float4 s_img[CS_MAX_D / 4];
    __shared__ float4 s_ref[CS_REF_FLOATS / 4];
    __shared__ double s_rn[CS_REF_ROWS], s_nc[CS_MAX_G], s_dv[CS_MAX_G], s_best[CS_MAX_G];
    __shared__ int s_refbad;
    const int g = blockIdx.x, o0 = offsets[g], n = offsets[g + 1] - o0;
    if (n == 0) return;                                // (the whole block)
    const int r0 = ref ? ref_offsets[g] : 0, nref = ref ? ref_offsets[g + 1] - r0 : 0;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const int d4 = (d + 3) >> 2, slab_rows = min(CS_REF_ROWS, CS_REF_FLOATS / (4 * d4));
    for (int i = tid; i < d4; i += CS_THREADS) s_img[i] = cs_load4<VEC>(img + (size_t)g * d, i, d);
    if (tid == 0) s_refbad = 0;
    if (tid < n) s_best[tid] = -__builtin_inf();
    __syncthreads();
    double nv = 0.0;                                   // every wave takes the image's squared norm for itself: the same bits
    for (int i = lane; i < d4; i += WAVE) nv = cs_dot(s_img[i], s_img[i], nv);
    nv = cs_wave_sum(nv);
    for (int rs = 0; rs == 0 || rs < nref; rs += slab_rows) {
        const int nr = min(slab_rows, nref - rs);
        if (rs) __syncthreads();                       // the slab before this one has been read
        for (int idx = tid; idx < nr * d4; idx += CS_THREADS) {
            const int r = idx / d4, i = idx - r * d4;
            s_ref[idx] = cs_load4<VEC>(ref + (size_t)(r0 + rs + r) * d, i, d);
        }
        __syncthreads();
        for (int r = wave; r < nr; r += CS_WAVES) {
            double ss = 0.0;
            for (int i = lane; i < d4; i += WAVE) ss = cs_dot(s_ref[r * d4 + i], s_ref[r * d4 + i], ss);
            ss = cs_wave_sum(ss);
            if (lane == 0) {
                s_rn[r] = ss;
                if (!cs_good(ss)) s_refbad = 1;        // (every writer writes the same 1)
            }
        }
        __syncthreads();
        for (int j = wave; j < n; j += CS_WAVES) {     // wave-uniform: every lane reaches every shuffle
            const float *row = cand + (size_t)(o0 + j) * d;
            float4 cv[CS_K];
#pragma unroll
            for (int k = 0; k < CS_K; ++k) {
                const int i = lane + WAVE * k;
                cv[k] = i < d4 ? cs_load4<VEC>(row, i, d) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
            double nc;
            if (rs == 0) {
                double dv = 0.0;
                nc = 0.0;
#pragma unroll
                for (int k = 0; k < CS_K; ++k) {
                    const int i = lane + WAVE * k;
                    if (i < d4) {
                        nc = cs_dot(cv[k], cv[k], nc);
                        dv = cs_dot(cv[k], s_img[i], dv);
                    }
                }
                nc = cs_wave_sum(nc);
                dv = cs_wave_sum(dv);
                if (lane == 0) {
                    s_nc[j] = nc;
                    s_dv[j] = dv;
                }
            } else {
                nc = s_nc[j];
            }
            double best = s_best[j];
            for (int r = 0; r < nr; ++r) {
                double dr = 0.0;
#pragma unroll
                for (int k = 0; k < CS_K; ++k) {
                    const int i = lane + WAVE * k;
                    if (i < d4) dr = cs_dot(cv[k], s_ref[r * d4 + i], dr);
                }
                dr = cs_wave_sum(dr);
                const double rn = s_rn[r];
                if (cs_good(rn)) best = fmax(best, dr / (sqrt(nc) * sqrt(rn)));      // (a NaN from a bad candidate is dropped:
            }                                                                        //  its columns are NaN whatever is here)
            if (lane == 0) s_best[j] = best;
        }
    }
    __syncthreads();
    if (wave != 0) return;
    // ---- wave 0, a lane per candidate: the four columns, then the order
    const float nanf = __builtin_nanf("");
    const bool have = lane < n;
    float key = nanf;
    if (have) {
        const double nc = s_nc[lane];
        const bool ok = cs_good(nc) && cs_good(nv);
        const double cosv = s_dv[lane] / (sqrt(nc) * sqrt(nv));
        const double clip = (double)w * fmax(cosv, 0.0);
        const bool ref_ok = ok && nref > 0 && !s_refbad;
        const double rsim = fmax(s_best[lane], 0.0), den = clip + rsim;
        const double rclip = den == 0.0 ? 0.0 : 2.0 * clip * rsim / den;
        key = ok ? (float)cosv : nanf;
        float *out = scores + 4 * (size_t)(o0 + lane);
        out[0] = key;
        out[1] = ok ? (float)clip : nanf;
        out[2] = ref_ok ? (float)rsim : nanf;
        out[3] = ref_ok ? (float)rclip : nanf;
    }
    int rank = 0;                                      // candidates that come before this lane's: a larger fp32 cosine, NaN
    for (int i = 0; i < n; ++i) {                      // last, equal values (and the NaNs among themselves) by row
        const float ki = __shfl(key, i, WAVE);
        const bool before = ki == ki && (key != key || ki > key);
        const bool same = (ki != ki && key != key) || ki == key;
        rank += (before || (same && i < lane)) ? 1 : 0;
    }
    if (have) order[o0 + rank] = o0 + lane;
}

}  // namespace

}  // namespace capdec

using namespace capdec;

extern "C" int capdec_clip_score(capdec_ctx *c, const float *cand, int rows, int d, const float *img, const int32_t *h_offsets,
                                 int groups, const float *ref, int ref_rows, const int32_t *h_ref_offsets, float w, float *scores,
                                 int32_t *order) {
    CAPDEC_CHECK(c, "clip_score: null context");
    CAPDEC_CHECK(rows >= 0 && groups >= 0 && ref_rows >= 0, "clip_score: negative count");
    CAPDEC_CHECK(d >= 1 && d <= CS_MAX_D, "clip_score: d must be in 1..2048");
    CAPDEC_CHECK((ref == nullptr) == (h_ref_offsets == nullptr), "clip_score: d_ref and h_ref_offsets go together");
    if (groups == 0) return 0;
    CAPDEC_CHECK(h_offsets, "clip_score: null offsets");
    CAPDEC_CHECK(h_offsets[0] == 0, "clip_score: offsets must start at 0");
    for (int k = 0; k < groups; ++k) {
        CAPDEC_CHECK(h_offsets[k + 1] >= h_offsets[k], "clip_score: offsets must not descend");
        CAPDEC_CHECK(h_offsets[k + 1] - h_offsets[k] <= CS_MAX_G, "clip_score: a group has more than 64 candidates");
    }
    CAPDEC_CHECK(h_offsets[groups] == rows, "clip_score: offsets must end at rows");
    if (ref) {
        CAPDEC_CHECK(h_ref_offsets[0] == 0, "clip_score: reference offsets must start at 0");
        for (int k = 0; k < groups; ++k)
            CAPDEC_CHECK(h_ref_offsets[k + 1] >= h_ref_offsets[k], "clip_score: reference offsets must not descend");
        CAPDEC_CHECK(h_ref_offsets[groups] == ref_rows, "clip_score: reference offsets must end at ref_rows");
    }
    if (rows == 0) return 0;
    CAPDEC_CHECK(cand && img && scores && order, "clip_score: null argument");
    CAPDEC_HIP(hipSetDevice(c->device));
    const size_t n_off = (size_t)groups + 1;
    CAPDEC_TRY(c->clipscore_off.ensure(2 * n_off * sizeof(int32_t)));
    int32_t *offsets = c->clipscore_off.as<int32_t>(), *ref_offsets = ref ? offsets + n_off : nullptr;
    CAPDEC_HIP(hipMemcpyAsync(offsets, h_offsets, n_off * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    if (ref) CAPDEC_HIP(hipMemcpyAsync(ref_offsets, h_ref_offsets, n_off * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    const bool vec = d % 4 == 0 && (((uintptr_t)cand | (uintptr_t)img | (uintptr_t)ref) & 15) == 0;
    int rc = 0;
    {
        ProfScope ps(c, F_OTHER);
        if (vec) hipLaunchKernelGGL(clip_score_kernel<true>, dim3(groups), dim3(CS_THREADS), 0, c->stream, cand, d, img, offsets, ref,
                                    ref_offsets, w, scores, order);
        else hipLaunchKernelGGL(clip_score_kernel<false>, dim3(groups), dim3(CS_THREADS), 0, c->stream, cand, d, img, offsets, ref,
                                ref_offsets, w, scores, order);
        if (hipGetLastError() != hipSuccess) {
            set_error("clip_score: the launch failed");
            rc = 1;
        }
    }
    if (hipStreamSynchronize(c->stream) != hipSuccess && rc == 0) {      // (the host offsets are the caller's: read by now)
        set_error("clip_score: hipStreamSynchronize failed");
        return 1;
    }
    return rc;
}
