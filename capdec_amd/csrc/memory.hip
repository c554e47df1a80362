// capdec_memory_*: project image embeddings onto a support memory of text embeddings (DeCap, Li et al., ICLR 2023) -- the
// training-free way across the modality gap.  Flash attention with K = V = the memory and a head dimension of up to 640: the
// [rows, memory rows] similarity matrix and the softmax weights never reach HBM.
//
// Contract (include/capdec.h; tests/memory_def.py restates it in fp64).
//     xn = x / max(||x||, 1e-12)     mn_j = m_j / max(||m_j||, 1e-12)
//     w = softmax_j(<xn, mn_j> / tau)     v = sum_j w_j mn_j     out = v / max(||v||, 1e-12)
// plus lse = logsumexp_j(<xn, mn_j> / tau), nearest = argmax_j <xn, mn_j> (lowest index among equals) and its similarity.
//
// Arithmetic.  Both products run on the fp32 matrix instruction (v_mfma_f32_32x32x2_f32): a k-ordered chain of fp32 FMAs,
// whatever the context's GEMM mode.  1 / tau = 100 multiplies every similarity error into the logits, and softmax weights
// span the whole fp32 exponent range (a quarter of a million weights of 4e-8 carry mass that matters): fp32 operands need no
// plane scaling for either, and cost the same LDS bytes as two fp16 planes.  The price is the rate: 1/16 of the fp16 matrix
// rate per instruction, against 3 + 6 instructions per product pair of a plane scheme that covers the weights' range.
//
// Kernels.
//   mem_normalize_kernel   a wave per row: unit rows, fp32, row stride dp = d rounded up to 128 (zero columns); a row holding
//                          a NaN or an inf becomes a zero row and is flagged.  The memory once per load (kept in the context,
//                          rows padded to MEM_MTILE with zero rows), the queries per row block.
//   mem_project_kernel     one block per (query tile, chunk of MEM_CHUNK memory rows): groups of four waves, a group per 32 query
//                          rows -- two groups (MEM_QTILE = 64 rows, two waves per SIMD: one group's softmax runs under the
//                          other's MFMAs) up to d = 512, one group at d = 640, where a wave's state needs more than 256
//                          registers.  Wave w of a group owns the columns [w dp/4, (w+1) dp/4) in BOTH products, so its slice
//                          of the query rows stays in registers for the whole chunk and only the memory tile (MEM_MTILE rows,
//                          staged once, serving both products and both groups) lives in LDS:
//                            S^T[j][i] partial over the wave's columns (A = memory rows, B = queries) -> the four partials
//                              meet in LDS and every wave adds them in wave order, so all four hold the same bits;
//                            online softmax: a query is a COLUMN of the accumulator tile, so its running max and sum are
//                              per lane -- 16 registers and one exchange between the two lane halves;
//                            O^T[c][i] += mn[j][c] P^T[j][i] for the wave's columns c: the accumulator tile of S^T is the B
//                              operand of this product as it stands (k-step r of a lane half holds memory row
//                              (r & 3) + 8 (r >> 2) + 4 half of the tile), no trip through LDS.
//                          The next memory tile travels global -> registers while the current one is computed on.  A chunk
//                          starts from a fresh (max, sum, vector) state and ends as one partial [dp | max, sum, best sim,
//                          best index] per query row.
//   mem_merge_kernel       a block per query row: folds the chunk partials in chunk order by the one merge formula, divides,
//                          normalises, writes the four outputs; flagged query rows get NaN / -1.
//
// Deterministic and batch-invariant: no atomics; the split of the memory is a function of the memory alone (every chunk
// always writes its partial, whatever the row count), a query's column of an accumulator tile does not depend on the other
// columns, and the merge is one left fold.  Queries are processed in row blocks sized so that the partials stay below
// MEM_PART_BYTES (at the largest memory, 2048 chunks of 644 floats per row, a block is still one 32-row group).
#include "context.h"

namespace capdec {

namespace {

constexpr int MEM_QTILE = 64;        // query rows per block of mem_project_kernel: MEM_QGROUPS groups of 32 (d <= 512; wider rows: one group)
constexpr int MEM_MTILE = 32;        // memory rows per LDS stage
constexpr int MEM_CHUNK = 2048;      // memory rows per partial: the unit the memory is split in
constexpr int MEM_WAVES = 4, MEM_THREADS = MEM_WAVES * WAVE;     // waves that share the columns of a group; threads of the row kernels
constexpr int MEM_QGROUPS = 2;       // two waves per SIMD, one group's softmax under the other's MFMAs -- where 256 registers hold a wave's state
constexpr int mem_groups(int ncb) { return ncb <= 4 ? MEM_QGROUPS : 1; }      // (dp = 640: 80 query + 80 accumulator registers; one group, 512 registers)
static_assert(MEM_QTILE == 32 * MEM_QGROUPS, "a group is one 32-column accumulator tile of queries");
constexpr int MEM_DPAD = 32 * MEM_WAVES;     // row stride granule: every wave owns a multiple of 32 columns
constexpr int MEM_LDS_PAD = 4;       // floats behind a staged row: rows 16 B apart in the banks
constexpr int MEM_TAIL = 4;          // floats behind a partial's vector: max, sum, best similarity, best index
constexpr int MEM_MAX_D = 640, MEM_MAX_ROWS = 4194304;
constexpr size_t MEM_PART_BYTES = (size_t)256 << 20;      // bound of the per-call workspace of partials
constexpr int MEM_NORM_MAX = MEM_MAX_D / WAVE;            // elements a lane of the normalising wave holds

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

inline int mem_dp(int d) { return (d + MEM_DPAD - 1) / MEM_DPAD * MEM_DPAD; }
inline int mem_chunks(int rows) { return (rows + MEM_CHUNK - 1) / MEM_CHUNK; }
inline size_t mem_lds_bytes(int dp, int groups) {
    return ((size_t)MEM_MTILE * (dp + MEM_LDS_PAD) + (size_t)groups * MEM_WAVES * 16 * WAVE) * sizeof(float);
}

// x [rows, d] -> out [rows, dp]: x / max(||x||, 1e-12), columns d .. dp zero; row_bad[row] (may be null) = the row holds a
// NaN or an inf (it is written as zeros), *any_bad (may be null) is set when one does
__global__ __launch_bounds__(MEM_THREADS) void mem_normalize_kernel(const float *__restrict__ x, int rows, int d, int dp,
                                                                    float *__restrict__ out, int *__restrict__ row_bad,
                                                                    int *__restrict__ any_bad) {
    const int row = blockIdx.x * MEM_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;          // (a whole wave leaves)
    const float *xr = x + (size_t)row * d;
    float v[MEM_NORM_MAX], ss = 0.f;
    bool bad = false;
#pragma unroll
    for (int e = 0; e < MEM_NORM_MAX; ++e) {
        const int k = lane + WAVE * e;
        v[e] = k < d ? xr[k] : 0.f;
        bad |= !(__builtin_fabsf(v[e]) <= 3.402823466e38f);
        ss += v[e] * v[e];
    }
    ss = wave_sum(ss);
    bad = __ballot(bad) != 0;
    const float den = fmaxf(sqrtf(ss), 1e-12f);
    float *o = out + (size_t)row * dp;
#pragma unroll
    for (int e = 0; e < MEM_NORM_MAX; ++e) {
        const int k = lane + WAVE * e;
        if (k < dp) o[k] = bad ? 0.f : v[e] / den;
    }
    if (lane == 0) {
        if (row_bad) row_bad[row] = bad ? 1 : 0;
        if (bad && any_bad) *any_bad = 1;
    }
}

// NCB = dp / 128: 32-column blocks per wave; G: query groups of 32 rows per block.  mn [rows up to MEM_MTILE, dp] zero padded, qn [nq, dp], part [nq, nchunks, dp + 4]
template <int NCB, int G>
__global__ __launch_bounds__(G * MEM_THREADS) void mem_project_kernel(const float *__restrict__ mn, int M, const float *__restrict__ qn,
                                                                  int nq, float tau, float *__restrict__ part, int nchunks) {
    constexpr int DP = MEM_DPAD * NCB, WD = 32 * NCB, LD = DP + MEM_LDS_PAD, NQ4 = WD / 8, PT = G * MEM_THREADS, NST = MEM_MTILE * DP / 4 / PT;
    extern __shared__ __attribute__((aligned(16))) float mem_lds[];
    const int tid = threadIdx.x, w = (tid >> 6) % MEM_WAVES, grp = tid / MEM_THREADS, lane = tid & 63, li = lane & 31, h = lane >> 5;
    float *tile = mem_lds, *xch = mem_lds + MEM_MTILE * LD + grp * (MEM_WAVES * 16 * WAVE);
    const int qi = (blockIdx.x * G + grp) * 32 + li, chunk = blockIdx.y;
    const bool live = (blockIdx.x * G + grp) * 32 < nq;      // a group past the last query row only stages tiles and meets barriers
    const int j0 = chunk * MEM_CHUNK, jend = min(M, j0 + MEM_CHUNK);

    // the wave's slice of the query tile as the B operand of S^T: k-step (t, u) of lane half h is column 8 t + 4 h + u
    float4 q[NQ4];
#pragma unroll
    for (int t = 0; t < NQ4; ++t)
        q[t] = qi < nq ? *reinterpret_cast<const float4 *>(qn + (size_t)qi * DP + w * WD + 8 * t + 4 * h) : make_float4(0.f, 0.f, 0.f, 0.f);

    f32x4 pre[NST];
#define MEM_FETCH(jt)                                                                                                      \
    _Pragma("unroll") for (int e = 0; e < NST; ++e) {                                                                      \
        const int f = tid + PT * e;                                                                                        \
        pre[e] = *reinterpret_cast<const f32x4 *>(mn + ((size_t)(jt) + f / (DP / 4)) * DP + 4 * (f % (DP / 4)));          \
    }
    MEM_FETCH(j0)

    float m = -INFINITY, l = 0.f, best = -INFINITY;
    int bidx = 0;
    f32x16 acc[NCB];
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[cb][r] = 0.f;

    for (int jt = j0; jt < jend; jt += MEM_MTILE) {
        __syncthreads();              // every wave is done with the previous tile and with the exchange buffer
#pragma unroll
        for (int e = 0; e < NST; ++e) {
            const int f = tid + PT * e;
            *reinterpret_cast<f32x4 *>(tile + (f / (DP / 4)) * LD + 4 * (f % (DP / 4))) = pre[e];
        }
        __syncthreads();
        if (jt + MEM_MTILE < jend) { MEM_FETCH(jt + MEM_MTILE) }

        // S^T over the wave's columns: A = memory row li, B = query li
        f32x16 s;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = 0.f;
        if (live) {
        const float *arow = tile + li * LD + w * WD + 4 * h;
#pragma unroll
        for (int t = 0; t < NQ4; ++t) {
            const float4 a = *reinterpret_cast<const float4 *>(arow + 8 * t);
            s = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, q[t].x, s, 0, 0, 0);
            s = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, q[t].y, s, 0, 0, 0);
            s = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, q[t].z, s, 0, 0, 0);
            s = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, q[t].w, s, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) xch[(w * 16 + r) * WAVE + lane] = s[r];
        }
        __syncthreads();
        if (!live) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r)
            s[r] = ((xch[r * WAVE + lane] + xch[(16 + r) * WAVE + lane]) + xch[(32 + r) * WAVE + lane]) + xch[(48 + r) * WAVE + lane];

        // the lane's query against memory rows jt + (r & 3) + 8 (r >> 2) + 4 h: ascending in r
        float tmax = -INFINITY, tb = -INFINITY;
        int tbi = 0x7fffffff;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int jg = jt + (r & 3) + 8 * (r >> 2) + 4 * h;
            const bool valid = jg < jend;
            if (valid && s[r] > tb) { tb = s[r]; tbi = jg; }
            s[r] = valid ? s[r] / tau : -INFINITY;
            tmax = fmaxf(tmax, s[r]);
        }
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
        const float ob = __shfl_xor(tb, 32);
        const int oi = __shfl_xor(tbi, 32);
        if (ob > tb || (ob == tb && oi < tbi)) { tb = ob; tbi = oi; }
        if (tb > best) { best = tb; bidx = tbi; }       // (earlier tiles hold the lower indices)
        const float mnew = fmaxf(m, tmax);              // finite: the tile holds at least one memory row
        const float sc = expf(m - mnew);
        float psum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            s[r] = expf(s[r] - mnew);
            psum += s[r];
        }
        psum += __shfl_xor(psum, 32);
        l = l * sc + psum;
        m = mnew;

        // O^T over the wave's columns: A = memory column (k-step r: rows (r & 3) + 8 (r >> 2) + 4 h), B = the weights as they lie
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) {
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[cb][r] *= sc;
            const float *vcol = tile + 4 * h * LD + w * WD + 32 * cb + li;
#pragma unroll
            for (int r = 0; r < 16; ++r)
                acc[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(vcol[((r & 3) + 8 * (r >> 2)) * LD], s[r], acc[cb], 0, 0, 0);
        }
    }

#undef MEM_FETCH
    if (qi >= nq) return;
    float *pr = part + ((size_t)qi * nchunks + chunk) * (DP + MEM_TAIL);
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
        for (int g = 0; g < 4; ++g)
            *reinterpret_cast<float4 *>(pr + w * WD + 32 * cb + 8 * g + 4 * h) =
                make_float4(acc[cb][4 * g], acc[cb][4 * g + 1], acc[cb][4 * g + 2], acc[cb][4 * g + 3]);
    if (w == 0 && h == 0) *reinterpret_cast<float4 *>(pr + DP) = make_float4(m, l, best, __int_as_float(bidx));
}

// one block per query row; the merge formula: (m, l, v) + (m', l', v') = (M = max(m, m'), l e^(m - M) + l' e^(m' - M), likewise v)
__global__ __launch_bounds__(MEM_THREADS) void mem_merge_kernel(const float *__restrict__ part, int nchunks, int dp, int d,
                                                                const int *__restrict__ row_bad, float *__restrict__ out,
                                                                float *__restrict__ lse, int32_t *__restrict__ nearest,
                                                                float *__restrict__ max_sim) {
    constexpr int NE = (MEM_MAX_D + MEM_THREADS - 1) / MEM_THREADS;
    __shared__ float red[MEM_WAVES];
    const int row = blockIdx.x, tid = threadIdx.x;
    if (row_bad[row]) {
        const float nan = __builtin_nanf("");
        for (int c = tid; c < d; c += MEM_THREADS) out[(size_t)row * d + c] = nan;
        if (tid == 0) {
            if (lse) lse[row] = nan;
            if (nearest) nearest[row] = -1;
            if (max_sim) max_sim[row] = nan;
        }
        return;
    }
    const size_t stride = (size_t)dp + MEM_TAIL;
    const float *p = part + (size_t)row * nchunks * stride;
    float o[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) o[e] = tid + MEM_THREADS * e < dp ? p[tid + MEM_THREADS * e] : 0.f;
    float m = p[dp], l = p[dp + 1], best = p[dp + 2];
    int bidx = __float_as_int(p[dp + 3]);
    for (int ch = 1; ch < nchunks; ++ch) {
        p += stride;
        const float mb = p[dp], lb = p[dp + 1], bb = p[dp + 2];
        const float mm = fmaxf(m, mb), sa = expf(m - mm), sb = expf(mb - mm);
        l = l * sa + lb * sb;
#pragma unroll
        for (int e = 0; e < NE; ++e)
            if (tid + MEM_THREADS * e < dp) o[e] = o[e] * sa + p[tid + MEM_THREADS * e] * sb;
        if (bb > best) { best = bb; bidx = __float_as_int(p[dp + 3]); }
        m = mm;
    }
    float ss = 0.f;
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        o[e] /= l;
        ss += o[e] * o[e];
    }
    ss = wave_sum(ss);
    if ((tid & 63) == 0) red[tid >> 6] = ss;
    __syncthreads();
    const float den = fmaxf(sqrtf(((red[0] + red[1]) + red[2]) + red[3]), 1e-12f);
#pragma unroll
    for (int e = 0; e < NE; ++e)
        if (tid + MEM_THREADS * e < d) out[(size_t)row * d + tid + MEM_THREADS * e] = o[e] / den;
    if (tid == 0) {
        if (lse) lse[row] = m + logf(l);
        if (nearest) nearest[row] = bidx;
        if (max_sim) max_sim[row] = best;
    }
}

template <int NCB>
int launch_project(capdec_ctx *c, int nq, float tau, int nchunks) {
    constexpr int G = mem_groups(NCB);
    const size_t lds = mem_lds_bytes(MEM_DPAD * NCB, G);
    if (lds > 64 * 1024) {            // once per (device, kernel): the limit belongs to the function on a device
        static bool raised[64] = {false};
        if (c->device < 0 || c->device >= 64 || !raised[c->device]) {
            CAPDEC_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&mem_project_kernel<NCB, G>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            if (c->device >= 0 && c->device < 64) raised[c->device] = true;
        }
    }
    hipLaunchKernelGGL((mem_project_kernel<NCB, G>), dim3((nq + 32 * G - 1) / (32 * G), nchunks), dim3(G * MEM_THREADS), lds, c->stream,
                       c->mem_n.as<float>(), c->mem_rows, c->mem_q.as<float>(), nq, tau, c->mem_part.as<float>(), nchunks);
    CAPDEC_HIP(hipGetLastError());
    return 0;
}

int memory_project_run(capdec_ctx *c, const float *x, int rows, int d, float tau, float *out, float *lse, int32_t *nearest,
                       float *max_sim) {
    const int dp = mem_dp(d), nchunks = mem_chunks(c->mem_rows);
    const size_t per_row = (size_t)nchunks * (dp + MEM_TAIL) * sizeof(float);
    // query rows per block: whole tiles, as many as keep the partials below MEM_PART_BYTES; one 32-row group where a whole
    // tile's would not (at most 5.3 MB per row -- 2048 chunks of 644 floats -- so 32 rows always do)
    const size_t rows_fit = MEM_PART_BYTES / per_row;
    const size_t fit = rows_fit >= MEM_QTILE ? rows_fit / MEM_QTILE * MEM_QTILE : 32;
    const int blk = (int)std::min<size_t>(fit, ((size_t)rows + MEM_QTILE - 1) / MEM_QTILE * MEM_QTILE);
    CAPDEC_TRY(c->mem_q.ensure((size_t)blk * dp * sizeof(float)));
    CAPDEC_TRY(c->mem_part.ensure((size_t)blk * per_row));
    CAPDEC_TRY(c->mem_bad.ensure(((size_t)blk + 1) * sizeof(int)));
    int *row_bad = c->mem_bad.as<int>() + 1;
    for (int r0 = 0; r0 < rows; r0 += blk) {
        const int nr = std::min(blk, rows - r0);
        ProfScope ps(c, F_OTHER);
        hipLaunchKernelGGL(mem_normalize_kernel, dim3((nr + MEM_WAVES - 1) / MEM_WAVES), dim3(MEM_THREADS), 0, c->stream,
                           x + (size_t)r0 * d, nr, d, dp, c->mem_q.as<float>(), row_bad, (int *)nullptr);
        CAPDEC_HIP(hipGetLastError());
        switch (dp / MEM_DPAD) {
            case 1: CAPDEC_TRY(launch_project<1>(c, nr, tau, nchunks)); break;
            case 2: CAPDEC_TRY(launch_project<2>(c, nr, tau, nchunks)); break;
            case 3: CAPDEC_TRY(launch_project<3>(c, nr, tau, nchunks)); break;
            case 4: CAPDEC_TRY(launch_project<4>(c, nr, tau, nchunks)); break;
            default: CAPDEC_TRY(launch_project<5>(c, nr, tau, nchunks)); break;
        }
        hipLaunchKernelGGL(mem_merge_kernel, dim3(nr), dim3(MEM_THREADS), 0, c->stream, c->mem_part.as<float>(), nchunks, dp, d,
                           row_bad, out + (size_t)r0 * d, lse ? lse + r0 : nullptr, nearest ? nearest + r0 : nullptr,
                           max_sim ? max_sim + r0 : nullptr);
        CAPDEC_HIP(hipGetLastError());
    }
    return 0;
}

// the new memory is normalised into an allocation of its own and replaces the old one only when every row was finite
int memory_load_run(capdec_ctx *c, const float *mem, int rows, int d) {
    const int dp = mem_dp(d);
    const size_t rows_p = ((size_t)rows + MEM_MTILE - 1) / MEM_MTILE * MEM_MTILE, bytes = rows_p * dp * sizeof(float);
    CAPDEC_TRY(c->mem_bad.ensure(sizeof(int)));
    int *flag = c->mem_bad.as<int>();
    float *fresh = nullptr;
    CAPDEC_HIP(hipMalloc(&fresh, bytes));
    int bad = 1;
    const int rc = [&]() -> int {
        CAPDEC_HIP(hipMemsetAsync(flag, 0, sizeof(int), c->stream));
        if (rows_p > (size_t)rows)
            CAPDEC_HIP(hipMemsetAsync(fresh + (size_t)rows * dp, 0, (rows_p - rows) * dp * sizeof(float), c->stream));
        hipLaunchKernelGGL(mem_normalize_kernel, dim3((rows + MEM_WAVES - 1) / MEM_WAVES), dim3(MEM_THREADS), 0, c->stream, mem, rows,
                           d, dp, fresh, (int *)nullptr, flag);
        CAPDEC_HIP(hipGetLastError());
        CAPDEC_HIP(hipMemcpyAsync(&bad, flag, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        CAPDEC_HIP(hipStreamSynchronize(c->stream));
        CAPDEC_CHECK(bad == 0, "memory_load: a memory row holds a NaN or an inf");
        return 0;
    }();
    if (rc) {
        (void)hipFree(fresh);
        return rc;
    }
    c->mem_n.release();
    c->mem_n.p = fresh;
    c->mem_n.cap = bytes;
    c->mem_rows = rows;
    c->mem_d = d;
    return 0;
}

}  // namespace

void memory_release(capdec_ctx *c) {
    c->mem_n.release();
    c->mem_rows = c->mem_d = 0;
}

}  // namespace capdec

using namespace capdec;

extern "C" int capdec_memory_load(capdec_ctx *c, const float *d_mem, int rows, int d) {
    CAPDEC_CHECK(c, "memory_load: null context");
    CAPDEC_CHECK(rows >= 1 && rows <= MEM_MAX_ROWS, "memory_load: rows must be in 1..4194304");
    CAPDEC_CHECK(d >= 32 && d % 32 == 0 && d <= MEM_MAX_D, "memory_load: d must be a multiple of 32 in 32..640");
    CAPDEC_CHECK(d_mem, "memory_load: null argument");
    CAPDEC_HIP(hipSetDevice(c->device));
    CAPDEC_HIP(hipStreamSynchronize(c->stream));       // nothing enqueued still reads the memory that goes
    return memory_load_run(c, d_mem, rows, d);
}

extern "C" int capdec_memory_free(capdec_ctx *c) {
    CAPDEC_CHECK(c, "memory_free: null context");
    CAPDEC_HIP(hipSetDevice(c->device));
    CAPDEC_HIP(hipStreamSynchronize(c->stream));
    memory_release(c);
    return 0;
}

extern "C" int capdec_memory_project(capdec_ctx *c, const float *d_x, int rows, int d, float temperature, float *d_out, float *d_lse,
                                     int32_t *d_nearest, float *d_max_sim) {
    CAPDEC_CHECK(c, "memory_project: null context");
    CAPDEC_CHECK(c->mem_rows > 0, "memory_project: no memory is loaded (capdec_memory_load)");
    CAPDEC_CHECK(d == c->mem_d, "memory_project: d is not the loaded memory's");
    CAPDEC_CHECK(temperature > 0.f && temperature <= 3.402823466e38f, "memory_project: temperature must be positive and finite");
    CAPDEC_CHECK(rows >= 0, "memory_project: negative row count");
    if (rows == 0) return 0;
    CAPDEC_CHECK(d_x && d_out, "memory_project: null argument");
    CAPDEC_HIP(hipSetDevice(c->device));
    const int rc = memory_project_run(c, d_x, rows, d, temperature, d_out, d_lse, d_nearest, d_max_sim);
    if (hipStreamSynchronize(c->stream) != hipSuccess && rc == 0) {
        set_error("memory_project: hipStreamSynchronize failed");
        return 1;
    }
    return rc;
}
