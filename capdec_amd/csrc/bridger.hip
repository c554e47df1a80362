// capdec_bridger_*: the supervised modality bridger of reference others/supervised_embedding_bridger.py -- an MLP of L Linear
// layers (nn.Linear layout) with ReLU between them, trained with MSELoss and torch.optim.SGD with momentum on (image embedding,
// text embedding) pairs, and applied between the normalisation and clip_project (predictions_runner.py --modality_bridger).
//
// Contract: include/capdec.h; tests/bridger_def.py restates it in fp64.  Arithmetic is plain fp32 (VALU FMAs); the loss sums
// its squares in fp64.  A step is far too small for the planner's GEMMs (24 products of 32 x 640 x 640): what it costs is
// launches and one pass over the weights, so a train step is 2 L + 1 launches:
//   bridger_forward_kernel   one kernel for every layer and every row count.  A block owns BRIDGER_FWD_ROWS rows x
//                            BRIDGER_FWD_COLS outputs, a thread one output; x and W go through LDS in chunks of BRIDGER_FWD_KC
//                            columns, the next chunk fetched into registers while this one is summed.  An output is four chains
//                            of FMAs (k mod 4), each over its k in order, added as (0 + 1) + (2 + 3), whatever n is and wherever
//                            the row sits: batch-invariant by construction.
//                            Bias, ReLU and the store of the post-activation (which the backward reads) are fused.
//   bridger_loss_kernel      one block (train) or one per batch (eval): sum of (out - y)^2 in fp64 -- a thread's strided
//                            float4 in order, then a fixed tree -- the fp32 loss, the running scalars, and for a train
//                            step dY = (out - y) * 2 / (batch * width).
//   bridger_backward_kernel  one launch per layer.  A block owns BRIDGER_BWD_COLS columns of W_l -- all its rows -- and walks them
//                            in chunks of BRIDGER_BWD_JC rows: dY's chunk goes to LDS, a thread owns four weights of the chunk
//                            and forms g = dY^T X for them from the saved input of the layer, while the block adds the chunk's
//                            share of dX = dY W_l for its columns from the weights as they were read (before the update); then
//                            v = momentum v + g, W -= lr v.  The weight gradient never exists in memory; every weight and
//                            every momentum element is read once and written once.  dX, masked by h > 0 on the saved
//                            post-activation, is the dY of the layer below.  Block 0 also sums the bias gradient and updates
//                            the bias.  No reduction crosses a block: no partials, no atomics, the same bits every time.
// capdec_bridger_train_epoch is a host loop over that step; nothing comes back to the host between steps.
// No address depends on a value; NaN / inf only ever flow through arithmetic.
#include "context.h"

namespace capdec {

namespace {

constexpr int BRIDGER_THREADS = 256;
constexpr int BRIDGER_LOSS_THREADS = 1024;         // the loss is one block per batch: its width is what hides the loads
constexpr int BRIDGER_FWD_ROWS = 16;               // rows of a forward block
constexpr int BRIDGER_FWD_COLS = 16;               // outputs per row of a forward block
constexpr int BRIDGER_FWD_KC = 128;                // columns of x and W staged at a time
constexpr int BRIDGER_BWD_COLS = 8;                // columns of W_l a backward block owns
constexpr int BRIDGER_BWD_JC = 128;                // rows of W_l (= columns of dY) a backward block stages at a time
constexpr int FWD_LD = BRIDGER_FWD_KC + 4;         // LDS row pitches: + 4 floats shifts consecutive rows by four banks
constexpr int BWD_LD = BRIDGER_BWD_JC + 4;
static_assert(BRIDGER_FWD_ROWS * BRIDGER_FWD_COLS == BRIDGER_THREADS, "a forward thread owns one output");
static_assert(BRIDGER_BWD_JC * BRIDGER_BWD_COLS == 4 * BRIDGER_THREADS, "a backward thread owns four weights of a chunk");
static_assert(BRIDGER_MAX_BATCH * BRIDGER_BWD_COLS == 2 * BRIDGER_THREADS, "a backward thread owns two entries of dX");

__device__ __forceinline__ float4 f4zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }

// ---------------------------------------------------------------------------- forward
// out[r, j] = act(b[j] + sum_k x[r, k] W[j, k]); x [n, K], W [N, K], out [n, N].  grid (ceil(N / COLS), ceil(n / ROWS)).
__global__ __launch_bounds__(BRIDGER_THREADS) void bridger_forward_kernel(const float *__restrict__ x, const float *__restrict__ W,
                                                                          const float *__restrict__ bias, float *__restrict__ out,
                                                                          int n, int K, int N, int relu) {
    __shared__ __attribute__((aligned(16))) float xs[BRIDGER_FWD_ROWS * FWD_LD];
    __shared__ __attribute__((aligned(16))) float ws[BRIDGER_FWD_COLS * FWD_LD];
    const int t = threadIdx.x;
    const int r0 = blockIdx.y * BRIDGER_FWD_ROWS, j0 = blockIdx.x * BRIDGER_FWD_COLS;
    constexpr int Q = BRIDGER_FWD_KC / 4;           // float4 per staged row
    // a thread stages two float4 of x and two of W per chunk: entry e = t + 256 * h -> row e / Q, float4 e % Q
    float4 px[2], pw[2];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int e = t + BRIDGER_THREADS * h, row = e / Q, k = k0 + 4 * (e % Q);
            px[h] = (r0 + row < n && k < K) ? *reinterpret_cast<const float4 *>(x + (size_t)(r0 + row) * K + k) : f4zero();
            pw[h] = (j0 + row < N && k < K) ? *reinterpret_cast<const float4 *>(W + (size_t)(j0 + row) * K + k) : f4zero();
        }
    };
    const int r = t / BRIDGER_FWD_COLS, j = t % BRIDGER_FWD_COLS;
    float4 acc = f4zero();                          // four chains, by column index mod 4; added in a fixed order at the end
    fetch(0);
    for (int k0 = 0; k0 < K; k0 += BRIDGER_FWD_KC) {
        __syncthreads();                            // the chunk before has been summed
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int e = t + BRIDGER_THREADS * h, row = e / Q, q = e % Q;
            *reinterpret_cast<float4 *>(xs + row * FWD_LD + 4 * q) = px[h];
            *reinterpret_cast<float4 *>(ws + row * FWD_LD + 4 * q) = pw[h];
        }
        __syncthreads();
        if (k0 + BRIDGER_FWD_KC < K) fetch(k0 + BRIDGER_FWD_KC);
        const int kn = min(BRIDGER_FWD_KC, K - k0) >> 2;
        const float4 *xr = reinterpret_cast<const float4 *>(xs + r * FWD_LD);
        const float4 *wr = reinterpret_cast<const float4 *>(ws + j * FWD_LD);
#pragma unroll 8
        for (int q = 0; q < kn; ++q) {              // each chain in column order (unrolled: the LDS reads of eight steps in flight)
            const float4 a = xr[q], b = wr[q];
            acc.x = fmaf(a.x, b.x, acc.x);
            acc.y = fmaf(a.y, b.y, acc.y);
            acc.z = fmaf(a.z, b.z, acc.z);
            acc.w = fmaf(a.w, b.w, acc.w);
        }
    }
    if (r0 + r < n && j0 + j < N) {
        float v = ((acc.x + acc.y) + (acc.z + acc.w)) + bias[j0 + j];
        if (relu) v = v > 0.f ? v : (v != v ? v : 0.f);      // a NaN stays a NaN, as in torch
        out[(size_t)(r0 + r) * N + j0 + j] = v;
    }
}

// ---------------------------------------------------------------------------- loss
// Block k takes the rows [k * batch, min(n, (k + 1) * batch)) of out and y [n, N].  train != 0 (one block): dy = (out - y) * 2 /
// count, the step's scalars.  train == 0: the batch's fp32 loss into losses[k].
__global__ __launch_bounds__(BRIDGER_LOSS_THREADS) void bridger_loss_kernel(const float *__restrict__ out, const float *__restrict__ y,
                                                                            int n, int batch, int N, float *__restrict__ dy,
                                                                            BridgerScalars *__restrict__ scal,
                                                                            float *__restrict__ losses, int train) {
    __shared__ double red[BRIDGER_LOSS_THREADS];
    const size_t row0 = (size_t)blockIdx.x * batch;
    const int rows = (int)min((size_t)batch, (size_t)n - row0);
    const size_t count = (size_t)rows * N, base = row0 * N;      // N is a multiple of 4: whole float4
    const float scale = 2.0f / (float)count;
    const float4 *o4 = reinterpret_cast<const float4 *>(out + base), *y4 = reinterpret_cast<const float4 *>(y + base);
    double s = 0.0;
#pragma unroll 4
    for (size_t i = threadIdx.x; i < count / 4; i += BRIDGER_LOSS_THREADS) {
        const float4 a = o4[i], b = y4[i];
        const float4 d = make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w);
        s = fma((double)d.x, (double)d.x, s);
        s = fma((double)d.y, (double)d.y, s);
        s = fma((double)d.z, (double)d.z, s);
        s = fma((double)d.w, (double)d.w, s);
        if (train) reinterpret_cast<float4 *>(dy)[i] = make_float4(d.x * scale, d.y * scale, d.z * scale, d.w * scale);
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = BRIDGER_LOSS_THREADS / 2; o; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float loss = (float)(red[0] / (double)count);
        if (train) {
            scal->last = loss;
            scal->sum += (double)loss;
            scal->steps += 1;
        } else {
            losses[blockIdx.x] = loss;
        }
    }
}

// the batch losses of an evaluation, added in batch order
__global__ void bridger_eval_sum_kernel(const float *__restrict__ losses, long long batches, BridgerScalars *__restrict__ scal) {
    if (threadIdx.x || blockIdx.x) return;
    double s = 0.0;
    for (long long k = 0; k < batches; ++k) s += (double)losses[k];
    scal->eval_sum = s;
    scal->eval_batches = batches;
}

// ---------------------------------------------------------------------------- backward + update
// Layer with W [N, K], input X [B, K] (the saved post-activation of the layer below, or the step's x), dY [B, N].  grid
// ceil(K / BRIDGER_BWD_COLS).  NEED_DX: dprev[r, k] = (X[r, k] > 0) * sum_j dY[r, j] W[j, k] (the layer below has a ReLU).
template <bool NEED_DX>
__global__ __launch_bounds__(BRIDGER_THREADS) void bridger_backward_kernel(const float *__restrict__ X, const float *__restrict__ dY,
                                                                           float *__restrict__ W, float *__restrict__ vW,
                                                                           float *__restrict__ bias, float *__restrict__ vbias,
                                                                           float *__restrict__ dprev, int B, int K, int N, float lr,
                                                                           float momentum) {
    constexpr int TK = BRIDGER_BWD_COLS, JC = BRIDGER_BWD_JC;
    __shared__ __attribute__((aligned(16))) float xs[BRIDGER_MAX_BATCH * TK];       // X[:, k0 .. k0 + TK)
    __shared__ __attribute__((aligned(16))) float dys[BRIDGER_MAX_BATCH * BWD_LD];  // dY[:, j0 .. j0 + JC)
    __shared__ __attribute__((aligned(16))) float wsm[JC * TK];                      // W[j0 .. j0 + JC, k0 .. k0 + TK) as read
    const int t = threadIdx.x, k0 = blockIdx.x * TK;
    // the block's strip of X (columns past K: zeros)
    for (int e = t; e < B * (TK / 4); e += BRIDGER_THREADS) {
        const int r = e / (TK / 4), k = k0 + 4 * (e % (TK / 4));
        *reinterpret_cast<float4 *>(xs + r * TK + 4 * (e % (TK / 4))) =
            k < K ? *reinterpret_cast<const float4 *>(X + (size_t)r * K + k) : f4zero();
    }
    // owner of four weights of a chunk: row oj of the chunk, columns k0 + 4 * oq ..
    const int oj = t / (TK / 4), oq = t % (TK / 4), ok = k0 + 4 * oq;
    // owner of dX[dr, k0 + dk] and dX[dr + 32, k0 + dk]
    const int dr = t / TK, dk = t % TK;
    float4 dx0 = f4zero(), dx1 = f4zero();          // four chains each, by row of W mod 4; added in a fixed order at the end
    // the next chunk travels in registers while this one is worked on
    constexpr int DYQ = BRIDGER_MAX_BATCH * (JC / 4) / BRIDGER_THREADS;      // float4 of dY per thread and chunk, at most
    float4 pdy[DYQ], pw = f4zero(), pv = f4zero();
    auto fetch = [&](int j0) {
        const int jn = min(JC, N - j0);
#pragma unroll
        for (int h = 0; h < DYQ; ++h) {
            const int e = t + BRIDGER_THREADS * h, r = e / (JC / 4), q = e % (JC / 4);
            pdy[h] = (r < B && 4 * q < jn) ? *reinterpret_cast<const float4 *>(dY + (size_t)r * N + j0 + 4 * q) : f4zero();
        }
        const bool own = oj < jn && ok < K;
        pw = own ? *reinterpret_cast<const float4 *>(W + (size_t)(j0 + oj) * K + ok) : f4zero();
        pv = own ? *reinterpret_cast<const float4 *>(vW + (size_t)(j0 + oj) * K + ok) : f4zero();
    };
    fetch(0);
    for (int j0 = 0; j0 < N; j0 += JC) {
        const int jn = min(JC, N - j0);
        __syncthreads();                            // the chunk before is done with dys and wsm (first turn: xs is written)
#pragma unroll
        for (int h = 0; h < DYQ; ++h) {
            const int e = t + BRIDGER_THREADS * h, r = e / (JC / 4), q = e % (JC / 4);
            *reinterpret_cast<float4 *>(dys + r * BWD_LD + 4 * q) = pdy[h];
        }
        const bool own = oj < jn && ok < K;
        float4 w = pw, v = pv;
        if (NEED_DX) *reinterpret_cast<float4 *>(wsm + oj * TK + 4 * oq) = w;
        __syncthreads();
        if (j0 + JC < N) fetch(j0 + JC);            // rows of W this block has not written yet
        // g = dY^T X for the four owned weights, rows in order
        if (own) {
            float4 g = f4zero();
#pragma unroll 8
            for (int r = 0; r < B; ++r) {
                const float d = dys[r * BWD_LD + oj];
                const float4 xv = *reinterpret_cast<const float4 *>(xs + r * TK + 4 * oq);
                g.x = fmaf(d, xv.x, g.x);
                g.y = fmaf(d, xv.y, g.y);
                g.z = fmaf(d, xv.z, g.z);
                g.w = fmaf(d, xv.w, g.w);
            }
            v.x = momentum * v.x + g.x;
            v.y = momentum * v.y + g.y;
            v.z = momentum * v.z + g.z;
            v.w = momentum * v.w + g.w;
            w.x -= lr * v.x;
            w.y -= lr * v.y;
            w.z -= lr * v.z;
            w.w -= lr * v.w;
            *reinterpret_cast<float4 *>(vW + (size_t)(j0 + oj) * K + ok) = v;
            *reinterpret_cast<float4 *>(W + (size_t)(j0 + oj) * K + ok) = w;
        }
        // the bias gradient and its update: block 0, a thread per row of the chunk
        if (blockIdx.x == 0 && t < jn) {
            float g = 0.f;
#pragma unroll 8
            for (int r = 0; r < B; ++r) g += dys[r * BWD_LD + t];
            const float vb = momentum * vbias[j0 + t] + g;
            vbias[j0 + t] = vb;
            bias[j0 + t] -= lr * vb;
        }
        // the chunk's share of dX, rows of W in order (rows past N hold zeros)
        if (NEED_DX) {
            const float4 *d0 = reinterpret_cast<const float4 *>(dys + dr * BWD_LD);
            const float4 *d1 = reinterpret_cast<const float4 *>(dys + (dr + BRIDGER_MAX_BATCH / 2) * BWD_LD);
            const bool two = dr + BRIDGER_MAX_BATCH / 2 < B;
            if (dr < B) {
#pragma unroll 4
                for (int q = 0; q < (jn + 3) / 4; ++q) {
                    const float w0 = wsm[(4 * q) * TK + dk], w1 = wsm[(4 * q + 1) * TK + dk], w2 = wsm[(4 * q + 2) * TK + dk],
                                w3 = wsm[(4 * q + 3) * TK + dk];
                    const float4 a = d0[q];
                    dx0.x = fmaf(a.x, w0, dx0.x);
                    dx0.y = fmaf(a.y, w1, dx0.y);
                    dx0.z = fmaf(a.z, w2, dx0.z);
                    dx0.w = fmaf(a.w, w3, dx0.w);
                    if (two) {
                        const float4 c = d1[q];
                        dx1.x = fmaf(c.x, w0, dx1.x);
                        dx1.y = fmaf(c.y, w1, dx1.y);
                        dx1.z = fmaf(c.z, w2, dx1.z);
                        dx1.w = fmaf(c.w, w3, dx1.w);
                    }
                }
            }
        }
    }
    if (NEED_DX && k0 + dk < K) {
        if (dr < B) dprev[(size_t)dr * K + k0 + dk] = xs[dr * TK + dk] > 0.f ? (dx0.x + dx0.y) + (dx0.z + dx0.w) : 0.f;
        const int r1 = dr + BRIDGER_MAX_BATCH / 2;
        if (r1 < B) dprev[(size_t)r1 * K + k0 + dk] = xs[r1 * TK + dk] > 0.f ? (dx1.x + dx1.y) + (dx1.z + dx1.w) : 0.f;
    }
}

// ---------------------------------------------------------------------------- host
int launch_forward(capdec_ctx *c, const float *x, const float *W, const float *b, float *out, int n, int K, int N, int relu) {
    const dim3 grid((N + BRIDGER_FWD_COLS - 1) / BRIDGER_FWD_COLS, (n + BRIDGER_FWD_ROWS - 1) / BRIDGER_FWD_ROWS);
    hipLaunchKernelGGL(bridger_forward_kernel, grid, dim3(BRIDGER_THREADS), 0, c->stream, x, W, b, out, n, K, N, relu);
    CAPDEC_HIP(hipGetLastError());
    return 0;
}

// the whole stack over n rows; the result lands in `out` (the activations between: br_f0 / br_f1 in turn)
int forward_rows(capdec_ctx *c, const float *x, int n, float *out) {
    Bridger &br = c->bridger;
    int widest = 0;
    for (int l = 1; l < br.L; ++l) widest = std::max(widest, br.dims[l]);
    if (br.L > 1) {
        CAPDEC_TRY(c->br_f0.ensure((size_t)n * widest * sizeof(float)));
        if (br.L > 2) CAPDEC_TRY(c->br_f1.ensure((size_t)n * widest * sizeof(float)));
    }
    // the grid's y dimension holds 65 535 blocks: more rows go in slices (a row's result does not depend on its slice)
    constexpr int SLICE = 65535 * BRIDGER_FWD_ROWS;
    ProfScope ps(c, F_OTHER);
    const float *cur = x;
    for (int l = 0; l < br.L; ++l) {
        const int K = br.dims[l], N = br.dims[l + 1];
        float *dst = l == br.L - 1 ? out : (l % 2 == 0 ? c->br_f0.as<float>() : c->br_f1.as<float>());
        for (int r0 = 0; r0 < n; r0 += SLICE)
            CAPDEC_TRY(launch_forward(c, cur + (size_t)r0 * K, br.w[l], br.b[l], dst + (size_t)r0 * N, std::min(SLICE, n - r0), K, N,
                                      l < br.L - 1));
        cur = dst;
    }
    return 0;
}

// one train step, enqueued: forward (activations saved), loss, backward with the update
int step_enqueue(capdec_ctx *c, const float *x, const float *y, int B, float lr, float momentum) {
    Bridger &br = c->bridger;
    ProfScope ps(c, F_OTHER);
    const float *cur = x;
    for (int l = 0; l < br.L; ++l) {
        CAPDEC_TRY(launch_forward(c, cur, br.w[l], br.b[l], br.act[l], B, br.dims[l], br.dims[l + 1], l < br.L - 1));
        cur = br.act[l];
    }
    hipLaunchKernelGGL(bridger_loss_kernel, dim3(1), dim3(BRIDGER_LOSS_THREADS), 0, c->stream, br.act[br.L - 1], y, B, B, br.dims[br.L],
                       br.dy[0], br.scal, (float *)nullptr, 1);
    CAPDEC_HIP(hipGetLastError());
    int turn = 0;
    for (int l = br.L - 1; l >= 0; --l) {
        const int K = br.dims[l], N = br.dims[l + 1];
        const dim3 grid((K + BRIDGER_BWD_COLS - 1) / BRIDGER_BWD_COLS), block(BRIDGER_THREADS);
        const float *X = l ? br.act[l - 1] : x;
        if (l)
            hipLaunchKernelGGL(bridger_backward_kernel<true>, grid, block, 0, c->stream, X, br.dy[turn], br.w[l], br.vw[l], br.b[l],
                               br.vb[l], br.dy[turn ^ 1], B, K, N, lr, momentum);
        else
            hipLaunchKernelGGL(bridger_backward_kernel<false>, grid, block, 0, c->stream, X, br.dy[turn], br.w[l], br.vw[l], br.b[l],
                               br.vb[l], (float *)nullptr, B, K, N, lr, momentum);
        CAPDEC_HIP(hipGetLastError());
        turn ^= 1;
    }
    br.last_batch = B;
    return 0;
}

int dev_zero(std::vector<void *> &owned, size_t n, float **out) {
    void *p = nullptr;
    CAPDEC_HIP(hipMalloc(&p, n * sizeof(float)));
    owned.push_back(p);
    CAPDEC_HIP(hipMemset(p, 0, n * sizeof(float)));
    *out = reinterpret_cast<float *>(p);
    return 0;
}

int load_run(capdec_ctx *c, int L, const int *dims, const float *const *h_w, const float *const *h_b) {
    Bridger &br = c->bridger;
    br.L = L;
    int widest = 0;
    for (int l = 0; l <= L; ++l) {
        br.dims[l] = dims[l];
        widest = std::max(widest, dims[l]);
    }
    for (int l = 0; l < L; ++l) {
        const size_t nw = (size_t)dims[l + 1] * dims[l], nb = (size_t)dims[l + 1];
        CAPDEC_TRY(upload(br.owned, h_w[l], nw, &br.w[l]));
        CAPDEC_TRY(upload(br.owned, h_b[l], nb, &br.b[l]));
        CAPDEC_TRY(dev_zero(br.owned, nw, &br.vw[l]));
        CAPDEC_TRY(dev_zero(br.owned, nb, &br.vb[l]));
        CAPDEC_TRY(dev_zero(br.owned, (size_t)BRIDGER_MAX_BATCH * nb, &br.act[l]));
    }
    for (int i = 0; i < 2; ++i) CAPDEC_TRY(dev_zero(br.owned, (size_t)BRIDGER_MAX_BATCH * widest, &br.dy[i]));
    float *s = nullptr;
    static_assert(sizeof(BridgerScalars) % sizeof(float) == 0, "BridgerScalars is zeroed as floats");
    CAPDEC_TRY(dev_zero(br.owned, sizeof(BridgerScalars) / sizeof(float), &s));
    br.scal = reinterpret_cast<BridgerScalars *>(s);
    br.loaded = true;
    return 0;
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

int sync_after(capdec_ctx *c, int rc, const char *what) {
    if (hipStreamSynchronize(c->stream) != hipSuccess && rc == 0) {
        set_error(std::string(what) + ": hipStreamSynchronize failed");
        return 1;
    }
    return rc;
}

}  // namespace

}  // namespace capdec

using namespace capdec;

#define BRIDGER_LOADED(c, what)                                   \
    CAPDEC_CHECK(c, what ": null context");                       \
    CAPDEC_CHECK((c)->bridger.loaded, what ": no bridger is loaded (capdec_bridger_load)")

extern "C" {

int capdec_bridger_load(capdec_ctx *c, int num_layers, const int *h_dims, const float *const *h_w, const float *const *h_b) {
    CAPDEC_CHECK(c, "bridger_load: null context");
    CAPDEC_CHECK(num_layers >= 1 && num_layers <= BRIDGER_MAX_LAYERS, "bridger_load: 1 to 16 layers");
    CAPDEC_CHECK(h_dims && h_w && h_b, "bridger_load: null argument");
    for (int l = 0; l <= num_layers; ++l)
        CAPDEC_CHECK(h_dims[l] >= 4 && h_dims[l] <= BRIDGER_MAX_WIDTH && h_dims[l] % 4 == 0,
                     "bridger_load: every width must be a multiple of 4 in 4..1024");
    for (int l = 0; l < num_layers; ++l) CAPDEC_CHECK(h_w[l] && h_b[l], "bridger_load: null weight or bias");
    CAPDEC_HIP(hipSetDevice(c->device));
    CAPDEC_HIP(hipStreamSynchronize(c->stream));       // nothing enqueued still reads the bridger that goes
    free_all(c->bridger.owned);
    c->bridger = Bridger();
    const int rc = load_run(c, num_layers, h_dims, h_w, h_b);
    if (rc) {                                          // half a bridger is no bridger
        free_all(c->bridger.owned);
        c->bridger = Bridger();
    }
    return rc;
}

int capdec_bridger_forward(capdec_ctx *c, const float *d_x, int n, float *d_out) {
    BRIDGER_LOADED(c, "bridger_forward");
    CAPDEC_CHECK(n >= 0, "bridger_forward: negative row count");
    if (n == 0) return 0;
    CAPDEC_CHECK(d_x && d_out, "bridger_forward: null argument");
    CAPDEC_CHECK(aligned16(d_x) && aligned16(d_out), "bridger_forward: d_x and d_out must be 16-byte aligned");
    CAPDEC_HIP(hipSetDevice(c->device));
    return sync_after(c, forward_rows(c, d_x, n, d_out), "bridger_forward");
}

int capdec_bridger_train_step(capdec_ctx *c, const float *d_x, const float *d_y, int batch, float lr, float momentum, float *loss) {
    BRIDGER_LOADED(c, "bridger_train_step");
    CAPDEC_CHECK(batch >= 1 && batch <= BRIDGER_MAX_BATCH, "bridger_train_step: batch must be 1..64");
    CAPDEC_CHECK(d_x && d_y, "bridger_train_step: null argument");
    CAPDEC_CHECK(aligned16(d_x) && aligned16(d_y), "bridger_train_step: d_x and d_y must be 16-byte aligned");
    CAPDEC_HIP(hipSetDevice(c->device));
    CAPDEC_TRY(step_enqueue(c, d_x, d_y, batch, lr, momentum));
    if (loss) {                                        // loss == NULL: nothing waits for the device
        CAPDEC_HIP(hipMemcpyAsync(loss, &c->bridger.scal->last, sizeof(float), hipMemcpyDeviceToHost, c->stream));
        CAPDEC_HIP(hipStreamSynchronize(c->stream));
    }
    return 0;
}

int capdec_bridger_train_epoch(capdec_ctx *c, const float *d_x, const float *d_y, int n, int batch, float lr, float momentum) {
    BRIDGER_LOADED(c, "bridger_train_epoch");
    CAPDEC_CHECK(n >= 0, "bridger_train_epoch: negative row count");
    CAPDEC_CHECK(batch >= 1 && batch <= BRIDGER_MAX_BATCH, "bridger_train_epoch: batch must be 1..64");
    if (n == 0) return 0;
    CAPDEC_CHECK(d_x && d_y, "bridger_train_epoch: null argument");
    CAPDEC_CHECK(aligned16(d_x) && aligned16(d_y), "bridger_train_epoch: d_x and d_y must be 16-byte aligned");
    CAPDEC_HIP(hipSetDevice(c->device));
    const Bridger &br = c->bridger;
    for (int r0 = 0; r0 < n; r0 += batch)              // torch's DataLoader, unshuffled, drop_last = False
        CAPDEC_TRY(step_enqueue(c, d_x + (size_t)r0 * br.dims[0], d_y + (size_t)r0 * br.dims[br.L], std::min(batch, n - r0), lr,
                                momentum));
    return 0;
}

int capdec_bridger_eval(capdec_ctx *c, const float *d_x, const float *d_y, int n, int batch, double *loss_sum, long long *batches) {
    BRIDGER_LOADED(c, "bridger_eval");
    CAPDEC_CHECK(n >= 0, "bridger_eval: negative row count");
    CAPDEC_CHECK(batch >= 1, "bridger_eval: batch must be at least 1");
    if (loss_sum) *loss_sum = 0.0;
    if (batches) *batches = 0;
    if (n == 0) return 0;
    CAPDEC_CHECK(d_x && d_y, "bridger_eval: null argument");
    CAPDEC_CHECK(aligned16(d_x) && aligned16(d_y), "bridger_eval: d_x and d_y must be 16-byte aligned");
    CAPDEC_HIP(hipSetDevice(c->device));
    Bridger &br = c->bridger;
    const int nb = (n - 1) / batch + 1, NL = br.dims[br.L];
    CAPDEC_TRY(c->br_ev.ensure(((size_t)n * NL + nb) * sizeof(float)));
    float *out = c->br_ev.as<float>(), *losses = out + (size_t)n * NL;
    CAPDEC_TRY(forward_rows(c, d_x, n, out));          // a row's output does not depend on its batch
    {
        ProfScope ps(c, F_OTHER);
        hipLaunchKernelGGL(bridger_loss_kernel, dim3(nb), dim3(BRIDGER_LOSS_THREADS), 0, c->stream, out, d_y, n, batch, NL, (float *)nullptr,
                           br.scal, losses, 0);
        CAPDEC_HIP(hipGetLastError());
        hipLaunchKernelGGL(bridger_eval_sum_kernel, dim3(1), dim3(1), 0, c->stream, losses, (long long)nb, br.scal);
        CAPDEC_HIP(hipGetLastError());
    }
    BridgerScalars h;
    CAPDEC_HIP(hipMemcpyAsync(&h, br.scal, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    CAPDEC_HIP(hipStreamSynchronize(c->stream));
    if (loss_sum) *loss_sum = h.eval_sum;
    if (batches) *batches = h.eval_batches;
    return 0;
}

int capdec_bridger_loss(capdec_ctx *c, float *last, double *sum, long long *steps, int reset) {
    BRIDGER_LOADED(c, "bridger_loss");
    CAPDEC_HIP(hipSetDevice(c->device));
    BridgerScalars h;
    CAPDEC_HIP(hipMemcpyAsync(&h, c->bridger.scal, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    CAPDEC_HIP(hipStreamSynchronize(c->stream));
    if (last) *last = h.last;
    if (sum) *sum = h.sum;
    if (steps) *steps = h.steps;
    if (reset) {                                       // the last loss stays; the sum and the count start again
        CAPDEC_HIP(hipMemsetAsync(&c->bridger.scal->sum, 0, sizeof(double) + sizeof(long long), c->stream));
        CAPDEC_HIP(hipStreamSynchronize(c->stream));
    }
    return 0;
}

int capdec_bridger_get(capdec_ctx *c, int kind, int which, float *d_out, size_t n) {
    BRIDGER_LOADED(c, "bridger_get");
    CAPDEC_CHECK(d_out, "bridger_get: null argument");
    const Bridger &br = c->bridger;
    const float *src = nullptr;
    size_t count = 0;
    if (kind == 0 || kind == 1) {
        CAPDEC_CHECK(which >= 0 && which < 2 * br.L, "bridger_get: which must be in [0, 2 L)");
        const int l = which / 2;
        if (which % 2 == 0) {
            src = kind == 0 ? br.w[l] : br.vw[l];
            count = (size_t)br.dims[l + 1] * br.dims[l];
        } else {
            src = kind == 0 ? br.b[l] : br.vb[l];
            count = (size_t)br.dims[l + 1];
        }
    } else if (kind == 2) {
        CAPDEC_CHECK(which >= 0 && which < br.L, "bridger_get: which must be in [0, L)");
        CAPDEC_CHECK(br.last_batch > 0, "bridger_get: no train step since the load");
        src = br.act[which];
        count = (size_t)br.last_batch * br.dims[which + 1];
    } else {
        CAPDEC_CHECK(false, "bridger_get: kind must be 0 (parameter), 1 (momentum buffer) or 2 (activation)");
    }
    CAPDEC_CHECK(n == count, "bridger_get: n does not match the tensor's size");
    CAPDEC_HIP(hipSetDevice(c->device));
    CAPDEC_HIP(hipMemcpyAsync(d_out, src, count * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    CAPDEC_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

}  // extern "C"
