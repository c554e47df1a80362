// fp32-accurate GEMM on the fp16 matrix cores with THREE MFMAs per product:  C[M,N] = epi( A[M,K] . Bt[N,K]^T )
//
// Why: rocprofv3 SQ counters of the six-product split-bf16 kernel (profiles/r2_pmc_sq_gemm_bf16x3p.txt) show the
// matrix pipe busy 71-78 % of the kernel's cycles and the waves issue-stalled on it 61 % of their time: that kernel
// is matrix-pipe-bound in cycles (the rest of the distance to the datasheet peak is clock), so the lever is FEWER
// MFMAs per fp32 product, not a denser schedule of the same six.
//
// How (format PK_F16X2, bf16x3.h): every fp32 value is  a = hi + 2^-11 lo  with two fp16 planes (11 + 11 significand
// bits, the low plane stored scaled by 2^11 so it never leaves fp16's normal range), hence
//     a b = hi_a hi_b + 2^-11 (hi_a lo_b + lo_a hi_b) + [2^-22 lo_a lo_b, dropped]
// The dropped term is <= 2^-22 |a b| (rms 2^-24.6 |a b|): measured against fp64 the result sits BELOW the rounding
// noise of an ordinary fp32 GEMM (max error / sum |a||b|: 2e-8 on unit-scale data, 1.7e-7 with a 10^6 dynamic range
// across k; torch's own fp32 matmul: 1.5e-7 / 2.4e-7).  v_mfma_f32_32x32x16_f16 products are exact in fp32 and
// accumulate in fp32; the 2^-11-weighted cross terms have their own accumulator set, joined once in the epilogue.
// Ceiling = dense fp16 MFMA peak / 3 = 833 TFLOP/s fp32-equivalent (the six-product scheme: 417).
//
// Structure: the packed-A LDS-DMA main loop of gemm_bf16x3.hip with 2 planes: 128x128 tile, 4 wavefronts x (2x2)
// 32x32 tiles x 2 accumulator sets (128 accumulator registers), BK = 16 per stage, stage = A block + B block =
// 16 KB, ring of NS stages (4: 64 KB, two blocks per CU).  Per k-step a wavefront issues 8 ds_read_b128 (tile
// kt+1 into the other fragment set), 4 LDS-DMA pieces (tile kt+NS) and 12 MFMAs (tile kt, from registers); one
// counted s_waitcnt vmcnt(4 (NS-2)) lgkmcnt(0) + raw s_barrier per k-step.  MFMA time per k-step halves against
// the six-product kernel, so the ring is one stage deeper to keep the same DMA lead in cycles.
#include <algorithm>
#include <cstdlib>

#include "bf16x3.h"
#include "gemm_epilogue.h"
#include "gemm_epilogue_lds.h"
#include "gemm_packed.h"

namespace capdec {

constexpr int H2_STAGE_B = 2 * H2_BLOCK_B;                 // 16 KB: A block + B block of one k-step
constexpr int H2_TOPK_LDS = 128 * CT_LD * 4;               // 66 048 B: logits tile of the fused lm_head epilogue
template <int NS> struct H2Geo {
    static constexpr int SMEM_B = NS * H2_STAGE_B > H2_TOPK_LDS ? NS * H2_STAGE_B : H2_TOPK_LDS;
};

// fp32 [N, K] -> two fp16 planes, TILE-MAJOR  out[tile][k_step][plane][row 0..127][16 fp16]  (rows past N zero):
// byte-for-byte the LDS image of one operand of a stage (16-B halves of a row swapped when bit 3 of the row is set)
__global__ void pack_planes_h2_kernel(const float *__restrict__ w, int ldw, _Float16 *__restrict__ out, int N, int K,
                                      int nk) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;   // one thread per (tile, k_step, row, half): 8 k
    const int tiles = (N + GEMM_BN - 1) / GEMM_BN;
    if (i >= (size_t)tiles * nk * 256) return;
    const int hk = i & 1, r = (i >> 1) & 127;
    const size_t tk = i >> 8;                       // tile * nk + k_step
    const int ks = (int)(tk % nk), tile = (int)(tk / nk);
    const int n = tile * GEMM_BN + r;
    float4 v0 = make_float4(0.f, 0.f, 0.f, 0.f), v1 = v0;
    if (n < N) {
        const float *src = w + (size_t)n * ldw + ks * 16 + hk * 8;
        v0 = reinterpret_cast<const float4 *>(src)[0];
        v1 = reinterpret_cast<const float4 *>(src)[1];
    }
    f16x4 h0, l0, h1, l1;
    split2h(v0, h0, l0);
    split2h(v1, h1, l1);
    _Float16 *dst = out + tk * (2 * 128 * 16) + r * 16 + ((hk ^ ((r >> 3) & 1)) << 3);
    reinterpret_cast<f16x4 *>(dst)[0] = h0;
    reinterpret_cast<f16x4 *>(dst)[1] = h1;
    reinterpret_cast<f16x4 *>(dst + 2048)[0] = l0;
    reinterpret_cast<f16x4 *>(dst + 2048)[1] = l1;
}

int launch_pack_planes_h2(hipStream_t st, const float *w, int ldw, int N, int K, void *out) {
    CAPDEC_CHECK(K % 64 == 0 && ldw % 4 == 0, "pack_planes_h2: K must be a multiple of 64");
    const int nk = K / X3_BK;
    const size_t tot = (size_t)((N + GEMM_BN - 1) / GEMM_BN) * nk * 256;
    hipLaunchKernelGGL(pack_planes_h2_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, w, ldw,
                       (_Float16 *)out, N, K, nk);
    CAPDEC_HIP(hipGetLastError());
    return 0;
}

// The TRANSPOSE of an fp32 matrix as a packed operand: src [rows][cols] row-major (row stride ld)  ->  the two fp16 planes of
// Mt [cols][Kp] (Mt[n][k] = src[k][n]; k >= rows zero-filled up to Kp, a multiple of 64; rows n >= cols of the last 128-row
// tile zero) -- the operands of a weight-gradient product dW = dY^T X, whose K runs over the ROWS of dY and X.  One block
// per 64 x 64 tile: rows read coalesced, transposed through LDS, every thread splits one (n, k-step) = 16 consecutive k.
// (Replaces a transpose_pad launch -- fp32 written and read back -- in front of the packer, train_ops.hip.)
__global__ __launch_bounds__(256) void pack_planes_h2_t_kernel(const float *__restrict__ src, int ld, int rows, int cols,
                                                               _Float16 *__restrict__ out, int nk) {
    __shared__ float tile[64][65];
    const int t = threadIdx.x, n0 = blockIdx.x * 64, k0 = blockIdx.y * 64;
    for (int i = t; i < 64 * 64; i += 256) {
        const int kk = i >> 6, nn = i & 63, k = k0 + kk, n = n0 + nn;
        tile[kk][nn] = (k < rows && n < cols) ? src[(size_t)k * ld + n] : 0.f;
    }
    __syncthreads();
    const int nn = t & 63, kq = t >> 6, n = n0 + nn;
    const int tl = n >> 7, r = n & 127, ks = (k0 >> 4) + kq;
    _Float16 *dst = out + ((size_t)tl * nk + ks) * (2 * 128 * 16) + r * 16;
#pragma unroll
    for (int hk = 0; hk < 2; ++hk) {
        float4 v0, v1;
        v0.x = tile[kq * 16 + hk * 8 + 0][nn]; v0.y = tile[kq * 16 + hk * 8 + 1][nn];
        v0.z = tile[kq * 16 + hk * 8 + 2][nn]; v0.w = tile[kq * 16 + hk * 8 + 3][nn];
        v1.x = tile[kq * 16 + hk * 8 + 4][nn]; v1.y = tile[kq * 16 + hk * 8 + 5][nn];
        v1.z = tile[kq * 16 + hk * 8 + 6][nn]; v1.w = tile[kq * 16 + hk * 8 + 7][nn];
        f16x4 h0, l0, h1, l1;
        split2h(v0, h0, l0);
        split2h(v1, h1, l1);
        _Float16 *d = dst + ((hk ^ ((r >> 3) & 1)) << 3);
        reinterpret_cast<f16x4 *>(d)[0] = h0;
        reinterpret_cast<f16x4 *>(d)[1] = h1;
        reinterpret_cast<f16x4 *>(d + 2048)[0] = l0;
        reinterpret_cast<f16x4 *>(d + 2048)[1] = l1;
    }
}
// out: x3_packed_bytes(cols, Kp, PK_F16X2) bytes
int launch_pack_planes_h2_t(hipStream_t st, const float *src, int ld, int rows, int cols, int Kp, void *out) {
    CAPDEC_CHECK(Kp % 64 == 0 && Kp >= rows && rows > 0 && cols > 0 && ld >= cols, "pack_planes_h2_t: K (padded rows) must be a multiple of 64");
    const int npad = (cols + 127) / 128 * 128;
    hipLaunchKernelGGL(pack_planes_h2_t_kernel, dim3(npad / 64, Kp / 64), dim3(256), 0, st, src, ld, rows, cols, (_Float16 *)out, Kp / X3_BK);
    CAPDEC_HIP(hipGetLastError());
    return 0;
}

// TR: MFMA operands swapped (D^T), a lane ends with four consecutive columns of one row (see gemm_bf16x3.hip).
// am = sum hi_a hi_b, ac = sum (hi_a lo_b + lo_a hi_b) (weight 2^-11, applied by h2_join).
// KIND: 0 = f16x2 (the fp32-accurate scheme above).  1 / 2 = ONE-plane fp16 / bf16 operands (formats PK_F16X1 /
// PK_BF16X1: the reduced-precision modes, one MFMA per product): the same ring, DMA pieces and fragment reads, but a
// stage holds TWO consecutive k-steps of the single plane where f16x2 holds the two planes of one k-step (both are
// 2 x 4 KB contiguous per operand), so a stage is 32 deep and carries 8 MFMAs per wavefront instead of 12.
// CONV (implicit-GEMM 3x3 convolution, stride 1, padding 1; resnet.hip / capi.hip): the A operand is not an im2col
// matrix but the ACTIVATION itself in packed form -- rows = pixels of an NHWC tensor [M = N H W][C], the very layout a
// GEMM epilogue writes with packed_out -- and K runs over (tap, channel): K = 9 C, stage ks = tap * ncs + cs.  Row m of
// the product is output pixel m, whose operand row for tap (ky, kx) is input pixel m + (ky - 1) W + (kx - 1) (stride 1:
// output and input pixels share their index) or a row of zeros outside the image.  Each thread owns the same 16-byte
// piece of the stage as in the GEMM (row t / 2, half t & 1) and re-derives its source address when the tap changes --
// nine times per tile; a piece is a 16-byte half of a 32-byte row chunk whose position inside the chunk depends on bit 3
// of the row (the LDS swizzle), so a piece copied from source row rs to tile row rd sits at half ^ sw(rd) ^ sw(rs).
struct ConvGeo {
    int H = 0, W = 0, M = 0;      // image height / width (pixels), rows of the product (= N H W)
    int ncs = 0;                  // stages per tap: C / 16 (two-plane f16x2) or C / 32 (one-plane formats)
    const char *zero = nullptr;   // >= ncs * 8 KB + 8 KB of zeros: the operand rows of the padding
};

template <bool TR, int NS, int KIND = 0, bool CONV = false>
__device__ __forceinline__ void h2p_mainloop(const _Float16 *__restrict__ Apk, const _Float16 *__restrict__ Bpk, int K,
                                             int tm, int tn, char *smem, f32x16 (&am)[2][2], f32x16 (&ac)[2][2],
                                             int ks0 = 0, int nks = -1, const ConvGeo cg = ConvGeo()) {
    static_assert(NS >= 3 && NS <= 9, "ring depth");
    const int t = threadIdx.x;
    const int lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int half = lane >> 5, l32 = lane & 31;
    const int nkf = K / (KIND == 0 ? X3_BK : 2 * X3_BK);                       // stages of the whole K (panel stride)
    const int nk = nks < 0 ? nkf : nks;                                        // stages of THIS block, even
    const _Float16 *ap = Apk + ((size_t)tm * nkf + ks0) * (H2_BLOCK_B / 2) + t * 8;    // this thread's 16-B piece
    const _Float16 *bp = Bpk + ((size_t)tn * nkf + ks0) * (H2_BLOCK_B / 2) + t * 8;
    char *dst0 = smem + wave * 1024;                                           // wave-uniform LDS base of its pieces
    // CONV: running (stage, tap, stage-in-tap) of the NEXT tile to send (the DMAs are issued in increasing stage order,
    // clamped at the last one) and this thread's source for the current tap
    int cv_ks = 0, cv_cs = 0, cv_tap = 0, cv_ox = 0, cv_oy = 0, cv_m = 0;
    bool cv_ok = false;
    const char *cv_cur = nullptr;
    auto cv_src = [&](int tap) -> const char * {
        const int ky = tap / 3, kx = tap - 3 * ky;
        const int iy = cv_oy + ky - 1, ix = cv_ox + kx - 1;
        const bool ok = cv_ok && (unsigned)iy < (unsigned)cg.H && (unsigned)ix < (unsigned)cg.W;
        const int pin = cv_m + (ky - 1) * cg.W + (kx - 1), pr = pin & 127;
        const size_t off = (size_t)(pin >> 7) * cg.ncs * H2_BLOCK_B + pr * X3_ROW_B +
                           ((((t & 1) ^ ((t >> 4) & 1) ^ ((pr >> 3) & 1))) << 4);
        return ok ? reinterpret_cast<const char *>(Apk) + off : cg.zero + ((t & 1) << 4);
    };
    if constexpr (CONV) {
        cv_m = tm * GEMM_BM + (t >> 1);
        cv_ok = cv_m < cg.M;
        if (!cv_ok) cv_m = 0;
        cv_ox = cv_m % cg.W;
        cv_oy = (cv_m / cg.W) % cg.H;
        cv_cur = cv_src(0);
    }
#define H2_DMA(stage, ks_)                                                                                     \
    {                                                                                                          \
        char *d = dst0 + (stage) * H2_STAGE_B;                                                                 \
        if constexpr (CONV) {                                                                                  \
            const char *sa = cv_cur + (size_t)cv_cs * H2_BLOCK_B;                                              \
            const _Float16 *sb = bp + (size_t)cv_ks * (H2_BLOCK_B / 2);                                        \
            _Pragma("unroll") for (int p = 0; p < 2; ++p) {                                                    \
                __builtin_amdgcn_global_load_lds((glb_void *)(sa + p * X3_PLANE_B), (lds_void *)(d + p * X3_PLANE_B), 16, 0, 0); \
                __builtin_amdgcn_global_load_lds((glb_void *)(sb + p * 2048), (lds_void *)(d + H2_BLOCK_B + p * X3_PLANE_B), 16, 0, 0); \
            }                                                                                                  \
            if (cv_ks < nk - 1) {                                                                              \
                ++cv_ks;                                                                                       \
                if (++cv_cs == cg.ncs) { cv_cs = 0; ++cv_tap; cv_cur = cv_src(cv_tap); }                       \
            }                                                                                                  \
        } else {                                                                                               \
            const _Float16 *sa = ap + (size_t)(ks_) * (H2_BLOCK_B / 2), *sb = bp + (size_t)(ks_) * (H2_BLOCK_B / 2); \
            _Pragma("unroll") for (int p = 0; p < 2; ++p) {                                                    \
                __builtin_amdgcn_global_load_lds((glb_void *)(sa + p * 2048), (lds_void *)(d + p * X3_PLANE_B), 16, 0, 0); \
                __builtin_amdgcn_global_load_lds((glb_void *)(sb + p * 2048), (lds_void *)(d + H2_BLOCK_B + p * X3_PLANE_B), 16, 0, 0); \
            }                                                                                                  \
        }                                                                                                      \
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) { am[i][j][r] = 0.f; ac[i][j][r] = 0.f; }

    const int swz = ((half ^ ((l32 >> 3) & 1)) << 4);
    const int a_rd = (wm * 64 + l32) * X3_ROW_B + swz;
    const int b_rd = H2_BLOCK_B + (wn * 64 + l32) * X3_ROW_B + swz;

    f16x8 f0a0[2], f0a1[2], f0b0[2], f0b1[2], f1a0[2], f1a1[2], f1b0[2], f1b1[2];
#define H2_READ(F, stage)                                                                           \
    {                                                                                               \
        const char *rs = smem + (stage) * H2_STAGE_B;                                               \
        _Pragma("unroll") for (int p = 0; p < 2; ++p) {                                             \
            F##a0[p] = *reinterpret_cast<const f16x8 *>(rs + p * X3_PLANE_B + a_rd);                 \
            F##a1[p] = *reinterpret_cast<const f16x8 *>(rs + p * X3_PLANE_B + a_rd + 32 * X3_ROW_B); \
            F##b0[p] = *reinterpret_cast<const f16x8 *>(rs + p * X3_PLANE_B + b_rd);                 \
            F##b1[p] = *reinterpret_cast<const f16x8 *>(rs + p * X3_PLANE_B + b_rd + 32 * X3_ROW_B); \
        }                                                                                           \
    }
#define H2_MM1(x, y, c) (KIND == 2 ? __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, x), __builtin_bit_cast(bf16x8, y), c, 0, 0, 0) \
                                   : __builtin_amdgcn_mfma_f32_32x32x16_f16(x, y, c, 0, 0, 0))
#define H2_MM(x, y, c) (TR ? H2_MM1(y, x, c) : H2_MM1(x, y, c))
#define H2_TERM(ACC, F, pa, pb)                                \
    ACC[0][0] = H2_MM(F##a0[pa], F##b0[pb], ACC[0][0]);        \
    ACC[0][1] = H2_MM(F##a0[pa], F##b1[pb], ACC[0][1]);        \
    ACC[1][0] = H2_MM(F##a1[pa], F##b0[pb], ACC[1][0]);        \
    ACC[1][1] = H2_MM(F##a1[pa], F##b1[pb], ACC[1][1]);
#define H2_MFMAS(F)                                                                      \
    if constexpr (KIND == 0) { H2_TERM(ac, F, 1, 0) H2_TERM(am, F, 0, 0) H2_TERM(ac, F, 0, 1) } \
    else { H2_TERM(am, F, 0, 0) H2_TERM(am, F, 1, 1) }
    // (the s_waitcnt builtin, not inline asm: the compiler's own waitcnt pass must see that the fragment reads have
    //  completed, or it puts an lgkmcnt(0) in front of the next MFMAs -- behind the freshly issued reads)
#define H2_SYNC()                                                                        \
    asm volatile("" ::: "memory");                                                       \
    __builtin_amdgcn_s_waitcnt(waitcnt_imm(4 * (NS - 2), 0));                            \
    __builtin_amdgcn_s_barrier();                                                        \
    asm volatile("" ::: "memory");
    // one memory operation in the shadow of each MFMA: 8 fragment reads, then the 4 DMA pieces
#define H2_INTERLEAVE()                                                                    \
    if constexpr (KIND == 0) {                                                             \
        _Pragma("unroll") for (int i_ = 0; i_ < 8; ++i_) {                                 \
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);   /* 1 MFMA    */           \
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);   /* 1 DS read */           \
        }                                                                                  \
        _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_) {                                 \
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                             \
            __builtin_amdgcn_sched_group_barrier(0x010, 1, 0);   /* 1 VMEM (LDS-DMA piece) */ \
        }                                                                                  \
    } else {   /* 8 MFMAs: 4 x (MFMA, 2 reads), 4 x (MFMA, 1 DMA piece) */                 \
        _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_) {                                 \
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                             \
            __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);                             \
        }                                                                                  \
        _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_) {                                 \
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                             \
            __builtin_amdgcn_sched_group_barrier(0x010, 1, 0);                             \
        }                                                                                  \
    }                                                                                      \
    __builtin_amdgcn_sched_barrier(0);

    // prologue: tiles 0 .. NS-1 in flight (stage s <- tile s); tile 0 landed -> fragments f0; tile 1 landed
#pragma unroll
    for (int s = 0; s < NS; ++s) H2_DMA(s, min(s, nk - 1))
    __builtin_amdgcn_s_waitcnt(waitcnt_imm(4 * (NS - 1), 15));    // tile 0 landed
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    H2_READ(f0, 0)
    H2_SYNC()                                                    // tile 1 landed, this wave's reads of stage 0 done
    // k-step kt: fragments of tile kt+1 are read from stage (kt+1)%NS, tile kt+NS is sent to stage kt%NS (whose
    // fragments every wave finished reading before the barrier that ended k-step kt-1), the MFMAs of tile kt run from
    // registers.  End of k-step: all but the NS-2 newest tiles have landed => tile kt+2 is in LDS.
    int s0 = 0;                                                  // kt % NS
    for (int kt = 0; kt < nk; kt += 2) {
        const int s1 = s0 + 1 == NS ? 0 : s0 + 1, s2 = s1 + 1 == NS ? 0 : s1 + 1;
        H2_READ(f1, s1)                                          // tile kt+1
        H2_DMA(s0, min(kt + NS, nk - 1))                         // unconditional (clamped): exact vmcnt count
        H2_MFMAS(f0)                                             // tile kt
        H2_INTERLEAVE()
        H2_SYNC()
        H2_READ(f0, s2)                                          // tile kt+2
        H2_DMA(s1, min(kt + 1 + NS, nk - 1))
        H2_MFMAS(f1)                                             // tile kt+1
        H2_INTERLEAVE()
        H2_SYNC()
        s0 = s2;
    }
    __builtin_amdgcn_s_waitcnt(waitcnt_imm(0, 15));              // clamped tail pieces must land before LDS is reused
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
#undef H2_DMA
#undef H2_READ
#undef H2_TERM
#undef H2_MM
#undef H2_MM1
#undef H2_MFMAS
#undef H2_SYNC
#undef H2_INTERLEAVE
}

// acc = am + 2^-11 ac
__device__ __forceinline__ void h2_join(f32x16 (&am)[2][2], const f32x16 (&ac)[2][2]) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) am[i][j][r] = fmaf(ac[i][j][r], 1.0f / H2_LO_SCALE, am[i][j][r]);
}

constexpr int H2_NS = 4;
// wave grid of the 128 x 128 kernels for the coalesced epilogues (gemm_epilogue_lds.h): 2 x 2 wavefronts of 64 x 64
struct H2Tile { static constexpr int WN = 2, TI = 2, TJ = 2; };

// f(std::integral_constant<int, KIND>()) for the KIND of a runtime operand format (the caller has checked the format)
template <class F>
inline void with_kind(int fmt, F &&f) {
    if (fmt == PK_F16X2) f(std::integral_constant<int, 0>());
    else if (fmt == PK_F16X1) f(std::integral_constant<int, 1>());
    else f(std::integral_constant<int, 2>());
}

__device__ __forceinline__ EpiArgs h2_epi_args(float *C, int ldc, int M, int N, int m0, int n0, const float *bias,
                                               const float *resid, int ldr, int act, char *packed_out, int fmt,
                                               const QkvScatter *sc) {
    EpiArgs ea;
    ea.C = C; ea.ldc = ldc; ea.M = M; ea.N = N; ea.m0 = m0; ea.n0 = n0;
    ea.bias = bias; ea.act = act; ea.ldr = ldr; ea.fmt = fmt;
    ea.packed = packed_out;
    if (packed_out) ea.resid_pk = reinterpret_cast<const char *>(resid);      // (with packed_out, `resid` is a PACKED residual)
    else ea.resid = resid;
    ea.sc = sc;
    return ea;
}

// (gemm_f16x2p_kernel and gemm_x1_kernel stay two kernels: a one-plane launch also names its output format, and sharing
//  their text through one device function changed the code the compiler emits for them)
template <bool VEC4, int NS>
__global__ __launch_bounds__(256, 2) void gemm_f16x2p_kernel(const _Float16 *__restrict__ Apk,
                                                             const _Float16 *__restrict__ Bpk, float *C, int ldc, int M,
                                                             int N, int K, const float *__restrict__ bias,
                                                             const float *resid, int ldr, int act, int tiles_m,
                                                             int tiles_n, char *packed_out, QkvScatter sc) {
    __shared__ __attribute__((aligned(16))) char smem[NS * H2_STAGE_B];
    // Persistent form: the launch has min(tiles, slots) blocks (two per CU: gemm_plan.h) and block b walks tiles b,
    // b + grid, ...  The hardware hands the blocks of a launch out breadth-first (one per CU, then the second slots), so the
    // tiles of a partly filled last round are taken one per CU by blocks that by then have the CU to themselves -- where one
    // block per tile lets the dispatcher put the leftovers two to a CU as slots free up (600 tiles: 2 x 37 us instead of
    // 37 + 15).  grid % 8 == 0 keeps a block's tiles on its own XCD's slice of the tile order.
    const int ntiles = tiles_m * tiles_n;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        int tm, tn;
        tile_coords(tiles_m, tiles_n, tm, tn, tile);
        f32x16 am[2][2], ac[2][2];
        h2p_mainloop<true, NS>(Apk, Bpk, K, tm, tn, smem, am, ac);      // ends with a barrier: the ring is free again
        h2_join(am, ac);
        if constexpr (VEC4) {
            const EpiArgs ea = h2_epi_args(C, ldc, M, N, tm * GEMM_BM, tn * GEMM_BN, bias, resid, ldr, act, packed_out, PK_F16X2, &sc);
            // (<.., true>: the tile's bias and residual quads are requested before the transposition -- the cross-term
            //  accumulators are dead after h2_join, their registers hold the 16 residual quads; gemm_epilogue_lds.h)
            epilogue_lds<H2Tile, true>(am, smem, ea);
            slab_release(tile + (int)gridDim.x < ntiles);
        } else if (packed_out) {
            epilogue_store_packed_t(am, packed_out, N >> 4, M, N, tm * GEMM_BM, tn * GEMM_BN, bias, act, PK_F16X2,
                                    reinterpret_cast<const char *>(resid));  // (with packed_out, `resid` is a PACKED residual)
        } else {
            epilogue_store_t<false>(am, C, ldc, M, N, tm * GEMM_BM, tn * GEMM_BN, bias, resid, ldr, act);
        }
    }
}

// one-plane (reduced-precision) operands on the same main loop: KIND 1 = fp16, 2 = bf16
// (NS = 4: 64 KB, two blocks per CU; NS = 3: 48 KB and <= 168 registers, THREE blocks per CU -- the vec4 form)
template <bool VEC4, int KIND, int NS>
__global__ __launch_bounds__(256, (NS == 3 ? 3 : 2)) void gemm_x1_kernel(const _Float16 *__restrict__ Apk, const _Float16 *__restrict__ Bpk,
                                                         float *C, int ldc, int M, int N, int K,
                                                         const float *__restrict__ bias, const float *resid, int ldr,
                                                         int act, int tiles_m, int tiles_n, char *packed_out, int out_fmt,
                                                         QkvScatter sc) {
    __shared__ __attribute__((aligned(16))) char smem[NS * H2_STAGE_B];
    const int ntiles = tiles_m * tiles_n;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {          // persistent form: see gemm_f16x2p_kernel
        int tm, tn;
        tile_coords(tiles_m, tiles_n, tm, tn, tile);
        f32x16 am[2][2], ac[2][2];
        h2p_mainloop<true, NS, KIND>(Apk, Bpk, K, tm, tn, smem, am, ac);
        if constexpr (VEC4) {
            const EpiArgs ea = h2_epi_args(C, ldc, M, N, tm * GEMM_BM, tn * GEMM_BN, bias, resid, ldr, act, packed_out, out_fmt, &sc);
            epilogue_lds<H2Tile>(am, smem, ea);
            slab_release(tile + (int)gridDim.x < ntiles);
        } else if (packed_out) {
            epilogue_store_packed_t(am, packed_out, N >> 4, M, N, tm * GEMM_BM, tn * GEMM_BN, bias, act, out_fmt,
                                    reinterpret_cast<const char *>(resid));  // (with packed_out, `resid` is a PACKED residual)
        } else {
            epilogue_store_t<false>(am, C, ldc, M, N, tm * GEMM_BM, tn * GEMM_BN, bias, resid, ldr, act);
        }
    }
}

template <int KSEL, int KIND>
__global__ __launch_bounds__(256, 2) void gemm_f16x2p_topk_kernel(const _Float16 *__restrict__ Apk,
                                                                  const _Float16 *__restrict__ Bpk, int M, int N, int K,
                                                                  float inv_temp, float *tile_max, float *tile_sum,
                                                                  float *cand_val, int *cand_idx, int tiles_m,
                                                                  int tiles_n) {
    __shared__ __attribute__((aligned(16))) char smem[H2Geo<H2_NS>::SMEM_B];
    int tm, tn;
    tile_coords(tiles_m, tiles_n, tm, tn);
    f32x16 am[2][2], ac[2][2];
    h2p_mainloop<false, H2_NS, KIND>(Apk, Bpk, K, tm, tn, smem, am, ac);      // ends with a barrier
    if constexpr (KIND == 0) h2_join(am, ac);
    epilogue_topk<KSEL, 2, true>(am, reinterpret_cast<float *>(smem), M, N, tm * GEMM_BM, tn * GEMM_BN, tn, tiles_n, inv_temp,
                                 tile_max, tile_sum, cand_val, cand_idx);
}

// split-K for under-filled grids: raw fp32 partial tiles to a workspace [S][M][N], summed in a fixed order by
// splitk_reduce_kernel (gemm_bf16x3.hip), which also applies the epilogue
template <int KIND>
__global__ __launch_bounds__(256, 2) void gemm_f16x2p_splitk_kernel(const _Float16 *__restrict__ Apk,
                                                                    const _Float16 *__restrict__ Bpk, float *part, int M,
                                                                    int N, int K, int tiles_m, int tiles_n, int S) {
    __shared__ __attribute__((aligned(16))) char smem[H2_NS * H2_STAGE_B];
    const int ntiles = tiles_m * tiles_n;
    const int slice = blockIdx.x / ntiles;
    int tm, tn;
    tile_coords(tiles_m, tiles_n, tm, tn, blockIdx.x - slice * ntiles);
    const int nks = K / (KIND == 0 ? X3_BK : 2 * X3_BK) / S;      // stages of this slice (one-plane: two k-steps each)
    f32x16 am[2][2], ac[2][2];
    h2p_mainloop<true, H2_NS, KIND>(Apk, Bpk, K, tm, tn, smem, am, ac, slice * nks, nks);
    if constexpr (KIND == 0) h2_join(am, ac);
    const EpiArgs ea = h2_epi_args(part + (size_t)slice * M * N, N, M, N, tm * GEMM_BM, tn * GEMM_BN, nullptr, nullptr, 0,
                                   CAPDEC_ACT_NONE, nullptr, PK_F16X2, nullptr);
    epilogue_lds_wave<2, 2, 0, CAPDEC_ACT_NONE>(am, reinterpret_cast<float *>(smem + (threadIdx.x >> 6) * EpiSlab<2>::BYTES),
                                                ea.m0 + (threadIdx.x >> 7) * 64, ea.n0 + ((threadIdx.x >> 6) & 1) * 64, ea);
}

// the same kernel (k = 5) over *m_dev rows of a compacted A operand: the exact second pass of the fused lm_head in the
// one-plane modes (decode.hip: lm_head_select; two-plane form: gemm_h2w.hip: gemm_h2w_topk_dev_kernel)
template <int KIND>
__global__ __launch_bounds__(256, 2) void gemm_x1_topk_dev_kernel(const _Float16 *__restrict__ Apk,
                                                                  const _Float16 *__restrict__ Bpk,
                                                                  const int *__restrict__ m_dev, int N, int K, float inv_temp,
                                                                  float *tile_max, float *tile_sum, float *cand_val,
                                                                  int *cand_idx, int tiles_n) {
    __shared__ __attribute__((aligned(16))) char smem[H2Geo<H2_NS>::SMEM_B];
    const int M = *m_dev;
    const int tiles_m = (M + GEMM_BM - 1) / GEMM_BM, ntiles = tiles_m * tiles_n;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        int tm, tn;
        tile_coords(tiles_m, tiles_n, tm, tn, tile);
        f32x16 am[2][2], ac[2][2];
        h2p_mainloop<false, H2_NS, KIND>(Apk, Bpk, K, tm, tn, smem, am, ac);      // ends with a barrier
        epilogue_topk<5, 2, true>(am, reinterpret_cast<float *>(smem), M, N, tm * GEMM_BM, tn * GEMM_BN, tn, tiles_n, inv_temp,
                                  tile_max, tile_sum, cand_val, cand_idx);
        __syncthreads();                                                             // the ring is free again
    }
}

int launch_gemm_x1_topk_dev(hipStream_t st, const void *Apacked, const void *Bpacked, const int *m_dev, int N, int K,
                            float inv_temp, const TopkOut &o, int fmt) {
    CAPDEC_CHECK(m_dev && N > 0 && K > 0 && K % 64 == 0, "gemm_x1_topk_dev: bad argument");
    CAPDEC_CHECK(fmt == PK_F16X1 || fmt == PK_BF16X1, "gemm_x1_topk_dev: one-plane operand formats only");
    const int tiles_n = (N + GEMM_BN - 1) / GEMM_BN;
    if (fmt == PK_F16X1)
        hipLaunchKernelGGL((gemm_x1_topk_dev_kernel<1>), dim3(512), dim3(256), 0, st, (const _Float16 *)Apacked,
                           (const _Float16 *)Bpacked, m_dev, N, K, inv_temp, o.tile_max, o.tile_sum, o.cand_val, o.cand_idx, tiles_n);
    else
        hipLaunchKernelGGL((gemm_x1_topk_dev_kernel<2>), dim3(512), dim3(256), 0, st, (const _Float16 *)Apacked,
                           (const _Float16 *)Bpacked, m_dev, N, K, inv_temp, o.tile_max, o.tile_sum, o.cand_val, o.cand_idx, tiles_n);
    CAPDEC_HIP(hipGetLastError());
    return 0;
}

// ---- launchers of the 128 x 128 kernels: what runs (kernel, slices, blocks) is the plan's decision (gemm_plan.h).
// fmt = PK_F16X2, or a one-plane format (both operands; a packed output is written in the same format)
int launch_gemm_f16x2p(hipStream_t st, const void *Apacked, const void *Bpacked, float *C, int ldc, int M, int N, int K,
                       const GemmEpilogue &epi, int fmt, const GemmPlan &plan) {
    CAPDEC_CHECK(fmt == PK_F16X2 || fmt == PK_F16X1 || fmt == PK_BF16X1, "gemm_f16x2p: two fp16 planes or a one-plane format");
    const std::string who = fmt == PK_F16X2 ? "gemm_f16x2p" : "gemm_x1";
    PackedArgs a;
    CAPDEC_TRY(packed_args(who, epi, plan, C, ldc, M, N, K, &a));
    CAPDEC_CHECK(plan.bm == GEMM_BM && plan.bn == GEMM_BN && plan.threads == 256, who + ": not a plan for the 128 x 128 kernels");
    const int tiles_m = (M + GEMM_BM - 1) / GEMM_BM, tiles_n = (N + GEMM_BN - 1) / GEMM_BN;
    const _Float16 *Ap = (const _Float16 *)Apacked, *Bp = (const _Float16 *)Bpacked;
    const dim3 grid(plan.grid), block(plan.threads);
    if (plan.S > 1) {
        with_kind(fmt, [&](auto KD) {
            hipLaunchKernelGGL(gemm_f16x2p_splitk_kernel<decltype(KD)::value>, grid, block, 0, st, Ap, Bp, a.part, M, N, K,
                               tiles_m, tiles_n, plan.S);
        });
        CAPDEC_HIP(hipGetLastError());
        return launch_splitk_reduce(st, a.part, plan.S, M, N, epi, C, ldc, fmt);
    }
    with_kind(fmt, [&](auto KD) {
        constexpr int kind = decltype(KD)::value;
        auto go = [&](auto V4) {
            constexpr bool v4 = decltype(V4)::value;
            if constexpr (kind == 0)
                hipLaunchKernelGGL((gemm_f16x2p_kernel<v4, H2_NS>), grid, block, 0, st, Ap, Bp, C, ldc, M, N, K, epi.bias, a.resid,
                                   epi.ldr, epi.act, tiles_m, tiles_n, (char *)epi.packed_out, a.sc);
            else      // (a packed output is written in the operands' format)
                hipLaunchKernelGGL((gemm_x1_kernel<v4, kind, (v4 ? 3 : H2_NS)>), grid, block, 0, st, Ap, Bp, C, ldc, M, N, K,
                                   epi.bias, a.resid, epi.ldr, epi.act, tiles_m, tiles_n, (char *)epi.packed_out, fmt, a.sc);
        };
        if (plan.vec4) go(std::true_type());
        else go(std::false_type());
    });
    CAPDEC_HIP(hipGetLastError());
    return 0;
}

int launch_gemm_f16x2p_topk(hipStream_t st, const void *Apacked, const void *Bpacked, int M, int N, int K, int k,
                            float inv_temp, const TopkOut &o, int fmt) {
    CAPDEC_CHECK(fmt == PK_F16X2 || fmt == PK_F16X1 || fmt == PK_BF16X1, "gemm_f16x2p_topk: two fp16 planes or a one-plane format");
    CAPDEC_CHECK(M > 0 && N > 0 && K > 0 && K % 64 == 0, "gemm_f16x2p_topk: K must be a multiple of 64");
    const int tiles_m = (M + GEMM_BM - 1) / GEMM_BM, tiles_n = (N + GEMM_BN - 1) / GEMM_BN;
    dim3 grid(tiles_m * tiles_n), block(256);
    CAPDEC_TRY(with_topk_k(k, "gemm_topk", [&](auto KS) {
        with_kind(fmt, [&](auto KD) {
            hipLaunchKernelGGL((gemm_f16x2p_topk_kernel<decltype(KS)::value, decltype(KD)::value>), grid, block, 0, st,
                               (const _Float16 *)Apacked, (const _Float16 *)Bpacked, M, N, K, inv_temp, o.tile_max, o.tile_sum,
                               o.cand_val, o.cand_idx, tiles_m, tiles_n);
        });
    }));
    CAPDEC_HIP(hipGetLastError());
    return 0;
}

// ---- implicit-GEMM 3x3 convolution (stride 1, padding 1) on the same main loop (CONV above).  act_pk = the input
// activation [M = N H W pixels][Cin] as a packed operand (format fmt); Bpacked = the folded weights [Cout][9 Cin] in
// (ky, kx, c) order; output as for the GEMMs (fp32 C with bias / activation / residual, or packed_out)
template <int KIND>
__global__ __launch_bounds__(256, 2) void conv3x3_packed_kernel(const _Float16 *__restrict__ Apk,
                                                                const _Float16 *__restrict__ Bpk, float *C, int ldc, int M,
                                                                int N, int K, const float *__restrict__ bias,
                                                                const float *resid, int ldr, int act, int tiles_m,
                                                                int tiles_n, char *packed_out, int fmt, ConvGeo cg) {
    __shared__ __attribute__((aligned(16))) char smem[H2_NS * H2_STAGE_B];
    int tm, tn;
    tile_coords(tiles_m, tiles_n, tm, tn);
    f32x16 am[2][2], ac[2][2];
    h2p_mainloop<true, H2_NS, KIND, true>(Apk, Bpk, K, tm, tn, smem, am, ac, 0, -1, cg);
    if constexpr (KIND == 0) h2_join(am, ac);
    const EpiArgs ea = h2_epi_args(C, ldc, M, N, tm * GEMM_BM, tn * GEMM_BN, bias, packed_out ? nullptr : resid, ldr, act, packed_out,
                                   fmt, nullptr);
    epilogue_lds<H2Tile>(am, smem, ea);
}

int launch_conv3x3_packed(hipStream_t st, const void *act_pk, const void *Bpacked, float *C, int ldc, int Nimg, int H,
                          int W, int Cin, int Cout, const GemmEpilogue &epi, int fmt, const void *zeros,
                          size_t zero_bytes) {
    CAPDEC_CHECK(fmt == PK_F16X2 || fmt == PK_F16X1 || fmt == PK_BF16X1, "conv3x3: operand format f16x2, f16 or bf16");
    CAPDEC_CHECK(Nimg > 0 && H > 0 && W > 0 && Cin % 64 == 0 && Cout % 4 == 0, "conv3x3: Cin % 64 == 0, Cout % 4 == 0");
    CAPDEC_CHECK((size_t)Nimg * H * W < ((size_t)1 << 31) - 256, "conv3x3: too many pixels for one launch");
    const int M = Nimg * H * W, N = Cout, K = 9 * Cin;
    ConvGeo cg;
    cg.H = H; cg.W = W; cg.M = M;
    cg.ncs = Cin / (fmt == PK_F16X2 ? 16 : 32);
    cg.zero = (const char *)zeros;
    CAPDEC_CHECK(zeros && zero_bytes >= (size_t)(cg.ncs + 1) * H2_BLOCK_B, "conv3x3: zero block too small");
    CAPDEC_CHECK(epi.packed_out == nullptr || (N % 64 == 0 && epi.resid == nullptr && ((uintptr_t)epi.bias & 15) == 0),
                 "conv3x3: packed output needs Cout % 64 == 0, a 16-byte aligned bias and no residual");
    CAPDEC_CHECK(epi.packed_out != nullptr || gemm_vec4(epi, C, ldc, N), "conv3x3: 16-byte aligned output rows, bias and residual");
    const int tiles_m = (M + GEMM_BM - 1) / GEMM_BM, tiles_n = (N + GEMM_BN - 1) / GEMM_BN;
    with_kind(fmt, [&](auto KD) {
        hipLaunchKernelGGL(conv3x3_packed_kernel<decltype(KD)::value>, dim3(tiles_m * tiles_n), dim3(256), 0, st,
                           (const _Float16 *)act_pk, (const _Float16 *)Bpacked, C, ldc, M, N, K, epi.bias, epi.resid, epi.ldr,
                           epi.act, tiles_m, tiles_n, (char *)epi.packed_out, fmt, cg);
    });
    CAPDEC_HIP(hipGetLastError());
    return 0;
}

// generic packer (any PackFmt): fp32 [N, K] (row stride ldw) -> tile-major planes, rows past N zero.  One thread per
// (padded row, quad of 4 k); used for the one-plane formats (the split formats have their own 16-byte-store packers)
__global__ void pack_planes_fmt_kernel(const float *__restrict__ w, int ldw, char *__restrict__ out, int N, int K,
                                       int rows_pad, int fmt) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int nq = K >> 2;
    if (i >= (size_t)rows_pad * nq) return;
    const int row = (int)(i / nq), qd = (int)(i - (size_t)row * nq);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row < N) v = *reinterpret_cast<const float4 *>(w + (size_t)row * ldw + qd * 4);
    x3_store_quad(out, K >> 4, row, qd >> 2, qd & 3, v, fmt);
}

int launch_pack_planes_fmt(hipStream_t st, const float *w, int ldw, int N, int K, void *out, int fmt) {
    CAPDEC_CHECK(K % 64 == 0 && ldw % 4 == 0, "pack_planes: K must be a multiple of 64");
    const int rows_pad = (N + 127) / 128 * 128;
    const size_t tot = (size_t)rows_pad * (K >> 2);
    hipLaunchKernelGGL(pack_planes_fmt_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, w, ldw, (char *)out,
                       N, K, rows_pad, fmt);
    CAPDEC_HIP(hipGetLastError());
    return 0;
}

CAPDEC_SAT_ACCESSOR(sat_count_gemm_f16x2)

}  // namespace capdec
