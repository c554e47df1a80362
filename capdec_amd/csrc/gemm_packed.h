// Device-side helpers the packed-operand GEMM units (gemm_f16x2.hip, gemm_h2w.hip, gemm_pp.hip, gemm_bf16x3.hip) share: the
// LDS-DMA address spaces, the s_waitcnt immediate and the end-of-tile slab release of the persistent kernels.
// (Their launchers share packed_args, common.h.)
#pragma once
#include "common.h"

namespace capdec {

typedef __attribute__((address_space(3))) void lds_void;
typedef const __attribute__((address_space(1))) void glb_void;

// s_waitcnt immediate (gfx9 encoding): vmcnt(N) expcnt(none) lgkmcnt(L: 0 = wait for all, 15 = do not wait)
__host__ __device__ constexpr int waitcnt_imm(int vm, int lgkm) {
    return (vm & 15) | (7 << 4) | ((lgkm & 15) << 8) | ((vm >> 4) << 14);
}

// end of a persistent block's tile: the next tile's LDS-DMA pieces land in the epilogue's slabs, so every wavefront must be
// done reading them
__device__ __forceinline__ void slab_release(bool more) {
    if (more) {
        asm volatile("" ::: "memory");
        __builtin_amdgcn_s_waitcnt(waitcnt_imm(63, 0));
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    }
}

}  // namespace capdec
