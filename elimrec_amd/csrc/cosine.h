// What the cosine kernels over the cached tables share (knn.hip, lists.hip): the reciprocal norm, the row load, the wave's LDS fence.
// (eval.hip's reciprocal norm goes through rcp_nr: another expression, other bits -- it stays there.)
#pragma once
#include <hip/hip_runtime.h>

namespace elimrec {

__device__ __forceinline__ float inv_norm(float sq) { return 1.f / fmaxf(sqrtf(sq), 1e-12f); }

__device__ __forceinline__ void wave_lds_sync() {          // LDS written by other lanes of this wave is read next
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// x <- four consecutive floats of a table row at src; vec: the table is 16-byte aligned and its ld % 4 == 0 -> one 16-byte load.
// (A macro: as a function -- returning the float4 or filling a reference -- the kernels come out with other register assignments
// than the statements written in place, and these kernels' results are pinned to their instruction streams.)
#define ELIMREC_LOAD_ROW4(x, src_expr, vec)                              \
    do {                                                                 \
        const float *src = (src_expr);                                   \
        if (vec) x = *reinterpret_cast<const float4 *>(src);             \
        else x = make_float4(src[0], src[1], src[2], src[3]);            \
    } while (0)

}  // namespace elimrec
