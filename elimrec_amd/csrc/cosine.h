// What the readers of the cached embedding tables share (knn.hip, lists.hip, rerank.hip, hardneg.hip, history.hip): the table
// contract and its host checks, the reciprocal norm, the row load, the wave's LDS fence, and the 16-lane group dot.
// (eval.hip's reciprocal norm goes through rcp_nr: another expression, other bits -- it stays there.)
//
// The table: [n_rows x blocks * d] float32 with unit column stride, block b = columns [b * d, (b + 1) * d), d % 4 == 0 and
// 4 <= d <= TABLE_MAXD, 1 <= blocks <= TABLE_MAXBLOCKS; its squared norms [n_rows x blocks]; a 16-byte aligned table with
// ld % 4 == 0 takes the vector load (table_vec).
//
// The group dot (ELIMREC_GROUP16_DOT; hardneg.hip and history.hip score with it): a GROUP of 16 lanes holds one row of a block in
// registers, lane g the float4s q = g, g + 16, ... (NQ = ceil(d / 64) of them, zeros beyond d / 4: ELIMREC_GROUP16_LOAD). Against a second
// row every lane runs four fmaf chains over its float4s in ascending q, one per component, folds them as (a0 + a1) + (a2 + a3), and
// a 16-lane xor butterfly (8, 4, 2, 1) adds the lanes' sums: the order is fixed by d alone, and all 16 lanes end with the same bits.
// The callers scale it as (dot * inv_a) * inv_b and add w_b * cos per block with w_b != 0, in block order.
#pragma once
#include <hip/hip_runtime.h>
#include "common.h"

namespace elimrec {

constexpr int TABLE_MAXD = 256, TABLE_MAXBLOCKS = 8;

struct TableView { const float *T; int64_t ld, n_rows; const float *sq; int64_t ld_sq; };
struct BlockWeights { float w[TABLE_MAXBLOCKS]; int blocks; };

// ---- host: the checks every entry point makes on its table, in its own order (the first failing check sets the message)
inline int table_dims(const char *who, int d, int blocks) {
    ELIMREC_REQUIRE(d >= 4 && d <= TABLE_MAXD && d % 4 == 0, "%s: d %% 4 == 0 and 4 <= d <= %d, got %d", who, TABLE_MAXD, d);
    ELIMREC_REQUIRE(blocks >= 1 && blocks <= TABLE_MAXBLOCKS, "%s: 1 <= blocks <= %d, got %d", who, TABLE_MAXBLOCKS, blocks);
    return 0;
}
// a row's float4s are single 16-byte loads
inline int table_vec(const float *d_T, int64_t ld) { return (reinterpret_cast<uintptr_t>(d_T) % 16 == 0 && ld % 4 == 0) ? 1 : 0; }
// after the entry point's early return: a table with rows has both pointers
inline int table_view(const char *who, const float *d_T, int64_t ld, int64_t n_rows, const float *d_sq, int64_t ld_sq, TableView *out,
                      int *vec) {
    ELIMREC_REQUIRE(n_rows == 0 || (d_T && d_sq), "%s: null pointer", who);
    *out = TableView{d_T, ld, n_rows, d_sq, ld_sq};
    *vec = table_vec(d_T, ld);
    return 0;
}
inline int load_weights(const char *who, const float *h_weights, int blocks, BlockWeights *out) {      // blocks: checked by table_dims
    ELIMREC_REQUIRE(h_weights, "%s: null weights", who);
    for (int b = 0; b < blocks; ++b) out->w[b] = h_weights[b];
    out->blocks = blocks;
    return 0;
}

// ---- device
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

constexpr int GROUP16 = 16;                                  // lanes of a group

// x[NQ] <- lane g's float4s of the d = 4 nq floats at row_expr, a block of a table row. (This and the dot below are macros for
// ELIMREC_LOAD_ROW4's reason: with either as a __forceinline__ function both kernels came out with other register assignments.)
#define ELIMREC_GROUP16_LOAD(x, NQ, row_expr, g, nq, vec)                \
    do {                                                                 \
        const float *row16 = (row_expr);                                 \
        _Pragma("unroll") for (int s = 0; s < NQ; ++s) {                 \
            const int q = (g) + s * GROUP16;                             \
            x[s] = make_float4(0.f, 0.f, 0.f, 0.f);                      \
            if (q < (nq)) ELIMREC_LOAD_ROW4(x[s], row16 + 4 * q, vec);   \
        }                                                                \
    } while (0)

// dot <- the dot product of the group's row x[NQ] with a second row; load_y: a statement that fills `float4 y` with that row's
// float4 `q` (from global memory through ELIMREC_LOAD_ROW4, or from LDS). The same bits on all 16 lanes.
#define ELIMREC_GROUP16_DOT(dot, x, NQ, g, nq, load_y)                                   \
    do {                                                                                 \
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;                                    \
        _Pragma("unroll") for (int s = 0; s < NQ; ++s) {                                 \
            const int q = (g) + s * GROUP16;                                             \
            if (q < (nq)) {                                                              \
                float4 y;                                                                \
                load_y;                                                                  \
                a0 = fmaf(x[s].x, y.x, a0); a1 = fmaf(x[s].y, y.y, a1);                  \
                a2 = fmaf(x[s].z, y.z, a2); a3 = fmaf(x[s].w, y.w, a3);                  \
            }                                                                            \
        }                                                                                \
        dot = (a0 + a1) + (a2 + a3);                                                     \
        _Pragma("unroll") for (int m = GROUP16 / 2; m >= 1; m >>= 1) dot += __shfl_xor(dot, m, GROUP16); \
    } while (0)

}  // namespace elimrec
