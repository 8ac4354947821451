// Hard-negative pick (dynamic negative sampling): per triplet the best of M candidate items under the current tables.
//
// pick_hard_negatives_kernel: a GROUP of 16 lanes owns ONE triplet (four triplets per wave, 16 per workgroup). The score of
// (user u, item i) is  sum over the blocks b with w_b != 0, in block order, of  w_b * cos_b(u, i),
//     cos_b(u, i) = ((U_b[u] . T_b[i]) * inv(squ[u, b])) * inv(sqi[i, b]),   inv(x) = 1 / max(sqrt(x), 1e-12)   (cosine.h's inv_norm)
// A candidate is "listed" when its id lies in [0, n_items); every entry is checked, an unlisted one is never dereferenced and
// never picked. The listed candidate with the largest score wins, the lowest column among equal scores; a triplet with no listed
// candidate, or with a user id outside [0, n_users), gets -1 / -1 / -inf.
// Mapping: lane g of the group holds the ids and the running scores of the columns j = g, g + 16, g + 32, g + 48 (M <= 64: four
// registers each, read with one coalesced load per 16 columns). Per active block the group loads its user's d floats once into
// registers -- lane g the float4s q = g, g + 16, ... of the block (NQ = ceil(d / 64) of them) -- and walks the columns in order:
// the column's id is broadcast from its owner lane, the group gathers the item's block (one 16-byte load per lane and 64 floats),
// each lane runs four fmaf chains over its float4s in ascending q, folds them as (a0 + a1) + (a2 + a3), and a 16-lane xor butterfly
// (8, 4, 2, 1) adds the lanes' sums: the order is fixed by d alone, and all 16 lanes end with the same bits. The owner lane adds
// w_b * cos to its running score. After the last block each lane keeps the best of its columns and a second butterfly reduces on
// (score, -column). No atomics, no LDS, no workspace: a triplet's outputs depend bit for bit on its two rows, d, blocks and the
// weights only -- not on M, the candidate's column, n, or where the triplet falls in the grid.
#include <cmath>
#include "common.h"
#include "cosine.h"

namespace elimrec {

constexpr int HN_MAXM = 64, HN_MAXD = 256, HN_MAXBLOCKS = 8;
constexpr int HN_GROUP = 16;                                 // lanes per triplet
constexpr int HN_THREADS = 256;                              // 16 triplets per workgroup
constexpr int HN_NONE = 0x7fffffff;                          // column of "no candidate"

struct HardNegArgs {
    const float *U; int64_t ld_u, n_users; const float *sq_u; int64_t ldsq_u;
    const float *T; int64_t ld_i, n_items; const float *sq_i; int64_t ldsq_i;
    float w[HN_MAXBLOCKS];
    int blocks, d, M;
    const int64_t *users; const int32_t *cands; int64_t n;
    int64_t *out_neg; int32_t *out_pos; float *out_score;
    int vec_u, vec_i;                  // the table is 16-byte aligned and its ld % 4 == 0 -> a row's float4s are single loads
};

// (score, column, id): b beats a when it is a candidate and a is none, or it is larger, or equal at a lower column
__device__ __forceinline__ void hn_better(float &s, int &col, int &id, float sb, int colb, int idb) {
    if (colb != HN_NONE && (col == HN_NONE || sb > s || (sb == s && colb < col))) { s = sb; col = colb; id = idb; }
}

template <int NQ>
__global__ __launch_bounds__(HN_THREADS) void pick_hard_negatives_kernel(HardNegArgs a) {
    const int g = threadIdx.x & (HN_GROUP - 1);
    const int64_t t = (int64_t)blockIdx.x * (HN_THREADS / HN_GROUP) + (threadIdx.x / HN_GROUP);
    if (t >= a.n) return;                                     // (whole groups leave: the shuffles below stay inside a group)
    const int M = a.M, d = a.d, nq = d >> 2;
    const int64_t u = a.users[t];
    const bool user_ok = u >= 0 && u < a.n_users && a.n_items > 0;
    int id[4];
    float part[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int j = k * HN_GROUP + g;
        id[k] = -1;
        part[k] = 0.f;
        if (user_ok && j < M) {
            const int32_t c = a.cands[t * M + j];
            if (c >= 0 && (int64_t)c < a.n_items) id[k] = c;
        }
    }
    if (user_ok) {
        for (int b = 0; b < a.blocks; ++b) {
            const float w = a.w[b];
            if (w == 0.f) continue;                           // a block with zero weight is not read
            float4 x[NQ];
            const float *urow = a.U + u * a.ld_u + (int64_t)b * d;
#pragma unroll
            for (int s = 0; s < NQ; ++s) {
                const int q = g + s * HN_GROUP;
                x[s] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (q < nq) ELIMREC_LOAD_ROW4(x[s], urow + 4 * q, a.vec_u);
            }
            const float iu = inv_norm(a.sq_u[u * a.ldsq_u + b]);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int lim = min(HN_GROUP, M - k * HN_GROUP);          // (wave-uniform)
                for (int jj = 0; jj < lim; ++jj) {
                    const int c = __shfl(id[k], jj, HN_GROUP);
                    const int64_t cc = c < 0 ? 0 : c;                     // an unlisted column reads row 0 and adds nothing
                    const float *irow = a.T + cc * a.ld_i + (int64_t)b * d;
                    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
                    for (int s = 0; s < NQ; ++s) {
                        const int q = g + s * HN_GROUP;
                        if (q < nq) {
                            float4 y;
                            ELIMREC_LOAD_ROW4(y, irow + 4 * q, a.vec_i);
                            a0 = fmaf(x[s].x, y.x, a0); a1 = fmaf(x[s].y, y.y, a1);
                            a2 = fmaf(x[s].z, y.z, a2); a3 = fmaf(x[s].w, y.w, a3);
                        }
                    }
                    float dot = (a0 + a1) + (a2 + a3);
#pragma unroll
                    for (int m = HN_GROUP / 2; m >= 1; m >>= 1) dot += __shfl_xor(dot, m, HN_GROUP);
                    const float cosv = (dot * iu) * inv_norm(a.sq_i[cc * a.ldsq_i + b]);
                    if (g == jj && c >= 0) part[k] = part[k] + w * cosv;
                }
            }
        }
    }
    float bs = -INFINITY;
    int bcol = HN_NONE, bid = -1;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (id[k] >= 0) hn_better(bs, bcol, bid, part[k], k * HN_GROUP + g, id[k]);
#pragma unroll
    for (int m = HN_GROUP / 2; m >= 1; m >>= 1) {
        const float so = __shfl_xor(bs, m, HN_GROUP);
        const int co = __shfl_xor(bcol, m, HN_GROUP), io = __shfl_xor(bid, m, HN_GROUP);
        hn_better(bs, bcol, bid, so, co, io);
    }
    if (g == 0) {
        const bool none = bcol == HN_NONE;
        a.out_neg[t] = none ? -1 : (int64_t)bid;
        if (a.out_pos) a.out_pos[t] = none ? -1 : bcol;
        if (a.out_score) a.out_score[t] = none ? -INFINITY : bs;
    }
}

}  // namespace elimrec

using namespace elimrec;

template <int NQ>
static int hn_launch(const HardNegArgs &a, hipStream_t s) {
    constexpr int per = HN_THREADS / HN_GROUP;
    hipLaunchKernelGGL((pick_hard_negatives_kernel<NQ>), dim3((unsigned)((a.n + per - 1) / per)), dim3(HN_THREADS), 0, s, a);
    ELIMREC_LAUNCH_CHECK("pick_hard_negatives");
    return 0;
}

extern "C" int elimrec_pick_hard_negatives(const float *d_U, int64_t ld_u, int64_t n_users, const float *d_sq_u, int64_t ldsq_u,
                                           const float *d_T, int64_t ld_i, int64_t n_items, const float *d_sq_i, int64_t ldsq_i,
                                           int blocks, int d, const float *h_weights, const int64_t *d_users, const int32_t *d_cands,
                                           int64_t n, int M, int64_t *d_out_neg, int32_t *d_out_pos, float *d_out_score, void *stream) {
    ELIMREC_REQUIRE(M >= 1 && M <= HN_MAXM, "pick_hard_negatives: 1 <= M <= %d, got %d", HN_MAXM, M);
    ELIMREC_REQUIRE(d >= 4 && d <= HN_MAXD && d % 4 == 0, "pick_hard_negatives: d %% 4 == 0 and 4 <= d <= %d, got %d", HN_MAXD, d);
    ELIMREC_REQUIRE(blocks >= 1 && blocks <= HN_MAXBLOCKS, "pick_hard_negatives: 1 <= blocks <= %d, got %d", HN_MAXBLOCKS, blocks);
    ELIMREC_REQUIRE(n >= 0 && n < (int64_t)INT32_MAX && n_users >= 0 && n_items >= 0 && n_items < (int64_t)INT32_MAX,
                    "pick_hard_negatives: need 0 <= n < 2^31 - 1, n_users >= 0 and 0 <= n_items < 2^31 - 1");
    ELIMREC_REQUIRE(ld_u >= (int64_t)blocks * d && ld_i >= (int64_t)blocks * d && ldsq_u >= blocks && ldsq_i >= blocks,
                    "pick_hard_negatives: a row stride < blocks * d, or a norm stride < blocks");
    ELIMREC_REQUIRE(h_weights, "pick_hard_negatives: null weights");
    if (n == 0) return 0;
    ELIMREC_REQUIRE(d_users && d_cands && d_out_neg, "pick_hard_negatives: null pointer");
    ELIMREC_REQUIRE(n_users == 0 || (d_U && d_sq_u), "pick_hard_negatives: null pointer");
    ELIMREC_REQUIRE(n_items == 0 || (d_T && d_sq_i), "pick_hard_negatives: null pointer");
    HardNegArgs a{d_U, ld_u, n_users, d_sq_u, ldsq_u, d_T, ld_i, n_items, d_sq_i, ldsq_i, {}, blocks, d, M, d_users, d_cands, n,
                  d_out_neg, d_out_pos, d_out_score,
                  (reinterpret_cast<uintptr_t>(d_U) % 16 == 0 && ld_u % 4 == 0) ? 1 : 0,
                  (reinterpret_cast<uintptr_t>(d_T) % 16 == 0 && ld_i % 4 == 0) ? 1 : 0};
    for (int b = 0; b < blocks; ++b) a.w[b] = h_weights[b];
    hipStream_t s = (hipStream_t)stream;
    switch ((d + 63) / 64) {
        case 1: return hn_launch<1>(a, s);
        case 2: return hn_launch<2>(a, s);
        case 3: return hn_launch<3>(a, s);
        default: return hn_launch<4>(a, s);
    }
}
