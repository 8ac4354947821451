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
// registers (cosine.h's ELIMREC_GROUP16_LOAD) and walks the columns in order: the column's id is broadcast from its owner lane, the group
// gathers the item's block (one 16-byte load per lane and 64 floats) into cosine.h's group dot -- its summation order, fixed by d
// alone, is stated there --, and the owner lane adds w_b * cos to its running score. After the last block each lane keeps the best of its columns and a second butterfly reduces on
// (score, -column). No atomics, no LDS, no workspace: a triplet's outputs depend bit for bit on its two rows, d, blocks and the
// weights only -- not on M, the candidate's column, n, or where the triplet falls in the grid.
#include <cmath>
#include "common.h"
#include "cosine.h"
#include "dispatch.h"

namespace elimrec {

constexpr int HN_MAXM = 64;
constexpr int HN_GROUP = GROUP16;                            // lanes per triplet
constexpr int HN_THREADS = 256;                              // 16 triplets per workgroup
constexpr int HN_NONE = 0x7fffffff;                          // column of "no candidate"

struct HardNegArgs {
    TableView users_t, items_t;
    BlockWeights w;
    int d, M;
    const int64_t *users; const int32_t *cands; int64_t n;
    int64_t *out_neg; int32_t *out_pos; float *out_score;
    int vec_u, vec_i;                  // cosine.h's table_vec of the two tables
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
    const TableView &U = a.users_t, &I = a.items_t;
    const bool user_ok = u >= 0 && u < U.n_rows && I.n_rows > 0;
    int id[4];
    float part[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int j = k * HN_GROUP + g;
        id[k] = -1;
        part[k] = 0.f;
        if (user_ok && j < M) {
            const int32_t c = a.cands[t * M + j];
            if (c >= 0 && (int64_t)c < I.n_rows) id[k] = c;
        }
    }
    if (user_ok) {
        for (int b = 0; b < a.w.blocks; ++b) {
            const float w = a.w.w[b];
            if (w == 0.f) continue;                           // a block with zero weight is not read
            float4 x[NQ];
            ELIMREC_GROUP16_LOAD(x, NQ, U.T + u * U.ld + (int64_t)b * d, g, nq, a.vec_u);
            const float iu = inv_norm(U.sq[u * U.ld_sq + b]);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int lim = min(HN_GROUP, M - k * HN_GROUP);          // (wave-uniform)
                for (int jj = 0; jj < lim; ++jj) {
                    const int c = __shfl(id[k], jj, HN_GROUP);
                    const int64_t cc = c < 0 ? 0 : c;                     // an unlisted column reads row 0 and adds nothing
                    const float *irow = I.T + cc * I.ld + (int64_t)b * d;
                    float dot;
                    ELIMREC_GROUP16_DOT(dot, x, NQ, g, nq, ELIMREC_LOAD_ROW4(y, irow + 4 * q, a.vec_i));
                    const float cosv = (dot * iu) * inv_norm(I.sq[cc * I.ld_sq + b]);
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

extern "C" int elimrec_pick_hard_negatives(const float *d_U, int64_t ld_u, int64_t n_users, const float *d_sq_u, int64_t ldsq_u,
                                           const float *d_T, int64_t ld_i, int64_t n_items, const float *d_sq_i, int64_t ldsq_i,
                                           int blocks, int d, const float *h_weights, const int64_t *d_users, const int32_t *d_cands,
                                           int64_t n, int M, int64_t *d_out_neg, int32_t *d_out_pos, float *d_out_score, void *stream) {
    const char *who = "pick_hard_negatives";
    ELIMREC_REQUIRE(M >= 1 && M <= HN_MAXM, "pick_hard_negatives: 1 <= M <= %d, got %d", HN_MAXM, M);
    if (int rc = table_dims(who, d, blocks)) return rc;
    ELIMREC_REQUIRE(n >= 0 && n < (int64_t)INT32_MAX && n_users >= 0 && n_items >= 0 && n_items < (int64_t)INT32_MAX,
                    "pick_hard_negatives: need 0 <= n < 2^31 - 1, n_users >= 0 and 0 <= n_items < 2^31 - 1");
    ELIMREC_REQUIRE(ld_u >= (int64_t)blocks * d && ld_i >= (int64_t)blocks * d && ldsq_u >= blocks && ldsq_i >= blocks,
                    "pick_hard_negatives: a row stride < blocks * d, or a norm stride < blocks");
    HardNegArgs a{};
    if (int rc = load_weights(who, h_weights, blocks, &a.w)) return rc;
    if (n == 0) return 0;
    ELIMREC_REQUIRE(d_users && d_cands && d_out_neg, "pick_hard_negatives: null pointer");
    if (int rc = table_view(who, d_U, ld_u, n_users, d_sq_u, ldsq_u, &a.users_t, &a.vec_u)) return rc;
    if (int rc = table_view(who, d_T, ld_i, n_items, d_sq_i, ldsq_i, &a.items_t, &a.vec_i)) return rc;
    a.d = d; a.M = M;
    a.users = d_users; a.cands = d_cands; a.n = n;
    a.out_neg = d_out_neg; a.out_pos = d_out_pos; a.out_score = d_out_score;
    constexpr int per = HN_THREADS / HN_GROUP;
    return with_quads(who, d, [&](auto nq) {
        hipLaunchKernelGGL((pick_hard_negatives_kernel<decltype(nq)::value>), dim3((unsigned)((n + per - 1) / per)), dim3(HN_THREADS), 0,
                           (hipStream_t)stream, a);
        ELIMREC_LAUNCH_CHECK("pick_hard_negatives");
        return 0;
    });
}
