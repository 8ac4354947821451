// History support: for a (user, target item) pair, which entries of the user's own history sit closest to the target.
//
// history_support_kernel: ONE WORKGROUP owns ONE row b of `lists` (a user) and a TILE of 16 of its K targets; a GROUP of 16 lanes
// owns ONE target (four targets per wave, 16 per workgroup). The score of history entry j against target i is
//     sum over the blocks b with w_b != 0, in block order, of  w_b * cos_b(j, i),
//     cos_b(j, i) = ((T_b[i] . T_b[j]) * inv(sq[i, b])) * inv(sq[j, b]),   inv(x) = 1 / max(sqrt(x), 1e-12)   (cosine.h's inv_norm)
// -- hardneg.hip's expression, the target in the place of its user row, the history entry in the place of its candidate: both
// kernels form the dot product with cosine.h's group dot, whose summation order (fixed by d alone) is stated there.
// The user's segment is walked ONCE per tile, in chunks of C = 64 / 32 / 16 / 16 entries (d <= 64 / 128 / 192 / 256: 16 KiB of rows
// at most): per chunk the ids are checked and staged (an id outside [0, n_items) becomes -1 and is never dereferenced), then per
// active block the workgroup gathers the chunk's rows of that block into LDS -- each row read from global memory once for all 16
// targets -- with their inv norms; every group reloads its target's block into registers (ELIMREC_GROUP16_LOAD: 16 rows per workgroup,
// cache hits after the first chunk) and walks the chunk: the group dot against the LDS row, and the lane that owns the entry
// (entry e of the chunk: lane e % 16, register e / 16) adds w_b * cos to the entry's running score. After the last block the group takes the chunk's entries in segment order: a listed one
// (staged id >= 0 and, with exclude_self, != the target) is counted, its score added to a float64 sum, and inserted into the
// group's running top list when it beats the list's `top`-th value. The list lives in registers, slot g in lane g, descending;
// an entry goes behind every slot with a value >= its own (the earlier position wins a tie), the slots behind it shift by one lane.
// No atomics, no workspace, nothing of size H x K in global memory. A pair's outputs depend bit for bit on the target's row, the
// segment's entries in order, d, blocks, the weights, top and exclude_self -- not on K, the target's column, B or the grid: the
// chunking follows the segment alone and no value crosses from one group to another.
#include <cmath>
#include "common.h"
#include "cosine.h"
#include "dispatch.h"

namespace elimrec {

constexpr int HS_MAXK = 256, HS_MAXTOP = 16;
constexpr int HS_GROUP = GROUP16;                            // lanes per target
constexpr int HS_THREADS = 256;
constexpr int HS_TILE = HS_THREADS / HS_GROUP;               // targets per workgroup
constexpr int HS_ROW_FLOATS = 4096;                          // LDS floats of a chunk's rows (16 KiB)

struct HistoryArgs {
    TableView t;
    BlockWeights w;
    int d;
    const int64_t *users; const int32_t *lists; int64_t B; int K;
    const int64_t *hist_ptr; const int32_t *hist_items; int64_t n_hist_rows;
    int top, exclude_self, tiles;
    int32_t *out_idx; float *out_val; int32_t *out_cnt; float *out_mean;
    int vec;                             // cosine.h's table_vec of the table
};

template <int NQ>
__global__ __launch_bounds__(HS_THREADS) void history_support_kernel(HistoryArgs a) {
    constexpr int C = NQ == 1 ? 64 : NQ == 2 ? 32 : 16;      // entries per chunk: C * d floats <= HS_ROW_FLOATS
    constexpr int NP = C / HS_GROUP;
    __shared__ __align__(16) float s_rows[HS_ROW_FLOATS];
    __shared__ float s_inv[C];
    __shared__ int s_id[C];
    const int tid = threadIdx.x, g = tid & (HS_GROUP - 1), grp = tid / HS_GROUP;
    const int64_t row = (int64_t)blockIdx.x / a.tiles;
    const int k = ((int)(blockIdx.x % a.tiles)) * HS_TILE + grp;
    const TableView &T = a.t;
    const int d = a.d, nq = d >> 2, top = a.top;
    const bool have = k < a.K;                                // (group-uniform)
    const int64_t u = a.users[row];
    const bool user_ok = u >= 0 && u < a.n_hist_rows;         // (workgroup-uniform)
    int tgt = -1;
    if (have && user_ok) {
        const int32_t t = a.lists[row * a.K + k];
        if (t >= 0 && (int64_t)t < T.n_rows) tgt = t;
    }
    float val = -INFINITY, thr = -INFINITY;                   // slot g of the group's top list; the list's top-th value
    int vid = -1, nf = 0, cnt = 0;
    double sum = 0.0;
    if (user_ok) {
        const int64_t beg = a.hist_ptr[u], end = a.hist_ptr[u + 1];
        for (int64_t base = beg; base < end; base += C) {
            const int cn = (int)(end - base < (int64_t)C ? end - base : (int64_t)C);
            __syncthreads();                                  // the previous chunk's ids are read no more
            if (tid < C) {
                int id = -1;
                if (tid < cn) {
                    const int32_t h = a.hist_items[base + tid];
                    if (h >= 0 && (int64_t)h < T.n_rows) id = h;
                }
                s_id[tid] = id;
            }
            __syncthreads();
            float part[NP];
#pragma unroll
            for (int p = 0; p < NP; ++p) part[p] = 0.f;
            for (int b = 0; b < a.w.blocks; ++b) {
                const float w = a.w.w[b];
                if (w == 0.f) continue;                       // a block with zero weight is not read
                for (int x = tid; x < cn * nq; x += HS_THREADS) {
                    const int e = x / nq, q = x - e * nq, id = s_id[e];
                    if (id >= 0) {
                        float4 y;
                        ELIMREC_LOAD_ROW4(y, T.T + (int64_t)id * T.ld + (int64_t)b * d + 4 * q, a.vec);
                        *reinterpret_cast<float4 *>(s_rows + e * d + 4 * q) = y;
                    }
                }
                if (tid < cn) {
                    const int id = s_id[tid];
                    s_inv[tid] = id >= 0 ? inv_norm(T.sq[(int64_t)id * T.ld_sq + b]) : 0.f;
                }
                __syncthreads();
                if (tgt >= 0) {
                    float4 x[NQ];
                    ELIMREC_GROUP16_LOAD(x, NQ, T.T + (int64_t)tgt * T.ld + (int64_t)b * d, g, nq, a.vec);
                    const float it = inv_norm(T.sq[(int64_t)tgt * T.ld_sq + b]);
#pragma unroll
                    for (int p = 0; p < NP; ++p) {
                        const int lim = min(HS_GROUP, cn - p * HS_GROUP);         // (workgroup-uniform)
                        for (int jj = 0; jj < lim; ++jj) {
                            const int e = p * HS_GROUP + jj;
                            if (s_id[e] < 0) continue;                            // (workgroup-uniform) its row was not staged
                            const float *hrow = s_rows + e * d;
                            float dot;
                            ELIMREC_GROUP16_DOT(dot, x, NQ, g, nq, y = *reinterpret_cast<const float4 *>(hrow + 4 * q));
                            const float cosv = (dot * it) * s_inv[e];
                            if (g == jj) part[p] = part[p] + w * cosv;
                        }
                    }
                }
                __syncthreads();                              // the block's rows are read no more
            }
            if (tgt >= 0) {                                   // the chunk's entries in segment order
#pragma unroll
                for (int p = 0; p < NP; ++p) {
                    const int lim = min(HS_GROUP, cn - p * HS_GROUP);
                    for (int jj = 0; jj < lim; ++jj) {
                        const int id = s_id[p * HS_GROUP + jj];
                        if (id < 0 || (a.exclude_self && id == tgt)) continue;    // (group-uniform)
                        const float s = __shfl(part[p], jj, HS_GROUP);
                        ++cnt;
                        sum += (double)s;
                        if (nf >= top && !(s > thr)) continue;
                        const bool keep = g < nf && val >= s;                     // a prefix of the group's lanes
                        const unsigned long long m = __ballot(keep);
                        const int pos = __popc((unsigned)((m >> (tid & 48)) & 0xffffull));
                        const float pv = __shfl_up(val, 1, HS_GROUP);
                        const int pi = __shfl_up(vid, 1, HS_GROUP);
                        if (g == pos) { val = s; vid = id; }
                        else if (g > pos) { val = pv; vid = pi; }
                        nf = min(nf + 1, HS_GROUP);
                        thr = __shfl(val, top - 1, HS_GROUP);
                    }
                }
            }
        }
    }
    if (!have) return;
    const int64_t o = row * a.K + k;
    if (g < top) {
        a.out_idx[o * top + g] = g < nf ? vid : -1;
        a.out_val[o * top + g] = g < nf ? val : -INFINITY;
    }
    if (g == 0) {
        if (a.out_cnt) a.out_cnt[o] = cnt;
        if (a.out_mean) a.out_mean[o] = cnt ? (float)(sum / (double)cnt) : NAN;
    }
}

}  // namespace elimrec

using namespace elimrec;

extern "C" int elimrec_history_max_top(void) { return HS_MAXTOP; }

extern "C" int elimrec_history_support(const float *d_T, int64_t ld, int64_t n_items, int blocks, int d, const float *d_sqnorm,
                                       int64_t ld_sq, const float *h_weights, const int64_t *d_users, const int32_t *d_lists,
                                       int64_t B, int K, const int64_t *d_hist_ptr, const int32_t *d_hist_items, int64_t n_hist_rows,
                                       int top, int exclude_self, int32_t *d_out_idx, float *d_out_val, int32_t *d_out_cnt,
                                       float *d_out_mean, void *stream) {
    const char *who = "history_support";
    ELIMREC_REQUIRE(K >= 1 && K <= HS_MAXK, "history_support: 1 <= K <= %d, got %d", HS_MAXK, K);
    ELIMREC_REQUIRE(top >= 1 && top <= HS_MAXTOP, "history_support: 1 <= top <= %d, got %d", HS_MAXTOP, top);
    if (int rc = table_dims(who, d, blocks)) return rc;
    const int tiles = (K + HS_TILE - 1) / HS_TILE;
    ELIMREC_REQUIRE(B >= 0 && B * tiles < (int64_t)INT32_MAX && n_hist_rows >= 0 && n_items >= 0 && n_items < (int64_t)INT32_MAX,
                    "history_support: need 0 <= B, B * ceil(K / %d) < 2^31 - 1, n_hist_rows >= 0 and 0 <= n_items < 2^31 - 1", HS_TILE);
    ELIMREC_REQUIRE(ld >= (int64_t)blocks * d && ld_sq >= blocks, "history_support: the row stride < blocks * d, or the norm stride < blocks");
    ELIMREC_REQUIRE(exclude_self == 0 || exclude_self == 1, "history_support: exclude_self is 0 or 1, got %d", exclude_self);
    if (B == 0) return 0;
    HistoryArgs a{};
    if (int rc = load_weights(who, h_weights, blocks, &a.w)) return rc;
    ELIMREC_REQUIRE(d_users && d_lists && d_out_idx && d_out_val, "history_support: null pointer");
    ELIMREC_REQUIRE(n_hist_rows == 0 || d_hist_ptr, "history_support: null pointer");
    if (int rc = table_view(who, d_T, ld, n_items, d_sqnorm, ld_sq, &a.t, &a.vec)) return rc;
    a.d = d;
    a.users = d_users; a.lists = d_lists; a.B = B; a.K = K;
    a.hist_ptr = d_hist_ptr; a.hist_items = d_hist_items; a.n_hist_rows = n_hist_rows;
    a.top = top; a.exclude_self = exclude_self; a.tiles = tiles;
    a.out_idx = d_out_idx; a.out_val = d_out_val; a.out_cnt = d_out_cnt; a.out_mean = d_out_mean;
    return with_quads(who, d, [&](auto nq) {
        hipLaunchKernelGGL((history_support_kernel<decltype(nq)::value>), dim3((unsigned)(B * tiles)), dim3(HS_THREADS), 0,
                           (hipStream_t)stream, a);
        ELIMREC_LAUNCH_CHECK("history_support");
        return 0;
    });
}
