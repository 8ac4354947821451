// Diversified re-ranking of a top-N pool: greedy maximal marginal relevance (MMR) over one table's rows.
//
// mmr_rerank_kernel: ONE workgroup owns ONE user's pool of N (id, score) positions (W = 1 wave for N <= 64, 4 waves above), and
// thread i owns pool position i for the whole launch. A position is "listed" when its id lies in [0, n_rows) and its score is
// finite; every entry is checked, an unlisted one is never dereferenced and never picked. Over the listed positions
//     rel_i = (s_i - s_min) / (s_max - s_min)         (fp32 IEEE division; 0 when s_max == s_min)
// and the K greedy steps pick, among the listed positions not picked yet, the largest
//     obj_t(i) = lambda * rel_i - (1 - lambda) * pen_t(i),   pen_0 = 0,  pen_t(i) = max over the picks j so far of cos(i, j),
//     cos(i, j) = (dot(i, j) * inv(sq_i)) * inv(sq_j),       inv(x) = 1 / max(sqrt(x), 1e-12)            (cosine.h's inv_norm)
// the lowest pool position winning among equal objectives. It stops after K picks or when no listed position is left; the slots
// left over are filled with -1, -1, -inf. Duplicate ids are positions like any other.
// The checked ids (-1 = not listed) and the reciprocal norms live in LDS, where the other threads read the picked position's;
// rel_i, pen_i and the alive flag are read and written by position i's own thread alone and stay in its registers (with them in
// LDS as well the N = 256 pool would pass 64 KiB). Two forms, chosen by (N, d) alone (mmr_rows_fit):
//   ROWS_IN_LDS: N * (d + 4) floats fit lists.hip's 60 KiB row budget: the pool's rows are gathered once (row stride d + 4 floats:
//     16-byte aligned b128 accesses) and every step reads the picked row (a broadcast) and the candidates' rows from LDS;
//   otherwise only the picked row is staged in LDS per step and every candidate's row is read from global memory again.
// A step's dot product is mmr_dot in both forms: four fmaf chains over the columns c = 0, 1, 2, 3 (mod 4) in ascending order, folded
// as (a0 + a1) + (a2 + a3) -- fixed by d alone. The argmax is a wave butterfly on (objective, -position), then the wave winners are
// compared in wave order through LDS (two parities, so one barrier per step orders them). No atomics, no global workspace: a user's
// outputs depend bit for bit on that user's pool, N, K, d and lambda only -- not on B, the place in the batch or the grid.
// LDS at N = 256, d = 56: 60 KiB of rows + 1 KiB ids + 1 KiB reciprocal norms + 64 B of wave winners = 62.1 KiB, two workgroups
// per CU; N = 256, d = 256 (rows in global memory): 3.1 KiB.
#include <cmath>
#include "common.h"
#include "cosine.h"

namespace elimrec {

constexpr int MMR_MAXN = 256, MMR_SMALLN = 64;
constexpr int MMR_ROW_FLOATS = 15 * 1024;                    // LDS floats for the staged rows (60 KiB, as lists.hip)
constexpr int MMR_NONE = 0x7fffffff;                         // position of "no candidate"

static inline bool mmr_rows_fit(int N, int d) { return N * (d + 4) <= MMR_ROW_FLOATS; }
static inline size_t mmr_lds_bytes(int N, int d) {
    return (size_t)(mmr_rows_fit(N, d) ? N : 1) * (d + 4) * 4 + (size_t)N * 8 + 64;
}

struct MmrArgs {
    const float *T; int64_t ld, n_rows; int d;
    const float *sq; int64_t ld_sq;
    const int32_t *pool_idx; const float *pool_val; int N, K;
    float lambda;
    int32_t *out_idx, *out_pos; float *out_val;
    int vec;                           // T is 16-byte aligned and ld % 4 == 0 -> a row's float4s are single loads
};

// dot of a candidate's row with the picked row in LDS; the order of the sum is fixed by d alone
template <bool VEC>
__device__ __forceinline__ float mmr_dot(const float *x, const float *p, int d) {
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    for (int c = 0; c < d; c += 4) {
        float4 u;
        ELIMREC_LOAD_ROW4(u, x + c, VEC);
        const float4 v = *reinterpret_cast<const float4 *>(p + c);
        a0 = fmaf(u.x, v.x, a0); a1 = fmaf(u.y, v.y, a1); a2 = fmaf(u.z, v.z, a2); a3 = fmaf(u.w, v.w, a3);
    }
    return (a0 + a1) + (a2 + a3);
}

// (objective, position): b beats a when it is larger, or equal at a lower position
__device__ __forceinline__ void mmr_better(float &o, int &p, float ob, int pb) {
    if (ob > o || (ob == o && pb < p)) { o = ob; p = pb; }
}

template <int W, bool ROWS_IN_LDS>
__global__ __launch_bounds__(64 * W) void mmr_rerank_kernel(MmrArgs a) {
    constexpr int NT = 64 * W;
    const int N = a.N, K = a.K, d = a.d, LD = d + 4;
    extern __shared__ __attribute__((aligned(16))) float mmr_smem[];
    float *s_rows = mmr_smem;                                // [N][LD] the pool's rows, or [LD] the picked row
    float *s_inv = s_rows + (ROWS_IN_LDS ? N : 1) * LD;      // [N]    reciprocal norms, 0 = not listed
    int *s_ids = (int *)(s_inv + N);                         // [N]    checked ids, -1 = not listed
    float *s_wobj = (float *)(s_ids + N);                    // [2][W] wave winners of the even / odd steps
    int *s_wpos = (int *)(s_wobj + 8);                       // [2][W]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t b = blockIdx.x;
    const float ninf = -__builtin_inff();

    // this thread's position: checked id, score, reciprocal norm
    int id = -1;
    float s = 0.f;
    if (tid < N) {
        id = a.pool_idx[b * N + tid];
        s = a.pool_val[b * N + tid];
        if (id < 0 || (int64_t)id >= a.n_rows || !(fabsf(s) < __builtin_inff())) id = -1;
        s_ids[tid] = id;
        s_inv[tid] = id >= 0 ? inv_norm(a.sq[(int64_t)id * a.ld_sq]) : 0.f;
    }
    const float *grow = a.T + (int64_t)(id >= 0 ? id : 0) * a.ld;      // (read only while this position is alive)

    // s_min, s_max over the listed positions (min / max: exact in any order)
    float lo = id >= 0 ? s : __builtin_inff(), hi = id >= 0 ? s : ninf;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, off, 64));
        hi = fmaxf(hi, __shfl_xor(hi, off, 64));
    }
    if (lane == 0) { s_wobj[wave] = lo; s_wobj[W + wave] = hi; }
    __syncthreads();                                         // s_ids, s_inv and the wave extrema are written
    for (int w = 0; w < W; ++w) { lo = fminf(lo, s_wobj[w]); hi = fmaxf(hi, s_wobj[W + w]); }
    const float rel = (id >= 0 && hi > lo) ? (s - lo) / (hi - lo) : 0.f;
    if (ROWS_IN_LDS) {
        const int c4n = d >> 2;
        for (int e = tid; e < N * c4n; e += NT) {
            const int r = e / c4n, c = (e - r * c4n) << 2;
            const int rid = s_ids[r];
            float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
            if (rid >= 0) ELIMREC_LOAD_ROW4(x, a.T + (int64_t)rid * a.ld + c, a.vec);
            *reinterpret_cast<float4 *>(s_rows + r * LD + c) = x;
        }
    }
    __syncthreads();                                         // the rows are staged; the wave extrema are read

    const float inv = tid < N ? s_inv[tid] : 0.f;
    bool alive = id >= 0;
    float pen = ninf;                                        // max cosine to the picks so far
    int picked = -1, t = 0;
    for (; t < K; ++t) {
        if (picked >= 0 && alive) {
            const float *prow = ROWS_IN_LDS ? s_rows + picked * LD : s_rows;
            float dot;
            if (ROWS_IN_LDS) dot = mmr_dot<true>(s_rows + tid * LD, prow, d);
            else dot = a.vec ? mmr_dot<true>(grow, prow, d) : mmr_dot<false>(grow, prow, d);
            pen = fmaxf(pen, (dot * inv) * s_inv[picked]);
        }
        const float obj = a.lambda * rel - (1.f - a.lambda) * (t == 0 ? 0.f : pen);
        float bo = alive ? obj : ninf;
        int bp = alive ? tid : MMR_NONE;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float oo = __shfl_xor(bo, off, 64);
            const int op = __shfl_xor(bp, off, 64);
            mmr_better(bo, bp, oo, op);
        }
        float *wo = s_wobj + (t & 1) * W;
        int *wp = s_wpos + (t & 1) * W;
        if (lane == 0) { wo[wave] = bo; wp[wave] = bp; }
        __syncthreads();                                     // wave winners of step t; every thread is done with the picked row
        bo = wo[0]; bp = wp[0];
        for (int w = 1; w < W; ++w) mmr_better(bo, bp, wo[w], wp[w]);
        if (bp == MMR_NONE) break;                           // (uniform) no listed position is left
        picked = bp;
        if (tid == picked) {
            alive = false;
            a.out_idx[b * K + t] = id;
            if (a.out_pos) a.out_pos[b * K + t] = picked;
            if (a.out_val) a.out_val[b * K + t] = bo;
        }
        if (!ROWS_IN_LDS && t + 1 < K) {
            const float *pg = a.T + (int64_t)s_ids[picked] * a.ld;
            for (int c = tid << 2; c < d; c += NT << 2) {
                float4 x;
                ELIMREC_LOAD_ROW4(x, pg + c, a.vec);
                *reinterpret_cast<float4 *>(s_rows + c) = x;
            }
            __syncthreads();                                 // the picked row is staged
        }
    }
    for (int k = t + tid; k < K; k += NT) {                  // fewer listed positions than K
        a.out_idx[b * K + k] = -1;
        if (a.out_pos) a.out_pos[b * K + k] = -1;
        if (a.out_val) a.out_val[b * K + k] = ninf;
    }
}

template <int W>
static int mmr_launch(const MmrArgs &a, int64_t B, hipStream_t s) {
    const size_t lds = mmr_lds_bytes(a.N, a.d);
    if (mmr_rows_fit(a.N, a.d)) hipLaunchKernelGGL((mmr_rerank_kernel<W, true>), dim3((unsigned)B), dim3(64 * W), lds, s, a);
    else hipLaunchKernelGGL((mmr_rerank_kernel<W, false>), dim3((unsigned)B), dim3(64 * W), lds, s, a);
    ELIMREC_LAUNCH_CHECK("mmr_rerank");
    return 0;
}

}  // namespace elimrec

using namespace elimrec;

extern "C" int elimrec_mmr_max_pool(void) { return MMR_MAXN; }
extern "C" int elimrec_mmr_rows_in_lds(int N, int d) {
    if (N < 1 || N > MMR_MAXN || d < 4 || d > TABLE_MAXD || d % 4 != 0) return -1;
    return mmr_rows_fit(N, d) ? 1 : 0;
}

extern "C" int elimrec_mmr_rerank(const float *d_T, int64_t ld, int64_t n_rows, int d, const float *d_sqnorm, int64_t ld_sq,
                                  const int32_t *d_pool_idx, const float *d_pool_val, int64_t B, int N, int K, float lambda,
                                  int32_t *d_out_idx, int32_t *d_out_pos, float *d_out_val, void *stream) {
    ELIMREC_REQUIRE(N >= 1 && N <= MMR_MAXN && K >= 1 && K <= N, "mmr_rerank: 1 <= K <= N <= %d, got K %d, N %d", MMR_MAXN, K, N);
    if (int rc = table_dims("mmr_rerank", d, 1)) return rc;
    ELIMREC_REQUIRE(lambda >= 0.f && lambda <= 1.f, "mmr_rerank: 0 <= lambda <= 1, got %g", (double)lambda);
    ELIMREC_REQUIRE(B >= 0 && B < (int64_t)INT32_MAX && n_rows >= 0 && n_rows < (int64_t)INT32_MAX,
                    "mmr_rerank: need 0 <= B < 2^31 - 1 and 0 <= n_rows < 2^31 - 1");
    ELIMREC_REQUIRE(ld >= (int64_t)d && ld_sq >= 1, "mmr_rerank: ld < d or ld_sq < 1");
    if (B == 0) return 0;
    ELIMREC_REQUIRE(d_pool_idx && d_pool_val && d_out_idx, "mmr_rerank: null pointer");
    ELIMREC_REQUIRE(n_rows == 0 || (d_T && d_sqnorm), "mmr_rerank: null pointer");
    MmrArgs a;
    a.T = d_T; a.ld = ld; a.n_rows = n_rows; a.d = d;
    a.sq = d_sqnorm; a.ld_sq = ld_sq;
    a.pool_idx = d_pool_idx; a.pool_val = d_pool_val; a.N = N; a.K = K;
    a.lambda = lambda;
    a.out_idx = d_out_idx; a.out_pos = d_out_pos; a.out_val = d_out_val;
    a.vec = table_vec(d_T, ld);
    hipStream_t s = (hipStream_t)stream;
    return N <= MMR_SMALLN ? mmr_launch<1>(a, B, s) : mmr_launch<4>(a, B, s);
}
