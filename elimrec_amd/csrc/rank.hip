// Exact catalogue rank of given items in a user's full ranking, and the per-pair / per-user rows of the rank report.
//
// rank_count_kernel: scores [B x I] (row stride lds >= I, masked items = -inf, as elimrec_score_topk leaves the caller's block),
// targets as CSR. For target t of row b with s = scores[b, t]:
//     rank = #{ j in [0, I) : scores[b, j] > s  or  (scores[b, j] == s and j < t) }
// the evaluator's (score descending, id ascending) order, 0-based; -1 where s == -inf (a masked item) or t lies outside [0, I).
// One workgroup per (user row, segment of RK_SEG columns): the segment is loaded ONCE, 16 bytes per lane and load, into
// registers (RK_VEC float4 per lane, a wave-instruction = 1 KiB contiguous); the row's targets are staged in LDS, RK_TPP per pass
// (longer lists loop over the same registers); per target every wave counts its registers and reduces, the four waves meet in an
// LDS integer, and one global integer atomic add per (workgroup, target) lands in the zeroed output. Integer sums commute: the
// result does not depend on the grid or on arrival order. Columns >= I of a padded row are never read (the last vector of a row is
// loaded element by element), a row without targets is not read at all. Duplicated targets each get their rank; -0.0 == 0.0 as
// IEEE compares them. NaN scores are outside the contract (every scoring call ends with the range check): a NaN compares false
// both ways and would simply not be counted.
// Bytes: B_listed x I x 4 read once (+ one 4-byte gather per (workgroup, target)), 4 bytes per target written.
#include "common.h"

namespace elimrec {

constexpr int RK_THREADS = 256, RK_VEC = 4, RK_SEG = RK_THREADS * 4 * RK_VEC, RK_TPP = 64;
constexpr int RK_MAXK = 16;

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ __forceinline__ int64_t rk_ptr(const int64_t *__restrict__ ptr, int64_t b, int64_t n) {
    const int64_t p = ptr[b];
    return p < 0 ? 0 : (p > n ? n : p);                         // (a pointer outside the list reads nothing)
}

// VEC: the block's base is 16-byte aligned and lds % 4 == 0, so every full float4 of a row is one 16-byte load
template <bool VEC>
__global__ __launch_bounds__(RK_THREADS) void rank_count_kernel(const float *__restrict__ scores, int64_t I, int64_t lds, int n_seg,
                                                                const int64_t *__restrict__ tptr, const int32_t *__restrict__ titems,
                                                                int64_t n_targets, int32_t *__restrict__ rank) {
    __shared__ int s_id[RK_TPP];
    __shared__ float s_val[RK_TPP];
    __shared__ int s_cnt[RK_TPP];
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t b = blockIdx.x / n_seg;
    const int seg = (int)(blockIdx.x % n_seg);
    const int64_t t_begin = rk_ptr(tptr, b, n_targets), t_end = rk_ptr(tptr, b + 1, n_targets);
    if (t_end <= t_begin) return;                               // (workgroup-uniform: no list, no read)
    const float *__restrict__ row = scores + b * lds;
    const int64_t seg0 = (int64_t)seg * RK_SEG;
    const float NEG = -__builtin_huge_valf();

    // the segment, once: element (v, c) of this lane is column seg0 + (v * RK_THREADS + tid) * 4 + c; what lies beyond I is
    // -inf, which no counted comparison accepts (targets at -inf are not counted at all)
    float x[RK_VEC][4];
#pragma unroll
    for (int v = 0; v < RK_VEC; ++v) {
        const int64_t j = seg0 + (int64_t)(v * RK_THREADS + tid) * 4;
        if (VEC && j + 4 <= I) {
            const float4 q = *reinterpret_cast<const float4 *>(row + j);
            x[v][0] = q.x; x[v][1] = q.y; x[v][2] = q.z; x[v][3] = q.w;
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c) x[v][c] = j + c < I ? row[j + c] : NEG;
        }
    }

    for (int64_t t0 = t_begin; t0 < t_end; t0 += RK_TPP) {
        const int m = (int)(t_end - t0 < RK_TPP ? t_end - t0 : RK_TPP);
        __syncthreads();                                        // (the previous pass has read its LDS)
        if (tid < m) {
            const int t = titems[t0 + tid];
            const bool ok = t >= 0 && t < I;
            const float s = ok ? row[t] : NEG;
            s_id[tid] = s == NEG ? -1 : t;                      // -1: masked or outside the catalogue -> rank -1, nothing counted
            s_val[tid] = s;
            s_cnt[tid] = 0;
        }
        __syncthreads();
        for (int k = 0; k < m; ++k) {
            const int t = s_id[k];
            if (t < 0) continue;                                // (workgroup-uniform)
            const float s = s_val[k];
            const int64_t d = (int64_t)t - seg0;                // columns of this segment below rel lie before the target
            const int rel = d < 0 ? 0 : (d > RK_SEG ? RK_SEG : (int)d);
            int n = 0;
#pragma unroll
            for (int v = 0; v < RK_VEC; ++v) {
                const int jl = (v * RK_THREADS + tid) * 4;
#pragma unroll
                for (int c = 0; c < 4; ++c) n += (x[v][c] > s || (x[v][c] == s && jl + c < rel)) ? 1 : 0;
            }
            n = wave_sum_i(n);
            if (lane == 0 && n) atomicAdd(&s_cnt[k], n);
        }
        __syncthreads();
        if (tid < m) {
            if (s_id[tid] < 0) {
                if (seg == 0) rank[t0 + tid] = -1;              // nobody adds to this slot: one plain store
            } else if (s_cnt[tid]) {
                atomicAdd(&rank[t0 + tid], s_cnt[tid]);
            }
        }
    }
}

// ---- per pair: rank, rr = 1 / (rank + 1), pct = rank / (n_cand - 1) (0 when n_cand <= 1), then hit@K = (rank < K); computed in
// double, rounded once; rank < 0 -> a NaN row
struct RankKs { int k[RK_MAXK]; };

__global__ __launch_bounds__(256) void rank_pair_rows_kernel(const int32_t *__restrict__ rank, const int32_t *__restrict__ n_cand,
                                                             int64_t P, RankKs ks, int n_k, float *__restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const int r = rank[p];
    const int C = 3 + n_k;
    float *__restrict__ o = out + p * C;
    if (r < 0) {
        for (int c = 0; c < C; ++c) o[c] = __builtin_nanf("");
        return;
    }
    const int nc = n_cand[p];
    o[0] = (float)(double)r;
    o[1] = (float)(1.0 / ((double)r + 1.0));
    o[2] = nc <= 1 ? 0.f : (float)((double)r / ((double)nc - 1.0));
    for (int c = 0; c < n_k; ++c) o[3 + c] = r < ks.k[c] ? 1.f : 0.f;
}

// ---- per user (one wave): over its T valid targets (rank >= 0), N_neg = n_cand_u - T:
//   auc = 1 - sum_t (rank_t - #valid targets of the user ranked above t) / (T N_neg)   (the sum is an exact integer)
//   mrr_full = 1 / (min rank + 1),  first_rank = min rank;  NaN when T == 0 or N_neg <= 0
__global__ __launch_bounds__(256) void rank_user_rows_kernel(const int32_t *__restrict__ rank, const int64_t *__restrict__ tptr,
                                                             int64_t n_targets, const int32_t *__restrict__ n_cand, int64_t B,
                                                             float *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;                                         // (wave-uniform)
    const int64_t t_begin = rk_ptr(tptr, b, n_targets), t_end = rk_ptr(tptr, b + 1, n_targets);
    long long sum = 0;
    int T = 0, first = INT32_MAX;
    for (int64_t t = t_begin + lane; t < t_end; t += 64) {
        const int r = rank[t];
        if (r < 0) continue;
        int above = 0;
        for (int64_t q = t_begin; q < t_end; ++q) {
            const int rq = rank[q];
            above += (rq >= 0 && rq < r) ? 1 : 0;
        }
        sum += (long long)(r - above);
        T += 1;
        first = r < first ? r : first;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        sum += __shfl_xor(sum, off, 64);
        T += __shfl_xor(T, off, 64);
        const int o = __shfl_xor(first, off, 64);
        first = o < first ? o : first;
    }
    if (lane) return;
    float *__restrict__ o = out + b * 3;
    const double n_neg = (double)n_cand[b] - (double)T;
    if (T == 0 || n_neg <= 0.0) {
        o[0] = o[1] = o[2] = __builtin_nanf("");
        return;
    }
    o[0] = (float)(1.0 - (double)sum / ((double)T * n_neg));
    o[1] = (float)(1.0 / ((double)first + 1.0));
    o[2] = (float)(double)first;
}

}  // namespace elimrec

using namespace elimrec;

extern "C" int elimrec_rank_segment(void) { return RK_SEG; }
extern "C" int elimrec_rank_targets_per_pass(void) { return RK_TPP; }

extern "C" int elimrec_rank_targets(const float *d_scores, int64_t B, int64_t I, int64_t lds, const int64_t *d_tgt_ptr,
                                    const int32_t *d_tgt_items, int64_t n_targets, int32_t *d_rank, void *stream) {
    ELIMREC_REQUIRE(B >= 0 && n_targets >= 0, "rank_targets: need B >= 0, n_targets >= 0");
    if (B == 0 || n_targets == 0) return 0;
    ELIMREC_REQUIRE(d_scores && d_tgt_ptr && d_tgt_items && d_rank, "rank_targets: null pointer");
    ELIMREC_REQUIRE(I >= 1 && I < (int64_t)INT32_MAX - RK_SEG, "rank_targets: the catalogue must hold 1 .. 2^31 - %d items", RK_SEG + 1);
    ELIMREC_REQUIRE(lds >= I, "rank_targets: lds < I");
    const int64_t n_seg = (I + RK_SEG - 1) / RK_SEG;
    ELIMREC_REQUIRE(B * n_seg < (int64_t)INT32_MAX, "rank_targets: %lld rows x %lld segments exceed one launch", (long long)B,
                    (long long)n_seg);
    hipStream_t s = (hipStream_t)stream;
    int rc = check_hip(hipMemsetAsync(d_rank, 0, (size_t)n_targets * sizeof(int32_t), s), "rank_targets (zero)");
    if (rc) return rc;
    const dim3 grid((unsigned)(B * n_seg));
    if (((uintptr_t)d_scores & 15) == 0 && lds % 4 == 0)
        hipLaunchKernelGGL(rank_count_kernel<true>, grid, dim3(RK_THREADS), 0, s, d_scores, I, lds, (int)n_seg, d_tgt_ptr, d_tgt_items,
                           n_targets, d_rank);
    else
        hipLaunchKernelGGL(rank_count_kernel<false>, grid, dim3(RK_THREADS), 0, s, d_scores, I, lds, (int)n_seg, d_tgt_ptr, d_tgt_items,
                           n_targets, d_rank);
    ELIMREC_LAUNCH_CHECK("rank_targets");
    return 0;
}

extern "C" int elimrec_rank_pair_rows(const int32_t *d_rank, const int32_t *d_n_cand, int64_t P, const int *ks, int n_k, float *d_out,
                                      void *stream) {
    ELIMREC_REQUIRE(P >= 0 && n_k >= 0 && n_k <= RK_MAXK, "rank_pair_rows: need P >= 0 and 0 .. %d values of K", RK_MAXK);
    ELIMREC_REQUIRE(n_k == 0 || ks, "rank_pair_rows: null pointer");
    if (P == 0) return 0;
    ELIMREC_REQUIRE(d_rank && d_n_cand && d_out, "rank_pair_rows: null pointer");
    ELIMREC_REQUIRE((P + 255) / 256 < (int64_t)INT32_MAX, "rank_pair_rows: too many pairs for one launch");
    RankKs k;
    for (int c = 0; c < RK_MAXK; ++c) k.k[c] = c < n_k ? ks[c] : 0;
    hipLaunchKernelGGL(rank_pair_rows_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_rank, d_n_cand, P,
                       k, n_k, d_out);
    ELIMREC_LAUNCH_CHECK("rank_pair_rows");
    return 0;
}

extern "C" int elimrec_rank_user_rows(const int32_t *d_rank, const int64_t *d_tgt_ptr, int64_t n_targets, const int32_t *d_n_cand,
                                      int64_t B, float *d_out, void *stream) {
    ELIMREC_REQUIRE(B >= 0 && n_targets >= 0, "rank_user_rows: need B >= 0, n_targets >= 0");
    if (B == 0) return 0;
    ELIMREC_REQUIRE(d_tgt_ptr && d_n_cand && d_out && (d_rank || n_targets == 0), "rank_user_rows: null pointer");
    ELIMREC_REQUIRE((B + 3) / 4 < (int64_t)INT32_MAX, "rank_user_rows: too many users for one launch");
    hipLaunchKernelGGL(rank_user_rows_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, (hipStream_t)stream, d_rank, d_tgt_ptr,
                       n_targets, d_n_cand, B, d_out);
    ELIMREC_LAUNCH_CHECK("rank_user_rows");
    return 0;
}
