// Calibrated re-ranking of a top-N pool (Steck, "Calibrated recommendations", RecSys 2018): pick K items so that the list's mix of
// item classes follows a target mix -- the user's own -- while giving up as little relevance as possible; and the class shares and
// the miscalibration C_KL of given lists.
//
// calibrate_rerank_kernel: mmr_rerank_kernel's launch shape -- ONE workgroup owns ONE user's pool of N (id, score) positions
// (W = 1 wave for N <= 64, 4 waves above), thread i owns pool position i. A position is "listed" when its id lies in [0, n_items),
// its score is finite and class_of[id] lies in [0, C); every entry is checked, an unlisted one is never dereferenced further and
// never picked. Over the listed positions, all in float64,
//     rel_i = (s_i - s_min) / (s_max - s_min)                                   (0 when s_max == s_min)
//     p_c   = target[b, c]                                                      (an entry that is negative or not finite: 0)
//     q_c   = (n_c(t) + [c == c']) / (t + 1),   q~_c = (1 - smooth) q_c + smooth p_c          (n_c(t): picks so far in class c)
//     KL_t(c') = sum over c ascending with p_c > 0 of p_c * log(p_c / q~_c)     (no positive p_c: 0)
// and step t picks, among the listed positions not picked yet, the largest obj_t(i) = lambda * rel_i - (1 - lambda) * KL_t(class_i),
// the lowest pool position winning among equal objectives, until K picks are made or no listed position is left; the slots left
// over are filled with -1, -1, -inf. lambda weighs the RELEVANCE, as in mmr_rerank (Steck's lambda weighs the calibration term).
// The penalty depends on a candidate only through its class: lane c < C of every wave keeps n_c in a register and forms the two
// terms class c can contribute -- p_c log(p_c / q~_c) with and without the candidate counted -- so a step costs two logs per lane;
// KL_t(c') is their sum in ascending c, handed round by wave shuffles (every wave forms the same C values: no LDS, no barrier), and
// a position takes the value of its class by one more shuffle. The argmax is rerank.hip's: a wave butterfly on (objective,
// -position), then the wave winners in wave order through LDS (two parities: one barrier per step). No atomics, no global
// workspace: a user's outputs depend bit for bit on its pool, the classes of its pool's ids, its target row, N, K, C, lambda and
// smooth only -- not on B, the place in the batch or the grid. LDS: 4 N + 128 bytes.
//
// class_shares_kernel: ONE wave per row (a CSR segment or a padded list), four rows per workgroup. Lane c < C counts class c: per
// 64 entries one ballot per class and a population count -- integers, exact in any order, no atomics of any kind. share_c =
// float(count_c) / float(listed) (one IEEE fp32 division; zeros when nothing is listed). With a target row the list form also
// writes kl = C_KL(p, q~), q_c = count_c / listed in float64 (0 when nothing is listed), by the formula above, rounded once.
#include <cmath>
#include "common.h"

namespace elimrec {

constexpr int CAL_MAXN = 256, CAL_SMALLN = 64, CAL_MAXC = 16;
constexpr int CAL_NONE = 0x7fffffff;                         // position of "no candidate"

struct CalArgs {
    const int32_t *pool_idx; const float *pool_val; int N, K;
    const int32_t *class_of; int64_t n_items;
    const float *target; int64_t ld_t; int C;
    double lambda, smooth;
    int32_t *out_idx, *out_pos; float *out_val;
};

// target entry -> p_c: float64, 0 when negative or not finite
__device__ __forceinline__ double cal_target(float x) { return (x > 0.f && x < __builtin_inff()) ? (double)x : 0.0; }

// p log(p / ((1 - smooth) q + smooth p)) for p > 0
__device__ __forceinline__ double cal_term(double p, double q, double smooth) {
    return p * log(p / ((1.0 - smooth) * q + smooth * p));
}

// (objective, position): b beats a when it is larger, or equal at a lower position
__device__ __forceinline__ void cal_better(double &o, int &p, double ob, int pb) {
    if (ob > o || (ob == o && pb < p)) { o = ob; p = pb; }
}

// sum over c ascending with p_c > 0 (bit c of `pos`) of lane c's term: `with` where c is the receiving lane, `without` elsewhere
__device__ __forceinline__ double cal_kl(double without, double with, unsigned pos, int C, int lane) {
    double sum = 0.0;
    for (int c = 0; c < C; ++c) {
        const double ta = __shfl(without, c, 64), tb = __shfl(with, c, 64);
        if ((pos >> c) & 1u) sum += (c == lane) ? tb : ta;
    }
    return sum;
}

template <int W>
__global__ __launch_bounds__(64 * W) void calibrate_rerank_kernel(CalArgs a) {
    constexpr int NT = 64 * W;
    const int N = a.N, K = a.K, C = a.C;
    __shared__ int s_cls[CAL_MAXN];                          // checked classes, -1 = not listed
    __shared__ double s_wobj[2 * W];                         // wave winners of the even / odd steps (and the wave extrema)
    __shared__ int s_wpos[2 * W];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t b = blockIdx.x;
    const float ninf = -__builtin_inff();

    // this thread's position: checked id, score, class
    int id = -1, cls = -1;
    float s = 0.f;
    if (tid < N) {
        id = a.pool_idx[b * N + tid];
        s = a.pool_val[b * N + tid];
        if (id >= 0 && (int64_t)id < a.n_items && fabsf(s) < __builtin_inff()) {
            cls = a.class_of[id];
            if (cls < 0 || cls >= C) cls = -1;
        }
        if (cls < 0) id = -1;
        s_cls[tid] = cls;
    }
    // s_min, s_max over the listed positions (min / max: exact in any order)
    float lo = id >= 0 ? s : __builtin_inff(), hi = id >= 0 ? s : ninf;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, off, 64));
        hi = fmaxf(hi, __shfl_xor(hi, off, 64));
    }
    if (lane == 0) { s_wobj[wave] = (double)lo; s_wobj[W + wave] = (double)hi; }
    __syncthreads();                                         // s_cls and the wave extrema are written
    double dlo = (double)lo, dhi = (double)hi;
    for (int w = 0; w < W; ++w) { dlo = fmin(dlo, s_wobj[w]); dhi = fmax(dhi, s_wobj[W + w]); }
    const double rel = (id >= 0 && dhi > dlo) ? ((double)s - dlo) / (dhi - dlo) : 0.0;
    const double lrel = a.lambda * rel, wkl = 1.0 - a.lambda;
    __syncthreads();                                         // the wave extrema are read (step 0 writes the same words)

    // lane c < C of every wave: class c's target and count
    const double p = lane < C ? cal_target(a.target[b * a.ld_t + lane]) : 0.0;
    const unsigned pos = (unsigned)(__ballot(p > 0.0) & 0xffffull);
    int n_c = 0;
    bool alive = id >= 0;
    int t = 0;
    for (; t < K; ++t) {
        double without = 0.0, with = 0.0;
        if (p > 0.0) {
            without = cal_term(p, (double)n_c / (double)(t + 1), a.smooth);
            with = cal_term(p, (double)(n_c + 1) / (double)(t + 1), a.smooth);
        }
        const double kl_lane = cal_kl(without, with, pos, C, lane);          // lane c' < C: KL_t(c')
        const double kl = __shfl(kl_lane, cls >= 0 ? cls : 0, 64);
        double bo = alive ? lrel - wkl * kl : (double)ninf;
        int bp = alive ? tid : CAL_NONE;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double oo = __shfl_xor(bo, off, 64);
            const int op = __shfl_xor(bp, off, 64);
            cal_better(bo, bp, oo, op);
        }
        double *wo = s_wobj + (t & 1) * W;
        int *wp = s_wpos + (t & 1) * W;
        if (lane == 0) { wo[wave] = bo; wp[wave] = bp; }
        __syncthreads();                                     // wave winners of step t
        bo = wo[0]; bp = wp[0];
        for (int w = 1; w < W; ++w) cal_better(bo, bp, wo[w], wp[w]);
        if (bp == CAL_NONE) break;                           // (uniform) no listed position is left
        if (lane == s_cls[bp]) ++n_c;
        if (tid == bp) {
            alive = false;
            a.out_idx[b * K + t] = id;
            if (a.out_pos) a.out_pos[b * K + t] = bp;
            if (a.out_val) a.out_val[b * K + t] = (float)bo;
        }
    }
    for (int k = t + tid; k < K; k += NT) {                  // fewer listed positions than K
        a.out_idx[b * K + k] = -1;
        if (a.out_pos) a.out_pos[b * K + k] = -1;
        if (a.out_val) a.out_val[b * K + k] = ninf;
    }
}

struct ShareArgs {
    const int64_t *ptr; const int32_t *items; int64_t nnz;  // CSR form (ptr != nullptr): segment b of items[0 .. nnz)
    int K;                                                   // list form: row b of items [B x K]
    int64_t B;
    const int32_t *class_of; int64_t n_items; int C;
    float *shares;                                           // [B x C]
    const float *target; int64_t ld_t; double smooth; float *kl;      // list form, optional
};

constexpr int SHARE_WAVES = 4;

__global__ __launch_bounds__(64 * SHARE_WAVES) void class_shares_kernel(ShareArgs a) {
    const int lane = threadIdx.x & 63, C = a.C;
    const int64_t b = (int64_t)blockIdx.x * SHARE_WAVES + (threadIdx.x >> 6);
    if (b >= a.B) return;                                    // (a whole wave)
    int64_t lo, hi;
    if (a.ptr) {                                             // a segment never reaches outside items[0 .. nnz), whatever ptr holds
        lo = a.ptr[b]; hi = a.ptr[b + 1];
        lo = lo < 0 ? 0 : lo;
        hi = hi > a.nnz ? a.nnz : hi;
    } else {
        lo = b * a.K; hi = lo + a.K;
    }
    int cnt = 0;                                             // lane c < C: entries of class c
    for (int64_t e0 = lo; e0 < hi; e0 += 64) {
        const int64_t e = e0 + lane;
        int cls = -1;
        if (e < hi) {
            const int id = a.items[e];
            if (id >= 0 && (int64_t)id < a.n_items) cls = a.class_of[id];
        }
        for (int c = 0; c < C; ++c) {
            const unsigned long long m = __ballot(cls == c);
            if (lane == c) cnt += __popcll(m);
        }
    }
    int listed = lane < C ? cnt : 0;
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) listed += __shfl_xor(listed, off, 64);       // (C <= 16: lanes 0 .. 15 hold the sum)
    listed = __shfl(listed, 0, 64);
    if (lane < C) a.shares[b * C + lane] = listed ? (float)cnt / (float)listed : 0.f;
    if (a.kl) {
        const double p = lane < C ? cal_target(a.target[b * a.ld_t + lane]) : 0.0;
        const unsigned pos = (unsigned)(__ballot(p > 0.0) & 0xffffull);
        const double term = p > 0.0 ? cal_term(p, listed ? (double)cnt / (double)listed : 0.0, a.smooth) : 0.0;
        const double kl = cal_kl(term, term, pos, C, lane);
        if (lane == 0) a.kl[b] = (float)kl;
    }
}

static int shares_launch(const ShareArgs &a, const char *who, hipStream_t s) {
    const int64_t blocks = (a.B + SHARE_WAVES - 1) / SHARE_WAVES;
    hipLaunchKernelGGL(class_shares_kernel, dim3((unsigned)blocks), dim3(64 * SHARE_WAVES), 0, s, a);
    ELIMREC_LAUNCH_CHECK(who);
    return 0;
}

}  // namespace elimrec

using namespace elimrec;

extern "C" int elimrec_calibrate_max_classes(void) { return CAL_MAXC; }

extern "C" int elimrec_calibrate_rerank(const int32_t *d_pool_idx, const float *d_pool_val, int64_t B, int N, int K,
                                        const int32_t *d_class_of, int64_t n_items, const float *d_target, int64_t ld_target, int C,
                                        double lambda, double smooth, int32_t *d_out_idx, int32_t *d_out_pos, float *d_out_val,
                                        void *stream) {
    ELIMREC_REQUIRE(N >= 1 && N <= CAL_MAXN && K >= 1 && K <= N, "calibrate_rerank: 1 <= K <= N <= %d, got K %d, N %d", CAL_MAXN, K, N);
    ELIMREC_REQUIRE(C >= 1 && C <= CAL_MAXC, "calibrate_rerank: 1 <= C <= %d, got %d", CAL_MAXC, C);
    ELIMREC_REQUIRE(lambda >= 0.0 && lambda <= 1.0, "calibrate_rerank: 0 <= lambda <= 1, got %g", lambda);
    ELIMREC_REQUIRE(smooth > 0.0 && smooth < 1.0, "calibrate_rerank: 0 < smooth < 1, got %g", smooth);
    ELIMREC_REQUIRE(B >= 0 && B < (int64_t)INT32_MAX && n_items >= 0 && n_items < (int64_t)INT32_MAX,
                    "calibrate_rerank: need 0 <= B < 2^31 - 1 and 0 <= n_items < 2^31 - 1");
    ELIMREC_REQUIRE(ld_target >= (int64_t)C, "calibrate_rerank: ld_target < C");
    if (B == 0) return 0;
    ELIMREC_REQUIRE(d_pool_idx && d_pool_val && d_target && d_out_idx, "calibrate_rerank: null pointer");
    ELIMREC_REQUIRE(n_items == 0 || d_class_of, "calibrate_rerank: null pointer");
    CalArgs a;
    a.pool_idx = d_pool_idx; a.pool_val = d_pool_val; a.N = N; a.K = K;
    a.class_of = d_class_of; a.n_items = n_items;
    a.target = d_target; a.ld_t = ld_target; a.C = C;
    a.lambda = lambda; a.smooth = smooth;
    a.out_idx = d_out_idx; a.out_pos = d_out_pos; a.out_val = d_out_val;
    hipStream_t s = (hipStream_t)stream;
    if (N <= CAL_SMALLN) hipLaunchKernelGGL((calibrate_rerank_kernel<1>), dim3((unsigned)B), dim3(64), 0, s, a);
    else hipLaunchKernelGGL((calibrate_rerank_kernel<4>), dim3((unsigned)B), dim3(256), 0, s, a);
    ELIMREC_LAUNCH_CHECK("calibrate_rerank");
    return 0;
}

extern "C" int elimrec_class_shares_csr(const int64_t *d_ptr, const int32_t *d_items, int64_t nnz, int64_t B, const int32_t *d_class_of,
                                        int64_t n_items, int C, float *d_shares, void *stream) {
    ELIMREC_REQUIRE(C >= 1 && C <= CAL_MAXC, "class_shares: 1 <= C <= %d, got %d", CAL_MAXC, C);
    ELIMREC_REQUIRE(B >= 0 && B < (int64_t)INT32_MAX && nnz >= 0 && n_items >= 0 && n_items < (int64_t)INT32_MAX,
                    "class_shares: need 0 <= B < 2^31 - 1, nnz >= 0 and 0 <= n_items < 2^31 - 1");
    if (B == 0) return 0;
    ELIMREC_REQUIRE(d_ptr && d_shares && (nnz == 0 || d_items), "class_shares: null pointer");
    ELIMREC_REQUIRE(n_items == 0 || d_class_of, "class_shares: null pointer");
    ShareArgs a;
    a.ptr = d_ptr; a.items = d_items; a.nnz = nnz; a.K = 0; a.B = B;
    a.class_of = d_class_of; a.n_items = n_items; a.C = C;
    a.shares = d_shares;
    a.target = nullptr; a.ld_t = 0; a.smooth = 0.0; a.kl = nullptr;
    return shares_launch(a, "class_shares", (hipStream_t)stream);
}

extern "C" int elimrec_list_calibration(const int32_t *d_lists, int64_t B, int K, const int32_t *d_class_of, int64_t n_items, int C,
                                        float *d_shares, const float *d_target, int64_t ld_target, double smooth, float *d_kl,
                                        void *stream) {
    ELIMREC_REQUIRE(K >= 1, "list_calibration: K >= 1, got %d", K);
    ELIMREC_REQUIRE(C >= 1 && C <= CAL_MAXC, "list_calibration: 1 <= C <= %d, got %d", CAL_MAXC, C);
    ELIMREC_REQUIRE(B >= 0 && B < (int64_t)INT32_MAX && n_items >= 0 && n_items < (int64_t)INT32_MAX,
                    "list_calibration: need 0 <= B < 2^31 - 1 and 0 <= n_items < 2^31 - 1");
    ELIMREC_REQUIRE((d_kl == nullptr) == (d_target == nullptr), "list_calibration: target and kl go together");
    ELIMREC_REQUIRE(!d_kl || (smooth > 0.0 && smooth < 1.0), "list_calibration: 0 < smooth < 1, got %g", smooth);
    ELIMREC_REQUIRE(!d_kl || ld_target >= (int64_t)C, "list_calibration: ld_target < C");
    if (B == 0) return 0;
    ELIMREC_REQUIRE(d_lists && d_shares, "list_calibration: null pointer");
    ELIMREC_REQUIRE(n_items == 0 || d_class_of, "list_calibration: null pointer");
    ShareArgs a;
    a.ptr = nullptr; a.items = d_lists; a.nnz = 0; a.K = K; a.B = B;
    a.class_of = d_class_of; a.n_items = n_items; a.C = C;
    a.shares = d_shares;
    a.target = d_target; a.ld_t = ld_target; a.smooth = smooth; a.kl = d_kl;
    return shares_launch(a, "list_calibration", (hipStream_t)stream);
}
