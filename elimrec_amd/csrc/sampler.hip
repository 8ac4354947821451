// On-device pairwise (BPR) sampler: the epoch-level contract of PairwiseSamplerV2
// (data/sampler.py:93-126,297-351; util/cython/random_choice.pyx:20-62) with a counter-based
// generator instead of libc rand().
#include "common.h"
#include "philox.h"

namespace elimrec {

// One id uniform over [0, I) outside the sorted training items [beg, end): rejection over the draw rounds 1 .. 255 of the stream
// whose counter word 3 is c3_low (low 24 bits) | round << 24, two 64-bit draws per round (output words 0, 1 and then 2, 3, high
// word first, each % I); ph.c[0 .. 2] and the key are the caller's. tests/sampler_model.py is the executable form of the streams.
__device__ inline int64_t draw_outside(Philox &ph, uint32_t c3_low, const int32_t *__restrict__ items, int64_t beg, int64_t end,
                                       int64_t I) {
    uint32_t r[4];
    int64_t cand = -1;
    for (uint32_t round = 1; round < 256 && cand < 0; ++round) {
        ph.c[3] = c3_low | (round << 24);
        ph.generate(r);
#pragma unroll
        for (int t = 0; t < 2 && cand < 0; ++t) {
            const uint64_t x = ((uint64_t)r[2 * t] << 32) | r[2 * t + 1];
            const int32_t a = (int32_t)(x % (uint64_t)I);
            int64_t lo = beg, hi = end;
            bool found = false;
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                const int32_t v = items[mid];
                if (v == a) { found = true; break; }
                if (v < a) lo = mid + 1; else hi = mid;
            }
            if (!found) cand = a;
        }
    }
    if (cand < 0) {   // a user who interacted with almost every item: the first id missing from the sorted list
        const int64_t cnt = end - beg;
        int64_t k = 0;
        while (k < cnt && items[beg + k] == (int32_t)k) ++k;
        cand = k;      // < I: the host rejects users with >= I training items
    }
    return cand;
}

// The user and the positive of triplet i: the stream's round 0 (counter word 3 = the epoch's bits 32 .. 55, top byte 0): the user's
// slot is the 64-bit draw of output words 0, 1 % n_train_users, the positive's place in the slice that of words 2, 3 % its length.
// -> the user's slice [beg, end) of items; ph is left keyed by seed with c[0 .. 2] = (i, epoch's low word).
__device__ inline void draw_user_pos(Philox &ph, int64_t i, uint64_t seed, uint64_t epoch, const int32_t *__restrict__ user_ids,
                                     const int64_t *__restrict__ ptr, const int32_t *__restrict__ items, int64_t n_train_users,
                                     int64_t &user, int64_t &pos, int64_t &beg, int64_t &end) {
    ph.k[0] = (uint32_t)seed; ph.k[1] = (uint32_t)(seed >> 32);
    ph.c[0] = (uint32_t)i; ph.c[1] = (uint32_t)((uint64_t)i >> 32);
    ph.c[2] = (uint32_t)epoch; ph.c[3] = (uint32_t)(epoch >> 32) & 0x00FFFFFFu;   // top byte = draw round
    uint32_t r[4];
    ph.generate(r);
    const uint64_t ru = ((uint64_t)r[0] << 32) | r[1];
    const uint64_t rp = ((uint64_t)r[2] << 32) | r[3];
    const int64_t ui = (int64_t)(ru % (uint64_t)n_train_users);
    beg = ptr[ui]; end = ptr[ui + 1];
    user = user_ids[ui];
    pos = items[beg + (int64_t)(rp % (uint64_t)(end - beg))];
}

__global__ void sample_triplets_kernel(const int32_t *__restrict__ user_ids, const int64_t *__restrict__ ptr,
                                       const int32_t *__restrict__ items, int64_t n_train_users, int64_t I, int64_t n,
                                       uint64_t seed, uint64_t epoch, int64_t *__restrict__ users,
                                       int64_t *__restrict__ pos, int64_t *__restrict__ neg) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Philox ph;
    int64_t beg, end;
    draw_user_pos(ph, i, seed, epoch, user_ids, ptr, items, n_train_users, users[i], pos[i], beg, end);
    // negatives: uniform over [0, I), rejected while in the user's (sorted) training items
    neg[i] = draw_outside(ph, (uint32_t)(epoch >> 32) & 0x00FFFFFFu, items, beg, end, I);
}

// M candidate negatives per triplet (hard-negative sampling, csrc/hardneg.hip picks among them): one thread per (triplet i,
// column j). Users, positives and column 0 are the words of sample_triplets_kernel for the same (seed, epoch, i). Column j > 0 is
// an independent draw of the same kind from a stream of its own: the LOW 24 BITS OF COUNTER WORD 3 CARRY j (1 .. 63), the top
// byte the draw round, words 0 .. 2 stay (i, the epoch's low word) and the key the seed. sample_triplets_kernel has the epoch's
// bits 32 .. 55 in those 24 bits -- zero for every epoch < 2^32 -- so no (i, epoch < 2^32, round) of it reaches a counter of a
// column j > 0, round 0 (the user / positive draw) included; two columns differ in word 3, two epochs in word 2.
__global__ void sample_triplet_candidates_kernel(const int32_t *__restrict__ user_ids, const int64_t *__restrict__ ptr,
                                                 const int32_t *__restrict__ items, int64_t n_train_users, int64_t I, int64_t n,
                                                 uint64_t seed, uint64_t epoch, int M, int64_t *__restrict__ users,
                                                 int64_t *__restrict__ pos, int32_t *__restrict__ cands) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n * M) return;
    const int64_t i = idx / M;
    const int j = (int)(idx - i * M);
    Philox ph;
    int64_t user, p, beg, end;
    draw_user_pos(ph, i, seed, epoch, user_ids, ptr, items, n_train_users, user, p, beg, end);
    if (j == 0) { users[i] = user; pos[i] = p; }
    cands[idx] = (int32_t)draw_outside(ph, j == 0 ? (uint32_t)(epoch >> 32) & 0x00FFFFFFu : (uint32_t)j, items, beg, end, I);
}


// Distinct negatives per user for sampled-negative evaluation (data/dataset.py:270-288; random_choice.pyx:20-62 with
// replace=False): n_neg distinct ids uniform over [0, I) minus the user's sorted exclusion list. One wave per user draws
// RANKS in [0, M), M = I - |exclusion|, 64 at a time (Philox: the key is the seed's two words, the counter (u lo, u hi, draw
// round, lane); the rank is the 64-bit draw of output words 0 and 1, % M), keeps those not
// drawn before -- the accepted ranks in LDS, duplicates within a round resolved in lane order -- and maps rank r to the
// r-th id not excluded (binary search over e_j - j, non-decreasing for a sorted unique list). Each kept rank is uniform
// over the ranks not yet kept: the draws are a uniform random n_neg-subset, in draw order.
// The closing fallback (NEG_ROUNDS rounds without n_neg distinct ranks) is UNREACHABLE for n_neg <= NEG_MAX and is kept as a
// guard against an endless loop only. Dropping duplicates in lane order makes the rounds one sequence of T = 64 * 2^16 = 4.19e6
// draws, and the fallback needs more than M - n_neg ranks undrawn after them. The slowest case the host admits is n_neg = 16000 of
// M = 16001 (on average M (H_M - 1) = 1.48e5 draws, 2.3e3 rounds): two given ranks are both undrawn with probability
// (1 - 2 / M)^T = e^-524, over M^2 / 2 = 1.3e8 pairs P < 1e-219; a smaller n_neg or a larger M lowers it further.
constexpr int NEG_MAX = 16000;
constexpr uint32_t NEG_ROUNDS = 1u << 16;

__global__ __launch_bounds__(64) void sample_negatives_kernel(const int64_t *__restrict__ ptr, const int32_t *__restrict__ excl,
                                                              int64_t I, int n_neg, uint64_t seed, int32_t *__restrict__ out) {
    extern __shared__ int32_t drawn[];                 // [n_neg] accepted ranks
    __shared__ int32_t round_c[64];
    const int64_t u = blockIdx.x;
    const int lane = threadIdx.x;
    const int64_t beg = ptr[u], ne = ptr[u + 1] - beg;
    const int64_t M = I - ne;
    int32_t *o = out + u * (int64_t)n_neg;
    if (M <= n_neg) {                                  // (the host rejects this: "There is not enough integers to be sampled.")
        for (int k = lane; k < n_neg; k += 64) o[k] = -1;
        return;
    }
    Philox ph;
    ph.k[0] = (uint32_t)seed; ph.k[1] = (uint32_t)(seed >> 32);
    ph.c[0] = (uint32_t)u; ph.c[1] = (uint32_t)((uint64_t)u >> 32);
    int n_acc = 0;
    for (uint32_t rnd = 0; rnd < NEG_ROUNDS && n_acc < n_neg; ++rnd) {
        ph.c[2] = rnd; ph.c[3] = (uint32_t)lane;
        uint32_t r[4];
        ph.generate(r);
        const int32_t c = (int32_t)((((uint64_t)r[0] << 32) | r[1]) % (uint64_t)M);
        round_c[lane] = c;
        __syncthreads();
        bool bad = false;
        for (int k = 0; k < n_acc; ++k) bad |= drawn[k] == c;          // (wave-uniform address: broadcast reads)
        for (int j = 0; j < lane; ++j) bad |= round_c[j] == c;
        const uint64_t ok = __ballot(!bad);
        const int pos = n_acc + __popcll(ok & ((1ull << lane) - 1ull));
        if (!bad && pos < n_neg) drawn[pos] = c;
        n_acc = min(n_neg, n_acc + __popcll(ok));
        __syncthreads();
    }
    if (n_acc < n_neg) {        // 2^16 rounds without completing: the smallest ranks left (unreachable for n_neg <= NEG_MAX, see above)
        if (lane == 0)
            for (int32_t c = 0; n_acc < n_neg; ++c) {
                bool in = false;
                for (int k = 0; k < n_acc; ++k) in |= drawn[k] == c;
                if (!in) drawn[n_acc++] = c;
            }
        __syncthreads();
    }
    for (int k = lane; k < n_neg; k += 64) {
        const int64_t rk = drawn[k];
        int64_t lo = 0, hi = ne;                       // lo = #{j : excl[j] - j <= rk}
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if ((int64_t)excl[beg + mid] - mid <= rk) lo = mid + 1; else hi = mid;
        }
        o[k] = (int32_t)(rk + lo);
    }
}

}  // namespace elimrec

using namespace elimrec;

extern "C" int elimrec_sample_triplets(const int32_t *d_user_ids, const int64_t *d_ptr, const int32_t *d_items,
                                       int64_t n_train_users, int64_t I, int64_t n, uint64_t seed, uint64_t epoch,
                                       int64_t *d_users, int64_t *d_pos, int64_t *d_neg, void *stream) {
    ELIMREC_REQUIRE(d_user_ids && d_ptr && d_items && d_users && d_pos && d_neg, "sample_triplets: null pointer");
    ELIMREC_REQUIRE(n_train_users > 0 && I > 0, "sample_triplets: 'user_pos_dict' cannot be empty.");
    if (n <= 0) return 0;
    hipLaunchKernelGGL(sample_triplets_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       d_user_ids, d_ptr, d_items, n_train_users, I, n, seed, epoch, d_users, d_pos, d_neg);
    ELIMREC_LAUNCH_CHECK("sample_triplets");
    return 0;
}

extern "C" int elimrec_sample_triplet_candidates(const int32_t *d_user_ids, const int64_t *d_ptr, const int32_t *d_items,
                                                 int64_t n_train_users, int64_t I, int64_t n, uint64_t seed, uint64_t epoch,
                                                 int n_cand, int64_t *d_users, int64_t *d_pos, int32_t *d_cands, void *stream) {
    ELIMREC_REQUIRE(d_user_ids && d_ptr && d_items && d_users && d_pos && d_cands, "sample_triplet_candidates: null pointer");
    ELIMREC_REQUIRE(n_train_users > 0 && I > 0, "sample_triplet_candidates: 'user_pos_dict' cannot be empty.");
    ELIMREC_REQUIRE(I < (int64_t)INT32_MAX, "sample_triplet_candidates: the candidates are int32, I < 2^31 - 1");
    ELIMREC_REQUIRE(n_cand >= 1 && n_cand <= 64, "sample_triplet_candidates: 1 <= n_cand <= 64, got %d", n_cand);
    if (n <= 0) return 0;
    ELIMREC_REQUIRE(n < ((int64_t)1 << 31), "sample_triplet_candidates: n < 2^31");
    hipLaunchKernelGGL(sample_triplet_candidates_kernel, dim3((unsigned)((n * n_cand + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, d_user_ids, d_ptr, d_items, n_train_users, I, n, seed, epoch, n_cand, d_users, d_pos,
                       d_cands);
    ELIMREC_LAUNCH_CHECK("sample_triplet_candidates");
    return 0;
}

extern "C" int elimrec_sample_negatives(const int64_t *d_excl_ptr, const int32_t *d_excl_items, int64_t n_users, int64_t I,
                                        int n_neg, uint64_t seed, int32_t *d_out, void *stream) {
    ELIMREC_REQUIRE(d_excl_ptr && d_out, "sample_negatives: null pointer");
    ELIMREC_REQUIRE(I > 0 && I < (int64_t)INT32_MAX, "sample_negatives: 0 < I < 2^31");
    ELIMREC_REQUIRE(n_neg > 0 && n_neg <= NEG_MAX, "sample_negatives: 0 < n_neg <= %d", NEG_MAX);
    if (n_users <= 0) return 0;
    hipLaunchKernelGGL(sample_negatives_kernel, dim3((unsigned)n_users), dim3(64), (size_t)n_neg * sizeof(int32_t), (hipStream_t)stream,
                       d_excl_ptr, d_excl_items, I, n_neg, seed, d_out);
    ELIMREC_LAUNCH_CHECK("sample_negatives");
    return 0;
}
