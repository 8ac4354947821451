// Neighbour votes (ItemKNN / content-KNN recommendations): per user the K items the neighbour lists of the user's history vote for.
// The lists are nbr_idx int32 / nbr_val fp32 [n x Kn] as cooccur_topk or cosine_topk write them (-1 / -inf fillers), the histories a
// CSR (int64 pointers, int32 ids), an optional second CSR names ids to leave out. Integer arithmetic up to the score.
//
// A vote is a pair (history position p of user u, slot s) with j = hist[p] in [0, n), i = nbr_idx[j, s] in [0, n) and nbr_val[j, s]
// finite; anything else is skipped and never dereferenced. A repeated history id votes again, a repeated id within a list votes again.
// The vote adds q = rint(double(val) * 2^24) (round half even; the product is exact) to an int64 sum S(u, i) and 1 to an int32 count
// c(u, i). An item is listed when c >= 1 and it is not left out -- left out are the ids of the history segment itself
// (exclude_history) and those of the second CSR's segment. score = float(double(S) * 2^-24); order (score descending, id ascending);
// fillers -1 / -inf / 0. Integer adds commute: a user's outputs depend bit for bit on the history as a multiset, the lists, the
// exclusions and K -- not on the arrival order, the form, B, the user's place in `users` or the grid. No floating-point atomics.
//
// One workgroup of 256 threads per user. V(u) = (history length) x Kn + (entries left out) picks the form:
//   LDS form   (V <= VOTE_SLOTS / 2): an open-addressing table of VOTE_SLOTS = 2048 (key, int64 sum, int32 count) entries in LDS,
//              32 KiB, home slot id % VOTE_SLOTS, linear probing; V bounds the entries, so the load factor is at most 0.5 whatever
//              the ids are. Insertion is an integer compare-and-swap on the key, a 64-bit integer add on the sum and an integer add
//              on the count. The left-out ids are entered first; their mark is a bit of the count (VOTE_MARK) no number of votes
//              reaches. The selection list (VOTE_CAP = 1024 keys and counts, 12 KiB) lies beside the table: 44 KiB a workgroup.
//   dense form (any V): at most VOTE_GROUPS workgroups loop over the rows that need it; each owns a row of n int64 sums and n int32
//              counts in the workspace, ZERO when the call starts. Pass 0 marks the left-out ids; pass 1 adds with integer atomics;
//              pass 2 walks the votes again and claims each touched entry through its COUNT (a sum may legitimately be 0) with an
//              exchange to 0, then takes the sum the same way; pass 3 claims the left-out ids no vote met. The row is clean again.
// The 16 lanes of a quarter wave share one history position and stride its list, so 16 positions are in flight per workgroup.
// The two forms' skeleton -- the table's insert, the dense form's row scheduler and its list with the cut rule, the outputs -- and the
// selection are co_select.h's, shared with cooccur.hip and walk.hip; the dense form compares the full key against the K-th kept key
// and, when the list could overflow, sorts it and cuts it to the K best. The traversal (history x list slots), the marks of the
// left-out ids and the (sum, count) pair are this file's own.
#include <cmath>
#include "common.h"
#include "co_select.h"

namespace elimrec {

constexpr int VOTE_SLOTS = 2048, VOTE_MAX_K = 256, VOTE_CAP = VOTE_SLOTS / 2, VOTE_GROUPS = 512, VOTE_FRAC_BITS = 24;
constexpr int VOTE_STEP = 2;                                 // votes a lane claims between two capacity checks of the dense form
constexpr int VOTE_MARK = 1 << 30;                           // the count's bit of a left-out id; a row has fewer votes than that
static_assert(VOTE_SLOTS * 16 + VOTE_CAP * 12 + 64 <= 64 * 1024, "the LDS form's table and list stay within 64 KiB");

struct VoteArgs {
    const int32_t *nbr_idx; const float *nbr_val; int64_t n; int Kn;
    const int64_t *hist_ptr; const int32_t *hist_items; int64_t n_hist;
    const int64_t *excl_ptr; const int32_t *excl_items; int64_t n_excl;       // excl_ptr may be null
    const int64_t *users; int64_t B;
    // the four integers lie together and arrive in one scalar load; with K apart in a CoOut, vote_lds_kernel measured 3 to 7 % slower
    int K, exclude_history, use_lds, groups;
    int32_t *idx; float *val; int32_t *cnt;                  // [B x K]; val and cnt may be null
    unsigned long long *sum; int32_t *ctr;                   // [groups][n] each: the dense form's rows
};

__device__ __forceinline__ CoOut vote_out(const VoteArgs &a) { return {a.K, a.idx, a.val, a.cnt}; }

__host__ __device__ inline bool vote_in_lds(int64_t V) { return V >= 0 && V <= VOTE_CAP; }

// one user's segments: the history [h0, h1), the second CSR's [x0, x1) (empty without one or for a user outside it), V
struct VoteRow { int64_t h0, h1, x0, x1, V; bool known; };
__device__ __forceinline__ VoteRow vote_row(const VoteArgs &a, int64_t b) {
    VoteRow r = {0, 0, 0, 0, 0, false};
    const int64_t u = a.users[b];
    if (u < 0 || u >= a.n_hist) return r;
    r.known = true;
    r.h0 = a.hist_ptr[u]; r.h1 = a.hist_ptr[u + 1];
    if (a.excl_ptr && u < a.n_excl) { r.x0 = a.excl_ptr[u]; r.x1 = a.excl_ptr[u + 1]; }
    r.V = (r.h1 - r.h0) * (int64_t)a.Kn + (a.exclude_history ? r.h1 - r.h0 : 0) + (r.x1 - r.x0);
    return r;
}

__device__ __forceinline__ long long vote_fixed(float v) { return (long long)rint((double)v * (double)(1 << VOTE_FRAC_BITS)); }
__device__ __forceinline__ float vote_score(long long S) { return (float)((double)S * (1.0 / (double)(1 << VOTE_FRAC_BITS))); }

// the e-th left-out id of a row: the history segment first (with exclude_history), then the second CSR's segment
__device__ __forceinline__ int64_t vote_left_out_count(const VoteArgs &a, const VoteRow &r) {
    return (a.exclude_history ? r.h1 - r.h0 : 0) + (r.x1 - r.x0);
}
__device__ __forceinline__ int vote_left_out(const VoteArgs &a, const VoteRow &r, int64_t e) {
    const int64_t nh = a.exclude_history ? r.h1 - r.h0 : 0;
    return e < nh ? a.hist_items[r.h0 + e] : a.excl_items[r.x0 + (e - nh)];
}

__global__ __launch_bounds__(CO_THREADS) void vote_lds_kernel(VoteArgs a) {
    __shared__ unsigned long long s_hs[VOTE_SLOTS];          // the table: sums, keys, counts
    __shared__ int s_hk[VOTE_SLOTS];
    __shared__ int s_hc[VOTE_SLOTS];
    __shared__ uint64_t s_key[VOTE_CAP];                     // the list
    __shared__ int s_c[VOTE_CAP];
    __shared__ int s_n;
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const CoOut out = vote_out(a);
    const VoteRow r = vote_row(a, b);
    if (!(a.use_lds && vote_in_lds(r.V))) {                  // (uniform) the dense form's row; without a row there it gets fillers
        if (a.groups == 0) co_fillers(out, b, 0, tid);
        return;
    }
    if (!r.known || r.h1 == r.h0) { co_fillers(out, b, 0, tid); return; }
    for (int s = tid; s < VOTE_SLOTS; s += CO_THREADS) { s_hk[s] = -1; s_hs[s] = 0; s_hc[s] = 0; }
    if (tid == 0) s_n = 0;
    __syncthreads();
    const int64_t n_out = vote_left_out_count(a, r);
    for (int64_t e = tid; e < n_out; e += CO_THREADS) {
        const int j = vote_left_out(a, r, e);
        if (j < 0 || j >= a.n) continue;
        atomicOr(&s_hc[co_slot<VOTE_SLOTS>(s_hk, j)], VOTE_MARK);
    }
    __syncthreads();
    const int g = tid >> 4, l = tid & 15;
    for (int64_t p = r.h0 + g; p < r.h1; p += 16) {
        const int64_t j = a.hist_items[p];
        if (j < 0 || j >= a.n) continue;
        const int32_t *li = a.nbr_idx + j * a.Kn;
        const float *lv = a.nbr_val + j * a.Kn;
        for (int s = l; s < a.Kn; s += 16) {
            const int i = li[s];
            const float v = lv[s];
            if (i < 0 || i >= a.n || !isfinite(v)) continue;
            const int at = co_slot<VOTE_SLOTS>(s_hk, i);
            atomicAdd(&s_hs[at], (unsigned long long)vote_fixed(v));
            atomicAdd(&s_hc[at], 1);
        }
    }
    __syncthreads();
    for (int s = tid; s < VOTE_SLOTS; s += CO_THREADS) {
        const int c = s_hc[s];
        if (s_hk[s] >= 0 && c > 0 && !(c & VOTE_MARK)) {
            const int pos = atomicAdd(&s_n, 1);              // at most V <= CAP entries
            s_key[pos] = co_key(vote_score((long long)s_hs[s]), s_hk[s]);
            s_c[pos] = c;
        }
    }
    __syncthreads();
    const int n = s_n;
    co_sort(s_key, s_c, n, tid);
    co_emit(out, b, s_key, s_c, n, tid);
}

// claim entry i of the row: its count (and with it the sum) is this lane's when c != 0, and both are zero afterwards
__device__ __forceinline__ int vote_claim(int32_t *ctr, unsigned long long *sum, int i, long long *S) {
    const int c = atomicExch(&ctr[i], 0);
    if (c != 0) *S = (long long)atomicExch(&sum[i], 0ull);
    return c;
}

__global__ __launch_bounds__(CO_THREADS) void vote_dense_kernel(VoteArgs a) {
    const int tid = threadIdx.x, g = tid >> 4, l = tid & 15;
    const CoOut out = vote_out(a);
    int32_t *ctr = a.ctr + (int64_t)blockIdx.x * a.n;
    unsigned long long *sum = a.sum + (int64_t)blockIdx.x * a.n;
    co_dense_rows<VOTE_CAP, VOTE_STEP, VOTE_MAX_K>(
        a.B, [&](int64_t b) { return !(a.use_lds && vote_in_lds(vote_row(a, b).V)); },
        [&](int64_t b, const CoList<VOTE_CAP, VOTE_STEP, VOTE_MAX_K> &list) {
            const VoteRow r = vote_row(a, b);
            if (!r.known || r.h1 == r.h0) { co_fillers(out, b, 0, tid); return; }
            list.reset(tid);
            // pass 0: mark the left-out ids
            const int64_t n_out = vote_left_out_count(a, r);
            for (int64_t e = tid; e < n_out; e += CO_THREADS) {
                const int j = vote_left_out(a, r, e);
                if (j >= 0 && j < a.n) atomicOr(&ctr[j], VOTE_MARK);
            }
            // pass 1: vote
            for (int64_t p = r.h0 + g; p < r.h1; p += 16) {
                const int64_t j = a.hist_items[p];
                if (j < 0 || j >= a.n) continue;
                const int32_t *li = a.nbr_idx + j * a.Kn;
                const float *lv = a.nbr_val + j * a.Kn;
                for (int s = l; s < a.Kn; s += 16) {
                    const int i = li[s];
                    const float v = lv[s];
                    if (i < 0 || i >= a.n || !isfinite(v)) continue;
                    atomicAdd(&sum[i], (unsigned long long)vote_fixed(v));
                    atomicAdd(&ctr[i], 1);
                }
            }
            __threadfence();
            __syncthreads();
            // pass 2: claim, 16 history positions at a time, VOTE_STEP slots a lane between two capacity checks
            for (int64_t p0 = r.h0; p0 < r.h1; p0 += 16) {
                const int64_t p = p0 + g;
                const int32_t *li = nullptr;
                int s1 = 0;
                if (p < r.h1) {
                    const int64_t j = a.hist_items[p];
                    if (j >= 0 && j < a.n) { li = a.nbr_idx + j * a.Kn; s1 = a.Kn; }
                }
                int s0 = 0;
                for (;;) {
                    const uint64_t thr = list.threshold();
#pragma unroll
                    for (int q = 0; q < VOTE_STEP; ++q) {
                        const int s = s0 + l + 16 * q;
                        if (s >= s1) continue;
                        const int i = li[s];
                        if (i < 0 || i >= a.n) continue;
                        long long S = 0;
                        const int c = vote_claim(ctr, sum, i, &S);
                        if (c <= 0 || (c & VOTE_MARK)) continue;       // another lane claimed it, no finite vote met it, or left out
                        list.offer(co_key(vote_score(S), i), c, thr);
                    }
                    s0 += 16 * VOTE_STEP;
                    const int more = __syncthreads_or(s0 < s1);
                    list.cut(out.K, tid);
                    if (!more) break;
                }
            }
            // pass 3: the left-out ids no vote met
            for (int64_t e = tid; e < n_out; e += CO_THREADS) {
                const int j = vote_left_out(a, r, e);
                long long S;
                if (j >= 0 && j < a.n) vote_claim(ctr, sum, j, &S);
            }
            __threadfence();
            list.finish(out, b, tid);
        });
}

static inline size_t vote_workspace(int64_t n_dense_rows, int64_t n) {
    return co_workspace(n_dense_rows, VOTE_GROUPS, n, sizeof(int64_t) + sizeof(int32_t));
}

}  // namespace elimrec

using namespace elimrec;

extern "C" int elimrec_vote_slots(void) { return VOTE_SLOTS; }
extern "C" int elimrec_vote_groups(void) { return VOTE_GROUPS; }
extern "C" int elimrec_vote_max_k(void) { return VOTE_MAX_K; }
extern "C" int elimrec_vote_frac_bits(void) { return VOTE_FRAC_BITS; }
extern "C" int elimrec_vote_rows_in_lds(int64_t V) { return V < 0 ? -1 : (vote_in_lds(V) ? 1 : 0); }
extern "C" size_t elimrec_vote_workspace(int64_t n_dense_rows, int64_t n) {
    if (n_dense_rows < 0 || n < 0 || n >= (int64_t)INT32_MAX) return 0;
    return vote_workspace(n_dense_rows, n);
}

extern "C" int elimrec_neighbour_vote_topk(const int32_t *d_nbr_idx, const float *d_nbr_val, int64_t n, int Kn, const int64_t *d_hist_ptr,
                                           const int32_t *d_hist_items, int64_t n_hist_rows, const int64_t *d_excl_ptr,
                                           const int32_t *d_excl_items, int64_t n_excl_rows, const int64_t *d_users, int64_t B, int K,
                                           int exclude_history, int use_lds, int64_t n_dense_rows, int32_t *d_idx, float *d_val,
                                           int32_t *d_cnt, void *d_workspace, size_t workspace_bytes, void *stream) {
    const char *who = "neighbour_vote_topk";
    if (int rc = co_check_forms(who, K, VOTE_MAX_K, use_lds)) return rc;
    ELIMREC_REQUIRE(n >= 0 && n < (int64_t)INT32_MAX && Kn >= 1, "%s: 0 <= n < 2^31 - 1 and Kn >= 1, got %lld and %d", who, (long long)n, Kn);
    ELIMREC_REQUIRE(n_hist_rows >= 0 && n_excl_rows >= 0, "%s: the CSRs need 0 or more rows, got %lld and %lld", who, (long long)n_hist_rows,
                    (long long)n_excl_rows);
    ELIMREC_REQUIRE(exclude_history == 0 || exclude_history == 1, "%s: exclude_history is 0 or 1, got %d", who, exclude_history);
    ELIMREC_REQUIRE(B >= 0 && B < (int64_t)INT32_MAX, "%s: 0 <= B < 2^31 - 1, got %lld", who, (long long)B);
    if (int rc = co_check_dense_rows(who, n_dense_rows, B, "B")) return rc;
    ELIMREC_REQUIRE(use_lds || n_dense_rows >= 1 || B == 0, "%s: without the LDS form every row is a dense row (n_dense_rows >= 1)", who);
    ELIMREC_REQUIRE((d_excl_ptr == nullptr) == (d_excl_items == nullptr), "%s: the second CSR comes whole or not at all", who);
    if (B == 0) return 0;
    ELIMREC_REQUIRE(d_hist_ptr && d_hist_items && d_users && d_idx && (n == 0 || (d_nbr_idx && d_nbr_val)), "%s: null pointer", who);
    if (int rc = co_check_workspace(who, n_dense_rows, n, vote_workspace(n_dense_rows, n), d_workspace, workspace_bytes)) return rc;
    VoteArgs a = {};
    a.nbr_idx = d_nbr_idx; a.nbr_val = d_nbr_val; a.n = n; a.Kn = Kn;
    a.hist_ptr = d_hist_ptr; a.hist_items = d_hist_items; a.n_hist = n_hist_rows;
    a.excl_ptr = d_excl_ptr; a.excl_items = d_excl_items; a.n_excl = n_excl_rows;
    a.users = d_users; a.B = B;
    a.exclude_history = exclude_history; a.use_lds = use_lds; a.groups = (int)co_groups(n_dense_rows, VOTE_GROUPS);
    a.K = K; a.idx = d_idx; a.val = d_val; a.cnt = d_cnt;
    a.sum = static_cast<unsigned long long *>(d_workspace);                   // the sums first (8-byte entries), the counts behind them
    a.ctr = reinterpret_cast<int32_t *>(a.sum + (size_t)a.groups * (size_t)n);
    return co_launch_forms(vote_lds_kernel, "neighbour_vote_topk (LDS form)", vote_dense_kernel, "neighbour_vote_topk (dense form)", B, use_lds,
                           a.groups, a, (hipStream_t)stream);
}
