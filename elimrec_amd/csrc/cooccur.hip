// Co-interaction neighbours ("users who took this also took ..."): per query row of one side of a bipartite graph the K rows of the
// same side with the largest co-occurrence score -- the top-K of a row of A^T A under a count, cosine or Jaccard measure (ItemKNN's
// neighbour lists). The graph comes as two CSRs: q_ptr / q_nbr maps a row of the query side to its neighbours on the other side
// (item -> its training users), o_ptr / o_nbr maps a row of the other side back (user -> items). Integer arithmetic up to the score.
//
// c(q, j), j != q, is the number of two-step walks q -> u -> j; a repeated edge is an edge of its own, so c is the product count.
// a = deg(q), b = deg(j) are q_ptr differences. score: count float(c); cosine c / sqrt(a b); jaccard c / (a + b - c) -- the last two
// in float64 with IEEE sqrt and division, rounded once to fp32. Only c >= 1 is listed, never q itself; order (score descending, id
// ascending); fillers -1 / -inf / 0.
//
// One workgroup of 256 threads per query row. W(q) = the sum of deg(u) over q's segment (cooccur_walk_kernel, int64) picks the form:
//   LDS form   (W <= COOCCUR_SLOTS / 2): an open-addressing table of COOCCUR_SLOTS = 4096 (key, count) pairs in LDS, 32 KiB, home
//              slot id % COOCCUR_SLOTS, linear probing; W bounds the entries, so the load factor is at most 0.5 whatever the ids are.
//              Insertion is an integer compare-and-swap on the key and an integer add on the count.
//   dense form (any W): a fixed number of workgroups (at most COOCCUR_GROUPS) loop over the rows that need it; each owns an int32
//              counter row of n entries in the workspace, ZERO when the call starts. Pass 1 walks the 2-hop entries and adds with
//              integer atomics; pass 2 walks them again and claims each touched counter with an exchange to 0: the lane that gets
//              c > 0 offers (c, j), and the row is clean again for the next query.
// The 16 lanes of a quarter wave share one u of q's segment and stride its list, so 16 users are in flight per workgroup.
//
// Selection. Candidates do not arrive in ascending id, so knn_select.h's threshold rule does not hold here. A candidate is ONE
// 64-bit key: the order-preserving image of the fp32 score in the high word, ~id in the low word -- a larger key ranks earlier under
// (score descending, id ascending), and keys are distinct because ids are. The keys (with c beside them) are gathered into a list
// of COOCCUR_CAP = 2048 slots in LDS -- the LDS form's table holds at most that many -- and sorted by a bitonic network over the
// next power of two, the empty key 0 behind every candidate (co_select.h, shared with vote.hip). The dense form compares the FULL key against the K-th kept key: a key
// at or below it can never be listed; when the list could overflow it is sorted and cut to the K best, which raises that key. A row's
// outputs therefore depend bit for bit on the graph, the row, K and the measure -- not on the arrival order, the form, Q, the row's
// place in `rows` or the grid. No floating-point atomics.
// A query id outside the side gives fillers; a neighbour id outside its side is skipped and never dereferenced.
#include <cmath>
#include "common.h"
#include "co_select.h"

namespace elimrec {

constexpr int COOCCUR_SLOTS = 4096, COOCCUR_MAX_K = 256, COOCCUR_CAP = COOCCUR_SLOTS / 2, COOCCUR_GROUPS = 512;
constexpr int CO_STEP = 4;                                   // CO_STEP: 2-hop entries a lane claims between two capacity checks
static_assert(COOCCUR_CAP >= 2 * CO_THREADS * CO_STEP && COOCCUR_CAP - CO_THREADS * CO_STEP >= COOCCUR_MAX_K, "the dense form's list");

struct CoArgs {
    const int64_t *q_ptr; const int32_t *q_nbr; int64_t n_query;
    const int64_t *o_ptr; const int32_t *o_nbr; int64_t n_other;
    const int32_t *rows; int64_t Q;
    int K, measure, use_lds, groups;
    int64_t *walk;                                           // [Q] W(q)
    int32_t *idx; float *val; int32_t *cnt;                  // [Q x K]; cnt may be null
    int32_t *ctr;                                            // [groups][n_query] the dense form's counter rows
};

__host__ __device__ inline bool co_in_lds(int64_t W) { return W >= 0 && W <= COOCCUR_SLOTS / 2; }

__device__ __forceinline__ float co_score(int measure, int c, int64_t a, int64_t b) {
    if (measure == 0) return (float)c;
    if (measure == 1) return (float)((double)c / sqrt((double)a * (double)b));
    return (float)((double)c / (double)(a + b - (int64_t)c));
}

__device__ __forceinline__ void co_fillers(const CoArgs &a, int64_t qi, int from, int tid) {
    for (int k = from + tid; k < a.K; k += CO_THREADS) {
        a.idx[qi * a.K + k] = -1;
        if (a.val) a.val[qi * a.K + k] = -__builtin_huge_valf();
        if (a.cnt) a.cnt[qi * a.K + k] = 0;
    }
}

// the sorted list's K best to row qi of the outputs, fillers behind them
__device__ __forceinline__ void co_emit(const CoArgs &a, int64_t qi, const uint64_t *key, const int *c, int n, int tid) {
    const int kept = n < a.K ? n : a.K;
    for (int k = tid; k < kept; k += CO_THREADS) {
        a.idx[qi * a.K + k] = co_key_id(key[k]);
        if (a.val) a.val[qi * a.K + k] = co_key_score(key[k]);
        if (a.cnt) a.cnt[qi * a.K + k] = c[k];
    }
    co_fillers(a, qi, kept, tid);
}

// W(q) of every query: one quarter wave per query
__global__ __launch_bounds__(CO_THREADS) void cooccur_walk_kernel(CoArgs a) {
    const int64_t qi = ((int64_t)blockIdx.x * CO_THREADS + threadIdx.x) >> 4;
    const int l = threadIdx.x & 15;
    long long w = 0;
    if (qi < a.Q) {
        const int64_t q = a.rows[qi];
        if (q >= 0 && q < a.n_query) {
            const int64_t p1 = a.q_ptr[q + 1];
            for (int64_t e = a.q_ptr[q] + l; e < p1; e += 16) {
                const int64_t u = a.q_nbr[e];
                if (u >= 0 && u < a.n_other) w += a.o_ptr[u + 1] - a.o_ptr[u];
            }
        }
    }
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) w += __shfl_xor(w, off, 16);
    if (qi < a.Q && l == 0) a.walk[qi] = w;
}

__global__ __launch_bounds__(CO_THREADS) void cooccur_lds_kernel(CoArgs a) {
    __shared__ uint64_t s_raw[COOCCUR_SLOTS];                // the table: keys, then counts; later the list's keys over the keys
    __shared__ int s_n;
    int *s_hk = reinterpret_cast<int *>(s_raw), *s_hc = s_hk + COOCCUR_SLOTS;
    const int tid = threadIdx.x;
    const int64_t qi = blockIdx.x;
    const int64_t W = a.walk[qi];
    if (!(a.use_lds && co_in_lds(W))) {                      // (uniform) the dense form's row; without a counter row it gets fillers
        if (a.groups == 0) co_fillers(a, qi, 0, tid);
        return;
    }
    const int64_t q = a.rows[qi];
    if (q < 0 || q >= a.n_query || W == 0) { co_fillers(a, qi, 0, tid); return; }
    for (int s = tid; s < COOCCUR_SLOTS; s += CO_THREADS) { s_hk[s] = -1; s_hc[s] = 0; }
    if (tid == 0) s_n = 0;
    __syncthreads();
    const int g = tid >> 4, l = tid & 15;
    const int64_t p0 = a.q_ptr[q], p1 = a.q_ptr[q + 1];
    for (int64_t e = p0 + g; e < p1; e += 16) {
        const int64_t u = a.q_nbr[e];
        if (u < 0 || u >= a.n_other) continue;
        const int64_t f1 = a.o_ptr[u + 1];
        for (int64_t f = a.o_ptr[u] + l; f < f1; f += 16) {
            const int j = a.o_nbr[f];
            if (j == q || j < 0 || j >= a.n_query) continue;
            int s = j & (COOCCUR_SLOTS - 1);
            for (;;) {                                       // at most W <= SLOTS / 2 distinct keys: a free slot always exists
                const int prev = atomicCAS(&s_hk[s], -1, j);
                if (prev == -1 || prev == j) { atomicAdd(&s_hc[s], 1); break; }
                s = (s + 1) & (COOCCUR_SLOTS - 1);
            }
        }
    }
    __syncthreads();
    // the table to registers, then the list over it
    constexpr int PER = COOCCUR_SLOTS / CO_THREADS;
    int k[PER], c[PER];
#pragma unroll
    for (int i = 0; i < PER; ++i) { k[i] = s_hk[tid + CO_THREADS * i]; c[i] = s_hc[tid + CO_THREADS * i]; }
    __syncthreads();
    uint64_t *s_key = s_raw;
    int *s_c = s_hc;
    const int64_t deg_q = p1 - p0;
#pragma unroll
    for (int i = 0; i < PER; ++i)
        if (k[i] >= 0) {
            const int pos = atomicAdd(&s_n, 1);
            s_key[pos] = co_key(co_score(a.measure, c[i], deg_q, a.q_ptr[k[i] + 1] - a.q_ptr[k[i]]), k[i]);
            s_c[pos] = c[i];
        }
    __syncthreads();
    const int n = s_n;
    co_sort(s_key, s_c, n, tid);
    co_emit(a, qi, s_key, s_c, n, tid);
}

__global__ __launch_bounds__(CO_THREADS) void cooccur_dense_kernel(CoArgs a) {
    __shared__ uint64_t s_key[COOCCUR_CAP];
    __shared__ int s_c[COOCCUR_CAP];
    __shared__ uint64_t s_thr;                               // the K-th kept key once K are kept, else 0
    __shared__ int s_n;
    __shared__ int s_flag[CO_THREADS];
    const int tid = threadIdx.x, g = tid >> 4, l = tid & 15;
    const int64_t G = gridDim.x, b = blockIdx.x;
    int32_t *ctr = a.ctr + b * a.n_query;
    for (int64_t base = 0; base * G < a.Q; base += CO_THREADS) {       // this workgroup's rows: positions p = b (mod G)
        const int64_t mine = (base + tid) * G + b;
        s_flag[tid] = mine < a.Q && !(a.use_lds && co_in_lds(a.walk[mine]));
        __syncthreads();
        for (int i = 0; i < CO_THREADS; ++i) {
            if (!s_flag[i]) continue;                        // (uniform)
            const int64_t qi = (base + i) * G + b;
            const int64_t q = a.rows[qi];
            if (q < 0 || q >= a.n_query) { co_fillers(a, qi, 0, tid); continue; }
            if (tid == 0) { s_n = 0; s_thr = 0; }
            const int64_t p0 = a.q_ptr[q], p1 = a.q_ptr[q + 1], deg_q = p1 - p0;
            // pass 1: count
            for (int64_t e = p0 + g; e < p1; e += 16) {
                const int64_t u = a.q_nbr[e];
                if (u < 0 || u >= a.n_other) continue;
                const int64_t f1 = a.o_ptr[u + 1];
                for (int64_t f = a.o_ptr[u] + l; f < f1; f += 16) {
                    const int j = a.o_nbr[f];
                    if (j == q || j < 0 || j >= a.n_query) continue;
                    atomicAdd(&ctr[j], 1);
                }
            }
            __threadfence();
            __syncthreads();
            // pass 2: claim, 16 users at a time, CO_STEP entries a lane between two capacity checks
            for (int64_t e0 = p0; e0 < p1; e0 += 16) {
                const int64_t e = e0 + g;
                int64_t f = 0, f1 = 0;
                if (e < p1) {
                    const int64_t u = a.q_nbr[e];
                    if (u >= 0 && u < a.n_other) { f = a.o_ptr[u]; f1 = a.o_ptr[u + 1]; }
                }
                for (;;) {
                    const uint64_t thr = s_thr;
#pragma unroll
                    for (int r = 0; r < CO_STEP; ++r) {
                        const int64_t ff = f + l + 16 * r;
                        if (ff >= f1) continue;
                        const int j = a.o_nbr[ff];
                        if (j == q || j < 0 || j >= a.n_query) continue;
                        const int c = atomicExch(&ctr[j], 0);
                        if (c <= 0) continue;                // another lane claimed it
                        const uint64_t key = co_key(co_score(a.measure, c, deg_q, a.q_ptr[j + 1] - a.q_ptr[j]), j);
                        if (key > thr) {
                            const int pos = atomicAdd(&s_n, 1);      // <= CAP - 1024 before the step, at most 1024 adds in it
                            s_key[pos] = key;
                            s_c[pos] = c;
                        }
                    }
                    f += 16 * CO_STEP;
                    const int more = __syncthreads_or(f < f1);
                    if (__syncthreads_or(s_n > COOCCUR_CAP - CO_THREADS * CO_STEP)) {
                        const int n = s_n;
                        co_sort(s_key, s_c, n, tid);
                        if (tid == 0 && n >= a.K) { s_n = a.K; s_thr = s_key[a.K - 1]; }
                        __syncthreads();
                    }
                    if (!more) break;
                }
            }
            __syncthreads();
            const int n = s_n;
            co_sort(s_key, s_c, n, tid);
            co_emit(a, qi, s_key, s_c, n, tid);
            __syncthreads();
        }
        __syncthreads();
    }
}

static inline int64_t co_groups(int64_t n_dense_rows) { return n_dense_rows < COOCCUR_GROUPS ? (n_dense_rows < 0 ? 0 : n_dense_rows) : COOCCUR_GROUPS; }
static inline size_t co_workspace(int64_t n_dense_rows, int64_t n) {
    return align_up((size_t)co_groups(n_dense_rows) * (size_t)n * sizeof(int32_t), 16);
}

static int co_graph(const char *who, CoArgs *a, const int64_t *q_ptr, const int32_t *q_nbr, int64_t n_query, const int64_t *o_ptr,
                    const int32_t *o_nbr, int64_t n_other, const int32_t *rows, int64_t Q) {
    ELIMREC_REQUIRE(n_query >= 0 && n_query < (int64_t)INT32_MAX && n_other >= 0 && n_other < (int64_t)INT32_MAX,
                    "%s: both sides need fewer than 2^31 - 1 rows, got %lld and %lld", who, (long long)n_query, (long long)n_other);
    ELIMREC_REQUIRE(Q >= 0 && Q < ((int64_t)INT32_MAX >> 4), "%s: 0 <= Q < 2^27, got %lld", who, (long long)Q);
    ELIMREC_REQUIRE(Q == 0 || (q_ptr && q_nbr && o_ptr && o_nbr && rows), "%s: null pointer", who);
    a->q_ptr = q_ptr; a->q_nbr = q_nbr; a->n_query = n_query; a->o_ptr = o_ptr; a->o_nbr = o_nbr; a->n_other = n_other;
    a->rows = rows; a->Q = Q;
    return 0;
}

}  // namespace elimrec

using namespace elimrec;

extern "C" int elimrec_cooccur_slots(void) { return COOCCUR_SLOTS; }
extern "C" int elimrec_cooccur_max_k(void) { return COOCCUR_MAX_K; }
extern "C" int elimrec_cooccur_groups(void) { return COOCCUR_GROUPS; }
extern "C" int elimrec_cooccur_rows_in_lds(int64_t W) { return W < 0 ? -1 : (co_in_lds(W) ? 1 : 0); }
extern "C" size_t elimrec_cooccur_workspace(int64_t n_dense_rows, int64_t n) {
    if (n_dense_rows < 0 || n < 0 || n >= (int64_t)INT32_MAX) return 0;
    return co_workspace(n_dense_rows, n);
}

extern "C" int elimrec_cooccur_walk(const int64_t *d_q_ptr, const int32_t *d_q_nbr, int64_t n_query, const int64_t *d_o_ptr,
                                    int64_t n_other, const int32_t *d_rows, int64_t Q, int64_t *d_walk, void *stream) {
    CoArgs a = {};
    if (int rc = co_graph("cooccur_walk", &a, d_q_ptr, d_q_nbr, n_query, d_o_ptr, d_q_nbr, n_other, d_rows, Q)) return rc;
    if (Q == 0) return 0;
    ELIMREC_REQUIRE(d_walk, "cooccur_walk: null pointer");
    a.walk = d_walk;
    hipLaunchKernelGGL(cooccur_walk_kernel, dim3((unsigned)((Q * 16 + CO_THREADS - 1) / CO_THREADS)), dim3(CO_THREADS), 0, (hipStream_t)stream, a);
    ELIMREC_LAUNCH_CHECK("cooccur_walk");
    return 0;
}

extern "C" int elimrec_cooccur_topk(const int64_t *d_q_ptr, const int32_t *d_q_nbr, int64_t n_query, const int64_t *d_o_ptr,
                                    const int32_t *d_o_nbr, int64_t n_other, const int32_t *d_rows, int64_t Q, int K, int measure,
                                    int use_lds, int64_t n_dense_rows, int64_t *d_walk, int32_t *d_idx, float *d_val, int32_t *d_cnt,
                                    void *d_workspace, size_t workspace_bytes, void *stream) {
    ELIMREC_REQUIRE(K >= 1 && K <= COOCCUR_MAX_K, "cooccur_topk: 1 <= K <= %d, got %d", COOCCUR_MAX_K, K);
    ELIMREC_REQUIRE(measure >= 0 && measure <= 2, "cooccur_topk: measure is 0 (count), 1 (cosine) or 2 (jaccard), got %d", measure);
    ELIMREC_REQUIRE(use_lds == 0 || use_lds == 1, "cooccur_topk: use_lds is 0 or 1, got %d", use_lds);
    CoArgs a = {};
    if (int rc = co_graph("cooccur_topk", &a, d_q_ptr, d_q_nbr, n_query, d_o_ptr, d_o_nbr, n_other, d_rows, Q)) return rc;
    ELIMREC_REQUIRE(n_dense_rows >= 0 && n_dense_rows <= Q, "cooccur_topk: 0 <= n_dense_rows <= Q, got %lld", (long long)n_dense_rows);
    ELIMREC_REQUIRE(use_lds || n_dense_rows == Q, "cooccur_topk: without the LDS form every row is a dense row (n_dense_rows = Q)");
    if (Q == 0) return 0;
    ELIMREC_REQUIRE(d_walk && d_idx, "cooccur_topk: null pointer");
    const size_t need = co_workspace(n_dense_rows, n_query);
    ELIMREC_REQUIRE(n_dense_rows == 0 || n_query == 0 || (d_workspace && workspace_bytes >= need && reinterpret_cast<uintptr_t>(d_workspace) % 16 == 0),
                    "cooccur_topk: the workspace needs %zu bytes, 16-byte aligned (got %zu)", need, workspace_bytes);
    a.K = K; a.measure = measure; a.use_lds = use_lds; a.groups = (int)co_groups(n_dense_rows);
    a.walk = d_walk; a.idx = d_idx; a.val = d_val; a.cnt = d_cnt; a.ctr = static_cast<int32_t *>(d_workspace);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(cooccur_walk_kernel, dim3((unsigned)((Q * 16 + CO_THREADS - 1) / CO_THREADS)), dim3(CO_THREADS), 0, s, a);
    ELIMREC_LAUNCH_CHECK("cooccur_topk (walk)");
    if (use_lds) {
        hipLaunchKernelGGL(cooccur_lds_kernel, dim3((unsigned)Q), dim3(CO_THREADS), 0, s, a);
        ELIMREC_LAUNCH_CHECK("cooccur_topk (LDS form)");
    }
    if (a.groups > 0) {
        hipLaunchKernelGGL(cooccur_dense_kernel, dim3((unsigned)a.groups), dim3(CO_THREADS), 0, s, a);
        ELIMREC_LAUNCH_CHECK("cooccur_topk (dense form)");
    }
    return 0;
}
