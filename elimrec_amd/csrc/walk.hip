// Weighted two-step walks (P3alpha / RP3beta, Adamic-Adar, resource allocation): per query row of one side of a bipartite graph the K
// rows of the same side with the largest walk score. The graph comes as cooccur.hip takes it: q_ptr / q_nbr maps a row of the query
// side to its neighbours on the other side (item -> its training users), o_ptr / o_nbr maps a row of the other side back. Where
// cooccur.hip counts the walks q -> u -> j with integer 1s, a walk here weighs mid_weight[u], a NON-NEGATIVE int64 in WALK_FRAC_BITS =
// 40 bit fixed point the host provides (RP3beta: rint(deg(u)^-alpha * 2^40)). Integer arithmetic up to the score:
//
//   S(q, j)   = the sum over the two-step walks q -> u -> j, j != q, of mid_weight[u]   (int64; a repeated edge is a walk of its own)
//   val(q, j) = (float)( (((double)S * 2^-40) * row_scale[q]) * col_scale[j] )           (float64, three multiplies left to right, one
//                                                                                         rounding to fp32; no pow on the device)
// row_scale / col_scale: float64 [n_query] from the host, finite and >= 0. THE CALLER keeps S within int64: (the largest W) x (the
// largest weight) < 2^62. Listed are the rows with at least one walk through a valid u -- a sum of 0 (weights of 0) is listed with
// score 0 -- never q itself; order (fp32 score descending, id ascending); fillers -1 / -inf. A query id outside the side gives
// fillers; a neighbour id outside its side is skipped and never dereferenced.
//
// One workgroup of 256 threads per query row; W(q) = the sum of deg(u) over q's segment (cooccur.hip's cooccur_walk_kernel) picks the
// form, as there:
//   LDS form   (W <= WALK_SLOTS / 2): an open-addressing table of WALK_SLOTS = 4096 (int32 key, int64 sum) entries in LDS, 48 KiB,
//              home slot id % WALK_SLOTS, linear probing; W bounds the entries, so the load factor is at most 0.5 whatever the ids
//              are. Insertion is an integer compare-and-swap on the key and a 64-bit integer add on the sum. The selection list
//              (WALK_CAP = 2048 keys, 24 KiB with co_sort's companion words) is written OVER the table once the table sits in
//              registers as keys.
//   dense form (any W): at most WALK_GROUPS workgroups loop over the rows that need it; each owns a row of n int64 sums in the
//              workspace, ZERO when the call starts. Pass 1 adds the weights with 64-bit integer atomics -- a weight of 0 sets the
//              word's top bit instead, which no sum reaches, so that a touched entry is never 0 --; pass 2 walks the entries again
//              and claims each touched sum with an exchange to 0: the lane that gets a word != 0 offers the candidate against the
//              K-th kept key, and the row is clean again for the next query. The cut-and-raise rule is cooccur.hip's.
// Selection is co_select.h's. Integer adds commute: a row's outputs depend bit for bit on the graph, the three arrays, the row and K
// -- not on the arrival order, the form, Q, the row's place in `rows` or the grid. No floating-point atomics, no floating-point sums.
#include <cmath>
#include "common.h"
#include "co_select.h"

namespace elimrec {

constexpr int WALK_SLOTS = 4096, WALK_MAX_K = 256, WALK_CAP = WALK_SLOTS / 2, WALK_GROUPS = 512, WALK_FRAC_BITS = 40;
constexpr int WALK_STEP = 4;                                 // 2-hop entries a lane claims between two capacity checks
constexpr unsigned long long WALK_MARK = 1ull << 63;         // the dense form's "touched by a weight of 0"; sums stay below 2^62
static_assert(WALK_CAP >= 2 * CO_THREADS * WALK_STEP && WALK_CAP - CO_THREADS * WALK_STEP >= WALK_MAX_K, "the dense form's list");
static_assert(WALK_SLOTS * 12 + 64 <= 64 * 1024 && WALK_CAP * 12 <= WALK_SLOTS * 8, "the LDS form's table within 64 KiB, the list over its sums");

struct WalkArgs {
    const int64_t *q_ptr; const int32_t *q_nbr; int64_t n_query;
    const int64_t *o_ptr; const int32_t *o_nbr; int64_t n_other;
    const int32_t *rows; int64_t Q;
    const int64_t *mid_weight;                               // [n_other] >= 0
    const double *row_scale, *col_scale;                     // [n_query] each
    int K, use_lds, groups;
    const int64_t *walk;                                     // [Q] W(q)
    int32_t *idx; float *val;                                // [Q x K]; val may be null
    unsigned long long *sum;                                 // [groups][n_query] the dense form's rows
};

__host__ __device__ inline bool walk_in_lds(int64_t W) { return W >= 0 && W <= WALK_SLOTS / 2; }

__device__ __forceinline__ float walk_score(long long S, double row_scale, double col_scale) {
    return (float)((((double)S * (1.0 / (double)(1ull << WALK_FRAC_BITS))) * row_scale) * col_scale);
}

__device__ __forceinline__ void walk_fillers(const WalkArgs &a, int64_t qi, int from, int tid) {
    for (int k = from + tid; k < a.K; k += CO_THREADS) {
        a.idx[qi * a.K + k] = -1;
        if (a.val) a.val[qi * a.K + k] = -__builtin_huge_valf();
    }
}

// the sorted list's K best to row qi of the outputs, fillers behind them
__device__ __forceinline__ void walk_emit(const WalkArgs &a, int64_t qi, const uint64_t *key, int n, int tid) {
    const int kept = n < a.K ? n : a.K;
    for (int k = tid; k < kept; k += CO_THREADS) {
        a.idx[qi * a.K + k] = co_key_id(key[k]);
        if (a.val) a.val[qi * a.K + k] = co_key_score(key[k]);
    }
    walk_fillers(a, qi, kept, tid);
}

__global__ __launch_bounds__(CO_THREADS) void walk_lds_kernel(WalkArgs a) {
    __shared__ unsigned long long s_hs[WALK_SLOTS];          // the table's sums; later the list's keys and companion words over them
    __shared__ int s_hk[WALK_SLOTS];                         // the table's keys
    __shared__ int s_n;
    const int tid = threadIdx.x;
    const int64_t qi = blockIdx.x;
    const int64_t W = a.walk[qi];
    if (!(a.use_lds && walk_in_lds(W))) {                    // (uniform) the dense form's row; without a row there it gets fillers
        if (a.groups == 0) walk_fillers(a, qi, 0, tid);
        return;
    }
    const int64_t q = a.rows[qi];
    if (q < 0 || q >= a.n_query || W == 0) { walk_fillers(a, qi, 0, tid); return; }
    for (int s = tid; s < WALK_SLOTS; s += CO_THREADS) { s_hk[s] = -1; s_hs[s] = 0; }
    if (tid == 0) s_n = 0;
    __syncthreads();
    const int g = tid >> 4, l = tid & 15;
    const int64_t p0 = a.q_ptr[q], p1 = a.q_ptr[q + 1];
    for (int64_t e = p0 + g; e < p1; e += 16) {
        const int64_t u = a.q_nbr[e];
        if (u < 0 || u >= a.n_other) continue;
        const unsigned long long w = (unsigned long long)a.mid_weight[u];
        const int64_t f1 = a.o_ptr[u + 1];
        for (int64_t f = a.o_ptr[u] + l; f < f1; f += 16) {
            const int j = a.o_nbr[f];
            if (j == q || j < 0 || j >= a.n_query) continue;
            int s = j & (WALK_SLOTS - 1);
            for (;;) {                                       // at most W <= SLOTS / 2 distinct keys: a free slot always exists
                const int prev = atomicCAS(&s_hk[s], -1, j);
                if (prev == -1 || prev == j) { atomicAdd(&s_hs[s], w); break; }
                s = (s + 1) & (WALK_SLOTS - 1);
            }
        }
    }
    __syncthreads();
    // the table to registers as the candidates' keys (0: an empty slot), then the list over it
    constexpr int PER = WALK_SLOTS / CO_THREADS;
    const double rs = a.row_scale[q];
    uint64_t key[PER];
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int k = s_hk[tid + CO_THREADS * i];
        key[i] = k >= 0 ? co_key(walk_score((long long)s_hs[tid + CO_THREADS * i], rs, a.col_scale[k]), k) : 0;
    }
    __syncthreads();
    uint64_t *s_key = reinterpret_cast<uint64_t *>(s_hs);
    int *s_c = reinterpret_cast<int *>(s_hs + WALK_CAP);     // co_sort's companion words: nothing rides beside a key here
#pragma unroll
    for (int i = 0; i < PER; ++i)
        if (key[i]) {
            const int pos = atomicAdd(&s_n, 1);              // at most W <= CAP entries
            s_key[pos] = key[i];
            s_c[pos] = 0;
        }
    __syncthreads();
    const int n = s_n;
    co_sort(s_key, s_c, n, tid);
    walk_emit(a, qi, s_key, n, tid);
}

__global__ __launch_bounds__(CO_THREADS) void walk_dense_kernel(WalkArgs a) {
    __shared__ uint64_t s_key[WALK_CAP];
    __shared__ int s_c[WALK_CAP];                            // co_sort's companion words
    __shared__ uint64_t s_thr;                               // the K-th kept key once K are kept, else 0
    __shared__ int s_n;
    __shared__ int s_flag[CO_THREADS];
    const int tid = threadIdx.x, g = tid >> 4, l = tid & 15;
    const int64_t G = gridDim.x, b = blockIdx.x;
    unsigned long long *sum = a.sum + b * a.n_query;
    for (int64_t base = 0; base * G < a.Q; base += CO_THREADS) {       // this workgroup's rows: positions p = b (mod G)
        const int64_t mine = (base + tid) * G + b;
        s_flag[tid] = mine < a.Q && !(a.use_lds && walk_in_lds(a.walk[mine]));
        __syncthreads();
        for (int i = 0; i < CO_THREADS; ++i) {
            if (!s_flag[i]) continue;                        // (uniform)
            const int64_t qi = (base + i) * G + b;
            const int64_t q = a.rows[qi];
            if (q < 0 || q >= a.n_query) { walk_fillers(a, qi, 0, tid); continue; }
            if (tid == 0) { s_n = 0; s_thr = 0; }
            const int64_t p0 = a.q_ptr[q], p1 = a.q_ptr[q + 1];
            const double rs = a.row_scale[q];
            // pass 1: add the weights
            for (int64_t e = p0 + g; e < p1; e += 16) {
                const int64_t u = a.q_nbr[e];
                if (u < 0 || u >= a.n_other) continue;
                const unsigned long long w = (unsigned long long)a.mid_weight[u];
                const int64_t f1 = a.o_ptr[u + 1];
                for (int64_t f = a.o_ptr[u] + l; f < f1; f += 16) {
                    const int j = a.o_nbr[f];
                    if (j == q || j < 0 || j >= a.n_query) continue;
                    if (w) atomicAdd(&sum[j], w); else atomicOr(&sum[j], WALK_MARK);
                }
            }
            __threadfence();
            __syncthreads();
            // pass 2: claim, 16 middle nodes at a time, WALK_STEP entries a lane between two capacity checks
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
                    for (int r = 0; r < WALK_STEP; ++r) {
                        const int64_t ff = f + l + 16 * r;
                        if (ff >= f1) continue;
                        const int j = a.o_nbr[ff];
                        if (j == q || j < 0 || j >= a.n_query) continue;
                        const unsigned long long v = atomicExch(&sum[j], 0ull);
                        if (v == 0) continue;                // another lane claimed it
                        const uint64_t key = co_key(walk_score((long long)(v & ~WALK_MARK), rs, a.col_scale[j]), j);
                        if (key > thr) {
                            const int pos = atomicAdd(&s_n, 1);      // <= CAP - 1024 before the step, at most 1024 adds in it
                            s_key[pos] = key;
                            s_c[pos] = 0;
                        }
                    }
                    f += 16 * WALK_STEP;
                    const int more = __syncthreads_or(f < f1);
                    if (__syncthreads_or(s_n > WALK_CAP - CO_THREADS * WALK_STEP)) {
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
            walk_emit(a, qi, s_key, n, tid);
            __syncthreads();
        }
        __syncthreads();
    }
}

static inline int64_t walk_groups(int64_t n_dense_rows) { return n_dense_rows < WALK_GROUPS ? (n_dense_rows < 0 ? 0 : n_dense_rows) : WALK_GROUPS; }
static inline size_t walk_workspace(int64_t n_dense_rows, int64_t n) {
    return align_up((size_t)walk_groups(n_dense_rows) * (size_t)n * sizeof(int64_t), 16);
}

}  // namespace elimrec

using namespace elimrec;

extern "C" int elimrec_walk_slots(void) { return WALK_SLOTS; }
extern "C" int elimrec_walk_max_k(void) { return WALK_MAX_K; }
extern "C" int elimrec_walk_groups(void) { return WALK_GROUPS; }
extern "C" int elimrec_walk_frac_bits(void) { return WALK_FRAC_BITS; }
extern "C" int elimrec_walk_rows_in_lds(int64_t W) { return W < 0 ? -1 : (walk_in_lds(W) ? 1 : 0); }
extern "C" size_t elimrec_walk_workspace(int64_t n_dense_rows, int64_t n) {
    if (n_dense_rows < 0 || n < 0 || n >= (int64_t)INT32_MAX) return 0;
    return walk_workspace(n_dense_rows, n);
}

extern "C" int elimrec_walk_topk(const int64_t *d_q_ptr, const int32_t *d_q_nbr, int64_t n_query, const int64_t *d_o_ptr,
                                 const int32_t *d_o_nbr, int64_t n_other, const int32_t *d_rows, int64_t Q, int K,
                                 const int64_t *d_mid_weight, const double *d_row_scale, const double *d_col_scale, int use_lds,
                                 int64_t n_dense_rows, int64_t *d_walk, int32_t *d_idx, float *d_val, void *d_workspace,
                                 size_t workspace_bytes, void *stream) {
    const char *who = "walk_topk";
    ELIMREC_REQUIRE(K >= 1 && K <= WALK_MAX_K, "%s: 1 <= K <= %d, got %d", who, WALK_MAX_K, K);
    ELIMREC_REQUIRE(use_lds == 0 || use_lds == 1, "%s: use_lds is 0 or 1, got %d", who, use_lds);
    ELIMREC_REQUIRE(n_query >= 0 && n_query < (int64_t)INT32_MAX && n_other >= 0 && n_other < (int64_t)INT32_MAX,
                    "%s: both sides need fewer than 2^31 - 1 rows, got %lld and %lld", who, (long long)n_query, (long long)n_other);
    ELIMREC_REQUIRE(Q >= 0 && Q < ((int64_t)INT32_MAX >> 4), "%s: 0 <= Q < 2^27, got %lld", who, (long long)Q);
    ELIMREC_REQUIRE(n_dense_rows >= 0 && n_dense_rows <= Q, "%s: 0 <= n_dense_rows <= Q, got %lld", who, (long long)n_dense_rows);
    ELIMREC_REQUIRE(use_lds || n_dense_rows == Q, "%s: without the LDS form every row is a dense row (n_dense_rows = Q)", who);
    if (Q == 0) return 0;
    ELIMREC_REQUIRE(d_q_ptr && d_q_nbr && d_o_ptr && d_o_nbr && d_rows && d_walk && d_idx, "%s: null pointer", who);
    ELIMREC_REQUIRE((n_other == 0 || d_mid_weight) && (n_query == 0 || (d_row_scale && d_col_scale)), "%s: null weights", who);
    const size_t need = walk_workspace(n_dense_rows, n_query);
    ELIMREC_REQUIRE(n_dense_rows == 0 || n_query == 0 || (d_workspace && workspace_bytes >= need && reinterpret_cast<uintptr_t>(d_workspace) % 16 == 0),
                    "%s: the workspace needs %zu bytes, 16-byte aligned (got %zu)", who, need, workspace_bytes);
    if (int rc = elimrec_cooccur_walk(d_q_ptr, d_q_nbr, n_query, d_o_ptr, n_other, d_rows, Q, d_walk, stream)) return rc;
    WalkArgs a = {};
    a.q_ptr = d_q_ptr; a.q_nbr = d_q_nbr; a.n_query = n_query; a.o_ptr = d_o_ptr; a.o_nbr = d_o_nbr; a.n_other = n_other;
    a.rows = d_rows; a.Q = Q;
    a.mid_weight = d_mid_weight; a.row_scale = d_row_scale; a.col_scale = d_col_scale;
    a.K = K; a.use_lds = use_lds; a.groups = (int)walk_groups(n_dense_rows);
    a.walk = d_walk; a.idx = d_idx; a.val = d_val; a.sum = static_cast<unsigned long long *>(d_workspace);
    hipStream_t s = (hipStream_t)stream;
    if (use_lds) {
        hipLaunchKernelGGL(walk_lds_kernel, dim3((unsigned)Q), dim3(CO_THREADS), 0, s, a);
        ELIMREC_LAUNCH_CHECK("walk_topk (LDS form)");
    }
    if (a.groups > 0) {
        hipLaunchKernelGGL(walk_dense_kernel, dim3((unsigned)a.groups), dim3(CO_THREADS), 0, s, a);
        ELIMREC_LAUNCH_CHECK("walk_topk (dense form)");
    }
    return 0;
}
