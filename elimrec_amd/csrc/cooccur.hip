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
// One workgroup of 256 threads per query row. W(q) = the sum of deg(u) over q's segment (cooccur_walk_kernel, int64) picks the form
// (co_select.h, and co_graph.h for the traversal walk.hip shares):
//   LDS form   (W <= COOCCUR_SLOTS / 2): an open-addressing table of COOCCUR_SLOTS = 4096 (key, count) pairs in LDS, 32 KiB, home
//              slot id % COOCCUR_SLOTS, linear probing; W bounds the entries, so the load factor is at most 0.5 whatever the ids are.
//              Insertion is an integer compare-and-swap on the key and an integer add on the count.
//   dense form (any W): a fixed number of workgroups (at most COOCCUR_GROUPS) loop over the rows that need it; each owns an int32
//              counter row of n entries in the workspace, ZERO when the call starts. Pass 1 walks the 2-hop entries and adds with
//              integer atomics; pass 2 walks them again and claims each touched counter with an exchange to 0: the lane that gets
//              c > 0 offers (c, j), and the row is clean again for the next query.
// The 16 lanes of a quarter wave share one u of q's segment and stride its list, so 16 users are in flight per workgroup.
//
// Selection is co_select.h's: one 64-bit key per candidate, a list of COOCCUR_SLOTS / 2 = 2048 slots in LDS -- the LDS form's table holds at
// most that many -- sorted by a bitonic network; the dense form compares the FULL key against the K-th kept key and, when the list
// could overflow, sorts it and cuts it to the K best. A row's outputs therefore depend bit for bit on the graph, the row, K and the
// measure -- not on the arrival order, the form, Q, the row's place in `rows` or the grid. No floating-point atomics.
// A query id outside the side gives fillers; a neighbour id outside its side is skipped and never dereferenced.
#include <cmath>
#include "common.h"
#include "co_select.h"
#include "co_graph.h"

namespace elimrec {

constexpr int COOCCUR_SLOTS = 4096, COOCCUR_MAX_K = 256, COOCCUR_GROUPS = 512;     // the list: COOCCUR_SLOTS / 2 slots (co_graph.h)
constexpr int CO_STEP = 4;                                   // CO_STEP: 2-hop entries a lane claims between two capacity checks

__device__ __forceinline__ float co_score(int measure, int c, int64_t a, int64_t b) {
    if (measure == 0) return (float)c;
    if (measure == 1) return (float)((double)c / sqrt((double)a * (double)b));
    return (float)((double)c / (double)(a + b - (int64_t)c));
}

// the accumulator of co_graph.h's traversal: an int32 count of the walks, scored against the two degrees
struct CoCount {
    using Word = int32_t;
    using Row = int64_t;                                     // deg(q)
    static constexpr bool COUNTS = true;
    int measure;
    __device__ __forceinline__ Word through(int64_t) const { return 1; }
    __device__ static __forceinline__ void touch(Word *at, Word w) { atomicAdd(at, w); }
    __device__ __forceinline__ Row row(const CoGraph &g, int64_t q) const { return g.q_ptr[q + 1] - g.q_ptr[q]; }
    __device__ __forceinline__ float score(const CoGraph &g, Row deg_q, int j, Word c, int *cnt) const {
        *cnt = c;
        return co_score(measure, c, deg_q, g.q_ptr[j + 1] - g.q_ptr[j]);
    }
};
using CoArgs = CoCall<CoCount>;

// W(q) of every query: one quarter wave per query
__global__ __launch_bounds__(CO_THREADS) void cooccur_walk_kernel(CoGraph a) {
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

__global__ __launch_bounds__(CO_THREADS) void cooccur_lds_kernel(CoArgs a) { co_lds_form<COOCCUR_SLOTS>(a.g, a.p); }
__global__ __launch_bounds__(CO_THREADS) void cooccur_dense_kernel(CoArgs a) { co_dense_form<COOCCUR_SLOTS, CO_STEP, COOCCUR_MAX_K>(a.g, a.p); }

static int co_launch_walk(const char *what, const CoGraph &g, hipStream_t s) {
    hipLaunchKernelGGL(cooccur_walk_kernel, dim3((unsigned)((g.Q * 16 + CO_THREADS - 1) / CO_THREADS)), dim3(CO_THREADS), 0, s, g);
    ELIMREC_LAUNCH_CHECK(what);
    return 0;
}

}  // namespace elimrec

using namespace elimrec;

extern "C" int elimrec_cooccur_slots(void) { return COOCCUR_SLOTS; }
extern "C" int elimrec_cooccur_max_k(void) { return COOCCUR_MAX_K; }
extern "C" int elimrec_cooccur_groups(void) { return COOCCUR_GROUPS; }
extern "C" int elimrec_cooccur_rows_in_lds(int64_t W) { return W < 0 ? -1 : (co_in_lds<COOCCUR_SLOTS>(W) ? 1 : 0); }
extern "C" size_t elimrec_cooccur_workspace(int64_t n_dense_rows, int64_t n) {
    if (n_dense_rows < 0 || n < 0 || n >= (int64_t)INT32_MAX) return 0;
    return co_workspace(n_dense_rows, COOCCUR_GROUPS, n, sizeof(int32_t));
}

extern "C" int elimrec_cooccur_walk(const int64_t *d_q_ptr, const int32_t *d_q_nbr, int64_t n_query, const int64_t *d_o_ptr,
                                    int64_t n_other, const int32_t *d_rows, int64_t Q, int64_t *d_walk, void *stream) {
    CoGraph g = {};
    if (int rc = co_graph("cooccur_walk", &g, d_q_ptr, d_q_nbr, n_query, d_o_ptr, nullptr, false, n_other, d_rows, Q)) return rc;
    if (Q == 0) return 0;
    ELIMREC_REQUIRE(d_walk, "cooccur_walk: null pointer");
    g.walk = d_walk;
    return co_launch_walk("cooccur_walk", g, (hipStream_t)stream);
}

extern "C" int elimrec_cooccur_topk(const int64_t *d_q_ptr, const int32_t *d_q_nbr, int64_t n_query, const int64_t *d_o_ptr,
                                    const int32_t *d_o_nbr, int64_t n_other, const int32_t *d_rows, int64_t Q, int K, int measure,
                                    int use_lds, int64_t n_dense_rows, int64_t *d_walk, int32_t *d_idx, float *d_val, int32_t *d_cnt,
                                    void *d_workspace, size_t workspace_bytes, void *stream) {
    const char *who = "cooccur_topk";
    if (int rc = co_check_forms(who, K, COOCCUR_MAX_K, use_lds)) return rc;
    ELIMREC_REQUIRE(measure >= 0 && measure <= 2, "%s: measure is 0 (count), 1 (cosine) or 2 (jaccard), got %d", who, measure);
    CoArgs a = {};
    if (int rc = co_graph(who, &a.g, d_q_ptr, d_q_nbr, n_query, d_o_ptr, d_o_nbr, true, n_other, d_rows, Q)) return rc;
    if (int rc = co_check_dense_rows(who, n_dense_rows, Q, "Q")) return rc;
    ELIMREC_REQUIRE(use_lds || n_dense_rows == Q, "%s: without the LDS form every row is a dense row (n_dense_rows = Q)", who);
    if (Q == 0) return 0;
    ELIMREC_REQUIRE(d_walk && d_idx, "%s: null pointer", who);
    if (int rc = co_check_workspace(who, n_dense_rows, n_query, co_workspace(n_dense_rows, COOCCUR_GROUPS, n_query, sizeof(int32_t)),
                                    d_workspace, workspace_bytes)) return rc;
    a.g.use_lds = use_lds; a.g.groups = (int)co_groups(n_dense_rows, COOCCUR_GROUPS);
    a.g.walk = d_walk; a.g.out = {K, d_idx, d_val, d_cnt}; a.g.acc = d_workspace;
    a.p.measure = measure;
    hipStream_t s = (hipStream_t)stream;
    if (int rc = co_launch_walk("cooccur_topk (walk)", a.g, s)) return rc;
    return co_launch_forms(cooccur_lds_kernel, "cooccur_topk (LDS form)", cooccur_dense_kernel, "cooccur_topk (dense form)", Q, use_lds, a.g.groups, a, s);
}
