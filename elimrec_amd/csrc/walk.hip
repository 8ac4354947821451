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
// form, as there -- the traversal and both forms are co_graph.h's, shared with cooccur.hip; this file is their 64-bit accumulator:
//   LDS form   (W <= WALK_SLOTS / 2): an open-addressing table of WALK_SLOTS = 4096 (int32 key, int64 sum) entries in LDS, 48 KiB,
//              home slot id % WALK_SLOTS, linear probing; W bounds the entries, so the load factor is at most 0.5 whatever the ids
//              are. Insertion is an integer compare-and-swap on the key and a 64-bit integer add on the sum. The selection list
//              (WALK_SLOTS / 2 = 2048 keys, 24 KiB with co_sort's companion words) is written OVER the table once the table sits in
//              registers as keys.
//   dense form (any W): at most WALK_GROUPS workgroups loop over the rows that need it; each owns a row of n int64 sums in the
//              workspace, ZERO when the call starts. Pass 1 adds the weights with 64-bit integer atomics -- a weight of 0 sets the
//              word's top bit instead, which no sum reaches, so that a touched entry is never 0 --; pass 2 walks the entries again
//              and claims each touched sum with an exchange to 0: the lane that gets a word != 0 offers the candidate against the
//              K-th kept key, and the row is clean again for the next query. The cut-and-raise rule is co_select.h's.
// Selection is co_select.h's. Integer adds commute: a row's outputs depend bit for bit on the graph, the three arrays, the row and K
// -- not on the arrival order, the form, Q, the row's place in `rows` or the grid. No floating-point atomics, no floating-point sums.
#include <cmath>
#include "common.h"
#include "co_select.h"
#include "co_graph.h"

namespace elimrec {

constexpr int WALK_SLOTS = 4096, WALK_MAX_K = 256, WALK_GROUPS = 512, WALK_FRAC_BITS = 40;     // the list: WALK_SLOTS / 2 slots
constexpr int WALK_STEP = 4;                                 // 2-hop entries a lane claims between two capacity checks
constexpr unsigned long long WALK_MARK = 1ull << 63;         // the dense form's "touched by a weight of 0"; sums stay below 2^62

__device__ __forceinline__ float walk_score(long long S, double row_scale, double col_scale) {
    return (float)((((double)S * (1.0 / (double)(1ull << WALK_FRAC_BITS))) * row_scale) * col_scale);
}

// the accumulator of co_graph.h's traversal: a 64-bit sum of the middle nodes' weights, scored with the two scales; nothing is listed
// beside a key (there is no cnt output)
struct WalkSum {
    using Word = unsigned long long;
    using Row = double;                                      // row_scale[q]
    static constexpr bool COUNTS = false;
    const int64_t *mid_weight;                               // [n_other] >= 0
    const double *row_scale, *col_scale;                     // [n_query] each
    __device__ __forceinline__ Word through(int64_t u) const { return (Word)mid_weight[u]; }
    __device__ static __forceinline__ void touch(Word *at, Word w) {
        if (w) atomicAdd(at, w); else atomicOr(at, WALK_MARK);
    }
    __device__ __forceinline__ Row row(const CoGraph &, int64_t q) const { return row_scale[q]; }
    __device__ __forceinline__ float score(const CoGraph &, Row rs, int j, Word S, int *cnt) const {
        *cnt = 0;
        return walk_score((long long)(S & ~WALK_MARK), rs, col_scale[j]);
    }
};
using WalkArgs = CoCall<WalkSum>;

__global__ __launch_bounds__(CO_THREADS) void walk_lds_kernel(WalkArgs a) { co_lds_form<WALK_SLOTS>(a.g, a.p); }
__global__ __launch_bounds__(CO_THREADS) void walk_dense_kernel(WalkArgs a) { co_dense_form<WALK_SLOTS, WALK_STEP, WALK_MAX_K>(a.g, a.p); }

}  // namespace elimrec

using namespace elimrec;

extern "C" int elimrec_walk_slots(void) { return WALK_SLOTS; }
extern "C" int elimrec_walk_max_k(void) { return WALK_MAX_K; }
extern "C" int elimrec_walk_groups(void) { return WALK_GROUPS; }
extern "C" int elimrec_walk_frac_bits(void) { return WALK_FRAC_BITS; }
extern "C" int elimrec_walk_rows_in_lds(int64_t W) { return W < 0 ? -1 : (co_in_lds<WALK_SLOTS>(W) ? 1 : 0); }
extern "C" size_t elimrec_walk_workspace(int64_t n_dense_rows, int64_t n) {
    if (n_dense_rows < 0 || n < 0 || n >= (int64_t)INT32_MAX) return 0;
    return co_workspace(n_dense_rows, WALK_GROUPS, n, sizeof(int64_t));
}

extern "C" int elimrec_walk_topk(const int64_t *d_q_ptr, const int32_t *d_q_nbr, int64_t n_query, const int64_t *d_o_ptr,
                                 const int32_t *d_o_nbr, int64_t n_other, const int32_t *d_rows, int64_t Q, int K,
                                 const int64_t *d_mid_weight, const double *d_row_scale, const double *d_col_scale, int use_lds,
                                 int64_t n_dense_rows, int64_t *d_walk, int32_t *d_idx, float *d_val, void *d_workspace,
                                 size_t workspace_bytes, void *stream) {
    const char *who = "walk_topk";
    if (int rc = co_check_forms(who, K, WALK_MAX_K, use_lds)) return rc;
    WalkArgs a = {};
    if (int rc = co_graph(who, &a.g, d_q_ptr, d_q_nbr, n_query, d_o_ptr, d_o_nbr, true, n_other, d_rows, Q)) return rc;
    if (int rc = co_check_dense_rows(who, n_dense_rows, Q, "Q")) return rc;
    ELIMREC_REQUIRE(use_lds || n_dense_rows == Q, "%s: without the LDS form every row is a dense row (n_dense_rows = Q)", who);
    if (Q == 0) return 0;
    ELIMREC_REQUIRE(d_walk && d_idx, "%s: null pointer", who);
    ELIMREC_REQUIRE((n_other == 0 || d_mid_weight) && (n_query == 0 || (d_row_scale && d_col_scale)), "%s: null weights", who);
    if (int rc = co_check_workspace(who, n_dense_rows, n_query, co_workspace(n_dense_rows, WALK_GROUPS, n_query, sizeof(int64_t)),
                                    d_workspace, workspace_bytes)) return rc;
    if (int rc = elimrec_cooccur_walk(d_q_ptr, d_q_nbr, n_query, d_o_ptr, n_other, d_rows, Q, d_walk, stream)) return rc;
    a.g.use_lds = use_lds; a.g.groups = (int)co_groups(n_dense_rows, WALK_GROUPS);
    a.g.walk = d_walk; a.g.out = {K, d_idx, d_val, nullptr}; a.g.acc = d_workspace;
    a.p = {d_mid_weight, d_row_scale, d_col_scale};
    return co_launch_forms(walk_lds_kernel, "walk_topk (LDS form)", walk_dense_kernel, "walk_topk (dense form)", Q, use_lds, a.g.groups, a,
                           (hipStream_t)stream);
}
