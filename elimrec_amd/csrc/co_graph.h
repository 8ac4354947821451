// The two-step walks q -> u -> j over a bipartite graph that cooccur.hip and walk.hip rank: one traversal, two accumulators. The graph
// comes as two CSRs: q_ptr / q_nbr maps a row of the query side to its neighbours on the other side (item -> its training users),
// o_ptr / o_nbr maps a row of the other side back (user -> items). A repeated edge is an edge of its own, so the walks from q to j are
// counted as a product. Never q itself (j != q); a query id outside the side gives fillers; a neighbour id outside its side is skipped
// and never dereferenced.
//
// One workgroup of 256 threads per query row (co_select.h). W(q) = the sum of deg(u) over q's segment (cooccur_walk_kernel, int64) --
// the number of 2-hop entries the row walks -- picks the form: the LDS form for W <= SLOTS / 2 (W bounds the table's entries), the
// dense form for any W. The 16 lanes of a quarter wave share one u of q's segment and stride its list, so 16 middle nodes are in
// flight per workgroup.
//
// What is accumulated per (q, j) and how it becomes a score is the family's policy P:
//   P::Word                       the accumulator word, int32 (a count) or 64-bit (a fixed-point sum); 0 = untouched
//   p.through(u)                  what a walk through u adds
//   P::touch(word, w)             adds it to a word of the DENSE form's row, so that a touched word is never 0
//   p.row(g, q) -> P::Row         what the row's scores need of q, read once per row
//   p.score(g, row, j, word, &c)  the claimed word's fp32 score, and the count listed beside it
//   P::COUNTS                     whether a count is listed at all: without one the cnt output is known to be null at compile time
#pragma once
#include "common.h"
#include "co_select.h"

namespace elimrec {

struct CoGraph {
    const int64_t *q_ptr; const int32_t *q_nbr; int64_t n_query;
    const int64_t *o_ptr; const int32_t *o_nbr; int64_t n_other;
    const int32_t *rows; int64_t Q;
    int use_lds, groups;
    CoOut out;                                               // [Q x K]
    int64_t *walk;                                           // [Q] W(q)
    void *acc;                                               // [groups][n_query] P::Word: the dense form's accumulator rows
};
template <class P> struct CoCall { CoGraph g; P p; };

// the sizes of a call and the pointers it needs: o_nbr only where the second hop is walked
static int co_graph(const char *who, CoGraph *g, const int64_t *q_ptr, const int32_t *q_nbr, int64_t n_query, const int64_t *o_ptr,
                    const int32_t *o_nbr, bool need_o_nbr, int64_t n_other, const int32_t *rows, int64_t Q) {
    ELIMREC_REQUIRE(n_query >= 0 && n_query < (int64_t)INT32_MAX && n_other >= 0 && n_other < (int64_t)INT32_MAX,
                    "%s: both sides need fewer than 2^31 - 1 rows, got %lld and %lld", who, (long long)n_query, (long long)n_other);
    ELIMREC_REQUIRE(Q >= 0 && Q < ((int64_t)INT32_MAX >> 4), "%s: 0 <= Q < 2^27, got %lld", who, (long long)Q);
    ELIMREC_REQUIRE(Q == 0 || (q_ptr && q_nbr && o_ptr && (o_nbr || !need_o_nbr) && rows), "%s: null pointer", who);
    g->q_ptr = q_ptr; g->q_nbr = q_nbr; g->n_query = n_query; g->o_ptr = o_ptr; g->o_nbr = o_nbr; g->n_other = n_other;
    g->rows = rows; g->Q = Q;
    return 0;
}

template <int SLOTS>
__host__ __device__ inline bool co_in_lds(int64_t W) { return W >= 0 && W <= SLOTS / 2; }

template <class P>
__device__ __forceinline__ CoOut co_out(const CoGraph &g) { return {g.out.K, g.out.idx, g.out.val, P::COUNTS ? g.out.cnt : nullptr}; }

// every 2-hop entry (u, j) of row q, j a valid id other than q, to visit(what a walk through u adds, j): a quarter wave of 16 lanes takes
// one u, its lanes stride u's list
template <class P, class Visit>
__device__ __forceinline__ void co_two_hops(const CoGraph &g, const P &p, int64_t q, int64_t p0, int64_t p1, int tid, Visit visit) {
    for (int64_t e = p0 + (tid >> 4); e < p1; e += 16) {
        const int64_t u = g.q_nbr[e];
        if (u < 0 || u >= g.n_other) continue;
        const typename P::Word w = p.through(u);
        const int64_t f1 = g.o_ptr[u + 1];
        for (int64_t f = g.o_ptr[u] + (tid & 15); f < f1; f += 16) {
            const int j = g.o_nbr[f];
            if (j == q || j < 0 || j >= g.n_query) continue;
            visit(w, j);
        }
    }
}

// The LDS form of row blockIdx.x: a table of SLOTS (int32 key, Word) entries; the selection list (SLOTS / 2 keys and counts) is
// written OVER the table once the table sits in registers as keys.
template <int SLOTS, class P>
__device__ __forceinline__ void co_lds_form(const CoGraph &g, const P &p) {
    using Word = typename P::Word;
    constexpr int CAP = SLOTS / 2, PER = SLOTS / CO_THREADS;
    static_assert(SLOTS * (sizeof(Word) + 4) + 64 <= 64 * 1024 && CAP * 12 <= SLOTS * sizeof(Word) + SLOTS * 4, "the table within 64 KiB, the list over it");
    __shared__ uint64_t s_raw[SLOTS * (sizeof(Word) + 4) / 8];          // the table: words, then keys; later the list over them
    __shared__ int s_n;
    Word *s_hw = reinterpret_cast<Word *>(s_raw);
    int *s_hk = reinterpret_cast<int *>(s_hw + SLOTS);
    const int tid = threadIdx.x;
    const int64_t qi = blockIdx.x;
    const CoOut out = co_out<P>(g);
    const int64_t W = g.walk[qi];
    if (!(g.use_lds && co_in_lds<SLOTS>(W))) {                // (uniform) the dense form's row; without a row there it gets fillers
        if (g.groups == 0) co_fillers(out, qi, 0, tid);
        return;
    }
    const int64_t q = g.rows[qi];
    if (q < 0 || q >= g.n_query || W == 0) { co_fillers(out, qi, 0, tid); return; }
    for (int s = tid; s < SLOTS; s += CO_THREADS) { s_hk[s] = -1; s_hw[s] = 0; }
    if (tid == 0) s_n = 0;
    __syncthreads();
    co_two_hops(g, p, q, g.q_ptr[q], g.q_ptr[q + 1], tid, [&](Word w, int j) { atomicAdd(&s_hw[co_slot<SLOTS>(s_hk, j)], w); });
    __syncthreads();
    // the table to registers, then the list over it. A thread's 16 slots take the fewer registers of the two: a 32-bit word stays a
    // (key, word) pair and is scored when the list is written; a 64-bit word becomes the candidate's finished key (0: an empty slot)
    const typename P::Row row = p.row(g, q);
    uint64_t *s_key = s_raw;
    int *s_c = reinterpret_cast<int *>(s_raw + CAP);
    if constexpr (sizeof(Word) == 4) {
        int k[PER];
        Word w[PER];
#pragma unroll
        for (int i = 0; i < PER; ++i) { k[i] = s_hk[tid + CO_THREADS * i]; w[i] = s_hw[tid + CO_THREADS * i]; }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < PER; ++i)
            if (k[i] >= 0) {
                const int pos = atomicAdd(&s_n, 1);          // at most W <= CAP entries
                s_key[pos] = co_key(p.score(g, row, k[i], w[i], &s_c[pos]), k[i]);
            }
    } else {
        uint64_t key[PER];
        int c[PER];
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int k = s_hk[tid + CO_THREADS * i];
            key[i] = 0; c[i] = 0;
            if (k >= 0) key[i] = co_key(p.score(g, row, k, s_hw[tid + CO_THREADS * i], &c[i]), k);
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < PER; ++i)
            if (key[i]) {
                const int pos = atomicAdd(&s_n, 1);          // at most W <= CAP entries
                s_key[pos] = key[i];
                s_c[pos] = c[i];
            }
    }
    __syncthreads();
    const int n = s_n;
    co_sort(s_key, s_c, n, tid);
    co_emit(out, qi, s_key, s_c, n, tid);
}

// The dense form: pass 1 adds what the walks weigh to this workgroup's row of Words; pass 2 walks the entries again and claims each
// touched word with an exchange to 0, 16 middle nodes at a time, STEP entries a lane between two capacity checks.
template <int SLOTS, int STEP, int MAX_K, class P>
__device__ __forceinline__ void co_dense_form(const CoGraph &g, const P &p) {
    using Word = typename P::Word;
    Word *acc = static_cast<Word *>(g.acc) + (int64_t)blockIdx.x * g.n_query;
    const int tid = threadIdx.x, l = tid & 15;
    const CoOut out = co_out<P>(g);
    co_dense_rows<SLOTS / 2, STEP, MAX_K>(
        g.Q, [&](int64_t qi) { return !(g.use_lds && co_in_lds<SLOTS>(g.walk[qi])); },
        [&](int64_t qi, const CoList<SLOTS / 2, STEP, MAX_K> &list) {
            const int64_t q = g.rows[qi];
            if (q < 0 || q >= g.n_query) { co_fillers(out, qi, 0, tid); return; }
            list.reset(tid);
            const int64_t p0 = g.q_ptr[q], p1 = g.q_ptr[q + 1];
            const typename P::Row row = p.row(g, q);
            co_two_hops(g, p, q, p0, p1, tid, [&](Word w, int j) { P::touch(&acc[j], w); });
            __threadfence();
            __syncthreads();
            for (int64_t e0 = p0; e0 < p1; e0 += 16) {
                const int64_t e = e0 + (tid >> 4);
                int64_t f = 0, f1 = 0;
                if (e < p1) {
                    const int64_t u = g.q_nbr[e];
                    if (u >= 0 && u < g.n_other) { f = g.o_ptr[u]; f1 = g.o_ptr[u + 1]; }
                }
                for (;;) {
                    const uint64_t thr = list.threshold();
#pragma unroll
                    for (int r = 0; r < STEP; ++r) {
                        const int64_t ff = f + l + 16 * r;
                        if (ff >= f1) continue;
                        const int j = g.o_nbr[ff];
                        if (j == q || j < 0 || j >= g.n_query) continue;
                        const Word v = atomicExch(&acc[j], (Word)0);
                        if (v == 0) continue;                // untouched by now: another lane claimed it (a touched word is never 0)
                        int c;
                        const float score = p.score(g, row, j, v, &c);
                        list.offer(co_key(score, j), c, thr);
                    }
                    f += 16 * STEP;
                    const int more = __syncthreads_or(f < f1);
                    list.cut(out.K, tid);
                    if (!more) break;
                }
            }
            list.finish(out, qi, tid);
        });
}

}  // namespace elimrec
