// The two-form top-K design cooccur.hip, walk.hip and vote.hip share: per row (a query row of a graph, a user) the K ids with the largest
// integer-exact score, gathered from candidates that arrive in no order. One workgroup of CO_THREADS = 256 threads handles a row, and a
// size the host knows too (W(q) of a walk, V(u) of a vote) picks one of two forms:
//   LDS form   (size <= SLOTS / 2): an open-addressing table of SLOTS entries in LDS, SLOTS a power of two, home slot id % SLOTS,
//              linear probing (co_slot). The size bounds the entries, so the load factor is at most 0.5 whatever the ids are and a
//              free slot always exists. Insertion is an integer compare-and-swap on the key and integer adds on the entry's words.
//   dense form (any size): a fixed number of workgroups (co_groups: at most GROUPS) loop over the rows that need it (co_dense_rows);
//              each owns one accumulator row of n entries in the workspace, ZERO when the call starts. A family's pass 1 adds with
//              integer atomics, its pass 2 walks the same entries again and claims each touched word with an exchange to 0: the lane
//              that gets a word != 0 offers the candidate, and the row is clean again for the next query -- EVERY CALL LEAVES THE
//              WORKSPACE ZERO, so one zeroed buffer serves call after call, and the three families in turn.
//
// Selection. Candidates do not arrive in ascending id, so knn_select.h's threshold rule does not hold here. A candidate is ONE 64-bit
// key: the order-preserving image of the fp32 score in the high word, ~id in the low word -- a larger key ranks earlier under (score
// descending, id ascending), and keys are distinct because ids are. The keys (an int32 count beside each) are gathered into a list of
// CAP = SLOTS / 2 slots in LDS -- the LDS form's table holds at most that many -- and sorted by a bitonic network over the next power
// of two, the empty key 0 behind every candidate (co_sort). The dense form (CoList) compares the FULL key against the K-th kept key: a
// key at or below it can never be listed; when the list could overflow within the next STEP claims of every lane it is sorted and cut
// to the K best, which raises that key. A row's outputs therefore depend bit for bit on the family's inputs, the row and K -- not on
// the arrival order, the form, the number of rows, the row's place among them or the grid. No floating-point atomics.
// Fillers behind the listed ids: -1 / -inf / 0 (co_fillers).
#pragma once
#include "common.h"

namespace elimrec {

constexpr int CO_THREADS = 256;

// (score, id) as one key: a larger key ranks earlier; 0 is no candidate (the image of a NaN no score takes)
__device__ __forceinline__ uint64_t co_key(float score, int id) {
    const uint32_t bits = __float_as_uint(score);
    const uint32_t hi = (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
    return ((uint64_t)hi << 32) | (uint32_t)~(uint32_t)id;
}
__device__ __forceinline__ float co_key_score(uint64_t key) {
    const uint32_t hi = (uint32_t)(key >> 32);
    return __uint_as_float((hi & 0x80000000u) ? (hi ^ 0x80000000u) : ~hi);
}
__device__ __forceinline__ int co_key_id(uint64_t key) { return (int)~(uint32_t)key; }

// the whole workgroup sorts key[0, n) (c beside it) descending: empty keys over [n, m), m the next power of two, a bitonic network
// over m. Ends with a barrier. The list holds at least m slots (a power of two of at least 64 slots that is >= n).
__device__ __forceinline__ void co_sort(uint64_t *key, int *c, int n, int tid) {
    int m = 64;
    while (m < n) m <<= 1;
    for (int i = n + tid; i < m; i += CO_THREADS) { key[i] = 0; c[i] = 0; }
    __syncthreads();
    for (int k = 2; k <= m; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < m; i += CO_THREADS) {
                const int l = i ^ j;
                if (l > i) {
                    const uint64_t x = key[i], y = key[l];
                    if (((i & k) == 0) ? x < y : x > y) {
                        key[i] = y; key[l] = x;
                        const int cx = c[i]; c[i] = c[l]; c[l] = cx;
                    }
                }
            }
            __syncthreads();
        }
}

// the outputs of a call: [rows x K] each; val and cnt may be null
struct CoOut { int K; int32_t *idx; float *val; int32_t *cnt; };

__device__ __forceinline__ void co_fillers(const CoOut &o, int64_t row, int from, int tid) {
    for (int k = from + tid; k < o.K; k += CO_THREADS) {
        o.idx[row * o.K + k] = -1;
        if (o.val) o.val[row * o.K + k] = -__builtin_huge_valf();
        if (o.cnt) o.cnt[row * o.K + k] = 0;
    }
}

// the sorted list's K best to row `row` of the outputs, fillers behind them
__device__ __forceinline__ void co_emit(const CoOut &o, int64_t row, const uint64_t *key, const int *c, int n, int tid) {
    const int kept = n < o.K ? n : o.K;
    for (int k = tid; k < kept; k += CO_THREADS) {
        o.idx[row * o.K + k] = co_key_id(key[k]);
        if (o.val) o.val[row * o.K + k] = co_key_score(key[k]);
        if (o.cnt) o.cnt[row * o.K + k] = c[k];
    }
    co_fillers(o, row, kept, tid);
}

// the slot of id j in the LDS form's table of SLOTS keys (-1: free), entered when new: the row's size bounds the distinct keys by
// SLOTS / 2, so a free slot always exists
template <int SLOTS>
__device__ __forceinline__ int co_slot(int *hk, int j) {
    static_assert(SLOTS > 0 && (SLOTS & (SLOTS - 1)) == 0, "the table's slot count is a power of two");
    int s = j & (SLOTS - 1);
    for (;;) {
        const int prev = atomicCAS(&hk[s], -1, j);
        if (prev == -1 || prev == j) return s;
        s = (s + 1) & (SLOTS - 1);
    }
}

// The dense form's selection list of CAP slots in LDS (co_dense_rows places it); STEP: candidates a lane offers between two cuts
template <int CAP, int STEP, int MAX_K>
struct CoList {
    static_assert(CAP >= 2 * CO_THREADS * STEP && CAP - CO_THREADS * STEP >= MAX_K, "the dense form's list");
    uint64_t *key; int *c;                                   // [CAP] the keys, the count beside each
    uint64_t *thr;                                           // the K-th kept key once K are kept, else 0
    int *n;

    // a new row; the barrier behind the family's pass 1 publishes it
    __device__ __forceinline__ void reset(int tid) const { if (tid == 0) { *n = 0; *thr = 0; } }
    __device__ __forceinline__ uint64_t threshold() const { return *thr; }
    // n <= CAP - CO_THREADS * STEP after a cut, and at most CO_THREADS * STEP offers follow before the next one
    __device__ __forceinline__ void offer(uint64_t k, int cnt, uint64_t threshold) const {
        if (k > threshold) {
            const int pos = atomicAdd(n, 1);
            key[pos] = k;
            c[pos] = cnt;
        }
    }
    // (the whole workgroup) could the next STEP offers of every lane overflow the list? then sort it, cut it to the K best and raise
    // the threshold to the K-th
    __device__ __forceinline__ void cut(int K, int tid) const {
        if (__syncthreads_or(*n > CAP - CO_THREADS * STEP)) {
            const int m = *n;
            co_sort(key, c, m, tid);
            if (tid == 0 && m >= K) { *n = K; *thr = key[K - 1]; }
            __syncthreads();
        }
    }
    // (the whole workgroup) the row is claimed: sort what is kept and write row `row` of the outputs
    __device__ __forceinline__ void finish(const CoOut &o, int64_t row, int tid) const {
        __syncthreads();
        const int m = *n;
        co_sort(key, c, m, tid);
        co_emit(o, row, key, c, m, tid);
        __syncthreads();
    }
};

// The dense form's row scheduler: workgroup b of G serves the positions p = b (mod G) of [0, n_pos) for which is_dense(p) holds, 256
// positions' flags at a time; row(p, list) runs with the whole workgroup, one position after the other.
template <int CAP, int STEP, int MAX_K, class IsDense, class Row>
__device__ __forceinline__ void co_dense_rows(int64_t n_pos, IsDense is_dense, Row row) {
    __shared__ uint64_t s_key[CAP];
    __shared__ int s_c[CAP];
    __shared__ uint64_t s_thr;
    __shared__ int s_n;
    __shared__ int s_flag[CO_THREADS];
    const CoList<CAP, STEP, MAX_K> list = {s_key, s_c, &s_thr, &s_n};
    const int tid = threadIdx.x;
    const int64_t G = gridDim.x, b = blockIdx.x;
    for (int64_t base = 0; base * G < n_pos; base += CO_THREADS) {
        const int64_t mine = (base + tid) * G + b;
        s_flag[tid] = mine < n_pos && is_dense(mine);
        __syncthreads();
        for (int i = 0; i < CO_THREADS; ++i)
            if (s_flag[i]) row((base + i) * G + b, list);   // (uniform)
        __syncthreads();
    }
}

// ---- the host side of the three entry points

// workgroups of the dense form, and the bytes of their accumulator rows of n entries of entry_bytes each
static inline int64_t co_groups(int64_t n_dense_rows, int max_groups) {
    return n_dense_rows < max_groups ? (n_dense_rows < 0 ? 0 : n_dense_rows) : max_groups;
}
static inline size_t co_workspace(int64_t n_dense_rows, int max_groups, int64_t n, size_t entry_bytes) {
    return align_up((size_t)co_groups(n_dense_rows, max_groups) * (size_t)n * entry_bytes, 16);
}

// K and use_lds of a call, checked first; then n_dense_rows, once the call's n_rows rows are checked (`rows`: their name in the
// header, "Q" or "B")
static inline int co_check_forms(const char *who, int K, int max_k, int use_lds) {
    ELIMREC_REQUIRE(K >= 1 && K <= max_k, "%s: 1 <= K <= %d, got %d", who, max_k, K);
    ELIMREC_REQUIRE(use_lds == 0 || use_lds == 1, "%s: use_lds is 0 or 1, got %d", who, use_lds);
    return 0;
}
static inline int co_check_dense_rows(const char *who, int64_t n_dense_rows, int64_t n_rows, const char *rows) {
    ELIMREC_REQUIRE(n_dense_rows >= 0 && n_dense_rows <= n_rows, "%s: 0 <= n_dense_rows <= %s, got %lld", who, rows, (long long)n_dense_rows);
    return 0;
}
// the dense form's workspace: `need` bytes (co_workspace), 16-byte aligned, unless no row or no entry needs it
static inline int co_check_workspace(const char *who, int64_t n_dense_rows, int64_t n, size_t need, const void *workspace, size_t workspace_bytes) {
    ELIMREC_REQUIRE(n_dense_rows == 0 || n == 0 || (workspace && workspace_bytes >= need && reinterpret_cast<uintptr_t>(workspace) % 16 == 0),
                    "%s: the workspace needs %zu bytes, 16-byte aligned (got %zu)", who, need, workspace_bytes);
    return 0;
}
// the LDS form over every row (rows that are not its own return at once), then the dense form's workgroups; the two names are what
// a failed launch reports
template <class Args>
static int co_launch_forms(void (*lds_kernel)(Args), const char *lds_name, void (*dense_kernel)(Args), const char *dense_name, int64_t n_rows,
                           int use_lds, int groups, const Args &a, hipStream_t s) {
    if (use_lds) {
        hipLaunchKernelGGL(lds_kernel, dim3((unsigned)n_rows), dim3(CO_THREADS), 0, s, a);
        ELIMREC_LAUNCH_CHECK(lds_name);
    }
    if (groups > 0) {
        hipLaunchKernelGGL(dense_kernel, dim3((unsigned)groups), dim3(CO_THREADS), 0, s, a);
        ELIMREC_LAUNCH_CHECK(dense_name);
    }
    return 0;
}

}  // namespace elimrec
