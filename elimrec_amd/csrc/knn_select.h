// What the chunked top-K kernels share (knn.hip: cosine_topk, audience.hip: audience_topk): everything but the multiply phase.
// Both run a grid of (query tiles x candidate chunks of KNN_CHUNK), keep a K-list per query row while a chunk streams by, leave
// [Q][chunks x K] (score, id) pairs in the workspace and end in elimrec_topk_merge.
//
// The K-list (device part): a row's list lives in LDS, CAP = K + KNN_SLACK (score, id) slots touched by one wave only. A wave owns
// 16 rows; after a 16-candidate tile lane (li, kq) holds the scores of candidate li against rows 4 kq .. 4 kq + 3. A score that is
// > the row's threshold (-inf until K are kept, then the K-th best kept score; candidates arrive in ascending id order, so an equal
// score later in the chunk loses the tie and is rightly dropped) is checked against the exclusions -- the caller's own clause, then
// a linear scan of the row's CSR list: only scores that beat the threshold get there -- and appended with an LDS integer add (a tile
// appends at most 16 entries per row). A row that holds more than CAP - 16 entries is ranked by its wave by (score descending, id
// ascending) by counting and cut to the K best in rank order, which raises the threshold; the order of arrival never reaches the
// result. At the end of the chunk every row is cut once more and written out, fillers (-inf, -1) behind its entries.
//
// The front end (host part): the chunk count, the workspace and its two halves, the requirements both entry points make in the
// same words, the all-fillers result, the launch and the closing merge.
#pragma once
#include "cosine.h"

namespace elimrec {

constexpr int KNN_CHUNK = 4096, KNN_TILE = 64, KNN_MAXK = 256, KNN_SMALLK = 64;   // K <= KNN_SMALLK: 4 waves a tile, else 1
constexpr int KNN_SLACK = 32;

// bytes of the lists of `rows` query rows: scores and ids [rows][K + KNN_SLACK], counts and thresholds [rows]
constexpr size_t knn_list_bytes(size_t rows, size_t K) { return rows * (K + KNN_SLACK) * 8 + rows * 8; }
// list entries a lane holds while its wave ranks a list: W = 4 waves serve K <= KNN_SMALLK, one wave K <= KNN_MAXK
constexpr int knn_list_regs(int W) { return ((W == 4 ? KNN_SMALLK : KNN_MAXK) + KNN_SLACK + 63) / 64; }

// ---- device
struct KnnLists { float *lv; int *li; int *cnt; float *thr; int cap; float *end; };   // the 16 lists of one wave; end: the first float behind all lists

// the wave's views of the lists carved from `base` for the `rows` query rows of the workgroup (knn_list_bytes of them)
__device__ __forceinline__ KnnLists knn_lists(float *base, int rows, int K, int wave) {
    const int cap = K + KNN_SLACK;
    int *li = (int *)(base + rows * cap);
    int *cnt = li + rows * cap;
    float *thr = (float *)(cnt + rows);
    return KnnLists{base + wave * 16 * cap, li + wave * 16 * cap, cnt + wave * 16, thr + wave * 16, cap, thr + rows};
}

// a row's first threshold: everything is kept until K are; a row that is no query keeps nothing
__device__ __forceinline__ float knn_thr0(bool valid) { return valid ? -__builtin_huge_valf() : __builtin_huge_valf(); }

__device__ __forceinline__ bool knn_before(float va, int ia, float vb, int ib) {   // a ranks before b (elimrec_topk_merge's order)
    return va > vb || (va == vb && ia < ib);
}

// the whole wave ranks the n entries of one list, leaves the K best in rank order, the new length and threshold
template <int E>
__device__ __forceinline__ void knn_compact(float *lv, int *li_, int *cnt, float *thr, int K, int lane) {
    const int n = *cnt;
    float v[E];
    int id[E], rk[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int c = lane + 64 * e;
        v[e] = c < n ? lv[c] : 0.f;
        id[e] = c < n ? li_[c] : 0;
        rk[e] = 0;
    }
    for (int j = 0; j < n; ++j) {
        const float vj = lv[j];
        const int ij = li_[j];
#pragma unroll
        for (int e = 0; e < E; ++e) rk[e] += knn_before(vj, ij, v[e], id[e]) ? 1 : 0;
    }
    wave_lds_sync();                                        // every lane has read the list
#pragma unroll
    for (int e = 0; e < E; ++e)
        if (lane + 64 * e < n && rk[e] < K) {
            lv[rk[e]] = v[e];
            li_[rk[e]] = id[e];
            if (rk[e] == K - 1) *thr = v[e];
        }
    if (lane == 0) *cnt = n < K ? n : K;
    wave_lds_sync();
}

// lane < 16 empties list `lane` of its wave; valid: that row is a query
__device__ __forceinline__ void knn_list_reset(const KnnLists &l, int lane, bool valid) {
    l.cnt[lane] = 0;
    l.thr[lane] = knn_thr0(valid);
}

// The offer step, after the caller's wave-uniform `if (__ballot(any) == 0ull) continue;`: the lane offers its scores s[4] of
// candidate `cand` (pass[r]: s[r] beat thr[r]) to rows 4 kq + r of the wave, queries q0 + 4 kq + r of the exclusion CSR; the lists
// that got nearly full are cut and thr[4] follows. keep0: the caller's own exclusion clause in terms of r (`true`: none -- the
// clause folds away). E = knn_list_regs(W). (A macro for ELIMREC_LOAD_ROW4's reason, cosine.h: the kernels' register budgets --
// audience_chunk_kernel<64, 1, *> sits at 256 VGPRs -- are pinned to these statements standing in place.)
#define KNN_OFFER(l, E, K, lane, kq, q0, cand, s, pass, thr, excl_ptr, excl_ids, keep0)                              \
    do {                                                                                                             \
        _Pragma("unroll") for (int r = 0; r < 4; ++r) {                                                              \
            if (!pass[r]) continue;                                                                                  \
            bool keep = (keep0);                                                                                     \
            if (keep && (excl_ptr)) {                                                                                \
                const int64_t q = (q0) + 4 * (kq) + r;                                                               \
                const int64_t e1 = (excl_ptr)[q + 1];                                                                \
                for (int64_t e = (excl_ptr)[q]; e < e1 && keep; ++e) keep = (excl_ids)[e] != (int)(cand);            \
            }                                                                                                        \
            if (keep) {                                                                                              \
                const int row = 4 * (kq) + r;                                                                        \
                const int pos = atomicAdd(&(l).cnt[row], 1);     /* <= cap - 16 before the tile, at most 16 adds per row and tile */ \
                (l).lv[row * (l).cap + pos] = s[r];                                                                  \
                (l).li[row * (l).cap + pos] = (int)(cand);                                                           \
            }                                                                                                        \
        }                                                                                                            \
        wave_lds_sync();                                                                                             \
        unsigned long long full = __ballot((lane) < 16 && (l).cnt[(lane) & 15] > (l).cap - 16) & 0xffffull;          \
        if (full) {                                              /* wave-uniform */                                  \
            while (full) {                                                                                           \
                const int row = __builtin_ctzll(full);                                                               \
                full &= full - 1;                                                                                    \
                knn_compact<E>((l).lv + row * (l).cap, (l).li + row * (l).cap, &(l).cnt[row], &(l).thr[row], K, lane); \
            }                                                                                                        \
            _Pragma("unroll") for (int r = 0; r < 4; ++r) thr[r] = (l).thr[4 * (kq) + r];                            \
        }                                                                                                            \
    } while (0)

// The flush: the chunk's K best of every query row q0 + row < Q of this wave, in rank order, fillers behind them, at
// (q * n_chunks + chunk) * K of the workspace.
#define KNN_FLUSH(l, E, K, lane, q0, Q, n_chunks, chunk, ws_val, ws_idx)                                             \
    for (int row = 0; row < 16; ++row) {                                                                             \
        const int64_t q = (q0) + row;                                                                                \
        if (q >= (Q)) break;                                     /* wave-uniform */                                  \
        knn_compact<E>((l).lv + row * (l).cap, (l).li + row * (l).cap, &(l).cnt[row], &(l).thr[row], K, lane);       \
        const int n = (l).cnt[row];                                                                                  \
        const int64_t o = (q * (n_chunks) + (chunk)) * (K);                                                          \
        for (int k = (lane); k < (K); k += 64) {                                                                     \
            (ws_val)[o + k] = k < n ? (l).lv[row * (l).cap + k] : -__builtin_huge_valf();                            \
            (ws_idx)[o + k] = k < n ? (l).li[row * (l).cap + k] : -1;                                                \
        }                                                                                                            \
    }

// ---- host: the front end of elimrec_cosine_topk / elimrec_audience_topk; `who` is the entry point's name in every message
struct KnnWorkspace { int64_t n_chunks; float *val; int32_t *idx; };   // [Q][n_chunks x K] scores, then ids from a 16-byte boundary

inline int64_t knn_chunks(int64_t n) { return (n + KNN_CHUNK - 1) / KNN_CHUNK; }

inline size_t knn_workspace_bytes(int64_t Q, int64_t n, int K) {
    if (Q <= 0 || n <= 0 || K <= 0) return 16;
    const size_t pairs = (size_t)Q * (size_t)knn_chunks(n) * (size_t)K;
    return align_up(pairs * 4, 16) + align_up(pairs * 4, 16);
}

inline int knn_check_k(const char *who, int K) {
    ELIMREC_REQUIRE(K >= 1 && K <= KNN_MAXK, "%s: 1 <= K <= %d, got %d", who, KNN_MAXK, K);
    return 0;
}

// once the entry point has its own pointers: the exclusion CSR's two arrays and the workspace for n candidates
inline int knn_check_buffers(const char *who, const void *excl_ptr, const void *excl_ids, const void *ws, size_t ws_bytes, int64_t Q,
                             int64_t n, int K) {
    ELIMREC_REQUIRE((excl_ptr == nullptr) == (excl_ids == nullptr), "%s: the exclusion CSR needs both arrays or neither", who);
    ELIMREC_REQUIRE(((uintptr_t)ws & 15) == 0, "%s: the workspace must be 16-byte aligned", who);
    const size_t need = knn_workspace_bytes(Q, n, K);
    ELIMREC_REQUIRE(ws_bytes >= need, "%s: workspace too small (%zu < %zu bytes)", who, ws_bytes, need);
    return 0;
}

// nothing to rank: every list is fillers
inline int knn_fill_empty(const char *who, int32_t *d_idx, float *d_val, int64_t Q, int K, hipStream_t s) {
    hipError_t e = hipMemsetAsync(d_idx, 0xff, (size_t)Q * K * sizeof(int32_t), s);
    if (e == hipSuccess && d_val) e = hipMemsetD32Async((hipDeviceptr_t)d_val, (int)0xff800000u /* -inf */, (size_t)Q * K, s);
    if (e == hipSuccess) return 0;
    set_error("%s (fill): %s", who, hipGetErrorString(e));
    return (int)e;
}

// the launch's and the merge's limits, then the workspace's halves; queries: the entry point's noun for its query rows
inline int knn_carve(const char *who, const char *queries, int64_t Q, int64_t n, int K, void *ws, KnnWorkspace *out) {
    const int64_t n_chunks = knn_chunks(n);
    ELIMREC_REQUIRE(n_chunks <= 65535, "%s: %lld chunks exceed one launch", who, (long long)n_chunks);
    ELIMREC_REQUIRE(Q < (int64_t)INT32_MAX && n_chunks * K < (int64_t)INT32_MAX, "%s: too many %s or chunks for the merge", who, queries);
    const size_t pairs = (size_t)Q * (size_t)n_chunks * (size_t)K;
    *out = KnnWorkspace{n_chunks, (float *)ws, (int32_t *)((char *)ws + align_up(pairs * 4, 16))};
    return 0;
}

// one chunk kernel over (n_tiles x n_chunks) workgroups of `threads`. The LDS limit is raised at every launch that needs it: the
// bytes grow with the run-time K, so a limit latched at the first call (dispatch.h's allow_lds) would be too small for a later one.
template <class Args>
int knn_launch_chunks(const char *who, void (*kernel)(Args), const Args &a, int64_t n_tiles, int64_t n_chunks, int threads, size_t lds,
                      hipStream_t s) {
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) {
            set_error("%s (LDS): %s", who, hipGetErrorString(e));
            return (int)e;
        }
    }
    hipLaunchKernelGGL(kernel, dim3((unsigned)n_tiles, (unsigned)n_chunks), dim3(threads), lds, s, a);
    ELIMREC_LAUNCH_CHECK(who);
    return 0;
}

inline int knn_merge(const KnnWorkspace &w, int64_t Q, int K, int32_t *d_idx, float *d_val, void *stream) {
    return elimrec_topk_merge(w.val, w.idx, (int)Q, (int)(w.n_chunks * K), K, d_idx, d_val, stream);
}

}  // namespace elimrec
