// The per-row K-list of the chunked top-K kernels (knn.hip, audience.hip): the order of a list and its compaction. A row's list
// lives in LDS, CAP = K + KNN_SLACK (score, id) slots touched by one wave only; entries are appended while their score beats the
// row's threshold, and when the list is nearly full its wave ranks it by counting and keeps the K best in rank order.
#pragma once
#include "cosine.h"

namespace elimrec {

constexpr int KNN_SLACK = 32;

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

}  // namespace elimrec
