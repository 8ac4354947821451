// The selection cooccur.hip and vote.hip share. Candidates arrive in no order, so a candidate is ONE 64-bit key: the order-preserving
// image of the fp32 score in the high word, ~id in the low word -- a larger key ranks earlier under (score descending, id ascending),
// and keys are distinct because ids are. The keys (an int32 count beside each) are gathered into a list in LDS and sorted by a bitonic
// network over the next power of two, the empty key 0 behind every candidate. One workgroup of CO_THREADS threads.
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

}  // namespace elimrec
