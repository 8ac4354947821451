// Insertion ranks by value: where would an item that is NOT in the catalogue land in a user's full ranking?
//
// rank_values_kernel: scores [B x I] (row stride lds >= I, masked items = -inf: the block rank_targets takes), values as CSR
// (val_ptr int64 [B + 1], vals float32), optionally one column per value to leave out (skip int32, -1 = none: the item's own
// catalogue entry when a catalogue item is folded in again). For value v of row b:
//     rank = #{ j in [0, I), j != skip : scores[b, j] >= v }
// the new item goes BEHIND every catalogue item of equal score (its id, num_items + q, is larger than every catalogue id), so the
// count is the 0-based position in the evaluator's (score descending, id ascending) order; -1 where v is not finite. A -inf score
// never counts (no finite v is <= it), -0.0 == 0.0 as IEEE compares them. NaN scores are outside the contract, as in rank.hip.
// Cost per row O(I log Q), not O(I Q): one workgroup per (row, segment of RV_SEG columns) sorts the row's values ascending in LDS
// (RV_VPP per pass: the bitonic network of co_select.h over 32-bit order-preserving keys, the value's list position beside it,
// non-finite values and the padding behind every finite one), streams its segment with 16-byte loads (the ragged end of a row
// element by element, columns >= I never read), and every score finds p = #{ sorted values <= score } by binary search and adds 1
// to the LDS integer bin p. Value k of the sorted list is beaten by the scores of the bins above k: a suffix sum over the bins
// gives every value its count, the epilogue takes the skip column's contribution off, and one global integer add per (workgroup,
// value) lands in the zeroed output. Integer sums commute: the result depends neither on the grid nor on arrival order; no
// floating-point atomics. Longer lists take further passes over the segment; a row without values is not read at all.
// Bytes: per pass B_listed x I x 4 read once, 4 (+ 4 with skip) bytes per value read and 4 written.
#include "common.h"

namespace elimrec {

constexpr int RV_THREADS = 256, RV_VEC = 4, RV_CHUNK = RV_THREADS * 4 * RV_VEC, RV_SEG = 4 * RV_CHUNK, RV_VPP = 1024;
// keys behind every finite key (whose largest is 0xFF7FFFFF): a non-finite value, then the padding, so that the n listed values
// are the sorted positions [0, n)
constexpr uint32_t RV_NONFINITE = 0xFFFFFFFEu, RV_PAD = 0xFFFFFFFFu;
static_assert(RV_VPP == 4 * RV_THREADS, "the suffix sum gives every thread four consecutive bins");

// order-preserving image of a finite fp32 (co_key's high word); -0.0 arrives as +0.0
__device__ __forceinline__ uint32_t rv_key(float v) {
    const uint32_t bits = __float_as_uint(v);
    return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}
__device__ __forceinline__ float rv_key_value(uint32_t key) {
    return __uint_as_float((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key);
}

__device__ __forceinline__ int64_t rv_ptr(const int64_t *__restrict__ ptr, int64_t b, int64_t n) {
    const int64_t p = ptr[b];
    return p < 0 ? 0 : (p > n ? n : p);                         // (a pointer outside the list reads nothing)
}

// the whole workgroup sorts key[0, m) ascending (pos beside it), m a power of two in [64, RV_VPP]: co_sort's network. Ends with a barrier.
__device__ __forceinline__ void rv_sort(uint32_t *key, int *pos, int m, int tid) {
    for (int k = 2; k <= m; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < m; i += RV_THREADS) {
                const int l = i ^ j;
                if (l > i) {
                    const uint32_t x = key[i], y = key[l];
                    if (((i & k) == 0) ? x > y : x < y) {
                        key[i] = y; key[l] = x;
                        const int px = pos[i]; pos[i] = pos[l]; pos[l] = px;
                    }
                }
            }
            __syncthreads();
        }
}

// p = #{ k in [0, n) : w[k] <= s } for ascending w (a -inf score gives 0, NaN gives 0)
__device__ __forceinline__ int rv_upper(const float *w, int n, float s) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (w[mid] <= s) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// VEC: the block's base is 16-byte aligned and lds % 4 == 0, so every full float4 of a row is one 16-byte load
template <bool VEC>
__global__ __launch_bounds__(RV_THREADS) void rank_values_kernel(const float *__restrict__ scores, int64_t I, int64_t lds, int n_seg,
                                                                 const int64_t *__restrict__ vptr, const float *__restrict__ vals,
                                                                 const int32_t *__restrict__ skip, int64_t n_vals,
                                                                 int32_t *__restrict__ rank) {
    __shared__ uint32_t s_key[RV_VPP];
    __shared__ int s_pos[RV_VPP];
    __shared__ float s_w[RV_VPP];
    __shared__ int s_bin[RV_VPP + 1];
    __shared__ int s_wave[RV_THREADS / 64];
    __shared__ int s_fin;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t b = blockIdx.x / n_seg;
    const int seg = (int)(blockIdx.x % n_seg);
    const int64_t v_begin = rv_ptr(vptr, b, n_vals), v_end = rv_ptr(vptr, b + 1, n_vals);
    if (v_end <= v_begin) return;                               // (workgroup-uniform: no values, no read)
    const float *__restrict__ row = scores + b * lds;
    const int64_t seg0 = (int64_t)seg * RV_SEG;
    const int64_t seg1 = seg0 + RV_SEG < I ? seg0 + RV_SEG : I;
    const float NEG = -__builtin_huge_valf();

    for (int64_t v0 = v_begin; v0 < v_end; v0 += RV_VPP) {
        const int n = (int)(v_end - v0 < RV_VPP ? v_end - v0 : RV_VPP);
        int m = 64;
        while (m < n) m <<= 1;
        __syncthreads();                                        // (the previous pass has read its LDS)
        if (tid == 0) s_fin = 0;
        for (int i = tid; i <= RV_VPP; i += RV_THREADS) s_bin[i] = 0;
        __syncthreads();
        int fin = 0;
        for (int i = tid; i < m; i += RV_THREADS) {
            uint32_t key = RV_PAD;
            if (i < n) {
                key = RV_NONFINITE;
                float v = vals[v0 + i];
                if (v == 0.f) v = 0.f;                          // -0.0 -> +0.0: one key for the two zeros
                if (v - v == 0.f) { key = rv_key(v); fin += 1; }    // finite (inf - inf and NaN - NaN are NaN)
            }
            s_key[i] = key;
            s_pos[i] = i;
        }
        if (fin) atomicAdd(&s_fin, fin);
        __syncthreads();
        rv_sort(s_key, s_pos, m, tid);
        const int n_fin = s_fin;                                // the finite values are s_key[0, n_fin), ascending
        for (int i = tid; i < n_fin; i += RV_THREADS) s_w[i] = rv_key_value(s_key[i]);
        __syncthreads();

        if (n_fin) {                                            // (workgroup-uniform)
            for (int64_t c0 = seg0; c0 < seg1; c0 += RV_CHUNK) {
                float x[RV_VEC][4];
#pragma unroll
                for (int v = 0; v < RV_VEC; ++v) {
                    const int64_t j = c0 + (int64_t)(v * RV_THREADS + tid) * 4;
                    if (VEC && j + 4 <= I) {
                        const float4 q = *reinterpret_cast<const float4 *>(row + j);
                        x[v][0] = q.x; x[v][1] = q.y; x[v][2] = q.z; x[v][3] = q.w;
                    } else {
#pragma unroll
                        for (int c = 0; c < 4; ++c) x[v][c] = j + c < I ? row[j + c] : NEG;
                    }
                }
#pragma unroll
                for (int v = 0; v < RV_VEC; ++v)
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const int p = rv_upper(s_w, n_fin, x[v][c]);
                        if (p) atomicAdd(&s_bin[p], 1);         // bin 0 (a score below every value, -inf, the padding) counts for nobody
                    }
            }
        }
        __syncthreads();

        // suffix sum: sorted value k is beaten by the scores of the bins k + 1 .. n_fin. Thread t owns the bins 4 t + 1 .. 4 t + 4
        // (beyond n_fin they are 0): own[i] = bins 4 t + 1 + i .. 4 t + 4, above = the sum of the later threads' bins.
        int own[4];
        {
            int run = 0;
#pragma unroll
            for (int i = 3; i >= 0; --i) { run += s_bin[4 * tid + 1 + i]; own[i] = run; }
        }
        int incl = own[0];                                      // inclusive suffix sum over the lanes of the wave
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int o = __shfl_down(incl, off, 64);
            if (lane + off < 64) incl += o;
        }
        if (lane == 0) s_wave[wave] = incl;
        __syncthreads();
        int above = incl - own[0];
        for (int w = wave + 1; w < RV_THREADS / 64; ++w) above += s_wave[w];

#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int k = 4 * tid + i;
            if (k >= n) continue;
            const int64_t slot = v0 + s_pos[k];                 // s_pos[k] < n: the padding's positions lie at k >= n
            if (k >= n_fin) {
                if (seg == 0) rank[slot] = -1;                  // not finite; nobody adds to this slot: one plain store
                continue;
            }
            int cnt = above + own[i];
            if (skip) {
                const int64_t c = skip[slot];
                if (c >= seg0 && c < seg1 && row[c] >= s_w[k]) cnt -= 1;    // this segment counted the item's own column
            }
            if (cnt) atomicAdd(&rank[slot], cnt);
        }
    }
}

}  // namespace elimrec

using namespace elimrec;

extern "C" int elimrec_rank_values_segment(void) { return RV_SEG; }
extern "C" int elimrec_rank_values_per_pass(void) { return RV_VPP; }

extern "C" int elimrec_rank_values(const float *d_scores, int64_t B, int64_t I, int64_t lds, const int64_t *d_val_ptr,
                                   const float *d_vals, const int32_t *d_skip, int64_t n_vals, int32_t *d_rank, void *stream) {
    ELIMREC_REQUIRE(B >= 0 && n_vals >= 0, "rank_values: need B >= 0, n_vals >= 0");
    if (B == 0 || n_vals == 0) return 0;
    ELIMREC_REQUIRE(d_scores && d_val_ptr && d_vals && d_rank, "rank_values: null pointer");
    ELIMREC_REQUIRE(I >= 1 && I < (int64_t)INT32_MAX - RV_SEG, "rank_values: the catalogue must hold 1 .. 2^31 - %d items", RV_SEG + 1);
    ELIMREC_REQUIRE(lds >= I, "rank_values: lds < I");
    const int64_t n_seg = (I + RV_SEG - 1) / RV_SEG;
    ELIMREC_REQUIRE(B * n_seg < (int64_t)INT32_MAX, "rank_values: %lld rows x %lld segments exceed one launch", (long long)B,
                    (long long)n_seg);
    hipStream_t s = (hipStream_t)stream;
    int rc = check_hip(hipMemsetAsync(d_rank, 0, (size_t)n_vals * sizeof(int32_t), s), "rank_values (zero)");
    if (rc) return rc;
    const dim3 grid((unsigned)(B * n_seg));
    if (((uintptr_t)d_scores & 15) == 0 && lds % 4 == 0)
        hipLaunchKernelGGL(rank_values_kernel<true>, grid, dim3(RV_THREADS), 0, s, d_scores, I, lds, (int)n_seg, d_val_ptr, d_vals,
                           d_skip, n_vals, d_rank);
    else
        hipLaunchKernelGGL(rank_values_kernel<false>, grid, dim3(RV_THREADS), 0, s, d_scores, I, lds, (int)n_seg, d_val_ptr, d_vals,
                           d_skip, n_vals, d_rank);
    ELIMREC_LAUNCH_CHECK("rank_values");
    return 0;
}
