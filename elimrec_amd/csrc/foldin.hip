// Fold-in of new users: a weighted sum of table rows over ragged per-request lists, float64 all the way to one rounding.
//
// segment_row_sum_kernel: table float32 [n_rows x C] (row stride ld, 16-byte aligned rows), the lists as CSR (ptr int64 [Q + 1],
// rows int32, weights float32 beside them), out float32 [Q x C]:
//     out[q, :] = sum_{j in [ptr[q], ptr[q + 1])} weights[j] * table[row_offset + rows[j], :]
// One workgroup of four waves per segment. Every lane owns one float4 column group, a wave covers FI_PASS = 256 columns (one
// 1-KiB wave-instruction per gathered row at C = 256) and a wider C takes further column passes. The segment is cut into chunks
// of FI_CHUNK = 64 entries, chunk c belongs to wave c % 4: the wave reads the chunk's ids and weights with ONE coalesced load
// each (lane l holds entry l), broadcasts them lane by lane (v_readlane: the loop counter is wave-uniform) and keeps FI_FLIGHT
// row gathers in flight; each product w * x is formed in float64 (exact: 24 x 24 bits) and added in entry order. The four waves'
// float64 partial sums meet in LDS and are added in wave order, the result is rounded to float32 once. No atomics, no workspace:
// a segment's bits depend on its own entries, C and the table alone -- not on Q, not on its neighbours in the batch, not on the
// grid. An empty segment writes zeros. An id outside [0, n_rows - row_offset) is rejected by the Python wrappers on the host;
// the kernel gives such an entry weight zero and reads row 0 of the window instead (nothing outside the table is ever read).
// Bytes: per entry one row of 4 C bytes gathered (plus 8 bytes of id and weight per column pass), 4 C bytes written per segment.
#include "common.h"

namespace elimrec {

constexpr int FI_THREADS = 256, FI_WAVES = FI_THREADS / 64, FI_CHUNK = 64, FI_PASS = 64 * 4, FI_FLIGHT = 8;
static_assert(FI_CHUNK == 64, "lane l of the owning wave holds entry l of a chunk");
static_assert(FI_CHUNK % FI_FLIGHT == 0, "a chunk is whole groups of gathers");

__device__ __forceinline__ int64_t fi_ptr(const int64_t *__restrict__ ptr, int64_t q, int64_t n) {
    const int64_t p = ptr[q];
    return p < 0 ? 0 : (p > n ? n : p);                         // (a pointer outside the list reads nothing)
}

__global__ __launch_bounds__(FI_THREADS) void segment_row_sum_kernel(const float *__restrict__ table, int64_t ld, int64_t n_window,
                                                                     int C, const int64_t *__restrict__ ptr,
                                                                     const int32_t *__restrict__ rows,
                                                                     const float *__restrict__ weights, int64_t n_entries,
                                                                     float *__restrict__ out, int64_t ldo) {
    __shared__ double s_part[FI_WAVES][FI_PASS];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t q = blockIdx.x;
    const int64_t begin = fi_ptr(ptr, q, n_entries), end = fi_ptr(ptr, q + 1, n_entries);
    const int64_t n = end > begin ? end - begin : 0;            // (workgroup-uniform)

    for (int p0 = 0; p0 < C; p0 += FI_PASS) {
        const int col = p0 + lane * 4;
        const bool live = col < C;                              // (C % 4 == 0: a lane's float4 is inside the row or outside it)
        const float *__restrict__ base = table + col;
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        for (int64_t c0 = (int64_t)wave * FI_CHUNK; c0 < n; c0 += (int64_t)FI_WAVES * FI_CHUNK) {
            const int cnt = (int)(n - c0 < FI_CHUNK ? n - c0 : FI_CHUNK);
            int my_row = 0;
            float my_w = 0.f;
            if (lane < cnt) {
                const int r = rows[begin + c0 + lane];
                const bool ok = r >= 0 && (int64_t)r < n_window;
                my_row = ok ? r : 0;
                my_w = ok ? weights[begin + c0 + lane] : 0.f;
            }
            for (int j = 0; j < cnt; j += FI_FLIGHT) {          // (j, cnt wave-uniform)
                float4 x[FI_FLIGHT];
                float w[FI_FLIGHT];
#pragma unroll
                for (int k = 0; k < FI_FLIGHT; ++k) {
                    x[k] = make_float4(0.f, 0.f, 0.f, 0.f);
                    w[k] = 0.f;
                    if (j + k < cnt) {
                        const int r = __builtin_amdgcn_readlane(my_row, j + k);
                        w[k] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_w), j + k));
                        if (live) x[k] = *reinterpret_cast<const float4 *>(base + (int64_t)r * ld);
                    }
                }
#pragma unroll
                for (int k = 0; k < FI_FLIGHT; ++k)
                    if (j + k < cnt) {
                        const double wd = (double)w[k];
                        acc[0] += wd * (double)x[k].x;
                        acc[1] += wd * (double)x[k].y;
                        acc[2] += wd * (double)x[k].z;
                        acc[3] += wd * (double)x[k].w;
                    }
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) s_part[wave][lane * 4 + e] = acc[e];
        __syncthreads();
        if (p0 + tid < C) {                                     // thread t: column p0 + t, the waves' partial sums in wave order
            double sum = s_part[0][tid];
#pragma unroll
            for (int w = 1; w < FI_WAVES; ++w) sum += s_part[w][tid];
            out[q * ldo + p0 + tid] = (float)sum;
        }
        __syncthreads();                                        // (the next pass writes s_part again)
    }
}

}  // namespace elimrec

using namespace elimrec;

extern "C" int elimrec_segment_row_sum_chunk(void) { return FI_CHUNK; }

extern "C" int elimrec_segment_row_sum(const float *d_table, int64_t n_rows, int64_t C, int64_t ld, int64_t row_offset,
                                       const int64_t *d_ptr, const int32_t *d_rows, const float *d_weights, int64_t Q,
                                       int64_t n_entries, float *d_out, int64_t ldo, void *stream) {
    ELIMREC_REQUIRE(Q >= 0 && n_entries >= 0 && n_rows >= 0, "segment_row_sum: need Q >= 0, n_entries >= 0, n_rows >= 0");
    if (Q == 0) return 0;
    ELIMREC_REQUIRE(d_ptr && d_out, "segment_row_sum: null pointer");
    ELIMREC_REQUIRE(C >= 4 && C <= 1280 && C % 4 == 0, "segment_row_sum: C must be a multiple of 4 in [4, 1280], got %lld", (long long)C);
    ELIMREC_REQUIRE(ld >= C && ld % 4 == 0 && ldo >= C && ldo % 4 == 0,
                    "segment_row_sum: the row strides must be multiples of 4 floats and at least C");
    ELIMREC_REQUIRE(((uintptr_t)d_table & 15) == 0 && ((uintptr_t)d_out & 15) == 0, "segment_row_sum: table and out must be 16-byte aligned");
    ELIMREC_REQUIRE(row_offset >= 0 && row_offset <= n_rows, "segment_row_sum: row_offset outside [0, n_rows]");
    ELIMREC_REQUIRE(Q < (int64_t)INT32_MAX, "segment_row_sum: %lld segments exceed one launch", (long long)Q);
    if (n_entries) {
        ELIMREC_REQUIRE(d_table && d_rows && d_weights, "segment_row_sum: null pointer");
        ELIMREC_REQUIRE(n_rows - row_offset >= 1, "segment_row_sum: the window behind row_offset holds no row");
    }
    hipLaunchKernelGGL(segment_row_sum_kernel, dim3((unsigned)Q), dim3(FI_THREADS), 0, (hipStream_t)stream,
                       d_table + row_offset * ld, ld, n_rows - row_offset, (int)C, d_ptr, d_rows, d_weights, n_entries, d_out, ldo);
    ELIMREC_LAUNCH_CHECK("segment_row_sum");
    return 0;
}
