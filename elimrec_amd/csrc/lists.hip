// The recommendation lists themselves: the mean pairwise cosine of each id list over a table (intra-list similarity), and how often
// every row of the catalogue is listed (exposure).
//
// list_pair_cosine_kernel: ONE workgroup owns ONE list of K ids (W = 1 wave for K <= LIST_SMALLK, 4 waves above). The ids are
// checked once -- an entry outside [0, n_rows) is "not listed", wherever it stands: id -1, a zero row, reciprocal norm 0, never
// dereferenced -- and kept in LDS, padded to KP = 16 ceil(K / 16) positions. Per column block h of the table the list's rows are
// gathered ONCE, in column chunks of DC = list_chunk_cols(KP, d) columns (all d columns when they fit 60 KiB of LDS, row stride
// DC + 4 floats: 16-byte aligned b128 stores, operand reads two-way at worst), and the K x K upper triangle is formed as 16 x 16
// tiles (ti <= tj) on v_mfma_f32_16x16x4_f32: wave w takes tiles w, w + W, ... in row-major triangle order; A = the rows of tile
// ti, B = the rows of tile tj, so lane (li, kq) ends with positions i = 16 ti + 4 kq + r against j = 16 tj + li. A pair i < j adds
//     (double)((dot * inv(sq_i)) * inv(sq_j)),   inv(x) = 1 / max(sqrt(x), 1e-12)            (cosine.h's inv_norm)
// to the lane's float64 sum; with several column chunks `dot` is the chunk's part of the dot product (the cosine is linear in it).
// The lane sums are folded by a fixed butterfly, the wave sums added in wave order, divided by the number of listed pairs in
// float64 and rounded ONCE to fp32: the sum's order is fixed by (K, d) alone, so a list's bits depend on its entries only -- not on
// B, its place in the batch, the grid or the other lists. Nothing of size K x K leaves the registers. Fewer than two listed
// entries give NaN; duplicates are pairs like any other.
// LDS at K = 256, d = 256: 256 rows x (56 + 4) floats = 60 KiB of rows (5 chunks: 56 x 4 + 32 columns), 1 KiB of reciprocal
// norms, 1 KiB of ids, 32 B of wave sums: 62.1 KiB, two workgroups per CU. K = 10, d = 64: 16 x 68 floats = 4.3 KiB, one chunk.
// list_exposure_kernel: counts[id] += 1 per listed entry, integer vector atomics: exact, whatever the order.
#include "common.h"
#include "cosine.h"

namespace elimrec {

constexpr int LIST_MAXK = 256, LIST_SMALLK = 32;
constexpr int LIST_ROW_FLOATS = 15 * 1024;                   // LDS floats for the staged rows (60 KiB)
typedef float list_v4f __attribute__((ext_vector_type(4)));

// columns of one LDS stage for KP padded list positions: all d when they fit, else the largest multiple of 4 that does
static inline int list_chunk_cols(int KP, int d) {
    const int fit = (LIST_ROW_FLOATS / KP - 4) & ~3;
    return fit < d ? fit : d;
}
static inline size_t list_lds_bytes(int KP, int dc) { return (size_t)KP * (dc + 4) * 4 + (size_t)KP * 8 + 64; }

struct ListArgs {
    const float *T; int64_t ld, n_rows; int d, blocks;
    const float *sq; int64_t ld_sq;
    const int32_t *lists; int K;
    float *out;
    int vec, dc;                       // vec: T is 16-byte aligned and ld % 4 == 0 -> a row's float4s are single loads
};

template <int W>
__global__ __launch_bounds__(64 * W) void list_pair_cosine_kernel(ListArgs a) {
    constexpr int NT = 64 * W;
    const int K = a.K, KT = (K + 15) / 16, KP = 16 * KT, d = a.d, DC = a.dc, LD = DC + 4;
    extern __shared__ __attribute__((aligned(16))) float list_smem[];
    float *s_rows = list_smem;                               // [KP][LD] the list's rows, one column chunk of one block
    float *s_inv = s_rows + KP * LD;                         // [KP]     their reciprocal norms in the current block
    int *s_ids = (int *)(s_inv + KP);                        // [KP]     the checked ids, -1 = not listed
    double *s_part = (double *)(s_ids + KP);                 // [W]      wave sums
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, kq = lane >> 4;
    const int64_t b = blockIdx.x;

    for (int k = tid; k < KP; k += NT) {
        int id = k < K ? a.lists[b * K + k] : -1;
        if (id < 0 || (int64_t)id >= a.n_rows) id = -1;
        s_ids[k] = id;
    }
    __syncthreads();
    int n = 0;                                               // listed entries (every wave counts them the same way)
    for (int k = lane; k < KP; k += 64) n += s_ids[k] >= 0 ? 1 : 0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off, 64);
    const int n_tiles = KT * (KT + 1) / 2;

    for (int h = 0; h < a.blocks; ++h) {
        double sum = 0.0;
        for (int c0 = 0; c0 < d; c0 += DC) {
            const int dcur = d - c0 < DC ? d - c0 : DC, c4n = dcur >> 2;
            __syncthreads();                                 // every wave is done with the previous stage (and its s_inv)
            if (c0 == 0)
                for (int k = tid; k < KP; k += NT) {
                    const int id = s_ids[k];
                    s_inv[k] = id >= 0 ? inv_norm(a.sq[(int64_t)id * a.ld_sq + h]) : 0.f;
                }
            for (int e = tid; e < KP * c4n; e += NT) {
                const int r = e / c4n, c = (e - r * c4n) << 2;
                const int id = s_ids[r];
                float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
                if (id >= 0) ELIMREC_LOAD_ROW4(x, a.T + (int64_t)id * a.ld + (int64_t)h * d + c0 + c, a.vec);
                *reinterpret_cast<float4 *>(s_rows + r * LD + c) = x;
            }
            __syncthreads();
            for (int t = wave; t < n_tiles; t += W) {        // (wave-uniform)
                int ti = 0, rem = t;
                while (rem >= KT - ti) { rem -= KT - ti; ++ti; }
                const int tj = ti + rem;
                const float *ap = s_rows + (16 * ti + li) * LD + kq;
                const float *bp = s_rows + (16 * tj + li) * LD + kq;
                list_v4f acc0 = (list_v4f){0.f, 0.f, 0.f, 0.f}, acc1 = acc0;   // two chains: even / odd k-steps
                int ks = 0;
                for (; ks + 1 < c4n; ks += 2) {
                    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[4 * ks], bp[4 * ks], acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[4 * ks + 4], bp[4 * ks + 4], acc1, 0, 0, 0);
                }
                if (ks < c4n) acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[4 * ks], bp[4 * ks], acc0, 0, 0, 0);
                // lane: position j = 16 tj + li against positions i = 16 ti + 4 kq + r
                const int j = 16 * tj + li;
                const float invj = s_inv[j];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int i = 16 * ti + 4 * kq + r;
                    const float dot = acc0[r] + acc1[r];
                    if (i < j) sum += (double)((dot * s_inv[i]) * invj);
                }
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
        if (lane == 0) s_part[wave] = sum;
        __syncthreads();
        if (tid == 0) {
            double s = 0.0;
            for (int w = 0; w < W; ++w) s += s_part[w];
            const double pairs = 0.5 * (double)n * (double)(n - 1);
            a.out[b * a.blocks + h] = n >= 2 ? (float)(s / pairs) : __builtin_nanf("");
        }
    }
}

__global__ __launch_bounds__(256) void list_exposure_kernel(const int32_t *__restrict__ lists, int64_t n, int64_t n_rows,
                                                            int32_t *__restrict__ counts) {
    const int64_t step = (int64_t)gridDim.x * 256;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += step) {
        const int id = lists[e];
        if (id >= 0 && (int64_t)id < n_rows) atomicAdd(&counts[id], 1);
    }
}

template <int W>
static int list_launch(const ListArgs &a, int64_t B, hipStream_t s) {
    const size_t lds = list_lds_bytes(16 * ((a.K + 15) / 16), a.dc);
    hipLaunchKernelGGL((list_pair_cosine_kernel<W>), dim3((unsigned)B), dim3(64 * W), lds, s, a);
    ELIMREC_LAUNCH_CHECK("list_pair_cosine");
    return 0;
}

}  // namespace elimrec

using namespace elimrec;

extern "C" int elimrec_list_max_k(void) { return LIST_MAXK; }
extern "C" int elimrec_list_pair_cosine_small_k(void) { return LIST_SMALLK; }
extern "C" int elimrec_list_pair_cosine_chunk_cols(int K, int d) {
    if (K < 1 || K > LIST_MAXK || d < 4 || d > TABLE_MAXD || d % 4 != 0) return 0;
    return list_chunk_cols(16 * ((K + 15) / 16), d);
}

extern "C" int elimrec_list_pair_cosine(const float *d_T, int64_t ld, int64_t n_rows, int blocks, int d, const float *d_sqnorm,
                                        int64_t ld_sq, const int32_t *d_lists, int64_t B, int K, float *d_out, void *stream) {
    ELIMREC_REQUIRE(K >= 1 && K <= LIST_MAXK, "list_pair_cosine: 1 <= K <= %d, got %d", LIST_MAXK, K);
    if (int rc = table_dims("list_pair_cosine", d, blocks)) return rc;
    ELIMREC_REQUIRE(B >= 0 && B < (int64_t)INT32_MAX && n_rows >= 0 && n_rows < (int64_t)INT32_MAX,
                    "list_pair_cosine: need 0 <= B < 2^31 - 1 and 0 <= n_rows < 2^31 - 1");
    ELIMREC_REQUIRE(ld >= (int64_t)blocks * d && ld_sq >= blocks, "list_pair_cosine: ld < blocks * d or ld_sq < blocks");
    if (B == 0) return 0;
    ELIMREC_REQUIRE(d_lists && d_out, "list_pair_cosine: null pointer");
    ELIMREC_REQUIRE(n_rows == 0 || (d_T && d_sqnorm), "list_pair_cosine: null pointer");
    ListArgs a;
    a.T = d_T; a.ld = ld; a.n_rows = n_rows; a.d = d; a.blocks = blocks;
    a.sq = d_sqnorm; a.ld_sq = ld_sq;
    a.lists = d_lists; a.K = K;
    a.out = d_out;
    a.vec = table_vec(d_T, ld);
    a.dc = list_chunk_cols(16 * ((K + 15) / 16), d);
    hipStream_t s = (hipStream_t)stream;
    return K <= LIST_SMALLK ? list_launch<1>(a, B, s) : list_launch<4>(a, B, s);
}

extern "C" int elimrec_list_exposure(const int32_t *d_lists, int64_t B, int K, int64_t n_rows, int32_t *d_counts, void *stream) {
    ELIMREC_REQUIRE(B >= 0 && K >= 1 && n_rows >= 0 && n_rows < (int64_t)INT32_MAX && B < (int64_t)INT32_MAX,
                    "list_exposure: need 0 <= B < 2^31 - 1, K >= 1 and 0 <= n_rows < 2^31 - 1");
    if (B == 0 || n_rows == 0) return 0;
    ELIMREC_REQUIRE(d_lists && d_counts, "list_exposure: null pointer");
    const int64_t n = B * (int64_t)K, want = (n + 255) / 256;
    hipLaunchKernelGGL(list_exposure_kernel, dim3((unsigned)(want < 4096 ? want : 4096)), dim3(256), 0, (hipStream_t)stream, d_lists, n,
                       n_rows, d_counts);
    ELIMREC_LAUNCH_CHECK("list_exposure");
    return 0;
}
