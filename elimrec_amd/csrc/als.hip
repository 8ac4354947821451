// One half-sweep of implicit-feedback ALS (Hu, Koren, Volinsky, ICDM 2008): per listed row r of the side being solved
//     A_r = A0 + reg[r] I + conf sum_{j in N(r)} f_j f_j^T,   b_r = (1 + conf) sum_{j in N(r)} f_j,   x_r = A_r^-1 b_r
// with A0 = F^T F (the Gram trick: the sum over ALL pairs costs d^2 per row) and f_j the fixed side's float32 factor rows.
//
// als_solve_kernel<D>: ONE workgroup of 4 waves per listed row. The neighbours' rows are gathered through one LDS stage of
// ALS_CHUNK rows (row stride D + 4 floats: 16-byte aligned b128 stores); the next chunk's ids and rows travel in registers while
// the current one is multiplied (two barriers per chunk, as knn.hip stages its candidates). The upper-triangle 16 x 16 tiles of
// sum f f^T are accumulated with v_mfma_f64_16x16x4_f64, four neighbours per instruction: tile t of the triangle (row-major over
// ti <= tj) belongs to wave t % 4, which walks the WHOLE list for it, so a tile's sum runs in the CSR order of the row's list.
// Operands as the f32 16x16x4 form, one double per lane (A[lane & 15][k = lane >> 4], B[k = lane >> 4][lane & 15]); C/D is the
// f64 map, col = lane & 15, row = (lane >> 4) + 4 * reg_idx. The MFMA form is the one that shipped; a plain-FMA form was not
// built beside it: measured at the Tiktok shape (tools/ials_time.py) a neighbour costs 0.11 us of accumulation against 71 us for
// the solve of a row, so at the degrees met there the choice cannot show. The float32 factors are widened, so every product is exact in
// float64 and a fused or unfused accumulate gives the same bits; rows behind the end of the list are zero operands (x + 0 = x).
// b is summed by wave 3 (the wave with the fewest tiles), lane c its column c, in list order.
// Everything is float64 and rounded to float32 once at the store; no floating-point atomics: a row's bits depend on A0, reg[r],
// conf and the listed rows of F in list order alone -- not on the grid, the position in `rows` or the other rows of the call.
// A_r = (A0 + reg on the diagonal) + conf * S, mirrored from the upper triangle (exactly symmetric), lives in LDS with a row
// stride of D + 1 doubles: 33 280 B at D = 64. With the stage (17 408 B), the diagonal and b the workgroup takes 51 712 B, within
// 64 KiB so that two fit on a CU -- that budget is a design choice, not a measurement.
// Solve: right-looking Cholesky A = L L^T in LDS by the whole workgroup (the threads as 16 x 16 over the trailing lower
// triangle, two barriers per column, IEEE sqrt and division), then forward and back substitution by wave 0, lane i = unknown i,
// the pivot unknown broadcast by a shuffle. A pivot that is <= 0 or not finite ends the row: status[0] += 1 (integer atomicAdd),
// status[1] = min(status[1], r), the row is written as zeros. A row with an empty list is zeros without a solve. The ids were
// checked by the host; an id outside the fixed side is a zero row all the same, and the kernel reads nothing outside its inputs.
#include "common.h"
#include "cosine.h"

namespace elimrec {

constexpr int ALS_CHUNK = 64, ALS_THREADS = 256, ALS_MIND = 16, ALS_MAXD = 64;
typedef double als_v4d __attribute__((ext_vector_type(4)));

struct AlsArgs {
    const float *F; int64_t ld, n_fixed; int vec;
    const double *A0;
    const int64_t *ptr; const int32_t *nbr; int64_t n;
    const int32_t *rows;
    const double *reg; double conf;
    float *out; int64_t ld_out;
    int32_t *status;
};

// dynamic LDS of one workgroup, in bytes (host and device agree through this one function)
constexpr size_t als_lds_bytes(int D) { return (size_t)D * (D + 1) * 8 + 2 * (size_t)D * 8 + (size_t)ALS_CHUNK * (D + 4) * 4; }

template <int D>
__global__ __launch_bounds__(ALS_THREADS) void als_solve_kernel(AlsArgs a) {
    constexpr int T = D / 16, NTILE = T * (T + 1) / 2, TPW = (NTILE + 3) / 4, LDA = D + 1, LDF = D + 4;
    constexpr int PFN = (ALS_CHUNK * D / 4 + ALS_THREADS - 1) / ALS_THREADS;
    extern __shared__ double als_smem[];
    double *s_A = als_smem;                                  // [D][LDA]
    double *s_diag = s_A + D * LDA;                          // [D] the diagonal of L
    double *s_b = s_diag + D;                                // [D]
    float *s_f = reinterpret_cast<float *>(s_b + D);         // [ALS_CHUNK][LDF] the stage's neighbour rows
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, kq = lane >> 4;
    const int64_t r = a.rows[blockIdx.x];
    if (r < 0 || r >= a.n) return;                           // (workgroup-uniform; the host checked the ids)
    const int64_t p0 = a.ptr[r], deg = a.ptr[r + 1] - p0;
    float *orow = a.out + r * a.ld_out;
    if (deg <= 0) {                                          // an empty list: zeros without a solve
        if (tid < D) orow[tid] = 0.f;
        return;
    }

    // this wave's tiles of the upper triangle: t = wave + 4 s, row-major over ti <= tj
    int tile_i[TPW], tile_j[TPW];
    als_v4d acc[TPW];
#pragma unroll
    for (int s = 0; s < TPW; ++s) {
        int t = wave + 4 * s, ti = 0;
        while (ti < T && t >= T - ti) { t -= T - ti; ++ti; }
        tile_i[s] = ti < T ? ti : -1;                        // -1: no such tile
        tile_j[s] = ti + t;
        acc[s] = (als_v4d){0.0, 0.0, 0.0, 0.0};
    }
    double bsum = 0.0;

    float4 pf[PFN];
    auto load_stage = [&](int64_t c0) {
#pragma unroll
        for (int p = 0; p < PFN; ++p) {
            const int e = (tid + ALS_THREADS * p) * 4;
            if (e < ALS_CHUNK * D) {
                const int row = e / D, c = e - row * D;
                float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
                if (c0 + row < deg) {
                    const int64_t id = a.nbr[p0 + c0 + row];
                    if (id >= 0 && id < a.n_fixed) ELIMREC_LOAD_ROW4(x, a.F + id * a.ld + c, a.vec);
                }
                pf[p] = x;
            }
        }
    };
    auto store_stage = [&]() {
#pragma unroll
        for (int p = 0; p < PFN; ++p) {
            const int e = (tid + ALS_THREADS * p) * 4;
            if (e < ALS_CHUNK * D) {
                const int row = e / D, c = e - row * D;
                *reinterpret_cast<float4 *>(s_f + row * LDF + c) = pf[p];
            }
        }
    };

    load_stage(0);
    store_stage();
    __syncthreads();
    for (int64_t c0 = 0; c0 < deg; c0 += ALS_CHUNK) {
        const bool more = c0 + ALS_CHUNK < deg;              // workgroup-uniform
        if (more) load_stage(c0 + ALS_CHUNK);
        const int left = deg - c0 < ALS_CHUNK ? (int)(deg - c0) : ALS_CHUNK;
#pragma unroll 1
        for (int j0 = 0; j0 < left; j0 += 4) {
            const float *fp = s_f + (j0 + kq) * LDF + li;
#pragma unroll
            for (int s = 0; s < TPW; ++s)
                if (tile_i[s] >= 0)                          // wave-uniform
                    acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64((double)fp[16 * tile_i[s]], (double)fp[16 * tile_j[s]], acc[s], 0, 0, 0);
        }
        if (wave == 3 && lane < D)
            for (int j = 0; j < left; ++j) bsum += (double)s_f[j * LDF + lane];
        __syncthreads();                                     // every wave is done with the stage
        if (more) store_stage();
        __syncthreads();
    }

    // A_r from the upper triangle, mirrored; b_r
    const double regr = a.reg[r];
#pragma unroll
    for (int s = 0; s < TPW; ++s) {
        if (tile_i[s] < 0) continue;
#pragma unroll
        for (int x = 0; x < 4; ++x) {
            const int gi = 16 * tile_i[s] + kq + 4 * x, gj = 16 * tile_j[s] + li;
            if (gi > gj) continue;                           // the lower half of a diagonal tile
            double v = a.A0[gi * D + gj];
            if (gi == gj) v = v + regr;
            v = v + a.conf * acc[s][x];
            s_A[gi * LDA + gj] = v;
            s_A[gj * LDA + gi] = v;
        }
    }
    if (wave == 3 && lane < D) s_b[lane] = (1.0 + a.conf) * bsum;

    // Cholesky, right-looking: column k scaled, then the trailing lower triangle updated
    const int tx = tid & 15, ty = tid >> 4;
    bool bad = false;
    for (int k = 0; k < D; ++k) {
        __syncthreads();
        const double p = s_A[k * LDA + k];                   // the same value on every thread
        if (!(p > 0.0) || p == __builtin_huge_val()) { bad = true; break; }
        const double lkk = sqrt(p);
        if (tid == 0) s_diag[k] = lkk;
        else if (k + tid < D) s_A[(k + tid) * LDA + k] = s_A[(k + tid) * LDA + k] / lkk;
        __syncthreads();
        for (int i = k + 1 + ty; i < D; i += 16) {
            const double lik = s_A[i * LDA + k];
            for (int j = k + 1 + tx; j <= i; j += 16) s_A[i * LDA + j] = s_A[i * LDA + j] - lik * s_A[j * LDA + k];
        }
    }
    if (bad) {                                               // workgroup-uniform
        if (tid == 0) {
            atomicAdd(&a.status[0], 1);
            atomicMin(&a.status[1], (int)r);
        }
        if (tid < D) orow[tid] = 0.f;
        return;
    }
    __syncthreads();
    if (wave != 0) return;
    // L y = b, then L^T x = y: lane i holds unknown i
    double v = lane < D ? s_b[lane] : 0.0;
    for (int k = 0; k < D; ++k) {
        if (lane == k) v = v / s_diag[k];
        const double yk = __shfl(v, k, 64);
        if (lane > k && lane < D) v = v - s_A[lane * LDA + k] * yk;
    }
    for (int k = D - 1; k >= 0; --k) {
        if (lane == k) v = v / s_diag[k];
        const double xk = __shfl(v, k, 64);
        if (lane < k) v = v - s_A[k * LDA + lane] * xk;
    }
    if (lane < D) orow[lane] = (float)v;
}

template <int D>
static int als_launch(const AlsArgs &a, int64_t Q, hipStream_t s) {
    static_assert(als_lds_bytes(D) <= 64 * 1024, "als_solve: the workgroup stays within 64 KiB of LDS");
    hipLaunchKernelGGL(als_solve_kernel<D>, dim3((unsigned)Q), dim3(ALS_THREADS), als_lds_bytes(D), s, a);
    ELIMREC_LAUNCH_CHECK("als_solve");
    return 0;
}

}  // namespace elimrec

using namespace elimrec;

extern "C" int elimrec_als_chunk(void) { return ALS_CHUNK; }

extern "C" int elimrec_als_solve(const float *d_F, int64_t ld, int64_t n_fixed, int d, const double *d_A0, const int64_t *d_ptr,
                                 const int32_t *d_nbr, int64_t n, const int32_t *d_rows, int64_t Q, const double *d_reg, double conf,
                                 float *d_out, int64_t ld_out, int32_t *d_status, void *stream) {
    ELIMREC_REQUIRE(d % 16 == 0 && d >= ALS_MIND && d <= ALS_MAXD, "als_solve: d %% 16 == 0 and %d <= d <= %d, got %d", ALS_MIND, ALS_MAXD, d);
    ELIMREC_REQUIRE(Q >= 0 && n >= 0 && n < (int64_t)INT32_MAX && n_fixed >= 0 && n_fixed < (int64_t)INT32_MAX,
                    "als_solve: need Q >= 0 and both sides' row counts in [0, 2^31 - 1)");
    ELIMREC_REQUIRE(ld >= d && ld_out >= d, "als_solve: ld < d or ld_out < d");
    ELIMREC_REQUIRE(conf >= 0.0 && conf <= 1.7976931348623157e308, "als_solve: conf must be finite and >= 0");
    if (Q == 0) return 0;
    ELIMREC_REQUIRE(Q < (int64_t)INT32_MAX, "als_solve: too many rows for one launch");
    ELIMREC_REQUIRE(d_A0 && d_ptr && d_rows && d_reg && d_out && d_status && (n_fixed == 0 || d_F), "als_solve: null pointer");
    AlsArgs a;
    a.F = d_F; a.ld = ld; a.n_fixed = n_fixed; a.vec = table_vec(d_F, ld);
    a.A0 = d_A0;
    a.ptr = d_ptr; a.nbr = d_nbr; a.n = n;
    a.rows = d_rows;
    a.reg = d_reg; a.conf = conf;
    a.out = d_out; a.ld_out = ld_out;
    a.status = d_status;
    hipStream_t s = (hipStream_t)stream;
    switch (d) {
    case 16: return als_launch<16>(a, Q, s);
    case 32: return als_launch<32>(a, Q, s);
    case 48: return als_launch<48>(a, Q, s);
    default: return als_launch<64>(a, Q, s);
    }
}
