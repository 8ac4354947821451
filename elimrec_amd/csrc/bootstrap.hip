// Paired, per-group, non-parametric bootstrap of a block of per-row values (include/elimrec_hip.h: elimrec_bootstrap_means):
// out[r, g, :] = the mean of n_g rows of group g drawn with replacement, the draws fixed by (seed, r, g, t) through Philox4x32-10.
//
// One workgroup of 256 threads per (group, tile of BOOT_TILE = 16 replicates), BOOT_LANES = 16 lanes per replicate. Lane s of a
// replicate takes the Philox calls b = s, s + 16, ... (call b serves the draws t = 4 b .. 4 b + 3) and adds its drawn rows, t
// ascending, into C float64 accumulators in registers; the 16 partials are then added in the fixed tree (s, s + 8), (.., + 4),
// (.., + 2), (.., + 1) and divided by n_g. The order is a function of n_g alone, there is no atomic and no workspace: the bits of
// out[r, g, c] do not depend on R, G, C, ld, the column's place, the grid or the form below.
// Two forms, chosen per group by (n_g, C) alone (boot_rows_fit): a group whose n_g x C values fit BOOT_LDS_DOUBLES float64 words
// is staged once per workgroup into LDS -- position-major, already converted (and, paired, already subtracted) -- and resampled
// from there; a larger group reads group_rows[ptr[g] + j] and the row from global memory (L2) at every draw. Both add the same
// float64 values in the same order. A call with both kinds of groups is two launches, each skipping the other's groups, so that
// the global form does not carry the LDS form's 64 KiB and keeps its occupancy.
#include "common.h"
#include "dispatch.h"
#include "philox.h"

namespace elimrec {

constexpr int BOOT_THREADS = 256;
constexpr int BOOT_LANES = 16;                            // lanes per replicate
constexpr int BOOT_TILE = BOOT_THREADS / BOOT_LANES;      // replicates per workgroup
constexpr int BOOT_CMAX = 16;                             // columns per call: 32 float64 accumulator registers, 8 waves per SIMD
constexpr int BOOT_LDS_DOUBLES = 8192;                    // 64 KiB: two workgroups per CU
constexpr uint32_t BOOT_DOMAIN = 0x626F6F74u;             // counter word 3: "boot"

__host__ __device__ inline bool boot_rows_fit(int64_t n_g, int C) { return n_g * (int64_t)C <= (int64_t)BOOT_LDS_DOUBLES; }

struct BootArgs {
    const float *rows, *rows_b;
    int64_t n, ld;
    int C;
    const int64_t *ptr;
    const int32_t *grows;
    int64_t n_listed;
    int64_t tiles;          // replicate tiles per group
    int R;
    uint32_t k0, k1;
    double *out;
    int64_t ld_group;       // G * ld_out: doubles between two replicates
    int64_t ld_out;
    int skip_fitting;       // global form only: leave the groups that fit LDS to the other launch
};

// The value of column c of listed row i; a row index outside [0, n) is never dereferenced (NaN).
__device__ __forceinline__ double boot_value(const BootArgs &a, int32_t i, int c) {
    if ((uint32_t)i >= (uint32_t)a.n) return __longlong_as_double(0x7ff8000000000000ll);
    const int64_t at = (int64_t)i * a.ld + c;
    const double v = (double)a.rows[at];
    return a.rows_b ? (double)a.rows_b[at] - v : v;
}

template <int CT, bool LDS> __global__ __launch_bounds__(BOOT_THREADS) void bootstrap_kernel(const BootArgs a) {
    extern __shared__ __attribute__((aligned(16))) double boot_lds[];
    const int64_t g = (int64_t)blockIdx.x / a.tiles, tile = (int64_t)blockIdx.x - g * a.tiles;
    int64_t beg = a.ptr[g], end = a.ptr[g + 1];
    if (beg < 0 || end < beg || end > a.n_listed || end - beg > (int64_t)INT32_MAX) end = beg = 0;   // a broken segment: empty (NaN)
    const uint32_t ng = (uint32_t)(end - beg);
    const int C = a.C;
    const bool fits = boot_rows_fit(ng, C);
    if (LDS ? !fits : (a.skip_fitting && fits)) return;
    const int tid = threadIdx.x, sub = tid & (BOOT_LANES - 1);
    const int64_t r = tile * BOOT_TILE + (tid >> 4);
    const int32_t *__restrict__ grows = a.grows + beg;
    if constexpr (LDS) {
        const int total = (int)ng * C;
        for (int at = tid; at < total; at += BOOT_THREADS) {
            const int j = at / C;
            boot_lds[at] = boot_value(a, grows[j], at - j * C);
        }
        __syncthreads();
    }
    double acc[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) acc[c] = 0.0;
    const uint32_t calls = r < a.R ? (ng + 3u) >> 2 : 0u;
    Philox ph;
    ph.k[0] = a.k0; ph.k[1] = a.k1;
    ph.c[1] = (uint32_t)r; ph.c[2] = (uint32_t)g; ph.c[3] = BOOT_DOMAIN;
    for (uint32_t b = sub; b < calls; b += BOOT_LANES) {
        uint32_t w[4];
        ph.c[0] = b;
        ph.generate(w);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (4u * b + k < ng) {
                const uint32_t j = __umulhi(w[k], ng);                   // (uint64(word) * n_g) >> 32, in [0, n_g)
                if constexpr (LDS) {
                    const double *__restrict__ p = boot_lds + (size_t)j * C;
#pragma unroll
                    for (int c = 0; c < CT; ++c)
                        if (c < C) acc[c] += p[c];
                } else {
                    const int32_t i = grows[j];
#pragma unroll
                    for (int c = 0; c < CT; ++c)
                        if (c < C) acc[c] += boot_value(a, i, c);
                }
            }
        }
    }
    double *__restrict__ o = a.out + r * a.ld_group + g * a.ld_out;
#pragma unroll
    for (int c = 0; c < CT; ++c) {
        if (c < C) {
            double v = acc[c];
#pragma unroll
            for (int off = BOOT_LANES / 2; off >= 1; off >>= 1) v += __shfl_down(v, off, BOOT_LANES);
            if (sub == 0 && r < a.R) o[c] = ng ? v / (double)ng : __longlong_as_double(0x7ff8000000000000ll);
        }
    }
}

}  // namespace elimrec

using namespace elimrec;

extern "C" int elimrec_bootstrap_max_columns(void) { return BOOT_CMAX; }
extern "C" int elimrec_bootstrap_replicate_tile(void) { return BOOT_TILE; }
extern "C" int elimrec_bootstrap_rows_in_lds(int64_t n_g, int C) {
    if (n_g < 0 || n_g > (int64_t)INT32_MAX || C < 1 || C > BOOT_CMAX) return -1;
    return boot_rows_fit(n_g, C) ? 1 : 0;
}

extern "C" int elimrec_bootstrap_means(const float *d_rows, const float *d_rows_b, int64_t n_rows, int C, int64_t ld,
                                       const int64_t *d_group_ptr, const int32_t *d_group_rows, int64_t n_listed_rows, int G,
                                       int64_t R, uint64_t seed, double *d_out, int64_t ld_out, int use_lds, void *stream) {
    ELIMREC_REQUIRE(R >= 1 && R < ((int64_t)1 << 31), "bootstrap_means: 1 <= R < 2^31, got %lld", (long long)R);
    ELIMREC_REQUIRE(C >= 1 && C <= BOOT_CMAX, "bootstrap_means: 1 <= C <= %d, got %d", BOOT_CMAX, C);
    ELIMREC_REQUIRE(n_rows >= 0 && n_rows < ((int64_t)1 << 31), "bootstrap_means: 0 <= n_rows < 2^31, got %lld", (long long)n_rows);
    ELIMREC_REQUIRE(n_listed_rows >= 0 && n_listed_rows < ((int64_t)1 << 31), "bootstrap_means: 0 <= n_listed_rows < 2^31, got %lld",
                    (long long)n_listed_rows);
    ELIMREC_REQUIRE(G >= 1, "bootstrap_means: G >= 1, got %d", G);
    ELIMREC_REQUIRE(ld >= C && ld_out >= C, "bootstrap_means: ld < C or ld_out < C");
    ELIMREC_REQUIRE(use_lds == 0 || use_lds == 1, "bootstrap_means: use_lds is 0 or 1, got %d", use_lds);
    ELIMREC_REQUIRE(d_group_ptr && d_out, "bootstrap_means: null pointer");
    ELIMREC_REQUIRE(n_listed_rows == 0 || (d_rows && d_group_rows && n_rows >= 1), "bootstrap_means: rows are listed, but there are none");
    const int64_t tiles = (R + BOOT_TILE - 1) / BOOT_TILE;
    ELIMREC_REQUIRE(tiles * G < (int64_t)INT32_MAX, "bootstrap_means: %lld replicate tiles x %d groups exceed one launch", (long long)tiles, G);
    BootArgs a;
    a.rows = d_rows; a.rows_b = d_rows_b; a.n = n_rows; a.ld = ld; a.C = C;
    a.ptr = d_group_ptr; a.grows = d_group_rows; a.n_listed = n_listed_rows;
    a.tiles = tiles; a.R = (int)R;
    a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32);
    a.out = d_out; a.ld_group = (int64_t)G * ld_out; a.ld_out = ld_out;
    a.skip_fitting = use_lds;
    const dim3 grid((unsigned)(tiles * G)), block(BOOT_THREADS);
    hipStream_t s = (hipStream_t)stream;
    auto launch = [&](auto ct) {
        constexpr int CT = decltype(ct)::value;
        if (use_lds) {
            hipLaunchKernelGGL((bootstrap_kernel<CT, true>), grid, block, (size_t)BOOT_LDS_DOUBLES * sizeof(double), s, a);
            ELIMREC_LAUNCH_CHECK("bootstrap_means (LDS form)");
        }
        hipLaunchKernelGGL((bootstrap_kernel<CT, false>), grid, block, 0, s, a);
        ELIMREC_LAUNCH_CHECK("bootstrap_means");
        return 0;
    };
    return C <= 4 ? launch(int_c<4>{}) : C <= 8 ? launch(int_c<8>{}) : launch(int_c<16>{});
}
