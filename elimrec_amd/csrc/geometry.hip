// Embedding geometry of one block of a cached table, over a LIST of row ids (a side's rows, or a group's): the all-pairs
// uniformity sum of Wang & Isola and the float64 Gram matrix of the unit rows, whose spectrum the host reads (reports.py).
// A list entry is VALID when its id lies in [0, n_rows) and its row's squared norm is > 0 and finite; any other entry takes part
// in nothing and its row is never read (an id outside the table is never dereferenced). A repeated id is an entry of its own.
//
// uniformity_cell_kernel: knn.hip's structure. The list's positions are cut into tiles of GEO_TILE = 64 (queries) and chunks of
// GEO_CHUNK = 2048 (candidates); a CELL is (tile, chunk). Only the cells that hold a pair p < q are launched: tile i meets the
// chunks c >= i / 32, and the 1-D grid runs over exactly those cells, tile-major (geo_cells_before), so the triangle costs no
// idle workgroups. A workgroup of 4 waves holds its 64 query rows -- a wave owns 16 of them as the A operands of
// v_mfma_f32_16x16x4_f32 (registers for d = 32 / 64 / 128, a lane-private LDS column otherwise) -- and streams the chunk's rows,
// gathered through the id list, through ONE LDS stage of SR rows (row stride d + 4 floats); the next stage travels in registers
// while the current one is multiplied (two barriers per stage). The diagonal cell starts at the stage that holds its tile.
// Lane (li, kq) ends a 16-candidate tile with the dot products of candidate li against queries 4 kq .. 4 kq + 3:
//     cos = (dot * inv_lo) * inv_hi,    e = expf(two_t * (cos - 1))
// knn.hip's expression with inv_lo <= inv_hi the two rows' 1 / max(sqrt(sq), 1e-12) in ascending order: which of the two rows is the
// query must not reach the bits (the dot product itself does not care: its products commute and the k-loop runs 0, 4, 8, ... for
// every pair), so a list and its reverse differ by the order of the float64 additions alone. IEEE division, the accurate expf, no
// contraction: a pair's bits depend on the two rows, d and t alone. Every e of a pair of valid entries at positions p < q is widened and added to the lane's ONE
// float64 accumulator (r = 0 .. 3 within a tile, tiles in ascending position); the 256 accumulators of the workgroup are folded by
// a fixed tree in LDS into the cell's ONE float64 in the workspace. uniformity_reduce_kernel (one workgroup) adds the cells --
// thread t takes cells t, t + 256, ... in ascending order, then the same fixed tree -- and counts the valid entries (integers):
// S, pairs = n_valid (n_valid - 1) / 2 and n_valid. No floating-point atomics: the order of every addition is fixed by n and
// these constants, so two calls give the same bits whatever the grid's scheduling.
// LDS: 2 KiB (tree) + SR (d + 4) 4 + SR 4 bytes, SR = 64 rows at d = 32 / 64, 32 at d = 128, 16 for the general d, plus the
// lane-private A columns d x 256 B there: 19.3 KiB at d = 64, 82.3 KiB at d = 256 (one workgroup per CU there).
//
// gram_partial_kernel + gram_reduce_kernel: kmeans_update's scheme. The grid of the first is (segments of GEO_SEGMENT = 512
// consecutive list positions x the 64 x 64 tiles (bi <= bj) of the upper triangle of G). A workgroup stages 64 entries at a time
// as unit rows x * (1 / max(sqrt(sq), 1e-12)) formed in fp32 (the tile's two column blocks, 32 KiB; zeros for an entry that is
// not valid) and every thread adds its 4 x 4 products double(x_a) * double(x_b) -- exact in float64 -- entry by entry in list
// order. The diagonal tiles also sum their 64 columns of the rows (m), tile (0, 0) counts the valid entries. The partials go to
// the workspace [segments][d x d] + [segments][d] float64 + [segments] int32; the second launch adds them in ascending segment
// order per element a <= b and mirrors. Only the order of additions is fixed by the code; the products carry no rounding.
#include <cmath>
#include "common.h"
#include "cosine.h"
#include "dispatch.h"

namespace elimrec {

constexpr int GEO_TILE = 64, GEO_CHUNK = 2048, GEO_SEGMENT = 512;
constexpr int GEO_R = GEO_CHUNK / GEO_TILE;                  // tiles per chunk
constexpr int GEO_GB = 64;                                   // Gram: columns per tile side, entries per stage
constexpr double GEO_MAX_T = 8.0;
typedef float geo_v4f __attribute__((ext_vector_type(4)));

__host__ __device__ __forceinline__ bool geo_norm_ok(float sq) { return sq > 0.f && sq < __builtin_inff(); }     // (NaN fails both)

// the live cells before the first tile of chunk-row g (tiles 32 g .. 32 g + 31 meet the chunks g .. nc - 1)
__host__ __device__ __forceinline__ int64_t geo_cells_before(int64_t g, int64_t nc) { return GEO_R * (g * nc - g * (g - 1) / 2); }
static inline int64_t geo_tiles(int64_t n) { return (n + GEO_TILE - 1) / GEO_TILE; }
static inline int64_t geo_chunks(int64_t n) { return (n + GEO_CHUNK - 1) / GEO_CHUNK; }
static inline int64_t geo_live_cells(int64_t n) {
    const int64_t nt = geo_tiles(n), nc = geo_chunks(n), g = nt / GEO_R;
    return geo_cells_before(g, nc) + (nt - g * GEO_R) * (nc - g);
}

struct UniArgs {
    TableView t; int d, vec;
    const int32_t *rows; int64_t n;                          // the list
    float two_t;
    int64_t n_chunks, n_cells;
    double *ws;                                              // [n_cells]
    double *sum; int64_t *counts;                            // S; (pairs, n_valid)
};

constexpr int geo_stage_rows(int D) { return D == 0 ? 16 : (D <= 64 ? 64 : 32); }
// dynamic LDS of one workgroup, in bytes (host and device agree through this one function)
static inline size_t geo_lds_bytes(int D, int d) {
    const size_t sr = (size_t)geo_stage_rows(D);
    return 256 * sizeof(double) + sr * (d + 4) * 4 + sr * 4 + (D == 0 ? (size_t)4 * (d / 4) * 64 * 4 : 0);
}

// the id of list position p: -1 beyond the list or outside the table
__device__ __forceinline__ int64_t geo_row_id(const UniArgs &a, int64_t p) {
    int64_t r = p < a.n ? (int64_t)a.rows[p] : -1;
    if (r < 0 || r >= a.t.n_rows) r = -1;
    return r;
}

// s_red[0] <- the sum of the 256 threads' values by a fixed tree
__device__ __forceinline__ double geo_tree_sum(double *s_red, double v, int tid) {
    __syncthreads();
    s_red[tid] = v;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if (tid < w) s_red[tid] += s_red[tid + w];
        __syncthreads();
    }
    return s_red[0];
}

// D: 32 / 64 / 128 = the dimension at compile time, query operands in registers; 0 = any d % 4 == 0 up to TABLE_MAXD.
template <int D>
__global__ __launch_bounds__(256) void uniformity_cell_kernel(UniArgs a) {
    constexpr int SR = geo_stage_rows(D), NT = 256;
    constexpr int PFN = (SR * (D ? D : TABLE_MAXD) / 4 + NT - 1) / NT;
    const int d = D ? D : a.d, LD = d + 4;
    extern __shared__ double smem_d[];
    double *s_red = smem_d;                                  // [256]    the tree
    float *s_b = reinterpret_cast<float *>(smem_d + 256);    // [SR][LD] the stage's candidate rows
    float *s_invc = s_b + SR * LD;                           // [SR]     their reciprocal norms, -1 = not valid
    float *s_a = s_invc + SR;                                // D == 0: [4][d / 4][64] lane-private query operands
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, kq = lane >> 4;

    // the cell: tile-major over the live cells
    const int64_t cell = blockIdx.x, nc = a.n_chunks;
    int64_t g = 0;
    while (g + 1 < nc && cell >= geo_cells_before(g + 1, nc)) ++g;
    const int64_t within = cell - geo_cells_before(g, nc), live = nc - g;
    const int64_t tile = g * GEO_R + within / live, chunk = g + within % live;
    const int64_t tile0 = tile * GEO_TILE, q0 = tile0 + wave * 16;
    const int64_t c_end = (chunk + 1) * GEO_CHUNK < a.n ? (chunk + 1) * GEO_CHUNK : a.n;
    // the diagonal cell starts at the stage that holds its tile: every earlier candidate has q <= p for all of its queries
    const int64_t c_begin = chunk == g ? tile0 - tile0 % SR : chunk * GEO_CHUNK;

    // A operands: the row of position q0 + li, element k = 4 ks + kq; a position without a row in the table is all zeros
    float qa[D ? D / 4 : 1];
    {
        const int64_t qr = geo_row_id(a, q0 + li);
        const float *row = qr >= 0 ? a.t.T + qr * a.t.ld + kq : nullptr;
        if (D) {
#pragma unroll
            for (int ks = 0; ks < (D ? D / 4 : 1); ++ks) qa[ks] = row ? row[4 * ks] : 0.f;
        } else {
            for (int ks = 0; ks < d / 4; ++ks) s_a[(wave * (d / 4) + ks) * 64 + lane] = row ? row[4 * ks] : 0.f;
        }
    }
    // the four query positions this lane's accumulators belong to
    int64_t qpos[4];
    float invq[4];
    bool okq[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        qpos[r] = q0 + 4 * kq + r;
        const int64_t qr = geo_row_id(a, qpos[r]);
        const float sq = qr >= 0 ? a.t.sq[qr * a.t.ld_sq] : 0.f;
        okq[r] = geo_norm_ok(sq);
        invq[r] = okq[r] ? inv_norm(sq) : 0.f;
    }

    // a stage's rows as float4 over the workgroup, its squared norms on the first SR threads
    float4 pf[PFN];
    float sq_pf = 0.f;
    auto load_stage = [&](int64_t s0) {
#pragma unroll
        for (int p = 0; p < PFN; ++p) {
            const int e = (tid + NT * p) * 4;
            if (e < SR * d) {
                const int r = e / d, c = e - r * d;
                const int64_t id = s0 + r < c_end ? geo_row_id(a, s0 + r) : -1;
                float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
                if (id >= 0) ELIMREC_LOAD_ROW4(x, a.t.T + id * a.t.ld + c, a.vec);
                pf[p] = x;
            }
        }
        if (tid < SR) {
            const int64_t id = s0 + tid < c_end ? geo_row_id(a, s0 + tid) : -1;
            sq_pf = id >= 0 ? a.t.sq[id * a.t.ld_sq] : 0.f;
        }
    };
    auto store_stage = [&]() {
#pragma unroll
        for (int p = 0; p < PFN; ++p) {
            const int e = (tid + NT * p) * 4;
            if (e < SR * d) {
                const int r = e / d, c = e - r * d;
                *reinterpret_cast<float4 *>(s_b + r * LD + c) = pf[p];
            }
        }
        if (tid < SR) s_invc[tid] = geo_norm_ok(sq_pf) ? inv_norm(sq_pf) : -1.f;
    };

    double sum = 0.0;
    load_stage(c_begin);
    store_stage();
    __syncthreads();
    for (int64_t s0 = c_begin; s0 < c_end; s0 += SR) {
        const bool more = s0 + SR < c_end;                   // workgroup-uniform
        if (more) load_stage(s0 + SR);
#pragma unroll 1
        for (int t = 0; t < SR / 16; ++t) {
            const int64_t t0 = s0 + 16 * t;
            if (t0 >= c_end) break;                          // workgroup-uniform
            if (t0 + 15 <= q0) continue;                     // wave-uniform: no candidate of the tile lies behind a query of this wave
            geo_v4f acc = (geo_v4f){0.f, 0.f, 0.f, 0.f};
            const float *bp = s_b + (16 * t + li) * LD + kq;
            if (D) {
#pragma unroll
                for (int ks = 0; ks < (D ? D / 4 : 1); ++ks) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[ks], bp[4 * ks], acc, 0, 0, 0);
            } else {
                const float *ap = s_a + wave * (d / 4) * 64 + lane;
                for (int ks = 0; ks < d / 4; ++ks) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[ks * 64], bp[4 * ks], acc, 0, 0, 0);
            }
            // lane: the candidate at position t0 + li against the queries at positions q0 + 4 kq + r
            const int64_t cand = t0 + li;
            const float invc = s_invc[16 * t + li];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float s = (acc[r] * fminf(invq[r], invc)) * fmaxf(invq[r], invc);
                const float e = expf(a.two_t * (s - 1.f));
                if (okq[r] && invc > 0.f && qpos[r] < cand) sum += (double)e;
            }
        }
        __syncthreads();                                     // every wave is done with the stage
        if (more) store_stage();
        __syncthreads();
    }
    const double total = geo_tree_sum(s_red, sum, tid);
    if (tid == 0) a.ws[cell] = total;
}

__global__ __launch_bounds__(256) void uniformity_reduce_kernel(UniArgs a) {
    __shared__ double s_red[256];
    __shared__ unsigned long long s_cnt;
    const int tid = threadIdx.x;
    if (tid == 0) s_cnt = 0ull;
    double s = 0.0;
    for (int64_t c = tid; c < a.n_cells; c += 256) s += a.ws[c];
    unsigned long long nv = 0;
    for (int64_t p = tid; p < a.n; p += 256) {
        const int64_t id = geo_row_id(a, p);
        if (id >= 0 && geo_norm_ok(a.t.sq[id * a.t.ld_sq])) ++nv;
    }
    const double total = geo_tree_sum(s_red, s, tid);       // (its first barrier publishes s_cnt = 0)
    atomicAdd(&s_cnt, nv);                                   // integers: exact in any order
    __syncthreads();
    if (tid == 0) {
        const int64_t n_valid = (int64_t)s_cnt;
        a.sum[0] = total;
        a.counts[0] = n_valid * (n_valid - 1) / 2;
        a.counts[1] = n_valid;
    }
}

struct GramArgs {
    TableView t; int d, vec, nb;                             // nb: 64-column blocks of d
    const int32_t *rows; int64_t n, n_seg;
    double *ws_g, *ws_m; int32_t *ws_cnt;                    // [n_seg][d x d], [n_seg][d], [n_seg]
    double *gram, *sum; int64_t *count;
};

__global__ __launch_bounds__(256) void gram_partial_kernel(GramArgs a) {
    __shared__ float s_x[2][GEO_GB][GEO_GB];                 // the stage's unit rows: columns of block bi, of block bj
    const int tid = threadIdx.x, d = a.d;
    // blockIdx.y -> the tile (bi <= bj) of the upper triangle, row-major
    int bi = 0, bj = blockIdx.y;
    while (bj >= a.nb - bi) { bj -= a.nb - bi; ++bi; }
    bj += bi;
    const int64_t seg = blockIdx.x, p0 = seg * GEO_SEGMENT;
    const int rows = (int)(a.n - p0 < GEO_SEGMENT ? a.n - p0 : GEO_SEGMENT);
    const int ty = tid >> 4, tx = tid & 15;                  // the thread's 4 x 4 elements: rows 4 ty + i of bi, columns 4 tx + j of bj
    const int sr = tid >> 2, sq4 = tid & 3;                  // staging: entry sr of the stage, columns 16 sq4 .. 16 sq4 + 15 of both blocks
    double acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
    double m = 0.0;
    int cnt = 0;
    for (int b0 = 0; b0 < rows; b0 += GEO_GB) {
        __syncthreads();                                     // the last stage is consumed
        int64_t id = -1;
        float inv = 0.f;
        if (b0 + sr < rows) {
            id = (int64_t)a.rows[p0 + b0 + sr];
            if (id < 0 || id >= a.t.n_rows) id = -1;
            if (id >= 0) {
                const float sq = a.t.sq[id * a.t.ld_sq];
                if (geo_norm_ok(sq)) inv = inv_norm(sq); else id = -1;
            }
        }
#pragma unroll
        for (int side = 0; side < 2; ++side) {
            const int c0 = (side ? bj : bi) * GEO_GB + 16 * sq4;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
                if (id >= 0 && c0 + 4 * q < d) ELIMREC_LOAD_ROW4(x, a.t.T + id * a.t.ld + c0 + 4 * q, a.vec);
                *reinterpret_cast<float4 *>(&s_x[side][sr][16 * sq4 + 4 * q]) = make_float4(x.x * inv, x.y * inv, x.z * inv, x.w * inv);
            }
        }
        cnt += __syncthreads_count(id >= 0 && sq4 == 0);    // (a barrier: the stage is written)
        const int nrow = rows - b0 < GEO_GB ? rows - b0 : GEO_GB;
        for (int r = 0; r < nrow; ++r) {
            const float4 xa = *reinterpret_cast<const float4 *>(&s_x[0][r][4 * ty]);
            const float4 xb = *reinterpret_cast<const float4 *>(&s_x[1][r][4 * tx]);
            const double va[4] = {(double)xa.x, (double)xa.y, (double)xa.z, (double)xa.w};
            const double vb[4] = {(double)xb.x, (double)xb.y, (double)xb.z, (double)xb.w};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] += va[i] * vb[j];
        }
        if (bi == bj && tid < GEO_GB)
            for (int r = 0; r < nrow; ++r) m += (double)s_x[0][r][tid];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int ra = bi * GEO_GB + 4 * ty + i;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int cb = bj * GEO_GB + 4 * tx + j;
            if (ra < d && cb < d) a.ws_g[(seg * d + ra) * d + cb] = acc[i][j];
        }
    }
    if (bi == bj && tid < GEO_GB && bi * GEO_GB + tid < d) a.ws_m[seg * d + bi * GEO_GB + tid] = m;
    if (blockIdx.y == 0 && tid == 0) a.ws_cnt[seg] = cnt;
}

// element e of [d x d] (a <= b: summed, written to both halves), then the d elements of m, then the count
__global__ __launch_bounds__(256) void gram_reduce_kernel(GramArgs a) {
    const int d = a.d;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x, dd = (int64_t)d * d;
    if (e < dd) {
        const int ra = (int)(e / d), cb = (int)(e - (int64_t)ra * d);
        if (ra > cb) return;
        double s = 0.0;
        for (int64_t seg = 0; seg < a.n_seg; ++seg) s += a.ws_g[(seg * d + ra) * d + cb];
        a.gram[(int64_t)ra * d + cb] = s;
        a.gram[(int64_t)cb * d + ra] = s;
    } else if (e < dd + d) {
        const int c = (int)(e - dd);
        double s = 0.0;
        for (int64_t seg = 0; seg < a.n_seg; ++seg) s += a.ws_m[seg * d + c];
        a.sum[c] = s;
    } else if (e == dd + d) {
        int64_t cnt = 0;
        for (int64_t seg = 0; seg < a.n_seg; ++seg) cnt += a.ws_cnt[seg];
        a.count[0] = cnt;
    }
}

static inline int64_t geo_segments(int64_t n) { return (n + GEO_SEGMENT - 1) / GEO_SEGMENT; }
static inline bool geo_dims_ok(int64_t n, int d) { return n >= 0 && n < (int64_t)INT32_MAX - GEO_CHUNK && d >= 4 && d <= TABLE_MAXD && d % 4 == 0; }
static inline size_t geo_uniformity_workspace(int64_t n) { return align_up((size_t)(n > 0 ? geo_live_cells(n) : 1) * sizeof(double), 16); }
static inline size_t geo_gram_workspace(int64_t n, int d) {
    const size_t segs = (size_t)(n > 0 ? geo_segments(n) : 1);
    return align_up(segs * ((size_t)d * d + d) * sizeof(double) + segs * sizeof(int32_t), 16);
}

// the checks both entry points share; after them the table, the list and d are in range
static int geo_dims(const char *who, int64_t n_rows, int d, int64_t ld, int64_t ld_sq, int64_t n) {
    if (int rc = table_dims(who, d, 1)) return rc;
    ELIMREC_REQUIRE(n_rows >= 0 && n_rows < (int64_t)INT32_MAX, "%s: need 0 <= n_rows < 2^31 - 1", who);
    ELIMREC_REQUIRE(n >= 0 && n < (int64_t)INT32_MAX - GEO_CHUNK, "%s: need 0 <= n < 2^31 - %d list entries", who, GEO_CHUNK + 1);
    ELIMREC_REQUIRE(ld >= d && ld_sq >= 1, "%s: ld < d or ld_sq < 1", who);
    return 0;
}

template <int D>
static int uniformity_launch(const UniArgs &a, hipStream_t s) {
    const size_t lds = geo_lds_bytes(D, a.d);
    if (D == 0) allow_lds<uniformity_cell_kernel<D>>(geo_lds_bytes(0, TABLE_MAXD));      // latched once: the largest d
    hipLaunchKernelGGL(uniformity_cell_kernel<D>, dim3((unsigned)a.n_cells), dim3(256), lds, s, a);
    ELIMREC_LAUNCH_CHECK("uniformity_sum");
    return 0;
}

// d -> the kernel's D: 32 / 64 / 128 in registers, 0 = the general form
template <class F> static int with_geo_dim(int d, F f) {
    switch (d) {
    case 32: return f(int_c<32>{});
    case 64: return f(int_c<64>{});
    case 128: return f(int_c<128>{});
    default: return f(int_c<0>{});
    }
}

}  // namespace elimrec

using namespace elimrec;

extern "C" int elimrec_geometry_tile(void) { return GEO_TILE; }
extern "C" int elimrec_geometry_chunk(void) { return GEO_CHUNK; }
extern "C" int elimrec_geometry_segment(void) { return GEO_SEGMENT; }

extern "C" size_t elimrec_uniformity_workspace(int64_t n, int d) { return geo_dims_ok(n, d) ? geo_uniformity_workspace(n) : 0; }
extern "C" size_t elimrec_gram_workspace(int64_t n, int d) { return geo_dims_ok(n, d) ? geo_gram_workspace(n, d) : 0; }

extern "C" int elimrec_uniformity_sum(const float *d_T, int64_t ld, int64_t n_rows, int d, const float *d_sqnorm, int64_t ld_sq,
                                      const int32_t *d_rows, int64_t n, double t, double *d_sum, int64_t *d_counts, void *d_workspace,
                                      size_t workspace_bytes, void *stream) {
    if (int rc = geo_dims("uniformity_sum", n_rows, d, ld, ld_sq, n)) return rc;
    ELIMREC_REQUIRE(t > 0.0 && t <= GEO_MAX_T, "uniformity_sum: 0 < t <= %g, got %g", GEO_MAX_T, t);
    ELIMREC_REQUIRE(d_sum && d_counts, "uniformity_sum: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (n == 0 || n_rows == 0) {                             // no valid entry
        if (int rc = check_hip(hipMemsetAsync(d_sum, 0, sizeof(double), s), "uniformity_sum (empty)")) return rc;
        return check_hip(hipMemsetAsync(d_counts, 0, 2 * sizeof(int64_t), s), "uniformity_sum (empty)");
    }
    UniArgs a;
    if (int rc = table_view("uniformity_sum", d_T, ld, n_rows, d_sqnorm, ld_sq, &a.t, &a.vec)) return rc;
    ELIMREC_REQUIRE(d_rows && d_workspace, "uniformity_sum: null pointer");
    ELIMREC_REQUIRE(workspace_bytes >= geo_uniformity_workspace(n) && reinterpret_cast<uintptr_t>(d_workspace) % 16 == 0,
                    "uniformity_sum: the workspace needs %zu bytes, 16-byte aligned (got %zu)", geo_uniformity_workspace(n), workspace_bytes);
    a.d = d; a.rows = d_rows; a.n = n; a.two_t = (float)(2.0 * t);
    a.n_chunks = geo_chunks(n); a.n_cells = geo_live_cells(n);
    ELIMREC_REQUIRE(a.n_cells < (int64_t)INT32_MAX, "uniformity_sum: too many cells for one launch");
    a.ws = static_cast<double *>(d_workspace); a.sum = d_sum; a.counts = d_counts;
    if (int rc = with_geo_dim(d, [&](auto D) { return uniformity_launch<decltype(D)::value>(a, s); })) return rc;
    hipLaunchKernelGGL(uniformity_reduce_kernel, dim3(1), dim3(256), 0, s, a);
    ELIMREC_LAUNCH_CHECK("uniformity_sum");
    return 0;
}

extern "C" int elimrec_gram_f64(const float *d_T, int64_t ld, int64_t n_rows, int d, const float *d_sqnorm, int64_t ld_sq,
                                const int32_t *d_rows, int64_t n, double *d_gram, double *d_sum, int64_t *d_count, void *d_workspace,
                                size_t workspace_bytes, void *stream) {
    if (int rc = geo_dims("gram_f64", n_rows, d, ld, ld_sq, n)) return rc;
    ELIMREC_REQUIRE(d_gram && d_sum && d_count, "gram_f64: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (n == 0 || n_rows == 0) {                             // no valid entry
        if (int rc = check_hip(hipMemsetAsync(d_gram, 0, (size_t)d * d * sizeof(double), s), "gram_f64 (empty)")) return rc;
        if (int rc = check_hip(hipMemsetAsync(d_sum, 0, (size_t)d * sizeof(double), s), "gram_f64 (empty)")) return rc;
        return check_hip(hipMemsetAsync(d_count, 0, sizeof(int64_t), s), "gram_f64 (empty)");
    }
    GramArgs a;
    if (int rc = table_view("gram_f64", d_T, ld, n_rows, d_sqnorm, ld_sq, &a.t, &a.vec)) return rc;
    ELIMREC_REQUIRE(d_rows && d_workspace, "gram_f64: null pointer");
    ELIMREC_REQUIRE(workspace_bytes >= geo_gram_workspace(n, d) && reinterpret_cast<uintptr_t>(d_workspace) % 16 == 0,
                    "gram_f64: the workspace needs %zu bytes, 16-byte aligned (got %zu)", geo_gram_workspace(n, d), workspace_bytes);
    a.d = d; a.nb = (d + GEO_GB - 1) / GEO_GB; a.rows = d_rows; a.n = n; a.n_seg = geo_segments(n);
    a.ws_g = static_cast<double *>(d_workspace);
    a.ws_m = a.ws_g + a.n_seg * d * d;
    a.ws_cnt = reinterpret_cast<int32_t *>(a.ws_m + a.n_seg * d);
    a.gram = d_gram; a.sum = d_sum; a.count = d_count;
    hipLaunchKernelGGL(gram_partial_kernel, dim3((unsigned)a.n_seg, (unsigned)(a.nb * (a.nb + 1) / 2)), dim3(256), 0, s, a);
    ELIMREC_LAUNCH_CHECK("gram_f64");
    hipLaunchKernelGGL(gram_reduce_kernel, dim3((unsigned)(((int64_t)d * d + d + 1 + 255) / 256)), dim3(256), 0, s, a);
    ELIMREC_LAUNCH_CHECK("gram_f64");
    return 0;
}
