// Spherical k-means over one block of a cached table (content clusters): the assignment of every row to the centroid with the
// largest cosine, and the new centroids as the normalised float64 sums of the members' unit rows. Lloyd's loop itself is the
// host's (ops.spherical_kmeans): one assign + one update per iteration, one int32 read back.
//
// kmeans_assign_kernel: a workgroup of 4 waves owns a tile of KM_TILE = 64 table rows, staged once in LDS (row stride d + 4
// floats, filled by 16-byte loads where table_vec allows them; rows outside the table are zeros and never read). A wave owns 16 of
// them as the A operands of v_mfma_f32_16x16x4_f32 (registers at d = 64, read from the staged tile otherwise). The C centroids
// go through ONE LDS stage of KM_CHUNK = 32 rows in ascending id order (two barriers per chunk; the centroids are at most 256 KiB
// and stay in L2): every wave multiplies both 16-centroid tiles of the stage against its rows, lane (li, kq) ends with the dot
// products of centroid t0 + li against rows 4 kq .. 4 kq + 3 and keeps a running (best, id) per row with a strict >:
//     score = (dot * (1 / max(sqrt(sq_row), 1e-12))) * (1 / max(sqrt(sq_centroid), 1e-12))
// as knn.hip forms it. A lane meets its centroids in ascending id, and the 16 lanes of a row are folded by an xor butterfly on
// (score descending, id ascending): the lowest id wins among equal cosines. The k-loop runs 0, 4, 8, ... for every pair, so a
// row's (assign, cos) depends bit for bit on the row, the centroids, d and C -- not on n, its place in the tile, or the grid.
// A row whose squared norm is 0 or not finite gets -1 / -inf; a centroid whose squared norm is 0 or not finite is never chosen.
// `changed` counts the rows whose assignment differs from prev (every row without prev): one integer atomicAdd per wave.
// LDS: (64 + 32) (d + 4) 4 + 128 bytes: 25.6 KiB at d = 64, 97.6 KiB at d = 256 (one workgroup per CU there).
//
// kmeans_partial_kernel + kmeans_reduce_kernel: the grid of the first is (segments of KMEANS_SEGMENT = 512 consecutive table rows
// x column slices). A workgroup keeps an accumulator [C x slice] of doubles in LDS (slice = 64 / 32 / 16 columns for C <= 64 /
// 128 / 256: 32 KiB); thread (g, col) owns column col of the clusters c with c % G == g, G = 256 / slice, so every element has ONE
// owner and the walk needs no barrier. The segment's assignments and reciprocal norms are staged in LDS, then every thread walks
// the segment in row order and the owner adds double(x * inv_norm(sq)) -- the unit row's component formed in fp32, as the
// assignment sees it -- to its element: members in ascending row order. An assignment outside [0, C), or a row whose squared norm
// is 0 or not finite, is skipped and its row never read. The partial [C x d] and the member counts go to the workspace
// [segments][C][d] float64 + [segments][C] int32. The second launch (one workgroup per cluster, thread = column) adds the
// partials in ascending segment order, forms |sum|^2 by a fixed tree over the 256 threads, and writes centroid = float(sum / |sum|)
// and its squared norm (the float64 tree sum of the rounded components, rounded once). A cluster without a member, or whose sum
// has norm 0 (or not finite), keeps its centroid and squared norm. No floating-point atomics: the bits depend on the table, the
// assignment, d and C only.
#include <cmath>
#include "common.h"
#include "cosine.h"

namespace elimrec {

constexpr int KMEANS_MAX_CLUSTERS = 256, KMEANS_SEGMENT = 512;
constexpr int KM_TILE = 64, KM_CHUNK = 32, KM_ACC = 4096;    // KM_ACC: doubles of the update's LDS accumulator
typedef float km_v4f __attribute__((ext_vector_type(4)));

struct KmAssignArgs {
    TableView t; int d, vec;
    const float *cen, *csq; int C, cvec;
    const int32_t *prev; int32_t *assign; float *cos; int32_t *changed;
};

__device__ __forceinline__ bool km_norm_ok(float sq) { return sq > 0.f && sq < __builtin_inff(); }     // (NaN fails both)

static inline size_t km_assign_lds(int d) { return (size_t)(KM_TILE + KM_CHUNK) * (d + 4) * 4 + KM_CHUNK * 4; }

// D: 64 = the dimension at compile time, row operands in registers; 0 = any d % 4 == 0 up to TABLE_MAXD.
template <int D>
__global__ __launch_bounds__(256) void kmeans_assign_kernel(KmAssignArgs a) {
    const int d = D ? D : a.d, LD = d + 4, C = a.C;
    extern __shared__ float smem[];
    float *s_x = smem;                                       // [KM_TILE][LD]  the tile's rows
    float *s_c = s_x + KM_TILE * LD;                         // [KM_CHUNK][LD] the stage's centroids
    float *s_invc = s_c + KM_CHUNK * LD;                     // [KM_CHUNK]     their reciprocal norms, -1 = never chosen
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, kq = lane >> 4;
    const int64_t n = a.t.n_rows;
    const int64_t tile0 = (int64_t)blockIdx.x * KM_TILE, q0 = tile0 + wave * 16;

    for (int e = tid * 4; e < KM_TILE * d; e += 1024) {
        const int r = e / d, c = e - r * d;
        float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
        if (tile0 + r < n) ELIMREC_LOAD_ROW4(x, a.t.T + (tile0 + r) * a.t.ld + c, a.vec);
        *reinterpret_cast<float4 *>(s_x + r * LD + c) = x;
    }
    // the four rows this lane's accumulators belong to
    bool ok[4];
    float invq[4], best[4];
    int bid[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t row = q0 + 4 * kq + r;
        const float sq = row < n ? a.t.sq[row * a.t.ld_sq] : 0.f;
        ok[r] = km_norm_ok(sq);
        invq[r] = ok[r] ? inv_norm(sq) : 0.f;
        best[r] = -__builtin_inff();
        bid[r] = -1;
    }
    float qa[D ? D / 4 : 1];
    const float *ap = s_x + (wave * 16 + li) * LD + kq;
    if (D) {
        __syncthreads();                                     // the tile is staged
#pragma unroll
        for (int ks = 0; ks < (D ? D / 4 : 1); ++ks) qa[ks] = ap[4 * ks];
    }

    for (int c0 = 0; c0 < C; c0 += KM_CHUNK) {
        __syncthreads();                                     // every wave is done with the last stage (first pass: the tile is staged)
        for (int e = tid * 4; e < KM_CHUNK * d; e += 1024) {
            const int j = e / d, c = e - j * d;
            float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
            if (c0 + j < C) ELIMREC_LOAD_ROW4(x, a.cen + (int64_t)(c0 + j) * d + c, a.cvec);
            *reinterpret_cast<float4 *>(s_c + j * LD + c) = x;
        }
        if (tid < KM_CHUNK) {
            const float sq = c0 + tid < C ? a.csq[c0 + tid] : 0.f;
            s_invc[tid] = km_norm_ok(sq) ? inv_norm(sq) : -1.f;
        }
        __syncthreads();
#pragma unroll 1
        for (int t = 0; t < KM_CHUNK / 16; ++t) {
            const int t0 = c0 + 16 * t;
            if (t0 >= C) break;                              // workgroup-uniform
            km_v4f acc = (km_v4f){0.f, 0.f, 0.f, 0.f};
            const float *bp = s_c + (16 * t + li) * LD + kq;
            if (D) {
#pragma unroll
                for (int ks = 0; ks < (D ? D / 4 : 1); ++ks) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[ks], bp[4 * ks], acc, 0, 0, 0);
            } else {
                for (int ks = 0; ks < d / 4; ++ks) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[4 * ks], bp[4 * ks], acc, 0, 0, 0);
            }
            // lane: centroid t0 + li against rows 4 kq + r of this wave
            const float invc = s_invc[16 * t + li];
            if (invc > 0.f) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float s = (acc[r] * invq[r]) * invc;
                    if (ok[r] && s > best[r]) { best[r] = s; bid[r] = t0 + li; }
                }
            }
        }
    }
    // the 16 lanes of a row: the largest score, the lowest id among equals (-1 = none, the largest id as unsigned)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int m = 8; m >= 1; m >>= 1) {
            const float os = __shfl_xor(best[r], m, 16);
            const int oi = __shfl_xor(bid[r], m, 16);
            if (os > best[r] || (os == best[r] && (unsigned)oi < (unsigned)bid[r])) { best[r] = os; bid[r] = oi; }
        }
    }
    // lane li < 4 of every 16 writes row 4 kq + li
    float bs = best[0];
    int bi = bid[0];
    if (li == 1) { bs = best[1]; bi = bid[1]; }
    if (li == 2) { bs = best[2]; bi = bid[2]; }
    if (li == 3) { bs = best[3]; bi = bid[3]; }
    const int64_t row = q0 + 4 * kq + li;
    bool chg = false;
    if (li < 4 && row < n) {
        a.assign[row] = bi;
        if (a.cos) a.cos[row] = bs;
        chg = a.prev ? a.prev[row] != bi : true;
    }
    const unsigned long long m = __ballot(chg);
    if (lane == 0 && m) atomicAdd(a.changed, __popcll(m));
}

struct KmUpdateArgs {
    TableView t; int d;
    const int32_t *assign; int C, slice;
    double *ws_sum; int32_t *ws_cnt;                         // [segments][C][d], [segments][C]
};

__global__ __launch_bounds__(256) void kmeans_partial_kernel(KmUpdateArgs a) {
    __shared__ double s_acc[KM_ACC];                         // [C][slice]
    __shared__ int s_a[KMEANS_SEGMENT];                      // checked assignments, -1 = skipped
    __shared__ float s_inv[KMEANS_SEGMENT];
    __shared__ int s_cnt[KMEANS_MAX_CLUSTERS];
    const int tid = threadIdx.x, C = a.C, slice = a.slice, d = a.d, G = 256 / slice;
    const int col = tid % slice, g = tid / slice;
    const int64_t seg = blockIdx.x, r0 = seg * KMEANS_SEGMENT;
    const int rows = (int)(a.t.n_rows - r0 < KMEANS_SEGMENT ? a.t.n_rows - r0 : KMEANS_SEGMENT);
    const int c_lo = blockIdx.y * slice + col;
    for (int e = tid; e < C * slice; e += 256) s_acc[e] = 0.0;
    for (int e = tid; e < C; e += 256) s_cnt[e] = 0;
    for (int i = tid; i < rows; i += 256) {
        int c = a.assign[r0 + i];
        float inv = 0.f;
        if (c >= 0 && c < C) {
            const float sq = a.t.sq[(r0 + i) * a.t.ld_sq];
            if (km_norm_ok(sq)) inv = inv_norm(sq); else c = -1;
        } else {
            c = -1;
        }
        s_a[i] = c;
        s_inv[i] = inv;
    }
    __syncthreads();
    const float *src = a.t.T + r0 * a.t.ld + c_lo;
    if (c_lo < d) {
        for (int i = 0; i < rows; ++i) {
            const int c = s_a[i];
            if (c >= 0 && c % G == g) {                      // this thread owns (c, col)
                s_acc[c * slice + col] += (double)(src[(int64_t)i * a.t.ld] * s_inv[i]);
                if (col == 0) s_cnt[c] += 1;
            }
        }
    }
    __syncthreads();
    for (int e = tid; e < C * slice; e += 256) {
        const int c = e / slice, k = blockIdx.y * slice + (e - c * slice);
        if (k < d) a.ws_sum[(seg * C + c) * d + k] = s_acc[e];
    }
    if (blockIdx.y == 0)
        for (int e = tid; e < C; e += 256) a.ws_cnt[seg * C + e] = s_cnt[e];
}

struct KmReduceArgs {
    const double *ws_sum; const int32_t *ws_cnt; int64_t n_seg; int d, C;
    float *cen, *csq; double *sums; int32_t *counts;
};

// s_red[0] <- the sum of the 256 threads' values by a fixed tree
__device__ __forceinline__ double km_tree_sum(double *s_red, double v, int tid) {
    __syncthreads();                                         // the last sum is read
    s_red[tid] = v;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if (tid < w) s_red[tid] += s_red[tid + w];
        __syncthreads();
    }
    return s_red[0];
}

__global__ __launch_bounds__(256) void kmeans_reduce_kernel(KmReduceArgs a) {
    __shared__ double s_red[256];
    __shared__ int s_count;
    const int tid = threadIdx.x, c = blockIdx.x, d = a.d, C = a.C;
    double s = 0.0;
    if (tid < d)
        for (int64_t seg = 0; seg < a.n_seg; ++seg) s += a.ws_sum[(seg * C + c) * d + tid];
    if (tid == 0) {
        int cnt = 0;
        for (int64_t seg = 0; seg < a.n_seg; ++seg) cnt += a.ws_cnt[seg * C + c];
        s_count = cnt;
        if (a.counts) a.counts[c] = cnt;
    }
    if (a.sums && tid < d) a.sums[(int64_t)c * d + tid] = s;
    const double norm2 = km_tree_sum(s_red, tid < d ? s * s : 0.0, tid);
    if (s_count <= 0 || !(norm2 > 0.0 && norm2 < (double)__builtin_inff())) return;      // (uniform) keeps its centroid
    const double norm = sqrt(norm2);
    float f = 0.f;
    if (tid < d) {
        f = (float)(s / norm);
        a.cen[(int64_t)c * d + tid] = f;
    }
    const double sq = km_tree_sum(s_red, (double)f * (double)f, tid);
    if (tid == 0) a.csq[c] = (float)sq;
}

static inline int km_slice(int C) { return C <= 64 ? 64 : (C <= 128 ? 32 : 16); }
static inline int64_t km_segments(int64_t n) { return (n + KMEANS_SEGMENT - 1) / KMEANS_SEGMENT; }
static inline size_t km_workspace(int64_t n, int d, int C) {
    const size_t cells = (size_t)km_segments(n) * (size_t)C;
    return align_up(cells * (size_t)d * sizeof(double) + cells * sizeof(int32_t), 16);
}

// the checks both entry points share; after them n_rows, d and C are in range
static int km_dims(const char *who, int64_t n_rows, int d, int64_t ld, int64_t ld_sq, int C) {
    if (int rc = table_dims(who, d, 1)) return rc;
    ELIMREC_REQUIRE(C >= 1 && C <= KMEANS_MAX_CLUSTERS, "%s: 1 <= C <= %d, got %d", who, KMEANS_MAX_CLUSTERS, C);
    ELIMREC_REQUIRE(n_rows >= 0 && n_rows < (int64_t)INT32_MAX - KMEANS_SEGMENT, "%s: need 0 <= n_rows < 2^31 - %d", who, KMEANS_SEGMENT + 1);
    ELIMREC_REQUIRE(ld >= d && ld_sq >= 1, "%s: ld < d or ld_sq < 1", who);
    return 0;
}

}  // namespace elimrec

using namespace elimrec;

extern "C" int elimrec_kmeans_max_clusters(void) { return KMEANS_MAX_CLUSTERS; }
extern "C" int elimrec_kmeans_segment(void) { return KMEANS_SEGMENT; }

extern "C" size_t elimrec_kmeans_workspace(int64_t n_rows, int d, int C) {
    if (n_rows < 0 || n_rows >= (int64_t)INT32_MAX - KMEANS_SEGMENT || d < 4 || d > TABLE_MAXD || C < 1 || C > KMEANS_MAX_CLUSTERS) return 0;
    return km_workspace(n_rows, d, C);
}

extern "C" int elimrec_kmeans_assign(const float *d_T, int64_t ld, int64_t n_rows, int d, const float *d_sqnorm, int64_t ld_sq,
                                     const float *d_centroids, const float *d_centroid_sqnorm, int C, const int32_t *d_prev,
                                     int32_t *d_assign, float *d_cos, int32_t *d_changed, void *stream) {
    if (int rc = km_dims("kmeans_assign", n_rows, d, ld, ld_sq, C)) return rc;
    if (n_rows == 0) return 0;
    KmAssignArgs a;
    if (int rc = table_view("kmeans_assign", d_T, ld, n_rows, d_sqnorm, ld_sq, &a.t, &a.vec)) return rc;
    ELIMREC_REQUIRE(d_centroids && d_centroid_sqnorm && d_assign && d_changed, "kmeans_assign: null pointer");
    a.d = d;
    a.cen = d_centroids; a.csq = d_centroid_sqnorm; a.C = C; a.cvec = table_vec(d_centroids, d);
    a.prev = d_prev; a.assign = d_assign; a.cos = d_cos; a.changed = d_changed;
    hipStream_t s = (hipStream_t)stream;
    if (int rc = check_hip(hipMemsetAsync(d_changed, 0, sizeof(int32_t), s), "kmeans_assign (changed)")) return rc;
    const size_t lds = km_assign_lds(d);
    const unsigned tiles = (unsigned)((n_rows + KM_TILE - 1) / KM_TILE);
    void (*kernel)(KmAssignArgs) = d == 64 ? kmeans_assign_kernel<64> : kmeans_assign_kernel<0>;
    if (lds > 64 * 1024) {
        if (int rc = check_hip(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds),
                               "kmeans_assign (LDS)"))
            return rc;
    }
    hipLaunchKernelGGL(kernel, dim3(tiles), dim3(256), lds, s, a);
    ELIMREC_LAUNCH_CHECK("kmeans_assign");
    return 0;
}

extern "C" int elimrec_kmeans_update(const float *d_T, int64_t ld, int64_t n_rows, int d, const float *d_sqnorm, int64_t ld_sq,
                                     const int32_t *d_assign, int C, float *d_centroids, float *d_centroid_sqnorm, double *d_sums,
                                     int32_t *d_counts, void *d_workspace, size_t workspace_bytes, void *stream) {
    if (int rc = km_dims("kmeans_update", n_rows, d, ld, ld_sq, C)) return rc;
    if (n_rows == 0) return 0;                               // no member anywhere: every cluster keeps its centroid
    KmUpdateArgs a;
    int vec;
    if (int rc = table_view("kmeans_update", d_T, ld, n_rows, d_sqnorm, ld_sq, &a.t, &vec)) return rc;
    ELIMREC_REQUIRE(d_assign && d_centroids && d_centroid_sqnorm && d_workspace, "kmeans_update: null pointer");
    ELIMREC_REQUIRE(workspace_bytes >= km_workspace(n_rows, d, C) && reinterpret_cast<uintptr_t>(d_workspace) % 16 == 0,
                    "kmeans_update: the workspace needs %zu bytes, 16-byte aligned (got %zu)", km_workspace(n_rows, d, C), workspace_bytes);
    const int64_t n_seg = km_segments(n_rows);
    a.d = d; a.assign = d_assign; a.C = C; a.slice = km_slice(C);
    a.ws_sum = static_cast<double *>(d_workspace);
    a.ws_cnt = reinterpret_cast<int32_t *>(a.ws_sum + n_seg * C * d);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(kmeans_partial_kernel, dim3((unsigned)n_seg, (unsigned)((d + a.slice - 1) / a.slice)), dim3(256), 0, s, a);
    ELIMREC_LAUNCH_CHECK("kmeans_update");
    KmReduceArgs r;
    r.ws_sum = a.ws_sum; r.ws_cnt = a.ws_cnt; r.n_seg = n_seg; r.d = d; r.C = C;
    r.cen = d_centroids; r.csq = d_centroid_sqnorm; r.sums = d_sums; r.counts = d_counts;
    hipLaunchKernelGGL(kmeans_reduce_kernel, dim3((unsigned)C), dim3(256), 0, s, r);
    ELIMREC_LAUNCH_CHECK("kmeans_update");
    return 0;
}
