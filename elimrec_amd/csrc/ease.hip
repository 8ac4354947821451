// EASE^R (Steck, "Embarrassingly Shallow Autoencoders for Sparse Data", WWW 2019): the closed-form item-item model
//     G = X^T X + l2 I,   P = G^-1,   B_ij = -P_ij / P_jj (i != j),   score_j(H) = -(sum_{i in H, i != j} P_ij) / P_jj
// in three entry points: the Gram matrix from the training graph, a dense symmetric positive definite inverse, and the top-K
// over "sum of the history's rows of P" scores. Everything is float64 up to the one rounding of a score to float32.
//
// gram_counts_kernel: ONE workgroup per item row i. The row of `out` is its own stage: its 8-byte slots are zeroed, count the
// walks i -> u -> j with 64-bit INTEGER atomics (wave per user u of i's list, lane per item j of u's list; only this workgroup
// touches the row), and are converted in place to double, + l2 on the diagonal. Integer counts: exact, whatever the geometry.
//
// spd_inverse: the symmetric block sweep, block width EASE_NB = 64. With D = A_kk, R = A_k,: and W = D^-1 R pivot block k does
//     A <- A - R^T W,   A_k,: <- W,   A_:,k <- W^T,   A_kk <- -D^-1
// and after the last block A = -G^-1. Three launches per pivot block:
//   spd_pivot_kernel  one workgroup: D into LDS, the square-root-free Cholesky D = L Delta L^T (als.hip's right-looking loop
//       without the root: a cold item's pivot is l2 itself and its row of the inverse comes out as e_j / l2 EXACTLY, which
//       (1 / sqrt l2)^2 would not), M = L^-1 by forward substitution (thread c its column c, kept in the unused upper triangle),
//       D^-1_ab = sum_{m >= b} M_ma (M_mb / Delta_m) in ascending m for a <= b, mirrored. A pivot <= 0 or not finite: status[0]
//       += 1, status[1] = min(status[1], its index), and every later launch of the call returns at once (A is left half swept;
//       nothing is read or written out of bounds whatever the values are). The smallest pivot seen goes to *pivot_min.
//   spd_panel_kernel  one workgroup per column block j != k: R_j (from the upper triangle: tile (k, j), or tile (j, k) transposed)
//       to the workspace, W_j = D^-1 R_j beside it.
//   spd_update_kernel one workgroup per tile (bi <= bj) of the UPPER block triangle (a linear grid of those tiles alone): A_ij -=
//       R_i^T W_j from the workspace's R and W (so no launch reads what it writes); the tiles of row / column k take W, W^T and -D^-1 instead. Diagonal tiles are
//       computed for gi <= gj and mirrored inside the tile, so they stay exactly symmetric. The lower block triangle is not
//       touched until spd_finish_kernel negates the upper one and mirrors it: P is exactly symmetric.
// Tile products: 4 waves, wave w the rows 16 w .. 16 w + 15 of the 64 x 64 tile as four 16 x 16 accumulators of
// v_mfma_f64_16x16x4_f64, operands and C/D map as als.hip (A[lane & 15][k = lane >> 4], B[k = lane >> 4][lane & 15]; col =
// lane & 15, row = (lane >> 4) + 4 reg). k runs 0, 4, .., 60 for every element, so an element's bits depend on A and EASE_NB alone.
// Both operand tiles sit in LDS as [64][64] doubles, the 16-column groups of row c exchanged by c & 3 so that the two 32-lane
// halves of a b64 read fall into different bank halves: 2 x 32 KiB = 64 KiB per workgroup, two on a CU. That budget is a design
// choice, not a measurement, until tools/ease_time.py's numbers say otherwise. n is padded to a multiple of 64 with an identity
// block that is never stored: a load outside [0, n)^2 gives (i == j), a store there is dropped.
//
// ease_chunk_kernel: grid (query tiles x candidate chunks of KNN_CHUNK), K-lists, offer, flush, launch and merge are
// knn_select.h's; the multiply phase is a gather-sum. A wave owns 16 users and walks its chunk in strips of 64 candidates, lane =
// candidate: per user the history ids pass through an LDS stage of EASE_HSTAGE ids, and every id adds its row of P at the
// strip's columns (one 512-byte read per id and wave) -- float64, in the history's order, the id equal to the candidate left out
// -- then score = float(-sum / P_jj). The 16 x 64 scores turn through LDS into the offer's layout (lane (li, kq): candidate li
// against users 4 kq .. 4 kq + 3). No [B x I] block is written. Left out: the user's segment of the exclusion CSR (the history
// itself when none is given), scanned only for scores that beat the threshold. A zero operand gives a zero: a cold item's
// column of P is zero off the diagonal, its score exactly 0.
#include "common.h"
#include "cosine.h"
#include "knn_select.h"

namespace elimrec {

constexpr int EASE_NB = 64, EASE_THREADS = 256, EASE_HSTAGE = 64, EASE_STRIP = 64;
typedef double ease_v4d __attribute__((ext_vector_type(4)));

// ---- Gram
__global__ __launch_bounds__(EASE_THREADS) void gram_counts_kernel(const int64_t *__restrict__ q_ptr, const int32_t *__restrict__ q_nbr,
                                                                  const int64_t *__restrict__ o_ptr, const int32_t *__restrict__ o_nbr,
                                                                  int64_t n, int64_t n_other, double l2, double *out, int64_t ld) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t i = blockIdx.x;
    unsigned long long *cnt = reinterpret_cast<unsigned long long *>(out + i * ld);   // the row's slots as integer counters
    for (int64_t j = tid; j < n; j += EASE_THREADS) cnt[j] = 0ull;
    __threadfence();
    __syncthreads();
    const int64_t p1 = q_ptr[i + 1];
    for (int64_t p = q_ptr[i] + wave; p < p1; p += EASE_THREADS / 64) {
        const int64_t u = q_nbr[p];
        if (u < 0 || u >= n_other) continue;                 // (wave-uniform; the host checked the ids)
        const int64_t e1 = o_ptr[u + 1];
        for (int64_t e = o_ptr[u] + lane; e < e1; e += 64) {
            const int64_t j = o_nbr[e];
            if (j >= 0 && j < n) atomicAdd(&cnt[j], 1ull);
        }
    }
    __threadfence();
    __syncthreads();
    for (int64_t j = tid; j < n; j += EASE_THREADS) {
        double v = (double)__hip_atomic_load(&cnt[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (j == i) v = v + l2;
        __hip_atomic_store(&cnt[j], (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- inverse
struct SpdArgs {
    double *A; int64_t n, ld; int nblk, k;
    double *dinv;                      // [64][64] D^-1 of the pivot block
    double *R, *W; int64_t ldw;        // [64][ldw = 64 nblk] the pivot block's row panel and D^-1 times it
    double *pivot_min; int32_t *status;
};

__device__ __forceinline__ double spd_load(const SpdArgs &a, int64_t i, int64_t j) {
    return (i < a.n && j < a.n) ? a.A[i * a.ld + j] : (i == j ? 1.0 : 0.0);
}
// element (c, col) of an operand tile in LDS
__device__ __forceinline__ int spd_at(int c, int col) { return c * EASE_NB + (col ^ ((c & 3) << 4)); }

// tile t of the upper block triangle, column-major over bi <= bj: t = bj (bj + 1) / 2 + bi (the grid holds these tiles alone)
__device__ __forceinline__ void spd_tile_of(unsigned t, int &bi, int &bj) {
    int64_t j = (int64_t)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while (j * (j + 1) / 2 > (int64_t)t) --j;
    while ((j + 1) * (j + 2) / 2 <= (int64_t)t) ++j;
    bj = (int)j;
    bi = (int)((int64_t)t - j * (j + 1) / 2);
}

// acc[t] += (sA^T sB)[16 wave + kq + 4 x][16 t + li]
__device__ __forceinline__ void spd_tile_product(const double *sA, const double *sB, int wave, int li, int kq, ease_v4d acc[4]) {
#pragma unroll 4
    for (int ks = 0; ks < EASE_NB / 4; ++ks) {
        const int c = 4 * ks + kq;
        const double x = sA[spd_at(c, 16 * wave + li)];
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(x, sB[spd_at(c, 16 * t + li)], acc[t], 0, 0, 0);
    }
}

__global__ void spd_init_kernel(double *pivot_min, int32_t *status) {
    if (threadIdx.x == 0) {
        *pivot_min = __builtin_huge_val();
        status[0] = 0;
        status[1] = INT32_MAX;
    }
}

__global__ __launch_bounds__(EASE_THREADS) void spd_pivot_kernel(SpdArgs a) {
    constexpr int NB = EASE_NB, LDA = NB + 1;
    __shared__ double s_A[NB * LDA];                         // lower: L, diagonal: Delta, upper: (L^-1)^T
    __shared__ double s_col[NB];
    if (a.status[0] != 0) return;                            // (workgroup-uniform) an earlier pivot block was refused
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int64_t k0 = (int64_t)a.k * NB;
    for (int e = tid; e < NB * NB; e += EASE_THREADS) {
        const int r = e / NB, c = e - r * NB;
        s_A[r * LDA + c] = spd_load(a, k0 + r, k0 + c);
    }
    double pmin = __builtin_huge_val();
    int bad = -1;
    for (int k = 0; k < NB; ++k) {
        __syncthreads();
        const double p = s_A[k * LDA + k];                   // the same value on every thread
        if (!(p > 0.0) || p == __builtin_huge_val()) { bad = k; break; }
        if (k0 + k < a.n) pmin = p < pmin ? p : pmin;
        if (tid > k && tid < NB) s_col[tid] = s_A[tid * LDA + k];
        __syncthreads();
        if (tid > k && tid < NB) s_A[tid * LDA + k] = s_col[tid] / p;
        for (int i = k + 1 + ty; i < NB; i += 16) {
            const double lik = s_col[i] / p;
            for (int j = k + 1 + tx; j <= i; j += 16) s_A[i * LDA + j] = s_A[i * LDA + j] - lik * s_col[j];
        }
    }
    if (bad >= 0) {                                          // workgroup-uniform
        if (tid == 0) {
            atomicAdd(&a.status[0], 1);
            atomicMin(&a.status[1], (int)(k0 + bad));
        }
        return;
    }
    if (tid == 0 && pmin < *a.pivot_min) *a.pivot_min = pmin;
    __syncthreads();
    if (tid < NB) {                                          // M = L^-1, column tid: M_ic at s_A[c][i]
        const int c = tid;
        for (int i = c + 1; i < NB; ++i) {
            double s = s_A[i * LDA + c];
            for (int m = c + 1; m < i; ++m) s = s + s_A[i * LDA + m] * s_A[c * LDA + m];
            s_A[c * LDA + i] = -s;
        }
    }
    __syncthreads();
    for (int e = tid; e < NB * NB; e += EASE_THREADS) {
        const int r = e / NB, c = e - r * NB;
        if (r > c) continue;
        double s = (r == c ? 1.0 : s_A[r * LDA + c]) * (1.0 / s_A[c * LDA + c]);           // m = c: M_cc = 1
        for (int m = c + 1; m < NB; ++m) s = s + s_A[r * LDA + m] * (s_A[c * LDA + m] / s_A[m * LDA + m]);
        a.dinv[r * NB + c] = s;
        a.dinv[c * NB + r] = s;
    }
}

__global__ __launch_bounds__(EASE_THREADS) void spd_panel_kernel(SpdArgs a) {
    constexpr int NB = EASE_NB;
    extern __shared__ double spd_smem[];
    double *sA = spd_smem, *sB = spd_smem + NB * NB;
    const int j = blockIdx.x;
    if (a.status[0] != 0 || j == a.k) return;                // (workgroup-uniform)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, kq = lane >> 4;
    const int64_t k0 = (int64_t)a.k * NB, j0 = (int64_t)j * NB;
    for (int e = tid; e < NB * NB; e += EASE_THREADS) {
        const int r = e / NB, c = e - r * NB;
        sA[spd_at(r, c)] = a.dinv[e];
        if (j > a.k) sB[spd_at(r, c)] = spd_load(a, k0 + r, j0 + c);          // tile (k, j)
        else sB[spd_at(c, r)] = spd_load(a, j0 + r, k0 + c);                  // tile (j, k), transposed
    }
    __syncthreads();
    for (int e = tid; e < NB * NB; e += EASE_THREADS) {
        const int r = e / NB, c = e - r * NB;
        a.R[r * a.ldw + j0 + c] = sB[spd_at(r, c)];
    }
    ease_v4d acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = (ease_v4d){0.0, 0.0, 0.0, 0.0};
    spd_tile_product(sA, sB, wave, li, kq, acc);             // D^-1 is symmetric: (D^-1)^T R = D^-1 R
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int x = 0; x < 4; ++x) a.W[(16 * wave + kq + 4 * x) * a.ldw + j0 + 16 * t + li] = acc[t][x];
}

__global__ __launch_bounds__(EASE_THREADS) void spd_update_kernel(SpdArgs a) {
    constexpr int NB = EASE_NB;
    extern __shared__ double spd_smem[];
    double *sA = spd_smem, *sB = spd_smem + NB * NB;
    int bi, bj;
    spd_tile_of(blockIdx.x, bi, bj);
    if (a.status[0] != 0) return;                            // (workgroup-uniform)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, kq = lane >> 4;
    const int64_t i0 = (int64_t)bi * NB, j0 = (int64_t)bj * NB;
    if (bi == a.k || bj == a.k) {                            // the pivot block's row and column: W, W^T, -D^-1
        for (int e = tid; e < NB * NB; e += EASE_THREADS) {
            const int r = e / NB, c = e - r * NB;
            const int64_t gi = i0 + r, gj = j0 + c;
            if (gi >= a.n || gj >= a.n) continue;
            double v;
            if (bi == bj) v = -a.dinv[e];
            else if (bi == a.k) v = a.W[r * a.ldw + gj];
            else v = a.W[c * a.ldw + gi];
            a.A[gi * a.ld + gj] = v;
        }
        return;
    }
    for (int e = tid; e < NB * NB; e += EASE_THREADS) {
        const int r = e / NB, c = e - r * NB;
        sA[spd_at(r, c)] = a.R[r * a.ldw + i0 + c];
        sB[spd_at(r, c)] = a.W[r * a.ldw + j0 + c];
    }
    __syncthreads();
    ease_v4d acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = (ease_v4d){0.0, 0.0, 0.0, 0.0};
    spd_tile_product(sA, sB, wave, li, kq, acc);
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int x = 0; x < 4; ++x) {
            const int64_t gi = i0 + 16 * wave + kq + 4 * x, gj = j0 + 16 * t + li;
            if (gi >= a.n || gj >= a.n || (bi == bj && gi > gj)) continue;
            const double v = a.A[gi * a.ld + gj] - acc[t][x];
            a.A[gi * a.ld + gj] = v;
            if (bi == bj && gi != gj) a.A[gj * a.ld + gi] = v;
        }
}

// A = -(upper block triangle), mirrored
__global__ __launch_bounds__(EASE_THREADS) void spd_finish_kernel(SpdArgs a) {
    constexpr int NB = EASE_NB;
    int bi, bj;
    spd_tile_of(blockIdx.x, bi, bj);
    if (a.status[0] != 0) return;
    const int64_t i0 = (int64_t)bi * NB, j0 = (int64_t)bj * NB;
    for (int e = threadIdx.x; e < NB * NB; e += EASE_THREADS) {
        const int r = e / NB, c = e - r * NB;
        const int64_t gi = i0 + r, gj = j0 + c;
        if (gi >= a.n || gj >= a.n) continue;
        const double v = -a.A[gi * a.ld + gj];
        a.A[gi * a.ld + gj] = v;
        if (bi != bj) a.A[gj * a.ld + gi] = v;
    }
}

constexpr size_t SPD_DINV_BYTES = (size_t)EASE_NB * EASE_NB * 8, SPD_TILE_LDS = 2 * SPD_DINV_BYTES;
static_assert(SPD_TILE_LDS <= 64 * 1024, "spd_inverse: a workgroup stays within 64 KiB of LDS");
inline int64_t spd_blocks(int64_t n) { return (n + EASE_NB - 1) / EASE_NB; }
inline size_t spd_workspace_bytes(int64_t n) {
    return n <= 0 ? 16 : SPD_DINV_BYTES + 2 * (size_t)EASE_NB * (size_t)spd_blocks(n) * EASE_NB * 8;
}

// ---- ranking
struct EaseArgs {
    const double *P; int64_t ld, n;
    const int64_t *h_ptr; const int32_t *h_items;           // the histories, one segment per user known
    const int64_t *e_ptr; const int32_t *e_items;           // what is left out, over the same segments
    int64_t n_seg;
    const int64_t *users; int64_t Q;                         // query b's segment
    int K, n_chunks;
    float *ws_val; int32_t *ws_idx;                          // [Q][n_chunks x K]
};

static inline size_t ease_lds_bytes(int W, int K) {
    return (size_t)W * (16 * EASE_STRIP * 4 + EASE_HSTAGE * 4) + knn_list_bytes(16 * (size_t)W, K);
}

__device__ __forceinline__ bool ease_keep(const int32_t *ids, int64_t e0, int64_t e1, int cand) {
    bool keep = true;
    for (int64_t e = e0; e < e1 && keep; ++e) keep = ids[e] != cand;
    return keep;
}

// W: waves per workgroup (4: K <= KNN_SMALLK; 1: larger K), as knn_chunk_kernel
template <int W>
__global__ __launch_bounds__(64 * W) void ease_chunk_kernel(EaseArgs a) {
    constexpr int ROWS = 16 * W, E = knn_list_regs(W);
    const int K = a.K;
    extern __shared__ float smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, kq = lane >> 4;
    float *sc = smem + wave * 16 * EASE_STRIP;                               // [16][EASE_STRIP] this wave's scores of a strip
    int *sh = reinterpret_cast<int *>(smem + W * 16 * EASE_STRIP) + wave * EASE_HSTAGE;   // this wave's stage of history ids
    const KnnLists my = knn_lists(smem + W * (16 * EASE_STRIP + EASE_HSTAGE), ROWS, K, wave);
    const int64_t q0 = (int64_t)blockIdx.x * ROWS + wave * 16;               // this wave's first query
    if (q0 >= a.Q) return;                                   // (wave-uniform; the kernel has no workgroup barrier)
    const int chunk = blockIdx.y;
    const int64_t c_begin = (int64_t)chunk * KNN_CHUNK;
    const int64_t c_end = c_begin + KNN_CHUNK < a.n ? c_begin + KNN_CHUNK : a.n;

    // the four users this lane's scores belong to: their left-out lists and thresholds (+inf: nothing is kept)
    int64_t e0[4], e1[4];
    float thr[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t q = q0 + 4 * kq + r;
        int64_t seg = q < a.Q ? a.users[q] : -1;
        if (seg >= a.n_seg) seg = -1;
        e0[r] = seg >= 0 ? a.e_ptr[seg] : 0;
        e1[r] = seg >= 0 ? a.e_ptr[seg + 1] : 0;
        thr[r] = knn_thr0(seg >= 0);
    }
    if (lane < 16) {
        const int64_t q = q0 + lane;
        int64_t seg = q < a.Q ? a.users[q] : -1;
        if (seg >= a.n_seg) seg = -1;
        knn_list_reset(my, lane, seg >= 0);
    }
    wave_lds_sync();

    for (int64_t c0 = c_begin; c0 < c_end; c0 += EASE_STRIP) {
        const int64_t c = c0 + lane;                         // this lane's candidate of the strip
        const bool c_ok = c < c_end;
        const double pjj = c_ok ? a.P[c * a.ld + c] : 1.0;
        for (int row = 0; row < 16; ++row) {
            const int64_t q = q0 + row;
            if (q >= a.Q) break;                             // wave-uniform
            const int64_t seg = a.users[q];
            if (seg < 0 || seg >= a.n_seg) continue;         // no query: its threshold is +inf, whatever sc holds
            const int64_t h0 = a.h_ptr[seg], hn = a.h_ptr[seg + 1] - h0;
            double acc = 0.0;
            for (int64_t s0 = 0; s0 < hn; s0 += EASE_HSTAGE) {
                const int cnt = hn - s0 < EASE_HSTAGE ? (int)(hn - s0) : EASE_HSTAGE;
                wave_lds_sync();                             // every lane is done with the stage before
                if (lane < cnt) sh[lane] = a.h_items[h0 + s0 + lane];
                wave_lds_sync();
#pragma unroll 4
                for (int t = 0; t < cnt; ++t) {
                    const int64_t h = sh[t];
                    double v = 0.0;
                    if (c_ok && h >= 0 && h < a.n && h != c) v = a.P[h * a.ld + c];
                    acc = acc + v;
                }
            }
            sc[row * EASE_STRIP + lane] = (float)(-acc / pjj);
        }
        wave_lds_sync();
#pragma unroll 1
        for (int sub = 0; sub < EASE_STRIP / 16; ++sub) {
            const int64_t cand = c0 + 16 * sub + li;
            const bool cand_ok = cand < c_end;
            float s[4];
            bool pass[4], any = false;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                s[r] = sc[(4 * kq + r) * EASE_STRIP + 16 * sub + li];
                pass[r] = cand_ok && s[r] > thr[r];
                any = any || pass[r];
            }
            if (__ballot(any) == 0ull) continue;             // wave-uniform: the steady state
            KNN_OFFER(my, E, K, lane, kq, q0, cand, s, pass, thr, ((const int64_t *)nullptr), ((const int32_t *)nullptr),
                      ease_keep(a.e_items, e0[r], e1[r], (int)cand));
        }
        wave_lds_sync();                                     // every lane has read the strip's scores
    }

    KNN_FLUSH(my, E, K, lane, q0, a.Q, a.n_chunks, chunk, a.ws_val, a.ws_idx);
}

template <int W>
static int ease_launch(const EaseArgs &a, int64_t n_tiles, hipStream_t s) {
    return knn_launch_chunks("ease_topk", ease_chunk_kernel<W>, a, n_tiles, a.n_chunks, 64 * W, ease_lds_bytes(W, a.K), s);
}

}  // namespace elimrec

using namespace elimrec;

extern "C" int elimrec_ease_block(void) { return EASE_NB; }
extern "C" int elimrec_ease_hist_stage(void) { return EASE_HSTAGE; }

extern "C" int elimrec_gram_counts(const int64_t *d_q_ptr, const int32_t *d_q_nbr, const int64_t *d_o_ptr, const int32_t *d_o_nbr, int64_t n,
                                   int64_t n_other, double l2, double *d_out, int64_t ld, void *stream) {
    ELIMREC_REQUIRE(n >= 0 && n < (int64_t)INT32_MAX && n_other >= 0 && n_other < (int64_t)INT32_MAX,
                    "gram_counts: both sides' row counts lie in [0, 2^31 - 1)");
    ELIMREC_REQUIRE(ld >= n, "gram_counts: ld < n");
    ELIMREC_REQUIRE(l2 >= 0.0 && l2 <= 1.7976931348623157e308, "gram_counts: l2 must be finite and >= 0");
    if (n == 0) return 0;
    ELIMREC_REQUIRE(d_q_ptr && d_o_ptr && d_out && (n_other == 0 || (d_q_nbr && d_o_nbr)), "gram_counts: null pointer");
    ELIMREC_REQUIRE(((uintptr_t)d_out & 7) == 0, "gram_counts: out must be 8-byte aligned");
    hipLaunchKernelGGL(gram_counts_kernel, dim3((unsigned)n), dim3(EASE_THREADS), 0, (hipStream_t)stream, d_q_ptr, d_q_nbr, d_o_ptr, d_o_nbr,
                       n, n_other, l2, d_out, ld);
    ELIMREC_LAUNCH_CHECK("gram_counts");
    return 0;
}

extern "C" size_t elimrec_spd_inverse_workspace(int64_t n) { return spd_workspace_bytes(n); }

extern "C" int elimrec_spd_inverse(double *d_A, int64_t n, int64_t ld, double *d_pivot_min, int32_t *d_status, void *d_workspace,
                                   size_t workspace_bytes, void *stream) {
    ELIMREC_REQUIRE(n >= 0 && ld >= n, "spd_inverse: need n >= 0 and ld >= n");
    const int64_t nblk = spd_blocks(n);
    ELIMREC_REQUIRE(nblk <= 65535, "spd_inverse: n <= %d", 65535 * EASE_NB);
    ELIMREC_REQUIRE(d_pivot_min && d_status, "spd_inverse: null pointer");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(spd_init_kernel, dim3(1), dim3(64), 0, s, d_pivot_min, d_status);
    ELIMREC_LAUNCH_CHECK("spd_inverse");
    if (n == 0) return 0;
    ELIMREC_REQUIRE(d_A && d_workspace, "spd_inverse: null pointer");
    ELIMREC_REQUIRE(((uintptr_t)d_workspace & 15) == 0 && workspace_bytes >= spd_workspace_bytes(n),
                    "spd_inverse: the workspace needs %zu bytes, 16-byte aligned (got %zu)", spd_workspace_bytes(n), workspace_bytes);
    SpdArgs a;
    a.A = d_A; a.n = n; a.ld = ld; a.nblk = (int)nblk; a.k = 0;
    a.dinv = (double *)d_workspace;
    a.ldw = nblk * EASE_NB;
    a.R = a.dinv + EASE_NB * EASE_NB;
    a.W = a.R + EASE_NB * a.ldw;
    a.pivot_min = d_pivot_min; a.status = d_status;
    const dim3 tiles((unsigned)(nblk * (nblk + 1) / 2));     // the upper block triangle: at most 65535 * 65536 / 2 < 2^31 - 1
    for (int k = 0; k < (int)nblk; ++k) {
        a.k = k;
        hipLaunchKernelGGL(spd_pivot_kernel, dim3(1), dim3(EASE_THREADS), 0, s, a);
        if (nblk > 1) hipLaunchKernelGGL(spd_panel_kernel, dim3((unsigned)nblk), dim3(EASE_THREADS), SPD_TILE_LDS, s, a);
        hipLaunchKernelGGL(spd_update_kernel, tiles, dim3(EASE_THREADS), SPD_TILE_LDS, s, a);
        ELIMREC_LAUNCH_CHECK("spd_inverse");
    }
    hipLaunchKernelGGL(spd_finish_kernel, tiles, dim3(EASE_THREADS), 0, s, a);
    ELIMREC_LAUNCH_CHECK("spd_inverse");
    return 0;
}

extern "C" size_t elimrec_ease_topk_workspace(int64_t Q, int64_t n, int K) { return knn_workspace_bytes(Q, n, K); }

extern "C" int elimrec_ease_topk(const double *d_P, int64_t ld, int64_t n, const int64_t *d_hist_ptr, const int32_t *d_hist_items,
                                 const int64_t *d_excl_ptr, const int32_t *d_excl_items, int64_t n_seg, const int64_t *d_users, int64_t Q,
                                 int K, int32_t *d_idx, float *d_val, void *d_workspace, size_t workspace_bytes, void *stream) {
    const char *who = "ease_topk";
    if (int rc = knn_check_k(who, K)) return rc;
    ELIMREC_REQUIRE(Q >= 0 && n >= 0 && n < (int64_t)INT32_MAX - KNN_CHUNK && n_seg >= 0, "%s: need Q >= 0, n_seg >= 0 and 0 <= n < 2^31 - %d",
                    who, KNN_CHUNK + 1);
    ELIMREC_REQUIRE(ld >= n, "%s: ld < n", who);
    if (Q == 0) return 0;
    ELIMREC_REQUIRE(d_users && d_idx && d_workspace && d_hist_ptr && d_hist_items && (n == 0 || d_P), "%s: null pointer", who);
    if (int rc = knn_check_buffers(who, d_excl_ptr, d_excl_items, d_workspace, workspace_bytes, Q, n, K)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) return knn_fill_empty(who, d_idx, d_val, Q, K, s);
    KnnWorkspace ws;
    if (int rc = knn_carve(who, "users", Q, n, K, d_workspace, &ws)) return rc;
    EaseArgs a;
    a.P = d_P; a.ld = ld; a.n = n;
    a.h_ptr = d_hist_ptr; a.h_items = d_hist_items;
    a.e_ptr = d_excl_ptr ? d_excl_ptr : d_hist_ptr;          // the default leaves the history itself out
    a.e_items = d_excl_ptr ? d_excl_items : d_hist_items;
    a.n_seg = n_seg;
    a.users = d_users; a.Q = Q;
    a.K = K; a.n_chunks = (int)ws.n_chunks;
    a.ws_val = ws.val; a.ws_idx = ws.idx;
    const int rows = K <= KNN_SMALLK ? KNN_TILE : 16;
    const int64_t n_tiles = (Q + rows - 1) / rows;
    ELIMREC_REQUIRE(n_tiles < (int64_t)INT32_MAX, "%s: too many user tiles for one launch", who);
    int rc = K <= KNN_SMALLK ? ease_launch<4>(a, n_tiles, s) : ease_launch<1>(a, n_tiles, s);
    if (rc) return rc;
    return knn_merge(ws, Q, K, d_idx, d_val, stream);
}
