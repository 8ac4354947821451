// Cosine top-K of table rows against the rows of the same table (similar items / similar users) or of a second table
// (cross_topk: the query rows come from a table of their own -- with unit squared norms on both sides the score is the plain dot
// product, inv_norm(1.0) being exactly 1: serving a factor model), and the overlap of two id lists.
//
// knn_chunk_kernel: the grid is (query tiles x candidate chunks). A workgroup of W waves holds 16 W query rows -- a wave owns 16
// of them as the A operands of v_mfma_f32_16x16x4_f32 (registers for d = 32 / 64 / 128, a lane-private LDS column otherwise) --
// and streams the KNN_CHUNK candidate rows of its chunk through ONE LDS stage of SR rows (row stride d + 4 floats: 16-byte
// aligned b128 stores, B-operand reads two-way at worst); the next stage's rows and squared norms travel in registers while the
// current one is multiplied (two barriers per stage). Every wave multiplies every 16-row candidate tile of the stage against its
// own queries: lane (li, kq) ends with the dot products of candidate li against query rows 4 kq .. 4 kq + 3.
//     score = (dot * (1 / max(sqrt(sq_q), 1e-12))) * (1 / max(sqrt(sq_c), 1e-12))
// in this order, IEEE division: a pair's bits depend on the two rows' values and d alone (the k-loop runs 0, 4, 8, ... for every
// pair; rows outside the table are zero operands and never read), not on its tile, stage, chunk or grid.
// Selection (per chunk) and everything else around the multiply is knn_select.h's, shared with audience.hip: the K-list per query
// row in LDS (CAP = K + 32 slots, its layout, the offer of a tile's scores with the exclusion scan, the cut to the K best, the
// flush of K pairs per query and chunk into the workspace [Q][chunks x K]) and the host front end (chunks, workspace, the shared
// requirements, the launch, elimrec_topk_merge). This kernel's own exclusion clause is the query row itself (exclude_self); after
// warm-up its epilogue is two multiplies and one compare per score.
// Query tile and LDS: K <= 64 -> 4 waves, 64 query rows, lists 64 x 96 x 8 B = 48 KiB, stage <= 17 KiB (64 rows at d <= 64, 32
// at d = 128, 16 otherwise), lane-private A columns d x 256 B for the general d (64 KiB at d = 256: one workgroup per CU there,
// two or more for every other shape). K > 64 -> the tile is cut to ONE wave, 16 query rows: lists 16 x 288 x 8 B = 36 KiB,
// stage 16 rows <= 16.3 KiB, A columns <= 16 KiB: at most 69 KiB, two workgroups per CU at K = 256 and any d.
// list_overlap_kernel: one wave per row, list b in LDS, every lane counts its entries of a; integer, exact.
#include "common.h"
#include "cosine.h"
#include "knn_select.h"

namespace elimrec {

constexpr int KNN_OVERLAP_MAXK = 1024;
typedef float knn_v4f __attribute__((ext_vector_type(4)));

struct KnnArgs {
    const float *T; int64_t ld, n_rows; int d;
    const float *sq; int64_t ld_sq;
    const float *Tq; int64_t ldq, nq_rows;   // the query table (cosine_topk: the table itself): rows, stride, row count,
    const float *sqq; int64_t ld_sqq;        // squared norms and their stride
    const int32_t *qrows; int64_t Q; int exclude_self;
    const int64_t *excl_ptr; const int32_t *excl_rows;
    int K, n_chunks, vec;              // vec: T is 16-byte aligned and ld % 4 == 0 -> a row's float4s are single loads
    float *ws_val; int32_t *ws_idx;    // [Q][n_chunks x K]
};

constexpr int knn_stage_rows(int D, int W) { return (D == 0 || W == 1) ? 16 : (D <= 64 ? 64 : 32); }
// dynamic LDS of one workgroup, in bytes (host and device agree through this one function)
static inline size_t knn_lds_bytes(int D, int W, int d, int K) {
    const size_t sr = (size_t)knn_stage_rows(D, W);
    return sr * (d + 4) * 4 + sr * 4 + knn_list_bytes(16 * (size_t)W, K) + (D == 0 ? (size_t)W * (d / 4) * 64 * 4 : 0);
}

// D: 32 / 64 / 128 = the dimension at compile time, query operands in registers; 0 = any d % 4 == 0 up to TABLE_MAXD.
// W: waves per workgroup (4: K <= KNN_SMALLK; 1: larger K)
template <int D, int W>
__global__ __launch_bounds__(64 * W) void knn_chunk_kernel(KnnArgs a) {
    constexpr int SR = knn_stage_rows(D, W), NT = 64 * W, ROWS = 16 * W;
    constexpr int E = knn_list_regs(W);
    constexpr int PFN = (SR * (D ? D : TABLE_MAXD) / 4 + NT - 1) / NT;
    const int d = D ? D : a.d, LD = d + 4, K = a.K;
    extern __shared__ float smem[];
    float *s_b = smem;                                       // [SR][LD] the stage's candidate rows
    float *s_invc = s_b + SR * LD;                           // [SR]     their reciprocal norms
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const KnnLists my = knn_lists(s_invc + SR, ROWS, K, wave);   // knn_list_bytes(ROWS, K): the query rows' K-lists, this wave's 16
    float *s_a = my.end;                                     // D == 0: [W][d / 4][64] lane-private query operands
    const int li = lane & 15, kq = lane >> 4;
    const int64_t q0 = (int64_t)blockIdx.x * ROWS + wave * 16;   // this wave's first query
    const int chunk = blockIdx.y;
    const int64_t c_begin = (int64_t)chunk * KNN_CHUNK;
    const int64_t c_end = c_begin + KNN_CHUNK < a.n_rows ? c_begin + KNN_CHUNK : a.n_rows;

    // A operands: query (q0 + li), element k = 4 ks + kq; a query outside [0, Q) or with an id outside the query table is all zeros
    float qa[D ? D / 4 : 1];
    {
        const int64_t q = q0 + li;
        int64_t qr = q < a.Q ? (int64_t)a.qrows[q] : -1;
        if (qr >= a.nq_rows) qr = -1;
        const float *row = qr >= 0 ? a.Tq + qr * a.ldq + kq : nullptr;
        if (D) {
#pragma unroll
            for (int ks = 0; ks < (D ? D / 4 : 1); ++ks) qa[ks] = row ? row[4 * ks] : 0.f;
        } else {
            for (int ks = 0; ks < d / 4; ++ks) s_a[(wave * (d / 4) + ks) * 64 + lane] = row ? row[4 * ks] : 0.f;
        }
    }
    // the four query rows this lane's accumulators belong to: ids, reciprocal norms, thresholds (+inf: nothing is kept)
    int qid[4];
    float invq[4], thr[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t q = q0 + 4 * kq + r;
        int64_t qr = q < a.Q ? (int64_t)a.qrows[q] : -1;
        if (qr >= a.nq_rows) qr = -1;
        qid[r] = (int)qr;
        invq[r] = qr >= 0 ? inv_norm(a.sqq[qr * a.ld_sqq]) : 0.f;
        thr[r] = knn_thr0(qr >= 0);
    }
    if (lane < 16) {
        const int64_t q = q0 + lane;
        int64_t qr = q < a.Q ? (int64_t)a.qrows[q] : -1;
        if (qr >= a.nq_rows) qr = -1;
        knn_list_reset(my, lane, qr >= 0);
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
                const int64_t cand = s0 + r;
                float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
                if (cand < c_end) ELIMREC_LOAD_ROW4(x, a.T + cand * a.ld + c, a.vec);
                pf[p] = x;
            }
        }
        if (tid < SR) sq_pf = s0 + tid < c_end ? a.sq[(s0 + tid) * a.ld_sq] : 1.f;
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
        if (tid < SR) s_invc[tid] = inv_norm(sq_pf);
    };

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
            knn_v4f acc = (knn_v4f){0.f, 0.f, 0.f, 0.f};
            const float *bp = s_b + (16 * t + li) * LD + kq;
            if (D) {
#pragma unroll
                for (int ks = 0; ks < (D ? D / 4 : 1); ++ks) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[ks], bp[4 * ks], acc, 0, 0, 0);
            } else {
                const float *ap = s_a + wave * (d / 4) * 64 + lane;
                for (int ks = 0; ks < d / 4; ++ks) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[ks * 64], bp[4 * ks], acc, 0, 0, 0);
            }
            // lane: candidate t0 + li against query rows 4 kq + r of this wave
            const int64_t cand = t0 + li;
            const bool cand_ok = cand < c_end;
            const float invc = s_invc[16 * t + li];
            float s[4];
            bool pass[4], any = false;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                s[r] = (acc[r] * invq[r]) * invc;
                pass[r] = cand_ok && s[r] > thr[r];
                any = any || pass[r];
            }
            if (__ballot(any) == 0ull) continue;             // wave-uniform: the steady state
            KNN_OFFER(my, E, K, lane, kq, q0, cand, s, pass, thr, a.excl_ptr, a.excl_rows, !(a.exclude_self && (int)cand == qid[r]));
        }
        __syncthreads();                                     // every wave is done with the stage
        if (more) store_stage();
        __syncthreads();
    }

    KNN_FLUSH(my, E, K, lane, q0, a.Q, a.n_chunks, chunk, a.ws_val, a.ws_idx);
}

__global__ __launch_bounds__(256) void list_overlap_kernel(const int32_t *__restrict__ la, const int32_t *__restrict__ lb, int64_t n_rows,
                                                           int K, int32_t *__restrict__ count) {
    extern __shared__ int s_list[];                          // [4][K]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t r = (int64_t)blockIdx.x * 4 + wave;
    if (r >= n_rows) return;                                 // (wave-uniform; no workgroup barrier below)
    int *b = s_list + wave * K;
    for (int k = lane; k < K; k += 64) b[k] = lb[r * K + k];
    wave_lds_sync();
    int n = 0;
    for (int k = lane; k < K; k += 64) {
        const int x = la[r * K + k];
        if (x < 0) continue;
        bool hit = false;
        for (int j = 0; j < K; ++j) hit = hit || b[j] == x;
        n += hit ? 1 : 0;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off, 64);
    if (lane == 0) count[r] = n;
}

template <int D, int W>
static int knn_launch(const char *who, const KnnArgs &a, int64_t n_tiles, hipStream_t s) {
    return knn_launch_chunks(who, knn_chunk_kernel<D, W>, a, n_tiles, a.n_chunks, 64 * W, knn_lds_bytes(D, W, a.d, a.K), s);
}

template <int W>
static int knn_dispatch(const char *who, const KnnArgs &a, int64_t n_tiles, hipStream_t s) {
    switch (a.d) {
    case 32: return knn_launch<32, W>(who, a, n_tiles, s);
    case 64: return knn_launch<64, W>(who, a, n_tiles, s);
    case 128: return knn_launch<128, W>(who, a, n_tiles, s);
    default: return knn_launch<0, W>(who, a, n_tiles, s);
    }
}

}  // namespace elimrec

using namespace elimrec;

extern "C" int elimrec_cosine_topk_chunk(void) { return KNN_CHUNK; }
extern "C" int elimrec_cosine_topk_tile(void) { return KNN_TILE; }

extern "C" size_t elimrec_cosine_topk_workspace(int64_t Q, int64_t n_rows, int K) {
    return knn_workspace_bytes(Q, n_rows, K);
}

// what the two entry points share; `who` names the caller in every message
static int knn_run(const char *who, const float *d_Tq, int64_t ldq, int64_t nq_rows, const float *d_sqq, int64_t ld_sqq, const float *d_T,
                   int64_t ld, int64_t n_rows, int d, const float *d_sqnorm, int64_t ld_sq, const int32_t *d_query_rows, int64_t Q,
                   int exclude_self, const int64_t *d_excl_ptr, const int32_t *d_excl_rows, int K, int32_t *d_idx, float *d_val,
                   void *d_workspace, size_t workspace_bytes, void *stream) {
    if (int rc = knn_check_k(who, K)) return rc;
    if (int rc = table_dims(who, d, 1)) return rc;
    ELIMREC_REQUIRE(Q >= 0 && n_rows >= 0 && n_rows < (int64_t)INT32_MAX - KNN_CHUNK, "%s: need Q >= 0 and 0 <= n_rows < 2^31 - %d", who,
                    KNN_CHUNK + 1);
    ELIMREC_REQUIRE(ld >= d && ld_sq >= 1, "%s: ld < d or ld_sq < 1", who);
    ELIMREC_REQUIRE(nq_rows >= 0 && ldq >= d && ld_sqq >= 1, "%s: the query table needs rows >= 0, ld >= d and ld_sq >= 1", who);
    if (Q == 0) return 0;
    ELIMREC_REQUIRE(d_query_rows && d_idx && d_workspace, "%s: null pointer", who);
    ELIMREC_REQUIRE(n_rows == 0 || (d_T && d_sqnorm), "%s: null pointer", who);
    ELIMREC_REQUIRE(nq_rows == 0 || (d_Tq && d_sqq), "%s: null pointer", who);
    if (int rc = knn_check_buffers(who, d_excl_ptr, d_excl_rows, d_workspace, workspace_bytes, Q, n_rows, K)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (n_rows == 0) return knn_fill_empty(who, d_idx, d_val, Q, K, s);       // an empty table
    KnnWorkspace ws;
    if (int rc = knn_carve(who, "queries", Q, n_rows, K, d_workspace, &ws)) return rc;
    KnnArgs a;
    a.T = d_T; a.ld = ld; a.n_rows = n_rows; a.d = d;
    a.sq = d_sqnorm; a.ld_sq = ld_sq;
    a.Tq = d_Tq; a.ldq = ldq; a.nq_rows = nq_rows;
    a.sqq = d_sqq; a.ld_sqq = ld_sqq;
    a.qrows = d_query_rows; a.Q = Q; a.exclude_self = exclude_self ? 1 : 0;
    a.excl_ptr = d_excl_ptr; a.excl_rows = d_excl_rows;
    a.K = K; a.n_chunks = (int)ws.n_chunks;
    a.vec = table_vec(d_T, ld);
    a.ws_val = ws.val; a.ws_idx = ws.idx;
    const int rows = K <= KNN_SMALLK ? KNN_TILE : 16;
    const int64_t n_tiles = (Q + rows - 1) / rows;
    ELIMREC_REQUIRE(n_tiles < (int64_t)INT32_MAX, "%s: too many query tiles for one launch", who);
    int rc = K <= KNN_SMALLK ? knn_dispatch<4>(who, a, n_tiles, s) : knn_dispatch<1>(who, a, n_tiles, s);
    if (rc) return rc;
    return knn_merge(ws, Q, K, d_idx, d_val, stream);
}

extern "C" int elimrec_cosine_topk(const float *d_T, int64_t ld, int64_t n_rows, int d, const float *d_sqnorm, int64_t ld_sq,
                                   const int32_t *d_query_rows, int64_t Q, int exclude_self, const int64_t *d_excl_ptr,
                                   const int32_t *d_excl_rows, int K, int32_t *d_idx, float *d_val, void *d_workspace,
                                   size_t workspace_bytes, void *stream) {
    return knn_run("cosine_topk", d_T, ld, n_rows, d_sqnorm, ld_sq, d_T, ld, n_rows, d, d_sqnorm, ld_sq, d_query_rows, Q, exclude_self,
                   d_excl_ptr, d_excl_rows, K, d_idx, d_val, d_workspace, workspace_bytes, stream);
}

extern "C" size_t elimrec_cross_topk_workspace(int64_t Q, int64_t n_rows, int K) {
    return knn_workspace_bytes(Q, n_rows, K);
}

extern "C" int elimrec_cross_topk(const float *d_Tq, int64_t ldq, int64_t nq_rows, const float *d_sqq, int64_t ld_sqq, const float *d_T,
                                  int64_t ld, int64_t n_rows, int d, const float *d_sqnorm, int64_t ld_sq, const int32_t *d_query_rows,
                                  int64_t Q, const int64_t *d_excl_ptr, const int32_t *d_excl_rows, int K, int32_t *d_idx, float *d_val,
                                  void *d_workspace, size_t workspace_bytes, void *stream) {
    return knn_run("cross_topk", d_Tq, ldq, nq_rows, d_sqq, ld_sqq, d_T, ld, n_rows, d, d_sqnorm, ld_sq, d_query_rows, Q, 0, d_excl_ptr,
                   d_excl_rows, K, d_idx, d_val, d_workspace, workspace_bytes, stream);
}

extern "C" int elimrec_list_overlap(const int32_t *d_a, const int32_t *d_b, int64_t n_rows, int K, int32_t *d_count, void *stream) {
    ELIMREC_REQUIRE(n_rows >= 0 && K >= 1 && K <= KNN_OVERLAP_MAXK, "list_overlap: need n_rows >= 0 and 1 <= K <= %d", KNN_OVERLAP_MAXK);
    if (n_rows == 0) return 0;
    ELIMREC_REQUIRE(d_a && d_b && d_count, "list_overlap: null pointer");
    ELIMREC_REQUIRE((n_rows + 3) / 4 < (int64_t)INT32_MAX, "list_overlap: too many rows for one launch");
    hipLaunchKernelGGL(list_overlap_kernel, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), (size_t)4 * K * sizeof(int), (hipStream_t)stream,
                       d_a, d_b, n_rows, K, d_count);
    ELIMREC_LAUNCH_CHECK("list_overlap");
    return 0;
}
