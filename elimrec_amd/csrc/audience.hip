// Audience lists: per query ITEM the K users with the largest predict() score for the (user, item) pair, under predict type
// normal / TE / TIE and fusion rubi / hm / sum (models/EliMRec.py:96-113, 155-212 read from the item's side).
//
// audience_chunk_kernel: the grid is (item tiles x user chunks). A workgroup of W waves holds 16 W query items -- a wave owns 16 of
// them as the A operands of v_mfma_f32_16x16x4_f32, every block of the row that the (fusion mode, head mask) pair uses: (1 + S) d / 4
// registers per lane for d = 32 / 64 (64 at d = 64, S = 3), a lane-private LDS column for any other d -- and streams the
// KNN_CHUNK user rows of its chunk through ONE LDS stage of SR rows. A staged row holds the columns of every used block side by side
// (row stride + 4 floats: 16-byte aligned b128 stores, B-operand reads two-way at worst), so a user row is read once per chunk; the
// next stage's rows, squared norms and row sums travel in registers while the current one is multiplied (two barriers per stage).
// The general-d form is one wave and stages one used block of the 16 rows at a time (a panel: <= 16.3 KiB instead of 65), the
// accumulators of the earlier blocks waiting in registers: every column still goes through LDS once per chunk. Block b of a row
// is read only if it is used: block 0 always, head h's (block h + 1) under TE / TIE with rubi when the mask holds h, with hm / sum always.
// Lane (li, kq) ends with the block dots of user li against items 4 kq .. 4 kq + 3 of its wave, and
//     ui = sigmoid(dot_0),  cos_h = (dot_h * inv(sq_u,h)) * inv(sq_i,h),  inv(x) = 1 / max(sqrt(x), 1e-12)   (cosine.h, IEEE)
//     normal: sigmoid(ui);  TE: sigmoid(fuse(ui, cos));  TIE: sigmoid(fuse(ui, cos) - fuse(m_u, cos)),  m_u = row_sum[u] / I_total
// with the expressions of score_math.h in the library's evaluator math mode (elimrec_score_set_math), the ones eval.hip's
// scorers use. The k-loop runs 0, 4, 8, ... for every pair and block: a pair's bits depend on the two rows, row_sum[u], d, S and
// the mode alone (rows outside the tables are zero operands and never read), not on its tile, stage, chunk or grid.
// Selection (per chunk) and everything else around the multiply is knn_select.h's, shared with knn.hip: the K-list per item in
// LDS (CAP = K + 32 slots; ties go to the lower user id), the scan of the item's exclusion list, the cut to the K best, the flush
// of K pairs per item and chunk into the workspace [Q][chunks x K], and the host front end down to elimrec_topk_merge. This kernel
// has no exclusion clause of its own. No [U x Q] block exists anywhere.
// Determinism: no float atomics. An item's list and scores depend on its own row, the user table, row_sum, its exclusion list, K,
// d, S and the mode only -- not on Q, the item's place in the query, the grid, or the arrival order inside a list.
// Tile and LDS per workgroup: K <= 64 and d = 32 / 64 -> 4 waves, 64 items: lists 64 x 96 x 8 B = 48 KiB, stage 32 rows at d = 32,
// 16 at d = 64 (<= 16.6 KiB): 65.5 KiB at most, two workgroups per CU. K > 64 or the general d -> ONE wave, 16 items: lists
// 16 x 288 x 8 B = 36 KiB at K = 256, stage <= 16.6 KiB, A columns (general d) <= 64 KiB: 53 KiB at K = 256 with d = 32 / 64 (three
// workgroups per CU), 117 KiB at d = 256, S = 3, K = 256 (one).
// audience_hits_kernel: one wave per item, the number of listed users found in the item's CSR list of users; integer, exact.
#include "common.h"
#include "cosine.h"
#include "dispatch.h"
#include "knn_select.h"
#include "score_math.h"

namespace elimrec {

constexpr int AUD_MAXB = 4;                                 // chunk, tile and K ranges: knn_select.h's
typedef float aud_v4f __attribute__((ext_vector_type(4)));

struct AudArgs {
    const float *Y; int64_t ldy, U, I; int d, S;
    uint32_t head_mask; int fusion_mode, predict_type;
    const float *sqn;                  // [(U + I) x (1 + S)] squared norms of every block of every row (elimrec_row_sqnorms)
    const float *row_sum; float I_total;   // TIE: [U] sums of sigmoid(u . i) over the catalogue, and the catalogue's size
    const int32_t *items; int64_t Q;
    const int64_t *excl_ptr; const int32_t *excl_users;
    int K, n_chunks, vec;              // vec: Y is 16-byte aligned and ldy % 4 == 0 -> a row's float4s are single loads
    int used;                          // bit b: block b of a row enters the score
    float *ws_val; int32_t *ws_idx;    // [Q][n_chunks x K]
};

constexpr int aud_stage_rows(int D, int W) { return (W == 4 && D == 32) ? 32 : 16; }
static inline int aud_popc(int x) { int n = 0; for (; x; x &= x - 1) ++n; return n; }
// dynamic LDS of one workgroup, in bytes (host and device agree through this one function); n_used: blocks that enter the score
static inline size_t aud_lds_bytes(int D, int W, int d, int n_used, int K) {
    const size_t sr = (size_t)aud_stage_rows(D, W);
    const size_t pw = D ? (size_t)n_used * d : (size_t)d;
    return sr * (pw + 4) * 4 + sr * AUD_MAXB * 4 + sr * 4 + knn_list_bytes(16 * (size_t)W, K) + (D == 0 ? (size_t)n_used * (d / 4) * 64 * 4 : 0);
}

// the score of one pair from its block dots; z: the heads' cosines (0 for a head that is not used: no fusion reads it)
template <bool FAST>
__device__ __forceinline__ float aud_score(int ptype, int fmode, int S, uint32_t mask, float dot0, const float *z, float m) {
    const float ui = sig_abs_<FAST>(dot0);
    if (ptype == 0) return sig_small_<FAST>(ui);
    if (ptype == 1) return sig_out_<FAST>(fmode, fuse_t<FAST>(fmode, ui, z, S, mask));
    float te, nde;
    fuse2_t<FAST>(fmode, ui, m, z, S, mask, te, nde);
    return sig_out_<FAST>(fmode, te - nde);
}

// D: 32 / 64 = the dimension at compile time, item operands in registers, W = 4 (K <= KNN_SMALLK) or 1; 0 = any d % 4 == 0 up
// to TABLE_MAXD, W = 1, item operands in lane-private LDS columns, one used block per panel.
template <int D, int W, bool FAST>
__global__ __launch_bounds__(64 * W) void audience_chunk_kernel(AudArgs a) {
    constexpr int SR = aud_stage_rows(D, W), NT = 64 * W, ROWS = 16 * W;
    constexpr int E = knn_list_regs(W);
    constexpr int PFN = (SR * (D ? AUD_MAXB * D : TABLE_MAXD) / 4 + NT - 1) / NT;
    constexpr int KS = D ? D / 4 : 1;
    static_assert(D != 0 || (W == 1 && SR == 16), "the general form is one wave and one 16-row tile per stage");
    const int d = D ? D : a.d, K = a.K, S = a.S, NB = 1 + S;
    // used blocks: their rank among the used ones fixes the column offset in a staged row / the A column in LDS
    int rank[AUD_MAXB], n_used = 0;
#pragma unroll
    for (int b = 0; b < AUD_MAXB; ++b) {
        rank[b] = n_used;
        n_used += (b < NB && (a.used >> b & 1)) ? 1 : 0;
    }
    const int NP = D ? 1 : n_used;                           // panels per stage
    const int PW = D ? n_used * d : d, LD = PW + 4;          // a panel's columns, the staged row's stride
    extern __shared__ float smem[];
    float *s_b = smem;                                       // [SR][LD] the stage's user rows (this panel's columns)
    float *s_inv = s_b + SR * LD;                            // [SR][AUD_MAXB] reciprocal norms of their head blocks (entry 1 + h)
    float *s_mean = s_inv + SR * AUD_MAXB;                   // [SR]     their catalogue means of ui (TIE)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const KnnLists my = knn_lists(s_mean + SR, ROWS, K, wave);   // knn_list_bytes(ROWS, K): the items' K-lists, this wave's 16
    float *s_a = my.end;                                     // D == 0: [n_used][d / 4][64] lane-private item operands
    const int li = lane & 15, kq = lane >> 4;
    const int64_t q0 = (int64_t)blockIdx.x * ROWS + wave * 16;   // this wave's first query item
    const int chunk = blockIdx.y;
    const int64_t c_begin = (int64_t)chunk * KNN_CHUNK;
    const int64_t c_end = c_begin + KNN_CHUNK < a.U ? c_begin + KNN_CHUNK : a.U;
    const bool tie = a.predict_type == 2;

    // A operands: item (q0 + li), element k = 4 ks + kq of every used block; a query outside [0, Q) or an id outside the
    // catalogue is all zeros and never read
    float qa[AUD_MAXB][KS];
    {
        const int64_t q = q0 + li;
        int64_t it = q < a.Q ? (int64_t)a.items[q] : -1;
        if (it >= a.I) it = -1;
        const float *row = it >= 0 ? a.Y + (a.U + it) * a.ldy + kq : nullptr;
#pragma unroll
        for (int b = 0; b < AUD_MAXB; ++b) {
            if (!(b < NB && (a.used >> b & 1))) continue;    // (uniform)
            if (D) {
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) qa[b][ks] = row ? row[b * D + 4 * ks] : 0.f;
            } else {
                for (int ks = 0; ks < d / 4; ++ks) s_a[(rank[b] * (d / 4) + ks) * 64 + lane] = row ? row[b * d + 4 * ks] : 0.f;
            }
        }
    }
    // the four items this lane's accumulators belong to: reciprocal head norms, thresholds (+inf: nothing is kept)
    float invq[4][AUD_MAXB - 1], thr[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t q = q0 + 4 * kq + r;
        int64_t it = q < a.Q ? (int64_t)a.items[q] : -1;
        if (it >= a.I) it = -1;
#pragma unroll
        for (int h = 0; h < AUD_MAXB - 1; ++h)
            invq[r][h] = (it >= 0 && h < S && (a.used >> (h + 1) & 1)) ? inv_norm(a.sqn[(a.U + it) * NB + h + 1]) : 0.f;
        thr[r] = knn_thr0(it >= 0);
    }
    if (lane < 16) {
        const int64_t q = q0 + lane;
        int64_t it = q < a.Q ? (int64_t)a.items[q] : -1;
        if (it >= a.I) it = -1;
        knn_list_reset(my, lane, it >= 0);
    }

    // a panel of a stage: its rows as float4 over the workgroup; the rows' squared head norms and row sums on the first SR threads
    float4 pf[PFN];
    float sq_pf[AUD_MAXB - 1] = {1.f, 1.f, 1.f}, rs_pf = 0.f;
    auto load_stage = [&](int64_t s0, int panel) {
#pragma unroll
        for (int p = 0; p < PFN; ++p) {
            const int e = (tid + NT * p) * 4;
            if (e < SR * PW) {
                const int r = e / PW, c = e - r * PW;
                int col;                                     // the column of Y behind column c of the panel
                if (D) {
                    const int k = c / d;                     // the k-th used block
                    int b = 0;
#pragma unroll
                    for (int bb = 0; bb < AUD_MAXB; ++bb) b = (bb < NB && (a.used >> bb & 1) && rank[bb] == k) ? bb : b;
                    col = b * d + (c - k * d);
                } else {
                    int b = 0;
#pragma unroll
                    for (int bb = 0; bb < AUD_MAXB; ++bb) b = (bb < NB && (a.used >> bb & 1) && rank[bb] == panel) ? bb : b;
                    col = b * d + c;
                }
                const int64_t u = s0 + r;
                float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
                if (u < c_end) ELIMREC_LOAD_ROW4(x, a.Y + u * a.ldy + col, a.vec);
                pf[p] = x;
            }
        }
        if (tid < SR && panel == 0) {
            const int64_t u = s0 + tid;
#pragma unroll
            for (int h = 0; h < AUD_MAXB - 1; ++h)
                sq_pf[h] = (u < c_end && h < S && (a.used >> (h + 1) & 1)) ? a.sqn[u * NB + h + 1] : 1.f;
            rs_pf = (u < c_end && tie) ? a.row_sum[u] : 0.f;
        }
    };
    auto store_stage = [&](int panel) {
#pragma unroll
        for (int p = 0; p < PFN; ++p) {
            const int e = (tid + NT * p) * 4;
            if (e < SR * PW) {
                const int r = e / PW, c = e - r * PW;
                *reinterpret_cast<float4 *>(s_b + r * LD + c) = pf[p];
            }
        }
        if (tid < SR && panel == 0) {
#pragma unroll
            for (int h = 0; h < AUD_MAXB - 1; ++h) s_inv[tid * AUD_MAXB + 1 + h] = inv_norm(sq_pf[h]);
            s_mean[tid] = rs_pf / a.I_total;
        }
    };

    aud_v4f acc[AUD_MAXB];
    int64_t s0 = c_begin;
    int panel = 0;
    load_stage(s0, 0);
    store_stage(0);
    __syncthreads();
    while (true) {
        int npanel = panel + 1;
        int64_t ns0 = s0;
        if (npanel == NP) { npanel = 0; ns0 = s0 + SR; }
        const bool more = ns0 < c_end;                       // workgroup-uniform
        if (more) load_stage(ns0, npanel);
#pragma unroll 1
        for (int t = 0; t < SR / 16; ++t) {
            const int64_t t0 = s0 + 16 * t;
            if (t0 >= c_end) break;                          // workgroup-uniform
            const float *bp = s_b + (16 * t + li) * LD + kq;
            if (D) {
#pragma unroll
                for (int b = 0; b < AUD_MAXB; ++b) {
                    acc[b] = (aud_v4f){0.f, 0.f, 0.f, 0.f};
                    if (!(b < NB && (a.used >> b & 1))) continue;    // (uniform)
                    const float *bb = bp + rank[b] * D;
#pragma unroll
                    for (int ks = 0; ks < KS; ++ks) acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[b][ks], bb[4 * ks], acc[b], 0, 0, 0);
                }
            } else {
                aud_v4f cur = (aud_v4f){0.f, 0.f, 0.f, 0.f};
                const float *ap = s_a + panel * (d / 4) * 64 + lane;
                for (int ks = 0; ks < d / 4; ++ks) cur = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[ks * 64], bp[4 * ks], cur, 0, 0, 0);
#pragma unroll
                for (int b = 0; b < AUD_MAXB; ++b) {
                    const bool mine = b < NB && (a.used >> b & 1) && rank[b] == panel;
                    if (panel == 0 && !mine) acc[b] = (aud_v4f){0.f, 0.f, 0.f, 0.f};
                    if (mine) acc[b] = cur;
                }
                if (panel != NP - 1) continue;               // (uniform) the other blocks' dots are still to come
            }
            // lane: user t0 + li against items 4 kq + r of this wave
            const int64_t cand = t0 + li;
            const bool cand_ok = cand < c_end;
            float invu[AUD_MAXB - 1];
#pragma unroll
            for (int h = 0; h < AUD_MAXB - 1; ++h) invu[h] = s_inv[(16 * t + li) * AUD_MAXB + 1 + h];
            const float m = s_mean[16 * t + li];
            float s[4];
            bool pass[4], any = false;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float z[4];
#pragma unroll
                for (int h = 0; h < AUD_MAXB - 1; ++h) z[h] = (acc[h + 1][r] * invu[h]) * invq[r][h];
                z[3] = 0.f;
                s[r] = aud_score<FAST>(a.predict_type, a.fusion_mode, S, a.head_mask, acc[0][r], z, m);
                pass[r] = cand_ok && s[r] > thr[r];
                any = any || pass[r];
            }
            if (__ballot(any) == 0ull) continue;             // wave-uniform: the steady state
            KNN_OFFER(my, E, K, lane, kq, q0, cand, s, pass, thr, a.excl_ptr, a.excl_users, true);
        }
        __syncthreads();                                     // every wave is done with the panel
        if (more) store_stage(npanel);
        __syncthreads();
        if (!more) break;
        s0 = ns0;
        panel = npanel;
    }

    KNN_FLUSH(my, E, K, lane, q0, a.Q, a.n_chunks, chunk, a.ws_val, a.ws_idx);
}

__global__ __launch_bounds__(256) void audience_hits_kernel(const int32_t *__restrict__ lists, int64_t Q, int K,
                                                            const int64_t *__restrict__ ptr, const int32_t *__restrict__ users,
                                                            int32_t *__restrict__ count) {
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= Q) return;                                      // (wave-uniform; no barrier below)
    const int64_t e0 = ptr[q], e1 = ptr[q + 1];
    int n = 0;
    for (int k = lane; k < K; k += 64) {
        const int x = lists[q * K + k];
        if (x < 0) continue;
        bool hit = false;
        for (int64_t e = e0; e < e1 && !hit; ++e) hit = users[e] == x;
        n += hit ? 1 : 0;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off, 64);
    if (lane == 0) count[q] = n;
}

template <int D, int W, bool FAST>
static int aud_launch(const AudArgs &a, int64_t n_tiles, hipStream_t s) {
    return knn_launch_chunks("audience_topk", audience_chunk_kernel<D, W, FAST>, a, n_tiles, a.n_chunks, 64 * W,
                             aud_lds_bytes(D, W, a.d, aud_popc(a.used), a.K), s);
}

template <bool FAST>
static int aud_dispatch(const AudArgs &a, int64_t Q, hipStream_t s) {
    const bool wide = a.K <= KNN_SMALLK && (a.d == 32 || a.d == 64);
    const int rows = wide ? KNN_TILE : 16;
    const int64_t n_tiles = (Q + rows - 1) / rows;
    ELIMREC_REQUIRE(n_tiles < (int64_t)INT32_MAX, "audience_topk: too many item tiles for one launch");
    if (a.d == 32) return wide ? aud_launch<32, 4, FAST>(a, n_tiles, s) : aud_launch<32, 1, FAST>(a, n_tiles, s);
    if (a.d == 64) return wide ? aud_launch<64, 4, FAST>(a, n_tiles, s) : aud_launch<64, 1, FAST>(a, n_tiles, s);
    return aud_launch<0, 1, FAST>(a, n_tiles, s);
}

}  // namespace elimrec

using namespace elimrec;

extern "C" int elimrec_audience_topk_chunk(void) { return KNN_CHUNK; }
extern "C" int elimrec_audience_topk_tile(void) { return KNN_TILE; }

extern "C" size_t elimrec_audience_topk_workspace(int64_t Q, int64_t U, int K) {
    return knn_workspace_bytes(Q, U, K);
}

extern "C" int elimrec_audience_topk(const float *d_Y, int64_t ldy, int64_t U, int64_t I, int d, int S, uint32_t head_mask, int fusion_mode,
                                     int predict_type, const float *d_sqnorm, const float *d_row_sum, int64_t I_total,
                                     const int32_t *d_items, int64_t Q, const int64_t *d_excl_ptr, const int32_t *d_excl_users, int K,
                                     int32_t *d_idx, float *d_val, void *d_workspace, size_t workspace_bytes, void *stream) {
    if (int rc = knn_check_k("audience_topk", K)) return rc;
    if (int rc = table_dims("audience_topk", d, 1)) return rc;
    ELIMREC_REQUIRE(S >= 0 && S <= AUD_MAXB - 1, "audience_topk: 0 <= S <= %d, got %d", AUD_MAXB - 1, S);
    ELIMREC_REQUIRE(fusion_mode >= 0 && fusion_mode <= 2 && predict_type >= 0 && predict_type <= 2,
                    "audience_topk: fusion mode %d / predict type %d outside 0 .. 2", fusion_mode, predict_type);
    ELIMREC_REQUIRE(Q >= 0 && U >= 0 && I >= 0 && U < (int64_t)INT32_MAX - KNN_CHUNK && I < (int64_t)INT32_MAX,
                    "audience_topk: need Q >= 0, 0 <= U < 2^31 - %d and 0 <= I < 2^31", KNN_CHUNK + 1);
    ELIMREC_REQUIRE(ldy >= (int64_t)(1 + S) * d, "audience_topk: ldy < (1 + S) d");
    if (Q == 0) return 0;
    ELIMREC_REQUIRE(d_items && d_idx && d_workspace, "audience_topk: null pointer");
    if (int rc = knn_check_buffers("audience_topk", d_excl_ptr, d_excl_users, d_workspace, workspace_bytes, Q, U, K)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (U == 0 || I == 0) return knn_fill_empty("audience_topk", d_idx, d_val, Q, K, s);    // no users, or no catalogue to query
    int used = 1;                                            // block 0 always; a head's block if the fusion reads its cosine
    for (int h = 0; h < S; ++h)
        if (predict_type != 0 && (fusion_mode != 0 || (head_mask >> h & 1u))) used |= 1 << (h + 1);
    ELIMREC_REQUIRE(d_Y, "audience_topk: null pointer");
    ELIMREC_REQUIRE(used == 1 || d_sqnorm, "audience_topk: the heads' cosines need d_sqnorm");
    ELIMREC_REQUIRE(predict_type != 2 || (d_row_sum && I_total > 0), "audience_topk: TIE needs d_row_sum and I_total > 0");
    KnnWorkspace ws;
    if (int rc = knn_carve("audience_topk", "items", Q, U, K, d_workspace, &ws)) return rc;
    AudArgs a;
    a.Y = d_Y; a.ldy = ldy; a.U = U; a.I = I; a.d = d; a.S = S;
    a.head_mask = head_mask; a.fusion_mode = fusion_mode; a.predict_type = predict_type;
    a.sqn = d_sqnorm; a.row_sum = d_row_sum; a.I_total = (float)(I_total > 0 ? I_total : 1);
    a.items = d_items; a.Q = Q; a.excl_ptr = d_excl_ptr; a.excl_users = d_excl_users;
    a.K = K; a.n_chunks = (int)ws.n_chunks; a.vec = table_vec(d_Y, ldy); a.used = used;
    a.ws_val = ws.val; a.ws_idx = ws.idx;
    if (int rc = with_fast(elimrec_score_get_math() != 0, [&](auto fast) { return aud_dispatch<fast.value>(a, Q, s); })) return rc;
    return knn_merge(ws, Q, K, d_idx, d_val, stream);
}

extern "C" int elimrec_audience_hits(const int32_t *d_lists, int64_t Q, int K, const int64_t *d_ptr, const int32_t *d_users,
                                     int32_t *d_count, void *stream) {
    ELIMREC_REQUIRE(Q >= 0 && K >= 1, "audience_hits: need Q >= 0 and K >= 1");
    if (Q == 0) return 0;
    ELIMREC_REQUIRE(d_lists && d_ptr && d_users && d_count, "audience_hits: null pointer");
    ELIMREC_REQUIRE((Q + 3) / 4 < (int64_t)INT32_MAX, "audience_hits: too many rows for one launch");
    hipLaunchKernelGGL(audience_hits_kernel, dim3((unsigned)((Q + 3) / 4)), dim3(256), 0, (hipStream_t)stream, d_lists, Q, K, d_ptr, d_users,
                       d_count);
    ELIMREC_LAUNCH_CHECK("audience_hits");
    return 0;
}
