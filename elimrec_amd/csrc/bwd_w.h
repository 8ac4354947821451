// Weight-gradient contraction (gemm.hip): problem table, decomposition and the fixed-order slab reduce, shared with the
// hop launches that can carry either phase as extra workgroups (slab.hip, elimrec_slab_hop_bwd_w).
#pragma once
#include "common.h"
#include <cstdlib>

namespace elimrec {

constexpr int kMaxBatch = 8;
typedef float v16f __attribute__((ext_vector_type(16)));
constexpr int TN1 = 64, TN2 = 64, TRB = 32;                    // output tile (one 32 x 32 MFMA tile per wave); rows per LDS stage
constexpr int ZT = 2;                                             // output tiles of one row chunk that ONE workgroup owns (below)
constexpr int BC4 = TN2 / 4, BRP = 256 / BC4, BPS = TRB / BRP;    // B loader geometry: float4 per row, rows per pass, passes

struct BwdProblem {
    elimrec_linear_bwd_desc d;
    int chunk_rows, chunks, t1, t2;       // decomposition
    int first_block;                      // prefix of (chunks * t1 * ceil(t2 / ZT)) over the problems before this one
    float *slabs, *cslabs;
};
struct BwdBatch { BwdProblem p[kMaxBatch]; int n; };

// One workgroup of the partial launch: a chunk of rows x a PAIR of adjacent 64 x TN2 output tiles (see gemm.hip, "weight grad").
// The chunk's A rows are fetched and staged once for both tiles of the pair (a 64 x 128 problem is one workgroup per chunk, a
// 64 x 256 one two; four tiles would need 64 accumulators + 40 staging registers: more than five workgroups per CU leave).
// As / Bs: the caller's LDS stages ([2][TRB * TN1], [2][TRB * TN2] floats = 32 KB: five workgroups per CU): As[s & 1] holds the A rows
// of stage s, Bs[z] the B rows of tile z of the stage being multiplied (one stage of each: two barriers per stage, around the
// store). The global loads of stage s + 1 are in flight during the MFMAs of stage s; a second register set (two stages ahead)
// does not fit the 96 registers of five workgroups per CU beside two accumulator tiles. The per-row weights of the weighted
// column sum stay in registers: lane k of wave 0 holds row k's, the sum reads it with v_readlane.
// The rows enter every output element's sum as before -- the same MFMA sequence over the same operands per element --, and
// the slab layout is the reduce's: same bits.
struct BwdStage { float4 a[2], b[ZT][BPS]; float w; };
__device__ __forceinline__ void bwd_w_partial_body(const BwdBatch &batch, int block, float (*As)[TRB * TN1], float (*Bs)[TRB * TN2]) {
    static_assert(ZT == 2 && TN2 == 64, "two B tiles share the two Bs stages");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int pi = 0;
    while (pi + 1 < batch.n && block >= batch.p[pi + 1].first_block) ++pi;
    const BwdProblem &pb = batch.p[pi];
    const int local = block - pb.first_block;
    const int n1_tiles = pb.t1, n2_tiles = pb.t2, n2_pairs = (n2_tiles + ZT - 1) / ZT;
    const int chunk = local / (n1_tiles * n2_pairs);
    const int tile = local - chunk * (n1_tiles * n2_pairs);
    const int tile_y = tile / n2_pairs, pair_z = tile - tile_y * n2_pairs;
    const float *__restrict__ A = pb.d.d_A;
    const float *__restrict__ B = pb.d.d_B;
    const int32_t *__restrict__ row_index = pb.d.d_row_index;
    const int32_t *__restrict__ range = pb.d.d_range;
    const int64_t lda = pb.d.lda, ldb = pb.d.ldb, R = pb.d.R;
    const int n1 = pb.d.n1, n2 = pb.d.n2, chunk_rows = pb.chunk_rows;
    float *__restrict__ slabs = pb.slabs;
    // the column sum is a function of the A rows alone: the workgroup of the first pair forms it
    float *__restrict__ colsum_slabs = (pb.d.d_colsum && pair_z == 0) ? pb.cslabs : nullptr;
    const float *__restrict__ cw = colsum_slabs ? pb.d.d_colsum_weight : nullptr;
    int64_t rb = 0, re = R;
    if (range) { rb = range[0]; re = range[1]; }
    const int64_t r0 = rb + (int64_t)chunk * chunk_rows;
    const int64_t r1 = (r0 + chunk_rows < re) ? r0 + chunk_rows : re;
    const int i_base = tile_y * TN1, j_base = pair_z * ZT * TN2;
    const bool tile1 = pair_z * ZT + 1 < n2_tiles;        // the pair's second tile exists

    // loader geometry: A block = 32 rows x 16 float4 (2 per thread); a B tile likewise (BPS per thread and tile)
    const int a_row = tid >> 4, a_c4 = tid & 15;          // + 16 rows on the second pass
    const int b_row = tid / BC4, b_c4 = tid % BC4;        // + BRP rows per pass, BPS passes
    const bool a_col_ok = (i_base + a_c4 * 4) < n1;       // n1, n2 are multiples of 4
    const bool b_col_ok0 = (j_base + b_c4 * 4) < n2;
    const bool b_col_ok1 = tile1 && (j_base + TN2 + b_c4 * 4) < n2;
    BwdStage P;                                            // the stage in flight
    P.w = 1.f;
    float rw_cur = 1.f;                                    // the weights of the stage in LDS
    auto load_block = [&](BwdStage &g, int64_t row0) {
        if (cw && tid < TRB) {
            const int64_t r = row0 + tid;
            g.w = r < r1 ? cw[row_index ? (int64_t)row_index[r] : r] : 0.f;
        }
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int64_t r = row0 + a_row + 16 * p;
            g.a[p] = (a_col_ok && r < r1) ? *reinterpret_cast<const float4 *>(A + r * lda + i_base + a_c4 * 4)
                                          : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int p = 0; p < BPS; ++p) {
            const int64_t r = row0 + b_row + BRP * p;
            float4 v0 = make_float4(0.f, 0.f, 0.f, 0.f), v1 = v0;
            if ((b_col_ok0 || b_col_ok1) && r < r1) {
                const int64_t br = row_index ? (int64_t)row_index[r] : r;
                const float *src = B + br * ldb + j_base + b_c4 * 4;
                if (b_col_ok0) v0 = *reinterpret_cast<const float4 *>(src);
                if (b_col_ok1) v1 = *reinterpret_cast<const float4 *>(src + TN2);
            }
            g.b[0][p] = v0;
            g.b[1][p] = v1;
        }
    };
    auto store_block = [&](const BwdStage &g, int abuf) {
        rw_cur = g.w;
#pragma unroll
        for (int p = 0; p < 2; ++p)
            *reinterpret_cast<float4 *>(&As[abuf][(a_row + 16 * p) * TN1 + a_c4 * 4]) = g.a[p];
#pragma unroll
        for (int p = 0; p < BPS; ++p) {
            *reinterpret_cast<float4 *>(&Bs[0][(b_row + BRP * p) * TN2 + b_c4 * 4]) = g.b[0][p];
            if (tile1) *reinterpret_cast<float4 *>(&Bs[1][(b_row + BRP * p) * TN2 + b_c4 * 4]) = g.b[1][p];
        }
    };

    const int wi = (wave & 1) * 32, wj = (wave >> 1) * (TN2 / 2);
    const int li = lane & 31, lk = lane >> 5;
    // a problem narrower than its tiles: the waves of an empty half do not multiply zeros or write them (the reduce never reads
    // the padding columns)
    const bool wave_on0 = (j_base + wj) < n2;
    const bool wave_on1 = tile1 && (j_base + TN2 + wj) < n2;
    v16f acc0 = {0}, acc1 = {0};
    float csum = 0.f;                                      // threads 0..63: column sum of A[:, i_base + tid]
    auto multiply = [&](int abuf) {
        const float *as = As[abuf], *bs0 = Bs[0], *bs1 = Bs[1];
        if (wave_on1) {                                    // (wave_on1 implies wave_on0)
#pragma unroll
            for (int kk = 0; kk < TRB; kk += 2) {
                const float a = as[(kk + lk) * TN1 + wi + li];
                const float b0 = bs0[(kk + lk) * TN2 + wj + li];
                const float b1 = bs1[(kk + lk) * TN2 + wj + li];
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b0, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b1, acc1, 0, 0, 0);
            }
        } else if (wave_on0) {
#pragma unroll
            for (int kk = 0; kk < TRB; kk += 2) {
                const float a = as[(kk + lk) * TN1 + wi + li];
                const float b0 = bs0[(kk + lk) * TN2 + wj + li];
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b0, acc0, 0, 0, 0);
            }
        }
        if (colsum_slabs && tid < TN1) {
            if (cw) {
#pragma unroll
                for (int k = 0; k < TRB; ++k)
                    csum += as[k * TN1 + tid] * __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, rw_cur), k));
            } else {
#pragma unroll 8
                for (int k = 0; k < TRB; ++k) csum += as[k * TN1 + tid];
            }
        }
    };
    if (r0 < r1) {
        load_block(P, r0);
        store_block(P, 0);
    }
    __syncthreads();
    int buf = 0;
    for (int64_t row0 = r0; row0 < r1; row0 += TRB) {
        const bool more = (row0 + TRB) < r1;
        if (more) load_block(P, row0 + TRB);               // in flight during the MFMAs below
        multiply(buf);
        if (!more) break;
        __syncthreads();                                   // every wave is done with Bs
        store_block(P, buf ^ 1);
        __syncthreads();
        buf ^= 1;
    }
    const int n1_pad = n1_tiles * TN1, n2_pad = n2_tiles * TN2;
    float *slab = slabs + (size_t)chunk * n1_pad * n2_pad;
    if (wave_on0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = i_base + wi + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            slab[(size_t)row * n2_pad + j_base + wj + li] = acc0[r];
            if (wave_on1) slab[(size_t)row * n2_pad + j_base + TN2 + wj + li] = acc1[r];
        }
    }
    if (colsum_slabs && tid < TN1) colsum_slabs[(size_t)chunk * n1_pad + i_base + tid] = csum;
}

// lane q of an output element's four: chunks q, q+4, q+8, ... in that order, four loads in flight
__device__ __forceinline__ float slab_lane_sum(const float *src, size_t stride, int chunks, int q) {
    float s = 0.f;
    int c = q;
    for (; c + 12 < chunks; c += 16) {
        const float v0 = src[(size_t)c * stride], v1 = src[(size_t)(c + 4) * stride];
        const float v2 = src[(size_t)(c + 8) * stride], v3 = src[(size_t)(c + 12) * stride];
        s += v0; s += v1; s += v2; s += v3;
    }
    for (; c < chunks; c += 4) s += src[(size_t)c * stride];
    return s;
}

// out[e] (+)= sum over chunks of slab[chunk][e] in a FIXED order: four adjacent lanes share one output
// element, lane q adds chunks q, q+4, q+8, ... (4 loads in flight each), then (q0+q1)+(q2+q3).
// by selects the problem; 256 threads per workgroup.
__device__ __forceinline__ void reduce_slabs_body(const BwdBatch &batch, int bx, int by) {
    const BwdProblem &pb = batch.p[by];
    const int n1 = pb.d.n1, n2 = pb.d.n2;
    const int n1_pad = pb.t1 * TN1, n2_pad = pb.t2 * TN2;
    const int gid = bx * 256 + (int)threadIdx.x;
    const int idx = gid >> 2, q = gid & 3;
    const int total = n1 * n2;
    int64_t rows = pb.d.d_range ? (int64_t)pb.d.d_range[1] - pb.d.d_range[0] : pb.d.R;
    if (rows < 0) rows = 0;
    const int chunks = (int)((rows + pb.chunk_rows - 1) / pb.chunk_rows);
    const float *src = nullptr;
    size_t stride = 0;
    float *dst = nullptr;
    if (idx < total) {
        const int i = idx / n2, j = idx - i * n2;
        src = pb.slabs + (size_t)i * n2_pad + j;
        stride = (size_t)n1_pad * n2_pad;
        dst = pb.d.d_out + (int64_t)i * pb.d.ldo + j;
    } else if (pb.d.d_colsum && idx < total + n1) {
        src = pb.cslabs + (idx - total);
        stride = (size_t)n1_pad;
        dst = pb.d.d_colsum + (idx - total);
    }
    float s = src ? slab_lane_sum(src, stride, chunks, q) : 0.f;
    s += __shfl_xor(s, 1, 64);       // (q0+q1), (q2+q3)
    s += __shfl_xor(s, 2, 64);       // sum of the two pairs
    if (src && q == 0) *dst = pb.d.accumulate ? (*dst + s) : s;
}


// The slab reduce with the optimizer behind it (the last adjoint hop's launch, slab.hip: sell_tier_adam_fold_kernel): what the
// projection weights' optimizer spans need of a problem. The thread group that owns an output element forms the gradient as
// reduce_slabs_body does, stores it, and applies Adam to the element at once -- the reduced gradient is not read back by a later
// launch. A span's pointers are those of the element the problem's output element 0 updates; p_in == nullptr: store only.
struct FoldSpan {
    const float *p_in;
    float *p_out, *m, *v, *copy_dst;       // copy_dst nullable: the pre-update parameters (the weight snapshot)
    float step_size, inv_sqrt_bc2;
};
struct FoldProblem {
    const float *slabs, *cslabs;           // cslabs == nullptr: no column sum
    const int32_t *range;
    float *out, *colsum;
    int64_t R, ldo;
    int chunk_rows, n1, n2, n1_pad, n2_pad, accumulate;
    FoldSpan w, b;                         // out's / colsum's elements
};
struct FoldBatch { FoldProblem p[kMaxBatch]; int n, gx; };

__device__ __forceinline__ void reduce_adam_body(const FoldBatch &batch, int bx, int by, float beta1, float beta2, float eps, float wd) {
    const FoldProblem &pb = batch.p[by];
    const int gid = bx * 256 + (int)threadIdx.x;
    const int idx = gid >> 2, q = gid & 3;
    const int total = pb.n1 * pb.n2;
    int64_t rows = pb.range ? (int64_t)pb.range[1] - pb.range[0] : pb.R;
    if (rows < 0) rows = 0;
    const int chunks = (int)((rows + pb.chunk_rows - 1) / pb.chunk_rows);
    // (the span's fields are picked by value: a pointer into the by-value argument block would put the whole block into scratch)
    const bool is_w = idx < total, is_b = !is_w && pb.cslabs && idx < total + pb.n1;
    const float *src = nullptr;
    size_t stride = 0;
    int64_t at = 0;
    if (is_w) {
        const int i = idx / pb.n2, j = idx - i * pb.n2;
        src = pb.slabs + (size_t)i * pb.n2_pad + j;
        stride = (size_t)pb.n1_pad * pb.n2_pad;
        at = (int64_t)i * pb.ldo + j;
    } else if (is_b) {
        src = pb.cslabs + (idx - total);
        stride = (size_t)pb.n1_pad;
        at = idx - total;
    }
    float s = src ? slab_lane_sum(src, stride, chunks, q) : 0.f;
    s += __shfl_xor(s, 1, 64);       // (q0+q1), (q2+q3)
    s += __shfl_xor(s, 2, 64);       // sum of the two pairs
    if (!src || q != 0) return;
    float *dst = (is_w ? pb.out : pb.colsum) + at;
    const float g = pb.accumulate ? (*dst + s) : s;
    *dst = g;
    const float *p_in = is_w ? pb.w.p_in : pb.b.p_in;
    if (!p_in) return;
    float *p_out = is_w ? pb.w.p_out : pb.b.p_out, *m = is_w ? pb.w.m : pb.b.m, *v = is_w ? pb.w.v : pb.b.v;
    float *copy_dst = is_w ? pb.w.copy_dst : pb.b.copy_dst;
    const float step_size = is_w ? pb.w.step_size : pb.b.step_size, inv_sqrt_bc2 = is_w ? pb.w.inv_sqrt_bc2 : pb.b.inv_sqrt_bc2;
    const float pi = p_in[at];                              // arithmetic of adam_jobs_body (slab.hip), element for element
    if (copy_dst) copy_dst[at] = pi;
    const float gi = fmaf(wd, pi, g);
    const float mo = m[at];
    const float mi = mo + (1.f - beta1) * (gi - mo);
    const float vi = fmaf(1.f - beta2, gi * gi, beta2 * v[at]);
    const float denom = sqrtf(vi) * inv_sqrt_bc2 + eps;
    m[at] = mi;
    v[at] = vi;
    p_out[at] = pi - step_size * (mi / denom);
}


// ---- host side
// Row-chunk size: the partial kernel holds 48 KB of LDS, i.e. 3 workgroups per CU = 768 resident at once;
// chunks are sized so that one problem's workgroups fill about a third of that (batches hold ~3 problems
// of equal weight) in ONE round, between 64 and 512 rows.
static inline void bwd_w_dims(int64_t R, int n1, int n2, int &chunk_rows, int &chunks, int &t1, int &t2) {
    const int tiles = ((n1 + TN1 - 1) / TN1) * ((n2 + TN2 - 1) / TN2);
    static int target = 0;
    if (!target) target = 480;
    int64_t want = (R * tiles + target - 1) / target;       // rows per workgroup for ~`target` workgroups per problem
    want = (want + TRB - 1) / TRB * TRB;
    chunk_rows = (int)(want < 64 ? 64 : (want > 512 ? 512 : want));
    chunks = (int)((R + chunk_rows - 1) / chunk_rows);
    if (chunks < 1) chunks = 1;
    t1 = (n1 + TN1 - 1) / TN1;
    t2 = (n2 + TN2 - 1) / TN2;
}

static inline size_t bwd_w_bytes(int64_t R, int n1, int n2) {
    int cr, chunks, t1, t2;
    bwd_w_dims(R, n1, n2, cr, chunks, t1, t2);
    return align_up(((size_t)chunks * t1 * TN1 * t2 * TN2 + (size_t)chunks * t1 * TN1) * sizeof(float), 256);
}


// fills the problem table of `n` contractions whose slabs live in d_workspace; blocks = workgroups of the partial launch,
// max_out = the largest problem's output elements (the reduce runs a (4 * max_out / 256) x n grid)
static inline int bwd_w_build_batch(const elimrec_linear_bwd_desc *descs, int n, void *d_workspace, BwdBatch &batch, int &blocks,
                                    int &max_out) {
    batch.n = n;
    char *ws = (char *)d_workspace;
    blocks = 0; max_out = 0;
    for (int i = 0; i < n; ++i) {
        const elimrec_linear_bwd_desc &d = descs[i];
        ELIMREC_REQUIRE(d.d_A && d.d_B && d.d_out, "linear_bwd_w: null pointer");
        ELIMREC_REQUIRE(d.R >= 0 && d.n1 > 0 && d.n2 > 0, "linear_bwd_w: bad shape");
        ELIMREC_REQUIRE(d.n1 % 4 == 0 && d.n2 % 4 == 0 && d.lda % 4 == 0 && d.ldb % 4 == 0,
                        "linear_bwd_w: n1, n2, lda, ldb must be multiples of 4");
        ELIMREC_REQUIRE(((uintptr_t)d.d_A % 16) == 0 && ((uintptr_t)d.d_B % 16) == 0,
                        "linear_bwd_w: A and B must be 16-byte aligned");
        BwdProblem &pb = batch.p[i];
        pb.d = d;
        bwd_w_dims(d.R, d.n1, d.n2, pb.chunk_rows, pb.chunks, pb.t1, pb.t2);
        pb.first_block = blocks;
        blocks += pb.chunks * pb.t1 * ((pb.t2 + ZT - 1) / ZT);
        pb.slabs = (float *)ws;
        pb.cslabs = pb.slabs + (size_t)pb.chunks * pb.t1 * TN1 * pb.t2 * TN2;
        ws += bwd_w_bytes(d.R, d.n1, d.n2);
        const int out_elems = d.n1 * d.n2 + (d.d_colsum ? d.n1 : 0);
        if (out_elems > max_out) max_out = out_elems;
    }
    return 0;
}

static inline size_t bwd_w_batched_bytes(const elimrec_linear_bwd_desc *descs, int n) {
    size_t total = 0;
    for (int i = 0; i < n; ++i) total += bwd_w_bytes(descs[i].R, descs[i].n1, descs[i].n2);
    return total;
}

}  // namespace elimrec
