// torch.ops.elimrec.* : a thin TORCH_LIBRARY registration over the C ABI of libelimrec_hip.so (include/elimrec_hip.h),
// the form SURVEY.md 8(b) names for a PyTorch host. Nothing is computed here: every op checks its tensors, unpacks
// pointers / strides, takes torch's current HIP stream, allocates its outputs and scratch with torch and calls ONE
// entry point of the C ABI; failures become c10::Error (RuntimeError in Python) carrying elimrec_last_error().
// The ctypes binding (elimrec_amd/_lib.py) stays for hosts without torch; both call the same library.
//
//   propagate(rowptr i32[N+1], col i32[nnz], val f32[nnz], X f32[N x C], L, transpose=False) -> mean over the L+1 layer tables
//       (transpose: with A^T -- the adjoint of a propagation matrix that is not self-adjoint)
//   segment_reduce(rows f32[n x ld], keys i32[n], split_key) -> (active keys, summed rows, seg_info): the deterministic
//       index_put(accumulate) of the backward pass; bpr_head_fwd's grad_rows + keys are its inputs (= "bpr_head_bwd")
//   linear_fwd(A, W, bias?) -> A W^T + bias                linear_bwd_w(A, B) -> (A^T B, column sums of A)
//   bpr_head_fwd(Y, U, I, users, pos, neg, d, block_weights) -> (loss_rows, grad_rows, keys)
//   adam_step_(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step) -> p
//   score_topk(Y, U, I, users, d, S, head_mask, fusion_mode, predict_type, train_ptr?, train_items?, K, tie_order=0) -> (idx, val)
//       (tie_order 1: the reference's partial_sort_copy order among equal scores, evaluate.h:26-33, replayed on the device)
//   rank_metrics(topk_idx, truth_ptr, truth_items, metric_ids) -> f32[B x n_metrics x K]
//   group_metric_means(rows f32[n x C], group_ptr i64[G+1], group_rows i32) -> f32[G x C]: per CSR segment of row indices the
//       column means, float64 sums in listed order (the indices are checked on the host first: a synchronisation)
//   rank_targets(scores f32[B x I], tgt_ptr i64[B+1], tgt_items i32) -> i32[n_targets]: the 0-based position of every listed item in
//       its row's full ranking by (score desc, id asc), -1 at -inf (the lists are checked on the host first: a synchronisation)
//   rank_values(scores f32[B x I], val_ptr i64[B+1], vals f32, skip i32?) -> i32[n_vals]: #{j != skip: scores[b, j] >= v}, where a new
//       item of that score would land in the row's full ranking; -1 for a value that is not finite (csrc/coldstart.hip)
//   segment_row_sum(table f32[n x C], ptr i64[Q+1], rows i32, weights f32, row_offset) -> f32[Q x C]: per list the weighted sum of
//       the rows table[row_offset + rows[j]], float64 products and sums rounded once (csrc/foldin.hip; ids and weights are
//       checked on the host first: a synchronisation)
//   list_pair_cosine(table f32[n x blocks*d], sqnorm f32[n x blocks], lists i32[B x K], blocks) -> f32[B x blocks]: per list and
//       column block the mean pairwise cosine of the listed rows (entries outside [0, n) are not listed; NaN below two)
//   list_exposure(lists i32[B x K], n_rows) -> i32[n_rows]: how often every row is listed
//   mmr_rerank(table f32[n x d], sqnorm f32[n], pool_idx i32[B x N], pool_val f32[B x N], K, lam) -> (idx i32, pos i32, val f32) [B x K]:
//       greedy maximal-marginal-relevance re-ranking of each pool (unlisted entries are never picked; -1 / -1 / -inf fillers)
//   calibrate_rerank(pool_idx i32[B x N], pool_val f32[B x N], class_of i32[I], target f32[B x C], K, lam, smooth) -> (idx i32, pos i32, val f32)
//       [B x K]: greedy calibrated re-ranking of each pool towards the row's target class shares, the objective in float64
//       (lam weighs the relevance; csrc/calibrate.hip)
//   list_calibration(lists i32[B x K], class_of i32[I], C, target f32[B x C], smooth) -> (shares f32[B x C], kl f32[B]): the class shares of
//       every list and its miscalibration C_KL against the row's target
//   kmeans_assign(table f32[n x d], sqnorm f32[n], centroids f32[C x d], centroid_sqnorm f32[C], prev i32[n]?) -> (assign i32[n], cos f32[n],
//       changed i32[1]): per row the centroid with the largest cosine, the lowest id among equals; -1 / -inf for a row without a norm
//   kmeans_update(table, sqnorm, assign i32[n], centroids, centroid_sqnorm) -> (centroids f32[C x d], centroid_sqnorm f32[C], sums f64[C x d],
//       counts i32[C]): the normalised float64 sums of the members' unit rows; an empty cluster keeps its centroid (csrc/kmeans.hip)
//   uniformity_sum(table f32[n x d], sqnorm f32[n], rows i32[m], t) -> (sum f64[1], counts i64[2] = (pairs, n_valid)): the sum over the
//       list's positions p < q, both valid, of expf(2 t (cos - 1)); row_gram(table, sqnorm, rows) -> (gram f64[d x d], sum f64[d], count
//       i64[1]): the float64 Gram matrix and sum of the list's unit rows (csrc/geometry.hip)
//   cooccur_topk(q_ptr i64[n + 1], q_nbr i32[E], o_ptr i64[m + 1], o_nbr i32[E], rows i32[Q], K, measure) -> (idx i32, val f32, cnt i32)
//       [Q x K]: per query row the K rows of its side with the largest co-occurrence score ("count", "cosine", "jaccard") over the
//       bipartite graph the two CSRs give, (score descending, id ascending), -1 / -inf / 0 fillers; both CSRs and the rows are checked
//       on the host (csrc/cooccur.hip)
//   walk_topk(q_ptr, q_nbr, o_ptr, o_nbr, rows i32[Q], K, mid_weight i64[m], row_scale f64[n], col_scale f64[n]) -> (idx i32, val f32) [Q x K]:
//       cooccur_topk's lists with every two-step walk q -> u -> j weighing mid_weight[u] (2^-40 fixed point), the int64 sum scaled by
//       row_scale[q] col_scale[j] in float64 and rounded once -- P3alpha / RP3beta; the weights, the scales and the overflow bound are
//       checked on the host (ValueError) (csrc/walk.hip)
//   cross_topk(query_table f32[nq x d], query_sqnorm f32[nq]?, table f32[n x d], sqnorm f32[n]?, query_rows i32[Q], excl_ptr i64[Q + 1]?,
//       excl_rows i32?, K) -> (idx i32, val f32) [Q x K]: cosine_topk with a query table of its own; a missing sqnorm is a vector of ones,
//       without both the score is the plain dot product (csrc/knn.hip)
//   als_solve(ptr i64[n + 1], nbr i32, F f32[n_fixed x d], A0 f64[d x d], reg f64[n], conf, rows i32[Q]?) -> f32[n x d]: one half-sweep of
//       implicit-feedback ALS, out[r] = (A0 + reg[r] I + conf sum f f^T)^-1 (1 + conf) sum f over row r's list, float64 Cholesky per row;
//       rows not listed are zero; the CSR (strictly ascending lists), reg and conf are checked on the host (csrc/als.hip). A row that
//       is not positive definite raises through TORCH_CHECK, a RuntimeError here (ops.als_solve raises ArithmeticError with the same words)
//   gram_counts(q_ptr i64[n + 1], q_nbr i32, o_ptr i64[n_other + 1], o_nbr i32, l2) -> f64[n x n]: the walks i -> u -> j of a bipartite
//       graph + l2 on the diagonal, X^T X + l2 I of a binary X; integer counts, exact (csrc/ease.hip)
//   spd_inverse(A f64[n x n]) -> (inverse f64[n x n], pivot_min f64[1]): the symmetric block sweep in float64 on a copy of A; a matrix
//       that is not positive definite raises through TORCH_CHECK (ops.spd_inverse works in place and raises ArithmeticError)
//   ease_topk(P f64[I x I], hist_ptr i64[R + 1], hist_items i32, excl_ptr i64[R + 1]?, excl_items i32?, users i64[B], K) -> (idx i32,
//       val f32) [B x K]: the K items with the largest -(sum_{i in H, i != j} P_ij) / P_jj, excl's ids (default: the history's) left out
//   neighbour_vote_topk(nbr_idx i32[n x Kn], nbr_val f32[n x Kn], hist_ptr i64[R + 1], hist_items i32, excl_ptr i64[R + 1]?, excl_items i32?,
//       users i64[B], K) -> (idx i32, val f32, cnt i32) [B x K]: the K items the neighbour lists of each user's history vote for, the
//       history's own ids and excl's left out; fixed-point int64 sums, the overflow bound and the form rule on the host (csrc/vote.hip)
//   pick_hard_negatives(user_table f32[U x blocks*d], user_sqnorm f32[U x blocks], item_table f32[I x blocks*d], item_sqnorm, weights
//     float[blocks], users i64[n], cands i32[n x M]) -> (neg i64, pos i32, score f32) [n]: per triplet the listed candidate with the largest
//     sum_b w_b cos_b(u, i), the lowest column among equals; -1 / -1 / -inf without one (csrc/hardneg.hip)
//   history_support(table f32[I x blocks*d], sqnorm f32[I x blocks], weights float[blocks], users i64[B], lists i32[B x K], hist_ptr i64[R + 1],
//     hist_items i32, top, exclude_self) -> (idx i32 [B x K x top], val f32 [B x K x top], cnt i32 [B x K], mean f32 [B x K]): per target the
//     `top` entries of its user's history (segment users[b] of the CSR) with the largest sum_b w_b cos_b, the lower position among equals;
//     -1 / -inf fillers, cnt / mean over the listed entries (csrc/history.hip)
//   bootstrap_means(rows f32[n x C], group_ptr i64[G+1], group_rows i32, R, seed) -> f64[R x G x C]: R bootstrap replicates of every
//     group's column means, the draws fixed by Philox4x32-10 at (seed, r, g, t); bootstrap_diff_means(rows_a, rows_b, ...): the same of
//     the paired differences rows_b - rows_a, taken in float64; blocks wider than 16 columns go through in slices (csrc/bootstrap.hip)
//   audience_topk(Y, U, I, items i32[Q], excl_ptr i64[Q + 1]?, excl_users i32?, d, S, head_mask, fusion_mode, predict_type, K, sqnorm?, row_sum
//     f32[U]? (TIE), I_total) -> (idx i32, val f32) [Q x K]: per query item the K users with the largest predict() score, the item's excluded
//     users left out; -1 / -inf fillers (the ids and the CSR are checked on the host first: a synchronisation; csrc/audience.hip)
//   sample_triplets(user_ids, ptr, items, num_items, n, seed, epoch) -> (users, pos, neg)
//   score_candidates(Y, U, I, users, d, S, head_mask, fusion_mode, predict_type, cand_ptr, cand_items, width) -> f32[B x width]
//       (each row: its candidates' scores in list order, then -inf)
//   sample_negatives(excl_ptr, excl_items, num_items, n_neg, seed) -> i32[n_users x n_neg]
//   score_effects(Y, U, I, users, d, S, head_mask, fusion_mode, cand_ptr, cand_items, width) -> f32[B x width x (6 + S)]
//       (per listed pair: ui, mean_ui, te, nde, score_te, score_tie, one cosine per head; NaN beyond a list and at bad ids)
#include <ATen/ATen.h>
#include <ATen/hip/HIPContext.h>
#include <torch/library.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/elimrec_hip.h"

namespace {

void *cur_stream() { return (void *)at::hip::getCurrentHIPStream().stream(); }

void check(int rc, const char *what) {
    if (rc != 0) {
        const char *msg = elimrec_last_error();
        TORCH_CHECK(false, "elimrec::", what, " failed (rc=", rc, "): ", msg ? msg : "?");
    }
}

void need(const at::Tensor &t, const char *name, at::ScalarType dt, int64_t dim = -1) {
    TORCH_CHECK(t.is_cuda(), "elimrec: '", name, "' must be a HIP device tensor (the hot path has no CPU implementation)");
    TORCH_CHECK(t.scalar_type() == dt, "elimrec: '", name, "' has dtype ", t.scalar_type(), ", expected ", dt);
    TORCH_CHECK(dim < 0 || t.dim() == dim, "elimrec: '", name, "' must be ", dim, "-D");
}

const at::Tensor rowmajor(const at::Tensor &t, const char *name) {
    need(t, name, at::kFloat, 2);
    return t.stride(1) == 1 ? t : t.contiguous();
}

// No unchecked id reaches a kernel: the host checks of id lists, in the ops' own words. index_error: the range failure is an
// IndexError (the ops that mirror ops.py's checked queries) or the plain error of the older ops.
// every id of t in [0, bound), else "elimrec::<who>: <what> span [lo, hi], <has> <bound> <unit>"
void checked_ids(const at::Tensor &t, int64_t bound, bool index_error, const char *who, const char *what, const char *has, const char *unit) {
    if (t.numel() == 0) return;
    const int64_t lo = t.min().item<int64_t>(), hi = t.max().item<int64_t>();
    if (index_error) TORCH_CHECK_INDEX(lo >= 0 && hi < bound, "elimrec::", who, ": ", what, " span [", lo, ", ", hi, "], ", has, " ", bound, " ", unit);
    TORCH_CHECK(lo >= 0 && hi < bound, "elimrec::", who, ": ", what, " span [", lo, ", ", hi, "], ", has, " ", bound, " ", unit);
}

// ptr (n_lists + 1 entries, the caller's check) ascends from 0 to len(ids) ...
void checked_csr(const at::Tensor &ptr, const at::Tensor &ids, int64_t n_lists, const char *who, const char *ptr_name, const char *ids_name) {
    const at::Tensor hp = ptr.cpu();
    const int64_t *p = hp.data_ptr<int64_t>();
    bool ok = p[0] == 0 && p[n_lists] == ids.numel();
    for (int64_t b = 0; b < n_lists && ok; ++b) ok = p[b + 1] >= p[b];
    TORCH_CHECK(ok, "elimrec::", who, ": ", ptr_name, " must ascend from 0 to len(", ids_name, ") = ", ids.numel());
}

// ... and its ids lie in [0, bound)
void checked_csr(const at::Tensor &ptr, const at::Tensor &ids, int64_t n_lists, int64_t bound, bool index_error, const char *who,
                 const char *ptr_name, const char *ids_name, const char *what, const char *has, const char *unit) {
    checked_csr(ptr, ids, n_lists, who, ptr_name, ids_name);
    checked_ids(ids, bound, index_error, who, what, has, unit);
}

at::Tensor propagate(const at::Tensor &rowptr, const at::Tensor &col, const at::Tensor &val, const at::Tensor &X, int64_t L,
                     bool transpose) {
    need(rowptr, "rowptr", at::kInt, 1); need(col, "col", at::kInt, 1); need(val, "val", at::kFloat, 1);
    need(X, "X", at::kFloat, 2);
    const at::Tensor x = X.contiguous();
    at::Tensor rp = rowptr.contiguous(), c = col.contiguous(), v = val.contiguous();
    const int64_t n = x.size(0), C = x.size(1);
    TORCH_CHECK(rp.numel() == n + 1, "elimrec::propagate: rowptr has ", rp.numel(), " entries for ", n, " rows");
    if (transpose) {
        // the adjoint's matrix (SparseAddmmBackward multiplies by A^T; 'pre' is self-adjoint, 'gcmc' / 'norm' are not): CSR of
        // A^T from CSR of A -- index bookkeeping only (a stable sort by column), the propagation itself is the same kernel
        const at::Tensor counts = (rp.slice(0, 1) - rp.slice(0, 0, n)).to(at::kLong);
        const at::Tensor rows = at::repeat_interleave(at::arange(n, counts.options()), counts);
        const at::Tensor cl = c.to(at::kLong);
        const at::Tensor order = at::argsort(cl * n + rows, /*stable=*/true, 0, false);
        rp = at::cat({at::zeros({1}, counts.options()), at::cumsum(at::bincount(cl, {}, n), 0)}).to(at::kInt);
        c = rows.index_select(0, order).to(at::kInt);
        v = v.index_select(0, order);
    }
    at::Tensor out = at::empty_like(x), t0 = at::empty_like(x), t1 = at::empty_like(x);
    check(elimrec_propagate(rp.data_ptr<int32_t>(), c.data_ptr<int32_t>(), v.data_ptr<float>(), n, (int)C, nullptr, (int)L,
                            x.data_ptr<float>(), t0.data_ptr<float>(), t1.data_ptr<float>(), out.data_ptr<float>(), cur_stream()),
          "propagate");
    return out;
}

at::Tensor linear_fwd(const at::Tensor &A, const at::Tensor &W, const c10::optional<at::Tensor> &bias) {
    const at::Tensor a = rowmajor(A, "A"), w = rowmajor(W, "W");
    TORCH_CHECK(a.size(1) == w.size(1), "elimrec::linear_fwd: A is [", a.size(0), " x ", a.size(1), "], W is [", w.size(0), " x ", w.size(1), "]");
    at::Tensor b;
    if (bias.has_value() && bias->defined()) { need(*bias, "bias", at::kFloat, 1); b = bias->contiguous(); }
    at::Tensor out = at::empty({a.size(0), w.size(0)}, a.options());
    check(elimrec_linear_fwd(a.data_ptr<float>(), a.stride(0), w.data_ptr<float>(), w.stride(0), b.defined() ? b.data_ptr<float>() : nullptr,
                             out.data_ptr<float>(), out.stride(0), a.size(0), (int)w.size(0), (int)a.size(1), cur_stream()),
          "linear_fwd");
    return out;
}

std::tuple<at::Tensor, at::Tensor> linear_bwd_w(const at::Tensor &A, const at::Tensor &B) {
    const at::Tensor a = rowmajor(A, "A"), b = rowmajor(B, "B");
    TORCH_CHECK(a.size(0) == b.size(0), "elimrec::linear_bwd_w: row counts differ");
    at::Tensor out = at::empty({a.size(1), b.size(1)}, a.options()), colsum = at::empty({a.size(1)}, a.options());
    const size_t need_ws = elimrec_linear_bwd_w_workspace(a.size(0), (int)a.size(1), (int)b.size(1));
    at::Tensor ws = at::empty({(int64_t)(need_ws ? need_ws : 1)}, a.options().dtype(at::kByte));
    check(elimrec_linear_bwd_w(a.data_ptr<float>(), a.stride(0), b.data_ptr<float>(), b.stride(0), nullptr, nullptr, a.size(0),
                               (int)a.size(1), (int)b.size(1), out.data_ptr<float>(), out.stride(0), colsum.data_ptr<float>(), 0,
                               ws.data_ptr(), (size_t)ws.numel(), cur_stream()),
          "linear_bwd_w");
    return {out, colsum};
}

std::tuple<at::Tensor, at::Tensor, at::Tensor> bpr_head_fwd(const at::Tensor &Y, int64_t U, int64_t I, const at::Tensor &users,
                                                            const at::Tensor &pos, const at::Tensor &neg, int64_t d,
                                                            std::vector<double> block_weights) {
    const at::Tensor y = rowmajor(Y, "Y");
    need(users, "users", at::kLong, 1); need(pos, "pos", at::kLong, 1); need(neg, "neg", at::kLong, 1);
    const int64_t B = users.numel();
    TORCH_CHECK(pos.numel() == B && neg.numel() == B, "elimrec::bpr_head_fwd: users / pos / neg differ in length");
    TORCH_CHECK(y.size(0) == U + I && y.size(1) == d * (int64_t)block_weights.size(), "elimrec::bpr_head_fwd: Y must be [(U+I) x d*blocks]");
    std::vector<float> w(block_weights.begin(), block_weights.end());
    at::Tensor loss = at::empty({B}, y.options()), grad = at::empty({3 * B, y.size(1)}, y.options());
    at::Tensor keys = at::empty({3 * B}, y.options().dtype(at::kInt));
    const at::Tensor u = users.contiguous(), p = pos.contiguous(), n = neg.contiguous();
    check(elimrec_bpr_head(y.data_ptr<float>(), y.stride(0), U, I, u.data_ptr<int64_t>(), p.data_ptr<int64_t>(), n.data_ptr<int64_t>(),
                           (int)B, (int)d, (int)w.size(), w.data(), loss.data_ptr<float>(), grad.data_ptr<float>(),
                           keys.data_ptr<int32_t>(), cur_stream()),
          "bpr_head_fwd");
    return {loss, grad, keys};
}

at::Tensor adam_step_(at::Tensor p, const at::Tensor &g, at::Tensor m, at::Tensor v, double lr, double beta1, double beta2,
                      double eps, double weight_decay, int64_t step) {
    need(p, "p", at::kFloat); need(g, "g", at::kFloat); need(m, "m", at::kFloat); need(v, "v", at::kFloat);
    TORCH_CHECK(p.is_contiguous() && g.is_contiguous() && m.is_contiguous() && v.is_contiguous(), "elimrec::adam_step_: contiguous tensors");
    TORCH_CHECK(g.numel() == p.numel() && m.numel() == p.numel() && v.numel() == p.numel(), "elimrec::adam_step_: sizes differ");
    check(elimrec_adam_step(p.data_ptr<float>(), g.data_ptr<float>(), m.data_ptr<float>(), v.data_ptr<float>(), p.numel(), (float)lr,
                            (float)beta1, (float)beta2, (float)eps, (float)weight_decay, step, cur_stream()),
          "adam_step_");
    return p;
}

std::tuple<at::Tensor, at::Tensor> score_topk(const at::Tensor &Y, int64_t U, int64_t I, const at::Tensor &users, int64_t d, int64_t S,
                                              int64_t head_mask, int64_t fusion_mode, int64_t predict_type,
                                              const c10::optional<at::Tensor> &train_ptr,
                                              const c10::optional<at::Tensor> &train_items, int64_t K, int64_t tie_order) {
    const at::Tensor y = rowmajor(Y, "Y");
    need(users, "users", at::kLong, 1);
    const at::Tensor u = users.contiguous();
    const int64_t B = u.numel();
    TORCH_CHECK(K >= 1, "elimrec::score_topk: K >= 1");
    TORCH_CHECK(tie_order == 0 || tie_order == 1, "elimrec::score_topk: tie_order 0 (score desc, id asc) or 1 (the reference's heap order)");
    at::Tensor tp, ti;
    if (train_ptr.has_value() && train_ptr->defined()) {
        TORCH_CHECK(train_items.has_value() && train_items->defined(), "elimrec::score_topk: train_ptr needs train_items");
        need(*train_ptr, "train_ptr", at::kLong, 1); need(*train_items, "train_items", at::kInt, 1);
        tp = train_ptr->contiguous(); ti = train_items->contiguous();
    }
    at::Tensor idx = at::empty({B, K}, y.options().dtype(at::kInt)), val = at::empty({B, K}, y.options());
    const size_t need_ws = elimrec_score_workspace2((int)B, U, I, (int)S, (int)K);
    at::Tensor ws = at::empty({(int64_t)(need_ws ? need_ws : 1)}, y.options().dtype(at::kByte));
    check(elimrec_score_topk_ordered(y.data_ptr<float>(), y.stride(0), U, I, u.data_ptr<int64_t>(), (int)B, (int)d, (int)S, (uint32_t)head_mask,
                                     (int)fusion_mode, (int)predict_type, nullptr, tp.defined() ? tp.data_ptr<int64_t>() : nullptr,
                                     ti.defined() ? ti.data_ptr<int32_t>() : nullptr, nullptr, 0, (int)K, idx.data_ptr<int32_t>(),
                                     val.data_ptr<float>(), ws.data_ptr(), (size_t)ws.numel(), (int)tie_order, cur_stream()),
          "score_topk");
    return {idx, val};
}

at::Tensor rank_metrics(const at::Tensor &topk_idx, const at::Tensor &truth_ptr, const at::Tensor &truth_items,
                        std::vector<int64_t> metric_ids) {
    need(topk_idx, "topk_idx", at::kInt, 2); need(truth_ptr, "truth_ptr", at::kLong, 1); need(truth_items, "truth_items", at::kInt, 1);
    const at::Tensor t = topk_idx.contiguous(), tp = truth_ptr.contiguous(), ti = truth_items.contiguous();
    std::vector<int> ids(metric_ids.begin(), metric_ids.end());
    at::Tensor out = at::empty({t.size(0), (int64_t)ids.size() * t.size(1)}, t.options().dtype(at::kFloat));
    check(elimrec_rank_metrics(t.data_ptr<int32_t>(), (int)t.size(0), (int)t.size(1), tp.data_ptr<int64_t>(), ti.data_ptr<int32_t>(),
                               ids.data(), (int)ids.size(), out.data_ptr<float>(), cur_stream()),
          "rank_metrics");
    return out;
}

at::Tensor group_metric_means(const at::Tensor &rows, const at::Tensor &group_ptr, const at::Tensor &group_rows) {
    const at::Tensor r = rowmajor(rows, "rows");
    need(group_ptr, "group_ptr", at::kLong, 1); need(group_rows, "group_rows", at::kInt, 1);
    const at::Tensor gp = group_ptr.contiguous(), gr = group_rows.contiguous();
    const int64_t G = gp.numel() - 1, n_listed = gr.numel();
    TORCH_CHECK(G >= 1, "elimrec::group_metric_means: group_ptr needs G + 1 >= 2 entries");
    checked_csr(gp, gr, G, r.size(0), false, "group_metric_means", "group_ptr", "group_rows", "row indices", "the block has", "rows");
    at::Tensor out = at::empty({G, r.size(1)}, r.options());
    const size_t need_ws = elimrec_group_metric_means_workspace(n_listed, (int)r.size(1), (int)G);
    at::Tensor ws = at::empty({(int64_t)(need_ws ? need_ws : 1)}, r.options().dtype(at::kByte));
    at::Tensor none = at::zeros({1}, gr.options());
    check(elimrec_group_metric_means(r.data_ptr<float>(), r.size(0), (int)r.size(1), r.stride(0), gp.data_ptr<int64_t>(),
                                     n_listed ? gr.data_ptr<int32_t>() : none.data_ptr<int32_t>(), n_listed, (int)G, out.data_ptr<float>(),
                                     ws.data_ptr(), (size_t)ws.numel(), cur_stream()),
          "group_metric_means");
    return out;
}

// IndexBackward / index_put(accumulate): rows with equal keys summed in ascending row order, deterministic.
// -> (active keys int32[n] (first n_active valid), reduced f32[n x ld], seg_info int32[8] = {n_active, #keys < split_key, ...})
std::tuple<at::Tensor, at::Tensor, at::Tensor> segment_reduce(const at::Tensor &rows, const at::Tensor &keys, int64_t split_key) {
    need(keys, "keys", at::kInt, 1);
    const at::Tensor r = rowmajor(rows, "rows").contiguous(), k = keys.contiguous();
    const int64_t n = r.size(0), ld = r.size(1);
    TORCH_CHECK(k.numel() == n, "elimrec::segment_reduce: one key per row");
    at::Tensor active = at::empty({n}, k.options()), reduced = at::empty({n, ld}, r.options());
    at::Tensor seg = at::zeros({8}, k.options());
    const size_t need_ws = elimrec_segment_reduce_workspace(n);
    at::Tensor ws = at::empty({(int64_t)(need_ws ? need_ws : 1)}, r.options().dtype(at::kByte));
    check(elimrec_segment_reduce_rows(r.data_ptr<float>(), k.data_ptr<int32_t>(), n, (int)ld, (int32_t)split_key, active.data_ptr<int32_t>(),
                                      reduced.data_ptr<float>(), nullptr, seg.data_ptr<int32_t>(), ws.data_ptr(), (size_t)ws.numel(),
                                      cur_stream()),
          "segment_reduce");
    return {active, reduced, seg};
}

std::tuple<at::Tensor, at::Tensor, at::Tensor> sample_triplets(const at::Tensor &user_ids, const at::Tensor &ptr, const at::Tensor &items,
                                                               int64_t num_items, int64_t n, int64_t seed, int64_t epoch) {
    need(user_ids, "user_ids", at::kInt, 1); need(ptr, "ptr", at::kLong, 1); need(items, "items", at::kInt, 1);
    const at::Tensor uid = user_ids.contiguous(), p = ptr.contiguous(), it = items.contiguous();
    at::Tensor u = at::empty({n}, p.options()), po = at::empty({n}, p.options()), ne = at::empty({n}, p.options());
    check(elimrec_sample_triplets(uid.data_ptr<int32_t>(), p.data_ptr<int64_t>(), it.data_ptr<int32_t>(), uid.numel(), num_items, n,
                                  (uint64_t)seed, (uint64_t)epoch, u.data_ptr<int64_t>(), po.data_ptr<int64_t>(), ne.data_ptr<int64_t>(),
                                  cur_stream()),
          "sample_triplets");
    return {u, po, ne};
}

// "bpr_head_bwd" of SURVEY.md 8(b): the row gradients bpr_head_fwd saved, scaled by the upstream gradient of the mean loss and
// reduced per node in ascending slot order (IndexBackward, deterministic) into a dense dY [n_rows x Cy].
at::Tensor bpr_head_bwd(const at::Tensor &grad_rows, const at::Tensor &keys, const at::Tensor &grad_out, int64_t n_rows) {
    need(keys, "keys", at::kInt, 1); need(grad_out, "grad_out", at::kFloat);
    TORCH_CHECK(grad_out.numel() == 1, "elimrec::bpr_head_bwd: grad_out is the gradient of the scalar loss");
    const at::Tensor r = rowmajor(grad_rows, "grad_rows").contiguous(), k = keys.contiguous();
    const int64_t n = r.size(0), ld = r.size(1);
    TORCH_CHECK(k.numel() == n && n_rows >= 1, "elimrec::bpr_head_bwd: one key per row");
    at::Tensor active = at::empty({n}, k.options()), reduced = at::empty({n, ld}, r.options()), seg = at::zeros({8}, k.options());
    const size_t need_ws = elimrec_segment_reduce_workspace(n);
    at::Tensor ws = at::empty({(int64_t)(need_ws ? need_ws : 1)}, r.options().dtype(at::kByte));
    check(elimrec_segment_reduce_rows(r.data_ptr<float>(), k.data_ptr<int32_t>(), n, (int)ld, 0, active.data_ptr<int32_t>(),
                                      reduced.data_ptr<float>(), nullptr, seg.data_ptr<int32_t>(), ws.data_ptr(), (size_t)ws.numel(),
                                      cur_stream()),
          "bpr_head_bwd");
    // rows behind the valid prefix go to a dump row (no host read-back of the count)
    const at::Tensor slot = at::arange(n, k.options());
    const at::Tensor dst = at::where(slot < seg[0], active, at::full({}, n_rows, k.options())).to(at::kLong);
    at::Tensor dY = at::zeros({n_rows + 1, ld}, r.options());
    dY.index_copy_(0, dst, reduced * grad_out.reshape({}));
    return dY.narrow(0, 0, n_rows);
}

// ---- item-sharded evaluation (elimrec_score_topk_shard phases 1 / 2, elimrec_topk_merge)
static void train_csr(const c10::optional<at::Tensor> &train_ptr, const c10::optional<at::Tensor> &train_items, at::Tensor &tp, at::Tensor &ti) {
    if (train_ptr.has_value() && train_ptr->defined()) {
        TORCH_CHECK(train_items.has_value() && train_items->defined(), "elimrec: train_ptr needs train_items");
        need(*train_ptr, "train_ptr", at::kLong, 1); need(*train_items, "train_items", at::kInt, 1);
        tp = train_ptr->contiguous(); ti = train_items->contiguous();
    }
}

at::Tensor score_shard_row_sums(const at::Tensor &Y, int64_t U, int64_t I, const at::Tensor &users, int64_t d, int64_t S, int64_t head_mask,
                                int64_t fusion_mode, int64_t I_total) {
    const at::Tensor y = rowmajor(Y, "Y");
    need(users, "users", at::kLong, 1);
    const at::Tensor u = users.contiguous();
    const int64_t B = u.numel();
    at::Tensor row_sum = at::zeros({B}, y.options());
    const size_t need_ws = elimrec_score_workspace_for((int)B, U, I, (int)S, 1, (int)d, 0);
    at::Tensor ws = at::empty({(int64_t)(need_ws ? need_ws : 1)}, y.options().dtype(at::kByte));
    check(elimrec_score_topk_shard(y.data_ptr<float>(), y.stride(0), U, I, u.data_ptr<int64_t>(), (int)B, (int)d, (int)S, (uint32_t)head_mask,
                                   (int)fusion_mode, 2, nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr, ws.data_ptr(),
                                   (size_t)ws.numel(), 1, row_sum.data_ptr<float>(), I_total, 0, cur_stream()),
          "score_shard_row_sums");
    return row_sum;
}

// ---- candidate lists (sampled-negative evaluation): the block norms and, for TIE, the catalogue row sums are computed here
at::Tensor score_candidates(const at::Tensor &Y, int64_t U, int64_t I, const at::Tensor &users, int64_t d, int64_t S, int64_t head_mask,
                            int64_t fusion_mode, int64_t predict_type, const at::Tensor &cand_ptr, const at::Tensor &cand_items, int64_t width) {
    const at::Tensor y = rowmajor(Y, "Y");
    need(users, "users", at::kLong, 1); need(cand_ptr, "cand_ptr", at::kLong, 1); need(cand_items, "cand_items", at::kInt, 1);
    const at::Tensor u = users.contiguous(), cp = cand_ptr.contiguous(), ci = cand_items.contiguous();
    const int64_t B = u.numel();
    TORCH_CHECK(cp.numel() == B + 1 && width >= 0, "elimrec::score_candidates: cand_ptr needs B + 1 entries, width >= 0");
    at::Tensor out = at::empty({B, width}, y.options());
    at::Tensor sqn = at::empty({U + I, S + 1}, y.options());
    check(elimrec_row_sqnorms(y.data_ptr<float>(), y.stride(0), U + I, (int)d, (int)S + 1, sqn.data_ptr<float>(), cur_stream()),
          "score_candidates(row_sqnorms)");
    at::Tensor row_sum;
    if (predict_type == 2) {
        row_sum = at::zeros({B}, y.options());
        const size_t need_ws = elimrec_score_workspace_for((int)B, U, I, (int)S, 1, (int)d, 0);
        at::Tensor ws = at::empty({(int64_t)(need_ws ? need_ws : 1)}, y.options().dtype(at::kByte));
        check(elimrec_score_topk_shard(y.data_ptr<float>(), y.stride(0), U, I, u.data_ptr<int64_t>(), (int)B, (int)d, (int)S,
                                       (uint32_t)head_mask, (int)fusion_mode, 2, sqn.data_ptr<float>(), nullptr, nullptr, nullptr, 0, 0,
                                       nullptr, nullptr, ws.data_ptr(), (size_t)ws.numel(), 1, row_sum.data_ptr<float>(), I, 0, cur_stream()),
              "score_candidates(row sums)");
    }
    check(elimrec_score_candidates(y.data_ptr<float>(), y.stride(0), U, I, u.data_ptr<int64_t>(), (int)B, (int)d, (int)S, (uint32_t)head_mask,
                                   (int)fusion_mode, (int)predict_type, sqn.data_ptr<float>(), cp.data_ptr<int64_t>(),
                                   ci.numel() ? ci.data_ptr<int32_t>() : nullptr, row_sum.defined() ? row_sum.data_ptr<float>() : nullptr, I,
                                   out.data_ptr<float>(), width, width, cur_stream()),
          "score_candidates");
    return out;
}

// ---- effect breakdown of candidate lists: block norms and the catalogue row sums are computed here
at::Tensor score_effects(const at::Tensor &Y, int64_t U, int64_t I, const at::Tensor &users, int64_t d, int64_t S, int64_t head_mask,
                         int64_t fusion_mode, const at::Tensor &cand_ptr, const at::Tensor &cand_items, int64_t width) {
    const at::Tensor y = rowmajor(Y, "Y");
    need(users, "users", at::kLong, 1); need(cand_ptr, "cand_ptr", at::kLong, 1); need(cand_items, "cand_items", at::kInt, 1);
    const at::Tensor u = users.contiguous(), cp = cand_ptr.contiguous(), ci = cand_items.contiguous();
    const int64_t B = u.numel();
    TORCH_CHECK(cp.numel() == B + 1 && width >= 0 && S >= 0, "elimrec::score_effects: cand_ptr needs B + 1 entries, width >= 0, S >= 0");
    at::Tensor out = at::empty({B, width, 6 + S}, y.options());
    if (B == 0 || width == 0) return out;
    at::Tensor sqn = at::empty({U + I, S + 1}, y.options());
    check(elimrec_row_sqnorms(y.data_ptr<float>(), y.stride(0), U + I, (int)d, (int)S + 1, sqn.data_ptr<float>(), cur_stream()),
          "score_effects(row_sqnorms)");
    at::Tensor row_sum = at::zeros({B}, y.options());
    const size_t need_ws = elimrec_score_workspace_for((int)B, U, I, (int)S, 1, (int)d, 0);
    at::Tensor ws = at::empty({(int64_t)(need_ws ? need_ws : 1)}, y.options().dtype(at::kByte));
    check(elimrec_score_topk_shard(y.data_ptr<float>(), y.stride(0), U, I, u.data_ptr<int64_t>(), (int)B, (int)d, (int)S,
                                   (uint32_t)head_mask, (int)fusion_mode, 2, sqn.data_ptr<float>(), nullptr, nullptr, nullptr, 0, 0,
                                   nullptr, nullptr, ws.data_ptr(), (size_t)ws.numel(), 1, row_sum.data_ptr<float>(), I, 0, cur_stream()),
          "score_effects(row sums)");
    check(elimrec_score_effects(y.data_ptr<float>(), y.stride(0), U, I, u.data_ptr<int64_t>(), (int)B, (int)d, (int)S, (uint32_t)head_mask,
                                (int)fusion_mode, sqn.data_ptr<float>(), cp.data_ptr<int64_t>(),
                                ci.numel() ? ci.data_ptr<int32_t>() : nullptr, row_sum.data_ptr<float>(), I, out.data_ptr<float>(), width,
                                cur_stream()),
          "score_effects");
    return out;
}

// ---- exact catalogue rank of listed items in rows of (masked) scores
at::Tensor rank_targets(const at::Tensor &scores, const at::Tensor &tgt_ptr, const at::Tensor &tgt_items) {
    need(scores, "scores", at::kFloat, 2);
    const at::Tensor sc = scores.stride(1) == 1 ? scores : scores.contiguous();
    need(tgt_ptr, "tgt_ptr", at::kLong, 1); need(tgt_items, "tgt_items", at::kInt, 1);
    const at::Tensor tp = tgt_ptr.contiguous(), ti = tgt_items.contiguous();
    const int64_t B = sc.size(0), I = sc.size(1), n = ti.numel();
    TORCH_CHECK(tp.numel() == B + 1, "elimrec::rank_targets: tgt_ptr needs B + 1 = ", B + 1, " entries, got ", tp.numel());
    checked_csr(tp, ti, B, I, false, "rank_targets", "tgt_ptr", "tgt_items", "item ids", "the catalogue has", "items");
    at::Tensor out = at::empty({n}, ti.options());
    if (n == 0 || B == 0) return out;
    check(elimrec_rank_targets(sc.data_ptr<float>(), B, I, sc.stride(0), tp.data_ptr<int64_t>(), ti.data_ptr<int32_t>(), n,
                               out.data_ptr<int32_t>(), cur_stream()),
          "rank_targets");
    return out;
}

// ---- insertion ranks by value: where an item outside the block would land in each row's full ranking
at::Tensor rank_values(const at::Tensor &scores, const at::Tensor &val_ptr, const at::Tensor &vals, const c10::optional<at::Tensor> &skip) {
    need(scores, "scores", at::kFloat, 2);
    const at::Tensor sc = scores.stride(1) == 1 ? scores : scores.contiguous();
    need(val_ptr, "val_ptr", at::kLong, 1); need(vals, "vals", at::kFloat, 1);
    const at::Tensor vp = val_ptr.contiguous(), v = vals.contiguous();
    const int64_t B = sc.size(0), I = sc.size(1), n = v.numel();
    TORCH_CHECK(vp.numel() == B + 1, "elimrec::rank_values: val_ptr needs B + 1 = ", B + 1, " entries, got ", vp.numel());
    checked_csr(vp, v, B, "rank_values", "val_ptr", "vals");
    at::Tensor sk;
    if (skip.has_value() && skip->defined()) {
        need(*skip, "skip", at::kInt, 1);
        sk = skip->contiguous();
        TORCH_CHECK(sk.numel() == n, "elimrec::rank_values: skip needs one entry per value (", n, "), got ", sk.numel());
        if (n) {
            const int64_t lo = sk.min().item<int64_t>(), hi = sk.max().item<int64_t>();
            TORCH_CHECK_INDEX(lo >= -1 && hi < I, "elimrec::rank_values: skipped columns span [", lo, ", ", hi, "], the block has ", I,
                              " columns (-1: none)");
        }
    }
    at::Tensor out = at::empty({n}, v.options().dtype(at::kInt));
    if (n == 0 || B == 0) return out;
    check(elimrec_rank_values(sc.data_ptr<float>(), B, I, sc.stride(0), vp.data_ptr<int64_t>(), v.data_ptr<float>(),
                              sk.defined() ? sk.data_ptr<int32_t>() : nullptr, n, out.data_ptr<int32_t>(), cur_stream()),
          "rank_values");
    return out;
}

// ---- weighted sums of table rows over ragged lists: the fold-in of new users
at::Tensor segment_row_sum(const at::Tensor &table, const at::Tensor &ptr, const at::Tensor &rows, const at::Tensor &weights, int64_t row_offset) {
    need(table, "table", at::kFloat, 2);
    const at::Tensor tb = table.stride(1) == 1 && table.stride(0) % 4 == 0 && ((uintptr_t)table.data_ptr<float>() & 15) == 0 ? table : table.contiguous();
    need(ptr, "ptr", at::kLong, 1); need(rows, "rows", at::kInt, 1); need(weights, "weights", at::kFloat, 1);
    const at::Tensor p = ptr.contiguous(), r = rows.contiguous(), w = weights.contiguous();
    const int64_t n = tb.size(0), C = tb.size(1), Q = p.numel() - 1, E = r.numel();
    TORCH_CHECK(Q >= 0, "elimrec::segment_row_sum: ptr needs Q + 1 >= 1 entries");
    TORCH_CHECK(C >= 4 && C <= 1280 && C % 4 == 0, "elimrec::segment_row_sum: C must be a multiple of 4 in [4, 1280], got ", C);
    TORCH_CHECK(w.numel() == E, "elimrec::segment_row_sum: weights needs one entry per row id (", E, "), got ", w.numel());
    TORCH_CHECK_INDEX(row_offset >= 0 && row_offset <= n, "elimrec::segment_row_sum: row_offset ", row_offset, " outside [0, ", n, "]");
    checked_csr(p, r, Q, n - row_offset, true, "segment_row_sum", "ptr", "rows", "row ids", "the table holds", "rows behind row_offset");
    TORCH_CHECK(E == 0 || at::isfinite(w).all().item<bool>(), "elimrec::segment_row_sum: weights holds an entry that is not finite");
    at::Tensor out = at::empty({Q, C}, tb.options());
    if (Q == 0) return out;
    check(elimrec_segment_row_sum(tb.data_ptr<float>(), n, C, tb.stride(0), row_offset, p.data_ptr<int64_t>(), E ? r.data_ptr<int32_t>() : nullptr,
                                  E ? w.data_ptr<float>() : nullptr, Q, E, out.data_ptr<float>(), C, cur_stream()),
          "segment_row_sum");
    return out;
}

// ---- cosine top-K of table rows against the rows of the same table; overlap of two id lists
std::tuple<at::Tensor, at::Tensor> cosine_topk(const at::Tensor &table, const at::Tensor &sqnorm, const at::Tensor &query_rows, int64_t K,
                                               bool exclude_self) {
    const at::Tensor t = rowmajor(table, "table");
    need(sqnorm, "sqnorm", at::kFloat, 1); need(query_rows, "query_rows", at::kInt, 1);
    const at::Tensor q = query_rows.contiguous();
    const int64_t n = t.size(0), d = t.size(1), Q = q.numel();
    TORCH_CHECK(K >= 1 && K <= 256, "elimrec::cosine_topk: 1 <= K <= 256, got ", K);
    TORCH_CHECK(d % 4 == 0 && d >= 4 && d <= 256, "elimrec::cosine_topk: the table needs d % 4 == 0 and 4 <= d <= 256 columns, got ", d);
    TORCH_CHECK(sqnorm.numel() == n, "elimrec::cosine_topk: sqnorm needs one entry per table row (", n, "), got ", sqnorm.numel());
    checked_ids(q, n, true, "cosine_topk", "query rows", "the table has", "rows");
    at::Tensor idx = at::empty({Q, K}, q.options()), val = at::empty({Q, K}, t.options());
    if (Q == 0) return {idx, val};
    const size_t need_ws = elimrec_cosine_topk_workspace(Q, n, (int)K);
    at::Tensor ws = at::empty({(int64_t)need_ws}, t.options().dtype(at::kByte));
    check(elimrec_cosine_topk(t.data_ptr<float>(), t.stride(0), n, (int)d, sqnorm.data_ptr<float>(), n > 1 ? sqnorm.stride(0) : 1,
                              q.data_ptr<int32_t>(), Q, exclude_self ? 1 : 0, nullptr, nullptr, (int)K, idx.data_ptr<int32_t>(),
                              val.data_ptr<float>(), ws.data_ptr(), (size_t)ws.numel(), cur_stream()),
          "cosine_topk");
    return {idx, val};
}

// ---- cosine_topk with a query table of its own; without norms the plain dot product (serving a factor model)
std::tuple<at::Tensor, at::Tensor> cross_topk(const at::Tensor &query_table, const c10::optional<at::Tensor> &query_sqnorm, const at::Tensor &table,
                                              const c10::optional<at::Tensor> &sqnorm, const at::Tensor &query_rows,
                                              const c10::optional<at::Tensor> &excl_ptr, const c10::optional<at::Tensor> &excl_rows, int64_t K) {
    const at::Tensor tq = rowmajor(query_table, "query_table"), t = rowmajor(table, "table");
    need(query_rows, "query_rows", at::kInt, 1);
    const at::Tensor q = query_rows.contiguous();
    const int64_t nq = tq.size(0), n = t.size(0), d = t.size(1), Q = q.numel();
    TORCH_CHECK_VALUE(K >= 1 && K <= 256, "elimrec::cross_topk: 1 <= K <= 256, got ", K);
    TORCH_CHECK_VALUE(d % 4 == 0 && d >= 4 && d <= 256, "elimrec::cross_topk: the table needs d % 4 == 0 and 4 <= d <= 256 columns, got ", d);
    TORCH_CHECK_VALUE(tq.size(1) == d, "elimrec::cross_topk: the two tables share d, got ", tq.size(1), " and ", d);
    TORCH_CHECK_VALUE(excl_ptr.has_value() == excl_rows.has_value(), "elimrec::cross_topk: excl_ptr and excl_rows come together");
    const at::Tensor sqq = query_sqnorm.has_value() ? *query_sqnorm : at::ones({std::max<int64_t>(nq, 1)}, tq.options());
    const at::Tensor sq = sqnorm.has_value() ? *sqnorm : at::ones({std::max<int64_t>(n, 1)}, t.options());
    need(sqq, "query_sqnorm", at::kFloat, 1); need(sq, "sqnorm", at::kFloat, 1);
    TORCH_CHECK_VALUE((!query_sqnorm.has_value() || sqq.numel() == nq) && (!sqnorm.has_value() || sq.numel() == n),
                      "elimrec::cross_topk: the squared norms need one entry per row of their table");
    checked_ids(q, nq, true, "cross_topk", "query rows", "the query table has", "rows");
    at::Tensor ep, er;
    if (excl_ptr.has_value()) {
        need(*excl_ptr, "excl_ptr", at::kLong, 1); need(*excl_rows, "excl_rows", at::kInt, 1);
        ep = excl_ptr->contiguous(); er = excl_rows->contiguous();
        TORCH_CHECK_VALUE(ep.numel() == Q + 1, "elimrec::cross_topk: excl_ptr needs Q + 1 = ", Q + 1, " entries, got ", ep.numel());
        checked_csr(ep, er, Q, n, true, "cross_topk", "excl_ptr", "excl_rows", "excluded rows", "the table has", "rows");
    }
    at::Tensor idx = at::empty({Q, K}, q.options()), val = at::empty({Q, K}, t.options());
    if (Q == 0) return {idx, val};
    const size_t need_ws = elimrec_cross_topk_workspace(Q, n, (int)K);
    at::Tensor ws = at::empty({(int64_t)need_ws}, t.options().dtype(at::kByte));
    check(elimrec_cross_topk(tq.data_ptr<float>(), tq.stride(0), nq, sqq.data_ptr<float>(), sqq.numel() > 1 ? sqq.stride(0) : 1, t.data_ptr<float>(),
                             t.stride(0), n, (int)d, sq.data_ptr<float>(), sq.numel() > 1 ? sq.stride(0) : 1, q.data_ptr<int32_t>(), Q,
                             ep.defined() ? ep.data_ptr<int64_t>() : nullptr, ep.defined() && er.numel() ? er.data_ptr<int32_t>() : (ep.defined() ? q.data_ptr<int32_t>() : nullptr),
                             (int)K, idx.data_ptr<int32_t>(), val.data_ptr<float>(), ws.data_ptr(), (size_t)ws.numel(), cur_stream()),
          "cross_topk");
    return {idx, val};
}

// ---- one half-sweep of implicit-feedback ALS (csrc/als.hip)
at::Tensor als_solve(const at::Tensor &ptr, const at::Tensor &nbr, const at::Tensor &F, const at::Tensor &A0, const at::Tensor &reg, double conf,
                     const c10::optional<at::Tensor> &rows) {
    need(ptr, "ptr", at::kLong, 1); need(nbr, "nbr", at::kInt, 1); need(A0, "A0", at::kDouble, 2); need(reg, "reg", at::kDouble, 1);
    const at::Tensor f = rowmajor(F, "F"), p = ptr.contiguous(), nb = nbr.contiguous(), a0 = A0.contiguous(), rg = reg.contiguous();
    const int64_t n = p.numel() - 1, n_fixed = f.size(0), d = f.size(1);
    TORCH_CHECK_VALUE(n >= 0, "elimrec::als_solve: ptr needs n + 1 >= 1 entries");
    TORCH_CHECK_VALUE(d % 16 == 0 && d >= 16 && d <= 64, "elimrec::als_solve: the factors need d % 16 == 0 and 16 <= d <= 64 columns, got ", d);
    TORCH_CHECK_VALUE(a0.size(0) == d && a0.size(1) == d, "elimrec::als_solve: A0 must be [", d, " x ", d, "]");
    TORCH_CHECK_VALUE(rg.numel() == n, "elimrec::als_solve: reg needs one entry per row (", n, "), got ", rg.numel());
    TORCH_CHECK_VALUE(std::isfinite(conf) && conf >= 0.0, "elimrec::als_solve: conf is finite and >= 0, got ", conf);
    TORCH_CHECK_VALUE(n == 0 || (at::isfinite(rg).all().item<bool>() && rg.min().item<double>() >= 0.0), "elimrec::als_solve: every reg is finite and >= 0");
    checked_csr(p, nb, n, n_fixed, true, "als_solve", "ptr", "nbr", "nbr", "the fixed side has", "rows");
    const at::Tensor hp = p.cpu(), hn = nb.cpu();
    const int64_t *pp = hp.data_ptr<int64_t>();
    const int32_t *nn = hn.data_ptr<int32_t>();
    for (int64_t r = 0; r < n; ++r)
        for (int64_t e = pp[r] + 1; e < pp[r + 1]; ++e)
            TORCH_CHECK_VALUE(nn[e] > nn[e - 1], "elimrec::als_solve: every list is strictly ascending (no repeated edge): row ", r, " lists ", nn[e - 1],
                              ", then ", nn[e]);
    at::Tensor q;
    if (rows.has_value()) {
        need(*rows, "rows", at::kInt, 1);
        q = rows->contiguous();
        checked_ids(q, n, true, "als_solve", "rows", "the side has", "rows");
    } else {
        q = at::argsort(p.slice(0, 0, n) - p.slice(0, 1), /*stable=*/true, 0, false).to(at::kInt);   // degree descending
    }
    at::Tensor out = at::zeros({n, d}, f.options());
    if (q.numel() == 0) return out;
    at::Tensor status = at::zeros({2}, nb.options());
    status.select(0, 1).fill_((int64_t)INT32_MAX);
    check(elimrec_als_solve(f.data_ptr<float>(), f.stride(0), n_fixed, (int)d, a0.data_ptr<double>(), p.data_ptr<int64_t>(),
                            nb.numel() ? nb.data_ptr<int32_t>() : nullptr, n, q.data_ptr<int32_t>(), q.numel(), rg.data_ptr<double>(), conf,
                            out.data_ptr<float>(), out.stride(0), status.data_ptr<int32_t>(), cur_stream()),
          "als_solve");
    const at::Tensor hs = status.cpu();
    TORCH_CHECK(hs.data_ptr<int32_t>()[0] == 0, "elimrec::als_solve: A_r is not positive definite for ", hs.data_ptr<int32_t>()[0],
                " row(s), the first is row ", hs.data_ptr<int32_t>()[1], " (written as zeros)");
    return out;
}

// ---- EASE (csrc/ease.hip): the Gram matrix of a bipartite graph, a dense SPD inverse, the top-K of the history's rows of P
static at::Tensor nonempty_ids(const at::Tensor &ids) { return ids.numel() ? ids.contiguous() : at::zeros({1}, ids.options()); }

at::Tensor gram_counts(const at::Tensor &q_ptr, const at::Tensor &q_nbr, const at::Tensor &o_ptr, const at::Tensor &o_nbr, double l2) {
    need(q_ptr, "q_ptr", at::kLong, 1); need(q_nbr, "q_nbr", at::kInt, 1); need(o_ptr, "o_ptr", at::kLong, 1); need(o_nbr, "o_nbr", at::kInt, 1);
    const at::Tensor qp = q_ptr.contiguous(), op = o_ptr.contiguous();
    const int64_t n = qp.numel() - 1, n_other = op.numel() - 1;
    TORCH_CHECK_VALUE(n >= 0 && n_other >= 0, "elimrec::gram_counts: both pointers need at least one entry");
    TORCH_CHECK_VALUE(std::isfinite(l2) && l2 >= 0.0, "elimrec::gram_counts: l2 is finite and >= 0, got ", l2);
    TORCH_CHECK_VALUE(q_nbr.numel() == o_nbr.numel(), "elimrec::gram_counts: the two CSRs hold the same edges, got ", q_nbr.numel(), " and ", o_nbr.numel());
    checked_csr(qp, q_nbr, n, n_other, true, "gram_counts", "q_ptr", "q_nbr", "q_nbr", "the other side has", "rows");
    checked_csr(op, o_nbr, n_other, n, true, "gram_counts", "o_ptr", "o_nbr", "o_nbr", "the query side has", "rows");
    at::Tensor out = at::empty({n, n}, qp.options().dtype(at::kDouble));
    if (n == 0) return out;
    const at::Tensor qn = nonempty_ids(q_nbr), on = nonempty_ids(o_nbr);
    check(elimrec_gram_counts(qp.data_ptr<int64_t>(), qn.data_ptr<int32_t>(), op.data_ptr<int64_t>(), on.data_ptr<int32_t>(), n, n_other, l2,
                              out.data_ptr<double>(), n, cur_stream()),
          "gram_counts");
    return out;
}

std::tuple<at::Tensor, at::Tensor> spd_inverse(const at::Tensor &A) {
    need(A, "A", at::kDouble, 2);
    TORCH_CHECK_VALUE(A.size(0) == A.size(1) && A.size(0) >= 1, "elimrec::spd_inverse: A must be square with n >= 1 rows");
    const int64_t n = A.size(0);
    at::Tensor out = A.clone(at::MemoryFormat::Contiguous);
    at::Tensor pivot = at::empty({1}, out.options()), status = at::empty({2}, out.options().dtype(at::kInt));
    at::Tensor ws = at::empty({(int64_t)elimrec_spd_inverse_workspace(n)}, out.options().dtype(at::kByte));
    check(elimrec_spd_inverse(out.data_ptr<double>(), n, n, pivot.data_ptr<double>(), status.data_ptr<int32_t>(), ws.data_ptr(), (size_t)ws.numel(),
                              cur_stream()),
          "spd_inverse");
    const at::Tensor hs = status.cpu();
    TORCH_CHECK(hs.data_ptr<int32_t>()[0] == 0, "elimrec::spd_inverse: the matrix is not positive definite: the pivot at index ",
                hs.data_ptr<int32_t>()[1], " is <= 0 or not finite");
    return {out, pivot};
}

std::tuple<at::Tensor, at::Tensor> ease_topk(const at::Tensor &P, const at::Tensor &hist_ptr, const at::Tensor &hist_items,
                                             const c10::optional<at::Tensor> &excl_ptr, const c10::optional<at::Tensor> &excl_items,
                                             const at::Tensor &users, int64_t K) {
    need(P, "P", at::kDouble, 2); need(hist_ptr, "hist_ptr", at::kLong, 1); need(hist_items, "hist_items", at::kInt, 1);
    need(users, "users", at::kLong, 1);
    TORCH_CHECK_VALUE(P.size(0) == P.size(1), "elimrec::ease_topk: P must be square");
    TORCH_CHECK_VALUE(K >= 1 && K <= 256, "elimrec::ease_topk: 1 <= K <= 256, got ", K);
    TORCH_CHECK_VALUE(excl_ptr.has_value() == excl_items.has_value(), "elimrec::ease_topk: excl_ptr and excl_items come together");
    const at::Tensor p = P.stride(1) == 1 ? P : P.contiguous(), hp = hist_ptr.contiguous(), u = users.contiguous();
    const int64_t n = p.size(0), n_seg = hp.numel() - 1, Q = u.numel();
    TORCH_CHECK_VALUE(n_seg >= 1, "elimrec::ease_topk: hist_ptr needs n_rows + 1 >= 2 entries");
    checked_csr(hp, hist_items, n_seg, n, true, "ease_topk", "hist_ptr", "hist_items", "history items", "the catalogue has", "items");
    checked_ids(u, n_seg, true, "ease_topk", "users", "the histories have", "segments");
    at::Tensor ep, ei;
    if (excl_ptr.has_value()) {
        need(*excl_ptr, "excl_ptr", at::kLong, 1); need(*excl_items, "excl_items", at::kInt, 1);
        ep = excl_ptr->contiguous();
        TORCH_CHECK_VALUE(ep.numel() == n_seg + 1, "elimrec::ease_topk: excl_ptr needs n_rows + 1 = ", n_seg + 1, " entries, got ", ep.numel());
        checked_csr(ep, *excl_items, n_seg, n, true, "ease_topk", "excl_ptr", "excl_items", "excluded items", "the catalogue has", "items");
        ei = nonempty_ids(*excl_items);
    }
    at::Tensor idx = at::empty({Q, K}, hist_items.options()), val = at::empty({Q, K}, p.options().dtype(at::kFloat));
    if (Q == 0) return {idx, val};
    const at::Tensor hi = nonempty_ids(hist_items);
    at::Tensor ws = at::empty({(int64_t)elimrec_ease_topk_workspace(Q, n, (int)K)}, p.options().dtype(at::kByte));
    check(elimrec_ease_topk(p.data_ptr<double>(), n > 1 ? p.stride(0) : n, n, hp.data_ptr<int64_t>(), hi.data_ptr<int32_t>(),
                            ep.defined() ? ep.data_ptr<int64_t>() : nullptr, ep.defined() ? ei.data_ptr<int32_t>() : nullptr, n_seg,
                            u.data_ptr<int64_t>(), Q, (int)K, idx.data_ptr<int32_t>(), val.data_ptr<float>(), ws.data_ptr(), (size_t)ws.numel(),
                            cur_stream()),
          "ease_topk");
    return {idx, val};
}

// ---- audience lists: per query item the K users with the largest predict() score (csrc/audience.hip)
std::tuple<at::Tensor, at::Tensor> audience_topk(const at::Tensor &Y, int64_t U, int64_t I, const at::Tensor &items,
                                                 const c10::optional<at::Tensor> &excl_ptr, const c10::optional<at::Tensor> &excl_users, int64_t d,
                                                 int64_t S, int64_t head_mask, int64_t fusion_mode, int64_t predict_type, int64_t K,
                                                 const c10::optional<at::Tensor> &sqnorm, const c10::optional<at::Tensor> &row_sum,
                                                 int64_t I_total) {
    const at::Tensor y = rowmajor(Y, "Y");
    need(items, "items", at::kInt, 1);
    const at::Tensor q = items.contiguous();
    const int64_t Q = q.numel();
    TORCH_CHECK(K >= 1 && K <= 256, "elimrec::audience_topk: 1 <= K <= 256, got ", K);
    TORCH_CHECK(d % 4 == 0 && d >= 4 && d <= 256, "elimrec::audience_topk: a block needs d % 4 == 0 and 4 <= d <= 256 columns, got ", d);
    TORCH_CHECK(S >= 0 && S <= 3, "elimrec::audience_topk: 0 <= S <= 3, got ", S);
    TORCH_CHECK(U >= 0 && I >= 0 && y.size(0) == U + I && y.size(1) >= (1 + S) * d, "elimrec::audience_topk: Y must be [U + I x >= (1 + S) d]");
    TORCH_CHECK(excl_ptr.has_value() == excl_users.has_value(), "elimrec::audience_topk: the exclusion CSR needs excl_ptr and excl_users, or neither");
    checked_ids(q, I, true, "audience_topk", "query items", "the catalogue has", "items");
    at::Tensor ep, eu;
    if (excl_ptr.has_value()) {
        need(*excl_ptr, "excl_ptr", at::kLong, 1); need(*excl_users, "excl_users", at::kInt, 1);
        ep = excl_ptr->contiguous(); eu = excl_users->contiguous();
        const int64_t n = eu.numel();
        TORCH_CHECK(ep.numel() == Q + 1, "elimrec::audience_topk: excl_ptr needs Q + 1 = ", Q + 1, " entries, got ", ep.numel());
        checked_csr(ep, eu, Q, U, true, "audience_topk", "excl_ptr", "excl_users", "excluded users", "the model has", "users");
        if (n == 0) eu = at::zeros({1}, q.options());      // the binding wants a device tensor; nothing of it is read
    }
    at::Tensor idx = at::empty({Q, K}, q.options()), val = at::empty({Q, K}, y.options());
    if (Q == 0) return {idx, val};
    at::Tensor sqn;
    if (sqnorm.has_value()) {
        need(*sqnorm, "sqnorm", at::kFloat, 2);
        TORCH_CHECK(sqnorm->size(0) == U + I && sqnorm->size(1) == S + 1, "elimrec::audience_topk: sqnorm must be [U + I x 1 + S]");
        sqn = sqnorm->contiguous();
    } else {
        sqn = at::empty({U + I, S + 1}, y.options());
        check(elimrec_row_sqnorms(y.data_ptr<float>(), y.stride(0), U + I, (int)d, (int)S + 1, sqn.data_ptr<float>(), cur_stream()),
              "audience_topk(row_sqnorms)");
    }
    at::Tensor rs;
    if (predict_type == 2) {
        TORCH_CHECK(row_sum.has_value(), "elimrec::audience_topk: predict type TIE needs row_sum [U]");
        need(*row_sum, "row_sum", at::kFloat, 1);
        TORCH_CHECK(row_sum->numel() == U, "elimrec::audience_topk: row_sum needs one entry per user (", U, "), got ", row_sum->numel());
        rs = row_sum->contiguous();
    }
    const size_t need_ws = elimrec_audience_topk_workspace(Q, U, (int)K);
    at::Tensor ws = at::empty({(int64_t)need_ws}, y.options().dtype(at::kByte));
    check(elimrec_audience_topk(y.data_ptr<float>(), y.stride(0), U, I, (int)d, (int)S, (uint32_t)head_mask, (int)fusion_mode, (int)predict_type,
                                sqn.data_ptr<float>(), rs.defined() ? rs.data_ptr<float>() : nullptr, I_total, q.data_ptr<int32_t>(), Q,
                                ep.defined() ? ep.data_ptr<int64_t>() : nullptr, eu.defined() ? eu.data_ptr<int32_t>() : nullptr, (int)K,
                                idx.data_ptr<int32_t>(), val.data_ptr<float>(), ws.data_ptr(), (size_t)ws.numel(), cur_stream()),
          "audience_topk");
    return {idx, val};
}

at::Tensor list_overlap(const at::Tensor &a, const at::Tensor &b) {
    need(a, "a", at::kInt, 2); need(b, "b", at::kInt, 2);
    const at::Tensor x = a.contiguous(), y = b.contiguous();
    TORCH_CHECK(x.sizes() == y.sizes() && x.size(1) >= 1 && x.size(1) <= 1024, "elimrec::list_overlap: two [n x K] lists of one shape, 1 <= K <= 1024");
    at::Tensor out = at::empty({x.size(0)}, x.options());
    check(elimrec_list_overlap(x.data_ptr<int32_t>(), y.data_ptr<int32_t>(), x.size(0), (int)x.size(1), out.data_ptr<int32_t>(), cur_stream()),
          "list_overlap");
    return out;
}

// ---- the lists themselves: mean pairwise cosine per list and column block; exposure counts of the catalogue
at::Tensor list_pair_cosine(const at::Tensor &table, const at::Tensor &sqnorm, const at::Tensor &lists, int64_t blocks) {
    const at::Tensor t = rowmajor(table, "table");
    need(sqnorm, "sqnorm", at::kFloat); need(lists, "lists", at::kInt, 2);
    const at::Tensor l = lists.contiguous();
    const int64_t n = t.size(0), B = l.size(0), K = l.size(1);
    TORCH_CHECK(blocks >= 1 && blocks <= 8 && t.size(1) % blocks == 0, "elimrec::list_pair_cosine: 1 <= blocks <= 8 equal column blocks, got ",
                blocks, " for ", t.size(1), " columns");
    const int64_t d = t.size(1) / blocks;
    TORCH_CHECK(K >= 1 && K <= 256, "elimrec::list_pair_cosine: 1 <= K <= 256, got ", K);
    TORCH_CHECK(d % 4 == 0 && d >= 4 && d <= 256, "elimrec::list_pair_cosine: a block needs d % 4 == 0 and 4 <= d <= 256 columns, got ", d);
    TORCH_CHECK(sqnorm.numel() == n * blocks && (sqnorm.dim() == 2 ? sqnorm.size(0) == n : (sqnorm.dim() == 1 && blocks == 1)),
                "elimrec::list_pair_cosine: sqnorm must be [", n, " x ", blocks, "]");
    const at::Tensor sq = (sqnorm.dim() == 1 || sqnorm.stride(1) == 1 || blocks == 1) ? sqnorm : sqnorm.contiguous();
    at::Tensor out = at::empty({B, blocks}, t.options());
    if (B == 0) return out;
    const int64_t ld_sq = std::max<int64_t>(blocks, n > 1 ? sq.stride(0) : blocks);
    check(elimrec_list_pair_cosine(t.data_ptr<float>(), t.stride(0), n, (int)blocks, (int)d, sq.data_ptr<float>(), ld_sq,
                                   l.data_ptr<int32_t>(), B, (int)K, out.data_ptr<float>(), cur_stream()),
          "list_pair_cosine");
    return out;
}

at::Tensor list_exposure(const at::Tensor &lists, int64_t n_rows) {
    need(lists, "lists", at::kInt, 2);
    const at::Tensor l = lists.contiguous();
    TORCH_CHECK(n_rows >= 0 && l.size(1) >= 1, "elimrec::list_exposure: n_rows >= 0 and [B x K] lists with K >= 1");
    at::Tensor counts = at::zeros({n_rows}, l.options());
    if (l.size(0) == 0 || n_rows == 0) return counts;
    check(elimrec_list_exposure(l.data_ptr<int32_t>(), l.size(0), (int)l.size(1), n_rows, counts.data_ptr<int32_t>(), cur_stream()),
          "list_exposure");
    return counts;
}

// ---- diversified re-ranking of top-N pools (greedy MMR)
std::tuple<at::Tensor, at::Tensor, at::Tensor> mmr_rerank(const at::Tensor &table, const at::Tensor &sqnorm, const at::Tensor &pool_idx,
                                                          const at::Tensor &pool_val, int64_t K, double lam) {
    const at::Tensor t = rowmajor(table, "table");
    need(sqnorm, "sqnorm", at::kFloat, 1); need(pool_idx, "pool_idx", at::kInt, 2); need(pool_val, "pool_val", at::kFloat, 2);
    const at::Tensor pi = pool_idx.contiguous(), pv = pool_val.contiguous();
    const int64_t n = t.size(0), d = t.size(1), B = pi.size(0), N = pi.size(1);
    TORCH_CHECK(pi.sizes() == pv.sizes(), "elimrec::mmr_rerank: pool_idx and pool_val must have one shape [B x N]");
    TORCH_CHECK(K >= 1 && K <= N && N <= elimrec_mmr_max_pool(), "elimrec::mmr_rerank: 1 <= K <= N <= ", elimrec_mmr_max_pool(), ", got K ", K,
                ", N ", N);
    TORCH_CHECK(d % 4 == 0 && d >= 4 && d <= 256, "elimrec::mmr_rerank: the table needs d % 4 == 0 and 4 <= d <= 256 columns, got ", d);
    TORCH_CHECK(lam >= 0.0 && lam <= 1.0, "elimrec::mmr_rerank: 0 <= lam <= 1, got ", lam);
    TORCH_CHECK(sqnorm.numel() == n, "elimrec::mmr_rerank: sqnorm needs one entry per table row (", n, "), got ", sqnorm.numel());
    at::Tensor idx = at::empty({B, K}, pi.options()), pos = at::empty({B, K}, pi.options()), val = at::empty({B, K}, pv.options());
    if (B == 0) return {idx, pos, val};
    check(elimrec_mmr_rerank(t.data_ptr<float>(), t.stride(0), n, (int)d, sqnorm.data_ptr<float>(), n > 1 ? sqnorm.stride(0) : 1,
                             pi.data_ptr<int32_t>(), pv.data_ptr<float>(), B, (int)N, (int)K, (float)lam, idx.data_ptr<int32_t>(),
                             pos.data_ptr<int32_t>(), val.data_ptr<float>(), cur_stream()),
          "mmr_rerank");
    return {idx, pos, val};
}

// ---- calibrated re-ranking of top-N pools towards per-user class shares; class shares and miscalibration of lists
std::tuple<at::Tensor, at::Tensor, at::Tensor> calibrate_rerank(const at::Tensor &pool_idx, const at::Tensor &pool_val, const at::Tensor &class_of,
                                                                const at::Tensor &target, int64_t K, double lam, double smooth) {
    need(pool_idx, "pool_idx", at::kInt, 2); need(pool_val, "pool_val", at::kFloat, 2); need(class_of, "class_of", at::kInt, 1);
    const at::Tensor pi = pool_idx.contiguous(), pv = pool_val.contiguous(), cl = class_of.contiguous(), tg = rowmajor(target, "target");
    const int64_t B = pi.size(0), N = pi.size(1), C = tg.size(1);
    TORCH_CHECK(pi.sizes() == pv.sizes(), "elimrec::calibrate_rerank: pool_idx and pool_val must have one shape [B x N]");
    TORCH_CHECK(K >= 1 && K <= N && N <= elimrec_mmr_max_pool(), "elimrec::calibrate_rerank: 1 <= K <= N <= ", elimrec_mmr_max_pool(),
                ", got K ", K, ", N ", N);
    TORCH_CHECK(tg.size(0) == B && C >= 1 && C <= elimrec_calibrate_max_classes(), "elimrec::calibrate_rerank: target must be [", B,
                " x C], 1 <= C <= ", elimrec_calibrate_max_classes(), ", got [", tg.size(0), " x ", C, "]");
    TORCH_CHECK(lam >= 0.0 && lam <= 1.0, "elimrec::calibrate_rerank: 0 <= lam <= 1, got ", lam);
    TORCH_CHECK(smooth > 0.0 && smooth < 1.0, "elimrec::calibrate_rerank: 0 < smooth < 1, got ", smooth);
    at::Tensor idx = at::empty({B, K}, pi.options()), pos = at::empty({B, K}, pi.options()), val = at::empty({B, K}, pv.options());
    if (B == 0) return {idx, pos, val};
    check(elimrec_calibrate_rerank(pi.data_ptr<int32_t>(), pv.data_ptr<float>(), B, (int)N, (int)K, cl.data_ptr<int32_t>(), cl.numel(),
                                   tg.data_ptr<float>(), B > 1 ? std::max<int64_t>(C, tg.stride(0)) : C, (int)C, lam, smooth,
                                   idx.data_ptr<int32_t>(), pos.data_ptr<int32_t>(), val.data_ptr<float>(), cur_stream()),
          "calibrate_rerank");
    return {idx, pos, val};
}

std::tuple<at::Tensor, at::Tensor> list_calibration(const at::Tensor &lists, const at::Tensor &class_of, int64_t C, const at::Tensor &target,
                                                    double smooth) {
    need(lists, "lists", at::kInt, 2); need(class_of, "class_of", at::kInt, 1);
    const at::Tensor l = lists.contiguous(), cl = class_of.contiguous(), tg = rowmajor(target, "target");
    const int64_t B = l.size(0), K = l.size(1);
    TORCH_CHECK(K >= 1, "elimrec::list_calibration: lists [B x K] with K >= 1");
    TORCH_CHECK(C >= 1 && C <= elimrec_calibrate_max_classes(), "elimrec::list_calibration: 1 <= C <= ", elimrec_calibrate_max_classes(), ", got ", C);
    TORCH_CHECK(tg.size(0) == B && tg.size(1) == C, "elimrec::list_calibration: target must be [", B, " x ", C, "]");
    TORCH_CHECK(smooth > 0.0 && smooth < 1.0, "elimrec::list_calibration: 0 < smooth < 1, got ", smooth);
    at::Tensor shares = at::empty({B, C}, tg.options()), kl = at::empty({B}, tg.options());
    if (B == 0) return {shares, kl};
    check(elimrec_list_calibration(l.data_ptr<int32_t>(), B, (int)K, cl.data_ptr<int32_t>(), cl.numel(), (int)C, shares.data_ptr<float>(),
                                   tg.data_ptr<float>(), B > 1 ? std::max<int64_t>(C, tg.stride(0)) : C, smooth, kl.data_ptr<float>(),
                                   cur_stream()),
          "list_calibration");
    return {shares, kl};
}

// ---- spherical k-means over one block of a table: the assignment, and the new centroids (csrc/kmeans.hip)
static void kmeans_table(const char *who, const at::Tensor &t, const at::Tensor &sqnorm, const at::Tensor &cen, const at::Tensor &csq) {
    need(sqnorm, "sqnorm", at::kFloat, 1); need(cen, "centroids", at::kFloat, 2); need(csq, "centroid_sqnorm", at::kFloat, 1);
    const int64_t n = t.size(0), d = t.size(1), C = cen.size(0);
    TORCH_CHECK(d % 4 == 0 && d >= 4 && d <= 256, "elimrec::", who, ": the table needs d % 4 == 0 and 4 <= d <= 256 columns, got ", d);
    TORCH_CHECK(sqnorm.numel() == n, "elimrec::", who, ": sqnorm needs one entry per table row (", n, "), got ", sqnorm.numel());
    TORCH_CHECK(C >= 1 && C <= elimrec_kmeans_max_clusters() && cen.size(1) == d && csq.numel() == C, "elimrec::", who,
                ": centroids must be [C x ", d, "] with C squared norms, 1 <= C <= ", elimrec_kmeans_max_clusters(), ", got [", C, " x ",
                cen.size(1), "] and ", csq.numel());
}

std::tuple<at::Tensor, at::Tensor, at::Tensor> kmeans_assign(const at::Tensor &table, const at::Tensor &sqnorm, const at::Tensor &centroids,
                                                             const at::Tensor &centroid_sqnorm, const c10::optional<at::Tensor> &prev) {
    const at::Tensor t = rowmajor(table, "table");
    kmeans_table("kmeans_assign", t, sqnorm, centroids, centroid_sqnorm);
    const at::Tensor cen = centroids.contiguous(), csq = centroid_sqnorm.contiguous();
    const int64_t n = t.size(0), d = t.size(1), C = cen.size(0);
    at::Tensor pv;
    if (prev.has_value()) {
        need(*prev, "prev", at::kInt, 1);
        TORCH_CHECK(prev->numel() == n, "elimrec::kmeans_assign: prev needs one entry per table row (", n, "), got ", prev->numel());
        pv = prev->contiguous();
    }
    at::Tensor assign = at::empty({n}, t.options().dtype(at::kInt)), cos = at::empty({n}, t.options());
    at::Tensor changed = at::zeros({1}, assign.options());
    if (n == 0) return {assign, cos, changed};
    check(elimrec_kmeans_assign(t.data_ptr<float>(), t.stride(0), n, (int)d, sqnorm.data_ptr<float>(), n > 1 ? sqnorm.stride(0) : 1,
                                cen.data_ptr<float>(), csq.data_ptr<float>(), (int)C, pv.defined() ? pv.data_ptr<int32_t>() : nullptr,
                                assign.data_ptr<int32_t>(), cos.data_ptr<float>(), changed.data_ptr<int32_t>(), cur_stream()),
          "kmeans_assign");
    return {assign, cos, changed};
}

std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> kmeans_update(const at::Tensor &table, const at::Tensor &sqnorm, const at::Tensor &assign,
                                                                         const at::Tensor &centroids, const at::Tensor &centroid_sqnorm) {
    const at::Tensor t = rowmajor(table, "table");
    kmeans_table("kmeans_update", t, sqnorm, centroids, centroid_sqnorm);
    need(assign, "assign", at::kInt, 1);
    const int64_t n = t.size(0), d = t.size(1), C = centroids.size(0);
    TORCH_CHECK(assign.numel() == n, "elimrec::kmeans_update: assign needs one entry per table row (", n, "), got ", assign.numel());
    const at::Tensor as = assign.contiguous();
    at::Tensor cen = centroids.contiguous().clone(), csq = centroid_sqnorm.contiguous().clone();     // the C entry point works in place
    at::Tensor sums = at::zeros({C, d}, t.options().dtype(at::kDouble)), counts = at::zeros({C}, as.options());
    if (n == 0) return {cen, csq, sums, counts};
    const size_t need_ws = elimrec_kmeans_workspace(n, (int)d, (int)C);
    at::Tensor ws = at::empty({(int64_t)need_ws}, t.options().dtype(at::kByte));
    check(elimrec_kmeans_update(t.data_ptr<float>(), t.stride(0), n, (int)d, sqnorm.data_ptr<float>(), n > 1 ? sqnorm.stride(0) : 1,
                                as.data_ptr<int32_t>(), (int)C, cen.data_ptr<float>(), csq.data_ptr<float>(), sums.data_ptr<double>(),
                                counts.data_ptr<int32_t>(), ws.data_ptr(), (size_t)ws.numel(), cur_stream()),
          "kmeans_update");
    return {cen, csq, sums, counts};
}

// ---- embedding geometry of one block of a table over a list of row ids: the uniformity sum, the float64 Gram (csrc/geometry.hip)
static void geometry_table(const char *who, const at::Tensor &t, const at::Tensor &sqnorm, const at::Tensor &rows) {
    need(sqnorm, "sqnorm", at::kFloat, 1); need(rows, "rows", at::kInt, 1);
    const int64_t n = t.size(0), d = t.size(1);
    TORCH_CHECK(d % 4 == 0 && d >= 4 && d <= 256, "elimrec::", who, ": the table needs d % 4 == 0 and 4 <= d <= 256 columns, got ", d);
    TORCH_CHECK(sqnorm.numel() == n, "elimrec::", who, ": sqnorm needs one entry per table row (", n, "), got ", sqnorm.numel());
}

std::tuple<at::Tensor, at::Tensor> uniformity_sum(const at::Tensor &table, const at::Tensor &sqnorm, const at::Tensor &rows, double t) {
    const at::Tensor T = rowmajor(table, "table");
    geometry_table("uniformity_sum", T, sqnorm, rows);
    TORCH_CHECK(t > 0.0 && t <= 8.0, "elimrec::uniformity_sum: 0 < t <= 8, got ", t);
    const at::Tensor r = rows.contiguous();
    const int64_t n_rows = T.size(0), d = T.size(1), n = r.numel();
    at::Tensor sum = at::zeros({1}, T.options().dtype(at::kDouble)), counts = at::zeros({2}, T.options().dtype(at::kLong));
    const size_t need_ws = elimrec_uniformity_workspace(n, (int)d);
    at::Tensor ws = at::empty({(int64_t)need_ws}, T.options().dtype(at::kByte));
    check(elimrec_uniformity_sum(T.data_ptr<float>(), T.stride(0), n_rows, (int)d, sqnorm.data_ptr<float>(), n_rows > 1 ? sqnorm.stride(0) : 1,
                                 r.data_ptr<int32_t>(), n, t, sum.data_ptr<double>(), counts.data_ptr<int64_t>(), ws.data_ptr(),
                                 (size_t)ws.numel(), cur_stream()),
          "uniformity_sum");
    return {sum, counts};
}

std::tuple<at::Tensor, at::Tensor, at::Tensor> row_gram(const at::Tensor &table, const at::Tensor &sqnorm, const at::Tensor &rows) {
    const at::Tensor T = rowmajor(table, "table");
    geometry_table("row_gram", T, sqnorm, rows);
    const at::Tensor r = rows.contiguous();
    const int64_t n_rows = T.size(0), d = T.size(1), n = r.numel();
    at::Tensor gram = at::zeros({d, d}, T.options().dtype(at::kDouble)), sum = at::zeros({d}, gram.options());
    at::Tensor count = at::zeros({1}, T.options().dtype(at::kLong));
    const size_t need_ws = elimrec_gram_workspace(n, (int)d);
    at::Tensor ws = at::empty({(int64_t)need_ws}, T.options().dtype(at::kByte));
    check(elimrec_gram_f64(T.data_ptr<float>(), T.stride(0), n_rows, (int)d, sqnorm.data_ptr<float>(), n_rows > 1 ? sqnorm.stride(0) : 1,
                           r.data_ptr<int32_t>(), n, gram.data_ptr<double>(), sum.data_ptr<double>(), count.data_ptr<int64_t>(), ws.data_ptr(),
                           (size_t)ws.numel(), cur_stream()),
          "row_gram");
    return {gram, sum, count};
}

// ---- co-interaction neighbours: the top-K of rows of A^T A over a bipartite graph given as two CSRs (csrc/cooccur.hip)
std::tuple<at::Tensor, at::Tensor, at::Tensor> cooccur_topk(const at::Tensor &q_ptr, const at::Tensor &q_nbr, const at::Tensor &o_ptr,
                                                            const at::Tensor &o_nbr, const at::Tensor &rows, int64_t K, std::string measure) {
    need(q_ptr, "q_ptr", at::kLong, 1); need(q_nbr, "q_nbr", at::kInt, 1); need(o_ptr, "o_ptr", at::kLong, 1);
    need(o_nbr, "o_nbr", at::kInt, 1); need(rows, "rows", at::kInt, 1);
    TORCH_CHECK(K >= 1 && K <= elimrec_cooccur_max_k(), "elimrec::cooccur_topk: 1 <= K <= ", elimrec_cooccur_max_k(), ", got ", K);
    const int m = measure == "count" ? 0 : measure == "cosine" ? 1 : measure == "jaccard" ? 2 : -1;
    TORCH_CHECK(m >= 0, "elimrec::cooccur_topk: measure is one of count, cosine, jaccard, got '", measure, "'");
    const at::Tensor qp = q_ptr.contiguous(), qn = q_nbr.contiguous(), op = o_ptr.contiguous(), on = o_nbr.contiguous(), r = rows.contiguous();
    const int64_t n_query = qp.numel() - 1, n_other = op.numel() - 1, Q = r.numel();
    TORCH_CHECK(n_query >= 0 && n_other >= 0, "elimrec::cooccur_topk: q_ptr and o_ptr need at least one entry");
    TORCH_CHECK(qn.numel() == on.numel(), "elimrec::cooccur_topk: the two CSRs hold the same edges, got ", qn.numel(), " and ", on.numel());
    checked_csr(qp, qn, n_query, n_other, true, "cooccur_topk", "q_ptr", "q_nbr", "q_nbr", "the other side has", "rows");
    checked_csr(op, on, n_other, n_query, true, "cooccur_topk", "o_ptr", "o_nbr", "o_nbr", "the query side has", "rows");
    checked_ids(r, n_query, true, "cooccur_topk", "query rows", "the side has", "rows");
    at::Tensor idx = at::empty({Q, K}, r.options()), val = at::empty({Q, K}, r.options().dtype(at::kFloat)), cnt = at::empty({Q, K}, r.options());
    if (Q == 0) return {idx, val, cnt};
    at::Tensor walk = at::empty({Q}, qp.options());
    check(elimrec_cooccur_walk(qp.data_ptr<int64_t>(), qn.data_ptr<int32_t>(), n_query, op.data_ptr<int64_t>(), n_other, r.data_ptr<int32_t>(), Q,
                               walk.data_ptr<int64_t>(), cur_stream()), "cooccur_topk (walk)");
    const int64_t n_dense = walk.gt(elimrec_cooccur_slots() / 2).sum().item<int64_t>();
    at::Tensor ws = at::zeros({(int64_t)std::max<size_t>(16, elimrec_cooccur_workspace(n_dense, n_query))}, r.options().dtype(at::kByte));
    check(elimrec_cooccur_topk(qp.data_ptr<int64_t>(), qn.data_ptr<int32_t>(), n_query, op.data_ptr<int64_t>(), on.data_ptr<int32_t>(), n_other,
                               r.data_ptr<int32_t>(), Q, (int)K, m, 1, n_dense, walk.data_ptr<int64_t>(), idx.data_ptr<int32_t>(),
                               val.data_ptr<float>(), cnt.data_ptr<int32_t>(), ws.data_ptr(), (size_t)ws.numel(), cur_stream()),
          "cooccur_topk");
    return {idx, val, cnt};
}

// ---- weighted two-step walks: cooccur_topk's lists with every walk q -> u -> j weighing mid_weight[u] (csrc/walk.hip)
std::tuple<at::Tensor, at::Tensor> walk_topk(const at::Tensor &q_ptr, const at::Tensor &q_nbr, const at::Tensor &o_ptr, const at::Tensor &o_nbr,
                                             const at::Tensor &rows, int64_t K, const at::Tensor &mid_weight, const at::Tensor &row_scale,
                                             const at::Tensor &col_scale) {
    need(q_ptr, "q_ptr", at::kLong, 1); need(q_nbr, "q_nbr", at::kInt, 1); need(o_ptr, "o_ptr", at::kLong, 1);
    need(o_nbr, "o_nbr", at::kInt, 1); need(rows, "rows", at::kInt, 1);
    need(mid_weight, "mid_weight", at::kLong, 1); need(row_scale, "row_scale", at::kDouble, 1); need(col_scale, "col_scale", at::kDouble, 1);
    TORCH_CHECK_VALUE(K >= 1 && K <= elimrec_walk_max_k(), "elimrec::walk_topk: 1 <= K <= ", elimrec_walk_max_k(), ", got ", K);
    const at::Tensor qp = q_ptr.contiguous(), qn = q_nbr.contiguous(), op = o_ptr.contiguous(), on = o_nbr.contiguous(), r = rows.contiguous();
    const at::Tensor mw = mid_weight.contiguous(), rs = row_scale.contiguous(), cs = col_scale.contiguous();
    const int64_t n_query = qp.numel() - 1, n_other = op.numel() - 1, Q = r.numel();
    TORCH_CHECK(n_query >= 0 && n_other >= 0, "elimrec::walk_topk: q_ptr and o_ptr need at least one entry");
    TORCH_CHECK(qn.numel() == on.numel(), "elimrec::walk_topk: the two CSRs hold the same edges, got ", qn.numel(), " and ", on.numel());
    TORCH_CHECK_VALUE(mw.numel() == n_other && rs.numel() == n_query && cs.numel() == n_query, "elimrec::walk_topk: mid_weight has one entry per row "
                      "of the other side (", n_other, "), row_scale and col_scale one per query-side row (", n_query, "), got ", mw.numel(), ", ",
                      rs.numel(), " and ", cs.numel());
    checked_csr(qp, qn, n_query, n_other, true, "walk_topk", "q_ptr", "q_nbr", "q_nbr", "the other side has", "rows");
    checked_csr(op, on, n_other, n_query, true, "walk_topk", "o_ptr", "o_nbr", "o_nbr", "the query side has", "rows");
    checked_ids(r, n_query, true, "walk_topk", "query rows", "the side has", "rows");
    const int64_t max_w = n_other ? mw.max().item<int64_t>() : 0;
    TORCH_CHECK_VALUE(n_other == 0 || mw.min().item<int64_t>() >= 0, "elimrec::walk_topk: mid_weight holds a negative entry");
    TORCH_CHECK_VALUE(n_query == 0 || (at::isfinite(rs).all().item<bool>() && at::isfinite(cs).all().item<bool>() && rs.min().item<double>() >= 0.0 &&
                                       cs.min().item<double>() >= 0.0),
                      "elimrec::walk_topk: row_scale and col_scale are finite and >= 0");
    at::Tensor idx = at::empty({Q, K}, r.options()), val = at::empty({Q, K}, r.options().dtype(at::kFloat));
    if (Q == 0) return {idx, val};
    at::Tensor walk = at::empty({Q}, qp.options());
    check(elimrec_cooccur_walk(qp.data_ptr<int64_t>(), qn.data_ptr<int32_t>(), n_query, op.data_ptr<int64_t>(), n_other, r.data_ptr<int32_t>(), Q,
                               walk.data_ptr<int64_t>(), cur_stream()), "walk_topk (walk)");
    const int64_t max_walk = walk.max().item<int64_t>();
    TORCH_CHECK_VALUE((unsigned __int128)max_walk * (unsigned __int128)max_w < ((unsigned __int128)1 << 62),
                      "elimrec::walk_topk: the int64 sums could overflow: ", max_walk, " (the longest walk) x ", max_w, " (the largest weight) >= 2^62");
    const double top = (((double)max_walk * (double)max_w * std::ldexp(1.0, -elimrec_walk_frac_bits())) * rs.max().item<double>()) * cs.max().item<double>();
    TORCH_CHECK_VALUE(std::isfinite(top), "elimrec::walk_topk: the scores leave float64: (the longest walk) x (the largest weight) x the largest scales");
    const int64_t n_dense = walk.gt(elimrec_walk_slots() / 2).sum().item<int64_t>();
    at::Tensor ws = at::zeros({(int64_t)std::max<size_t>(16, elimrec_walk_workspace(n_dense, n_query))}, r.options().dtype(at::kByte));
    check(elimrec_walk_topk(qp.data_ptr<int64_t>(), qn.data_ptr<int32_t>(), n_query, op.data_ptr<int64_t>(), on.data_ptr<int32_t>(), n_other,
                            r.data_ptr<int32_t>(), Q, (int)K, mw.data_ptr<int64_t>(), rs.data_ptr<double>(), cs.data_ptr<double>(), 1, n_dense,
                            walk.data_ptr<int64_t>(), idx.data_ptr<int32_t>(), val.data_ptr<float>(), ws.data_ptr(), (size_t)ws.numel(), cur_stream()),
          "walk_topk");
    return {idx, val};
}

// ---- neighbour votes: per user the K items the neighbour lists of the user's history vote for (csrc/vote.hip)
std::tuple<at::Tensor, at::Tensor, at::Tensor> neighbour_vote_topk(const at::Tensor &nbr_idx, const at::Tensor &nbr_val, const at::Tensor &hist_ptr,
                                                                   const at::Tensor &hist_items, const c10::optional<at::Tensor> &excl_ptr,
                                                                   const c10::optional<at::Tensor> &excl_items, const at::Tensor &users, int64_t K) {
    need(nbr_idx, "nbr_idx", at::kInt, 2); need(nbr_val, "nbr_val", at::kFloat, 2); need(hist_ptr, "hist_ptr", at::kLong, 1);
    need(hist_items, "hist_items", at::kInt, 1); need(users, "users", at::kLong, 1);
    TORCH_CHECK(K >= 1 && K <= elimrec_vote_max_k(), "elimrec::neighbour_vote_topk: 1 <= K <= ", elimrec_vote_max_k(), ", got ", K);
    TORCH_CHECK(nbr_idx.sizes() == nbr_val.sizes() && nbr_idx.size(1) >= 1, "elimrec::neighbour_vote_topk: nbr_idx and nbr_val are both [n x Kn], Kn >= 1");
    TORCH_CHECK(excl_ptr.has_value() == excl_items.has_value(), "elimrec::neighbour_vote_topk: excl_ptr and excl_items come together");
    const at::Tensor li = nbr_idx.contiguous(), lv = nbr_val.contiguous(), hp = hist_ptr.contiguous(), hi = hist_items.contiguous(), u = users.contiguous();
    const int64_t n = li.size(0), Kn = li.size(1), n_hist = hp.numel() - 1, B = u.numel();
    TORCH_CHECK(n_hist >= 0, "elimrec::neighbour_vote_topk: hist_ptr needs at least one entry");
    checked_csr(hp, hi, n_hist, "neighbour_vote_topk", "hist_ptr", "hist_items");
    checked_ids(u, n_hist, true, "neighbour_vote_topk", "users", "the histories have", "segments");
    at::Tensor ep, ei;
    if (excl_ptr.has_value()) {
        need(*excl_ptr, "excl_ptr", at::kLong, 1); need(*excl_items, "excl_items", at::kInt, 1);
        ep = excl_ptr->contiguous(); ei = excl_items->contiguous();
        TORCH_CHECK(ep.numel() == n_hist + 1, "elimrec::neighbour_vote_topk: hist_ptr and excl_ptr name the same users: ", n_hist + 1, " and ",
                    ep.numel(), " entries");
        checked_csr(ep, ei, n_hist, "neighbour_vote_topk", "excl_ptr", "excl_items");
    }
    at::Tensor idx = at::empty({B, K}, li.options()), val = at::empty({B, K}, lv.options()), cnt = at::empty({B, K}, li.options());
    if (B == 0) return {idx, val, cnt};
    // the host's bounds: the int64 sums cannot overflow, a user's votes stay below the count's mark bit
    const at::Tensor len = hp.slice(0, 1) - hp.slice(0, 0, n_hist);
    const int64_t longest = n_hist ? len.max().item<int64_t>() : 0;
    const double max_abs = li.numel() ? at::where(at::isfinite(lv), lv.abs(), at::zeros_like(lv)).max().item<double>() : 0.0;
    const double q = std::ceil(max_abs * (double)(1 << elimrec_vote_frac_bits()));
    TORCH_CHECK_VALUE(q < 4.0e18 && (unsigned __int128)(uint64_t)q * (unsigned __int128)longest * (unsigned __int128)Kn < ((unsigned __int128)1 << 62),
                      "elimrec::neighbour_vote_topk: the int64 sums could overflow: ceil(", max_abs, " * 2^24) x ", longest,
                      " (the longest history) x ", Kn, " (Kn) >= 2^62");
    TORCH_CHECK_VALUE((unsigned __int128)longest * (unsigned __int128)Kn < ((unsigned __int128)1 << 30),
                      "elimrec::neighbour_vote_topk: ", longest, " (the longest history) x ", Kn, " (Kn) votes of one user, fewer than 2^30 are taken");
    at::Tensor V = len * (Kn + 1);
    if (excl_ptr.has_value()) V = V + (ep.slice(0, 1) - ep.slice(0, 0, n_hist));
    const int64_t n_dense = V.index_select(0, u).gt(elimrec_vote_slots() / 2).sum().item<int64_t>();
    at::Tensor ws = at::zeros({(int64_t)std::max<size_t>(16, elimrec_vote_workspace(n_dense, n))}, li.options().dtype(at::kByte));
    check(elimrec_neighbour_vote_topk(li.data_ptr<int32_t>(), lv.data_ptr<float>(), n, (int)Kn, hp.data_ptr<int64_t>(), hi.data_ptr<int32_t>(), n_hist,
                                      excl_ptr.has_value() ? ep.data_ptr<int64_t>() : nullptr, excl_ptr.has_value() ? ei.data_ptr<int32_t>() : nullptr,
                                      excl_ptr.has_value() ? n_hist : 0, u.data_ptr<int64_t>(), B, (int)K, 1, 1, n_dense, idx.data_ptr<int32_t>(),
                                      val.data_ptr<float>(), cnt.data_ptr<int32_t>(), ws.data_ptr(), (size_t)ws.numel(), cur_stream()),
          "neighbour_vote_topk");
    return {idx, val, cnt};
}

// ---- hard-negative pick: per triplet the best of M candidates over the tables' column blocks
std::tuple<at::Tensor, at::Tensor, at::Tensor> pick_hard_negatives(const at::Tensor &user_table, const at::Tensor &user_sqnorm,
                                                                   const at::Tensor &item_table, const at::Tensor &item_sqnorm,
                                                                   at::ArrayRef<double> weights, const at::Tensor &users,
                                                                   const at::Tensor &cands) {
    const at::Tensor ut = rowmajor(user_table, "user_table"), it = rowmajor(item_table, "item_table");
    need(user_sqnorm, "user_sqnorm", at::kFloat); need(item_sqnorm, "item_sqnorm", at::kFloat);
    need(users, "users", at::kLong, 1); need(cands, "cands", at::kInt, 2);
    const at::Tensor us = users.contiguous(), c = cands.contiguous();
    const int64_t blocks = (int64_t)weights.size(), n = c.size(0), M = c.size(1), U = ut.size(0), I = it.size(0);
    TORCH_CHECK(blocks >= 1 && blocks <= 8 && ut.size(1) % blocks == 0 && ut.size(1) == it.size(1),
                "elimrec::pick_hard_negatives: 1 <= blocks <= 8 weights, and two tables of one width that splits into as many blocks");
    const int64_t d = ut.size(1) / blocks;
    TORCH_CHECK(d % 4 == 0 && d >= 4 && d <= 256, "elimrec::pick_hard_negatives: a block needs d % 4 == 0 and 4 <= d <= 256 columns, got ", d);
    TORCH_CHECK(M >= 1 && M <= 64 && us.numel() == n, "elimrec::pick_hard_negatives: cands [n x M] with 1 <= M <= 64 and users [n]");
    TORCH_CHECK(user_sqnorm.numel() == U * blocks && item_sqnorm.numel() == I * blocks && (blocks == 1 || (user_sqnorm.dim() == 2 && item_sqnorm.dim() == 2)),
                "elimrec::pick_hard_negatives: the sqnorms must be [rows x ", blocks, "]");
    const at::Tensor su = (user_sqnorm.dim() == 1 || user_sqnorm.stride(1) == 1 || blocks == 1) ? user_sqnorm : user_sqnorm.contiguous();
    const at::Tensor si = (item_sqnorm.dim() == 1 || item_sqnorm.stride(1) == 1 || blocks == 1) ? item_sqnorm : item_sqnorm.contiguous();
    float w[8];
    for (int64_t b = 0; b < blocks; ++b) w[b] = (float)weights[b];
    at::Tensor neg = at::empty({n}, us.options()), pos = at::empty({n}, c.options()), score = at::empty({n}, ut.options());
    if (n == 0) return {neg, pos, score};
    check(elimrec_pick_hard_negatives(ut.data_ptr<float>(), ut.stride(0), U, su.data_ptr<float>(), std::max<int64_t>(blocks, U > 1 ? su.stride(0) : blocks),
                                      it.data_ptr<float>(), it.stride(0), I, si.data_ptr<float>(), std::max<int64_t>(blocks, I > 1 ? si.stride(0) : blocks),
                                      (int)blocks, (int)d, w, us.data_ptr<int64_t>(), c.data_ptr<int32_t>(), n, (int)M,
                                      neg.data_ptr<int64_t>(), pos.data_ptr<int32_t>(), score.data_ptr<float>(), cur_stream()),
          "pick_hard_negatives");
    return {neg, pos, score};
}

// ---- history support: per (user, target) the closest entries of the user's own history
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> history_support(const at::Tensor &table, const at::Tensor &sqnorm,
                                                                           at::ArrayRef<double> weights, const at::Tensor &users,
                                                                           const at::Tensor &lists, const at::Tensor &hist_ptr,
                                                                           const at::Tensor &hist_items, int64_t top, bool exclude_self) {
    const at::Tensor t = rowmajor(table, "table");
    need(sqnorm, "sqnorm", at::kFloat); need(users, "users", at::kLong, 1); need(lists, "lists", at::kInt, 2);
    need(hist_ptr, "hist_ptr", at::kLong, 1); need(hist_items, "hist_items", at::kInt, 1);
    const at::Tensor us = users.contiguous(), l = lists.contiguous(), hp = hist_ptr.contiguous(), hi = hist_items.contiguous();
    const int64_t blocks = (int64_t)weights.size(), B = l.size(0), K = l.size(1), I = t.size(0), R = hp.numel() - 1, n = hi.numel();
    TORCH_CHECK(blocks >= 1 && blocks <= 8 && t.size(1) % blocks == 0,
                "elimrec::history_support: 1 <= blocks <= 8 weights, and a table whose width splits into as many blocks");
    const int64_t d = t.size(1) / blocks;
    TORCH_CHECK(d % 4 == 0 && d >= 4 && d <= 256, "elimrec::history_support: a block needs d % 4 == 0 and 4 <= d <= 256 columns, got ", d);
    TORCH_CHECK(K >= 1 && K <= 256 && us.numel() == B, "elimrec::history_support: lists [B x K] with 1 <= K <= 256 and users [B]");
    TORCH_CHECK(top >= 1 && top <= elimrec_history_max_top(), "elimrec::history_support: 1 <= top <= ", elimrec_history_max_top(), ", got ", top);
    TORCH_CHECK(sqnorm.numel() == I * blocks && (blocks == 1 || sqnorm.dim() == 2),
                "elimrec::history_support: sqnorm must be [rows x ", blocks, "]");
    const at::Tensor sq = (sqnorm.dim() == 1 || sqnorm.stride(1) == 1 || blocks == 1) ? sqnorm : sqnorm.contiguous();
    TORCH_CHECK(R >= 1, "elimrec::history_support: hist_ptr needs n_rows + 1 >= 2 entries");
    checked_csr(hp, hi, R, "history_support", "hist_ptr", "hist_items");     // the ids' range is the kernel's to check
    float w[8];
    for (int64_t b = 0; b < blocks; ++b) w[b] = (float)weights[b];
    at::Tensor idx = at::empty({B, K, top}, l.options()), val = at::empty({B, K, top}, t.options());
    at::Tensor cnt = at::empty({B, K}, l.options()), mean = at::empty({B, K}, t.options());
    if (B == 0) return {idx, val, cnt, mean};
    check(elimrec_history_support(t.data_ptr<float>(), t.stride(0), I, (int)blocks, (int)d, sq.data_ptr<float>(),
                                  std::max<int64_t>(blocks, I > 1 ? sq.stride(0) : blocks), w, us.data_ptr<int64_t>(), l.data_ptr<int32_t>(), B,
                                  (int)K, hp.data_ptr<int64_t>(), n ? hi.data_ptr<int32_t>() : nullptr, R, (int)top, exclude_self ? 1 : 0,
                                  idx.data_ptr<int32_t>(), val.data_ptr<float>(), cnt.data_ptr<int32_t>(), mean.data_ptr<float>(), cur_stream()),
          "history_support");
    return {idx, val, cnt, mean};
}

// ---- bootstrap replicates of group means (one resample per (replicate, group), shared by the columns)
static at::Tensor bootstrap_impl(const at::Tensor &rows, const at::Tensor *rows_b, const at::Tensor &group_ptr, const at::Tensor &group_rows,
                                 int64_t R, int64_t seed, const char *who) {
    at::Tensor r = rowmajor(rows, "rows"), b;
    need(group_ptr, "group_ptr", at::kLong, 1); need(group_rows, "group_rows", at::kInt, 1);
    if (rows_b) {
        TORCH_CHECK(rows_b->sizes() == rows.sizes(), "elimrec::", who, ": rows_a and rows_b must have one shape");
        r = r.contiguous(); b = rowmajor(*rows_b, "rows_b").contiguous();                     // (one row stride for both)
    }
    const at::Tensor gp = group_ptr.contiguous(), gr = group_rows.contiguous();
    const int64_t G = gp.numel() - 1, n_listed = gr.numel(), n = r.size(0), C = r.size(1);
    TORCH_CHECK(G >= 1, "elimrec::", who, ": group_ptr needs G + 1 >= 2 entries");
    TORCH_CHECK(R >= 1 && R < ((int64_t)1 << 31), "elimrec::", who, ": 1 <= R < 2^31, got ", R);
    TORCH_CHECK(C >= 1, "elimrec::", who, ": rows needs at least one column");
    checked_csr(gp, gr, G, n, false, who, "group_ptr", "group_rows", "row indices", "the block has", "rows");
    at::Tensor out = at::empty({R, G, C}, r.options().dtype(at::kDouble));
    at::Tensor none = at::zeros({1}, gr.options());
    const int64_t step = elimrec_bootstrap_max_columns(), ld = n > 1 ? r.stride(0) : C;
    for (int64_t c0 = 0; c0 < C; c0 += step)
        check(elimrec_bootstrap_means(r.data_ptr<float>() + c0, rows_b ? b.data_ptr<float>() + c0 : nullptr, n, (int)std::min(step, C - c0), ld,
                                      gp.data_ptr<int64_t>(), n_listed ? gr.data_ptr<int32_t>() : none.data_ptr<int32_t>(), n_listed, (int)G, R,
                                      (uint64_t)seed, out.data_ptr<double>() + c0, C, 1, cur_stream()), who);
    return out;
}

at::Tensor bootstrap_means(const at::Tensor &rows, const at::Tensor &group_ptr, const at::Tensor &group_rows, int64_t R, int64_t seed) {
    return bootstrap_impl(rows, nullptr, group_ptr, group_rows, R, seed, "bootstrap_means");
}

at::Tensor bootstrap_diff_means(const at::Tensor &rows_a, const at::Tensor &rows_b, const at::Tensor &group_ptr, const at::Tensor &group_rows,
                                int64_t R, int64_t seed) {
    return bootstrap_impl(rows_a, &rows_b, group_ptr, group_rows, R, seed, "bootstrap_diff_means");
}

at::Tensor sample_negatives(const at::Tensor &excl_ptr, const at::Tensor &excl_items, int64_t num_items, int64_t n_neg, int64_t seed) {
    need(excl_ptr, "excl_ptr", at::kLong, 1); need(excl_items, "excl_items", at::kInt, 1);
    const at::Tensor p = excl_ptr.contiguous(), it = excl_items.contiguous();
    const int64_t n_users = p.numel() - 1;
    const at::Tensor counts = (p.narrow(0, 1, n_users) - p.narrow(0, 0, n_users)).cpu();
    TORCH_CHECK(n_users == 0 || counts.max().item<int64_t>() < num_items - n_neg, "There is not enough integers to be sampled.");
    at::Tensor out = at::empty({n_users, n_neg}, it.options());
    check(elimrec_sample_negatives(p.data_ptr<int64_t>(), it.numel() ? it.data_ptr<int32_t>() : nullptr, n_users, num_items, (int)n_neg,
                                   (uint64_t)seed, out.data_ptr<int32_t>(), cur_stream()),
          "sample_negatives");
    return out;
}

std::tuple<at::Tensor, at::Tensor> score_topk_shard(const at::Tensor &Y, int64_t U, int64_t I, const at::Tensor &users, int64_t d, int64_t S,
                                                    int64_t head_mask, int64_t fusion_mode, int64_t predict_type,
                                                    const c10::optional<at::Tensor> &train_ptr, const c10::optional<at::Tensor> &train_items,
                                                    int64_t K, const at::Tensor &row_sum, int64_t I_total, int64_t id_offset) {
    const at::Tensor y = rowmajor(Y, "Y");
    need(users, "users", at::kLong, 1); need(row_sum, "row_sum", at::kFloat, 1);
    const at::Tensor u = users.contiguous(), rs = row_sum.contiguous();
    const int64_t B = u.numel();
    TORCH_CHECK(K >= 1 && rs.numel() == B, "elimrec::score_topk_shard: K >= 1, one row sum per user");
    at::Tensor tp, ti;
    train_csr(train_ptr, train_items, tp, ti);
    at::Tensor idx = at::empty({B, K}, y.options().dtype(at::kInt)), val = at::empty({B, K}, y.options());
    const size_t need_ws = elimrec_score_workspace_for((int)B, U, I, (int)S, (int)K, (int)d, 0);
    at::Tensor ws = at::empty({(int64_t)(need_ws ? need_ws : 1)}, y.options().dtype(at::kByte));
    check(elimrec_score_topk_shard(y.data_ptr<float>(), y.stride(0), U, I, u.data_ptr<int64_t>(), (int)B, (int)d, (int)S, (uint32_t)head_mask,
                                   (int)fusion_mode, (int)predict_type, nullptr, tp.defined() ? tp.data_ptr<int64_t>() : nullptr,
                                   ti.defined() ? ti.data_ptr<int32_t>() : nullptr, nullptr, 0, (int)K, idx.data_ptr<int32_t>(),
                                   val.data_ptr<float>(), ws.data_ptr(), (size_t)ws.numel(), 2, rs.data_ptr<float>(), I_total, id_offset,
                                   cur_stream()),
          "score_topk_shard");
    return {idx, val};
}

std::tuple<at::Tensor, at::Tensor> topk_merge(const at::Tensor &cand_val, const at::Tensor &cand_idx, int64_t K) {
    need(cand_val, "cand_val", at::kFloat, 2); need(cand_idx, "cand_idx", at::kInt, 2);
    const at::Tensor v = cand_val.contiguous(), i = cand_idx.contiguous();
    TORCH_CHECK(v.sizes() == i.sizes() && K >= 1 && K <= v.size(1), "elimrec::topk_merge: [B x n] values and ids, 1 <= K <= n");
    at::Tensor idx = at::empty({v.size(0), K}, i.options()), val = at::empty({v.size(0), K}, v.options());
    check(elimrec_topk_merge(v.data_ptr<float>(), i.data_ptr<int32_t>(), (int)v.size(0), (int)v.size(1), (int)K, idx.data_ptr<int32_t>(),
                             val.data_ptr<float>(), cur_stream()),
          "topk_merge");
    return {idx, val};
}

// ---- row-sharded feature constants: the all-to-all id lookup (elimrec_lookup_counts / _pack / _unpack). user_bounds / item_bounds:
// world + 1 ascending row bounds of the owners' blocks.
static void bounds(const std::vector<int64_t> &ub, const std::vector<int64_t> &ib, int64_t &world) {
    world = (int64_t)ub.size() - 1;
    TORCH_CHECK(world >= 1 && world <= ELIMREC_MAX_RANKS && ib.size() == ub.size(), "elimrec::lookup: user_bounds / item_bounds hold world + 1 entries");
}

at::Tensor lookup_counts(const at::Tensor &acts, int64_t U, int64_t I, std::vector<int64_t> user_bounds, std::vector<int64_t> item_bounds) {
    int64_t world;
    bounds(user_bounds, item_bounds, world);
    need(acts, "acts", at::kInt, 2);
    const at::Tensor a = acts.contiguous();
    TORCH_CHECK(a.size(0) == world, "elimrec::lookup_counts: one active-row list per rank");
    at::Tensor counts = at::empty({world, world}, a.options());
    check(elimrec_lookup_counts(a.data_ptr<int32_t>(), (int)world, a.size(1), U, I, user_bounds.data(), item_bounds.data(),
                                counts.data_ptr<int32_t>(), cur_stream()),
          "lookup_counts");
    return counts;
}

std::tuple<at::Tensor, at::Tensor> lookup_pack(const at::Tensor &acts, int64_t U, int64_t I, std::vector<int64_t> user_bounds,
                                               std::vector<int64_t> item_bounds, int64_t me, const at::Tensor &shard, int64_t row_bytes) {
    int64_t world;
    bounds(user_bounds, item_bounds, world);
    need(acts, "acts", at::kInt, 2);
    const at::Tensor a = acts.contiguous();
    TORCH_CHECK(shard.is_cuda() && shard.is_contiguous() && row_bytes % 16 == 0 && me >= 0 && me < world && a.size(0) == world,
                "elimrec::lookup_pack: contiguous device shard, rows padded to 16 bytes, 0 <= me < world");
    at::Tensor send = at::empty({world * a.size(1), row_bytes}, a.options().dtype(at::kByte));     // worst case: every listed row is mine
    at::Tensor off = at::empty({world + 1}, a.options());
    check(elimrec_lookup_pack(a.data_ptr<int32_t>(), (int)world, a.size(1), U, I, user_bounds.data(), item_bounds.data(), (int)me,
                              shard.data_ptr(), row_bytes, send.data_ptr(), off.data_ptr<int32_t>(), cur_stream()),
          "lookup_pack");
    return {send, off};
}

std::tuple<at::Tensor, at::Tensor> lookup_unpack(const at::Tensor &act, int64_t U, int64_t I, std::vector<int64_t> user_bounds,
                                                 std::vector<int64_t> item_bounds, int64_t me, const at::Tensor &rows, int64_t row_bytes,
                                                 int64_t dtype, int64_t sum_d, bool direct) {
    int64_t world;
    bounds(user_bounds, item_bounds, world);
    need(act, "act", at::kInt, 1);
    const at::Tensor a = act.contiguous();
    TORCH_CHECK(rows.is_cuda() && rows.is_contiguous() && sum_d >= 1 && dtype >= 0 && dtype <= 2, "elimrec::lookup_unpack: bad arguments");
    at::Tensor S = at::zeros({a.numel(), sum_d}, a.options().dtype(at::kFloat)), c = at::zeros({a.numel()}, a.options().dtype(at::kFloat));
    check(elimrec_lookup_unpack(a.data_ptr<int32_t>(), (int)world, a.numel(), U, I, user_bounds.data(), item_bounds.data(), (int)me,
                                rows.data_ptr(), row_bytes, (int)dtype, (int)sum_d, direct ? 1 : 0, S.data_ptr<float>(), S.stride(0),
                                c.data_ptr<float>(), cur_stream()),
          "lookup_unpack");
    return {S, c};
}

}  // namespace

TORCH_LIBRARY(elimrec, m) {
    m.def("propagate(Tensor rowptr, Tensor col, Tensor val, Tensor X, int L, bool transpose=False) -> Tensor");
    m.def("segment_reduce(Tensor rows, Tensor keys, int split_key) -> (Tensor, Tensor, Tensor)");
    m.def("linear_fwd(Tensor A, Tensor W, Tensor? bias) -> Tensor");
    m.def("linear_bwd_w(Tensor A, Tensor B) -> (Tensor, Tensor)");
    m.def("bpr_head_fwd(Tensor Y, int U, int I, Tensor users, Tensor pos, Tensor neg, int d, float[] block_weights) -> (Tensor, Tensor, Tensor)");
    m.def("adam_step_(Tensor(a!) p, Tensor g, Tensor(b!) m, Tensor(c!) v, float lr, float beta1, float beta2, float eps, float weight_decay, int step) -> Tensor(a!)");
    m.def("score_topk(Tensor Y, int U, int I, Tensor users, int d, int S, int head_mask, int fusion_mode, int predict_type, Tensor? train_ptr, Tensor? train_items, int K, int tie_order=0) -> (Tensor, Tensor)");
    m.def("rank_metrics(Tensor topk_idx, Tensor truth_ptr, Tensor truth_items, int[] metric_ids) -> Tensor");
    m.def("group_metric_means(Tensor rows, Tensor group_ptr, Tensor group_rows) -> Tensor");
    m.def("sample_triplets(Tensor user_ids, Tensor ptr, Tensor items, int num_items, int n, int seed, int epoch) -> (Tensor, Tensor, Tensor)");
    m.def("bpr_head_bwd(Tensor grad_rows, Tensor keys, Tensor grad_out, int n_rows) -> Tensor");
    m.def("score_shard_row_sums(Tensor Y, int U, int I, Tensor users, int d, int S, int head_mask, int fusion_mode, int I_total) -> Tensor");
    m.def("score_topk_shard(Tensor Y, int U, int I, Tensor users, int d, int S, int head_mask, int fusion_mode, int predict_type, Tensor? train_ptr, Tensor? train_items, int K, Tensor row_sum, int I_total, int id_offset) -> (Tensor, Tensor)");
    m.def("topk_merge(Tensor cand_val, Tensor cand_idx, int K) -> (Tensor, Tensor)");
    m.def("score_candidates(Tensor Y, int U, int I, Tensor users, int d, int S, int head_mask, int fusion_mode, int predict_type, Tensor cand_ptr, Tensor cand_items, int width) -> Tensor");
    m.def("score_effects(Tensor Y, int U, int I, Tensor users, int d, int S, int head_mask, int fusion_mode, Tensor cand_ptr, Tensor cand_items, int width) -> Tensor");
    m.def("rank_targets(Tensor scores, Tensor tgt_ptr, Tensor tgt_items) -> Tensor");
    m.def("rank_values(Tensor scores, Tensor val_ptr, Tensor vals, Tensor? skip) -> Tensor");
    m.def("segment_row_sum(Tensor table, Tensor ptr, Tensor rows, Tensor weights, int row_offset) -> Tensor");
    m.def("cosine_topk(Tensor table, Tensor sqnorm, Tensor query_rows, int K, bool exclude_self) -> (Tensor, Tensor)");
    m.def("audience_topk(Tensor Y, int U, int I, Tensor items, Tensor? excl_ptr, Tensor? excl_users, int d, int S, int head_mask, int fusion_mode, "
          "int predict_type, int K, Tensor? sqnorm, Tensor? row_sum, int I_total) -> (Tensor, Tensor)");
    m.def("list_overlap(Tensor a, Tensor b) -> Tensor");
    m.def("list_pair_cosine(Tensor table, Tensor sqnorm, Tensor lists, int blocks) -> Tensor");
    m.def("list_exposure(Tensor lists, int n_rows) -> Tensor");
    m.def("mmr_rerank(Tensor table, Tensor sqnorm, Tensor pool_idx, Tensor pool_val, int K, float lam) -> (Tensor, Tensor, Tensor)");
    m.def("calibrate_rerank(Tensor pool_idx, Tensor pool_val, Tensor class_of, Tensor target, int K, float lam, float smooth) -> (Tensor, Tensor, Tensor)");
    m.def("list_calibration(Tensor lists, Tensor class_of, int C, Tensor target, float smooth) -> (Tensor, Tensor)");
    m.def("kmeans_assign(Tensor table, Tensor sqnorm, Tensor centroids, Tensor centroid_sqnorm, Tensor? prev) -> (Tensor, Tensor, Tensor)");
    m.def("kmeans_update(Tensor table, Tensor sqnorm, Tensor assign, Tensor centroids, Tensor centroid_sqnorm) -> (Tensor, Tensor, Tensor, Tensor)");
    m.def("uniformity_sum(Tensor table, Tensor sqnorm, Tensor rows, float t) -> (Tensor, Tensor)");
    m.def("row_gram(Tensor table, Tensor sqnorm, Tensor rows) -> (Tensor, Tensor, Tensor)");
    m.def("cross_topk(Tensor query_table, Tensor? query_sqnorm, Tensor table, Tensor? sqnorm, Tensor query_rows, Tensor? excl_ptr, Tensor? excl_rows, int K) -> (Tensor, Tensor)");
    m.def("als_solve(Tensor ptr, Tensor nbr, Tensor F, Tensor A0, Tensor reg, float conf, Tensor? rows) -> Tensor");
    m.def("gram_counts(Tensor q_ptr, Tensor q_nbr, Tensor o_ptr, Tensor o_nbr, float l2) -> Tensor");
    m.def("spd_inverse(Tensor A) -> (Tensor, Tensor)");
    m.def("ease_topk(Tensor P, Tensor hist_ptr, Tensor hist_items, Tensor? excl_ptr, Tensor? excl_items, Tensor users, int K) -> (Tensor, Tensor)");
    m.def("cooccur_topk(Tensor q_ptr, Tensor q_nbr, Tensor o_ptr, Tensor o_nbr, Tensor rows, int K, str measure) -> (Tensor, Tensor, Tensor)");
    m.def("walk_topk(Tensor q_ptr, Tensor q_nbr, Tensor o_ptr, Tensor o_nbr, Tensor rows, int K, Tensor mid_weight, Tensor row_scale, Tensor col_scale) -> (Tensor, Tensor)");
    m.def("neighbour_vote_topk(Tensor nbr_idx, Tensor nbr_val, Tensor hist_ptr, Tensor hist_items, Tensor? excl_ptr, Tensor? excl_items, Tensor users, int K) -> (Tensor, Tensor, Tensor)");
    m.def("pick_hard_negatives(Tensor user_table, Tensor user_sqnorm, Tensor item_table, Tensor item_sqnorm, float[] weights, Tensor users, "
          "Tensor cands) -> (Tensor, Tensor, Tensor)");
    m.def("history_support(Tensor table, Tensor sqnorm, float[] weights, Tensor users, Tensor lists, Tensor hist_ptr, Tensor hist_items, int top, "
          "bool exclude_self) -> (Tensor, Tensor, Tensor, Tensor)");
    m.def("bootstrap_means(Tensor rows, Tensor group_ptr, Tensor group_rows, int R, int seed) -> Tensor");
    m.def("bootstrap_diff_means(Tensor rows_a, Tensor rows_b, Tensor group_ptr, Tensor group_rows, int R, int seed) -> Tensor");
    m.def("sample_negatives(Tensor excl_ptr, Tensor excl_items, int num_items, int n_neg, int seed) -> Tensor");
    m.def("lookup_counts(Tensor acts, int U, int I, int[] user_bounds, int[] item_bounds) -> Tensor");
    m.def("lookup_pack(Tensor acts, int U, int I, int[] user_bounds, int[] item_bounds, int me, Tensor shard, int row_bytes) -> (Tensor, Tensor)");
    m.def("lookup_unpack(Tensor act, int U, int I, int[] user_bounds, int[] item_bounds, int me, Tensor rows, int row_bytes, int dtype, int sum_d, bool direct) -> (Tensor, Tensor)");
}

TORCH_LIBRARY_IMPL(elimrec, CUDA, m) {
    m.impl("propagate", &propagate);
    m.impl("segment_reduce", &segment_reduce);
    m.impl("linear_fwd", &linear_fwd);
    m.impl("linear_bwd_w", &linear_bwd_w);
    m.impl("bpr_head_fwd", &bpr_head_fwd);
    m.impl("adam_step_", &adam_step_);
    m.impl("score_topk", &score_topk);
    m.impl("rank_metrics", &rank_metrics);
    m.impl("group_metric_means", &group_metric_means);
    m.impl("sample_triplets", &sample_triplets);
    m.impl("bpr_head_bwd", &bpr_head_bwd);
    m.impl("score_shard_row_sums", &score_shard_row_sums);
    m.impl("score_topk_shard", &score_topk_shard);
    m.impl("topk_merge", &topk_merge);
    m.impl("score_candidates", &score_candidates);
    m.impl("score_effects", &score_effects);
    m.impl("rank_targets", &rank_targets);
    m.impl("rank_values", &rank_values);
    m.impl("segment_row_sum", &segment_row_sum);
    m.impl("cosine_topk", &cosine_topk);
    m.impl("audience_topk", &audience_topk);
    m.impl("list_overlap", &list_overlap);
    m.impl("list_pair_cosine", &list_pair_cosine);
    m.impl("list_exposure", &list_exposure);
    m.impl("mmr_rerank", &mmr_rerank);
    m.impl("calibrate_rerank", &calibrate_rerank);
    m.impl("list_calibration", &list_calibration);
    m.impl("kmeans_assign", &kmeans_assign);
    m.impl("kmeans_update", &kmeans_update);
    m.impl("uniformity_sum", &uniformity_sum);
    m.impl("row_gram", &row_gram);
    m.impl("cross_topk", &cross_topk);
    m.impl("als_solve", &als_solve);
    m.impl("gram_counts", &gram_counts);
    m.impl("spd_inverse", &spd_inverse);
    m.impl("ease_topk", &ease_topk);
    m.impl("cooccur_topk", &cooccur_topk);
    m.impl("walk_topk", &walk_topk);
    m.impl("neighbour_vote_topk", &neighbour_vote_topk);
    m.impl("pick_hard_negatives", &pick_hard_negatives);
    m.impl("history_support", &history_support);
    m.impl("bootstrap_means", &bootstrap_means);
    m.impl("bootstrap_diff_means", &bootstrap_diff_means);
    m.impl("sample_negatives", &sample_negatives);
    m.impl("lookup_counts", &lookup_counts);
    m.impl("lookup_pack", &lookup_pack);
    m.impl("lookup_unpack", &lookup_unpack);
}
