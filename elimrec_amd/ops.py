"""Tensor-level wrappers over the C ABI (include/elimrec_hip.h).

torch is plumbing here: it owns device memory and the current HIP stream; every function below
hands raw device pointers to libelimrec_hip.so. Inputs must live on a HIP device -- anything
else raises (no CPU path).
"""
import collections
import ctypes
import math

import numpy as np

import torch

from . import _lib


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream():
    """Handle of torch's current HIP stream on the current device (the fast private accessor when present)."""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def _dev(t, name, dtype=torch.float32):
    if t is None:
        return None
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError("elimrec_amd.ops: '%s' must be a HIP device tensor (the hot path has no CPU "
                           "implementation)" % name)
    if t.dtype != dtype:
        raise TypeError("elimrec_amd.ops: '%s' must be %s, got %s" % (name, dtype, t.dtype))
    return t.data_ptr()


def _rowmajor(t, name):
    """(pointer, leading dimension) of a 2-D tensor whose rows are contiguous."""
    if t.dim() != 2 or t.stride(1) != 1:
        raise ValueError("elimrec_amd.ops: '%s' must be 2-D with unit column stride" % name)
    return _dev(t, name), t.stride(0)


def linear_fwd(A, W, bias, out, act=None):
    """out[m, n] = act(sum_k A[m,k] W[n,k] + bias[n]); A/out may be column slices of wider tables. act: None | 'relu'."""
    lib = _lib.load()
    a, lda = _rowmajor(A, "A")
    w, ldw = _rowmajor(W, "W")
    c, ldc = _rowmajor(out, "out")
    M, K = A.shape
    N = W.shape[0]
    assert W.shape[1] == K and out.shape[0] == M and out.shape[1] == N
    if act is None:
        _lib.check(lib.elimrec_linear_fwd(a, lda, w, ldw, _dev(bias, "bias"), c, ldc, M, N, K, _stream()), "linear_fwd")
        return out
    if act != "relu":
        raise ValueError("linear_fwd: the fused epilogue knows 'relu' only (got %r)" % (act,))
    arr = (_lib.LinearDesc * 1)(_lib.LinearDesc(a, lda, w, ldw, _dev(bias, "bias"), c, ldc, M, N, K, None, None, 0, None, None, 1))
    _lib.check(lib.elimrec_linear_fwd_batched(arr, 1, _stream()), "linear_fwd(relu)")
    return out


def linear_fwd_batched(problems):
    """problems: list of (A, W, bias, out[, rowscale, add[, row_index, row_count]]) -- independent Linears sharing
    one launch (<= 8).  out = A.W^T + rowscale[:, None] * bias + add   (rowscale, add optional).
    row_index (int32 [M]): output row m reads row row_index[m] of A / rowscale / add; row_range (device int32[2]):
    only output rows [begin, min(end, M)) are produced."""
    n = len(problems)
    arr = (_lib.LinearDesc * n)()
    for i, pr in enumerate(problems):
        A, W, bias, out = pr[:4]
        rowscale = pr[4] if len(pr) > 4 else None
        add = pr[5] if len(pr) > 5 else None
        row_index = pr[6] if len(pr) > 6 else None
        row_range = pr[7] if len(pr) > 7 else None
        a, lda = _rowmajor(A, "A")
        w, ldw = _rowmajor(W, "W")
        c, ldc = _rowmajor(out, "out")
        K = A.shape[1]
        M = A.shape[0] if row_index is None else row_index.numel()
        N = W.shape[0]
        assert W.shape[1] == K and out.shape[0] == M and out.shape[1] == N
        ad, ldadd = (None, 0)
        if add is not None:
            assert add.shape == (A.shape[0], N)
            ad, ldadd = _rowmajor(add, "add")
        if rowscale is not None:
            assert rowscale.is_contiguous() and rowscale.numel() == A.shape[0]
        arr[i] = _lib.LinearDesc(a, lda, w, ldw, _dev(bias, "bias"), c, ldc, M, N, K, _dev(rowscale, "rowscale"), ad, ldadd,
                                 _dev(row_index, "row_index", torch.int32), _dev(row_range, "row_range", torch.int32))
    _lib.check(_lib.load().elimrec_linear_fwd_batched(arr, n, _stream()), "linear_fwd_batched")


def _bwd_descs(problems):
    n = len(problems)
    arr = (_lib.LinearBwdDesc * n)()
    for i, pr in enumerate(problems):
        a, lda = _rowmajor(pr["A"], "A")
        b, ldb = _rowmajor(pr["B"], "B")
        o, ldo = _rowmajor(pr["out"], "out")
        R = pr["A"].shape[0] if pr.get("rows") is None else pr["rows"]
        n1, n2 = pr["out"].shape
        arr[i] = _lib.LinearBwdDesc(a, lda, b, ldb, _dev(pr.get("row_index"), "row_index", torch.int32),
                                    _dev(pr.get("rng"), "range", torch.int32), R, n1, n2, o, ldo,
                                    _dev(pr.get("colsum"), "colsum"), 1 if pr.get("accumulate") else 0,
                                    _dev(pr.get("colsum_weight"), "colsum_weight"))
    return arr, n


def linear_bwd_w_batched_workspace(shapes):
    """shapes: list of (R, n1, n2)."""
    n = len(shapes)
    arr = (_lib.LinearBwdDesc * n)()
    for i, (R, n1, n2) in enumerate(shapes):
        arr[i] = _lib.LinearBwdDesc(None, 0, None, 0, None, None, R, n1, n2, None, 0, None, 0)
    return int(_lib.load().elimrec_linear_bwd_w_batched_workspace(arr, n))


def linear_bwd_w_batched(problems, workspace, merge=None, defer_reduce=False, defer_all=False):
    """problems: list of dicts(A, B, out[, row_index, rng, colsum, accumulate, rows]) in one launch pair.
    merge: dict(rows, keys, world, U, I, srcA, srcB, mask, M) -- the arguments of slab.merge_rows, run as extra workgroups
    of the partial launch (elimrec_linear_bwd_w_batched_merge).
    defer_reduce: stop after the partial launch and return the handle `linear_bwd_w_reduce` / `slab.hop(bwd_w=)` finish
    the gradients with (the outputs hold nothing until then). defer_all: launch nothing, return the handle: both phases
    ride in hop launches (slab.hop(bwd_w=handle, bwd_w_phase=0), then bwd_w_phase=1)."""
    arr, n = _bwd_descs(problems)
    if defer_all:
        assert merge is None
        need = int(_lib.load().elimrec_linear_bwd_w_batched_workspace(arr, n))
        assert workspace.numel() >= need, "linear_bwd_w: workspace too small"
        return (arr, n, workspace)
    wsp, wsn = _dev(workspace, "workspace", torch.uint8), workspace.numel()
    if merge is None and not defer_reduce:
        _lib.check(_lib.load().elimrec_linear_bwd_w_batched(arr, n, wsp, wsn, _stream()), "linear_bwd_w_batched")
        return None
    if merge is not None:
        rows, keys, srcA, srcB, M, world = merge["rows"], merge["keys"], merge["srcA"], merge["srcB"], merge["M"], merge["world"]
        R = keys.numel() // world
        assert rows.is_contiguous() and rows.shape == (world * R, (M if M else 2) * srcA.cols)
        assert merge["mask"].numel() * 32 >= merge["U"] + merge["I"]
        margs = (_dev(rows, "rows"), _dev(keys, "keys", torch.int32), int(world), R, int(merge["U"]), int(merge["I"]), srcA.ns, srcA.w,
                 int(M), _dev(srcA.data, "srcA"), _dev(srcB.data, "srcB"), _dev(merge["mask"], "mask", torch.int32))
    else:
        margs = (None, None, 1, 1, 0, 0, 1, 4, 0, None, None, None)
    _lib.check(_lib.load().elimrec_linear_bwd_w_batched_merge(arr, n, wsp, wsn, *margs, 1 if defer_reduce else 0, _stream()),
               "linear_bwd_w_batched_merge")
    return (arr, n, workspace) if defer_reduce else None


def linear_bwd_w_reduce(handle):
    """The fixed-order slab reduce of a `linear_bwd_w_batched(..., defer_reduce=True)` launch, as a launch of its own."""
    arr, n, workspace = handle
    _lib.check(_lib.load().elimrec_linear_bwd_w_reduce(arr, n, _dev(workspace, "workspace", torch.uint8), workspace.numel(), _stream()),
               "linear_bwd_w_reduce")


def linear_bwd_w_workspace(R, n1, n2):
    return int(_lib.load().elimrec_linear_bwd_w_workspace(R, n1, n2))


def linear_bwd_w(A, B, out, workspace, row_index=None, rng=None, colsum=None, accumulate=False, rows=None):
    """out[i, j] (+)= sum_r A[r, i] * B[row_index[r] or r, j]; colsum[i] (+)= sum_r A[r, i]."""
    lib = _lib.load()
    a, lda = _rowmajor(A, "A")
    b, ldb = _rowmajor(B, "B")
    o, ldo = _rowmajor(out, "out")
    R = A.shape[0] if rows is None else rows
    n1, n2 = out.shape
    _lib.check(lib.elimrec_linear_bwd_w(a, lda, b, ldb, _dev(row_index, "row_index", torch.int32),
                                        _dev(rng, "range", torch.int32), R, n1, n2, o, ldo, _dev(colsum, "colsum"),
                                        1 if accumulate else 0, _dev(workspace, "workspace", torch.uint8),
                                        workspace.numel(), _stream()), "linear_bwd_w")
    return out


def assemble_x0(user_emb, item_emb, X0, M):
    U, d = user_emb.shape
    I = item_emb.shape[0]
    assert X0.is_contiguous() and X0.shape == (U + I, M * d)
    assert user_emb.is_contiguous() and item_emb.is_contiguous()
    _lib.check(_lib.load().elimrec_assemble_x0(_dev(user_emb, "user_emb"), _dev(item_emb, "item_emb"), _dev(X0, "X0"),
                                               U, I, d, M, _stream()), "assemble_x0")
    return X0


LONG_ROW_THRESHOLD = 64   # rows with more non-zeros are split across waves (csrc/spmm.hip)


class Csr:
    """Device CSR (int32 rowptr/col, fp32 val) + the optional row-split plan for long rows."""

    def __init__(self, rowptr, col, val, n_rows):
        self.rowptr, self.col, self.val, self.n_rows = rowptr, col, val, n_rows
        self._split = None
        self._split_tensors = None

    @staticmethod
    def from_scipy(m, device, C=None, threshold=LONG_ROW_THRESHOLD):
        import numpy as np
        m = m.tocsr()
        m.sort_indices()
        if m.nnz >= 2 ** 31:
            raise ValueError("CSR with >= 2^31 non-zeros is not supported")
        csr = Csr(torch.from_numpy(m.indptr.astype(np.int32)).to(device),
                  torch.from_numpy(m.indices.astype(np.int32)).to(device),
                  torch.from_numpy(m.data.astype(np.float32)).to(device), m.shape[0])
        if C is not None:
            csr.build_split(C, threshold)
        return csr

    def build_split(self, C, threshold=LONG_ROW_THRESHOLD):
        """Cut rows with more than `threshold` non-zeros into segments of <= threshold (host, once)."""
        import numpy as np
        rowptr = self.rowptr.cpu().numpy().astype(np.int64)
        deg = np.diff(rowptr)
        long_rows = np.nonzero(deg > threshold)[0]
        dev = self.rowptr.device
        # rows in order of decreasing length (split rows count as empty in the main pass): a scheduling hint
        order = np.argsort(-np.where(deg > threshold, 0, deg), kind="stable").astype(np.int32)
        self._row_order = torch.from_numpy(order).to(dev)
        ro = self._row_order.data_ptr()
        # (row, begin, end) of the rows that are not split, in that order: the streaming form of the row kernel
        keep = order[deg[order] <= threshold].astype(np.int64)
        items = np.stack([keep, rowptr[keep], rowptr[keep + 1]], 1).astype(np.int32)
        self._row_items = torch.from_numpy(np.ascontiguousarray(items)).to(dev)
        ri, n_items = self._row_items.data_ptr(), int(len(keep))
        if len(long_rows) == 0:
            self._split_tensors = None
            self._split = _lib.CsrSplit(0, 0, 0, None, None, None, None, None, ro, None, ri, n_items)
            self._split_C = C
            return self
        nseg = (deg[long_rows] + threshold - 1) // threshold
        seg_ptr = np.concatenate([[0], np.cumsum(nseg)])
        total = int(seg_ptr[-1])
        seg_row = np.repeat(np.arange(len(long_rows)), nseg)
        k = np.arange(total) - seg_ptr[seg_row]
        beg = rowptr[long_rows][seg_row] + k * threshold
        end = np.minimum(beg + threshold, rowptr[long_rows + 1][seg_row])
        t = (torch.from_numpy(long_rows.astype(np.int32)).to(dev), torch.from_numpy(seg_ptr.astype(np.int32)).to(dev),
             torch.from_numpy(np.stack([beg, end], 1).astype(np.int32).copy()).to(dev),
             torch.empty(total, 2 * C, dtype=torch.float32, device=dev),   # wide + narrow partial regions
             torch.from_numpy(seg_row.astype(np.int32)).to(dev),
             torch.zeros(2 * len(long_rows), dtype=torch.int32, device=dev))
        self._split_tensors = t
        self._split = _lib.CsrSplit(int(threshold), len(long_rows), total, t[0].data_ptr(), t[1].data_ptr(),
                                    t[2].data_ptr(), t[3].data_ptr(), t[4].data_ptr(), ro, t[5].data_ptr(), ri, n_items)
        self._split_C = C
        return self

    def desc(self):
        """struct elimrec_csr for the block-CSR entry points (keeps the tensors alive through self)."""
        sp = self._split if self._split is not None else _lib.CsrSplit(0, 0, 0, None, None, None, None, None, None, None, None, 0)
        self._desc = _lib.CsrDesc(self.n_rows, self.rowptr.data_ptr(), self.col.data_ptr(), self.val.data_ptr(), sp)
        return ctypes.byref(self._desc)

    def split_ref(self, C):
        if self._split is None or self._split.n_long == 0:
            return None
        if self._split_C < C:
            raise ValueError("row-split plan was built for C=%d, got C=%d" % (self._split_C, C))
        return ctypes.byref(self._split)


def spmm_hop(csr, Xin, Xout=None, acc_in=None, acc_out=None, scale=1.0):
    C = Xin.shape[1]
    assert Xin.is_contiguous()
    _lib.check(_lib.load().elimrec_spmm_hop(_dev(csr.rowptr, "rowptr", torch.int32), _dev(csr.col, "col", torch.int32),
                                            _dev(csr.val, "val"), csr.n_rows, C, csr.split_ref(C), _dev(Xin, "Xin"),
                                            _dev(Xout, "Xout"), _dev(acc_in, "acc_in"), _dev(acc_out, "acc_out"),
                                            float(scale), _stream()), "spmm_hop")


def propagate(csr, X0, L, tmp0, tmp1, out):
    C = X0.shape[1]
    assert X0.is_contiguous() and out.is_contiguous() and out.shape == X0.shape
    _lib.check(_lib.load().elimrec_propagate(_dev(csr.rowptr, "rowptr", torch.int32), _dev(csr.col, "col", torch.int32),
                                             _dev(csr.val, "val"), csr.n_rows, C, csr.split_ref(C), L, _dev(X0, "X0"),
                                             _dev(tmp0, "tmp0"), _dev(tmp1, "tmp1"), _dev(out, "out"), _stream()),
               "propagate")
    return out


def bipartite_workspace(U, I, d, M):
    return int(_lib.load().elimrec_bipartite_workspace(U, I, d, M))


def propagate_bipartite(P, Q, U, I, d, M, L, user_emb, XI, out, workspace, narrow_out=None):
    assert user_emb.is_contiguous() and XI.is_contiguous() and out.is_contiguous()
    assert XI.shape == (I, d * M) and out.shape == (U + I, d * M) and user_emb.shape == (U, d)
    assert narrow_out is None or (narrow_out.is_contiguous() and narrow_out.shape == (U + I, d))
    _lib.check(_lib.load().elimrec_propagate_bipartite(P.desc(), Q.desc(), U, I, d, M, L, _dev(user_emb, "user_emb"),
                                                       _dev(XI, "XI"), _dev(out, "out"), _dev(narrow_out, "narrow_out"),
                                                       _dev(workspace, "workspace", torch.uint8), workspace.numel(),
                                                       _stream()), "propagate_bipartite")
    return out


def propagate_bipartite_bwd(PT, QT, U, I, d, M, L, G, H, active_rows, seg_info, gXI, gEu, workspace):
    assert G.is_contiguous() and H.is_contiguous() and gXI.is_contiguous() and gEu.is_contiguous()
    assert G.shape == (U + I, d * M) and H.shape == (U + I, d) and gXI.shape == (I, d * M) and gEu.shape == (U, d)
    _lib.check(_lib.load().elimrec_propagate_bipartite_bwd(PT.desc(), QT.desc(), U, I, d, M, L, _dev(G, "G"), _dev(H, "H"),
                                                           _dev(active_rows, "active_rows", torch.int32),
                                                           _dev(seg_info, "seg_info", torch.int32), active_rows.numel(),
                                                           _dev(gXI, "gXI"), _dev(gEu, "gEu"),
                                                           _dev(workspace, "workspace", torch.uint8), workspace.numel(),
                                                           _stream()), "propagate_bipartite_bwd")


def folded_workspace(N, d):
    return int(_lib.load().elimrec_folded_workspace(N, d))


def propagate_folded(A, U, I, d, L, X0, out0, narrow, workspace):
    """out0: [N x d] window (unit column stride) of a wider table; X0, narrow: contiguous [N x d]."""
    assert X0.is_contiguous() and narrow.is_contiguous() and X0.shape == (U + I, d) and narrow.shape == (U + I, d)
    o, ldo = _rowmajor(out0, "out0")
    assert out0.shape == (U + I, d)
    _lib.check(_lib.load().elimrec_propagate_folded(A.desc(), U, I, d, L, _dev(X0, "X0"), o, ldo, _dev(narrow, "narrow"),
                                                    _dev(workspace, "workspace", torch.uint8), workspace.numel(),
                                                    _stream()), "propagate_folded")


def source_rows_split(dOutR, count, d, M, world, out):
    """out[w][s] = [H | G] of dOutR[s] (H = sum of its M column blocks, G = block 0) in peer w's column slice, s < count:
    out [world x n x 2*d/world]."""
    n = dOutR.shape[0]
    assert dOutR.is_contiguous() and out.is_contiguous() and dOutR.shape[1] == d * M and out.shape == (world, n, 2 * d // world)
    _lib.check(_lib.load().elimrec_source_rows_split(_dev(dOutR, "dOutR"), _dev(count, "count", torch.int32), n, d, M, world,
                                                     _dev(out, "out"), _stream()), "source_rows_split")


def propagate_folded_bwd(AT, U, I, d, M, L, dOutR, active_rows, seg_info, srcA, srcB, grad, workspace, active_mask=None):
    """dOutR None: srcA / srcB and active_mask were prefilled by the caller."""
    for t in (srcA, srcB, grad):
        assert t.is_contiguous()
    assert grad.shape == (U + I, d) and (dOutR is None or (dOutR.is_contiguous() and dOutR.shape[1] == d * M))
    _lib.check(_lib.load().elimrec_propagate_folded_bwd(AT.desc(), U, I, d, M, L, _dev(dOutR, "dOutR"),
                                                        _dev(active_rows, "active_rows", torch.int32),
                                                        _dev(seg_info, "seg_info", torch.int32),
                                                        0 if active_rows is None else active_rows.numel(),
                                                        _dev(srcA, "srcA"), _dev(srcB, "srcB"), _dev(grad, "grad"),
                                                        _dev(active_mask, "active_mask", torch.int32),
                                                        _dev(workspace, "workspace", torch.uint8), workspace.numel(),
                                                        _stream()), "propagate_folded_bwd")


def block_spmm(A, Xin, Xout=None, add1=None, acc_out=None, scale=1.0):
    """r = A . Xin (a column window of a wider table is fine); Xout = r; acc_out = (r + add1) * scale."""
    x, ld = _rowmajor(Xin, "Xin")
    W = Xin.shape[1]
    for t in (Xout, add1, acc_out):
        assert t is None or (t.stride(0) == ld and t.stride(1) == 1 and t.shape[1] == W)
    _lib.check(_lib.load().elimrec_block_spmm(A.desc(), W, ld, x, _dev(Xout, "Xout"), _dev(add1, "add1"),
                                              _dev(acc_out, "acc_out"), float(scale), _stream()), "block_spmm")


def blocksum_rows(G, active_rows, seg_info, d, M, H, slot_major=False):
    """H[node] = sum over the M column blocks of the node's row of G (rows of G indexed by node, or by slot)."""
    assert G.is_contiguous() and H.is_contiguous()
    _lib.check(_lib.load().elimrec_blocksum_rows(_dev(G, "G"), _dev(active_rows, "active_rows", torch.int32),
                                                 _dev(seg_info, "seg_info", torch.int32), active_rows.numel(), d, M,
                                                 1 if slot_major else 0, _dev(H, "H"), _stream()), "blocksum_rows")


def copy_cols(src, dst):
    s, lds = _rowmajor(src, "src")
    t, ldt = _rowmajor(dst, "dst")
    assert src.shape == dst.shape
    _lib.check(_lib.load().elimrec_copy_cols(s, lds, t, ldt, src.shape[0], src.shape[1], _stream()), "copy_cols")
    return dst


def triplet_rows(users, pos, neg, U, rows, src=None, dst=None, I=None, err=None):
    """rows[3b + (0,1,2)] = users[b], U + pos[b], U + neg[b]; dst[slot] = src[rows[slot]] when src is given. With I and
    err (int32[1]): range-checked -- a bad index sets a bit of err and is replaced by 0."""
    B = users.numel()
    if err is not None:
        _lib.check(_lib.load().elimrec_triplet_rows_checked(_dev(users, "users", torch.int64), _dev(pos, "pos", torch.int64),
                                                            _dev(neg, "neg", torch.int64), B, U, int(I),
                                                            _dev(rows, "rows", torch.int32), _dev(err, "err", torch.int32),
                                                            _stream()), "triplet_rows_checked")
        return rows
    s, lds, t, ldt, cols = None, 0, None, 0, 0
    if src is not None:
        s, lds = _rowmajor(src, "src")
        t, ldt = _rowmajor(dst, "dst")
        cols = src.shape[1]
        assert dst.shape == (3 * B, cols)
    _lib.check(_lib.load().elimrec_triplet_rows(_dev(users, "users", torch.int64), _dev(pos, "pos", torch.int64),
                                                _dev(neg, "neg", torch.int64), B, U, _dev(rows, "rows", torch.int32),
                                                s, lds, cols, t, ldt, _stream()), "triplet_rows")
    return rows


def batch_plan(users, pos, neg, U, I, keys, active_rows, seg_info, slot_seg, workspace, err, pad_key, key_bitmap=None):
    """triplet_rows (range-checked) + segment_plan + padding of the active-row list in one launch (elimrec_batch_plan)."""
    B = users.numel()
    _lib.check(_lib.load().elimrec_batch_plan(_dev(users, "users", torch.int64), _dev(pos, "pos", torch.int64),
                                              _dev(neg, "neg", torch.int64), B, int(U), int(I), _dev(keys, "keys", torch.int32),
                                              _dev(active_rows, "active_rows", torch.int32),
                                              _dev(seg_info, "seg_info", torch.int32), _dev(slot_seg, "slot_seg", torch.int32),
                                              _dev(key_bitmap, "key_bitmap", torch.int32), int(pad_key),
                                              _dev(err, "err", torch.int32), _dev(workspace, "workspace", torch.uint8),
                                              workspace.numel(), _stream()), "batch_plan")
    return keys


def gather_rows(src, rows, dst, count=None):
    """dst[r] = src[rows[r]] for r < min(count, len(rows))."""
    s, lds = _rowmajor(src, "src")
    t, ldt = _rowmajor(dst, "dst")
    assert dst.shape == (rows.numel(), src.shape[1])
    _lib.check(_lib.load().elimrec_gather_rows(s, lds, _dev(rows, "rows", torch.int32), _dev(count, "count", torch.int32),
                                               rows.numel(), src.shape[1], t, ldt, _stream()), "gather_rows")
    return dst


def bpr_head(Y, U, I, users, pos, neg, d, block_weights, loss_rows, grad_rows=None, keys=None):
    y, ldy = _rowmajor(Y, "Y")
    nb = len(block_weights)
    w = (ctypes.c_float * nb)(*[float(x) for x in block_weights])
    B = users.numel()
    _lib.check(_lib.load().elimrec_bpr_head(y, ldy, U, I, _dev(users, "users", torch.int64), _dev(pos, "pos", torch.int64),
                                            _dev(neg, "neg", torch.int64), B, d, nb, w, _dev(loss_rows, "loss_rows"),
                                            _dev(grad_rows, "grad_rows"), _dev(keys, "keys", torch.int32), _stream()),
               "bpr_head")


def _bpr_head_rows(Y, slot_rows, d, block_weights, loss_rows, grad_rows, loss_out, ticket, pub, what):
    y, ldy = _rowmajor(Y, "Y")
    nb = len(block_weights)
    w = (ctypes.c_float * nb)(*[float(x) for x in block_weights])
    B = slot_rows.numel() // 3
    _lib.check(_lib.load().elimrec_bpr_head_rows(y, ldy, _dev(slot_rows, "slot_rows", torch.int32), B, d, nb, w,
                                                 _dev(loss_rows, "loss_rows"), _dev(grad_rows, "grad_rows"),
                                                 _dev(loss_out, "loss_out"), _dev(ticket, "ticket", torch.int32), pub, _stream()),
               what)


def bpr_head_rows(Y, slot_rows, d, block_weights, loss_rows, grad_rows=None):
    """bpr_head over a compact table: slot 3b+j of triplet b reads row slot_rows[3b+j] of Y."""
    _bpr_head_rows(Y, slot_rows, d, block_weights, loss_rows, grad_rows, None, None, None, "bpr_head_rows")


def bpr_head_rows_sum(Y, slot_rows, d, block_weights, loss_rows, grad_rows, loss_out, ticket):
    """bpr_head_rows + the fixed-order sum of its loss rows into loss_out (0-dim / 1-element fp32) in one launch; ticket: a
    zero-initialised int32 the kernel leaves at zero."""
    if loss_out is None or ticket is None:
        raise ValueError("bpr_head_rows_sum: loss_out and ticket are required")
    _bpr_head_rows(Y, slot_rows, d, block_weights, loss_rows, grad_rows, loss_out, ticket, None, "bpr_head_rows_sum")


def bpr_head_rows_sum_pub(Y, slot_rows, d, block_weights, loss_rows, grad_rows, loss_out, ticket, pub):
    """bpr_head_rows_sum whose summing workgroup also publishes the loss to the host (pub: LossPublisher.handle)."""
    if loss_out is None or ticket is None or not pub:
        raise ValueError("bpr_head_rows_sum_pub: loss_out, ticket and pub are required")
    _bpr_head_rows(Y, slot_rows, d, block_weights, loss_rows, grad_rows, loss_out, ticket, pub, "bpr_head_rows_sum_pub")


class LossPublisher(object):
    """elimrec_loss_pub_*: a ring of coherent host words the loss-summing launch of a step writes (sequence number, value) into,
    so that the caller's `loss.item()` (main.py:102 of the reference) waits for THAT launch and not for the whole step."""

    def __init__(self, n_slots=64):
        h = ctypes.c_void_p()
        _lib.check(_lib.load().elimrec_loss_pub_create(int(n_slots), ctypes.byref(h)), "loss_pub_create")
        self.handle = h
        self._val = ctypes.c_float()

    def issued(self):
        return int(_lib.load().elimrec_loss_pub_issued(self.handle))

    def wait(self, seq, timeout_s=60.0):
        """The loss launch `seq` published, or None when the ring has wrapped past it."""
        rc = _lib.load().elimrec_loss_pub_wait(self.handle, int(seq), float(timeout_s), ctypes.byref(self._val))
        if rc == 0:
            return float(self._val.value)
        if rc == 10002:            # ELIMREC_E_UNSUPPORTED: overwritten by a later step
            return None
        _lib.check(rc, "loss_pub_wait")

    def __del__(self):
        try:
            if self.handle:
                _lib.load().elimrec_loss_pub_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


def fixed_order_sum(x, out):
    _lib.check(_lib.load().elimrec_sum(_dev(x, "x"), x.numel(), _dev(out, "out"), _stream()), "sum")
    return out


def segment_reduce_workspace(n):
    return int(_lib.load().elimrec_segment_reduce_workspace(n))


def segment_plan_workspace(n):
    return int(_lib.load().elimrec_segment_plan_workspace(n))


def segment_plan_form(n, key_space):
    """The planner segment_plan / batch_plan (n = 3B, key_space = U + I) runs for these sizes: 0 = one workgroup, 1 = the
    device-wide bitmap plan, 2 = the radix sort (also under ELIMREC_PLAN_SORTED=1 wherever 1 would run). Host only."""
    return int(_lib.load().elimrec_segment_plan_form(int(n), int(key_space)))


def segment_plan(keys, split_key, key_space, active_rows, seg_info, slot_seg, workspace, key_bitmap=None):
    """Plan of a key list: active_rows (sorted unique keys), seg_info, slot_seg (segment of every slot); the member
    lists stay in `workspace` for segment_apply. key_bitmap (int32 words, >= key_space bits): bit k <=> k is active."""
    n = keys.numel()
    assert key_bitmap is None or key_bitmap.numel() * 32 >= key_space
    _lib.check(_lib.load().elimrec_segment_plan(_dev(keys, "keys", torch.int32), n, int(split_key), int(key_space),
                                                _dev(active_rows, "active_rows", torch.int32),
                                                _dev(seg_info, "seg_info", torch.int32),
                                                _dev(slot_seg, "slot_seg", torch.int32),
                                                _dev(key_bitmap, "key_bitmap", torch.int32),
                                                _dev(workspace, "workspace", torch.uint8), workspace.numel(), _stream()),
               "segment_plan")


def segment_apply(rows, seg_info, reduced, workspace, scale=None):
    n, ld = rows.shape
    assert rows.is_contiguous() and reduced.is_contiguous()
    _lib.check(_lib.load().elimrec_segment_apply(_dev(rows, "rows"), n, ld, _dev(seg_info, "seg_info", torch.int32),
                                                 _dev(scale, "scale"), _dev(reduced, "reduced"),
                                                 _dev(workspace, "workspace", torch.uint8), workspace.numel(), _stream()),
               "segment_apply")


def segment_reduce_rows(rows, keys, split_key, active_rows, reduced, seg_info, workspace, scale=None):
    n, ld = rows.shape
    assert rows.is_contiguous() and reduced.is_contiguous()
    _lib.check(_lib.load().elimrec_segment_reduce_rows(_dev(rows, "rows"), _dev(keys, "keys", torch.int32), n, ld,
                                                       int(split_key), _dev(active_rows, "active_rows", torch.int32),
                                                       _dev(reduced, "reduced"), _dev(scale, "scale"),
                                                       _dev(seg_info, "seg_info", torch.int32),
                                                       _dev(workspace, "workspace", torch.uint8), workspace.numel(),
                                                       _stream()), "segment_reduce_rows")


def head_bwd_input(dY, active_rows, seg_info, U, d, C, head_mblock, W_user, W_item, W_heads, gscale, G0,
                   scatter_cols=None, compact=None):
    """G0[node, 0:scatter_cols] (row stride G0.stride(0)) and/or compact[slot, 0:C] receive the input gradient."""
    S = len(W_heads)
    dy, lddy = _rowmajor(dY, "dY")
    mb = (ctypes.c_int * max(S, 1))(*head_mblock) if S else (ctypes.c_int * 1)(0)
    wp = (ctypes.c_void_p * max(S, 1))(*[_dev(w, "W_head") for w in W_heads]) if S else (ctypes.c_void_p * 1)(None)
    for w in list(W_heads) + [W_user, W_item]:
        assert w.is_contiguous()
    g0, ldg = (None, 0)
    if G0 is not None:
        g0, ldg = _rowmajor(G0, "G0")
    if scatter_cols is None:
        scatter_cols = C if G0 is not None else 0
    assert compact is None or (compact.is_contiguous() and compact.shape[1] == C and compact.shape[0] >= dY.shape[0])
    _lib.check(_lib.load().elimrec_head_bwd_input(dy, lddy, _dev(active_rows, "active_rows", torch.int32),
                                                  _dev(seg_info, "seg_info", torch.int32), dY.shape[0], U, d, C, S, mb,
                                                  _dev(W_user, "W_user"), _dev(W_item, "W_item"), wp, float(gscale),
                                                  g0, ldg, int(scatter_cols), _dev(compact, "compact"), _stream()),
               "head_bwd_input")


def segment_apply_head_bwd(rows, active_rows, seg_info, reduced, plan_workspace, U, d, C, head_mblock, W_user, W_item,
                           W_heads, compact, scale=None, pack_bwd=None, sources=None):
    """segment_apply + head_bwd_input(compact=...) in one launch; `reduced` receives dY. pack_bwd: the backward region of
    the fused head's packed weights (a view starting at head_pack_bwd_offset floats), if the forward left it behind.
    sources = (srcA, srcB) slab tables: the kernel also fills the adjoint sources at the active rows (one rank, recdim 64,
    packed weights: elimrec_head_bwd_sinks); ("split", send, world): the peers' [H | G] column slices."""
    n, ld = rows.shape
    S = len(W_heads)
    assert rows.is_contiguous() and reduced.is_contiguous() and reduced.shape[1] == ld and compact.is_contiguous()
    assert compact.shape[1] == C and compact.shape[0] >= n and reduced.shape[0] >= n
    mb = (ctypes.c_int * max(S, 1))(*head_mblock) if S else (ctypes.c_int * 1)(0)
    wp = (ctypes.c_void_p * max(S, 1))(*[_dev(w, "W_head") for w in W_heads]) if S else (ctypes.c_void_p * 1)(None)
    for w in list(W_heads) + [W_user, W_item]:
        assert w.is_contiguous()
    sinks = None
    if sources is not None and sources[0] == "split":          # ("split", send [W x n_max x 2*dl], W)
        _, send, world = sources
        assert pack_bwd is not None and send.is_contiguous() and send.shape == (world, send.shape[1], 2 * (d // world)) and send.shape[1] >= n
        sinks = _lib.HeadBwdSinks(d_split=_dev(send, "send"), n_max=send.shape[1], world=int(world))
    elif sources is not None:
        srcA, srcB = sources
        assert pack_bwd is not None and srcA.ns == srcB.ns and srcA.w == srcB.w and srcA.n == srcB.n
        sinks = _lib.HeadBwdSinks(d_SrcA=_dev(srcA.data, "srcA"), d_SrcB=_dev(srcB.data, "srcB"), N=srcA.n, ns=srcA.ns, w=srcA.w)
    _lib.check(_lib.load().elimrec_segment_apply_head_bwd(
        _dev(rows, "rows"), n, ld, _dev(active_rows, "active_rows", torch.int32), _dev(seg_info, "seg_info", torch.int32),
        _dev(scale, "scale"), _dev(reduced, "reduced"), _dev(plan_workspace, "plan_workspace", torch.uint8),
        plan_workspace.numel(), U, d, C, S, mb, _dev(W_user, "W_user"), _dev(W_item, "W_item"), wp,
        _dev(compact, "compact"), _dev(pack_bwd, "pack_bwd"), None if sinks is None else ctypes.byref(sinks), _stream()),
        "segment_apply_head_bwd")


def embed_grad(G, U, I, d, M, grad_user, grad_item):
    assert G.is_contiguous() and grad_user.is_contiguous() and grad_item.is_contiguous()
    _lib.check(_lib.load().elimrec_embed_grad(_dev(G, "G"), U, I, d, M, _dev(grad_user, "grad_user"),
                                              _dev(grad_item, "grad_item"), _stream()), "embed_grad")


def adam_step(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step):
    for t in (p, g, m, v):
        assert t.is_contiguous()
    _lib.check(_lib.load().elimrec_adam_step(_dev(p, "p"), _dev(g, "g"), _dev(m, "m"), _dev(v, "v"), p.numel(),
                                             float(lr), float(beta1), float(beta2), float(eps), float(weight_decay),
                                             int(step), _stream()), "adam_step")


def adam_step_raw(p_ptr, g_ptr, m_ptr, v_ptr, n, lr, beta1, beta2, eps, weight_decay, step):
    """Same kernel on raw device addresses (a span covering several adjacent tensors)."""
    _lib.check(_lib.load().elimrec_adam_step(p_ptr, g_ptr, m_ptr, v_ptr, int(n), float(lr), float(beta1), float(beta2),
                                             float(eps), float(weight_decay), int(step), _stream()), "adam_step")


def score_workspace(B, U, I, S, K, topk_only=False, d=None):
    """Bytes of score_topk's workspace. topk_only: the call will ask for top-K lists only (no score matrix). With the
    recdim `d` given the library itself decides whether that call takes the chunked form (no [B x I] block) and returns
    the layout it will use -- the full one for a recdim / K / scorer switch outside the chunked form's range -- with room
    for one chunk's bf16 piece planes (the default scorer of recdim 32 / 64, for lists and for score matrices alike)."""
    if d is not None:
        return int(_lib.load().elimrec_score_workspace_for(B, U, I, S, K, int(d), 0 if topk_only else 1))
    if topk_only:
        return int(_lib.load().elimrec_score_workspace_topk(B, U, I, S, K))
    return int(_lib.load().elimrec_score_workspace2(B, U, I, S, K))


def row_sqnorms(Y, d, n_blocks, out):
    y, ldy = _rowmajor(Y, "Y")
    assert out.is_contiguous() and out.shape == (Y.shape[0], n_blocks)
    _lib.check(_lib.load().elimrec_row_sqnorms(y, ldy, Y.shape[0], d, n_blocks, _dev(out, "out"), _stream()), "row_sqnorms")
    return out


FUSION_MODES = {"rubi": 0, "hm": 1, "sum": 2}
PREDICT_TYPES = {"TE": 1, "TIE": 2}   # anything else -> 0 ("normal", models/EliMRec.py:113)


TIE_ORDERS = {"id": 0, "reference": 1}   # among equal scores: lowest item id first / the reference's heap order (evaluate.h:26-33)


def score_topk(Y, U, I, users, d, S, head_mask, fusion_mode, predict_type, workspace, scores=None, K=0,
               topk_idx=None, topk_val=None, train_ptr=None, train_items=None, sqnorm=None, tie_order="id"):
    y, ldy = _rowmajor(Y, "Y")
    B = users.numel()
    sp, lds = (None, 0)
    if scores is not None:
        sp, lds = _rowmajor(scores, "scores")
    _lib.check(_lib.load().elimrec_score_topk_ordered(y, ldy, U, I, _dev(users, "users", torch.int64), B, d, S, int(head_mask),
                                                      FUSION_MODES[fusion_mode], PREDICT_TYPES.get(predict_type, 0),
                                                      _dev(sqnorm, "sqnorm"), _dev(train_ptr, "train_ptr", torch.int64),
                                                      _dev(train_items, "train_items", torch.int32), sp, lds, int(K),
                                                      _dev(topk_idx, "topk_idx", torch.int32), _dev(topk_val, "topk_val"),
                                                      _dev(workspace, "workspace", torch.uint8), workspace.numel(),
                                                      TIE_ORDERS[tie_order], _stream()),
               "score_topk")


def topk_reference_order(scores, K, out_idx, out_val=None):
    """Rows of masked scores on the device -> the reference's top-K lists (std::partial_sort_copy's order, evaluate.h:26-33)."""
    sp, lds = _rowmajor(scores, "scores")
    B, I = scores.shape
    assert out_idx.is_contiguous() and out_idx.shape == (B, K) and (out_val is None or (out_val.is_contiguous() and out_val.shape == (B, K)))
    _lib.check(_lib.load().elimrec_topk_reference_order_device(sp, B, I, lds, int(K), _dev(out_idx, "out_idx", torch.int32),
                                                               _dev(out_val, "out_val"), _stream()), "topk_reference_order_device")
    return out_idx, out_val


def score_range_violations(reset=True):
    """Waves of the scorer launches since the last reset that saw a score outside their launch's range invariant (a host
    synchronisation with the current stream)."""
    n = ctypes.c_int64(0)
    _lib.check(_lib.load().elimrec_score_range_violations(ctypes.byref(n), 1 if reset else 0, _stream()), "score_range_violations")
    return int(n.value)


def score_range_check(topk_val, topk_idx, predict_type, fusion_mode, row_mean=None):
    """The range check every scoring call ends with, over lists the caller holds (counted into score_range_violations)."""
    B, K = topk_val.shape
    assert topk_val.is_contiguous() and topk_idx.is_contiguous() and topk_idx.shape == (B, K)
    _lib.check(_lib.load().elimrec_score_range_check(_dev(topk_val, "topk_val"), _dev(topk_idx, "topk_idx", torch.int32), B, K,
                                                     PREDICT_TYPES.get(predict_type, 0), FUSION_MODES[fusion_mode],
                                                     _dev(row_mean, "row_mean"), _stream()), "score_range_check")


def score_topk_shard(Y, U, I, users, d, S, head_mask, fusion_mode, predict_type, workspace, phase, row_sum, I_total, id_offset,
                     scores=None, K=0, topk_idx=None, topk_val=None, train_ptr=None, train_items=None, sqnorm=None):
    """elimrec_score_topk_shard: Y = [all user rows ; this shard's I item rows]. phase 1 -> row_sum [B] (TIE), phase 2 ->
    scores [B x I] and / or top-K (catalogue ids) given the all-reduced row_sum."""
    y, ldy = _rowmajor(Y, "Y")
    B = users.numel()
    sp, lds = (None, 0)
    if scores is not None:
        sp, lds = _rowmajor(scores, "scores")
    _lib.check(_lib.load().elimrec_score_topk_shard(y, ldy, U, I, _dev(users, "users", torch.int64), B, d, S, int(head_mask),
                                                    FUSION_MODES[fusion_mode], PREDICT_TYPES.get(predict_type, 0),
                                                    _dev(sqnorm, "sqnorm"), _dev(train_ptr, "train_ptr", torch.int64),
                                                    _dev(train_items, "train_items", torch.int32), sp, lds, int(K),
                                                    _dev(topk_idx, "topk_idx", torch.int32), _dev(topk_val, "topk_val"),
                                                    _dev(workspace, "workspace", torch.uint8), workspace.numel(), int(phase),
                                                    _dev(row_sum, "row_sum"), int(I_total), int(id_offset), _stream()),
               "score_topk_shard")


def topk_merge(cand_val, cand_idx, K, out_idx, out_val=None):
    """[B x n] candidate (value, id) lists -> the K best per row by (score desc, id asc)."""
    B, n = cand_val.shape
    assert cand_val.is_contiguous() and cand_idx.is_contiguous() and cand_idx.shape == (B, n) and out_idx.shape == (B, K)
    _lib.check(_lib.load().elimrec_topk_merge(_dev(cand_val, "cand_val"), _dev(cand_idx, "cand_idx", torch.int32), B, n, int(K),
                                              _dev(out_idx, "out_idx", torch.int32), _dev(out_val, "out_val"), _stream()), "topk_merge")


def rank_metrics(topk_idx, truth_ptr, truth_items, metric_ids, out):
    B, K = topk_idx.shape
    ids = (ctypes.c_int * len(metric_ids))(*metric_ids)
    assert topk_idx.is_contiguous() and out.is_contiguous()
    _lib.check(_lib.load().elimrec_rank_metrics(_dev(topk_idx, "topk_idx", torch.int32), B, K,
                                                _dev(truth_ptr, "truth_ptr", torch.int64),
                                                _dev(truth_items, "truth_items", torch.int32), ids, len(metric_ids),
                                                _dev(out, "out"), _stream()), "rank_metrics")
    return out


class CandidateScoringError(ValueError):
    """A candidate-list (sampled-negative) evaluation or scoring call this package does not run: item-sharded / lean tables,
    or a top-K beyond the shortest candidate list."""


class GroupIndex(object):
    """Groups of rows as CSR (group_ptr [G + 1], group_rows: row indices into a block of n_rows rows), CHECKED ON THE HOST --
    ptr[0] = 0, ascending, ptr[G] = len(group_rows), every index in [0, n_rows) -- and then resident on `device`:
    group_metric_means takes it as is, call after call, and no unchecked index ever reaches a kernel."""

    def __init__(self, group_ptr, group_rows, n_rows, device):
        ptr, rows = _checked_csr(group_ptr, group_rows, None, n_rows, "GroupIndex",
                                 ("group_ptr", "group_rows", "G", "row indices span [%d, %d], the block has %d rows"))
        self.n_rows, self.n_groups, self.n_listed = int(n_rows), int(ptr.size - 1), int(rows.size)
        self.sizes = np.diff(ptr)
        self.ptr = torch.from_numpy(ptr).to(device)
        self.rows = _resident_ids(rows, device)


def _host(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _checked_ids(ids, bound, who, name, span):
    """Host array of ids (flat): an integer dtype, every id in [0, bound). span: the IndexError's words, %% (min, max, bound)."""
    ids = _host(ids).reshape(-1)
    _integer_ids(ids, who, name)
    _ids_in_range(ids, bound, who, span)
    return ids


def _integer_ids(ids, who, name):
    if ids.size and not np.issubdtype(ids.dtype, np.integer):
        raise TypeError("elimrec_amd.ops.%s: %s must hold integers, got %s" % (who, name, ids.dtype))


def _ids_in_range(ids, bound, who, span):
    if ids.size and (int(ids.min()) < 0 or int(ids.max()) >= int(bound)):
        raise IndexError("elimrec_amd.ops.%s: " % who + span % (int(ids.min()), int(ids.max()), int(bound)))


def _checked_csr(ptr, ids, n_lists, bound, who, names):
    """The host checks of a CSR of ids, in this order: entry count of ptr (n_lists + 1; n_lists = None: any number of lists >= 1),
    integer ids, ptr ascending from 0 to len(ids), every id in [0, bound) (bound = None: the ids' range is left to the kernel). names = (ptr's name, ids' name, the letter of the list
    count, the range error's words). -> (ptr int64, ids) as flat host arrays."""
    ptr_name, ids_name, letter, span = names
    p = np.ascontiguousarray(_host(ptr), dtype=np.int64).reshape(-1)
    ids = _host(ids).reshape(-1)
    if n_lists is None:
        if p.size < 2:
            raise ValueError("elimrec_amd.ops.%s: %s needs %s + 1 >= 2 entries" % (who, ptr_name, letter))
    elif p.size != int(n_lists) + 1:
        raise ValueError("elimrec_amd.ops.%s: %s needs %s + 1 = %d entries, got %d" % (who, ptr_name, letter, int(n_lists) + 1, p.size))
    _integer_ids(ids, who, ids_name)
    if p[0] != 0 or p[-1] != ids.size or (np.diff(p) < 0).any():
        raise ValueError("elimrec_amd.ops.%s: %s must ascend from 0 to len(%s) = %d" % (who, ptr_name, ids_name, ids.size))
    if bound is not None:
        _ids_in_range(ids, bound, who, span)
    return p, ids


def _resident_ids(ids, device):
    """Checked ids as an int32 device tensor (never empty: the kernels read nothing of it when there are no ids, the binding still
    wants a device tensor)."""
    return torch.from_numpy(np.ascontiguousarray(ids if ids.size else np.zeros(1), dtype=np.int32)).to(device)


def ragged(lists, dtype=np.int64, check=None, cast=None):
    """A list of lists (or of arrays) of ids as CSR on the host: (ptr int64 [n + 1], flat ids of `dtype` in list order, lens int64 [n]). cast:
    applied to every id before it is stored (int: a Python integer beyond `dtype` raises OverflowError instead of wrapping).
    check = (bound, message): every id must lie in [0, bound), else IndexError(message); None: nothing is checked."""
    lens = np.fromiter((len(x) for x in lists), dtype=np.int64, count=len(lists))
    ptr = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum(lens, out=ptr[1:])
    if cast is None and len(lists) and all(isinstance(x, np.ndarray) for x in lists):
        flat = np.concatenate(lists).astype(dtype)
    else:
        ids = (i for x in lists for i in x) if cast is None else (cast(i) for x in lists for i in x)
        flat = np.fromiter(ids, dtype=dtype, count=int(ptr[-1]))
    if check is not None and flat.size and (flat.min() < 0 or flat.max() >= check[0]):
        raise IndexError(check[1])
    return ptr, flat, lens


def ragged_padded(flat, lens, width=None, dtype=np.int32):
    """ragged()'s ids as [n x width] rows of `dtype` (width default: the longest list), -1 beyond each list's length."""
    width = (int(lens.max()) if lens.size else 0) if width is None else int(width)
    out = np.full((lens.size, width), -1, dtype=dtype)
    out[np.arange(width)[None, :] < lens[:, None]] = flat
    return out


def _group_index_for(who, rows, group_ptr, group_rows):
    """group_metric_means' reading of its group arguments: a GroupIndex (checked once) as is, raw arrays checked on the host now."""
    n = rows.shape[0]
    if isinstance(group_ptr, GroupIndex):
        index = group_ptr
        if group_rows is not None and group_rows is not index.rows:
            raise ValueError("elimrec_amd.ops.%s: a GroupIndex carries its own rows (pass group_rows=None)" % who)
        if index.n_rows > n or index.ptr.device != rows.device:
            raise IndexError("elimrec_amd.ops.%s: the GroupIndex was checked for %d rows on %s, the block has %d on %s"
                             % (who, index.n_rows, index.ptr.device, n, rows.device))
        return index
    return GroupIndex(group_ptr, group_rows, n, rows.device)


def group_metric_means(rows, group_ptr, group_rows, out, workspace=None):
    """out [G x C] (float32, contiguous) = per group the column means of rows [n x C] (a column slice of a wider block is
    fine): float64 sums in listed order, divided in float64, rounded once (elimrec_group_metric_means). group_ptr / group_rows:
    the groups as CSR, host arrays or tensors -- checked on the host at every call (device tensors are copied back for it: a
    synchronisation) -- or group_ptr = a GroupIndex (group_rows = None), checked once when it was built. workspace: uint8 device
    tensor of at least elimrec_group_metric_means_workspace bytes (default: allocated here)."""
    lib = _lib.load()
    rp, ld = _rowmajor(rows, "rows")
    n, C = rows.shape
    index = _group_index_for("group_metric_means", rows, group_ptr, group_rows)
    G = index.n_groups
    if not (isinstance(out, torch.Tensor) and out.is_contiguous() and tuple(out.shape) == (G, C)):
        raise ValueError("elimrec_amd.ops.group_metric_means: out must be a contiguous [%d x %d] tensor" % (G, C))
    if workspace is None:
        workspace = torch.empty(max(1, int(lib.elimrec_group_metric_means_workspace(index.n_listed, C, G))), dtype=torch.uint8,
                                device=rows.device)
    _lib.check(lib.elimrec_group_metric_means(rp, n, C, ld, _dev(index.ptr, "group_ptr", torch.int64),
                                              _dev(index.rows, "group_rows", torch.int32), index.n_listed, G, _dev(out, "out"),
                                              _dev(workspace, "workspace", torch.uint8), workspace.numel(), _stream()),
               "group_metric_means")
    return out


def bootstrap_rows_in_lds(n_g, C):
    """Which form bootstrap_means takes for a group of n_g listed rows in a call (or column slice) of C columns (host arithmetic
    only): True = the group's values are staged once per workgroup into LDS, False = every draw gathers from global memory. Both
    forms give the same bits. ValueError outside 0 <= n_g < 2^31, 1 <= C <= BOOTSTRAP_MAX_COLUMNS."""
    form = int(_lib.load().elimrec_bootstrap_rows_in_lds(int(n_g), int(C)))
    if form < 0:
        raise ValueError("elimrec_amd.ops.bootstrap_rows_in_lds: 0 <= n_g < 2^31 and 1 <= C <= %d, got n_g %d, C %d"
                         % (_lib.load().elimrec_bootstrap_max_columns(), n_g, C))
    return bool(form)


def bootstrap_means(rows, group_ptr, group_rows, R, seed, out=None, rows_b=None, lds=True):
    """elimrec_bootstrap_means: out float64 [R x G x C] on the rows' device <- R bootstrap replicates of every group's column means
    of rows [n x C] float32 (unit column stride; a column slice of a wider block is fine) -- with rows_b (same shape, strides,
    device) of the paired differences rows_b - rows, taken exactly in float64. Replicate r of group g draws n_g of the group's
    listed rows with replacement: draw t is position (uint64(word) * n_g) >> 32, word = output t & 3 of Philox4x32-10 keyed by the
    64-bit seed at counter (t >> 2, r, g, 0x626F6F74); one draw takes the whole row, so the columns share a resample. NaN for an
    empty group. group_ptr / group_rows: the groups as group_metric_means takes them (host arrays or tensors, checked on the host at
    every call, or a GroupIndex with group_rows = None). A block wider than BOOTSTRAP_MAX_COLUMNS goes through in column slices:
    the same bits, the resample does not depend on the column. lds = False keeps every group on the global-memory form (the
    default takes the LDS form where bootstrap_rows_in_lds says so; both give the same bits). No workspace, no atomics: a
    replicate's bits depend on the seed, r, g, the group's rows in order and the values alone (csrc/bootstrap.hip)."""
    who = "bootstrap_means"
    for t, name in ((rows, "rows"),) + (((rows_b, "rows_b"),) if rows_b is not None else ()):
        if not isinstance(t, torch.Tensor):
            raise RuntimeError("elimrec_amd.ops: '%s' must be a HIP device tensor (the hot path has no CPU implementation)" % name)
        if t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
            raise ValueError("elimrec_amd.ops.%s: %s must be 2-D with unit column stride" % (who, name))
        if t.dtype != torch.float32:
            raise TypeError("elimrec_amd.ops.%s: %s must be float32, got %s" % (who, name, t.dtype))
    n, C = rows.shape
    if rows_b is not None and (rows_b.shape != rows.shape or rows_b.stride(0) != rows.stride(0) or rows_b.device != rows.device):
        raise ValueError("elimrec_amd.ops.%s: rows_b must have the shape, row stride and device of rows" % who)
    if isinstance(R, bool) or not isinstance(R, (int, np.integer)) or not 1 <= R < 2 ** 31:
        raise ValueError("elimrec_amd.ops.%s: R must be an integer in [1, 2^31), got %r" % (who, R))
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= seed < 2 ** 64:
        raise ValueError("elimrec_amd.ops.%s: seed must be an integer in [0, 2^64), got %r" % (who, seed))
    if C < 1 or n >= 2 ** 31:
        raise ValueError("elimrec_amd.ops.%s: rows needs at least one column and fewer than 2^31 rows, got [%d x %d]" % (who, n, C))
    index = _group_index_for(who, rows, group_ptr, group_rows)
    G, R = index.n_groups, int(R)
    if out is None:
        if not rows.is_cuda:
            raise RuntimeError("elimrec_amd.ops: 'rows' must be a HIP device tensor (the hot path has no CPU implementation)")
        out = torch.empty(R, G, C, dtype=torch.float64, device=rows.device)
    elif not (isinstance(out, torch.Tensor) and out.is_contiguous() and tuple(out.shape) == (R, G, C) and out.dtype == torch.float64
              and out.device == rows.device):
        raise ValueError("elimrec_amd.ops.%s: out must be a contiguous float64 [%d x %d x %d] tensor on the rows' device" % (who, R, G, C))
    lib = _lib.load()
    rp, bp, op = _dev(rows, "rows"), _dev(rows_b, "rows_b"), _dev(out, "out", torch.float64)
    ld = int(rows.stride(0)) if n > 1 else C
    if ld < C:
        raise ValueError("elimrec_amd.ops.%s: rows must be 2-D with unit column stride and rows that do not overlap" % who)
    step = int(lib.elimrec_bootstrap_max_columns())
    for c0 in range(0, C, step):
        _lib.check(lib.elimrec_bootstrap_means(rp + 4 * c0, bp + 4 * c0 if bp is not None else None, n, min(step, C - c0), ld,
                                               _dev(index.ptr, "group_ptr", torch.int64), _dev(index.rows, "group_rows", torch.int32),
                                               index.n_listed, G, R, int(seed), op + 8 * c0, C, 1 if lds else 0, _stream()), who)
    return out


class TargetIndex(object):
    """Target items per score row as CSR (ptr [B + 1], items: item ids of an I-item catalogue), CHECKED ON THE HOST -- B + 1
    entries, ptr[0] = 0, ascending, ptr[B] = len(items), every id in [0, I) -- and then resident on `device`: rank_targets takes
    it as is, call after call, and no unchecked id ever reaches a kernel (the counterpart of GroupIndex)."""

    def __init__(self, ptr, items, B, I, device):
        p, it = _checked_csr(ptr, items, B, I, "TargetIndex", ("ptr", "items", "B", "item ids span [%d, %d], the catalogue has %d items"))
        self.n_rows, self.n_items, self.n_targets = int(B), int(I), int(it.size)
        self.sizes = np.diff(p)
        self.ptr = torch.from_numpy(p).to(device)
        self.items = _resident_ids(it, device)


def rank_targets(scores, tgt_ptr, tgt_items, out):
    """elimrec_rank_targets: out int32 [>= n_targets] <- the 0-based position of every listed target in its row's full ranking by
    (score descending, id ascending): #{j: scores[b, j] > s or (scores[b, j] == s and j < t)}; -1 for a target at -inf (masked).
    scores [B x I] float32, unit column stride (a padded block's columns beyond I are not read). tgt_ptr / tgt_items: the lists as
    CSR, host arrays or tensors -- checked on the host at every call (a synchronisation for device tensors) -- or tgt_ptr = a
    TargetIndex (tgt_items = None), checked once. Entries of out beyond n_targets are left alone."""
    sp, lds = _rowmajor(scores, "scores")
    B, I = scores.shape
    if isinstance(tgt_ptr, TargetIndex):
        index = tgt_ptr
        if tgt_items is not None and tgt_items is not index.items:
            raise ValueError("elimrec_amd.ops.rank_targets: a TargetIndex carries its own items (pass tgt_items=None)")
        if index.n_rows != B or index.n_items > I or index.ptr.device != scores.device:
            raise IndexError("elimrec_amd.ops.rank_targets: the TargetIndex was checked for %d rows of %d items on %s, the block is "
                             "[%d x %d] on %s" % (index.n_rows, index.n_items, index.ptr.device, B, I, scores.device))
    else:
        index = TargetIndex(tgt_ptr, tgt_items, B, I, scores.device)
    if not (isinstance(out, torch.Tensor) and out.dim() == 1 and out.is_contiguous() and out.numel() >= index.n_targets):
        raise ValueError("elimrec_amd.ops.rank_targets: out must be a contiguous 1-D tensor of at least %d entries" % index.n_targets)
    _lib.check(_lib.load().elimrec_rank_targets(sp, B, I, lds, _dev(index.ptr, "tgt_ptr", torch.int64),
                                                _dev(index.items, "tgt_items", torch.int32), index.n_targets,
                                                _dev(out, "out", torch.int32), _stream()), "rank_targets")
    return out


def rank_values(scores, val_ptr, vals, out, skip=None):
    """elimrec_rank_values: out int32 [>= n_vals] <- where each listed value would land in its row's full ranking,
    #{j != skip: scores[b, j] >= v}: a new item goes behind every catalogue item of equal score (its id is the larger one); -1 for
    a value that is not finite. scores [B x I] float32, unit column stride, masked entries -inf (rank_targets' block; columns
    beyond I of a padded block are not read). val_ptr int64 [B + 1] / vals float32: the values as CSR -- val_ptr a host array or a
    tensor, checked on the host at every call (a synchronisation for a device tensor), vals a contiguous device tensor. skip
    (optional): one column per value that is not counted -- the item's own catalogue entry -- or -1; a host array or a tensor,
    checked on the host: a column outside [0, I) is an IndexError. Entries of out beyond n_vals are left alone. O(I log Q) per row
    (csrc/coldstart.hip): RANK_VALUES_PER_PASS values are sorted per pass, RANK_VALUES_SEGMENT columns go to one workgroup."""
    sp, lds = _rowmajor(scores, "scores")
    B, I = scores.shape
    vp = _dev(vals, "vals")
    if vals.dim() != 1 or not vals.is_contiguous() or vals.device != scores.device:
        raise ValueError("elimrec_amd.ops.rank_values: vals must be a contiguous 1-D tensor on the block's device")
    n = int(vals.numel())
    p = np.ascontiguousarray(_host(val_ptr), dtype=np.int64).reshape(-1)
    if p.size != B + 1:
        raise ValueError("elimrec_amd.ops.rank_values: val_ptr needs B + 1 = %d entries, got %d" % (B + 1, p.size))
    if p[0] != 0 or p[-1] != n or (np.diff(p) < 0).any():
        raise ValueError("elimrec_amd.ops.rank_values: val_ptr must ascend from 0 to len(vals) = %d" % n)
    sk = None
    if skip is not None:
        s = _host(skip).reshape(-1)
        _integer_ids(s, "rank_values", "skip")
        if s.size != n:
            raise ValueError("elimrec_amd.ops.rank_values: skip needs one entry per value (%d), got %d" % (n, s.size))
        if s.size and (int(s.min()) < -1 or int(s.max()) >= I):
            raise IndexError("elimrec_amd.ops.rank_values: skipped columns span [%d, %d], the block has %d columns (-1: none)"
                             % (int(s.min()), int(s.max()), I))
        sk = skip.contiguous() if isinstance(skip, torch.Tensor) and skip.is_cuda and skip.dtype == torch.int32 else _resident_ids(s, scores.device)
    if not (isinstance(out, torch.Tensor) and out.dim() == 1 and out.is_contiguous() and out.numel() >= n):
        raise ValueError("elimrec_amd.ops.rank_values: out must be a contiguous 1-D tensor of at least %d entries" % n)
    ptr = val_ptr.contiguous() if isinstance(val_ptr, torch.Tensor) and val_ptr.is_cuda and val_ptr.dtype == torch.int64 \
        else torch.from_numpy(p).to(scores.device)
    _lib.check(_lib.load().elimrec_rank_values(sp, B, I, lds, _dev(ptr, "val_ptr", torch.int64), vp, _dev(sk, "skip", torch.int32), n,
                                               _dev(out, "out", torch.int32), _stream()), "rank_values")
    return out


FOLDIN_MAX_COLUMNS = 1280               # the widest table segment_row_sum takes (csrc/foldin.hip), known without the library


def segment_row_sum(table, ptr, rows, weights, out, row_offset=0):
    """elimrec_segment_row_sum: out float32 [Q x C] <- per list the weighted sum of table rows,
    out[q] = sum_j weights[j] * table[row_offset + rows[j]] over j in [ptr[q], ptr[q + 1]) -- the fold-in of a new user from its
    history. Every product and every sum in float64, rounded to float32 once; an empty list gives zeros. table float32 [n x C],
    unit column stride, a row stride that is a multiple of 4 floats, 16-byte aligned, C % 4 == 0, 4 <= C <= FOLDIN_MAX_COLUMNS.
    ptr int64 [Q + 1] / rows int32 / weights float32 (as long as rows): host arrays or tensors, checked on the host at every call
    (a synchronisation for device tensors) -- ptr ascends from 0 to len(rows) (ValueError), every id in [0, n - row_offset)
    (IndexError), every weight finite (ValueError) -- before anything is launched; Q = 0 launches nothing. One workgroup per list,
    chunks of FOLDIN_CHUNK entries dealt to its four waves in turn, no atomics and no workspace: a list's bits depend on its own
    entries, C and the table alone, not on Q or on the other lists of the call (csrc/foldin.hip)."""
    who = "segment_row_sum"
    tp, ld = _rowmajor(table, "table")
    n, C = table.shape
    if C % 4 or not 4 <= C <= FOLDIN_MAX_COLUMNS:
        raise ValueError("elimrec_amd.ops.%s: C must be a multiple of 4 in [4, %d], got %d" % (who, FOLDIN_MAX_COLUMNS, C))
    if ld % 4 or tp % 16:
        raise ValueError("elimrec_amd.ops.%s: table needs a row stride that is a multiple of 4 floats and a 16-byte aligned base" % who)
    row_offset = int(row_offset)
    if not 0 <= row_offset <= n:
        raise IndexError("elimrec_amd.ops.%s: row_offset %d outside [0, %d]" % (who, row_offset, n))
    if not (isinstance(out, torch.Tensor) and out.dim() == 2 and out.shape[1] == C and (out.shape[0] == 0 or out.stride(1) == 1)
            and out.device == table.device):
        raise ValueError("elimrec_amd.ops.%s: out must be a [Q x %d] tensor with unit column stride on the table's device" % (who, C))
    Q = int(out.shape[0])
    p, ids = _checked_csr(ptr, rows, Q, n - row_offset, who,
                          ("ptr", "rows", "Q", "row ids span [%d, %d], the table holds %d rows behind row_offset"))
    E = int(ids.size)
    w = _host(weights).reshape(-1)
    if w.size != E:
        raise ValueError("elimrec_amd.ops.%s: weights needs one entry per row id (%d), got %d" % (who, E, w.size))
    if E and (w.dtype.kind != "f" or not np.isfinite(w).all()):
        raise ValueError("elimrec_amd.ops.%s: weights must be finite floats" % who)
    if Q == 0:
        return out
    op, ldo = _rowmajor(out, "out")
    if (Q > 1 and ldo % 4) or op % 16:
        raise ValueError("elimrec_amd.ops.%s: out needs a row stride that is a multiple of 4 floats and a 16-byte aligned base" % who)
    dev = table.device
    keep = lambda x, dt: isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == dt and x.device == dev and x.dim() == 1 and x.is_contiguous()
    ptr_t = ptr if keep(ptr, torch.int64) else torch.from_numpy(p).to(dev)
    rows_t = rows if keep(rows, torch.int32) and E else _resident_ids(ids, dev)
    w_t = weights if keep(weights, torch.float32) and E else torch.from_numpy(np.ascontiguousarray(w if E else np.zeros(1), dtype=np.float32)).to(dev)
    _lib.check(_lib.load().elimrec_segment_row_sum(tp, n, C, ld, row_offset, _dev(ptr_t, "ptr", torch.int64), _dev(rows_t, "rows", torch.int32),
                                                   _dev(w_t, "weights"), Q, E, op, max(ldo, C) if Q > 1 else C, _stream()), who)
    return out


RANK_PAIR_COLUMNS = ("rank", "rr", "pct")
RANK_USER_COLUMNS = ("auc", "mrr_full", "first_rank")


def rank_pair_columns(ks):
    """Column names of rank_pair_rows' output: rank, rr, pct, then hit@K for every K of ks."""
    return RANK_PAIR_COLUMNS + tuple("hit@%d" % int(k) for k in ks)


def rank_pair_rows(rank, n_cand, ks, out):
    """elimrec_rank_pair_rows: out [P x (3 + len(ks))] (float32, contiguous) = per pair rank, rr = 1 / (rank + 1),
    pct = rank / (n_cand - 1) (0 when n_cand <= 1), hit@K = (rank < K) for each K of ks (at most 16); a NaN row where rank < 0.
    rank, n_cand: int32 [P]."""
    P = rank.numel()
    ks = [int(k) for k in ks]
    if n_cand.numel() != P or not rank.is_contiguous() or not n_cand.is_contiguous():
        raise ValueError("elimrec_amd.ops.rank_pair_rows: rank and n_cand must be contiguous with one entry per pair")
    if not (isinstance(out, torch.Tensor) and out.is_contiguous() and tuple(out.shape) == (P, 3 + len(ks))):
        raise ValueError("elimrec_amd.ops.rank_pair_rows: out must be a contiguous [%d x %d] tensor" % (P, 3 + len(ks)))
    _lib.check(_lib.load().elimrec_rank_pair_rows(_dev(rank, "rank", torch.int32), _dev(n_cand, "n_cand", torch.int32), P,
                                                  (ctypes.c_int * max(1, len(ks)))(*ks), len(ks), _dev(out, "out"), _stream()),
               "rank_pair_rows")
    return out


def rank_user_rows(rank, tgt_ptr, n_cand, out):
    """elimrec_rank_user_rows: out [B x 3] (float32, contiguous) = per user auc, mrr_full, first_rank over its targets with
    rank >= 0 (NaN when it has none, or no candidate besides them). rank int32 [n_targets]; tgt_ptr: int64 [B + 1] device tensor
    or a TargetIndex; n_cand int32 [B]: the user's candidates (the catalogue without its masked items)."""
    if isinstance(tgt_ptr, TargetIndex):
        tgt_ptr = tgt_ptr.ptr
    B = n_cand.numel()
    if tgt_ptr.numel() != B + 1 or not rank.is_contiguous() or not n_cand.is_contiguous() or not tgt_ptr.is_contiguous():
        raise ValueError("elimrec_amd.ops.rank_user_rows: tgt_ptr needs B + 1 entries for the %d users of n_cand" % B)
    if not (isinstance(out, torch.Tensor) and out.is_contiguous() and tuple(out.shape) == (B, 3)):
        raise ValueError("elimrec_amd.ops.rank_user_rows: out must be a contiguous [%d x 3] tensor" % B)
    _lib.check(_lib.load().elimrec_rank_user_rows(_dev(rank, "rank", torch.int32), _dev(tgt_ptr, "tgt_ptr", torch.int64),
                                                  rank.numel(), _dev(n_cand, "n_cand", torch.int32), B, _dev(out, "out"),
                                                  _stream()), "rank_user_rows")
    return out


def __getattr__(name):
    if name == "GROUP_MEAN_CHUNK":       # listed rows per partial sum of group_metric_means (a compile-time constant of the library)
        return int(_lib.load().elimrec_group_metric_means_chunk())
    if name == "RANK_SEGMENT":           # columns of a score row one workgroup of rank_targets counts
        return int(_lib.load().elimrec_rank_segment())
    if name == "RANK_TARGETS_PER_PASS":  # targets rank_targets stages per pass over a segment
        return int(_lib.load().elimrec_rank_targets_per_pass())
    if name == "RANK_VALUES_SEGMENT":    # columns of a score row one workgroup of rank_values streams
        return int(_lib.load().elimrec_rank_values_segment())
    if name == "RANK_VALUES_PER_PASS":   # values rank_values sorts in LDS per pass over a segment
        return int(_lib.load().elimrec_rank_values_per_pass())
    if name == "FOLDIN_CHUNK":           # entries of a list one wave of segment_row_sum takes at a time
        return int(_lib.load().elimrec_segment_row_sum_chunk())
    if name == "KNN_CHUNK":              # candidate rows one workgroup of cosine_topk streams
        return int(_lib.load().elimrec_cosine_topk_chunk())
    if name == "KNN_TILE":               # query rows one workgroup of cosine_topk holds (16 when K > 64)
        return int(_lib.load().elimrec_cosine_topk_tile())
    if name == "AUDIENCE_CHUNK":         # user rows one workgroup of audience_topk streams
        return int(_lib.load().elimrec_audience_topk_chunk())
    if name == "AUDIENCE_TILE":          # query items one workgroup of audience_topk holds (16 when K > 64 or d is not 32 / 64)
        return int(_lib.load().elimrec_audience_topk_tile())
    if name == "LIST_SMALL_K":          # lists up to this K take one wave of list_pair_cosine, longer ones four
        return int(_lib.load().elimrec_list_pair_cosine_small_k())
    if name == "HISTORY_MAX_TOP":        # entries of a history history_support names per target
        return int(_lib.load().elimrec_history_max_top())
    if name == "BOOTSTRAP_MAX_COLUMNS":  # columns one bootstrap_means launch takes (wider blocks go through in slices)
        return int(_lib.load().elimrec_bootstrap_max_columns())
    if name == "BOOTSTRAP_TILE":         # replicates one workgroup of bootstrap_means serves
        return int(_lib.load().elimrec_bootstrap_replicate_tile())
    if name == "MMR_MAX_POOL":           # positions of a pool mmr_rerank takes (one thread each)
        return int(_lib.load().elimrec_mmr_max_pool())
    if name == "CALIBRATE_MAX_CLASSES":  # item classes calibrate_rerank / class_shares / list_calibration take (one lane each)
        return int(_lib.load().elimrec_calibrate_max_classes())
    if name == "KMEANS_MAX_CLUSTERS":    # centroids kmeans_assign / kmeans_update take
        return int(_lib.load().elimrec_kmeans_max_clusters())
    if name == "KMEANS_SEGMENT":         # consecutive table rows per partial sum of kmeans_update
        return int(_lib.load().elimrec_kmeans_segment())
    if name == "GEOMETRY_TILE":          # list positions one workgroup of uniformity_sum holds as queries
        return int(_lib.load().elimrec_geometry_tile())
    if name == "GEOMETRY_CHUNK":         # list positions one workgroup of uniformity_sum streams as candidates
        return int(_lib.load().elimrec_geometry_chunk())
    if name == "GEOMETRY_SEGMENT":       # consecutive list positions per partial sum of row_gram
        return int(_lib.load().elimrec_geometry_segment())
    if name == "COOCCUR_SLOTS":          # (key, count) pairs of the LDS form's table of cooccur_topk
        return int(_lib.load().elimrec_cooccur_slots())
    if name == "COOCCUR_GROUPS":         # workgroups (and counter rows) of cooccur_topk's dense form at most
        return int(_lib.load().elimrec_cooccur_groups())
    if name == "VOTE_SLOTS":             # (key, sum, count) entries of the LDS form's table of neighbour_vote_topk
        return int(_lib.load().elimrec_vote_slots())
    if name == "VOTE_GROUPS":            # workgroups (and workspace rows) of neighbour_vote_topk's dense form at most
        return int(_lib.load().elimrec_vote_groups())
    if name == "ALS_CHUNK":              # neighbour rows one workgroup of als_solve stages in LDS at a time
        return int(_lib.load().elimrec_als_chunk())
    if name == "EASE_BLOCK":             # block width of spd_inverse's sweep
        return int(_lib.load().elimrec_ease_block())
    if name == "EASE_HIST_STAGE":        # history ids one wave of ease_topk stages in LDS at a time
        return int(_lib.load().elimrec_ease_hist_stage())
    raise AttributeError("module %r has no attribute %r" % (__name__, name))


def sample_triplets(user_ids, ptr, items, num_items, n, seed, epoch, users, pos, neg):
    _lib.check(_lib.load().elimrec_sample_triplets(_dev(user_ids, "user_ids", torch.int32), _dev(ptr, "ptr", torch.int64),
                                                   _dev(items, "items", torch.int32), user_ids.numel(), num_items, n,
                                                   int(seed), int(epoch), _dev(users, "users", torch.int64),
                                                   _dev(pos, "pos", torch.int64), _dev(neg, "neg", torch.int64),
                                                   _stream()), "sample_triplets")


HARD_NEG_MAX_CANDIDATES = 64            # candidates per triplet sample_triplet_candidates draws and pick_hard_negatives takes


def sample_triplet_candidates(user_ids, ptr, items, num_items, n, seed, epoch, n_cand, users, pos, cands):
    """elimrec_sample_triplet_candidates: sample_triplets with n_cand candidate negatives per triplet. users / pos int64 [n]: bit
    for bit sample_triplets' for the same (seed, epoch); cands int32 [n x n_cand] contiguous: column 0 is sample_triplets' negative,
    every further column an independent draw of the same kind from a Philox stream of its own (duplicates within a row are
    allowed). 1 <= n_cand <= HARD_NEG_MAX_CANDIDATES."""
    n, n_cand = int(n), int(n_cand)
    if not 1 <= n_cand <= HARD_NEG_MAX_CANDIDATES:
        raise ValueError("elimrec_amd.ops.sample_triplet_candidates: 1 <= n_cand <= %d, got %d" % (HARD_NEG_MAX_CANDIDATES, n_cand))
    if not (isinstance(cands, torch.Tensor) and cands.is_contiguous() and tuple(cands.shape) == (n, n_cand)):
        raise ValueError("elimrec_amd.ops.sample_triplet_candidates: cands must be a contiguous [%d x %d] tensor" % (n, n_cand))
    if users.numel() < n or pos.numel() < n or not users.is_contiguous() or not pos.is_contiguous():
        raise ValueError("elimrec_amd.ops.sample_triplet_candidates: users and pos must be contiguous with at least %d entries" % n)
    _lib.check(_lib.load().elimrec_sample_triplet_candidates(
        _dev(user_ids, "user_ids", torch.int32), _dev(ptr, "ptr", torch.int64), _dev(items, "items", torch.int32), user_ids.numel(),
        num_items, n, int(seed), int(epoch), n_cand, _dev(users, "users", torch.int64), _dev(pos, "pos", torch.int64),
        _dev(cands, "cands", torch.int32), _stream()), "sample_triplet_candidates")


def score_candidates(Y, U, I, users, d, S, head_mask, fusion_mode, predict_type, cand_ptr, cand_items, out, sqnorm=None,
                     row_sum=None, I_total=0):
    """elimrec_score_candidates: out [B x width] (rows contiguous) = each user's candidate scores in list order, then -inf.
    cand_ptr int64 [B + 1] / cand_items int32: the lists as CSR. TIE: row_sum [B] (score_topk_shard phase 1) and I_total."""
    y, ldy = _rowmajor(Y, "Y")
    op, lds = _rowmajor(out, "out")
    B = users.numel()
    if out.shape[0] != B or cand_ptr.numel() != B + 1:
        raise ValueError("elimrec_amd.ops.score_candidates: out needs one row and cand_ptr B + 1 entries for each of the %d users" % B)
    items = cand_items if cand_items.numel() else None
    _lib.check(_lib.load().elimrec_score_candidates(y, ldy, U, I, _dev(users, "users", torch.int64), B, d, S, int(head_mask),
                                                    FUSION_MODES[fusion_mode], PREDICT_TYPES.get(predict_type, 0),
                                                    _dev(sqnorm, "sqnorm"), _dev(cand_ptr, "cand_ptr", torch.int64),
                                                    _dev(items, "cand_items", torch.int32), _dev(row_sum, "row_sum"),
                                                    int(I_total), op, lds, out.shape[1], _stream()), "score_candidates")
    return out


EFFECT_COLUMNS = ("ui", "mean_ui", "te", "nde", "score_te", "score_tie")


def effect_columns(mods):
    """Column names of score_effects' output: the six terms, then one cosine per single-modal head (mods: the heads' modality
    letters in head order, e.g. ("v", "a", "t"))."""
    return EFFECT_COLUMNS + tuple("cos_" + str(m) for m in mods)


def score_effects(Y, U, I, users, d, S, head_mask, fusion_mode, cand_ptr, cand_items, out, sqnorm, row_sum, I_total):
    """elimrec_score_effects: out [B x width x (6 + S)] (float32, contiguous) = per listed (user, item) pair the columns of
    effect_columns(); NaN beyond a list's length and at ids outside [0, I). cand_ptr int64 [B + 1] / cand_items int32: the lists
    as CSR. row_sum [B] (score_topk_shard phase 1 over the whole catalogue) and I_total always; sqnorm whenever S > 0."""
    y, ldy = _rowmajor(Y, "Y")
    B = users.numel()
    C = len(EFFECT_COLUMNS) + S
    if not (isinstance(out, torch.Tensor) and out.dim() == 3 and out.is_contiguous() and out.shape[0] == B and out.shape[2] == C):
        raise ValueError("elimrec_amd.ops.score_effects: out must be a contiguous [%d x width x %d] tensor" % (B, C))
    if cand_ptr.numel() != B + 1:
        raise ValueError("elimrec_amd.ops.score_effects: cand_ptr needs B + 1 entries for the %d users" % B)
    if row_sum is None or row_sum.numel() != B or int(I_total) <= 0:
        raise ValueError("elimrec_amd.ops.score_effects: row_sum needs one catalogue sum for each of the %d users, and I_total > 0" % B)
    if S > 0 and sqnorm is None:
        raise ValueError("elimrec_amd.ops.score_effects: %d single-modal heads need the squared-norm table" % S)
    items = cand_items if cand_items.numel() else None
    _lib.check(_lib.load().elimrec_score_effects(y, ldy, U, I, _dev(users, "users", torch.int64), B, d, S, int(head_mask),
                                                 FUSION_MODES[fusion_mode], _dev(sqnorm, "sqnorm"),
                                                 _dev(cand_ptr, "cand_ptr", torch.int64), _dev(items, "cand_items", torch.int32),
                                                 _dev(row_sum, "row_sum"), int(I_total), _dev(out, "out"), out.shape[1], _stream()),
               "score_effects")
    return out


def check_negative_room(excl_ptr, num_items, n_neg):
    """The reference's condition (random_choice.pyx:35-37) on the host, before any launch: every row must leave more than
    n_neg ids outside its exclusion list."""
    counts = np.diff(np.asarray(excl_ptr, dtype=np.int64))
    if n_neg <= 0:
        raise ValueError("'size' must be a positive integer.")
    if counts.size and (num_items <= counts).any():
        raise ValueError("The number of 'exclusion' is greater than 'high'.")
    if counts.size and (num_items - counts <= n_neg).any():
        raise ValueError("There is not enough integers to be sampled.")


def sample_negatives(excl_ptr, excl_items, num_items, n_neg, seed, out):
    """elimrec_sample_negatives: out int32 [n_users x n_neg] = per row n_neg distinct ids of [0, num_items) outside the row's
    sorted exclusion list (excl_ptr int64 [n_users + 1] / excl_items int32, device tensors)."""
    n_users = excl_ptr.numel() - 1
    if tuple(out.shape) != (n_users, n_neg) or not out.is_contiguous():
        raise ValueError("elimrec_amd.ops.sample_negatives: out must be a contiguous [%d x %d] tensor" % (n_users, n_neg))
    check_negative_room(excl_ptr.cpu().numpy(), num_items, n_neg)
    items = excl_items if excl_items.numel() else None
    _lib.check(_lib.load().elimrec_sample_negatives(_dev(excl_ptr, "excl_ptr", torch.int64), _dev(items, "excl_items", torch.int32),
                                                    n_users, int(num_items), int(n_neg), int(seed), _dev(out, "out", torch.int32),
                                                    _stream()), "sample_negatives")
    return out


def head_pack_floats(dims):
    arr = (ctypes.c_int * max(len(dims), 1))(*dims)
    return int(_lib.load().elimrec_head_pack_floats(len(dims), arr))


def head_pack_bwd_offset(dims):
    arr = (ctypes.c_int * max(len(dims), 1))(*dims)
    return int(_lib.load().elimrec_head_pack_bwd_offset(len(dims), arr))


def _head_weights(D, Wm, bm, Wf_user, bf_user, Wf_item, bf_item, Ws, bs, pack, d):
    """struct elimrec_head_weights of the lists over the feature tables (more tables than the struct holds: n_mod says so and
    the library answers ELIMREC_E_UNSUPPORTED)."""
    for t in list(Wm) + list(Ws) + [Wf_user, Wf_item]:
        assert t.is_contiguous()
    hw = _lib.HeadWeights(n_mod=len(D), recdim=int(d), d_Wf_user=_dev(Wf_user, "Wf_user"), d_bf_user=_dev(bf_user, "bf_user"),
                          d_Wf_item=_dev(Wf_item, "Wf_item"), d_bf_item=_dev(bf_item, "bf_item"), d_pack=_dev(pack, "pack"),
                          pack_floats=pack.numel())
    for m in range(min(len(D), _lib.HEAD_MAX_TABLES)):
        hw.D[m] = D[m]
        hw.d_Wm[m], hw.d_bm[m], hw.d_Ws[m], hw.d_bs[m] = (_dev(ts[m], "table") for ts in (Wm, bm, Ws, bs))
    return hw


def _head_fwd_fused(hin, hw, act, seg_info, OutAct, YAct, phase, what, c=None, S=()):
    """The one call behind the four head_fwd_fused* forms. c / S: the fp32 constants of the forms that read them. Returns False
    when the shape is outside the fused kernel's range."""
    hin.d_c = _dev(c, "c")
    for m, t in enumerate(S[:_lib.HEAD_MAX_TABLES]):
        hin.d_S[m], hin.ldS[m] = _dev(t, "table"), t.stride(0)
    rc = _lib.load().elimrec_head_fwd_fused(
        ctypes.byref(hin), ctypes.byref(hw), _dev(act, "act", torch.int32), _dev(seg_info, "seg_info", torch.int32), act.numel(),
        _dev(OutAct, "OutAct"), OutAct.stride(0), _dev(YAct, "YAct"), YAct.stride(0), int(phase), _stream())
    if rc == 10002:           # ELIMREC_E_UNSUPPORTED
        return False
    _lib.check(rc, what)
    return True


def head_fwd_fused_rows(rows, act, seg_info, c, S, Wm, bm, Wf_user, bf_user, Wf_item, bf_item, Ws, bs, pack, OutAct, YAct, d):
    """elimrec_head_fwd_fused, rows form: phase 4 of head_fwd_fused with the rows launch folded in. rows: dict(plan, ns, w, L, U,
    layers (L + 1 flat tensors, the last may be None), long_tab, narrow). Returns False when the shape is outside the fused
    kernel's range."""
    hin = _lib.HeadFwdIn()
    hr = hin.rows
    hr.A = ctypes.pointer(rows["plan"].desc)
    hr.ns, hr.w, hr.L, hr.U = int(rows["ns"]), int(rows["w"]), int(rows["L"]), int(rows["U"])
    for k, t in enumerate(rows["layers"]):
        hr.layers[k] = None if t is None else _dev(t, "layer")
    hr.d_long = _dev(rows["long_tab"], "long_tab")
    nar = rows["narrow"]
    assert nar.stride(1) == 1
    hr.d_narrow_out, hr.ld_narrow_out = _dev(nar, "narrow"), nar.stride(0)
    hw = _head_weights([t.shape[1] for t in S], Wm, bm, Wf_user, bf_user, Wf_item, bf_item, Ws, bs, pack, d)
    return _head_fwd_fused(hin, hw, act, seg_info, OutAct, YAct, 4, "head_fwd_fused_rows", c, S)


def head_fwd_fused(act, seg_info, out0, narrow, c, S, Wm, bm, Wf_user, bf_user, Wf_item, bf_item, Ws, bs, pack, OutAct, YAct, d, phase=0,
                   peers=None):
    """elimrec_head_fwd_fused: S / Wm / bm / Ws / bs are lists over the feature tables. phase 0: pack the weights and
    run the head; 1: pack only; 2: head only (pack holds the packed weights); 3 / 4: the head in two launches (the feature
    blocks without the shared part -- no out0 / narrow needed --, then the rest). Returns False when the shape is outside the
    fused kernel's range (the caller keeps the batched GEMMs). peers: the forward exchange's received buffer [W, R, 2 * dl]
    (out0 | narrow pieces of every peer) read in place of out0 / narrow (elimrec_head_fwd_in::d_recv)."""
    hw = _head_weights([t.shape[1] for t in S], Wm, bm, Wf_user, bf_user, Wf_item, bf_item, Ws, bs, pack, d)
    if peers is not None:
        assert peers.dim() == 3 and peers.is_contiguous() and peers.shape[1] == act.numel() and peers.shape[2] % 2 == 0
        hin = _lib.HeadFwdIn(d_recv=_dev(peers, "peers"), world=peers.shape[0], dl=peers.shape[2] // 2)
        return _head_fwd_fused(hin, hw, act, seg_info, OutAct, YAct, phase, "head_fwd_fused_peers", c, S)
    hin = _lib.HeadFwdIn(d_out0=_dev(out0, "out0"), ld_out0=out0.stride(0), d_narrow=_dev(narrow, "narrow"), ld_nar=narrow.stride(0))
    return _head_fwd_fused(hin, hw, act, seg_info, OutAct, YAct, phase, "head_fwd_fused", c, S)


def head_fwd_fused_src16(fshard, S_out, c_out, act, seg_info, out0, narrow, Wm, bm, Wf_user, bf_user, Wf_item, bf_item, Ws, bs, pack,
                         OutAct, YAct, d, phase=0):
    """elimrec_head_fwd_fused, 16-bit source: head_fwd_fused with the feature constants read from `fshard`'s 16-bit rows
    (lookup.FeatureShard holding EVERY row: one rank); S_out [R x sum_d] / c_out [R] (or None) receive the widened rows of the
    active nodes."""
    hin = _lib.HeadFwdIn(d_out0=_dev(out0, "out0"), ld_out0=out0.stride(0), d_narrow=_dev(narrow, "narrow"), ld_nar=narrow.stride(0))
    src = hin.src16
    src.d_table, src.row_elems, src.dtype = fshard.table.data_ptr(), fshard.row_elems, fshard.code
    if S_out is not None:
        assert S_out.stride(1) == 1 and S_out.shape[0] >= act.numel() and S_out.shape[1] == fshard.sum_d and c_out.numel() >= act.numel()
        src.d_S_out, src.ld_S_out, src.d_c_out = _dev(S_out, "S_out"), S_out.stride(0), _dev(c_out, "c_out")
    hw = _head_weights(fshard.dims, Wm, bm, Wf_user, bf_user, Wf_item, bf_item, Ws, bs, pack, d)
    return _head_fwd_fused(hin, hw, act, seg_info, OutAct, YAct, phase, "head_fwd_fused_src16")


def peer_cols_to_rows(recv, out0, out1):
    """recv [W x R x 2*dl] (per peer: layer mean | shared part of my rows in its columns) -> out0 / out1 [R x W*dl] row views."""
    W, R, two_dl = recv.shape
    dl = two_dl // 2
    assert recv.is_contiguous() and out0.stride(1) == 1 and out1.stride(1) == 1 and out0.shape == (R, W * dl) and out1.shape == (R, W * dl)
    _lib.check(_lib.load().elimrec_peer_cols_to_rows(_dev(recv, "recv"), W, R, dl, _dev(out0, "out0"), out0.stride(0), _dev(out1, "out1"),
                                                    out1.stride(0), _stream()), "peer_cols_to_rows")


KNN_MAX_K, KNN_MAX_D = 256, 256


class _ListQuery(object):
    """What NeighbourQuery and AudienceQuery share: query ids in [0, bound) and, optionally, per query a list of ids in
    [0, excl_bound) to leave out as CSR, checked on the host and then resident on `device` as ids / excl_ptr / excl_ids. The two
    classes give the nouns: names = (the ids' name, the excluded ids' name), spans = the two IndexErrors' words."""

    def __init__(self, ids, bound, device, excl_ptr, excl_ids, excl_bound, names, spans):
        who = type(self).__name__
        q = _checked_ids(ids, bound, who, names[0], spans[0])
        if (excl_ptr is None) != (excl_ids is None):
            raise ValueError("elimrec_amd.ops.%s: the exclusion CSR needs excl_ptr and %s, or neither" % (who, names[1]))
        self.n_queries = int(q.size)
        self.ids = _resident_ids(q, device)
        self.excl_ptr = self.excl_ids = None
        if excl_ptr is not None:
            p, e = _checked_csr(excl_ptr, excl_ids, q.size, excl_bound, who, ("excl_ptr", names[1], "Q", spans[1]))
            self.excl_ptr = torch.from_numpy(p).to(device)
            self.excl_ids = _resident_ids(e, device)


class NeighbourQuery(_ListQuery):
    """Query rows of an n_rows-row table and, optionally, per query a list of rows to leave out as CSR (excl_ptr [Q + 1],
    excl_rows), CHECKED ON THE HOST -- every query id and every exclusion id in [0, n_rows), ptr[0] = 0, ascending,
    ptr[Q] = len(excl_rows) -- and then resident on `device`: cosine_topk takes it as is, call after call, and no unchecked id
    ever reaches a kernel (the counterpart of TargetIndex). Exclusion lists may repeat ids, in any order, and may be empty."""

    def __init__(self, rows, n_rows, device, excl_ptr=None, excl_rows=None):
        _ListQuery.__init__(self, rows, n_rows, device, excl_ptr, excl_rows, n_rows, ("rows", "excl_rows"),
                            ("query rows span [%d, %d], the table has %d rows", "excluded rows span [%d, %d], the table has %d rows"))
        self.n_rows = int(n_rows)
        self.rows, self.excl_rows = self.ids, self.excl_ids


def cosine_topk_workspace(Q, n_rows, K):
    """Bytes of workspace cosine_topk needs (host arithmetic only)."""
    return int(_lib.load().elimrec_cosine_topk_workspace(int(Q), int(n_rows), int(K)))


def _rows_out(t, name, dtype, B, K, who, device=None):
    """Device pointer of an output of B rows of K entries: `dtype`, contiguous, [>= B x K] or 1-D with at least B * K entries
    (device: and on that device, the table's)."""
    if t is None:
        raise RuntimeError("elimrec_amd.ops: '%s' must be a HIP device tensor (the hot path has no CPU implementation)" % name)
    p = _dev(t, name, dtype)
    ok = t.is_contiguous() and (device is None or t.device == device) and (
        (t.dim() == 2 and t.shape[1] == K and t.shape[0] >= B) or (t.dim() == 1 and t.numel() >= B * K))
    if not ok:
        raise ValueError("elimrec_amd.ops.%s: %s must be contiguous%s, [>= %d x %d] or 1-D with at least %d entries"
                         % (who, name, "" if device is None else " on the table's device", B, K, B * K))
    return p


def _topk_dims(who, K, max_k, d, what):
    """The first two checks of cosine_topk / audience_topk, made before the query is looked at. what: the noun of the d message."""
    if not 1 <= K <= max_k:
        raise ValueError("elimrec_amd.ops.%s: 1 <= K <= %d, got %d" % (who, max_k, K))
    if d % 4 != 0 or not 4 <= d <= KNN_MAX_D:
        raise ValueError("elimrec_amd.ops.%s: %s needs d %% 4 == 0 and 4 <= d <= %d columns, got %d" % (who, what, KNN_MAX_D, d))


def _topk_call(who, n_cand, query, K, out_idx, out_val, workspace, device, out_device, head):
    """The back half of cosine_topk / audience_topk (elimrec_<who> and elimrec_<who>_workspace): the outputs, the workspace, the
    empty query, the call. n_cand: the candidate rows the workspace is sized for; head(): the entry point's arguments before K,
    built only when the call is made."""
    lib = _lib.load()
    Q = query.n_queries
    ip = _rows_out(out_idx, "out_idx", torch.int32, Q, K, who, out_device)
    vp = _rows_out(out_val, "out_val", torch.float32, Q, K, who, out_device) if out_val is not None else None
    need = int(getattr(lib, "elimrec_%s_workspace" % who)(Q, n_cand, K))
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=device)
    wp = _dev(workspace, "workspace", torch.uint8)
    if workspace.numel() < need or not workspace.is_contiguous() or wp % 16:
        raise ValueError("elimrec_amd.ops.%s: the workspace needs %d contiguous bytes, 16-byte aligned (got %d)"
                         % (who, need, workspace.numel()))
    if Q == 0:
        return out_idx
    _lib.check(getattr(lib, "elimrec_" + who)(*(head() + (K, ip, vp, wp, workspace.numel(), _stream()))), who)
    return out_idx


def cosine_topk(table, sqnorm, query_rows, K, out_idx, out_val=None, exclude_self=True, excl_ptr=None, excl_rows=None,
                workspace=None):
    """elimrec_cosine_topk: per query row the K rows of `table` closest to it by cosine, by (score descending, row id ascending):
    out_idx int32 / out_val float32 (optional) [Q x K], -1 / -inf where fewer than K candidates exist; entries of the outputs beyond
    [Q x K] are left alone. table [n x d] float32 with unit column stride (a column block of a wider matrix is fine), d % 4 == 0,
    4 <= d <= 256; sqnorm: 1-D float32, n entries, any stride (a column of row_sqnorms' table): the rows' squared norms. 1 <= K <= 256.
    Left out: the query itself (exclude_self), then the query's list of the CSR excl_ptr [Q + 1] / excl_rows. query_rows and the
    CSR: host arrays or tensors -- checked on the host at every call (a synchronisation for device tensors) -- or query_rows = a
    NeighbourQuery (excl_ptr = excl_rows = None), checked once. workspace: uint8 device tensor of at least cosine_topk_workspace
    bytes, 16-byte aligned (default: allocated here)."""
    if not isinstance(table, torch.Tensor) or not table.is_cuda:
        _dev(table, "table")
    tp, ld = _rowmajor(table, "table")
    n, d = table.shape
    sp = _dev(sqnorm, "sqnorm")
    if sqnorm.dim() != 1 or sqnorm.numel() != n or sqnorm.device != table.device:
        raise ValueError("elimrec_amd.ops.cosine_topk: sqnorm must be 1-D with one entry per table row (%d) on the table's device" % n)
    ld_sq = max(1, int(sqnorm.stride(0)))
    K = int(K)
    _topk_dims("cosine_topk", K, KNN_MAX_K, d, "the table")
    if isinstance(query_rows, NeighbourQuery):
        query = query_rows
        if excl_ptr is not None or excl_rows is not None:
            raise ValueError("elimrec_amd.ops.cosine_topk: a NeighbourQuery carries its own exclusions (pass excl_ptr=excl_rows=None)")
        if query.n_rows > n or query.rows.device != table.device:
            raise IndexError("elimrec_amd.ops.cosine_topk: the NeighbourQuery was checked for %d rows on %s, the table has %d on %s"
                             % (query.n_rows, query.rows.device, n, table.device))
    else:
        query = NeighbourQuery(query_rows, n, table.device, excl_ptr, excl_rows)
    return _topk_call("cosine_topk", n, query, K, out_idx, out_val, workspace, table.device, None, lambda: (
        tp, ld, n, d, sp, ld_sq, _dev(query.rows, "query_rows", torch.int32), query.n_queries, 1 if exclude_self else 0,
        _dev(query.excl_ptr, "excl_ptr", torch.int64), _dev(query.excl_rows, "excl_rows", torch.int32)))


class CrossQuery(_ListQuery):
    """Query rows of an n_query_rows-row query table and, optionally, per query a list of CANDIDATE rows (of the n_rows-row
    candidate table) to leave out as CSR (excl_ptr [Q + 1], excl_rows), CHECKED ON THE HOST -- every query id in
    [0, n_query_rows), every exclusion id in [0, n_rows), ptr[0] = 0, ascending, ptr[Q] = len(excl_rows) -- and then resident on
    `device`: cross_topk takes it as is, call after call. Exclusion lists may repeat ids, in any order, and may be empty."""

    def __init__(self, rows, n_query_rows, n_rows, device, excl_ptr=None, excl_rows=None):
        _ListQuery.__init__(self, rows, n_query_rows, device, excl_ptr, excl_rows, n_rows, ("rows", "excl_rows"),
                            ("query rows span [%d, %d], the query table has %d rows", "excluded rows span [%d, %d], the table has %d rows"))
        self.n_query_rows, self.n_rows = int(n_query_rows), int(n_rows)
        self.rows, self.excl_rows = self.ids, self.excl_ids


def _cross_side(t, sq, name, sq_name):
    """One side of cross_topk before the device is required: (rows, d) of a 2-D tensor with unit column stride and its squared
    norms' entry count (None: ones)."""
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.stride(1) != 1:
        raise ValueError("elimrec_amd.ops.cross_topk: %s must be a 2-D tensor with unit column stride" % name)
    if sq is not None and (not isinstance(sq, torch.Tensor) or sq.dim() != 1 or sq.numel() != t.shape[0] or sq.device != t.device):
        raise ValueError("elimrec_amd.ops.cross_topk: %s must be 1-D with one entry per row of %s (%d) on its device" % (sq_name, name, t.shape[0]))
    return int(t.shape[0]), int(t.shape[1])


def cross_topk(query_table, query_sqnorm, table, sqnorm, query_rows, K, out_idx, out_val=None, excl_ptr=None, excl_rows=None,
               workspace=None):
    """elimrec_cross_topk: cosine_topk with a query table of its own -- per query row (a row of `query_table` [nq x d]) the K rows
    of `table` [n x d] with the largest score, by (score descending, row id ascending); out_idx int32 / out_val float32 (optional)
    [Q x K], -1 / -inf where fewer than K candidates exist. Both tables float32 with unit column stride on one device, the same d,
    d % 4 == 0, 4 <= d <= 256. score = (dot * inv(query_sqnorm[q])) * inv(sqnorm[c]) as cosine_topk forms it; query_sqnorm / sqnorm =
    None means a vector of ones on that side, and with both None the score is the plain fp32 dot product (1 / max(sqrt(1), 1e-12)
    is exactly 1): top-K_i x_u . y_i of a factor model. Left out: the query's list of the CSR excl_ptr [Q + 1] / excl_rows, ids of
    CANDIDATE rows; there is no exclude_self. query_rows and the CSR: host arrays or tensors, checked on the host at every call, or
    query_rows = a CrossQuery (excl_ptr = excl_rows = None), checked once. The same kernel, chunks (KNN_CHUNK), workspace
    (cosine_topk_workspace bytes), selection and merge as cosine_topk. Every argument error is raised before the device is
    required. 1 <= K <= 256. Dot products are unbounded: a score of +inf is listed first (ties by row id), a score of -inf or
    NaN is no candidate and is never listed."""
    who = "cross_topk"
    nq, dq = _cross_side(query_table, query_sqnorm, "query_table", "query_sqnorm")
    n, d = _cross_side(table, sqnorm, "table", "sqnorm")
    if dq != d or query_table.device != table.device:
        raise ValueError("elimrec_amd.ops.cross_topk: the two tables share d and the device, got d = %d on %s and %d on %s"
                         % (dq, query_table.device, d, table.device))
    K = int(K)
    _topk_dims(who, K, KNN_MAX_K, d, "the table")
    if isinstance(query_rows, CrossQuery):
        query = query_rows
        if excl_ptr is not None or excl_rows is not None:
            raise ValueError("elimrec_amd.ops.cross_topk: a CrossQuery carries its own exclusions (pass excl_ptr=excl_rows=None)")
        if query.n_query_rows > nq or query.n_rows > n or query.rows.device != table.device:
            raise IndexError("elimrec_amd.ops.cross_topk: the CrossQuery was checked for %d query rows and %d rows on %s, the tables have "
                             "%d and %d on %s" % (query.n_query_rows, query.n_rows, query.rows.device, nq, n, table.device))
    else:
        query = CrossQuery(query_rows, nq, n, table.device, excl_ptr, excl_rows)
    qp, ldq = _rowmajor(query_table, "query_table")
    tp, ld = _rowmajor(table, "table")
    if query_sqnorm is None:
        query_sqnorm = torch.ones(max(1, nq), dtype=torch.float32, device=table.device)
    if sqnorm is None:
        sqnorm = torch.ones(max(1, n), dtype=torch.float32, device=table.device)
    sqp, sp = _dev(query_sqnorm, "query_sqnorm"), _dev(sqnorm, "sqnorm")
    ld_sqq, ld_sq = max(1, int(query_sqnorm.stride(0))), max(1, int(sqnorm.stride(0)))
    return _topk_call(who, n, query, K, out_idx, out_val, workspace, table.device, None, lambda: (
        qp, ldq, nq, sqp, ld_sqq, tp, ld, n, d, sp, ld_sq, _dev(query.rows, "query_rows", torch.int32), query.n_queries,
        _dev(query.excl_ptr, "excl_ptr", torch.int64), _dev(query.excl_rows, "excl_rows", torch.int32)))


def list_overlap(a, b, out):
    """elimrec_list_overlap: out int32 [n] <- per row the number of ids >= 0 of a[r, :] that also occur in b[r, :]; a, b int32
    [n x K] contiguous, lists of distinct ids and -1 fillers, K <= 1024."""
    ap, bp = _dev(a, "a", torch.int32), _dev(b, "b", torch.int32)
    if a.dim() != 2 or a.shape != b.shape or not a.is_contiguous() or not b.is_contiguous() or a.shape[1] < 1:
        raise ValueError("elimrec_amd.ops.list_overlap: a and b must be contiguous [n x K] tensors of one shape, K >= 1")
    n, K = a.shape
    op = _dev(out, "out", torch.int32)
    if out.dim() != 1 or not out.is_contiguous() or out.numel() < n:
        raise ValueError("elimrec_amd.ops.list_overlap: out must be a contiguous 1-D tensor of at least %d entries" % n)
    _lib.check(_lib.load().elimrec_list_overlap(ap, bp, n, K, op, _stream()), "list_overlap")
    return out


AUDIENCE_MAX_K = 256


class AudienceQuery(_ListQuery):
    """Query items of an n_items catalogue and, optionally, per item a list of users to leave out as CSR (excl_ptr [Q + 1],
    excl_users: typically the item's training users), CHECKED ON THE HOST -- every item id in [0, n_items), every excluded user id
    in [0, n_users), ptr[0] = 0, ascending, ptr[Q] = len(excl_users) -- and then resident on `device`: audience_topk takes it as is,
    call after call, and no unchecked id ever reaches a kernel (the counterpart of NeighbourQuery). Exclusion lists may repeat ids,
    in any order, and may be empty."""

    def __init__(self, items, n_items, n_users, device, excl_ptr=None, excl_users=None):
        _ListQuery.__init__(self, items, n_items, device, excl_ptr, excl_users, n_users, ("items", "excl_users"),
                            ("query items span [%d, %d], the catalogue has %d items", "excluded users span [%d, %d], the model has %d users"))
        self.n_items, self.n_users = int(n_items), int(n_users)
        self.items, self.excl_users = self.ids, self.excl_ids


def audience_topk_workspace(Q, U, K):
    """Bytes of workspace audience_topk needs (host arithmetic only)."""
    return int(_lib.load().elimrec_audience_topk_workspace(int(Q), int(U), int(K)))


def audience_topk(Y, U, I, query, d, S, head_mask, fusion_mode, predict_type, K, out_idx, out_val=None, sqnorm=None, row_sum=None,
                  I_total=None, workspace=None):
    """elimrec_audience_topk: per query item the K users with the largest predict() score for the (user, item) pair, by (score
    descending, user id ascending): out_idx int32 / out_val float32 (optional) [Q x K], -1 / -inf where fewer than K users are
    eligible; entries of the outputs beyond [Q x K] are left alone. Y [U + I x >= (1 + S) d] float32 with unit column stride, users
    first (the table the scorers read); d % 4 == 0, 4 <= d <= 256, 0 <= S <= 3, 1 <= K <= 256. fusion_mode 'rubi' / 'hm' / 'sum',
    head_mask as score_topk reads it, predict_type 'TE' / 'TIE' / anything else = normal. query: an AudienceQuery (checked once),
    or host / device item ids, checked here at every call. sqnorm [(U + I) x (1 + S)]: row_sqnorms' table (default: computed here).
    row_sum [U] float32 (TIE: required): the users' sums of sigmoid(u . i) over the catalogue of I_total items (default I), from
    score_topk_shard phase 1. workspace: uint8 device tensor of at least audience_topk_workspace bytes, 16-byte aligned (default:
    allocated here). The scores follow the evaluator's math mode (elimrec_score_set_math)."""
    if not isinstance(Y, torch.Tensor) or not Y.is_cuda:
        _dev(Y, "Y")
    y, ldy = _rowmajor(Y, "Y")
    U, I, d, S, K = int(U), int(I), int(d), int(S), int(K)
    _topk_dims("audience_topk", K, AUDIENCE_MAX_K, d, "a block")
    if not 0 <= S <= 3:
        raise ValueError("elimrec_amd.ops.audience_topk: 0 <= S <= 3, got %d" % S)
    if fusion_mode not in FUSION_MODES:
        raise ValueError("elimrec_amd.ops.audience_topk: fusion_mode is one of %s, got %r" % (sorted(FUSION_MODES), fusion_mode))
    if U < 0 or I < 0 or Y.dim() != 2 or Y.shape[0] != U + I or Y.shape[1] < (1 + S) * d:
        raise ValueError("elimrec_amd.ops.audience_topk: Y must be [U + I = %d x >= (1 + S) d = %d], got %s"
                         % (U + I, (1 + S) * d, tuple(Y.shape)))
    if isinstance(query, AudienceQuery):
        if query.n_items > I or query.n_users > U or query.items.device != Y.device:
            raise IndexError("elimrec_amd.ops.audience_topk: the AudienceQuery was checked for %d items and %d users on %s, the table "
                             "has %d and %d on %s" % (query.n_items, query.n_users, query.items.device, I, U, Y.device))
    else:
        query = AudienceQuery(query, I, U, Y.device)
    tie = PREDICT_TYPES.get(predict_type, 0) == 2
    if tie:
        if row_sum is None:
            raise ValueError("elimrec_amd.ops.audience_topk: predict type TIE needs row_sum [U] (score_topk_shard phase 1 over all users)")
        if row_sum.dim() != 1 or row_sum.numel() != U or not row_sum.is_contiguous() or row_sum.device != Y.device:
            raise ValueError("elimrec_amd.ops.audience_topk: row_sum must be contiguous, 1-D with one entry per user (%d) on Y's device" % U)
    I_total = I if I_total is None else int(I_total)
    if sqnorm is None:
        sqnorm = row_sqnorms(Y, d, 1 + S, torch.empty((U + I, 1 + S), dtype=torch.float32, device=Y.device))
    elif tuple(sqnorm.shape) != (U + I, 1 + S) or not sqnorm.is_contiguous() or sqnorm.device != Y.device:
        raise ValueError("elimrec_amd.ops.audience_topk: sqnorm must be contiguous [U + I x 1 + S] = [%d x %d] on Y's device" % (U + I, 1 + S))
    return _topk_call("audience_topk", U, query, K, out_idx, out_val, workspace, Y.device, Y.device, lambda: (
        y, ldy, U, I, d, S, int(head_mask), FUSION_MODES[fusion_mode], PREDICT_TYPES.get(predict_type, 0), _dev(sqnorm, "sqnorm"),
        _dev(row_sum, "row_sum") if tie else None, I_total, _dev(query.items, "items", torch.int32), query.n_queries,
        _dev(query.excl_ptr, "excl_ptr", torch.int64), _dev(query.excl_users, "excl_users", torch.int32)))


def audience_hits(lists, ptr, users, out):
    """elimrec_audience_hits: out int32 [Q] <- per row the number of ids >= 0 of lists[q, :] (int32 [Q x K] contiguous) that occur in
    segment q of the CSR ptr int64 [Q + 1] / users int32 (device tensors, checked by the caller: a TargetIndex-style host check)."""
    lp = _dev(lists, "lists", torch.int32)
    if lists.dim() != 2 or not lists.is_contiguous() or lists.shape[1] < 1:
        raise ValueError("elimrec_amd.ops.audience_hits: lists must be a contiguous [Q x K] tensor, K >= 1")
    Q, K = lists.shape
    pp, up, op = _dev(ptr, "ptr", torch.int64), _dev(users, "users", torch.int32), _dev(out, "out", torch.int32)
    if ptr.numel() != Q + 1 or not ptr.is_contiguous() or not users.is_contiguous() or out.dim() != 1 or not out.is_contiguous() or out.numel() < Q:
        raise ValueError("elimrec_amd.ops.audience_hits: ptr needs Q + 1 = %d contiguous entries, out at least %d" % (Q + 1, Q))
    _lib.check(_lib.load().elimrec_audience_hits(lp, Q, K, pp, up, op, _stream()), "audience_hits")
    return out


def neighbour_columns(mods):
    """Column names of the neighbour report: overlap_<m> per single-modal head (the share of the fused list that the head's list
    repeats), then the mean cosine of the fused list and of each head's, then the mean training-interaction count of the listed
    neighbours (mods: the heads' modality letters in head order)."""
    mods = tuple(str(m) for m in mods)
    return (tuple("overlap_" + m for m in mods) + ("cos_fused",) + tuple("cos_" + m for m in mods)
            + ("pop_fused",) + tuple("pop_" + m for m in mods))


LIST_MAX_K, LIST_MAX_BLOCKS = 256, 8


def list_chunk_cols(K, d):
    """Columns of one LDS stage of list_pair_cosine for lists of K ids over blocks of d columns (host arithmetic only)."""
    return int(_lib.load().elimrec_list_pair_cosine_chunk_cols(int(K), int(d)))


def _int_lists(lists, name, what):
    p = _dev(lists, name, torch.int32)
    if lists.dim() != 2 or not lists.is_contiguous() or lists.shape[1] < 1:
        raise ValueError("elimrec_amd.ops.%s: %s must be a contiguous [B x K] tensor, K >= 1" % (what, name))
    return p


def list_pair_cosine(table, sqnorm, lists, out, blocks=1):
    """elimrec_list_pair_cosine: out[b, h] float32 <- the mean, over the position pairs i < j of lists[b] whose entries are both
    listed, of the cosine of the two rows in column block h of `table` (intra-list similarity); NaN with fewer than two listed
    entries. table [n x blocks * d] float32 with unit column stride (a column block of a wider matrix is fine), block h = columns
    [h * d, (h + 1) * d), d % 4 == 0, 4 <= d <= 256, 1 <= blocks <= 8; sqnorm [n x blocks] float32 with unit column stride (row_sqnorms'
    table or a column slice of it; 1-D with any stride when blocks == 1): the rows' squared norms per block. lists int32 [B x K]
    contiguous on the table's device, 1 <= K <= LIST_MAX_K: an entry < 0 or >= n is not listed (the kernel checks every entry, no
    host check is needed), duplicates are pairs. out: float32, contiguous, [>= B x blocks] or 1-D with at least B * blocks entries;
    entries beyond [B x blocks] are left alone. A list's bits depend on its entries alone (csrc/lists.hip)."""
    if not isinstance(table, torch.Tensor) or not table.is_cuda:
        _dev(table, "table")
    tp, ld = _rowmajor(table, "table")
    n, width = table.shape
    blocks = int(blocks)
    if not 1 <= blocks <= LIST_MAX_BLOCKS:
        raise ValueError("elimrec_amd.ops.list_pair_cosine: 1 <= blocks <= %d, got %d" % (LIST_MAX_BLOCKS, blocks))
    if width % blocks != 0:
        raise ValueError("elimrec_amd.ops.list_pair_cosine: the table's %d columns do not split into %d equal blocks" % (width, blocks))
    d = width // blocks
    if d % 4 != 0 or not 4 <= d <= KNN_MAX_D:
        raise ValueError("elimrec_amd.ops.list_pair_cosine: a block needs d %% 4 == 0 and 4 <= d <= %d columns, got %d" % (KNN_MAX_D, d))
    sp = _dev(sqnorm, "sqnorm")
    if sqnorm.device != table.device:
        raise ValueError("elimrec_amd.ops.list_pair_cosine: sqnorm must live on the table's device")
    if sqnorm.dim() == 1 and blocks == 1 and sqnorm.numel() == n:
        ld_sq = max(1, int(sqnorm.stride(0)))
    elif sqnorm.dim() == 2 and tuple(sqnorm.shape) == (n, blocks) and (sqnorm.stride(1) == 1 or blocks == 1):
        ld_sq = max(blocks, int(sqnorm.stride(0)))
    else:
        raise ValueError("elimrec_amd.ops.list_pair_cosine: sqnorm must be [%d x %d] with unit column stride (or 1-D with %d entries "
                         "when blocks == 1)" % (n, blocks, n))
    lp = _int_lists(lists, "lists", "list_pair_cosine")
    if lists.device != table.device:
        raise ValueError("elimrec_amd.ops.list_pair_cosine: lists must live on the table's device")
    B, K = lists.shape
    if not 1 <= K <= LIST_MAX_K:
        raise ValueError("elimrec_amd.ops.list_pair_cosine: 1 <= K <= %d, got %d" % (LIST_MAX_K, K))
    op = _rows_out(out, "out", torch.float32, B, blocks, "list_pair_cosine", device=table.device)
    if B == 0:
        return out
    _lib.check(_lib.load().elimrec_list_pair_cosine(tp, ld, n, blocks, d, sp, ld_sq, lp, B, K, op, _stream()), "list_pair_cosine")
    return out


def list_exposure(lists, counts):
    """elimrec_list_exposure: counts[i] += the number of entries of lists (int32 [B x K] contiguous) equal to i, for i in
    [0, len(counts)); entries outside are skipped. counts: int32, 1-D, contiguous, on the lists' device; it ACCUMULATES over calls
    (zero it first). Integer atomics: exact, whatever the order."""
    lp = _int_lists(lists, "lists", "list_exposure")
    cp = _dev(counts, "counts", torch.int32)
    if counts.dim() != 1 or not counts.is_contiguous() or counts.device != lists.device:
        raise ValueError("elimrec_amd.ops.list_exposure: counts must be a contiguous 1-D tensor on the lists' device")
    B, K = lists.shape
    if B and counts.numel():
        _lib.check(_lib.load().elimrec_list_exposure(lp, B, K, counts.numel(), cp, _stream()), "list_exposure")
    return counts


def list_columns(mods):
    """Column names of the list report's user rows: ils_fused and ils_<m> per single-modal head (the mean pairwise cosine of the
    user's list in that space), then pop (the mean training-interaction count of the listed items); mods: the heads' modality
    letters in head order."""
    return ("ils_fused",) + tuple("ils_" + str(m) for m in mods) + ("pop",)


def mmr_rows_in_lds(N, d):
    """Which form mmr_rerank takes for pools of N positions over d columns (host arithmetic only): True = the pool's rows are
    gathered once into LDS, False = the candidates' rows are read from global memory at every step. ValueError outside the limits."""
    form = int(_lib.load().elimrec_mmr_rows_in_lds(int(N), int(d)))
    if form < 0:
        raise ValueError("elimrec_amd.ops.mmr_rows_in_lds: 1 <= N <= %d, d %% 4 == 0 and 4 <= d <= %d, got N %d, d %d"
                         % (_lib.load().elimrec_mmr_max_pool(), KNN_MAX_D, N, d))
    return bool(form)


def mmr_rerank(table, sqnorm, pool_idx, pool_val, K, lam, out_idx, out_pos=None, out_val=None):
    """elimrec_mmr_rerank: greedy maximal-marginal-relevance re-ranking of each row's pool. pool_idx int32 / pool_val float32
    [B x N] contiguous on the table's device, 1 <= K <= N <= MMR_MAX_POOL: a position is listed when its id lies in [0, n) and its
    score is finite (the kernel checks every entry, no host check is needed). With rel = the listed scores scaled to [0, 1] per pool
    (0 when they are all equal), step t picks the listed, not yet picked position with the largest
    lam * rel_i - (1 - lam) * max_{picked j} cos(i, j) (no penalty at t = 0), the lowest position among equals; 0 <= lam <= 1.
    table [n x d] float32 with unit column stride (a column block of a wider matrix is fine), d % 4 == 0, 4 <= d <= 256; sqnorm: 1-D
    float32, n entries, any stride: the rows' squared norms. out_idx int32 [B x K] <- the picked ids, out_pos int32 (optional) their
    pool positions, out_val float32 (optional) their objectives at pick time; -1 / -1 / -inf once no listed position is left.
    Outputs: contiguous, [>= B x K] or 1-D with at least B * K entries; entries beyond [B x K] are left alone. A row's bits depend
    on its pool, N, K, d and lam alone (csrc/rerank.hip)."""
    for t, name in ((table, "table"), (sqnorm, "sqnorm"), (pool_idx, "pool_idx"), (pool_val, "pool_val"), (out_idx, "out_idx")):
        if not isinstance(t, torch.Tensor):
            raise RuntimeError("elimrec_amd.ops: '%s' must be a HIP device tensor (the hot path has no CPU implementation)" % name)
    if table.dim() != 2 or table.stride(1) != 1:
        raise ValueError("elimrec_amd.ops.mmr_rerank: table must be 2-D with unit column stride")
    n, d = table.shape
    if d % 4 != 0 or not 4 <= d <= KNN_MAX_D:
        raise ValueError("elimrec_amd.ops.mmr_rerank: the table needs d %% 4 == 0 and 4 <= d <= %d columns, got %d" % (KNN_MAX_D, d))
    if sqnorm.dim() != 1 or sqnorm.numel() != n or sqnorm.device != table.device:
        raise ValueError("elimrec_amd.ops.mmr_rerank: sqnorm must be 1-D with one entry per table row (%d) on the table's device" % n)
    if (pool_idx.dim() != 2 or pool_idx.shape != pool_val.shape or not pool_idx.is_contiguous() or not pool_val.is_contiguous()
            or pool_idx.device != table.device or pool_val.device != table.device):
        raise ValueError("elimrec_amd.ops.mmr_rerank: pool_idx and pool_val must be contiguous [B x N] tensors of one shape on the "
                         "table's device")
    B, N = pool_idx.shape
    if isinstance(K, bool) or int(K) != K:
        raise ValueError("elimrec_amd.ops.mmr_rerank: K must be an integer, got %r" % (K,))
    K = int(K)
    max_pool = int(_lib.load().elimrec_mmr_max_pool())
    if not 1 <= K <= N <= max_pool:
        raise ValueError("elimrec_amd.ops.mmr_rerank: 1 <= K <= N <= %d, got K %d, N %d" % (max_pool, K, N))
    lam = float(lam)
    if not 0.0 <= lam <= 1.0:                                        # (NaN fails too)
        raise ValueError("elimrec_amd.ops.mmr_rerank: 0 <= lam <= 1, got %r" % lam)
    tp, ld = _rowmajor(table, "table")
    sp = _dev(sqnorm, "sqnorm")
    ld_sq = max(1, int(sqnorm.stride(0)))
    pi, pv = _dev(pool_idx, "pool_idx", torch.int32), _dev(pool_val, "pool_val", torch.float32)
    ip = _rows_out(out_idx, "out_idx", torch.int32, B, K, "mmr_rerank", device=table.device)
    pp = _rows_out(out_pos, "out_pos", torch.int32, B, K, "mmr_rerank", device=table.device) if out_pos is not None else None
    vp = _rows_out(out_val, "out_val", torch.float32, B, K, "mmr_rerank", device=table.device) if out_val is not None else None
    if B == 0:
        return out_idx
    _lib.check(_lib.load().elimrec_mmr_rerank(tp, ld, n, d, sp, ld_sq, pi, pv, B, N, K, lam, ip, pp, vp, _stream()), "mmr_rerank")
    return out_idx


def _cal_tensors(who, *named):
    for t, name in named:
        if not isinstance(t, torch.Tensor):
            raise RuntimeError("elimrec_amd.ops: '%s' must be a HIP device tensor (the hot path has no CPU implementation)" % name)


def _cal_classes(who, class_of, C, device):
    """(n_items, C) of a class table: int32, 1-D, contiguous, on `device`; 1 <= C <= CALIBRATE_MAX_CLASSES."""
    if class_of.dim() != 1 or class_of.dtype != torch.int32 or not class_of.is_contiguous() or class_of.device != device:
        raise ValueError("elimrec_amd.ops.%s: class_of must be a contiguous 1-D int32 tensor (one class per item) on the lists' device" % who)
    if isinstance(C, bool) or int(C) != C:
        raise ValueError("elimrec_amd.ops.%s: C must be an integer, got %r" % (who, C))
    max_c = int(_lib.load().elimrec_calibrate_max_classes())
    if not 1 <= int(C) <= max_c:
        raise ValueError("elimrec_amd.ops.%s: 1 <= C <= %d, got %d" % (who, max_c, C))
    return class_of.numel(), int(C)


def _cal_target(who, target, B, C, device):
    """Row stride of a target block: float32 [B x C] with unit column stride (a column block of a wider matrix is fine)."""
    ok = target.dim() == 2 and target.dtype == torch.float32 and target.device == device and target.shape[0] == B and (
        C is None or target.shape[1] == C) and (target.stride(1) == 1 or target.shape[1] == 1)
    if not ok:
        raise ValueError("elimrec_amd.ops.%s: target must be a float32 [%d x %s] tensor with unit column stride on the lists' device"
                         % (who, B, "C" if C is None else C))
    return max(int(target.shape[1]), int(target.stride(0))) if B > 1 else int(target.shape[1])


def _cal_smooth(who, smooth):
    smooth = float(smooth)
    if not 0.0 < smooth < 1.0:                                       # (NaN fails too)
        raise ValueError("elimrec_amd.ops.%s: 0 < smooth < 1, got %r" % (who, smooth))
    return smooth


def calibrate_rerank(pool_idx, pool_val, class_of, target, K, lam, out_idx, out_pos=None, out_val=None, smooth=0.01):
    """elimrec_calibrate_rerank: greedy calibrated re-ranking of each row's pool (Steck, RecSys 2018): K items whose mix of item
    classes follows the row's target mix. pool_idx int32 / pool_val float32 [B x N] contiguous on one device, 1 <= K <= N <=
    MMR_MAX_POOL; class_of int32 [n_items]: every item's class; target float32 [B x C] with unit column stride (any row stride),
    1 <= C <= CALIBRATE_MAX_CLASSES: the target share p_c of every class (a negative or non-finite entry counts as 0). A position
    is listed when its id lies in [0, n_items), its score is finite and its class lies in [0, C) (the kernel checks every entry, no
    host check is needed). With rel = the listed scores scaled to [0, 1] per pool and q~ = (1 - smooth) q + smooth p, q = the class
    shares of the picks so far plus the candidate, step t picks the listed, not yet picked position with the largest
    lam * rel_i - (1 - lam) * sum_{c: p_c > 0} p_c log(p_c / q~_c) -- all in float64 --, the lowest position among equals.
    lam weighs the RELEVANCE, as in mmr_rerank (Steck's lambda weighs the calibration term): lam = 1 keeps a sorted pool's order;
    0 <= lam <= 1, 0 < smooth < 1. out_idx int32 [B x K] <- the picked ids, out_pos int32 (optional) their pool positions, out_val
    float32 (optional) their objectives at pick time; -1 / -1 / -inf once no listed position is left. Outputs: contiguous,
    [>= B x K] or 1-D with at least B * K entries; entries beyond [B x K] are left alone. A row's bits depend on its pool, the
    classes of its ids, its target row, N, K, C, lam and smooth alone (csrc/calibrate.hip)."""
    who = "calibrate_rerank"
    _cal_tensors(who, (pool_idx, "pool_idx"), (pool_val, "pool_val"), (class_of, "class_of"), (target, "target"), (out_idx, "out_idx"))
    if (pool_idx.dim() != 2 or pool_idx.shape != pool_val.shape or not pool_idx.is_contiguous() or not pool_val.is_contiguous()
            or pool_idx.dtype != torch.int32 or pool_val.dtype != torch.float32 or pool_idx.device != pool_val.device):
        raise ValueError("elimrec_amd.ops.calibrate_rerank: pool_idx (int32) and pool_val (float32) must be contiguous [B x N] tensors "
                         "of one shape on one device")
    B, N = pool_idx.shape
    dev = pool_idx.device
    if target.dim() != 2:
        raise ValueError("elimrec_amd.ops.calibrate_rerank: target must be a float32 [%d x C] tensor with unit column stride on the "
                         "lists' device" % B)
    n_items, C = _cal_classes(who, class_of, target.shape[1], dev)
    ld_t = _cal_target(who, target, B, C, dev)
    if isinstance(K, bool) or int(K) != K:
        raise ValueError("elimrec_amd.ops.calibrate_rerank: K must be an integer, got %r" % (K,))
    K = int(K)
    max_pool = int(_lib.load().elimrec_mmr_max_pool())
    if not 1 <= K <= N <= max_pool:
        raise ValueError("elimrec_amd.ops.calibrate_rerank: 1 <= K <= N <= %d, got K %d, N %d" % (max_pool, K, N))
    lam = float(lam)
    if not 0.0 <= lam <= 1.0:                                        # (NaN fails too)
        raise ValueError("elimrec_amd.ops.calibrate_rerank: 0 <= lam <= 1, got %r" % lam)
    smooth = _cal_smooth(who, smooth)
    pi, pv = _dev(pool_idx, "pool_idx", torch.int32), _dev(pool_val, "pool_val", torch.float32)
    cp, tp = _dev(class_of, "class_of", torch.int32), _dev(target, "target")
    ip = _rows_out(out_idx, "out_idx", torch.int32, B, K, who, device=dev)
    pp = _rows_out(out_pos, "out_pos", torch.int32, B, K, who, device=dev) if out_pos is not None else None
    vp = _rows_out(out_val, "out_val", torch.float32, B, K, who, device=dev) if out_val is not None else None
    if B == 0:
        return out_idx
    _lib.check(_lib.load().elimrec_calibrate_rerank(pi, pv, B, N, K, cp, n_items, tp, ld_t, C, lam, smooth, ip, pp, vp, _stream()), who)
    return out_idx


def class_shares(ptr, items, class_of, C, out):
    """elimrec_class_shares_csr: out float32 [B x C] <- per segment b of the CSR ptr int64 [B + 1] / items int32 the share of every
    item class among its listed entries: float(count_c) / float(listed), one fp32 division; zeros for a segment without a listed
    entry. class_of int32 [n_items]; an entry outside [0, n_items) or with a class outside [0, C) is skipped (the kernel checks
    every entry and clips every segment to the items it is given: no host check is needed), a repeated id counts each time.
    1 <= C <= CALIBRATE_MAX_CLASSES. out: contiguous, [>= B x C] or 1-D with at least B * C entries; entries beyond are left alone.
    Integer counts: exact in any order (csrc/calibrate.hip)."""
    who = "class_shares"
    _cal_tensors(who, (ptr, "ptr"), (items, "items"), (class_of, "class_of"), (out, "out"))
    if (ptr.dim() != 1 or ptr.numel() < 1 or ptr.dtype != torch.int64 or not ptr.is_contiguous() or items.dim() != 1
            or items.dtype != torch.int32 or not items.is_contiguous() or items.device != ptr.device):
        raise ValueError("elimrec_amd.ops.class_shares: ptr (int64, B + 1 entries) and items (int32) must be contiguous 1-D tensors on "
                         "one device")
    B = ptr.numel() - 1
    n_items, C = _cal_classes(who, class_of, C, ptr.device)
    pp, ip = _dev(ptr, "ptr", torch.int64), _dev(items, "items", torch.int32)
    cp = _dev(class_of, "class_of", torch.int32)
    op = _rows_out(out, "out", torch.float32, B, C, who, device=ptr.device)
    if B == 0:
        return out
    _lib.check(_lib.load().elimrec_class_shares_csr(pp, ip, items.numel(), B, cp, n_items, C, op, _stream()), who)
    return out


def list_calibration(lists, class_of, C, out_shares, target=None, smooth=0.01, out_kl=None):
    """elimrec_list_calibration: out_shares float32 [B x C] <- the class shares of every row of lists (int32 [B x K] contiguous,
    K >= 1), as class_shares forms them (-1 fillers and ids outside the catalogue are skipped). With target (float32 [B x C], unit
    column stride, any row stride) and out_kl (float32, at least B entries) -- both or neither -- also the rows' miscalibration
    out_kl[b] = sum_{c: p_c > 0} p_c log(p_c / ((1 - smooth) q_c + smooth p_c)), q = the row's class shares in float64, p =
    target[b] as calibrate_rerank reads it: Steck's C_KL, rounded once to fp32; 0 < smooth < 1."""
    who = "list_calibration"
    _cal_tensors(who, (lists, "lists"), (class_of, "class_of"), (out_shares, "out_shares"))
    if lists.dim() != 2 or lists.dtype != torch.int32 or not lists.is_contiguous() or lists.shape[1] < 1:
        raise ValueError("elimrec_amd.ops.list_calibration: lists must be a contiguous int32 [B x K] tensor, K >= 1")
    B, K = lists.shape
    dev = lists.device
    n_items, C = _cal_classes(who, class_of, C, dev)
    if (target is None) != (out_kl is None):
        raise ValueError("elimrec_amd.ops.list_calibration: target and out_kl go together")
    tp = kp = None
    ld_t = C
    if target is not None:
        _cal_tensors(who, (target, "target"), (out_kl, "out_kl"))
        ld_t = _cal_target(who, target, B, C, dev)
        smooth = _cal_smooth(who, smooth)
        if out_kl.dim() != 1 or out_kl.dtype != torch.float32 or not out_kl.is_contiguous() or out_kl.numel() < B or out_kl.device != dev:
            raise ValueError("elimrec_amd.ops.list_calibration: out_kl must be a contiguous 1-D float32 tensor with at least %d entries "
                             "on the lists' device" % B)
        tp, kp = _dev(target, "target"), _dev(out_kl, "out_kl")
    lp, cp = _dev(lists, "lists", torch.int32), _dev(class_of, "class_of", torch.int32)
    op = _rows_out(out_shares, "out_shares", torch.float32, B, C, who, device=dev)
    if B == 0:
        return out_shares
    _lib.check(_lib.load().elimrec_list_calibration(lp, B, K, cp, n_items, C, op, tp, ld_t, float(smooth), kp, _stream()), who)
    return out_shares


def kmeans_workspace(n, d, C):
    """Bytes of workspace kmeans_update needs (host arithmetic only; 0 for arguments out of range)."""
    return int(_lib.load().elimrec_kmeans_workspace(int(n), int(d), int(C)))


def _kmeans_table(who, table, sqnorm, centroids, centroid_sqnorm):
    """The checks kmeans_assign / kmeans_update share -> (table pointer, ld, n, d, norm pointer, norm ld, centroid pointer, centroid
    norm pointer, C)."""
    for t, name in ((table, "table"), (sqnorm, "sqnorm"), (centroids, "centroids"), (centroid_sqnorm, "centroid_sqnorm")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            _dev(t if isinstance(t, torch.Tensor) else 0, name)
    tp, ld = _rowmajor(table, "table")
    n, d = table.shape
    if d % 4 != 0 or not 4 <= d <= KNN_MAX_D:
        raise ValueError("elimrec_amd.ops.%s: the table needs d %% 4 == 0 and 4 <= d <= %d columns, got %d" % (who, KNN_MAX_D, d))
    sp = _dev(sqnorm, "sqnorm")
    if sqnorm.dim() != 1 or sqnorm.numel() != n or sqnorm.device != table.device:
        raise ValueError("elimrec_amd.ops.%s: sqnorm must be 1-D with one entry per table row (%d) on the table's device" % (who, n))
    max_c = int(_lib.load().elimrec_kmeans_max_clusters())
    cp, qp = _dev(centroids, "centroids"), _dev(centroid_sqnorm, "centroid_sqnorm")
    if (centroids.dim() != 2 or centroids.shape[1] != d or not 1 <= centroids.shape[0] <= max_c or not centroids.is_contiguous()
            or centroids.device != table.device):
        raise ValueError("elimrec_amd.ops.%s: centroids must be a contiguous float32 [C x %d] tensor on the table's device, 1 <= C <= %d, "
                         "got %s" % (who, d, max_c, tuple(centroids.shape)))
    C = centroids.shape[0]
    if centroid_sqnorm.dim() != 1 or centroid_sqnorm.numel() != C or not centroid_sqnorm.is_contiguous() or centroid_sqnorm.device != table.device:
        raise ValueError("elimrec_amd.ops.%s: centroid_sqnorm must be a contiguous 1-D float32 tensor with one entry per centroid (%d) on "
                         "the table's device" % (who, C))
    return tp, ld, n, d, sp, max(1, int(sqnorm.stride(0))), cp, qp, C


def _kmeans_rows(who, t, name, dtype, n, device):
    """Device pointer of a contiguous 1-D tensor with one entry per table row."""
    p = _dev(t, name, dtype)
    if t.dim() != 1 or t.numel() != n or not t.is_contiguous() or t.device != device:
        raise ValueError("elimrec_amd.ops.%s: %s must be a contiguous 1-D tensor with one entry per table row (%d) on the table's device"
                         % (who, name, n))
    return p


def kmeans_assign(table, sqnorm, centroids, centroid_sqnorm, out_assign, out_cos=None, prev=None):
    """elimrec_kmeans_assign: out_assign int32 [n] <- per row of `table` the centroid with the largest cosine, the lowest id among
    equal cosines; out_cos float32 [n] (optional) <- that cosine, (dot * 1 / max(|row|, 1e-12)) * 1 / max(|centroid|, 1e-12) as
    cosine_topk forms it. table [n x d] float32 with unit column stride (a column block of a wider matrix is fine), d % 4 == 0,
    4 <= d <= 256; sqnorm 1-D float32, n entries, any stride; centroids float32 [C x d] contiguous with their squared norms
    centroid_sqnorm [C], 1 <= C <= KMEANS_MAX_CLUSTERS. A row whose squared norm is 0 or not finite gets -1 / -inf; a centroid whose
    squared norm is 0 or not finite is never chosen. -> changed: the number of rows whose assignment differs from prev (int32 [n],
    optional; without it every row counts, so changed == n) -- ONE integer read back from the device (a synchronisation). A row's
    bits depend on that row, the centroids, d and C alone (csrc/kmeans.hip)."""
    who = "kmeans_assign"
    tp, ld, n, d, sp, ld_sq, cp, qp, C = _kmeans_table(who, table, sqnorm, centroids, centroid_sqnorm)
    dev = table.device
    if out_assign is None:
        raise RuntimeError("elimrec_amd.ops: 'out_assign' must be a HIP device tensor (the hot path has no CPU implementation)")
    ap = _kmeans_rows(who, out_assign, "out_assign", torch.int32, n, dev)
    op = _kmeans_rows(who, out_cos, "out_cos", torch.float32, n, dev) if out_cos is not None else None
    pp = _kmeans_rows(who, prev, "prev", torch.int32, n, dev) if prev is not None else None
    if n == 0:
        return 0
    changed = torch.empty(1, dtype=torch.int32, device=dev)
    _lib.check(_lib.load().elimrec_kmeans_assign(tp, ld, n, d, sp, ld_sq, cp, qp, C, pp, ap, op, changed.data_ptr(), _stream()), who)
    return int(changed.item())


def kmeans_update(table, sqnorm, assign, centroids, centroid_sqnorm, out_sums=None, out_counts=None, workspace=None):
    """elimrec_kmeans_update: centroids float32 [C x d] and centroid_sqnorm float32 [C] are updated IN PLACE: centroid c <- the float64
    sum of the unit rows x / max(|x|, 1e-12) (formed in fp32, as kmeans_assign sees them) of the rows with assign[r] == c, divided by
    its float64 norm and rounded once; centroid_sqnorm[c] <- its squared norm. A cluster without a member, or whose sum has norm 0,
    keeps both. assign int32 [n]: entries outside [0, C) are skipped, and so is a row whose squared norm is 0 or not finite. The sums
    are formed over KMEANS_SEGMENT consecutive rows in row order and added in segment order, no floating-point atomics: the bits
    depend on the table, assign, d and C alone. out_sums float64 [C x d] / out_counts int32 [C] (optional, contiguous) <- the sums and
    the members. workspace: uint8 device tensor of at least kmeans_workspace(n, d, C) bytes, 16-byte aligned (default: allocated
    here). -> centroids (csrc/kmeans.hip)."""
    who = "kmeans_update"
    tp, ld, n, d, sp, ld_sq, cp, qp, C = _kmeans_table(who, table, sqnorm, centroids, centroid_sqnorm)
    dev = table.device
    ap = _kmeans_rows(who, assign, "assign", torch.int32, n, dev)
    up = kp = None
    if out_sums is not None:
        up = _dev(out_sums, "out_sums", torch.float64)
        if tuple(out_sums.shape) != (C, d) or not out_sums.is_contiguous() or out_sums.device != dev:
            raise ValueError("elimrec_amd.ops.kmeans_update: out_sums must be a contiguous float64 [%d x %d] tensor on the table's device" % (C, d))
    if out_counts is not None:
        kp = _dev(out_counts, "out_counts", torch.int32)
        if tuple(out_counts.shape) != (C,) or not out_counts.is_contiguous() or out_counts.device != dev:
            raise ValueError("elimrec_amd.ops.kmeans_update: out_counts must be a contiguous int32 [%d] tensor on the table's device" % C)
    need = kmeans_workspace(n, d, C)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    wp = _dev(workspace, "workspace", torch.uint8)
    if workspace.numel() < need or not workspace.is_contiguous() or wp % 16:
        raise ValueError("elimrec_amd.ops.kmeans_update: the workspace needs %d contiguous bytes, 16-byte aligned (got %d)"
                         % (need, workspace.numel()))
    if n == 0:                                                       # no member anywhere: every cluster keeps its centroid
        if out_sums is not None:
            out_sums.zero_()
        if out_counts is not None:
            out_counts.zero_()
        return centroids
    _lib.check(_lib.load().elimrec_kmeans_update(tp, ld, n, d, sp, ld_sq, ap, C, cp, qp, up, kp, wp, workspace.numel(), _stream()), who)
    return centroids


KMeans = collections.namedtuple("KMeans", ("assign", "cos", "centroids", "counts", "n_iter", "converged", "cohesion"))


def _kmeans_params(who, C, iters):
    """(C, iters) as integers in range; checked before anything touches the device."""
    for what, v in (("the number of clusters", C), ("iters", iters)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError("elimrec_amd.ops.%s: %s must be an integer, got %r" % (who, what, v))
    if not 1 <= int(C) <= 256:                                       # KMEANS_MAX_CLUSTERS (csrc/kmeans.hip), known without the library
        raise ValueError("elimrec_amd.ops.%s: 1 <= C <= 256 clusters, got %d" % (who, C))
    if int(iters) < 1:
        raise ValueError("elimrec_amd.ops.%s: iters >= 1, got %d" % (who, iters))
    return int(C), int(iters)


def spherical_kmeans(table, sqnorm, C, iters=25, seed=2022, init=None):
    """Spherical k-means (Lloyd's loop on the device) of the rows of `table` -- as kmeans_assign takes it, with its squared norms --
    into C clusters by cosine: KMeans(assign int32 [n], cos float32 [n], centroids float32 [C x d], counts int32 [C] -- device
    tensors --, n_iter, converged, cohesion). init: C distinct row indices whose rows are the first centroids; default the first C
    entries of np.random.default_rng(seed).permutation(rows with a finite, non-zero squared norm), drawn on the host (fewer than C
    such rows: ValueError). Iteration i = 1, 2, ... is ONE kmeans_assign against the centroids of iteration i - 1 (the init rows
    for i = 1), the read of its one `changed` integer, and -- unless it is 0 -- ONE kmeans_update. The loop stops when no assignment
    changed (converged = True: the update is skipped, the centroids ARE the normalised sums of the returned assignment) or after
    `iters` iterations (converged = False: assign and cos belong to the PREDECESSORS of the returned centroids, which are the
    normalised sums of the returned assignment). n_iter = the assign launches made; counts = the members of the returned
    assignment. A row whose squared norm is 0 or not finite belongs to no cluster (-1 / -inf); a cluster that loses every member
    keeps its centroid. cohesion = the float64 mean of cos over the assigned rows, summed on the host in numpy's fixed pairwise
    order (NaN without an assigned row). Same table, C, iters and init: same bits."""
    who = "spherical_kmeans"
    C, iters = _kmeans_params(who, C, iters)
    if not isinstance(table, torch.Tensor) or not table.is_cuda:
        _dev(table if isinstance(table, torch.Tensor) else 0, "table")
    if table.dim() != 2:
        raise ValueError("elimrec_amd.ops.spherical_kmeans: 'table' must be 2-D with unit column stride")
    n, d = table.shape
    dev = table.device
    if d % 4 != 0 or not 4 <= d <= KNN_MAX_D:
        raise ValueError("elimrec_amd.ops.spherical_kmeans: the table needs d %% 4 == 0 and 4 <= d <= %d columns, got %d" % (KNN_MAX_D, d))
    _dev(sqnorm, "sqnorm")
    if sqnorm.dim() != 1 or sqnorm.numel() != n or sqnorm.device != dev:
        raise ValueError("elimrec_amd.ops.spherical_kmeans: sqnorm must be 1-D with one entry per table row (%d) on the table's device" % n)
    if init is None:
        sq = sqnorm.detach().cpu().numpy()
        good = np.flatnonzero(np.isfinite(sq) & (sq > 0))
        if good.size < C:
            raise ValueError("elimrec_amd.ops.spherical_kmeans: %d clusters need as many rows with a finite, non-zero norm, the table "
                             "has %d" % (C, good.size))
        init = good[np.random.default_rng(seed).permutation(good.size)[:C]]
    init = np.asarray(init)
    if init.ndim != 1 or init.size != C or init.dtype.kind not in "iu" or (C and not 0 <= int(init.min()) <= int(init.max()) < n):
        raise ValueError("elimrec_amd.ops.spherical_kmeans: init must hold %d row indices in [0, %d)" % (C, n))
    rows = torch.from_numpy(init.astype(np.int64)).to(dev)
    centroids = table.index_select(0, rows).contiguous()
    csq = sqnorm.index_select(0, rows).contiguous()
    assign = [torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2)]
    cos = torch.empty(n, dtype=torch.float32, device=dev)
    counts = torch.empty(C, dtype=torch.int32, device=dev)
    workspace = torch.empty(kmeans_workspace(n, d, C), dtype=torch.uint8, device=dev)
    n_iter, converged, cur = 0, False, 0
    for it in range(iters):
        cur = it & 1
        changed = kmeans_assign(table, sqnorm, centroids, csq, assign[cur], cos, prev=assign[1 - cur] if it else None)
        n_iter += 1
        if it and changed == 0:
            converged = True
            break
        kmeans_update(table, sqnorm, assign[cur], centroids, csq, out_counts=counts, workspace=workspace)
    a_host, c_host = assign[cur].cpu().numpy(), cos.cpu().numpy()
    listed = a_host >= 0
    cohesion = float(c_host[listed].astype(np.float64).sum() / listed.sum()) if listed.any() else float("nan")
    return KMeans(assign[cur], cos, centroids, counts, n_iter, converged, cohesion)


GEOMETRY_MAX_T = 8.0                     # the largest temperature uniformity_sum takes (csrc/geometry.hip), known without the library


def uniformity_workspace(n, d):
    """Bytes of workspace uniformity_sum needs for a list of n entries (host arithmetic only; 0 for arguments out of range)."""
    return int(_lib.load().elimrec_uniformity_workspace(int(n), int(d)))


def row_gram_workspace(n, d):
    """Bytes of workspace row_gram needs for a list of n entries (host arithmetic only; 0 for arguments out of range)."""
    return int(_lib.load().elimrec_gram_workspace(int(n), int(d)))


def _geometry_t(who, t):
    """The temperature as a float in (0, GEOMETRY_MAX_T]; checked before anything touches the device."""
    if isinstance(t, bool) or not isinstance(t, (int, float, np.integer, np.floating)) or not 0.0 < float(t) <= GEOMETRY_MAX_T:
        raise ValueError("elimrec_amd.ops.%s: 0 < t <= %g, got %r" % (who, GEOMETRY_MAX_T, t))
    return float(t)


def _geometry_table(who, table, sqnorm, rows):
    """The checks uniformity_sum / row_gram share, cosine_topk's -> (table pointer, ld, n_rows, d, norm pointer, norm ld, rows
    pointer, n). rows: an int32 device tensor, 1-D and contiguous; its ids are checked by the kernel, entry by entry."""
    for t, name in ((table, "table"), (sqnorm, "sqnorm"), (rows, "rows")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            _dev(t if isinstance(t, torch.Tensor) else 0, name)
    tp, ld = _rowmajor(table, "table")
    n_rows, d = table.shape
    if d % 4 != 0 or not 4 <= d <= KNN_MAX_D:
        raise ValueError("elimrec_amd.ops.%s: the table needs d %% 4 == 0 and 4 <= d <= %d columns, got %d" % (who, KNN_MAX_D, d))
    sp = _dev(sqnorm, "sqnorm")
    if sqnorm.dim() != 1 or sqnorm.numel() != n_rows or sqnorm.device != table.device:
        raise ValueError("elimrec_amd.ops.%s: sqnorm must be 1-D with one entry per table row (%d) on the table's device" % (who, n_rows))
    rp = _dev(rows, "rows", torch.int32)
    if rows.dim() != 1 or not rows.is_contiguous() or rows.device != table.device:
        raise ValueError("elimrec_amd.ops.%s: rows must be a contiguous 1-D int32 tensor on the table's device" % who)
    return tp, ld, n_rows, d, sp, max(1, int(sqnorm.stride(0))), rp, rows.numel()


def _geometry_workspace(who, workspace, need, dev):
    if workspace is None:
        workspace = torch.empty(max(16, need), dtype=torch.uint8, device=dev)
    wp = _dev(workspace, "workspace", torch.uint8)
    if workspace.numel() < need or not workspace.is_contiguous() or wp % 16:
        raise ValueError("elimrec_amd.ops.%s: the workspace needs %d contiguous bytes, 16-byte aligned (got %d)" % (who, need, workspace.numel()))
    return workspace, wp


def uniformity_sum_device(table, sqnorm, rows, t=2.0, workspace=None):
    """uniformity_sum without the read back: (S float64 [1], counts int64 [2] = (pairs, n_valid)) on the device."""
    who = "uniformity_sum"
    t = _geometry_t(who, t)
    tp, ld, n_rows, d, sp, ld_sq, rp, n = _geometry_table(who, table, sqnorm, rows)
    dev = table.device
    workspace, wp = _geometry_workspace(who, workspace, uniformity_workspace(n, d), dev)
    S = torch.empty(1, dtype=torch.float64, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    _lib.check(_lib.load().elimrec_uniformity_sum(tp, ld, n_rows, d, sp, ld_sq, rp, n, t, S.data_ptr(), counts.data_ptr(), wp,
                                                  workspace.numel(), _stream()), who)
    return S, counts


def uniformity_sum(table, sqnorm, rows, t=2.0, workspace=None):
    """elimrec_uniformity_sum: the all-pairs sum of the uniformity term of Wang & Isola (ICML'20) over a LIST of rows of `table`:
    -> (S, pairs, n_valid), S = the float64 sum over the list's positions p < q, both valid, of expf(2 t (cos(p, q) - 1)),
    pairs = n_valid (n_valid - 1) / 2; the uniformity is log(S / pairs) (uniformity_value). table [n_rows x d] float32 with unit column
    stride (a column block of a wider matrix is fine), d % 4 == 0, 4 <= d <= 256; sqnorm: 1-D float32, n_rows entries, any stride.
    rows: int32 device tensor [n], contiguous: an entry is valid when its id lies in [0, n_rows) and its row's squared norm is
    > 0 and finite -- any other entry (-1, an id past the table, a row without a norm) is skipped by the kernel and missing from
    n_valid; a repeated id is an entry of its own. 0 < t <= 8. The cosine is cosine_topk's, (dot * inv_lo) * inv_hi on the fp32
    matrix cores with the two reciprocal norms in ascending order, so a pair's term does not depend on which row comes first and
    the reversed list differs by the order of the float64 additions alone; every term is widened to float64 before it is added, in an order fixed by n, GEOMETRY_TILE and GEOMETRY_CHUNK
    alone, without floating-point atomics: two calls give the same bits. workspace: uint8 device tensor of at least
    uniformity_workspace(n, d) bytes, 16-byte aligned (default: allocated here). The three numbers are read back (a
    synchronisation); uniformity_sum_device leaves them on the device (csrc/geometry.hip)."""
    S, counts = uniformity_sum_device(table, sqnorm, rows, t, workspace)
    counts = counts.cpu()
    return float(S.cpu().item()), int(counts[0]), int(counts[1])


def uniformity_value(S, pairs):
    """log(S / pairs) in float64; NaN with fewer than two valid rows."""
    return float(np.log(np.float64(S) / np.float64(pairs))) if pairs > 0 and S > 0 else float("nan")


def row_gram_device(table, sqnorm, rows, out_gram=None, out_sum=None, workspace=None):
    """row_gram without the read back: (G, m, n_valid int64 [1]) on the device."""
    who = "row_gram"
    tp, ld, n_rows, d, sp, ld_sq, rp, n = _geometry_table(who, table, sqnorm, rows)
    dev = table.device
    for out, name, shape in ((out_gram, "out_gram", (d, d)), (out_sum, "out_sum", (d,))):
        if out is not None:
            _dev(out, name, torch.float64)
            if tuple(out.shape) != shape or not out.is_contiguous() or out.device != dev:
                raise ValueError("elimrec_amd.ops.row_gram: %s must be a contiguous float64 %s tensor on the table's device"
                                 % (name, " x ".join(str(x) for x in shape).join("[]")))
    workspace, wp = _geometry_workspace(who, workspace, row_gram_workspace(n, d), dev)
    G = out_gram if out_gram is not None else torch.empty(d, d, dtype=torch.float64, device=dev)
    m = out_sum if out_sum is not None else torch.empty(d, dtype=torch.float64, device=dev)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    _lib.check(_lib.load().elimrec_gram_f64(tp, ld, n_rows, d, sp, ld_sq, rp, n, G.data_ptr(), m.data_ptr(), count.data_ptr(), wp,
                                            workspace.numel(), _stream()), who)
    return G, m, count


def row_gram(table, sqnorm, rows, out_gram=None, out_sum=None, workspace=None):
    """elimrec_gram_f64: -> (G float64 [d x d], m float64 [d] -- device tensors --, n_valid): G = the sum of x^ x^T and m = the sum
    of x^ over the valid entries of the list `rows`, x^ = x / max(|x|, 1e-12) formed in fp32 (as uniformity_sum and cosine_topk see
    the rows) and widened: every product is exact in float64. They are added over segments of GEOMETRY_SEGMENT consecutive list
    positions in list order and the partials in segment order, no floating-point atomics; the upper triangle is computed and
    mirrored, so G is exactly symmetric. table / sqnorm / rows as uniformity_sum takes them. out_gram / out_sum: contiguous
    float64 outputs (default: allocated here); workspace: uint8 device tensor of at least row_gram_workspace(n, d) bytes, 16-byte
    aligned (default: allocated here). n_valid is read back (a synchronisation); row_gram_device leaves it on the device. The
    covariance's spectrum is reports.spectrum_summary(G, m, n_valid) (csrc/geometry.hip)."""
    G, m, count = row_gram_device(table, sqnorm, rows, out_gram, out_sum, workspace)
    return G, m, int(count.cpu().item())


def _block_table(table, sqnorm, blocks, name, who):
    """(pointer, ld, rows, d, norm pointer, norm ld) of a [rows x blocks * d] table with its [rows x blocks] squared norms, as
    list_pair_cosine takes the pair."""
    if not isinstance(table, torch.Tensor) or not isinstance(sqnorm, torch.Tensor):
        raise RuntimeError("elimrec_amd.ops: '%s' and its sqnorm must be HIP device tensors (the hot path has no CPU implementation)" % name)
    if table.dim() != 2 or table.stride(1) != 1:
        raise ValueError("elimrec_amd.ops.%s: %s must be 2-D with unit column stride" % (who, name))
    rows, width = table.shape
    if width % blocks != 0:
        raise ValueError("elimrec_amd.ops.%s: the %d columns of %s do not split into %d equal blocks" % (who, width, name, blocks))
    d = width // blocks
    if d % 4 != 0 or not 4 <= d <= KNN_MAX_D:
        raise ValueError("elimrec_amd.ops.%s: a block needs d %% 4 == 0 and 4 <= d <= %d columns, got %d" % (who, KNN_MAX_D, d))
    if sqnorm.dim() == 1 and blocks == 1 and sqnorm.numel() == rows:
        ld_sq = max(1, int(sqnorm.stride(0)))
    elif sqnorm.dim() == 2 and tuple(sqnorm.shape) == (rows, blocks) and (sqnorm.stride(1) == 1 or blocks == 1):
        ld_sq = max(blocks, int(sqnorm.stride(0)))
    else:
        raise ValueError("elimrec_amd.ops.%s: the sqnorm of %s must be [%d x %d] with unit column stride (or 1-D with %d entries when "
                         "blocks == 1)" % (who, name, rows, blocks, rows))
    if sqnorm.device != table.device:
        raise ValueError("elimrec_amd.ops.%s: the sqnorm of %s must live on its device" % (who, name))
    tp, ld = _rowmajor(table, name)
    return tp, ld, rows, d, _dev(sqnorm, name + " sqnorm"), ld_sq


def _weights(weights, who):
    """(blocks, c_float[blocks]) of a host sequence of block weights."""
    w = [float(x) for x in (weights.tolist() if hasattr(weights, "tolist") else weights)]
    if not 1 <= len(w) <= LIST_MAX_BLOCKS:
        raise ValueError("elimrec_amd.ops.%s: weights needs 1 <= blocks <= %d entries, got %d" % (who, LIST_MAX_BLOCKS, len(w)))
    return len(w), (ctypes.c_float * len(w))(*w)


def _users_beside(users, lists, name, dev, where, who):
    """Device pointer of users int64 [n] beside `lists` ([n x .], called `name`), both on `dev` (`where` in the message)."""
    p = _dev(users, "users", torch.int64)
    n = lists.shape[0]
    if users.dim() != 1 or users.numel() != n or not users.is_contiguous() or users.device != dev or lists.device != dev:
        raise ValueError("elimrec_amd.ops.%s: users must be a contiguous [%d] tensor, one per row of %s, both on the %s device"
                         % (who, n, name, where))
    return p


def pick_hard_negatives(user_table, user_sqnorm, item_table, item_sqnorm, weights, users, cands, out_neg, out_pos=None, out_score=None):
    """elimrec_pick_hard_negatives: per triplet the candidate the tables score highest. user_table [U x blocks * d] / item_table
    [I x blocks * d] float32 with unit column stride (column slices of wider matrices are fine), block b = columns
    [b * d, (b + 1) * d), d % 4 == 0, 4 <= d <= 256; user_sqnorm [U x blocks] / item_sqnorm [I x blocks] with unit column stride
    (1-D with any stride when blocks == 1): the rows' squared norms per block (row_sqnorms' table or a slice of it). weights: a HOST
    sequence of 1 <= blocks <= 8 floats; score(u, i) = sum_b weights[b] * cos_b(u, i) over the blocks with a non-zero weight, in
    block order -- a block with zero weight is not read. users int64 [n], cands int32 [n x M] contiguous, 1 <= M <=
    HARD_NEG_MAX_CANDIDATES, on the tables' device: a candidate outside [0, I) is not listed (the kernel checks every entry, no host
    check is needed). out_neg int64 [n] <- the id of the listed candidate with the largest score, the lowest column among equals;
    out_pos int32 [n] (optional) its column, out_score float32 [n] (optional) its score; -1 / -1 / -inf for a row with no listed
    candidate or a user outside [0, U). Outputs: contiguous 1-D with at least n entries; entries beyond n are left alone. A
    triplet's bits depend on its rows, d, blocks and weights alone (csrc/hardneg.hip)."""
    blocks, wp = _weights(weights, "pick_hard_negatives")
    up, ld_u, U, d, squ, ldsq_u = _block_table(user_table, user_sqnorm, blocks, "user_table", "pick_hard_negatives")
    ip, ld_i, I, d_i, sqi, ldsq_i = _block_table(item_table, item_sqnorm, blocks, "item_table", "pick_hard_negatives")
    if d_i != d or item_table.device != user_table.device:
        raise ValueError("elimrec_amd.ops.pick_hard_negatives: the two tables need one block width and one device")
    cp = _int_lists(cands, "cands", "pick_hard_negatives")
    n, M = cands.shape
    if not 1 <= M <= HARD_NEG_MAX_CANDIDATES:
        raise ValueError("elimrec_amd.ops.pick_hard_negatives: 1 <= M <= %d, got %d" % (HARD_NEG_MAX_CANDIDATES, M))
    dev = user_table.device
    usp = _users_beside(users, cands, "cands", dev, "tables'", "pick_hard_negatives")
    np_ = _rows_out(out_neg, "out_neg", torch.int64, n, 1, "pick_hard_negatives", device=dev)
    pp = _rows_out(out_pos, "out_pos", torch.int32, n, 1, "pick_hard_negatives", device=dev) if out_pos is not None else None
    sp = _rows_out(out_score, "out_score", torch.float32, n, 1, "pick_hard_negatives", device=dev) if out_score is not None else None
    if n == 0:
        return out_neg
    _lib.check(_lib.load().elimrec_pick_hard_negatives(up, ld_u, U, squ, ldsq_u, ip, ld_i, I, sqi, ldsq_i, blocks, d,
                                                       wp, usp, cp, n, M, np_, pp, sp, _stream()),
               "pick_hard_negatives")
    return out_neg


class HistoryIndex(object):
    """The users' histories as CSR (ptr [n_rows + 1], items: item ids), CHECKED ON THE HOST -- at least two entries of ptr,
    ptr[0] = 0, ascending, ptr[n_rows] = len(items), integer ids that fit int32 -- and then resident on `device`: history_support
    takes it as is, call after call (the counterpart of TargetIndex). n_items = None: the ids' range is left to the kernel, which
    checks every entry and never dereferences one outside its table; n_items = I: every id must lie in [0, I) (IndexError).
    Segments may repeat ids, in any order, and may be empty."""

    def __init__(self, ptr, items, device, n_items=None):
        p, it = _checked_csr(ptr, items, None, n_items, "HistoryIndex",
                             ("ptr", "items", "n_rows", "item ids span [%d, %d], the catalogue has %d items"))
        if it.size and (int(it.min()) < -2 ** 31 or int(it.max()) >= 2 ** 31):
            raise IndexError("elimrec_amd.ops.HistoryIndex: item ids span [%d, %d]: they must fit int32" % (int(it.min()), int(it.max())))
        self.n_rows, self.n_items, self.n_entries = int(p.size - 1), (None if n_items is None else int(n_items)), int(it.size)
        self.sizes = np.diff(p)
        self.ptr = torch.from_numpy(p).to(device)
        self.items = _resident_ids(it, device)


def history_columns(mods):
    """Column names of the history report: per space (fused, then the heads' modality letters in head order) sup_max_<space> (the
    largest score of a history entry against the listed item), sup_mean_<space> (the mean over the history) and unexpected_<space>
    (1 - sup_max_<space>), then hist_n (the number of history entries behind the pair)."""
    spaces = ("fused",) + tuple(str(m) for m in mods)
    return (tuple("sup_max_" + s for s in spaces) + tuple("sup_mean_" + s for s in spaces)
            + tuple("unexpected_" + s for s in spaces) + ("hist_n",))


def _flat_out(t, name, dtype, n, who, device):
    """Device pointer of an output of n entries: `dtype`, contiguous, any shape with at least n entries, on `device`."""
    if t is None:
        raise RuntimeError("elimrec_amd.ops: '%s' must be a HIP device tensor (the hot path has no CPU implementation)" % name)
    p = _dev(t, name, dtype)
    if not t.is_contiguous() or t.device != device or t.numel() < n:
        raise ValueError("elimrec_amd.ops.%s: %s must be contiguous on the table's device with at least %d entries" % (who, name, n))
    return p


def history_support(table, sqnorm, weights, users, lists, hist, top, out_idx, out_val, out_cnt=None, out_mean=None, exclude_self=True):
    """elimrec_history_support: per (row b, target lists[b, k]) the entries of user users[b]'s history that score highest against
    the target. table [I x blocks * d] float32 with unit column stride (a column slice of a wider matrix is fine), block b = columns
    [b * d, (b + 1) * d), d % 4 == 0, 4 <= d <= 256; sqnorm [I x blocks] with unit column stride (1-D with any stride when blocks
    == 1): the rows' squared norms per block; weights: a HOST sequence of 1 <= blocks <= 8 floats, score(j, i) = sum_b weights[b] *
    cos_b(j, i) over the blocks with a non-zero weight, in block order -- a block with zero weight is not read (pick_hard_negatives'
    expression). users int64 [B], lists int32 [B x K] contiguous, 1 <= K <= LIST_MAX_K, on the table's device; hist: a HistoryIndex
    on that device, users[b] names its segment. A target is listed when its id lies in [0, I) and its user in [0, hist.n_rows); an
    entry when its id lies in [0, I) and, with exclude_self, differs from the target (the kernel checks every id, no host check is
    needed); a repeated id is an entry of its own. 1 <= top <= HISTORY_MAX_TOP. out_idx int32 / out_val float32 [B x K x top] <- the
    ids and scores of the `top` listed entries with the largest score, in that order, the lower position in the segment first among
    equals, -1 / -inf where fewer exist or the target is not listed; out_cnt int32 / out_mean float32 [B x K] (optional) <- the
    number of listed entries and their mean score (float64 sum in segment order, rounded once), 0 / NaN without one. Outputs:
    contiguous with at least B * K * top (B * K) entries; entries beyond are left alone. A pair's bits depend on the target's row,
    the segment in order, d, blocks, weights, top and exclude_self alone (csrc/history.hip)."""
    blocks, wp = _weights(weights, "history_support")
    if not isinstance(hist, HistoryIndex):
        raise TypeError("elimrec_amd.ops.history_support: hist must be an ops.HistoryIndex, got %s" % type(hist).__name__)
    if isinstance(top, bool) or not isinstance(top, (int, np.integer)):
        raise ValueError("elimrec_amd.ops.history_support: top must be an integer, got %r" % (top,))
    top = int(top)
    max_top = int(_lib.load().elimrec_history_max_top())
    if not 1 <= top <= max_top:
        raise ValueError("elimrec_amd.ops.history_support: 1 <= top <= %d, got %d" % (max_top, top))
    tp, ld, I, d, sqp, ld_sq = _block_table(table, sqnorm, blocks, "table", "history_support")
    lp = _int_lists(lists, "lists", "history_support")
    B, K = lists.shape
    if K > LIST_MAX_K:
        raise ValueError("elimrec_amd.ops.history_support: 1 <= K <= %d, got %d" % (LIST_MAX_K, K))
    dev = table.device
    up = _users_beside(users, lists, "lists", dev, "table's", "history_support")
    if hist.ptr.device != dev:
        raise ValueError("elimrec_amd.ops.history_support: the HistoryIndex lives on %s, the table on %s" % (hist.ptr.device, dev))
    ip = _flat_out(out_idx, "out_idx", torch.int32, B * K * top, "history_support", dev)
    vp = _flat_out(out_val, "out_val", torch.float32, B * K * top, "history_support", dev)
    cp = _flat_out(out_cnt, "out_cnt", torch.int32, B * K, "history_support", dev) if out_cnt is not None else None
    mp = _flat_out(out_mean, "out_mean", torch.float32, B * K, "history_support", dev) if out_mean is not None else None
    if B == 0:
        return out_idx
    _lib.check(_lib.load().elimrec_history_support(tp, ld, I, blocks, d, sqp, ld_sq, wp, up, lp, B, K,
                                                   _dev(hist.ptr, "hist_ptr", torch.int64), _dev(hist.items, "hist_items", torch.int32),
                                                   hist.n_rows, top, 1 if exclude_self else 0, ip, vp, cp, mp, _stream()),
               "history_support")
    return out_idx


COOCCUR_MAX_K = 256                      # the longest list cooccur_topk keeps (csrc/cooccur.hip), known without the library
COOCCUR_MEASURES = {"count": 0, "cosine": 1, "jaccard": 2}
COOCCUR_WORKSPACE_BUDGET = 1 << 30       # bytes cooccur_topk allocates for the dense form's counter rows at most (workspace=None)


# The two-form calls (cooccur_topk, walk_topk, neighbour_vote_topk; csrc/co_select.h) share one host front end. `family` is the
# middle of the library's symbols: elimrec_<family>_slots / _groups / _rows_in_lds / _workspace.

def _form_rows_in_lds(family, name, size):
    form = int(getattr(_lib.load(), "elimrec_%s_rows_in_lds" % family)(int(size)))
    if form < 0:
        raise ValueError("elimrec_amd.ops.%s_rows_in_lds: %s >= 0, got %d" % (family, name, size))
    return bool(form)


def _form_workspace(family, n_dense_rows, n):
    if n_dense_rows < 0 or not 0 <= n < 2 ** 31 - 1:
        raise ValueError("elimrec_amd.ops.%s_workspace: n_dense_rows >= 0 and 0 <= n < 2^31 - 1, got %d and %d" % (family, n_dense_rows, n))
    return int(getattr(_lib.load(), "elimrec_%s_workspace" % family)(int(n_dense_rows), int(n)))


def _form_k(who, K, max_k):
    if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or not 1 <= K <= max_k:
        raise ValueError("elimrec_amd.ops.%s: K must be an integer, 1 <= K <= %d, got %r" % (who, max_k, K))
    return int(K)


def _form_call(who, family, sizes, at, lds, n, K, outs, workspace, dev, where):
    """The back half of a two-form call, before anything is launched. sizes()[at]: the host's size of every row of the call (W of a
    walk, V of a vote), which picks its form -- a callable, asked only when rows take the LDS form; where: whose device `dev` is; n: the entries of a dense row; outs: (out_idx, out_val, out_cnt), the last two optional. -> None for a
    call without rows, else ((idx, val, cnt) device pointers, n_dense, the workspace tensor -- the caller holds it until its launch
    is queued): a default workspace is allocated and zeroed here under COOCCUR_WORKSPACE_BUDGET, a caller's is checked (ValueError)."""
    R = int(at.size)
    out_idx, out_val, out_cnt = outs
    ip = _rows_out(out_idx, "out_idx", torch.int32, R, K, who, dev)
    vp = _rows_out(out_val, "out_val", torch.float32, R, K, who, dev) if out_val is not None else None
    cp = _rows_out(out_cnt, "out_cnt", torch.int32, R, K, who, dev) if out_cnt is not None else None
    if R == 0:
        return None
    lib = _lib.load()
    n_dense = int((sizes()[at] > getattr(lib, "elimrec_%s_slots" % family)() // 2).sum()) if lds else R
    need = _form_workspace(family, n_dense, n)
    if workspace is None:
        if need > COOCCUR_WORKSPACE_BUDGET:
            raise ValueError("elimrec_amd.ops.%s: the dense form's rows need %d bytes (%d rows of %d entries), the budget is %d: pass a "
                             "workspace" % (who, need, min(n_dense, getattr(lib, "elimrec_%s_groups" % family)()), n, COOCCUR_WORKSPACE_BUDGET))
        workspace = torch.zeros(max(16, need), dtype=torch.uint8, device=dev)
    wp = _dev(workspace, "workspace", torch.uint8)
    if workspace.numel() < need or not workspace.is_contiguous() or wp % 16 or workspace.device != dev:
        raise ValueError("elimrec_amd.ops.%s: the workspace needs %d contiguous bytes on the %s device, 16-byte aligned (got %d)"
                         % (who, need, where, workspace.numel()))
    return (ip, vp, cp), n_dense, workspace


def cooccur_rows_in_lds(W):
    """Which form cooccur_topk takes for a query row whose walk is W = the sum of deg(u) over the row's segment (host arithmetic
    only): True = the LDS form (W <= COOCCUR_SLOTS / 2: the hash table's load factor is at most 0.5 whatever the ids are), False =
    the dense form. Both forms give the same bits. ValueError for W < 0."""
    return _form_rows_in_lds("cooccur", "W", W)


def cooccur_workspace(n_dense_rows, n):
    """Bytes of the dense form's counter rows for a call with n_dense_rows rows on that form over a query side of n rows (host
    arithmetic only): min(n_dense_rows, COOCCUR_GROUPS) int32 rows of n entries."""
    return _form_workspace("cooccur", n_dense_rows, n)


def _cooccur_measure(who, measure):
    if not isinstance(measure, str) or measure not in COOCCUR_MEASURES:
        raise ValueError("elimrec_amd.ops.%s: measure is one of %s, got %r" % (who, ", ".join(sorted(COOCCUR_MEASURES)), measure))
    return COOCCUR_MEASURES[measure]


class CooccurIndex(object):
    """One bipartite graph as two CSRs of the same edges, CHECKED ON THE HOST and then resident on `device`: q_ptr [n_query + 1] /
    q_nbr maps a row of the query side to its neighbours on the other side (for item queries: item -> its training users), o_ptr
    [n_other + 1] / o_nbr maps a row of the other side back (user -> items). Checked: the entry counts of the pointers, both
    ascending from 0 to the edge count, the two edge counts equal (ValueError); integer ids, q_nbr in [0, n_other) and o_nbr in
    [0, n_query) (IndexError). That o is q transposed is the caller's word -- the kernel needs only what is checked to stay within
    its arrays. A repeated edge is an edge of its own. cooccur_topk takes the index as is, call after call. Kept on the host:
    deg (the query side's degrees), deg_other (the other side's), walk (int64 [n_query]: W(q) = the sum of deg(u) over q's segment, which picks a row's form)
    and has_neighbour (bool [n_query]: one of the row's neighbours has degree >= 2, so some other row shares it)."""

    def __init__(self, q_ptr, q_nbr, o_ptr, o_nbr, n_query, n_other, device):
        who = "CooccurIndex"
        n_query, n_other = int(n_query), int(n_other)
        if not (0 <= n_query < 2 ** 31 - 1 and 0 <= n_other < 2 ** 31 - 1):
            raise ValueError("elimrec_amd.ops.%s: both sides need 0 <= rows < 2^31 - 1, got %d and %d" % (who, n_query, n_other))
        qp, qn = _checked_csr(q_ptr, q_nbr, n_query, n_other, who, ("q_ptr", "q_nbr", "n_query", "q_nbr spans [%d, %d], the other side has %d rows"))
        op, on = _checked_csr(o_ptr, o_nbr, n_other, n_query, who, ("o_ptr", "o_nbr", "n_other", "o_nbr spans [%d, %d], the query side has %d rows"))
        if qn.size != on.size:
            raise ValueError("elimrec_amd.ops.%s: the two CSRs hold the same edges, got %d and %d" % (who, qn.size, on.size))
        self.n_query, self.n_other, self.n_edges = n_query, n_other, int(qn.size)
        self.deg = np.diff(qp)
        self.deg_other = deg_o = np.diff(op)
        along = np.zeros(qn.size + 1, dtype=np.int64)
        np.cumsum(deg_o[qn], out=along[1:])
        self.walk = along[qp[1:]] - along[qp[:-1]]
        np.cumsum(deg_o[qn] >= 2, out=along[1:])
        self.has_neighbour = (along[qp[1:]] - along[qp[:-1]]) > 0
        self.device = torch.device(device)
        self.q_ptr, self.o_ptr = torch.from_numpy(qp).to(device), torch.from_numpy(op).to(device)
        self.q_nbr, self.o_nbr = _resident_ids(qn, device), _resident_ids(on, device)

    @classmethod
    def from_train(cls, user_train_dict, num_users, num_items, side, device):
        """The training graph: side "item" -- the rows are items, their neighbours the users who took them -- or "user" (the rows
        are users, co-counted over shared items). user_train_dict: user id -> that user's items."""
        if side not in ("item", "user"):
            raise ValueError("elimrec_amd.ops.CooccurIndex.from_train: side is 'item' or 'user', got %r" % (side,))
        U, I = int(num_users), int(num_items)
        if not isinstance(user_train_dict, dict):
            raise TypeError("user_train_dict must be a dict")
        if any(not 0 <= int(u) < U for u in user_train_dict):
            raise IndexError("user ids must lie in [0, %d)" % U)
        none = np.zeros(0, dtype=np.int64)
        up, ui, lens = ragged([user_train_dict.get(u, none) for u in range(U)], dtype=np.int64,
                              check=(I, "item ids must lie in [0, %d)" % I), cast=int)
        order = np.argsort(ui, kind="stable")
        ip = np.zeros(I + 1, dtype=np.int64)
        np.cumsum(np.bincount(ui, minlength=I), out=ip[1:])
        iu = np.repeat(np.arange(U, dtype=np.int64), lens)[order]
        if side == "item":
            return cls(ip, iu, up, ui, I, U, device)
        return cls(up, ui, ip, iu, U, I, device)


def _cooccur_rows(who, index, rows):
    """The query ids of a cooccur call: an ops.CooccurIndex, and rows as a flat host array checked against its side."""
    if not isinstance(index, CooccurIndex):
        raise TypeError("elimrec_amd.ops.%s: index must be an ops.CooccurIndex, got %s" % (who, type(index).__name__))
    return _checked_ids(rows, index.n_query, who, "rows", "query rows span [%d, %d], the side has %d rows")


def cooccur_walk(index, rows):
    """elimrec_cooccur_walk: int64 device tensor [Q] <- W(q) of every query row, the sum of deg(u) over the row's segment -- the
    number of 2-hop entries cooccur_topk walks for it, which alone picks its form (cooccur_rows_in_lds). rows: host array or tensor
    of ids, checked on the host (IndexError). index.walk holds the same numbers for every row, from the host's CSR."""
    q = _cooccur_rows("cooccur_walk", index, rows)
    out = torch.zeros(max(1, q.size), dtype=torch.int64, device=index.device)[:q.size]
    if q.size:
        _lib.check(_lib.load().elimrec_cooccur_walk(_dev(index.q_ptr, "q_ptr", torch.int64), _dev(index.q_nbr, "q_nbr", torch.int32),
                                                    index.n_query, _dev(index.o_ptr, "o_ptr", torch.int64), index.n_other,
                                                    _dev(_resident_ids(q, index.device), "rows", torch.int32), q.size, out.data_ptr(),
                                                    _stream()), "cooccur_walk")
    return out


def cooccur_topk(index, rows, K, out_idx, out_val=None, out_cnt=None, measure="cosine", lds=True, workspace=None):
    """elimrec_cooccur_topk: per query row q the K rows j != q of the same side that share the most neighbours with it -- "users who
    took this also took ...", the top-K of a row of A^T A (csrc/cooccur.hip). index: an ops.CooccurIndex. rows: host array or
    tensor of ids, checked on the host (IndexError; a synchronisation for a device tensor); a repeated id is a row of its own.
    c(q, j) = the number of two-step walks q -> u -> j (a repeated edge is an edge of its own: the product count), a = deg(q),
    b = deg(j). measure "count": float(c); "cosine": c / sqrt(a b); "jaccard": c / (a + b - c) -- the last two in float64 with IEEE
    sqrt and division, rounded once to fp32. Only c >= 1 is listed, never q itself. out_idx int32 / out_val float32 (optional) /
    out_cnt int32 (optional: the raw c) [Q x K] on the index's device <- the K best by (score descending, id ascending), -1 /
    -inf / 0 behind them; entries of the outputs beyond [Q x K] are left alone. 1 <= K <= COOCCUR_MAX_K = 256. A row with
    cooccur_rows_in_lds(index.walk[q]) takes the LDS form (a hash table of COOCCUR_SLOTS pairs), every other row -- with lds=False
    every row -- the dense form, whose counter rows live in `workspace`: a uint8 device tensor of at least cooccur_workspace(
    n_dense_rows, index.n_query) bytes, 16-byte aligned, ZERO before its first use (every call leaves it zero); default: allocated
    and zeroed here, at most COOCCUR_WORKSPACE_BUDGET bytes. A workspace that is too small, or a default past the budget, is a
    ValueError before any launch. Both forms give the same bits: a row's outputs depend on the graph, the row, K and the measure
    alone. Every argument error is raised before the device is touched. An empty `rows` returns without a launch."""
    who = "cooccur_topk"
    K = _form_k(who, K, COOCCUR_MAX_K)
    m = _cooccur_measure(who, measure)
    q = _cooccur_rows(who, index, rows)
    Q, dev = int(q.size), index.device
    call = _form_call(who, "cooccur", lambda: index.walk, q, lds, index.n_query, K, (out_idx, out_val, out_cnt), workspace, dev, "index's")
    if call is None:
        return out_idx
    (ip, vp, cp), n_dense, ws = call
    walk = torch.empty(Q, dtype=torch.int64, device=dev)
    _lib.check(_lib.load().elimrec_cooccur_topk(_dev(index.q_ptr, "q_ptr", torch.int64), _dev(index.q_nbr, "q_nbr", torch.int32), index.n_query,
                                                _dev(index.o_ptr, "o_ptr", torch.int64), _dev(index.o_nbr, "o_nbr", torch.int32), index.n_other,
                                                _dev(_resident_ids(q, dev), "rows", torch.int32), Q, K, m, 1 if lds else 0, n_dense,
                                                walk.data_ptr(), ip, vp, cp, ws.data_ptr(), ws.numel(), _stream()), who)
    return out_idx


WALK_MAX_K = 256                         # the longest list walk_topk keeps (csrc/walk.hip), known without the library
WALK_FRAC_BITS = 40                      # fraction bits of a walk's fixed-point weight: mid_weight = rint(weight * 2^40)
WALK_SLOTS = 4096                        # (key, sum) entries of the LDS form's table of walk_topk: W <= WALK_SLOTS / 2 takes that form


def walk_rows_in_lds(W):
    """Which form walk_topk takes for a query row whose walk is W = the sum of deg(u) over the row's segment (index.walk,
    cooccur_walk; host arithmetic only): True = the LDS form (W <= WALK_SLOTS / 2), False = the dense form. Both forms give the
    same bits. ValueError for W < 0."""
    return _form_rows_in_lds("walk", "W", W)


def walk_workspace(n_dense_rows, n):
    """Bytes of the dense form's rows for a call with n_dense_rows rows on that form over a query side of n rows (host arithmetic
    only): min(n_dense_rows, 512) rows of n int64 sums."""
    return _form_workspace("walk", n_dense_rows, n)


class WalkWeights(object):
    """The three arrays of a weighted two-step walk (walk_topk), CHECKED ONCE ON THE HOST and then resident on `device`:
    mid_weight int64 [n_other], every entry >= 0 -- the weight of a walk through u in WALK_FRAC_BITS = 40 bit fixed point --,
    row_scale and col_scale float64 [n_query], finite and >= 0. An integer dtype for mid_weight and float64 for the scales, one
    dimension each, the scales of one length, else ValueError. Kept on the host: n_other, n_query, max_weight (a Python int) and
    max_scale = max(row_scale) * max(col_scale), which walk_topk's bounds use."""

    def __init__(self, mid_weight, row_scale, col_scale, device):
        who = "WalkWeights"
        w, r, c = _host(mid_weight), _host(row_scale), _host(col_scale)
        if w.ndim != 1 or not np.issubdtype(w.dtype, np.integer) or w.dtype == np.uint64:
            raise ValueError("elimrec_amd.ops.%s: mid_weight is a flat array of a signed integer dtype, got %s %s" % (who, w.dtype, w.shape))
        if r.ndim != 1 or c.ndim != 1 or r.dtype != np.float64 or c.dtype != np.float64 or r.shape != c.shape:
            raise ValueError("elimrec_amd.ops.%s: row_scale and col_scale are flat float64 arrays of one length, got %s %s and %s %s"
                             % (who, r.dtype, r.shape, c.dtype, c.shape))
        w = np.ascontiguousarray(w, dtype=np.int64)
        if w.size and int(w.min()) < 0:
            raise ValueError("elimrec_amd.ops.%s: mid_weight holds a negative weight (%d)" % (who, int(w.min())))
        for name, x in (("row_scale", r), ("col_scale", c)):
            if x.size and not (np.isfinite(x).all() and float(x.min()) >= 0.0):
                raise ValueError("elimrec_amd.ops.%s: %s is finite and >= 0 everywhere" % (who, name))
        self.n_other, self.n_query = int(w.size), int(r.size)
        self.max_weight = int(w.max()) if w.size else 0
        self.max_scale = (float(r.max()) * float(c.max())) if r.size else 0.0
        self.device = torch.device(device)
        pad = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x if x.size else np.zeros(1), dtype=dt)).to(self.device)
        self.mid_weight, self.row_scale, self.col_scale = pad(w, np.int64), pad(r, np.float64), pad(c, np.float64)


def _rp3_params(who, alpha, beta):
    """RP3beta's two exponents as floats: finite numbers in [0, 4], anything else is a ValueError."""
    for name, x in (("alpha", alpha), ("beta", beta)):
        if isinstance(x, bool) or not isinstance(x, (int, float, np.integer, np.floating)) or not (math.isfinite(x) and 0.0 <= x <= 4.0):
            raise ValueError("%s: %s is a finite number in [0, 4], got %r" % (who, name, x))
    return float(alpha), float(beta)


def rp3_weights(index, alpha, beta):
    """The ops.WalkWeights of P3alpha / RP3beta (Cooper et al. 2014, Paudel et al. 2016) over an ops.CooccurIndex, in numpy float64
    from the index's degrees: the walk q -> u -> j has probability (1 / deg(q))^alpha (1 / deg(u))^alpha, and the target pays
    deg(j)^-beta for its popularity. mid_weight[u] = rint(deg(u)^-alpha * 2^40), row_scale[q] = deg(q)^-alpha, col_scale[j] =
    deg(j)^-beta; a row of degree 0 gets 0 in all three. alpha and beta are finite numbers in [0, 4] (ValueError). alpha = beta =
    0 counts the walks: every weight is 2^40 and every scale 1."""
    if not isinstance(index, CooccurIndex):
        raise TypeError("elimrec_amd.ops.rp3_weights: index must be an ops.CooccurIndex, got %s" % type(index).__name__)
    alpha, beta = _rp3_params("elimrec_amd.ops.rp3_weights", alpha, beta)

    def power(deg, p):
        d = deg.astype(np.float64)
        return np.where(deg > 0, np.power(np.maximum(d, 1.0), -p), 0.0)

    mid = np.rint(power(index.deg_other, alpha) * 2.0 ** WALK_FRAC_BITS).astype(np.int64)
    return WalkWeights(mid, power(index.deg, alpha), power(index.deg, beta), index.device)


def _walk_bounds(who, index, q, weights):
    """The host's bounds of a walk call: the weights fit the index; the int64 sums cannot overflow; the scores stay in float64."""
    if not isinstance(weights, WalkWeights):
        raise TypeError("elimrec_amd.ops.%s: weights must be an ops.WalkWeights, got %s" % (who, type(weights).__name__))
    if weights.n_other != index.n_other or weights.n_query != index.n_query:
        raise ValueError("elimrec_amd.ops.%s: the index has %d query rows and %d rows on the other side, the weights %d scales and %d weights"
                         % (who, index.n_query, index.n_other, weights.n_query, weights.n_other))
    if weights.device != index.device:
        raise ValueError("elimrec_amd.ops.%s: the index lives on %s, the weights on %s" % (who, index.device, weights.device))
    longest = int(index.walk[q].max()) if q.size else 0
    if longest * weights.max_weight >= 2 ** 62:
        raise ValueError("elimrec_amd.ops.%s: the int64 sums could overflow: %d (the longest walk) x %d (the largest weight) >= 2^62"
                         % (who, longest, weights.max_weight))
    if not math.isfinite(float(longest * weights.max_weight) * 2.0 ** -WALK_FRAC_BITS * weights.max_scale):
        raise ValueError("elimrec_amd.ops.%s: the scores leave float64: %d (the longest walk) x %d (the largest weight) x 2^-%d x %r"
                         % (who, longest, weights.max_weight, WALK_FRAC_BITS, weights.max_scale))


def walk_topk(index, rows, K, weights, out_idx, out_val=None, lds=True, workspace=None):
    """elimrec_walk_topk: cooccur_topk's lists with every two-step walk weighted by the node it passes through (csrc/walk.hip) --
    P3alpha / RP3beta with rp3_weights, Adamic-Adar or resource allocation with other weights. index: an ops.CooccurIndex;
    weights: an ops.WalkWeights of its two sides; rows: host array or tensor of ids, checked on the host (IndexError).
    S(q, j) = the sum over the walks q -> u -> j, j != q, of mid_weight[u] (int64; a repeated edge is a walk of its own);
    val = float32((float64(S) * 2^-40) * row_scale[q] * col_scale[j]), float64 left to right, rounded once. Listed: the rows
    with at least one walk, never q itself. out_idx int32 / out_val float32 (optional) [Q x K] on the index's device <- the K best
    by (fp32 score descending, id ascending), -1 / -inf behind them. 1 <= K <= WALK_MAX_K = 256. A row with
    walk_rows_in_lds(index.walk[q]) takes the LDS form, every other row -- with lds=False every row -- the dense form, whose int64
    rows live in `workspace`: a uint8 device tensor of at least walk_workspace(n_dense_rows, index.n_query) bytes, 16-byte aligned,
    ZERO before its first use (every call leaves it zero); default: allocated and zeroed here, at most COOCCUR_WORKSPACE_BUDGET
    bytes. Refused before any launch (ValueError): (the longest walk of the rows) x (the largest weight) >= 2^62, scores that would
    leave float64, weights that do not fit the index, K, a workspace that is too small, a default workspace past the budget.
    Both forms give the same bits: a row's outputs depend on the graph, the three arrays, the row and K alone. An empty `rows`
    returns without a launch."""
    who = "walk_topk"
    K = _form_k(who, K, WALK_MAX_K)
    q = _cooccur_rows(who, index, rows)
    _walk_bounds(who, index, q, weights)
    Q, dev = int(q.size), index.device
    call = _form_call(who, "walk", lambda: index.walk, q, lds, index.n_query, K, (out_idx, out_val, None), workspace, dev, "index's")
    if call is None:
        return out_idx
    (ip, vp, _), n_dense, ws = call
    walk = torch.empty(Q, dtype=torch.int64, device=dev)
    _lib.check(_lib.load().elimrec_walk_topk(_dev(index.q_ptr, "q_ptr", torch.int64), _dev(index.q_nbr, "q_nbr", torch.int32), index.n_query,
                                             _dev(index.o_ptr, "o_ptr", torch.int64), _dev(index.o_nbr, "o_nbr", torch.int32), index.n_other,
                                             _dev(_resident_ids(q, dev), "rows", torch.int32), Q, K,
                                             _dev(weights.mid_weight, "mid_weight", torch.int64), _dev(weights.row_scale, "row_scale", torch.float64),
                                             _dev(weights.col_scale, "col_scale", torch.float64), 1 if lds else 0, n_dense, walk.data_ptr(),
                                             ip, vp, ws.data_ptr(), ws.numel(), _stream()), who)
    return out_idx


VOTE_MAX_K = 256                         # the longest list neighbour_vote_topk keeps (csrc/vote.hip), known without the library
VOTE_FRAC_BITS = 24                      # fraction bits of a vote's fixed-point value: q = rint(double(val) * 2^24)
VOTE_MAX_VOTES = 1 << 30                 # (history length) x Kn of one user stays below this: the count's mark bit of a left-out id


class NeighbourLists(object):
    """Neighbour lists idx int32 / val float32 [n x Kn] as cooccur_topk or cosine_topk write them (-1 / -inf fillers), CHECKED ONCE ON
    THE HOST -- two dimensions, equal shapes, Kn >= 1, n < 2^31 - 1, the dtypes, contiguous (ValueError / TypeError) -- and then
    resident on `device`: neighbour_vote_topk takes them as is, call after call. idx and val: host arrays or tensors (device tensors
    stay where they are when they already live on `device`). max_abs = the largest |val| over the FINITE values (0.0 without one),
    taken here once -- for device tensors that read is a synchronisation; neighbour_vote_topk's overflow bound uses it. The ids'
    range is left to the kernel, which checks every entry and never dereferences one outside [0, n). scale_exp / zero_votes: the
    power of two EliMRec.neighbour_lists multiplied the values by before they came here, and the share of listed entries whose
    fixed-point vote is 0 (source "rp3"; 0 / None otherwise)."""

    scale_exp, zero_votes = 0, None

    def __init__(self, idx, val, device):
        who = "NeighbourLists"
        it = idx if isinstance(idx, torch.Tensor) else torch.from_numpy(np.asarray(idx))
        vt = val if isinstance(val, torch.Tensor) else torch.from_numpy(np.asarray(val))
        if it.dim() != 2 or vt.dim() != 2 or it.shape != vt.shape or it.shape[1] < 1:
            raise ValueError("elimrec_amd.ops.%s: idx and val are both [n x Kn] with Kn >= 1, got %s and %s"
                             % (who, tuple(it.shape), tuple(vt.shape)))
        if it.dtype != torch.int32 or vt.dtype != torch.float32:
            raise TypeError("elimrec_amd.ops.%s: idx must be int32 and val float32, got %s and %s" % (who, it.dtype, vt.dtype))
        if not (it.is_contiguous() and vt.is_contiguous()):
            raise ValueError("elimrec_amd.ops.%s: idx and val must be contiguous" % who)
        if it.shape[0] >= 2 ** 31 - 1:
            raise ValueError("elimrec_amd.ops.%s: n < 2^31 - 1, got %d" % (who, it.shape[0]))
        self.n, self.Kn = int(it.shape[0]), int(it.shape[1])
        self.device = torch.device(device)
        self.idx, self.val = it.to(self.device), vt.to(self.device)
        finite = torch.isfinite(self.val)
        self.max_abs = float(torch.where(finite, self.val.abs(), torch.zeros_like(self.val)).max().item()) if self.n else 0.0


def vote_rows_in_lds(V):
    """Which form neighbour_vote_topk takes for a user with V = (history length) x Kn + (entries left out) (host arithmetic only):
    True = the LDS form (V <= VOTE_SLOTS / 2: the hash table's load factor is at most 0.5 whatever the ids are), False = the dense
    form. Both forms give the same bits. ValueError for V < 0."""
    return _form_rows_in_lds("vote", "V", V)


def vote_workspace(n_dense_rows, n):
    """Bytes of the dense form's rows for a call with n_dense_rows users on that form over lists of n items (host arithmetic only):
    min(n_dense_rows, VOTE_GROUPS) rows of n int64 sums and n int32 counts."""
    return _form_workspace("vote", n_dense_rows, n)


def _vote_indexes(who, lists, hist, excl):
    if not isinstance(lists, NeighbourLists):
        raise TypeError("elimrec_amd.ops.%s: lists must be an ops.NeighbourLists, got %s" % (who, type(lists).__name__))
    if not isinstance(hist, HistoryIndex):
        raise TypeError("elimrec_amd.ops.%s: hist must be an ops.HistoryIndex, got %s" % (who, type(hist).__name__))
    if excl is not None:
        if not isinstance(excl, HistoryIndex):
            raise TypeError("elimrec_amd.ops.%s: excl must be an ops.HistoryIndex or None, got %s" % (who, type(excl).__name__))
        if excl.n_rows != hist.n_rows:
            raise ValueError("elimrec_amd.ops.%s: hist and excl name the same users: %d and %d segments" % (who, hist.n_rows, excl.n_rows))


def vote_votes(lists, hist, excl=None, exclude_history=True):
    """Host int64 [hist.n_rows]: V of every segment = (history length) x Kn + (entries left out: the history's own with
    exclude_history, plus excl's) -- the number that alone picks a user's form in neighbour_vote_topk (vote_rows_in_lds)."""
    _vote_indexes("vote_votes", lists, hist, excl)
    V = hist.sizes.astype(np.int64) * (lists.Kn + (1 if exclude_history else 0))
    return V if excl is None else V + excl.sizes


def neighbour_vote_topk(lists, hist, users, K, out_idx, out_val=None, out_cnt=None, excl=None, exclude_history=True, lds=True,
                        workspace=None):
    """elimrec_neighbour_vote_topk: per user the K items the neighbour lists of the user's history vote for -- ItemKNN (lists from
    cooccur_topk) or content-KNN (lists from cosine_topk) recommendations (csrc/vote.hip). lists: an ops.NeighbourLists [n x Kn];
    hist: an ops.HistoryIndex, the histories; excl: a second HistoryIndex of the same segments, ids to leave out on top (optional);
    users: host array or tensor of segment ids, checked on the host (IndexError; a synchronisation for a device tensor), a repeated
    id is a row of its own. A vote is a pair (history position p, slot s) with j = hist[p] in [0, n), i = idx[j, s] in [0, n) and
    val[j, s] finite -- anything else is skipped; a repeated history id votes again, a repeated id within a list votes again. It
    adds q = rint(double(val) * 2^24) (round half even) to an int64 sum S and 1 to an int32 count c. Listed: c >= 1 and not left
    out (the history's own ids with exclude_history, excl's segment). score = float(double(S) * 2^-24). out_idx int32 / out_val
    float32 (optional) / out_cnt int32 (optional: c) [B x K] on the lists' device <- the K best by (score descending, id
    ascending), -1 / -inf / 0 behind them. 1 <= K <= VOTE_MAX_K = 256.
    Refused before any launch (ValueError): sums that could overflow -- ceil(lists.max_abs * 2^24) x (hist's longest segment) x Kn
    >= 2^62 --, (longest segment) x Kn >= 2^30, a workspace that is too small, a default workspace past COOCCUR_WORKSPACE_BUDGET.
    A user with vote_rows_in_lds(V) (vote_votes) takes the LDS form, every other user -- with lds=False every user -- the dense
    form, whose rows live in `workspace`: a uint8 device tensor of at least vote_workspace(n_dense_rows, n) bytes, 16-byte aligned,
    ZERO before its first use (every call leaves it zero); default: allocated and zeroed here. Both forms give the same bits: a
    user's outputs depend on the history as a multiset, the lists, the exclusions and K alone. Every argument error is raised before
    the device is touched. An empty `users` returns without a launch."""
    who = "neighbour_vote_topk"
    K = _form_k(who, K, VOTE_MAX_K)
    _vote_indexes(who, lists, hist, excl)
    u = _checked_ids(users, hist.n_rows, who, "users", "users span [%d, %d], the histories have %d segments")
    B, dev = int(u.size), lists.device
    longest = int(hist.sizes.max()) if hist.sizes.size else 0
    if math.ceil(lists.max_abs * 2.0 ** VOTE_FRAC_BITS) * longest * lists.Kn >= 2 ** 62:
        raise ValueError("elimrec_amd.ops.%s: the int64 sums could overflow: ceil(%r * 2^%d) x %d (the longest history) x %d (Kn) >= 2^62"
                         % (who, lists.max_abs, VOTE_FRAC_BITS, longest, lists.Kn))
    if longest * lists.Kn >= VOTE_MAX_VOTES:
        raise ValueError("elimrec_amd.ops.%s: %d (the longest history) x %d (Kn) votes of one user, fewer than 2^30 are taken"
                         % (who, longest, lists.Kn))
    if hist.ptr.device != dev or (excl is not None and excl.ptr.device != dev):
        raise ValueError("elimrec_amd.ops.%s: the lists live on %s, the histories on %s" % (who, dev, hist.ptr.device))
    call = _form_call(who, "vote", lambda: vote_votes(lists, hist, excl, exclude_history), u, lds, lists.n, K,
                      (out_idx, out_val, out_cnt), workspace, dev, "lists'")
    if call is None:
        return out_idx
    (ip, vp, cp), n_dense, ws = call
    up = torch.from_numpy(np.ascontiguousarray(u, dtype=np.int64)).to(dev)
    ep, ei, en = (None, None, 0) if excl is None else (_dev(excl.ptr, "excl_ptr", torch.int64), _dev(excl.items, "excl_items", torch.int32),
                                                       excl.n_rows)
    _lib.check(_lib.load().elimrec_neighbour_vote_topk(_dev(lists.idx, "nbr_idx", torch.int32), _dev(lists.val, "nbr_val", torch.float32),
                                                       lists.n, lists.Kn, _dev(hist.ptr, "hist_ptr", torch.int64),
                                                       _dev(hist.items, "hist_items", torch.int32), hist.n_rows, ep, ei, en,
                                                       _dev(up, "users", torch.int64), B, K, 1 if exclude_history else 0, 1 if lds else 0,
                                                       n_dense, ip, vp, cp, ws.data_ptr(), ws.numel(), _stream()), who)
    return out_idx


ALS_FACTORS = (16, 32, 48, 64)           # the factor dimensions als_solve takes (csrc/als.hip), known without the library


class AlsIndex(object):
    """The CSR of the side an ALS half-sweep solves (ptr [n + 1] / nbr: a row's neighbours on the fixed side of n_fixed rows),
    CHECKED ON THE HOST and then resident on `device`: ptr[0] = 0, ascending, ptr[n] = len(nbr) and EVERY LIST STRICTLY ASCENDING
    -- no repeated edge, so als_solve's formula is the whole definition -- (ValueError); integer ids in [0, n_fixed) (IndexError).
    als_solve takes it as is, call after call, so a fit checks each side once. Kept on the host: deg (int64 [n]) and by_degree
    (int32 [n]: all rows, degree descending, equal degrees by ascending id -- the order als_solve launches them in)."""

    def __init__(self, ptr, nbr, n, n_fixed, device):
        who = "AlsIndex"
        n, n_fixed = int(n), int(n_fixed)
        if not (0 <= n < 2 ** 31 - 1 and 0 <= n_fixed < 2 ** 31 - 1):
            raise ValueError("elimrec_amd.ops.%s: both sides need 0 <= rows < 2^31 - 1, got %d and %d" % (who, n, n_fixed))
        p, ids = _checked_csr(ptr, nbr, n, n_fixed, who, ("ptr", "nbr", "n", "nbr spans [%d, %d], the fixed side has %d rows"))
        if ids.size > 1:
            bad = np.diff(ids.astype(np.int64)) <= 0
            starts = p[1:-1]
            bad[starts[(starts > 0) & (starts < ids.size)] - 1] = False      # the step from one list into the next
            if bad.any():
                at = int(np.flatnonzero(bad)[0])
                raise ValueError("elimrec_amd.ops.%s: every list is strictly ascending (no repeated edge): row %d lists %d, then %d"
                                 % (who, int(np.searchsorted(p, at, side="right") - 1), int(ids[at]), int(ids[at + 1])))
        self.n, self.n_fixed, self.n_edges = n, n_fixed, int(ids.size)
        self.deg = np.diff(p)
        self.by_degree = np.argsort(-self.deg, kind="stable").astype(np.int32)
        self.device = torch.device(device)
        self.ptr = torch.from_numpy(p).to(device)
        self.nbr = _resident_ids(ids, device)


def _als_params(who, d, conf):
    if d not in ALS_FACTORS:
        raise ValueError("elimrec_amd.ops.%s: the factors need d %% 16 == 0 and 16 <= d <= 64 columns, got %d" % (who, d))
    if isinstance(conf, bool) or not isinstance(conf, (int, float, np.integer, np.floating)) or not (math.isfinite(conf) and conf >= 0):
        raise ValueError("elimrec_amd.ops.%s: conf is finite and >= 0, got %r" % (who, conf))
    return float(conf)


def _ials_params(who, factors=64, iters=15, conf=1.0, reg=0.01, reg_scale=0.0, seed=2022):
    """The parameters of an iALS fit (EliMRec.fit_ials, BaselineReport, the --baseline_* switches), checked before anything touches
    the device (ValueError): -> (factors, iters, conf, reg, reg_scale, seed)."""
    def number(x):
        return not isinstance(x, bool) and isinstance(x, (int, float, np.integer, np.floating)) and math.isfinite(x)
    if isinstance(factors, bool) or not isinstance(factors, (int, np.integer)) or factors not in ALS_FACTORS:
        raise ValueError("%s: factors must be one of %s, got %r" % (who, ALS_FACTORS, factors))
    if isinstance(iters, bool) or not isinstance(iters, (int, np.integer)) or not 1 <= iters <= 100:
        raise ValueError("%s: iters must be an integer in [1, 100], got %r" % (who, iters))
    if not (number(conf) and conf >= 0):
        raise ValueError("%s: conf must be finite and >= 0, got %r" % (who, conf))
    if not (number(reg) and reg > 0):
        raise ValueError("%s: reg must be finite and > 0, got %r" % (who, reg))
    if not (number(reg_scale) and 0 <= reg_scale <= 1):
        raise ValueError("%s: reg_scale must lie in [0, 1], got %r" % (who, reg_scale))
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or seed < 0:
        raise ValueError("%s: seed must be an integer >= 0, got %r" % (who, seed))
    return int(factors), int(iters), float(conf), float(reg), float(reg_scale), int(seed)


def _als_reg(who, reg, n, device):
    """The per-row ridge as a float64 device tensor [n]: a number (every row's), a host array or a tensor; finite and >= 0
    (ValueError) -- a host value is checked before anything touches the device, a device tensor by a read back."""
    if isinstance(reg, torch.Tensor) and reg.is_cuda:
        if reg.dtype != torch.float64 or reg.dim() != 1 or reg.numel() != n or not reg.is_contiguous():
            raise ValueError("elimrec_amd.ops.%s: reg must be a contiguous float64 tensor with one entry per row (%d)" % (who, n))
        if n and not bool((torch.isfinite(reg) & (reg >= 0)).all().item()):
            raise ValueError("elimrec_amd.ops.%s: every reg is finite and >= 0" % who)
        return None, reg
    host = np.asarray(_host(reg), dtype=np.float64)
    host = np.full(n, float(host), dtype=np.float64) if host.ndim == 0 else np.ascontiguousarray(host.reshape(-1))
    if host.size != n:
        raise ValueError("elimrec_amd.ops.%s: reg needs one entry per row (%d), got %d" % (who, n, host.size))
    if n and not (np.isfinite(host) & (host >= 0)).all():
        raise ValueError("elimrec_amd.ops.%s: every reg is finite and >= 0" % who)
    return host, None


def als_solve(index, F, A0, reg, conf, out, rows=None):
    """elimrec_als_solve: one half-sweep of implicit-feedback ALS (Hu, Koren, Volinsky, ICDM 2008; csrc/als.hip). For every listed
    row r of the side `index` (an ops.AlsIndex) describes, N(r) its neighbours and f_j row j of F:
        A_r = A0 + reg[r] I + conf sum_{j in N(r)} f_j f_j^T,   b_r = (1 + conf) sum_{j in N(r)} f_j,   out[r] = A_r^-1 b_r
    F float32 [n_fixed x d] with unit column stride (a column block of a wider matrix is fine), d in ALS_FACTORS = {16, 32, 48, 64};
    A0 float64 [d x d] contiguous: F^T F, from row_gram(F, ones, arange(n_fixed))[0] -- with unit norms the exact-product float64
    Gram in a fixed order; only its upper triangle is read. reg: the per-row ridge, a number, a host array or a float64 device
    tensor [n], finite and >= 0; conf: a number, finite and >= 0. out float32 [n x d] with unit column stride: row r is written for
    every listed r, other rows are left alone. rows: host array or tensor of ids (IndexError), default every row; they are
    launched by degree descending, and a row's bits do not depend on that: everything is float64 with exact products, summed in
    the CSR order of the row's list (ALS_CHUNK rows per LDS stage), rounded to float32 once. A row with an empty list is zeros.
    A row whose A_r is not positive definite (a Cholesky pivot <= 0 or not finite) is written as zeros and the call raises
    ArithmeticError naming the lowest such row, after every other row has been solved. The status word is read back (a
    synchronisation). Every argument error is raised before the device is required. -> out."""
    who = "als_solve"
    if not isinstance(index, AlsIndex):
        raise TypeError("elimrec_amd.ops.%s: index must be an ops.AlsIndex, got %s" % (who, type(index).__name__))
    if not isinstance(F, torch.Tensor) or F.dim() != 2 or F.stride(1) != 1 or F.shape[0] != index.n_fixed:
        raise ValueError("elimrec_amd.ops.%s: F must be [%d x d] with unit column stride" % (who, index.n_fixed))
    d = int(F.shape[1])
    conf = _als_params(who, d, conf)
    reg_host, reg_dev = _als_reg(who, reg, index.n, index.device)
    if rows is None:
        q = index.by_degree
    else:
        q = _checked_ids(rows, index.n, who, "rows", "rows span [%d, %d], the side has %d rows")
        q = q[np.argsort(-index.deg[q], kind="stable")]
    dev = index.device
    fp, ld = _rowmajor(F, "F")
    ap = _dev(A0, "A0", torch.float64)
    if tuple(A0.shape) != (d, d) or not A0.is_contiguous() or A0.device != dev or F.device != dev:
        raise ValueError("elimrec_amd.ops.%s: A0 must be a contiguous float64 [%d x %d] tensor, with F on the index's device" % (who, d, d))
    op, ld_out = _rowmajor(out, "out")
    if tuple(out.shape) != (index.n, d) or out.device != dev:
        raise ValueError("elimrec_amd.ops.%s: out must be [%d x %d] on the index's device" % (who, index.n, d))
    if q.size == 0:
        return out
    if reg_dev is None:
        reg_dev = torch.from_numpy(reg_host).to(dev)
    status = torch.tensor([0, 2 ** 31 - 1], dtype=torch.int32, device=dev)
    _lib.check(_lib.load().elimrec_als_solve(fp, ld, index.n_fixed, d, ap, _dev(index.ptr, "ptr", torch.int64),
                                             _dev(index.nbr, "nbr", torch.int32), index.n, _dev(_resident_ids(q, dev), "rows", torch.int32),
                                             int(q.size), reg_dev.data_ptr(), conf, op, ld_out, status.data_ptr(), _stream()), who)
    bad, first = (int(x) for x in status.cpu())
    if bad:
        raise ArithmeticError("elimrec_amd.ops.%s: A_r is not positive definite for %d row(s), the first is row %d (written as zeros)"
                              % (who, bad, first))
    return out


EASE_MAX_K = 256                         # the longest list ease_topk keeps (csrc/ease.hip), known without the library
# the largest catalogue EliMRec.fit_ease takes: 8 I^2 = 214.7 GB at I = 163 840 (2560 sweep blocks of 64), + 2 * 64 * I * 8 B = 0.17 GB
# of sweep workspace, leaves 73 GB of a 288 GB card: the evaluator's tables ([U + I] x 256 floats: below 1 GB at such a catalogue), the
# graph and the top-K workspace (users x ceil(I / 4096) x K x 8 B: 2.6 GB for 31 504 users at K = 256) fit many times over
EASE_MAX_ITEMS = 163840


def _ease_params(who, l2=500.0, num_items=None):
    """The parameter of an EASE fit (EliMRec.fit_ease, BaselineReport, --baseline_l2), checked before anything touches the device
    (ValueError): l2 finite and > 0; num_items (when given) at most EASE_MAX_ITEMS. -> l2 as a float."""
    if isinstance(l2, bool) or not isinstance(l2, (int, float, np.integer, np.floating)) or not (math.isfinite(l2) and l2 > 0):
        raise ValueError("%s: l2 must be finite and > 0, got %r" % (who, l2))
    if num_items is not None and int(num_items) > EASE_MAX_ITEMS:
        raise ValueError("%s: the dense item-item matrix takes 8 I^2 bytes; I <= EASE_MAX_ITEMS = %d, got %d" % (who, EASE_MAX_ITEMS, num_items))
    return float(l2)


def _square_f64(who, t, name, n=None):
    """A float64 device matrix [n x >= n] with unit column stride: (pointer, ld, n)."""
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.stride(1) != 1 or t.shape[1] != t.shape[0] or (n is not None and t.shape[0] != n):
        raise ValueError("elimrec_amd.ops.%s: %s must be a 2-D square tensor%s with unit column stride"
                         % (who, name, "" if n is None else " [%d x %d]" % (n, n)))
    p = _dev(t, name, torch.float64)
    n = int(t.shape[0])
    ld = int(t.stride(0)) if n > 1 else max(n, int(t.stride(0)))
    if ld < n:
        raise ValueError("elimrec_amd.ops.%s: %s needs a row stride >= %d" % (who, name, n))
    return p, ld, n


def gram_counts(index, l2, out):
    """elimrec_gram_counts (csrc/ease.hip): out float64 [n x n] (unit column stride, row stride >= n) <- X^T X + l2 I of the
    bipartite graph `index` describes -- an ops.CooccurIndex whose query side are the n rows of the result (for EASE: side "item":
    item -> its training users, user -> items). Entry (i, j) counts the walks i -> u -> j, so with lists that hold no repeated edge
    it is the Gram matrix of the binary X; the counts are integers, the result is exact and does not depend on the launch
    geometry. l2: a number, finite and >= 0. Every argument error is raised before the device is required. -> out."""
    who = "gram_counts"
    if not isinstance(index, CooccurIndex):
        raise TypeError("elimrec_amd.ops.%s: index must be an ops.CooccurIndex, got %s" % (who, type(index).__name__))
    if isinstance(l2, bool) or not isinstance(l2, (int, float, np.integer, np.floating)) or not (math.isfinite(l2) and l2 >= 0):
        raise ValueError("elimrec_amd.ops.%s: l2 is finite and >= 0, got %r" % (who, l2))
    op, ld, n = _square_f64(who, out, "out", index.n_query)
    if out.device != index.device:
        raise ValueError("elimrec_amd.ops.%s: out lives on %s, the index on %s" % (who, out.device, index.device))
    if n == 0:
        return out
    _lib.check(_lib.load().elimrec_gram_counts(_dev(index.q_ptr, "q_ptr", torch.int64), _dev(index.q_nbr, "q_nbr", torch.int32),
                                               _dev(index.o_ptr, "o_ptr", torch.int64), _dev(index.o_nbr, "o_nbr", torch.int32), n,
                                               index.n_other, float(l2), op, ld, _stream()), who)
    return out


def spd_inverse_workspace(n):
    """Bytes of workspace spd_inverse needs for an [n x n] matrix (host arithmetic only)."""
    return int(_lib.load().elimrec_spd_inverse_workspace(int(n)))


def spd_inverse(A, workspace=None):
    """elimrec_spd_inverse (csrc/ease.hip): A float64 [n x n], n >= 1, symmetric positive definite with both triangles stored (unit
    column stride) <- its inverse, in place, all float64: the symmetric block sweep of width 64 on v_mfma_f64_16x16x4_f64. The
    result is exactly symmetric and its bits depend on A alone (two calls on copies agree bit for bit). workspace: a uint8 device
    tensor of at least spd_inverse_workspace(n) bytes, 16-byte aligned; default: allocated here. -> the smallest pivot of the
    blocks' square-root-free Cholesky factorisations (a float; read back: a synchronisation). A pivot that is <= 0 or not finite
    raises ArithmeticError naming its index; A is then left half swept. Every argument error is raised before the device is
    required."""
    who = "spd_inverse"
    if isinstance(A, torch.Tensor) and A.dim() == 2 and A.shape[0] == A.shape[1] == 0:
        raise ValueError("elimrec_amd.ops.%s: A needs n >= 1 rows" % who)
    ap, ld, n = _square_f64(who, A, "A")
    lib = _lib.load()
    need = int(lib.elimrec_spd_inverse_workspace(n))
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=A.device)
    wp = _dev(workspace, "workspace", torch.uint8)
    if workspace.numel() < need or not workspace.is_contiguous() or wp % 16 or workspace.device != A.device:
        raise ValueError("elimrec_amd.ops.%s: the workspace needs %d contiguous bytes on A's device, 16-byte aligned (got %d)"
                         % (who, need, workspace.numel()))
    pivot = torch.empty(1, dtype=torch.float64, device=A.device)
    status = torch.empty(2, dtype=torch.int32, device=A.device)
    _lib.check(lib.elimrec_spd_inverse(ap, n, ld, pivot.data_ptr(), status.data_ptr(), wp, workspace.numel(), _stream()), who)
    bad, first = (int(x) for x in status.cpu())
    if bad:
        raise ArithmeticError("elimrec_amd.ops.%s: the matrix is not positive definite: the pivot at index %d is <= 0 or not finite "
                              "(A is left half swept)" % (who, first))
    return float(pivot.item())


_EaseQuery = collections.namedtuple("_EaseQuery", ("n_queries",))


def ease_topk_workspace(Q, n, K):
    """Bytes of workspace ease_topk needs (host arithmetic only)."""
    return int(_lib.load().elimrec_ease_topk_workspace(int(Q), int(n), int(K)))


def ease_topk(P, hist, users, K, out_idx, out_val=None, excl=None, workspace=None):
    """elimrec_ease_topk (csrc/ease.hip): per user the K items j with the largest EASE score
        s_j = float32(-(sum_{i in H, i != j} P[i, j]) / P[j, j]),
    the sum in float64 in the order of the user's history H, by (score descending, id ascending). P float64 [I x I] with unit
    column stride: G^-1 of an EASE fit, or any table with a non-zero diagonal. hist: an ops.HistoryIndex built with n_items = I;
    users: host array or tensor of its segment ids, checked on the host (IndexError), a repeated id is a row of its own. excl: a
    second HistoryIndex over the same segments, the ids left out INSTEAD of the history (so an item of the history can be listed:
    the sum then skips it); default: the history itself is left out. out_idx int32 / out_val float32 (optional) [B x K] on P's
    device, -1 / -inf where fewer than K items are left. An empty history scores 0 everywhere: the lowest ids that are not left
    out. No [B x I] block is written; grid, K-lists, workspace (ease_topk_workspace bytes) and merge as cosine_topk. Every argument
    error is raised before the device is required. 1 <= K <= 256. An empty `users` returns without a launch."""
    who = "ease_topk"
    K = int(K)
    if not 1 <= K <= EASE_MAX_K:
        raise ValueError("elimrec_amd.ops.%s: 1 <= K <= %d, got %d" % (who, EASE_MAX_K, K))
    if not isinstance(P, torch.Tensor) or P.dim() != 2 or P.stride(1) != 1 or P.shape[0] != P.shape[1]:
        raise ValueError("elimrec_amd.ops.%s: P must be a 2-D square tensor with unit column stride" % who)
    n = int(P.shape[0])
    for h, name in ((hist, "hist"), (excl, "excl")):
        if h is None and name == "excl":
            continue
        if not isinstance(h, HistoryIndex):
            raise TypeError("elimrec_amd.ops.%s: %s must be an ops.HistoryIndex%s, got %s"
                            % (who, name, " or None" if name == "excl" else "", type(h).__name__))
        if h.n_items is None or h.n_items > n:
            raise IndexError("elimrec_amd.ops.%s: %s must be checked against the catalogue (n_items <= %d), got %r" % (who, name, n, h.n_items))
    if excl is not None and excl.n_rows != hist.n_rows:
        raise ValueError("elimrec_amd.ops.%s: hist and excl name the same users: %d and %d segments" % (who, hist.n_rows, excl.n_rows))
    u = _checked_ids(users, hist.n_rows, who, "users", "users span [%d, %d], the histories have %d segments")
    pp, ld, n = _square_f64(who, P, "P")
    dev = P.device
    if hist.ptr.device != dev or (excl is not None and excl.ptr.device != dev):
        raise ValueError("elimrec_amd.ops.%s: P lives on %s, the histories on %s" % (who, dev, hist.ptr.device))
    up = torch.from_numpy(np.ascontiguousarray(u if u.size else np.zeros(1), dtype=np.int64)).to(dev)
    ep, ei = (None, None) if excl is None else (_dev(excl.ptr, "excl_ptr", torch.int64), _dev(excl.items, "excl_items", torch.int32))
    return _topk_call(who, n, _EaseQuery(int(u.size)), K, out_idx, out_val, workspace, dev, dev, lambda: (
        pp, ld, n, _dev(hist.ptr, "hist_ptr", torch.int64), _dev(hist.items, "hist_items", torch.int32), ep, ei, hist.n_rows,
        _dev(up, "users", torch.int64), int(u.size)))
