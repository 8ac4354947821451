"""A plain torch model of predict() (models/EliMRec.py:96-113, 155-212) on the table the scorers read, the tolerance rule the
scorer tests share and the input families they run on. Nothing here calls elimrec_amd or oracle/: it is the independent side.

Y [U + I, >= (1 + S) d]: block 0 of a row is the fused embedding, block h + 1 the pre-fusion embedding of head h; the first U rows
are users, the rest items. The model computes in the dtype of Y: float64 for the truth, float32 for the yardstick E32."""
import torch

EPS = 1e-12                    # both the F.normalize floor and the eps inside the logarithms of hm / sum
PAIRS = [("normal", "rubi"), ("TE", "rubi"), ("TE", "hm"), ("TE", "sum"), ("TIE", "rubi"), ("TIE", "hm"), ("TIE", "sum")]


def blocks(Y, U, users, d, S):
    """User rows [B, 1 + S, d] and item rows [I, 1 + S, d] of the (1 + S) d leading columns."""
    W = (1 + S) * d
    ub = Y[users.long()][:, :W]
    ib = Y[U:, :W]
    return ub.reshape(ub.shape[0], 1 + S, d), ib.reshape(ib.shape[0], 1 + S, d)


def unit(x):
    """F.normalize(x, dim=-1): each row divided by max(norm, 1e-12)."""
    return x / x.norm(dim=-1, keepdim=True).clamp_min(EPS)


def logits(ub, ib):
    return ub[:, 0] @ ib[:, 0].T


def cosines(ub, ib):
    return [unit(ub[:, h]) @ unit(ib[:, h]).T for h in range(1, ub.shape[1])]


def fuse(x, z, head_mask, fusion):
    """general_cm_fusion(x, ...) given the heads' cosines z: rubi multiplies the sigmoids of the heads in the mask, hm and sum take
    every head whatever the mask says."""
    if fusion == "rubi":
        for h, zh in enumerate(z):
            if (head_mask >> h) & 1:
                x = x * torch.sigmoid(zh)
        return x
    if fusion == "hm":
        t = torch.sigmoid(x)
        for zh in z:
            t = t * torch.sigmoid(zh)
        return torch.log(t + EPS) - torch.log1p(t)
    assert fusion == "sum"
    for zh in z:
        x = x + zh
    return torch.log(torch.sigmoid(x) + EPS)


def predict(a, z, head_mask, fusion, ptype, mean=None):
    """Scores [B, I] from the logits a and the cosines z. mean [B, 1]: the catalogue-wide row mean of sigmoid(a) where the rows of
    `a` are only a part of the catalogue (a shard, a candidate list); None: the mean over a's own columns."""
    ui = torch.sigmoid(a)
    if ptype == "TE":
        return torch.sigmoid(fuse(ui, z, head_mask, fusion))
    if ptype == "TIE":
        m = ui.mean(-1, keepdim=True) if mean is None else mean
        return torch.sigmoid(fuse(ui, z, head_mask, fusion) - fuse(m, z, head_mask, fusion))
    return torch.sigmoid(ui)


def score_model(Y, U, users, d, S, head_mask, fusion, ptype, I_total=None, row_sum=None):
    """predict() for `users` over every item row of Y. row_sum [B] and I_total: the TIE mean is row_sum / I_total (item shards)."""
    ub, ib = blocks(Y, U, users, d, S)
    mean = None if row_sum is None else (row_sum.to(Y.dtype) / I_total).reshape(-1, 1)
    return predict(logits(ub, ib), cosines(ub, ib), head_mask, fusion, ptype, mean)


# --------------------------------------------------------------------------- the tolerance rule
FP32_STEP = 2.4e-7           # one fp32 round-off step of a score
FAST_EXTRA = 4e-7            # the documented distance between the FAST and the EXACT math mode
E32_CAP = 1e-6               # plain fp32 torch is never this far from fp64 on a score in [0, 1] (2.5e-7 is the worst measured): a
                             # yardstick beyond it is itself broken (a reduced-precision GEMM), and must not widen the tolerance


def tolerance(ref64, ref32, fast, keep=None):
    """(tol, E32): E32 = max |model_fp32 - model_fp64| over the kept elements; EXACT tol = max(4 E32, 2.4e-7), FAST + 4e-7."""
    e = (ref32.double() - ref64).abs()
    if keep is not None:
        e = e[keep]
    e32 = float(e.max()) if e.numel() else 0.0
    assert e32 <= E32_CAP, ("the float32 yardstick is off", e32)
    return max(4.0 * e32, FP32_STEP) + (FAST_EXTRA if fast else 0.0), e32


def worst_error(got, ref64, keep=None):
    """max |got - ref64| over the kept elements; inf if any of them is NaN (an element nobody wrote fails, it is not skipped)."""
    e = (got.double() - ref64).abs()
    if keep is not None:
        e = e[keep]
    if not e.numel():
        return 0.0
    if bool(torch.isnan(e).any()):
        return float("inf")
    return float(e.max())


# --------------------------------------------------------------------------- input families
def make_table(family, U, I, d, S, seed):
    """float32 [U + I, (1 + S) d] on the CPU.
    benign: randn * 0.3. saturated: randn * 0.4, 30 item rows x 6 and 10 more x 40 (logits beyond +-88). zero: benign with all-zero
    head blocks on user 1 (head 0) and items 0, 2, I - 1 (one head each) and one head block of norm 1e-10 on item 3."""
    g = torch.Generator().manual_seed(seed)
    W = (1 + S) * d
    if family == "saturated":
        Y = torch.randn(U + I, W, generator=g) * 0.4
        n = min(40, I)
        Y[U:U + n * 3 // 4] *= 6.0
        Y[U + n * 3 // 4:U + n] *= 40.0
        return Y
    Y = torch.randn(U + I, W, generator=g) * 0.3
    if family == "zero":
        assert S >= 1 and I >= 5 and U >= 2
        Y[1, d:2 * d] = 0.0
        for k, i in enumerate((0, 2, I - 1)):
            h = k % S
            Y[U + i, (h + 1) * d:(h + 2) * d] = 0.0
        h = S - 1
        blk = Y[U + 3, (h + 1) * d:(h + 2) * d]
        Y[U + 3, (h + 1) * d:(h + 2) * d] = blk / blk.norm() * 1e-10
    else:
        assert family == "benign"
    return Y
