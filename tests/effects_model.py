"""A plain torch model of the effect breakdown (models/EliMRec.py:96-113, 155-212): what predict()'s TE and TIE scores are made
of, per listed (user, item) pair. Built from score_model's blocks / logits / cosines / fuse; nothing here calls elimrec_amd.

Columns: ui = sigmoid(u0 . i0), mean_ui = the mean of ui over the WHOLE catalogue, te = fuse(ui), nde = fuse(mean_ui),
score_te = sigmoid(te), score_tie = sigmoid(te - nde) -- the expressions of score_model.predict, operation for operation --
then the cosine of every head."""
import torch

import score_model as sm

BASE = ("ui", "mean_ui", "te", "nde", "score_te", "score_tie")


def effects(Y, U, users, d, S, head_mask, fusion, lists):
    """[B x W x (6 + S)] in the dtype of Y, W = the longest list; row b = the breakdown of (users[b], lists[b][k]) in list order,
    NaN beyond the list."""
    ub, ib = sm.blocks(Y, U, users, d, S)
    a, z = sm.logits(ub, ib), sm.cosines(ub, ib)
    ui = torch.sigmoid(a)
    m = ui.mean(-1, keepdim=True)
    te = sm.fuse(ui, z, head_mask, fusion)
    nde = sm.fuse(m, z, head_mask, fusion)                  # [B, 1] where no head enters (rubi without masked heads)
    cols = [ui, m.expand_as(ui), te, nde.expand_as(ui), torch.sigmoid(te), torch.sigmoid(te - nde)] + list(z)
    full = torch.stack(cols, dim=-1)                        # [B, I, C]
    W = max((len(c) for c in lists), default=0)
    out = torch.full((len(lists), W, full.shape[-1]), float("nan"), dtype=Y.dtype)
    for b, c in enumerate(lists):
        if len(c):
            out[b, :len(c)] = full[b, torch.as_tensor(c, dtype=torch.long)]
    return out
