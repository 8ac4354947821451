"""The block-wise top-K lists the effect and the list report share (reports._Report.top_lists) against ONE predict_device call."""
import numpy as np
import pytest
import torch

from helpers import build_model_from_fixture, load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def test_top_lists_in_blocks_are_one_predict_call():
    """7 users in blocks of 3 (3 + 3 + 1), one of them without train items, K = 5 over the ml3 fixture's 110 items (the smallest catalogue the fixtures build directly)."""
    from elimrec_amd.reports import EffectReport, ListReport
    g = load_golden("ml3")
    model, _ = build_model_from_fixture(g, DEV)
    model.bpr_loss(_t(g["step1/users"]), _t(g["step1/pos"]), _t(g["step1/neg"]))
    K, users = 5, list(model.dataset.get_user_test_dict().keys())[:7]
    train = {u: list(model.dataset.get_user_train_dict().get(u, [])) for u in users}
    assert all(len(v) for v in train.values())
    del train[users[4]]                                                        # a user without train items
    test = {u: [0] for u in users}
    flat = [i for u in users for i in train.get(u, [])]
    tptr = _t(np.cumsum([0] + [len(train.get(u, [])) for u in users]).astype(np.int64))
    want = model.predict_device(_t(np.asarray(users, dtype=np.int64)), top_k=K, train_ptr=tptr, train_items=_t(np.asarray(flat, dtype=np.int32)))[0]
    effect, lists = EffectReport(model.dataset, train, test, K), ListReport(model.dataset, train, test, K)
    effect.block_users = lists.block_users = 3
    blocks = list(effect.top_lists(model, users, K, 3, "id"))
    assert [(a, b) for a, b, _, _ in blocks] == [(0, 3), (3, 6), (6, 7)]
    assert torch.equal(torch.cat([u for _, _, u, _ in blocks]).cpu(), torch.as_tensor(users, dtype=torch.int64))
    assert torch.equal(torch.cat([idx for _, _, _, idx in blocks]), want) and want.dtype == torch.int32 and tuple(want.shape) == (7, K)
    # the two reports built on it see the same lists: the list report returns them, the effect report's rows are the breakdown of them
    rows, columns, got, _ = lists.list_rows(model)
    assert torch.equal(got, want)
    erows, ecolumns = effect.effect_rows(model)
    direct = torch.empty(7, K, len(ecolumns), dtype=torch.float32, device=DEV)
    model.effects_device(_t(np.asarray(users, dtype=np.int64)), torch.arange(8, dtype=torch.int64, device=DEV) * K, want.reshape(-1), direct)
    assert torch.equal(erows.view(torch.int32), direct.view(7 * K, -1).view(torch.int32))
