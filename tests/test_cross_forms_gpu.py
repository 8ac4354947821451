"""One zeroed workspace across the three two-form families (csrc/co_select.h): the dense forms of ops.cooccur_topk, ops.walk_topk and
ops.neighbour_vote_topk each find their accumulator rows zero and leave them zero, so ONE buffer serves them in turn -- which is what
lets EliMRec keep a single workspace for co_neighbours_device, walk_neighbours_device and knn_recommend_device. Everything is exact
against the families' host models (tests/cooccur_model.py, walk_model.py, vote_model.py): idx and cnt equal, val bit for bit."""
import pytest
import torch

import cooccur_cases as cc
from test_cooccur_gpu import DEV, Graph as CoGraph
from test_vote_gpu import _resident, _same as _same_votes
from test_walk_gpu import Graph as WalkGraph

pytestmark = pytest.mark.gpu


def test_one_workspace_serves_the_three_families_in_turn():
    """Every row forced dense (lds=False): second_pass (300 rows, one of them with 3 x 2048 candidates) counted and then walked
    with RP3beta weights, cut_rising voted (the list cut again and again), then the counts once more -- the int32 counters, the
    int64 sums with their mark bit and the (sum, count) pairs lie over the same bytes."""
    from elimrec_amd import ops
    case = cc.case("second_pass")
    rows, K = list(case.rows), 64
    co, walk, votes = CoGraph(case.users, case.n_query), WalkGraph(case.users, case.n_query), _resident("cut_rising")
    users = votes.case.users
    need = max(ops.cooccur_workspace(len(rows), case.n_query), ops.walk_workspace(len(rows), case.n_query),
               ops.vote_workspace(len(users), votes.lists.n))
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    first = co.check(rows, K, "cosine", lds=False, workspace=ws)
    assert not ws.any()
    walk.check(rows, K, "rp3", lds=False, workspace=ws)
    assert not ws.any()
    _same_votes(votes.run(users, K, lds=False, workspace=ws), votes.want(users, K), "cut_rising")
    assert not ws.any()
    again = co.check(rows, K, "cosine", lds=False, workspace=ws)
    assert not ws.any()
    assert all((a == b).all() for a, b in zip(first, again))
