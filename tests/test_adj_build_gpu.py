"""The propagation matrix built on the device (csrc/adj.hip: elimrec_build_adj through adjacency.build_adj_device) against
model.create_adj_mat -- which tests/test_host_logic.py holds bit-identical to the reference's matrix -- on the graphs of
tests/graph_build_cases.py: no interactions, one, a node of the maximum degree (the power table's last index), complete, isolated
first and last nodes, node ids above 65 536, user degrees on every tier boundary. Row pointers, columns and the uint32 view of the
values are equal. Then the chain the large configurations run: device adjacency -> device plan, against the host plan of the host
matrix. Needs a GPU: `-m gpu`."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import graph_build_cases as gc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E_BADARG, E_WORKSPACE = 10001, 10003
_WANT = {}


def _want(name, adj_type):
    """create_adj_mat of a case, once per session."""
    from elimrec_amd.model import create_adj_mat
    if (name, adj_type) not in _WANT:
        _WANT[(name, adj_type)] = create_adj_mat(*gc.adj_cases()[name], adj_type)
    return _WANT[(name, adj_type)]


def _assert_same_csr(got, want):
    rp, cl, vl = got
    assert rp.dtype == torch.int32 and cl.dtype == torch.int32 and vl.dtype == torch.float32
    assert np.array_equal(rp.cpu().numpy(), want.indptr)
    assert np.array_equal(cl.cpu().numpy(), want.indices)
    assert np.array_equal(vl.cpu().numpy().view(np.uint32), want.data.astype(np.float32).view(np.uint32))


@pytest.mark.parametrize("adj_type", gc.ADJ_TYPES)
@pytest.mark.parametrize("name", list(gc.adj_cases()))
def test_device_adjacency_is_create_adj_mat(name, adj_type):
    from elimrec_amd.adjacency import build_adj_device
    u, i, U, I = gc.adj_cases()[name]
    want = _want(name, adj_type)
    if len(u) == 0:                  # the diagonal alone (I for mean, D'^-1 I = I for norm), or no entry at all
        assert want.nnz == (U + I if adj_type in ("norm", "mean") else 0) and np.all(want.data == 1.0)
    _assert_same_csr(build_adj_device(u, i, U, I, adj_type, DEV), want)


@pytest.mark.parametrize("where", ["first two", "last two", "far apart"])
def test_a_repeated_pair_is_refused_wherever_it_stands(where):
    from elimrec_amd.adjacency import build_adj_device
    u, i, U, I = gc.duplicate_lists()[where]
    for adj_type in ("pre", "norm"):
        with pytest.raises(ValueError, match="duplicate"):
            build_adj_device(u, i, U, I, adj_type, DEV)
    keep = np.ones(len(u), dtype=bool)
    keep[{"first two": 0, "last two": len(u) - 1, "far apart": 700}[where]] = False          # the same list without the repeat builds
    from elimrec_amd.model import create_adj_mat
    _assert_same_csr(build_adj_device(u[keep], i[keep], U, I, "pre", DEV), create_adj_mat(u[keep], i[keep], U, I, "pre"))


def _direct(u, i, U, I, code, table, table_len, ws_short=0):
    """elimrec_build_adj as build_adj_device calls it: (rc, error bits, rowptr, col, val); outputs start as -7 / NaN."""
    from elimrec_amd import _lib
    from elimrec_amd.ops import _stream
    lib = _lib.load()
    E, N = len(u), U + I
    diag = 1 if code >= 3 else 0
    nnz = 2 * E + (N if diag else 0)
    du, di = torch.from_numpy(u).to(DEV), torch.from_numpy(i).to(DEV)
    rowptr = torch.full((N + 1,), -7, dtype=torch.int32, device=DEV)
    col = torch.full((max(nnz, 1),), -7, dtype=torch.int32, device=DEV)
    val = torch.full((max(nnz, 1),), float("nan"), dtype=torch.float32, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    ws = torch.empty(int(lib.elimrec_build_adj_workspace(E, N, diag)), dtype=torch.uint8, device=DEV)
    rc = lib.elimrec_build_adj(du.data_ptr(), di.data_ptr(), E, U, I, code, table.data_ptr(), table_len, rowptr.data_ptr(), col.data_ptr(),
                               val.data_ptr(), err.data_ptr(), ws.data_ptr(), ws.numel() - ws_short, _stream())
    torch.cuda.synchronize()
    return rc, int(err.item()), rowptr, col, val


def test_the_power_table_is_read_to_its_last_entry_and_not_beyond(monkeypatch):
    """One user with all 300 items: 'norm' reads pow_table[d + 1] = pow_table[301], the last of max_deg + 2 entries. Told that the
    table is one entry shorter, the kernel flags the degree (error bit 2) instead of reading it; the wrapper turns the flag into a
    RuntimeError. A workspace one byte short and an unknown adjacency type are refused before any launch."""
    from elimrec_amd import _lib, adjacency
    u, i, U, I = gc.adj_cases()["one user, all 300 items"]
    full = adjacency._pow_table("norm", 300)
    assert len(full) == 302
    table = torch.from_numpy(full).to(DEV)
    rc, bits, rowptr, col, val = _direct(u, i, U, I, 3, table, 302)
    assert (rc, bits) == (0, 0)
    _assert_same_csr((rowptr, col, val), _want("one user, all 300 items", "norm"))
    rc, bits, rowptr, col, val = _direct(u, i, U, I, 3, table, 301)               # (the buffer itself keeps all 302 entries)
    assert (rc, bits) == (0, 2)
    assert bool(torch.isnan(val[:301]).all()) and not bool(torch.isnan(val[301:]).any())      # row 0 (the user's 300 + 1 entries) is flagged, not written
    real = adjacency._pow_table
    monkeypatch.setattr(adjacency, "_pow_table", lambda adj_type, max_deg: real(adj_type, max_deg)[:-1])
    with pytest.raises(RuntimeError, match="power table"):
        adjacency.build_adj_device(u, i, U, I, "norm", DEV)
    monkeypatch.undo()
    _assert_same_csr(adjacency.build_adj_device(u, i, U, I, "norm", DEV), _want("one user, all 300 items", "norm"))
    # refused before any launch: nothing is written
    for code, short, rc_want in ((3, 1, E_WORKSPACE), (5, 0, E_BADARG)):
        rc, bits, rowptr, col, val = _direct(u, i, U, I, code, table, 302, ws_short=short)
        assert rc == rc_want and bits == 0
        assert bool((rowptr == -7).all()) and bool((col == -7).all()) and bool(torch.isnan(val).all())
        with pytest.raises(RuntimeError, match="build_adj"):
            _lib.check(rc, "build_adj")


@pytest.mark.parametrize("adj_type", ["pre", "gcmc"])
def test_device_adjacency_then_device_plan_is_the_host_plan(adj_type):
    """build_adj_device -> SellPlan.on_device on the bipartite ladder (user degrees on every tier boundary of a (32, 8) plan) equals
    SellPlan(create_adj_mat(...), tiered=True): the graph never has to exist on a host. gcmc's matrix is not symmetric: its
    transpose gets a plan of its own, as the engine builds planT."""
    from elimrec_amd import slab
    from elimrec_amd.adjacency import build_adj_device
    u, i, U, I = gc.adj_cases()["bipartite ladder"]
    T, G = gc.LADDER_ADJ
    N = U + I
    want = _want("bipartite ladder", adj_type)
    rp, cl, vl = build_adj_device(u, i, U, I, adj_type, DEV)
    devp = slab.SellPlan.on_device(rp.long(), cl, vl, N, threshold=T, side_split=U, ipw=G)
    host = slab.SellPlan(want, DEV, threshold=T, side_split=U, tiered=True, ipw=G)
    gc.plans_equal(host, devp)
    c = gc.check_plan_against_matrix(devp, want, T, G)
    assert min(c.values()) > 0
    if adj_type == "gcmc":
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a.astype(dt))).to(DEV)
        got_t = sp.csr_matrix((vl.cpu().numpy(), cl.cpu().numpy(), rp.cpu().numpy()), shape=(N, N)).T.tocsr()
        got_t.sort_indices()
        want_t = want.T.tocsr()
        want_t.sort_indices()
        assert (abs(want - want_t)).nnz > 0
        devp = slab.SellPlan.on_device(up(got_t.indptr, np.int64), up(got_t.indices, np.int32), up(got_t.data, np.float32), N, threshold=T,
                                       side_split=U, ipw=G)
        gc.plans_equal(slab.SellPlan(want_t, DEV, threshold=T, side_split=U, tiered=True, ipw=G), devp)
        gc.check_plan_against_matrix(devp, want_t, T, G)
