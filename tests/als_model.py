"""Float64 numpy model of the implicit-feedback ALS baseline (csrc/als.hip, EliMRec.fit_ials): the half-sweep's normal equations,
the fit step for step, the loss by the Gram trick, and the condition numbers the solve's error bound needs."""
import numpy as np


def normal_equations(ptr, nbr, F, reg, conf, r, A0=None):
    """(A_r, b_r) of row r: A0 + reg[r] I + conf sum f f^T and (1 + conf) sum f over the row's list, float64."""
    F = np.asarray(F, dtype=np.float64)
    d = F.shape[1]
    A0 = F.T @ F if A0 is None else np.asarray(A0, dtype=np.float64)
    N = F[np.asarray(nbr[int(ptr[r]):int(ptr[r + 1])], dtype=np.int64)]
    return A0 + float(reg[r]) * np.eye(d) + float(conf) * (N.T @ N), (1.0 + float(conf)) * N.sum(0)


def solve_rows(ptr, nbr, F, reg, conf, rows, A0=None):
    """x64 [len(rows) x d]: per listed row np.linalg.solve of its normal equations; a row with an empty list is zeros."""
    F = np.asarray(F, dtype=np.float64)
    A0 = F.T @ F if A0 is None else A0
    out = np.zeros((len(rows), F.shape[1]))
    for q, r in enumerate(rows):
        if ptr[r + 1] > ptr[r]:
            A, b = normal_equations(ptr, nbr, F, reg, conf, int(r), A0)
            out[q] = np.linalg.solve(A, b)
    return out


def cond(ptr, nbr, F, reg, conf, rows):
    """The 2-norm condition number of every listed row's A_r."""
    F = np.asarray(F, dtype=np.float64)
    A0 = F.T @ F
    return np.asarray([np.linalg.cond(normal_equations(ptr, nbr, F, reg, conf, int(r), A0)[0]) for r in rows])


def solve_bound(x64, cnd, d):
    """The per-row bound on |got - x64| (derived, not measured): one rounding to float32, 2^-24 |x64| entry by entry, plus the
    Cholesky backward-error bound with a loose constant, 64 d cond(A_r) 2^-53 max|x64|. -> [rows x d]."""
    x64 = np.asarray(x64, dtype=np.float64)
    return 2.0 ** -24 * np.abs(x64) + (64.0 * d * np.asarray(cnd) * 2.0 ** -53 * np.abs(x64).max(1))[:, None]


def graph(lists, n_other):
    """The training graph as the two CSRs the fit solves over: every list de-duplicated and sorted, and the transpose likewise.
    -> (ptr, nbr int32, t_ptr, t_nbr int32)."""
    lists = [np.unique(np.asarray(x, dtype=np.int64)) for x in lists]
    ptr = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum([x.size for x in lists], out=ptr[1:])
    nbr = np.concatenate(lists) if lists else np.zeros(0, dtype=np.int64)
    rows = np.repeat(np.arange(len(lists), dtype=np.int64), np.diff(ptr))
    order = np.argsort(nbr, kind="stable")
    t_ptr = np.zeros(n_other + 1, dtype=np.int64)
    np.cumsum(np.bincount(nbr, minlength=n_other), out=t_ptr[1:])
    return ptr, nbr.astype(np.int32), t_ptr, rows[order].astype(np.int32)


def ridge(ptr, reg, reg_scale):
    """reg[r] = reg * (deg(r) + 1) ** reg_scale, float64."""
    return float(reg) * (np.diff(ptr).astype(np.float64) + 1.0) ** float(reg_scale)


def objective(ptr, nbr, X, Y, reg_x, reg_y, conf):
    """The iALS loss by the Gram trick: <G_X, G_Y>_F + sum_obs [(1 + conf)(1 - s)^2 - s^2] + sum_r reg[r] |x_r|^2 over both sides."""
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    rows = np.repeat(np.arange(X.shape[0]), np.diff(ptr))
    s = (X[rows] * Y[np.asarray(nbr, dtype=np.int64)]).sum(1)
    return float(((X.T @ X) * (Y.T @ Y)).sum() + ((1.0 + conf) * (1.0 - s) ** 2 - s * s).sum()
                 + (reg_x * (X * X).sum(1)).sum() + (reg_y * (Y * Y).sum(1)).sum())


def objective_all_pairs(ptr, nbr, X, Y, reg_x, reg_y, conf):
    """The same loss as the sum over ALL pairs: (s - 0)^2 for an unobserved pair, (1 + conf)(s - 1)^2 for an observed one."""
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    total = 0.0
    for u in range(X.shape[0]):
        seen = set(int(i) for i in nbr[int(ptr[u]):int(ptr[u + 1])])
        for i in range(Y.shape[0]):
            s = float(X[u] @ Y[i])
            total += (1.0 + conf) * (s - 1.0) ** 2 if i in seen else s * s
    return total + float((reg_x * (X * X).sum(1)).sum() + (reg_y * (Y * Y).sum(1)).sum())


def fit(lists, n_items, factors=64, iters=15, conf=1.0, reg=0.01, reg_scale=0.0, seed=2022):
    """EliMRec.fit_ials step for step: items = float32(0.01 N(0, 1)), users zero; per iteration the users from the items, then the
    items from the users, each half-sweep's output rounded to float32 as the device does. -> (users, items float32, objective
    [2 iters], conds [2 iters]: the largest cond(A_r) of each half-sweep)."""
    ptr, nbr, t_ptr, t_nbr = graph(lists, n_items)
    U = len(lists)
    reg_u, reg_i = ridge(ptr, reg, reg_scale), ridge(t_ptr, reg, reg_scale)
    Y = (0.01 * np.random.default_rng(seed).standard_normal((n_items, factors))).astype(np.float32)
    X = np.zeros((U, factors), dtype=np.float32)
    obj, conds = [], []
    for _ in range(iters):
        conds.append(float(cond(ptr, nbr, Y, reg_u, conf, np.arange(U)).max()))
        X = solve_rows(ptr, nbr, Y, reg_u, conf, np.arange(U)).astype(np.float32)
        obj.append(objective(ptr, nbr, X, Y, reg_u, reg_i, conf))
        conds.append(float(cond(t_ptr, t_nbr, X, reg_i, conf, np.arange(n_items)).max()))
        Y = solve_rows(t_ptr, t_nbr, X, reg_i, conf, np.arange(n_items)).astype(np.float32)
        obj.append(objective(ptr, nbr, X, Y, reg_u, reg_i, conf))
    return X, Y, np.asarray(obj), np.asarray(conds)


N_FIXED = 300                            # fixed-side rows of the solve cases
SOLVE_CONFS = (0.0, 1.0, 40.0)
SOLVE_REGS = ("constant", "per row")


def solve_case(d, chunk, seed=0):
    """The solve case of the GPU tests (chunk = ops.ALS_CHUNK): rows of degree 0, 1, 2, chunk - 1, chunk, chunk + 1, 3 chunk + 5,
    N_FIXED (every fixed row), 7 and 0 over N_FIXED fixed rows of 0.1 N(0, 1) factors -> (ptr, nbr int32, F float32)."""
    rng = np.random.default_rng(seed)
    lists = [np.sort(rng.permutation(N_FIXED)[:k]) for k in (0, 1, 2, chunk - 1, chunk, chunk + 1, 3 * chunk + 5, N_FIXED, 7, 0)]
    ptr = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum([x.size for x in lists], out=ptr[1:])
    return ptr, np.concatenate(lists).astype(np.int32), (0.1 * rng.standard_normal((N_FIXED, d))).astype(np.float32)


def solve_reg(kind, ptr):
    """The two ridges of the solve cases, chosen so that the model alone keeps cond(A_r) <= 1e6 (tests/test_als_cpu.py)."""
    return np.full(ptr.size - 1, 0.05) if kind == "constant" else ridge(ptr, 0.05, 0.5)
